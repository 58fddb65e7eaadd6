#!/usr/bin/env python
"""The backward of the encoder / decoder linears: the library's own kernels against torch's, and the cfg-3 training step with the
split-product training path off and on.

    python tools/bench_linear_backward.py [--out profiles/linear_backward_bench.json] [--rows 44446] [--skip-step]

Per shape (M rows, K -> N features; the cfg-3 encoder's token count at bs 2 and its four linear shapes) it times, in ONE process on the
same tensors, in alternating rounds:
  * own16 / own6   the backward of fused.linear_train under 16 (fp16 pieces) and 6 (bf16) terms: operand statistics (with the bias
                   gradient) + input gradient + weight gradient -- tf_linear_grad_stats_f32 x 2, tf_linear_dgrad_packed_f32,
                   tf_linear_wgrad_split_f32 and its second pass;
  * torch          torch.autograd's backward of F.linear on the same tensors (the fp32 library GEMMs + a column sum): the path the
                   training step takes with the switch off.
Each sample is `reps` backward calls between two device events (the graph of the forward is kept: only the backward is inside); the
figure reported is the median over the rounds, with the smallest and the largest next to it.  Then tools/bench_train.py (the cfg-3
step) runs as a child process with TF_SPLIT_LINEAR_TRAIN unset and set to 1, alternating.  There is no threshold: the ratios are
reported as measured.  Without a GPU the tool fails; it measures nothing on a CPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = [(256, 256), (256, 128), (256, 1024), (1024, 256)]   # (K, N)


def _backward_callable(kind, x, w, b, dy):
    from trackformer_amd import fused
    params = [t.detach().clone().requires_grad_(True) for t in (x, w, b)]
    if kind == "torch":
        y = F.linear(*params)
    else:
        fused.set_split_terms(16 if kind == "own16" else 6)
        y = fused.linear_train(*params)
        assert y is not None
    return lambda: torch.autograd.grad(y, params, dy, retain_graph=True)


def bench_shape(device, M, K, N, rounds, reps):
    from trackformer_amd import fused
    g = torch.Generator().manual_seed(K + N)
    x = torch.randn(M, K, generator=g).to(device)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(device)
    b = torch.randn(N, generator=g).to(device)
    dy = (torch.randn(M, N, generator=g) * 1e-3).to(device)
    kinds = ("own16", "own6", "torch")
    prev_terms = fused.split_terms()
    calls = {k: _backward_callable(k, x, w, b, dy) for k in kinds}
    fused.train_route_counts(reset=True)
    results = {k: calls[k]() for k in kinds}     # warm-up of every path (weight images, library algorithm selection) ...
    for k in kinds:
        for _ in range(3):
            calls[k]()
    counts = fused.train_route_counts()
    assert counts["dgrad_torch"] == 0 and counts["wgrad_torch"] == 0 and counts["bias_torch"] == 0, counts   # ... on the own kernels
    # the same numbers before the same time: the own gradients against torch's, normalised by the largest |gradient|
    diff = {k: [float((a - r).abs().max() / r.abs().max()) for a, r in zip(results[k], results["torch"])] for k in ("own16", "own6")}
    samples = {k: [] for k in kinds}
    for _ in range(rounds):
        for k in kinds:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                calls[k]()
            stop.record()
            stop.synchronize()
            samples[k].append(start.elapsed_time(stop) * 1e3 / reps)
    fused.set_split_terms(prev_terms)
    out = {"M": M, "K": K, "N": N, "rounds": rounds, "reps": reps,
           "max_abs_diff_to_torch_over_max_abs": {k: dict(zip(("dx", "dw", "db"), v)) for k, v in diff.items()}}
    for k in kinds:
        out[k + "_us"] = {"median": round(statistics.median(samples[k]), 1), "min": round(min(samples[k]), 1), "max": round(max(samples[k]), 1)}
    for k in ("own16", "own6"):
        out[k + "_over_torch"] = round(out[k + "_us"]["median"] / out["torch_us"]["median"], 3)
    return out


def bench_step(rounds, steps, warmup):
    """tools/bench_train.py with the switch off and on, alternating; every run is a fresh child process."""
    runs = {"off": [], "on": []}
    for _ in range(rounds):
        for name in ("off", "on"):
            env = dict(os.environ)
            env.pop("TF_SPLIT_LINEAR_TRAIN", None)
            if name == "on":
                env["TF_SPLIT_LINEAR_TRAIN"] = "1"
            p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)],
                               env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError("tools/bench_train.py (%s) failed:\n%s" % (name, p.stderr[-2000:]))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            r = json.loads(line)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "runs": runs}
    for name in runs:
        out[name + "_ms_per_step_median"] = round(statistics.median(r["ms_per_step"] for r in runs[name]), 2)
    out["on_over_off"] = round(out["on_ms_per_step_median"] / out["off_ms_per_step_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linear_backward_bench.json"))
    ap.add_argument("--rows", type=int, default=44446)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_linear_backward.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
              "what": "backward of one linear (stats + dgrad + wgrad [+ second pass]) per call, microseconds, device events around "
                      "`reps` calls; torch = autograd of F.linear on the same tensors in the same process",
              "shapes": [bench_shape(device, args.rows, K, N, args.rounds, args.reps) for K, N in SHAPES]}
    for s in report["shapes"]:
        print(json.dumps(s), flush=True)
    if not args.skip_step:
        torch.cuda.empty_cache()
        report["cfg3_train_step"] = bench_step(args.step_rounds, args.steps, args.warmup)
        print(json.dumps(report["cfg3_train_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
