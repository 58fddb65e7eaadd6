#!/usr/bin/env python
"""The training path of the residual + LayerNorm sites: the library's own forward + backward against torch's, the two kernels alone,
and the cfg-3 training step / the headline benchmark against a checkout of the parent commit.

    python tools/bench_layernorm_train.py [--out profiles/layernorm_train_bench.json] [--parent DIR] [--skip-kernels] [--skip-step]

Operator level.  Per shape (rows x C: the cfg-2 encoder stream at N = 2, the decoder's 2 x 400 queries, hidden 288 of cfg 4) it times,
in ONE process on the same tensors, in alternating rounds:
  * own     fused.layernorm_train(x, res, norm) and its backward: tf_add_layernorm_train_f32, then tf_add_layernorm_bwd_f32 (one pass over
            the rows + the column reduction);
  * torch   F.layer_norm(x + res, ...) and torch.autograd's backward of it: the add that writes the sum, the library's LayerNorm forward,
            its backward and its gamma / beta reduction -- the path the training step takes with the switch off.
Each sample is `reps` forward + backward calls between two device events; the figure reported is the median over the rounds, with the
smallest and the largest next to it.
Kernel level.  The tool starts itself under `rocprofv3 --kernel-trace --stats` (a run of its own, --kernels-only) and reports the average
time of add_layernorm_kernel<., true> and add_layernorm_bwd_kernel at the encoder shape with the fraction of 8 TB/s their algorithmic
traffic gives: forward reads x, res and writes out (3 rows C 4 bytes); backward reads dy, x, res and writes dz (4 rows C 4 bytes).
Step level (--parent DIR: a built checkout of the parent commit).  tools/bench_train.py (cfg 3) as alternating child processes: parent,
this tree with the switch off, this tree with TF_LAYERNORM_TRAIN=1; and bench.py --steps 120 --warmup 8 --dump-outputs for the parent
against this tree, alternating, with the dumped tracker outputs compared bit for bit (the inference kernel's template was touched).
There is no threshold: the figures are reported as measured.  Without a GPU the tool fails; it measures nothing on a CPU."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = [("encoder cfg 2, N = 2", 44446, 256), ("decoder, 2 x 400 queries", 800, 256), ("encoder hidden 288 (cfg 4), N = 2", 44446, 288),
          ("decoder hidden 288", 800, 288)]
HBM_BYTES_PER_S = 8.0e12


def _operands(device, rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x, res, dy = (torch.randn(rows, C, generator=g).to(device) for _ in range(3))
    norm = torch.nn.LayerNorm(C).to(device)
    with torch.no_grad():
        norm.weight.copy_(0.5 + torch.rand(C, generator=g))
        norm.bias.copy_(torch.randn(C, generator=g))
    return x, res, dy * 1e-3, norm


def _callable(kind, x, res, dy, norm):
    from trackformer_amd import fused
    xs, rs = x.detach().clone().requires_grad_(True), res.detach().clone().requires_grad_(True)
    params = (xs, rs, norm.weight, norm.bias)

    def call():
        y = fused.layernorm_train(xs, rs, norm) if kind == "own" else F.layer_norm(xs + rs, (x.shape[-1],), norm.weight, norm.bias, norm.eps)
        return torch.autograd.grad(y, params, dy)
    return call


def bench_shape(device, name, rows, C, rounds, reps):
    from trackformer_amd import fused
    x, res, dy, norm = _operands(device, rows, C)
    kinds = ("own", "torch")
    calls = {k: _callable(k, x, res, dy, norm) for k in kinds}
    fused.layernorm_train_counts(reset=True)
    results = {k: calls[k]() for k in kinds}
    for k in kinds:
        for _ in range(3):
            calls[k]()
    counts = fused.layernorm_train_counts()
    assert counts["torch"] == 0 and counts["own"] == 4, counts
    for _ in range(2):          # clocks and allocator warm before the first sample
        for k in kinds:
            for _ in range(reps):
                calls[k]()
    torch.cuda.synchronize(device)
    diff = [float((a - r).abs().max() / r.abs().max()) for a, r in zip(results["own"], results["torch"])]
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
    out = {"shape": name, "rows": rows, "C": C, "rounds": rounds, "reps": reps,
           "max_abs_diff_to_torch_over_max_abs": dict(zip(("dx", "dres", "dgamma", "dbeta"), diff))}
    for k in kinds:
        out[k + "_us"] = {"median": round(statistics.median(samples[k]), 1), "min": round(min(samples[k]), 1), "max": round(max(samples[k]), 1)}
    out["own_over_torch"] = round(out["own_us"]["median"] / out["torch_us"]["median"], 3)
    return out


def kernels_only(device, rows, C, iters):
    """What the profiler run executes: `iters` forward + backward calls of the own route at one shape."""
    call = _callable("own", *_operands(device, rows, C))
    for _ in range(iters):
        call()
    torch.cuda.synchronize(device)


def bench_kernels(rows, C, iters):
    """This tool under rocprofv3 --kernel-trace --stats (a run of its own) -> average time and fraction of 8 TB/s per kernel."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="ln_prof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--rows", str(rows), "--hidden", str(C), "--iters", str(iters)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n%s" % p.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        traffic = {"add_layernorm_kernel": 3, "add_layernorm_bwd_kernel": 4, "add_layernorm_bwd_reduce_kernel": 0}
        out = {"rows": rows, "C": C, "calls_per_kernel": iters, "tensor_bytes": rows * C * 4}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                if "::LnDropout>" in row["Name"]:   # add_layernorm_bwd_kernel under its dropout policy: tools/bench_dropout_train.py's row
                    continue
                for key, tensors in traffic.items():
                    if key + "<" in row["Name"] or (key in row["Name"] and key.endswith("reduce_kernel")):
                        avg_us = float(row["AverageNs"]) / 1e3
                        entry = {"name": row["Name"], "calls": int(row["Calls"]), "average_us": round(avg_us, 2),
                                 "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
                        if tensors:
                            nbytes = tensors * rows * C * 4
                            entry["algorithmic_bytes"] = nbytes
                            entry["fraction_of_8_TB_per_s"] = round(nbytes / (avg_us * 1e-6) / HBM_BYTES_PER_S, 3)
                        out[key] = entry
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _child(cmd, cwd, env, timeout=900):
    p = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError("%s (in %s) failed:\n%s" % (" ".join(cmd), cwd, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _spread(runs, key):
    vals = [r[key] for r in runs]
    return {"median": round(statistics.median(vals), 3), "min": min(vals), "max": max(vals)}


def bench_step(parent, rounds, steps, warmup):
    """tools/bench_train.py: the parent commit, this tree with the switch off, this tree with the switch on; alternating child processes."""
    legs = [("parent", parent, None), ("off", REPO, None), ("on", REPO, "1")]
    runs = {name: [] for name, root, _ in legs if root}
    for _ in range(rounds):
        for name, root, flag in legs:
            if not root:
                continue
            env = dict(os.environ)
            env.pop("TF_LAYERNORM_TRAIN", None)
            if flag:
                env["TF_LAYERNORM_TRAIN"] = flag
            r = _child([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)], root, env)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "runs": runs}
    for name in runs:
        out[name + "_ms_per_step"] = _spread(runs[name], "ms_per_step")
    base = "parent" if "parent" in runs else "off"
    out["on_over_" + base] = round(out["on_ms_per_step"]["median"] / out[base + "_ms_per_step"]["median"], 3)
    return out


def bench_headline(parent, rounds, steps, warmup):
    """bench.py (the inference benchmark) for the parent commit against this tree, alternating, with the dumped outputs compared bit for bit."""
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="ln_dump_")
    try:
        runs = {"parent": [], "this": []}
        dumps = {}
        for i in range(rounds):
            for name, root in (("parent", parent), ("this", REPO)):
                d = os.path.join(tmp, "%s_%d" % (name, i))
                r = _child([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--dump-outputs", d], root, dict(os.environ), timeout=1200)
                runs[name].append({"ms_per_step": r["ms_per_step"], "value": r["value"]})
                dumps.setdefault(name, []).append(d)
        names = sorted(os.listdir(dumps["parent"][0]))
        identical = names == sorted(os.listdir(dumps["this"][0])) and len(names) > 0
        differing = []
        for n in names:
            a, b = np.load(os.path.join(dumps["parent"][0], n)), np.load(os.path.join(dumps["this"][0], n))
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                differing.append(n)
        out = {"steps": steps, "warmup": warmup, "runs": runs, "dumped_arrays": len(names),
               "dumps_bit_identical": bool(identical and not differing), "differing_arrays": differing}
        for name in runs:
            out[name + "_ms_per_step"] = _spread(runs[name], "ms_per_step")
        p, t = out["parent_ms_per_step"], out["this_ms_per_step"]["median"]
        out["this_median_inside_parent_spread"] = bool(p["min"] <= t <= p["max"])
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layernorm_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (step level and headline against it)")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--headline-rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="(the profiler's child) run the own route --iters times and exit")
    ap.add_argument("--rows", type=int, default=44446)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    if not torch.cuda.is_available():
        sys.exit("tools/bench_layernorm_train.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    if args.kernels_only:
        kernels_only(device, args.rows, args.hidden, args.iters)
        return
    report = {"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
              "what": "forward + backward of one residual + LayerNorm site per call, microseconds, device events around `reps` calls; "
                      "torch = F.layer_norm(x + res) and its autograd on the same tensors in the same process, alternating rounds",
              "shapes": [bench_shape(device, name, rows, C, args.rounds, args.reps) for name, rows, C in SHAPES]}
    def save():   # after every stage: a later stage that fails leaves the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    for s in report["shapes"]:
        print(json.dumps(s), flush=True)
    save()
    torch.cuda.empty_cache()
    if not args.skip_kernels:
        report["kernels"] = bench_kernels(args.rows, args.hidden, args.iters)
        print(json.dumps(report["kernels"]), flush=True)
        save()
    if not args.skip_step:
        report["cfg3_train_step"] = bench_step(args.parent, args.step_rounds, args.steps, args.warmup)
        print(json.dumps(report["cfg3_train_step"]), flush=True)
        save()
    if args.parent and not args.skip_headline:
        report["headline_against_parent"] = bench_headline(args.parent, args.headline_rounds, 120, 8)
        print(json.dumps(report["headline_against_parent"]), flush=True)
        save()


if __name__ == "__main__":
    main()
