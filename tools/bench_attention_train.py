#!/usr/bin/env python
"""Training through the decoder self-attention (fused.set_attention_training): forward + backward of the whole site -- projections,
attention core, out-projection -- on the library's own kernels against today's nn.MultiheadAttention call, the kernels alone, and the
cfg-3 training step / the headline benchmark against a checkout of the parent commit.

    python tools/bench_attention_train.py [--out profiles/attention_train_bench.json] [--parent DIR] [--skip-kernels] [--skip-step]

Site level, in ONE process on the same tensors and the same module, in alternating rounds, forward + backward per call:
  shapes  2 x 400 x 256, 8 heads (cfg 2 / 3)  and  2 x 800 x 288, 8 heads (cfg 4, head dimension 36); each with dropout 0 and 0.1
    * own     DeformableTransformerDecoderLayer.self_attention_training with set_attention_training(True) (and set_dropout_training(True)
              where the module drops); the projections are F.linear, or fused.linear_train with --split-linear
    * torch   the same method with the switch off: q = k = tgt + pos, self_attn(q^T, k^T, tgt^T)[0]^T
Each sample is `reps` calls between two device events; the figure reported is the median over the rounds with the smallest and the
largest next to it.  peak_bytes_above_inputs: torch.cuda.max_memory_allocated over one call, above what was allocated before it.
Kernel level.  The tool starts itself under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters; --kernels-only ROUTE) once
per route and reports every kernel's calls and average time, and the dispatches per site.
Step level (--parent DIR: a built checkout of the parent commit).  tools/bench_train.py (cfg 3) as alternating child processes: parent,
this tree with the switch off, this tree with TF_ATTENTION_TRAIN=1 (TF_DROPOUT_TRAIN=1 TF_LAYERNORM_TRAIN=1 TF_SPLIT_LINEAR_TRAIN=1 in
every leg: the step trains with dropout 0.1 and a site that drops needs the generator contract); and bench.py --steps 120 --warmup 8
--dump-outputs for the parent against this tree, alternating, with the dumped tracker outputs compared bit for bit (mha_core.hip was
recompiled).
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.bench_layernorm_train import _child, _spread, bench_headline   # noqa: E402

SHAPES = [("cfg 2 / 3: 2 x 400 x 256, 8 heads", 2, 400, 256, 8), ("cfg 4: 2 x 800 x 288, 8 heads (D = 36)", 2, 800, 288, 8)]
DROPOUTS = (0.0, 0.1)
KINDS = ("own", "torch")
STEP_ROUTES = {"TF_DROPOUT_TRAIN": "1", "TF_LAYERNORM_TRAIN": "1", "TF_SPLIT_LINEAR_TRAIN": "1"}


def _site(device, n, length, e, heads, p, split_linear=False):
    from trackformer_amd import fused
    from trackformer_amd.deformable_transformer import DeformableTransformerDecoderLayer
    torch.manual_seed(length + e)
    layer = DeformableTransformerDecoderLayer(d_model=e, d_ffn=64, dropout=p, n_levels=1, n_heads=heads, n_points=1).to(device).train()
    g = torch.Generator().manual_seed(length)
    tgt, pos, dy = (torch.randn(n, length, e, generator=g).to(device) for _ in range(3))
    dy *= 1e-3
    tgt.requires_grad_(True)
    mha = layer.self_attn
    params = (tgt, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias)

    def call(kind):
        fused.set_attention_training(kind == "own")
        fused.set_dropout_training(kind == "own" and p > 0)
        fused.set_split_linear_training(kind == "own" and split_linear)
        y = layer.self_attention_training(tgt, pos, None)
        return torch.autograd.grad(y, params, dy)
    return call


def _switches_off():
    from trackformer_amd import fused
    for flag in (fused.set_attention_training, fused.set_dropout_training, fused.set_split_linear_training):
        flag(None)


def bench_site(device, call, rounds, reps, **describe):
    for k in KINDS:
        for _ in range(4):
            call(k)
    for _ in range(2):          # clocks and allocator warm before the first sample
        for k in KINDS:
            for _ in range(reps):
                call(k)
    torch.cuda.synchronize(device)
    peak = {}
    for k in KINDS:
        torch.cuda.synchronize(device)
        torch.cuda.reset_peak_memory_stats(device)
        base = torch.cuda.memory_allocated(device)
        call(k)
        torch.cuda.synchronize(device)
        peak[k] = int(torch.cuda.max_memory_allocated(device) - base)
    samples = {k: [] for k in KINDS}
    for _ in range(rounds):
        for k in KINDS:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                call(k)
            stop.record()
            stop.synchronize()
            samples[k].append(start.elapsed_time(stop) * 1e3 / reps)
    out = dict(describe, rounds=rounds, reps=reps, peak_bytes_above_inputs=peak)
    for k in KINDS:
        out[k + "_us"] = {"median": round(statistics.median(samples[k]), 1), "min": round(min(samples[k]), 1), "max": round(max(samples[k]), 1)}
    out["own_over_torch"] = round(out["own_us"]["median"] / out["torch_us"]["median"], 3)
    return out


def kernels_only(device, route, iters, p):
    """What the profiler run executes: `iters` forward + backward calls of one route at the cfg-2 / 3 shape."""
    _, n, length, e, heads = SHAPES[0]
    call = _site(device, n, length, e, heads, p)
    for _ in range(iters):
        call(route)
    torch.cuda.synchronize(device)


def bench_kernels(iters, p):
    """This tool under rocprofv3 --kernel-trace --stats, one run per route -> the kernels of a site, their calls and average times."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    out = {"sites_per_run": iters, "shape": SHAPES[0][0], "dropout": p}
    for route in KINDS:
        tmp = tempfile.mkdtemp(prefix="attention_prof_")
        try:
            cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--kernels-only", route, "--iters", str(iters), "--kernel-dropout", str(p)]
            r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("rocprofv3 run failed:\n%s" % r.stderr[-2000:])
            files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
            kernels, calls, total_ns = [], 0, 0.0
            with open(files[0]) as f:
                for row in csv.DictReader(f):
                    c = int(row["Calls"])
                    if c < iters:      # set-up kernels (parameter initialisation, the operands): not part of a site
                        continue
                    calls += c
                    total_ns += float(row["TotalDurationNs"])
                    kernels.append({"name": row["Name"][:120], "calls": c, "average_us": round(float(row["AverageNs"]) / 1e3, 2)})
            out[route] = {"dispatches_per_site": round(calls / iters, 1), "kernel_us_per_site": round(total_ns / 1e3 / iters, 1),
                          "kernels": kernels}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return out


def bench_step(parent, rounds, steps, warmup):
    legs = [("parent", parent, None), ("off", REPO, None), ("on", REPO, "1")]
    runs = {name: [] for name, root, _ in legs if root}
    for _ in range(rounds):
        for name, root, flag in legs:
            if not root:
                continue
            env = dict(os.environ, **STEP_ROUTES)
            env.pop("TF_ATTENTION_TRAIN", None)
            if flag:
                env["TF_ATTENTION_TRAIN"] = flag
            r = _child([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)], root, env)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "environment_of_every_leg": STEP_ROUTES, "runs": runs}
    for name in runs:
        out[name + "_ms_per_step"] = _spread(runs[name], "ms_per_step")
    base = "parent" if "parent" in runs else "off"
    out["on_over_" + base] = round(out["on_ms_per_step"]["median"] / out[base + "_ms_per_step"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attention_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (step level and headline against it)")
    ap.add_argument("--split-linear", action="store_true", help="the own route's projections through fused.linear_train")
    ap.add_argument("--skip-sites", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--headline-rounds", type=int, default=2)
    ap.add_argument("--kernels-only", default=None, choices=KINDS, help="(the profiler's child) run one route --iters times and exit")
    ap.add_argument("--kernel-dropout", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    if not torch.cuda.is_available():
        sys.exit("tools/bench_attention_train.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    if args.kernels_only:
        kernels_only(device, args.kernels_only, args.iters, args.kernel_dropout)
        return
    report = {}
    if os.path.exists(args.out):      # the stages may be run one at a time: a stage replaces its own section only
        with open(args.out) as f:
            report = json.load(f)
    report.update({"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
                   "what": "forward + backward of one decoder self-attention site per call (projections, core, out-projection), microseconds, "
                           "device events around `reps` calls; own / torch on the same tensors in the same process, alternating rounds (see "
                           "the tool's docstring)"})

    def save():   # after every stage: a later stage that fails leaves the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    if not args.skip_sites:
        from trackformer_amd import fused
        fused.attention_train_counts(reset=True)
        sites = []
        for name, n, length, e, heads in SHAPES:
            for p in DROPOUTS:
                sites.append(bench_site(device, _site(device, n, length, e, heads, p, args.split_linear), args.rounds, args.reps, shape=name,
                                        dropout=p, projections="linear_train" if args.split_linear else "F.linear"))
                print(json.dumps(sites[-1]), flush=True)
        counts = fused.attention_train_counts()
        assert counts["own"] > 0 and counts["own_dropout"] > 0 and counts["torch"] == 0, counts
        report["sites"] = sites
        _switches_off()
        save()
        torch.cuda.empty_cache()
    if not args.skip_kernels:
        report["kernels"] = bench_kernels(args.iters, args.kernel_dropout)
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
