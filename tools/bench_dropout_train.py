#!/usr/bin/env python
"""Dropout inside the training kernels (fused.set_dropout_training): the library's own forward + backward per site against today's routes,
the kernels alone, and the cfg-3 training step / the headline benchmark against a checkout of the parent commit.

    python tools/bench_dropout_train.py [--out profiles/dropout_train_bench.json] [--parent DIR] [--skip-kernels] [--skip-step]

Operator level, in ONE process on the same tensors, in alternating rounds, forward + backward per call, dropout 0.1:
  residual sites (rows x C: the cfg-2 encoder stream at N = 2, hidden 288 of cfg 4, the decoder's 2 x 400 queries)
    * own     tf_add_dropout_layernorm_train_f32 + tf_add_dropout_layernorm_bwd_f32 (the mask recomputed, nothing of it stored)
    * optin   F.dropout(res) + fused.layernorm_train: today's route with set_layernorm_training(True)
    * plain   F.layer_norm(x + F.dropout(res)) and torch.autograd's backward of it
  the feed-forward hidden site (44 446 x 256 -> 1024)
    * own     fused.linear_train(x, w, b, relu=True, dropout=module)
    * optin   F.dropout(fused.linear_train(x, w, b, relu=True)): today's route with set_split_linear_training(True)
    * plain   F.dropout(relu(F.linear(x, w, b)))
Each sample is `reps` calls between two device events; the figure reported is the median over the rounds with the smallest and the
largest next to it.  peak_bytes_above_inputs: torch.cuda.max_memory_allocated over one call, above what was allocated before it.
Kernel level.  The tool starts itself under `rocprofv3 --kernel-trace --stats` (a run of its own, --kernels-only) and reports the average
time of the four new kernels with the fraction of 8 TB/s their algorithmic traffic gives.
Step level (--parent DIR: a built checkout of the parent commit).  tools/bench_train.py (cfg 3, dropout 0.1) as alternating child
processes with TF_LAYERNORM_TRAIN=1 TF_SPLIT_LINEAR_TRAIN=1 in every leg (the parent routes of the new one): parent, this tree with the
switch off, this tree with TF_DROPOUT_TRAIN=1; and bench.py --steps 120 --warmup 8 --dump-outputs for the parent against this tree,
alternating, with the dumped tracker outputs compared bit for bit (fused_ops.hip was recompiled).
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

from tools.bench_layernorm_train import HBM_BYTES_PER_S, _child, _spread, bench_headline   # noqa: E402

P = 0.1
LN_SHAPES = [("encoder cfg 2, N = 2", 44446, 256), ("encoder hidden 288 (cfg 4), N = 2", 44446, 288), ("decoder, 2 x 400 queries", 800, 256)]
FFN_SHAPE = ("encoder feed-forward hidden, cfg 2, N = 2", 44446, 256, 1024)
KINDS = ("own", "optin", "plain")
PARENT_ROUTES = {"TF_LAYERNORM_TRAIN": "1", "TF_SPLIT_LINEAR_TRAIN": "1"}


def _ln_site(device, rows, C):
    from trackformer_amd import fused
    g = torch.Generator().manual_seed(rows + C)
    x, res, dy = (torch.randn(rows, C, generator=g).to(device) for _ in range(3))
    dy *= 1e-3
    norm = torch.nn.LayerNorm(C).to(device)
    drop = torch.nn.Dropout(P).train()
    xs, rs = x.requires_grad_(True), res.requires_grad_(True)
    params = (xs, rs, norm.weight, norm.bias)

    def call(kind):
        if kind == "own":
            y = fused.dropout_residual_norm(xs, rs, norm, drop)
        elif kind == "optin":
            y = fused.layernorm_train(xs, F.dropout(rs, P, True), norm)
        else:
            y = F.layer_norm(xs + F.dropout(rs, P, True), (C,), norm.weight, norm.bias, norm.eps)
        return torch.autograd.grad(y, params, dy)
    return call


def _ffn_site(device, rows, K, N):
    from trackformer_amd import fused
    g = torch.Generator().manual_seed(rows + N)
    x = torch.randn(rows, K, generator=g).to(device).requires_grad_(True)
    dy = torch.randn(rows, N, generator=g).to(device) * 1e-3
    lin = torch.nn.Linear(K, N).to(device)
    drop = torch.nn.Dropout(P).train()
    params = (x, lin.weight, lin.bias)

    def call(kind):
        if kind == "own":
            y = fused.linear_train(x, lin.weight, lin.bias, relu=True, dropout=drop)
        elif kind == "optin":
            y = F.dropout(fused.linear_train(x, lin.weight, lin.bias, relu=True), P, True)
        else:
            y = F.dropout(torch.relu(F.linear(x, lin.weight, lin.bias)), P, True)
        return torch.autograd.grad(y, params, dy)
    return call


def _switches_on():
    from trackformer_amd import fused
    fused.set_dropout_training(True)
    fused.set_layernorm_training(True)
    fused.set_split_linear_training(True)


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
    out = dict(describe, rounds=rounds, reps=reps, dropout=P, peak_bytes_above_inputs=peak)
    for k in KINDS:
        out[k + "_us"] = {"median": round(statistics.median(samples[k]), 1), "min": round(min(samples[k]), 1), "max": round(max(samples[k]), 1)}
    out["own_over_optin"] = round(out["own_us"]["median"] / out["optin_us"]["median"], 3)
    out["own_over_plain"] = round(out["own_us"]["median"] / out["plain_us"]["median"], 3)
    return out


def kernels_only(device, iters):
    """What the profiler run executes: `iters` forward + backward calls of the own route at the encoder shapes."""
    _switches_on()
    ln, ffn = _ln_site(device, *LN_SHAPES[0][1:]), _ffn_site(device, *FFN_SHAPE[1:])
    for _ in range(iters):
        ln("own")
        ffn("own")
    torch.cuda.synchronize(device)


def bench_kernels(iters):
    """This tool under rocprofv3 --kernel-trace --stats (a run of its own) -> average time and fraction of 8 TB/s per kernel."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="dropout_prof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--iters", str(iters)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n%s" % p.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        rows, C, F_ = LN_SHAPES[0][1], LN_SHAPES[0][2], FFN_SHAPE[3]
        # kernel -> algorithmic bytes: forward reads x, res and writes out; backward reads dy, x, res and writes dx, dres; in place reads
        # and writes y; the ReLU + dropout backward reads dy, y and writes out
        # the backward is add_layernorm_bwd_kernel under its dropout policy: the policy type among the template arguments tells it from the
        # instantiations without dropout (LnNoDropout), so every part of a key must occur in the profiler's name
        traffic = {("add_dropout_layernorm_kernel",): 3 * rows * C * 4, ("add_layernorm_bwd_kernel<", "::LnDropout>"): 5 * rows * C * 4,
                   ("dropout_inplace_kernel",): 2 * rows * F_ * 4, ("relu_dropout_bwd_kernel",): 3 * rows * F_ * 4}
        out = {"calls_per_kernel": iters, "ln_shape": [rows, C], "ffn_hidden_shape": [rows, F_]}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for parts, nbytes in traffic.items():
                    if all(part in row["Name"] for part in parts):
                        key = "".join(parts).replace("::", "")
                        avg_us = float(row["AverageNs"]) / 1e3
                        out[key] = {"name": row["Name"], "calls": int(row["Calls"]), "average_us": round(avg_us, 2),
                                    "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2),
                                    "algorithmic_bytes": nbytes, "fraction_of_8_TB_per_s": round(nbytes / (avg_us * 1e-6) / HBM_BYTES_PER_S, 3)}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def bench_step(parent, rounds, steps, warmup):
    """tools/bench_train.py with the parent routes on: the parent commit, this tree with the switch off, this tree with it on."""
    legs = [("parent", parent, None), ("off", REPO, None), ("on", REPO, "1")]
    runs = {name: [] for name, root, _ in legs if root}
    for _ in range(rounds):
        for name, root, flag in legs:
            if not root:
                continue
            env = dict(os.environ, **PARENT_ROUTES)
            env.pop("TF_DROPOUT_TRAIN", None)
            if flag:
                env["TF_DROPOUT_TRAIN"] = flag
            r = _child([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)], root, env)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "environment_of_every_leg": PARENT_ROUTES, "runs": runs}
    for name in runs:
        out[name + "_ms_per_step"] = _spread(runs[name], "ms_per_step")
    base = "parent" if "parent" in runs else "off"
    out["on_over_" + base] = round(out["on_ms_per_step"]["median"] / out[base + "_ms_per_step"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dropout_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (step level and headline against it)")
    ap.add_argument("--skip-sites", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--headline-rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true", help="(the profiler's child) run the own route --iters times and exit")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    if not torch.cuda.is_available():
        sys.exit("tools/bench_dropout_train.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    if args.kernels_only:
        kernels_only(device, args.iters)
        return
    report = {}
    if os.path.exists(args.out):      # the stages may be run one at a time: a stage replaces its own section only
        with open(args.out) as f:
            report = json.load(f)
    report.update({"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
                   "what": "forward + backward of one dropout site per call, microseconds, device events around `reps` calls; own / optin / "
                           "plain on the same tensors in the same process, alternating rounds (see the tool's docstring)"})

    def save():   # after every stage: a later stage that fails leaves the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    if not args.skip_sites:
        from trackformer_amd import fused
        _switches_on()
        fused.dropout_train_counts(reset=True)
        report["residual_sites"] = [bench_site(device, _ln_site(device, rows, C), args.rounds, args.reps, shape=name, rows=rows, C=C)
                                    for name, rows, C in LN_SHAPES]
        name, rows, K, N = FFN_SHAPE
        report["ffn_hidden_site"] = bench_site(device, _ffn_site(device, rows, K, N), args.rounds, max(args.reps // 4, 2), shape=name, rows=rows,
                                               K=K, N=N)
        counts = fused.dropout_train_counts()
        assert counts["ln_own"] > 0 and counts["ln_torch"] == 0, counts
        for s in report["residual_sites"] + [report["ffn_hidden_site"]]:
            print(json.dumps(s), flush=True)
        for flag in (fused.set_dropout_training, fused.set_layernorm_training, fused.set_split_linear_training):
            flag(None)
        save()
        torch.cuda.empty_cache()
    if not args.skip_kernels:
        report["kernels"] = bench_kernels(args.iters)
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
