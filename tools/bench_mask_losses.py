#!/usr/bin/env python
"""The fused mask losses against today's torch chain at the shape a cfg-5 mask-model step hands SetCriterion.loss_masks, the memory each
route needs, the three kernels' own times, and the cfg-3 step / the headline against a checkout of the parent commit.

    python tools/bench_mask_losses.py [--out profiles/mask_losses_bench.json] [--parent DIR] [--skip-ops] [--skip-kernels] [--skip-step]
                                      [--skip-headline]

Operator level.  The problem is BUILT FROM THE SHAPES of a cfg-5 step at 800 x 1333, batch 2: pred_masks [2, 300, 100, 167] (the mask
head works at 1 / 8 of the padded image), 30 box-shaped bool masks per image, 30 pairs per image from a seeded permutation -- not
captured from a running model: the full-size mask-model training step did not finish inside one benchmark run (it was ended after seven
silent minutes before any kernel of this tool had been launched; the cause was not established), so the tool runs no such step.  A
second, small shape (2 x 24 queries of 32 x 40 against 5 masks per image at 128 x 160) shows the launch-bound end.  On those tensors, in
ONE process, in alternating rounds: forward + backward of loss_masks (autograd.grad of a weighted sum of the two losses with respect to
pred_masks) with criterion.set_fused_masks on (own) and off (torch).  Each sample is `reps` calls between two device events and between
two host clocks; median, smallest and largest over the rounds.  Memory: torch.cuda.max_memory_allocated over one call of each route,
above what was allocated before it.
Kernels.  The tool starts itself under `rocprofv3 --kernel-trace --stats` (a run of its own, --profile-child) on the full-size problem
and reads the three kernels' average times from the statistics.
Step level (--parent DIR: a built checkout of the parent commit).  The switch is off by default and no default path changes; what is
measured is that: tools/bench_train.py (cfg 3) as alternating child processes, parent against this tree, and ONE pair of
bench.py --steps 120 --warmup 8 runs (fused_ops.hip is recompiled).  The mask-model step with the switch on is NOT measured (see above).
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
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

KERNELS = ("mask_loss_fwd_kernel", "mask_loss_finish_kernel", "mask_loss_bwd_kernel")
SWITCH = "TF_CRITERION_FUSED_MASKS"


class Problem:
    """What one SetCriterion.loss_masks call works on."""

    def __init__(self, name, pred_masks, targets, indices, num_boxes, criterion):
        self.name, self.pred_masks, self.targets, self.indices, self.num_boxes, self.criterion = name, pred_masks, targets, indices, num_boxes, criterion
        self.weights = torch.tensor([1.25, 0.75], device=pred_masks.device)

    def dims(self):
        B, Q, h, w = self.pred_masks.shape
        H, W = max(t["masks"].shape[1] for t in self.targets), max(t["masks"].shape[2] for t in self.targets)
        return {"B": B, "Q": Q, "h": h, "w": w, "H": H, "W": W, "n": sum(len(s) for s, _ in self.indices),
                "targets": sum(t["masks"].shape[0] for t in self.targets)}


def box_masks(boxes, h, w):
    """One bool [h, w] mask per cxcywh box: the box's pixels."""
    m = torch.zeros(len(boxes), h, w, dtype=torch.bool)
    for k, (cx, cy, bw, bh) in enumerate(boxes.tolist()):
        m[k, max(0, int((cy - bh / 2) * h)):int((cy + bh / 2) * h) + 1, max(0, int((cx - bw / 2) * w)):int((cx + bw / 2) * w) + 1] = True
    return m


def mask_criterion():
    from trackformer_amd.criterion import SetCriterion
    from trackformer_amd.matcher import HungarianMatcher
    mt = HungarianMatcher(2.0, 5.0, 2.0, focal_loss=True, focal_alpha=0.25, focal_gamma=2.0)
    return SetCriterion(1, mt, {}, 0.1, ["labels", "boxes", "cardinality", "masks"], True, 0.25, 2.0, False, 0.0)


def synthetic(device, criterion, B=2, Q=24, h=32, w=40, H=128, W=160, per_image=5, name=None):
    g = torch.Generator().manual_seed(B * Q + h)
    pred = torch.randn(B, Q, h, w, generator=g).to(device)
    targets, indices = [], []
    for _ in range(B):
        boxes = torch.cat([torch.rand(per_image, 2, generator=g) * 0.8 + 0.1, torch.rand(per_image, 2, generator=g) * 0.15 + 0.03], 1)
        targets.append({"masks": box_masks(boxes, H, W).to(device)})
        indices.append((torch.randperm(Q, generator=g)[:per_image].sort().values, torch.randperm(per_image, generator=g)))
    return Problem(name or "synthetic, %d x %d -> %d x %d" % (h, w, H, W), pred, targets, indices, float(B * per_image), criterion)


def route_callable(prob, own):
    from trackformer_amd import criterion as C
    pm = prob.pred_masks.clone().requires_grad_(True)

    def call():
        prev = C._fused_masks
        C.set_fused_masks(own)
        try:
            out = prob.criterion.loss_masks({"pred_masks": pm}, prob.targets, prob.indices, prob.num_boxes)
        finally:
            C.set_fused_masks(prev)
        total = out["loss_mask"] * prob.weights[0] + out["loss_dice"] * prob.weights[1]
        grad, = torch.autograd.grad(total, pm)
        return grad, torch.stack([out["loss_mask"].detach(), out["loss_dice"].detach()])
    return call


def peak_memory(device, call):
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(device)
    torch.cuda.reset_peak_memory_stats(device)
    out = call()
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - base
    del out
    return peak


def bench_pair(device, prob, rounds, reps):
    from trackformer_amd import criterion as C
    calls = {"own": route_callable(prob, True), "torch": route_callable(prob, False)}
    C.fused_mask_counts(reset=True)
    results = {k: calls[k]() for k in calls}
    counts = C.fused_mask_counts(reset=True)
    if counts != {"own": 1, "torch": 0}:
        raise RuntimeError("the own route did not run on %s: %r" % (prob.name, counts))
    for k in calls:
        for _ in range(2):
            calls[k]()
    torch.cuda.synchronize(device)
    diff = [float((a - r).abs().max() / r.abs().max().clamp_min(1e-30)) for a, r in zip(results["own"], results["torch"])]
    del results
    mem = {k: peak_memory(device, calls[k]) for k in calls}
    ev, wall = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(rounds):
        for k in calls:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            start.record()
            for _ in range(reps):
                calls[k]()
            stop.record()
            stop.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e6 / reps)
            ev[k].append(start.elapsed_time(stop) * 1e3 / reps)
    out = {"shape": prob.name, **prob.dims(), "rounds": rounds, "reps": reps,
           "max_abs_diff_to_torch_over_max_abs (grad, losses)": [float("%.3g" % d) for d in diff]}
    for k in calls:
        out[k + "_us"] = {"median": round(statistics.median(ev[k]), 1), "min": round(min(ev[k]), 1), "max": round(max(ev[k]), 1)}
        out[k + "_host_us"] = {"median": round(statistics.median(wall[k]), 1), "min": round(min(wall[k]), 1), "max": round(max(wall[k]), 1)}
        out[k + "_peak_bytes_above_inputs"] = int(mem[k])
    out["own_over_torch"] = round(out["own_us"]["median"] / out["torch_us"]["median"], 3)
    return out


def full_size(device, criterion):
    """The shape of a cfg-5 step at 800 x 1333, batch 2 (module docstring)."""
    return synthetic(device, criterion, 2, 300, 100, 167, 800, 1333, 30, "cfg-5 shape: 2 x 300 queries of 100 x 167 against 30 masks per image at 800 x 1333")


def profile_child(device, iters):
    """(the profiler's child) `iters` forward + backward calls of the own route on the step's problem."""
    prob = full_size(device, mask_criterion().to(device))
    call = route_callable(prob, True)
    call()
    torch.cuda.synchronize(device)
    for _ in range(iters):
        call()
    torch.cuda.synchronize(device)


def bench_kernels(iters):
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    tmp = tempfile.mkdtemp(prefix="mask_prof_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--profile-child", "--iters", str(iters)]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run failed:\n%s" % p.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % tmp)
        out = {"iters": iters}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
                    if k in row.get("Name", ""):
                        out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 1),
                                  "min_us": round(float(row["MinNs"]) / 1e3, 1), "max_us": round(float(row["MaxNs"]) / 1e3, 1)}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _child(cmd, cwd, env, timeout=1200):
    p = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError("%s (in %s) failed:\n%s" % (" ".join(cmd), cwd, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _spread(runs, key):
    vals = [r[key] for r in runs]
    return {"median": round(statistics.median(vals), 3), "min": min(vals), "max": max(vals)}


def bench_step(parent, rounds, steps, warmup):
    """tools/bench_train.py (cfg 3; the switch is off): the parent commit against this tree, alternating child processes."""
    legs = [("cfg3_parent", parent), ("cfg3_this", REPO)]
    runs = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, root in legs:
            env = dict(os.environ)
            env.pop(SWITCH, None)
            print("step: %s ..." % name, flush=True)
            r = _child([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)], root, env)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "runs": runs}
    for name in runs:
        out[name + "_ms_per_step"] = _spread(runs[name], "ms_per_step")
    out["cfg3_this_over_parent"] = round(out["cfg3_this_ms_per_step"]["median"] / out["cfg3_parent_ms_per_step"]["median"], 3)
    return out


def bench_headline(parent, steps, warmup):
    """ONE pair of bench.py runs, the parent commit against this tree."""
    out = {"steps": steps, "warmup": warmup}
    for name, root in (("parent", parent), ("this", REPO)):
        print("headline: %s ..." % name, flush=True)
        r = _child([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], root,
                   dict(os.environ))
        out[name] = {"ms_per_step": r.get("ms_per_step"), "value": r.get("value")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mask_losses_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (cfg-3 step and headline against it)")
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-child", action="store_true", help="(the profiler's child) run the own route --iters times and exit")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    if not torch.cuda.is_available():
        sys.exit("tools/bench_mask_losses.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    if args.profile_child:
        profile_child(device, args.iters)
        return
    report = {}
    if os.path.exists(args.out):          # the stages may be run one call at a time: keep what an earlier call measured
        with open(args.out) as f:
            report = json.load(f)
    report.update({"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
                   "what": "loss_masks: forward + backward (gradient entering pred_masks) per call; microseconds, `reps` calls between "
                           "device events (_us) and host clocks (_host_us); torch = today's chain on the same tensors in the same process, "
                           "alternating rounds; peak bytes: torch.cuda.max_memory_allocated over one call above what was allocated before it"})

    def save():   # after every stage: a later stage that fails leaves the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    if not args.skip_ops:
        crit = mask_criterion().to(device)
        step, small = full_size(device, crit), synthetic(device, crit)
        report["loss_masks"] = []
        for p in (step, small):
            print("loss_masks: %s ..." % p.name, flush=True)
            report["loss_masks"].append(bench_pair(device, p, args.rounds, args.reps if p is step else 4 * args.reps))
            print(json.dumps(report["loss_masks"][-1]), flush=True)
        save()
        del step, small
        torch.cuda.empty_cache()
    if not args.skip_kernels:
        report["kernels"] = bench_kernels(args.iters)
        print(json.dumps(report["kernels"]), flush=True)
        save()
    if args.parent and not args.skip_step:
        report["train_step"] = bench_step(args.parent, args.step_rounds, args.steps, args.warmup)
        print(json.dumps(report["train_step"]), flush=True)
        save()
    if args.parent and not args.skip_headline:
        report["headline_against_parent"] = bench_headline(args.parent, 120, 8)
        print(json.dumps(report["headline_against_parent"]), flush=True)
        save()


if __name__ == "__main__":
    main()
