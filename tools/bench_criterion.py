#!/usr/bin/env python
"""The fused set criterion and the matching-cost kernel against today's torch chains, the launch count of each route, and the cfg-3
training step / the headline benchmark against a checkout of the parent commit.

    python tools/bench_criterion.py [--out profiles/criterion_fused_bench.json] [--parent DIR] [--skip-ops] [--skip-launches]
                                    [--skip-step] [--skip-headline]

Operator level.  The shape is READ FROM A REAL STEP: the tool builds the cfg-3 model of tools/bench_train.py, runs one training step
and keeps what SetCriterion.forward and the matcher were handed (the stacked predictions of the decoder layers, the targets, the
matcher's pairs) -- L, B, Q, C and T are whatever that step produced.  A second shape has 91 classes and 300 queries (6 layers, 2
images, the step's number of targets), matched by the same matcher.  On those tensors, in ONE process, in alternating rounds:
  * criterion   own: SetCriterion._layers_fused (numpy tgt_of + one upload + tf_set_criterion_fwd_f32) and autograd.grad of the
                weighted sum (tf_set_criterion_bwd_f32); torch: SetCriterion._layers_at_once and its autograd -- forward + backward.
                Both include what engine.train_step does with the dict: the weighted sum over the 3 L loss keys, one multiply and one
                add per key and their backward (the same launches in both routes);
  * cost        own: fused.match_cost (tf_match_cost_f32); torch: HungarianMatcher._cost_torch -- the device part of match_many, without
                the copy to the host that both share.
Each sample is `reps` calls between two device events AND between two host clocks (the second after a synchronize): these routes are
launch-bound, the host time is the one a host-bound training step pays.  Median, smallest and largest over the rounds.
Launches.  The tool starts itself under `rocprofv3 --kernel-trace` once per route (a run of its own each, --count-route) on tensors of
the step's shape and counts the kernel dispatches from the trace, with `iters` and with 2 x `iters` calls: the difference is what the
calls themselves launch.
Step level (--parent DIR: a built checkout of the parent commit).  tools/bench_train.py (cfg 3) as alternating child processes: parent,
this tree with both switches off, this tree with TF_CRITERION_FUSED=1 TF_MATCHER_FUSED_COST=1; and ONE pair of
bench.py --steps 120 --warmup 8 runs, parent against this tree (fused_ops.hip is recompiled).
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

ROUTES = ("criterion_own", "criterion_torch", "cost_own", "cost_torch")


class Problem:
    """What one SetCriterion.forward call of a step works on."""

    def __init__(self, name, logits, boxes, targets, all_indices, num_boxes, criterion):
        self.name, self.logits, self.boxes, self.targets, self.all_indices = name, logits, boxes, targets, all_indices
        self.num_boxes, self.criterion = num_boxes, criterion
        self.L, self.B, self.Q, self.C = logits.shape
        self.T = sum(len(t["labels"]) for t in targets)
        g = torch.Generator().manual_seed(self.Q + self.C)
        self.weights = (torch.rand(self.L, 3, generator=g) + 0.5).to(logits.device)

    def dims(self):
        return {"L": self.L, "B": self.B, "Q": self.Q, "C": self.C, "T": self.T}

    def layer_outputs(self, lg, bx):
        return [{"pred_logits": lg[l], "pred_boxes": bx[l]} for l in range(self.L)]


def capture_step(device):
    """One cfg-3 training step of tools/bench_train.py -> the Problem its criterion saw (detached copies)."""
    from tools import bench_train
    from trackformer_amd import config, engine, factory
    margs = config.make_args('deformable', 'tracking', 'mot17', device=str(device))
    torch.manual_seed(42)
    model, criterion, _ = factory.build_model(margs)
    model.to(device).train()
    criterion.train()
    optimizer, _ = engine.build_optimizer(model, margs)
    samples, targets = bench_train.synthetic_batch(device, 2, 800, 1333, seed=0)
    seen = {}
    orig_forward, orig_match = criterion.forward, criterion.matcher.match_many

    def match_many(outputs_list, tg):
        res = orig_match(outputs_list, tg)
        if len(outputs_list) > 1:
            seen["indices"] = res
        return res

    def forward(outputs, tg):
        layers = [outputs] + list(outputs.get("aux_outputs", []))
        seen["logits"] = torch.stack([o["pred_logits"].detach() for o in layers]).clone()
        seen["boxes"] = torch.stack([o["pred_boxes"].detach() for o in layers]).clone()
        seen["targets"] = [{"labels": t["labels"].clone(), "boxes": t["boxes"].clone()} for t in tg]
        return orig_forward(outputs, tg)

    criterion.forward = forward
    criterion.matcher.__dict__["match_many"] = match_many
    try:
        tg = [dict(t, prev_target=dict(t['prev_target'])) for t in targets]
        engine.train_step(model, criterion, optimizer, samples, tg, clip_max_norm=margs.clip_max_norm)
    finally:
        criterion.forward = orig_forward
        criterion.matcher.__dict__.pop("match_many", None)
    torch.cuda.synchronize(device)
    num_boxes = float(max(sum(len(t["labels"]) for t in seen["targets"]), 1))
    prob = Problem("cfg-3 step", seen["logits"], seen["boxes"], seen["targets"], seen["indices"], num_boxes, criterion)
    del model, optimizer
    torch.cuda.empty_cache()
    return prob


def synthetic(device, criterion, L, B, Q, C, per_image, name):
    """Random predictions of the given shape, matched by the criterion's own matcher."""
    g = torch.Generator().manual_seed(L * Q + C)
    logits = (torch.randn(L, B, Q, C, generator=g) * 2 - 3).to(device)
    boxes = torch.cat([torch.rand(L, B, Q, 2, generator=g) * 0.8 + 0.1, torch.rand(L, B, Q, 2, generator=g) * 0.15 + 0.03], -1).to(device)
    targets = []
    for _ in range(B):
        tb = torch.cat([torch.rand(per_image, 2, generator=g) * 0.8 + 0.1, torch.rand(per_image, 2, generator=g) * 0.15 + 0.03], -1)
        targets.append({"labels": torch.randint(0, C, (per_image,), generator=g).to(device), "boxes": tb.to(device)})
    from trackformer_amd.criterion import SetCriterion
    crit = SetCriterion(C, criterion.matcher, {}, 0.1, ["labels", "boxes", "cardinality"], True, criterion.focal_alpha, criterion.focal_gamma,
                        False, 0.0).to(device)
    prob = Problem(name, logits, boxes, targets, None, float(B * per_image), crit)
    prob.all_indices = crit.matcher.match_many(prob.layer_outputs(logits, boxes), targets)
    return prob


def route_callable(prob, route):
    from trackformer_amd import fused
    crit = prob.criterion
    if route.startswith("criterion"):
        lg, bx = prob.logits.clone().requires_grad_(True), prob.boxes.clone().requires_grad_(True)
        fn = crit._layers_fused if route == "criterion_own" else crit._layers_at_once
        keys = [k + s for s in [""] + ["_%d" % i for i in range(prob.L - 1)] for k in ("loss_ce", "loss_bbox", "loss_giou")]
        w = prob.weights.reshape(-1)

        def call():
            out = fn(prob.layer_outputs(lg, bx), prob.targets, prob.all_indices, prob.num_boxes)
            total = sum(out[k] * w[i] for i, k in enumerate(keys))
            return torch.autograd.grad(total, (lg, bx)) + (torch.stack([out[k].detach() for k in keys]),)
        return call
    mt = crit.matcher
    lg, bx = prob.logits.flatten(0, 2), prob.boxes.flatten(0, 2)
    ids, tb = torch.cat([t["labels"] for t in prob.targets]), torch.cat([t["boxes"] for t in prob.targets])
    if route == "cost_own":
        return lambda: (fused.match_cost(lg, bx, ids, tb, mt.cost_class, mt.cost_bbox, mt.cost_giou, mt.focal_alpha, mt.focal_gamma),)
    return lambda: (mt._cost_torch(lg, bx, ids, tb),)


def bench_pair(device, prob, own, ref, rounds, reps):
    calls = {k: route_callable(prob, k) for k in (own, ref)}
    with torch.no_grad() if own.startswith("cost") else torch.enable_grad():
        results = {k: calls[k]() for k in calls}
        for _ in range(2):
            for k in calls:
                for _ in range(reps):
                    calls[k]()
        torch.cuda.synchronize(device)
        diff = [float((a - r).abs().max() / r.abs().max().clamp_min(1e-30)) for a, r in zip(results[own], results[ref])]
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
    out = {"shape": prob.name, **prob.dims(), "rounds": rounds, "reps": reps, "max_abs_diff_to_torch_over_max_abs": [float("%.3g" % d) for d in diff]}
    for k, label in ((own, "own"), (ref, "torch")):
        out[label + "_us"] = {"median": round(statistics.median(ev[k]), 1), "min": round(min(ev[k]), 1), "max": round(max(ev[k]), 1)}
        out[label + "_host_us"] = {"median": round(statistics.median(wall[k]), 1), "min": round(min(wall[k]), 1), "max": round(max(wall[k]), 1)}
    out["own_over_torch"] = round(out["own_us"]["median"] / out["torch_us"]["median"], 3)
    return out


def count_route(device, route, dims, iters):
    """(the profiler's child) `iters` calls of one route on tensors of the given shape."""
    from trackformer_amd.criterion import SetCriterion
    from trackformer_amd.matcher import HungarianMatcher
    mt = HungarianMatcher(2.0, 5.0, 2.0, focal_loss=True, focal_alpha=0.25, focal_gamma=2.0)
    crit = SetCriterion(dims["C"], mt, {}, 0.1, ["labels", "boxes", "cardinality"], True, 0.25, 2.0, False, 0.0).to(device)
    prob = synthetic(device, crit, dims["L"], dims["B"], dims["Q"], dims["C"], dims["T"] // dims["B"], "count")
    call = route_callable(prob, route)
    with torch.no_grad() if route.startswith("cost") else torch.enable_grad():
        call()
        torch.cuda.synchronize(device)
        print("COUNT_BEGIN", flush=True)
        for _ in range(iters):
            call()
    torch.cuda.synchronize(device)


def bench_launches(dims, iters):
    """Kernel dispatches per call of every route: this tool under rocprofv3 --kernel-trace, once per route, with `iters` and with
    2 x `iters` calls -- the difference is what the calls themselves launch (set-up and matching excluded)."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"skipped": "rocprofv3 not found"}
    out = {"shape": dims, "iters": iters}
    for route in ROUTES:
        counts = []
        for n in (iters, 2 * iters):
            tmp = tempfile.mkdtemp(prefix="crit_prof_")
            try:
                cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--count-route",
                       route, "--iters", str(n)] + [a for k, v in dims.items() for a in ("--" + k, str(v))]
                p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise RuntimeError("rocprofv3 run failed:\n%s" % p.stderr[-2000:])
                files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
                if not files:
                    raise RuntimeError("rocprofv3 wrote no kernel_trace.csv under %s" % tmp)
                with open(files[0]) as f:
                    counts.append(sum(1 for _ in csv.DictReader(f)))
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        out[route] = {"dispatches_at_iters": counts[0], "dispatches_at_2_iters": counts[1], "launches_per_call": round((counts[1] - counts[0]) / iters, 2)}
    return out


def _child(cmd, cwd, env, timeout=900):
    p = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError("%s (in %s) failed:\n%s" % (" ".join(cmd), cwd, p.stderr[-2000:]))
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _spread(runs, key):
    vals = [r[key] for r in runs]
    return {"median": round(statistics.median(vals), 3), "min": min(vals), "max": max(vals)}


SWITCHES = ("TF_CRITERION_FUSED", "TF_MATCHER_FUSED_COST")


def bench_step(parent, rounds, steps, warmup):
    """tools/bench_train.py: the parent commit, this tree with both switches off, this tree with both on; alternating child processes."""
    legs = [("parent", parent, False), ("off", REPO, False), ("on", REPO, True)]
    runs = {name: [] for name, root, _ in legs if root}
    for _ in range(rounds):
        for name, root, on in legs:
            if not root:
                continue
            env = dict(os.environ)
            for k in SWITCHES:
                env.pop(k, None)
                if on:
                    env[k] = "1"
            r = _child([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)], root, env)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "runs": runs}
    for name in runs:
        out[name + "_ms_per_step"] = _spread(runs[name], "ms_per_step")
    base = "parent" if "parent" in runs else "off"
    out["on_over_" + base] = round(out["on_ms_per_step"]["median"] / out[base + "_ms_per_step"]["median"], 3)
    lo = max(out[n + "_ms_per_step"]["min"] for n in runs)
    hi = min(out[n + "_ms_per_step"]["max"] for n in runs)
    out["spreads_overlap"] = bool(lo <= hi)
    return out


def bench_headline(parent, steps, warmup):
    """ONE pair of bench.py runs, the parent commit against this tree."""
    out = {"steps": steps, "warmup": warmup}
    for name, root in (("parent", parent), ("this", REPO)):
        r = _child([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], root,
                   dict(os.environ), timeout=1200)
        out[name] = {"ms_per_step": r.get("ms_per_step"), "value": r.get("value")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "criterion_fused_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (step level and headline against it)")
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--count-route", default=None, choices=ROUTES, help="(the profiler's child) run one route --iters times and exit")
    ap.add_argument("--iters", type=int, default=10)
    for k in ("L", "B", "Q", "C", "T"):
        ap.add_argument("--" + k, type=int, default=0)
    args = ap.parse_args()
    if args.parent:
        args.parent = os.path.abspath(args.parent)
    if not torch.cuda.is_available():
        sys.exit("tools/bench_criterion.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    if args.count_route:
        count_route(device, args.count_route, {k: getattr(args, k) for k in ("L", "B", "Q", "C", "T")}, args.iters)
        return
    report = {}
    if os.path.exists(args.out):          # the stages may be run one call at a time: keep what an earlier call measured
        with open(args.out) as f:
            report = json.load(f)
    report.update({"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
                   "what": "criterion: forward + backward of the class / box / cardinality losses of all decoder layers per call; cost: the "
                           "matching cost matrix per call; microseconds, `reps` calls between device events (_us) and host clocks (_host_us); "
                           "torch = today's chain on the same tensors in the same process, alternating rounds"})

    def save():   # after every stage: a later stage that fails leaves the earlier figures
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

    if not args.skip_ops:
        step = capture_step(device)
        wide = synthetic(device, step.criterion, 6, 2, 300, 91, max(step.T // 2, 1), "91 classes, 300 queries")
        report["step_shape"] = step.dims()
        report["criterion"] = [bench_pair(device, p, "criterion_own", "criterion_torch", args.rounds, args.reps) for p in (step, wide)]
        report["cost"] = [bench_pair(device, p, "cost_own", "cost_torch", args.rounds, args.reps) for p in (step, wide)]
        for s in report["criterion"] + report["cost"]:
            print(json.dumps(s), flush=True)
        save()
        del step, wide
        torch.cuda.empty_cache()
    if not args.skip_launches:
        if "step_shape" not in report:
            sys.exit("--skip-ops needs a report with the step's shape (run the operator stage first)")
        report["launches"] = bench_launches(report["step_shape"], args.iters)
        print(json.dumps(report["launches"]), flush=True)
        save()
    if not args.skip_step:
        report["cfg3_train_step"] = bench_step(args.parent, args.step_rounds, args.steps, args.warmup)
        print(json.dumps(report["cfg3_train_step"]), flush=True)
        save()
    if args.parent and not args.skip_headline:
        report["headline_against_parent"] = bench_headline(args.parent, 120, 8)
        print(json.dumps(report["headline_against_parent"]), flush=True)
        save()


if __name__ == "__main__":
    main()
