#!/usr/bin/env python
"""The backward of the six stride-2 convolutions of ResNet-50's layer2 - layer4: the library's own kernels
(fused.set_strided_conv_training) against torch's, and the cfg-3 training step with both convolution training switches off and on
(and, with --parent, on a checkout of the parent commit).  The sibling of tools/bench_conv_backward.py, whose method it shares.

    python tools/bench_conv_strided_backward.py [--out profiles/conv_strided_backward_bench.json] [--skip-step] [--parent DIR]

Per strided layer at two images of 800 x 1333 -- the 3 x 3 conv2 of each stage's first block (128 / 256 / 512 planes, input at
200 x 334, 100 x 167 and 50 x 84 pixels) and the 1 x 1 projection of its identity branch (2 planes -> 4 planes of the next stage) --
in ONE process on the same channels_last tensors, in alternating rounds:
  * own     the backward of fused.conv_train with the switch on: tf_linear_grad_stats_f32 x 2, tf_conv_dgrad_stride2_packed_f32 (one
            launch per parity class + the assembling pass) and the weight gradient (tf_conv3x3_wgrad_split_f32 /
            tf_conv1x1_strided_wgrad_split_f32 and its second pass);
  * torch   torch.autograd's backward of F.conv2d on the same tensors.
The figure reported is the median over the rounds with the smallest and the largest next to it.  There is no threshold."""
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

# (name, kernel, cin, cout, input H, input W)
SHAPES = [("layer2.0.conv2", 3, 128, 128, 200, 334), ("layer3.0.conv2", 3, 256, 256, 100, 167), ("layer4.0.conv2", 3, 512, 512, 50, 84),
          ("layer2.0.downsample", 1, 256, 512, 200, 334), ("layer3.0.downsample", 1, 512, 1024, 100, 167),
          ("layer4.0.downsample", 1, 1024, 2048, 50, 84)]


def _backward_callable(kind, x, w4, dy):
    from trackformer_amd import fused
    cout, cin, ks, _ = w4.shape
    xr = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    wr = w4.detach().clone().requires_grad_(True)
    if kind == "torch":
        y = F.conv2d(xr, wr.contiguous(memory_format=torch.channels_last), None, 2, ks // 2)
    else:
        y = fused.conv_train(xr, wr.permute(0, 2, 3, 1).reshape(cout, ks * ks * cin), 2)
        assert y is not None
    return lambda: torch.autograd.grad(y, (xr, wr), dy, retain_graph=True)


def bench_shape(device, name, ks, cin, cout, h, w, nimg, rounds, reps):
    from trackformer_amd import fused
    g = torch.Generator().manual_seed(cin + cout + ks)
    x = torch.randn(nimg, cin, h, w, generator=g).to(device).contiguous(memory_format=torch.channels_last)
    w4 = (torch.randn(cout, cin, ks, ks, generator=g) / (ks * ks * cin) ** 0.5).to(device)
    dy = (torch.randn(nimg, cout, (h - 1) // 2 + 1, (w - 1) // 2 + 1, generator=g) * 1e-3).to(device).contiguous(memory_format=torch.channels_last)
    kinds = ("own", "torch")
    calls = {k: _backward_callable(k, x, w4, dy) for k in kinds}
    fused.conv_train_counts(reset=True)
    results = {k: calls[k]() for k in kinds}
    for k in kinds:
        for _ in range(3):
            calls[k]()
    cc = fused.conv_train_counts()
    assert cc["dgrad_torch"] == 0 and cc["wgrad_torch"] == 0 and cc["dgrad_own"] == 4, cc
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
    out = {"layer": name, "kernel": ks, "cin": cin, "cout": cout, "nimg": nimg, "H": h, "W": w, "rounds": rounds, "reps": reps,
           "max_abs_diff_to_torch_over_max_abs": dict(zip(("dx", "dw"), diff))}
    for k in kinds:
        out[k + "_us"] = {"median": round(statistics.median(samples[k]), 1), "min": round(min(samples[k]), 1), "max": round(max(samples[k]), 1)}
    out["own_over_torch"] = round(out["own_us"]["median"] / out["torch_us"]["median"], 3)
    return out


def bench_step(rounds, steps, warmup, parent):
    """tools/bench_train.py in alternating child processes: [the parent commit's checkout,] this tree with both switches off, and on."""
    parent = os.path.abspath(parent) if parent else None
    settings = ([("parent", parent, None)] if parent else []) + [("off", REPO, None), ("on", REPO, "1")]
    runs = {name: [] for name, _, _ in settings}
    for _ in range(rounds):
        for name, root, flag in settings:
            env = dict(os.environ)
            for var in ("TF_SPLIT_CONV_TRAIN", "TF_STRIDED_CONV_TRAIN"):
                env.pop(var, None)
                if flag:
                    env[var] = flag
            p = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)],
                               env=env, cwd=root, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError("tools/bench_train.py (%s) failed:\n%s" % (name, p.stderr[-2000:]))
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
            print(name, runs[name][-1], flush=True)
    out = {"steps": steps, "warmup": warmup, "runs": runs}
    for name in runs:
        ms = [r["ms_per_step"] for r in runs[name]]
        out[name + "_ms_per_step"] = {"median": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_strided_backward_bench.json"))
    ap.add_argument("--nimg", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its step is timed next to this tree's")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_conv_strided_backward.py measures on a GPU; none is available")
    from trackformer_amd import fused
    device = torch.device("cuda:0")
    fused.set_strided_conv_training(True)
    report = {"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
              "what": "backward of one stride-2 convolution (stats + dgrad + wgrad [+ second pass]) per call, microseconds, device events "
                      "around `reps` calls; torch = autograd of F.conv2d on the same channels_last tensors in the same process",
              "shapes": []}
    for name, ks, cin, cout, h, w in SHAPES:
        report["shapes"].append(bench_shape(device, name, ks, cin, cout, h, w, args.nimg, args.rounds, args.reps))
        print(json.dumps(report["shapes"][-1]), flush=True)
    if not args.skip_step:
        torch.cuda.empty_cache()
        report["cfg3_train_step"] = bench_step(args.step_rounds, args.steps, args.warmup, args.parent)
        print(json.dumps(report["cfg3_train_step"]), flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
