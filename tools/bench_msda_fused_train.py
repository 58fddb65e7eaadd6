#!/usr/bin/env python
"""Training through the fused MSDeformAttn entry against today's module chain, and the cfg-3 training step with the switch off and on.

    python tools/bench_msda_fused_train.py [--out profiles/msda_fused_train_bench.json] [--skip-step] [--skip-kernels]

Per shape (the cfg-2 encoder at N = 2: S = Lq = 22 223, M 8, D 32, L 4, P 4; the decoder: Lq = 400) it times forward + backward, in
ONE process on the same tensors, in alternating rounds:
  * fused   msda.ms_deform_attn_fused on the raw projection qproj [N, Lq, 3 M L P]: the fused forward, then in the backward
            tf_msda_fused_prologue_f32, the operator's backward, tf_msda_fused_backward_epilogue_f32;
  * chain   today's training graph from the outputs of the two linears on: view / softmax / division / add over
            [N, Lq, M, L, P, 2] and MSDeformAttnFunction, and autograd's walk back through them.
The linears themselves are left out on both sides (one 256 -> 384 GEMM against 256 -> 256 + 256 -> 128: tools/bench_linear_backward.py
measures those).  Each sample is `reps` forward + backward calls between two device events; the figure reported is the median over
the rounds with the smallest and the largest next to it, after a warm-up of every path.
The two new kernels' own times come from a run of their own under `rocprofv3 --kernel-trace --stats` (a child process that only
calls the two entries), reported with the bytes the shapes imply over the time as a share of 8 TB/s.
Then tools/bench_train.py (the cfg-3 step) runs as a child process with TF_MSDA_FUSED_TRAIN unset and set to 1, alternating.  There is
no threshold: everything is reported as measured.  Without a GPU the tool fails; it measures nothing on a CPU."""
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

CFG2_SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]
S_CFG2 = sum(h * w for h, w in CFG2_SHAPES)
SHAPES = [("cfg2_encoder_n2", dict(N=2, M=8, D=32, Lq=S_CFG2, P=4, encoder=True)),
          ("cfg2_decoder_n2", dict(N=2, M=8, D=32, Lq=400, P=4, encoder=False))]
PEAK_BYTES_PER_S = 8.0e12
KERNELS = ("msda_fused_prologue_kernel", "msda_fused_bwd_epilogue_kernel")


def make(device, N, M, D, Lq, P, encoder):
    from trackformer_amd import msda
    g = torch.Generator().manual_seed(Lq)
    L = len(CFG2_SHAPES)
    value = torch.randn(N, S_CFG2, M, D, generator=g).to(device)
    qproj = torch.randn(N, Lq, 3 * M * L * P, generator=g)
    qproj[..., :2 * M * L * P] *= 2.0
    if encoder:   # one query per pyramid pixel, at its centre
        pts = torch.cat([torch.stack(torch.meshgrid((torch.arange(w) + 0.5) / w, (torch.arange(h) + 0.5) / h, indexing="xy"), -1)
                         .reshape(-1, 2) for h, w in CFG2_SHAPES])
        refp = pts.view(1, -1, 1, 2).expand(N, -1, L, 2).contiguous()
    else:
        refp = torch.rand(N, Lq, L, 2, generator=g) * 0.8 + 0.1
    grad_out = torch.randn(N, Lq, M * D, generator=g).to(device)
    shapes = msda.attach_host_shapes(torch.tensor(CFG2_SHAPES, device=device), CFG2_SHAPES)
    return value, shapes, refp.to(device), qproj.to(device), grad_out


def chain(value, shapes, refp, qproj, M, L, P):
    from trackformer_amd import msda
    N, Lq = qproj.shape[:2]
    mlp = M * L * P
    off = qproj[..., :2 * mlp].view(N, Lq, M, L, P, 2)
    attn = F.softmax(qproj[..., 2 * mlp:].view(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    loc = refp[:, :, None, :, None, :] + off / shapes[None, None, None, :, None, :]
    return msda.MSDeformAttnFunction.apply(value, shapes, loc, attn, 64)


def bench_shape(device, name, kw, rounds, reps):
    from trackformer_amd import msda
    value, shapes, refp, qproj, grad_out = make(device, **kw)
    M, L, P = kw["M"], len(CFG2_SHAPES), kw["P"]
    leaves = [t.detach().clone().requires_grad_(True) for t in (value, qproj)]

    def fused_step():
        out = msda.ms_deform_attn_fused(leaves[0], shapes, refp, leaves[1], M, L, P)
        return torch.autograd.grad(out, leaves, grad_out)

    def chain_step():
        return torch.autograd.grad(chain(leaves[0], shapes, refp, leaves[1], M, L, P), leaves, grad_out)

    calls = {"fused": fused_step, "chain": chain_step}
    first = {k: calls[k]() for k in calls}
    for k in calls:
        for _ in range(3):
            calls[k]()
    diff = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(first["fused"], first["chain"])]
    samples = {k: [] for k in calls}
    for _ in range(rounds):
        for k in calls:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                calls[k]()
            stop.record()
            stop.synchronize()
            samples[k].append(start.elapsed_time(stop) * 1e3 / reps)
    out = dict(kw, name=name, rounds=rounds, reps=reps,
               max_abs_diff_to_chain_over_max_abs=dict(zip(("grad_value", "grad_qproj"), diff)))
    for k in calls:
        out[k + "_us"] = {"median": round(statistics.median(samples[k]), 1), "min": round(min(samples[k]), 1), "max": round(max(samples[k]), 1)}
    out["fused_over_chain"] = round(out["fused_us"]["median"] / out["chain_us"]["median"], 3)
    return out


def kernels_only(device, reps):
    """The child under the profiler: the two entries alone, `reps` times per shape (backward's gradients stand in as random tensors)."""
    import ctypes
    from trackformer_amd import _cabi, msda
    lib = _cabi.lib()
    for _, kw in SHAPES:
        value, shapes, refp, qproj, _ = make(device, **kw)
        N, Lq, M, L, P = kw["N"], kw["Lq"], kw["M"], len(CFG2_SHAPES), kw["P"]
        mlp = M * L * P
        loc = torch.empty(N, Lq, M, L, P, 2, device=device)
        attn = torch.empty(N, Lq, M, L, P, device=device)
        gl, ga = torch.randn_like(loc), torch.randn_like(attn)
        gq, gref = torch.empty_like(qproj), torch.empty_like(refp)
        shp = ctypes.cast(msda._shape_array(tuple(CFG2_SHAPES)), ctypes.c_void_p)
        stream = torch.cuda.current_stream().cuda_stream
        for _ in range(reps):
            _cabi.check(lib.tf_msda_fused_prologue_f32(refp.data_ptr(), 2, qproj.data_ptr(), 3 * mlp, 0, 2 * mlp, shp, loc.data_ptr(),
                                                       attn.data_ptr(), N, M, L, Lq, P, stream), "prologue")
            _cabi.check(lib.tf_msda_fused_backward_epilogue_f32(refp.data_ptr(), 2, qproj.data_ptr(), 3 * mlp, 0, 2 * mlp, shp,
                                                                attn.data_ptr(), gl.data_ptr(), ga.data_ptr(), gq.data_ptr(), 3 * mlp, 0,
                                                                2 * mlp, gref.data_ptr(), N, M, L, Lq, P, stream), "epilogue")
        torch.cuda.synchronize()


def kernel_bytes(kw):
    """Bytes the shapes imply (fp32; 2-d references): prologue reads qproj + ref, writes loc + attn; epilogue reads attn, grad_attn,
    grad_loc, the offsets of qproj (the range test) + ref, writes grad_qproj + grad_ref."""
    N, Lq, M, P = kw["N"], kw["Lq"], kw["M"], kw["P"]
    L = len(CFG2_SHAPES)
    mlp, rows = M * L * P, N * Lq
    ref = rows * L * 2 * 4
    return {KERNELS[0]: rows * mlp * 4 * (3 + 3) + ref, KERNELS[1]: rows * mlp * 4 * (1 + 1 + 2 + 2 + 3) + 2 * ref}


def bench_kernels(reps):
    """One shape per child process under `rocprofv3 --kernel-trace --stats`; the two kernels' average times from its statistics."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"status": "not measured: rocprofv3 is not installed"}
    out = {}
    for idx, (name, kw) in enumerate(SHAPES):
        tmp = tempfile.mkdtemp(prefix="msda_fused_train_prof_")
        try:
            cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                   "--kernels-only", str(idx), "--reps", str(reps)]
            p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                # a child that fails may have faulted the device: nothing more is started on it -- main() writes the report and exits
                out[name] = {"status": "not measured: the profiled run failed", "returncode": p.returncode, "stderr": p.stderr[-500:]}
                out["stopped"] = True
                break
            rows = []
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                with open(path, newline="") as f:
                    rows += list(csv.DictReader(f))
            res = {}
            nbytes = kernel_bytes(kw)
            for k in KERNELS:
                hit = [r for r in rows if k in r.get("Name", "")]
                if not hit:
                    res[k] = {"status": "not measured: the kernel is not in the profiler's statistics"}
                    continue
                avg_us = float(hit[0]["AverageNs"]) / 1e3
                res[k] = {"calls": int(hit[0]["Calls"]), "average_us": round(avg_us, 2), "min_us": round(float(hit[0]["MinNs"]) / 1e3, 2),
                          "max_us": round(float(hit[0]["MaxNs"]) / 1e3, 2), "bytes_from_shapes": nbytes[k],
                          "share_of_8_TB_per_s": round(nbytes[k] / (avg_us * 1e-6) / PEAK_BYTES_PER_S, 3)}
            out[name] = res
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return out


def bench_step(rounds, steps, warmup):
    """tools/bench_train.py with the switch off and on, alternating; every run is a fresh child process."""
    runs = {"off": [], "on": []}
    for _ in range(rounds):
        for name in ("off", "on"):
            env = dict(os.environ)
            env.pop("TF_MSDA_FUSED_TRAIN", None)
            if name == "on":
                env["TF_MSDA_FUSED_TRAIN"] = "1"
            p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_train.py"), "--steps", str(steps), "--warmup", str(warmup)],
                               env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise RuntimeError("tools/bench_train.py (%s) failed:\n%s" % (name, p.stderr[-2000:]))
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            r = json.loads(line)
            runs[name].append({"ms_per_step": r["ms_per_step"], "images_per_s": r["value"], "last_loss": r["last_loss"]})
    out = {"steps": steps, "warmup": warmup, "runs": runs}
    for name in runs:
        ms = [r["ms_per_step"] for r in runs[name]]
        out[name + "_ms_per_step_median"] = round(statistics.median(ms), 2)
        out[name + "_ms_per_step_spread"] = round(max(ms) - min(ms), 2)   # between the runs of ONE setting
    out["on_minus_off_ms_per_step"] = round(out["on_ms_per_step_median"] - out["off_ms_per_step_median"], 2)
    out["on_over_off"] = round(out["on_ms_per_step_median"] / out["off_ms_per_step_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "msda_fused_train_bench.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels-only", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_msda_fused_train.py measures on a GPU; none is available")
    device = torch.device("cuda:0")
    if args.kernels_only is not None:
        global SHAPES
        SHAPES = [SHAPES[args.kernels_only]]
        kernels_only(device, args.reps)
        return
    report = {"device": torch.cuda.get_device_name(device), "torch": torch.__version__,
              "what": "forward + backward of the operator from the raw projection on, microseconds per call, device events around "
                      "`reps` calls, alternating rounds in one process; chain = view / softmax / division / add / MSDeformAttnFunction",
              "shapes": [bench_shape(device, name, kw, args.rounds, args.reps) for name, kw in SHAPES]}
    for s in report["shapes"]:
        print(json.dumps(s), flush=True)
    torch.cuda.empty_cache()
    report["kernels"] = {"status": "not measured: --skip-kernels"} if args.skip_kernels else bench_kernels(args.reps)
    print(json.dumps(report["kernels"]), flush=True)
    stopped = bool(report["kernels"].get("stopped"))
    if stopped:
        report["cfg3_train_step"] = {"status": "not measured: the tool stopped after the profiled run failed"}
    elif args.skip_step:
        report["cfg3_train_step"] = {"status": "not measured: --skip-step"}
    else:
        report["cfg3_train_step"] = bench_step(args.step_rounds, args.steps, args.warmup)
    print(json.dumps(report["cfg3_train_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    if stopped:
        sys.exit("tools/bench_msda_fused_train.py: the profiled run failed; stopped (report written to %s)" % args.out)


if __name__ == "__main__":
    main()
