#!/usr/bin/env python
"""SHA-256 of the output bytes of every MSDeformAttn kernel on seeded inputs: two builds of the library compute the same
thing exactly when the two JSON files are equal.

    python tools/msda_output_digest.py --json new.json                  # GPU: tables of tests/test_msda_numerics_gpu.py
    TF_MSDA_LIB=/path/to/other/libtf_msda.so python tools/msda_output_digest.py --json other.json
    python tools/msda_output_digest.py --emu --json emu.json            # the emulated kernels: tests/test_emu_kernels.py

Every case is the tests' own (shape, options) for the kernel it names, in the profiles PROFILES; the dispatch is asserted by
name after each call.  Backward cases digest grad_sampling_loc and grad_attn_weight of the default kernels; grad_value is
taken from the deterministic backward only (the default grad_value sums with float atomics and is not reproducible from run
to run), next to that run's grad_sampling_loc and grad_attn_weight.  The table runs twice (--runs) and a case whose digest
differs between the two runs is written as "not compared" instead: the row-gather backward at a head dimension that is not a
power of two sums grad_sampling_loc / grad_attn_weight with LDS float atomics.  Two runs do not always show it: when two
libraries are compared, a case that either file marks is not compared.  The GPU table ends with the tests' SHAPE_CASES, among
them msda_bwd_rowgather<f32> at D = 1, whose gradients are reproducible.  The emulator runs one workgroup at a time, so
there all three gradients of the default kernels are digested.
"""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

PROFILES = ("unit", "wide")   # both are forward, backward and fused profiles; "wide" has samples outside the levels
# msda_bwd_rowgather with D / VEC not a power of two sums grad_loc / grad_attn across the waves of a pair with LDS float atomics
UNSTABLE = "not compared: differs from run to run of one library"


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def fused_kw(kw):
    kw = dict(kw)
    return kw, kw.pop("ref_dim", 2), kw.pop("encoder", False)


def gpu_digests():
    import torch
    from tests import test_msda_numerics_gpu as T
    from tests import util_msda_numerics as U
    from trackformer_amd import fused, msda
    fused.set_split_linear(False)
    dev = torch.device("cuda:0")
    out = {}

    def np_(t):
        return t.detach().cpu().contiguous().numpy()

    def forward(key, kernel, opts, kw, double=False):
        for profile in PROFILES:
            case = U.make_case(profile, seed=len(key) + len(profile), **kw)
            if double:
                case = [t.double() if t.is_floating_point() else t for t in case]
            with T.options(opts):
                d = [case[0].to(dev), T._shapes_on(dev, case[1]), case[2].to(dev), case[3].to(dev)]
                y = msda.ms_deform_attn_forward(*d, 64)
                assert msda.last_kernel() == kernel, (key, msda.last_kernel())
            out["fwd/%s/%s" % (key, profile)] = sha(np_(y))

    def backward(key, kernel, opts, kw, double=False):
        for profile in PROFILES:
            case = U.make_case(profile, seed=len(key) + len(profile), **kw)
            if double:
                case = [t.double() if t.is_floating_point() else t for t in case]
            with T.options(opts):
                d = [case[0].to(dev), T._shapes_on(dev, case[1])] + [t.to(dev) for t in case[2:]]
                _, gl, ga = msda.ms_deform_attn_backward(*d, 64)
                assert msda.last_kernel() == kernel, (key, msda.last_kernel())
                det = msda.ms_deform_attn_backward(*d, 64, deterministic=True)
            out["bwd/%s/%s/grad_loc" % (key, profile)] = sha(np_(gl))
            out["bwd/%s/%s/grad_attn" % (key, profile)] = sha(np_(ga))
            for name, g in zip(("grad_value", "grad_loc", "grad_attn"), det):
                out["bwd/%s/%s/%s_det" % (key, profile, name)] = sha(np_(g))

    for cid, kernel, opts, kw in T.FWD:
        forward(cid, kernel, opts, kw)
    forward(*T.FWD_F64, double=True)
    for cid, kernel, opts, kw in T.FUSED:
        kw, ref_dim, enc = fused_kw(kw)
        M, L, P = kw["M"], len(kw["shapes"]), kw["P"]
        for profile in PROFILES:
            value, shapes, refp, qproj = U.make_fused_case(profile, seed=len(cid) + len(profile), ref_dim=ref_dim, encoder=enc, **kw)
            with T.options(opts):
                y = msda.ms_deform_attn_forward_fused(value.to(dev), T._shapes_on(dev, shapes), refp.to(dev), qproj.to(dev), M, L, P)
                assert msda.last_kernel() == kernel, (cid, msda.last_kernel())
            out["fused/%s/%s" % (cid, profile)] = sha(np_(y))
    for cid, kernel, opts, kw in T.BWD:
        backward(cid, kernel, opts, kw)
    backward(*T.BWD_F64, double=True)
    # the shape edges: among them msda_bwd_rowgather<f32> at D = 1 and D = 1024, where a pair's lanes are a power of two and
    # grad_sampling_loc / grad_attn_weight are reproducible
    for cid, (fk, bk), kw, host in T.SHAPE_CASES:
        case = U.make_case("wide", seed=len(cid), **kw)
        d = [case[0].to(dev), T._shapes_on(dev, case[1], host)] + [t.to(dev) for t in case[2:]]
        y = msda.ms_deform_attn_forward(*d[:4], 64)
        assert msda.last_kernel() == fk, (cid, msda.last_kernel())
        _, gl, ga = msda.ms_deform_attn_backward(*d, 64)
        assert msda.last_kernel() == bk, (cid, msda.last_kernel())
        for name, t in (("out", y), ("grad_loc", gl), ("grad_attn", ga)):
            out["shape/%s/%s" % (cid, name)] = sha(np_(t))
    return out


def emu_digests():
    os.environ["HIPEMU_THREADS"] = "1"   # one workgroup at a time: the float atomics of the backward add in a fixed order
    from tests import emu_lib
    from tests import test_emu_kernels as T
    from tests import util_msda_numerics as U
    out = {}
    for cid, kernel, opts, kw in T.NU_FWD:
        for profile in PROFILES:
            v, s, l, a, _ = [t.numpy() for t in U.make_case(profile, seed=len(cid), **kw)]
            prev = emu_lib.set_options(**opts)
            try:
                y = emu_lib.msda_forward(v, s, l, a)
                assert emu_lib.last_kernel() == kernel, (cid, emu_lib.last_kernel())
            finally:
                emu_lib.set_options(**prev)
            out["fwd/%s/%s" % (cid, profile)] = sha(y)
    for cid, kernel, opts, kw in T.NU_FUSED:
        kw, ref_dim, enc = fused_kw(kw)
        M, L, P = kw["M"], len(kw["shapes"]), kw["P"]
        for profile in PROFILES:
            value, shapes, refp, qproj = U.make_fused_case(profile, seed=len(cid), ref_dim=ref_dim, encoder=enc, **kw)
            prev = emu_lib.set_options(**opts)
            try:
                y = emu_lib.msda_forward_fused(value.numpy(), shapes.numpy(), refp.numpy(), qproj.numpy(), M, L, P)
                assert emu_lib.last_kernel() == kernel, (cid, emu_lib.last_kernel())
            finally:
                emu_lib.set_options(**prev)
            out["fused/%s/%s" % (cid, profile)] = sha(y)
    for cid, kernel, kw in T.NU_BWD:
        for profile in PROFILES:
            got = emu_lib.msda_backward(*[t.numpy() for t in U.make_case(profile, seed=len(cid), **kw)])
            assert emu_lib.last_kernel() == kernel, (cid, emu_lib.last_kernel())
            for name, g in zip(("grad_value", "grad_loc", "grad_attn"), got):
                out["bwd/%s/%s/%s" % (cid, profile, name)] = sha(g)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--emu", action="store_true", help="run the emulated kernels on the CPU instead of the GPU library")
    ap.add_argument("--json", default=None, help="write the digests here (default: standard output)")
    ap.add_argument("--runs", type=int, default=None,
                    help="repeat the table this often (default: 2 on the GPU, 1 on the emulator); a case whose digest differs "
                         "between the runs is written as 'not compared' instead of a digest")
    args = ap.parse_args()
    run = emu_digests if args.emu else gpu_digests
    digests = run()
    for _ in range((args.runs or (1 if args.emu else 2)) - 1):
        again = run()
        digests = {k: v if again[k] == v else UNSTABLE for k, v in digests.items()}
    text = json.dumps({k: digests[k] for k in sorted(digests)}, indent=1)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
        print("%d digests -> %s" % (len(digests), args.json))
    else:
        print(text)


if __name__ == "__main__":
    main()
