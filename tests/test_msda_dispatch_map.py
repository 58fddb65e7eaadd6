"""The dispatch map of the MSDeformAttn C ABI: which kernel (tf_msda_last_kernel) every entry point reaches for a shape,
a dtype and a set of tf_msda_set_option knobs.  The expected names were recorded by running this table against the
emulated library built from the commit BEFORE the host-side dispatch code moved into csrc/msda_dispatch.h and are
literals: they pin the map across refactors of that code and are never derived from the library under test.

The table runs twice: on the emulated library (tests/emu_lib.py, host pointers; part of -m "not gpu") and, marked gpu,
on libtf_msda.so with device tensors.  Only the kernel's name and the status TF_MSDA_OK are checked (the numerics of
every kernel named here: tests/test_emu_kernels.py, tests/test_msda_numerics_gpu.py).

No case depends on the number of compute units (the emulator's differs from the card's): the persistent kernels' tile
plan does, the kernel chosen for a plan does not, and at this pyramid a tile always fits."""
import ctypes

import numpy as np
import pytest

from tests import emu_lib

PYR = [(6, 10), (3, 5), (2, 3), (1, 2)]   # the smallest pyramid at which every window kernel still plans a tile
S = sum(h * w for h, w in PYR)            # 83
N, M = 1, 2
TF_MSDA_OK = 0

EIGHT_WAVES = dict(pquad_waves=8, pquad_npass=1, pquad_wg_per_cu=2, pquad_lds_kb=78)

# (id, case, options, expected kernel).  case: entry = fwd | fused | bwd; dtype, D, P, Lq, ref_dim; dshapes: the
# device-shapes entry; loc_offset: bytes added to the loc pointer.
FORWARD = [
    ("defaults", dict(), dict(), "msda_fwd_f32_pquad2<%s,4w,2p>"),
    ("pquad_v2=0", dict(), dict(pquad_v2=0), "msda_fwd_f32_pquad<%s>"),
    ("pquad=0", dict(), dict(pquad=0), "msda_fwd_f32_quad<%s>"),
    ("tiled=0", dict(), dict(tiled=0), "msda_fwd_f32_direct<%s>"),
    ("pquad_prefetch=2", dict(), dict(pquad_prefetch=2), "msda_fwd_f32_quad<%s>"),
    ("pquad_npass=1", dict(), dict(pquad_npass=1), "msda_fwd_f32_pquad2<%s,4w,1p>"),
    ("pquad_cf=1", dict(), dict(pquad_cf=1), "msda_fwd_f32_pquad2<%s,4w,2p,cf>"),
    ("eight_waves", dict(), EIGHT_WAVES, "msda_fwd_f32_pquad2<%s,8w,1p>"),
    ("eight_waves_cf", dict(), dict(EIGHT_WAVES, pquad_cf=1), "msda_fwd_f32_pquad2<%s,8w,1p,cf>"),
    ("pquad_waves=8", dict(), dict(pquad_waves=8), "msda_fwd_f32_pquad2<%s,4w,2p>"),
    ("pquad_waves=8,pquad_v2=0", dict(), dict(pquad_waves=8, pquad_v2=0), "msda_fwd_f32_pquad<%s>"),
    ("pquad_npass=3", dict(), dict(pquad_npass=3), "msda_fwd_f32_pquad<%s>"),
    ("pquad_wide=0", dict(), dict(pquad_wide=0), "msda_fwd_f32_pquad<%s>"),
    ("quad_ta_mask=12", dict(), dict(pquad=0, quad_ta_mask=12), "msda_fwd_f32_quad<%s>"),
    ("quad_waves=8,quad_npass=1", dict(), dict(pquad=0, quad_waves=8, quad_npass=1), "msda_fwd_f32_quad<%s>"),
    ("quad_waves=8,quad_npass=3", dict(), dict(pquad=0, quad_waves=8), "msda_fwd_f32_direct<%s>"),
    ("D=36", dict(D=36), dict(), "msda_fwd_f32_pquad<%s,D=36>"),
    ("D=36,pquad_npass=1", dict(D=36), dict(pquad_npass=1), "msda_fwd_f32_direct9<%s>"),
    ("D=36,pquad=0", dict(D=36), dict(pquad=0), "msda_fwd_f32_direct9<%s>"),
    ("D=36,pquad=0,direct9=0", dict(D=36), dict(pquad=0, direct9=0), "msda_fwd_f32_buf<%s>"),
    ("Lq=S-1", dict(Lq=S - 1), dict(), "msda_fwd_f32_direct<%s>"),
    ("P=2", dict(P=2), dict(), "msda_fwd_f32_buf<%s>"),
]
CASES = []
for _id, _case, _opts, _want in FORWARD:
    for _entry, _tag in (("fwd", "plain"), ("fused", "fused")):
        CASES.append(("%s-%s" % (_entry, _id), dict(_case, entry=_entry), _opts, _want % _tag))
CASES += [
    ("fwd-D=30", dict(entry="fwd", D=30), dict(), "msda_fwd_rowgather<f32>"),
    ("fwd-f64", dict(entry="fwd", dtype="f64"), dict(), "msda_fwd_rowgather<f64>"),
    ("fwd-dshapes", dict(entry="fwd", dshapes=True), dict(), "msda_fwd_f32_direct<plain>"),
    ("fwd-dshapes-D=36", dict(entry="fwd", dshapes=True, D=36), dict(), "msda_fwd_f32_direct9<plain>"),
    ("fwd-loc+4", dict(entry="fwd", loc_offset=4), dict(), "msda_fwd_f32_buf<plain>"),
    ("fused-ref_dim=4", dict(entry="fused", ref_dim=4), dict(), "msda_fwd_f32_quad<fused>"),
    ("bwd-defaults", dict(entry="bwd"), dict(), "msda_bwd_f32_sorted2"),
    ("bwd-Lq=S-1", dict(entry="bwd", Lq=S - 1), dict(), "msda_bwd_f32_buf<rowatom>"),
    ("bwd-D=36", dict(entry="bwd", D=36), dict(), "msda_bwd_rowgather<f32>"),
    ("bwd-D=30", dict(entry="bwd", D=30), dict(), "msda_bwd_rowgather<f32>"),
    ("bwd-D=16", dict(entry="bwd", D=16), dict(), "msda_bwd_f32_buf"),
    ("bwd-f64", dict(entry="bwd", dtype="f64"), dict(), "msda_bwd_rowgather<f64>"),
    ("bwd-dshapes", dict(entry="bwd", dshapes=True), dict(), "msda_bwd_f32_buf<rowatom>"),
]
# D = 30: the plain entry gathers rows (above); the fused entry takes multiples of 4 only and answers with a status
FUSED_D30_STATUS = -2   # TF_MSDA_ERR_BAD_DIMS


def _inputs(case):
    """Host arrays of one case: every query samples around its own reference point (the centre of its pixel)."""
    D, P, Lq = case.get("D", 32), case.get("P", 4), case.get("Lq", S)
    ref_dim = case.get("ref_dim", 2)
    dt = np.float64 if case.get("dtype") == "f64" else np.float32
    L = len(PYR)
    rng = np.random.default_rng(5)
    centres = np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                              for h, w in PYR])[:Lq]
    a = dict(value=rng.standard_normal((N, S, M, D)).astype(dt), shapes=np.array(PYR, np.int64))
    if case["entry"] == "fused":
        ref = np.full((N, Lq, L, ref_dim), 0.5, np.float32)
        ref[..., :2] = centres[None, :, None, :]
        a.update(ref=ref, qproj=(0.5 * rng.standard_normal((N * Lq, 3 * M * L * P))).astype(np.float32))
    else:
        loc = centres[None, :, None, None, None, :] + 0.02 * rng.standard_normal((N, Lq, M, L, P, 2))
        a.update(loc=loc.astype(dt), attn=np.full((N, Lq, M, L, P), 1.0 / (L * P), dt))
    if case["entry"] == "bwd":
        a.update(grad_out=rng.standard_normal((N, Lq, M * D)).astype(dt))
    return a, dt, (D, L, Lq, P, ref_dim)


class _Host:
    """Buffers of the emulated library: 64-byte aligned host memory."""
    def __init__(self):
        self.lib = emu_lib.lib()
        self.keep = []

    def put(self, a, offset=0):
        buf = np.zeros(a.nbytes + 128, np.uint8)
        self.keep.append(buf)
        p = buf.ctypes.data + (-buf.ctypes.data) % 64 + offset
        ctypes.memmove(p, np.ascontiguousarray(a).ctypes.data, a.nbytes)
        return p

    def sync(self):
        pass


class _Device:
    """Buffers of libtf_msda.so: device tensors (the caching allocator aligns them to 512 bytes)."""
    def __init__(self):
        import torch
        from trackformer_amd import _cabi
        if not torch.cuda.is_available():
            pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
        self.torch, self.lib = torch, _cabi.lib()
        self.keep = []

    def put(self, a, offset=0):
        t = self.torch.zeros(a.nbytes + 128, dtype=self.torch.uint8, device="cuda")
        t[offset:offset + a.nbytes] = self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        self.keep.append(t)
        return t.data_ptr() + offset

    def sync(self):
        self.torch.cuda.synchronize()


def _dispatch(be, case):
    """Runs one case on a backend; returns (status, kernel name)."""
    a, dt, (D, L, Lq, P, ref_dim) = _inputs(case)
    suf = "f64" if dt == np.float64 else "f32"
    tail = "_dshapes" if case.get("dshapes") else ""
    lib = be.lib
    value = be.put(a["value"])
    # host shapes stay on the host; the device-shapes entry reads them from the backend's memory
    shapes = be.put(a["shapes"]) if case.get("dshapes") else a["shapes"].ctypes.data
    if case["entry"] == "fused":
        out = be.put(np.zeros((N, Lq, M * D), np.float32))
        rc = lib.tf_msda_forward_fused_f32(value, shapes, be.put(a["ref"]), ref_dim, be.put(a["qproj"]), 3 * M * L * P, 0,
                                           2 * M * L * P, out, N, S, M, D, L, Lq, P, None)
    else:
        loc, attn = be.put(a["loc"], case.get("loc_offset", 0)), be.put(a["attn"])
        if case["entry"] == "fwd":
            out = be.put(np.zeros((N, Lq, M * D), dt))
            rc = getattr(lib, "tf_msda_forward_%s%s" % (suf, tail))(value, shapes, loc, attn, out, N, S, M, D, L, Lq, P, None)
        else:
            gv, gl, ga = be.put(np.zeros_like(a["value"])), be.put(np.zeros_like(a["loc"])), be.put(np.zeros_like(a["attn"]))
            rc = getattr(lib, "tf_msda_backward_%s%s" % (suf, tail))(value, shapes, loc, attn, be.put(a["grad_out"]), gv, gl, ga,
                                                                    N, S, M, D, L, Lq, P, None)
    be.sync()
    return rc, lib.tf_msda_last_kernel().decode()


def _check(be, case, opts, want):
    prev = {k: be.lib.tf_msda_set_option(k.encode(), int(v)) for k, v in opts.items()}
    try:
        rc, got = _dispatch(be, case)
    finally:
        for k, v in prev.items():
            be.lib.tf_msda_set_option(k.encode(), v)
    print("%s %s -> status %d, %s" % (case, opts, rc, got))
    assert rc == TF_MSDA_OK
    assert got == want


_IDS = [c[0] for c in CASES]


@pytest.mark.skipif(not emu_lib.available(), reason="needs a host clang++ (ROCm's llvm) to build the emulated library")
@pytest.mark.parametrize("name,case,opts,want", CASES, ids=_IDS)
def test_dispatch_map_emulated(name, case, opts, want):
    _check(_Host(), case, opts, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case,opts,want", CASES, ids=_IDS)
def test_dispatch_map_gpu(name, case, opts, want):
    _check(_Device(), case, opts, want)


@pytest.mark.skipif(not emu_lib.available(), reason="needs a host clang++ (ROCm's llvm) to build the emulated library")
def test_fused_entry_refuses_head_dim_30_emulated():
    assert _dispatch(_Host(), dict(entry="fused", D=30))[0] == FUSED_D30_STATUS


@pytest.mark.gpu
def test_fused_entry_refuses_head_dim_30_gpu():
    assert _dispatch(_Device(), dict(entry="fused", D=30))[0] == FUSED_D30_STATUS
