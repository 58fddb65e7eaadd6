"""CPU: the deterministic MSDeformAttn backward (tf_msda_backward_det_*, trackformer_amd/csrc/msda_bwd_det.h).

  * the real library without a launch: workspace size, status codes and their order;
  * msda.deterministic_backward_enabled(): argument > setter > TF_MSDA_DETERMINISTIC > torch's flag;
  * the kernels' own source under the SIMT emulator (tests/emu/): every operand profile against the float64 yardstick of
    tests/util_msda_numerics.py, and bit equality of all three gradients across host-thread interleavings of the workgroups,
    poisoned workspace / outputs, host and device shapes, and N = 2 against its two N = 1 slices;
  * the gfx950 assembly of the new kernels holds no floating-point atomic -- repeated runs can only fail to find a
    difference, this shows there is none to find;
  * host tensors: the flag is accepted and changes nothing."""
import ctypes
import importlib.util
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import msda_oracle
from tests import emu_lib
from tests import util_msda_numerics as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PYR = [(25, 42), (13, 21), (7, 11), (4, 6)]
S_PYR = sum(h * w for h, w in PYR)
SMALL8 = [(6, 9), (3, 5), (2, 2), (1, 1)] * 2

needs_emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ to build the emulated library with")

CASES = [   # id, dtype, dict(N, M, D, Lq, P, shapes, encoder)
    ("d5_p3_one_pixel_level", np.float32, dict(N=2, M=3, D=5, Lq=33, P=3, shapes=[(7, 3), (1, 1), (2, 9)])),
    ("d16", np.float32, dict(N=2, M=4, D=16, Lq=90, P=2, shapes=[(12, 20), (6, 10), (3, 5), (2, 3)])),
    ("d32_p4_encoder", np.float32, dict(N=2, M=2, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("d36_l8", np.float32, dict(N=2, M=2, D=36, Lq=60, P=4, shapes=SMALL8)),
    ("f64", np.float64, dict(N=2, M=3, D=8, Lq=40, P=4, shapes=[(7, 3), (1, 1), (2, 9)])),
]


@pytest.fixture(scope="module")
def emu():
    return emu_lib.lib()


def _filled(shape, dtype, fill):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = fill
    return a


def det_backward(L, case, dshapes=False, fill=0x00, threads=8, slack=0):
    """tf_msda_backward_det_* of the emulated library on numpy operands; outputs and workspace start as `fill` bytes."""
    value, shapes, loc, attn, grad_out = case
    dt = value.dtype
    suf = "f32" if dt == np.float32 else "f64"
    N, S, M, D = value.shape
    _, Lq, _, Ln, P, _ = loc.shape
    nbytes = L.tf_msda_backward_det_workspace_bytes(dt.itemsize, N, S, M, D, Ln, Lq, P)
    assert nbytes > 0
    ws = _filled((nbytes + 7) // 8, np.uint64, fill)
    gv, gl, ga = _filled(value.shape, dt, fill), _filled(loc.shape, dt, fill), _filled(attn.shape, dt, fill)
    before = os.environ.get("HIPEMU_THREADS")
    os.environ["HIPEMU_THREADS"] = str(threads)          # read at every launch
    try:
        fn = getattr(L, "tf_msda_backward_det_%s%s" % (suf, "_dshapes" if dshapes else ""))
        rc = fn(value.ctypes.data, shapes.ctypes.data, loc.ctypes.data, attn.ctypes.data, grad_out.ctypes.data, gv.ctypes.data,
                gl.ctypes.data, ga.ctypes.data, ws.ctypes.data, nbytes + slack, N, S, M, D, Ln, Lq, P, None)
    finally:
        if before is None:
            os.environ.pop("HIPEMU_THREADS", None)
        else:
            os.environ["HIPEMU_THREADS"] = before
    return rc, (gv, gl, ga)


def _numpy_case(profile, dtype, kw, seed):
    case = U.make_case(profile, seed=seed, **kw)
    return tuple(np.ascontiguousarray(t.numpy().astype(dtype) if t.is_floating_point() else t.numpy()) for t in case)


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the real library: validation only, nothing is launched ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real():
    from trackformer_amd import _cabi, build
    build.build_all()
    return _cabi.lib()


def test_workspace_bytes_rejects_bad_dimensions(real):
    good = dict(elem=4, N=2, S=10, M=2, D=8, L=2, Lq=5, P=4)
    assert real.tf_msda_backward_det_workspace_bytes(*good.values()) > 0
    for k in ("N", "S", "M", "D", "L", "Lq", "P"):
        for bad in (0, -3):
            args = dict(good, **{k: bad})
            assert real.tf_msda_backward_det_workspace_bytes(*args.values()) == -2, (k, bad)
    assert real.tf_msda_backward_det_workspace_bytes(*dict(good, L=17).values()) == -2
    assert real.tf_msda_backward_det_workspace_bytes(*dict(good, elem=2).values()) == -2
    # 4 Lq L P corner slots of one (batch, head) block must fit 32 bits
    assert real.tf_msda_backward_det_workspace_bytes(4, 1, 10, 1, 8, 16, 2 ** 27, 8) == -2
    # about 2 x 4 N Lq M L P x (8 + sizeof T) bytes, and fp64 needs more than fp32
    n32 = real.tf_msda_backward_det_workspace_bytes(4, 1, 1000, 8, 32, 4, 1000, 4)
    n64 = real.tf_msda_backward_det_workspace_bytes(8, 1, 1000, 8, 32, 4, 1000, 4)
    items = 4 * 1000 * 8 * 16
    assert items * 20 <= n32 <= items * 24 and n32 < n64 <= items * 28


def test_status_codes_before_any_gpu_work(real):
    """NULL -> -1, dimensions -> -2, workspace -> -6, shape sum -> -3, in that order: a call whose only fault is the shape sum shows
    that a workspace of exactly the reported size is accepted, without launching anything."""
    assert real.tf_msda_strerror(-6) not in (b"", b"unknown tf_msda status")
    shp = (ctypes.c_int64 * 2)(2, 2)
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    dims = (1, 5, 1, 4, 1, 1, 1)   # S = 5 != 2 * 2
    need = real.tf_msda_backward_det_workspace_bytes(4, *dims)
    assert need > 0
    for fn in (real.tf_msda_backward_det_f32, real.tf_msda_backward_det_f64):
        elem = 4 if fn is real.tf_msda_backward_det_f32 else 8
        need = real.tf_msda_backward_det_workspace_bytes(elem, *dims)
        assert fn(one, shp, one, one, one, one, one, one, one, need - 1, *dims, None) == -6
        assert fn(one, shp, one, one, one, one, one, one, one, need, *dims, None) == -3       # accepted; the shapes are wrong
        assert fn(one, shp, one, one, one, one, one, one, None, need, *dims, None) == -1
        assert fn(None, shp, one, one, one, one, one, one, one, need, *dims, None) == -1
        assert fn(one, None, one, one, one, one, one, one, one, need, *dims, None) == -1
        assert fn(one, shp, one, one, one, one, one, one, one, need, 1, 5, 1, 4, 1, 0, 1, None) == -2
        assert fn(one, shp, one, one, one, one, one, one, one, need, 1, 5, 1, 4, 17, 1, 1, None) == -2
        assert fn(one, shp, one, one, one, one, one, one, one, -1, *dims, None) == -6
    for fn in (real.tf_msda_backward_det_f32_dshapes, real.tf_msda_backward_det_f64_dshapes):
        assert fn(one, None, one, one, one, one, one, one, one, 1 << 30, *dims, None) == -1
        assert fn(one, one, one, one, one, one, one, one, one, 0, *dims, None) == -6
    from trackformer_amd import _cabi
    with pytest.raises(_cabi.MSDAError, match="workspace"):
        _cabi.check(-6, "unit test")


# ---- the resolver --------------------------------------------------------------------------------------------------------------------------
def test_resolver_precedence():
    from trackformer_amd import msda
    env = os.environ.pop("TF_MSDA_DETERMINISTIC", None)
    flag = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    prev = msda.set_deterministic_backward(None)
    try:
        torch.use_deterministic_algorithms(False)
        assert msda.deterministic_backward_enabled() is False
        torch.use_deterministic_algorithms(True)
        assert msda.deterministic_backward_enabled() is True                  # torch's flag alone
        os.environ["TF_MSDA_DETERMINISTIC"] = "0"
        assert msda.deterministic_backward_enabled() is False                 # the environment beats torch's flag
        torch.use_deterministic_algorithms(False)
        os.environ["TF_MSDA_DETERMINISTIC"] = "1"
        assert msda.deterministic_backward_enabled() is True
        assert msda.set_deterministic_backward(False) is None                 # returns the previous setting
        assert msda.deterministic_backward_enabled() is False                 # the setter beats the environment
        os.environ["TF_MSDA_DETERMINISTIC"] = "0"
        assert msda.set_deterministic_backward(True) is False
        assert msda.deterministic_backward_enabled() is True
        assert msda.deterministic_backward_enabled(False) is False            # the argument beats everything
        assert msda.set_deterministic_backward(False) is True
        assert msda.deterministic_backward_enabled(True) is True
        assert msda.set_deterministic_backward(None) is False
        assert msda.deterministic_backward_enabled() is False                 # back to the environment ("0")
    finally:
        msda.set_deterministic_backward(prev)
        torch.use_deterministic_algorithms(flag, warn_only=warn)
        if env is None:
            os.environ.pop("TF_MSDA_DETERMINISTIC", None)
        else:
            os.environ["TF_MSDA_DETERMINISTIC"] = env


# ---- the kernels under the emulator -------------------------------------------------------------------------------------------------------
@needs_emu
@pytest.mark.parametrize("profile", U.PROFILES)
@pytest.mark.parametrize("cid,dtype,kw", CASES, ids=[c[0] for c in CASES])
def test_yardstick_and_bit_equality(emu, cid, dtype, kw, profile):
    seed = len(cid) + len(profile)
    case = _numpy_case(profile, dtype, kw, seed)
    rc, got = det_backward(emu, case, threads=8, fill=0x00)
    assert rc == 0
    assert emu_lib.last_kernel() == ("msda_bwd_det<f32>" if dtype == np.float32 else "msda_bwd_det<f64>")
    tc = [torch.from_numpy(a) for a in case]
    rv, rl, ra, left = U.backward_reference(*tc)
    assert left < U.EXCLUDE_MAX, left
    oracle = msda_oracle.msda_backward(*case) if dtype == np.float32 else (None, None, None)
    for name, y, want, o in zip(("grad_value", "grad_loc", "grad_attn"), got, (rv, rl, ra), oracle):
        print(cid, profile, name, U.check(y, want, fp32=o, what=(cid, profile, name)))
    # rows nobody samples hold +0, not -0 and not what the buffer held
    untouched = (rv.n == 0).numpy()
    assert not got[0][untouched].view(np.uint8).any()
    # workgroups in another interleaving; poisoned workspace and outputs; device shapes
    for what, kwargs in (("1 host thread", dict(threads=1)), ("0xFF fill", dict(fill=0xFF)), ("device shapes", dict(dshapes=True, fill=0xFF))):
        rc, other = det_backward(emu, case, **kwargs)
        assert rc == 0 and _same_bits(got, other), what
    # batch invariance: N = 2 against its two N = 1 slices
    for n in range(case[0].shape[0]):
        one = tuple(np.ascontiguousarray(a[n:n + 1]) if i != 1 else a for i, a in enumerate(case))
        rc, part = det_backward(emu, one, fill=0xFF)
        assert rc == 0 and _same_bits([g[n:n + 1] for g in got], part), n


@needs_emu
def test_workspace_of_exactly_the_reported_size(emu):
    case = _numpy_case("unit", np.float32, CASES[0][2], 1)
    rc, got = det_backward(emu, case)
    assert rc == 0
    rc, _ = det_backward(emu, case, slack=-1)
    assert rc == -6


@needs_emu
@pytest.mark.parametrize("D", [5, 32, 36])
def test_exact_edges(emu, D):
    case = U.exact_edge_case(1, 4, D, 4, [(4, 8), (2, 2), (1, 1), (1, 4)], seed=D)
    npc = tuple(np.ascontiguousarray(t.numpy()) for t in case)
    rc, got = det_backward(emu, npc, fill=0xFF)
    assert rc == 0
    rv, rl, ra, left = U.backward_reference(*case, exact=True)
    assert left == 0.0
    oracle = msda_oracle.msda_backward(*npc)
    for name, y, want, o in zip(("grad_value", "grad_loc", "grad_attn"), got, (rv, rl, ra), oracle):
        U.check(y, want, fp32=o, what=name)


@needs_emu
def test_hot_row_longer_than_many_chunks(emu):
    """Every sample of a level on one pixel: one row's list is thousands of items long (many chunks, many rounds of the reduce
    workgroup), and the result still meets the yardstick and does not depend on the interleaving."""
    value, shapes, loc, attn, grad_out = U.make_case("unit", 1, 2, 32, 700, 4, [(6, 8), (3, 4)], seed=5)
    loc[:, :, :, 0] = torch.tensor([(3 + 0.5 + 0.3) / 8, (2 + 0.5 + 0.2) / 6])
    case = (value, shapes, loc.contiguous(), attn, grad_out)
    npc = tuple(np.ascontiguousarray(t.numpy()) for t in case)
    rc, got = det_backward(emu, npc, threads=8)
    assert rc == 0
    rv, rl, ra, _ = U.backward_reference(*case)
    assert int(rv.n.max()) >= 700 * 4
    oracle = msda_oracle.msda_backward(*npc)
    for y, want, o in zip(got, (rv, rl, ra), oracle):
        U.check(y, want, fp32=o)
    rc, other = det_backward(emu, npc, threads=1, fill=0xFF)
    assert rc == 0 and _same_bits(got, other)
    untouched = (rv.n == 0).numpy()                       # the other pixels of that level: +0 by a plain store, in both runs
    assert untouched.sum() >= 40 * 2 * 32 and not other[0][untouched].view(np.uint8).any()


@needs_emu
def test_python_glue_on_the_emulator(emu):
    """msda.ms_deform_attn_backward(deterministic=...) and MSDeformAttnFunction.backward on the device path (the emulated library
    in place of libtf_msda.so): workspace from torch.empty, host and device shapes, the resolver read at backward time."""
    from tests.util_emu_gpu_path import gpu_path_on_emulator
    from trackformer_amd import msda
    case = U.make_case("unit", 2, 3, 8, 20, 2, [(5, 4), (2, 3)], seed=9)
    _, want = det_backward(emu, tuple(np.ascontiguousarray(t.numpy()) for t in case))
    with gpu_path_on_emulator() as lib:
        for host in (True, False):
            shp = case[1].clone()
            if host:
                msda.attach_host_shapes(shp, case[1].tolist())
            got = msda.ms_deform_attn_backward(case[0], shp, case[2], case[3], case[4], 64, deterministic=True)
            assert msda.last_kernel() == "msda_bwd_det<f32>"
            assert _same_bits([g.numpy() for g in got], want), host
        assert lib.calls["tf_msda_backward_det_f32"] == 1 and lib.calls["tf_msda_backward_det_f32_dshapes"] == 1
        msda.ms_deform_attn_backward(*case, 64)
        assert msda.last_kernel() != "msda_bwd_det<f32>"                      # off by default
        prev = msda.set_deterministic_backward(True)
        try:
            v, l, a = case[0].clone().requires_grad_(True), case[2].clone().requires_grad_(True), case[3].clone().requires_grad_(True)
            msda.MSDeformAttnFunction.apply(v, case[1], l, a, 64).backward(case[4])
            assert msda.last_kernel() == "msda_bwd_det<f32>"
            assert _same_bits([v.grad.numpy(), l.grad.numpy(), a.grad.numpy()], want)
        finally:
            msda.set_deterministic_backward(prev)


# ---- no float atomics in the compiled kernels ------------------------------------------------------------------------------------------
FLOAT_ATOMICS = ("atomic_add_f32", "atomic_add_f64", "atomic_pk_add", "ds_add_f32", "ds_add_rtn_f32", "ds_add_f64", "atomic_fadd",
                 "atomic_fmin", "atomic_fmax")


def test_no_float_atomics_in_the_compiled_kernels(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "hipcc is needed to compile msda_hip.hip to assembly"
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(REPO, "tools", "isa_audit.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    asm = audit.assembly("msda_hip.hip", str(tmp_path))     # build.py's flags, --cuda-device-only -S
    bodies = {name: ins for name, ins, _ in audit.kernels(asm)}
    new = {n: ins for n, ins in bodies.items() if "msda_bwd_det" in n}
    for stem in ("emit", "hist", "scan", "scatter", "bounds", "reduce"):
        assert any("msda_bwd_det_" + stem in n for n in new), stem
    assert sum("msda_bwd_det_emit" in n for n in new) == 2 and sum("msda_bwd_det_reduce" in n for n in new) == 2   # float, double
    for name, ins in new.items():
        assert len(ins) > 10, name
        for line in ins:
            assert not any(word in line for word in FLOAT_ATOMICS), (name, line)
    # the check has power: the default backward kernels of the same file do scatter with float atomics
    old = [line for n, ins in bodies.items() if "msda_bwd_f32_buf" in n or "msda_bwd_rowgather" in n for line in ins]
    assert any("atomic_add_f32" in line for line in old) and any("atomic_add_f64" in line for line in old)


# ---- host tensors --------------------------------------------------------------------------------------------------------------------------
def test_host_tensors_accept_and_ignore_the_flag(real):
    from trackformer_amd import msda
    case = U.make_case("unit", 2, 3, 8, 20, 2, [(5, 4), (2, 3)], seed=9)
    want = msda.ms_deform_attn_backward(*case, 64)
    for flag in (True, False, None):
        got = msda.ms_deform_attn_backward(*case, 64, deterministic=flag)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), flag
    prev = msda.set_deterministic_backward(True)
    try:
        got = msda.ms_deform_attn_backward(*case, 64)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    finally:
        msda.set_deterministic_backward(prev)
