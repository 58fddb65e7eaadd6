"""GPU (-m gpu): every MSDeformAttn kernel against the float64 yardstick of tests/util_msda_numerics.py, per output element,
in every operand profile, at the shape edges where kernels go wrong, at exact sample positions, with NaN pixels, and with a
value tensor past the 32-bit buffer range.  Each case names the kernel it must reach and how it forces it (shape, dtype,
alignment, tf_msda_set_option); msda.last_kernel() is asserted after every call, and one test asserts that the cases reach
every kernel of the table.

With MSDA_NUMERICS_REPORT=<file> the worst normalised excess per (kernel, profile) is written there as JSON."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import msda_oracle
from tests import util_msda_numerics as U
from tests.util_msda import CFG2_SHAPES

pytestmark = pytest.mark.gpu

PYR = [(25, 42), (13, 21), (7, 11), (4, 6)]
S_PYR = sum(h * w for h, w in PYR)
CFG4_DEC = CFG2_SHAPES * 2
RAGGED16 = [(1, 1), (1, 7), (5, 1), (3, 4), (1, 1), (2, 9), (6, 1), (1, 3), (4, 4), (1, 1), (3, 1), (1, 2), (2, 2), (1, 5),
            (7, 1), (1, 1)]
RAGGED16 = [(1, 1)] + [(h, w) for h, w in RAGGED16[1:]]        # coarse level first
THREADS = 16

FWD = [   # id, kernel, options, dict(N, M, D, Lq, P, shapes, encoder)
    ("rowgather_f32", "msda_fwd_rowgather<f32>", {}, dict(N=2, M=3, D=5, Lq=33, P=3, shapes=[(7, 3), (1, 1), (2, 9)])),
    ("buf", "msda_fwd_f32_buf<plain>", {}, dict(N=1, M=4, D=64, Lq=100, P=4, shapes=[(12, 10), (6, 5)])),
    ("direct", "msda_fwd_f32_direct<plain>", {}, dict(N=1, M=8, D=32, Lq=300, P=4, shapes=CFG2_SHAPES)),
    ("direct9", "msda_fwd_f32_direct9<plain>", {}, dict(N=1, M=8, D=36, Lq=400, P=4, shapes=CFG4_DEC)),
    ("buf_d36", "msda_fwd_f32_buf<plain>", {"direct9": 0}, dict(N=2, M=8, D=36, Lq=70, P=4, shapes=PYR * 2)),
    ("quad", "msda_fwd_f32_quad<plain>", {"tiled": 1, "pquad": 0}, dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad", "msda_fwd_f32_pquad<plain>", {"pquad_v2": 0}, dict(N=2, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad_d36", "msda_fwd_f32_pquad<plain,D=36>", {}, dict(N=1, M=8, D=36, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2", "msda_fwd_f32_pquad2<plain,4w,2p>", {}, dict(N=2, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_1p", "msda_fwd_f32_pquad2<plain,4w,1p>", {"pquad_npass": 1},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_8w", "msda_fwd_f32_pquad2<plain,8w,1p>", {"pquad_waves": 8, "pquad_npass": 1, "pquad_wg_per_cu": 2, "pquad_lds_kb": 78},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_cf", "msda_fwd_f32_pquad2<plain,4w,2p,cf>", {"pquad_cf": 1},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_8w_cf", "msda_fwd_f32_pquad2<plain,8w,1p,cf>",
     {"pquad_cf": 1, "pquad_waves": 8, "pquad_npass": 1, "pquad_wg_per_cu": 2, "pquad_lds_kb": 78},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
]
FWD_F64 = ("rowgather_f64", "msda_fwd_rowgather<f64>", {}, dict(N=2, M=3, D=8, Lq=40, P=4, shapes=[(7, 3), (1, 1), (2, 9)]))
FUSED = [  # id, kernel, options, dict(..., ref_dim)
    ("buf", "msda_fwd_f32_buf<fused>", {}, dict(N=2, M=4, D=16, Lq=77, P=2, shapes=PYR, ref_dim=4)),
    ("direct", "msda_fwd_f32_direct<fused>", {}, dict(N=1, M=8, D=32, Lq=300, P=4, shapes=CFG2_SHAPES, ref_dim=2)),
    ("direct_r4", "msda_fwd_f32_direct<fused>", {}, dict(N=1, M=8, D=32, Lq=300, P=4, shapes=CFG2_SHAPES, ref_dim=4)),
    ("direct9", "msda_fwd_f32_direct9<fused>", {}, dict(N=1, M=8, D=36, Lq=400, P=4, shapes=CFG4_DEC, ref_dim=4)),
    ("quad", "msda_fwd_f32_quad<fused>", {"tiled": 1, "pquad": 0}, dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad", "msda_fwd_f32_pquad<fused>", {"pquad_v2": 0}, dict(N=2, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad_d36", "msda_fwd_f32_pquad<fused,D=36>", {}, dict(N=1, M=8, D=36, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2", "msda_fwd_f32_pquad2<fused,4w,2p>", {}, dict(N=2, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_1p", "msda_fwd_f32_pquad2<fused,4w,1p>", {"pquad_npass": 1},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_8w", "msda_fwd_f32_pquad2<fused,8w,1p>", {"pquad_waves": 8, "pquad_npass": 1, "pquad_wg_per_cu": 2, "pquad_lds_kb": 78},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_cf", "msda_fwd_f32_pquad2<fused,4w,2p,cf>", {"pquad_cf": 1},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("pquad2_8w_cf", "msda_fwd_f32_pquad2<fused,8w,1p,cf>",
     {"pquad_cf": 1, "pquad_waves": 8, "pquad_npass": 1, "pquad_wg_per_cu": 2, "pquad_lds_kb": 78},
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
]
BWD = [
    ("rowgather_f32", "msda_bwd_rowgather<f32>", {}, dict(N=2, M=3, D=5, Lq=33, P=3, shapes=[(7, 3), (1, 1), (2, 9)])),
    ("buf", "msda_bwd_f32_buf", {}, dict(N=2, M=4, D=16, Lq=90, P=2, shapes=PYR)),
    ("buf_rowatom", "msda_bwd_f32_buf<rowatom>", {}, dict(N=1, M=8, D=32, Lq=300, P=4, shapes=CFG2_SHAPES)),
    ("sorted2", "msda_bwd_f32_sorted2", {}, dict(N=2, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True)),
    ("rowgather_d36_cfg4", "msda_bwd_rowgather<f32>", {}, dict(N=1, M=8, D=36, Lq=200, P=4, shapes=CFG4_DEC)),
]
BWD_F64 = ("rowgather_f64", "msda_bwd_rowgather<f64>", {}, dict(N=2, M=3, D=8, Lq=40, P=4, shapes=[(7, 3), (1, 1), (2, 9)]))

TABLE = {c[1] for c in FWD + FUSED + BWD} | {FWD_F64[1], BWD_F64[1]}
REACHED = set()
REPORT = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    torch.set_num_threads(min(torch.get_num_threads(), THREADS))
    yield torch.device("cuda:0")
    path = os.environ.get("MSDA_NUMERICS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: REPORT[k] for k in sorted(REPORT)}, f, indent=1)


@pytest.fixture(autouse=True)
def _fp32_linears():
    from trackformer_amd import fused
    prev = fused.set_split_linear(False)
    yield
    fused.set_split_linear(prev)


@contextlib.contextmanager
def options(opts):
    from trackformer_amd import _cabi
    lib = _cabi.lib()
    prev = {k: lib.tf_msda_set_option(k.encode(), int(v)) for k, v in opts.items()}
    try:
        yield
    finally:
        for k, v in prev.items():
            lib.tf_msda_set_option(k.encode(), v)


def _ran(kernel):
    from trackformer_amd import msda
    got = msda.last_kernel()
    assert got == kernel, "dispatch reached %s, expected %s" % (got, kernel)
    REACHED.add(kernel)


def _record(kernel, profile, what, worst):
    key = "%s | %s | %s" % (kernel, profile, what)
    REPORT[key] = max(REPORT.get(key, 0.0), worst.value)


def _shapes_on(dev, shapes, host=True):
    from trackformer_amd import msda
    t = shapes.to(dev)
    if host:
        msda.attach_host_shapes(t, shapes.tolist())
    return t


def run_forward(dev, kernel, case, host=True, sample=None, profile="", exact=False):
    """case = (value, shapes, loc, attn, ...) on the CPU; runs the plain entry and checks every (sampled) query."""
    from trackformer_amd import msda
    value, shapes, loc, attn = case[:4]
    d = [value.to(dev), _shapes_on(dev, shapes, host), loc.to(dev), attn.to(dev)]
    out = msda.ms_deform_attn_forward(*d, 64)
    _ran(kernel)
    if sample is not None:
        idx = sample.to(dev)
        out, d[2], d[3] = out[:, idx], d[2][:, idx], d[3][:, idx]
        loc, attn = loc[:, sample], attn[:, sample]
    r = U.forward_reference(d[0], shapes, d[2], d[3], exact=exact)
    f32 = msda_oracle.msda_forward(value.numpy(), shapes.numpy(), loc.contiguous().numpy(), attn.contiguous().numpy(),
                                   nthreads=THREADS) if value.dtype == torch.float32 else None
    worst = U.check(out, r, fp32=f32, what=kernel)
    _record(kernel, profile, "out", worst)
    return out, r


def run_backward(dev, kernel, case, host=True, profile="", exact=False, fp32=True):
    from trackformer_amd import msda
    value, shapes, loc, attn, grad_out = case
    d = [value.to(dev), _shapes_on(dev, shapes, host), loc.to(dev), attn.to(dev), grad_out.to(dev)]
    gv, gl, ga = msda.ms_deform_attn_backward(*d, 64)
    _ran(kernel)
    rv, rl, ra, left = U.backward_reference(d[0], shapes, d[2], d[3], d[4], exact=exact)
    if exact:
        assert left == 0.0
    else:
        assert left < U.EXCLUDE_MAX, left
    ov = ol = oa = None
    if fp32 and value.dtype == torch.float32:
        ov, ol, oa = msda_oracle.msda_backward(*[t.numpy() for t in case])
    for name, got, want, o in (("grad_value", gv, rv, ov), ("grad_loc", gl, rl, ol), ("grad_attn", ga, ra, oa)):
        _record(kernel, profile, name, U.check(got, want, fp32=o, what=(kernel, name)))
    return gv, gl, ga


def run_fused(dev, kernel, shapes, value, refp, qproj, M, L, P, profile=""):
    from trackformer_amd import msda
    ds = _shapes_on(dev, shapes)
    out = msda.ms_deform_attn_forward_fused(value.to(dev), ds, refp.to(dev), qproj.to(dev), M, L, P)
    _ran(kernel)
    loc, a, dloc, da = U.fused_locations(shapes, refp.to(dev), qproj.to(dev), M, L, P)
    r = U.forward_reference(value.to(dev), shapes, loc, a, dloc=dloc, da=da)
    # the fp32 yardstick: the C oracle on the fp32 prologue (softmax with its max shift, x / H_l, y / W_l)
    hw = shapes.float().view(1, 1, 1, L, 1, 2)
    N, Lq = qproj.shape[:2]
    off = qproj[..., :2 * M * L * P].reshape(N, Lq, M, L, P, 2)
    fa = torch.softmax(qproj[..., 2 * M * L * P:3 * M * L * P].reshape(N, Lq, M, L * P), -1).reshape(N, Lq, M, L, P)
    if refp.shape[-1] == 2:
        floc = refp[:, :, None, :, None, :] + off / hw
    else:
        floc = refp[:, :, None, :, None, :2] + off / P * refp[:, :, None, :, None, 2:] * 0.5
    f32 = msda_oracle.msda_forward(value.numpy(), shapes.numpy(), floc.contiguous().numpy(), fa.contiguous().numpy(),
                                   nthreads=THREADS)
    worst = U.check(out, r, fp32=f32, what=kernel)
    _record(kernel, profile, "out", worst)
    return out


# ---- the coverage table x operand profiles ----------------------------------------------------------------------------------------------
def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("profile", U.PROFILES)
@pytest.mark.parametrize("cid,kernel,opts,kw", FWD, ids=_ids(FWD))
def test_forward_kernels(dev, cid, kernel, opts, kw, profile):
    case = U.make_case(profile, seed=len(cid) + len(profile), **kw)
    with options(opts):
        run_forward(dev, kernel, case, profile=profile)


@pytest.mark.parametrize("profile", ["unit", "large", "small"])
def test_forward_float64_kernel(dev, profile):
    cid, kernel, opts, kw = FWD_F64
    case = [t.double() if t.is_floating_point() else t for t in U.make_case(profile, seed=3, **kw)]
    run_forward(dev, kernel, case, profile=profile)


@pytest.mark.parametrize("profile", U.FUSED_PROFILES)
@pytest.mark.parametrize("cid,kernel,opts,kw", FUSED, ids=_ids(FUSED))
def test_fused_kernels(dev, cid, kernel, opts, kw, profile):
    kw = dict(kw)
    ref_dim = kw.pop("ref_dim", 2)
    enc = kw.pop("encoder", False)
    M, L, P = kw["M"], len(kw["shapes"]), kw["P"]
    value, shapes, refp, qproj = U.make_fused_case(profile, seed=len(cid) + len(profile), ref_dim=ref_dim, encoder=enc, **kw)
    with options(opts):
        run_fused(dev, kernel, shapes, value, refp, qproj, M, L, P, profile=profile)


@pytest.mark.parametrize("profile", U.PROFILES)
@pytest.mark.parametrize("cid,kernel,opts,kw", BWD, ids=_ids(BWD))
def test_backward_kernels(dev, cid, kernel, opts, kw, profile):
    case = U.make_case(profile, seed=len(cid) + len(profile), **kw)
    with options(opts):
        run_backward(dev, kernel, case, profile=profile)


@pytest.mark.parametrize("profile", ["unit", "small", "hot_pixel"])
def test_backward_float64_kernel(dev, profile):
    cid, kernel, opts, kw = BWD_F64
    case = [t.double() if t.is_floating_point() else t for t in U.make_case(profile, seed=4, **kw)]
    run_backward(dev, kernel, case, profile=profile)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------------
SHAPE_CASES = [  # id, (fwd kernel, bwd kernel), kw, host shapes
    ("d1_p1_m1_n3", ("msda_fwd_rowgather<f32>", "msda_bwd_rowgather<f32>"), dict(N=3, M=1, D=1, Lq=17, P=1, shapes=PYR), True),
    ("d3_p2_m3", ("msda_fwd_rowgather<f32>", "msda_bwd_rowgather<f32>"), dict(N=1, M=3, D=3, Lq=29, P=2, shapes=PYR), True),
    ("d16_p8_m8_n2", ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf"), dict(N=2, M=8, D=16, Lq=41, P=8, shapes=PYR), True),
    ("d128_p2_m1", ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf"), dict(N=1, M=1, D=128, Lq=40, P=2, shapes=PYR), True),
    ("d1024_p1", ("msda_fwd_f32_buf<plain>", "msda_bwd_rowgather<f32>"), dict(N=1, M=1, D=1024, Lq=9, P=1, shapes=[(6, 5), (3, 2)]), True),
    ("l16_ragged_one_pixel", ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf"), dict(N=1, M=3, D=8, Lq=50, P=2, shapes=RAGGED16), True),
    ("l16_p8_d64", ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf"), dict(N=1, M=1, D=64, Lq=20, P=8, shapes=RAGGED16), True),
    ("cfg4_d36_l8", ("msda_fwd_f32_direct9<plain>", "msda_bwd_rowgather<f32>"), dict(N=1, M=8, D=36, Lq=300, P=4, shapes=CFG4_DEC), True),
    ("device_shapes_d32", ("msda_fwd_f32_direct<plain>", "msda_bwd_f32_buf<rowatom>"), dict(N=2, M=8, D=32, Lq=130, P=4, shapes=PYR), False),
    ("device_shapes_encoder", ("msda_fwd_f32_direct<plain>", "msda_bwd_f32_buf<rowatom>"),
     dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True), False),
    ("device_shapes_d8", ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf"), dict(N=1, M=2, D=8, Lq=30, P=2, shapes=RAGGED16), False),
]


@pytest.mark.parametrize("profile", ["unit", "wide"])
@pytest.mark.parametrize("cid,kernels,kw,host", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_edges(dev, cid, kernels, kw, host, profile):
    case = U.make_case(profile, seed=len(cid), **kw)
    run_forward(dev, kernels[0], case, host=host, profile=profile)
    run_backward(dev, kernels[1], case, host=host, profile=profile)


def test_misaligned_value_d256(dev):
    """value one float off 16-byte alignment: the buffer kernels need aligned rows, the row-gather kernel takes the call."""
    from trackformer_amd import msda
    value, shapes, loc, attn, grad_out = U.make_case("unit", 1, 2, 256, 40, 4, PYR, seed=6)
    buf = torch.empty(value.numel() + 1, device=dev)
    v = buf[1:].view(value.shape)
    v.copy_(value.to(dev))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    ds = _shapes_on(dev, shapes)
    out = msda.ms_deform_attn_forward(v, ds, loc.to(dev), attn.to(dev), 64)
    _ran("msda_fwd_rowgather<f32>")
    f32 = msda_oracle.msda_forward(value.numpy(), shapes.numpy(), loc.numpy(), attn.numpy(), nthreads=THREADS)
    _record("msda_fwd_rowgather<f32>", "misaligned", "out", U.check(out, U.forward_reference(v, shapes, loc.to(dev), attn.to(dev)), fp32=f32))
    gv, gl, ga = msda.ms_deform_attn_backward(v, ds, loc.to(dev), attn.to(dev), grad_out.to(dev), 64)
    _ran("msda_bwd_rowgather<f32>")
    rv, rl, ra, _ = U.backward_reference(v, shapes, loc.to(dev), attn.to(dev), grad_out.to(dev))
    for got, want in ((gv, rv), (gl, rl), (ga, ra)):
        U.check(got, want)


# ---- full sizes: cfg 2 encoder / decoder, cfg 4 -------------------------------------------------------------------------------------------
def _sample(Lq, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(Lq, generator=g)[:k].sort().values


@pytest.mark.parametrize("profile", ["unit", "permuted", "level_spread"])
def test_full_cfg2_encoder_forward(dev, profile):
    S = sum(h * w for h, w in CFG2_SHAPES)
    case = U.make_case(profile, 1, 8, 32, S, 4, CFG2_SHAPES, seed=21, encoder=True)
    run_forward(dev, "msda_fwd_f32_pquad2<plain,4w,2p>", case, sample=_sample(S, 3000, 1), profile="cfg2_" + profile)


@pytest.mark.parametrize("profile", ["unit", "hot_pixel"])
def test_full_cfg2_encoder_backward(dev, profile):
    S = sum(h * w for h, w in CFG2_SHAPES)
    case = U.make_case(profile, 2, 8, 32, S, 4, CFG2_SHAPES, seed=22, encoder=True)
    run_backward(dev, "msda_bwd_f32_sorted2", case, profile="cfg2_" + profile)


@pytest.mark.parametrize("Lq", [300, 400])
def test_full_cfg2_decoder(dev, Lq):
    case = U.make_case("wide", 1, 8, 32, Lq, 4, CFG2_SHAPES, seed=Lq)
    run_forward(dev, "msda_fwd_f32_direct<plain>", case, profile="cfg2_decoder")
    run_backward(dev, "msda_bwd_f32_buf<rowatom>", case, profile="cfg2_decoder")


def test_full_cfg4(dev):
    case = U.make_case("unit", 1, 8, 36, 800, 4, CFG4_DEC, seed=8)
    run_forward(dev, "msda_fwd_f32_direct9<plain>", case, profile="cfg4_decoder")
    S = sum(h * w for h, w in CFG2_SHAPES)
    enc = U.make_case("unit", 1, 8, 36, S, 4, CFG2_SHAPES, seed=9, encoder=True)
    run_forward(dev, "msda_fwd_f32_pquad<plain,D=36>", enc, sample=_sample(S, 2000, 2), profile="cfg4_encoder")


# ---- exact positions, NaN pixels --------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(4, 8), (2, 2), (1, 1), (1, 4)]
S_EXACT = sum(h * w for h, w in EXACT_SHAPES)


@pytest.mark.parametrize("fk,bk,D,opts", [("msda_fwd_f32_direct<plain>", "msda_bwd_f32_buf<rowatom>", 32, {}),
                                          ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf", 16, {}),
                                          ("msda_fwd_rowgather<f32>", "msda_bwd_rowgather<f32>", 5, {}),
                                          ("msda_fwd_f32_direct9<plain>", "msda_bwd_rowgather<f32>", 36, {})],
                         ids=["direct", "buf", "rowgather", "direct9"])
def test_exact_edges(dev, fk, bk, D, opts):
    case = U.exact_edge_case(1, 8, D, 4, EXACT_SHAPES, seed=D)
    with options(opts):
        run_forward(dev, fk, case, profile="exact", exact=True)
        run_backward(dev, bk, case, profile="exact", exact=True)


@pytest.mark.parametrize("fk,opts", [("msda_fwd_f32_pquad2<plain,4w,2p>", {}), ("msda_fwd_f32_quad<plain>", {"tiled": 1, "pquad": 0}),
                                     ("msda_fwd_f32_pquad<plain>", {"pquad_v2": 0})], ids=["pquad2", "quad", "pquad"])
def test_exact_edges_encoder_shape(dev, fk, opts):
    case = U.exact_edge_case(1, 8, 32, 4, EXACT_SHAPES, seed=7, Lq=S_EXACT)
    with options(opts):
        run_forward(dev, fk, case, profile="exact", exact=True)
    run_backward(dev, "msda_bwd_f32_sorted2", case, profile="exact", exact=True)


NAN_CASES = [("msda_fwd_f32_direct<plain>", "msda_bwd_f32_buf<rowatom>", dict(N=1, M=8, D=32, Lq=300, P=4, shapes=PYR)),
             ("msda_fwd_f32_buf<plain>", "msda_bwd_f32_buf", dict(N=1, M=4, D=16, Lq=200, P=2, shapes=PYR)),
             ("msda_fwd_rowgather<f32>", "msda_bwd_rowgather<f32>", dict(N=1, M=3, D=5, Lq=200, P=3, shapes=PYR)),
             ("msda_fwd_f32_direct9<plain>", "msda_bwd_rowgather<f32>", dict(N=1, M=8, D=36, Lq=200, P=4, shapes=PYR)),
             ("msda_fwd_f32_pquad2<plain,4w,2p>", "msda_bwd_f32_sorted2", dict(N=1, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, encoder=True))]


@pytest.mark.parametrize("fk,bk,kw", NAN_CASES, ids=["direct", "buf", "rowgather", "direct9", "pquad2_sorted2"])
def test_nan_pixels(dev, fk, bk, kw):
    case = list(U.make_case("unit", seed=31, **kw))
    U.add_nan_pixels(case[0], case[2], case[1], 6, seed=5)
    _, r = run_forward(dev, fk, case, profile="nan")
    assert bool(r.expect_nan.any()) and not bool(r.expect_nan.all())
    run_backward(dev, bk, case, profile="nan")


# ---- the 32-bit buffer range ----------------------------------------------------------------------------------------------------------
def test_value_past_the_buffer_range_leaves_the_buffer_kernels(dev):
    """value of 4 GiB (kOobBase = 2^32 - 256 bytes, msda_common.h): buf_path_ok must send forward and backward to the row-gather
    kernels, whose 64-bit addressing reaches the last level's pixels; the results meet the bound there."""
    from trackformer_amd import msda
    shapes_l = [(1024, 2048), (1024, 2048)]
    N, M, D, Lq, P = 1, 8, 32, 64, 4
    S = sum(h * w for h, w in shapes_l)
    assert N * S * M * D * 4 > 0xFFFFFF00
    g = torch.Generator(device=dev).manual_seed(3)
    value = torch.randn(N, S, M, D, device=dev, generator=g)
    small = U.make_case("wide", N, M, D, Lq, P, [(4, 8)] * 2, seed=3)   # loc / attn / grad_out only
    loc, attn, grad_out = small[2].to(dev), small[3].to(dev), small[4].to(dev)
    loc[:, :, :, 1] = loc[:, :, :, 1].clamp(0.9, 1.02)                   # the far end of the second level (past 2^32 bytes)
    shapes = torch.tensor(shapes_l)
    ds = _shapes_on(dev, shapes)
    out = msda.ms_deform_attn_forward(value, ds, loc, attn, 64)
    _ran("msda_fwd_rowgather<f32>")
    _record("msda_fwd_rowgather<f32>", "past_4GiB", "out", U.check(out, U.forward_reference(value, shapes, loc, attn)))
    gv, gl, ga = msda.ms_deform_attn_backward(value, ds, loc, attn, grad_out, 64)
    _ran("msda_bwd_rowgather<f32>")
    rv, rl, ra, _ = U.backward_reference(value, shapes, loc, attn, grad_out)
    for name, got, want in (("grad_value", gv, rv), ("grad_loc", gl, rl), ("grad_attn", ga, ra)):
        _record("msda_bwd_rowgather<f32>", "past_4GiB", name, U.check(got, want))


# ---- subnormal addends in the fp32 atomics ------------------------------------------------------------------------------------------
def test_subnormal_addends_survive_the_atomics(dev):
    """Probe (recorded in the report): 4096 addends of 2^-140 summed by device atomics (index_add_), and the grad_value of the
    atomic backward kernels with every contribution below 2^-126.  grad_value's floor assumes the addends are kept."""
    acc = torch.zeros(1, device=dev).index_add_(0, torch.zeros(4096, dtype=torch.long, device=dev),
                                                 torch.full((4096,), 2.0 ** -140, device=dev))
    REPORT["probe | index_add_ 4096 x 2^-140 | got / exact"] = float(acc.cpu().double()) / (4096 * 2.0 ** -140)
    value, shapes, loc, attn, grad_out = U.make_case("hot_pixel", 1, 8, 32, 300, 4, PYR, seed=12)
    grad_out = grad_out * 2.0 ** -128
    for kernel, case in (("msda_bwd_f32_buf<rowatom>", (value, shapes, loc, attn, grad_out)),):
        gv, _, _ = run_backward(dev, kernel, case, profile="subnormal_addends")
        rv = U.backward_reference(value.to(dev), shapes, loc.to(dev), attn.to(dev), grad_out.to(dev))[0]
        REPORT["probe | %s grad_value sum | got / exact" % kernel] = float(gv.double().sum() / rv.ref.sum())
    assert float(acc.cpu().double()) == 4096 * 2.0 ** -140


# ---- the fused entry's input layout ---------------------------------------------------------------------------------------------------
def test_fused_entry_input_layouts(dev):
    """A column slice of a wider projection (passed with its row stride), a transposed view (copied), an fp16 qproj and a
    non-contiguous value (refused): each gives the right result or raises."""
    from trackformer_amd import msda
    M, L, P = 8, len(CFG2_SHAPES), 4
    value, shapes, refp, qproj = U.make_fused_case("unit", 2, M, 32, 300, P, CFG2_SHAPES, seed=13)
    ds = _shapes_on(dev, shapes)
    want = run_fused(dev, "msda_fwd_f32_direct<fused>", shapes, value, refp, qproj, M, L, P, profile="layout")
    W = qproj.shape[-1]
    wide = torch.randn(2, 300, W + 40, device=dev)
    wide[..., 24:24 + W] = qproj.to(dev)
    got = msda.ms_deform_attn_forward_fused(value.to(dev), ds, refp.to(dev), wide[..., 24:24 + W], M, L, P)
    assert torch.equal(got, want)
    t = qproj.to(dev).transpose(1, 2).contiguous().transpose(1, 2)
    assert not t.is_contiguous()
    assert torch.equal(msda.ms_deform_attn_forward_fused(value.to(dev), ds, refp.to(dev), t, M, L, P), want)
    with pytest.raises(RuntimeError, match="float32"):
        msda.ms_deform_attn_forward_fused(value.to(dev), ds, refp.to(dev), qproj.to(dev).half(), M, L, P)
    with pytest.raises(RuntimeError, match="float32"):
        msda.ms_deform_attn_forward_fused(value.to(dev), ds, refp.to(dev).double(), qproj.to(dev), M, L, P)
    vt = value.to(dev).transpose(2, 3).contiguous().transpose(2, 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        msda.ms_deform_attn_forward_fused(vt, ds, refp.to(dev), qproj.to(dev), M, L, P)


def test_every_kernel_of_the_table_is_reached(dev):
    """Runs last in this module: the cases above reached every kernel name the table lists."""
    assert TABLE - REACHED == set(), sorted(TABLE - REACHED)
