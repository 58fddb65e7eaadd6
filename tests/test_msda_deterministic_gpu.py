"""GPU (-m gpu): the deterministic MSDeformAttn backward (msda_bwd_det<T>, trackformer_amd/csrc/msda_bwd_det.h) on the device.

  * every output against the float64 yardstick of tests/util_msda_numerics.py -- the bound the atomic kernels are held to -- on
    the shapes of the existing backward table, the full cfg-2 encoder at N = 2, the cfg-2 decoder and cfg 4;
  * bit equality of grad_value, grad_loc and grad_attn across repeated calls, a side stream, HIP-graph replay onto poisoned
    buffers, a GEMM loop on a second stream, host and device shapes, tf_msda_set_option knobs, and N = 2 against N = 1 slices;
  * gradcheck in fp64 with nondet_tol = 0, MSDeformAttn in training mode, torch.use_deterministic_algorithms, the compiled drop-in;
  * with the mode off the default kernels are dispatched as before."""
import ctypes
import os

import pytest
import torch

from oracle import msda_oracle
from tests import util_msda_numerics as U
from tests.test_msda_numerics_gpu import BWD, BWD_F64, CFG4_DEC
from tests.util_msda import CFG2_SHAPES

pytestmark = pytest.mark.gpu

THREADS = 16
S_CFG2 = sum(h * w for h, w in CFG2_SHAPES)
ENCODER = dict(N=2, M=8, D=32, Lq=S_CFG2, P=4, shapes=CFG2_SHAPES, encoder=True)
DECODER = dict(N=2, M=8, D=32, Lq=300, P=4, shapes=CFG2_SHAPES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    from trackformer_amd import _cabi
    _cabi.lib()
    torch.set_num_threads(min(torch.get_num_threads(), THREADS))
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_mode():
    """Every test starts with the mode unset everywhere and leaves it so."""
    from trackformer_amd import msda
    env = os.environ.pop("TF_MSDA_DETERMINISTIC", None)
    prev = msda.set_deterministic_backward(None)
    flag = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(False)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(flag, warn_only=warn)
        msda.set_deterministic_backward(prev)
        os.environ.pop("TF_MSDA_DETERMINISTIC", None)
        if env is not None:
            os.environ["TF_MSDA_DETERMINISTIC"] = env


def _kernel(dtype):
    return "msda_bwd_det<f32>" if dtype == torch.float32 else "msda_bwd_det<f64>"


def _on(dev, case, host=True):
    from trackformer_amd import msda
    value, shapes, loc, attn, grad_out = case
    ds = shapes.to(dev)
    if host:
        msda.attach_host_shapes(ds, shapes.tolist())
    return [value.to(dev), ds, loc.to(dev), attn.to(dev), grad_out.to(dev)]


def det(d):
    from trackformer_amd import msda
    grads = msda.ms_deform_attn_backward(*d, 64, deterministic=True)
    assert msda.last_kernel() == _kernel(d[0].dtype), msda.last_kernel()
    return grads


def _equal(a, b):
    """Bit equality (torch.equal would call -0 == +0 and miss a NaN)."""
    return all(torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int64),
                           y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)) for x, y in zip(a, b))


def run_yardstick(dev, case, host=True, fp32=True):
    d = _on(dev, case, host)
    gv, gl, ga = det(d)
    rv, rl, ra, left = U.backward_reference(d[0], case[1], d[2], d[3], d[4])
    assert left < U.EXCLUDE_MAX, left
    ov = ol = oa = None
    if fp32 and case[0].dtype == torch.float32:
        ov, ol, oa = msda_oracle.msda_backward(*[t.numpy() for t in case])
    for name, got, want, o in (("grad_value", gv, rv, ov), ("grad_loc", gl, rl, ol), ("grad_attn", ga, ra, oa)):
        print(name, U.check(got, want, fp32=o, what=name))
    assert not bool(gv[rv.n == 0].view(torch.int32 if gv.dtype == torch.float32 else torch.int64).any())   # +0 where nobody samples
    return gv, gl, ga


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["unit", "signed", "small", "hot_pixel", "permuted"])
@pytest.mark.parametrize("cid,kernel,opts,kw", BWD, ids=[c[0] for c in BWD])
def test_backward_table_shapes(dev, cid, kernel, opts, kw, profile):
    run_yardstick(dev, U.make_case(profile, seed=len(cid) + len(profile), **kw))


@pytest.mark.parametrize("profile", ["unit", "small", "hot_pixel"])
def test_float64(dev, profile):
    case = [t.double() if t.is_floating_point() else t for t in U.make_case(profile, seed=4, **BWD_F64[3])]
    run_yardstick(dev, case)


@pytest.mark.parametrize("profile", ["unit", "hot_pixel"])
def test_full_cfg2_encoder(dev, profile):
    run_yardstick(dev, U.make_case(profile, seed=22, **ENCODER))


@pytest.mark.parametrize("Lq", [300, 400])
def test_full_cfg2_decoder(dev, Lq):
    run_yardstick(dev, U.make_case("wide", 1, 8, 32, Lq, 4, CFG2_SHAPES, seed=Lq))


@pytest.mark.parametrize("shapes", [CFG4_DEC, CFG2_SHAPES * 4], ids=["l8", "l16"])
def test_full_cfg4_decoder(dev, shapes):
    run_yardstick(dev, U.make_case("unit", 1, 8, 36, 800, 4, shapes, seed=8))


def test_device_shapes_and_exact_edges(dev):
    case = U.exact_edge_case(1, 8, 32, 4, [(4, 8), (2, 2), (1, 1), (1, 4)], seed=7)
    d = _on(dev, case, host=False)
    got = det(d)
    rv, rl, ra, left = U.backward_reference(d[0], case[1], d[2], d[3], d[4], exact=True)
    assert left == 0.0
    for y, want, o in zip(got, (rv, rl, ra), msda_oracle.msda_backward(*[t.numpy() for t in case])):
        U.check(y, want, fp32=o)


# ---- bit equality ---------------------------------------------------------------------------------------------------------------------------
def _poison(*tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(0xFF)


@pytest.mark.parametrize("shape", ["encoder", "decoder"])
def test_bitwise_reproducible(dev, shape):
    from trackformer_amd import _cabi, msda
    kw = ENCODER if shape == "encoder" else DECODER
    case = U.make_case("hot_pixel" if shape == "decoder" else "unit", seed=31, **kw)
    d = _on(dev, case)
    want = det(d)
    torch.cuda.synchronize()

    for _ in range(5):                                         # consecutive calls
        assert _equal(det(d), want)

    side = torch.cuda.Stream(device=dev)                       # a side stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = det(d)
    side.synchronize()
    assert _equal(got, want)

    # a captured graph, replayed three times onto poisoned outputs and a poisoned workspace (the C ABI with a caller-owned one)
    lib = _cabi.lib()
    N, S, M, D = d[0].shape
    Lq, L, P = d[2].shape[1], d[2].shape[3], d[2].shape[4]
    nbytes = lib.tf_msda_backward_det_workspace_bytes(4, N, S, M, D, L, Lq, P)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    outs = [torch.empty_like(d[0]), torch.empty_like(d[2]), torch.empty_like(d[3])]
    shp_keep = msda._shape_array(tuple(tuple(hw) for hw in case[1].tolist()))
    shp = ctypes.cast(shp_keep, ctypes.c_void_p)

    def call():
        rc = lib.tf_msda_backward_det_f32(d[0].data_ptr(), shp, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                          outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), nbytes,
                                          N, S, M, D, L, Lq, P, torch.cuda.current_stream().cuda_stream)
        _cabi.check(rc, "tf_msda_backward_det_f32")
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        _poison(ws, *outs)
        graph.replay()
        torch.cuda.synchronize()
        assert _equal(outs, want)

    # other work on the device meanwhile: a GEMM loop on a second stream
    a, b = torch.randn(4096, 4096, device=dev), torch.randn(4096, 4096, device=dev)
    busy = torch.cuda.Stream(device=dev)
    busy.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(busy):
        for _ in range(40):
            torch.matmul(a, b)
    got = det(d)
    torch.cuda.synchronize()
    assert _equal(got, want)

    # host against device shapes, grad_value included
    assert _equal(det(_on(dev, case, host=False)), want)

    # kernel-selection knobs must not matter.  The guarantee rests on the code, not on this loop: backward_det_impl reads no option
    # and no environment variable at all (the backward switches TF_MSDA_BWD_ROWATOM / TF_MSDA_BWD_SORTED are read once per process
    # by the default path only and cannot be toggled here), so this can only pass; it pins that no knob is wired in later.
    for name, value in (("tiled", 0), ("quad_waves", 8), ("pquad", 0), ("direct9", 0)):
        prev = lib.tf_msda_set_option(name.encode(), value)
        try:
            assert _equal(det(d), want), name
        finally:
            lib.tf_msda_set_option(name.encode(), prev)

    # batch invariance: N = 2 against its N = 1 slices
    for n in range(N):
        one = [t[n:n + 1].contiguous() if i != 1 else t for i, t in enumerate(case)]
        assert _equal(det(_on(dev, one)), [g[n:n + 1] for g in want]), n


def test_batch_chunks_encoder_n3(dev):
    """The batch is walked in chunks of the images whose workspace fits 512 MiB: two at the cfg-2 encoder shape (240 MB per image),
    so N = 3 runs as chunks of 2 + 1 -- a second pass through the same workspace with offset operands and a ragged last chunk.
    The yardstick holds on all three images and each equals its own N = 1 call bit for bit."""
    from trackformer_amd import _cabi
    lib = _cabi.lib()
    dims = (S_CFG2, 8, 32, 4, S_CFG2, 4)
    one, two, three = (lib.tf_msda_backward_det_workspace_bytes(4, n, *dims) for n in (1, 2, 3))
    assert two == three and one < two < 512 << 20 < 3 * one, (one, two, three)        # N = 3 does not fit one chunk
    case = U.make_case("unit", seed=23, **dict(ENCODER, N=3))
    want = run_yardstick(dev, case)
    for n in range(3):
        part = [t[n:n + 1].contiguous() if i != 1 else t for i, t in enumerate(case)]
        assert _equal(det(_on(dev, part)), [g[n:n + 1] for g in want]), n


def test_gradcheck_with_zero_nondeterminism_tolerance(dev):
    from trackformer_amd import msda
    value, shapes, loc, attn, _ = [t.double() if t.is_floating_point() else t
                                   for t in U.make_case("unit", 1, 2, 4, 3, 2, [(6, 4), (3, 2)], seed=2)]
    value, loc, attn = value.to(dev), loc.clamp(0.05, 0.95).to(dev), attn.to(dev)
    ds = shapes.to(dev)
    for t in (value, loc, attn):
        t.requires_grad_(True)
    msda.set_deterministic_backward(True)
    seen = []   # the kernel behind every backward of the check (gradcheck itself ends with forward calls)
    value.register_hook(lambda g: seen.append(msda.last_kernel()))
    assert torch.autograd.gradcheck(lambda v, l, a: msda.MSDeformAttnFunction.apply(v, ds, l, a, 64), (value, loc, attn),
                                    eps=1e-6, atol=1e-5, rtol=1e-3, nondet_tol=0.0)
    assert seen and set(seen) == {"msda_bwd_det<f64>"}, seen


def _module_step(dev, mod, seed, seen=None):
    """One forward + backward; `seen` collects the library's last kernel as the autograd thread sees it when the input's gradient
    arrives (tf_msda_last_kernel is per thread, and backward runs on autograd's device thread)."""
    from trackformer_amd import msda
    g = torch.Generator().manual_seed(seed)
    shapes = torch.tensor([(25, 42), (13, 21), (7, 11), (4, 6)])
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    src = torch.randn(2, S, 256, generator=g).to(dev).requires_grad_(True)
    if seen is not None:
        src.register_hook(lambda grad: seen.append(msda.last_kernel()))
    query = torch.randn(2, 300, 256, generator=g).to(dev)
    refp = torch.rand(2, 300, 4, 2, generator=g).to(dev)
    ds = msda.attach_host_shapes(shapes.to(dev), shapes.tolist())
    mod.zero_grad(set_to_none=True)
    out = mod(query, refp, src, ds)
    (out * torch.randn(out.shape, generator=g).to(dev)).sum().backward()
    return [src.grad] + [p.grad for p in mod.parameters()]


def test_module_in_training_mode(dev):
    from trackformer_amd import msda
    torch.manual_seed(0)
    mod = msda.MSDeformAttn(256, 4, 8, 4).to(dev).train()
    with torch.no_grad():   # the initial sampling offsets do not depend on the query: perturb them so that every gradient is live
        mod.sampling_offsets.weight.normal_(0, 0.01)
        mod.attention_weights.weight.normal_(0, 0.01)
    msda.set_deterministic_backward(True)
    seen = []
    first = _module_step(dev, mod, 5, seen)
    assert seen == ["msda_bwd_det<f32>"], seen
    second = _module_step(dev, mod, 5)
    assert all(g is not None and bool(g.abs().sum() > 0) for g in first)
    assert _equal(first, second)
    # torch's flag alone selects the kernel (resolved at backward time)
    msda.set_deterministic_backward(None)
    seen = []
    _module_step(dev, mod, 5, seen)
    assert seen == ["msda_bwd_f32_buf<rowatom>"], seen
    torch.use_deterministic_algorithms(True)
    try:
        case = U.make_case("unit", seed=3, **DECODER)
        d = _on(dev, case)
        v, l, a = d[0].requires_grad_(True), d[2].requires_grad_(True), d[3].requires_grad_(True)
        seen = []
        v.register_hook(lambda grad: seen.append(msda.last_kernel()))
        msda.MSDeformAttnFunction.apply(v, d[1], l, a, 64).backward(d[4])
        assert seen == ["msda_bwd_det<f32>"], seen
        assert _equal([v.grad, l.grad, a.grad], det(d))
    finally:
        torch.use_deterministic_algorithms(False)


# ---- the compiled drop-in ---------------------------------------------------------------------------------------------------------------
def test_compiled_dropin_follows_the_environment_and_torch(dev):
    from trackformer_amd import dropin, msda
    ext = dropin.install(compiled=True)
    try:
        assert ext.__file__.endswith(".so")
        case = U.make_case("unit", seed=6, **DECODER)
        for host in (True, False):
            d = _on(dev, case, host)
            shp = case[1] if host else d[1]             # the extension takes host shapes as a CPU tensor
            want = det(d)
            ext.ms_deform_attn_backward(d[0], shp, d[2], d[3], d[4], 64)
            assert msda.last_kernel() == "msda_bwd_f32_buf<rowatom>"
            os.environ["TF_MSDA_DETERMINISTIC"] = "1"
            got = ext.ms_deform_attn_backward(d[0], shp, d[2], d[3], d[4], 64)
            assert msda.last_kernel() == "msda_bwd_det<f32>" and _equal(got, want)
            os.environ.pop("TF_MSDA_DETERMINISTIC")
            torch.use_deterministic_algorithms(True)
            try:
                got = ext.ms_deform_attn_backward(d[0], shp, d[2], d[3], d[4], 64)
                assert msda.last_kernel() == "msda_bwd_det<f32>" and _equal(got, want)
                os.environ["TF_MSDA_DETERMINISTIC"] = "0"           # the environment beats torch's flag
                ext.ms_deform_attn_backward(d[0], shp, d[2], d[3], d[4], 64)
                assert msda.last_kernel() == "msda_bwd_f32_buf<rowatom>"
            finally:
                torch.use_deterministic_algorithms(False)
                os.environ.pop("TF_MSDA_DETERMINISTIC", None)
    finally:
        dropin.install()


# ---- mode off: nothing changes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kernel,opts,kw", [c for c in BWD if c[0] in ("sorted2", "buf_rowatom", "rowgather_f32")],
                         ids=["rowgather", "buf_rowatom", "sorted2"])
def test_mode_off_dispatches_the_default_kernels(dev, cid, kernel, opts, kw):
    from trackformer_amd import msda
    d = _on(dev, U.make_case("unit", seed=1, **kw))
    assert msda.deterministic_backward_enabled() is False
    msda.ms_deform_attn_backward(*d, 64)
    assert msda.last_kernel() == kernel
    msda.ms_deform_attn_backward(*d, 64, deterministic=False)
    assert msda.last_kernel() == kernel
    os.environ["TF_MSDA_DETERMINISTIC"] = "1"
    msda.ms_deform_attn_backward(*d, 64)
    assert msda.last_kernel() == _kernel(d[0].dtype)
    os.environ["TF_MSDA_DETERMINISTIC"] = "0"
    msda.ms_deform_attn_backward(*d, 64)
    assert msda.last_kernel() == kernel
