"""Multi-scale deformable attention: the operator, its autograd wrapper and the nn.Module.

Host-side mirror of the reference's operator interface (names, argument meaning, error behaviour):

    reference (under /root/reference/src/trackformer/models/ops/)          here
    --------------------------------------------------------------------   ------------------------------
    MSDA.ms_deform_attn_forward / _backward   src/vision.cpp:4-7            ms_deform_attn_forward / _backward
    MSDeformAttnFunction                      functions/ms_deform_attn_func.py:14-31   MSDeformAttnFunction
    MSDeformAttn                              modules/ms_deform_attn.py:16-89          MSDeformAttn

All compute goes through the C ABI of libtf_msda.so (include/tf_msda.h).  Like the reference's dispatcher
(src/ms_deform_attn.h:16-28,37-49) the operator branches on where `value` lives: device tensors -> the HIP
kernels on the current stream (no host fallback, ever); host tensors -> tf_msda_*_host_* of the same library
(csrc/msda_host.cpp), the real CPU path SURVEY.md section 8(b) asks for where the reference raises
"Not implemented on the CPU".  All tensors of a call must live on the same device; a missing library fails both.
"""
import ctypes
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.init import constant_, xavier_uniform_

from . import _cabi, fused

import os as _os

# inference fast path of MSDeformAttn.forward (fused projections + fused operator prologue)
FUSED_INFERENCE = _os.environ.get("TF_MSDA_FUSED", "1") != "0"

_HOST_SHAPE_ATTR = "_tf_msda_host_shapes"
_shape_array_cache = {}


def attach_host_shapes(spatial_shapes, host_shapes):
    """Remember the (H_l, W_l) list of a device-resident `spatial_shapes` tensor on the tensor object.

    The reference keeps `spatial_shapes` only as an int64 device tensor (deformable_transformer.py:156)
    and reads it inside the kernel.  Callers that know the shapes on the host (our transformer does)
    attach them so that the operator can pass them by value and validate sum(H*W) == S without a
    device->host copy.  Purely an optimisation: without the attribute the *_dshapes entry points are used.
    """
    setattr(spatial_shapes, _HOST_SHAPE_ATTR, tuple((int(h), int(w)) for h, w in host_shapes))
    return spatial_shapes


def _host_shapes_of(spatial_shapes):
    hs = getattr(spatial_shapes, _HOST_SHAPE_ATTR, None)
    if hs is not None:
        return hs
    if not spatial_shapes.is_cuda:
        return tuple((int(h), int(w)) for h, w in spatial_shapes.tolist())
    return None


def _shape_array(host_shapes):
    arr = _shape_array_cache.get(host_shapes)
    if arr is None:
        flat = [v for hw in host_shapes for v in hw]
        arr = (ctypes.c_int64 * len(flat))(*flat)
        _shape_array_cache[host_shapes] = arr
    return arr


def _suffix(dtype):
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    raise RuntimeError("ms_deform_attn: only float32 and float64 are supported, got %s" % dtype)


def _check_inputs(value, spatial_shapes, sampling_loc, attn_weight, im2col_step):
    if not value.is_contiguous():
        raise RuntimeError("value tensor has to be contiguous")  # cu:29
    for name, t in (("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        if value.is_cuda and not t.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor" % name)  # cu:33-34 (HIP device here)
        if t.device != value.device:
            raise RuntimeError("%s is on %s but value is on %s" % (name, t.device, value.device))
        if t.dtype != value.dtype:
            raise RuntimeError("%s has dtype %s but value has %s" % (name, t.dtype, value.dtype))
    if value.dim() != 4 or sampling_loc.dim() != 6 or attn_weight.dim() != 5:
        raise RuntimeError("ms_deform_attn: expected value[N,S,M,D], sampling_loc[N,Lq,M,L,P,2], "
                           "attn_weight[N,Lq,M,L,P]")
    N, S, M, D = value.shape
    N2, Lq, M2, L, P, two = sampling_loc.shape
    if (N2, M2, two) != (N, M, 2) or tuple(attn_weight.shape) != (N, Lq, M, L, P):
        raise RuntimeError("ms_deform_attn: inconsistent tensor shapes")
    if spatial_shapes.dim() != 2 or tuple(spatial_shapes.shape) != (L, 2) \
            or spatial_shapes.dtype != torch.int64:
        raise RuntimeError("spatial_shapes must be an int64 tensor of shape [L, 2]")
    step = min(N, int(im2col_step))
    if step <= 0 or N % step != 0:  # cu:44-48
        raise RuntimeError("batch(%d) must divide im2col_step(%d)" % (N, step))
    return N, S, M, D, L, Lq, P


def _host_shape_tensor(spatial_shapes):
    """Contiguous int64 [L, 2] in host memory (host-tensor calls)."""
    if spatial_shapes.is_cuda:
        raise RuntimeError("spatial_shapes is on %s but value is on the CPU" % spatial_shapes.device)
    return spatial_shapes.contiguous()


def _shape_args(spatial_shapes, value):
    """Returns (tail, pointer-ish, keepalive) for the host- or device-shape entry point."""
    hs = _host_shapes_of(spatial_shapes)
    if hs is not None:
        arr = _shape_array(hs)
        return "", ctypes.cast(arr, ctypes.c_void_p), arr
    if spatial_shapes.device != value.device:
        raise RuntimeError("spatial_shapes must be a CUDA tensor")  # cu:32
    ss = spatial_shapes.contiguous()
    return "_dshapes", ctypes.c_void_p(ss.data_ptr()), ss


def last_kernel():
    """Name of the device kernel this thread's most recent operator call enqueued (tf_msda_last_kernel, include/tf_msda.h):
    what the library dispatched, not what the options suggest -- bench.py labels its roofline with it."""
    return _cabi.lib().tf_msda_last_kernel().decode()


_deterministic_backward = None   # set_deterministic_backward: True / False, None = follow the environment / torch


def set_deterministic_backward(flag):
    """True / False: device-tensor backward calls use (do not use) the bitwise-reproducible kernels (tf_msda_backward_det_*,
    include/tf_msda.h) whatever the environment and torch say; None: follow them again.  Returns the previous setting."""
    global _deterministic_backward
    prev = _deterministic_backward
    _deterministic_backward = None if flag is None else bool(flag)
    return prev


def deterministic_backward_enabled(deterministic=None):
    """Whether a backward call with `deterministic=` this argument runs the deterministic kernels: the argument, else
    set_deterministic_backward, else the environment variable TF_MSDA_DETERMINISTIC (1 / 0), else
    torch.are_deterministic_algorithms_enabled().  Read at every call (MSDeformAttnFunction: at backward time)."""
    if deterministic is not None:
        return bool(deterministic)
    if _deterministic_backward is not None:
        return _deterministic_backward
    env = _os.environ.get("TF_MSDA_DETERMINISTIC", "")
    if env in ("0", "1"):
        return env == "1"
    return bool(torch.are_deterministic_algorithms_enabled())


def ms_deform_attn_forward(value, spatial_shapes, sampling_loc, attn_weight, im2col_step=64):
    """value[N,S,M,D], spatial_shapes[L,2] i64, sampling_loc[N,Lq,M,L,P,2], attn_weight[N,Lq,M,L,P]
    -> output[N,Lq,M*D].   Same contract as the reference's MSDA.ms_deform_attn_forward
    (src/cuda/ms_deform_attn_cuda.cu:19-86); `im2col_step` is validated like the reference does and
    otherwise ignored (it never changed results)."""
    N, S, M, D, L, Lq, P = _check_inputs(value, spatial_shapes, sampling_loc, attn_weight,
                                         im2col_step)
    suf = _suffix(value.dtype)
    sampling_loc = sampling_loc.contiguous()
    attn_weight = attn_weight.contiguous()
    lib = _cabi.lib()
    if not value.is_cuda:   # host tensors: the library's host entry point (synchronous)
        out = torch.empty((N, Lq, M * D), dtype=value.dtype)
        shp = _host_shape_tensor(spatial_shapes)
        rc = getattr(lib, "tf_msda_forward_host_" + suf)(
            value.data_ptr(), shp.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(), out.data_ptr(),
            N, S, M, D, L, Lq, P)
        _cabi.check(rc, "ms_deform_attn_forward")
        return out
    with torch.cuda.device(value.device):
        out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
        tail, shp, keep = _shape_args(spatial_shapes, value)
        stream = torch.cuda.current_stream().cuda_stream
        rc = getattr(lib, "tf_msda_forward_%s%s" % (suf, tail))(
            value.data_ptr(), shp, sampling_loc.data_ptr(), attn_weight.data_ptr(), out.data_ptr(),
            N, S, M, D, L, Lq, P, stream)
    del keep
    _cabi.check(rc, "ms_deform_attn_forward")
    return out


def ms_deform_attn_backward(value, spatial_shapes, sampling_loc, attn_weight, grad_output,
                            im2col_step=64, deterministic=None):
    """-> [grad_value, grad_sampling_loc, grad_attn_weight], shaped like the respective inputs
    (reference: src/cuda/ms_deform_attn_cuda.cu:89-168).
    deterministic (device tensors; see deterministic_backward_enabled for None): the three gradients are bit-identical from
    call to call, on any stream, in a captured graph and for every batch size (no float atomics; slower, and it takes a
    workspace from torch's allocator).  Host tensors: accepted and ignored, that path is deterministic already."""
    N, S, M, D, L, Lq, P = _check_inputs(value, spatial_shapes, sampling_loc, attn_weight,
                                         im2col_step)
    suf = _suffix(value.dtype)
    if grad_output.device != value.device or grad_output.dtype != value.dtype \
            or grad_output.numel() != N * Lq * M * D:
        raise RuntimeError("grad_output must be a tensor of shape [N, Lq, M*D] on value's device with value's dtype")
    sampling_loc = sampling_loc.contiguous()
    attn_weight = attn_weight.contiguous()
    grad_output = grad_output.contiguous()  # autograd may hand over a strided view
    lib = _cabi.lib()
    if not value.is_cuda:
        grad_value, grad_loc, grad_attn = torch.empty_like(value), torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
        shp = _host_shape_tensor(spatial_shapes)
        rc = getattr(lib, "tf_msda_backward_host_" + suf)(
            value.data_ptr(), shp.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(), grad_output.data_ptr(),
            grad_value.data_ptr(), grad_loc.data_ptr(), grad_attn.data_ptr(), N, S, M, D, L, Lq, P)
        _cabi.check(rc, "ms_deform_attn_backward")
        return [grad_value, grad_loc, grad_attn]
    with torch.cuda.device(value.device):
        grad_value = torch.empty_like(value)  # zero-filled by the library on the stream
        grad_loc = torch.empty_like(sampling_loc)
        grad_attn = torch.empty_like(attn_weight)
        tail, shp, keep = _shape_args(spatial_shapes, value)
        stream = torch.cuda.current_stream().cuda_stream
        if deterministic_backward_enabled(deterministic):
            nbytes = lib.tf_msda_backward_det_workspace_bytes(value.element_size(), N, S, M, D, L, Lq, P)
            if nbytes < 0:
                _cabi.check(int(nbytes), "ms_deform_attn_backward (deterministic)")
            workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=value.device)
            rc = getattr(lib, "tf_msda_backward_det_%s%s" % (suf, tail))(
                value.data_ptr(), shp, sampling_loc.data_ptr(), attn_weight.data_ptr(),
                grad_output.data_ptr(), grad_value.data_ptr(), grad_loc.data_ptr(),
                grad_attn.data_ptr(), workspace.data_ptr(), int(nbytes), N, S, M, D, L, Lq, P, stream)
        else:
            rc = getattr(lib, "tf_msda_backward_%s%s" % (suf, tail))(
                value.data_ptr(), shp, sampling_loc.data_ptr(), attn_weight.data_ptr(),
                grad_output.data_ptr(), grad_value.data_ptr(), grad_loc.data_ptr(),
                grad_attn.data_ptr(), N, S, M, D, L, Lq, P, stream)
    del keep
    _cabi.check(rc, "ms_deform_attn_backward")
    return [grad_value, grad_loc, grad_attn]


def _qproj_rows(qproj):
    """(qproj, ld) as the fused entries read it: row (b, q) of qproj at (b * Lq + q) * ld.  A view whose columns are adjacent and
    whose batches are Lq rows apart (a column slice of a wider projection) is passed with its row stride, anything else as a
    contiguous copy."""
    N, Lq = qproj.shape[:2]
    ld = qproj.stride(1)
    if not (Lq > 1 and qproj.stride(2) == 1 and (N == 1 or qproj.stride(0) == Lq * ld) and ld >= qproj.shape[-1]
            and ld % 2 == 0 and qproj.data_ptr() % 8 == 0):
        qproj = qproj.contiguous()
        ld = qproj.shape[-1]
    return qproj, ld


def ms_deform_attn_forward_fused(value, spatial_shapes, reference_points, qproj, n_heads, n_levels,
                                 n_points):
    """Inference-only fused operator: softmax + sampling-location arithmetic + sampling in one launch.

    value [N,S,M,D]; reference_points [N,Lq,L,2|4]; qproj [N,Lq,3*M*L*P] = the query projected by the
    concatenated (sampling_offsets | attention_weights) Linear.  Equivalent to
    ms_deform_attn.py:69-86 followed by ms_deform_attn_forward; returns [N,Lq,M*D]."""
    hs = _host_shapes_of(spatial_shapes)
    if hs is None:
        raise RuntimeError("ms_deform_attn_forward_fused needs host-side level shapes "
                           "(attach_host_shapes)")
    if value.dim() != 4 or qproj.dim() != 3 or reference_points.dim() != 4:
        raise RuntimeError("ms_deform_attn_forward_fused: expected value[N,S,M,D], reference_points[N,Lq,L,2|4], "
                           "qproj[N,Lq,3*M*L*P]")
    for name, t in (("value", value), ("reference_points", reference_points), ("qproj", qproj)):
        if t.dtype != torch.float32:
            raise RuntimeError("ms_deform_attn_forward_fused: %s must be float32, got %s" % (name, t.dtype))
        if not t.is_cuda or t.device != value.device:
            raise RuntimeError("ms_deform_attn_forward_fused: %s must be a CUDA tensor on value's device" % name)
    if not value.is_contiguous():
        raise RuntimeError("ms_deform_attn_forward_fused: value tensor has to be contiguous")
    N, S, M, D = value.shape
    Lq = qproj.shape[1]
    L, P = n_levels, n_points
    if M != n_heads or qproj.shape[-1] != 3 * M * L * P or qproj.shape[0] != N \
            or tuple(reference_points.shape[:3]) != (N, Lq, L):
        raise RuntimeError("ms_deform_attn_forward_fused: inconsistent tensor shapes")
    reference_points = reference_points.contiguous()
    qproj, ld = _qproj_rows(qproj)
    lib = _cabi.lib()
    with torch.cuda.device(value.device):
        out = torch.empty((N, Lq, M * D), dtype=value.dtype, device=value.device)
        arr = _shape_array(hs)
        rc = lib.tf_msda_forward_fused_f32(
            value.data_ptr(), ctypes.cast(arr, ctypes.c_void_p), reference_points.data_ptr(),
            reference_points.shape[-1], qproj.data_ptr(), ld, 0, 2 * M * L * P,
            out.data_ptr(), N, S, M, D, L, Lq, P, torch.cuda.current_stream().cuda_stream)
    _cabi.check(rc, "ms_deform_attn_forward_fused")
    return out


class _CatProjection:
    """(sampling_offsets | attention_weights) as ONE Linear: the two projections share their input, so
    the inference path runs them as a single GEMM (refreshed when the parameters change)."""

    def __init__(self):
        self.key = None
        self.srcs = None
        self.weight = None
        self.bias = None

    def get(self, mod):
        srcs = (mod.sampling_offsets.weight, mod.sampling_offsets.bias,
                mod.attention_weights.weight, mod.attention_weights.bias)
        key = tuple(fused.source_key(t) for t in srcs)
        if key != self.key or not fused.same_sources(self.srcs, srcs):
            with torch.no_grad():
                self.weight = torch.cat([srcs[0], srcs[2]], 0).contiguous()
                self.bias = torch.cat([srcs[1], srcs[3]], 0).contiguous()
            self.key, self.srcs = key, srcs
        return self.weight, self.bias


# TRAINING THROUGH THE FUSED ENTRY (opt-in).  With gradients enabled MSDeformAttn runs the reference's module graph: two linears,
# view / softmax / division / add over [N, Lq, M, L, P, 2] and MSDeformAttnFunction, and its backward walks the same ATen chain in
# reverse.  set_fused_training(True) / TF_MSDA_FUSED_TRAIN=1 trains through the operator that is deployed instead: ONE linear over
# the concatenated (sampling_offsets | attention_weights) parameters and ms_deform_attn_fused, whose backward recomputes loc / attn
# (tf_msda_fused_prologue_f32), runs the operator's own backward and carries its gradients back to the raw projection
# (tf_msda_fused_backward_epilogue_f32).  OFF by default: whether a training step is faster with it is a measurement
# (tools/bench_msda_fused_train.py, profiles/msda_fused_train_bench.json), not a promise.
_fused_training = None   # None: follow TF_MSDA_FUSED_TRAIN (unset: off)
_FUSED_TRAIN_MAX_ROW_SAMPLES = 2048   # M*L*P the prologue / epilogue entries take (include/tf_msda.h); beyond it: today's graph
_fused_train_counts = {"fused": 0, "reference": 0}


def fused_training_enabled():
    if _fused_training is not None:
        return _fused_training
    return _os.environ.get("TF_MSDA_FUSED_TRAIN", "0") not in ("", "0")


def set_fused_training(flag):
    """Switch training through the fused entry on or off (process-wide; None: follow TF_MSDA_FUSED_TRAIN again); returns the
    previous setting."""
    global _fused_training
    prev = fused_training_enabled()
    _fused_training = None if flag is None else bool(flag)
    return prev


def fused_train_counts(reset=False):
    """With the switch on: how many MSDeformAttn forwards with gradients enabled took the fused path and how many the reference's
    module graph (a query_attn_mask, host tensors, no host shapes, another dtype or shape)."""
    out = dict(_fused_train_counts)
    if reset:
        for k in _fused_train_counts:
            _fused_train_counts[k] = 0
    return out


class MSDeformAttnFusedFunction(Function):
    """ms_deform_attn_fused: the fused entry with a backward.  Saves value, the reference points and qproj only."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, reference_points, qproj, n_heads, n_levels, n_points, deterministic):
        ctx.host_shapes = _host_shapes_of(spatial_shapes)
        ctx.dims = (n_heads, n_levels, n_points)
        ctx.deterministic = deterministic
        output = ms_deform_attn_forward_fused(value, spatial_shapes, reference_points, qproj, n_heads, n_levels, n_points)
        ctx.save_for_backward(value, spatial_shapes, reference_points, qproj)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, spatial_shapes, reference_points, qproj = ctx.saved_tensors
        attach_host_shapes(spatial_shapes, ctx.host_shapes)
        M, L, P = ctx.dims
        N, Lq = qproj.shape[:2]
        mlp = M * L * P
        ref_dim = reference_points.shape[-1]
        need_value, _, need_ref, need_q = ctx.needs_input_grad[:4]
        reference_points = reference_points.contiguous()
        qproj, ld = _qproj_rows(qproj)
        lib = _cabi.lib()
        shp = ctypes.cast(_shape_array(ctx.host_shapes), ctypes.c_void_p)
        with torch.cuda.device(value.device):
            stream = torch.cuda.current_stream().cuda_stream
            loc = torch.empty((N, Lq, M, L, P, 2), dtype=torch.float32, device=value.device)
            attn = torch.empty((N, Lq, M, L, P), dtype=torch.float32, device=value.device)
            rc = lib.tf_msda_fused_prologue_f32(reference_points.data_ptr(), ref_dim, qproj.data_ptr(), ld, 0, 2 * mlp, shp,
                                                loc.data_ptr(), attn.data_ptr(), N, M, L, Lq, P, stream)
            _cabi.check(rc, "ms_deform_attn_fused (prologue)")
            grad_value, grad_loc, grad_attn = ms_deform_attn_backward(value, spatial_shapes, loc, attn, grad_output,
                                                                      deterministic=ctx.deterministic)
            grad_q = grad_ref = None
            if need_q or need_ref:
                grad_q = torch.empty((N, Lq, 3 * mlp), dtype=torch.float32, device=value.device)
                grad_ref = torch.empty_like(reference_points) if need_ref else None
                rc = lib.tf_msda_fused_backward_epilogue_f32(
                    reference_points.data_ptr(), ref_dim, qproj.data_ptr(), ld, 0, 2 * mlp, shp, attn.data_ptr(),
                    grad_loc.data_ptr(), grad_attn.data_ptr(), grad_q.data_ptr(), 3 * mlp, 0, 2 * mlp,
                    0 if grad_ref is None else grad_ref.data_ptr(), N, M, L, Lq, P, stream)
                _cabi.check(rc, "ms_deform_attn_fused (epilogue)")
        return (grad_value if need_value else None, None, grad_ref, grad_q if need_q else None, None, None, None, None)


def ms_deform_attn_fused(value, spatial_shapes, reference_points, qproj, n_heads, n_levels, n_points, deterministic=None):
    """ms_deform_attn_forward_fused with gradients (fp32 device tensors, host shapes attached): the output is that entry's, bit for
    bit; the backward returns the gradients with respect to value, reference_points and the RAW projection qproj
    [N, Lq, 3*M*L*P] -- tf_msda_fused_prologue_f32 (loc / attn again, nothing but the three inputs is saved), then
    ms_deform_attn_backward(..., deterministic=deterministic) (None: see deterministic_backward_enabled, resolved at backward
    time), then tf_msda_fused_backward_epilogue_f32.  Apart from the operator's backward no float atomic is involved: with
    deterministic=True all three gradients are bit-identical from call to call.  Not differentiable twice."""
    return MSDeformAttnFusedFunction.apply(value, spatial_shapes, reference_points, qproj, n_heads, n_levels, n_points,
                                           deterministic)


class MSDeformAttnFunction(Function):
    """Autograd wrapper; mirrors functions/ms_deform_attn_func.py:14-31."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, sampling_locations, attention_weights,
                im2col_step):
        ctx.im2col_step = im2col_step
        ctx.host_shapes = _host_shapes_of(value_spatial_shapes)
        output = ms_deform_attn_forward(value, value_spatial_shapes, sampling_locations,
                                        attention_weights, ctx.im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, sampling_locations, attention_weights)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, value_spatial_shapes, sampling_locations, attention_weights = ctx.saved_tensors
        if ctx.host_shapes is not None:
            attach_host_shapes(value_spatial_shapes, ctx.host_shapes)
        grad_value, grad_sampling_loc, grad_attn_weight = ms_deform_attn_backward(
            value, value_spatial_shapes, sampling_locations, attention_weights, grad_output,
            ctx.im2col_step)
        return grad_value, None, grad_sampling_loc, grad_attn_weight, None


class _Normed:
    """Marker: MSDeformAttn._forward already applied the caller's residual add and LayerNorm."""
    __slots__ = ("value",)

    def __init__(self, value):
        self.value = value


class MSDeformAttn(nn.Module):
    """Same constructor, parameters (state_dict keys) and forward contract as the reference module
    (modules/ms_deform_attn.py:16-89)."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, im2col_step=64):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError("d_model must be divisible by n_heads, got %d and %d" %
                             (d_model, n_heads))
        self.im2col_step = im2col_step
        self.d_model = d_model
        self.n_levels = n_levels
        self.n_heads = n_heads
        self.n_points = n_points

        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._cat_proj = _CatProjection()
        self._reset_parameters()

    def _reset_parameters(self):
        # modules/ms_deform_attn.py:34-47.  The 8-direction table of the reference is the set of
        # unit steps ordered (-1,-1),(-1,0),(-1,1),(0,-1),(0,1),(1,-1),(1,0),(1,1); like the
        # reference it only fits n_heads == 8.
        # (in place on the parameters under no_grad, never through `.data`: a write through `.data` leaves no trace for the caches of
        # the weight images, and _reset_parameters() of a module that has already run would go unnoticed)
        with torch.no_grad():
            constant_(self.sampling_offsets.weight, 0.)
        dirs = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]
        if self.n_heads != len(dirs):
            raise ValueError("MSDeformAttn bias initialisation requires n_heads == 8")
        grid = torch.tensor(dirs, dtype=torch.float32).view(self.n_heads, 1, 1, 2)
        grid = grid.repeat(1, self.n_levels, self.n_points, 1)
        scale = torch.arange(1, self.n_points + 1, dtype=torch.float32).view(1, 1, -1, 1)
        with torch.no_grad():
            self.sampling_offsets.bias = nn.Parameter((grid * scale).reshape(-1))
            constant_(self.attention_weights.weight, 0.)
            constant_(self.attention_weights.bias, 0.)
            xavier_uniform_(self.value_proj.weight)
            constant_(self.value_proj.bias, 0.)
            xavier_uniform_(self.output_proj.weight)
            constant_(self.output_proj.bias, 0.)

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes,
                input_padding_mask=None, query_attn_mask=None, residual_norm=None, query_pos=None, value=None):
        """query[N,Lq,C], reference_points[N,Lq,L,2|4] in [0,1], input_flatten[N,S,C],
        input_spatial_shapes[L,2] (H_l,W_l), input_padding_mask[N,S] (True = padding)
        -> [N,Lq,C]   (modules/ms_deform_attn.py:49-89).
        residual_norm = (residual, nn.LayerNorm) (an extension used by the inference path of the layers): return
        norm(residual + attention output) instead -- the output projection, the add and the norm can then be one launch.
        query_pos (extension, inference path): the query is `query + query_pos`; the add can then ride in the projection.
        value (extension, inference path): value_proj(input_flatten) [N, S, C], computed by the caller (the decoder projects the
        memory for all its layers in one launch); the padding mask is still applied here."""
        if residual_norm is not None:
            out = self._forward(query, reference_points, input_flatten, input_spatial_shapes, input_padding_mask,
                                query_attn_mask, residual_norm, query_pos, value)
            if isinstance(out, _Normed):
                return out.value
            return fused.residual_norm(residual_norm[0], out, residual_norm[1], True)
        return self._forward(query, reference_points, input_flatten, input_spatial_shapes, input_padding_mask, query_attn_mask,
                             None, query_pos, value)

    def _forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_padding_mask, query_attn_mask,
                 residual_norm, query_pos=None, value=None):
        N, Len_q, _ = query.shape
        N, Len_in, _ = input_flatten.shape
        hs = _host_shapes_of(input_spatial_shapes)
        if hs is not None:
            if sum(h * w for h, w in hs) != Len_in:
                raise AssertionError("sum of H_l*W_l does not match the flattened input length")
        else:  # reference behaviour (one device sync), ms_deform_attn.py:62
            assert (input_spatial_shapes[:, 0] * input_spatial_shapes[:, 1]).sum() == Len_in

        M, L, P = self.n_heads, self.n_levels, self.n_points
        inference = not self.training and not torch.is_grad_enabled()
        # what the fused inference entry needs, apart from an fp32 device `value` (checked where it is used; linear_groups checks its input)
        fused_inference = (FUSED_INFERENCE and hs is not None and query_attn_mask is None and inference
                           and reference_points.shape[-1] in (2, 4) and (self.d_model // M) % 4 == 0 and P in (1, 2, 4, 8))
        qproj = None
        if value is not None and not inference:
            raise ValueError("MSDeformAttn: a precomputed `value` is an inference-path extension")
        if (value is None and fused_inference and query_pos is not None and input_flatten is query and fused.proj_groups_enabled("enc")
                and fused.pos_add_fused_enabled()):
            # the encoder layer: value_proj(src) and the query projections of src + pos share their rows: one launch
            w, b = self._cat_proj.get(self)
            ys = fused.linear_groups(query, query_pos, [(self.value_proj.weight, self.value_proj.bias, False), (w, b, True)])
            if ys is not None:
                value, qproj = ys
        if value is None:
            value = fused.module_linear(self.value_proj, input_flatten, inference)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], float(0))
        value = value.view(N, Len_in, M, self.d_model // M)

        if fused_inference and value.is_cuda and value.dtype == torch.float32:
            # inference: one GEMM for both query projections, prologue arithmetic inside the kernel
            w, b = self._cat_proj.get(self)
            if qproj is None and query_pos is not None:   # opt-in: the positional add inside the projection GEMM
                qproj = fused.linear_add(query, query_pos, w, b)
                if qproj is None:
                    query = query + query_pos
            if qproj is None:
                qproj = fused.linear(query, w, b) if fused.split_linear_enabled() else None
            if qproj is None:
                qproj = F.linear(query, w, b)
            output = ms_deform_attn_forward_fused(value, input_spatial_shapes, reference_points,
                                                  qproj, M, L, P)
            if residual_norm is not None:
                y = fused.linear_residual_norm(output, self.output_proj, residual_norm[0], residual_norm[1])
                if y is not None:
                    return _Normed(y)
            return fused.module_linear(self.output_proj, output, True)

        if query_pos is not None:
            query = query + query_pos
        if torch.is_grad_enabled() and fused_training_enabled():
            if (hs is not None and query_attn_mask is None and value.is_cuda and value.dtype == torch.float32
                    and query.is_cuda and query.dtype == torch.float32 and reference_points.is_cuda
                    and reference_points.dtype == torch.float32 and reference_points.shape[-1] in (2, 4)
                    and (self.d_model // M) % 4 == 0 and P in (1, 2, 4, 8) and M * L * P <= _FUSED_TRAIN_MAX_ROW_SAMPLES):
                # training through the deployed operator: ONE linear over a differentiable concatenation (autograd splits dW / db
                # back to the two modules; the weight images fused caches on the temporary die with it), then the fused entry
                _fused_train_counts["fused"] += 1
                w = torch.cat([self.sampling_offsets.weight, self.attention_weights.weight], 0)
                b = torch.cat([self.sampling_offsets.bias, self.attention_weights.bias], 0)
                qproj = fused.linear_train(query, w, b) if fused.train_route(query) else None
                if qproj is None:
                    qproj = F.linear(query, w, b)
                output = ms_deform_attn_fused(value, input_spatial_shapes, reference_points, qproj, M, L, P)
                return fused.module_linear(self.output_proj, output, False)
            _fused_train_counts["reference"] += 1
        sampling_offsets = fused.module_linear(self.sampling_offsets, query, False).view(N, Len_q, M, L, P, 2)
        attention_weights = fused.module_linear(self.attention_weights, query, False).view(N, Len_q, M, L * P)
        attention_weights = F.softmax(attention_weights, -1).view(N, Len_q, M, L, P)
        if query_attn_mask is not None:
            attention_weights = attention_weights.masked_fill(
                query_attn_mask[..., None, None, None], float(0))

        if reference_points.shape[-1] == 2:
            # NB: the divisor is (H_l, W_l) applied to (x, y) offsets, as written in the reference
            # (ms_deform_attn.py:78-79); checkpoints were trained with it.
            sampling_locations = reference_points[:, :, None, :, None, :] \
                + sampling_offsets / input_spatial_shapes[None, None, None, :, None, :]
        elif reference_points.shape[-1] == 4:
            sampling_locations = reference_points[:, :, None, :, None, :2] \
                + sampling_offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        else:
            raise ValueError('Last dim of reference_points must be 2 or 4, but get {} instead.'
                             .format(reference_points.shape[-1]))
        output = MSDeformAttnFunction.apply(value, input_spatial_shapes, sampling_locations,
                                            attention_weights, self.im2col_step)
        return fused.module_linear(self.output_proj, output, False)
