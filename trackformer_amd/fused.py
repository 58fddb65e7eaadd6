"""Python front-end of the fused element-wise HIP kernels (include/tf_fused.h).

The first part serves the inference path (eval mode, gradients disabled) on GPU tensors.  The training sections further down (THE
TRAINING PATH OF ..., DROPOUT INSIDE THE TRAINING KERNELS) are opt-in autograd Functions over the library's own backward kernels, each
behind a process-wide switch that is off by default.  Everywhere else the callers keep the plain PyTorch formulation (these helpers
return None when they do not apply)."""
import ctypes
import os
import threading

import torch
import torch.nn.functional as F

from . import _cabi


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _param_ok(t, x):
    """A parameter tensor the kernels can read next to `x`: same device, fp32, contiguous, 16-byte aligned."""
    return (t.device == x.device and t.dtype == torch.float32 and t.is_contiguous()
            and t.data_ptr() % 16 == 0)


# ---------------------------------------------------------------------------------------------------------
# COHERENCE OF THE CACHED WEIGHT IMAGES.  The inference path never reads an nn.Parameter directly: it reads an image derived from
# it (16-bit pieces, fragment-order packings, BN-folded / tap-major convolution weights, concatenated projections), built once and
# cached.  Every such cache keys on source_key() of each tensor it was derived from; a cache stored on a MODULE also remembers the
# source tensor objects (same_sources): a parameter object that was replaced starts again at version 0.  What this detects by itself:
# every write that bumps the version counter (in place under no_grad, load_state_dict, optimiser steps, writes through detach(),
# set_) and every change of the storage or the tensor object behind a parameter (p.data = t, vector_to_parameters, module.to(),
# load_state_dict(assign=True), a new nn.Parameter, swap_tensors, copy.deepcopy).  What it cannot: a write THROUGH `.data`
# (p.data.mul_(), nn.init.*_(p.data)) leaves no trace on the tensor -- call weights_changed() after one.
_weight_epoch = 0
_route_epoch = 0              # see route_epoch() below


def weight_epoch():
    return _weight_epoch


def weights_changed():
    """Tell the library that weights were changed in a way it cannot see: a write through `.data` (`p.data.mul_(2)`,
    `nn.init.normal_(p.data)`), which leaves the tensor's version counter, storage and identity as they were.  Bumps a process-wide
    weight epoch that is part of every cached weight image's key: every image (split pieces, packed fragments, folded convolution
    weights, concatenated projections, cached reference points) is rebuilt lazily at its next use, and a GraphedDetector drops its
    captured graphs at its next call.  Everything else -- in-place writes under no_grad, load_state_dict, optimiser steps, `p.data = t`,
    module.to(), a replaced nn.Parameter -- is detected without this call (a GraphedDetector that replays graphs notices those at
    load_state_dict, at Tracker.reset() and at revalidate()).  Cheap to call, costly afterwards: the next forward rebuilds every
    image.  Returns the new epoch."""
    global _weight_epoch
    _weight_epoch += 1
    return _weight_epoch


def source_key(t):
    """The part of a cache key that stands for one source tensor (None allowed): version counter, address, device, dtype and the
    weight epoch.  The address alone would not do (a freed parameter's address is handed to the next model's parameters by the
    caching allocator): caches live ON the tensor object or remember it (same_sources)."""
    if t is None:
        return None
    return (t._version, t.data_ptr(), t.device, t.dtype, _weight_epoch)


def same_sources(held, srcs):
    """The tensor OBJECTS a module-level cache was built from are the ones the module holds now."""
    return held is not None and len(held) == len(srcs) and all(a is b for a, b in zip(held, srcs))


def _switched(prev, new):
    """A process-wide switch was set: what a forward enqueues changes exactly when its value does -> route_epoch()."""
    global _route_epoch
    if prev != new:
        _route_epoch += 1
    return prev


def bias_act_(x, bias, residual=None, relu=True):
    """In place: x = act(x + bias[c] (+ residual)) for a channels_last [N,C,H,W] fp32 GPU tensor.
    Returns x, or None when the tensors do not qualify -- a residual that is x itself included -- (caller falls back to ATen ops)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last)):
        return None
    C = x.shape[1]
    if C % 4 or not _param_ok(bias, x) or x.data_ptr() % 16:
        return None
    if residual is not None and not (residual.data_ptr() != x.data_ptr() and residual.shape == x.shape and residual.dtype == x.dtype
                                     and residual.device == x.device and residual.data_ptr() % 16 == 0
                                     and residual.is_contiguous(memory_format=torch.channels_last)):
        return None
    with torch.cuda.device(x.device):   # the launch goes to x's device and its current stream
        rc = _cabi.lib().tf_bias_act_f32(x.data_ptr(), bias.data_ptr(),
                                         0 if residual is None else residual.data_ptr(), x.numel(), C,
                                         1 if relu else 0, _stream(x.device))
    _cabi.check(rc, "tf_bias_act_f32")
    return x


def add_layernorm(x, res, norm):
    """LayerNorm(x + res) with `norm`'s affine parameters in one pass (res may be None).
    Returns a new tensor, or None when the fused kernel does not apply."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            and norm.elementwise_affine and len(norm.normalized_shape) == 1):
        return None
    C = norm.normalized_shape[0]
    if x.shape[-1] != C or C % 4 or C > 4096 or x.data_ptr() % 16:
        return None
    if not (_param_ok(norm.weight, x) and _param_ok(norm.bias, x)):
        return None
    if res is not None:
        if res.shape != x.shape or res.dtype != x.dtype or res.device != x.device:
            return None
        res = res.contiguous()
        if res.data_ptr() % 16:
            return None
    with torch.cuda.device(x.device):
        out = torch.empty_like(x)
        rc = _cabi.lib().tf_add_layernorm_f32(x.data_ptr(), 0 if res is None else res.data_ptr(),
                                              norm.weight.data_ptr(), norm.bias.data_ptr(),
                                              out.data_ptr(), x.numel() // C, C, float(norm.eps),
                                              _stream(x.device))
    _cabi.check(rc, "tf_add_layernorm_f32")
    return out


def residual_norm(x, res, norm, inference, dropout=None):
    """norm(x + res): fused on the GPU inference path; with gradients enabled and set_layernorm_training(True) the same kernel with the
    library's own backward (layernorm_train); plain PyTorch otherwise.  dropout: the site's nn.Dropout, norm(x + dropout(res)) -- applied
    here, at the point the caller used to apply it, unless set_dropout_training() takes the site (dropout_residual_norm)."""
    if dropout is not None:
        if not inference:
            y = dropout_residual_norm(x, res, norm, dropout)
            if y is not None:
                return y
        res = dropout(res)
    if inference:
        y = add_layernorm(x, res, norm)
        if y is not None:
            return y
    elif layernorm_train_route(x):
        y = layernorm_train(x, res, norm)
        if y is not None:
            return y
    return norm(x + res)


# ---------------------------------------------------------------------------------------------------------
# nn.Linear as a bf16 split product on the matrix cores (include/tf_fused.h: tf_linear_split_f32).  ON by default
# in the GPU inference path (TF_SPLIT_LINEAR=0 / set_split_linear(False): the fp32 library GEMMs): faster than the
# tuned hipBLASLt selections at the encoder shapes, 172.3 -> 173.2 frames/s end to end (4 sequences; 128.6 -> 131.3
# with one), and inside the parity bar at the BASELINE sizes (tests/test_full_size_gpu.py: boxes 1e-6, logits 6e-5,
# track ids exact).
_split_linear = os.environ.get("TF_SPLIT_LINEAR", "1") not in ("", "0")


def split_linear_enabled():
    return _split_linear


def set_split_linear(on):
    """Switch the split-product linears on or off (process-wide); returns the previous setting."""
    global _split_linear
    prev, _split_linear = _split_linear, bool(on)
    return _switched(prev, _split_linear)


# The arithmetic of a split product (include/tf_fused.h, THE SPLIT PRODUCT; csrc/split_product.h):
#   6   bf16 pieces (hi, mid, lo) per operand, six terms: all 24 significand bits, dropped terms below 2^-24 of the product -- the
#       reference's fp32 arithmetic in another summation order.
#   16  fp16 pieces: (hi, lo) of the activation x (hi, lo, hi 2^-11) of the weight, THREE terms: 22 + 1 significand bits, the only
#       dropped product below 2^-22; weights scaled per output channel and the lo piece stored times 2^11 so that nothing falls
#       into fp16's subnormals.  Half the matrix work of 6 at fp32-class accuracy: THE DEFAULT (round 4).  MI355X, cfg 2: 396.9
#       frames/s against 295.6 with six terms (410.3 with three bf16 terms, 193.9 on the fp32 libraries); full-size logits 1.2e-5 /
#       boxes 5.4e-7 from the reference (six terms: 1.6e-5 / 5.4e-7); the reference's track ids on all 64 frames of the 64-frame
#       fixture in both runs (six terms: 26 frames, the fp32 libraries 59 / 26): profiles/r04_id_parity_64_with_fp16.txt.
# (3 = bf16 pieces (hi, mid), three terms, products good to 2^-16 -- the "fast mode" of rounds 2-4 -- was REMOVED in round 5: the
# fp16 product runs at the same speed, and the 64-frame reference-Tracker fixture keeps the reference's track ids for 59 frames
# under fp32 library GEMMs but only 14 under three bf16 terms, profiles/r04_id_parity_64.txt.)
def _parse_terms(v):
    v = str(v).strip().lower()
    if v in ("6", "16"):
        return int(v)
    if v in ("f16", "fp16", "half"):
        return 16
    if v == "3":
        raise ValueError("split terms 3 (the three-term bf16 fast mode) was removed in round 5: use 16 (fp16 pieces, the default: "
                         "same speed, fp32-class accuracy) or 6 (six bf16 terms)")
    raise ValueError("split terms: 6 or 16 (fp16 pieces)")


_split_terms = _parse_terms(os.environ.get("TF_SPLIT_TERMS", "16"))
_tls = threading.local()   # .terms: a routed layer's six-term product, for the CALLING thread only (see _ranged)


def split_terms():
    return _split_terms


def _terms():
    """The split product of the call being made: the calling thread's override (a layer routed to six terms) or the process-wide
    setting.  Every kernel call and every weight-image cache of this module reads it through here."""
    return getattr(_tls, "terms", None) or _split_terms


def set_split_terms(n):
    """6 (bf16 pieces, six terms) or 16 (fp16 pieces, three terms) per split product (process-wide; cached weight images are kept per
    setting); returns the previous value."""
    global _split_terms
    n = _parse_terms(n)
    prev, _split_terms = _split_terms, n
    return _switched(prev, _split_terms)


# The same product with the weight packed once in matrix-core fragment order (tf_linear_packed_f32,
# csrc/linear_stream.hip): bit-identical results.  Used where it measured faster (profiles/r02_split_gemm_packed.txt):
# many rows and a wide output or a long K -- the FFN linears of the encoder (22 223 x 256 -> 1024: 76.2 -> 59.3 us,
# 1024 -> 256: 63.6 -> 50.5 us).  TF_LINEAR_PACKED=0 / set_packed_linear(False): the unpacked kernel everywhere.
_packed_linear = os.environ.get("TF_LINEAR_PACKED", "1") not in ("", "0")
_PACKED_MIN_ROWS = 4096


def _use_packed(M, K, N):
    """Shapes tf_linear_packed_f32 (the stream GEMM: weight fragments from L2, only the activations through LDS) is the faster
    kernel for.  Its column blocks (64 / 128 / 256 wide) must be mostly full.  Six terms: every many-row shape with K >= 256 -- at
    equal matrix work it beats the LDS-staged block kernel there (22 223 rows: 256 -> 256 23.9 vs 26.3 us, 256 -> 1024 67.5 vs
    84.7, 1024 -> 256 65.6 vs 88.0, profiles/r04_pmc_dense_six_terms.txt; the reducing 1 x 1 convolutions of ResNet-50 25.2 vs
    35.6 / 24.8 vs 28.9 / 35.9 vs 42.2 us) but not under a short K, where its prologue is most of the block (the expanding 1 x 1
    convolutions with their residual: K = 64: 34.8 vs 30.4 us, K = 128: 28.8 vs 26.0; profiles/r04_conv_per_layer_stream_vs_block.txt).
    Two stored weight pieces (the fp16 product): a wide output or a long K only (at K = 256, N <= 384 the many small blocks of the
    block kernel hide the memory latency better: 21.4 vs 22.8 us)."""
    if not _packed_linear or M <= _PACKED_MIN_ROWS or K % 64:
        return False
    tail = N % 256
    full = N <= 128 or tail == 0 or tail > 128
    if _terms() == 6:
        return full and K >= 256
    # two stored weight pieces (fp16 pieces; measured: profiles/r04_f16_harness.txt: 22 223 x 256 -> 256 18.4 vs 18.7 us, 16 700 x 512 -> 128 16.1 vs 21.6, 66 800 x 64 -> 256
    # 20.8 vs 19.3, 16 700 x 128 -> 512 17.3 vs 17.4)
    return (N >= 512 or K >= 512) and full


def set_packed_linear(on):
    """Switch the packed-weight kernel for the many-row linears on or off (process-wide); returns the previous setting."""
    global _packed_linear
    prev, _packed_linear = _packed_linear, bool(on)
    return _switched(prev, _packed_linear)


def _publish_barrier(device):
    """Cached weight images are built on the caller's current stream and then published on the tensor for EVERY stream
    (one tracker thread per sequence, each on its own HIP stream, share one model): wait for the building stream before
    publishing, so that a second thread's first GEMM cannot read a half-written image.  Once per weight."""
    if getattr(_tls, "one_stream", 0) and os.environ.get("TF_TRAIN_PUBLISH_BARRIER") != "1":
        return   # (a training step: the images are rebuilt every step for the stream that uses them next, see one_stream())
    if not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).synchronize()


class one_stream:
    """with fused.one_stream(): weight images built inside are used by the calling thread's current stream only -- no host
    synchronisation when they are published.  The previous-frame pass of a TRAINING step (no_grad, inference kernels: backbone.
    _fold_mode) rebuilds the images of every trainable convolution after every optimiser step; ~80 stream synchronisations per
    step otherwise."""

    def __enter__(self):
        _tls.one_stream = getattr(_tls, "one_stream", 0) + 1

    def __exit__(self, *exc):
        _tls.one_stream -= 1
        return False


def _packed_weight(weight, rows):
    """Fragment-order image (the bf16 pieces of the current split_terms()) of `weight` (or of its row block `rows`), built by
    tf_linear_pack_weight_f32 and cached on the tensor object under its source_key(), like _split_weight below."""
    cache = getattr(weight, "_tf_packed", None)
    key = source_key(weight)
    if cache is None or cache[0] != key:
        cache = (key, {})
        weight._tf_packed = cache
    terms = _terms()
    hit = cache[1].get((rows, terms))
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            return None   # never build a cached buffer inside a graph's memory pool: this call takes the unpacked kernel
        N, K = weight.shape
        a, b = (0, N) if rows is None else rows
        nbytes = _cabi.lib().tf_linear_packed_bytes(K, b - a, terms)
        if nbytes <= 0:
            return None
        w = weight.detach()
        with torch.cuda.device(weight.device):
            hit = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
            rc = _cabi.lib().tf_linear_pack_weight_f32(w.data_ptr() + a * K * 4, hit.data_ptr(), K, b - a, terms,
                                                       _stream(weight.device))
        _cabi.check(rc, "tf_linear_pack_weight_f32")
        _publish_barrier(weight.device)
        cache[1][(rows, terms)] = hit
    return hit


def _split_weight(weight):
    """The 16-bit pieces of an fp32 weight [N, K] for the kernels that take them as separate tensors (include/tf_fused.h, THE
    SPLIT PRODUCT) -> (p0, p1, p2, scale):
      split_terms() 6       bf16 hi, mid, lo; scale None
      split_terms() 16      fp16 wh = f16(w t_n), wl = f16(w t_n - wh), None, and scale[n] = 16 / t_n (fp32), t_n the power of two
                            that puts the largest |w| of output channel n into [2^13, 2^14)
    (round to nearest even at every step).  Cached ON THE TENSOR OBJECT under its source_key(): version counter (an
    in-place update bumps it), address, device and dtype (`p.data = t`, module.to() change the storage and keep the
    version) and the weight epoch (weights_changed(): writes through `.data`).  Not keyed by data_ptr ALONE in a table: a
    freed parameter's address is handed to the next model's parameters by the caching allocator, and a pointer-keyed cache
    then serves another tensor's pieces (seen as a golden failure when two test models were built one after the
    other).  Callers pass persistent tensors (module parameters, _CatProjection's concatenation), and use `rows=` of
    linear() for a row block instead of a temporary slice."""
    if _terms() == 16:
        hit = getattr(weight, "_tf_split_f16", None)
        key = source_key(weight)
        if hit is None or hit[0] != key:
            w = weight.detach()
            amax = w.abs().amax(dim=1)
            _, e = torch.frexp(amax)                                   # amax = m 2^e with m in [0.5, 1): floor(log2 amax) = e - 1
            # 2^(14 - e) from its exponent bits (torch.ldexp goes through pow(), which is not exact on every device)
            t = ((torch.clamp(14 - e, -100, 126).to(torch.int32) + 127) << 23).view(torch.float32)   # (cap: split_product.h)
            t = torch.where((amax > 0) & (amax < 3.0e38), t, torch.ones_like(t))
            ws = w * t[:, None]                                        # exact: powers of two
            hi = ws.to(torch.float16)
            lo = (ws - hi.float()).to(torch.float16)
            hit = (key, hi.contiguous(), lo.contiguous(), None, (16.0 / t).contiguous())
            if w.is_cuda and torch.cuda.is_current_stream_capturing():
                return hit[1], hit[2], hit[3], hit[4]   # built inside a graph's memory pool: part of the graph, never a cached buffer
            if w.is_cuda:
                _publish_barrier(w.device)
            weight._tf_split_f16 = hit
        return hit[1], hit[2], hit[3], hit[4]
    hit = getattr(weight, "_tf_split", None)
    key = source_key(weight)
    if hit is None or hit[0] != key:
        w = weight.detach()
        hi = w.to(torch.bfloat16)
        r = w - hi.float()                      # exact in fp32
        mid = r.to(torch.bfloat16)
        lo = (r - mid.float()).to(torch.bfloat16).contiguous()
        hit = (key, hi.contiguous(), mid.contiguous(), lo)
        if w.is_cuda and torch.cuda.is_current_stream_capturing():
            return hit[1], hit[2], hit[3], None   # (as above: not cached)
        if w.is_cuda:
            _publish_barrier(w.device)
        weight._tf_split = hit
    return hit[1], hit[2], hit[3], None


def _rows_of(pieces, rows):
    """The row block `rows` = (a, b) of _split_weight's pieces (views: a row block is contiguous)."""
    return tuple(None if p is None else p[rows[0]:rows[1]] for p in pieces)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def linear(x, weight, bias=None, relu=False, rows=None, residual=None):
    """act(x @ weight^T + bias) through tf_linear_split_f32 for fp32 GPU tensors with K % 32 == 0; returns None when
    it does not apply (switched off, other dtype / device / shape): the caller keeps its PyTorch formulation.
    rows = (a, b): use output features a..b of `weight` only (a row block of a packed projection such as
    nn.MultiheadAttention.in_proj_weight); `bias` is then the matching slice.
    residual: fp32 [rows of x, N], added before the activation (tf_linear_split_res_f32)."""
    if not (_split_linear and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32
            and weight.dim() == 2 and weight.is_contiguous() and weight.device == x.device):
        return None
    N, K = weight.shape
    if rows is not None:
        if not (0 <= rows[0] < rows[1] <= N):
            return None
        N = rows[1] - rows[0]
    if x.shape[-1] != K or K % 32 or x.numel() == 0:
        return None
    if bias is not None and not (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N
                                 and bias.device == x.device):
        return None
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if residual is not None and not (residual.dtype == torch.float32 and residual.is_contiguous() and residual.device == x.device
                                     and residual.numel() == x2.shape[0] * N):
        return None
    if _use_packed(x2.shape[0], K, N) and not (x2.data_ptr() & 15) and (x2.shape[0] + 256) * N * 4 < 0xC0000000:
        packed = _packed_weight(weight, rows)
        if packed is not None:
            with torch.cuda.device(x.device):
                y = torch.empty((x2.shape[0], N), dtype=torch.float32, device=x.device)
                rc = _cabi.lib().tf_linear_packed_f32(x2.data_ptr(), packed.data_ptr(),
                                                      0 if bias is None else bias.data_ptr(), _ptr(residual), y.data_ptr(),
                                                      x2.shape[0], K, N, 1 if relu else 0, _terms(), _stream(x.device))
            _cabi.check(rc, "tf_linear_packed_f32")
            return y.view(*x.shape[:-1], N)
    pieces = _split_weight(weight)
    if rows is not None:
        pieces = _rows_of(pieces, rows)
    hi, mid, lo, wsc = pieces
    if (x2.data_ptr() | hi.data_ptr() | mid.data_ptr() | _ptr(lo)) & 15:
        return None
    with torch.cuda.device(x.device):
        y = torch.empty((x2.shape[0], N), dtype=torch.float32, device=x.device)
        if residual is None:
            rc = _cabi.lib().tf_linear_split_f32(x2.data_ptr(), hi.data_ptr(), mid.data_ptr(), _ptr(lo), _ptr(wsc),
                                                 0 if bias is None else bias.data_ptr(), y.data_ptr(), x2.shape[0], K, N,
                                                 1 if relu else 0, _stream(x.device))
        else:
            rc = _cabi.lib().tf_linear_split_res_f32(x2.data_ptr(), hi.data_ptr(), mid.data_ptr(), _ptr(lo), _ptr(wsc),
                                                     0 if bias is None else bias.data_ptr(), residual.data_ptr(),
                                                     y.data_ptr(), x2.shape[0], K, N, 1 if relu else 0, _stream(x.device))
    _cabi.check(rc, "tf_linear_split_f32")
    return y.view(*x.shape[:-1], N)


# DEFAULT since round 3 (TF_FFN_FUSED=0 / set_ffn_fused(False) switches it off): linear1 -> ReLU -> linear2 -> + residual -> LayerNorm of a transformer
# layer in ONE launch (tf_ffn_fused_f32, csrc/ffn_fused.hip): the d_ffn-wide intermediate (91 MB per encoder layer at
# 800 x 1333) never leaves the CU.  Same split products as linear(), bit-identical before the LayerNorm.  MI355X, 22 223 rows, d_ffn 1024: 72.3 us against
# 116.0 us for linear1 + ReLU, linear2, residual + LayerNorm (profiles/r03_optin_ffn_fused.txt).
_ffn_fused = os.environ.get("TF_FFN_FUSED", "1") != "0"
_FFN_FUSED_MIN_ROWS = int(os.environ.get("TF_FFN_FUSED_MIN_ROWS", "4096"))   # below: too few 96-row blocks to fill the CUs


def ffn_fused_enabled():
    return _ffn_fused


def set_ffn_fused(on):
    """Switch the one-launch feed-forward block on or off (process-wide); returns the previous setting."""
    global _ffn_fused
    prev, _ffn_fused = _ffn_fused, bool(on)
    return _switched(prev, _ffn_fused)


def ffn(x, linear1, linear2, norm=None, residual=None):
    """[norm](residual + linear2(relu(linear1(x)))) through tf_ffn_fused_f32 (reference: deformable_transformer.py:282-297
    forward_ffn + norm2).  x [..., 256 | 288] fp32 on the GPU; linear1 / linear2: nn.Linear; norm: nn.LayerNorm or None;
    residual: like x or None.  Returns None when the kernel does not apply (the caller keeps the separate kernels)."""
    if not (_ffn_fused and _split_linear and x.is_cuda and x.dtype == torch.float32):
        return None
    w1, w2 = linear1.weight, linear2.weight
    F_, D = w1.shape
    if D not in (256, 288) or x.shape[-1] != D or tuple(w2.shape) != (D, F_) or F_ % 16 or F_ < 128 or x.numel() == 0:
        return None
    if not all(w.dtype == torch.float32 and w.is_contiguous() and w.device == x.device for w in (w1, w2)):
        return None
    x2 = x.reshape(-1, D)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if M < _FFN_FUSED_MIN_ROWS or (M + 128) * D * 4 > 0xFFFFFFFF:
        return None
    vecs = [linear1.bias, linear2.bias]
    if norm is not None:
        if not (norm.elementwise_affine and tuple(norm.normalized_shape) == (D,)):
            return None
        vecs += [norm.weight, norm.bias]
    if not all(v is None or _param_ok(v, x) for v in vecs):
        return None
    if residual is not None:
        if residual.dtype != torch.float32 or residual.device != x.device or residual.numel() != x2.numel():
            return None
        residual = residual.reshape(-1, D)
        if not residual.is_contiguous():
            residual = residual.contiguous()
    if (x2.data_ptr() | (0 if residual is None else residual.data_ptr())) & 15:
        return None
    p1, p2 = _packed_weight(w1, None), _packed_weight(w2, None)
    if p1 is None or p2 is None:
        return None
    ptr = lambda t: 0 if t is None else t.data_ptr()
    with torch.cuda.device(x.device):
        y = torch.empty((M, D), dtype=torch.float32, device=x.device)
        rc = _cabi.lib().tf_ffn_fused_f32(x2.data_ptr(), p1.data_ptr(), ptr(linear1.bias), p2.data_ptr(), ptr(linear2.bias),
                                          ptr(residual), 0 if norm is None else norm.weight.data_ptr(),
                                          0 if norm is None else norm.bias.data_ptr(), 0.0 if norm is None else float(norm.eps),
                                          y.data_ptr(), M, D, F_, _terms(), _stream(x.device))
    _cabi.check(rc, "tf_ffn_fused_f32")
    return y.view(x.shape)


# DEFAULT since round 3 (TF_LINLN_FUSED=0 / set_linear_ln_fused(False) switches it off): a 256 -> 256 linear, the layer's residual add and its LayerNorm in
# ONE launch (tf_linear_res_ln_f32, csrc/ffn_fused.hip) -- the attention's output projection + norm1.  MI355X: 19.4-22.1 us
# against 34.5 us at 22 223 rows, 6.9 against 17.1 us at 400 rows (profiles/r03_optin_ffn_fused.txt).
_linln_fused = os.environ.get("TF_LINLN_FUSED", "1") != "0"
_LINLN_MIN_ROWS = int(os.environ.get("TF_LINLN_MIN_ROWS", "256"))


def linear_ln_fused_enabled():
    return _linln_fused


def set_linear_ln_fused(on):
    """Switch the one-launch projection + residual + LayerNorm on or off (process-wide); returns the previous setting."""
    global _linln_fused
    prev, _linln_fused = _linln_fused, bool(on)
    return _switched(prev, _linln_fused)


def linear_residual_norm(x, linear, residual, norm):
    """norm(residual + linear(x)) through tf_linear_res_ln_f32 for a 256 -> 256 or 288 -> 288 nn.Linear (reference:
    ms_deform_attn.py:87 output_proj + deformable_transformer.py:285-292).  Returns None when the kernel does not apply."""
    if not (_linln_fused and _split_linear and x.is_cuda and x.dtype == torch.float32):
        return None
    w = linear.weight
    D = w.shape[0]
    if D not in (256, 288) or tuple(w.shape) != (D, D) or x.shape[-1] != D or x.numel() == 0:
        return None
    if not (w.dtype == torch.float32 and w.is_contiguous() and w.device == x.device
            and norm.elementwise_affine and tuple(norm.normalized_shape) == (D,)):
        return None
    x2 = x.reshape(-1, D)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if M < _LINLN_MIN_ROWS or (M + 128) * D * 4 > 0xFFFFFFFF:
        return None
    if not all(v is None or _param_ok(v, x) for v in (linear.bias, norm.weight, norm.bias)):
        return None
    if residual.dtype != torch.float32 or residual.device != x.device or residual.numel() != x2.numel():
        return None
    residual = residual.reshape(-1, D)
    if not residual.is_contiguous():
        residual = residual.contiguous()
    if (x2.data_ptr() | residual.data_ptr()) & 15:
        return None
    packed = _packed_weight(w, None)
    if packed is None:
        return None
    with torch.cuda.device(x.device):
        y = torch.empty((M, D), dtype=torch.float32, device=x.device)
        rc = _cabi.lib().tf_linear_res_ln_f32(x2.data_ptr(), packed.data_ptr(), 0 if linear.bias is None else linear.bias.data_ptr(),
                                              residual.data_ptr(), norm.weight.data_ptr(), norm.bias.data_ptr(), float(norm.eps),
                                              y.data_ptr(), M, D, D, _terms(), _stream(x.device))
    _cabi.check(rc, "tf_linear_res_ln_f32")
    return y.view(x.shape)


# DEFAULT since round 3 (TF_STEM_POOL_FUSED=0 / set_stem_pool_fused(False) switches it off; stem 147.4 -> 66.4 us with the
# convolution below, profiles/r03_optin_conv_per_layer.txt): FrozenBN shift + ReLU + MaxPool2d(3, 2, 1) after the stem
# convolution in one pass (tf_bias_relu_maxpool_f32) instead of bias_act_ + F.max_pool2d; bit-identical.
_stem_pool_fused = os.environ.get("TF_STEM_POOL_FUSED", "1") != "0"


def stem_pool_fused_enabled():
    return _stem_pool_fused


def set_stem_pool_fused(on):
    global _stem_pool_fused
    prev, _stem_pool_fused = _stem_pool_fused, bool(on)
    return _switched(prev, _stem_pool_fused)


# DEFAULT since round 3 (TF_STEM_CONV_SPLIT=0 / set_stem_conv_split(False) switches it off): the 7 x 7 stem convolution as a split product on the matrix cores
# (tf_stem_conv7x7_f32, csrc/stem_conv.hip) instead of the library convolution.
_stem_conv_split = os.environ.get("TF_STEM_CONV_SPLIT", "1") != "0"


def stem_conv_split_enabled():
    return _stem_conv_split


def set_stem_conv_split(on):
    global _stem_conv_split
    prev, _stem_conv_split = _stem_conv_split, bool(on)
    return _switched(prev, _stem_conv_split)


def _stem_packed(weight):
    """Packed [64, 176] image (k = (c * 7 + ky) * 8 + kx, zero padded) of a [64, 3, 7, 7] weight, cached on the tensor under its
    source_key()."""
    hit = getattr(weight, "_tf_stem_packed", None)
    terms = _terms()
    key = (source_key(weight), terms)
    if hit is None or hit[0] != key:
        if torch.cuda.is_current_stream_capturing():
            return None
        w = weight.detach()
        w2 = torch.zeros((64, 176), dtype=torch.float32, device=w.device)
        w2[:, :168] = F.pad(w, (0, 1)).reshape(64, 168)
        nbytes = _cabi.lib().tf_linear_packed_bytes(176, 64, terms)
        with torch.cuda.device(w.device):
            packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
            rc = _cabi.lib().tf_linear_pack_weight_f32(w2.data_ptr(), packed.data_ptr(), 176, 64, terms, _stream(w.device))
        _cabi.check(rc, "tf_linear_pack_weight_f32")
        _publish_barrier(w.device)
        hit = (key, packed)
        weight._tf_stem_packed = hit
    return hit[1]


def stem_conv(x, weight, bias=None, relu=False):
    """conv2d(x, weight, stride 2, padding 3) (+ bias, ReLU) for x [N, 3, H, W] fp32 on the GPU and a [64, 3, 7, 7] weight
    (reference: torchvision resnet50.conv1 under models/backbone.py:93-104) -> channels_last [N, 64, Ho, Wo], or None."""
    if not (_stem_conv_split and _split_linear and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
            and tuple(weight.shape) == (64, 3, 7, 7) and weight.dtype == torch.float32 and weight.device == x.device
            and x.numel() > 0):
        return None
    if bias is not None and not (_param_ok(bias, x) and bias.numel() == 64):
        return None
    x = x if x.is_contiguous() else x.contiguous()
    n, _, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if n > 65535 or n * ho * wo * 256 >= 0xC0000000 or n * 3 * h * w >= 2 ** 31:
        return None
    packed = _stem_packed(weight)
    if packed is None:
        return None
    with torch.cuda.device(x.device):
        y = torch.empty((n, 64, ho, wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        rc = _cabi.lib().tf_stem_conv7x7_f32(x.data_ptr(), packed.data_ptr(), 0 if bias is None else bias.data_ptr(), y.data_ptr(),
                                             n, h, w, 1 if relu else 0, _terms(), _stream(x.device))
    _cabi.check(rc, "tf_stem_conv7x7_f32")
    return y


def bias_relu_maxpool(x, bias):
    """maxpool3x3/s2/p1(relu(x + bias[c])) of a channels_last [N, C, H, W] fp32 GPU tensor -> channels_last
    [N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1], or None when the kernel does not apply."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and x.numel() > 0 and x.shape[1] % 4 == 0 and _param_ok(bias, x) and bias.numel() == x.shape[1]
            and x.data_ptr() % 16 == 0):
        return None
    n, c, h, w = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty((n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device,
                          memory_format=torch.channels_last)
        rc = _cabi.lib().tf_bias_relu_maxpool_f32(x.data_ptr(), bias.data_ptr(), out.data_ptr(), n, h, w, c, _stream(x.device))
    _cabi.check(rc, "tf_bias_relu_maxpool_f32")
    return out


# DEFAULT since round 3 (TF_HEADS_SPLIT=0 / set_heads_split(False) switches it off; +2.9 % frames/s on its own,
# profiles/r03_optin_single_routes.txt): the small head GEMMs (box-regression MLPs, class heads: 400 rows) through
# the split-product kernels as well instead of hipBLASLt -- 24 launches per frame; the class logits then carry the split
# product's fp32-class error like everything else (parity and track ids: tests/test_full_size_gpu.py).
_heads_split = os.environ.get("TF_HEADS_SPLIT", "1") != "0"


def heads_split_enabled():
    return _heads_split


def set_heads_split(on):
    global _heads_split
    prev, _heads_split = _heads_split, bool(on)
    return _switched(prev, _heads_split)


def head_linear(module, x, relu=False):
    """act(module(x)) for a head's nn.Linear: the split product when the opt-in is on (inference on the GPU), else the module."""
    if _heads_split and not module.training and not torch.is_grad_enabled():
        y = linear(x, module.weight, module.bias, relu=relu)
        if y is not None:
            return y
    y = module(x)
    return F.relu(y) if relu else y


# DEFAULT since round 3 (TF_POS_ADD_FUSED=0 / set_pos_add_fused(False) switches it off): `with_pos_embed(x, pos)` in front of a projection is done inside the
# GEMM while the activation tile is staged (tf_linear_split_add_f32) instead of as its own pass over the tokens; bit-identical.
_pos_add_fused = os.environ.get("TF_POS_ADD_FUSED", "1") != "0"


def pos_add_fused_enabled():
    return _pos_add_fused


def set_pos_add_fused(on):
    global _pos_add_fused
    prev, _pos_add_fused = _pos_add_fused, bool(on)
    return _switched(prev, _pos_add_fused)


def linear_add(x, x2, weight, bias=None, rows=None):
    """(x + x2) @ weight^T + bias through tf_linear_split_add_f32 (same conditions and `rows` meaning as linear());
    returns None when it does not apply."""
    if not (_pos_add_fused and _split_linear and x.is_cuda and x.dtype == torch.float32 and x2.dtype == torch.float32
            and x2.shape == x.shape and x2.device == x.device and weight.dtype == torch.float32 and weight.dim() == 2
            and weight.is_contiguous() and weight.device == x.device):
        return None
    N, K = weight.shape
    if rows is not None:
        if not (0 <= rows[0] < rows[1] <= N):
            return None
        N = rows[1] - rows[0]
    if x.shape[-1] != K or K % 32 or x.numel() == 0:
        return None
    if bias is not None and not (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == N
                                 and bias.device == x.device):
        return None
    a, b = x.reshape(-1, K), x2.reshape(-1, K)
    a = a if a.is_contiguous() else a.contiguous()
    b = b if b.is_contiguous() else b.contiguous()
    pieces = _split_weight(weight)
    if rows is not None:
        pieces = _rows_of(pieces, rows)
    hi, mid, lo, wsc = pieces
    if (a.data_ptr() | b.data_ptr() | hi.data_ptr() | mid.data_ptr() | _ptr(lo)) & 15:
        return None
    with torch.cuda.device(x.device):
        y = torch.empty((a.shape[0], N), dtype=torch.float32, device=x.device)
        rc = _cabi.lib().tf_linear_split_add_f32(a.data_ptr(), b.data_ptr(), hi.data_ptr(), mid.data_ptr(), _ptr(lo), _ptr(wsc),
                                                 0 if bias is None else bias.data_ptr(), y.data_ptr(), a.shape[0], K, N,
                                                 _stream(x.device))
    _cabi.check(rc, "tf_linear_split_add_f32")
    return y.view(*x.shape[:-1], N)


# Several projections of the same rows in ONE launch (tf_linear_groups_f32, csrc/ffn_fused.hip): the token tile is fetched and split
# once per workgroup instead of once per launch and 128-column block.  Bit-identical to linear() / linear_add() per group.  Two
# callers, each with its own default (profiles/proj_groups_bench.json): the encoder layer's value + query
# projections ("enc") and the six decoder layers' cross-attention value projections of the encoder memory ("dec").
# TF_PROJ_GROUPS=0 / set_proj_groups(False) switches both off, TF_PROJ_GROUPS=1 both on, TF_PROJ_GROUPS=enc | dec one of them.
def _parse_proj_groups(v):
    v = str(v).strip().lower()
    if v in ("", "0", "off", "false"):
        return frozenset()
    if v in ("1", "on", "true", "all"):
        return frozenset(("enc", "dec"))
    routes = frozenset(t.strip() for t in v.split(",") if t.strip())
    if not routes <= {"enc", "dec"}:
        raise ValueError("TF_PROJ_GROUPS: 0, 1 or a comma-separated subset of enc,dec")
    return routes


_PROJ_GROUPS_DEFAULT = "enc,dec"
_proj_groups = _parse_proj_groups(os.environ.get("TF_PROJ_GROUPS", _PROJ_GROUPS_DEFAULT))
_PROJ_GROUPS_MIN_ROWS = int(os.environ.get("TF_PROJ_GROUPS_MIN_ROWS", "4096"))   # the other fused routes' threshold; only 22 223 rows were measured


def proj_groups_enabled(route=None):
    """Whether the grouped projection launch is on for `route` ("enc" / "dec"; None: for any)."""
    return bool(_proj_groups) if route is None else route in _proj_groups


def set_proj_groups(on):
    """Switch the grouped projection launches (process-wide): False / True for both callers, or "enc" / "dec" / "enc,dec" / an
    iterable of those names; returns the previous setting (a frozenset, accepted back)."""
    global _proj_groups
    if isinstance(on, (set, frozenset, list, tuple)):
        new = _parse_proj_groups(",".join(sorted(on)))
    elif isinstance(on, str):
        new = _parse_proj_groups(on)
    else:
        new = _parse_proj_groups("1" if on else "0")
    prev, _proj_groups = _proj_groups, new
    return _switched(prev, _proj_groups)


def set_proj_groups_min_rows(n):
    """Rows from which linear_groups() applies (process-wide); returns the previous value."""
    global _PROJ_GROUPS_MIN_ROWS
    prev, _PROJ_GROUPS_MIN_ROWS = _PROJ_GROUPS_MIN_ROWS, int(n)
    return _switched(prev, _PROJ_GROUPS_MIN_ROWS)


def linear_groups(x, x2, groups):
    """[(x + x2 if add else x) @ weight^T + bias for (weight, bias, add) in groups] through ONE tf_linear_groups_f32 launch; None when
    it does not apply (the caller keeps linear() / linear_add()).  x [..., 256] fp32 on the GPU, x2 like x (or None if no group
    adds); weights: persistent [N, 256] fp32 tensors (their packed images are _packed_weight's, cached on them), N % 32 == 0."""
    if not (_split_linear and x.is_cuda and x.dtype == torch.float32 and 1 <= len(groups) <= 8 and x.numel()):
        return None
    if _split_terms == 16 and (_n_six_term_routes or debug_checks_active()):
        return None   # per-layer six-term routes, the range audit and the finite check live on the per-layer wrappers
    K = x.shape[-1]
    if K != 256:
        return None
    any_add = any(add for _w, _b, add in groups)
    if any_add and (x2 is None or x2.dtype != torch.float32 or x2.shape != x.shape or x2.device != x.device):
        return None
    a = x.reshape(-1, K)
    a = a if a.is_contiguous() else a.contiguous()
    M = a.shape[0]
    if M < _PROJ_GROUPS_MIN_ROWS or (M + 128) * K * 4 > 0xFFFFFFFF:
        return None
    b = None
    if any_add:
        b = x2.reshape(-1, K)
        b = b if b.is_contiguous() else b.contiguous()
    if (a.data_ptr() | _ptr(b)) & 15:
        return None
    cols = 0
    for w, bias, _add in groups:
        if not (w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.device == x.device and w.shape[1] == K
                and w.shape[0] % 32 == 0 and (M + 128) * w.shape[0] * 4 <= 0xFFFFFFFF):
            return None
        if bias is not None and not (_param_ok(bias, x) and bias.numel() == w.shape[0]):
            return None
        cols += (w.shape[0] + 255) // 256 * 256
    if cols > 4096:
        return None
    packed = [_packed_weight(w, None) for w, _b, _add in groups]
    if any(p is None for p in packed):   # (capturing while an image is missing: this call takes the separate kernels)
        return None
    descs = (_cabi.ProjGroup * len(groups))()
    with torch.cuda.device(x.device):
        ys = [torch.empty((M, w.shape[0]), dtype=torch.float32, device=x.device) for w, _b, _add in groups]
        for d, (w, bias, add), p, y in zip(descs, groups, packed, ys):
            d.w_packed, d.bias, d.y, d.N, d.add_x2 = p.data_ptr(), (bias.data_ptr() if bias is not None else None), y.data_ptr(), w.shape[0], int(bool(add))
        rc = _cabi.lib().tf_linear_groups_f32(a.data_ptr(), _ptr(b) or None, descs, len(groups), M, K, _terms(), _stream(x.device))
    _cabi.check(rc, "tf_linear_groups_f32")
    return [y.view(*x.shape[:-1], y.shape[1]) for y in ys]


def conv3x3(x, w_taps, bias, relu, stride):
    """3 x 3 convolution (padding 1) -- or, with a [Cout, Cin] weight, a strided 1 x 1 convolution without padding -- of a
    channels_last fp32 GPU activation through tf_conv3x3_split_f32 / tf_conv1x1_strided_split_f32.
    x [N, Cin, H, W] (channels_last), w_taps [Cout, 9 * Cin] (the [Cout, 3, 3, Cin] storage of a channels_last weight, a
    persistent tensor: its bf16 pieces are cached on it), bias [Cout] or None.  Returns [N, Cout, Hout, Wout]
    (channels_last) or None when the kernel does not apply."""
    if not (_split_linear and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last) and w_taps.dtype == torch.float32
            and w_taps.dim() == 2 and w_taps.is_contiguous() and w_taps.device == x.device):
        return None
    n, cin, h, w = x.shape
    cout = w_taps.shape[0]
    ks = 3 if w_taps.shape[1] == 9 * cin else 1   # [Cout, Cin]: a strided 1 x 1 projection (no padding)
    if w_taps.shape[1] != ks * ks * cin or cin % 32 or stride not in (1, 2) or x.numel() == 0:
        return None
    if bias is not None and not (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout
                                 and bias.device == x.device):
        return None
    pad = 1 if ks == 3 else 0
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    # (the stream form takes Cin % 64; its halo form -- stride-1 3 x 3 -- Cin % 32: the mask head's 288- and 32-channel layers)
    cin_ok = cin % 64 == 0 or (ks == 3 and stride == 1 and _conv_halo and cin % 32 == 0)
    stream_route = (_conv_stream and _conv_stream_wins(n * ho * wo, cout) and cin_ok and not (x.data_ptr() & 15)
                    and n * h * w * cin * 4 < 0xC0000000 and (n * ho * wo + 256) * cout * 4 < 0xC0000000)
    halo = ks == 3 and stride == 1 and _conv_halo and stream_route   # (the halo form of the stream route: its own split policy)
    ksplit = _conv_ksplit(n * ho * wo, ks * ks * cin, cout, _HALO_KSPLIT_POLICY if halo else None)
    if ks == 1 and (ksplit < _CONV1X1_MIN_PIECES or not _conv1x1_splitk):
        ksplit = 1
    if stream_route:
        packed = _packed_weight(w_taps, None)
        if packed is not None:
            with torch.cuda.device(x.device):
                y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
                ws = torch.empty((ksplit, n * ho * wo * cout), dtype=torch.float32, device=x.device) if ksplit > 1 else None
                rc = _cabi.lib().tf_conv_packed_f32(x.data_ptr(), packed.data_ptr(), _ptr(bias), 0, y.data_ptr(), _ptr(ws), ksplit,
                                                    n, h, w, cin, cout, ks, stride, 1 if relu else 0, _terms(), _stream(x.device))
            _cabi.check(rc, "tf_conv_packed_f32")
            return y.permute(0, 3, 1, 2)   # NCHW shape over NHWC storage = channels_last
    # the block kernels address input, output and weight pieces through buffer resources: every byte offset below 3 GiB
    if (n * h * w * cin * 4 >= 0xC0000000 or (n * ho * wo + 256) * cout * 4 >= 0xC0000000 or cout * ks * ks * cin * 2 >= 0xC0000000):
        return None
    hi, mid, lo, wsc = _split_weight(w_taps)
    if (x.data_ptr() | hi.data_ptr() | mid.data_ptr() | _ptr(lo)) & 15:
        return None
    with torch.cuda.device(x.device):
        y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
        if ksplit > 1:   # few output pixels under a long K: split the K loop over workgroups (deterministic second pass)
            ws = torch.empty((ksplit, n * ho * wo * cout), dtype=torch.float32, device=x.device)
            fn = _cabi.lib().tf_conv3x3_splitk_f32 if ks == 3 else _cabi.lib().tf_conv1x1_splitk_f32
            rc = fn(x.data_ptr(), hi.data_ptr(), mid.data_ptr(), _ptr(lo), _ptr(wsc), 0 if bias is None else bias.data_ptr(), y.data_ptr(),
                    ws.data_ptr(), ksplit, n, h, w, cin, cout, stride, 1 if relu else 0, _stream(x.device))
        else:
            fn = _cabi.lib().tf_conv3x3_split_f32 if ks == 3 else _cabi.lib().tf_conv1x1_strided_split_f32
            rc = fn(x.data_ptr(), hi.data_ptr(), mid.data_ptr(), _ptr(lo), _ptr(wsc), 0 if bias is None else bias.data_ptr(), y.data_ptr(),
                    n, h, w, cin, cout, stride, 1 if relu else 0, _stream(x.device))
    _cabi.check(rc, "tf_conv3x3_split_f32")
    return y.permute(0, 3, 1, 2)   # NCHW shape over NHWC storage = channels_last


_conv_splitk = os.environ.get("TF_CONV_SPLITK", "1") not in ("", "0")

# Round 4 (TF_CONV_STREAM=0 / set_conv_stream(False): the LDS-staged block kernel of linear_split.hip): the convolutions through
# the stream GEMM (tf_conv_packed_f32, csrc/linear_stream.hip) -- weight fragments straight from L2, only the shifted input
# pixels through LDS.  Same products in the same order: bit-identical without split-K.
_conv_stream = os.environ.get("TF_CONV_STREAM", "1") not in ("", "0")
_CONV_STREAM_ALL = os.environ.get("TF_CONV_STREAM") == "all"   # A/B aid / tests: every shape through the stream form


def _conv_stream_wins(m, cout):
    """Where the stream form of the 3 x 3 / strided convolutions measured faster than the LDS-staged block kernel on MI355X
    (profiles/r04_conv_per_layer_stream_vs_block.txt, 800 x 1333 frame): many output pixels under at least 128 output channels
    -- layer2's 3 x 3 convolutions (six terms 47.5 vs 51.3 us, three terms 30.6 vs 34.9), its strided first one (45.9 vs 51.2 /
    31.4 vs 36.4).  Not the 64-channel layer1 (two column tiles only: 47.7 vs 43.6 us) and not the few-pixel layers whose K loop
    is cut into pieces (layer3 / layer4: 49.0 vs 46.9, 48.8 vs 48.6) -- there the two forms are within noise or the block kernel
    wins, and it stays."""
    # fp16 pieces: every shape (per frame 1321 us with the stream form everywhere against 1362 with the block kernels,
    # profiles/r04_f16_conv_per_layer.txt)
    return _CONV_STREAM_ALL or _terms() == 16 or (cout >= 128 and m >= 8192)


def set_conv_stream(on):
    """True: where it measured faster (the default); "all": every shape (tests, A/B); False: never.  Returns the previous setting."""
    global _conv_stream, _CONV_STREAM_ALL
    prev = "all" if (_conv_stream and _CONV_STREAM_ALL) else _conv_stream
    _conv_stream, _CONV_STREAM_ALL = bool(on), on == "all"
    return _switched(prev, "all" if (_conv_stream and _CONV_STREAM_ALL) else _conv_stream)



# Split-K policy of the 3 x 3 convolutions: (workgroups aimed at, launches with at least this many blocks are left alone,
# fewest K-slices a piece may have, fewest K-slices a layer must have).  Swept on the MI355X at the 800 x 1333 frame
# (profiles/r03_conv3_ksplit.txt; us of backbone convolutions per frame): 384,160,8,64 (rounds 2-3) 1473, 768,300,8,32 1396,
# 1024,300,6,32 1409, 1024,600,4,16 1418, 2048,600,4,16 1493.
_KSPLIT_POLICY = tuple(int(v) for v in os.environ.get("TF_CONV_KSPLIT_POLICY", "768,300,8,32").split(","))


def set_conv_ksplit_policy(target_blocks, leave_alone_blocks, min_slices_per_piece, min_slices):
    """-> the previous policy tuple."""
    global _KSPLIT_POLICY
    prev, _KSPLIT_POLICY = _KSPLIT_POLICY, (int(target_blocks), int(leave_alone_blocks), int(min_slices_per_piece), int(min_slices))
    return _switched(prev, _KSPLIT_POLICY)


def conv1x1_wants_split_k(m, cin, cout):
    """True when a stride-1 1 x 1 convolution over m pixels is better off in the convolution kernel with its K loop cut
    (tf_conv1x1_splitk_f32) than in the plain split GEMM: few workgroups, each walking a long K.  Default since round 3
    (TF_CONV1X1_SPLITK=0 / set_conv1x1_splitk(False) switches it off), measured at the 800 x 1333 frame
    (profiles/r03_conv1x1_splitk.txt): layer3.1-5.conv1 (1024 -> 256 at 50 x 84, 4 pieces) 30.2 -> 21.8 us, layer4.1-2.conv1
    (2048 -> 512 at 25 x 42, 8 pieces) 40.1 -> 23.9 us; two pieces did not pay (layer4.0.conv1 31.1 -> 32.5 us, the strided
    projection of layer4 33.6 -> 34.0 us): a 1 x 1 convolution is only cut into three pieces or more."""
    return _conv1x1_splitk and _conv_ksplit(m, cin, cout) >= _CONV1X1_MIN_PIECES


_conv1x1_splitk = os.environ.get("TF_CONV1X1_SPLITK", "1") not in ("", "0")
_CONV1X1_MIN_PIECES = 3


def set_conv1x1_splitk(on):
    global _conv1x1_splitk
    prev, _conv1x1_splitk = _conv1x1_splitk, bool(on)
    return _switched(prev, _conv1x1_splitk)


# The halo form of the stride-1 3 x 3 convolutions (csrc/linear_stream.hip conv3x3_halo_kernel, round 6; TF_CONV_HALO=0 /
# set_conv_halo(False): the stream form): a block stages the halo of its patch once per channel slice and runs all nine taps from it.
# Its blocks carry 18 x the matrix work per barrier of the stream form's, so it wants fewer, longer pieces: swept on the MI355X
# (profiles/r06_conv3_halo.txt).
_conv_halo = os.environ.get("TF_CONV_HALO", "1") not in ("", "0")
_HALO_KSPLIT_POLICY = tuple(int(v) for v in os.environ.get("TF_CONV_HALO_KSPLIT_POLICY", "512,300,9,32").split(","))


def set_conv_halo(on):
    """Switch the halo form of the stride-1 3 x 3 convolutions on or off (process-wide, also inside the library); returns the previous setting."""
    global _conv_halo
    prev, _conv_halo = _conv_halo, bool(on)
    _cabi.lib().tf_msda_set_option(b"conv_halo", 1 if on else 0)
    return _switched(prev, _conv_halo)


def _conv_ksplit(m, k, cout, policy=None):
    """Pieces the K loop (k = 9 Cin or Cin) of a split-product convolution is cut into: 1 unless the launch would leave most of the chip
    with one workgroup or none while every one of them walks a long K (at 800 x 1333: layer2's stride-1 layers 261
    workgroups of 36 K-slices -> 2 pieces, layer3 132 of 72 -> 5, layer4 68 of 144 -> 11, the extra pyramid level 10 of
    576 -> 64)."""
    if not _conv_splitk or cout % 4:
        return 1
    target, alone, per_piece, min_slices = policy or _KSPLIT_POLICY
    blocks = -(-m // 64) * -(-cout // (128 if cout >= 128 else 64))
    slices = k // 32
    if blocks >= alone or slices < min_slices:
        return 1
    return max(1, min(64, target // blocks, slices // per_piece))


# DEFAULT since round 3 (TF_INPUT_PROJ_FUSED=0 / set_input_proj_fused(False) switches it off; +4.3 % frames/s on its own,
# profiles/r03_optin_single_routes.txt): the reference's `input_proj`
# levels with a 1 x 1 convolution (models/deformable_detr.py:73-90: Conv2d(C, hidden, 1) -> GroupNorm(32, hidden)) as the
# split-product GEMM over the pixels + the library's own channels-innermost GroupNorm (tf_groupnorm_nhwc_f32), instead
# of a CK convolution, a layout copy and three ATen kernels per level.
_input_proj_fused = os.environ.get("TF_INPUT_PROJ_FUSED", "1") != "0"


def set_input_proj_fused(on):
    global _input_proj_fused
    prev, _input_proj_fused = _input_proj_fused, bool(on)
    return _switched(prev, _input_proj_fused)


def groupnorm_nhwc(x2, n_img, gn, relu=False):
    """GroupNorm [+ ReLU] of x2 [n_img * HW, C] (channels innermost) with nn.GroupNorm `gn`'s parameters; returns a new tensor of
    the same shape or None when the kernel does not apply."""
    if not (x2.is_cuda and x2.dtype == torch.float32 and x2.dim() == 2 and x2.is_contiguous()
            and gn.weight is not None and gn.bias is not None and _param_ok(gn.weight, x2) and _param_ok(gn.bias, x2)):
        return None
    rows, c = x2.shape
    if rows % n_img or c != gn.num_channels or c % 4 or c > 1024 or gn.num_groups > 256 or n_img > 65535 or (x2.data_ptr() & 15):
        return None
    hw = rows // n_img
    with torch.cuda.device(x2.device):
        out = torch.empty_like(x2)
        ws = torch.empty(2 * n_img * gn.num_groups, dtype=torch.float64, device=x2.device)
        fn = _cabi.lib().tf_groupnorm_relu_nhwc_f32 if relu else _cabi.lib().tf_groupnorm_nhwc_f32
        rc = fn(x2.data_ptr(), gn.weight.data_ptr(), gn.bias.data_ptr(), out.data_ptr(), ws.data_ptr(), n_img, hw, c, gn.num_groups,
                float(gn.eps), hw * c, hw * c, _stream(x2.device))
    _cabi.check(rc, "tf_groupnorm_nhwc_f32")
    return out


def mask_label_map(logits, order, pad_hw, img_hw, out_hw, threshold=0.5):
    """The tracker's mask post-processing in one launch (tf_mask_label_map_f32): logits [n, h, w] fp32 on the GPU (mask-head outputs),
    order: per track the row of `logits` that is its mask (-1: none) -> int16 [out_h, out_w], the owning track per pixel or -1 (also
    where any track's probability is NaN, as `stack -> max -> best > threshold`).  None when not applicable."""
    if not (_postprocess_fused and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
            and 0 < len(order) <= 32767 and logits.numel() > 0):
        return None
    n, h, w = logits.shape
    if any(r >= n for r in order) or img_hw[0] > pad_hw[0] or img_hw[1] > pad_hw[1]:
        return None
    with torch.cuda.device(logits.device):
        order_dev = torch.tensor(list(order), dtype=torch.int32).to(logits.device, non_blocking=True)
        label = torch.empty((int(out_hw[0]), int(out_hw[1])), dtype=torch.int16, device=logits.device)
        rc = _cabi.lib().tf_mask_label_map_f32(logits.data_ptr(), order_dev.data_ptr(), label.data_ptr(), len(order), h, w, int(pad_hw[0]),
                                               int(pad_hw[1]), int(img_hw[0]), int(img_hw[1]), int(out_hw[0]), int(out_hw[1]), float(threshold),
                                               _stream(logits.device))
    _cabi.check(rc, "tf_mask_label_map_f32")
    return label


def upsample_add(low, fpn, q_per_image):
    """The mask head's FPN merge (detr_segmentation._merge) in one pass: F.interpolate(low, size=fpn.shape[-2:], mode="nearest") +
    fpn broadcast over the queries of its image.  low [N, C, h, w], fpn [N / q_per_image, C, H, W], both channels_last -> [N, C, H, W]
    channels_last, bit-identical to the two ATen passes; None when not applicable."""
    if not (low.is_cuda and low.dtype == torch.float32 and fpn.dtype == torch.float32 and low.dim() == 4 and fpn.dim() == 4
            and fpn.device == low.device and low.shape[1] == fpn.shape[1] and low.shape[1] % 4 == 0 and q_per_image > 0
            and low.shape[0] == fpn.shape[0] * q_per_image and low.is_contiguous(memory_format=torch.channels_last)
            and fpn.is_contiguous(memory_format=torch.channels_last) and not ((low.data_ptr() | fpn.data_ptr()) & 15)):
        return None
    n, c, h, w = low.shape
    H, W = fpn.shape[-2:]
    if n * H * W * c >= 1 << 33:
        return None
    with torch.cuda.device(low.device):
        out = torch.empty((n, H, W, c), dtype=torch.float32, device=low.device)
        rc = _cabi.lib().tf_upsample_add_nhwc_f32(low.data_ptr(), fpn.data_ptr(), out.data_ptr(), n, q_per_image, h, w, H, W, c, _stream(low.device))
    _cabi.check(rc, "tf_upsample_add_nhwc_f32")
    return out.permute(0, 3, 1, 2)   # NCHW shape over NHWC storage = channels_last


def groupnorm_stats(x, gn):
    """The statistics pass of GroupNorm alone for a channels_last x [N, C, H, W]: 2 * N * groups doubles (sum | sum of squares per image
    and group) for a consumer that normalises in its own fetch (conv3x3_merged).  None when not applicable."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and gn.num_channels == x.shape[1] and x.shape[1] % 4 == 0 and x.shape[1] <= 1024 and gn.num_groups <= 256
            and x.shape[0] <= 65535 and not (x.data_ptr() & 15)):
        return None
    n, c, h, w = x.shape
    with torch.cuda.device(x.device):
        ws = torch.empty(2 * n * gn.num_groups, dtype=torch.float64, device=x.device)
        rc = _cabi.lib().tf_groupnorm_stats_nhwc_f32(x.data_ptr(), ws.data_ptr(), n, h * w, c, gn.num_groups, h * w * c, _stream(x.device))
    _cabi.check(rc, "tf_groupnorm_stats_nhwc_f32")
    return ws


def conv3x3_merged(low, fpn, q_per_image, w_taps, bias, gn=None, ws=None):
    """3 x 3 / padding 1 convolution over  act(low) up-sampled (nearest) to fpn's size + fpn broadcast over the q_per_image queries of
    its image  -- the mask head's FPN merge -- computed in the convolution's fetch (tf_conv3x3_merge_packed_f32): the merged tensor is
    never written.  act = relu(gn(low)) from `ws` (groupnorm_stats of low) when gn is given, else identity.  low [N, Cin, h, w], fpn
    [N / q_per_image, Cin, H, W] channels_last, w_taps [Cout, 9 * Cin] tap-major (a persistent tensor).  -> [N, Cout, H, W] channels_last,
    or None when not applicable."""
    if not (_split_linear and _conv_halo and low.is_cuda and low.dtype == torch.float32 and fpn.dtype == torch.float32 and low.dim() == 4
            and fpn.dim() == 4 and fpn.device == low.device and low.shape[1] == fpn.shape[1] and q_per_image > 0
            and low.shape[0] == fpn.shape[0] * q_per_image and low.is_contiguous(memory_format=torch.channels_last)
            and fpn.is_contiguous(memory_format=torch.channels_last) and w_taps.dtype == torch.float32 and w_taps.dim() == 2
            and w_taps.is_contiguous() and w_taps.device == low.device and not ((low.data_ptr() | fpn.data_ptr()) & 15)):
        return None
    n, cin, lh, lw = low.shape
    H, W = fpn.shape[-2:]
    cout = w_taps.shape[0]
    if w_taps.shape[1] != 9 * cin or cin % 32 or cin > 320 or (gn is not None and (ws is None or gn.num_channels != cin or gn.weight is None)):
        return None
    if bias is not None and not (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout and bias.device == low.device):
        return None
    if (n * H * W + 256) * cout * 4 >= 0xC0000000 or n * lh * lw * cin * 4 >= 0xC0000000 or fpn.numel() * 4 >= 0xC0000000:
        return None
    packed = _packed_weight(w_taps, None)
    if packed is None:
        return None
    with torch.cuda.device(low.device):
        y = torch.empty((n, H, W, cout), dtype=torch.float32, device=low.device)
        rc = _cabi.lib().tf_conv3x3_merge_packed_f32(
            low.data_ptr(), fpn.data_ptr(), 0 if gn is None else ws.data_ptr(), 0 if gn is None else gn.weight.data_ptr(),
            0 if gn is None else gn.bias.data_ptr(), 1 if gn is None else gn.num_groups, 0.0 if gn is None else float(gn.eps), packed.data_ptr(),
            _ptr(bias), y.data_ptr(), n, q_per_image, lh, lw, H, W, cin, cout, 0, _terms(), _stream(low.device))
    _cabi.check(rc, "tf_conv3x3_merge_packed_f32")
    return y.permute(0, 3, 1, 2)   # NCHW shape over NHWC storage = channels_last


def groupnorm_relu_conv3x3_c1(x, gn, conv):
    """conv(relu(gn(x))) for a 3 x 3 / padding 1 convolution to ONE channel (the mask head's out_lay behind gn5) of a channels_last
    x [N, C, H, W], C in {16, 32}: the normalised activation is never written.  -> [N, 1, H, W]; None when not applicable."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
            and x.shape[1] in (16, 32) and gn.num_channels == x.shape[1] and gn.weight is not None and gn.bias is not None
            and conv.out_channels == 1 and conv.in_channels == x.shape[1] and conv.kernel_size == (3, 3) and conv.stride == (1, 1)
            and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and x.shape[0] <= 65535
            and _param_ok(gn.weight, x) and _param_ok(gn.bias, x) and conv.weight.device == x.device
            and conv.weight.dtype == torch.float32 and (conv.bias is None or conv.bias.dtype == torch.float32)
            and not (x.data_ptr() & 15)):
        return None
    n, c, H, W = x.shape
    hit = getattr(conv, "_tf_c1_taps", None)   # [9, C] tap-major + the bias as a Python float (one synchronising read per change of the weight or the bias)
    srcs = (conv.weight, conv.bias)
    key = (source_key(conv.weight), source_key(conv.bias))
    if hit is None or hit[0] != key or not same_sources(hit[3], srcs):
        if torch.cuda.is_current_stream_capturing():
            return None
        hit = conv._tf_c1_taps = (key, conv.weight.detach()[0].permute(1, 2, 0).reshape(9, c).contiguous(),
                                  0.0 if conv.bias is None else float(conv.bias.detach()), srcs)
    with torch.cuda.device(x.device):
        out = torch.empty((n, 1, H, W), dtype=torch.float32, device=x.device)
        ws = torch.empty(2 * n * gn.num_groups, dtype=torch.float64, device=x.device)
        rc = _cabi.lib().tf_groupnorm_relu_conv3x3_c1_nhwc_f32(x.data_ptr(), gn.weight.data_ptr(), gn.bias.data_ptr(), hit[1].data_ptr(), hit[2],
                                                               out.data_ptr(), ws.data_ptr(), n, H, W, c, gn.num_groups, float(gn.eps),
                                                               _stream(x.device))
    _cabi.check(rc, "tf_groupnorm_relu_conv3x3_c1_nhwc_f32")
    return out


def _input_proj_taps(conv):
    """The persistent [Cout, 9 * Cin] tap-major image of the extra level's 3 x 3 weight: the split pieces are cached on it."""
    cout, cin = conv.out_channels, conv.in_channels
    hit = getattr(conv, "_tf_wtaps", None)
    key = source_key(conv.weight)
    if hit is None or hit[0] != key or hit[2] is not conv.weight:
        prev_img = None if hit is None else hit[1]
        hit = (key, conv.weight.detach().permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous(), conv.weight)
        inherit_route(hit[1], conv.weight, prev_img)
        conv._tf_wtaps = hit
    return hit[1]


def _input_proj_w2d(conv):
    """The persistent [Cout, Cin] view of a 1 x 1 level's weight: the split pieces are cached on it."""
    cout, cin = conv.out_channels, conv.in_channels
    hit = getattr(conv, "_tf_w2d", None)
    key = source_key(conv.weight)
    if hit is None or hit[0] != key or hit[2] is not conv.weight:
        prev_img = None if hit is None else hit[1]
        hit = (key, conv.weight.detach().reshape(cout, cin).contiguous(), conv.weight)
        inherit_route(hit[1], conv.weight, prev_img)
        if hit[1].is_cuda and hit[1].data_ptr() != conv.weight.data_ptr():   # a copy made on this stream: publish for the others
            _publish_barrier(hit[1].device)
        conv._tf_w2d = hit
    return hit[1]


def input_proj_1x1(x, conv, gn):
    """GroupNorm(conv(x)) for the input projections -- 1 x 1 convolutions, and the extra level's 3 x 3 / stride 2 one -- of a
    channels_last fp32 GPU activation x [N, Cin, H, W]; returns [N, Cout, H', W']
    (channels_last) or None when the fused route does not apply (the caller keeps the nn.Sequential)."""
    if not (_input_proj_fused and _split_linear and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and conv.groups == 1):
        return None
    if conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.dilation == (1, 1):
        # the extra pyramid level (deformable_detr.py:55-79: Conv2d(2048, hidden, 3, stride 2, padding 1) + GroupNorm)
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        cout = conv.out_channels
        y = conv3x3(x, _input_proj_taps(conv), conv.bias, False, 2)
        if y is None:
            return None
        n, _, ho, wo = y.shape
        z2 = groupnorm_nhwc(y.permute(0, 2, 3, 1).reshape(n * ho * wo, cout), n, gn)
        return None if z2 is None else z2.view(n, ho, wo, cout).permute(0, 3, 1, 2)
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)):
        return None
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    n, cin, h, w = x.shape
    cout = conv.out_channels
    w2d = _input_proj_w2d(conv)
    y2 = None
    if conv1x1_wants_split_k(n * h * w, cin, cout):   # the coarse levels: 1050 / 4200 pixels under K = 2048 / 1024
        y = conv3x3(x, w2d, conv.bias, False, 1)
        y2 = None if y is None else y.permute(0, 2, 3, 1)
    if y2 is None:
        y2 = linear(x.permute(0, 2, 3, 1).reshape(n * h * w, cin), w2d, conv.bias)
    if y2 is None:
        return None
    z2 = groupnorm_nhwc(y2.reshape(n * h * w, cout), n, gn)
    if z2 is None:
        return None
    return z2.view(n, h, w, cout).permute(0, 3, 1, 2)


# ALL input-projection levels of a frame normalised by ONE tf_groupnorm_levels_nhwc_f32 call (two launches) straight into the
# encoder's token buffer [N, S, C] (TF_INPUT_PROJ_LEVELS=0 / set_input_proj_levels(False): the per-level route above).  The coarse
# levels' GEMMs leave their split-K partial sums (tf_conv_packed_partials_f32) and the statistics pass adds them, so per frame the
# split-K reduce launches behind those levels, four x (zero, statistics, apply) and the concatenation in DeformableTransformer.encode
# are gone: 16 launches -> 2 at 800 x 1333, and no atomics (bitwise reproducible).  Measurements: profiles/gn_levels_bench.json.
# From 4096 rows on, as the other fused routes (only the full-size frame was measured).
_input_proj_levels = os.environ.get("TF_INPUT_PROJ_LEVELS", "1") != "0"
_INPUT_PROJ_LEVELS_MIN_ROWS = int(os.environ.get("TF_INPUT_PROJ_LEVELS_MIN_ROWS", "4096"))


def input_proj_levels_enabled():
    return _input_proj_levels


def set_input_proj_levels(on):
    """Switch the all-levels GroupNorm route of the input projections on or off (process-wide); returns the previous setting."""
    global _input_proj_levels
    prev, _input_proj_levels = _input_proj_levels, bool(on)
    return _switched(prev, _input_proj_levels)


def set_input_proj_levels_min_rows(n):
    """Rows (summed over images and levels) from which input_proj_levels() applies (process-wide); returns the previous value."""
    global _INPUT_PROJ_LEVELS_MIN_ROWS
    prev, _INPUT_PROJ_LEVELS_MIN_ROWS = _INPUT_PROJ_LEVELS_MIN_ROWS, int(n)
    return _switched(prev, _INPUT_PROJ_LEVELS_MIN_ROWS)


def _conv_partials(x, w_taps, bias, stride):
    """conv3x3()'s stream route (tf_conv_packed_f32) for a shape whose K loop is cut, with the second pass left to the consumer
    (tf_conv_packed_partials_f32) -> (partials [pieces', M * Cout] fp32, pieces the launch wrote); pieces == 1: the first M * Cout floats
    are the finished output, bias added.  None where conv3x3() would not take that route with a split: the caller keeps conv3x3()."""
    if not (_split_linear and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last) and w_taps.dtype == torch.float32
            and w_taps.dim() == 2 and w_taps.is_contiguous() and w_taps.device == x.device):
        return None
    n, cin, h, w = x.shape
    cout = w_taps.shape[0]
    ks = 3 if w_taps.shape[1] == 9 * cin else 1
    if w_taps.shape[1] != ks * ks * cin or cin % 64 or stride not in (1, 2) or x.numel() == 0 or (ks == 3 and stride == 1):
        return None   # (the stride-1 3 x 3 layers -- the halo form, its own split policy -- are no input projection)
    if bias is not None and not (_param_ok(bias, x) and bias.numel() == cout):
        return None
    pad = 1 if ks == 3 else 0
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    m = n * ho * wo
    if not (_conv_stream and _conv_stream_wins(m, cout) and not (x.data_ptr() & 15) and n * h * w * cin * 4 < 0xC0000000
            and (m + 256) * cout * 4 < 0xC0000000):
        return None
    ksplit = _conv_ksplit(m, ks * ks * cin, cout)
    if ksplit <= 1 or (ks == 1 and (ksplit < _CONV1X1_MIN_PIECES or not _conv1x1_splitk)):
        return None
    packed = _packed_weight(w_taps, None)
    if packed is None:
        return None
    pieces = ctypes.c_int(0)
    with torch.cuda.device(x.device):
        ws = torch.empty((ksplit, m * cout), dtype=torch.float32, device=x.device)
        rc = _cabi.lib().tf_conv_packed_partials_f32(x.data_ptr(), packed.data_ptr(), _ptr(bias), ws.data_ptr(), ksplit, n, h, w, cin, cout,
                                                     ks, stride, _terms(), ctypes.byref(pieces), _stream(x.device))
    _cabi.check(rc, "tf_conv_packed_partials_f32")
    return ws, pieces.value


def _groupnorm_levels(levels, n, total, c, groups, eps, device):
    """One tf_groupnorm_levels_nhwc_f32 call: levels [(src: y [n, HW, c] or partial sums [pieces', n * HW * c], pieces, bias or None, gn, HW)]
    normalised into consecutive rows of a fresh [n, total, c] buffer, which is returned (None: the entry would refuse the table)."""
    table = (_cabi.GnLevel * len(levels))()
    row0 = 0
    for d, (src, pieces, bias, gn, hw) in zip(table, levels):
        d.src, d.bias, d.gamma, d.beta = src.data_ptr(), _ptr(bias) or None, gn.weight.data_ptr(), gn.bias.data_ptr()
        d.pieces, d.HW, d.row0 = pieces, hw, row0
        row0 += hw
    L = _cabi.lib()
    n_ws = L.tf_groupnorm_levels_workspace_doubles(table, len(levels), n, c, groups)
    if n_ws <= 0:
        return None
    with torch.cuda.device(device):
        out = torch.empty((n, total, c), dtype=torch.float32, device=device)
        ws = torch.empty(n_ws, dtype=torch.float64, device=device)
        rc = L.tf_groupnorm_levels_nhwc_f32(table, len(levels), n, c, groups, eps, out.data_ptr(), total * c, ws.data_ptr(), _stream(device))
    _cabi.check(rc, "tf_groupnorm_levels_nhwc_f32")
    return out


def input_proj_levels(items):
    """GroupNorm(conv(x)) of ALL input-projection levels of a frame -- items: [(x [N, Cin, H, W], conv, gn)] in token order, the
    levels input_proj_1x1() takes -- through the level GEMMs (the coarse ones leaving their split-K partial sums) and ONE
    tf_groupnorm_levels_nhwc_f32 call into a fresh token buffer [N, S, C].  Returns the per-level [N, C, H', W'] views of that buffer
    (channels_last strides; consecutive: DeformableTransformer.encode uses the buffer itself), or None when it does not apply --
    switched off, gradients, fewer rows than the threshold, or any level the per-level route would decline: the caller keeps that route."""
    if not (_input_proj_levels and _input_proj_fused and _split_linear and 1 <= len(items) <= 8) or torch.is_grad_enabled():
        return None
    if _split_terms == 16 and (_n_six_term_routes or debug_checks_active()):
        return None   # per-layer six-term routes, the range audit and the finite check live on the per-layer wrappers
    x0, _conv0, gn0 = items[0]
    if not (x0.is_cuda and x0.dim() == 4):
        return None
    n, c, groups, eps = x0.shape[0], gn0.num_channels, gn0.num_groups, float(gn0.eps)
    if c % 4 or c > 1024 or groups > 256 or n > 65535:
        return None
    geom = []
    for x, conv, gn in items:
        if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.device == x0.device and x.shape[0] == n and x.numel()
                and conv.groups == 1 and conv.in_channels == x.shape[1] and conv.out_channels == c and conv.weight.device == x.device
                and conv.weight.dtype == torch.float32
                and gn.num_channels == c and gn.num_groups == groups and float(gn.eps) == eps and gn.weight is not None
                and gn.bias is not None and _param_ok(gn.weight, x) and _param_ok(gn.bias, x)):
            return None
        h, w = x.shape[-2:]
        if conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.dilation == (1, 1):
            geom.append((3, (h - 1) // 2 + 1, (w - 1) // 2 + 1))
        elif conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0):
            geom.append((1, h, w))
        else:
            return None
    total = sum(ho * wo for _ks, ho, wo in geom)
    if n * total < _INPUT_PROJ_LEVELS_MIN_ROWS:
        return None
    srcs = []   # (tensor that holds y or the partial sums, pieces, bias)
    for (x, conv, _gn), (ks, ho, wo) in zip(items, geom):
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        if ks == 3:
            wimg = _input_proj_taps(conv)
            part = _conv_partials(x, wimg, conv.bias, 2)
            if part is None:
                y = conv3x3(x, wimg, conv.bias, False, 2)
                part = None if y is None else (y.permute(0, 2, 3, 1), 1)
        else:
            wimg = _input_proj_w2d(conv)
            part = None
            if conv1x1_wants_split_k(n * ho * wo, x.shape[1], c):   # the coarse levels: 1050 / 4200 pixels under K = 2048 / 1024
                part = _conv_partials(x, wimg, conv.bias, 1)
                if part is None:
                    y = conv3x3(x, wimg, conv.bias, False, 1)
                    part = None if y is None else (y.permute(0, 2, 3, 1), 1)
            if part is None:
                y2 = linear(x.permute(0, 2, 3, 1).reshape(n * ho * wo, x.shape[1]), wimg, conv.bias)
                part = None if y2 is None else (y2, 1)
        if part is None or not part[0].is_contiguous() or (part[0].data_ptr() & 15):
            return None
        srcs.append((part[0], part[1], conv.bias if part[1] > 1 else None))
    out = _groupnorm_levels([(src, pieces, bias, gn, ho * wo) for (src, pieces, bias), (_x, _conv, gn), (_ks, ho, wo) in zip(srcs, items, geom)],
                            n, total, c, groups, eps, x0.device)
    if out is None:
        return None
    views, row0 = [], 0
    for _ks, ho, wo in geom:
        views.append(out[:, row0:row0 + ho * wo].view(n, ho, wo, c).permute(0, 3, 1, 2))   # NCHW shape over the level's rows = channels_last strides
        row0 += ho * wo
    return views


# DEFAULT since round 3 (TF_BOX_REFINE_FUSED=0 / set_box_refine_fused(False) switches it off; +5.1 % frames/s on its own):
# the decoder's iterative box refinement in one launch
# (tf_box_refine_f32) instead of ~12 element-wise ATen launches per layer on [queries, 4] tensors.
_box_refine_fused = os.environ.get("TF_BOX_REFINE_FUSED", "1") != "0"


def set_box_refine_fused(on):
    global _box_refine_fused
    prev, _box_refine_fused = _box_refine_fused, bool(on)
    return _switched(prev, _box_refine_fused)


def box_refine(delta, reference_points):
    """sigmoid(delta + inverse_sigmoid(reference_points)) (4-d references) / the 2-d variant of
    deformable_transformer.py:331-343; delta [..., 4], reference_points [..., 2 or 4].  None when not applicable."""
    if not (_box_refine_fused and delta.is_cuda and delta.dtype == torch.float32 and reference_points.dtype == torch.float32
            and delta.shape[-1] == 4 and reference_points.shape[-1] in (2, 4)
            and delta.shape[:-1] == reference_points.shape[:-1] and delta.is_contiguous()
            and reference_points.is_contiguous() and reference_points.device == delta.device and delta.numel() > 0):
        return None
    with torch.cuda.device(delta.device):
        out = torch.empty_like(delta)
        rc = _cabi.lib().tf_box_refine_f32(delta.data_ptr(), reference_points.data_ptr(), out.data_ptr(), delta.numel() // 4,
                                           reference_points.shape[-1], 1e-5, _stream(delta.device))
    _cabi.check(rc, "tf_box_refine_f32")
    return out


# DEFAULT since round 6 (TF_POSTPROCESS_FUSED=0 / set_postprocess_fused(False): the post-processor module + clip + cat, ~17
# element-wise ATen launches on [queries, 4] tensors outside the HIP graph, every frame): what the tracker's association reads
# -- scaled, clipped xyxy boxes, best score, label -- in ONE launch (tf_postprocess_pack_f32).
_postprocess_fused = os.environ.get("TF_POSTPROCESS_FUSED", "1") != "0"


def set_postprocess_fused(on):
    global _postprocess_fused
    prev, _postprocess_fused = _postprocess_fused, bool(on)
    return _switched(prev, _postprocess_fused)


def postprocess_pack(logits, boxes, img_h, img_w, clip):
    """[Q, 6] = (x0, y0, x1, y1, score, label) of DeformablePostProcess + clip_boxes_to_image for ONE image: logits [Q, C],
    boxes [Q, 4] cxcywh in [0, 1]; the arithmetic of the separate ATen kernels, operation by operation.  None when not applicable."""
    if not (_postprocess_fused and logits.is_cuda and logits.dtype == torch.float32 and boxes.dtype == torch.float32
            and logits.dim() == 2 and boxes.dim() == 2 and boxes.shape == (logits.shape[0], 4) and logits.shape[0] > 0
            and logits.shape[1] > 0 and logits.is_contiguous() and boxes.is_contiguous() and boxes.device == logits.device
            and boxes.data_ptr() % 16 == 0):
        return None
    with torch.cuda.device(logits.device):
        out = torch.empty((logits.shape[0], 6), dtype=torch.float32, device=logits.device)
        rc = _cabi.lib().tf_postprocess_pack_f32(logits.data_ptr(), boxes.data_ptr(), out.data_ptr(), logits.shape[0], logits.shape[1],
                                                 float(img_h), float(img_w), 1 if clip else 0, _stream(logits.device))
    _cabi.check(rc, "tf_postprocess_pack_f32")
    return out


def module_linear(module, x, inference):
    """module(x) for an nn.Linear: the split product on the GPU inference path when enabled, else the module (with gradients enabled and
    set_split_linear_training(True): the split product with its own backward, linear_train)."""
    if inference and _split_linear:
        y = linear(x, module.weight, module.bias)
        if y is not None:
            return y
    elif not inference and train_route(x):
        y = linear_train(x, module.weight, module.bias)
        if y is not None:
            return y
    return module(x)


# ---------------------------------------------------------------------------------------------------------
def mha_core(qk, v, num_heads, key_padding_mask=None):
    """softmax(q k^T / sqrt(d)) v for the decoder's query self-attention (include/tf_fused.h: tf_mha_core_f32).
    qk [N, L, 2E]: the shared q | k projection of one GEMM; v [N, L, E]; key_padding_mask [N, L] bool (True = ignore)
    or None.  Returns [N, L, E], or None when the kernel does not apply (the caller keeps torch's SDPA)."""
    if os.environ.get("TF_NO_MHA") == "1":   # debugging aid: keep torch's SDPA
        return None
    if not (qk.is_cuda and qk.dtype == torch.float32 and v.dtype == torch.float32 and v.device == qk.device
            and qk.dim() == 3 and v.dim() == 3 and qk.is_contiguous() and v.is_contiguous()):
        return None
    n, length, e2 = qk.shape
    e = e2 // 2
    if e2 != 2 * e or v.shape != (n, length, e) or e % num_heads:
        return None
    d = e // num_heads
    if d not in (16, 32, 36, 64) or e % 4 or length > 2300 or (qk.data_ptr() | v.data_ptr()) & 15 or (e * 4) % 16:
        return None
    mask_ptr = 0
    if key_padding_mask is not None:
        # bool / uint8 only (non-zero = ignore): a float mask is ADDITIVE for nn.MultiheadAttention (-inf = ignore, 0 = keep)
        if (key_padding_mask.shape != (n, length) or key_padding_mask.device != qk.device
                or key_padding_mask.dtype not in (torch.bool, torch.uint8)):
            return None
        key_padding_mask = key_padding_mask.to(torch.uint8).contiguous()
        mask_ptr = key_padding_mask.data_ptr()
    with torch.cuda.device(qk.device):
        out = torch.empty((n, length, e), dtype=torch.float32, device=qk.device)
        q_ptr = qk.data_ptr()
        rc = _cabi.lib().tf_mha_core_f32(q_ptr, q_ptr + e * 4, v.data_ptr(), out.data_ptr(), mask_ptr, n, length, length,
                                         num_heads, d, e2, e2, e, e, float(d) ** -0.5, _stream(qk.device))
    if rc == -2:   # TF_MSDA_ERR_BAD_DIMS: more keys than the score tile has LDS for -> the caller keeps torch's SDPA
        return None
    _cabi.check(rc, "tf_mha_core_f32")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# The fp16 split product's activation range (csrc/split_product.h): activations are scaled by 2^-4 into fp16, so |x| up to
# 65504 * 16 = 1.05e6 is representable; beyond it the hi piece is inf and the output row is NaN -- loudly: every ReLU epilogue
# propagates NaN (v < 0 ? 0 : v, as torch.relu does), none maps it to zero.  The reference's fp32 arithmetic has no such limit,
# so three tools make the contract explicit instead of silent:
#   * set_check_finite(True) / TF_SPLIT_CHECK_FINITE=1 -- debug mode: every split-product call checks its result and raises a
#     FloatingPointError naming the operation (one host synchronisation per call: not for timed runs);
#   * audit_activation_range() -- a context manager: run the model once under it on representative input; it records the
#     largest |activation| every split-product layer was given (and, for the fused feed-forward block, its hidden
#     activation) and, on exit, routes each layer that came within `safety` of the limit through the SIX-TERM bf16 product
#     (all 24 significand bits, fp32's exponent range) for the rest of the process; the report lists them;
#   * route_six_terms(weight) -- the same routing by hand.
# With no layer routed, no audit running and the check off the wrappers cost one comparison per call.
import contextlib
import functools

F16_ACTIVATION_LIMIT = 65504.0 * 16.0
_check_finite = os.environ.get("TF_SPLIT_CHECK_FINITE", "0") not in ("", "0")
_n_six_term_routes = 0        # weights marked `_tf_six_terms` (their layers run the six-term product while the default is the fp16 one)
_range_audit = None           # {(operation, ids of the weights): [weights, shapes, largest |activation|]} while audit_activation_range() runs
# _route_epoch (defined at the top of the module) is bumped whenever what a forward enqueues changes: a six-term route, the finite
# check, an audit, and every process-wide set_* switch of this module, of backbone and of detr_segmentation -- when, and only when,
# the switch changes VALUE (_switched).  GraphedDetector drops the HIP graphs it captured under another epoch (kernels are baked into
# a graph).  Its counterpart for the weights themselves is weight_epoch() / weights_changed().

# HIP graphs (graphed.GraphedDetector, the default path of bench.py and dist_utils.track_sequences): a replay calls none of the
# wrappers below, so (1) an audit or the finite check sees nothing inside a graph -- GraphedDetector therefore runs EAGERLY while
# either is active (debug_checks_active()), and a capture attempted with one of them on raises instead of synchronising inside
# the capture; (2) a route added after a graph was captured would not reach it -- route_epoch() is part of what a graph was
# captured under, a change drops the graphs and they are captured again with the routed kernels.  Run the audit BEFORE timing.


def route_epoch():
    return _route_epoch


def debug_checks_active():
    """An activation-range audit is running or the finite check is on: forwards must run eagerly (not from a captured graph)."""
    return _check_finite or _range_audit is not None


def set_check_finite(on):
    global _check_finite
    prev, _check_finite = _check_finite, bool(on)
    return _switched(prev, _check_finite)


def _routed(weight):
    return getattr(weight, "_tf_six_terms", False)


def route_six_terms(weight, on=True):
    """Route every split product of this weight tensor through the six-term bf16 product (while the default is the fp16 one).
    The mark lives ON THE TENSOR OBJECT (like the cached pieces: an address can be freed and handed to another weight) and is
    inherited by the images derived from it (inherit_route: a convolution's tap-major / 2-d image, re-created when the weight
    changes)."""
    global _n_six_term_routes, _route_epoch
    if bool(_routed(weight)) != bool(on):
        weight._tf_six_terms = bool(on)
        _n_six_term_routes += 1 if on else -1
        _route_epoch += 1


def inherit_route(new, *sources):
    """`new` is an image derived from `sources` (the parameter, the image it replaces): it runs six terms if one of them does."""
    if any(src is not None and _routed(src) for src in sources) and not _routed(new):
        route_six_terms(new)
    return new


def six_term_routes():
    return _n_six_term_routes


@contextlib.contextmanager
def audit_activation_range(route=True, safety=4.0):
    """-> report dict, filled on exit: {"limit", "largest", "layers": [(operation, weight shape, largest |activation|)...],
    "routed": n}.  Layers whose activations came within `safety` of the fp16 product's limit are routed to six terms.
    Forwards under the audit run eagerly (GraphedDetector steps aside); graphs captured before it are dropped if it routes."""
    global _range_audit, _route_epoch
    report = {"limit": F16_ACTIVATION_LIMIT, "safety": safety, "largest": 0.0, "layers": [], "routed": 0}
    prev, _range_audit = _range_audit, {}
    _route_epoch += 1
    try:
        yield report
    finally:
        seen, _range_audit = _range_audit, prev
        _route_epoch += 1
        for (name, _ids), (ws, shapes, amax) in sorted(seen.items(), key=lambda kv: -kv[1][2]):
            report["layers"].append((name, shapes, amax))
            report["largest"] = max(report["largest"], amax)
            if route and not (amax * safety < F16_ACTIVATION_LIMIT):   # also catches NaN / inf
                for w in ws:
                    route_six_terms(w)
                report["routed"] += 1


def _amax(t):
    return float(t.detach().abs().max()) if t is not None and t.numel() else 0.0


def _ranged(name, weights_of, acts_of):
    def deco(fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            if _split_terms != 16 or not (_n_six_term_routes or _check_finite or _range_audit is not None):
                return fn(*a, **k)
            ws = [w for w in weights_of(*a, **k) if w is not None]
            checks = _check_finite or _range_audit is not None
            if checks and ws and ws[0].is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("fused.%s: an activation-range audit / the finite check (set_check_finite, TF_SPLIT_CHECK_FINITE) "
                                   "reads results on the host and cannot run while a HIP graph is being captured -- run the model "
                                   "eagerly under them (GraphedDetector does so by itself), then capture" % name)
            route6 = any(_routed(w) for w in ws)
            if route6:
                _tls.terms = 6     # this thread's calls only: another tracker thread of the same model keeps its own arithmetic
            try:
                y = fn(*a, **k)
            finally:
                if route6:
                    _tls.terms = None
            if y is None:
                return y
            if _range_audit is not None:
                key = (name, tuple(id(w) for w in ws))
                rec = _range_audit.setdefault(key, [ws, tuple(tuple(w.shape) for w in ws), 0.0])   # (holds the weights: ids stay unique)
                rec[2] = max(rec[2], max(_amax(t) for t in acts_of(*a, **k)))
            if _check_finite and not bool(torch.isfinite(y).all()):
                raise FloatingPointError(
                    "%s produced a non-finite result (largest |input| %.3g; the fp16 split product represents activations up to "
                    "%.3g -- fused.audit_activation_range() routes such layers through the six-term product, "
                    "fused.set_split_terms(6) all of them)" % (name, max(_amax(t) for t in acts_of(*a, **k)), F16_ACTIVATION_LIMIT))
            return y
        return wrapped
    return deco


def _ffn_acts(x, linear1, linear2, norm=None, residual=None):
    hidden = F.relu(F.linear(x, linear1.weight, linear1.bias)) if _range_audit is not None else None   # audit only: the hidden activation
    return (x, hidden)


linear = _ranged("linear", lambda x, weight, *a, **k: (weight,), lambda x, *a, **k: (x,))(linear)
linear_add = _ranged("linear_add", lambda x, x2, weight, *a, **k: (weight,), lambda x, x2, *a, **k: (x + x2,))(linear_add)
ffn = _ranged("ffn", lambda x, linear1, linear2, *a, **k: (linear1.weight, linear2.weight), _ffn_acts)(ffn)
linear_residual_norm = _ranged("linear_residual_norm", lambda x, linear, *a, **k: (linear.weight,), lambda x, *a, **k: (x,))(linear_residual_norm)
stem_conv = _ranged("stem_conv", lambda x, weight, *a, **k: (weight,), lambda x, *a, **k: (x,))(stem_conv)
conv3x3 = _ranged("conv3x3", lambda x, w_taps, *a, **k: (w_taps,), lambda x, *a, **k: (x,))(conv3x3)


# ------------------------------------------------------------------------------------------------------------------------------
# THE TRAINING PATH OF THE LINEARS (opt-in; include/tf_fused.h: THE BACKWARD OF A LINEAR; csrc/linear_bwd.h).  With gradients
# enabled every nn.Linear of the encoder / decoder runs on the fp32 library, forward and backward.  set_split_linear_training(True) /
# TF_SPLIT_LINEAR_TRAIN=1 routes module_linear, the feed-forward block's first linear and the four projections of MSDeformAttn through
# linear_train instead: the forward is linear() (bit-identical to the inference path), the backward the library's own input-gradient,
# weight-gradient and bias-gradient kernels -- no float atomics, bit-identical from call to call.  NOT covered: convolutions,
# nn.MultiheadAttention's internals (the residual + LayerNorm sites have a switch of their own: set_layernorm_training below).  OFF by default: whether it is faster inside a training step is a measurement
# (tools/bench_linear_backward.py, profiles/linear_backward_bench.json), not a promise.
_split_linear_train = None    # None: follow TF_SPLIT_LINEAR_TRAIN (unset: off)
_train_counts = {"dgrad_own": 0, "dgrad_torch": 0, "wgrad_own": 0, "wgrad_torch": 0, "bias_own": 0, "bias_torch": 0}


def split_linear_training_enabled():
    if _split_linear_train is not None:
        return _split_linear_train
    return os.environ.get("TF_SPLIT_LINEAR_TRAIN", "0") not in ("", "0")


def set_split_linear_training(flag):
    """Switch the split-product training path of the linears on or off (process-wide; None: follow TF_SPLIT_LINEAR_TRAIN again);
    returns the previous setting."""
    global _split_linear_train
    prev = split_linear_training_enabled()
    _split_linear_train = None if flag is None else bool(flag)
    return _switched(prev, split_linear_training_enabled())


def train_route(x):
    """A call with gradients enabled that linear_train takes: the switch is on and x is an fp32 tensor on the device."""
    return split_linear_training_enabled() and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32


def train_route_counts(reset=False):
    """How many input / weight / bias gradients of linear_train went to the library's own kernels and how many to torch."""
    return _read_counts(_train_counts, reset)


def _read_counts(counts, reset):
    """A copy of one of the training sections' counters; reset: the counters start again at 0."""
    out = dict(counts)
    if reset:
        for k in counts:
            counts[k] = 0
    return out


def _aligned(t):
    """t where the kernels can read it as it is (contiguous, 16-byte aligned), else a contiguous copy."""
    return t if t.is_contiguous() and not t.data_ptr() & 15 else t.clone(memory_format=torch.contiguous_format)


def _route_terms(weight):
    """The terms a backward runs with: those of the forward (a layer routed to six terms while the default is the fp16 product)."""
    return 6 if (_split_terms == 16 and _routed(weight)) else _split_terms


class _NotApplicable(Exception):
    pass


def _packed_image(t, attr, rows, cols, terms, source):
    """Fragment-order image (tf_linear_pack_weight_f32) of the contiguous [rows, cols] tensor source() derives from t, cached on t as
    `attr` under its source_key(), per `terms`; None when it cannot be built (shape; stream capture without a cached image).  The
    images of the training path only: no publish barrier, the stream that built an image is remembered instead.
    rows and cols may be LISTS (source() then returns as many tensors): the images one behind the other in one buffer."""
    many = isinstance(rows, (list, tuple))
    shapes = list(zip(rows, cols)) if many else [(rows, cols)]
    cache = getattr(t, attr, None)
    key = source_key(t)
    if cache is None or cache[0] != key:
        cache = (key, {})
        setattr(t, attr, cache)
    capturing = torch.cuda.is_current_stream_capturing()
    hit = cache[1].get(terms)
    if hit is None:
        if capturing:
            return None   # never build a cached buffer inside a graph's memory pool
        sizes = [_cabi.lib().tf_linear_packed_bytes(r, c, terms) for r, c in shapes]
        if min(sizes) <= 0:
            return None
        with torch.cuda.device(t.device):
            srcs = source() if many else [source()]
            buf = torch.empty(sum(sizes), dtype=torch.uint8, device=t.device)
            at = buf.data_ptr()
            for src, (r, c), nbytes in zip(srcs, shapes, sizes):
                rc = _cabi.lib().tf_linear_pack_weight_f32(src.data_ptr(), at, r, c, terms, _stream(t.device))
                _cabi.check(rc, "tf_linear_pack_weight_f32")
                at += nbytes
        hit = (buf, torch.cuda.current_stream(t.device))
        cache[1][terms] = hit
    elif not capturing and hit[1] != torch.cuda.current_stream(t.device):
        # built on another stream (a training step rebuilds it for the stream that runs the backward: no host synchronisation)
        torch.cuda.current_stream(t.device).wait_stream(hit[1])
    return hit[0]


def _packed_weight_t(weight, terms):
    """Fragment-order image of weight^T (the `weight` of the input gradient dx = dy . w), cached on the parameter under its
    source_key() like _packed_weight; None when it cannot be built (shape; stream capture without a cached image)."""
    N, K = weight.shape
    return _packed_image(weight, "_tf_packed_t", N, K, terms, lambda: weight.detach().t().contiguous())


def _grad_stats(a, role, terms, colsum):
    """tf_linear_grad_stats_f32 of a [M, C] -> (scale2: {s, 1 / s} for role 0, t[C] | 1 / t[C] for role 1; colsum [C] or None), on the
    device."""
    L = _cabi.lib()
    M, C = a.shape
    nbytes = L.tf_linear_grad_stats_workspace_bytes(M, C, role, 1 if colsum else 0)
    if nbytes < 0:
        _cabi.check(-2, "tf_linear_grad_stats_f32")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=a.device)
    scale2 = torch.empty(2 if role == 0 else 2 * C, dtype=torch.float32, device=a.device)
    cs = torch.empty(C, dtype=torch.float32, device=a.device) if colsum else None
    rc = L.tf_linear_grad_stats_f32(a.data_ptr(), scale2.data_ptr(), _ptr(cs), ws.data_ptr(), int(nbytes), M, C, role, terms,
                                    _stream(a.device))
    _cabi.check(rc, "tf_linear_grad_stats_f32")
    return scale2, cs


class _LinearTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        with one_stream():   # a training step: the weight images are rebuilt every step for the stream that uses them next
            y = linear(x, weight, bias, relu=relu)
        if y is None:
            # linear() declined.  For a SHAPE reason (K % 32) on tensors it would otherwise take, the forward is torch's and the backward
            # below still runs (own kernels where they take the shape, torch where not); any other reason: not this function's call
            if not (_split_linear and x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and weight.dim() == 2
                    and weight.device == x.device and x.shape[-1] == weight.shape[1] and x.numel() > 0
                    and (bias is None or (bias.dtype == torch.float32 and bias.device == x.device))):
                raise _NotApplicable()
            y = F.linear(x, weight, bias)
            if relu:
                y = torch.relu(y)
        drop = getattr(ctx, "drop", None)   # (_LinearDropoutTrain: (p, rng), dropout on the fresh ReLU output, in place)
        if drop is not None:
            if not (relu and y.is_contiguous() and y.numel() % 4 == 0 and y.data_ptr() % 16 == 0):
                raise _NotApplicable()
            with torch.cuda.device(y.device):
                rc = _cabi.lib().tf_dropout_inplace_f32(y.data_ptr(), drop[1].data_ptr(), drop[0], y.numel(), _stream(y.device))
            _cabi.check(rc, "tf_dropout_inplace_f32")
        ctx.relu = relu
        ctx.terms = _route_terms(weight)
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        N, K = weight.shape
        terms = ctx.terms
        dy2 = dy.reshape(-1, N)
        drop = getattr(ctx, "drop", None)
        if ctx.relu and drop is not None:
            # y is the dropped-and-scaled activation: positive exactly where the unit was active and kept (scale >= 1)
            dy2 = _aligned(dy2)
            with torch.cuda.device(dy2.device):
                masked = torch.empty_like(dy2)
                rc = _cabi.lib().tf_relu_dropout_bwd_f32(dy2.data_ptr(), y.data_ptr(), drop[0], masked.data_ptr(), dy2.numel(),
                                                         _stream(dy2.device))
            _cabi.check(rc, "tf_relu_dropout_bwd_f32")
            dy2 = masked
        elif ctx.relu:
            dy2 = torch.ops.aten.threshold_backward(dy2, y.reshape(-1, N), 0.0)
        x2 = x.reshape(-1, K)
        dy2, x2 = _aligned(dy2), _aligned(x2)
        M = dy2.shape[0]
        L = _cabi.lib()
        own = K % 4 == 0 and N % 4 == 0 and max(M * N, M * K, N * K) * 4 < 0xC0000000 and dy2.dtype == torch.float32
        dx = dw = db = None
        with torch.cuda.device(dy2.device), one_stream():
            stream = _stream(dy2.device)
            s_dy = s_x = None
            if own and (need_x or need_w or need_b):
                s_dy, db = _grad_stats(dy2, 0, terms, need_b)
            if need_b:
                _train_counts["bias_own" if db is not None else "bias_torch"] += 1
                if db is None:
                    db = dy2.sum(0)
            if need_x:
                packed_t = _packed_weight_t(weight, terms) if own and N % 64 == 0 and (M + 256) * K * 4 < 0xC0000000 else None
                if packed_t is not None:
                    dx = torch.empty((M, K), dtype=torch.float32, device=dy2.device)
                    ks = getattr(ctx, "dgrad_ksplit", 1)   # (_Conv1x1Train: the contraction over N cut into pieces; the linears: one)
                    if ks > 1:
                        wsx = torch.empty((ks, M * K), dtype=torch.float32, device=dy2.device)
                        rc = L.tf_linear_dgrad_splitk_packed_f32(dy2.data_ptr(), s_dy.data_ptr(), packed_t.data_ptr(), dx.data_ptr(),
                                                                 wsx.data_ptr(), ks, M, K, N, terms, stream)
                    else:
                        rc = L.tf_linear_dgrad_packed_f32(dy2.data_ptr(), s_dy.data_ptr(), packed_t.data_ptr(), dx.data_ptr(), M, K, N, terms, stream)
                    _cabi.check(rc, "tf_linear_dgrad_packed_f32")
                    _train_counts["dgrad_own"] += 1
                else:
                    dx = dy2 @ weight.detach()
                    _train_counts["dgrad_torch"] += 1
                dx = dx.view(x.shape)
            if need_w:
                if own:
                    s_x, _ = _grad_stats(x2, 1, terms, False)
                    nbytes = int(L.tf_linear_wgrad_workspace_bytes(M, K, N))
                    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dy2.device)
                    dw = torch.empty((N, K), dtype=torch.float32, device=dy2.device)
                    rc = L.tf_linear_wgrad_split_f32(dy2.data_ptr(), x2.data_ptr(), s_dy.data_ptr(), s_x.data_ptr(), dw.data_ptr(),
                                                     ws.data_ptr(), nbytes, M, K, N, terms, stream)
                    _cabi.check(rc, "tf_linear_wgrad_split_f32")
                    _train_counts["wgrad_own"] += 1
                else:
                    dw = dy2.t() @ x2
                    _train_counts["wgrad_torch"] += 1
        return dx, dw, db, None


class _LinearDropoutTrain(torch.autograd.Function):
    """dropout(relu(x @ weight^T + bias)): _LinearTrain with tf_dropout_inplace_f32 behind its forward and tf_relu_dropout_bwd_f32 in place
    of the ReLU's threshold_backward.  Saves what _LinearTrain saves (x, weight and the one activation tensor)."""
    @staticmethod
    def forward(ctx, x, weight, bias, p, rng):
        ctx.drop = (p, rng)
        return _LinearTrain.forward(ctx, x, weight, bias, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        dx, dw, db, _ = _LinearTrain.backward(ctx, dy)
        return dx, dw, db, None, None


def linear_train(x, weight, bias=None, relu=False, dropout=None):
    """act(x @ weight^T + bias) with the library's own backward: the forward IS linear() (bit-identical to the inference path; None
    where linear() declines the tensors -- host tensors, another dtype, split linears switched off: the caller keeps module(x); a
    shape linear() does not take, K % 32 != 0, is computed by torch inside so that the function never fails for a shape reason), the
    backward runs tf_linear_grad_stats_f32 on dy (with the bias
    gradient) and on x, tf_linear_dgrad_packed_f32 and tf_linear_wgrad_split_f32 (include/tf_fused.h).  A gradient whose kernel does
    not take the shape (K or N not a multiple of 4; the input gradient: N not a multiple of 64) is computed by torch inside the
    backward: train_route_counts() tells which path ran.
    dropout (an nn.Dropout in training mode with 0 < p < 1, relu=True only): dropout(relu(.)) with the mask of the library's counter-based
    generator (include/tf_fused.h: DROPOUT INSIDE THE TRAINING KERNELS); the caller has checked set_dropout_training()."""
    try:
        if dropout is not None:
            if not (relu and x.is_cuda and weight.shape[0] % 4 == 0 and _dropout_active(dropout)):
                return None
            return _LinearDropoutTrain.apply(x, weight, bias, float(dropout.p), dropout_rng(x.device))
        return _LinearTrain.apply(x, weight, bias, relu)
    except _NotApplicable:
        return None


# ------------------------------------------------------------------------------------------------------------------------------
# THE TRAINING PATH OF THE RESIDUAL + LAYERNORM SITES (opt-in; include/tf_fused.h: THE BACKWARD OF THE RESIDUAL LAYERNORM;
# csrc/layernorm_bwd.h).  With gradients enabled every residual_norm() site is norm(x + res): an ATen add that writes the sum, the
# library's LayerNorm forward, its backward and its two-kernel gamma / beta reduction.  set_layernorm_training(True) /
# TF_LAYERNORM_TRAIN=1 routes these sites through layernorm_train instead: the forward is the inference kernel (bit-identical to
# add_layernorm) plus the rows' (mean, rstd), the backward one pass over the rows and a small column reduction -- no atomics,
# bit-identical from call to call.  Dropout sits before the add and stays a torch op (unless set_dropout_training, below, takes the site), so the route holds under dropout 0.1.  NOT
# covered: GroupNorm, the LayerNorm epilogues of the fused inference kernels (linear_residual_norm, ffn), nn.MultiheadAttention's
# internals.  OFF by default: whether it is faster inside a training step is a measurement (tools/bench_layernorm_train.py,
# profiles/layernorm_train_bench.json), not a promise.
_layernorm_train = None    # None: follow TF_LAYERNORM_TRAIN (unset: off)
_layernorm_train_counts = {"own": 0, "torch": 0}


def layernorm_training_enabled():
    if _layernorm_train is not None:
        return _layernorm_train
    return os.environ.get("TF_LAYERNORM_TRAIN", "0") not in ("", "0")


def set_layernorm_training(flag):
    """Switch the training path of the residual + LayerNorm sites on or off (process-wide; None: follow TF_LAYERNORM_TRAIN again);
    returns the previous setting."""
    global _layernorm_train
    prev = layernorm_training_enabled()
    _layernorm_train = None if flag is None else bool(flag)
    return _switched(prev, layernorm_training_enabled())


def layernorm_train_route(x):
    """A call with gradients enabled that layernorm_train takes: the switch is on and x is an fp32 tensor on the device."""
    return layernorm_training_enabled() and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32


def layernorm_train_counts(reset=False):
    """How many layernorm_train calls ran the library's own kernels ("own") and how many were declined ("torch": the caller kept
    norm(x + res))."""
    return _read_counts(_layernorm_train_counts, reset)


def _layernorm_train_forward(ctx, x, res, weight, bias, eps, drop=None):
    """The forward of both LayerNorm Functions.  drop: None | (p, rng), the residual dropped inside the kernel (res is a tensor then)."""
    C = x.shape[-1]
    rows = x.numel() // C
    L = _cabi.lib()
    with torch.cuda.device(x.device):
        out = torch.empty_like(x)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        tail = (out.data_ptr(), stats.data_ptr(), rows, C, float(eps), _stream(x.device))
        if drop is None:
            name = "tf_add_layernorm_train_f32"
            rc = L.tf_add_layernorm_train_f32(x.data_ptr(), _ptr(res), weight.data_ptr(), bias.data_ptr(), *tail)
        else:
            name = "tf_add_dropout_layernorm_train_f32"
            rc = L.tf_add_dropout_layernorm_train_f32(x.data_ptr(), res.data_ptr(), weight.data_ptr(), bias.data_ptr(), drop[1].data_ptr(),
                                                      drop[0], *tail)
    _cabi.check(rc, name)
    # what torch keeps for this chain, and (seed, offset) under dropout: no sum, no normalised activation, no mask, no dropped tensor
    if drop is None:
        ctx.save_for_backward(x, res, weight, stats)
    else:
        ctx.p = drop[0]
        ctx.save_for_backward(x, res, weight, stats, drop[1])
    return out


def _layernorm_train_backward(ctx, dy):
    """The backward of both: the gradients of (x, res, weight, bias).  Without dropout ONE tensor is the gradient of x and of res; with
    it dres = keep scale dx is a tensor of its own.  Nothing is launched when nothing is needed."""
    x, res, weight, stats, *rng = ctx.saved_tensors
    need_x, need_res, need_w, need_b = ctx.needs_input_grad[:4]
    C = x.shape[-1]
    rows = x.numel() // C
    dy = _aligned(dy)
    L = _cabi.lib()
    name = "tf_add_dropout_layernorm_bwd_f32" if rng else "tf_add_layernorm_bwd_f32"
    dx = dres = dw = db = ws = None
    nbytes = 0
    with torch.cuda.device(x.device):
        if need_x or (need_res and not rng):
            dx = torch.empty_like(x)
        if need_res and rng:
            dres = torch.empty_like(x)
        if need_w:
            dw = torch.empty_like(weight)
        if need_b:
            db = torch.empty_like(weight)
        if need_w or need_b:
            nbytes = int(L.tf_add_layernorm_bwd_workspace_bytes(rows, C))
            if nbytes < 0:
                _cabi.check(-2, name)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        if dx is not None or dres is not None or ws is not None:
            head = (dy.data_ptr(), x.data_ptr(), _ptr(res), weight.data_ptr(), stats.data_ptr())
            tail = (_ptr(dw), _ptr(db), _ptr(ws), nbytes, rows, C, _stream(x.device))
            if rng:
                rc = L.tf_add_dropout_layernorm_bwd_f32(*head, rng[0].data_ptr(), ctx.p, _ptr(dx), _ptr(dres), *tail)
            else:
                rc = L.tf_add_layernorm_bwd_f32(*head, _ptr(dx), *tail)
            _cabi.check(rc, name)
    if not rng:
        dres = dx
    return (dx if need_x else None), (dres if need_res else None), dw, db


class _LayerNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        return _layernorm_train_forward(ctx, x, res, weight, bias, eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return _layernorm_train_backward(ctx, dy) + (None,)


def layernorm_train(x, res, norm):
    """norm(x + res) (res may be None) with the library's own backward: the forward IS the inference kernel (bit-identical to
    add_layernorm) and saves x, res, norm.weight and the rows' (mean, rstd); the backward is tf_add_layernorm_bwd_f32
    (include/tf_fused.h) and returns ONE tensor as the gradient of both x and res.  None -- the caller keeps norm(x + res) -- for
    anything the kernels do not take: not fp32, not on the device, a non-contiguous x, C % 4 != 0 or C > 4096, no affine parameters,
    misaligned pointers, a res of another shape / dtype / device.  A non-contiguous res of the right shape (the decoder's transposed
    self-attention output) is copied first, as add_layernorm does on the inference path; the copy is a torch op and differentiable.
    layernorm_train_counts() tells which way the calls went."""
    ok, res = _layernorm_train_gates(x, res, norm)
    if not ok:
        _layernorm_train_counts["torch"] += 1
        return None
    _layernorm_train_counts["own"] += 1
    return _LayerNormTrain.apply(x, res, norm.weight, norm.bias, norm.eps)


def _layernorm_train_gates(x, res, norm):
    """(what the LayerNorm training kernels take, res made contiguous)."""
    ok = (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0 and x.data_ptr() % 16 == 0
          and norm.elementwise_affine and norm.bias is not None and len(norm.normalized_shape) == 1)
    if ok:
        C = norm.normalized_shape[0]
        ok = x.shape[-1] == C and C % 4 == 0 and C <= 4096 and _param_ok(norm.weight, x) and _param_ok(norm.bias, x)
    if ok and res is not None:
        ok = res.shape == x.shape and res.dtype == x.dtype and res.device == x.device
        if ok and not res.is_contiguous():
            res = res.contiguous()   # as add_layernorm: the decoder's self-attention output arrives transposed (a differentiable copy)
        ok = ok and res.data_ptr() % 16 == 0
    return ok, res


# ------------------------------------------------------------------------------------------------------------------------------
# DROPOUT INSIDE THE TRAINING KERNELS (opt-in; include/tf_fused.h: DROPOUT INSIDE THE TRAINING KERNELS; csrc/dropout_rng.h,
# csrc/dropout_train.h).  The reference trains with dropout 0.1: every residual_norm() site is norm(x + dropout(res)) and every
# feed-forward block dropout(relu(linear1(x))), each an ATen dropout that writes a dropped copy and a byte mask and keeps both for the
# backward.  set_dropout_training(True) / TF_DROPOUT_TRAIN=1 lets the library's kernels decide the mask themselves, from a counter-based
# generator (Philox4x32-10 on (seed, offset, element index)), forward and backward: no mask and no dropped tensor exist.  It rides on
# the parent routes: a residual site needs set_layernorm_training (layernorm_train_route), a feed-forward site
# set_split_linear_training (train_route); a site whose parent route is off, or whose tensors the kernels do not take, runs today's
# lines (counted *_torch).  (seed, offset) are drawn per site on the device with torch's generator (dropout_rng): torch.manual_seed
# governs them and a captured graph advances them as it advances torch's own dropout.  "reference" / TF_DROPOUT_TRAIN=reference draws
# at the same sites in the same order but computes with torch ops and the mask of tf_dropout_keep_u8, in any floating dtype: the oracle
# of the layer-level test and a debugging aid.  NOT covered: plain DETR's transformer.py, the dropout inside nn.MultiheadAttention, the
# fused inference epilogues, host tensors, a forward without gradients (the tracking model's previous-frame pass).  OFF by default: whether it is faster inside a training step is a measurement
# (tools/bench_dropout_train.py, profiles/dropout_train_bench.json), not a promise.
_dropout_train = None    # None: follow TF_DROPOUT_TRAIN (unset: off); else False / True / "reference"
_dropout_train_counts = {"ln_own": 0, "ln_torch": 0, "ffn_own": 0, "ffn_torch": 0}


def dropout_training_enabled():
    """False, True or "reference"."""
    if _dropout_train is not None:
        return _dropout_train
    v = os.environ.get("TF_DROPOUT_TRAIN", "0")
    return "reference" if v == "reference" else v not in ("", "0")


def set_dropout_training(flag):
    """Switch dropout inside the training kernels on or off, or to the torch-op "reference" mode (process-wide; None: follow
    TF_DROPOUT_TRAIN again); returns the previous setting."""
    global _dropout_train
    prev = dropout_training_enabled()
    _dropout_train = None if flag is None else ("reference" if flag == "reference" else bool(flag))
    return _switched(prev, dropout_training_enabled())


def dropout_train_counts(reset=False):
    """With the switch on: how many dropout sites in training mode ran the library's own kernels ("ln_own": residual + LayerNorm,
    "ffn_own": feed-forward hidden activation) and how many kept today's torch ops ("ln_torch", "ffn_torch")."""
    return _read_counts(_dropout_train_counts, reset)


def dropout_rng(device):
    """(seed, offset) of one dropout site: int64[2] on the device, drawn with torch's generator of that device -- no host
    synchronisation, and inside a captured graph a draw that every replay repeats with fresh values."""
    return torch.empty(2, dtype=torch.int64, device=device).random_()


def dropout_scale(p):
    """The float 1.0f / (1.0f - p) of the generator contract, as a Python float."""
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(float(p), dtype=torch.float32)))


def dropout_keep(rng, p, n, first=0):
    """The keep decisions (uint8 [n], 1 = kept) of elements first .. first + n - 1 of the stream `rng` (tf_dropout_keep_u8)."""
    keep = torch.empty(n, dtype=torch.uint8, device=rng.device)
    with torch.cuda.device(rng.device):
        rc = _cabi.lib().tf_dropout_keep_u8(rng.data_ptr(), float(p), first, n, keep.data_ptr(), _stream(rng.device))
    _cabi.check(rc, "tf_dropout_keep_u8")
    return keep


def _dropout_active(dropout):
    return dropout.training and 0.0 < dropout.p < 1.0


def _reference_factor(t, p):
    """keep scale for the elements of t (its logical order), in t's dtype: what "reference" mode multiplies with."""
    keep = dropout_keep(dropout_rng(t.device), p, t.numel()).view(t.shape)
    return keep.to(t.dtype) * dropout_scale(p)


class _DropoutLayerNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, bias, eps, p, rng):
        return _layernorm_train_forward(ctx, x, res, weight, bias, eps, drop=(p, rng))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        return _layernorm_train_backward(ctx, dy) + (None, None, None)


def dropout_residual_norm(x, res, norm, dropout):
    """norm(x + dropout(res)) where set_dropout_training() takes the site, else None (the caller applies dropout(res) and goes on as
    before).  True: tf_add_dropout_layernorm_train_f32 / _bwd_f32 when layernorm_train_route(x) holds, the module is in training mode with
    0 < p < 1 and the tensors pass layernorm_train's gates (counted ln_own; an active site that is declined: ln_torch).  "reference":
    torch ops with the mask of tf_dropout_keep_u8, any floating dtype on the device."""
    mode = dropout_training_enabled()
    if not mode or not _dropout_active(dropout) or not torch.is_grad_enabled():   # (a forward without gradients keeps torch's dropout, uncounted)
        return None
    if mode == "reference":
        if not (x.is_cuda and res.is_cuda and res.is_floating_point() and res.numel() > 0 and res.numel() % 4 == 0):
            return None
        return norm(x + res * _reference_factor(res, dropout.p))
    ok = layernorm_train_route(x) and res is not None
    if ok:
        ok, res = _layernorm_train_gates(x, res, norm)
    if not ok:
        _dropout_train_counts["ln_torch"] += 1
        return None
    _dropout_train_counts["ln_own"] += 1
    return _DropoutLayerNormTrain.apply(x, res, norm.weight, norm.bias, norm.eps, float(dropout.p), dropout_rng(x.device))


def dropout_ffn_hidden(x, linear_module, relu, dropout):
    """dropout(relu(linear(x))) where set_dropout_training() takes the site, else None (the caller runs today's lines).  True:
    linear_train(..., relu=True, dropout=dropout) when train_route(x) holds (counted ffn_own; an active site that is declined:
    ffn_torch).  "reference": torch ops with the mask of tf_dropout_keep_u8."""
    mode = dropout_training_enabled()
    if not mode or not _dropout_active(dropout) or not torch.is_grad_enabled():   # (a forward without gradients keeps torch's dropout, uncounted)
        return None
    if mode == "reference":
        n = x.numel() // max(x.shape[-1], 1) * linear_module.weight.shape[0]
        if not (relu and x.is_cuda and x.is_floating_point() and n > 0 and n % 4 == 0):
            return None
        y = torch.relu(F.linear(x, linear_module.weight, linear_module.bias))
        return y * _reference_factor(y, dropout.p)
    y = linear_train(x, linear_module.weight, linear_module.bias, relu=True, dropout=dropout) if relu and train_route(x) else None
    _dropout_train_counts["ffn_own" if y is not None else "ffn_torch"] += 1
    return y


# ------------------------------------------------------------------------------------------------------------------------------
# TRAINING THROUGH THE DECODER SELF-ATTENTION (opt-in; include/tf_fused.h: TRAINING THROUGH THE ATTENTION CORE; csrc/mha_bwd.h).  With
# gradients enabled the decoder layer's query self-attention is nn.MultiheadAttention's chain: an in-projection, three transposes,
# baddbmm, a masked softmax, an ATen dropout that writes a dropped [N H, L, L] copy and a byte mask, bmm, the head-averaged weights
# nobody reads, the out-projection -- and the reverse of all of it.  set_attention_training(True) / TF_ATTENTION_TRAIN=1 routes the site
# (DeformableTransformerDecoderLayer.self_attention_training) through two projections (linear_train where train_route() holds),
# mha_core_train below and the out-projection, batch-first, without a transpose: the forward is the deployed attention core plus the
# rows' softmax statistics, the backward ONE launch that rebuilds the weights -- nothing of size L x L is stored, no atomics, bit-identical
# from call to call.  Dropout on the weights follows THE MASK CONTRACT of the header: decided by the counter-based generator, recomputed
# in the backward.  A site whose nn.MultiheadAttention drops (dropout > 0, training mode) needs set_dropout_training() as well: True --
# the kernels decide the mask from dropout_rng(); "reference" -- the same draw, the mask of tf_dropout_keep_u8 over the padded rows and
# torch ops in any floating dtype (the oracle of the layer test); False -- today's line.  NOT covered: plain DETR's transformer.py, the
# track-attention layers, head dimensions other than 32 and 36, more than 1024 queries, float (additive) masks, host tensors, a forward
# without gradients.  OFF by default: whether it is faster inside a training step is a measurement (tools/bench_attention_train.py,
# profiles/attention_train_bench.json), not a promise.
_attention_train = None    # None: follow TF_ATTENTION_TRAIN (unset: off)
_attention_train_counts = {"own": 0, "own_dropout": 0, "reference": 0, "torch": 0}
_ATTENTION_TRAIN_HEAD_DIMS = (32, 36)
_ATTENTION_TRAIN_MAX_L = 1024


def attention_training_enabled():
    if _attention_train is not None:
        return _attention_train
    return os.environ.get("TF_ATTENTION_TRAIN", "0") not in ("", "0")


def set_attention_training(flag):
    """Switch the training path of the decoder's query self-attention on or off (process-wide; None: follow TF_ATTENTION_TRAIN again);
    returns the previous setting."""
    global _attention_train
    prev = attention_training_enabled()
    _attention_train = None if flag is None else bool(flag)
    return _switched(prev, attention_training_enabled())


def attention_train_counts(reset=False):
    """With the switch on: how many self-attention sites with gradients ran the library's own kernels without dropout ("own") or with the
    mask decided inside them ("own_dropout"), the torch-op reference mode ("reference"), or today's nn.MultiheadAttention call ("torch")."""
    return _read_counts(_attention_train_counts, reset)


def _attention_mask_ok(key_padding_mask, x):
    """None, or a bool / uint8 [N, L] mask on x's device (a float mask is ADDITIVE for nn.MultiheadAttention: not taken)."""
    return key_padding_mask is None or (key_padding_mask.dtype in (torch.bool, torch.uint8) and key_padding_mask.device == x.device
                                        and key_padding_mask.shape == x.shape[:2])


def attention_train_applies(mha, x, key_padding_mask=None):
    """The gate of the own route for nn.MultiheadAttention `mha` on the batch-first x [N, L, E]: gradients enabled, fp32 device tensors,
    the packed in-projection, head dimension 32 or 36, 1 <= L <= 1024, mask None or bool / uint8 [N, L]."""
    if not (torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0):
        return False
    w, b = mha.in_proj_weight, mha.in_proj_bias
    E, H = mha.embed_dim, mha.num_heads
    if w is None or b is None or mha.bias_k is not None or mha.add_zero_attn or x.shape[-1] != E or E % H:
        return False
    if not (_param_ok(w, x) and _param_ok(b, x) and w.shape == (3 * E, E)):
        return False
    return (E // H in _ATTENTION_TRAIN_HEAD_DIMS and x.shape[1] <= _ATTENTION_TRAIN_MAX_L and x.shape[0] <= 65535
            and _attention_mask_ok(key_padding_mask, x))


def attention_train_site(mha, x, key_padding_mask=None):
    """How one self-attention site of a training-graph forward runs, counted: None -- today's nn.MultiheadAttention call (uncounted with
    the switch off, "torch" with it on) --, ("own", 0.0, None), ("own_dropout", p, rng) or ("reference", p, rng).  rng is drawn HERE,
    once per site that drops, in both modes: the own route and the reference mode see the same masks under one seed.  A forward without
    gradients (the tracking model's previous-frame pass) keeps today's call, uncounted, as at the other training sites."""
    if not attention_training_enabled() or not torch.is_grad_enabled():
        return None
    drops = mha.training and mha.dropout > 0.0
    mode = dropout_training_enabled() if drops else True
    route = None
    if mode == "reference":
        w = mha.in_proj_weight
        if (torch.is_grad_enabled() and x.is_cuda and x.is_floating_point() and x.dim() == 3 and x.numel() > 0 and w is not None
                and mha.in_proj_bias is not None and w.dtype == x.dtype and mha.bias_k is None and not mha.add_zero_attn
                and mha.dropout < 1.0 and _attention_mask_ok(key_padding_mask, x)):
            route = ("reference", float(mha.dropout), dropout_rng(x.device))
    elif mode and (not drops or mha.dropout < 1.0) and attention_train_applies(mha, x, key_padding_mask):
        route = ("own_dropout", float(mha.dropout), dropout_rng(x.device)) if drops else ("own", 0.0, None)
    _attention_train_counts[route[0] if route else "torch"] += 1
    return route


class _MhaCoreTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qk, v, num_heads, mask, p, rng):
        n, length, e2 = qk.shape
        e = e2 // 2
        d = e // num_heads
        with torch.cuda.device(qk.device):
            out = torch.empty((n, length, e), dtype=torch.float32, device=qk.device)
            stats = torch.empty((n, num_heads, length, 2), dtype=torch.float32, device=qk.device)
            q_ptr = qk.data_ptr()
            rc = _cabi.lib().tf_mha_core_train_f32(q_ptr, q_ptr + e * 4, v.data_ptr(), out.data_ptr(), _ptr(mask), stats.data_ptr(), _ptr(rng),
                                                   float(p), n, length, length, num_heads, d, e2, e2, e, e, float(d) ** -0.5,
                                                   _stream(qk.device))
        _cabi.check(rc, "tf_mha_core_train_f32")
        ctx.num_heads, ctx.p = num_heads, float(p)
        ctx.save_for_backward(qk, v, out, stats, mask, rng)   # the operands, the output and two floats per row: nothing of size L x L
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        qk, v, out, stats, mask, rng = ctx.saved_tensors
        n, length, e2 = qk.shape
        e = e2 // 2
        d = e // ctx.num_heads
        dout = _aligned(dout)
        with torch.cuda.device(qk.device):
            dqk, dv = torch.empty_like(qk), torch.empty_like(v)   # dq | dk: the halves of the shared projection's gradient, no cat
            q_ptr, g_ptr = qk.data_ptr(), dqk.data_ptr()
            rc = _cabi.lib().tf_mha_core_bwd_f32(dout.data_ptr(), q_ptr, q_ptr + e * 4, v.data_ptr(), out.data_ptr(), stats.data_ptr(),
                                                 _ptr(mask), _ptr(rng), ctx.p, g_ptr, g_ptr + e * 4, dv.data_ptr(), n, length, length,
                                                 ctx.num_heads, d, e, e2, e2, e, e, e2, e2, e, float(d) ** -0.5, _stream(qk.device))
        _cabi.check(rc, "tf_mha_core_bwd_f32")
        return dqk, dv, None, None, None, None


def mha_core_train(qk, v, num_heads, key_padding_mask=None, p=0.0, rng=None):
    """dropout_p(softmax(q k^T / sqrt(d))) v with the library's own backward (include/tf_fused.h: tf_mha_core_train_f32 /
    tf_mha_core_bwd_f32).  qk [N, L, 2E]: the shared q | k projection, v [N, L, E], fp32, contiguous, on the device; head dimension 32 or
    36, L <= 1024; key_padding_mask [N, L] bool / uint8 (True = ignore) or None; rng: the int64[2] (seed, offset) tensor of
    dropout_rng(), or None for no dropout (p is not read then).  Saves qk, v, out, the rows' statistics, the uint8 mask and rng; its
    backward returns (dqk, dv).  Anything the kernels do not take is an error (attention_train_applies is the gate)."""
    if not (qk.is_cuda and qk.dtype == torch.float32 and v.dtype == torch.float32 and v.device == qk.device and qk.dim() == 3
            and v.dim() == 3):
        raise ValueError("mha_core_train: fp32 device tensors [N, L, 2E] and [N, L, E] expected")
    qk, v = _aligned(qk), _aligned(v)
    n, length, e2 = qk.shape
    if e2 % 2 or v.shape != (n, length, e2 // 2) or (e2 // 2) % num_heads:
        raise ValueError("mha_core_train: shapes %s / %s with %d heads" % (tuple(qk.shape), tuple(v.shape), num_heads))
    mask = None
    if key_padding_mask is not None:
        if not _attention_mask_ok(key_padding_mask, qk):
            raise ValueError("mha_core_train: key_padding_mask must be bool / uint8 [N, L] on the device")
        mask = key_padding_mask.to(torch.uint8).contiguous()
    return _MhaCoreTrain.apply(qk, v, num_heads, mask, p, rng)


def attention_reference(x, value_in, mha, key_padding_mask, p, rng):
    """The "reference" mode of the site: out_proj(dropout(softmax(q k^T / sqrt(d))) v) in torch ops, batch-first, any floating dtype, with
    the mask of tf_dropout_keep_u8 over the padded weight tensor [N, H, L, 4 ceil(L / 4)] (THE MASK CONTRACT)."""
    E, H = mha.embed_dim, mha.num_heads
    n, length, _ = x.shape
    d = E // H
    w, b = mha.in_proj_weight, mha.in_proj_bias
    qk = F.linear(x, w[:2 * E], b[:2 * E]).view(n, length, 2, H, d)
    v = F.linear(value_in, w[2 * E:], b[2 * E:]).view(n, length, H, d)
    s = (qk[:, :, 0].permute(0, 2, 1, 3) @ qk[:, :, 1].permute(0, 2, 3, 1)) * (float(d) ** -0.5)
    if key_padding_mask is not None:
        s = s.masked_fill(key_padding_mask.to(torch.bool)[:, None, None, :], float("-inf"))
    lk4 = 4 * ((length + 3) // 4)
    keep = dropout_keep(rng, p, n * H * length * lk4).view(n, H, length, lk4)[..., :length]
    weights = torch.softmax(s, -1) * (keep.to(x.dtype) * dropout_scale(p))
    o = (weights @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(n, length, E)
    return mha.out_proj(o)


# ------------------------------------------------------------------------------------------------------------------------------
# THE TRAINING PATH OF THE BACKBONE'S CONVOLUTIONS (opt-in; include/tf_fused.h: THE BACKWARD OF A 3 x 3 CONVOLUTION; csrc/conv_bwd.h).
# The switch lives with its caller (backbone.set_split_conv_training / TF_SPLIT_CONV_TRAIN=1: the trainable bottlenecks' conv + FrozenBN
# pairs); conv_train below is the operator.  3 x 3, padding 1, stride 1 or 2: the forward is conv3x3() (bit-identical to the inference
# route), the backward the library's statistics, input-gradient (stride 1) and weight-gradient kernels.  1 x 1, stride 1: _LinearTrain on
# the pixel matrix of the channels_last activation.  No float atomics: bit-identical from call to call.
# The STRIDE-2 layers (set_strided_conv_training below / TF_STRIDED_CONV_TRAIN=1, a switch of its own, off by default; include/tf_fused.h:
# THE BACKWARD OF THE STRIDE-2 CONVOLUTIONS; csrc/conv_strided_bwd.h): the input gradient of a stride-2 3 x 3 by parity classes
# (tf_conv_dgrad_stride2_packed_f32), and the strided 1 x 1 projection -- forward conv3x3(), input gradient the same entry point with
# ks = 1, weight gradient tf_conv1x1_strided_wgrad_split_f32.  With that switch off the strided 1 x 1 is not conv_train's and the input
# gradient of a stride-2 3 x 3 is torch's (counted).  NOT covered: the stem, input_proj, the mask head, GroupNorm.
_conv_train_counts = {"fwd_own": 0, "fwd_torch": 0, "dgrad_own": 0, "dgrad_torch": 0, "wgrad_own": 0, "wgrad_torch": 0}
_strided_conv_train = None    # None: follow TF_STRIDED_CONV_TRAIN (unset: off)


def conv_train_counts(reset=False):
    """How conv_train's calls went: forwards it ran (fwd_own) or declined on device tensors (fwd_torch: the caller's F.conv2d), and
    the input / weight gradients of its 3 x 3 and strided 1 x 1 calls by the library's own kernels or by torch.  (The gradients of
    the stride-1 1 x 1 calls are linear_train's: train_route_counts().)"""
    return _read_counts(_conv_train_counts, reset)


def strided_conv_training_enabled():
    if _strided_conv_train is not None:
        return _strided_conv_train
    return os.environ.get("TF_STRIDED_CONV_TRAIN", "0") not in ("", "0")


def set_strided_conv_training(flag):
    """Switch conv_train's own backward of the stride-2 convolutions on or off (process-wide; None: follow TF_STRIDED_CONV_TRAIN again);
    returns the previous setting."""
    global _strided_conv_train
    prev = strided_conv_training_enabled()
    _strided_conv_train = None if flag is None else bool(flag)
    return _switched(prev, strided_conv_training_enabled())


def _packed_weight_classes(w, terms, ks):
    """Fragment-order images of the four parity-class weights W_c [Cin, T_c Cout] of a tap-major 3 x 3 weight [Cout, 9 Cin] -- or of the
    one class w^T of a 1 x 1 weight [Cout, Cin] -- one behind the other in one buffer (the `wcls_packed` of
    tf_conv_dgrad_stride2_packed_f32), cached on w under its source_key() with the rules of _packed_weight_rot; None when it cannot
    be built (shape; stream capture without a cached image)."""
    cout = w.shape[0]
    if ks == 1:
        cin = w.shape[1]
        return _packed_image(w, "_tf_packed_cls", [cout], [cin], terms, lambda: [w.detach().t().contiguous()])
    cin = w.shape[1] // 9
    taps = ((1,), (2, 0))   # by parity: the tap rows (columns) in the order of the dy rows (columns) a, a + 1 they read

    def classes():
        w4 = w.detach().view(cout, 3, 3, cin)
        return [torch.stack([w4[:, ky, kx] for ky in taps[py] for kx in taps[px]]).permute(2, 0, 1).reshape(cin, -1).contiguous()
                for py in (0, 1) for px in (0, 1)]
    return _packed_image(w, "_tf_packed_cls", [t * cout for t in (1, 2, 2, 4)], [cin] * 4, terms, classes)


def _strided_dgrad_gates(n, h, w, cin, cout):
    """The shapes tf_conv_dgrad_stride2_packed_f32 takes (its own checks, made here so that the fallback is chosen before any work)."""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return cout % 64 == 0 and cin % 4 == 0 and (n * h * w + 256) * cin * 4 < 0xC0000000 and n * ho * wo * cout * 4 < 0xC0000000


# _conv_ksplit's policy tuple for the stride-2 input gradient, PINNED to the values the forward's policy has today (pieces of at least
# 256 products): set_conv_ksplit_policy / TF_CONV_KSPLIT_POLICY tune the inference route and do not move this cut.  Measured on an
# MI355X in the cfg-3 small step, tests/test_conv_strided_backward_step_gpu.py: with this tuple backbone layer3's worst element stands
# at 3.8 / 3.4-3.8 of the harness's 4 yardsticks (the switches alone / every training switch on); pieces of 128 products from 256 products
# on, (768, 300, 4, 8), were tried and are WORSE there: 4.2, outside the bound.
_STRIDED_DGRAD_KSPLIT_POLICY = (768, 300, 8, 32)


def _strided_dgrad_ksplit(n, h, w, cin, cout, ks):
    """Pieces the longest contraction of the stride-2 input gradient (4 Cout products of the odd-odd class; Cout for a 1 x 1) is cut
    into: _conv_ksplit on that class's (pixels, products, Cin) -- a function of the shape alone.  The shorter classes are cut in
    proportion inside the library."""
    if ks == 1:
        return _conv_ksplit(n * ((h + 1) // 2) * ((w + 1) // 2), cout, cin, _STRIDED_DGRAD_KSPLIT_POLICY)
    return _conv_ksplit(max(1, n * (h // 2) * (w // 2)), 4 * cout, cin, _STRIDED_DGRAD_KSPLIT_POLICY)


def _strided_dgrad(dyn, s_dy, packed, n, h, w, cin, cout, ks, terms, stream):
    """tf_conv_dgrad_stride2_packed_f32 -> dx [n, h, w, cin] (NHWC)."""
    L = _cabi.lib()
    ksplit = _strided_dgrad_ksplit(n, h, w, cin, cout, ks)
    nbytes = int(L.tf_conv_dgrad_stride2_workspace_bytes(n, h, w, cin, cout, ks, ksplit))
    if nbytes < 0:
        _cabi.check(-2, "tf_conv_dgrad_stride2_packed_f32")
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dyn.device)
    dxn = torch.empty((n, h, w, cin), dtype=torch.float32, device=dyn.device)
    rc = L.tf_conv_dgrad_stride2_packed_f32(dyn.data_ptr(), s_dy.data_ptr(), packed.data_ptr(), dxn.data_ptr(), ws.data_ptr(), nbytes, ksplit,
                                            n, h, w, cin, cout, ks, terms, stream)
    _cabi.check(rc, "tf_conv_dgrad_stride2_packed_f32")
    return dxn


def _packed_weight_rot(w_taps, terms):
    """Fragment-order image of w_rot[ci, ky, kx, co] = w[co, 2 - ky, 2 - kx, ci] as [Cin, 9 Cout] (the `weight` of the input gradient
    dx = conv3x3(dy, w_rot)), cached on the tap-major weight under its source_key() like _packed_weight_t; None when it cannot be
    built (shape; stream capture without a cached image).  The cache serves a weight tensor that persists; backbone._conv_bn hands
    conv_train a new image of the folded weight every step, so there the image is packed once per call, and a training step captured
    into a HIP graph finds none: its 3 x 3 input gradients are torch's (counted in conv_train_counts)."""
    cout, cin = w_taps.shape[0], w_taps.shape[1] // 9
    return _packed_image(w_taps, "_tf_packed_rot", 9 * cout, cin, terms,
                         lambda: w_taps.detach().view(cout, 3, 3, cin).flip(1, 2).permute(3, 1, 2, 0).contiguous())


def _own_tensor(v):
    """A tensor object of its own over the storage of v (a view made inside a Function's forward): what the Function returns is then
    no view to autograd, and the caller may go on in place (backbone._BiasAct) as it does on F.conv2d's output."""
    return torch.empty(0, dtype=v.dtype, device=v.device).set_(v.untyped_storage(), v.storage_offset(), v.size(), v.stride())


class _Conv1x1Train(torch.autograd.Function):
    """_LinearTrain on the [N H W, Cin] view of a channels_last activation: conv1x1_as_gemm with linear_train as its linear_fn (no bias,
    residual or ReLU).  `bias` is always None: it keeps the argument positions _LinearTrain.backward reads.  Few pixels under a long
    contraction are cut into pieces by the inference route's rule (conv1x1_wants_split_k / _conv_ksplit), in the forward (the
    convolution kernel with its K loop cut, as backbone._conv_bn runs it in inference) and in the input gradient
    (tf_linear_dgrad_splitk_packed_f32): more workgroups, and no matrix-core accumulator over the whole sum."""

    @staticmethod
    def forward(ctx, x, w2d, bias):
        n, cin, h, wd = x.shape
        cout, M = w2d.shape[0], n * h * wd
        x2 = x.permute(0, 2, 3, 1).reshape(M, cin)   # a view: NHWC storage
        y = None
        if cin % 4 == 0 and conv1x1_wants_split_k(M, cin, cout):
            with one_stream():
                y = conv3x3(x, w2d, None, False, 1)
        if y is not None:
            ctx.relu = False
            ctx.terms = _route_terms(w2d)
            ctx.save_for_backward(x2, w2d, None)
        else:
            y = _LinearTrain.forward(ctx, x2, w2d, None, False).view(n, h, wd, cout).permute(0, 3, 1, 2)
        ks = _conv_ksplit(M, cout, cin) if (_conv1x1_splitk and cin % 4 == 0) else 1
        ctx.dgrad_ksplit = ks if ks >= _CONV1X1_MIN_PIECES else 1
        ctx.x_shape = (n, h, wd, cin)
        return _own_tensor(y)   # NCHW shape over NHWC storage = channels_last

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        n, h, wd, cin = ctx.x_shape
        dx2, dw, _, _ = _LinearTrain.backward(ctx, dy.permute(0, 2, 3, 1).reshape(n * h * wd, dy.shape[1]))
        return (None if dx2 is None else dx2.view(n, h, wd, cin).permute(0, 3, 1, 2)), dw, None


def _conv_backward(needs, dy, x, w2, ks, stride, terms):
    """(dx, dw) of conv_train's convolutions -- ks = 3: padding 1, stride 1 or 2, w2 [Cout, 9 Cin] tap-major; ks = 1: the stride-2
    projection without padding, w2 [Cout, Cin] --: the statistics of dy, the input gradient (stride 1: tf_conv3x3_dgrad_packed_f32;
    stride 2: tf_conv_dgrad_stride2_packed_f32 under set_strided_conv_training), the statistics of x (one scale per input channel over
    ALL pixels of x) and the weight gradient (tf_conv3x3_wgrad_split_f32 / tf_conv1x1_strided_wgrad_split_f32); a gradient whose
    kernel does not take the call is torch.ops.aten.convolution_backward on the same tensors.  Counted in _conv_train_counts."""
    need_x, need_w = needs[0], needs[1]
    n, cin, h, w = x.shape
    cout, taps = w2.shape[0], ks * ks
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    M = n * ho * wo
    L = _cabi.lib()
    dyn = _aligned(dy.permute(0, 2, 3, 1))   # NHWC: the storage of a channels_last gradient
    xn = x.permute(0, 2, 3, 1)     # (contiguous: conv3x3 took x)
    if xn.data_ptr() % 16:
        xn = xn.clone(memory_format=torch.contiguous_format)
    fp32 = dy.dtype == torch.float32
    own_w = fp32 and cin % 4 == 0 and cout % 4 == 0 and max(M * cout, n * h * w * cin, cout * taps * cin) * 4 < 0xC0000000
    own_x = (fp32 and ks == 3 and stride == 1 and cout % 64 == 0 and cin % 4 == 0 and (M + 256) * cin * 4 < 0xC0000000
             and M * cout * 4 < 0xC0000000)
    own_x2 = fp32 and stride == 2 and (ks == 1 or strided_conv_training_enabled()) and _strided_dgrad_gates(n, h, w, cin, cout)
    dx = dw = None
    with torch.cuda.device(dy.device), one_stream():
        stream = _stream(dy.device)
        packed_rot = _packed_weight_rot(w2, terms) if need_x and own_x else None
        packed_cls = _packed_weight_classes(w2, terms, ks) if need_x and own_x2 else None
        do_x, do_w = packed_rot is not None or packed_cls is not None, need_w and own_w
        s_dy = _grad_stats(dyn.view(M, cout), 0, terms, False)[0] if (do_x or do_w) else None
        if packed_cls is not None:   # stride 2: stride-1 windows over dy, one per parity class of the input pixel
            dx = _strided_dgrad(dyn, s_dy, packed_cls, n, h, w, cin, cout, ks, terms, stream).permute(0, 3, 1, 2)
        elif do_x:
            # the contraction is cut as the forward's is (few pixels under a long K: more workgroups, and no accumulator walks
            # all 9 Cout products)
            ksplit = _conv_ksplit(M, 9 * cout, cin, _HALO_KSPLIT_POLICY if _conv_halo else None)
            dxn = torch.empty((n, h, w, cin), dtype=torch.float32, device=dy.device)
            wsx = torch.empty((ksplit, M * cin), dtype=torch.float32, device=dy.device) if ksplit > 1 else None
            rc = L.tf_conv3x3_dgrad_packed_f32(dyn.data_ptr(), s_dy.data_ptr(), packed_rot.data_ptr(), dxn.data_ptr(), _ptr(wsx), ksplit,
                                               n, h, w, cin, cout, terms, stream)
            _cabi.check(rc, "tf_conv3x3_dgrad_packed_f32")
            dx = dxn.permute(0, 3, 1, 2)
        if do_w:
            s_x, _ = _grad_stats(xn.view(n * h * w, cin), 1, terms, False)
            name = "tf_conv3x3_wgrad" if ks == 3 else "tf_conv1x1_strided_wgrad"
            nbytes = int(getattr(L, name + "_workspace_bytes")(n, h, w, cin, cout, stride))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dy.device)
            dw = torch.empty((cout, taps * cin), dtype=torch.float32, device=dy.device)
            rc = getattr(L, name + "_split_f32")(dyn.data_ptr(), xn.data_ptr(), s_dy.data_ptr(), s_x.data_ptr(), dw.data_ptr(), ws.data_ptr(),
                                                 nbytes, n, h, w, cin, cout, stride, terms, stream)
            _cabi.check(rc, name + "_split_f32")
        mask = [need_x and not do_x, need_w and not do_w, False]
        if mask[0] or mask[1]:   # what the kernels do not take: torch, on the same tensors
            w4 = w2.detach().view(cout, ks, ks, cin).permute(0, 3, 1, 2)   # OIHW shape over its channels_last storage
            pad = ks // 2
            tx, tw, _ = torch.ops.aten.convolution_backward(dy, x, w4, None, [stride, stride], [pad, pad], [1, 1], False, [0, 0], 1, mask)
            if mask[0]:
                dx = tx
            if mask[1]:
                dw = tw.permute(0, 2, 3, 1).reshape(cout, taps * cin)
    if need_x:
        _conv_train_counts["dgrad_own" if do_x else "dgrad_torch"] += 1
    if need_w:
        _conv_train_counts["wgrad_own" if do_w else "wgrad_torch"] += 1
    return dx, dw


class _Conv3x3Train(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_taps, stride, terms):
        with one_stream():   # a training step: the weight images are rebuilt every step for the stream that uses them next
            y = conv3x3(x, w_taps, None, False, stride)
        if y is None:
            raise _NotApplicable()
        ctx.stride, ctx.terms = stride, terms
        ctx.save_for_backward(x, w_taps)
        return _own_tensor(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w_taps = ctx.saved_tensors
        return _conv_backward(ctx.needs_input_grad, dy, x, w_taps, 3, ctx.stride, ctx.terms) + (None, None)


class _Conv1x1StridedTrain(torch.autograd.Function):
    """The stride-2 1 x 1 projection of a bottleneck's identity branch (no padding): forward conv3x3() with the [Cout, Cin] weight, as the
    inference route runs it; backward (_conv_backward) the statistics, tf_conv_dgrad_stride2_packed_f32 with ks = 1 (the even-even
    pixels get dy . w, every other pixel +0) and tf_conv1x1_strided_wgrad_split_f32 (the rows x[n, 2 ho, 2 wo, :] read in place); torch
    for a gradient whose kernel does not take the shape, counted in conv_train_counts."""

    @staticmethod
    def forward(ctx, x, w2d, terms):
        with one_stream():
            y = conv3x3(x, w2d, None, False, 2)
        if y is None:
            raise _NotApplicable()
        ctx.terms = terms
        ctx.save_for_backward(x, w2d)
        return _own_tensor(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w2d = ctx.saved_tensors
        return _conv_backward(ctx.needs_input_grad, dy, x, w2d, 1, 2, ctx.terms) + (None,)


def conv_train(x, w, stride):
    """A backbone convolution with the library's own backward, or None where the forward kernel declines (the caller keeps F.conv2d).
    x [N, Cin, H, W]: channels_last, fp32, on the device.
    w [Cout, 9 Cin] -- the tap-major image `w4.permute(0, 2, 3, 1).reshape(Cout, 9 Cin)` of an OIHW weight, taken OUTSIDE so that autograd
    carries dw back to the parameter (and through the FrozenBN fold): 3 x 3, padding 1, stride 1 or 2.  The forward IS
    conv3x3(x, w, None, False, stride); the backward runs tf_linear_grad_stats_f32 on dy, tf_conv3x3_dgrad_packed_f32 (stride 1,
    Cout % 64 == 0), tf_linear_grad_stats_f32 on x and tf_conv3x3_wgrad_split_f32 (Cin % 4 == 0, Cout % 4 == 0); a gradient whose kernel
    does not take the call (the input gradient under stride 2, Cout % 64 != 0, misaligned or over-size tensors) is computed by
    torch.ops.aten.convolution_backward inside the backward.  conv_train_counts() tells which path ran.
    w [Cout, Cin]: 1 x 1, stride 1, no padding: _LinearTrain on the [N H W, Cin] view of the activation (no bias, residual or ReLU), few
    pixels under a long contraction cut into pieces as the inference route cuts them (_Conv1x1Train).
    With set_strided_conv_training(True): the input gradient of the stride-2 3 x 3 is tf_conv_dgrad_stride2_packed_f32 (Cout % 64 == 0,
    Cin % 4 == 0; else torch, counted), and w [Cout, Cin] with stride 2 (no padding) is taken too (_Conv1x1StridedTrain: forward
    conv3x3(x, w, None, False, 2), own input and weight gradients, torch inside the backward where a gate fails, counted)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and w.dim() == 2 and w.dtype == torch.float32
            and w.device == x.device):
        return None
    y = None
    n, cin, h, wd = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and x.numel() > 0:
        if w.shape[1] == 9 * cin and stride in (1, 2):
            try:
                y = _Conv3x3Train.apply(x, w, stride, _terms())
            except _NotApplicable:
                y = None
        elif w.shape[1] == cin and stride == 1:
            try:
                y = _Conv1x1Train.apply(x, w, None)
            except _NotApplicable:
                y = None
            if y is not None and cin % 32:   # (linear() does not take K % 32 != 0: _LinearTrain's forward was F.linear, its backward ran)
                _conv_train_counts["fwd_torch"] += 1
                return y
        elif w.shape[1] == cin and stride == 2 and strided_conv_training_enabled():
            try:
                y = _Conv1x1StridedTrain.apply(x, w, _terms())
            except _NotApplicable:
                y = None
    _conv_train_counts["fwd_own" if y is not None else "fwd_torch"] += 1
    return y



# ------------------------------------------------------------------------------------------------------------------------------
# THE SET CRITERION AND THE MATCHING COST (opt-in; include/tf_fused.h; csrc/criterion.h).  The operators live in criterion_ops.py and
# are re-exported here: every function DEFINED in this module whose name starts with set_ is a process-wide switch that returns its
# previous value (tests/test_weight_coherence_cpu.py walks them), and set_criterion is an operator -- "set" as in set prediction --,
# not a switch.  The switches of the routes live with their callers: criterion.set_fused, criterion.set_fused_masks (THE MASK LOSSES;
# csrc/mask_loss.h: mask_losses / mask_losses_applies), matcher.set_fused_cost.
from .criterion_ops import criterion_applies, mask_losses, mask_losses_applies, match_cost, set_criterion   # noqa: E402,F401
