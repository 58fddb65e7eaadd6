"""TEST INFRASTRUCTURE of tests/test_weight_coherence_cpu.py and tests/test_weight_coherence_gpu.py: is a kernel handed the CURRENT
weights?

The inference path reads images derived from the parameters (split pieces, packed fragments, folded / tap-major convolution
weights, concatenated projections, cached reference points), built once and cached.  A stale image gives a finite, plausible
result that every float64 bound accepts, so the oracle here is not arithmetic but a COLD TWIN: a newly constructed module loaded
from the mutated module's state_dict, which has never run and therefore holds no image at all.  The kernels are pure functions of
their arguments, so the warm module and its cold twin must agree BIT FOR BIT; and the output after the mutation must differ from
the output before it, or the mutation tested nothing.

MUTATIONS: the ways a weight changes after the first forward, by what they leave behind
  V  the version counter moves           in place under no_grad, load_state_dict, an SGD step, an AdamW step, a write through detach()
  P  the storage or the object changes   p.data = t, vector_to_parameters, load_state_dict(assign=True), a new nn.Parameter,
                                         swap_tensors, copy.deepcopy (then the copy changes; both are checked)
  U  no trace at all                     p.data.mul_(), p.data.copy_(), nn.init.normal_(p.data) -- each followed by fused.weights_changed()
CONSUMERS: one small nn.Module per cached route, at the smallest shape that still takes it, with the parameters and buffers whose
change must reach its output (TARGETS) and the entry point that has to have run (ENTRY)."""
import contextlib
import copy

import torch
from torch import nn

from trackformer_amd import backbone, fused, msda
from trackformer_amd import deformable_transformer as dt
from trackformer_amd import detr_segmentation as ds


# ------------------------------------------------------------------------------------------------------------------- comparisons
def _tensors(y):
    if torch.is_tensor(y):
        return [y]
    out = []
    for v in (y.values() if isinstance(y, dict) else y):
        out += _tensors(v)
    return out


def bits_equal(a, b):
    """Bit for bit (NaN payloads and the sign of zero included): the comparison of a warm object with its cold twin."""
    a, b = _tensors(a), _tensors(b)
    if len(a) != len(b):
        return False
    for s, t in zip(a, b):
        if s.shape != t.shape or s.dtype != t.dtype or s.device != t.device:
            return False
        if s.dtype == torch.float32:
            s, t = s.contiguous().view(torch.int32), t.contiguous().view(torch.int32)
        elif s.dtype in (torch.float16, torch.bfloat16):
            s, t = s.contiguous().view(torch.int16), t.contiguous().view(torch.int16)
        if not torch.equal(s, t):
            return False
    return True


# --------------------------------------------------------------------------------------------------------------------- mutations
def owner_of(m, name):
    path, _, leaf = name.rpartition(".")
    return (m.get_submodule(path) if path else m), leaf


def tensor_of(m, name):
    o, leaf = owner_of(m, name)
    return getattr(o, leaf)


def _wave(p):
    i = torch.arange(p.numel(), dtype=torch.float32)
    return (0.0625 * torch.cos(0.7 * i + 0.3)).reshape(p.shape).to(p.device, p.dtype)


def perturbed(p):
    """New values for `p` in a new tensor: every element moves (zero-initialised weights too), a running_var in [0.5, 1.5] stays
    positive."""
    return p.detach() * 1.25 + _wave(p)


def mut_inplace(m, name):
    p = tensor_of(m, name)
    with torch.no_grad():
        p.mul_(1.25).add_(_wave(p))


def _state(m, name):
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert name in sd, name
    sd[name] = perturbed(tensor_of(m, name))
    return sd


def mut_load_state_dict(m, name):
    m.load_state_dict(_state(m, name))


def mut_sgd_step(m, name):
    p = tensor_of(m, name)
    p.grad = (p.detach() - perturbed(p)) / 0.5
    torch.optim.SGD([p], lr=0.5).step()
    p.grad = None


def mut_adamw_step(m, name):
    p = tensor_of(m, name)
    p.grad = _wave(p)
    torch.optim.AdamW([p], lr=0.05).step()   # (the default `foreach`)
    p.grad = None


def mut_detach_write(m, name):
    p = tensor_of(m, name)
    p.detach().mul_(1.25).add_(_wave(p))


def mut_data_assign(m, name):
    p = tensor_of(m, name)
    p.data = perturbed(p)


def mut_vector_to_parameters(m, name):
    p = tensor_of(m, name)
    torch.nn.utils.vector_to_parameters(perturbed(p).flatten(), [p])


def mut_load_state_dict_assign(m, name):
    m.load_state_dict(_state(m, name), assign=True)


def mut_new_parameter(m, name):
    o, leaf = owner_of(m, name)
    p = getattr(o, leaf)
    setattr(o, leaf, nn.Parameter(perturbed(p)) if isinstance(p, nn.Parameter) else perturbed(p))


def mut_swap_tensors(m, name):
    p = tensor_of(m, name)
    other = nn.Parameter(perturbed(p)) if isinstance(p, nn.Parameter) else perturbed(p)
    torch.utils.swap_tensors(p, other)


def mut_data_write_then_tell(m, name):
    p = tensor_of(m, name)
    p.data.mul_(1.25).add_(_wave(p))
    fused.weights_changed()


def mut_data_copy_then_tell(m, name):
    p = tensor_of(m, name)
    p.data.copy_(perturbed(p))
    fused.weights_changed()


def mut_init_through_data_then_tell(m, name):
    p = tensor_of(m, name)
    nn.init.normal_(p.data, mean=float(p.detach().mean()) + 0.01, std=0.02 + 0.1 * float(p.detach().std()) if p.numel() > 1 else 0.02)
    fused.weights_changed()


DEEPCOPY = "deepcopy"   # handled by check(): copy the warmed module, change the copy, check the copy AND the original

# (id, mutation, applies to parameters only -- an optimiser steps no buffer)
MUTATIONS = {
    "V": [("inplace_no_grad", mut_inplace, False), ("load_state_dict", mut_load_state_dict, False), ("sgd_step", mut_sgd_step, True),
          ("adamw_step", mut_adamw_step, True), ("detach_write", mut_detach_write, False)],
    "P": [("data_assign", mut_data_assign, False), ("vector_to_parameters", mut_vector_to_parameters, False),
          ("load_state_dict_assign", mut_load_state_dict_assign, False), ("new_parameter", mut_new_parameter, False),
          ("swap_tensors", mut_swap_tensors, False), ("deepcopy", DEEPCOPY, False)],
    "U": [("data_write_then_weights_changed", mut_data_write_then_tell, False),
          ("data_copy_then_weights_changed", mut_data_copy_then_tell, False),
          ("init_through_data_then_weights_changed", mut_init_through_data_then_tell, False)],
}
ALL_MUTATIONS = [(cls + ":" + mid, fn, params_only) for cls, rows in MUTATIONS.items() for mid, fn, params_only in rows]


# --------------------------------------------------------------------------------------------------------------------- consumers
def randomize(m, seed=1):
    """Values under which every parameter and buffer matters (the package's initialisers leave several at zero)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, t in list(m.named_parameters()) + list(m.named_buffers()):
            if not t.is_floating_point():
                continue
            if n.endswith("running_var"):
                v = torch.rand(t.shape, generator=g) + 0.5
            elif t.dim() > 1:
                v = torch.randn(t.shape, generator=g) * t[0].numel() ** -0.5
            elif n.endswith("weight"):
                v = 1.0 + 0.2 * torch.randn(t.shape, generator=g)
            else:
                v = 0.2 * torch.randn(t.shape, generator=g)
            t.copy_(v)
    return m.eval()


def _need(y, what):
    assert y is not None, "%s declined the call: the cached route did not run" % what
    return y


class Consumer(nn.Module):
    TARGETS = ()
    ENTRY = ()            # entry points of the library of which at least one call must have been made (emulator: lib.calls)
    NEEDS_LIBRARY = True  # False: plain PyTorch on cached tensors (runs on CPU tensors without the emulator)

    @staticmethod
    def inputs(g):
        raise NotImplementedError

    @contextlib.contextmanager
    def patches(self):
        yield


class LinearC(Consumer):
    """fused.linear: _split_weight's pieces of lin.weight (33 x 96 -> 200; rows: a row block of it)."""
    TARGETS = ("lin.weight", "lin.bias")
    ENTRY = ("tf_linear_split_f32",)

    def __init__(self, rows=None):
        super().__init__()
        self.lin, self.rows = nn.Linear(96, 200), rows

    @staticmethod
    def inputs(g):
        return (torch.randn(33, 96, generator=g),)

    def forward(self, x):
        b = self.lin.bias if self.rows is None else self.lin.bias[self.rows[0]:self.rows[1]]
        return _need(fused.linear(x, self.lin.weight, b, rows=self.rows), "fused.linear")


class LinearRowsC(LinearC):
    def __init__(self):
        super().__init__(rows=(64, 136))


class PackedLinearC(Consumer):
    """fused.linear through tf_linear_packed_f32 (_packed_weight), forced as tests/test_linear_split_gpu.py does: 130 x 64 -> 400."""
    TARGETS = ("lin.weight",)
    ENTRY = ("tf_linear_packed_f32",)

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(64, 400)

    @staticmethod
    def inputs(g):
        return (torch.randn(130, 64, generator=g),)

    @contextlib.contextmanager
    def patches(self):
        old, old_on = fused._use_packed, fused.set_packed_linear(True)
        fused._use_packed = lambda m, k, n: fused._packed_linear and k % 64 == 0
        try:
            yield
        finally:
            fused._use_packed = old
            fused.set_packed_linear(old_on)

    def forward(self, x):
        return _need(fused.linear(x, self.lin.weight, self.lin.bias, relu=True), "fused.linear (packed)")


class LinearAddC(Consumer):
    """tf_linear_split_add_f32: 300 x 256 -> 384."""
    TARGETS = ("lin.weight",)
    ENTRY = ("tf_linear_split_add_f32",)

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(256, 384)

    @staticmethod
    def inputs(g):
        return (torch.randn(300, 256, generator=g), torch.randn(300, 256, generator=g))

    def forward(self, x, x2):
        return _need(fused.linear_add(x, x2, self.lin.weight, self.lin.bias), "fused.linear_add")


@contextlib.contextmanager
def _min_rows_one():
    old = fused._FFN_FUSED_MIN_ROWS, fused._LINLN_MIN_ROWS
    fused._FFN_FUSED_MIN_ROWS = fused._LINLN_MIN_ROWS = 1
    try:
        yield
    finally:
        fused._FFN_FUSED_MIN_ROWS, fused._LINLN_MIN_ROWS = old


class FfnC(Consumer):
    """fused.ffn (tf_ffn_fused_f32, two packed images): D 256, F 128, 97 rows.  norm.weight is passed by pointer: a control."""
    TARGETS = ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm.weight")
    ENTRY = ("tf_ffn_fused_f32",)

    def __init__(self):
        super().__init__()
        self.linear1, self.linear2, self.norm = nn.Linear(256, 128), nn.Linear(128, 256), nn.LayerNorm(256)

    @staticmethod
    def inputs(g):
        return (torch.randn(97, 256, generator=g), torch.randn(97, 256, generator=g))

    def patches(self):
        return _min_rows_one()

    def forward(self, x, res):
        return _need(fused.ffn(x, self.linear1, self.linear2, self.norm, res), "fused.ffn")


class LinearLnC(Consumer):
    """fused.linear_residual_norm (tf_linear_res_ln_f32): D 256, 97 rows.  norm.weight: a control."""
    TARGETS = ("linear.weight", "linear.bias", "norm.weight")
    ENTRY = ("tf_linear_res_ln_f32",)

    def __init__(self):
        super().__init__()
        self.linear, self.norm = nn.Linear(256, 256), nn.LayerNorm(256)

    @staticmethod
    def inputs(g):
        return (torch.randn(97, 256, generator=g), torch.randn(97, 256, generator=g))

    def patches(self):
        return _min_rows_one()

    def forward(self, x, res):
        return _need(fused.linear_residual_norm(x, self.linear, res, self.norm), "fused.linear_residual_norm")


class StemDirectC(Consumer):
    """fused.stem_conv on a parameter: _stem_packed's own key.  Image 1 x 3 x 9 x 7."""
    TARGETS = ("conv1.weight",)
    ENTRY = ("tf_stem_conv7x7_f32",)

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)

    @staticmethod
    def inputs(g):
        return (torch.randn(1, 3, 9, 7, generator=g),)

    def forward(self, x):
        return _need(fused.stem_conv(x, self.conv1.weight, None, relu=True), "fused.stem_conv")


class StemC(StemDirectC):
    """The backbone's stem: conv1 + FrozenBN folded by _FoldCache, the packed image cached on the folded weight."""
    TARGETS = ("conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var")

    def __init__(self):
        super().__init__()
        self.bn1, self.maxpool, self._fold = backbone.FrozenBatchNorm2d(64), nn.MaxPool2d(3, 2, 1), backbone._FoldCache()

    def forward(self, x):
        return _need(backbone._stem_pooled(x, self.conv1, self.bn1, self.maxpool, self._fold), "backbone._stem_pooled")


class BottleneckC(Consumer):
    """One ResNet bottleneck with a downsample branch through _FoldCache: 256 -> 64 (1 x 1) -> 64 (3 x 3) -> 256 (1 x 1 + residual) at
    5 x 3 pixels -- the smallest 1 x 1 and 3 x 3 entries of CONV in tests/test_split_product_gpu.py.  All five sources of a fold."""
    TARGETS = ("block.conv2.weight", "block.bn2.weight", "block.bn2.bias", "block.bn2.running_mean", "block.bn2.running_var",
               "block.conv1.weight", "block.bn1.running_var", "block.conv3.weight", "block.bn3.bias",
               "block.downsample.0.weight", "block.downsample.1.running_mean")
    ENTRY = ("tf_conv_packed_f32", "tf_conv3x3_split_f32", "tf_conv3x3_splitk_f32")

    def __init__(self):
        super().__init__()
        down = nn.Sequential(nn.Conv2d(256, 256, 1, bias=False), backbone.FrozenBatchNorm2d(256))
        self.block = backbone.Bottleneck(256, 64, 1, down)

    @staticmethod
    def inputs(g):
        return (torch.randn(1, 256, 5, 3, generator=g).contiguous(memory_format=torch.channels_last),)

    def forward(self, x):
        return self.block(x)


class InputProj1x1C(Consumer):
    """fused.input_proj_1x1, the 1 x 1 form (_tf_w2d) with its GroupNorm (gn.weight by pointer: a control)."""
    TARGETS = ("conv.weight", "conv.bias", "gn.weight")
    ENTRY = ("tf_linear_split_f32", "tf_conv1x1_splitk_f32", "tf_conv_packed_f32")
    KS = 1

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(64, 64, 1) if self.KS == 1 else nn.Conv2d(64, 64, 3, 2, 1)
        self.gn = nn.GroupNorm(32, 64)

    @staticmethod
    def inputs(g):
        return (torch.randn(1, 64, 5, 7, generator=g).contiguous(memory_format=torch.channels_last),)

    def forward(self, x):
        return _need(fused.input_proj_1x1(x, self.conv, self.gn), "fused.input_proj_1x1")


class InputProj3x3C(InputProj1x1C):
    """... and the extra pyramid level's 3 x 3 / stride-2 form (_tf_wtaps)."""
    ENTRY = ("tf_conv_packed_f32", "tf_conv3x3_split_f32", "tf_conv3x3_splitk_f32")
    KS = 3


class MaskHeadC(Consumer):
    """MaskHeadSmallConv at the shape of tests/test_emu_model_path.py (B 1, Q 3, 5 x 7): _tf_taps (lay2 .. lay5), _tf_taps_part (lay1's
    image part), _tf_c1_taps (out_lay's weight AND its bias, kept as a Python float)."""
    TARGETS = ("head.lay3.weight", "head.lay1.weight", "head.out_lay.weight", "head.out_lay.bias", "head.lay2.weight")
    ENTRY = ("tf_groupnorm_relu_conv3x3_c1_nhwc_f32",)

    def __init__(self):
        super().__init__()
        self.head = ds.MaskHeadSmallConv(264, [1024, 512, 256], 256)

    @staticmethod
    def inputs(g):
        h, w = 5, 7
        return (torch.randn(1, 256, h, w, generator=g), torch.rand(1, 3, 8, h, w, generator=g),
                torch.randn(1, 1024, 2 * h, 2 * w, generator=g) * 0.3, torch.randn(1, 512, 4 * h, 4 * w, generator=g) * 0.3,
                torch.randn(1, 256, 8 * h, 8 * w, generator=g) * 0.3)

    def forward(self, x, bm, f0, f1, f2):
        return self.head(x, bm, [f0, f1, f2])


class MsdaC(Consumer):
    """The MSDeformAttn module: d_model 256, 8 heads, 2 levels of 12 x 16 and 6 x 8 -- _CatProjection's four sources, value_proj and
    output_proj."""
    TARGETS = ("attn.sampling_offsets.weight", "attn.sampling_offsets.bias", "attn.attention_weights.weight",
               "attn.attention_weights.bias", "attn.value_proj.weight", "attn.output_proj.weight")
    ENTRY = ("tf_msda_forward_fused_f32",)
    SHAPES = ((12, 16), (6, 8))

    def __init__(self):
        super().__init__()
        self.attn = msda.MSDeformAttn(256, n_levels=2, n_heads=8, n_points=4)

    @classmethod
    def inputs(cls, g):
        s = sum(h * w for h, w in cls.SHAPES)
        return (torch.randn(1, 40, 256, generator=g), torch.rand(1, 40, 2, 2, generator=g), torch.randn(1, s, 256, generator=g))

    def forward(self, query, ref, flat):
        shapes = msda.attach_host_shapes(torch.tensor(self.SHAPES, dtype=torch.long, device=query.device), self.SHAPES)
        return self.attn(query, ref, flat, shapes)


def _small_transformer():
    return dt.DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=64,
                                    dropout=0.0, num_feature_levels=2)


class RefPointsC(Consumer):
    """DeformableTransformer._object_reference_points: kept until the query parameter or the Linear behind it changes."""
    TARGETS = ("query.weight", "tr.reference_points.weight", "tr.reference_points.bias")
    NEEDS_LIBRARY = False

    def __init__(self):
        super().__init__()
        self.tr, self.query = _small_transformer(), nn.Embedding(7, 512)

    @staticmethod
    def inputs(g):
        return ()

    def forward(self):
        qp = self.query.weight
        qe = torch.split(qp, 256, dim=1)[0].unsqueeze(0).expand(1, -1, -1)
        return self.tr._object_reference_points(qp, qe, 1)


class LevelPosC(Consumer):
    """DeformableTransformer._level_position_embedding on per-geometry position tensors: kept until level_embed changes."""
    TARGETS = ("tr.level_embed",)
    NEEDS_LIBRARY = False

    def __init__(self):
        super().__init__()
        self.tr = _small_transformer()

    @staticmethod
    def inputs(g):
        pos = [torch.randn(1, 256, 3, 4, generator=g), torch.randn(1, 256, 2, 2, generator=g)]
        return tuple(pos)

    def forward(self, p0, p1):
        for p in (p0, p1):
            p._tf_cached_geometry = True   # what position_encoding.py marks its cached tensors with
        return self.tr._level_position_embedding([p0, p1])


CONSUMERS = [LinearC, LinearRowsC, PackedLinearC, LinearAddC, FfnC, LinearLnC, StemDirectC, StemC, BottleneckC, InputProj1x1C,
             InputProj3x3C, MaskHeadC, MsdaC, RefPointsC, LevelPosC]


def _is_buffer(target):
    """FrozenBatchNorm2d keeps its four tensors as buffers: no optimiser steps them."""
    parts = target.split(".")
    return parts[-2].startswith("bn") or parts[-3:-1] == ["downsample", "1"]


def matrix():
    """(consumer, target, class, mutation id, mutation): every (consumer, target) pair meets one mutation of EACH class, and the pairs
    walk through the table so that every mutation meets several consumers (the full table x both split products is run on
    _split_weight itself, tests/test_weight_coherence_cpu.py (a))."""
    rows, i = [], 0
    for c in CONSUMERS:
        for target in c.TARGETS:
            for cls, table in MUTATIONS.items():
                turn = [table[(i + step) % len(table)] for step in range(len(table))]
                mid, fn, _ = next(row for row in turn if not (row[2] and _is_buffer(target)))
                rows.append((c, target, cls, mid, fn))
            i += 1
    return rows


def matrix_ids(rows):
    return ["%s-%s-%s:%s" % (c.__name__, t, cls, mid) for c, t, cls, mid, _ in rows]


# ----------------------------------------------------------------------------------------------------------------------- harness
def make(consumer, device="cpu", seed=1):
    return randomize(consumer(), seed).to(device)


def cold_twin(consumer, warm, device="cpu"):
    """The same values in a newly constructed module that has never run."""
    twin = consumer().to(device).eval()
    twin.load_state_dict({k: v.detach().clone() for k, v in warm.state_dict().items()})
    return twin


def run(m, inputs):
    with torch.no_grad(), m.patches():
        y = m(*inputs)
    return [t.detach().clone() for t in _tensors(y)]


def check(consumer, target, mutation, device="cpu", seed=1):
    """Warm the consumer, change `target` by `mutation`, run again: the output must have moved, and must equal the cold twin's bit for
    bit.  DEEPCOPY: the warmed module is copied, the copy is changed in place; the copy answers like ITS twin and the original
    still answers as before (and like its own twin)."""
    g = torch.Generator().manual_seed(100 + seed)
    inputs = tuple(t.to(device) for t in consumer.inputs(g))
    warm = make(consumer, device, seed)
    before = run(warm, inputs)
    subject = warm
    if mutation is DEEPCOPY:
        subject = copy.deepcopy(warm)
        mut_inplace(subject, target)
    else:
        mutation(warm, target)
    after = run(subject, inputs)
    want = run(cold_twin(consumer, subject, device), inputs)
    assert bits_equal(after, want), "%s.%s after %s: the warm module and its cold twin differ (max |d| %.3g): a stale weight image" % (
        consumer.__name__, target, getattr(mutation, "__name__", mutation),
        max(float((a.double() - b.double()).abs().max()) for a, b in zip(after, want)))
    assert not bits_equal(after, before), "%s of %s.%s did not change the output: the case tests nothing" % (
        getattr(mutation, "__name__", mutation), consumer.__name__, target)
    if mutation is DEEPCOPY:
        again = run(warm, inputs)
        assert bits_equal(again, before), "changing a deep copy changed what the ORIGINAL %s computes" % consumer.__name__
        assert bits_equal(again, run(cold_twin(consumer, warm, device), inputs))
