"""One training step of the small model of tests/util_models.py, gradient tensor by gradient tensor, against float64.

tests/util_models.train_step reduces every gradient to its L2 norm and compare_train_to_golden looks at 13 of the 184 norms at
rtol 2e-3: a gradient with x and y swapped, heads permuted, a transposed block, the gradient of another layer of the same shape
or a scale error below 0.2 % passes, and so does anything wrong in the other 171 parameters.  This module compares EVERY gradient
tensor of a step, element-wise, with the same step in float64:

    reference_step(masks, train)   model.double() on the CPU with oracle/msda_grid_sample.py (pure torch: F.grid_sample, shares no
                                   code with the kernels or the host operator) patched in as the operator;
    yardstick(masks, train)        the same step in fp32 on the CPU (module graph, the same grid-sample operator, no native code):
                                   what a correct fp32 implementation of the step differs from float64 by -- per class of
                                   parameters, the worst of the class;
    compare(step, ref, yard)       every parameter: rel. L2 error and largest element error (relative to max |g64|) at most
                                   FP32_FACTOR x the yardstick of its class; every loss: the same against the fp32 CPU step's loss
                                   error; the set of names equal to the reference's; and -- asserted, never skipped -- the
                                   matcher's assignments of every decoder output and the track-query bookkeeping equal to the
                                   reference's (otherwise two different loss functions would be compared);

    reference_for(step, ...)       the float64 step EVALUATED ON THE STEP'S SIDE OF EVERY KINK: see that function.  The loss is not
                                   differentiable where a ReLU's pre-activation is zero; float64 puts ~1 unit in 25 000 within fp32
                                   round-off of zero, an fp32 run decides those either way, and ONE such decision moves every
                                   gradient upstream of it by ~1e-4 (the product's host path turns a unit of encoder layer 1 with
                                   pre-activation 3.0e-7 that the fp32 grid-sample step does not turn; an MI355X step turns one in
                                   layer3 of the backbone).  The undetermined set comes from the float64 step alone; outside it the
                                   decisions must equal float64's -- asserted, like the assignments.

The bound.  FP32_FACTOR = 4.0 is the project's constant (util_msda_numerics, util_norm_attn_numerics, util_postproc_numerics,
util_split_numerics).  Where the yardstick is as good as exact the bound is CLASS_MIN = 2^-21, util_split_numerics.FP32_CLASS_MIN:
four units in the last place of fp32, which no chain of fp32 operations stays below by more than luck.  It only ever acts on
losses (the cardinality errors are integers and 0 in every run; a loss may round exactly on the CPU).

Measured on the CPU (x86-64, 8 threads).  Per class: the fp32 CPU step's worst rel. L2 (the yardstick), its best (the step's own
floor: how exact fp32 gets on the class's easiest tensor) and the worst element error relative to max |g64|:

    small model:
        backbone layer2        yardstick 1.60e-06   floor 7.10e-07   element 2.37e-06
        backbone layer3        yardstick 1.20e-06   floor 6.05e-07   element 1.36e-06
        backbone layer4        yardstick 8.31e-07   floor 6.14e-07   element 8.72e-07
        input_proj             yardstick 8.47e-07   floor 3.70e-07   element 7.74e-07
        encoder                yardstick 5.03e-06   floor 1.57e-07   element 1.11e-05
        decoder                yardstick 2.28e-06   floor 1.26e-07   element 1.62e-06
        heads and embeddings   yardstick 2.10e-06   floor 1.03e-07   element 2.26e-06
        losses: worst error 1.23e-07
    mask model: the same to two digits, and
        mask head              yardstick 1.47e-06   floor 5.49e-08   element 1.79e-06
    eval mode with gradients: the figures of the small model; TRACK_QUERY_SEED: 9.7e-07 / 1.0e-06 / 8.4e-07 / 7.3e-07 / 1.7e-06 /
    2.4e-06 / 2.2e-06, losses 2.1e-07.

Every yardstick lies above CLASS_MIN and every floor within a factor 8 of it (asserted by tests/test_train_gradients_cpu.py).
Before the ReLU decisions were taken out the layer2 yardstick was 7.3e-04 (one decision of the CPU step at a 16 x 20 map).

Measured on an MI355X (profiles/train_step_gradients_gpu_first_run.txt holds the runs): worst rel. L2 of the class as a multiple of
its yardstick (the bound is 4), and how many undetermined decisions the route took the other way (none outside the set, ever):

    route (worst rel. L2 / yardstick) flips    layer2    layer3    layer4   in_proj   encoder   decoder     heads   mask hd
    default                              0      0.72      0.94      0.92      0.82      0.28      0.92      1.25         -
    deterministic_backward               1      0.64      0.91      0.96      0.75      0.28      1.03      1.64         -
    fused_training                       1      0.61      0.99      0.92      0.85      0.34      0.86      0.85         -
    fused_training_deterministic         0      0.65      0.92      0.87      0.73      0.28      0.93      0.89         -
    split_linear_three_terms             2      0.59      0.90      0.84      0.65      0.31      0.87      0.97         -
    split_linear_six_terms               3      0.54      1.09      1.00      0.77      0.35      0.85      0.95         -
    all_on                               1      0.58      0.86      0.83      0.70      0.25      0.84      1.01         -
    reference_formulations               0      1.04      1.21      1.04      0.98      1.00      0.97      1.29         -
    eval_mode_with_gradients_all_on      1      0.73      1.00      0.93      0.76      0.31      0.90      1.10         -
    mask_model_default                   1      0.47      1.03      1.01      0.87      0.27      0.89      0.90      0.63
    mask_model_all_on                    1      0.65      0.95      0.89      0.72      0.22      0.84      0.89      0.53
    track_queries_default                1      1.00      0.92      0.90      0.97      1.12      0.85      1.01         -
    track_queries_all_on                 0      0.89      0.79      0.82      0.86      0.73      0.76      0.75         -

    two steps with every switch on and the convolution library's deterministic solvers: all 184 gradients bit-identical.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import msda_grid_sample
from tests import util_models as um

FP32_FACTOR = 4.0
CLASS_MIN = 2.0 ** -21
TRACK_QUERY_SEED = 2     # host-RNG seed under which the augmentation appends track queries (util_models' own seed, 7, draws none)

CLASSES = ("backbone layer2", "backbone layer3", "backbone layer4", "input_proj", "encoder", "decoder", "heads and embeddings",
           "mask head")
_HEAD_MARKS = ("class_embed", "bbox_embed", "query_embed", "level_embed", "reference_points")


def class_of(name):
    """The class whose yardstick bounds this parameter.  Every name must have one: a new kind of parameter is an error, not a pass."""
    for k in (2, 3, 4):
        if name.startswith("backbone.0.body.layer%d." % k):
            return "backbone layer%d" % k
    if any(m in name for m in _HEAD_MARKS):      # (bbox_embed / class_embed are registered below transformer.decoder too)
        return "heads and embeddings"
    if name.startswith("input_proj."):
        return "input_proj"
    if name.startswith("transformer.encoder."):
        return "encoder"
    if name.startswith("transformer.decoder."):
        return "decoder"
    if name.startswith("bbox_attention.") or name.startswith("mask_head."):
        return "mask head"
    raise KeyError("no gradient class for parameter %r" % name)


class Step:
    """What one step leaves: losses {name: float}, total, grads {name: tensor on the CPU}, matches (every assignment the matcher
    made, in call order: previous frame, then final + auxiliary decoder outputs), bookkeeping (the augmented track-query fields of
    the targets)."""

    def __init__(self, losses, total, grads, matches, bookkeeping, relu=None, undetermined=None, margins=None):
        self.losses, self.total, self.grads, self.matches, self.bookkeeping = losses, total, grads, matches, bookkeeping
        self.relu = relu                     # per feed-forward block, in call order: which hidden units are on [N, Lq, d_ffn] (bool)
        self.undetermined = undetermined     # (float64 only) which of them lie within fp32 round-off of zero
        self.margins = margins               # (float64 only) |z| / (|x| . |w|^T + |b|) of every unit
        self.matters = None                  # (float64 only) which units a non-zero gradient reaches

    def with_grads(self, grads):
        other = Step(self.losses, self.total, grads, self.matches, self.bookkeeping, self.relu, self.undetermined, self.margins)
        other.matters = self.matters
        return other

    def norms(self):
        return {n: float(g.double().norm()) for n, g in self.grads.items()}


def _record_matcher(matcher, log):
    """Every match_many result of this matcher instance goes to `log` (forward() calls match_many); returns the undo function."""
    orig = matcher.match_many

    def recording(outputs_list, targets):
        result = orig(outputs_list, targets)
        for per_set in result:
            log.append([(i.tolist(), j.tolist()) for i, j in per_set])
        return result
    matcher.__dict__["match_many"] = recording
    return lambda: matcher.__dict__.pop("match_many", None)


_BOOK_KEYS = ("track_query_match_ids", "track_queries_mask", "track_queries_fal_pos_mask")
UNDETERMINED = 4 * 2.0 ** -20     # |z| <= this * (|x| . |w|^T + |b|): the sign of an fp32-class pre-activation z is not determined
#                                   (util_split_numerics.BOUND, the forward's own bound, with the factor tests/test_linear_backward_gpu.py
#                                   uses for the same purpose)


class _Decisions:
    """The ReLU decisions of one step that a gradient passes through, site by site in call order: the trainable bottlenecks of the
    backbone (layer2-4: three per block, backbone._conv_bn) and the feed-forward blocks of the transformer
    (deformable_transformer._ffn_hidden).  A run under test only records them (from the product's own output: y > 0).  The float64
    step computes the site itself -- the same arithmetic as the module graph -- and records besides: which units are undetermined
    (|z| <= UNDETERMINED * sum |x w|), their margins, and which units the loss depends on at all (a non-zero gradient arrives: the
    padded tokens of the second image get none, and their position encoding -- sin / cos of -pi * 1e6 in rows without a valid
    pixel -- is round-off in every precision); the units listed in `flips` [(site, flat index)] take the OTHER side of the kink."""

    def __init__(self, float64_flips):
        self.float64 = float64_flips is not None
        self.flips = float64_flips or ()
        self.relu, self.undetermined, self.margins, self.matters = [], [], [], {}

    def record(self, y):
        self.relu.append((y.detach() > 0).cpu())
        return y

    def decide(self, z, scale):
        site = len(self.relu)
        on = z.detach() > 0
        self.undetermined.append(z.detach().abs() <= UNDETERMINED * scale)
        self.margins.append((z.detach().abs() / scale).float())
        mine = [i for b, i in self.flips if b == site]
        if mine:
            on = on.clone()
            on.view(-1)[mine] = ~on.view(-1)[mine]
        self.relu.append(on)
        y = z * on
        y.register_hook(lambda g: self.matters.__setitem__(site, g != 0))
        return y

    def patch(self):
        from trackformer_amd import backbone as bb
        from trackformer_amd import deformable_transformer as dt
        orig_ffn, orig_conv = dt._ffn_hidden, bb._conv_bn

        def ffn_hidden(linear, activation, x, inference):
            if not torch.is_grad_enabled() or activation is not F.relu:
                return orig_ffn(linear, activation, x, inference)
            if not self.float64:
                return self.record(orig_ffn(linear, activation, x, inference))
            with torch.no_grad():
                scale = x.abs() @ linear.weight.abs().t() + linear.bias.abs()
            return self.decide(linear(x), scale)

        def conv_bn(x, conv, bn, cache, relu, fold, residual=None):
            if not (relu and torch.is_grad_enabled() and conv.weight.requires_grad):
                return orig_conv(x, conv, bn, cache, relu, fold, residual)
            if not self.float64:
                return self.record(orig_conv(x, conv, bn, cache, relu, fold, residual))
            z = bn(conv(x))                      # (the module graph, backbone._conv_bn's last branch)
            with torch.no_grad():
                w_scale, shift = bn.scale_shift()
                scale = F.conv2d(x.abs(), (conv.weight * w_scale.reshape(-1, 1, 1, 1)).abs(), None, conv.stride, conv.padding,
                                 conv.dilation, conv.groups) + shift.abs().reshape(1, -1, 1, 1)
            if residual is not None:
                z = z + residual
                scale = scale + residual.detach().abs()
            return self.decide(z, scale)
        dt._ffn_hidden, bb._conv_bn = ffn_hidden, conv_bn

        def undo():
            dt._ffn_hidden, bb._conv_bn = orig_ffn, orig_conv
        return undo


def run_step(model, criterion, samples, targets, train=True, rng_seed=7, _float64_flips=None):
    """tests/util_models.train_step's sequence (engine.train_step without the optimiser), keeping the gradient TENSORS, the matcher's
    assignments, the track-query bookkeeping and the ReLU decisions of the feed-forward blocks.  train=False: model.eval() with
    gradients enabled (gradient checks, saliency)."""
    model.train(train)
    criterion.train(train)
    model.zero_grad()
    torch.manual_seed(rng_seed)      # host RNG of the track-query augmentation
    prev_benchmark = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False       # (see util_models.train_step)
    matches, dec = [], _Decisions(_float64_flips)
    undo = [dec.patch()]
    for m in {id(m): m for m in (getattr(model, "_matcher", None), criterion.matcher) if m is not None}.values():
        undo.append(_record_matcher(m, matches))
    try:
        outputs, targets, *_ = model(samples, targets)
        loss_dict = criterion(outputs, targets)
        weight_dict = criterion.weight_dict
        total = sum(loss_dict[k] * weight_dict[k] for k in loss_dict.keys() if k in weight_dict)
        total.backward()
    finally:
        torch.backends.cudnn.benchmark = prev_benchmark
        for u in undo:
            u()
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
    book = [{k: t[k].tolist() for k in _BOOK_KEYS if k in t} | {"n_track_queries": int(t["track_query_hs_embeds"].shape[0])}
            for t in targets]
    step = Step({k: float(v.detach().double()) for k, v in loss_dict.items()}, float(total.detach().double()), grads, matches, book,
                dec.relu)
    if dec.float64:
        step.undetermined, step.margins = dec.undetermined, dec.margins
        step.matters = [dec.matters.get(i, torch.zeros_like(r)) for i, r in enumerate(dec.relu)]
    return step


def _to_dtype(obj, dtype):
    if torch.is_tensor(obj):
        return obj.to(dtype) if obj.is_floating_point() else obj
    if isinstance(obj, dict):
        return {k: _to_dtype(v, dtype) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_dtype(v, dtype) for v in obj)
    return obj


def _cpu_step(dtype, masks, train, flips=None, rng_seed=7):
    from trackformer_amd import config, factory, msda
    model, criterion, _ = um.build_train(factory.build_model, config.make_args, masks=masks)
    samples, targets = um.train_batch(masks=masks)
    if dtype == torch.float64:
        model, criterion = model.double(), criterion.double()
        samples, targets = _to_dtype(samples, dtype), _to_dtype(targets, dtype)
    prev = msda.MSDeformAttnFunction
    msda.MSDeformAttnFunction = msda_grid_sample.make_torch_function()
    try:
        return run_step(model, criterion, samples, targets, train=train, rng_seed=rng_seed, _float64_flips=flips)
    finally:
        msda.MSDeformAttnFunction = prev


@functools.lru_cache(maxsize=None)
def _reference_step(masks, train, flips, rng_seed):
    step = _cpu_step(torch.float64, masks, train, flips, rng_seed)
    assert all(g.dtype == torch.float64 for g in step.grads.values())
    return step


def reference_step(masks=False, train=True, flips=(), rng_seed=7):
    """The step in float64 on the CPU with the grid-sample operator.  Computed once per process and configuration; read-only.
    flips: see reference_for."""
    return _reference_step(bool(masks), bool(train), tuple(flips), int(rng_seed))


def relu_flips(step, ref):
    """[(site, flat index)] of the units the loss depends on that `step` decided differently from the float64 step `ref`, and how
    many of them lie OUTSIDE the undetermined set."""
    assert len(step.relu) == len(ref.relu) and len(ref.relu) > 0, (len(step.relu), len(ref.relu))
    flips, outside = [], 0
    for b, (mine, theirs, und, matters) in enumerate(zip(step.relu, ref.relu, ref.undetermined, ref.matters)):
        d = (mine != theirs).reshape(-1) & matters.reshape(-1)
        outside += int((d & ~und.reshape(-1)).sum())
        flips += [(b, int(i)) for i in d.nonzero()[:, 0]]
    return tuple(flips), outside


def reference_for(step, masks=False, train=True, rng_seed=7):
    """The float64 reference a step is compared with.  The loss is not differentiable where a ReLU's pre-activation is zero, and
    float64 puts a few units of every site (_Decisions: the trainable bottlenecks and the feed-forward blocks) so close to zero
    (|z| <= UNDETERMINED * sum |x w|: about 1 in 25 000) that an fp32 forward decides them either way; each such decision changes
    every gradient upstream of the site by ~1e-4 -- twenty to a hundred times the yardstick -- without either side being wrong.
    So: outside the undetermined set the step's decisions must EQUAL float64's wherever the loss depends on the unit (asserted,
    like the matcher's assignments); the undetermined units it decided the other way are evaluated on that side of the kink in
    float64 too -- same model, same operator, same arithmetic: the other one-sided derivative.  The set is computed from the
    float64 step alone, never from the step under test."""
    ref = reference_step(masks, train, (), rng_seed)
    flips, outside = relu_flips(step, ref)
    assert outside == 0, "%d ReLU decisions differ from float64 outside the undetermined set" % outside
    return reference_step(masks, train, flips, rng_seed) if flips else ref


def errors(grads, ref):
    """{name: (rel. L2 error, largest element error / max |g64|)} over the names both have."""
    out = {}
    for n, r in ref.grads.items():
        g = grads.get(n)
        if g is None or g.shape != r.shape:
            continue
        d = g.double() - r
        out[n] = (float(d.norm() / r.norm()), float(d.abs().max() / r.abs().max()))
    return out


def loss_errors(step, ref):
    out = {k: abs(step.losses[k] - v) / max(1.0, abs(v)) for k, v in ref.losses.items() if k in step.losses}
    out["total"] = abs(step.total - ref.total) / max(1.0, abs(ref.total))
    return out


def yardstick(masks=False, train=True, rng_seed=7):
    return _yardstick(bool(masks), bool(train), int(rng_seed))


@functools.lru_cache(maxsize=None)
def _yardstick(masks, train, rng_seed):
    """-> {"l2": {class: worst rel. L2 of the fp32 CPU step}, "max": {class: worst element error}, "floor": {class: its best rel. L2},
    "loss": {name: error}}.  The fp32 CPU step must itself satisfy the precondition (same assignments as float64)."""
    step = _cpu_step(torch.float32, masks, train, None, rng_seed)
    ref = reference_for(step, masks, train, rng_seed)
    assert sorted(step.grads) == sorted(ref.grads)
    assert step.matches == ref.matches and step.bookkeeping == ref.bookkeeping, "the fp32 CPU step matches differently from float64"
    yard = {"l2": {}, "max": {}, "floor": {}, "loss": loss_errors(step, ref)}
    for n, (l2, mx) in errors(step.grads, ref).items():
        c = class_of(n)
        yard["l2"][c] = max(yard["l2"].get(c, 0.0), l2)
        yard["max"][c] = max(yard["max"].get(c, 0.0), mx)
        yard["floor"][c] = min(yard["floor"].get(c, float("inf")), l2)
    return yard


class Report:
    def __init__(self):
        self.failures = []     # (what, name, value, bound)
        self.worst = {}        # class -> (rel. L2, name, largest element error, name)
        self.loss = {}         # name -> (error, bound)

    def __bool__(self):
        return not self.failures

    def failed(self, what=None, name=None):
        return [f for f in self.failures if (what is None or f[0] == what) and (name is None or f[1] == name)]

    def table(self, yard):
        rows = ["%-22s %11s %11s  %11s %11s  %s" % ("class", "yard L2", "worst L2", "yard max", "worst max", "worst parameter (L2)")]
        for c in CLASSES:
            if c in self.worst:
                l2, n_l2, mx, _ = self.worst[c]
                rows.append("%-22s %11.3e %11.3e  %11.3e %11.3e  %s" % (c, yard["l2"][c], l2, yard["max"][c], mx, n_l2))
        rows.append("losses: worst error %.3e (%s), its yardstick %.3e" % max(
            ((e, k, yard["loss"].get(k, 0.0)) for k, (e, _) in self.loss.items()), default=(0.0, "-", 0.0)))
        return "\n".join(rows)

    def assert_ok(self):
        assert not self.failures, "%d failures, first ones: %r" % (len(self.failures), self.failures[:8])


def compare(step, ref, yard):
    """-> Report.  Preconditions first (assignments, bookkeeping, the set of names), then every loss and every gradient tensor."""
    rep = Report()
    if step.matches != ref.matches:
        rep.failures.append(("matcher indices", None, None, None))
    if step.bookkeeping != ref.bookkeeping:
        rep.failures.append(("track-query bookkeeping", None, None, None))
    for n in sorted(set(ref.grads) - set(step.grads)):
        rep.failures.append(("missing gradient", n, None, None))
    for n in sorted(set(step.grads) - set(ref.grads)):
        rep.failures.append(("unexpected gradient", n, None, None))
    for k in sorted(set(ref.losses) ^ set(step.losses)):
        rep.failures.append(("loss names", k, None, None))
    for k, e in loss_errors(step, ref).items():
        bound = max(FP32_FACTOR * yard["loss"].get(k, 0.0), CLASS_MIN)
        rep.loss[k] = (e, bound)
        if not e <= bound:
            rep.failures.append(("loss", k, e, bound))
    for n in ref.grads:
        if n in step.grads and step.grads[n].shape != ref.grads[n].shape:
            rep.failures.append(("gradient shape", n, tuple(step.grads[n].shape), tuple(ref.grads[n].shape)))
    for n, (l2, mx) in errors(step.grads, ref).items():
        c = class_of(n)
        w = rep.worst.get(c, (-1.0, None, -1.0, None))
        rep.worst[c] = (l2, n, w[2], w[3]) if not l2 <= w[0] else w      # (NaN counts as worst)
        w = rep.worst[c]
        rep.worst[c] = (w[0], w[1], mx, n) if not mx <= w[2] else w
        b_l2, b_mx = max(FP32_FACTOR * yard["l2"][c], CLASS_MIN), max(FP32_FACTOR * yard["max"][c], CLASS_MIN)
        if not l2 <= b_l2:
            rep.failures.append(("rel L2", n, l2, b_l2))
        if not mx <= b_mx:
            rep.failures.append(("max element", n, mx, b_mx))
    return rep


# ------------------------------------------------------------------------------------------------ mutations of a passing gradient set
def _enc0(suffix):
    return "transformer.encoder.layers.0." + suffix


def mutate_xy_swap(grads, name=_enc0("self_attn.sampling_offsets.weight")):
    g = grads[name]
    out = dict(grads)
    out[name] = g.view(-1, 2, g.shape[1])[:, [1, 0]].reshape(g.shape).contiguous()
    return out, name


def mutate_heads_swapped(grads, name=_enc0("self_attn.value_proj.weight"), heads=8):
    g = grads[name].clone()
    d = g.shape[0] // heads
    g[:d], g[d:2 * d] = grads[name][d:2 * d], grads[name][:d]
    return dict(grads, **{name: g}), name


def mutate_block_transposed(grads, name=_enc0("linear1.weight"), at=(64, 32), size=32):
    g = grads[name].clone()
    r, c = at
    g[r:r + size, c:c + size] = grads[name][r:r + size, c:c + size].t()
    return dict(grads, **{name: g}), name


def mutate_split_shifted(grads, layer="transformer.decoder.layers.1.cross_attn."):
    a, b = layer + "sampling_offsets.weight", layer + "attention_weights.weight"
    cat = torch.roll(torch.cat([grads[a], grads[b]], 0), -1, 0)
    return dict(grads, **{a: cat[:grads[a].shape[0]].contiguous(), b: cat[grads[a].shape[0]:].contiguous()}), (a, b)


def mutate_layers_exchanged(grads):
    a, b = ("transformer.decoder.layers.%d.cross_attn.output_proj.weight" % i for i in (0, 1))
    return dict(grads, **{a: grads[b], b: grads[a]}), (a, b)


def mutate_scaled(grads, name="transformer.decoder.layers.2.linear2.weight", factor=1.001):
    return dict(grads, **{name: grads[name] * factor}), name


def mutate_missing(grads, name=_enc0("self_attn.output_proj.bias")):
    return {k: v for k, v in grads.items() if k != name}, name
