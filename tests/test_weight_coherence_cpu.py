"""CPU: are the kernels handed the CURRENT weights?  The float64 suites build their operands fresh for every call; the inference path
reads cached images of the parameters (tests/util_weight_coherence.py), and a stale image gives a finite, plausible result.
  (a) fused._split_weight on CPU tensors: every mutation of the table x both split products, against the pieces of a clone;
  (b) changes of device / dtype, at the cache functions only (no kernel is launched with what they return);
  (c) every cached route through the SIMT emulator's build of the kernels: warm module against its cold twin, bit for bit; one
      whole-model case (cfg 2: load_state_dict of perturbed weights);
  (d) fused.route_epoch() moves if and only if a process-wide switch changes value;
  (e) _reset_parameters() of a model that has already run (emulator) -- with (c)'s whole model."""
import copy
import inspect

import pytest
import torch
from torch import nn

from tests import emu_lib, util_models as um, util_weight_coherence as wc
from tests.util_emu_gpu_path import gpu_path_on_emulator
from trackformer_amd import backbone, config, factory, fused, msda
from trackformer_amd import detr_segmentation as ds

needs_emulator = pytest.mark.skipif(not emu_lib.available(), reason="needs a host clang++ (ROCm's llvm) to build the emulated library")


@pytest.fixture()
def emulator():
    with gpu_path_on_emulator() as lib:
        yield lib


@pytest.fixture(params=[6, 16], ids=["six_terms", "fp16_pieces"])
def terms(request):
    prev = fused.set_split_terms(request.param)
    yield request.param
    fused.set_split_terms(prev)


# ------------------------------------------------------------------------------------------------------------------------- (a)
def _pieces(w):
    return [p.clone() for p in fused._split_weight(w) if p is not None]


@pytest.mark.parametrize("mid,mutation", [(m[0], m[1]) for m in wc.ALL_MUTATIONS], ids=[m[0] for m in wc.ALL_MUTATIONS])
def test_split_weight_pieces_follow_every_mutation(terms, mid, mutation):
    """The 16-bit pieces of a weight whose pieces were already cached equal, after the mutation, the pieces of a clone of it (and
    differ from the ones before).  Keyed on the version counter alone this failed for p.data.mul_(), p.data.copy_-style writes,
    `p.data = t`, nn.init through .data and vector_to_parameters."""
    m = wc.randomize(nn.Linear(32, 8, bias=False), seed=3)
    before = _pieces(m.weight)
    subject = m
    if mutation is wc.DEEPCOPY:
        subject = copy.deepcopy(m)
        wc.mut_inplace(subject, "weight")
    else:
        mutation(m, "weight")
    after = _pieces(subject.weight)
    want = _pieces(subject.weight.detach().clone())
    assert not wc.bits_equal(after, before), "the mutation changed nothing"
    assert wc.bits_equal(after, want), "stale pieces after %s" % mid
    if mutation is wc.DEEPCOPY:
        assert wc.bits_equal(_pieces(m.weight), before)


def test_the_harness_rejects_a_cache_that_never_refreshes(emulator, monkeypatch):
    """The yardstick itself: with _split_weight answering every tensor with the first pieces it ever built for it, the warm module
    keeps computing with the old weight and check() must say so."""
    real, first = fused._split_weight, {}

    def frozen(weight):
        return first.setdefault(id(weight), (weight, real(weight)))[1]
    monkeypatch.setattr(fused, "_split_weight", frozen)
    with pytest.raises(AssertionError, match="stale weight image"):
        wc.check(wc.LinearC, "lin.weight", wc.mut_inplace)
    monkeypatch.setattr(fused, "_split_weight", real)
    wc.check(wc.LinearC, "lin.weight", wc.mut_inplace)


# ------------------------------------------------------------------------------------------------------------------------- (b)
def _bottleneck():
    down = nn.Sequential(nn.Conv2d(256, 256, 1, bias=False), backbone.FrozenBatchNorm2d(256))
    return wc.randomize(backbone.Bottleneck(256, 64, 1, down), seed=5)


def _fold_images(block):
    """The folded images of conv1 (1 x 1) and conv2 (3 x 3) as _conv_bn asks for them."""
    out = []
    for conv, bn, cache in ((block.conv1, block.bn1, block._folds[0]), (block.conv2, block.bn2, block._folds[1])):
        with torch.no_grad():
            out.append(cache.get(conv, bn))
            out.append(cache.weight2d if conv.kernel_size == (1, 1) else cache.weight_taps)
    return out


@pytest.mark.parametrize("move", ["to_float64", "to_meta", "data_to_float64"])
def test_fold_cache_follows_a_module_to_another_dtype_or_device(move):
    block = _bottleneck()
    warm = [t.clone() for t in _fold_images(block)]
    if move == "to_float64":
        block.to(torch.float64)
    elif move == "to_meta":
        block.to("meta")
    else:
        block.conv1.weight.data = block.conv1.weight.data.double() * 2
        block.bn1.double()
        block.conv2.weight.data = block.conv2.weight.data.double() * 2
        block.bn2.double()
    got = _fold_images(block)
    dev, dt_ = block.conv1.weight.device, block.conv1.weight.dtype
    assert all(t.device == dev and t.dtype == dt_ for t in got), [(t.device, t.dtype) for t in got]
    if move != "to_meta":
        twin = copy.deepcopy(block)
        twin._folds = [backbone._FoldCache() for _ in range(4)]
        assert wc.bits_equal(got, _fold_images(twin))
        if move == "data_to_float64":
            assert not any(torch.equal(a.double(), b) for a, b in zip(warm, got))


@pytest.mark.parametrize("move", ["to_float64", "to_meta", "data_other"])
def test_cat_projection_and_mask_head_taps_follow_a_move(move):
    attn = wc.randomize(msda.MSDeformAttn(256, n_levels=2, n_heads=8, n_points=4), seed=6)
    head = wc.randomize(ds.MaskHeadSmallConv(264, [1024, 512, 256], 256), seed=7)

    def images():
        with torch.no_grad():
            return list(attn._cat_proj.get(attn)) + [head._taps(head.lay2, 288), head._taps(head.lay3, 128), head._taps_part(0, 256)]
    warm = [t.clone() for t in images()]
    if move == "data_other":
        for p in (attn.sampling_offsets.weight, attn.attention_weights.bias, head.lay2.weight, head.lay3.weight, head.lay1.weight):
            p.data = p.data * 2 + 1
    else:
        for m in (attn, head):
            m.to(torch.float64 if move == "to_float64" else "meta")
    got = images()
    dev, dt_ = head.lay2.weight.device, head.lay2.weight.dtype
    assert all(t.device == dev and t.dtype == dt_ for t in got), [(t.device, t.dtype) for t in got]
    if move != "to_meta":
        with torch.no_grad():
            w = torch.cat([attn.sampling_offsets.weight, attn.attention_weights.weight], 0)
            b = torch.cat([attn.sampling_offsets.bias, attn.attention_weights.bias], 0)
            taps3 = head.lay3.weight.permute(0, 2, 3, 1).reshape(head.lay3.out_channels, -1)
            part = head.lay1.weight[:, :256].permute(0, 2, 3, 1).reshape(head.lay1.out_channels, -1)
        assert torch.equal(got[0], w) and torch.equal(got[1], b) and torch.equal(got[3], taps3) and torch.equal(got[4], part)
        assert torch.equal(got[2].view(-1, 3, 3, 288)[..., :264], head.lay2.weight.detach().permute(0, 2, 3, 1))
        assert (move == "to_float64") == torch.equal(warm[3].double(), got[3].double())


@pytest.mark.parametrize("move", ["to_float64", "data_to_float64", "data_other"])
def test_split_weight_follows_a_change_of_storage_or_dtype(terms, move):
    lin = wc.randomize(nn.Linear(32, 8, bias=False), seed=8)
    before = _pieces(lin.weight)
    if move == "to_float64":
        lin.to(torch.float64)
    elif move == "data_to_float64":
        lin.weight.data = lin.weight.data.double() * 3
    else:
        lin.weight.data = lin.weight.data * 3
    after = _pieces(lin.weight)
    assert wc.bits_equal(after, _pieces(lin.weight.detach().clone()))
    assert all(p.device == lin.weight.device for p in after)
    if move != "to_float64":
        assert not wc.bits_equal(after, before)


# ------------------------------------------------------------------------------------------------------------------------- (c)
_MATRIX = wc.matrix()


def test_the_matrix_uses_every_mutation_and_every_class_on_every_target():
    assert {r[3] for r in _MATRIX} == {mid for rows in wc.MUTATIONS.values() for mid, _, _ in rows}
    per_target = {}
    for c, target, cls, _, _ in _MATRIX:
        per_target.setdefault((c, target), set()).add(cls)
    assert all(v == {"V", "P", "U"} for v in per_target.values()) and len(per_target) == sum(len(c.TARGETS) for c in wc.CONSUMERS)


@needs_emulator
@pytest.mark.parametrize("consumer,target,cls,mid,mutation", _MATRIX, ids=wc.matrix_ids(_MATRIX))
def test_warm_module_equals_its_cold_twin_after_a_weight_change(emulator, consumer, target, cls, mid, mutation):
    wc.check(consumer, target, mutation)
    if consumer.NEEDS_LIBRARY:   # the cached route really ran (not a declined call answered by PyTorch)
        assert any(emulator.calls.get(name) for name in consumer.ENTRY), (consumer.ENTRY, dict(emulator.calls))


@needs_emulator
@pytest.mark.parametrize("consumer", [wc.LinearC, wc.LinearRowsC, wc.PackedLinearC, wc.FfnC, wc.BottleneckC], ids=lambda c: c.__name__)
def test_weight_change_reaches_the_six_term_product_too(emulator, consumer):
    prev = fused.set_split_terms(6)
    try:
        wc.check(consumer, consumer.TARGETS[0], wc.mut_data_assign)
        wc.check(consumer, consumer.TARGETS[0], wc.mut_data_write_then_tell)
    finally:
        fused.set_split_terms(prev)


def _perturbed_state(model, scale=0.02):
    g = torch.Generator().manual_seed(17)
    sd = {}
    for k, v in model.state_dict().items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v * (1.0 + scale * torch.randn(v.shape, generator=g)) + scale * 0.1 * torch.randn(v.shape, generator=g)
            if k.endswith("running_var"):
                v = v.abs() + 1e-3
        sd[k] = v
    return sd


def _cfg2():
    model, post, args = um.build("cfg2_deformable_tracking", factory.build_model, config.make_args)
    model.tracking()
    return model, args


def _forward(model, img, target):
    with torch.no_grad():
        out, _, _, memory, hs = model(img, [dict(target[0])], None)
    return [t.clone() for t in wc._tensors([out["pred_logits"], out["pred_boxes"], hs])]


@needs_emulator
def test_whole_model_after_load_state_dict_and_after_reset_parameters(emulator):
    """cfg 2's test model, warmed on the emulated GPU path: (c) load_state_dict of perturbed weights, then (e) _reset_parameters() of
    the DeformableDETR, its DeformableTransformer and every MSDeformAttn -- each time the warm model answers like a cold twin loaded
    from its state_dict, bit for bit, and not like before."""
    prev = [(s, s(True)) for s in (fused.set_input_proj_fused, fused.set_box_refine_fused, fused.set_ffn_fused, fused.set_linear_ln_fused)]
    prev.append((fused.set_conv_stream, fused.set_conv_stream("all")))
    rows = fused._LINLN_MIN_ROWS, fused._FFN_FUSED_MIN_ROWS
    fused._LINLN_MIN_ROWS = fused._FFN_FUSED_MIN_ROWS = 1
    try:
        model, args = _cfg2()
        # (a frame of 64 x 96: two ResNet strides further it is 2 x 3 pixels -- every route of the model, a fraction of the emulator's time)
        g = torch.Generator().manual_seed(19)
        img = torch.randn(1, 3, 64, 96, generator=g)
        target = [{'track_query_hs_embeds': torch.randn(5, args.hidden_dim, generator=g),
                   'track_query_boxes': torch.rand(5, 4, generator=g) * 0.5 + 0.2, 'image_id': torch.tensor([1])}]
        y0 = _forward(model, img, target)
        assert emulator.calls.get("tf_ffn_fused_f32") and emulator.calls.get("tf_conv_packed_f32") and emulator.calls.get("tf_stem_conv7x7_f32")
        model.load_state_dict(_perturbed_state(model))
        y1 = _forward(model, img, target)
        twin, _ = _cfg2()
        twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
        assert not wc.bits_equal(y1, y0)
        assert wc.bits_equal(y1, _forward(twin, img, target)), "stale weight image after load_state_dict"
        torch.manual_seed(23)
        model.transformer._reset_parameters()   # (calls every MSDeformAttn's; the order of the construction: the heads come last)
        model._reset_parameters()
        y2 = _forward(model, img, target)
        twin, _ = _cfg2()
        twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
        assert not wc.bits_equal(y2, y1)
        assert wc.bits_equal(y2, _forward(twin, img, target)), "stale weight image after _reset_parameters()"
    finally:
        fused._LINLN_MIN_ROWS, fused._FFN_FUSED_MIN_ROWS = rows
        for setter, value in prev:
            setter(value)


# ------------------------------------------------------------------------------------------------------------------------- (e)
@needs_emulator
def test_reset_parameters_of_a_warmed_msdeformattn_is_noticed(emulator):
    def reset(m, _name):
        torch.manual_seed(29)
        m.attn._reset_parameters()
        with torch.no_grad():   # (the reference's initialisation zeroes both query projections: give the output something to show)
            m.attn.sampling_offsets.weight.add_(wc._wave(m.attn.sampling_offsets.weight))
    wc.check(wc.MsdaC, "attn.value_proj.weight", reset)


def test_reset_parameters_keep_their_values_and_write_through_the_parameter():
    """The initialisers were rewritten from `.data` writes to no_grad writes on the parameter: same values for the same seed as the
    reference's formulation, and every parameter they touch shows it on its version counter."""
    torch.manual_seed(31)
    attn = msda.MSDeformAttn(256, n_levels=2, n_heads=8, n_points=4)
    torch.manual_seed(31)
    ref = msda.MSDeformAttn(256, n_levels=2, n_heads=8, n_points=4)
    torch.manual_seed(37)
    nn.init.constant_(ref.sampling_offsets.weight.data, 0.)
    nn.init.constant_(ref.attention_weights.weight.data, 0.)
    nn.init.constant_(ref.attention_weights.bias.data, 0.)
    nn.init.xavier_uniform_(ref.value_proj.weight.data)
    nn.init.constant_(ref.value_proj.bias.data, 0.)
    nn.init.xavier_uniform_(ref.output_proj.weight.data)
    nn.init.constant_(ref.output_proj.bias.data, 0.)
    versions = {k: v._version for k, v in attn.named_parameters()}
    bias = attn.sampling_offsets.bias
    torch.manual_seed(37)
    attn._reset_parameters()
    for (k, a), (_, b) in zip(attn.named_parameters(), ref.named_parameters()):
        assert torch.equal(a, b), k
        assert a._version > versions[k] or (k == "sampling_offsets.bias" and a is not bias), k
    grid = attn.sampling_offsets.bias.view(8, 2, 4, 2)
    assert torch.equal(grid[0, 0, :, 0], -torch.arange(1., 5.)) and torch.equal(grid[7, 1, :, 1], torch.arange(1., 5.))
    model, _ = _cfg2()
    before = {k: v._version for k, v in model.named_parameters()}
    model.transformer._reset_parameters()
    model._reset_parameters()
    touched = [k for k, v in model.named_parameters() if v._version > before[k]]
    assert any(k.startswith("class_embed") for k in touched) and any("bbox_embed" in k for k in touched)
    assert any(k.startswith("input_proj") for k in touched) and "transformer.reference_points.weight" in touched
    p = 0.01
    import math
    assert all(torch.equal(h.bias, torch.full_like(h.bias, -math.log((1 - p) / p))) for h in model.class_embed)
    last = model.bbox_embed[0].layers[-1]
    assert float(last.weight.detach().abs().max()) == 0 and last.bias.tolist() == [0.0, 0.0, -2.0, -2.0]
    if model.with_box_refine:
        assert all(b.layers[-1].bias.tolist() == [0.0] * 4 for b in list(model.bbox_embed)[1:])


# ------------------------------------------------------------------------------------------------------------------------- (d)
def _switches():
    """Every public set_* of fused and backbone, with a value other than the current one (-> args), found by introspection."""
    out = []
    for mod in (fused, backbone):
        for name, fn in sorted(vars(mod).items()):
            if name.startswith("set_") and inspect.isfunction(fn) and fn.__module__ == mod.__name__:
                out.append((mod, name))
    return out


_OTHER = {   # current value -> a different one, for the switches that are not booleans
    "set_split_terms": lambda cur: (6 if cur == 16 else 16,),
    "set_conv_stream": lambda cur: (False if cur else "all",),
    "set_conv_ksplit_policy": lambda cur: tuple(v + 1 for v in cur),
    "set_conv_split_skip": lambda cur: ([(64, 64, 3, 1)] if not cur else [],),
}


@pytest.mark.parametrize("mod,name", _switches(), ids=["%s.%s" % (m.__name__.split(".")[-1], n) for m, n in _switches()])
def test_route_epoch_moves_if_and_only_if_a_switch_changes_value(mod, name):
    setter = getattr(mod, name)
    keep_train = fused._split_linear_train
    e0 = fused.route_epoch()
    cur = setter(*_probe_args(name, setter))            # learn the current value: every setter returns the previous one
    try:
        back = cur if isinstance(cur, tuple) and name == "set_conv_ksplit_policy" else (cur,)
        setter(*back)
        e1 = fused.route_epoch()
        other = _OTHER[name](cur) if name in _OTHER else (not cur,)
        assert setter(*other) == cur
        assert fused.route_epoch() == e1 + 1, "%s: a changed value must move route_epoch()" % name
        setter(*other)
        setter(*other)
        assert fused.route_epoch() == e1 + 1, "%s: setting the value it already has must not move route_epoch()" % name
        setter(*back)
        assert fused.route_epoch() == e1 + 2
    finally:
        setter(*back)
        fused._split_linear_train = keep_train
    assert e1 - e0 in (0, 2)   # (the probe itself: there and back, or nothing)


def _probe_args(name, setter):
    if name == "set_conv_ksplit_policy":
        return fused._KSPLIT_POLICY
    if name == "set_split_terms":
        return (fused.split_terms(),)
    if name == "set_conv_split_skip":
        return (backbone._conv_split_skip,)
    if name == "set_conv_stream":
        return ("all" if (fused._conv_stream and fused._CONV_STREAM_ALL) else fused._conv_stream,)
    return (True,)


def test_the_switch_list_is_the_one_the_issue_names():
    names = {n for _, n in _switches()}
    assert {"set_split_terms", "set_split_linear", "set_packed_linear", "set_ffn_fused", "set_linear_ln_fused", "set_stem_pool_fused",
            "set_stem_conv_split", "set_heads_split", "set_pos_add_fused", "set_conv_stream", "set_conv_ksplit_policy",
            "set_conv1x1_splitk", "set_conv_halo", "set_input_proj_fused", "set_box_refine_fused", "set_postprocess_fused",
            "set_check_finite", "set_conv1x1_split", "set_conv3x3_split", "set_conv_split_skip"} <= names


def test_weights_changed_moves_the_weight_epoch_and_every_key():
    w = torch.randn(8, 32)
    k0, e0 = fused.source_key(w), fused.weight_epoch()
    assert fused.source_key(w) == k0 and fused.source_key(None) is None
    assert fused.weights_changed() == e0 + 1 == fused.weight_epoch()
    assert fused.source_key(w) != k0
    assert fused.weights_changed.__doc__ and ".data" in fused.weights_changed.__doc__


# ------------------------------------------------------------------------------------------- GraphedDetector, host side (no GPU)
class _Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(4, 4)
        self.register_buffer("stat", torch.ones(4))


@pytest.fixture()
def no_device(monkeypatch):
    """Dropping graphs waits for the device first; the stand-in graphs below have none."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)


def _wrapper_with_a_graph(model):
    from trackformer_amd.graphed import GraphedDetector
    det = GraphedDetector(model)
    det._sync_epoch()                 # the first call after construction takes the fingerprint
    det._graphs["key"] = object()     # stands for a captured graph (never replayed here)
    return det


@pytest.mark.parametrize("change", ["nothing", "load_state_dict", "weights_changed", "switch"])
def test_graphed_detector_compares_epochs_on_every_call(change, no_device):
    model = _Toy()
    det = _wrapper_with_a_graph(model)
    if change == "load_state_dict":
        model.load_state_dict({k: v.clone() + 1 for k, v in model.state_dict().items()})
    elif change == "weights_changed":
        model.lin.weight.data.mul_(2)
        fused.weights_changed()
    elif change == "switch":
        prev = fused.set_split_terms(6 if fused.split_terms() == 16 else 16)
    try:
        det._sync_epoch()
    finally:
        if change == "switch":
            fused.set_split_terms(prev)
    assert len(det._graphs) == (1 if change == "nothing" else 0)


@pytest.mark.parametrize("change", ["nothing", "inplace", "optimizer", "data_assign", "new_parameter", "buffer", "load_state_dict_assign"])
def test_revalidate_drops_the_graphs_when_any_parameter_or_buffer_changed(change, no_device):
    model = _Toy()
    det = _wrapper_with_a_graph(model)
    if change == "inplace":
        with torch.no_grad():
            model.lin.bias.add_(1)
    elif change == "optimizer":
        model.lin.weight.grad = torch.ones_like(model.lin.weight)
        torch.optim.SGD(model.parameters(), lr=0.1).step()
    elif change == "data_assign":
        model.lin.weight.data = model.lin.weight.data * 2
    elif change == "new_parameter":
        model.lin.weight = nn.Parameter(model.lin.weight.detach().clone())
    elif change == "buffer":
        model.stat.mul_(2)
    elif change == "load_state_dict_assign":
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(sd, assign=True)
        det._wepoch = fused.weight_epoch()   # (isolate revalidate(): the hook of load_state_dict is tested above)
    det._sync_epoch()
    assert len(det._graphs) == 1          # a call alone does no host work on the weights: it cannot know ...
    assert det.revalidate() == (change == "nothing")
    assert len(det._graphs) == (1 if change == "nothing" else 0)   # ... revalidate() does
    assert det.revalidate()               # and the new state is the reference from now on


def test_one_load_state_dict_hook_per_model_however_many_wrappers():
    from trackformer_amd.graphed import GraphedDetector
    model = _Toy()
    for _ in range(3):
        GraphedDetector(model)
    assert len(model._load_state_dict_post_hooks) == 1
    e = fused.weight_epoch()
    model.load_state_dict(model.state_dict())
    assert fused.weight_epoch() == e + 1
