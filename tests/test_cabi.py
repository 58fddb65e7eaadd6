"""CPU: the C-ABI shared library loads and exports exactly what include/tf_msda.h and include/tf_fused.h declare, and the
binding read from those headers (_cabi.signatures / bind) gives every function the types the prototypes state;
argument validation works without a GPU (no compute is launched here)."""
import ctypes
import os
import re

import pytest

from trackformer_amd import _cabi, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build_all()
    return _cabi.lib()


def _declared_symbols():
    names = set()
    for header in sorted(os.listdir(os.path.join(REPO, "include"))):
        if not header.endswith(".h"):
            continue
        text = open(os.path.join(REPO, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names.update(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


def test_parser_finds_every_declared_name():
    """The binder's parse against the cruder, independent list above: it cannot silently skip a prototype."""
    assert sorted(_cabi.signatures()) == _declared_symbols()
    assert sorted(_cabi.EXPORTED_SYMBOLS) == _declared_symbols()
    assert len(set(_cabi.EXPORTED_SYMBOLS)) == len(_cabi.EXPORTED_SYMBOLS)


_VP, _CI, _I64, _CF = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
# Written by hand, one function of each kind: (restype, argtypes) as the hand-written binding had them.
PINNED = {
    "tf_msda_abi_version": (_CI, []),
    "tf_msda_strerror": (ctypes.c_char_p, [_CI]),
    "tf_msda_set_option": (_CI, [ctypes.c_char_p, _CI]),
    "tf_msda_debug_trace_buffer": (None, [_VP]),
    "tf_linear_packed_bytes": (_I64, [_CI, _CI, _CI]),
    "tf_groupnorm_nhwc_f32": (_CI, [_VP, _VP, _VP, _VP, _VP, _CI, _CI, _CI, _CI, _CF, _I64, _I64, _VP]),
    "tf_groupnorm_relu_conv3x3_c1_nhwc_f32": (_CI, [_VP, _VP, _VP, _VP, _CF, _VP, _VP, _CI, _CI, _CI, _CI, _CI, _CF, _VP]),
    "tf_dropout_keep_u8": (_CI, [_VP, _CF, _I64, _I64, _VP, _VP]),
    "tf_msda_backward_det_f32": (_CI, [_VP] * 9 + [_I64] + [_CI] * 7 + [_VP]),
    "tf_linear_groups_f32": (_CI, [_VP, _VP, ctypes.POINTER(_cabi.ProjGroup), _CI, _I64, _CI, _CI, _VP]),
    "tf_conv_packed_partials_f32": (_CI, [_VP, _VP, _VP, _VP] + [_CI] * 9 + [_VP, _VP]),
    "tf_mha_core_bwd_f32": (_CI, [_VP] * 8 + [_CF] + [_VP] * 3 + [_CI] * 13 + [_CF, _VP]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    assert _cabi.signatures()[name] == PINNED[name]


def test_parser_raises_on_a_type_outside_the_rule():
    for text, func in (("int tf_x(long double v);", "tf_x"), ("int tf_y(int a, size_t n);", "tf_y"),
                       ("unsigned tf_z(void);", "tf_z"), ("float *tf_w(int a);", "tf_w"), ("int tf_v(int);", "tf_v")):
        with pytest.raises(TypeError, match=func):
            _cabi.parse_prototypes(text)


def test_parser_reads_a_prototype_over_three_lines_with_comments():
    text = """
    /* int tf_not_this(int a); */
    // int tf_nor_this(int a);
    int64_t tf_x(const float *a,   /* the input: tf_inner(1) */
                 double *ws, int64_t n,  // a size
                 float eps, const char *name, void *stream);
    const char *tf_y(void);
    """
    assert _cabi.parse_prototypes(text) == {
        "tf_x": (_I64, [_VP, _VP, _I64, _CF, ctypes.c_char_p, _VP]),
        "tf_y": (ctypes.c_char_p, []),
    }


_FIELD_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}


@pytest.mark.parametrize("c_name,cls", [("tf_proj_group", _cabi.ProjGroup), ("tf_gn_level", _cabi.GnLevel)])
def test_structs_match_the_header(c_name, cls):
    """Field names, order and C types of the hand-written ctypes.Structure against the typedef's body in tf_fused.h."""
    text = open(os.path.join(REPO, "include", "tf_fused.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        m = re.fullmatch(r"(.*[\s*])(\w+)", " ".join(decl.split()))
        c_type = m.group(1).strip()
        fields.append((m.group(2), ctypes.c_void_p if c_type.endswith("*") else _FIELD_TYPES[c_type]))
    assert fields == list(cls._fields_)


def test_every_declared_symbol_is_bound(lib):
    """Nothing on the loaded library is left at ctypes' defaults (argtypes None, restype c_int by accident)."""
    for name in _declared_symbols():
        fn = getattr(lib, name)
        restype, argtypes = _cabi.signatures()[name]
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes, name
        assert fn.restype is restype, name


def test_every_declared_symbol_is_exported(lib):
    raw = ctypes.CDLL(_cabi.LIB_PATH)
    for name in _declared_symbols():
        assert hasattr(raw, name), name


def test_abi_version_and_strerror(lib):
    assert lib.tf_msda_abi_version() == _cabi.ABI_VERSION
    assert lib.tf_msda_strerror(0) == b"ok"
    for code in (-1, -2, -3, -4, -5, -99):
        assert len(lib.tf_msda_strerror(code)) > 0


def test_null_and_bad_dims_are_rejected_before_any_gpu_work(lib):
    shp = (ctypes.c_int64 * 2)(2, 2)
    one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
    assert lib.tf_msda_forward_f32(None, shp, one, one, one, 1, 4, 1, 4, 1, 1, 1, None) == -1
    assert lib.tf_msda_forward_f32(one, None, one, one, one, 1, 4, 1, 4, 1, 1, 1, None) == -1
    assert lib.tf_msda_forward_f32(one, shp, one, one, one, 0, 4, 1, 4, 1, 1, 1, None) == -2
    assert lib.tf_msda_forward_f32(one, shp, one, one, one, 1, 4, 1, 4, 17, 1, 1, None) == -2
    assert lib.tf_msda_forward_f32(one, shp, one, one, one, 1, 5, 1, 4, 1, 1, 1, None) == -3
    assert lib.tf_msda_backward_f64(one, shp, one, one, one, one, one, None, 1, 4, 1, 4, 1, 1, 1,
                                    None) == -1
    assert lib.tf_msda_backward_f32(one, shp, one, one, one, one, one, one, 1, 5, 1, 4, 1, 1, 1,
                                    None) == -3
    with pytest.raises(_cabi.MSDAError):
        _cabi.check(-3, "unit test")


def test_option_knobs_round_trip_without_a_gpu(lib):
    """tf_msda_set_option / tf_msda_set_tiled only touch host state: names, previous values, unknown names."""
    int_min = -2 ** 31
    assert lib.tf_msda_set_option(b"no_such_option", 1) == int_min
    assert lib.tf_msda_set_option(None, 1) == int_min
    prev = lib.tf_msda_set_option(b"quad_lds_kb", 48)
    assert prev == 40                                     # the shipped default (4 workgroups per CU)
    assert lib.tf_msda_set_option(b"quad_lds_kb", prev) == 48
    for name, default in ((b"quad_ta_mask", 0), (b"quad_waves", 4), (b"quad_npass", 3), (b"quad_split", 1)):
        assert lib.tf_msda_set_option(name, default) == default
    before = lib.tf_msda_set_tiled(0)
    assert before == -1                                   # -1: follow TF_MSDA_TILED (unset: the quad kernel)
    assert lib.tf_msda_set_option(b"tiled", 2) == 0
    assert lib.tf_msda_set_tiled(-1) == 2


def test_pquad_and_linear_knobs_round_trip_without_a_gpu(lib):
    """The persistent encoder kernel's options and the split GEMM's block-shape variant are host state as well."""
    int_min = -2 ** 31
    for name, default in ((b"pquad", 1), (b"pquad_wide", 1), (b"pquad_npass", 2), (b"pquad_lds_kb", 52),
                          (b"pquad_halo_y", 6), (b"pquad_halo_x", 10), (b"pquad_wg_per_cu", 3),
                          (b"pquad_prefetch", 0), (b"pquad_skew", 0)):
        assert lib.tf_msda_set_option(name, default) == default, name
    assert lib.tf_msda_set_option(b"pquad_no_such", 1) == int_min
    prev = lib.tf_msda_set_option(b"linear_stream_ti", 3)
    assert prev in (0, 3)                                 # 0: per-shape choice (the default)
    assert lib.tf_msda_set_option(b"linear_stream_ti", prev) == 3
    # knobs of experiments that were measured and removed are unknown names now (include/tf_msda.h lists what is left)
    for gone in (b"linear_variant", b"linear_bufstore", b"linear_deep", b"conv3_bufload", b"linear_astat"):
        assert lib.tf_msda_set_option(gone, 1) == int_min, gone
