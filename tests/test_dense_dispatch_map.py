"""The host-side dispatch of the dense kernels (csrc/host_dispatch.h, the knob table in csrc/msda_hip.hip), pinned: what
every dense tf_msda_set_option knob accepts, returns and reads from the environment, and which branch a call takes for a
value of it.  The companion of tests/test_msda_dispatch_map.py, with the same standing: every expected value below is a
literal, recorded by running this table against the emulated library built from the commit BEFORE the nine knobs moved
into one table, and is never derived from the library under test.  The only rows that differ from that recording are the
two deliberate deviations of "mha_mfma" (include/tf_msda.h), marked DEVIATION where they stand.

The tests run in the order of this file:
  * knob semantics in this process -- a sequence of set calls per knob and the previous value each returns -- on the
    emulated library (-m "not gpu") and, marked gpu, on libtf_msda.so (host code only).  The first return of a sequence
    is whatever earlier tests left in force and is not pinned here;
  * the defaults and the environment, each in a fresh child process (the library reads a variable once): what the first
    set call returns with no variable set, and with the knob's variable at an in-range value, an out-of-range value and 0;
  * the branch a call takes: the dense kernels report no name through tf_msda_last_kernel, so a branch is told by the work
    the emulator counts for the call, (blocks, barriers, wave_ops) of emu_lib.stats() -- reproducible run to run on the
    recording commit, and different for every pair of branches compared here.  Recorded with the emulator's default of 4
    compute units (HIPEMU_CUS unset) for both term schemes; the weight packing of the wrappers is part of every count.
    Only the counts and the status are checked (the numerics of these kernels: tests/test_emu_kernels.py,
    tests/test_proj_groups_emu.py, tests/test_linear_backward_cpu.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import emu_lib

emu = pytest.mark.skipif(not emu_lib.available(), reason="needs a host clang++ (ROCm's llvm) to build the emulated library")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MIN = -2 ** 31

# knob -> [(value set, previous value returned)]: an in-range value, each edge of the range, one below, one above and a negative,
# with an in-range value behind each so that what the refused value became is read back
SEQUENCES = {
    "ffn_ti": [(2, None), (1, 2), (3, 1), (0, 3), (2, 3), (4, 2), (2, 3), (-7, 2), (1, 3)],
    "ffn_tail_split": [(0, None), (1, 0), (0, 1), (5, 0), (0, 1), (-3, 0), (0, 1)],
    "linln_ti": [(2, None), (0, 2), (3, 0), (-1, 3), (2, 0), (4, 2), (2, 0), (-7, 2), (1, 0)],
    "groups_ti": [(2, None), (1, 2), (3, 1), (0, 3), (2, 0), (4, 2), (2, 0), (-7, 2), (1, 0)],
    "linear_stream_ti": [(2, None), (1, 2), (4, 1), (0, 4), (2, 0), (5, 2), (2, 0), (-7, 2), (1, 0)],
    "conv_halo": [(0, None), (1, 0), (0, 1), (5, 0), (0, 1), (-3, 0), (0, 1)],
    "linear_dma": [(4, None), (0, 4), (9, 0), (-1, 9), (4, 0), (10, 4), (4, 0), (-7, 4), (1, 0)],
    "mha_mfma": [(2, None), (0, 2), (2, 0), (-1, 2), (0, 1), (3, 0), (0, 1), (-7, 0), (2, 1)],
    "wgrad_msplit": [(5, None), (1, 5), (64, 1), (0, 64), (5, 0), (65, 5), (5, 0), (-7, 5), (2, 0)],
}
# what the first set call of a fresh process returns with no variable set
DEFAULTS = {"ffn_ti": 3, "ffn_tail_split": 1, "linln_ti": 0, "groups_ti": 0, "linear_stream_ti": 0, "conv_halo": 1, "linear_dma": 0,
            "mha_mfma": 1,   # DEVIATION: the recording commit returned -1 (not read yet) before the first attention call
            "wgrad_msplit": 0}
# (knob, variable, value) -> what the first set call of a fresh process returns: in range, out of range, "0"
ENVIRONMENT = [
    ("ffn_ti", "TF_FFN_TI", "2", 2), ("ffn_ti", "TF_FFN_TI", "4", 3), ("ffn_ti", "TF_FFN_TI", "0", 3),
    ("ffn_tail_split", "TF_FFN_TAIL_SPLIT", "1", 1), ("ffn_tail_split", "TF_FFN_TAIL_SPLIT", "7", 1), ("ffn_tail_split", "TF_FFN_TAIL_SPLIT", "0", 0),
    ("linln_ti", "TF_LINLN_TI", "2", 2), ("linln_ti", "TF_LINLN_TI", "4", 0), ("linln_ti", "TF_LINLN_TI", "0", 0),
    ("linear_stream_ti", "TF_LINEAR_STREAM_TI", "3", 3), ("linear_stream_ti", "TF_LINEAR_STREAM_TI", "5", 0),
    ("linear_stream_ti", "TF_LINEAR_STREAM_TI", "0", 0),
    ("conv_halo", "TF_CONV_HALO", "1", 1), ("conv_halo", "TF_CONV_HALO", "7", 1), ("conv_halo", "TF_CONV_HALO", "0", 0),
    ("linear_dma", "TF_LINEAR_DMA", "2", 2), ("linear_dma", "TF_LINEAR_DMA", "10", 0), ("linear_dma", "TF_LINEAR_DMA", "0", 0),
    # DEVIATION (all three): the recording commit returned -1 here whatever the variable held, and handed an out-of-range value
    # to the dispatch unchanged (the LDS-staged kernel); now the variable goes through the setter's 0..2 rule
    ("mha_mfma", "TF_MHA_MFMA", "2", 2), ("mha_mfma", "TF_MHA_MFMA", "5", 1), ("mha_mfma", "TF_MHA_MFMA", "0", 0),
]
DENSE_VARIABLES = sorted({v for _, v, _, _ in ENVIRONMENT})


def _check_sequence(lib, knob):
    first = lib.tf_msda_set_option(knob.encode(), SEQUENCES[knob][0][0])
    try:
        for value, want in SEQUENCES[knob][1:]:
            got = lib.tf_msda_set_option(knob.encode(), value)
            print("%s <- %d returned %d" % (knob, value, got))
            assert got == want
    finally:
        lib.tf_msda_set_option(knob.encode(), first)


@emu
@pytest.mark.parametrize("knob", list(SEQUENCES))
def test_knob_sequence_emulated(knob):
    _check_sequence(emu_lib.lib(), knob)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", list(SEQUENCES))
def test_knob_sequence_gpu(knob):
    from trackformer_amd import _cabi
    _check_sequence(_cabi.lib(), knob)


@emu
def test_unknown_names_emulated():
    lib = emu_lib.lib()
    for name in (b"ffn", b"ffn_ti2", b"mha", b"", b"TF_FFN_TI"):
        assert lib.tf_msda_set_option(name, 1) == INT_MIN
    assert lib.tf_msda_set_option(None, 1) == INT_MIN


_CHILD = """
import ctypes, sys
from tests.emu import build_emu
from trackformer_amd import _cabi
L = _cabi.bind(ctypes.CDLL(build_emu.build()))
print(" ".join("%s=%d" % (k, L.tf_msda_set_option(k.encode(), 1)) for k in sys.argv[1:]))
"""


def _fresh_process(knobs, variable=None, value=None):
    """The first tf_msda_set_option return of every knob in a new process that loads the emulated library."""
    env = {k: v for k, v in os.environ.items() if k not in DENSE_VARIABLES}
    if variable:
        env[variable] = value
    emu_lib.lib()   # built here, not by the child
    out = subprocess.run([sys.executable, "-c", _CHILD] + list(knobs), cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    print(variable, value, out.stdout.strip())
    return {k: int(v) for k, v in (item.split("=") for item in out.stdout.split())}


@emu
def test_defaults_in_a_fresh_process():
    assert _fresh_process(list(DEFAULTS)) == DEFAULTS


@emu
@pytest.mark.parametrize("knob,variable,value,want", ENVIRONMENT, ids=["%s=%s" % (v, x) for _, v, x, _ in ENVIRONMENT])
def test_environment_in_a_fresh_process(knob, variable, value, want):
    assert _fresh_process([knob], variable, value)[knob] == want


# ---- which branch a call takes: (blocks, barriers, wave_ops) per call, terms 6 | 16 --------------------------------------------
_RNG = np.random.default_rng(11)


def _randn(*shape):
    return _RNG.standard_normal(shape).astype(np.float32)


_X200, _X300, _W, _W2, _B = _randn(200, 256), _randn(300, 256), _randn(256, 256) / 16, _randn(256, 256) / 16, _randn(256)
_Q, _K, _V = _randn(1, 20, 2, 32), _randn(1, 20, 2, 32), _randn(1, 20, 2, 32)
_CX, _CW = _randn(1, 9, 11, 64), _randn(64, 3, 3, 64) / 24
_DY, _WX = _randn(256, 128), _randn(256, 128)   # 8 slices of 32 rows: the smallest row count that one and two chunks split differently


def _linear_packed():
    emu_lib.linear_packed(_X200, _W, _B)


def _linear_res_ln():
    emu_lib.linear_res_ln(_X200, _W, _B, residual=_X200, ln=(_B, _B))


def _ffn_fused():
    emu_lib.ffn_fused(_X300, _W, _B, _W2, _B, residual=_X300, ln=(_B, _B))


def _mha_core():
    emu_lib.mha_core(_Q, _K, _V, 32 ** -0.5)


def _conv_packed():
    emu_lib.conv_packed(_CX, _CW, _B[:64])


def _linear_groups():
    from tests.test_proj_groups_emu import linear_groups
    rc, _ = linear_groups(_X200, None, [(_W, _B, False)])
    assert rc == 0


def _wgrad():
    from tests.test_linear_backward_cpu import wgrad
    wgrad(_DY, _WX, emu_lib.TERMS)


# (id, call, options, {terms: (blocks, barriers, wave_ops)})
BRANCHES = [
    ("linear_packed", _linear_packed, dict(), {6: (40, 36, 6176), 16: (104, 27, 5024)}),
    ("linear_packed-linear_stream_ti=2", _linear_packed, dict(linear_stream_ti=2), {6: (40, 36, 6176), 16: (104, 36, 4640)}),
    ("linear_packed-linear_stream_ti=3", _linear_packed, dict(linear_stream_ti=3), {6: (40, 27, 6944), 16: (104, 27, 5024)}),
    ("linear_packed-linear_stream_ti=4", _linear_packed, dict(linear_stream_ti=4), {6: (40, 18, 6176), 16: (104, 18, 4640)}),
    ("linear_packed-linear_dma=1", _linear_packed, dict(linear_dma=1), {6: (48, 32, 7488), 16: (112, 32, 5696)}),
    ("linear_packed-linear_dma=2", _linear_packed, dict(linear_dma=2), {6: (64, 64, 8064), 16: (128, 64, 6272)}),
    ("linear_res_ln-linln_ti=1", _linear_res_ln, dict(linln_ti=1), {6: (39, 28, 5460), 16: (103, 28, 4308)}),
    ("linear_res_ln-linln_ti=2", _linear_res_ln, dict(linln_ti=2), {6: (36, 16, 6224), 16: (100, 16, 4688)}),
    ("linear_res_ln-linln_ti=3", _linear_res_ln, dict(linln_ti=3), {6: (36, 16, 6224), 16: (99, 12, 5076)}),
    ("ffn_fused-ffn_ti=1", _ffn_fused, dict(ffn_ti=1), {6: (74, 80, 15480), 16: (202, 80, 10872)}),
    ("ffn_fused-ffn_ti=2", _ffn_fused, dict(ffn_ti=2, ffn_tail_split=1), {6: (70, 48, 15464), 16: (198, 48, 10856)}),
    ("ffn_fused-ffn_ti=2,ffn_tail_split=0", _ffn_fused, dict(ffn_ti=2, ffn_tail_split=0), {6: (69, 40, 15460), 16: (197, 40, 10852)}),
    ("ffn_fused-ffn_ti=3", _ffn_fused, dict(ffn_ti=3, ffn_tail_split=1), {6: (70, 48, 15464), 16: (196, 32, 12400)}),
    ("mha_core-mha_mfma=0", _mha_core, dict(mha_mfma=0), {6: (4, 20, 192), 16: (4, 20, 192)}),
    ("mha_core-mha_mfma=1", _mha_core, dict(mha_mfma=1), {6: (4, 12, 656), 16: (4, 12, 656)}),
    ("mha_core-mha_mfma=2", _mha_core, dict(mha_mfma=2), {6: (4, 24, 272), 16: (4, 24, 272)}),
    ("conv_packed-conv_halo=0", _conv_packed, dict(conv_halo=0, linear_stream_ti=0), {6: (80, 38, 1760), 16: (144, 38, 2432)}),
    ("conv_packed-conv_halo=0,linear_stream_ti=2", _conv_packed, dict(conv_halo=0, linear_stream_ti=2), {6: (80, 19, 1760), 16: (144, 19, 2432)}),
    ("conv_packed-conv_halo=1", _conv_packed, dict(conv_halo=1, linear_stream_ti=0), {6: (80, 12, 3488), 16: (144, 12, 3296)}),
    ("conv_packed-conv_halo=1,linear_stream_ti=2", _conv_packed, dict(conv_halo=1, linear_stream_ti=2), {6: (80, 6, 3488), 16: (144, 6, 3296)}),
    ("linear_groups-groups_ti=1", _linear_groups, dict(groups_ti=1), {6: (39, 7, 5404), 16: (103, 7, 4252)}),
    ("linear_groups-groups_ti=2", _linear_groups, dict(groups_ti=2), {6: (39, 7, 5404), 16: (100, 4, 4624)}),
    ("linear_groups-groups_ti=3", _linear_groups, dict(groups_ti=3), {6: (39, 7, 5404), 16: (99, 3, 5004)}),
    ("wgrad-wgrad_msplit=1", _wgrad, dict(wgrad_msplit=1), {6: (12, 105, 1540), 16: (12, 105, 772)}),
    ("wgrad-wgrad_msplit=2", _wgrad, dict(wgrad_msplit=2), {6: (29, 105, 1544), 16: (29, 105, 776)}),
]


def _triple(call, opts, terms):
    prev_terms = emu_lib.set_terms(terms)
    prev = emu_lib.set_options(**opts)
    try:
        emu_lib.stats(reset=True)
        call()
        s = emu_lib.stats()
    finally:
        emu_lib.set_options(**prev)
        emu_lib.set_terms(prev_terms)
    return s["blocks"], s["barriers"], s["wave_ops"]


@emu
@pytest.mark.parametrize("terms", [6, 16])
@pytest.mark.parametrize("name,call,opts,want", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_branch_taken(name, call, opts, want, terms):
    got = _triple(call, opts, terms)
    print("%s terms %d: %s" % (name, terms, got))
    assert got == want[terms]


def test_every_knob_separates_two_branches():
    """Every dense knob appears in at least two rows whose counts differ (in at least one term scheme)."""
    for knob in SEQUENCES:
        seen = {(terms, row[3][terms]) for row in BRANCHES if knob in row[2] for terms in (6, 16)}
        assert len({t for t, _ in seen}) < len(seen), knob
