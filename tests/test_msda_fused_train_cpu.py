"""CPU: the two kernels of the trainable fused MSDeformAttn entry (trackformer_amd/csrc/msda_fused_bwd.h) under the SIMT emulator,
against the float64 restatement and the bounds of tests/util_msda_fused_train.py: prologue and epilogue on every shape of its
table but the encoder-sized one, a strided layout with canaries, the status codes and the emulator's divergence counters."""
import pytest
import torch

from tests import emu_lib
from tests import util_msda_fused_train as T
from tests import util_msda_numerics as U

pytestmark = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

PROFILES = ["unit", "wide", "large_logits"]
CANARY = -1234.5


@pytest.fixture(scope="module")
def lib():
    return emu_lib.lib()


def _grads(shape_loc, seed):
    """Synthetic grad_loc / grad_attn: normal values over a wide range of magnitudes, some exact zeros."""
    g = torch.Generator().manual_seed(seed)
    gl = torch.randn(shape_loc, generator=g) * torch.exp2(torch.randint(-12, 13, shape_loc, generator=g).float())
    ga = torch.randn(shape_loc[:-1], generator=g) * torch.exp2(torch.randint(-6, 7, shape_loc[:-1], generator=g).float())
    gl[torch.rand(shape_loc, generator=g) < 0.1] = 0.0
    ga[torch.rand(shape_loc[:-1], generator=g) < 0.1] = 0.0
    return gl.contiguous(), ga.contiguous()


def _run(lib, cid, profile, ld=None, off_col=0, logit_col=None, ld_g=None, goff_col=0, glogit_col=None, guard=0):
    (value, shapes, refp, qproj, _), (M, L, P) = T.make(cid, profile)
    N, Lq = qproj.shape[:2]
    mlp = M * L * P
    ld = ld or 3 * mlp + (mlp & 1)        # (ld must be even: an odd M L P needs a padded row)
    logit_col = 2 * mlp if logit_col is None else logit_col
    ld_g = ld_g or 3 * mlp + (mlp & 1)
    glogit_col = 2 * mlp if glogit_col is None else glogit_col
    qbuf = torch.full((N * Lq, ld), float("nan"))
    qbuf[:, off_col:off_col + 2 * mlp] = qproj.reshape(N * Lq, -1)[:, :2 * mlp]
    qbuf[:, logit_col:logit_col + mlp] = qproj.reshape(N * Lq, -1)[:, 2 * mlp:]
    emu_lib.stats(reset=True)
    rc, loc, attn = T.prologue(lib, shapes, refp, qbuf, ld, off_col, logit_col, N, Lq, M, L, P)
    assert rc == 0
    assert emu_lib.last_kernel() == "msda_fused_prologue<f32>"
    T.check_prologue(loc, attn, shapes, refp, qproj, M, L, P, what="%s %s" % (cid, profile))
    gl, ga = _grads(tuple(loc.shape), T.SEED + 2)
    want = T.epilogue_reference(shapes, refp, qproj, attn, gl, ga, M, L, P, loc=loc)
    gq = torch.full((N * Lq + guard, ld_g), CANARY)
    rc, gref = T.epilogue(lib, shapes, refp, qbuf, ld, off_col, logit_col, attn, gl, ga, gq, ld_g, goff_col, glogit_col, True, M, L, P)
    assert rc == 0
    assert emu_lib.last_kernel() == "msda_fused_bwd_epilogue<f32>"
    st = emu_lib.stats()
    assert st["divergent_ops"] == 0 and st["inactive_reads"] == 0, st
    rows = gq[:N * Lq]
    T.check_epilogue(rows[:, goff_col:goff_col + 2 * mlp].reshape(loc.shape), rows[:, glogit_col:glogit_col + mlp].reshape(attn.shape),
                     gref, want, what="%s %s" % (cid, profile))
    # without grad_ref: the same columns, bit for bit
    gq2 = torch.full_like(gq, CANARY)
    rc, none = T.epilogue(lib, shapes, refp, qbuf, ld, off_col, logit_col, attn, gl, ga, gq2, ld_g, goff_col, glogit_col, False, M, L, P)
    assert rc == 0 and none is None and T.bits_equal(gq, gq2)
    return gq, (N * Lq, mlp), attn


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("cid", T.CPU_IDS + list(T.EXTRA_CASES))
def test_prologue_and_epilogue(lib, cid, profile):
    gq, (rows, mlp), attn = _run(lib, cid, profile)
    if cid == "p1l1":   # softmax of one element: the weight is exactly 1 and its gradient exactly 0
        assert bool((attn == 1).all())
        assert not bool(gq[:, 2 * mlp:].view(torch.int32).bitwise_and(0x7FFFFFFF).any())


def test_strided_layout_leaves_the_gaps_alone(lib):
    (_, _, _, qproj, _), (M, L, P) = T.make("dec_r2", "unit")
    mlp = M * L * P
    ld_g, goff, glogit = 3 * mlp + 14, 4, 2 * mlp + 10
    gq, (rows, _), _ = _run(lib, "dec_r2", "unit", ld=3 * mlp + 10, off_col=2, logit_col=2 * mlp + 6, ld_g=ld_g, goff_col=goff,
                            glogit_col=glogit, guard=3)
    written = torch.zeros(ld_g, dtype=torch.bool)
    written[goff:goff + 2 * mlp] = True
    written[glogit:glogit + mlp] = True
    assert bool((gq[:rows][:, ~written] == CANARY).all()), "the epilogue wrote between its column ranges"
    assert bool((gq[rows:] == CANARY).all()), "the epilogue wrote behind the last row"
    assert not bool((gq[:rows][:, written] == CANARY).any())


def test_status_codes_in_the_documented_order(lib):
    (value, shapes, refp, qproj, _), (M, L, P) = T.make("odd", "unit")
    N, Lq = qproj.shape[:2]
    mlp = M * L * P
    q2 = qproj.reshape(N * Lq, -1).contiguous()
    NULL, DIMS = -1, -2
    rc, loc, attn = T.prologue(lib, shapes, refp, q2, 3 * mlp, 0, 2 * mlp, N, Lq, M, L, P)
    assert rc == 0
    gl, ga = _grads(tuple(loc.shape), 3)
    gq = torch.zeros(N * Lq, 3 * mlp)

    def pro(**kw):
        a = dict(shapes=shapes, refp=refp, qbuf=q2, ld=3 * mlp, off_col=0, logit_col=2 * mlp, N=N, Lq=Lq, M=M, L=L, P=P)
        a.update(kw)
        return T.prologue(lib, **a)[0]

    def epi(want_ref=True, **kw):
        a = dict(shapes=shapes, refp=refp, qbuf=q2, ld=3 * mlp, off_col=0, logit_col=2 * mlp, attn=attn, gl=gl, ga=ga, gq=gq,
                 ld_g=3 * mlp, goff_col=0, glogit_col=2 * mlp, want_ref=want_ref, M=M, L=L, P=P)
        a.update(kw)
        return T.epilogue(lib, **a)[0]

    class _Null:   # a tensor stand-in whose pointer is NULL
        def __init__(self, like):
            self.shape, self.device, self.is_cuda = like.shape, like.device, False

        def data_ptr(self):
            return None

    # NULL wins over a bad dimension
    assert pro(qbuf=_Null(q2), P=3) == NULL
    assert pro(refp=_Null(refp), ld=3 * mlp + 1) == NULL
    assert epi(attn=_Null(attn), P=3) == NULL
    assert epi(gl=_Null(gl), ld_g=5) == NULL
    assert epi(ga=_Null(ga)) == NULL
    assert epi(gq=_Null(gq), goff_col=1) == NULL
    assert epi(want_ref=False) == 0          # grad_ref may be NULL
    # dimensions
    for kw in (dict(P=3), dict(ld=3 * mlp + 1), dict(off_col=1), dict(logit_col=2 * mlp + 1), dict(ld=3 * mlp - 2), dict(L=17),
               dict(off_col=-2)):
        assert pro(**kw) == DIMS, kw
        assert epi(**kw) == DIMS, kw
    for kw in (dict(ld_g=3 * mlp + 1), dict(goff_col=1), dict(ld_g=3 * mlp - 2), dict(glogit_col=mlp), dict(glogit_col=-1)):
        assert epi(**kw) == DIMS, kw
    bad_shapes = shapes.clone()
    bad_shapes[0, 0] = 0
    assert pro(shapes=bad_shapes) == DIMS and epi(shapes=bad_shapes) == DIMS
    r3 = refp[..., :3].contiguous()
    assert pro(refp=r3) == DIMS              # ref_dim 3
