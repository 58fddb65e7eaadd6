"""Shared by tests/test_groupnorm_levels_emu.py (SIMT emulator, host pointers) and tests/test_groupnorm_levels_gpu.py (device):
tf_groupnorm_levels_nhwc_f32 -- GroupNorm of several pyramid levels in two launches into one token buffer (csrc/fused_ops.hip) -- and
tf_conv_packed_partials_f32, the convolution entry that leaves its split-K partial sums for it.

  * restate(): the kernels' arithmetic operation by operation in numpy -- the order of every sum is part of the contract (no atomics:
    two calls give the same bits), so the comparison is BITWISE
  * run_levels(): one call with guard rows before, between and behind the levels' rows of the output, an image stride that is not
    HW * C, and a guarded workspace, on either backend

A backend is a pair (lib, up, down): `up(numpy array) -> (keep-alive object, address)`, `down(object) -> numpy array`."""
import numpy as np

from trackformer_amd import _cabi

GUARD_ROWS = 2
SENTINEL = np.float32(-7.25e11)       # what guard rows and unwritten output rows hold
WS_SENTINEL = -3.5e101
ROWS_PER_BLOCK = 64                   # kGnRowsPerBlock


GnLevel = _cabi.GnLevel


# ---- the arithmetic, restated ------------------------------------------------------------------------------------------------------
def rows_per_block(pieces, C):
    """Rows a statistics workgroup owns (gn_levels_rows_per_block): 64, fewer where every element costs `pieces` loads."""
    if pieces <= 1:
        return ROWS_PER_BLOCK
    nslots = 256 // (C // 4)
    rows = (ROWS_PER_BLOCK // min(pieces, ROWS_PER_BLOCK)) // nslots * nslots
    return max(rows, nslots)


def reduce_y(parts, bias):
    """y = ((p0 + p1) + ... + p_last) + bias in fp32, z ascending, then the bias: stream_splitk_reduce_kernel's order.
    parts [pieces, N, HW, C] fp32, bias [C] or None."""
    y = parts[0].astype(np.float32).copy()
    for z in range(1, parts.shape[0]):
        y = y + parts[z]
    if bias is not None:
        y = y + bias.astype(np.float32)
    assert y.dtype == np.float32
    return y


def slot_sums(y, G, pieces):
    """[N, slots, G, 2] doubles: what the statistics pass leaves in the workspace for y [N, HW, C] fp32.  A thread owns one channel quad
    of every nslots-th row of the block and adds its rows in order (each element widened first; a a is exact in double); a group's
    total adds the threads' sums row slot by row slot, inside a slot the group's channels ascending."""
    N, HW, C = y.shape
    nslots, cpg, rpb = 256 // (C // 4), C // G, rows_per_block(pieces, C)
    nsb = -(-HW // rpb)
    yd = y.astype(np.float64)
    out = np.zeros((N, nsb, G, 2))
    for b in range(nsb):
        r0, r1 = b * rpb, min(HW, (b + 1) * rpb)
        S, Q = np.zeros((N, nslots, C)), np.zeros((N, nslots, C))
        for rs in range(nslots):
            for r in range(r0 + rs, r1, nslots):
                S[:, rs] = S[:, rs] + yd[:, r]
                Q[:, rs] = Q[:, rs] + yd[:, r] * yd[:, r]
        for st, T in enumerate((S, Q)):
            Tg = T.reshape(N, nslots, G, cpg)
            a = np.zeros((N, G))
            for rs in range(nslots):
                for k in range(cpg):
                    a = a + Tg[:, rs, :, k]
            out[:, b, :, st] = a
    return out


def restate(y, gamma, beta, G, eps, pieces):
    """The normalised level [N, HW, C] fp32 exactly as the two kernels compute it from y [N, HW, C] fp32 (for pieces > 1: reduce_y of
    the partial sums): slot_sums; per group, chain p of P = 256 // G adds the slots p, p + P, ..., then the chains in order; mean / rstd
    in double as groupnorm_apply_kernel, rounded to fp32; ((y - mean) * rstd) * gamma + beta, every operation rounded on its own."""
    N, HW, C = y.shape
    cpg = C // G
    slots = slot_sums(y, G, pieces)
    P = 256 // G
    chains = []
    for p in range(P):
        a = np.zeros((N, G, 2))
        for s in range(p, slots.shape[1], P):
            a = a + slots[:, s]
        chains.append(a)
    tot = chains[0]
    for a in chains[1:]:
        tot = tot + a
    cnt = np.float64(HW) * np.float64(cpg)
    mean = tot[..., 0] / cnt
    var = tot[..., 1] / cnt - mean * mean
    var = np.where(var < 0.0, 0.0, var)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    mean_c = np.repeat(mean.astype(np.float32), cpg, axis=1)[:, None, :]
    rstd_c = np.repeat(rstd.astype(np.float32), cpg, axis=1)[:, None, :]
    out = ((y - mean_c) * rstd_c) * gamma.astype(np.float32) + beta.astype(np.float32)
    assert out.dtype == np.float32
    return out


def launch_pieces(k, ksplit):
    """Pieces launch_stream makes of `ksplit` for a K loop of k / 32 slices: an even number of slices per piece."""
    slices = k // 32
    if ksplit <= 1:
        return 1
    kslices = ((slices + ksplit - 1) // ksplit + 1) & ~1
    gz = -(-slices // kslices)
    return gz if gz > 1 else 1


# ---- one call ------------------------------------------------------------------------------------------------------------------------
def host_backend(L):
    """Host pointers (the emulated library)."""
    def up(a):
        a = np.ascontiguousarray(a)
        buf = np.zeros(a.nbytes + 16, np.uint8)
        off = (-buf.ctypes.data) % 16
        out = buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out, out.ctypes.data
    return L, up, lambda o: o


def device_backend(L, device="cuda"):
    import torch

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return t, t.data_ptr()

    def down(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return L, up, down


def run_levels(backend, levels, N, C, G, eps=1e-5, stream=None, order=None):
    """levels: [dict(src = y [N, HW, C] | parts [pieces, N, HW, C], pieces, bias [C] | None, gamma, beta)] in TABLE order; their rows of
    the output follow `order` (a permutation of the table indices; default: table order) with GUARD_ROWS sentinel rows before, between
    and behind them, and the image stride one more row than that.
    -> (status, [the level's rows of the output [N, HW, C]], untouched: bool, workspace doubles stated)."""
    L, up, down = backend
    order = list(range(len(levels))) if order is None else list(order)
    row0, rows = {}, GUARD_ROWS
    for i in order:
        row0[i] = rows
        rows += levels[i]["src"].shape[-2] + GUARD_ROWS
    stride = (rows + 1) * C
    keep = []
    table = (GnLevel * len(levels))()
    for i, (d, lv) in enumerate(zip(table, levels)):
        ptrs = []
        for name in ("src", "bias", "gamma", "beta"):
            a = lv.get(name)
            if a is None:
                ptrs.append(None)
            else:
                o, p = up(np.asarray(a, np.float32))
                keep.append(o)
                ptrs.append(p)
        d.src, d.bias, d.gamma, d.beta = ptrs
        d.pieces, d.HW, d.row0 = lv["pieces"], lv["src"].shape[-2], row0[i]
    n_ws = L.tf_groupnorm_levels_workspace_doubles(table, len(levels), N, C, G)
    assert n_ws > 0, n_ws
    out_o, out_p = up(np.full((N, stride), SENTINEL, np.float32))
    ws_o, ws_p = up(np.full(n_ws + 16, WS_SENTINEL, np.float64))
    rc = L.tf_groupnorm_levels_nhwc_f32(table, len(levels), N, C, G, eps, out_p, stride, ws_p, stream)
    out = down(out_o).reshape(N, rows + 1, C)
    ws = down(ws_o)
    written = np.zeros(rows + 1, bool)
    got = [None] * len(levels)
    for i, lv in enumerate(levels):
        hw = lv["src"].shape[-2]
        got[i] = out[:, row0[i]:row0[i] + hw].copy()
        written[row0[i]:row0[i] + hw] = True
    untouched = bool((out[:, ~written].view(np.uint32) == SENTINEL.view(np.uint32)).all()) and bool((ws[n_ws:] == WS_SENTINEL).all())
    ws_all_written = bool((ws[:n_ws] != WS_SENTINEL).all())
    return rc, got, untouched and (rc != 0 or ws_all_written), n_ws


def make_level(profile, N, HW, C, G, pieces, seed, with_bias=True):
    """A level's operands from tests/util_norm_attn_numerics.norm_operands: for pieces > 1 the profile's x cut into `pieces` partial
    sums of uneven weight (their fp32 sum in z order, plus the bias, is the y the level is normalised from)."""
    from tests import util_norm_attn_numerics as A
    x, _, gamma, beta = A.norm_operands(profile, N, HW, C, seed=seed, groups=G)
    x, gamma, beta = x.numpy(), gamma.numpy(), beta.numpy()
    if pieces == 1:
        return dict(src=x, pieces=1, bias=None, gamma=gamma, beta=beta, y=x)
    g = np.random.default_rng(seed)
    wts = g.uniform(0.2, 1.0, pieces)
    wts = (wts / wts.sum()).astype(np.float32)
    parts = np.stack([x * w for w in wts]).astype(np.float32)
    parts[-1] += (0.01 * g.standard_normal(x.shape)).astype(np.float32) * np.abs(x).mean()
    bias = (0.1 * g.standard_normal(C)).astype(np.float32) if with_bias else None
    return dict(src=parts, pieces=pieces, bias=bias, gamma=gamma, beta=beta, y=reduce_y(parts, bias))
