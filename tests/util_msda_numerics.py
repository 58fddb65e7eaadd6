"""The float64 yardstick of multi-scale deformable attention (trackformer_amd/csrc/msda_*.hip) and the operand profiles every
MSDA numerics test draws its inputs from.

Every output element y of a kernel is held to the float64 result `ref` of the same operation on the same fp32 inputs:

    (|y - ref| - floor) / S  <=  2^-20 sqrt(max(n, 64) / 64)

where S is the sum of the magnitudes of the terms (so the bound is relative to what the arithmetic could cancel, not to |ref|),
floor is an absolute allowance for errors that do not scale with S, and n is the number of terms of the sum.

Forward, plain entry.  px = loc_x W - 0.5 is formed in float64 from the fp32 loc (py alike); a sample is in range when
-1 < px < W and -1 < py < H; its bilinear weights w_c over the four corners, corners outside the level reading zero.
    ref    sum_{l,p} a sum_c w_c v_c
    S      sum_{l,p} |a| sum_c w_c |v_c|                     (in-range samples, in-range corners)
    n      4 L P
  The kernels form px with one rounding (fma(loc, W, -0.5)); the reference formula rounds twice (fl(fl(loc W) - 0.5)).  Either
  is within dx = 2^-23 (|px| + 1) of the exact px: 2^-24 |px| for one rounding, 2^-24 (|px| + 0.5) + 2^-24 |px| for two.  The
  output is Lipschitz in px with constant |a| (gy (|v1| + |v2|) + fy (|v3| + |v4|)) <= |a| sum_c |v_c|, and continuous at the
  cell edges and at the range limits (the weight of the corner that appears or vanishes there is zero), so moving px by dx
  moves the output by at most |a| dx sum_c |v_c|.  Near a cell edge (fx < dx or gx < dx) the kernel may sit in the neighbouring
  cell: the corners of that cell join the sum; near a range limit (within dx of -1 or W) a sample the reference drops may be
  taken, so the location term runs over every sample within dx of the range.
    floor  sum |a| (dx A_x + dy A_y)  +  2^-149 (4 + 12 L P)
  A_x = sum_c |v_c| (plus the neighbouring column's corners near an x cell edge); the second term is fp32's subnormal spacing
  for each of the (at most 12 per sample) rounding steps: it matters for outputs of order 1e-38 only.

Fused entry (tf_msda_forward_fused_f32: softmax over the L P logits and the location arithmetic in the kernel).  The reference
does both in float64 from the fp32 qproj and reference points: loc = r + off / H (2-d references; x over H_l as written in
the reference module) or r + off / P * r_wh * 0.5 (4-d).  The kernels divide, or multiply by v_rcp_f32(H) (1 ulp; msda_pquad
/ pquad2), and round the add: |dloc| <= 2^-22 |off term| + 2^-23 |loc|, so dx gains W |dloc|.  Softmax: __expf(z - z_max)
rounds z - z_max, scales it by log2(e) and rounds the exp2: a relative error of u (3 + 3 |z_i - z_max|) per exponential
(u = 2^-24); the sum of L P positive terms (sequential in the buffer kernel) and the reciprocal add u (L P + 2) to a common
factor.  A weight below 2^-126 is good to an absolute 2^-126 only: the LDS-window kernels' exponential and reciprocal do not
keep fp32 subnormal results (measured on MI355X under logits x 30: 7e-39 off on an output whose S is 1.8e-38, where the
buffer and direct kernels and torch keep them).  So |da_i| <= a_i u (3 + 3 |z_i - z_max|) + a_i u (L P + 2 + sum_j a_j (3 +
3 |z_j - z_max|)) + 2^-126, and the floor gains sum |da_i| sum_c w_c |v_c|.

Backward (grad_output g [N, Lq, M D]); each gradient is bounded on its own:
    grad_value  ref sum a w_c g_d over the K contributions to the element; S = sum |a w_c g_d|; n = K (per element).  floor:
                |a g_d| (dx + dy) for each contribution of a sample within dx of the range (the weights move by at most the
                location error; near a cell edge the neighbouring cell's corners receive up to dx |a g_d|), + 2^-149 (4K + 4).
    grad_attn   ref sum_d g_d sum_c w_c v_c; S = sum_d |g_d| sum_c w_c |v_c|; n = 4 D; floor as the forward (per sample).
    grad_loc    ref W a sum_d g_d (gy (v2 - v1) + fy (v4 - v3)) for x (H and the transposed form for y); S = |a| W sum_d |g_d|
                sum_c |v_c|; n = 4 D.  Inside a cell grad_loc_x does not depend on px, and depends on py through gy, fy with
                |d grad_loc_x / dpy| <= S: the cross term floor is dy S (dx S for y), + 2^-149 W (8 D + 8).
                grad_loc_x jumps where px crosses an integer (a cell edge, and -1 and W, the range limits): samples within 2 dx
                of one are left out of that coordinate's comparison (Ref.keep).  Random profiles leave out fewer than 0.1 %.
                With exact positions (dx = 0, exact=True) nothing is left out.

Bound.  2^-20 for up to 64 terms; beyond it 2^-20 sqrt(n / 64): the rounding of a sum of n terms grows as sqrt(n) for
errors of random sign (the C oracle's fp32 forward reaches 2^-21.x at L P = 64 on positive operands, where partial sums grow
linearly; at n = 4096 (grad_attn with D = 1024) sequential fp32 sums stay within 2^-20 sqrt(n / 64)).  Next to the fixed bound a
kernel is held to the fp32 C oracle (oracle/msda_ref.c) on the same case: its worst normalised excess may be at most 4 times the
oracle's own, or 2^-21 where the oracle is as good as exact.  A kernel that is fp32-class passes; weights rounded to bf16 (2^-9)
or fp16 (2^-12), corners dropped below a weight of 2^-10, loc rounded to fp16 or fp16 accumulation do not
(tests/test_msda_numerics_cpu.py).

Non-finite contract: exactly the outputs the float64 reference makes NaN must be NaN (a NaN pixel read at a nonzero weight);
every other output is finite and within the bound.

Everything here is torch and runs on the CPU or, in float64, on the GPU.  The excess is reported divided by sqrt(max(n, 64) / 64)
("normalised excess"), so one number compares with 2^-20 whatever the length of the sum."""
import math

import numpy as np
import torch

BOUND = 2.0 ** -20            # the fixed bound on (|y - ref| - floor) / S for sums of up to BOUND_N terms ...
BOUND_N = 64                  # ... beyond it 2^-20 sqrt(n / 64)
FP32_FACTOR = 4.0             # the fp32 comparison: at most 4 x the C oracle's own worst normalised excess ...
FP32_CLASS_MIN = 2.0 ** -21   # ... or 2^-21 where the oracle itself is as good as exact
U32 = 2.0 ** -24              # fp32 unit roundoff
SUB = 2.0 ** -149             # fp32 subnormal spacing
SMALLEST_NORMAL = 2.0 ** -126  # the fused entry's attention weights are held to this absolute error (module docstring)
EXCLUDE_MAX = 1e-3            # random profiles may leave at most this fraction of grad_loc coordinates out

PROFILES = ["unit", "wide", "signed", "large", "small", "level_spread", "hot_pixel", "permuted"]
FUSED_PROFILES = ["unit", "wide", "large", "small", "level_spread", "large_logits"]


class Ref:
    """One output's yardstick: the float64 result, S, the floor, the outputs that must be NaN, the term count n (int or
    per-element tensor) and the elements compared (keep: all when None)."""

    def __init__(self, ref, scale, floor, expect_nan, n, keep=None):
        self.ref, self.scale, self.floor, self.expect_nan, self.n, self.keep = ref, scale, floor, expect_nan, n, keep

    def to(self, device):
        mv = lambda t: t.to(device) if torch.is_tensor(t) else t   # noqa: E731
        return Ref(mv(self.ref), mv(self.scale), mv(self.floor), mv(self.expect_nan), mv(self.n), mv(self.keep))

    def select(self, index, dim=1):
        """The elements at `index` along `dim` (a query sample)."""
        sel = lambda t: t.index_select(dim, index.to(t.device)) if torch.is_tensor(t) and t.dim() > dim else t   # noqa: E731
        return Ref(sel(self.ref), sel(self.scale), sel(self.floor), sel(self.expect_nan), sel(self.n), sel(self.keep))


class Excess:
    """The worst element of a comparison: its normalised excess, where it is, the values there, and the C oracle's own."""

    def __init__(self, value, index, got, want, scale, floor, fp32_err):
        self.value, self.index, self.got, self.want, self.scale, self.floor, self.fp32_err = \
            value, index, got, want, scale, floor, fp32_err

    def __repr__(self):
        return ("max (|y - ref| - floor) / S / sqrt(max(n, 64) / 64) = %.3e at %s (y %r, ref %r, S %.3e, floor %.3e); "
                "fp32 oracle's own %.3e" % (self.value, self.index, self.got, self.want, self.scale, self.floor, self.fp32_err))


def growth(n):
    """sqrt(max(n, 64) / 64) for an int or a tensor of term counts."""
    if torch.is_tensor(n):
        return (n.double().clamp_min(BOUND_N) / BOUND_N).sqrt()
    return math.sqrt(max(n, BOUND_N) / BOUND_N)


def _normalised(err, scale):
    """err / scale with 0 / 0 = 0 and e / 0 = inf (an output whose S is zero must come out within its floor)."""
    err = err.clamp_min(0)
    pos = scale > 0
    return torch.where(pos, err / torch.where(pos, scale, torch.ones_like(scale)),
                       torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def _as_tensor(y, like):
    if isinstance(y, np.ndarray):
        y = torch.from_numpy(y)
    return y.to(like.device).double().reshape(like.shape)


def excess(y, r, fp32=None):
    """Per-element normalised excess of y over r (a Ref) and the worst element (Excess); asserts the NaN contract."""
    ref = r.ref
    y = _as_tensor(y, ref)
    nan_ok = r.expect_nan
    bad = torch.isnan(y) != nan_ok
    if r.keep is not None:
        bad = bad & r.keep
    assert not bool(bad.any()), "NaN outputs differ from the expected ones at %s (y %r, ref %r)" % (
        tuple(int(v) for v in bad.nonzero()[0]), float(y[bad][0]), float(ref[bad][0]))
    keep = ~nan_ok if r.keep is None else (~nan_ok & r.keep)
    assert bool(torch.isfinite(y[keep]).all()), "non-finite output where none is expected"
    g = growth(r.n)
    zero = torch.zeros_like(ref)
    e = torch.where(keep, _normalised((y - ref).abs() - r.floor, r.scale) / g, zero)
    fp32_err = 0.0
    if fp32 is not None:
        f = _as_tensor(fp32, ref)
        fe = torch.where(keep & torch.isfinite(f), _normalised((f - ref).abs() - r.floor, r.scale) / g, zero)
        fp32_err = float(fe.max()) if fe.numel() else 0.0
    if e.numel() == 0:
        return e, Excess(0.0, (), 0.0, 0.0, 0.0, 0.0, fp32_err)
    flat = int(e.argmax())
    idx = tuple(int(v) for v in np.unravel_index(flat, tuple(e.shape)))
    return e, Excess(float(e.reshape(-1)[flat]), idx, float(y[idx]), float(ref[idx]), float(r.scale.expand_as(ref)[idx]),
                     float(r.floor.expand_as(ref)[idx]), fp32_err)


def check(y, r, fp32=None, what=""):
    """Assert the yardstick (module docstring) and return the worst element (Excess)."""
    _, worst = excess(y, r, fp32)
    assert worst.value <= BOUND, (what, worst)
    if fp32 is not None:
        assert worst.value <= max(FP32_FACTOR * worst.fp32_err, FP32_CLASS_MIN), (what, worst)
    return worst


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------------
def _starts(shapes):
    hw = [(int(h), int(w)) for h, w in (shapes.tolist() if torch.is_tensor(shapes) else shapes)]
    st, acc = [], 0
    for h, w in hw:
        st.append(acc)
        acc += h * w
    return hw, st


class _Level:
    """Per-sample geometry of one level: positions, location error, in-range masks, corners and their weights."""

    def __init__(self, lx, ly, H, W, dlx=None, dly=None, exact=False):
        self.H, self.W = H, W
        px, py = lx * W - 0.5, ly * H - 0.5
        if exact:
            dx, dy = torch.zeros_like(px), torch.zeros_like(py)
        else:
            dx = 2.0 ** -23 * (px.abs() + 1)
            dy = 2.0 ** -23 * (py.abs() + 1)
            if dlx is not None:
                dx = dx + W * dlx
                dy = dy + H * dly
        fin = torch.isfinite(px) & torch.isfinite(py)
        dx, dy = torch.where(fin, dx, torch.zeros_like(dx)), torch.where(fin, dy, torch.zeros_like(dy))
        self.inr = fin & (px > -1) & (py > -1) & (px < W) & (py < H)
        self.near = fin & (px > -1 - dx) & (py > -1 - dy) & (px < W + dx) & (py < H + dy)
        pxs, pys = torch.where(self.near, px, torch.zeros_like(px)), torch.where(self.near, py, torch.zeros_like(py))
        self.x0, self.y0 = pxs.floor(), pys.floor()
        self.fx, self.fy = pxs - self.x0, pys - self.y0
        self.gx, self.gy = 1 - self.fx, 1 - self.fy
        self.dx, self.dy = dx, dy
        self.px, self.py = pxs, pys
        # within 2 d of an integer (a cell edge or a range limit): grad_loc of that coordinate jumps there
        self.edge_x = self.near & ((pxs - pxs.round()).abs() < 2 * dx)
        self.edge_y = self.near & ((pys - pys.round()).abs() < 2 * dy)

    def corners(self):
        """(dy, dx, weight) of the four corners in the order of msda_ref.c (v1 .. v4)."""
        return [(0, 0, self.gy * self.gx), (0, 1, self.gy * self.fx), (1, 0, self.fy * self.gx), (1, 1, self.fy * self.fx)]

    def neighbours(self):
        """(dy, dx, mask, which) of the corners of the neighbouring cells the kernel may use near a cell edge."""
        fx_n, gx_n = self.fx < self.dx, self.gx < self.dx
        fy_n, gy_n = self.fy < self.dy, self.gy < self.dy
        return [(0, -1, fx_n, "x"), (1, -1, fx_n, "x"), (0, 2, gx_n, "x"), (1, 2, gx_n, "x"),
                (-1, 0, fy_n, "y"), (-1, 1, fy_n, "y"), (2, 0, gy_n, "y"), (2, 1, gy_n, "y")]

    def index(self, cy, cx, start):
        """(flat pixel index clamped into the level, in-level mask) of corner (y0 + cy, x0 + cx)."""
        yi, xi = self.y0 + cy, self.x0 + cx
        ok = self.near & (yi >= 0) & (xi >= 0) & (yi <= self.H - 1) & (xi <= self.W - 1)
        pix = start + (yi.clamp(0, self.H - 1) * self.W + xi.clamp(0, self.W - 1)).long()
        return pix, ok


def _gather(value, pix, ok):
    """value [N, S, M, D] at pixel index pix [N, Q, M, P] (per batch and head) -> float64 [N, Q, M, P, D], zero where not ok."""
    N, S, M, D = value.shape
    n_i = torch.arange(N, device=value.device).view(N, 1, 1, 1)
    m_i = torch.arange(M, device=value.device).view(1, 1, M, 1)
    v = value[n_i, pix, m_i].double()
    return torch.where(ok[..., None], v, torch.zeros((), dtype=torch.float64, device=v.device))


def _split_loc(loc, l):
    return loc[:, :, :, l, :, 0].double(), loc[:, :, :, l, :, 1].double()


def forward_reference(value, shapes, loc, attn, dloc=None, da=None, exact=False, chunk=4096):
    """float64 forward of value [N, S, M, D], shapes [L, 2], loc [N, Lq, M, L, P, 2], attn [N, Lq, M, L, P] -> Ref of
    [N, Lq, M D].  dloc: (dlx, dly) [N, Lq, M, L, P] location errors of the fused entry; da: [N, Lq, M, L, P] its attention
    weight errors; exact: the positions are exact in fp32 (no location term)."""
    hw, st = _starts(shapes)
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    outs = []
    for q0 in range(0, Lq, chunk):
        sl = slice(q0, min(Lq, q0 + chunk))
        lc, ac = loc[:, sl], attn[:, sl].double()
        dac = None if da is None else da[:, sl].double()
        Q = lc.shape[1]
        ref = torch.zeros(N, Q, M, D, dtype=torch.float64, device=value.device)
        scale, floor = torch.zeros_like(ref), torch.zeros_like(ref)
        for l, (H, W) in enumerate(hw):
            lx, ly = _split_loc(lc, l)
            dlx = dly = None
            if dloc is not None:
                dlx, dly = dloc[0][:, sl][:, :, :, l].double(), dloc[1][:, sl][:, :, :, l].double()
            g = _Level(lx, ly, H, W, dlx, dly, exact)
            a = ac[:, :, :, l]
            aa = a.abs()
            samp = torch.zeros(N, Q, M, P, D, dtype=torch.float64, device=value.device)
            sabs, absum = torch.zeros_like(samp), torch.zeros_like(samp)
            for cy, cx, w in g.corners():
                pix, ok = g.index(cy, cx, st[l])
                v = _gather(value, pix, ok)
                samp = samp + w[..., None] * v
                va = v.abs()
                sabs = sabs + w[..., None] * va
                absum = absum + torch.nan_to_num(va, nan=0.0)
            ax, ay = absum, absum.clone()
            for cy, cx, m, which in g.neighbours():
                pix, ok = g.index(cy, cx, st[l])
                ok = ok & m
                if bool(ok.any()):
                    va = torch.nan_to_num(_gather(value, pix, ok).abs(), nan=0.0)
                    if which == "x":
                        ax = ax + va
                    else:
                        ay = ay + va
            inr = g.inr[..., None]
            zero = torch.zeros((), dtype=torch.float64, device=value.device)
            ref = ref + torch.where(inr, a[..., None] * samp, zero).sum(3)
            scale = scale + torch.where(inr, aa[..., None] * sabs, zero).sum(3)
            loc_t = g.dx[..., None] * ax + g.dy[..., None] * ay
            fl = torch.where(g.near[..., None], aa[..., None] * loc_t, zero)
            if dac is not None:
                fl = fl + torch.where(inr, dac[:, :, :, l][..., None] * torch.nan_to_num(sabs, nan=0.0), zero)
            floor = floor + fl.sum(3)
        floor = floor + SUB * (4 + 12 * L * P)
        outs.append((ref, scale, floor))
    ref = torch.cat([o[0] for o in outs], 1).reshape(N, Lq, M * D)
    scale = torch.cat([o[1] for o in outs], 1).reshape(N, Lq, M * D)
    floor = torch.cat([o[2] for o in outs], 1).reshape(N, Lq, M * D)
    return Ref(ref, torch.nan_to_num(scale, nan=0.0), floor, torch.isnan(ref), 4 * L * P)


def backward_reference(value, shapes, loc, attn, grad_out, exact=False, chunk=2048):
    """float64 gradients -> (Ref of grad_value [N, S, M, D], Ref of grad_loc [N, Lq, M, L, P, 2], Ref of grad_attn
    [N, Lq, M, L, P], fraction of grad_loc coordinates left out)."""
    hw, st = _starts(shapes)
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    dev = value.device
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    gv = torch.zeros(N * S * M, D, dtype=torch.float64, device=dev)
    gv_s, gv_f = torch.zeros_like(gv), torch.zeros_like(gv)
    gv_k = torch.zeros(N * S * M, dtype=torch.float64, device=dev)
    gl = torch.zeros(N, Lq, M, L, P, 2, dtype=torch.float64, device=dev)
    gl_s, gl_f = torch.zeros_like(gl), torch.zeros_like(gl)
    gl_keep = torch.ones(gl.shape, dtype=torch.bool, device=dev)
    ga = torch.zeros(N, Lq, M, L, P, dtype=torch.float64, device=dev)
    ga_s, ga_f = torch.zeros_like(ga), torch.zeros_like(ga)
    n_i = torch.arange(N, device=dev).view(N, 1, 1, 1)
    m_i = torch.arange(M, device=dev).view(1, 1, M, 1)
    go = grad_out.reshape(N, Lq, M, D)
    for q0 in range(0, Lq, chunk):
        sl = slice(q0, min(Lq, q0 + chunk))
        lc, ac = loc[:, sl], attn[:, sl].double()
        g = go[:, sl].double()[:, :, :, None, :]          # [N, Q, M, 1, D]
        gabs = g.abs()
        for l, (H, W) in enumerate(hw):
            lx, ly = _split_loc(lc, l)
            geo = _Level(lx, ly, H, W, exact=exact)
            a = ac[:, :, :, l]
            aa = a.abs()
            inr = geo.inr[..., None]
            near = geo.near[..., None]
            vs = []
            samp = torch.zeros(a.shape + (D,), dtype=torch.float64, device=dev)
            sabs, absum = torch.zeros_like(samp), torch.zeros_like(samp)
            for cy, cx, w in geo.corners():
                pix, ok = geo.index(cy, cx, st[l])
                v = _gather(value, pix, ok)
                vs.append(v)
                samp = samp + w[..., None] * v
                sabs = sabs + w[..., None] * v.abs()
                absum = absum + torch.nan_to_num(v.abs(), nan=0.0)
                # grad_value: a w g into the corner's row
                rows = ((n_i * S + pix) * M + m_i)
                okc = ok & geo.inr
                contrib = torch.where(okc[..., None], (a * w)[..., None] * g, zero)
                gv.index_add_(0, rows[okc], contrib[okc])
                gv_s.index_add_(0, rows[okc], contrib[okc].abs())
                gv_k.index_add_(0, rows[okc], torch.ones_like(rows[okc], dtype=torch.float64))
                okn = ok & geo.near
                fl = (aa * (geo.dx + geo.dy))[..., None] * gabs
                gv_f.index_add_(0, rows[okn], fl.expand(okn.shape + (D,))[okn])
            ax, ay = absum, absum.clone()
            for cy, cx, m, which in geo.neighbours():
                pix, ok = geo.index(cy, cx, st[l])
                ok = ok & m
                if not bool(ok.any()):
                    continue
                va = torch.nan_to_num(_gather(value, pix, ok).abs(), nan=0.0)
                d = geo.dx if which == "x" else geo.dy
                if which == "x":
                    ax = ax + va
                else:
                    ay = ay + va
                rows = ((n_i * S + pix) * M + m_i)
                fl = (aa * d)[..., None] * gabs
                gv_f.index_add_(0, rows[ok], fl.expand(ok.shape + (D,))[ok])
            # grad_attn
            ga[:, sl, :, l] = torch.where(inr, g * samp, zero).sum(-1)
            ga_s[:, sl, :, l] = torch.where(inr, gabs * torch.nan_to_num(sabs, nan=0.0), zero).sum(-1)
            ga_f[:, sl, :, l] = torch.where(near, gabs * (geo.dx[..., None] * ax + geo.dy[..., None] * ay), zero).sum(-1) \
                + SUB * 12 * D
            # grad_loc
            v1, v2, v3, v4 = vs
            cwx = geo.gy[..., None] * (v2 - v1) + geo.fy[..., None] * (v4 - v3)
            cwy = geo.gx[..., None] * (v3 - v1) + geo.fx[..., None] * (v4 - v2)
            base = (gabs * absum).sum(-1) * aa                             # |a| sum_d |g_d| sum_c |v_c|
            base_in = torch.where(geo.inr, base, zero)
            base_near = torch.where(geo.near, base, zero)    # (a sample within d of the range: the kernel may take it)
            gl[:, sl, :, l, :, 0] = torch.where(geo.inr, W * a * (g * cwx).sum(-1), zero)
            gl[:, sl, :, l, :, 1] = torch.where(geo.inr, H * a * (g * cwy).sum(-1), zero)
            gl_s[:, sl, :, l, :, 0] = W * base_in
            gl_s[:, sl, :, l, :, 1] = H * base_in
            gl_f[:, sl, :, l, :, 0] = geo.dy * W * base_near + SUB * W * (8 * D + 8)
            gl_f[:, sl, :, l, :, 1] = geo.dx * H * base_near + SUB * H * (8 * D + 8)
            gl_keep[:, sl, :, l, :, 0] = ~geo.edge_x
            gl_keep[:, sl, :, l, :, 1] = ~geo.edge_y
    gv_f = gv_f + SUB * (4 * gv_k[:, None] + 4)
    shape = (N, S, M, D)
    r_gv = Ref(gv.reshape(shape), gv_s.reshape(shape), gv_f.reshape(shape), torch.zeros(shape, dtype=torch.bool, device=dev),
               gv_k.reshape(N, S, M, 1).expand(shape))
    r_gl = Ref(gl, torch.nan_to_num(gl_s, nan=0.0), gl_f, torch.isnan(gl), 4 * D, gl_keep)
    r_ga = Ref(ga, torch.nan_to_num(ga_s, nan=0.0), ga_f, torch.isnan(ga), 4 * D)
    left_out = 1.0 - float(gl_keep.double().mean())
    return r_gv, r_gl, r_ga, left_out


def fused_locations(shapes, ref_points, qproj, M, L, P):
    """The fused entry's prologue in float64 from the fp32 qproj [N, Lq, >= 3 M L P] (offsets, then logits) and reference
    points [N, Lq, L, 2|4] -> (loc [N, Lq, M, L, P, 2], attn, (dlx, dly), da) for forward_reference(dloc=, da=)."""
    hw, _ = _starts(shapes)
    N, Lq = qproj.shape[:2]
    LP = L * P
    q = qproj.double()
    off = q[..., :2 * M * LP].reshape(N, Lq, M, L, P, 2)
    z = q[..., 2 * M * LP:3 * M * LP].reshape(N, Lq, M, LP)
    zmax = z.amax(-1, keepdim=True)
    a = torch.softmax(z, -1)
    d = (z - zmax).abs()
    per = a * U32 * (3 + 3 * d)
    common = U32 * (LP + 2 + (a * (3 + 3 * d)).sum(-1, keepdim=True))
    da = (per + a * common + SMALLEST_NORMAL).reshape(N, Lq, M, L, P)
    a = a.reshape(N, Lq, M, L, P)
    r = ref_points.double()
    if r.shape[-1] == 2:
        hws = torch.tensor(hw, dtype=torch.float64, device=q.device)          # (H, W): x / H_l, y / W_l as written
        t = off / hws.view(1, 1, 1, L, 1, 2)
        base = r[:, :, None, :, None, :]
    else:
        t = off / P * r[:, :, None, :, None, 2:] * 0.5
        base = r[:, :, None, :, None, :2]
    loc = base + t
    dl = 2.0 ** -22 * t.abs() + 2.0 ** -23 * loc.abs()
    return loc, a, (dl[..., 0], dl[..., 1]), da


def oracle_f64_forward(value, shapes, loc, attn):
    """oracle/msda_ref.c's float64 path on the same fp32 inputs (numpy)."""
    from oracle import msda_oracle
    return msda_oracle.msda_forward(_np(value).astype(np.float64), _np(shapes), _np(loc).astype(np.float64),
                                    _np(attn).astype(np.float64), nthreads=8)


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


# ---- operand profiles -------------------------------------------------------------------------------------------------------------------
def encoder_refs(shapes, N, M, L, P):
    """One query per pyramid pixel at its pixel centre -> [N, S, M, L, P, 2]."""
    hw, _ = _starts(shapes)
    pts = torch.cat([torch.stack(torch.meshgrid((torch.arange(w) + 0.5) / w, (torch.arange(h) + 0.5) / h, indexing="xy"), -1)
                     .reshape(-1, 2) for h, w in hw])
    return pts.view(1, -1, 1, 1, 1, 2).expand(N, -1, M, L, P, 2)


def make_case(profile, N, M, D, Lq, P, shapes, seed, encoder=False):
    """Seeded fp32 (value [N, S, M, D], shapes, loc, attn, grad_out) on the CPU for `profile` (module PROFILES)."""
    g = torch.Generator().manual_seed(seed)
    hw, st = _starts(shapes)
    L = len(hw)
    S = sum(h * w for h, w in hw)
    shp = torch.tensor(hw, dtype=torch.long)
    value = torch.randn(N, S, M, D, generator=g)
    sz = torch.tensor([(w, h) for h, w in hw], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    if encoder or (profile == "permuted" and Lq == S):
        assert Lq == S
        base = encoder_refs(hw, N, M, L, P)
    else:
        base = torch.rand(N, Lq, 1, 1, 1, 2, generator=g)
    loc = base + torch.randn(N, Lq, M, L, P, 2, generator=g) * 2.0 / sz          # local: N(0, 2 px) around the reference
    attn = torch.rand(N, Lq, M, L, P, generator=g) + 1e-3
    attn = attn / attn.sum((-1, -2), keepdim=True)
    grad_out = torch.randn(N, Lq, M * D, generator=g)
    if profile == "wide":
        loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.6 - 0.3
    elif profile == "signed":
        attn = attn * torch.where(torch.rand(attn.shape, generator=g) < 0.5, -1.0, 1.0)
    elif profile == "large":
        value = value * 2.0 ** 60
    elif profile == "small":
        value = value * 2.0 ** -60
        tiny = torch.rand(attn.shape, generator=g) < 0.2                          # a * w * v in the fp32 subnormals
        attn = torch.where(tiny, attn * 2.0 ** -70, attn)
    elif profile == "level_spread":
        for l, (h, w) in enumerate(hw):
            value[:, st[l]:st[l] + h * w] *= 2.0 ** (10 * (l % 4))
    elif profile == "hot_pixel":
        # half of the samples of every level land next to one of three pixels (fixed fractional offsets: four nonzero weights)
        hot = torch.rand(N, Lq, M, L, P, generator=g) < 0.5
        k = torch.randint(0, 3, (N, Lq, M, L, P), generator=g)
        whs = sz.expand(N, Lq, M, L, P, 2)
        cx = (k.float() * 0.37 * whs[..., 0]).floor().clamp(max=whs[..., 0] - 1)
        cy = (k.float() * 0.29 * whs[..., 1]).floor().clamp(max=whs[..., 1] - 1)
        hx = (cx + 0.5 + 0.3) / whs[..., 0]
        hy = (cy + 0.5 + 0.2) / whs[..., 1]
        loc = torch.where(hot[..., None], torch.stack([hx, hy], -1), loc)
    elif profile == "permuted":
        perm = torch.randperm(Lq, generator=g)
        loc, attn = loc[:, perm], attn[:, perm]
    elif profile not in ("unit",):
        raise ValueError(profile)
    return value.contiguous(), shp, loc.contiguous(), attn.contiguous(), grad_out.contiguous()


def make_fused_case(profile, N, M, D, Lq, P, shapes, seed, ref_dim=2, encoder=False):
    """Seeded fp32 (value, shapes, reference points [N, Lq, L, ref_dim], qproj [N, Lq, 3 M L P]) for the fused entry."""
    g = torch.Generator().manual_seed(seed)
    hw, st = _starts(shapes)
    L = len(hw)
    S = sum(h * w for h, w in hw)
    value = torch.randn(N, S, M, D, generator=g)
    qproj = torch.randn(N, Lq, 3 * M * L * P, generator=g)
    qproj[..., :2 * M * L * P] *= 2.0
    if encoder:
        assert Lq == S and ref_dim == 2
        refp = encoder_refs(hw, N, 1, L, 1)[:, :, 0, :, 0, :].contiguous()
    elif ref_dim == 2:
        refp = torch.rand(N, Lq, L, 2, generator=g) * 0.8 + 0.1
    else:
        refp = torch.cat([torch.rand(N, Lq, L, 2, generator=g) * 0.8 + 0.1, torch.rand(N, Lq, L, 2, generator=g) * 0.3 + 0.05], -1)
    if profile == "wide":
        qproj[..., :2 * M * L * P] *= 8.0
    elif profile == "large":
        value = value * 2.0 ** 60
    elif profile == "small":
        value = value * 2.0 ** -60
    elif profile == "level_spread":
        for l, (h, w) in enumerate(hw):
            value[:, st[l]:st[l] + h * w] *= 2.0 ** (10 * (l % 4))
    elif profile == "large_logits":
        qproj[..., 2 * M * L * P:] *= 30.0
    elif profile != "unit":
        raise ValueError(profile)
    return value.contiguous(), torch.tensor(hw, dtype=torch.long), refp.contiguous(), qproj.contiguous()


def exact_edge_case(N, M, D, P, shapes, seed, Lq=None):
    """Positions exact in fp32 on power-of-two levels: px, py in {-1, -1 + ulp, -0.5, integer centres, W - 1, W - 0.5,
    W - ulp, W} (out-of-range -1 and W included) -> (value, shapes, loc, attn, grad_out) with enough queries to cover every
    pair of positions (or Lq of them: an encoder-shaped call)."""
    hw, _ = _starts(shapes)
    for h, w in hw:
        assert h & (h - 1) == 0 and w & (w - 1) == 0, "exact positions need power-of-two level sizes"
    g = torch.Generator().manual_seed(seed)
    L = len(hw)

    def positions(size):
        # px in {-1, -1 + 2^-24, -0.5, 0, 1, 2, size - 1, size - 0.5, size - ulp, size}; size - ulp = size (1 - 2^-23) is the
        # last position below size whose loc = (px + 0.5) / size is an fp32 number
        pxs = [-1.0, -1.0 + 2.0 ** -24, -0.5] + [float(k) for k in range(min(size, 3))] + \
              [size - 1.0, size - 0.5, size * (1 - 2.0 ** -23), float(size)]
        locs = sorted({(p + 0.5) / size for p in pxs})
        for v in locs:
            assert float(np.float32(v)) == v
        return np.array(locs, np.float32)

    per_level = [(positions(w), positions(h)) for h, w in hw]
    K = max(len(px) * len(py) for px, py in per_level)
    Lq = Lq or -(-K // P)
    loc = torch.zeros(N, Lq, M, L, P, 2)
    for l, (px, py) in enumerate(per_level):
        grid = torch.from_numpy(np.stack(np.meshgrid(px, py, indexing="ij"), -1).reshape(-1, 2))
        idx = torch.arange(Lq * P) % grid.shape[0]
        pts = grid[idx].view(Lq, P, 2)
        for m in range(M):
            loc[:, :, m, l] = pts.roll(m, 0)
    S = sum(h * w for h, w in hw)
    value = torch.randn(N, S, M, D, generator=g)
    attn = torch.rand(N, Lq, M, L, P, generator=g) + 0.1
    attn = attn / attn.sum((-1, -2), keepdim=True)
    grad_out = torch.randn(N, Lq, M * D, generator=g)
    # every position really is exact: fl32(loc W - 0.5) == loc W - 0.5 in float64
    for l, (h, w) in enumerate(hw):
        for c, size in ((0, w), (1, h)):
            p64 = loc[:, :, :, l, :, c].double() * size - 0.5
            assert torch.equal(p64.float().double(), p64)
    return value, torch.tensor(hw, dtype=torch.long), loc, attn, grad_out


def add_nan_pixels(value, loc, shapes, count, seed):
    """NaN at `count` pixels of `value` (all heads and channels of them) that no sample reads at exactly zero weight: pixels
    one of whose neighbours is read at a zero weight are skipped.  Returns the pixel rows."""
    hw, st = _starts(shapes)
    g = torch.Generator().manual_seed(seed)
    N, S, M, D = value.shape
    L = len(hw)
    zero_hit = torch.zeros(S, dtype=torch.bool)
    for l, (H, W) in enumerate(hw):
        lx, ly = _split_loc(loc, l)
        geo = _Level(lx, ly, H, W, exact=True)
        for cy, cx, w in geo.corners():
            pix, ok = geo.index(cy, cx, st[l])
            hit = ok & geo.inr & (w == 0)
            zero_hit[pix[hit].unique()] = True
    cand = (~zero_hit).nonzero().view(-1)
    rows = cand[torch.randperm(cand.numel(), generator=g)[:count]]
    value[:, rows] = float("nan")
    return rows
