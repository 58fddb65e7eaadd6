"""The float64 yardstick of the fused mask losses (trackformer_amd/csrc/mask_loss.h; include/tf_fused.h: THE MASK LOSSES), the cases
their tests draw from and the checks both test files share.  The value-with-error-scale type V, the bound, the floor, the logit
profiles and the second criterion are those of tests/util_criterion_fused.py (imported, unchanged); this file states the reference of
the two losses and of the gradient entering pred_masks ONCE, in V:

    lambda          the interpolation weight (num % (2 H)) / (2 H) of the integer coordinates is a LEAF with E = |lambda|: the kernel
                    rounds it once
    x               the upsampled logit (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11): V arithmetic
    focal elements  util_criterion_fused.focal_reference (the stable form; S = |ref| (1 + gamma |log(1 - p_t)|)) plus |d focal / dx| E(x);
                    their gradients likewise, with the second derivative from float64 autograd through the same formula
    p, p (1 - p)    from e = exp(-|x|), inv = 1 / (1 + e): V arithmetic
    sums            V.sum: accumulated wider than fp32 and rounded once
    losses          sum_i (focal_i / (H W)) / num_boxes and sum_i (1 - (2 spt_i + 1) / (sp_i + st_i + 1)) / num_boxes: V arithmetic
    gradient        a source pixel's sum of the V terms (wy wx) g_x over the output pixels that have it as a corner, as V.sum;
                    g_x = cm dfocal/dx + cd[t] p (1 - p) with cm, cd in V arithmetic from G, num_boxes and the pairs' sums

    (|got - ref| - 4 . 2^-149) / S  <=  2^-20        no element exempt

SECOND CRITERION: at most FP32_FACTOR x the excess of torch's own fp32 SetCriterion.loss_masks on the CPU, or FP32_CLASS_MIN, applied
only where torch's own excess is itself within the bound (on `wide` logits its 1 - sigmoid(x) loses the gradients: it bounds nothing
there, as the docstring of util_criterion_fused describes for the class loss).

THE KERNELS' OWN FIGURES, first run on an MI355X (tests/test_mask_losses_gpu.py; worst normalised excess over all its cases in units
of 2^-20): losses 0.010 (tiny logits; 0.009 unit, 0.007 wide), gradient 0.024 (wide; 0.015 unit, 0.016 tiny); torch's own fp32 chain on
the same cases: losses 0.019, gradient 0.11 on unit and tiny logits and 6.7e3 on wide ones (the 9 x 9 -> 9 x 9 case), where it bounds
nothing.  The emulated library (the host's libm) gives the same figures to the digits shown (tests/test_mask_losses_cpu.py -s).

Everything here is torch, float64, and runs on the CPU or the device."""
import torch
import torch.nn.functional as F

from tests import util_criterion_fused as Y
from trackformer_amd import criterion

V = Y.V
BOUND, LOGIT_PROFILES = Y.BOUND, Y.LOGIT_PROFILES
OUTPUTS = ("losses", "grad")
TILE_ROWS = 8          # the forward's tile rule (csrc/mask_loss.h: kMaskTileRows): tiles = ceil(H / 8), a function of the shape alone

# (h, w, H, W): the smallest at which each thing can go wrong
SHAPES = [
    (5, 7, 19, 23),         # non-integer ratios; odd W: target rows are misaligned
    (16, 20, 64, 80),       # ratio 4
    (16, 20, 128, 160),     # ratio 8, the training fixture's image; 16 row tiles per pair: the second launch adds several partials
    (9, 9, 9, 9),           # ratio 1: every lambda is 0
    (13, 21, 100, 167),     # mixed non-integer ratios; wider than one wave in x
    (1, 1, 6, 5),           # every output pixel clamps to the one source pixel
    (2, 3, 7, 3),           # w == W with h upsampled
    (3, 50, 10, 300),       # wider than one 256-column chunk: the workgroup walks two chunks and stages the source columns twice
]
TARGET_KINDS = ("box", "zeros", "ones")
B, Q = 2, 4                                  # the rows of pred_masks: two images of four queries
PER_IMAGE = (3, 2)                           # target masks per image: the padded stack has 2 x 3 rows, one of them padding
PAIRS = {0: [], 1: [(1, 1, 1)], 3: [(0, 1, 2), (0, 3, 0), (1, 2, 1)]}   # n -> (image, query, target of the image): unmatched rows between


def tiles_of(H):
    return (H + TILE_ROWS - 1) // TILE_ROWS


class Case:
    """One seeded problem: pred_masks [B, Q, h, w] fp32, the images' target masks (bool [n_b, H, W]) and their padded stack [T, H, W], a
    matching of n pairs, and the weights G of a weighted sum of the two losses."""

    def __init__(self, shape, n=3, profile="unit", targets="box", seed=0, device="cpu"):
        h, w, H, W = shape
        gen = torch.Generator().manual_seed(1000003 * seed + 7919 * h + 101 * w + 13 * H + W + n)
        self.shape, self.n, self.profile, self.kind, self.seed = shape, n, profile, targets, seed
        self.pred_masks = (torch.randn(B, Q, h, w, generator=gen) * LOGIT_PROFILES[profile]).contiguous()
        masks = []
        for nb in PER_IMAGE:
            m = torch.zeros(nb, H, W, dtype=torch.bool)
            for k in range(nb):
                if targets == "ones":
                    m[k] = True
                elif targets == "box":
                    y0, x0 = int(torch.randint(0, H, (1,), generator=gen)), int(torch.randint(0, W, (1,), generator=gen))
                    y1, x1 = int(torch.randint(y0, H, (1,), generator=gen)) + 1, int(torch.randint(x0, W, (1,), generator=gen)) + 1
                    m[k, y0:y1, x0:x1] = True
            masks.append(m)
        self.masks = masks
        self.per_image = max(PER_IMAGE)
        stack = torch.zeros(B, self.per_image, H, W, dtype=torch.bool)
        for b, m in enumerate(masks):
            stack[b, :m.shape[0]] = m
        self.tgt = stack.flatten(0, 1).contiguous()                     # [T, H, W], T = 6 > n
        pairs = PAIRS[n]
        self.indices = [(torch.tensor([q for (i, q, _) in pairs if i == b], dtype=torch.int64),
                         torch.tensor([t for (i, _, t) in pairs if i == b], dtype=torch.int64)) for b in range(B)]
        self.pair_src = torch.tensor([b * Q + q for (b, q, _) in pairs], dtype=torch.int32)
        self.pair_tgt = torch.tensor([b * self.per_image + t for (b, _, t) in pairs], dtype=torch.int32)
        self.row_pair = torch.full((B * Q,), -1, dtype=torch.int32)
        self.row_pair[self.pair_src.long()] = torch.arange(n, dtype=torch.int32)
        self.num_boxes = float(max(n, 1))
        self.G = torch.rand(2, generator=gen) + 0.5
        self.device = device
        if device != "cpu":
            for k in ("pred_masks", "tgt", "pair_src", "pair_tgt", "row_pair", "G"):
                setattr(self, k, getattr(self, k).to(device))
            self.masks = [m.to(device) for m in self.masks]

    def what(self):
        return "%s / %s %r n%d" % (self.profile, self.kind, self.shape, self.n)

    def targets(self, device=None):
        """The targets as SetCriterion.loss_masks takes them."""
        return [{"masks": m.to(device or m.device), "labels": torch.zeros(m.shape[0], dtype=torch.int64, device=device or m.device)}
                for m in self.masks]


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def coords(n_in, n_out, device="cpu"):
    """The integer coordinates of one axis -> (i0 int64 [n_out], i1 int64 [n_out], lambda float64 [n_out], exact quotients)."""
    o = torch.arange(n_out, dtype=torch.int64, device=device)
    num = ((2 * o + 1) * n_in - n_out).clamp_min(0)
    i0 = num // (2 * n_out)
    lam = (num % (2 * n_out)).double() / (2 * n_out)
    return i0, i0 + (i0 < n_in - 1).long(), lam


def upsample(s, H, W):
    """s float64 [n, h, w] -> (x V [n, H, W], the four corner weights as V [H, W] and the corner indices)."""
    h, w = s.shape[-2:]
    y0, y1, ly = coords(h, H, s.device)
    x0, x1, lx = coords(w, W, s.device)
    ly, lx = V(ly[:, None], ly[:, None].abs()), V(lx[None, :], lx[None, :].abs())
    my, mx = 1.0 - ly, 1.0 - lx

    def at(yi, xi):
        return V(s[:, yi][:, :, xi])
    x = my * (mx * at(y0, x0) + lx * at(y0, x1)) + ly * (mx * at(y1, x0) + lx * at(y1, x1))
    corners = (((y0, x0), my * mx), ((y0, x1), my * lx), ((y1, x0), ly * mx), ((y1, x1), ly * lx))
    return x, corners


def _focal(x, pos, alpha, gamma):
    """focal_reference at the V logit x: the elements, their derivative, both with |d/dx| E(x) added."""
    with torch.enable_grad():
        xv = x.v.detach().clone().requires_grad_(True)
        f, df = Y.focal_reference(xv, pos, alpha, gamma)
        d2, = torch.autograd.grad(df.v.sum(), xv)
    f, df = V(f.v.detach(), f.E.detach()), V(df.v.detach(), df.E.detach())
    return V(f.v, f.E + df.v.abs() * x.E), V(df.v, df.E + d2.abs() * x.E)


def reference(case, alpha, gamma):
    """{"losses": V [2], "grad": V [B, Q, h, w]} in float64 on the case's device; the gradient is that of sum(G * losses)."""
    h, w, H, W = case.shape
    dev = case.pred_masks.device
    n = case.n
    src = case.pred_masks.double().view(B * Q, h, w)
    grad = V(torch.zeros(B * Q, h, w, dtype=torch.float64, device=dev))
    if n == 0:
        return {"losses": V(torch.zeros(2, dtype=torch.float64, device=dev)), "grad": V(grad.v.view(B, Q, h, w), grad.E.view(B, Q, h, w))}
    rows = case.pair_src.long()
    pos = case.tgt[case.pair_tgt.long()] != 0
    x, corners = upsample(src[rows], H, W)
    f, df = _focal(x, pos, alpha, gamma)
    e = (-x.abs()).exp()
    inv = 1.0 / (1.0 + e)
    p = V.where(x.v >= 0, inv, e * inv)
    pq = inv * (e * inv)
    zero = V(torch.zeros_like(x.v))
    nb = V(torch.tensor(case.num_boxes, dtype=torch.float64, device=dev))
    hw = V(torch.tensor(float(H * W), dtype=torch.float64, device=dev))
    sf, spt, sp = f.sum((1, 2)), V.where(pos, p, zero).sum((1, 2)), p.sum((1, 2))
    st = V(pos.double().sum((1, 2)))                                   # a count: exact
    num, den = spt.exact(2.0) + 1.0, (sp + st) + 1.0
    loss_mask = (sf / hw).sum(0) / nb
    loss_dice = (1.0 - num / den).sum(0) / nb
    G = V(case.G.double())
    cm = G[0] / (nb * hw)
    gd = G[1] / nb
    cd0, cd1 = gd * (num / (den * den)), gd * (-(den.exact(2.0) - num) / (den * den))
    g = cm * df + V.where(pos, cd1[:, None, None], cd0[:, None, None]) * pq         # [n, H, W]
    gv = torch.zeros(n, h * w, dtype=torch.float64, device=dev)
    gE = torch.zeros_like(gv)
    for (yi, xi), wgt in corners:
        term = wgt * g
        idx = (yi[:, None] * w + xi[None, :]).reshape(-1)
        gv.index_add_(1, idx, term.v.reshape(n, -1))
        gE.index_add_(1, idx, term.E.reshape(n, -1))
    grad.v[rows] = gv.view(n, h, w)
    grad.E[rows] = (gE + gv.abs()).view(n, h, w)
    return {"losses": Y.stack([loss_mask, loss_dice]), "grad": V(grad.v.view(B, Q, h, w), grad.E.view(B, Q, h, w))}


def torch_loss_masks(case, pred_masks, alpha=0.25, gamma=2.0):
    """SetCriterion.loss_masks (today's lines) on `pred_masks` -> [2]; with another alpha / gamma than loss_masks' own, the same lines
    with them."""
    dev = pred_masks.device
    if (alpha, gamma) == (0.25, 2.0):
        out = Y.criterion_for(1, alpha, gamma).loss_masks({"pred_masks": pred_masks}, case.targets(dev), case.indices, case.num_boxes)
        return torch.stack([out["loss_mask"], out["loss_dice"]])
    tm = case.tgt.to(dev)[case.pair_tgt.long().to(dev)].to(pred_masks).flatten(1)
    sm = F.interpolate(pred_masks.flatten(0, 1)[case.pair_src.long().to(dev)][:, None], size=case.shape[2:], mode="bilinear",
                       align_corners=False)[:, 0].flatten(1)
    return torch.stack([criterion.sigmoid_focal_loss(sm, tm, case.num_boxes, alpha=alpha, gamma=gamma),
                        criterion.dice_loss(sm, tm, case.num_boxes)])


def fp32_formulation(case, alpha, gamma):
    """torch's own fp32 loss_masks and autograd through it, on the CPU."""
    if case.n == 0:
        return None
    cpu = case if case.device == "cpu" else Case(case.shape, case.n, case.profile, case.kind, seed=case.seed)   # (seeded: the same tensors)
    with torch.enable_grad():
        pm = cpu.pred_masks.detach().clone().requires_grad_(True)
        losses = torch_loss_masks(cpu, pm, alpha, gamma)
        grad, = torch.autograd.grad((losses * cpu.G).sum(), pm)
    return {"losses": losses.detach(), "grad": grad}


def check(got, ref, fp32, what=""):
    """Both criteria for both outputs -> {name: Excess}; prints the figures (pytest -s) before it asserts."""
    return {name: Y.check_one(name, got[name].detach().cpu(), V(ref[name].v.cpu(), ref[name].E.cpu()), None if fp32 is None else fp32[name],
                              what) for name in OUTPUTS}
