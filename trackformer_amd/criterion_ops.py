"""The operators over the set-criterion and matching-cost kernels (include/tf_fused.h: THE SET CRITERION AND THE MATCHING COST;
csrc/criterion.h), re-exported as fused.set_criterion / fused.match_cost / fused.criterion_applies.

The losses of the stacked decoder layers (criterion.SetCriterion._layers_at_once: several dozen library launches forward, as many again
in the backward) in ONE launch each way, and the matcher's focal cost matrix in one.  The switches live with their callers --
criterion.set_fused() / TF_CRITERION_FUSED=1 and matcher.set_fused_cost() / TF_MATCHER_FUSED_COST=1, both OFF by default --; the
functions here are the plain operators.

The mask losses of the matched pairs (SetCriterion.loss_masks: a bilinear upsampling to the padded image size and about 25 element-wise
passes over [n, H, W] fp32 tensors) are mask_losses / mask_losses_applies below (include/tf_fused.h: THE MASK LOSSES; csrc/mask_loss.h),
behind criterion.set_fused_masks() / TF_CRITERION_FUSED_MASKS=1, OFF by default."""
import torch

from . import _cabi


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _labels_in_range(labels, hi, what):
    """The labels live on the device and the kernels do not assert: one copy of T integers to the host, checked there."""
    if labels is not None and labels.numel() > 0:
        lab = labels.cpu()
        if int(lab.min()) < 0 or int(lab.max()) > hi:
            _cabi.check(-2, "%s (a label outside [0, %d])" % (what, hi))


class _SetCriterion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, boxes, tgt_of, labels, tboxes, tgt_len, alpha, gamma, num_boxes):
        L, B, Q, C = logits.shape
        T = 0 if labels is None else labels.numel()
        with torch.cuda.device(logits.device):
            losses = torch.empty((L, 3), dtype=torch.float32, device=logits.device)
            card = torch.empty((L,), dtype=torch.float32, device=logits.device)
            class_error = torch.empty((1,), dtype=torch.float32, device=logits.device)
            rc = _cabi.lib().tf_set_criterion_fwd_f32(logits.data_ptr(), boxes.data_ptr(), tgt_of.data_ptr(), _ptr(labels), _ptr(tboxes),
                                                      tgt_len.data_ptr(), losses.data_ptr(), card.data_ptr(), class_error.data_ptr(), L, B, Q,
                                                      C, T, alpha, gamma, num_boxes, _stream(logits.device))
        _cabi.check(rc, "tf_set_criterion_fwd_f32")
        ctx.save_for_backward(logits, boxes, tgt_of, labels, tboxes)   # the inputs only: the backward recomputes
        ctx.scalars = (alpha, gamma, num_boxes)
        ctx.mark_non_differentiable(card, class_error)
        return losses, card, class_error

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_losses, _g_card, _g_class_error):
        logits, boxes, tgt_of, labels, tboxes = ctx.saved_tensors
        alpha, gamma, num_boxes = ctx.scalars
        L, B, Q, C = logits.shape
        T = 0 if labels is None else labels.numel()
        G = g_losses.to(torch.float32).contiguous()
        gl = gb = None
        with torch.cuda.device(logits.device):
            if ctx.needs_input_grad[0]:
                gl = torch.empty_like(logits)
            if ctx.needs_input_grad[1]:
                gb = torch.empty_like(boxes)
            if gl is not None or gb is not None:
                rc = _cabi.lib().tf_set_criterion_bwd_f32(G.data_ptr(), logits.data_ptr(), boxes.data_ptr(), tgt_of.data_ptr(), _ptr(labels),
                                                          _ptr(tboxes), _ptr(gl), _ptr(gb), L, B, Q, C, T, alpha, gamma, num_boxes,
                                                          _stream(logits.device))
                _cabi.check(rc, "tf_set_criterion_bwd_f32")
        return gl, gb, None, None, None, None, None, None, None


def criterion_applies(logits, boxes):
    """The stacked predictions the criterion kernels take: fp32, on the device, contiguous [L, B, Q, C] / [L, B, Q, 4], boxes 16-byte
    aligned."""
    return (logits.is_cuda and logits.dtype == torch.float32 and boxes.dtype == torch.float32 and boxes.device == logits.device
            and logits.dim() == 4 and boxes.shape == logits.shape[:3] + (4,) and logits.numel() > 0 and logits.is_contiguous()
            and boxes.is_contiguous() and boxes.data_ptr() % 16 == 0)


def set_criterion(logits, boxes, tgt_of, labels, tboxes, tgt_len, alpha, gamma, num_boxes, check_labels=True):
    """The focal class, L1, GIoU and cardinality losses of L stacked decoder layers through tf_set_criterion_fwd_f32 /
    tf_set_criterion_bwd_f32 (include/tf_fused.h) -> (losses [L, 3] = (loss_ce, loss_bbox, loss_giou), differentiable with respect to
    logits and boxes; card [L]; class_error [1]).  logits [L, B, Q, C], boxes [L, B, Q, 4] fp32 on the device; tgt_of int32 [L, B, Q]
    (global target index or -1), labels int64 [T], tboxes fp32 [T, 4], tgt_len int32 [B]; labels / tboxes may be None for T == 0.
    Anything the kernels do not take is an error here, not a fall-back (the caller decides the route: criterion_applies).
    check_labels: copy the labels to the host and raise on one outside [0, C]."""
    if not criterion_applies(logits, boxes):
        raise ValueError("set_criterion: contiguous fp32 device tensors [L, B, Q, C] and [L, B, Q, 4] expected")
    T = 0 if labels is None else labels.numel()
    if T == 0:
        labels = tboxes = None
    else:
        if labels.dtype != torch.int64 or tboxes.dtype != torch.float32 or tuple(tboxes.shape) != (T, 4):
            raise ValueError("set_criterion: labels int64 [T] and tboxes fp32 [T, 4] expected")
        labels, tboxes = labels.contiguous(), tboxes.contiguous()
        if check_labels:
            _labels_in_range(labels, logits.shape[3], "tf_set_criterion_fwd_f32")
    if tgt_of.dtype != torch.int32 or tgt_of.numel() != logits.numel() // logits.shape[3] or tgt_len.dtype != torch.int32 \
            or tgt_len.numel() != logits.shape[1] or not tgt_of.is_contiguous() or not tgt_len.is_contiguous():
        raise ValueError("set_criterion: tgt_of int32 [L, B, Q] and tgt_len int32 [B] expected")
    return _SetCriterion.apply(logits, boxes, tgt_of, labels, tboxes, tgt_len, float(alpha), float(gamma), float(num_boxes))


def match_cost(logits, boxes, tgt_ids, tgt_bbox, w_class, w_bbox, w_giou, alpha, gamma, check_labels=True):
    """The focal matching cost [R, T] of HungarianMatcher.match_many through tf_match_cost_f32 (one launch; include/tf_fused.h), or
    None when the tensors are not fp32 / int64 on the device (the caller keeps the torch chain).  logits [R, C], boxes [R, 4],
    tgt_ids int64 [T], tgt_bbox [T, 4].  check_labels: copy tgt_ids to the host and raise on one outside [0, C)."""
    ok = (logits.is_cuda and logits.dtype == torch.float32 and boxes.dtype == torch.float32 and logits.dim() == 2 and boxes.dim() == 2
          and boxes.shape == (logits.shape[0], 4) and tgt_ids.dtype == torch.int64 and tgt_bbox.dtype == torch.float32
          and tgt_ids.device == logits.device and tgt_bbox.device == logits.device and tuple(tgt_bbox.shape) == (tgt_ids.numel(), 4))
    if not ok:
        return None
    logits, boxes, tgt_ids, tgt_bbox = logits.contiguous(), boxes.contiguous(), tgt_ids.contiguous(), tgt_bbox.contiguous()
    R, C = logits.shape
    T = tgt_ids.numel()
    if check_labels:
        _labels_in_range(tgt_ids, C - 1, "tf_match_cost_f32")
    with torch.cuda.device(logits.device):
        cost = torch.empty((R, T), dtype=torch.float32, device=logits.device)
        rc = _cabi.lib().tf_match_cost_f32(logits.data_ptr(), boxes.data_ptr(), tgt_ids.data_ptr(), tgt_bbox.data_ptr(), cost.data_ptr(), R, C,
                                           T, float(w_class), float(w_bbox), float(w_giou), float(alpha), float(gamma),
                                           _stream(logits.device))
    _cabi.check(rc, "tf_match_cost_f32")
    return cost


# ---- THE MASK LOSSES (include/tf_fused.h: THE MASK LOSSES; csrc/mask_loss.h) -----------------------------------------------------------
class _MaskLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_masks, tgt, pair_src, pair_tgt, row_pair, alpha, gamma, num_boxes):
        B, Q, h, w = pred_masks.shape
        T, H, W = tgt.shape
        n = pair_src.numel()
        dev = pred_masks.device
        lib = _cabi.lib()
        with torch.cuda.device(dev):
            losses = torch.empty((2,), dtype=torch.float32, device=dev)
            sums = torch.empty((n, 4), dtype=torch.float64, device=dev)
            nbytes = lib.tf_mask_loss_workspace_bytes(n, H, W)
            if nbytes < 0:
                _cabi.check(-2, "tf_mask_loss_workspace_bytes")
            ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
            rc = lib.tf_mask_loss_fwd_f32(pred_masks.data_ptr(), tgt.data_ptr(), pair_src.data_ptr(), pair_tgt.data_ptr(), sums.data_ptr(),
                                          losses.data_ptr(), ws.data_ptr(), nbytes, n, B * Q, T, h, w, H, W, alpha, gamma, num_boxes,
                                          _stream(dev))
        _cabi.check(rc, "tf_mask_loss_fwd_f32")
        ctx.save_for_backward(pred_masks, tgt, pair_tgt, row_pair, sums)   # the inputs and [n, 4] sums: the backward recomputes
        ctx.scalars = (alpha, gamma, num_boxes)
        return losses

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_losses):
        pred_masks, tgt, pair_tgt, row_pair, sums = ctx.saved_tensors
        alpha, gamma, num_boxes = ctx.scalars
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        B, Q, h, w = pred_masks.shape
        T, H, W = tgt.shape
        G = g_losses.to(torch.float32).contiguous()
        with torch.cuda.device(pred_masks.device):
            grad = torch.empty_like(pred_masks)
            rc = _cabi.lib().tf_mask_loss_bwd_f32(G.data_ptr(), pred_masks.data_ptr(), tgt.data_ptr(), pair_tgt.data_ptr(), row_pair.data_ptr(),
                                                  sums.data_ptr(), grad.data_ptr(), pair_tgt.numel(), B * Q, T, h, w, H, W, alpha, gamma,
                                                  num_boxes, _stream(pred_masks.device))
        _cabi.check(rc, "tf_mask_loss_bwd_f32")
        return (grad,) + (None,) * 7


def mask_losses_applies(pred_masks, target_masks):
    """What the mask-loss kernels take: fp32 contiguous pred_masks [B, Q, h, w] on the device and bool / uint8 target masks [T, H, W] on
    the same device with H >= h and W >= w (the kernels upsample; they do not downsample)."""
    return (pred_masks.is_cuda and pred_masks.dtype == torch.float32 and pred_masks.dim() == 4 and pred_masks.numel() > 0
            and pred_masks.is_contiguous() and target_masks.dtype in (torch.bool, torch.uint8) and target_masks.device == pred_masks.device
            and target_masks.dim() == 3 and target_masks.shape[1] >= pred_masks.shape[2] and target_masks.shape[2] >= pred_masks.shape[3])


def mask_losses(pred_masks, target_masks, pair_src, pair_tgt, alpha, gamma, num_boxes, row_pair=None):
    """The sigmoid focal and dice losses of the matched masks through tf_mask_loss_fwd_f32 / tf_mask_loss_bwd_f32 (include/tf_fused.h:
    THE MASK LOSSES) -> [2] = (loss_mask, loss_dice), differentiable with respect to pred_masks.  pred_masks [B, Q, h, w] fp32 on the
    device; target_masks bool / uint8 [T, H, W], the padded stack of all images' masks -- read as bytes, never converted or gathered;
    pair_src int32 [n] (b * Q + q of every matched prediction), pair_tgt int32 [n] (its row of target_masks); row_pair int32 [B * Q]
    (the pair of each row or -1; built here on the device when None -- the route uploads it with the pairs).  The bilinear upsampling to
    H x W happens inside the kernels; only pred_masks, the index tensors and [n, 4] sums are kept for the backward.  Anything the kernels
    do not take is an error here, not a fall-back (the caller decides the route: mask_losses_applies)."""
    if not mask_losses_applies(pred_masks, target_masks):
        raise ValueError("mask_losses: contiguous fp32 device pred_masks [B, Q, h, w] and bool / uint8 targets [T, H >= h, W >= w] expected")
    n, rows = pair_src.numel(), pred_masks.shape[0] * pred_masks.shape[1]
    for t, size in ((pair_src, n), (pair_tgt, n)) + (() if row_pair is None else ((row_pair, rows),)):
        if t.dtype != torch.int32 or t.numel() != size or t.device != pred_masks.device or not t.is_contiguous():
            raise ValueError("mask_losses: pair_src / pair_tgt int32 [n] and row_pair int32 [B Q] on the device expected")
    tgt = target_masks.contiguous()
    tgt = tgt.view(torch.uint8) if tgt.dtype == torch.bool else tgt
    if row_pair is None:
        row_pair = torch.full((rows,), -1, dtype=torch.int32, device=pred_masks.device)
        if n:
            row_pair[pair_src.long()] = torch.arange(n, dtype=torch.int32, device=pred_masks.device)
    return _MaskLosses.apply(pred_masks, tgt, pair_src, pair_tgt, row_pair, float(alpha), float(gamma), float(num_boxes))
