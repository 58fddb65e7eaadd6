"""Hungarian matching between predictions and ground truth with TrackFormer's track-query constraints.

Same module surface as the reference's models/matcher.py (HungarianMatcher :12-131, build_matcher
:134-141).  The cost matrix is built on the device exactly as there (focal / softmax class cost +
L1 + GIoU); the track-query constraints, which the reference writes with a Python double loop over
every query (:104-125), are applied as three vectorised index assignments on the host copy.
"""
import os

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment
from torch import nn

from . import fused
from .box_ops import box_cxcywh_to_xyxy, generalized_box_iou

# THE FUSED COST (opt-in): with focal_loss set and fp32 tensors on the device, match_many builds the cost matrix of all prediction
# sets with ONE kernel (fused.match_cost; include/tf_fused.h: tf_match_cost_f32) instead of the ~25 launches of the torch chain below;
# 1 - p is formed as sigmoid(-x) there, never as an fp32 subtraction.  NOT covered: the softmax (plain DETR) cost; the track-query
# constraints and linear_sum_assignment work on the host copy as before, and the cost still reaches the host in ONE copy.  OFF by
# default (tools/bench_criterion.py, profiles/criterion_fused_bench.json).
_fused_cost = None    # None: follow TF_MATCHER_FUSED_COST (unset: off)
_fused_cost_counts = {"own": 0, "torch": 0}


def fused_cost_enabled():
    if _fused_cost is not None:
        return _fused_cost
    return os.environ.get("TF_MATCHER_FUSED_COST", "0") not in ("", "0")


def set_fused_cost(on):
    """Switch the fused matching cost on or off (process-wide; None: follow TF_MATCHER_FUSED_COST again); returns the previous
    setting."""
    global _fused_cost
    prev = fused_cost_enabled()
    _fused_cost = None if on is None else bool(on)
    return fused._switched(prev, fused_cost_enabled())


def fused_cost_counts(reset=False):
    """How many match_many calls with the switch on built their cost with the library's own kernel ("own") and how many kept the torch
    chain ("torch")."""
    out = dict(_fused_cost_counts)
    if reset:
        for k in _fused_cost_counts:
            _fused_cost_counts[k] = 0
    return out


class HungarianMatcher(nn.Module):
    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1,
                 focal_loss: bool = False, focal_alpha: float = 0.25, focal_gamma: float = 2.0):
        super().__init__()
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        self.focal_loss = focal_loss
        self.focal_alpha = focal_alpha
        self.focal_gamma = focal_gamma
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"

    @torch.no_grad()
    def forward(self, outputs, targets):
        """outputs: pred_logits [B,Q,C], pred_boxes [B,Q,4]; targets: list of dicts with labels,
        boxes (+ track_query_match_ids / track_queries_mask / track_queries_fal_pos_mask).
        -> list of (query indices, target indices) int64 tensors, one pair per sample."""
        return self.match_many([outputs], targets)[0]

    @torch.no_grad()
    def match_many(self, outputs_list, targets):
        """forward() for several prediction sets against the SAME targets (the criterion's final + auxiliary decoder layers:
        models/detr.py:266-289 of the reference calls the matcher once per layer) -> one list of index pairs per set.  The cost
        matrices of all sets are built by ONE chain of device kernels and reach the host in ONE copy (per call of forward(): ~25
        launches and three synchronising copies per target); the arithmetic per element is forward()'s, so are the assignments."""
        n_sets = len(outputs_list)
        batch_size, num_queries = outputs_list[0]["pred_logits"].shape[:2]
        logits = torch.stack([o["pred_logits"] for o in outputs_list]).flatten(0, 2)       # [sets * B * Q, C]
        out_bbox = torch.stack([o["pred_boxes"] for o in outputs_list]).flatten(0, 2)
        tgt_ids = torch.cat([v["labels"] for v in targets])
        tgt_bbox = torch.cat([v["boxes"] for v in targets])
        cost_matrix = None
        if fused_cost_enabled():
            if self.focal_loss:
                cost_matrix = fused.match_cost(logits, out_bbox, tgt_ids, tgt_bbox, self.cost_class, self.cost_bbox, self.cost_giou,
                                               self.focal_alpha, self.focal_gamma)
            _fused_cost_counts["own" if cost_matrix is not None else "torch"] += 1
        if cost_matrix is None:
            cost_matrix = self._cost_torch(logits, out_bbox, tgt_ids, tgt_bbox)
        cost_all = cost_matrix.view(n_sets, batch_size, num_queries, -1).cpu()
        return self._assign(cost_all, targets, n_sets, num_queries)

    def _cost_torch(self, logits, out_bbox, tgt_ids, tgt_bbox):
        """The cost matrix [sets * B * Q, T] by the reference's chain of device kernels."""
        out_prob = logits.sigmoid() if self.focal_loss else logits.softmax(-1)
        if self.focal_loss:
            neg = (1 - self.focal_alpha) * (out_prob ** self.focal_gamma) \
                * (-(1 - out_prob + 1e-8).log())
            pos = self.focal_alpha * ((1 - out_prob) ** self.focal_gamma) \
                * (-(out_prob + 1e-8).log())
            cost_class = pos[:, tgt_ids] - neg[:, tgt_ids]
        else:
            cost_class = -out_prob[:, tgt_ids]
        cost_bbox = torch.cdist(out_bbox, tgt_bbox, p=1)
        cost_giou = -generalized_box_iou(box_cxcywh_to_xyxy(out_bbox),
                                         box_cxcywh_to_xyxy(tgt_bbox))
        return self.cost_bbox * cost_bbox + self.cost_class * cost_class \
            + self.cost_giou * cost_giou

    @staticmethod
    def _assign(cost_all, targets, n_sets, num_queries):
        """cost_all [sets, B, Q, T] on the host -> the index pairs of every set, track-query constraints applied."""
        sizes = [len(v["boxes"]) for v in targets]
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        constraints = []   # per sample: (false-positive mask, pinned rows, pinned columns) on the host, once for all sets
        for i, target in enumerate(targets):
            if 'track_query_match_ids' not in target:
                constraints.append(None)
                continue
            fal_pos = target['track_queries_fal_pos_mask'].cpu()[:num_queries]
            is_track = target['track_queries_mask'].cpu()[:num_queries] & ~fal_pos
            rows = is_track.nonzero()[:, 0]
            cols = target['track_query_match_ids'].cpu()[:len(rows)] + int(offsets[i])
            constraints.append((fal_pos, rows, cols))
        result = []
        for s in range(n_sets):
            cost_matrix = cost_all[s]
            for i, con in enumerate(constraints):
                if con is None:
                    continue
                fal_pos, rows, cols = con
                # false positive track queries must stay unmatched; true ones are pinned to their target
                cost_matrix[i, fal_pos] = np.inf
                cost_matrix[i, rows] = np.inf
                cost_matrix[i][:, cols] = np.inf
                cost_matrix[i, rows, cols] = -1
            indices = [linear_sum_assignment(c[i])
                       for i, c in enumerate(cost_matrix.split(sizes, -1))]
            result.append([(torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64))
                           for i, j in indices])
        return result


def build_matcher(args):
    return HungarianMatcher(cost_class=args.set_cost_class, cost_bbox=args.set_cost_bbox,
                            cost_giou=args.set_cost_giou, focal_loss=args.focal_loss,
                            focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma)
