"""Hungarian matcher with the cost matrices computed on the GPU: the host side of `dod_match_cost` (include/dinodet.h).

Mirrors `dino_detector.matching.HungarianMatcher` (matching.py:9-121): same constructor, same `forward(outputs, targets)`
contract (a list of (index_i, index_j) int64 CPU tensors per image).  The focal / L1 / GIoU cost of every image
(matching.py:79-98) is one kernel launch over the packed detections and the concatenated targets, one device-to-host copy
brings all matrices back, and scipy's `linear_sum_assignment` solves them on the host as in the reference (:105).
No CPU fallback for the cost computation: without the HIP library this module raises.

Reference behaviour kept on purpose: the reference builds each image's matrix over ALL B*Q predictions and then keeps
`C[:num_queries]` (matching.py:102) -- the rows of image 0 for every image.  `per_image_rows=False` (default) reproduces
that; `per_image_rows=True` matches each image's targets against its own predictions.

`HungarianMatcher.match_table` is the opt-in device path: the same costs, then `assign` (`dod_match_assign`, a device
restatement of scipy's solver whose result is bit-identical to scipy's) writes the criterion's match table on the GPU, with
no host sync.  Errors become per-image status codes the caller reads later (`losses.SetCriterion.check_assignment`).
"""
import numpy as np
import torch
import torch.nn as nn
from scipy.optimize import linear_sum_assignment

from . import _native as nat


def match_cost(det, num_classes, labels, gt_boxes, offsets, cost_class=1.0, cost_bbox=5.0, cost_giou=2.0,
               focal_alpha=0.25, focal_gamma=2.0, rows_from=0):
    """det: packed [B,Q,C+4] fp32 CUDA tensor; labels int64 [G], gt_boxes fp32 [G,4] (cx,cy,w,h), offsets int32 [B+1]
    (CUDA tensors).  Returns the flat fp32 CUDA buffer [G*Q]: image b's [Q, n_b] matrix at offsets[b]*Q."""
    if not (det.is_cuda and det.dtype == torch.float32 and det.dim() == 3):
        raise ValueError("det must be a CUDA fp32 tensor [B, Q, C+4]")
    B, Q, W = det.shape
    if W != num_classes + 4:
        raise ValueError(f"det has {W} columns, expected num_classes + 4 = {num_classes + 4}")
    G = int(labels.numel())
    if gt_boxes.numel() != 4 * G or offsets.numel() != B + 1:
        raise ValueError("targets: gt_boxes must be [G,4] and offsets [B+1]")
    cost = torch.empty(max(1, G * Q), dtype=torch.float32, device=det.device)
    nat.check(nat.lib().dod_match_cost(nat.ptr(det.contiguous()), B, Q, num_classes, nat.ptr(labels), nat.ptr(gt_boxes),
                                       nat.ptr(offsets), G, float(cost_class), float(cost_bbox), float(cost_giou),
                                       float(focal_alpha), float(focal_gamma), int(rows_from), nat.ptr(cost), nat.stream_ptr()))
    return cost[: G * Q]


# dod_match_assign status codes (include/dinodet.h) -> what the host path raises for that image
ASSIGN_OK, ASSIGN_INVALID, ASSIGN_INFEASIBLE, ASSIGN_LABEL = 0, 1, 2, 3
ASSIGN_ERRORS = {ASSIGN_INVALID: (ValueError, "matrix contains invalid numeric entries"),
                 ASSIGN_INFEASIBLE: (ValueError, "cost matrix is infeasible"),
                 ASSIGN_LABEL: (IndexError, "target label out of range")}


def assign(cost, offsets, num_queries, labels=None, num_classes=None):
    """scipy's linear_sum_assignment of every image's [Q, n_b] matrix in the flat fp32 CUDA buffer `cost` (image b at
    offsets[b] * Q, as `match_cost` writes it), on the device.  offsets: int32 CUDA [B+1]; labels (optional, int64 CUDA
    [G]) are checked against [0, num_classes).  Returns (match int32 [B*Q]: offsets[b] + target or -1, status int32 [B]:
    ASSIGN_*), both CUDA tensors; nothing is read back."""
    Q = int(num_queries)
    if not (cost.is_cuda and cost.dtype == torch.float32):
        raise ValueError("cost must be a CUDA fp32 tensor")
    if not (offsets.is_cuda and offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 2):
        raise ValueError("offsets must be a CUDA int32 tensor [B+1]")
    if Q <= 0 or cost.numel() % Q:
        raise ValueError(f"cost holds {cost.numel()} entries, not a multiple of num_queries = {Q}")
    B, G = offsets.numel() - 1, cost.numel() // Q
    if labels is not None:
        if num_classes is None or labels.numel() != G:
            raise ValueError("labels need num_classes and one entry per target")
        labels = labels.to(cost.device, torch.int64).contiguous()
    cost, offsets = cost.contiguous(), offsets.contiguous()
    L = nat.lib()
    ws = torch.empty(L.dod_match_assign_workspace_bytes(B, Q, G), dtype=torch.uint8, device=cost.device)
    match = torch.empty(B * Q, dtype=torch.int32, device=cost.device)
    status = torch.empty(B, dtype=torch.int32, device=cost.device)
    nat.check(L.dod_match_assign(nat.ptr(cost) if G else None, nat.ptr(offsets), B, Q, G, nat.ptr(labels),
                                 int(num_classes) if labels is not None else 0, nat.ptr(match), nat.ptr(status), nat.ptr(ws),
                                 ws.numel(), nat.stream_ptr()))
    return match, status


class HungarianMatcher(nn.Module):
    """Drop-in for dino_detector.matching.HungarianMatcher (constructor matching.py:23-40, forward :43-121)."""

    def __init__(self, cost_class=1, cost_bbox=5, cost_giou=2, focal_alpha=0.25, focal_gamma=2.0, per_image_rows=False):
        super().__init__()
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou
        self.focal_alpha, self.focal_gamma = focal_alpha, focal_gamma
        self.per_image_rows = per_image_rows
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "at least one cost should be non-zero"

    @torch.no_grad()
    def forward(self, outputs, targets):
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        bs, num_queries, C = logits.shape
        dev = logits.device
        # views of one packed buffer (the engine's output) are used as they are; anything else is packed once
        det = torch.cat([logits, boxes], dim=-1).float().contiguous()
        counts, lab, box = [], [], []
        for t in targets:
            if len(t) == 0:                       # matching.py:73-75: an EMPTY DICT short-circuits
                counts.append(0)
                continue
            counts.append(int(t["labels"].numel()))
            lab.append(t["labels"].reshape(-1).to(dev, torch.int64))
            box.append(t["boxes"].reshape(-1, 4).to(dev, torch.float32))
        G = sum(counts)
        empty = (torch.tensor([], dtype=torch.int64), torch.tensor([], dtype=torch.int64))
        if G == 0:
            return [empty for _ in targets]
        labels = torch.cat(lab)
        if int(labels.min()) < 0 or int(labels.max()) >= C:
            raise IndexError("target label out of range")        # pos_cost_class[:, tgt_ids] would raise (matching.py:86)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        cost = match_cost(det, C, labels, torch.cat(box).contiguous(), torch.from_numpy(offs).to(dev),
                          self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha, self.focal_gamma,
                          -1 if self.per_image_rows else 0).cpu().numpy()
        out = []
        for b, n in enumerate(counts):
            if len(targets[b]) == 0:
                out.append(empty)
                continue
            Cm = cost[offs[b] * num_queries:(offs[b] + n) * num_queries].reshape(num_queries, n)
            i, j = linear_sum_assignment(Cm)                     # matching.py:105
            out.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        return out

    @torch.no_grad()
    def match_table(self, outputs, targets):
        """The criterion's match table straight from the device: (match int32 [B*Q], status int32 [B]) CUDA tensors, equal to
        `losses.match_table(self(outputs, targets), counts, Q)` wherever `forward` returns.  Nothing here synchronises: the
        label check is status 3 and scipy's errors are statuses 1 / 2 (ASSIGN_ERRORS), for the caller to read later."""
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        bs, num_queries, C = logits.shape
        dev = logits.device
        if not logits.is_cuda:
            raise ValueError("match_table needs CUDA outputs")
        det = torch.cat([logits, boxes], dim=-1).float().contiguous()
        counts, lab, box = [], [], []
        for t in targets:
            if len(t) == 0:
                counts.append(0)
                continue
            counts.append(int(t["labels"].numel()))
            lab.append(t["labels"].reshape(-1).to(dev, torch.int64))
            box.append(t["boxes"].reshape(-1, 4).to(dev, torch.float32))
        if sum(counts) == 0:
            return (torch.full((bs * num_queries,), -1, dtype=torch.int32, device=dev),
                    torch.zeros(bs, dtype=torch.int32, device=dev))
        labels = torch.cat(lab)
        offs = torch.empty(len(counts) + 1, dtype=torch.int32, pin_memory=True)
        offs.numpy()[:] = np.concatenate([[0], np.cumsum(counts)])
        offs = offs.to(dev, non_blocking=True)                  # pinned: an async copy (a pageable one synchronises)
        cost = match_cost(det, C, labels, torch.cat(box).contiguous(), offs, self.cost_class, self.cost_bbox, self.cost_giou,
                          self.focal_alpha, self.focal_gamma, -1 if self.per_image_rows else 0)
        return assign(cost, offs, num_queries, labels, C)


def build_matcher(args):
    """matching.py:124-134"""
    return HungarianMatcher(cost_class=args.set_cost_class, cost_bbox=args.set_cost_bbox, cost_giou=args.set_cost_giou,
                            focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma)
