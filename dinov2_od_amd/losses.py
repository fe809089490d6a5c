"""Set-prediction loss with a native gradient: a drop-in for `dino_detector.losses` (losses.py:9-254).

`SetCriterion` keeps the reference's constructor, attributes and `forward(outputs, targets)` contract: it calls
`self.matcher(outputs, targets)` (ours, `dinov2_od_amd.matching.HungarianMatcher`, or the reference's), normalises by
`num_boxes` = the number of targets (all-reduced under an initialised `torch.distributed`, clamped to 1), and returns
`{loss_ce, loss_bbox, loss_giou}` weighted by `weight_dict` exactly as losses.py:236-240 does.

On the GPU the three unweighted losses come from `dod_set_criterion_forward` (two launches: per-workgroup partials, then a
fixed-order sum) and their gradient from ONE `dod_set_criterion_backward` launch (include/dinodet.h, csrc/criterion.hip):
the logits and boxes are read in place -- the views of the packed [B, Q, C+4] detections `engine.split_detections` hands
out included -- the assignment travels as an int32 [B*Q] match table built on the host from the matcher's CPU indices and
uploaded with one async copy, and `num_boxes` stays a device scalar: no host sync of the criterion's own.  With
`device_assignment=True` the table comes from `matcher.match_table` instead (the device solver, bit-identical to scipy), so
the whole call runs without a host sync; its errors wait for `check_assignment()`.  CPU tensors take
`composite_losses`, a torch composite of the same math (the CPU test suite pins it to the reference's autograd).
There is no fall-back: a CUDA input without the HIP library raises.

Reference behaviour kept: an image whose target tensors are empty contributes only background; `num_boxes == 0` is clamped
to 1; a label equal to `num_classes` is background (the one-hot's dropped column, losses.py:125-128); a prediction index
>= Q or a target index >= n_b raises IndexError (the reference's `loss_boxes` indexing raises there); a `num_classes` other
than the logits' C raises RuntimeError (a broadcast error in the reference).
Deliberate deviation: a prediction index repeated within one image raises ValueError.  The reference's CUDA `index_put_`
keeps an unspecified one of the repeats, so there is no defined behaviour to copy, and no matcher produces repeats.
"""
import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

LOSS_KEYS = ("loss_ce", "loss_bbox", "loss_giou")


# ------------------------------------------------------------------ composite (CPU, and the GPU tests' yardstick)
def focal_terms(logits, onehot, alpha, gamma):
    """a_t * (1 - p_t)^gamma * BCE-with-logits, element-wise (losses.py:130-138)"""
    p = logits.sigmoid()
    pt = p * onehot + (1 - p) * (1 - onehot)
    at = alpha * onehot + (1 - alpha) * (1 - onehot)
    return at * (1 - pt) ** gamma * F.binary_cross_entropy_with_logits(logits, onehot, reduction="none")


def pair_giou(a, b):
    """generalized IoU of matched pairs of cxcywh boxes [K, 4] (utils.py:73-88 and :124-164, on the diagonal only)"""
    def xyxy(x):
        cx, cy, w, h = x.unbind(-1)
        return cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h
    ax1, ay1, ax2, ay2 = xyxy(a)
    bx1, by1, bx2, by2 = xyxy(b)
    area1, area2 = (ax2 - ax1) * (ay2 - ay1), (bx2 - bx1) * (by2 - by1)
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(min=0)
    ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(min=0)
    inter = iw * ih
    union = area1 + area2 - inter
    ew = (torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)).clamp(min=0)
    eh = (torch.maximum(ay2, by2) - torch.minimum(ay1, by1)).clamp(min=0)
    earea = ew * eh
    return inter / union - (earea - union) / earea


def composite_losses(logits, boxes, labels, gt_boxes, match, num_boxes, alpha=0.25, gamma=2.0):
    """The three unweighted losses [3] = (loss_ce, loss_bbox, loss_giou) in torch, differentiable, on any device.
    logits [B,Q,C], boxes [B,Q,4], labels int64 [G], gt_boxes [G,4], match int [B*Q] (-1 = background), num_boxes: a
    tensor holding the (all-reduced) target count; clamped to 1 here."""
    B, Q, C = logits.shape
    G = labels.numel()
    m = match.reshape(-1).to(logits.device, torch.int64)
    valid = (m >= 0) & (m < G)
    mv = m.clamp(0, max(G - 1, 0))
    cls = torch.full((B * Q,), -1, dtype=torch.int64, device=logits.device)
    if G:
        cls = torch.where(valid, labels.to(logits.device)[mv], cls)
    onehot = (cls[:, None] == torch.arange(C, device=logits.device)).to(logits.dtype).view(B, Q, C)
    nb = num_boxes.reshape(()).to(logits.device, logits.dtype).clamp(min=1)
    ce = focal_terms(logits, onehot, alpha, gamma).sum() / nb
    src = boxes.reshape(B * Q, 4)[valid]
    tgt = gt_boxes.to(logits.device, logits.dtype)[m[valid]]
    l1 = F.l1_loss(src, tgt, reduction="none").sum() / nb
    gi = (1 - pair_giou(src, tgt)).sum() / nb
    return torch.stack([ce, l1, gi])


# ------------------------------------------------------------------ native
def _rows(t, last):
    """(tensor, row stride) with rows r = b*Q + q at base + r * stride, unit element stride; copies only odd layouts"""
    if t.dtype != torch.float32:
        t = t.float()
    B, Q = t.shape[0], t.shape[1]
    s = t.stride()
    if not (s[2] == 1 and s[1] >= last and (B == 1 or s[0] == Q * s[1])):
        t = t.contiguous()
        s = t.stride()
    return t, s[1]


class _CriterionFn(torch.autograd.Function):
    """(pred_logits, pred_boxes) -> fp32[3] unweighted losses; backward = one dod_set_criterion_backward launch"""

    @staticmethod
    def forward(ctx, logits, boxes, labels, gt_boxes, match, num_boxes, alpha, gamma):
        from . import _native as nat
        B, Q, C = logits.shape
        lg, ls = _rows(logits, C)
        bx, bs = _rows(boxes, 4)
        G = labels.numel()
        L = nat.lib()
        ws = torch.empty(L.dod_set_criterion_workspace_bytes(B, Q, C) // 4, dtype=torch.float32, device=logits.device)
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        nat.check(L.dod_set_criterion_forward(nat.ptr(lg), ls, nat.ptr(bx), bs, B, Q, C, nat.ptr(labels), nat.ptr(gt_boxes), G,
                                              nat.ptr(match), B * Q, nat.ptr(num_boxes), float(alpha), float(gamma), nat.ptr(out),
                                              None, nat.ptr(ws), ws.numel() * 4, nat.stream_ptr()))
        ctx.save_for_backward(lg, bx, labels, gt_boxes, match, num_boxes)
        ctx.meta = (ls, bs, float(alpha), float(gamma), logits.dtype, boxes.dtype)
        return out

    @staticmethod
    def backward(ctx, d_losses):
        from . import _native as nat
        lg, bx, labels, gt_boxes, match, num_boxes = ctx.saved_tensors
        ls, bs, alpha, gamma, ldt, bdt = ctx.meta
        B, Q, C = lg.shape
        d = d_losses.to(torch.float32).contiguous()
        d_logits = torch.empty((B, Q, C), dtype=torch.float32, device=lg.device)
        d_boxes = torch.empty((B, Q, 4), dtype=torch.float32, device=lg.device)
        nat.check(nat.lib().dod_set_criterion_backward(nat.ptr(lg), ls, nat.ptr(bx), bs, B, Q, C, nat.ptr(labels), nat.ptr(gt_boxes),
                                                       labels.numel(), nat.ptr(match), B * Q, nat.ptr(num_boxes), alpha, gamma,
                                                       nat.ptr(d), None, nat.ptr(d_logits), nat.ptr(d_boxes), nat.stream_ptr()))
        return d_logits.to(ldt), d_boxes.to(bdt), None, None, None, None, None, None


def native_losses(logits, boxes, labels, gt_boxes, match, num_boxes, alpha=0.25, gamma=2.0):
    """The three unweighted losses [3] on the GPU (same arguments as `composite_losses`; match int32 [B*Q] and num_boxes a
    fp32 [1] tensor on the logits' device).  Under no_grad, or when no input requires grad, only the forward runs."""
    if not logits.is_cuda:
        raise ValueError("native_losses needs CUDA tensors (use composite_losses on the CPU)")
    dev = logits.device
    labels = labels.to(dev, torch.int64).contiguous()
    gt_boxes = gt_boxes.to(dev, torch.float32).contiguous()
    match = match.to(dev, torch.int32).contiguous()
    num_boxes = num_boxes.to(dev, torch.float32).contiguous()
    if gt_boxes.numel() != 4 * labels.numel():
        raise ValueError("gt_boxes must be [G, 4] with G = len(labels)")
    if match.numel() != logits.shape[0] * logits.shape[1]:
        raise ValueError("match must hold B*Q entries")
    if boxes.shape[:2] != logits.shape[:2] or boxes.shape[-1] != 4:
        raise ValueError("pred_boxes must be [B, Q, 4]")
    return _CriterionFn.apply(logits, boxes, labels, gt_boxes, match, num_boxes, alpha, gamma)


def _packed_layers(ts, last):
    """L tensors [B, Q, last] -> (base tensor, row stride, keepalive) with layer l's row (b, q) at base + ((l*B + b)*Q + q) *
    stride: in place when they are consecutive slices of one packed buffer (the [L, B, Q, C+4] detections of the native
    deep-supervision step), else one stacked copy"""
    rows = [_rows(t, last) for t in ts]
    t0, s0 = rows[0]
    step = t0.shape[0] * t0.shape[1] * s0 * 4
    if all(s == s0 and t.data_ptr() == t0.data_ptr() + l * step for l, (t, s) in enumerate(rows)):
        return t0, s0, [t for t, _ in rows]
    st = torch.stack([t for t, _ in rows]).contiguous()
    return st, last, [st]


class _CriterionLayersFn(torch.autograd.Function):
    """(L x pred_logits, L x pred_boxes) -> fp32 [L, 3] unweighted losses, all layers in the two launches of
    dod_set_criterion_layers_forward; backward = one dod_set_criterion_layers_backward launch"""

    @staticmethod
    def forward(ctx, nl, labels, gt_boxes, match, num_boxes, alpha, gamma, *preds):
        from . import _native as nat
        logits, boxes = preds[:nl], preds[nl:]
        B, Q, C = logits[0].shape
        lg, ls, keep_l = _packed_layers(logits, C)
        bx, bs, keep_b = _packed_layers(boxes, 4)
        L = nat.lib()
        ws = torch.empty(L.dod_set_criterion_layers_workspace_bytes(nl, B, Q, C) // 4, dtype=torch.float32, device=lg.device)
        out = torch.empty((nl, 3), dtype=torch.float32, device=lg.device)
        nat.check(L.dod_set_criterion_layers_forward(nat.ptr(lg), ls, nat.ptr(bx), bs, nl, B, Q, C, nat.ptr(labels), nat.ptr(gt_boxes),
                                                     labels.numel(), nat.ptr(match), nl * B * Q, nat.ptr(num_boxes), float(alpha),
                                                     float(gamma), nat.ptr(out), None, nat.ptr(ws), ws.numel() * 4, nat.stream_ptr()))
        ctx.save_for_backward(labels, gt_boxes, match, num_boxes, *keep_l, *keep_b)
        ctx.meta = (nl, B, Q, C, lg.data_ptr(), ls, bx.data_ptr(), bs, len(keep_l), float(alpha), float(gamma),
                    [t.dtype for t in preds])
        return out

    @staticmethod
    def backward(ctx, d_losses):
        from . import _native as nat
        labels, gt_boxes, match, num_boxes, *keep = ctx.saved_tensors
        nl, B, Q, C, lgp, ls, bxp, bs, nkl, alpha, gamma, dts = ctx.meta
        assert keep[0].data_ptr() == lgp and keep[nkl].data_ptr() == bxp       # the saved tensors ARE the buffers the forward read
        d = d_losses.to(torch.float32).contiguous()
        dev = keep[0].device
        d_logits = torch.empty((nl, B, Q, C), dtype=torch.float32, device=dev)
        d_boxes = torch.empty((nl, B, Q, 4), dtype=torch.float32, device=dev)
        nat.check(nat.lib().dod_set_criterion_layers_backward(lgp, ls, bxp, bs, nl, B, Q, C, nat.ptr(labels), nat.ptr(gt_boxes),
                                                              labels.numel(), nat.ptr(match), nl * B * Q, nat.ptr(num_boxes), alpha,
                                                              gamma, nat.ptr(d), None, nat.ptr(d_logits), nat.ptr(d_boxes),
                                                              nat.stream_ptr()))
        grads = list(d_logits.unbind(0)) + list(d_boxes.unbind(0))
        return (None,) * 7 + tuple(g.to(dt) for g, dt in zip(grads, dts))


def native_losses_layers(logits, boxes, labels, gt_boxes, match, num_boxes, alpha=0.25, gamma=2.0):
    """The unweighted losses [L, 3] of L layers' predictions (lists of [B,Q,C] / [B,Q,4] CUDA tensors) against one set of
    targets; match int32 [L*B*Q]: each layer's own table, in the order of the lists"""
    nl = len(logits)
    if nl == 0 or len(boxes) != nl or not all(t.is_cuda for t in logits):
        raise ValueError("native_losses_layers needs L >= 1 CUDA predictions (use composite_losses on the CPU)")
    dev = logits[0].device
    labels = labels.to(dev, torch.int64).contiguous()
    gt_boxes = gt_boxes.to(dev, torch.float32).contiguous()
    match = match.to(dev, torch.int32).contiguous()
    num_boxes = num_boxes.to(dev, torch.float32).contiguous()
    if gt_boxes.numel() != 4 * labels.numel():
        raise ValueError("gt_boxes must be [G, 4] with G = len(labels)")
    if match.numel() != nl * logits[0].shape[0] * logits[0].shape[1]:
        raise ValueError("match must hold L*B*Q entries")
    for lg, bx in zip(logits, boxes):
        if lg.shape != logits[0].shape or bx.shape[:2] != lg.shape[:2] or bx.shape[-1] != 4:
            raise ValueError("every layer needs pred_logits [B, Q, C] and pred_boxes [B, Q, 4] of the same shape")
    return _CriterionLayersFn.apply(nl, labels, gt_boxes, match, num_boxes, alpha, gamma, *logits, *boxes)


# ------------------------------------------------------------------ host glue
def match_table(indices, counts, Q, pin=False):
    """int32 [B*Q] table from the matcher's (pred_idx, tgt_idx) pairs: entry b*Q + i = offset_b + j, else -1"""
    B = len(counts)
    table = torch.full((B * Q,), -1, dtype=torch.int32, pin_memory=pin)
    tv = table.numpy()
    off = 0
    for b, (i, j) in enumerate(indices):
        i = np.asarray(torch.as_tensor(i).cpu(), dtype=np.int64).reshape(-1)
        j = np.asarray(torch.as_tensor(j).cpu(), dtype=np.int64).reshape(-1)
        if i.shape != j.shape:
            raise ValueError(f"image {b}: {len(i)} prediction indices against {len(j)} target indices")
        n = counts[b]
        if i.size:
            if i.min() < -Q or i.max() >= Q:
                raise IndexError(f"image {b}: prediction index out of range for {Q} queries")
            if j.min() < -n or j.max() >= n:
                raise IndexError(f"image {b}: target index out of range for {n} targets")
            i, j = i % Q, j % n                          # negative indices address from the end, as torch indexing does
            if np.unique(i).size != i.size:
                raise ValueError(f"image {b}: a prediction index is matched twice")
            tv[b * Q + i] = off + j
        off += n
    return table


class SetCriterion(nn.Module):
    """Drop-in for dino_detector.losses.SetCriterion (constructor losses.py:79-98, forward :204-242)."""

    def __init__(self, matcher, num_classes, weight_dict, focal_alpha=0.25, focal_gamma=2.0, device_assignment=False):
        """device_assignment=True: the match table comes from `matcher.match_table` (the device solver, no host sync) instead of
        scipy on the host; its errors are deferred to `check_assignment()`.  The default keeps scipy and raises at once."""
        super().__init__()
        self.matcher = matcher
        self.num_classes = num_classes
        self.weight_dict = weight_dict
        self.focal_alpha = focal_alpha
        self.focal_gamma = focal_gamma
        if device_assignment and not callable(getattr(matcher, "match_table", None)):
            raise TypeError(f"device_assignment needs a matcher with match_table(); {type(matcher).__name__} has none")
        self.device_assignment = bool(device_assignment)
        self.last_assignment_status = None

    def check_assignment(self):
        """Synchronises and raises what the host path would have raised for the last device-assigned call: IndexError when a
        label of any image is out of range, else the scipy ValueError of the first failing image.  No-op in host mode."""
        from .matching import ASSIGN_ERRORS, ASSIGN_LABEL
        if self.last_assignment_status is None:
            return
        st = self.last_assignment_status.cpu().tolist()
        if ASSIGN_LABEL in st:
            exc, msg = ASSIGN_ERRORS[ASSIGN_LABEL]
            raise exc(msg)
        for s in st:
            if s:
                exc, msg = ASSIGN_ERRORS[s]
                raise exc(msg)

    def _forward_layers(self, outputs, targets):
        """DETR's deep supervision (`outputs["aux_outputs"]`: the heads on decoder layers 0 .. L-2): every layer gets its own
        assignment from the unchanged matcher, all share one num_boxes, the result gains loss_*_{i}; a key k_i is weighted by
        weight_dict[k_i] if present, else weight_dict[k], else 1.  On the GPU all layers go through ONE layered call."""
        aux = list(outputs["aux_outputs"])
        layers = aux + [{k: outputs[k] for k in ("pred_logits", "pred_boxes")}]       # memory order of the native step's packed detections
        B, Q, C = outputs["pred_logits"].shape
        for o in layers:
            if o["pred_logits"].shape[-1] != self.num_classes:
                raise RuntimeError(f"criterion.num_classes = {self.num_classes} but pred_logits has {o['pred_logits'].shape[-1]} classes")
        dev = outputs["pred_logits"].device
        counts = [int(len(t["labels"])) for t in targets]
        if self.device_assignment:
            if dev.type != "cuda":
                raise ValueError("device_assignment needs CUDA outputs")
            tabs = [self.matcher.match_table(o, targets) for o in layers]
            match = torch.cat([m for m, _ in tabs])
            self.last_assignment_status = torch.cat([tabs[-1][1]] + [st for _, st in tabs[:-1]])      # the last layer's B, then each aux layer's
        else:
            pin = dev.type == "cuda"
            match = torch.cat([match_table(self.matcher(o, targets), counts, Q, pin=False) for o in layers])
            if pin:
                match = match.pin_memory().to(dev, non_blocking=True)
        nb = torch.full((1,), float(sum(counts)), dtype=torch.float32, device=dev)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(nb)                              # once for all layers
        if sum(counts):
            labels = torch.cat([t["labels"].reshape(-1).to(dev, torch.int64) for t in targets if len(t["labels"])])
            gt = torch.cat([t["boxes"].reshape(-1, 4).to(dev, torch.float32) for t in targets if len(t["labels"])])
        else:
            labels = torch.zeros(0, dtype=torch.int64, device=dev)
            gt = torch.zeros((0, 4), dtype=torch.float32, device=dev)
        lgs, bxs = [o["pred_logits"] for o in layers], [o["pred_boxes"] for o in layers]
        if dev.type == "cuda":
            losses = native_losses_layers(lgs, bxs, labels, gt, match, nb, self.focal_alpha, self.focal_gamma)
        else:
            losses = torch.stack([composite_losses(lg, bx, labels, gt, match[l * B * Q:(l + 1) * B * Q], nb, self.focal_alpha, self.focal_gamma)
                                  for l, (lg, bx) in enumerate(zip(lgs, bxs))])
        w = self.weight_dict
        out = {k: w[k] * losses[-1, n] if k in w else losses[-1, n] for n, k in enumerate(LOSS_KEYS)}
        for i in range(len(aux)):
            for n, k in enumerate(LOSS_KEYS):
                ki = f"{k}_{i}"
                out[ki] = w[ki] * losses[i, n] if ki in w else (w[k] * losses[i, n] if k in w else losses[i, n])
        return out

    def forward(self, outputs, targets):
        if "aux_outputs" in outputs:
            return self._forward_layers(outputs, targets)
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        B, Q, C = logits.shape
        if C != self.num_classes:
            raise RuntimeError(f"criterion.num_classes = {self.num_classes} but pred_logits has {C} classes")
        if self.device_assignment:
            if not logits.is_cuda:
                raise ValueError("device_assignment needs CUDA outputs")
            match, self.last_assignment_status = self.matcher.match_table(outputs, targets)
        else:
            indices = self.matcher(outputs, targets)
        dev = logits.device
        counts = [int(len(t["labels"])) for t in targets]
        nb = torch.full((1,), float(sum(counts)), dtype=torch.float32, device=dev)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(nb)                              # device tensor, never read back
        if sum(counts):
            labels = torch.cat([t["labels"].reshape(-1).to(dev, torch.int64) for t in targets if len(t["labels"])])
            gt = torch.cat([t["boxes"].reshape(-1, 4).to(dev, torch.float32) for t in targets if len(t["labels"])])
        else:
            labels = torch.zeros(0, dtype=torch.int64, device=dev)
            gt = torch.zeros((0, 4), dtype=torch.float32, device=dev)
        if self.device_assignment:                           # the table is already on the device
            losses = native_losses(logits, boxes, labels, gt, match, nb, self.focal_alpha, self.focal_gamma)
        elif logits.is_cuda:
            table = match_table(indices, counts, Q, pin=True)
            match = table.to(dev, non_blocking=True)         # pinned host table: one async copy
            losses = native_losses(logits, boxes, labels, gt, match, nb, self.focal_alpha, self.focal_gamma)
        else:
            table = match_table(indices, counts, Q)
            losses = composite_losses(logits, boxes, labels, gt, table, nb, self.focal_alpha, self.focal_gamma)
        out = {k: losses[n] for n, k in enumerate(LOSS_KEYS)}
        return {k: self.weight_dict[k] * out[k] if k in self.weight_dict else out[k] for k in out}


class _FocalFn(torch.autograd.Function):
    """FocalLoss on the criterion's row kernel: row r's target is labels[r], no boxes; reduction 'none' through elem_loss"""

    @staticmethod
    def forward(ctx, inputs, targets, alpha, gamma, reduction):
        from . import _native as nat
        N, C = inputs.shape
        x = inputs.float().contiguous()
        dev = x.device
        L = nat.lib()
        ws = torch.empty(L.dod_set_criterion_workspace_bytes(1, N, C) // 4, dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        elem = torch.empty((N, C), dtype=torch.float32, device=dev) if reduction == "none" else None
        nb = torch.full((1,), float(N * C), dtype=torch.float32, device=dev) if reduction == "mean" else None
        nat.check(L.dod_set_criterion_forward(nat.ptr(x), C, None, 4, 1, N, C, nat.ptr(targets), None, N, None, 0, nat.ptr(nb),
                                              float(alpha), float(gamma), nat.ptr(out), nat.ptr(elem), nat.ptr(ws), ws.numel() * 4,
                                              nat.stream_ptr()))
        ctx.save_for_backward(x, targets, nb)
        ctx.meta = (float(alpha), float(gamma), reduction, inputs.dtype)
        return (elem if reduction == "none" else out[0]).to(inputs.dtype)

    @staticmethod
    def backward(ctx, g):
        from . import _native as nat
        x, targets, nb = ctx.saved_tensors
        alpha, gamma, reduction, dt = ctx.meta
        N, C = x.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        d_losses = torch.zeros(3, dtype=torch.float32, device=x.device)
        if reduction != "none":
            d_losses[0:1].copy_(g.reshape(1))
        nat.check(nat.lib().dod_set_criterion_backward(nat.ptr(x), C, None, 4, 1, N, C, nat.ptr(targets), None, N, None, 0,
                                                       nat.ptr(nb), alpha, gamma, nat.ptr(d_losses),
                                                       nat.ptr(g) if reduction == "none" else None, nat.ptr(dx), None,
                                                       nat.stream_ptr()))
        return dx.to(dt), None, None, None, None


class FocalLoss(nn.Module):
    """Drop-in for dino_detector.losses.FocalLoss (losses.py:9-68): inputs [N, C] logits, targets [N] class indices in
    [0, C); reduction 'none' | 'mean' | 'sum'.  A target outside [0, C) raises as F.one_hot does."""

    def __init__(self, alpha=0.25, gamma=2.0, reduction="none"):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction

    def forward(self, inputs, targets):
        N, C = inputs.shape
        targets = targets.reshape(-1)
        if targets.numel() != N:
            raise ValueError(f"targets must hold {N} class indices")
        if N and (int(targets.min()) < 0 or int(targets.max()) >= C):
            raise RuntimeError("Class values must be non-negative and smaller than num_classes.")
        red = self.reduction if self.reduction in ("mean", "sum") else "none"
        if inputs.is_cuda and N:
            return _FocalFn.apply(inputs, targets.to(inputs.device, torch.int64).contiguous(), self.alpha, self.gamma, red)
        onehot = F.one_hot(targets.to(torch.int64), num_classes=C).to(inputs.dtype)
        loss = focal_terms(inputs, onehot, self.alpha, self.gamma)
        if red == "mean":
            return loss.mean()
        if red == "sum":
            return loss.sum()
        return loss


def build_criterion(matcher, num_classes, weight_dict, focal_alpha=0.25, focal_gamma=2.0):
    """losses.py:244-254"""
    return SetCriterion(matcher=matcher, num_classes=num_classes, weight_dict=weight_dict, focal_alpha=focal_alpha,
                        focal_gamma=focal_gamma)
