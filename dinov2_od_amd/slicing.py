"""Sliced and flip-augmented inference: views of the source images in, merged detections out.

The forward runs on a fixed square, so a 640 x 480 image gets a 16 x 16 or 37 x 37 patch grid and an object of a few dozen pixels
one or two patches.  The standard remedy is to run the model on overlapping tiles of the source image next to the whole image,
optionally on mirrored copies, and to merge all the answers in source-image coordinates:

    plan = plan_views(shapes, tile=320, overlap=0.2, flip=True, size=(224, 224), pairs=Q * C)      # pure host code
    u8 = extract_views(images, plan, (224, 224))             # dod_preprocess_aug_u8: crop + resize + mirror, Pillow-exact
    det = model.forward_packed_u8(u8)                        # [V, Q, C+4]
    r = detect_views_packed(det, C, plan, shapes, top_k=300, nms_iou=0.5, nms_metric="ios", edge_margin=2.0)

`DINOv2ObjectDetector.detect_sliced` is the four together.  The merge is one launch (`dod_detect_views`, include/dinodet.h; restated
in numpy in tests/detect_views_cases.py) without a host sync: top-k over all views of an image, every box mapped back through its
view's rectangle and mirror flag, greedy NMS across the views -- or, with merge="fuse", weighted boxes fusion (`dod_fuse_views`,
restated in tests/fuse_views_cases.py).  No CPU fallback: without the HIP library this module raises.
"""
import collections
import math

import numpy as np
import torch

from . import _native as nat
from . import augment as _aug
from . import preprocess as _pre
from .postprocess import Detections, MAX_TOP_K, _alloc, _check_det, _check_top_k, _sizes_rows

MAX_CANDIDATES = 1 << 20                 # include/dinodet.h dod_detect_views: (views of one image) * Q * C
NMS_METRICS = {"iou": 0, "ios": 1}       # intersection over union / over the smaller box
MERGES = ("nms", "fuse")                 # dod_detect_views / dod_fuse_views
FUSE_CONFS = {"max": 0, "avg": 1}        # dod_fuse_views' conf: the founder's score / the mean scaled by the views that agree

ViewPlan = collections.namedtuple("ViewPlan", ["offsets", "rects", "flips"])
ViewPlan.__doc__ = """offsets int32 [B+1], rects int32 [V, 4] (left, top, width, height), flips uint8 [V]: the views of image b are rows
offsets[b] .. offsets[b+1]-1 -- what dod_detect_views reads as view_offsets / view_rects / view_flips and dod_preprocess_aug* as crops /
flips.  numpy arrays from plan_views; the same tuple of CUDA tensors once staged."""


class SlicedDetections(Detections):
    """postprocess.Detections (scores, labels, boxes, queries, counts) with one more tensor, `views` [B, K] int32: the view, local to
    its image, every row came from (-1 in padding rows).  It is a Detections: detections_to_list and draw_detections take it."""

    def __new__(cls, scores, labels, boxes, queries, counts, views):
        self = super().__new__(cls, scores, labels, boxes, queries, counts)
        self.views = views
        return self


class FusedDetections(SlicedDetections):
    """SlicedDetections of merge="fuse": scores, labels and boxes are the clusters' fused ones, views and queries their founders', and
    `members` [B, K] int32 is the number of candidates fused into every row (0 in padding rows)."""

    def __new__(cls, scores, labels, boxes, queries, counts, views, members):
        self = super().__new__(cls, scores, labels, boxes, queries, counts, views)
        self.members = members
        return self


def axis_starts(L, t, overlap):
    """tile starts along an axis of length L: [0] when L <= t (the extent is then L); otherwise 0, step, 2 step, ... with
    step = t - floor(t * overlap), up to the first start s with s + t >= L, which is moved to L - t"""
    L, t = int(L), int(t)
    if L <= t:
        return [0], L
    step = t - math.floor(t * overlap)
    if step < 1:
        raise ValueError(f"overlap {overlap} leaves no step for a tile of {t}")
    starts, s = [], 0
    while s + t < L:
        starts.append(s)
        s += step
    starts.append(L - t)
    return starts, t


def _hw(x):
    return (int(x), int(x)) if np.isscalar(x) else (int(x[0]), int(x[1]))


def plan_views(shapes, tile, overlap=0.2, full_view=True, flip=False, size=None, pairs=None):
    """shapes: (H, W) per source image; tile: the tile's side or (height, width) in source pixels; overlap: the fraction of a tile
    shared with its neighbour.  Per image: the whole image first (full_view), then the tiles row-major, then with `flip` the same list
    again with the mirror flag set; a tile identical to the whole image is not listed twice.  size: the (height, width) the views will
    be resized to -- a view needing more than dod_preprocess_aug's 32 filter taps raises; pairs: Q * C of the model -- an image whose
    views exceed dod_detect_views' 2^20 candidates raises.  Pure host code: returns ViewPlan(offsets, rects, flips) of numpy arrays."""
    th, tw = _hw(tile)
    if th < 1 or tw < 1:
        raise ValueError(f"tile must be at least 1 x 1, got {tile}")
    if not (0.0 <= float(overlap) < 1.0):
        raise ValueError(f"overlap must be in [0, 1), got {overlap}")
    out = None if size is None else _pre._out_size(size)
    offsets, rects, flips = [0], [], []
    for b, (H, W) in enumerate(shapes):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"image {b}: empty shape {(H, W)}")
        ys, eh = axis_starts(H, th, overlap)
        xs, ew = axis_starts(W, tw, overlap)
        full = (0, 0, W, H)
        views = [full] if full_view else []
        views += [r for r in ((x, y, ew, eh) for y in ys for x in xs) if not (full_view and r == full)]
        if out is not None:
            for (_, _, w, h) in views:
                taps = max(-(-w // out[1]), -(-h // out[0])) * 2 + 1
                if taps > _aug.MAX_TAPS:
                    raise ValueError(f"image {b}: a {h}x{w} view is more than 15x the output {out[0]}x{out[1]}: the resize filter would need {taps} taps (> {_aug.MAX_TAPS})")
        nv = len(views) * (2 if flip else 1)
        if pairs is not None and nv * int(pairs) > MAX_CANDIDATES:
            raise ValueError(f"image {b}: {nv} views x {int(pairs)} (query, class) pairs exceed the {MAX_CANDIDATES} candidates of one merge")
        rects += views
        flips += [0] * len(views)
        if flip:
            rects += views
            flips += [1] * len(views)
        offsets.append(len(rects))
    return ViewPlan(np.asarray(offsets, dtype=np.int32), np.asarray(rects, dtype=np.int32).reshape(-1, 4), np.asarray(flips, dtype=np.uint8))


def plan_to_device(plan, device):
    """the plan as CUDA tensors (a plan that already is passes through): three small copies, the last host work of a sliced call"""
    if all(isinstance(t, torch.Tensor) for t in plan):
        return ViewPlan(*(t.to(device) for t in plan))
    dev = torch.device(device)
    return ViewPlan(torch.from_numpy(np.ascontiguousarray(plan.offsets, dtype=np.int32)).to(dev),
                    torch.from_numpy(np.ascontiguousarray(plan.rects, dtype=np.int32).reshape(-1, 4)).to(dev),
                    torch.from_numpy(np.ascontiguousarray(plan.flips, dtype=np.uint8)).to(dev))


def _extract(arrs, plan, plan_dev, size, dev):
    out_h, out_w = _pre._out_size(size)
    offsets, rects = np.asarray(plan.offsets, dtype=np.int64), np.asarray(plan.rects)
    shapes = arrs.shapes
    B, V = len(arrs), len(rects)
    if offsets.shape != (B + 1,) or offsets[0] != 0 or offsets[-1] != V or (np.diff(offsets) < 0).any():
        raise ValueError(f"plan: offsets must run from 0 to the {V} views in {B} non-decreasing steps, got {offsets.tolist()}")
    owner = np.repeat(np.arange(B), np.diff(offsets))
    if V == 0:
        return _pre._out_buffer(0, out_h, out_w, True, dev)
    crops, flips, _ = _aug._check_params([shapes[b] for b in owner], rects, plan.flips, None, out_h, out_w)
    src, src_offs, hs, ws = arrs.stage(dev)                 # every source image once; its views share the offset
    return _aug._launch_aug(src, src_offs[owner], hs[owner], ws[owner], crops, flips, None, out_h, out_w, True, (plan_dev.rects, plan_dev.flips))


def extract_views(images, plan, size=(224, 224), device="cuda"):
    """images: as `preprocess_batch` takes them; plan: plan_views' result for their shapes.  Returns uint8 [V, height, width, 3] on
    `device`, view v being Pillow's crop(rect) -> resize(size, BILINEAR) -> transpose(FLIP_LEFT_RIGHT) of its image, bit for bit: one
    dod_preprocess_aug_u8 call over all views.  Every source image is staged once; its views read it through the same offset."""
    arrs = _pre._sources(images)
    dev = torch.device(device)
    return _extract(arrs, plan, plan_to_device(plan, dev), size, dev)


def detect_views_packed(det, num_classes, plan, sizes, top_k=100, threshold=0.05, nms_iou=0.5, nms_metric="iou", class_agnostic=False,
                        clamp=True, edge_margin=0.0, skip_background=True, merge="nms", fuse_conf="avg"):
    """det: packed detections [V, Q, C+4] fp32 on the GPU of all views of `plan` (view-major); sizes: (height, width) of the source
    images -- one pair, one per image or a [B, 2] tensor.  Per image the `top_k` highest-logit (view, query, class) triples, ranked and
    thresholded as detect_packed does, their boxes mapped into source pixels through the view's rectangle and mirror flag; with
    edge_margin > 0 a box within that many pixels of a view border that is not a border of the source image is dropped (an object cut
    by the tile); with nms_iou (>= 0; None = no NMS) greedy NMS across the views, nms_metric "iou" or "ios" (intersection over the
    smaller box).  Returns SlicedDetections: detect_packed's Detections plus views [B, K] i32.  top_k <= 1024 with or without NMS.
    merge="fuse" replaces the NMS by weighted boxes fusion (dod_fuse_views): candidates whose IoU with a cluster's running fused box
    exceeds nms_iou (required then; "ios" has no meaning against a growing box and raises) are averaged with their scores as weights.
    fuse_conf="avg" scores a cluster with its members' mean score, scaled by members / (views covering the fused box) when fewer
    agree than could have; "max" keeps the founder's score.  Fused scores are not thresholded again.  Returns FusedDetections:
    SlicedDetections plus members [B, K] i32.
    One launch on the current stream, no host sync."""
    V, Q, Cn = _check_det(det, num_classes, "V")
    B = int(plan.offsets.shape[0]) - 1
    if B < 1 or Q < 1 or Q * Cn > MAX_CANDIDATES:
        raise ValueError(f"need at least one image and one query and at most 2^20 (query, class) pairs, got B={B} Q={Q} C={Cn}")
    if int(plan.rects.shape[0]) != V or int(plan.flips.shape[0]) != V:
        raise ValueError(f"plan holds {int(plan.rects.shape[0])} views, det {V}")
    if not isinstance(plan.offsets, torch.Tensor):
        off = np.asarray(plan.offsets, dtype=np.int64)
        if off[0] != 0 or off[-1] != V or (np.diff(off) < 0).any():
            raise ValueError(f"plan: offsets must run from 0 to the {V} views without decreasing, got {off.tolist()}")
        if int(np.diff(off).max()) * Q * Cn > MAX_CANDIDATES:
            raise ValueError(f"an image has {int(np.diff(off).max())} views: more than {MAX_CANDIDATES} candidates with Q={Q} C={Cn}")
    first, K, iou = _check_top_k(Cn, top_k, nms_iou, skip_background, MAX_TOP_K)
    if nms_metric not in NMS_METRICS:
        raise ValueError(f"nms_metric must be one of {sorted(NMS_METRICS)}, got {nms_metric!r}")
    if merge not in MERGES:
        raise ValueError(f"merge must be one of {list(MERGES)}, got {merge!r}")
    fuse = merge == "fuse"
    if fuse:
        if fuse_conf not in FUSE_CONFS:
            raise ValueError(f"fuse_conf must be one of {sorted(FUSE_CONFS)}, got {fuse_conf!r}")
        if nms_iou is None:
            raise ValueError("merge='fuse' needs nms_iou: it is the IoU above which a candidate joins a cluster")
        if nms_metric != "iou":
            raise ValueError(f"merge='fuse' matches by IoU only, got nms_metric={nms_metric!r}")
    st = _sizes_rows(sizes, B)
    if st is None:
        raise ValueError("sizes: the source images' (height, width) are needed to place the views")
    if not det.is_cuda:                                       # last: every argument is checked whether or not a GPU is present
        raise ValueError("det must be a CUDA fp32 tensor [V, Q, C+4] (there is no CPU fallback)")
    det = det.contiguous()
    L = nat.lib()
    dev = det.device
    pd = plan_to_device(plan, dev)
    st = st.to(device=dev, dtype=torch.float32).contiguous()
    ws = torch.empty(L.dod_detect_views_workspace_bytes(V, Q, Cn, K), dtype=torch.uint8, device=dev)     # dod_fuse_views' is the same
    # the two entry points share their arguments up to the IoU threshold and from the class-agnostic flag to the boxes
    head = (nat.ptr(det) if V else None, B, V, Q, Cn, nat.ptr(pd.offsets), nat.ptr(pd.rects) if V else None, nat.ptr(pd.flips) if V else None,
            nat.ptr(st), first, float(threshold), K, iou)
    flags = (int(bool(class_agnostic)), int(bool(clamp)), float(edge_margin))
    out = _alloc(FusedDetections, B, K, dev, 2) if fuse else _alloc(SlicedDetections, B, K, dev, 1)
    rows = (nat.ptr(out.scores), nat.ptr(out.labels), nat.ptr(out.views), nat.ptr(out.queries), nat.ptr(out.boxes))
    tail = (nat.ptr(out.counts), nat.ptr(ws), ws.numel(), nat.stream_ptr())
    if fuse:
        nat.check(L.dod_fuse_views(*head, *flags, FUSE_CONFS[fuse_conf], *rows, nat.ptr(out.members), *tail))
    else:
        nat.check(L.dod_detect_views(*head, NMS_METRICS[nms_metric], *flags, *rows, *tail))
    return out


def detect_sliced(model, images, size=None, tile=None, overlap=0.2, full_view=True, flip=False, max_batch=64, **kw):
    """DINOv2ObjectDetector.detect_sliced (models/detector.py); `model` is in eval mode and grad is off.  **kw goes to
    detect_views_packed: merge="fuse" (with nms_iou and fuse_conf) fuses the views' boxes instead of suppressing them."""
    arrs = _pre._sources(images)
    shapes = arrs.shapes
    size = _pre._out_size((224, 224) if size is None else size)
    tile = size if tile is None else tile
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError(f"max_batch must be at least 1, got {max_batch}")
    dc = model._dc_cfg
    Q, Cn = int(dc.num_queries), int(dc.num_classes)
    plan = plan_views(shapes, tile, overlap, full_view, flip, size=size, pairs=Q * Cn)
    dev = next(model.parameters()).device
    pd = plan_to_device(plan, dev)
    sizes = torch.from_numpy(np.asarray(shapes, dtype=np.float32).reshape(-1, 2)).to(dev)
    u8 = _extract(arrs, plan, pd, size, dev)                 # staging ends here: nothing below touches the host's copy of anything
    V = int(u8.shape[0])
    det = torch.empty(V, Q, Cn + 4, dtype=torch.float32, device=dev)
    for s in range(0, V, max_batch):
        det[s:s + max_batch] = model.forward_packed_u8(u8[s:s + max_batch])
    return detect_views_packed(det, Cn, pd, sizes, **kw)     # plan_views built the plan: the device copy needs no second validation
