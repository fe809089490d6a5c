"""COCO bbox evaluation on the GPU: the host side of `dod_coco_eval_*` (include/dinodet.h, csrc/cocoeval.hip).

Replaces the reference's `compute_coco_metrics(results, annotation_file)` (dino_detector/utils.py:243-276), i.e. pycocotools'
`COCO.loadRes` + `COCOeval(gt, dt, 'bbox')` `.evaluate() / .accumulate() / .summarize()` with default parameters and
useCats = 1.  The device code restates COCOeval operation for operation in double precision: `precision` and `recall` are
the arrays pycocotools builds, bit for bit, and the 12 `stats` their means.

    compute_coco_metrics(results, annotation_file)   the reference's function: same signature, same six keys
    COCOEvaluator(annotations, device)               .add_records / .add_packed / .evaluate / .reset
    validate_coco(model, dataloader, device, annotations)   forward -> add_packed per batch (no host sync) -> one evaluate

The evaluator compares what it is given: the reference emits normalised boxes and class indices as `category_id`
(utils.py:225-233), and neither is "fixed" here.  One deviation from pycocotools: an empty result list evaluates (AP = AR = 0
where ground truth exists) instead of raising.

The host part of this module (annotation loading and grouping, input checks) is plain numpy and runs without a GPU; the
evaluation itself has no CPU fallback.
"""
import ctypes as C
import json

import numpy as np

from . import _native as nat
from .postprocess import RECORD_DTYPE

# COCOeval's Params.setDetParams, as numpy computes them (uploaded as they are; the device never recomputes them)
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RANGES = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))
MAX_DETS = (1, 10, 100)
MAX_GT_PER_GROUP = 1024
MAX_DETECTIONS = 1 << 24
METRIC_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")

# struct dod_coco_det: one detection with the doubles a results list holds
COCO_DET_DTYPE = np.dtype([("image_id", "<i8"), ("category_id", "<i8"), ("bbox", "<f8", (4,)), ("score", "<f8")])
assert COCO_DET_DTYPE.itemsize == 56


class Annotations:
    """What COCOeval reads of an annotation file, grouped: `image_ids` / `category_ids` are the sorted unique ids (COCOeval's
    imgIds / catIds); the ground truths of known images and categories are ordered by group = category index * I + image index,
    each group in the file's order: `gt_group`, `gt_bbox` [G,4] xywh, `gt_area` (the annotation's field), `gt_iscrowd`, and
    `gt_ann_index` (their positions in the file's annotation list)."""

    def __init__(self, image_ids, category_ids, gt_group, gt_bbox, gt_area, gt_iscrowd, gt_ann_index):
        self.image_ids, self.category_ids = image_ids, category_ids
        self.gt_group, self.gt_bbox, self.gt_area, self.gt_iscrowd, self.gt_ann_index = gt_group, gt_bbox, gt_area, gt_iscrowd, gt_ann_index

    @property
    def num_groups(self):
        return int(np.unique(self.gt_group).size)


def _index_of(sorted_ids, ids):
    """positions of `ids` in the sorted unique `sorted_ids`, -1 where absent"""
    ids = np.asarray(ids, np.int64)
    if sorted_ids.size == 0:
        return np.full(ids.shape, -1, np.int64)
    pos = np.minimum(np.searchsorted(sorted_ids, ids), sorted_ids.size - 1)
    return np.where(sorted_ids[pos] == ids, pos, -1)


def load_annotations(annotations):
    """annotations: a path to a COCO json or the loaded dict.  Returns `Annotations`.  Raises ValueError for a ground-truth id
    <= 0 (COCOeval stores the id as the match and reads 0 as "unmatched"), a missing bbox / area, or more than 1024 ground
    truths in one (image, category) group.  A missing `iscrowd` counts as 0."""
    if isinstance(annotations, Annotations):
        return annotations
    if not isinstance(annotations, dict):
        with open(annotations) as f:
            annotations = json.load(f)
    image_ids = np.unique(np.asarray([int(im["id"]) for im in annotations.get("images", [])], np.int64))
    category_ids = np.unique(np.asarray([int(c["id"]) for c in annotations.get("categories", [])], np.int64))
    if image_ids.size == 0 or category_ids.size == 0:
        raise ValueError("the annotations list no images or no categories")
    anns = annotations.get("annotations", [])
    n = len(anns)
    img, cat = np.empty(n, np.int64), np.empty(n, np.int64)
    bbox, area, crowd = np.empty((n, 4), np.float64), np.empty(n, np.float64), np.zeros(n, np.uint8)
    for j, a in enumerate(anns):
        if int(a["id"]) <= 0:
            raise ValueError(f"ground-truth annotation id {a['id']} is not positive")
        if "bbox" not in a or len(a["bbox"]) != 4 or "area" not in a:
            raise ValueError(f"ground-truth annotation {a['id']} lacks a 4-number bbox or its area")
        img[j], cat[j] = int(a["image_id"]), int(a["category_id"])
        bbox[j], area[j] = a["bbox"], a["area"]
        crowd[j] = 1 if a.get("iscrowd", 0) else 0
    ii, kk = _index_of(image_ids, img), _index_of(category_ids, cat)
    keep = np.nonzero((ii >= 0) & (kk >= 0))[0]                     # COCOeval fetches the annotations of its imgIds and catIds only
    key = kk[keep] * image_ids.size + ii[keep]
    order = np.argsort(key, kind="stable")
    key, keep = key[order], keep[order]
    if key.size and np.unique(key, return_counts=True)[1].max() > MAX_GT_PER_GROUP:
        raise ValueError(f"more than {MAX_GT_PER_GROUP} ground truths in one (image, category) group")
    return Annotations(image_ids, category_ids, np.ascontiguousarray(key, np.int64), np.ascontiguousarray(bbox[keep]),
                       np.ascontiguousarray(area[keep]), np.ascontiguousarray(crowd[keep]), keep)


def to_coco_dets(records, ann):
    """records: the reference's list of {'image_id', 'category_id', 'bbox', 'score'} dicts, or a RECORD_DTYPE /
    COCO_DET_DTYPE array.  Returns a COCO_DET_DTYPE array in the same order.  Raises ValueError for an image id the
    annotations lack (COCO.loadRes asserts it) and for a score that is not finite."""
    if isinstance(records, np.ndarray):
        if records.dtype not in (RECORD_DTYPE, COCO_DET_DTYPE):
            raise ValueError("a record array must have postprocess.RECORD_DTYPE or cocoeval.COCO_DET_DTYPE")
        out = np.empty(records.shape[0], COCO_DET_DTYPE)
        for f in COCO_DET_DTYPE.names:
            out[f] = records[f]                                     # float32 -> float64 is exact
    else:
        out = np.empty(len(records), COCO_DET_DTYPE)
        for j, r in enumerate(records):
            if len(r["bbox"]) != 4:
                raise ValueError(f"detection {j}: bbox must have 4 numbers")
            out[j] = (int(r["image_id"]), int(r["category_id"]), tuple(float(v) for v in r["bbox"]), float(r["score"]))
    if out.size:
        if not np.isfinite(out["score"]).all():
            raise ValueError("a detection's score is not finite")
        missing = _index_of(ann.image_ids, out["image_id"]) < 0
        if missing.any():
            raise ValueError(f"detection image id {int(out['image_id'][missing][0])} is not in the annotations")
    return out


class COCOEvaluator:
    """Holds the grouped ground truth and the appended detections in one device workspace (sized for `max_detections`)."""

    def __init__(self, annotations, device=None, max_detections=1 << 20):
        import torch
        self.ann = load_annotations(annotations)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError("COCOEvaluator runs on the GPU (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        a = self.ann
        self.I, self.K, self.G = int(a.image_ids.size), int(a.category_ids.size), int(a.gt_group.size)
        self.max_detections = int(max_detections)
        L = nat.lib()
        nbytes = L.dod_coco_eval_workspace_bytes(self.max_detections, self.I, self.K, self.G)
        if nbytes == 0:
            raise ValueError(f"unsupported evaluator size: max_detections {self.max_detections} (<= {MAX_DETECTIONS}), {self.I} images, "
                             f"{self.K} categories, {self.G} ground truths")
        with torch.cuda.device(self.device):
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._call(L.dod_coco_eval_set_gt, _np(a.image_ids), _np(a.category_ids), _np(a.gt_group), _np(a.gt_bbox), _np(a.gt_area),
                       _np(a.gt_iscrowd), _np(IOU_THRS), _np(REC_THRS))
        self._n = self._ng = 0

    def _call(self, fn, *args):
        nat.check(fn(nat.ptr(self._ws), self._ws.numel(), self.max_detections, self.I, self.K, self.G, *args, nat.stream_ptr()))

    def reset(self):
        import torch
        with torch.cuda.device(self.device):
            self._call(nat.lib().dod_coco_eval_reset)

    def add_records(self, records):
        """a results list (dicts) or a RECORD_DTYPE array, e.g. what postprocess_packed returns"""
        import torch
        dets = np.ascontiguousarray(to_coco_dets(records, self.ann))
        with torch.cuda.device(self.device):
            self._call(nat.lib().dod_coco_eval_append_host, _np(dets), dets.shape[0])

    def add_packed(self, det, image_ids=None, threshold=0.05):
        """det: packed detections [B, Q, C+4] fp32 on the GPU (forward_packed); image_ids as for postprocess_packed.  Runs
        dod_postprocess and appends its records on the device: no host synchronisation, nothing crosses PCIe."""
        import torch
        if not (isinstance(det, torch.Tensor) and det.is_cuda and det.dtype == torch.float32 and det.dim() == 3 and det.shape[-1] >= 6):
            raise ValueError("det must be a CUDA fp32 tensor [B, Q, C+4]")
        det = det.contiguous()
        B, Q, W = det.shape
        Cn = W - 4
        ids_t = None
        if image_ids is not None:
            if isinstance(image_ids, torch.Tensor):
                ids_t = image_ids.to(device=det.device, dtype=torch.int64).contiguous()
            else:
                ids_t = torch.tensor([i if v is None else int(v) for i, v in enumerate(image_ids)], dtype=torch.int64).to(det.device, non_blocking=True)
            if ids_t.numel() != B:
                raise ValueError("image_ids must have one entry per image")
        L = nat.lib()
        cap = B * Q * (Cn - 1)
        with torch.cuda.device(det.device):
            ws = torch.empty(max(1, L.dod_postprocess_workspace_bytes(B, Q, Cn)), dtype=torch.uint8, device=det.device)
            out = torch.empty(cap * RECORD_DTYPE.itemsize, dtype=torch.uint8, device=det.device)
            count = torch.empty(1, dtype=torch.int64, device=det.device)
            nat.check(L.dod_postprocess(nat.ptr(det), B, Q, Cn, nat.ptr(ids_t), float(threshold), nat.ptr(out), cap, nat.ptr(count),
                                        nat.ptr(ws), ws.numel(), nat.stream_ptr()))
            self._call(L.dod_coco_eval_append, nat.ptr(out), nat.ptr(count), cap)

    def evaluate(self):
        """{'stats': the 12 COCOeval.stats, 'precision': [10,101,K,4,3], 'recall': [10,K,4,3]} (numpy float64)"""
        import torch
        stats, n, ng = (C.c_double * 12)(), C.c_int64(0), C.c_int32(0)
        with torch.cuda.device(self.device):
            prec = torch.empty((len(IOU_THRS), len(REC_THRS), self.K, 4, 3), dtype=torch.float64, device=self.device)
            rec = torch.empty((len(IOU_THRS), self.K, 4, 3), dtype=torch.float64, device=self.device)
            self._call(nat.lib().dod_coco_eval_evaluate, C.cast(stats, C.c_void_p), nat.ptr(prec), nat.ptr(rec), C.c_void_p(C.addressof(n)),
                       C.c_void_p(C.addressof(ng)))
        self._n, self._ng = int(n.value), int(ng.value)
        return {"stats": [float(v) for v in stats], "precision": prec.cpu().numpy(), "recall": rec.cpu().numpy()}

    def matches(self):
        """After evaluate(): what evaluateImg decided.  Per detection in (category, image, score descending) order: 'index' (the
        input position), 'rank' in its group, 'matched' / 'ignored' uint64 with bit a*10+t for area range a and threshold t
        (meaningful for rank < 100); per ground-truth group: 'group_key' (category index * I + image index) and 'npig' [., 4]."""
        import torch
        n, ng = self._n, self._ng
        with torch.cuda.device(self.device):
            t = lambda m, dt: torch.zeros(max(m, 1), dtype=dt, device=self.device)      # noqa: E731
            idx, rank, dm, dig = t(n, torch.int32), t(n, torch.int32), t(n, torch.int64), t(n, torch.int64)
            gkey, npig = t(ng, torch.int64), t(ng * 4, torch.int32)
            nat.check(nat.lib().dod_coco_eval_matches(nat.ptr(self._ws), self._ws.numel(), self.max_detections, self.I, self.K, self.G, n,
                                                      nat.ptr(idx), nat.ptr(rank), nat.ptr(dm), nat.ptr(dig), ng, nat.ptr(gkey), nat.ptr(npig),
                                                      nat.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        return {"index": idx[:n].cpu().numpy(), "rank": rank[:n].cpu().numpy(), "matched": dm[:n].cpu().numpy().view(np.uint64),
                "ignored": dig[:n].cpu().numpy().view(np.uint64), "group_key": gkey[:ng].cpu().numpy(),
                "npig": npig[:ng * 4].cpu().numpy().reshape(ng, 4)}


def _np(a):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


def metrics_from_stats(stats):
    """the reference's six keys (utils.py:266-273) from COCOeval.stats"""
    return {k: float(stats[i]) for i, k in enumerate(METRIC_KEYS)}


def compute_coco_metrics(results, annotation_file):
    """Drop-in for dino_detector.utils.compute_coco_metrics (utils.py:243-276): results = the list evaluate_coco returns,
    annotation_file = the COCO ground-truth json.  Returns {'AP', 'AP50', 'AP75', 'APs', 'APm', 'APl'} as Python floats."""
    ev = COCOEvaluator(annotation_file, max_detections=max(1, len(results)))
    ev.add_records(results)
    return metrics_from_stats(ev.evaluate()["stats"])


def validate_coco(model, dataloader, device, annotations, threshold=0.05, max_detections=1 << 20):
    """evaluate_coco + compute_coco_metrics without the host in between: forward -> add_packed per batch -> one evaluate.
    Returns the six metrics plus 'stats' (all 12)."""
    import torch
    ev = COCOEvaluator(annotations, device, max_detections)
    model.eval()
    with torch.no_grad():
        for images, targets in dataloader:
            images = images.to(device)
            if hasattr(model, "forward_packed"):
                det = model.forward_packed(images)
            else:                                            # any module with the reference's output dict
                o = model(images)
                det = torch.cat([o["pred_logits"], o["pred_boxes"]], dim=-1).float()
            ids = [t.get("image_id", None) for t in targets]   # utils.py:203: default = index in the batch
            ev.add_packed(det, [None if v is None else int(v) for v in ids], threshold)
    stats = ev.evaluate()["stats"]
    return dict(metrics_from_stats(stats), stats=stats)
