"""COCO bbox evaluation on the GPU: the host side of `dod_coco_eval_*` (include/dinodet.h, csrc/cocoeval.hip).

Replaces the reference's `compute_coco_metrics(results, annotation_file)` (dino_detector/utils.py:243-276), i.e. pycocotools'
`COCO.loadRes` + `COCOeval(gt, dt, 'bbox')` `.evaluate() / .accumulate() / .summarize()` with default parameters and
useCats = 1.  The device code restates COCOeval operation for operation in double precision: `precision` and `recall` are
the arrays pycocotools builds, bit for bit, and the 12 `stats` their means.

    compute_coco_metrics(results, annotation_file)   the reference's function: same signature, same six keys
    COCOEvaluator(annotations, device)               .add_records / .add_packed / .add_detections / .evaluate / .confusion_matrix / .reset
    validate_coco(model, dataloader, device, annotations)   forward -> add_packed per batch (no host sync) -> one evaluate
    validate_coco(..., detect=dict(...) | sliced=dict(...), category_ids=table)   model.detect / detect_sliced -> add_detections
    per_category_metrics(result, annotations)        AP / AP50 / AR100 of every category from evaluate()'s arrays (host only)

The evaluator compares what it is given: the reference emits normalised boxes and class indices as `category_id`
(utils.py:225-233), and neither is "fixed" in `add_packed` or in `validate_coco` without `detect=` / `sliced=`.  `add_detections`
takes what `model.detect` and `detect_sliced` return -- pixel xyxy boxes in each image's own size, a label per row -- and maps the
labels through `category_ids`, which is what a real COCO annotation file (pixel boxes, COCO category ids) is scored against.
One deviation from pycocotools: an empty result list evaluates (AP = AR = 0 where ground truth exists) instead of raising.

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
MAX_CONFUSION_CATEGORIES = 2048          # include/dinodet.h dod_coco_eval_confusion
MAX_GT_PER_IMAGE = 1024                  #   non-crowd ground truths of one image, all categories
MAX_APPEND_IMAGES = 1 << 16              # include/dinodet.h dod_coco_eval_append_detections: images of one call
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

    def gt_per_image(self):
        """non-crowd ground truths of every image, all categories together [I]: what the confusion matrix matches against"""
        I = self.image_ids.size
        return np.bincount((self.gt_group % I)[self.gt_iscrowd == 0], minlength=I).astype(np.int64)


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


def _id_list(ids, n, name):
    """ids (a sequence or an integer tensor) -> a tuple of Python ints, or the tensor itself when it is on a GPU (reading it would
    synchronise); ValueError unless it is one-dimensional with n entries (n None: at least one)"""
    import torch
    if isinstance(ids, torch.Tensor):
        if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise ValueError(f"{name} must be a one-dimensional integer tensor or a sequence of ints")
        out, size = (ids if ids.is_cuda else tuple(int(v) for v in ids.tolist())), ids.numel()
    else:
        try:
            out = tuple(int(v) for v in ids)
        except TypeError:
            raise ValueError(f"{name} must be a one-dimensional integer tensor or a sequence of ints") from None
        size = len(out)
    if size < 1 or (n is not None and size != n):
        raise ValueError(f"{name} must have {'at least one entry' if n is None else f'one entry per image ({n})'}, got {size}")
    return out


def _ids_on(ids, device):
    """what _id_list returned -> an int64 tensor on device, without a host synchronisation"""
    import torch
    if isinstance(ids, tuple):
        return torch.tensor(ids, dtype=torch.int64).to(device, non_blocking=True)
    return ids.to(device=device, dtype=torch.int64).contiguous()


def check_detections(result, image_ids, category_ids=None):
    """The argument checks of COCOEvaluator.add_detections, the device looked at last so that every argument is checked whether or not
    a GPU is present.  -> ((scores, labels, boxes, counts), image ids, category table or None), the last two as _id_list returns them"""
    import torch
    try:
        t = (result.scores, result.labels, result.boxes, result.counts)
    except AttributeError:
        raise ValueError("result must be a postprocess.Detections (scores, labels, boxes, queries, counts)") from None
    scores, labels, boxes, counts = t
    if not all(isinstance(v, torch.Tensor) for v in t):
        raise ValueError("result must hold tensors")
    if scores.dim() != 2 or scores.dtype != torch.float32 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise ValueError("result.scores must be fp32 [B, Kd] with B >= 1 and Kd >= 1")
    B, Kd = scores.shape
    if B > MAX_APPEND_IMAGES:
        raise ValueError(f"at most {MAX_APPEND_IMAGES} images per call, got {B}")
    if tuple(labels.shape) != (B, Kd) or labels.dtype != torch.int32:
        raise ValueError(f"result.labels must be int32 [{B}, {Kd}]")
    if tuple(boxes.shape) != (B, Kd, 4) or boxes.dtype != torch.float32:
        raise ValueError(f"result.boxes must be fp32 [{B}, {Kd}, 4]")
    if tuple(counts.shape) != (B,) or counts.dtype != torch.int32:
        raise ValueError(f"result.counts must be int32 [{B}]")
    ids = _id_list(image_ids, B, "image_ids")
    table = None if category_ids is None else _id_list(category_ids, None, "category_ids")
    if not all(v.is_cuda for v in t) or len({v.device for v in t}) != 1:
        raise ValueError("result must hold CUDA tensors of one device (there is no CPU fallback)")
    return t, ids, table


def check_confusion_limits(n_categories, max_gt_per_image):
    """ValueError beyond what dod_coco_eval_confusion takes (include/dinodet.h)"""
    if n_categories > MAX_CONFUSION_CATEGORIES:
        raise ValueError(f"the confusion matrix takes at most {MAX_CONFUSION_CATEGORIES} categories, the annotations have {n_categories}")
    if max_gt_per_image > MAX_GT_PER_IMAGE:
        raise ValueError(f"the confusion matrix takes at most {MAX_GT_PER_IMAGE} non-crowd ground truths per image, one image has {max_gt_per_image}")


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
        self.max_gt_per_image = int(a.gt_per_image().max())      # what confusion_matrix checks against its limit
        self._catmap = None
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

    def add_detections(self, result, image_ids, category_ids=None):
        """result: a postprocess.Detections (so slicing.SlicedDetections / FusedDetections too) of CUDA tensors -- scores [B, Kd]
        fp32, labels [B, Kd] int32, boxes [B, Kd, 4] fp32 pixel xyxy, counts [B] int32 -- as model.detect / detect_sliced return it;
        image_ids: a sequence or tensor of B ids; category_ids: the table label -> annotation category id (a sequence or tensor,
        kept on the device per evaluator), None = the label is the id.  Appends rows 0 .. counts[b]-1 of every image, images in
        order, as xywh double records on the device (dod_coco_eval_append_detections): no host synchronisation."""
        import torch
        (scores, labels, boxes, counts), ids, table = check_detections(result, image_ids, category_ids)
        B, Kd = scores.shape
        if scores.device != self.device:
            raise ValueError(f"result is on {scores.device}, the evaluator on {self.device}")
        with torch.cuda.device(self.device):
            ids_t = _ids_on(ids, self.device)
            map_t = None if table is None else self._category_map(table)
            scores, labels, boxes, counts = (t.contiguous() for t in (scores, labels, boxes, counts))
            self._call(nat.lib().dod_coco_eval_append_detections, nat.ptr(boxes), nat.ptr(scores), nat.ptr(labels), nat.ptr(counts), B, Kd,
                       nat.ptr(ids_t), nat.ptr(map_t), 0 if map_t is None else map_t.numel())

    def _category_map(self, table):
        """the label -> category id table on the evaluator's device.  A host table is uploaded once and kept until another one comes (a
        validation loop passes the same one every batch); a tensor that is on a GPU already is the caller's own cache"""
        if not isinstance(table, tuple):
            return _ids_on(table, self.device)
        if self._catmap is None or self._catmap[0] != table:
            self._catmap = (table, _ids_on(table, self.device))
        return self._catmap[1]

    def confusion_matrix(self, score_threshold=0.25, iou_threshold=0.5):
        """int64 numpy [K+1, K+1]: matrix[p][g] counts (predicted category index p, ground-truth category index g) pairs over the
        appended detections with score >= score_threshold, greedily matched in score order to the non-crowd ground truths of
        their image at IoU >= iou_threshold across categories (include/dinodet.h dod_coco_eval_confusion); index K is
        "background": matrix[p][K] unmatched detections, matrix[K][g] missed ground truths.  Indices follow `ann.category_ids`."""
        import torch
        score_threshold, iou_threshold = float(score_threshold), float(iou_threshold)
        if score_threshold != score_threshold or iou_threshold != iou_threshold:
            raise ValueError("score_threshold and iou_threshold must not be NaN")
        check_confusion_limits(self.K, self.max_gt_per_image)
        with torch.cuda.device(self.device):
            m = torch.empty((self.K + 1, self.K + 1), dtype=torch.int64, device=self.device)
            self._call(nat.lib().dod_coco_eval_confusion, score_threshold, iou_threshold, nat.ptr(m))
            return m.cpu().numpy()

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


def per_category_metrics(result, annotations):
    """result: what COCOEvaluator.evaluate() returned; annotations: as for load_annotations.  -> {category id: {'AP', 'AP50',
    'AR100'}}: COCOeval.summarize's rule restricted to one category -- the mean over the entries > -1 of precision[:, :, k, 0, 2]
    (AP), precision[0, :, k, 0, 2] (AP50) and recall[:, k, 0, 2] (AR100), area range 'all' and maxDets 100; -1 when there are none.
    Host only."""
    ann = load_annotations(annotations)
    prec, rec = np.asarray(result["precision"]), np.asarray(result["recall"])
    K = int(ann.category_ids.size)
    if prec.shape != (len(IOU_THRS), len(REC_THRS), K, 4, 3) or rec.shape != (len(IOU_THRS), K, 4, 3):
        raise ValueError(f"precision / recall are not the arrays of an evaluation over these {K} categories")

    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return {int(c): {"AP": mean(prec[:, :, k, 0, 2]), "AP50": mean(prec[0, :, k, 0, 2]), "AR100": mean(rec[:, k, 0, 2])}
            for k, c in enumerate(ann.category_ids)}


def compute_coco_metrics(results, annotation_file):
    """Drop-in for dino_detector.utils.compute_coco_metrics (utils.py:243-276): results = the list evaluate_coco returns,
    annotation_file = the COCO ground-truth json.  Returns {'AP', 'AP50', 'AP75', 'APs', 'APm', 'APl'} as Python floats."""
    ev = COCOEvaluator(annotation_file, max_detections=max(1, len(results)))
    ev.add_records(results)
    return metrics_from_stats(ev.evaluate()["stats"])


def validate_coco(model, dataloader, device, annotations, threshold=0.05, max_detections=1 << 20, *, detect=None, sliced=None,
                  category_ids=None):
    """evaluate_coco + compute_coco_metrics without the host in between: forward -> add_packed per batch -> one evaluate.
    Returns the six metrics plus 'stats' (all 12).  That scores the reference's records: normalised boxes, the class index as id.
    detect=dict(top_k=..., threshold=..., nms_iou=..., ...): model.detect(images, sizes=every target's 'orig_size' (height, width),
    the input's own (H, W) where a target has none, **detect) -> add_detections per batch instead: pixel boxes, labels mapped through
    category_ids (None = the label is the id), which is what a COCO annotation file holds.  sliced=dict(...): the loader yields
    lists of raw uint8 [H_i, W_i, 3] images and model.detect_sliced(images, **sliced) runs instead.  These two also return
    evaluate()'s 'precision' and 'recall'.  `threshold` is add_packed's and is not read by them."""
    import torch
    if detect is not None and sliced is not None:
        raise ValueError("detect= and sliced= exclude each other")
    if detect is None and sliced is None and category_ids is not None:
        raise ValueError("category_ids maps the labels of detect= / sliced=; without either the class index is the id")
    for name, kw in (("detect", detect), ("sliced", sliced)):
        if kw is not None and not isinstance(kw, dict):
            raise ValueError(f"{name}= takes a dict of keyword arguments")
    if detect is not None and "sizes" in detect:
        raise ValueError("detect= takes no 'sizes': they come from every target's 'orig_size'")
    if category_ids is not None:
        category_ids = _id_list(category_ids, None, "category_ids")
    ev = COCOEvaluator(annotations, device, max_detections)
    if detect is not None or sliced is not None:
        for images, targets in dataloader:
            ids = [i if t.get("image_id", None) is None else int(t["image_id"]) for i, t in enumerate(targets)]
            if sliced is not None:
                res = model.detect_sliced(images, **sliced)
            else:
                images = images.to(device)
                own = (int(images.shape[-2]), int(images.shape[-1]))
                sizes = [[float(v) for v in torch.as_tensor(t["orig_size"]).reshape(2).tolist()] if "orig_size" in t else own for t in targets]
                res = model.detect(images, sizes=sizes, **detect)
            ev.add_detections(res, ids, category_ids)
        out = ev.evaluate()
        return dict(metrics_from_stats(out["stats"]), **out)      # with 'precision' and 'recall': per_category_metrics reads them
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
