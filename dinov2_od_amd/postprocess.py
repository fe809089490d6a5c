"""Detection post-processing on the GPU: the host side of `dod_postprocess` (include/dinodet.h).

Mirrors the reference's `evaluate_coco(model, dataloader, device, output_file=None)` (dino_detector/utils.py:167-240): same
signature, same list of `{'image_id', 'category_id', 'bbox', 'score'}` dicts in the same order, same JSON dump -- but the
sigmoid / threshold / box conversion / compaction of utils.py:195-233 (a triple Python loop with a `.cpu().numpy()` per
class) runs as three small HIP kernels over the packed detections, and only the kept records cross PCIe.
`detect_packed` is the other consumer of the packed buffer (`dod_detect`): per image the `top_k` best (query, class) pairs as
pixel xyxy boxes with score and label, optionally after greedy NMS, in fixed-shape tensors and without a host sync.
No CPU fallback: without the HIP library this module raises.
"""
import collections
import ctypes as C
import json

import numpy as np
import torch

from . import _native as nat

RECORD_DTYPE = np.dtype([("image_id", "<i8"), ("category_id", "<i4"), ("query", "<i4"), ("bbox", "<f4", (4,)),
                         ("score", "<f4"), ("reserved", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(nat.DodDetection) == 40


def postprocess_packed(det, num_classes, image_ids=None, threshold=0.05, max_out=None):
    """det: packed detections [B, Q, C+4] fp32 on the GPU (DINOv2ObjectDetector.forward_packed).  image_ids: sequence of
    ints / None (None -> the index in the batch, utils.py:203) or an int64 CUDA tensor.
    Returns a numpy structured array (RECORD_DTYPE) of the kept detections in the reference's order."""
    if not (isinstance(det, torch.Tensor) and det.is_cuda and det.dtype == torch.float32 and det.dim() == 3):
        raise ValueError("det must be a CUDA fp32 tensor [B, Q, C+4]")
    B, Q, W = det.shape
    Cn = int(num_classes)
    if W != Cn + 4 or Cn < 2:
        raise ValueError(f"det has {W} columns, expected num_classes + 4 = {Cn + 4}")
    det = det.contiguous()
    L = nat.lib()
    ids_t = None
    if image_ids is not None:
        if isinstance(image_ids, torch.Tensor):
            ids_t = image_ids.to(device=det.device, dtype=torch.int64).contiguous()
        else:
            ids_t = torch.tensor([i if v is None else int(v) for i, v in enumerate(image_ids)], dtype=torch.int64,
                                 device=det.device)
        if ids_t.numel() != B:
            raise ValueError("image_ids must have one entry per image")
    cap = B * Q * (Cn - 1) if max_out is None else int(max_out)
    ws = torch.empty(max(1, L.dod_postprocess_workspace_bytes(B, Q, Cn)), dtype=torch.uint8, device=det.device)
    out = torch.empty(max(1, cap) * RECORD_DTYPE.itemsize, dtype=torch.uint8, device=det.device)
    count = torch.zeros(1, dtype=torch.int64, device=det.device)
    nat.check(L.dod_postprocess(nat.ptr(det), B, Q, Cn, nat.ptr(ids_t), float(threshold), nat.ptr(out), cap, nat.ptr(count),
                                nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    n = min(int(count.item()), cap)                       # the one host sync: how many records to fetch
    return out[: n * RECORD_DTYPE.itemsize].cpu().numpy().view(RECORD_DTYPE).copy()


Detections = collections.namedtuple("Detections", ["scores", "labels", "boxes", "queries", "counts"])
MAX_TOP_K, MAX_TOP_K_NMS = 1024, 512      # include/dinodet.h dod_detect


def _sizes_rows(sizes, B):
    """None / one (h, w) / a sequence of B pairs / a [B, 2] tensor -> a [B, 2] tensor of (height, width) on its own device, or None"""
    if sizes is None:
        return None
    t = sizes if isinstance(sizes, torch.Tensor) else torch.from_numpy(np.asarray(sizes, dtype=np.float32))
    if t.dim() == 1 and t.numel() == 2:
        t = t.reshape(1, 2).expand(B, 2)
    if t.dim() != 2 or tuple(t.shape) != (B, 2):
        raise ValueError(f"sizes must be None, one (height, width) or one pair per image ({B}), got shape {tuple(t.shape)}")
    return t


def _check_det(det, num_classes, rows="B"):
    """det [rows, Q, C+4] against num_classes -> (rows, Q, C).  The device is not looked at: the callers check it last, so that every
    argument is checked whether or not a GPU is present"""
    if not (isinstance(det, torch.Tensor) and det.dtype == torch.float32 and det.dim() == 3):
        raise ValueError(f"det must be a CUDA fp32 tensor [{rows}, Q, C+4]")
    n, Q, W = det.shape
    Cn = int(num_classes)
    if W != Cn + 4 or Cn < 1:
        raise ValueError(f"det has {W} columns, expected num_classes + 4 = {Cn + 4}")
    return n, Q, Cn


def _check_top_k(Cn, top_k, nms_iou, skip_background, max_k_nms):
    """-> (first_class, K, iou_threshold as the C entry points take it: -1 without NMS); max_k_nms: the entry point's K limit with NMS"""
    first = 1 if skip_background else 0
    if first >= Cn:
        raise ValueError("skip_background leaves no class (num_classes == 1)")
    nms = nms_iou is not None
    if nms and not float(nms_iou) >= 0.0:
        raise ValueError(f"nms_iou must be None or >= 0, got {nms_iou}")
    K, kmax = int(top_k), max_k_nms if nms else MAX_TOP_K
    if not 1 <= K <= kmax:
        raise ValueError(f"top_k must be in 1..{kmax}{' with NMS' if kmax < MAX_TOP_K else ''}, got {K}")
    return first, K, float(nms_iou) if nms else -1.0


def _alloc(cls, B, K, dev, extra=0):
    """cls(scores, labels, boxes, queries, counts, then `extra` more [B, K] int32 tensors) uninitialised on dev"""
    def i32():
        return torch.empty(B, K, dtype=torch.int32, device=dev)
    return cls(torch.empty(B, K, dtype=torch.float32, device=dev), i32(), torch.empty(B, K, 4, dtype=torch.float32, device=dev), i32(),
               torch.empty(B, dtype=torch.int32, device=dev), *(i32() for _ in range(extra)))


def detect_packed(det, num_classes, sizes=None, top_k=100, threshold=-1.0, nms_iou=None, class_agnostic=False, clamp=True,
                  skip_background=True):
    """det: packed detections [B, Q, C+4] fp32 on the GPU.  Per image the `top_k` highest-logit (query, class) pairs -- of those with
    sigmoid(logit) > threshold when threshold >= 0, class 0 left out when skip_background -- in (logit descending, q*C + c ascending)
    order, as xyxy boxes scaled by sizes (height, width; None keeps them normalised) and clamped to the image when clamp; with
    nms_iou (>= 0) greedy NMS, per class unless class_agnostic, removes later boxes whose IoU with a survivor exceeds it.
    Returns Detections(scores [B,K] f32, labels [B,K] i32, boxes [B,K,4] f32, queries [B,K] i32, counts [B] i32) of CUDA tensors; rows
    at and beyond counts[b] are padding (score 0, label -1, query -1, box 0).  One launch on the current stream, no host sync."""
    B, Q, Cn = _check_det(det, num_classes)
    if B < 1 or Q < 1 or Q * Cn > (1 << 20):
        raise ValueError(f"need at least one image and one query and at most 2^20 (query, class) pairs per image, got B={B} Q={Q} C={Cn}")
    first, K, iou = _check_top_k(Cn, top_k, nms_iou, skip_background, MAX_TOP_K_NMS)
    st = _sizes_rows(sizes, B)
    if not det.is_cuda:                                       # last: every argument is checked whether or not a GPU is present
        raise ValueError("det must be a CUDA fp32 tensor [B, Q, C+4] (there is no CPU fallback)")
    det = det.contiguous()
    L = nat.lib()
    dev = det.device
    if st is not None:
        st = st.to(device=dev, dtype=torch.float32).contiguous()
    ws = torch.empty(L.dod_detect_workspace_bytes(B, Q, Cn, K), dtype=torch.uint8, device=dev)
    out = _alloc(Detections, B, K, dev)
    nat.check(L.dod_detect(nat.ptr(det), B, Q, Cn, first, nat.ptr(st), float(threshold), K, iou,
                           int(bool(class_agnostic)), int(bool(clamp)), nat.ptr(out.scores), nat.ptr(out.labels), nat.ptr(out.queries),
                           nat.ptr(out.boxes), nat.ptr(out.counts), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    return out


def detections_to_list(result):
    """Detections -> per image {"boxes" [n,4], "scores" [n], "labels" [n]} trimmed to counts (the one host sync: it reads counts)"""
    counts = result.counts.tolist()
    return [{"boxes": result.boxes[b, :n], "scores": result.scores[b, :n], "labels": result.labels[b, :n]} for b, n in enumerate(counts)]


def records_to_coco(rec):
    """structured records -> the reference's list of dicts (utils.py:227-232): python ints / floats"""
    return [{"image_id": int(r["image_id"]), "category_id": int(r["category_id"]),
             "bbox": [float(v) for v in r["bbox"]], "score": float(r["score"])} for r in rec]


def evaluate_coco(model, dataloader, device, output_file=None, threshold=0.05):
    """Drop-in for dino_detector.utils.evaluate_coco (utils.py:167-240) for the engine-backed detector."""
    model.eval()
    results = []
    with torch.no_grad():
        for images, targets in dataloader:
            images = images.to(device)
            if hasattr(model, "forward_packed"):
                det = model.forward_packed(images)
                ncls = det.shape[-1] - 4
            else:                                            # any module with the reference's output dict
                o = model(images)
                det = torch.cat([o["pred_logits"], o["pred_boxes"]], dim=-1).float()
                ncls = o["pred_logits"].shape[-1]
            ids = [t.get("image_id", None) for t in targets]   # utils.py:203: default = index in the batch
            ids = [None if v is None else int(v) for v in ids]
            results.extend(records_to_coco(postprocess_packed(det, ncls, ids, threshold)))
    if output_file is not None:
        with open(output_file, "w") as f:
            json.dump(results, f)
    return results
