"""Yardsticks of `COCOEvaluator.add_detections` and `.confusion_matrix` (a helper, not a test): plain numpy and Python loops,
independent of dinov2_od_amd.

    scene_to_detections      a scene's result list packed as model.detect returns it: padded [B, Kd] arrays, counts, a label table
    detections_to_records    include/dinodet.h dod_coco_eval_append_detections restated: the records those arrays stand for
    confusion_ref            include/dinodet.h dod_coco_eval_confusion restated: the cross-class greedy match, in loops
"""
import numpy as np


def scene_to_detections(dataset, results, Kd, pad="nan"):
    """-> dict of boxes [B, Kd, 4] f32 xyxy, scores [B, Kd] f32, labels [B, Kd] i32, counts [B] i32, image_ids [B] i64 and the
    table category_ids [n] i64.  Images in the file's order, rows in list order, x2 = float32(x + w) (so the width read back,
    x2 - x1, is generally not the list's w: detections_to_records says what it is).  labels index category_ids, which holds one id no
    result uses, in front, so that no label equals a category index by accident.  Padding rows: NaN boxes and scores and label
    -1 (pad='nan'), or zeros (pad='zero')."""
    image_ids = [int(im["id"]) for im in dataset["images"]]
    used = {int(r["category_id"]) for r in results} | {int(c["id"]) for c in dataset["categories"]}
    table = [max(used) + 1000] + [int(c["id"]) for c in dataset["categories"]] + sorted(used - {int(c["id"]) for c in dataset["categories"]})
    label_of = {c: n for n, c in enumerate(table)}
    B = len(image_ids)
    fill = np.nan if pad == "nan" else 0.0
    boxes = np.full((B, Kd, 4), fill, np.float32)
    scores = np.full((B, Kd), fill, np.float32)
    labels = np.full((B, Kd), -1 if pad == "nan" else 0, np.int32)
    counts = np.zeros(B, np.int32)
    row_of = {i: b for b, i in enumerate(image_ids)}
    for r in results:
        b = row_of[int(r["image_id"])]
        n = int(counts[b])
        if n >= Kd:
            raise ValueError(f"image {r['image_id']} has more than Kd = {Kd} results")
        x, y, w, h = (float(v) for v in r["bbox"])
        boxes[b, n] = (np.float32(x), np.float32(y), np.float32(x + w), np.float32(y + h))
        scores[b, n] = np.float32(r["score"])
        labels[b, n] = label_of[int(r["category_id"])]
        counts[b] = n + 1
    return {"boxes": boxes, "scores": scores, "labels": labels, "counts": counts, "image_ids": np.asarray(image_ids, np.int64),
            "category_ids": np.asarray(table, np.int64)}


def detections_to_records(boxes, scores, labels, counts, image_ids, category_ids=None):
    """the result list the arrays stand for: rows 0 .. counts[b]-1 of every image, images in order; x = x1, y = y1, w = x2 - x1 and
    h = y2 - y1 computed in double from the widened floats; category_id = category_ids[label], or the label without a table"""
    out = []
    for b in range(len(counts)):
        for r in range(int(counts[b])):
            x1, y1, x2, y2 = (float(v) for v in boxes[b, r])
            lab = int(labels[b, r])
            out.append({"image_id": int(image_ids[b]), "category_id": lab if category_ids is None else int(category_ids[lab]),
                        "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(scores[b, r])})
    return out


def _iou(d, g):
    """maskApi.c bbIou for a non-crowd ground truth, xywh doubles"""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    return i / (d[2] * d[3] + g[2] * g[3] - i)


def confusion_ref(dataset, records, score_threshold, iou_threshold):
    """int64 [K+1, K+1].  Per image: candidates = its records of a category the annotations hold with score >= score_threshold, by
    (score descending, list order) with -0.0 == 0.0; ground truths = its non-crowd annotations of all categories by (category index,
    file order).  Each candidate takes, of the ground truths not yet taken, the one of the highest IoU >= min(iou_threshold,
    1 - 1e-10), the later one on a tie.  matrix[pred][gt] per match, matrix[pred][K] per candidate left, matrix[K][gt] per ground
    truth left."""
    img_ids = sorted({int(im["id"]) for im in dataset["images"]})
    cat_ids = sorted({int(c["id"]) for c in dataset["categories"]})
    kidx = {c: k for k, c in enumerate(cat_ids)}
    K = len(cat_ids)
    M = np.zeros((K + 1, K + 1), np.int64)
    gts = {i: [] for i in img_ids}
    for a in dataset["annotations"]:
        if a["image_id"] in gts and a["category_id"] in kidx and not a.get("iscrowd", 0):
            gts[a["image_id"]].append((kidx[a["category_id"]], [float(v) for v in a["bbox"]]))
    dts = {i: [] for i in img_ids}
    for r in records:
        assert r["image_id"] in dts
        if r["category_id"] in kidx and float(r["score"]) >= score_threshold:
            dts[r["image_id"]].append((kidx[r["category_id"]], [float(v) for v in r["bbox"]], float(r["score"])))
    thr = min(iou_threshold, 1 - 1e-10)
    for i in img_ids:
        gt = sorted(gts[i], key=lambda e: e[0])                       # stable: file order inside a category
        dt = [dts[i][j] for j in np.argsort([-d[2] for d in dts[i]], kind="mergesort")] if dts[i] else []
        taken = [False] * len(gt)
        for p, box, _ in dt:
            best, m = thr, -1
            for g, (_, gbox) in enumerate(gt):
                if taken[g]:
                    continue
                v = _iou(box, gbox)
                if not v >= best:
                    continue
                best, m = v, g
            if m < 0:
                M[p, K] += 1
            else:
                taken[m] = True
                M[p, gt[m][0]] += 1
        for g, t in enumerate(taken):
            if not t:
                M[K, gt[g][0]] += 1
    return M
