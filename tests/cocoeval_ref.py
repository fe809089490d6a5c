"""Yardstick of the device COCO evaluator (a helper, not a test): pycocotools' COCOeval for iouType 'bbox', useCats = 1 and
default parameters, restated in plain numpy loop for loop -- `_prepare`, `computeIoU` (maskApi.c bbIou), `evaluateImg`,
`accumulate`, `summarize` -- from the published algorithm and independent of dinov2_od_amd.  pycocotools itself is not
installed where this project runs.  Also a seeded scene generator whose scenes hold every case the evaluator must get right.
"""
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def bb_iou(dt, gt, iscrowd):
    """maskApi.c bbIou: dt [D][4], gt [G][4] xywh doubles -> o[d][g]"""
    o = np.zeros((len(dt), len(gt)), np.float64)
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        crowd = bool(iscrowd[g])
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


class RefCOCOeval:
    def __init__(self, dataset, results):
        self.img_ids = sorted({int(im["id"]) for im in dataset["images"]})
        self.cat_ids = sorted({int(c["id"]) for c in dataset["categories"]})
        imgs, cats = set(self.img_ids), set(self.cat_ids)
        # _prepare
        self.gts, self.dts = defaultdict(list), defaultdict(list)
        for a in dataset["annotations"]:
            if a["image_id"] in imgs and a["category_id"] in cats:
                g = {"bbox": [float(v) for v in a["bbox"]], "area": float(a["area"]), "iscrowd": int(a.get("iscrowd", 0)), "id": a["id"]}
                g["ignore"] = g["iscrowd"]
                self.gts[a["image_id"], a["category_id"]].append(g)
        for n, r in enumerate(results):                    # COCO.loadRes: id = position + 1, area = w * h
            assert r["image_id"] in imgs
            bb = [float(v) for v in r["bbox"]]
            self.dts[r["image_id"], r["category_id"]].append({"bbox": bb, "area": bb[2] * bb[3], "score": float(r["score"]), "id": n + 1})
        self.eval_imgs = {}

    def compute_iou(self, img, cat):
        gt, dt = self.gts[img, cat], self.dts[img, cat]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in inds]
        if len(dt) > MAX_DETS[-1]:
            dt = dt[0:MAX_DETS[-1]]
        if len(gt) == 0 or len(dt) == 0:
            return []
        return bb_iou([d["bbox"] for d in dt], [g["bbox"] for g in gt], [g["iscrowd"] for g in gt])

    def evaluate_img(self, img, cat, a_rng, max_det):
        gt, dt = self.gts[img, cat], self.dts[img, cat]
        if len(gt) == 0 and len(dt) == 0:
            return None
        gt_ignore = [1 if (g["ignore"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
        gtind = np.argsort(gt_ignore, kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:max_det]]
        iscrowd = [int(g["iscrowd"]) for g in gt]
        ious = self.ious[img, cat]
        ious = ious[:, gtind] if len(ious) > 0 else ious
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([gt_ignore[i] for i in gtind])
        dt_ig = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"dt_ids": [d["id"] for d in dt], "dt_matches": dtm, "dt_scores": [d["score"] for d in dt], "gt_ignore": gt_ig, "dt_ignore": dt_ig}

    def evaluate(self):
        self.ious = {(i, c): self.compute_iou(i, c) for i in self.img_ids for c in self.cat_ids}
        max_det = MAX_DETS[-1]
        self.eval_list = [self.evaluate_img(i, c, a, max_det) for c in self.cat_ids for a in AREA_RNG for i in self.img_ids]

    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        I0 = len(self.img_ids)
        precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
        for k in range(K):
            Nk = k * A * I0
            for a in range(A):
                Na = a * I0
                for m, max_det in enumerate(MAX_DETS):
                    E = [self.eval_list[Nk + Na + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dt_scores = np.concatenate([e["dt_scores"][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    dtm = np.concatenate([e["dt_matches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e["dt_ignore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e["gt_ignore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp, fp = np.array(tp), np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds_r = np.searchsorted(rc, REC_THRS, side="left")
                        try:
                            for ri, pi in enumerate(inds_r):
                                q[ri] = pr[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
        self.precision, self.recall = precision, recall

    def summarize(self):
        def _s(ap, iou_thr=None, area=0, m=2):
            if ap:
                s = self.precision
                if iou_thr is not None:
                    s = s[np.where(iou_thr == IOU_THRS)[0]]
                s = s[:, :, :, area, m]
            else:
                s = self.recall[:, :, area, m]
            return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
        self.stats = [_s(1), _s(1, .5), _s(1, .75), _s(1, area=1), _s(1, area=2), _s(1, area=3),
                      _s(0, m=0), _s(0, m=1), _s(0, m=2), _s(0, area=1), _s(0, area=2), _s(0, area=3)]
        return self.stats


def evaluate(dataset, results):
    """-> {'stats' [12], 'precision' [10,101,K,4,3], 'recall' [10,K,4,3], 'groups'}.  groups: {(category index, image index):
    {'dt_index' [D] input positions in rank order (D <= 100), 'matched' / 'ignored' bool [4,10,D], 'npig' [4]}} for every
    (image, category) that has a ground truth or a detection."""
    e = RefCOCOeval(dataset, results)
    e.evaluate()
    e.accumulate()
    e.summarize()
    groups = {}
    I0, A = len(e.img_ids), len(AREA_RNG)
    for k in range(len(e.cat_ids)):
        for i in range(I0):
            per_a = [e.eval_list[k * A * I0 + a * I0 + i] for a in range(A)]
            if per_a[0] is None:
                continue
            groups[k, i] = {"dt_index": np.array([d - 1 for d in per_a[0]["dt_ids"]], np.int64),
                            "matched": np.stack([x["dt_matches"] != 0 for x in per_a]),
                            "ignored": np.stack([np.asarray(x["dt_ignore"], bool) for x in per_a]),
                            "npig": np.array([np.count_nonzero(x["gt_ignore"] == 0) for x in per_a], np.int64)}
    return {"stats": e.stats, "precision": e.precision, "recall": e.recall, "groups": groups}


# ---------------------------------------------------------------------------------------------------------- scenes
def _f32(v):
    return float(np.float32(v))


def make_scene(seed, n_images=10, n_cats=6, crowded=True):
    """A seeded (dataset, results) pair.  Every scene holds: tied scores; an (image, category) group with more than 100
    detections; crowd ground truths (and annotations without an `iscrowd` key); a category without ground truth and one with
    neither ground truth nor detections; images with ground truth and no detections, and the reverse; ground-truth areas of
    exactly 1024 and 9216; the pair det [0,0,2,1] / gt [0,0,2,2] whose IoU is exactly 0.5; annotation ids, image ids and
    category ids that are neither contiguous nor in file order.  Detection boxes and scores are float32 values."""
    rng = np.random.default_rng(seed)
    image_ids = [int(v) for v in rng.choice(np.arange(3, 5000), n_images, replace=False)]
    cat_ids = [int(v) for v in rng.choice(np.arange(1, 91), n_cats, replace=False)]
    gt_cats = cat_ids[:-2]                                   # cat_ids[-2]: detections only; cat_ids[-1]: nothing at all
    no_gt_imgs, no_dt_imgs = set(image_ids[:2]), set(image_ids[2:4])
    anns, results = [], []
    next_id = [int(rng.integers(1, 50))]

    def add_gt(img, cat, bbox, area=None, crowd=None):
        a = {"id": next_id[0], "image_id": img, "category_id": cat, "bbox": [float(v) for v in bbox],
             "area": float(bbox[2] * bbox[3] if area is None else area)}
        if crowd is not None:
            a["iscrowd"] = int(crowd)
        next_id[0] += int(rng.integers(1, 4))
        anns.append(a)

    def add_dt(img, cat, bbox, score):
        results.append({"image_id": img, "category_id": cat, "bbox": [_f32(v) for v in bbox], "score": _f32(score)})

    tied = [k / 16 for k in range(1, 16)]
    for img in image_ids:
        if img in no_gt_imgs:
            continue
        for _ in range(int(rng.integers(1, 9))):
            cat = gt_cats[int(rng.integers(len(gt_cats)))]
            x, y = rng.uniform(0, 400, 2)
            w, h = rng.uniform(4, 220, 2)
            crowd = None if rng.random() < 0.3 else int(crowded and rng.random() < 0.2)
            add_gt(img, cat, [x, y, w, h], area=w * h * rng.uniform(0.4, 1.0), crowd=crowd)
            if img in no_dt_imgs:
                continue
            for _ in range(int(rng.integers(0, 4))):         # jittered copies: true positives, duplicates, near misses
                j = rng.normal(0, 0.12, 4) * [w, h, w, h]
                score = tied[int(rng.integers(len(tied)))] if rng.random() < 0.5 else rng.uniform(0.05, 1.0)
                add_dt(img, cat, [x + j[0], y + j[1], max(1.0, w + j[2]), max(1.0, h + j[3])], score)
    for img in image_ids:                                    # clutter, also on images without ground truth
        if img in no_dt_imgs:
            continue
        for _ in range(int(rng.integers(2, 12))):
            cat = cat_ids[int(rng.integers(len(cat_ids) - 1))]
            x, y = rng.uniform(0, 400, 2)
            w, h = rng.uniform(2, 200, 2)
            add_dt(img, cat, [x, y, w, h], tied[int(rng.integers(len(tied)))] if rng.random() < 0.4 else rng.uniform(0.05, 1.0))
    # fixed cases on the first image that has both
    both = [i for i in image_ids if i not in no_gt_imgs and i not in no_dt_imgs]
    img0, img1, c0, c1 = both[0], both[1], gt_cats[0], gt_cats[1]
    add_gt(img0, c0, [500, 10, 32, 32], area=1024.0, crowd=0)          # inclusive bounds: small AND medium
    add_gt(img0, c0, [500, 60, 96, 96], area=9216.0, crowd=0)          # medium AND large
    add_dt(img0, c0, [500, 10, 32, 32], 0.9)
    add_dt(img0, c0, [500, 60, 96, 96], 0.9)
    add_gt(img1, c1, [0, 0, 2, 2], crowd=0)                            # IoU with [0,0,2,1] is exactly 0.5
    add_dt(img1, c1, [0, 0, 2, 1], 0.75)
    if crowded:
        add_gt(img1, c0, [300, 300, 150, 150], crowd=1)                # a crowd absorbs several detections
        for s in (0.8, 0.8, 0.6):
            add_dt(img1, c0, [310 + 40 * s, 320, 50, 60], s)
    for n in range(130):                                               # more than maxDets[-1] in one group, many ties
        x, y = rng.uniform(0, 400, 2)
        add_dt(img0, c1, [x, y, rng.uniform(5, 150), rng.uniform(5, 150)], tied[n % len(tied)] if n % 3 else rng.uniform(0.05, 1.0))
    order = rng.permutation(len(results))
    results = [results[i] for i in order]
    anns = [anns[i] for i in rng.permutation(len(anns))]
    dataset = {"images": [{"id": i} for i in rng.permutation(image_ids).tolist()],
               "categories": [{"id": c} for c in rng.permutation(cat_ids).tolist()], "annotations": anns}
    return dataset, results
