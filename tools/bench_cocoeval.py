#!/usr/bin/env python3
"""COCO evaluation timing on a synthetic COCO-val-sized scene: 5 000 images, 80 categories, ~37 k ground truths, 100 queries per
image thresholded at 0.05 (the records dod_postprocess would emit, built here in numpy so that the host legs need no GPU).
  device     COCOEvaluator.evaluate() on the whole scene: hipEvent pairs around the call (it includes its two host round trips),
             warm-up first, median / p10 / p90 over --steps
  dicts      the path it replaces in front of pycocotools: records -> one Python dict per detection -> json dump -> json load
  restate    tests/cocoeval_ref.py (pycocotools' loops in numpy, the yardstick) on the first --ref-images images, and the device
             on the same subset, whose precision / recall must equal the restatement's bit for bit (--ref-images 0 skips it)
  --detections  instead of the legs above: COCOEvaluator.add_detections of a detect() result of 64 x 300 rows (hipEvent pairs, the
             evaluator reset outside them) against the host route detections_to_list -> one dict per row -> add_records (wall clock,
             once); and confusion_matrix(0.25, 0.5) on the whole scene, with the numpy restatement of tests/eval_detections_cases.py
             on the first --ref-images images, which the device must equal cell for cell
One JSON line on stdout.
    python tools/bench_cocoeval.py [--steps 10] [--warmup 2] [--images 5000] [--ref-images 250] [--host-only] [--detections]
--host-only: the dicts and restate legs without a GPU."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from dinov2_od_amd.postprocess import RECORD_DTYPE, records_to_coco  # noqa: E402
from tests import cocoeval_ref as ref  # noqa: E402


def make_scene(n_images, n_cats=80, Q=100, gt_per_image=7.4, thr=0.05, seed=0):
    """(dataset dict, RECORD_DTYPE records in evaluate_coco's order: image, class, query)"""
    rng = np.random.default_rng(seed)
    C = n_cats + 1
    image_ids = np.sort(rng.choice(np.arange(1, 600000), n_images, replace=False))
    recs, anns = [], []
    for b0 in range(0, n_images, 250):                       # in slabs: the logits of 5 000 images are 160 MB
        B = min(250, n_images - b0)
        logits = rng.normal(-5.0, 1.2, (B, Q, C)).astype(np.float32)
        cxcy, wh = rng.uniform(0.15, 0.85, (B, Q, 2)), np.exp(rng.uniform(np.log(0.01), np.log(0.6), (B, Q, 2)))
        box = np.concatenate([cxcy - wh / 2, wh], -1).astype(np.float32) * np.float32(640)      # pixel xywh: all three area ranges occur
        for b in range(B):
            for q in rng.choice(Q, min(Q, rng.poisson(gt_per_image)), replace=False):
                c = int(rng.integers(1, C))
                logits[b, q, c] = rng.normal(1.0, 1.5)                                   # a confident detection of this object
                x, y, w, h = (float(v) for v in box[b, q] * rng.uniform(0.92, 1.08, 4))
                anns.append({"id": len(anns) + 1, "image_id": int(image_ids[b0 + b]), "category_id": c, "bbox": [x, y, w, h],
                             "area": w * h * float(rng.uniform(0.5, 1.0)), "iscrowd": int(rng.random() < 0.02)})
        score = (1.0 / (1.0 + np.exp(-logits))).astype(np.float32)
        bi, ci, qi = np.nonzero(score.transpose(0, 2, 1)[:, 1:, :] > np.float32(thr))   # image-major, class 1..C-1, query
        r = np.zeros(bi.size, RECORD_DTYPE)
        r["image_id"], r["category_id"], r["query"] = image_ids[b0 + bi], ci + 1, qi
        r["bbox"], r["score"] = box[bi, qi], score[bi, qi, ci + 1]
        recs.append(r)
    ds = {"images": [{"id": int(i)} for i in image_ids], "categories": [{"id": c} for c in range(1, C)], "annotations": anns}
    return ds, np.concatenate(recs)


def _subset(ds, rec, n):
    ids = {im["id"] for im in ds["images"][:n]}
    keep = np.isin(rec["image_id"], np.fromiter(ids, np.int64))
    return {"images": ds["images"][:n], "categories": ds["categories"], "annotations": [a for a in ds["annotations"] if a["image_id"] in ids]}, rec[keep]


def _stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 3), "p10_ms": round(float(np.percentile(a, 10)), 3), "p90_ms": round(float(np.percentile(a, 90)), 3),
            "steps": len(ms)}


def _device_evaluate(ds, rec, steps, warmup):
    import torch
    from dinov2_od_amd import cocoeval as ce
    ev = ce.COCOEvaluator(ds, max_detections=max(1, rec.size))
    t0 = time.perf_counter()
    ev.add_records(rec)
    upload = time.perf_counter() - t0
    for _ in range(warmup):
        out = ev.evaluate()
    ms = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = ev.evaluate()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return out, dict(_stats(ms), upload_records_s=round(upload, 4), workspace_mb=round(ev._ws.numel() / 2 ** 20, 1))


def _timed(fn, steps, warmup, before=None):
    """hipEvent pairs around fn() after a warm-up; before() runs outside the timed region"""
    import torch
    ms = []
    for i in range(warmup + steps):
        if before is not None:
            before()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(e))
    return _stats(ms)


def _detections_leg(ds, rec, steps, warmup, ref_images, B=64, Kd=300):
    """add_detections of a [B, Kd] detect() result against detections_to_list -> dicts -> add_records, and confusion_matrix on the
    whole scene against the numpy restatement (tests/eval_detections_cases.py) on the first ref_images images, which must agree"""
    import torch
    from dinov2_od_amd import cocoeval as ce
    from dinov2_od_amd.postprocess import Detections, detections_to_list
    from tests import eval_detections_cases as edc
    rng = np.random.default_rng(1)
    ids = [im["id"] for im in ds["images"][:B]]
    xy, wh = rng.uniform(0, 500, (B, Kd, 2)), rng.uniform(4, 140, (B, Kd, 2))
    res = Detections(torch.from_numpy(rng.uniform(0.05, 1, (B, Kd)).astype(np.float32)).cuda(), torch.from_numpy(rng.integers(0, 80, (B, Kd)).astype(np.int32)).cuda(),
                     torch.from_numpy(np.concatenate([xy, xy + wh], -1).astype(np.float32)).cuda(), torch.full((B, Kd), -1, dtype=torch.int32).cuda(),
                     torch.full((B,), Kd, dtype=torch.int32).cuda())
    table = list(range(1, 81))
    ev = ce.COCOEvaluator(ds, max_detections=B * Kd)
    leg = {"rows": B * Kd, "add_detections": _timed(lambda: ev.add_detections(res, ids, table), steps, warmup, before=ev.reset)}

    def host_route():
        records = []
        for i, one in zip(ids, detections_to_list(res)):
            for box, score, label in zip(one["boxes"].cpu().numpy().tolist(), one["scores"].cpu().numpy().tolist(), one["labels"].cpu().numpy().tolist()):
                records.append({"image_id": i, "category_id": table[label], "bbox": [box[0], box[1], box[2] - box[0], box[3] - box[1]], "score": score})
        ev.add_records(records)
    ev.reset()
    t0 = time.perf_counter()
    host_route()
    torch.cuda.synchronize()
    leg["list_dicts_add_records_s"] = round(time.perf_counter() - t0, 4)
    full = ce.COCOEvaluator(ds, max_detections=max(1, rec.size))
    full.add_records(rec)
    leg["confusion_matrix"] = dict(_timed(lambda: full.confusion_matrix(0.25, 0.5), steps, warmup), detections=int(rec.size),
                                   max_gt_per_image=full.max_gt_per_image)
    if ref_images > 0:
        sds, srec = _subset(ds, rec, ref_images)
        sd = records_to_coco(srec)
        t0 = time.perf_counter()
        want = edc.confusion_ref(sds, sd, 0.25, 0.5)
        leg["restatement"] = {"images": ref_images, "detections": int(srec.size), "confusion_ref_s": round(time.perf_counter() - t0, 2)}
        sub = ce.COCOEvaluator(sds, max_detections=max(1, srec.size))
        sub.add_records(srec)
        leg["restatement"]["confusion_matrix"] = _timed(lambda: sub.confusion_matrix(0.25, 0.5), steps, warmup)
        same = bool(np.array_equal(sub.confusion_matrix(0.25, 0.5), want))
        leg["restatement"]["equal"] = same
        assert same, leg
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--ref-images", type=int, default=250)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--detections", action="store_true")
    a = ap.parse_args()
    t0 = time.perf_counter()
    ds, rec = make_scene(a.images)
    out = {"tool": "bench_cocoeval", "images": a.images, "categories": 80, "ground_truths": len(ds["annotations"]), "detections": int(rec.size),
           "scene_build_s": round(time.perf_counter() - t0, 2), "host_only": a.host_only}
    if a.detections:                                          # this leg alone: the evaluate legs are the default run's
        if a.host_only:
            raise SystemExit("--detections times device calls: it cannot run --host-only")
        import torch
        out["device"] = torch.cuda.get_device_name(0)
        out["detections_leg"] = _detections_leg(ds, rec, a.steps, a.warmup, a.ref_images)
        print(json.dumps(out))
        return
    if not a.host_only:
        import torch
        out["device"] = torch.cuda.get_device_name(0)
        res, out["device_evaluate"] = _device_evaluate(ds, rec, a.steps, a.warmup)
        out["stats"] = [round(v, 6) for v in res["stats"]]
    t0 = time.perf_counter()
    dicts = records_to_coco(rec)
    t1 = time.perf_counter()
    json.loads(json.dumps(dicts))
    out["dicts"] = {"records_to_coco_s": round(t1 - t0, 3), "json_dump_load_s": round(time.perf_counter() - t1, 3)}
    del dicts
    if a.ref_images > 0:
        sds, srec = _subset(ds, rec, a.ref_images)
        sd = records_to_coco(srec)
        t0 = time.perf_counter()
        want = ref.evaluate(sds, sd)
        leg = {"images": a.ref_images, "detections": int(srec.size), "restatement_s": round(time.perf_counter() - t0, 2)}
        if not a.host_only:
            got, leg["device_evaluate"] = _device_evaluate(sds, srec, a.steps, a.warmup)
            same = all(np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)) for k in ("precision", "recall"))
            leg["max_stats_diff"] = float(np.abs(np.array(got["stats"]) - np.array(want["stats"])).max())
            leg["precision_recall_bit_identical"] = bool(same)
            assert same and leg["max_stats_diff"] <= 1e-10, leg
        out["restate"] = leg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
