#!/usr/bin/env python3
"""Sliced-inference merge timing: dod_detect_views (slicing.detect_views_packed: one launch) against the torch composite a user would
write on the packed buffer of all views for the same result -- concatenate the views of an image, sigmoid, topk, gather, map the boxes
through their view's rectangle and mirror flag, clamp, and a greedy NMS in torch (pairwise overlap, one masked update per candidate,
stable compaction; torchvision is not a dependency), all without a host sync.
  shapes     8 images x 13 views x 100 queries x 91 classes and 1 image x 16 views x 300 queries, both at K = 300, each without and with
             NMS (0.5, intersection over the smaller box, per class); 480 x 640 sources, views from slicing.plan_views, half of them
             flagged as mirrored
  legs       native = slicing.detect_views_packed on a staged plan (allocates its outputs and workspace per call, as a user calls it);
             native_c_call = dod_detect_views alone into preallocated buffers; torch_composite
  timing     hipEvent pairs around `reps` back-to-back calls, native and composite samples alternating in one process, warm-up first;
             median / p10 / p90 of the per-call time
  agreement  per leg: equal counts, the share of identical (view, query, label) rows (asserted >= 0.99), the largest box and score
             difference on those rows
  step       what slicing costs end to end: model.detect_sliced(raw images) against preprocess_batch + model.detect of the same images
             (ViT-B/14, 224 x 224 views, 100 queries, bf16), for 8 images and for 1 image, host staging included; and for the
             single image the forward of its 13 views against the merge of them, which runs on one workgroup, i.e. one CU
  --fuse     instead of the legs above: dod_fuse_views (weighted boxes fusion, IoU 0.5, per class, "avg" scores) beside dod_detect_views
             with NMS (the settings above) on the same inputs, both as C calls into preallocated buffers, samples alternating: the
             two shapes above and the second one again at K = 1024; per scene the clusters and survivors per image and the largest
             cluster.  The fusion's chain over the candidates is serial on one wave, so its time grows with K and with the number
             of clusters a candidate is compared with.
One JSON line on stdout.
    python tools/bench_detect_views.py [--steps 30] [--warmup 5] [--fuse]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dinov2_od_amd import _native as nat, slicing, synth  # noqa: E402

HW = (480, 640)
# (images, tile (height, width), queries, classes, K): plan_views gives 1 + 3 x 4 = 13 and 1 + 3 x 5 = 16 views of a 480 x 640 image
SHAPES = [(8, (224, 224), 100, 91, 300), (1, (224, 180), 300, 91, 300)]
IOU, METRIC = 0.5, "ios"


def make_case(B, tile, Q, C, seed=0):
    plan = slicing.plan_views([HW] * B, tile, 0.2)
    plan = slicing.ViewPlan(plan.offsets, plan.rects, (np.arange(len(plan.rects)) % 2).astype(np.uint8))
    V = len(plan.rects)
    logits = synth.normal(seed, f"bench_views.{V}.{Q}.{C}", (V, Q, C), 1.5, -4.0)
    u = synth.uniform01(seed + 1, f"bench_views.boxes.{V}.{Q}", (V, Q, 4)).astype(np.float32)
    boxes = np.concatenate([u[..., :2], np.float32(0.02) + np.float32(0.38) * u[..., 2:]], -1)
    return torch.from_numpy(np.concatenate([logits, boxes], -1).astype(np.float32)).cuda(), plan


def torch_views(det, B, C, K, rects, flips, hw, iou=None, ios=True):
    """the composite: (scores, labels, boxes, queries, views, counts) with detect_views_packed's meaning (background skipped, clamp on,
    no edge margin); every image has the same number of views"""
    V, Q, _ = det.shape
    nv = V // B
    d = det.view(B, nv * Q, C + 4)                                     # the views of an image, concatenated
    scores = torch.sigmoid(d[..., 1:C]).reshape(B, -1)
    top, idx = torch.topk(scores, K, dim=1)
    r, lab = idx // (C - 1), idx % (C - 1) + 1
    vi, q = r // Q, r % Q
    bx = torch.gather(d[..., C:], 1, r[..., None].expand(-1, -1, 4))
    rc = torch.gather(rects.view(B, nv, 4).float(), 1, vi[..., None].expand(-1, -1, 4))
    fl = torch.gather(flips.view(B, nv).bool(), 1, vi)
    cx, cy, w, h = bx.unbind(-1)
    x1, y1, x2, y2 = cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h
    x1, x2 = torch.where(fl, 1.0 - x2, x1), torch.where(fl, 1.0 - x1, x2)
    xyxy = torch.stack([x1 * rc[..., 2] + rc[..., 0], y1 * rc[..., 3] + rc[..., 1], x2 * rc[..., 2] + rc[..., 0], y2 * rc[..., 3] + rc[..., 1]], -1)
    lim = torch.tensor([hw[1], hw[0], hw[1], hw[0]], dtype=torch.float32, device=det.device)
    xyxy = torch.minimum(xyxy.clamp_min(0.0), lim)
    counts = torch.full((B,), K, dtype=torch.int32, device=det.device)
    if iou is None:
        return top, lab.int(), xyxy, q.int(), vi.int(), counts
    x1, y1, x2, y2 = xyxy.unbind(-1)
    area = (x2 - x1).clamp_min(0) * (y2 - y1).clamp_min(0)
    iw = (torch.minimum(x2[:, :, None], x2[:, None, :]) - torch.maximum(x1[:, :, None], x1[:, None, :])).clamp_min(0)
    ih = (torch.minimum(y2[:, :, None], y2[:, None, :]) - torch.maximum(y1[:, :, None], y1[:, None, :])).clamp_min(0)
    inter = iw * ih
    ref = torch.minimum(area[:, :, None], area[:, None, :]) if ios else (area[:, :, None] + area[:, None, :]) - inter
    sup = (inter > iou * ref) & (lab[:, :, None] == lab[:, None, :])
    sup &= torch.ones(K, K, dtype=torch.bool, device=det.device).triu(1)
    removed = torch.zeros(B, K, dtype=torch.bool, device=det.device)
    for i in range(K):                                        # greedy: a surviving i removes what it suppresses
        removed |= sup[:, i] & ~removed[:, i:i + 1]
    order = torch.argsort(removed.to(torch.uint8), dim=1, stable=True)      # survivors first, in order
    counts = (~removed).sum(1).int()
    pad = torch.arange(K, device=det.device)[None, :] >= counts[:, None]
    g = lambda t: torch.gather(t, 1, order)
    top, lab, q, vi = g(top).masked_fill(pad, 0.0), g(lab).masked_fill(pad, -1), g(q).masked_fill(pad, -1), g(vi).masked_fill(pad, -1)
    xyxy = torch.gather(xyxy, 1, order[..., None].expand(-1, -1, 4)).masked_fill(pad[..., None], 0.0)
    return top, lab.int(), xyxy, q.int(), vi.int(), counts


def c_call(det, B, C, K, pd, st, iou):
    """dod_detect_views into buffers allocated once"""
    L = nat.lib()
    V, Q, _ = det.shape
    dev = det.device
    sc, bx = torch.empty(B, K, device=dev), torch.empty(B, K, 4, device=dev)
    lb, vs, qs, ct = (torch.empty(n, dtype=torch.int32, device=dev) for n in ((B, K), (B, K), (B, K), (B,)))
    ws = torch.empty(L.dod_detect_views_workspace_bytes(V, Q, C, K), dtype=torch.uint8, device=dev)
    keep = (sc, bx, lb, vs, qs, ct, ws)

    def call():
        nat.check(L.dod_detect_views(nat.ptr(det), B, V, Q, C, nat.ptr(pd.offsets), nat.ptr(pd.rects), nat.ptr(pd.flips), nat.ptr(st), 1, -1.0, K,
                                     -1.0 if iou is None else iou, slicing.NMS_METRICS[METRIC], 0, 1, 0.0, nat.ptr(sc), nat.ptr(lb), nat.ptr(vs),
                                     nat.ptr(qs), nat.ptr(bx), nat.ptr(ct), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return keep
    return call


def c_call_fuse(det, B, C, K, pd, st, iou, conf):
    """dod_fuse_views into buffers allocated once"""
    L = nat.lib()
    V, Q, _ = det.shape
    dev = det.device
    sc, bx = torch.empty(B, K, device=dev), torch.empty(B, K, 4, device=dev)
    lb, vs, qs, mb, ct = (torch.empty(n, dtype=torch.int32, device=dev) for n in ((B, K), (B, K), (B, K), (B, K), (B,)))
    ws = torch.empty(L.dod_fuse_views_workspace_bytes(V, Q, C, K), dtype=torch.uint8, device=dev)
    keep = (sc, bx, lb, vs, qs, ct, ws, mb)

    def call():
        nat.check(L.dod_fuse_views(nat.ptr(det), B, V, Q, C, nat.ptr(pd.offsets), nat.ptr(pd.rects), nat.ptr(pd.flips), nat.ptr(st), 1, -1.0, K, iou, 0, 1,
                                   0.0, slicing.FUSE_CONFS[conf], nat.ptr(sc), nat.ptr(lb), nat.ptr(vs), nat.ptr(qs), nat.ptr(bx), nat.ptr(mb),
                                   nat.ptr(ct), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return keep
    return call


def fuse_legs(out, steps, warmup):
    reps = 50
    for B, tile, Q, C, K in SHAPES + [SHAPES[1][:4] + (1024,)]:
        det, plan = make_case(B, tile, Q, C)
        nv = len(plan.rects) // B
        pd = slicing.plan_to_device(plan, det.device)
        st = torch.tensor([HW] * B, dtype=torch.float32, device=det.device)
        nms, fuse = c_call(det, B, C, K, pd, st, IOU), c_call_fuse(det, B, C, K, pd, st, IOU, "avg")
        rn, rf = nms(), fuse()
        torch.cuda.synchronize()
        leg = {"nms_kept_per_image": round(float(rn[5].float().mean()), 1), "clusters_per_image": round(float(rf[5].float().mean()), 1),
               "largest_cluster": int(rf[7].max()), "members_per_image": round(float(rf[7].sum()) / B, 1)}
        for _ in range(warmup):
            _time(nms, reps), _time(fuse, reps)
        tn, tf = [], []
        for _ in range(steps):                                # alternating: both sides see the same machine
            tn.append(_time(nms, reps))
            tf.append(_time(fuse, reps))
        leg["nms_c_call"], leg["fuse_c_call"] = _stats(tn, reps), _stats(tf, reps)
        leg["fuse_over_nms_median"] = round(leg["fuse_c_call"]["median_ms"] / leg["nms_c_call"]["median_ms"], 2)
        out[f"B{B}_V{nv}_Q{Q}_C{C}_K{K}_fuse"] = leg


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def _stats(ms, reps):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4),
            "samples": len(ms), "calls_per_sample": reps}


def merge_legs(out, steps, warmup):
    for B, tile, Q, C, K in SHAPES:
        det, plan = make_case(B, tile, Q, C)
        nv = len(plan.rects) // B
        pd = slicing.plan_to_device(plan, det.device)
        st = torch.tensor([HW] * B, dtype=torch.float32, device=det.device)
        for iou in (None, IOU):
            native = lambda: slicing.detect_views_packed(det, C, pd, st, top_k=K, threshold=-1.0, nms_iou=iou, nms_metric=METRIC)
            comp = lambda: torch_views(det, B, C, K, pd.rects, pd.flips, HW, iou)
            raw = c_call(det, B, C, K, pd, st, iou)
            r, t = native(), comp()
            torch.cuda.synchronize()
            rows = (r.queries == t[3]) & (r.labels == t[1]) & (r.views == t[4])
            agree = {"counts_equal": bool(torch.equal(r.counts, t[5])), "rows_equal": round(float(rows.float().mean()), 5),
                     "max_box_diff": float((r.boxes - t[2])[rows].abs().max()), "max_score_diff": float((r.scores - t[0])[rows].abs().max()),
                     "kept_per_image": round(float(r.counts.float().mean()), 1)}
            assert agree["rows_equal"] >= 0.99, agree          # an exact tie among the top logits may be ordered differently by torch.topk
            reps_n, reps_t = 50, (2 if iou is not None else 20)
            for _ in range(warmup):
                _time(native, reps_n), _time(raw, reps_n), _time(comp, reps_t)
            tn, tr, tt = [], [], []
            for _ in range(steps):                            # alternating: every side sees the same machine
                tn.append(_time(native, reps_n))
                tr.append(_time(raw, reps_n))
                tt.append(_time(comp, reps_t))
            leg = {"native": _stats(tn, reps_n), "native_c_call": _stats(tr, reps_n), "torch_composite": _stats(tt, reps_t), "agreement": agree}
            leg["speedup_median"] = round(leg["torch_composite"]["median_ms"] / leg["native"]["median_ms"], 1)
            out[f"B{B}_V{nv}_Q{Q}_C{C}_K{K}_{'nms' if iou is not None else 'topk'}"] = leg


def step_legs(out, steps, warmup):
    from dinov2_od_amd.models import DINOv2ObjectDetector
    from dinov2_od_amd.preprocess import preprocess_batch
    m = DINOv2ObjectDetector(dino_model_name="facebook/dinov2-base", pretrained=False, precision="bf16", num_queries=100)
    sd = synth.detector_state_dict(m._bb_cfg, m._dc_cfg, seed=1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    C = m._dc_cfg.num_classes
    rng = np.random.default_rng(0)
    kw = dict(top_k=300, threshold=0.05, nms_iou=IOU)
    for B in (8, 1):
        imgs = [rng.integers(0, 256, (*HW, 3), dtype=np.uint8) for _ in range(B)]
        sliced = lambda: m.detect_sliced(imgs, size=224, tile=224, overlap=0.2, nms_metric=METRIC, **kw)
        plain = lambda: m.detect(preprocess_batch(imgs, (224, 224)), sizes=HW, **kw)
        nv = int(np.diff(slicing.plan_views([HW], 224, 0.2).offsets)[0])
        for _ in range(warmup):
            _time(sliced, 3), _time(plain, 3)
        ts, tp = [], []
        for _ in range(steps):
            ts.append(_time(sliced, 3))
            tp.append(_time(plain, 3))
        leg = {"views_per_image": nv, "detect_sliced": _stats(ts, 3), "detect": _stats(tp, 3)}
        leg["cost_ratio_median"] = round(leg["detect_sliced"]["median_ms"] / leg["detect"]["median_ms"], 2)
        if B == 1:                                            # one image: the merge is one workgroup on one CU -- against the forward of its views
            plan = slicing.plan_views([HW], 224, 0.2)
            pd = slicing.plan_to_device(plan, "cuda")
            u8 = slicing.extract_views(imgs, plan, 224)
            with torch.no_grad():
                det = m.forward_packed_u8(u8).clone()
                fwd = lambda: m.forward_packed_u8(u8)
                st = torch.tensor([HW], dtype=torch.float32, device="cuda")
                raw = c_call(det, 1, C, 300, pd, st, IOU)
                for _ in range(warmup):
                    _time(fwd, 5), _time(raw, 50)
                tf, tm = [], []
                for _ in range(steps):
                    tf.append(_time(fwd, 5))
                    tm.append(_time(raw, 50))
            leg["forward_of_views"], leg["merge_c_call"] = _stats(tf, 5), _stats(tm, 50)
            leg["forward_over_merge_median"] = round(leg["forward_of_views"]["median_ms"] / leg["merge_c_call"]["median_ms"], 1)
        out[f"step_B{B}_vitb224_Q100"] = leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fuse", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_detect_views needs a GPU"
    out = {"tool": "bench_detect_views", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "sizes": HW, "nms_iou": IOU,
           "nms_metric": METRIC}
    if a.fuse:
        fuse_legs(out, a.steps, a.warmup)
    else:
        merge_legs(out, a.steps, a.warmup)
        step_legs(out, a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
