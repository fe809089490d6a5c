#!/usr/bin/env python3
"""Detection output timing: dod_detect (postprocess.detect_packed: one launch) against the torch composite a user would write on the
packed buffer for the same result -- sigmoid, topk, gather, scale, clamp, and a greedy NMS in torch (pairwise IoU, one masked update
per candidate, stable compaction; torchvision is not a dependency), all without a host sync.
  shapes     B=64 Q=100 C=91 K=100 and B=32 Q=300 C=91 K=300, each without and with NMS (IoU 0.5, per class), sizes 480 x 640
  legs       native = postprocess.detect_packed (allocates its outputs and workspace per call, as a user calls it); native_c_call =
             dod_detect alone into preallocated buffers (what a C caller or a captured graph pays); torch_composite
  timing     hipEvent pairs around `reps` back-to-back calls (one call is tens of microseconds: a single pair would time the events),
             native and composite samples alternating in one process, warm-up first; median / p10 / p90 of the per-call time
  agreement  reported per leg: equal counts, the share of identical (query, label) rows (asserted >= 0.99), the largest box and
             score difference on those rows
One JSON line on stdout.
    python tools/bench_detect.py [--steps 30] [--warmup 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dinov2_od_amd import _native as nat, synth  # noqa: E402
from dinov2_od_amd.postprocess import detect_packed  # noqa: E402

SHAPES = [(64, 100, 91, 100), (32, 300, 91, 300)]
HW = (480.0, 640.0)
IOU = 0.5


def make_det(B, Q, C, seed=0):
    logits = synth.normal(seed, f"bench_detect.{B}.{Q}.{C}", (B, Q, C), 1.5, -4.0)
    u = synth.uniform01(seed + 1, f"bench_detect.boxes.{B}.{Q}", (B, Q, 4)).astype(np.float32)
    boxes = np.concatenate([u[..., :2], np.float32(0.02) + np.float32(0.38) * u[..., 2:]], -1)
    return torch.from_numpy(np.concatenate([logits, boxes], -1).astype(np.float32)).cuda()


def torch_detect(det, C, K, hw, iou=None):
    """the composite: (scores, labels, boxes, queries, counts) with detect_packed's meaning (background skipped, clamp on)"""
    B = det.shape[0]
    scores = torch.sigmoid(det[..., 1:C]).reshape(B, -1)
    top, idx = torch.topk(scores, K, dim=1)
    q, lab = idx // (C - 1), idx % (C - 1) + 1
    bx = torch.gather(det[..., C:], 1, q[..., None].expand(-1, -1, 4))
    cx, cy, w, h = bx.unbind(-1)
    scale = torch.tensor([hw[1], hw[0], hw[1], hw[0]], dtype=torch.float32, device=det.device)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1) * scale
    xyxy = torch.minimum(xyxy.clamp_min(0.0), scale)
    counts = torch.full((B,), K, dtype=torch.int32, device=det.device)
    if iou is None:
        return top, lab.int(), xyxy, q.int(), counts
    x1, y1, x2, y2 = xyxy.unbind(-1)
    area = (x2 - x1).clamp_min(0) * (y2 - y1).clamp_min(0)
    iw = (torch.minimum(x2[:, :, None], x2[:, None, :]) - torch.maximum(x1[:, :, None], x1[:, None, :])).clamp_min(0)
    ih = (torch.minimum(y2[:, :, None], y2[:, None, :]) - torch.maximum(y1[:, :, None], y1[:, None, :])).clamp_min(0)
    inter = iw * ih
    sup = (inter > iou * ((area[:, :, None] + area[:, None, :]) - inter)) & (lab[:, :, None] == lab[:, None, :])
    sup &= torch.ones(K, K, dtype=torch.bool, device=det.device).triu(1)
    removed = torch.zeros(B, K, dtype=torch.bool, device=det.device)
    for i in range(K):                                        # greedy: a surviving i removes what it suppresses
        removed |= sup[:, i] & ~removed[:, i:i + 1]
    order = torch.argsort(removed.to(torch.uint8), dim=1, stable=True)      # survivors first, in order
    counts = (~removed).sum(1).int()
    pad = torch.arange(K, device=det.device)[None, :] >= counts[:, None]
    g = lambda t: torch.gather(t, 1, order)
    top, lab, q = g(top).masked_fill(pad, 0.0), g(lab).masked_fill(pad, -1), g(q).masked_fill(pad, -1)
    xyxy = torch.gather(xyxy, 1, order[..., None].expand(-1, -1, 4)).masked_fill(pad[..., None], 0.0)
    return top, lab.int(), xyxy, q.int(), counts


def c_call(det, C, K, hw, iou):
    """dod_detect into buffers allocated once"""
    L = nat.lib()
    B, Q, _ = det.shape
    dev = det.device
    sc, bx = torch.empty(B, K, device=dev), torch.empty(B, K, 4, device=dev)
    lb, qs, ct = (torch.empty(n, dtype=torch.int32, device=dev) for n in ((B, K), (B, K), (B,)))
    st = torch.tensor([hw] * B, dtype=torch.float32, device=dev)
    ws = torch.empty(L.dod_detect_workspace_bytes(B, Q, C, K), dtype=torch.uint8, device=dev)
    keep = (sc, bx, lb, qs, ct, st, ws)

    def call():
        nat.check(L.dod_detect(nat.ptr(det), B, Q, C, 1, nat.ptr(st), -1.0, K, -1.0 if iou is None else iou, 0, 1, nat.ptr(sc), nat.ptr(lb),
                               nat.ptr(qs), nat.ptr(bx), nat.ptr(ct), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return keep
    return call


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_detect needs a GPU"
    out = {"tool": "bench_detect", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "sizes": HW, "nms_iou": IOU}
    for B, Q, C, K in SHAPES:
        det = make_det(B, Q, C)
        for iou in (None, IOU):
            native = lambda: detect_packed(det, C, HW, top_k=K, nms_iou=iou)
            comp = lambda: torch_detect(det, C, K, HW, iou)
            raw = c_call(det, C, K, HW, iou)
            r, t = native(), comp()
            torch.cuda.synchronize()
            rows = (r.queries == t[3]) & (r.labels == t[1])
            agree = {"counts_equal": bool(torch.equal(r.counts, t[4])), "rows_equal": round(float(rows.float().mean()), 5),
                     "max_box_diff": float((r.boxes - t[2])[rows].abs().max()), "max_score_diff": float((r.scores - t[0])[rows].abs().max()),
                     "kept_per_image": round(float(r.counts.float().mean()), 1)}
            assert agree["rows_equal"] >= 0.99, agree          # an exact tie among the top logits may be ordered differently by torch.topk
            reps_n, reps_t = 50, (2 if iou is not None else 20)
            for _ in range(a.warmup):
                _time(native, reps_n), _time(raw, reps_n), _time(comp, reps_t)
            tn, tr, tt = [], [], []
            for _ in range(a.steps):                          # alternating: every side sees the same machine
                tn.append(_time(native, reps_n))
                tr.append(_time(raw, reps_n))
                tt.append(_time(comp, reps_t))
            leg = {"native": _stats(tn, reps_n), "native_c_call": _stats(tr, reps_n), "torch_composite": _stats(tt, reps_t), "agreement": agree}
            leg["speedup_median"] = round(leg["torch_composite"]["median_ms"] / leg["native"]["median_ms"], 1)
            out[f"B{B}_Q{Q}_C{C}_K{K}_{'nms' if iou is not None else 'topk'}"] = leg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
