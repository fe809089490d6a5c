#!/usr/bin/env python3
"""Drawing timing: dod_draw_detections (visualize.draw_detections: one launch, no host sync) against what a user does without it -- copy
the batch and the boxes to the host and draw with Pillow's ImageDraw in a Python loop on one core.
  scenes     B=64 518x518 with 100 predictions per image, and B=16 224x224 with 100 predictions + 20 ground-truth boxes; each plain
             (outline 2, no fill, no captions) and full (fill alpha 64, captions at scale 1 with class names and scores)
  legs       native = visualize.draw_detections (allocates its output and pads nothing: tensors in, tensor out); native_c_call =
             dod_draw_detections alone into a preallocated output; host_pillow = D2H copy of images, boxes, labels, scores and counts
             + ImageDraw.rectangle (and ImageDraw.text with Pillow's built-in font for the full style), the result left on the host
  timing     hipEvent pairs around `reps` back-to-back native calls, wall clock around the host leg (it synchronises by its copies),
             samples alternating in one process, warm-up first; median / p10 / p90 per call
  bandwidth  achieved GB/s of the C call against its 2 * B * H * W * 3 algorithmic bytes (reported, not gated)
  agreement  the plain style's outlines are compared: the share of bytes equal between the native output and the Pillow drawing
One JSON line on stdout.
    python tools/bench_draw.py [--steps 10] [--warmup 2]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

from dinov2_od_amd import _native as nat, synth, visualize as V  # noqa: E402
from dinov2_od_amd.postprocess import Detections  # noqa: E402

SCENES = [(64, 518, 518, 100, 0), (16, 224, 224, 100, 20)]
STYLES = {"plain": dict(thickness=2, fill_alpha=0, font_scale=0), "full": dict(thickness=2, fill_alpha=64, font_scale=1)}
NAMES = [f"class{i}" for i in range(91)]


def make_scene(B, H, W, K, G, seed=0):
    img = torch.from_numpy((synth.uniform01(seed, f"bench_draw.{B}.{H}", (B, H, W, 3)) * 256).astype(np.uint8)).cuda()
    u = synth.uniform01(seed + 1, f"bench_draw.boxes.{B}.{K}", (B, K, 4)).astype(np.float32)
    cx, cy, w, h = u[..., 0] * W, u[..., 1] * H, (0.05 + 0.3 * u[..., 2]) * W, (0.05 + 0.3 * u[..., 3]) * H
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
    labels = (synth.uniform01(seed + 2, f"bench_draw.labels.{B}.{K}", (B, K)) * 90).astype(np.int32) + 1
    scores = synth.uniform01(seed + 3, f"bench_draw.scores.{B}.{K}", (B, K)).astype(np.float32) * 0.9 + 0.1
    det = Detections(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(boxes).cuda(),
                     torch.zeros(B, K, dtype=torch.int32, device="cuda"), torch.full((B,), K, dtype=torch.int32, device="cuda"))
    tg = None
    if G:
        g = synth.uniform01(seed + 4, f"bench_draw.gt.{B}.{G}", (B, G, 4)).astype(np.float32)
        g[..., 2:] = 0.05 + 0.4 * g[..., 2:]
        tg = {"boxes": torch.from_numpy(g).cuda(), "labels": torch.from_numpy((g[..., 0] * 90).astype(np.int32) + 1).cuda(),
              "counts": torch.full((B,), G, dtype=torch.int32, device="cuda")}
    return img, det, tg


def host_pillow(img, det, tg, style):
    """the user's path today: everything to the host, one ImageDraw per image"""
    x = img.cpu().numpy()
    boxes, labels, scores, counts = det.boxes.cpu().numpy(), det.labels.cpu().numpy(), det.scores.cpu().numpy(), det.counts.cpu().numpy()
    gt = None if tg is None else (tg["boxes"].cpu().numpy(), tg["labels"].cpu().numpy(), tg["counts"].cpu().numpy())
    font = ImageFont.load_default()
    t, a, cap = style["thickness"], style["fill_alpha"], style["font_scale"] > 0
    out = []
    B, H, W, _ = x.shape
    for b in range(B):
        im = Image.fromarray(x[b], "RGB")
        d = ImageDraw.Draw(im, "RGBA")
        if gt is not None:
            for i in range(int(gt[2][b]) - 1, -1, -1):
                cx, cy, w, h = gt[0][b, i]
                r = [int(np.floor((cx - w / 2) * W)), int(np.floor((cy - h / 2) * H)), int(np.ceil((cx + w / 2) * W)) - 1, int(np.ceil((cy + h / 2) * H)) - 1]
                d.rectangle(r, outline=(255, 255, 255, 255), width=t)
                if cap:
                    d.text((r[0], r[1] - 10), NAMES[gt[1][b, i]], fill=(0, 0, 0, 255), font=font)
        for i in range(int(counts[b]) - 1, -1, -1):
            x1, y1, x2, y2 = boxes[b, i]
            c = V.PALETTE[labels[b, i] % len(V.PALETTE)]
            r = [int(np.floor(x1)), int(np.floor(y1)), int(np.ceil(x2)) - 1, int(np.ceil(y2)) - 1]
            if a:
                d.rectangle(r, fill=c + (a,))
            d.rectangle(r, outline=c + (255,), width=t)
            if cap:
                d.text((r[0], r[1] - 10), f"{NAMES[labels[b, i]]} {int(scores[b, i] * 100 + 0.5)}%", fill=(0, 0, 0, 255), font=font)
        out.append(np.asarray(im))
    return np.stack(out)


def c_call(img, det, tg, style):
    """dod_draw_detections into an output allocated once"""
    L = nat.lib()
    B, H, W, _ = img.shape
    out = torch.empty_like(img)
    above, below = nat.DodDrawLayer(), nat.DodDrawLayer()
    above.boxes, above.labels, above.scores, above.counts = (t.data_ptr() for t in (det.boxes, det.labels, det.scores, det.counts))
    above.K, above.format, above.score_threshold, above.use_palette = det.boxes.shape[1], 0, 0.0, 1
    if tg is not None:
        below.boxes, below.labels, below.counts = tg["boxes"].data_ptr(), tg["labels"].data_ptr(), tg["counts"].data_ptr()
        below.K, below.format, below.score_threshold = tg["boxes"].shape[1], 1, -1.0
        below.color[0] = below.color[1] = below.color[2] = 255
    st = nat.DodDrawStyle()
    st.thickness, st.fill_alpha, st.font_scale = style["thickness"], style["fill_alpha"], style["font_scale"]
    pal = torch.tensor(V.PALETTE, dtype=torch.uint8, device="cuda")
    font = torch.from_numpy(np.array(V.FONT_5X7)).cuda()
    names = torch.from_numpy(V.names_table(NAMES)).cuda()
    st.palette, st.palette_size, st.font, st.names, st.n_names, st.name_len = pal.data_ptr(), len(V.PALETTE), font.data_ptr(), names.data_ptr(), len(NAMES), V.NAME_LEN
    keep = (out, pal, font, names, above, below, st)

    def call():
        nat.check(L.dod_draw_detections(nat.ptr(img), 0, B, H, W, C.byref(below) if tg is not None else None, C.byref(above), C.byref(st), nat.ptr(out), nat.stream_ptr()))
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


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def _stats(ms, reps):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4),
            "samples": len(ms), "calls_per_sample": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_draw needs a GPU"
    out = {"tool": "bench_draw", "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    for B, H, W, K, G in SCENES:
        img, det, tg = make_scene(B, H, W, K, G)
        for sname, style in STYLES.items():
            native = lambda: V.draw_detections(img, det, tg, NAMES, **style)
            raw = c_call(img, det, tg, style)
            host = lambda: host_pillow(img, det, tg, style)
            leg = {}
            if sname == "plain":
                leg["bytes_equal_to_pillow"] = round(float((native().cpu().numpy() == host()).mean()), 6)
            reps = 20
            for _ in range(a.warmup):
                _time(native, reps), _time(raw, reps)
            _wall(host)
            tn, tr, th = [], [], []
            for i in range(a.steps):                          # alternating: every side sees the same machine
                tn.append(_time(native, reps))
                tr.append(_time(raw, reps))
                if i < 3:                                     # the host leg takes tens of milliseconds to seconds: three samples
                    th.append(_wall(host))
            leg.update({"native": _stats(tn, reps), "native_c_call": _stats(tr, reps), "host_pillow": _stats(th, 1)})
            leg["speedup_median"] = round(leg["host_pillow"]["median_ms"] / leg["native"]["median_ms"], 1)
            leg["c_call_gb_per_s"] = round(2.0 * B * H * W * 3 / (leg["native_c_call"]["median_ms"] * 1e-3) / 1e9, 1)
            out[f"B{B}_{H}x{W}_K{K}_G{G}_{sname}"] = leg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
