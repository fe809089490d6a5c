"""dod_draw_detections (include/dinodet.h) restated in numpy, and the seeded scenes of tests/test_draw_cpu.py and tests/test_gpu_draw.py.

The restatement follows the header to the letter: the fp32 -> byte rule and the box conversion in float32 with one rounding per
operation, everything else in integers; the pixel rectangle from floor / ceil with saturation before the conversion; rows skipped
for a NaN, an inverted or empty rectangle, a rectangle with no pixel in the image, a score at or below the threshold; the outline by
the distance to the nearest side, the fill by Pillow's div255 blend, the caption by the closed form per pixel over the one font table
(dinov2_od_amd.visualize.FONT_5X7); painter's order: layer below then above, rows count - 1 down to 0, a row's caption right after it.
"""
import numpy as np

from dinov2_od_amd import synth
from dinov2_od_amd.visualize import FONT_5X7
from tests import detect_cases as dc

F = np.float32


def to_bytes(x):
    """fp32 [B, 3, H, W] -> uint8 [B, H, W, 3]: v = x * 255; v = v + 0.5; NaN -> 0; clamp to [0, 255]; truncate"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(x, np.float32) * F(255.0)).astype(np.float32)
        v = (v + F(0.5)).astype(np.float32)
        v = np.where(np.isnan(v), F(0.0), v)
        v = np.clip(v, F(0.0), F(255.0))
    return np.ascontiguousarray(v.astype(np.int32).astype(np.uint8).transpose(0, 2, 3, 1))


def _sat_int(v):
    return int(np.clip(F(v), F(-32768.0), F(32767.0)))


def pixel_rect(box, fmt, H, W):
    """one row -> (xa, ya, xb, yb), or None when the row is skipped for its geometry"""
    b = np.asarray(box, np.float32)
    if fmt == 1:
        b = dc.boxes_of(b.reshape(1, 4), (F(H), F(W)), False)[0]
    if np.isnan(b).any():
        return None
    xa, ya = _sat_int(np.floor(b[0])), _sat_int(np.floor(b[1]))
    xb, yb = _sat_int(np.ceil(b[2])) - 1, _sat_int(np.ceil(b[3])) - 1
    if xb < xa or yb < ya or xb < 0 or yb < 0 or xa >= W or ya >= H:
        return None
    return xa, ya, xb, yb


def _decimal(m):
    return str(int(m)).encode()


def caption_text(label, score, names):
    """bytes of a caption: the class name (or the decimal label), then ' <percent>%' when the row has a score"""
    label = int(label)
    text = b""
    if names is not None and 0 <= label < len(names):
        row = bytes(names[label].tolist())
        text = row.split(b"\0")[0]
    if not text:
        text = _decimal(label)
    if score is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.floor((F(score) * F(100.0)).astype(np.float32) + F(0.5))
        p = F(0.0) if np.isnan(p) else np.clip(p, F(0.0), F(999.0))
        text += b" " + _decimal(int(p)) + b"%"
    return text


def caption_rect(xa, ya, n, s, H, W):
    cw, ch = min(6 * s * n + s, W), min(9 * s, H)
    cy0 = ya - ch if ya - ch >= 0 else ya
    cy0 = min(max(cy0, 0), H - ch)
    cx0 = min(max(xa, 0), W - cw)
    return cx0, cy0, cw, ch


def caption_bitmap(text, s, font=FONT_5X7):
    """bool [9 s, 6 s n + s]: the TEXT pixels of an uncut caption, by the header's closed form"""
    n = len(text)
    v, u = np.mgrid[0:9 * s, 0:6 * s * n + s]
    u, v = u - s, v - s
    ok = (u >= 0) & (v >= 0)
    uu, vv = np.where(ok, u, 0), np.where(ok, v, 0)
    ci, gx, gy = uu // (6 * s), (uu % (6 * s)) // s, vv // s
    ok &= (ci < n) & (gx < 5) & (gy < 7)
    codes = np.array([c - 0x20 if 0x20 <= c <= 0x7F else 95 for c in text], np.int64)
    ci, gx, gy = np.where(ok, ci, 0), np.where(ok, gx, 0), np.where(ok, gy, 0)
    bits = (font[codes[ci], gy].astype(np.int64) >> (4 - gx)) & 1
    return ok & (bits == 1)


def div255(u):
    u = u + 128
    return (u + (u >> 8)) >> 8


def layer(boxes, labels, counts=None, scores=None, fmt=0, threshold=-1.0, use_palette=False, color=(255, 255, 255)):
    boxes = np.ascontiguousarray(boxes, np.float32)
    return {"boxes": boxes, "labels": np.ascontiguousarray(labels, np.int32), "counts": None if counts is None else np.ascontiguousarray(counts, np.int32),
            "scores": None if scores is None else np.ascontiguousarray(scores, np.float32), "format": fmt, "threshold": float(threshold),
            "use_palette": bool(use_palette), "color": tuple(color)}


def style(thickness=2, fill_alpha=0, font_scale=1, palette=None, names=None):
    from dinov2_od_amd.visualize import PALETTE
    return {"thickness": thickness, "fill_alpha": fill_alpha, "font_scale": font_scale,
            "palette": np.asarray(PALETTE if palette is None else palette, np.uint8).reshape(-1, 3), "names": names}


def draw_ref(images, below, above, st, return_touched=False):
    """images: uint8 [B, H, W, 3] or fp32 [B, 3, H, W].  -> uint8 [B, H, W, 3] (and the bool mask of pixels inside any drawn rectangle or
    caption rectangle)"""
    img = to_bytes(images) if images.dtype == np.float32 else np.array(images, np.uint8)
    B, H, W, _ = img.shape
    out = img.astype(np.int64)
    touched = np.zeros((B, H, W), bool)
    t, a, s = st["thickness"], st["fill_alpha"], st["font_scale"]
    for ly in (below, above):
        if ly is None or ly["boxes"].shape[1] == 0:
            continue
        K = ly["boxes"].shape[1]
        for b in range(B):
            n = K if ly["counts"] is None else min(max(int(ly["counts"][b]), 0), K)
            for row in range(n - 1, -1, -1):
                score = None if ly["scores"] is None else ly["scores"][b, row]
                if score is not None and not ly["threshold"] < 0 and score <= F(ly["threshold"]):
                    continue
                rect = pixel_rect(ly["boxes"][b, row], ly["format"], H, W)
                if rect is None:
                    continue
                xa, ya, xb, yb = rect
                label = int(ly["labels"][b, row])
                col = st["palette"][label % len(st["palette"])].astype(np.int64) if ly["use_palette"] else np.asarray(ly["color"], np.int64)
                X0, X1, Y0, Y1 = max(xa, 0), min(xb, W - 1), max(ya, 0), min(yb, H - 1)
                ys, xs = np.mgrid[Y0:Y1 + 1, X0:X1 + 1]
                d = np.minimum(np.minimum(xs - xa, xb - xs), np.minimum(ys - ya, yb - ys))
                reg = out[b, Y0:Y1 + 1, X0:X1 + 1]
                inner = div255(reg * (255 - a) + col * a) if a > 0 else reg
                out[b, Y0:Y1 + 1, X0:X1 + 1] = np.where((d < t)[..., None], col, inner)
                touched[b, Y0:Y1 + 1, X0:X1 + 1] = True
                if s > 0:
                    text = caption_text(label, score, st["names"])
                    cx0, cy0, cw, ch = caption_rect(xa, ya, len(text), s, H, W)
                    bm = caption_bitmap(text, s)[:ch, :cw]
                    tc = 0 if 299 * col[0] + 587 * col[1] + 114 * col[2] >= 128000 else 255
                    out[b, cy0:cy0 + ch, cx0:cx0 + cw] = np.where(bm[..., None], tc, col)
                    touched[b, cy0:cy0 + ch, cx0:cx0 + cw] = True
    out = out.astype(np.uint8)
    return (out, touched) if return_touched else out


# ------------------------------------------------------------------------------------------------ scenes
NAMES = ["background", "person", "bicycle", "car", "traffic_light", "a.b:c-d_e", "Zebra 9%", "", "x" * 40, "café", "dog"]


def names_array(names=NAMES):
    from dinov2_od_amd.visualize import names_table
    return names_table(names)


def rand_images_u8(seed, B, H, W):
    return (synth.uniform01(seed, f"draw.u8.{B}.{H}.{W}", (B, H, W, 3)) * 256).astype(np.uint8)


def rand_xyxy(seed, B, K, H, W, max_side=0.5):
    """pixel boxes with fractional corners; about one in ten reaches over an image edge, every fifth has integer corners"""
    u = synth.uniform01(seed, f"draw.xyxy.{B}.{K}.{H}.{W}", (B, K, 4)).astype(np.float32)
    cx, cy = (u[..., 0] * F(1.2) - F(0.1)) * F(W), (u[..., 1] * F(1.2) - F(0.1)) * F(H)
    w, h = (F(0.04) + u[..., 2] * F(max_side)) * F(W), (F(0.04) + u[..., 3] * F(max_side)) * F(H)
    bx = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)
    bx[:, ::5] = np.round(bx[:, ::5])
    return bx


def rand_cxcywh(seed, B, G):
    u = synth.uniform01(seed, f"draw.cxcywh.{B}.{G}", (B, G, 4)).astype(np.float32)
    bx = np.empty_like(u)
    bx[..., :2] = u[..., :2] * F(1.1) - F(0.05)
    bx[..., 2:] = F(0.05) + u[..., 2:] * F(0.5)
    return bx


def rand_scene(seed, B, H, W, K, G, n_labels=30):
    """(images uint8, below = G ground-truth rows in format 1, above = K prediction rows with scores, labels and ragged counts)"""
    u = synth.uniform01(seed, f"draw.scene.{B}.{K}.{G}", (B, K + G + 2))
    pred = layer(rand_xyxy(seed + 1, B, K, H, W), (u[:, :K] * n_labels).astype(np.int32), np.maximum(1, (u[:, K + G] * (K + 1)).astype(np.int32)),
                 synth.uniform01(seed + 2, f"draw.scores.{B}.{K}", (B, K)), 0, 0.2, True)
    gt = layer(rand_cxcywh(seed + 3, B, G), (u[:, K:K + G] * n_labels).astype(np.int32), np.maximum(1, (u[:, K + G + 1] * (G + 1)).astype(np.int32)),
               None, 1, -1.0, False, (255, 255, 255))
    return rand_images_u8(seed, B, H, W), gt, pred


def fp32_edges(seed, H, W):
    """fp32 [1, 3, H, W] in [0, 1) with the special values scattered in: 0, 1, k/255 - 0.5/255 one ulp either side (the rounding edges of
    the byte rule), NaN, -1, 2, +-inf"""
    x = synth.uniform01(seed, f"draw.f32.{H}.{W}", (1, 3, H, W)).astype(np.float32).reshape(-1)
    pick = synth.uniform01(seed + 1, f"draw.f32.pick.{H}.{W}", x.shape)
    k = (synth.uniform01(seed + 2, f"draw.f32.k.{H}.{W}", x.shape) * 255).astype(np.int32) + 1
    edge = ((k.astype(np.float64) - 0.5) / 255.0).astype(np.float32)
    x = np.where(pick < 0.1, np.nextafter(edge, F(0)), x)
    x = np.where((pick >= 0.1) & (pick < 0.2), np.nextafter(edge, F(2)), x)
    x = np.where((pick >= 0.2) & (pick < 0.3), edge, x)
    for i, v in enumerate([0.0, 1.0, np.nan, -1.0, 2.0, np.inf, -np.inf, -0.0]):
        x = np.where((pick >= 0.3 + 0.02 * i) & (pick < 0.32 + 0.02 * i), F(v), x)
    return x.astype(np.float32).reshape(1, 3, H, W)
