"""Shared cases and oracles of the train-time augmentation tests (tests/test_augment_cpu.py, tests/test_gpu_augment.py).

Two oracles of the image chain  crop -> brightness -> contrast -> saturation -> resize(BILINEAR) -> horizontal flip:
  * `pillow_chain`: Pillow itself (Image.crop, ImageEnhance.{Brightness, Contrast, Color}, Image.resize, Image.transpose);
  * `restated_chain`: numpy.  Each enhancer is Image.blend(degenerate, img, f): per byte v = d + f * (p - d) in float32, product and
    sum rounded separately; (uint8) truncation for 0 <= f <= 1, else clipped to [0, 255] first.  Degenerates: 0; the integer mean
    (int)(sum L / count + 0.5) of the crop's luma L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 after the brightness step; the
    pixel's own L after both.  Then oracle.preprocess_oracle.resize_bilinear_u8, the flip, to_tensor.
The CPU test pins the second against the first over CASES, which licenses it as the GPU test's second oracle.
`targets_f64` evaluates the target transform in float64.
"""
import functools

import numpy as np

from oracle import preprocess_oracle as ppo

FACTORS = (0.0, 0.37, 0.999, 1.0, 1.0001, 1.9)      # truncation branch, identity, clip branch


def luma(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def blend_u8(d, p, f):
    """Image.blend(d, p, f) on uint8 arrays (d may be a scalar)"""
    f = np.float32(f)
    d = np.asarray(d).astype(np.int32)
    diff = (p.astype(np.int32) - d).astype(np.float32)
    v = d.astype(np.float32) + f * diff
    assert v.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return v.astype(np.uint8)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.uint8)


def jitter_u8(img, factors):
    """brightness -> contrast -> saturation on a uint8 [H, W, 3] image"""
    bf, cf, sf = (np.float32(f) for f in factors)
    img = blend_u8(0, img, bf)
    L = luma(img)
    m = int(float(L.sum()) / L.size + 0.5)
    img = blend_u8(m, img, cf)
    return blend_u8(luma(img)[..., None].astype(np.uint8), img, sf)


def restated_chain(img, crop, flip, factors, out_h, out_w):
    """uint8 [out_h, out_w, 3]"""
    l, t, w, h = (int(v) for v in crop)
    im = np.ascontiguousarray(img[t:t + h, l:l + w])
    if factors is not None:
        im = jitter_u8(im, factors)
    im = ppo.resize_bilinear_u8(im, out_h, out_w)
    return np.ascontiguousarray(im[:, ::-1]) if flip else im


def pillow_chain(img, crop, flip, factors, out_h, out_w):
    """uint8 [out_h, out_w, 3], by Pillow"""
    from PIL import Image, ImageEnhance
    l, t, w, h = (int(v) for v in crop)
    im = Image.fromarray(img).crop((l, t, l + w, t + h))
    if factors is not None:
        for enh, f in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), factors):
            im = enh(im).enhance(float(np.float32(f)))
    im = im.resize((out_w, out_h), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.array(im)


# ------------------------------------------------------------------------------------------------------------------ image cases
def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(shape[0], shape[1], 3), dtype=np.uint8)


def _hard(shape):
    """the 0 / 255 column pattern of tests/test_gpu_preprocess.py: rounding and clipping"""
    im = np.zeros((shape[0], shape[1], 3), dtype=np.uint8)
    im[:, ::2] = 255
    return im


def _flat(shape, rgb):
    return np.broadcast_to(np.array(rgb, dtype=np.uint8), (shape[0], shape[1], 3)).copy()


def _case(images, crops, flips, jitter, size):
    B = len(images)
    assert len(crops) == B and len(flips) == B and (jitter is None or len(jitter) == B)
    return dict(images=images, crops=np.array(crops, dtype=np.int32), flips=np.array(flips, dtype=np.uint8),
                jitter=None if jitter is None else np.array(jitter, dtype=np.float32), size=size)


def _edges():
    # (H, W) = (40, 50): boxes touching the right, bottom, left and top edge, a 1-pixel-wide and a 1-pixel-high crop
    imgs = [_rand((40, 50), 10 + i) for i in range(6)]
    crops = [(10, 5, 40, 20), (4, 15, 30, 25), (0, 3, 33, 21), (7, 0, 21, 33), (7, 3, 1, 20), (3, 7, 20, 1)]
    return _case(imgs, crops, [0, 1, 1, 0, 1, 0], None, (56, 56))


def _upscale():
    # a 20 x 15 crop -> 56 x 42
    return _case([_rand((30, 40), 20), _hard((30, 40))], [(11, 9, 20, 15), (3, 2, 20, 15)], [1, 0], [(1.0, 1.0, 1.0), (0.8, 1.3, 0.5)], (42, 56))


def _downscale():
    # a 600 x 800 crop -> 42 x 56: 14.3x, 31 of the 32 taps
    return _case([_rand((820, 640), 21)], [(23, 11, 600, 800)], [1], [(1.1, 0.9, 1.2)], (56, 42))


def _two_blocks():
    # out_w = 300: a flipped row spans two 256-column blocks
    return _case([_rand((30, 400), 22), _rand((25, 310), 23)], [(50, 5, 330, 20), (0, 0, 310, 25)], [1, 0],
                 [(1.2, 1.0, 1.0), (1.0, 1.0, 0.3)], (20, 300))


def _all_differ():
    shapes = [(61, 47), (33, 90), (50, 50), (77, 31), (20, 120)]
    crops = [(3, 9, 40, 50), (10, 0, 71, 33), (0, 0, 50, 50), (1, 30, 29, 40), (60, 2, 55, 17)]
    jitter = [(0.6, 1.4, 0.0), (1.9, 0.37, 1.0001), (1.0, 1.0, 1.0), (0.999, 1.0001, 1.9), (0.0, 1.23, 0.6)]
    return _case([_rand(s, 30 + i) for i, s in enumerate(shapes)], crops, [1, 0, 1, 0, 1], jitter, (56, 56))


def _largest_image_smallest_crop():
    # the grid is bounded by the largest crop (the small image's), not by the largest image
    return _case([_rand((200, 300), 40), _rand((40, 50), 41)], [(5, 5, 10, 12), (0, 0, 50, 40)], [0, 1],
                 [(1.3, 0.7, 1.1), (1.0, 1.0, 1.0)], (56, 56))


def _factors():
    # every factor alone in every enhancer, on random bytes, then chained; the hard-edged image under the clip branch
    imgs, crops, flips, jit = [], [], [], []
    for k in range(3):
        for i, f in enumerate(FACTORS):
            fs = [1.0, 1.0, 1.0]
            fs[k] = f
            imgs.append(_rand((24, 31), 50 + 6 * k + i)); crops.append((2, 1, 27, 22)); flips.append((k + i) & 1); jit.append(tuple(fs))
    for i, fs in enumerate([(0.37, 0.999, 0.0), (1.0001, 1.9, 1.0001), (1.9, 0.0, 1.9), (0.999, 1.0001, 0.37)]):
        imgs.append(_rand((24, 31), 80 + i)); crops.append((0, 0, 31, 24)); flips.append(i & 1); jit.append(fs)
    imgs.append(_hard((24, 31))); crops.append((1, 1, 29, 22)); flips.append(1); jit.append((1.9, 1.9, 1.9))
    return _case(imgs, crops, flips, jit, (56, 56))


def _flat_contrast():
    # a flat grey image under contrast: the mean is the pixel and nothing changes; next to it one under all three, and a flat
    # coloured one, whose mean is its luma
    return _case([_flat((30, 30), (137, 137, 137)), _flat((30, 30), (17, 17, 17)), _flat((30, 30), (200, 100, 50))],
                 [(2, 3, 20, 25), (0, 0, 30, 30), (1, 1, 28, 28)], [0, 1, 0], [(1.0, 1.9, 1.0), (1.4, 0.37, 1.9), (1.0, 1.9, 1.0)], (56, 56))


def _one_contrast():
    # a contrast factor != 1 on one image only
    return _case([_rand((35, 45), 90 + i) for i in range(3)], [(5, 5, 30, 25), (0, 0, 45, 35), (9, 1, 36, 30)], [0, 0, 1],
                 [(1.0, 1.0, 1.0), (1.0, 0.6, 1.0), (1.0, 1.0, 1.0)], (56, 56))


CASES = {"edges": _edges, "upscale": _upscale, "downscale": _downscale, "two_blocks": _two_blocks, "all_differ": _all_differ,
         "largest_image_smallest_crop": _largest_image_smallest_crop, "factors": _factors, "flat_contrast": _flat_contrast,
         "one_contrast": _one_contrast}


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and the restated chain's uint8 [B, out_h, out_w, 3] result, computed once (read-only)"""
    c = CASES[name]()
    want = np.stack([restated_chain(im, c["crops"][b], c["flips"][b], None if c["jitter"] is None else c["jitter"][b], *c["size"])
                     for b, im in enumerate(c["images"])])
    want.setflags(write=False)
    return c, want


# ---------------------------------------------------------------------------------------------------------------- target cases
def targets_f64(boxes, shape, crop, flip, min_visibility=0.0):
    """the target transform in float64: (keep mask [n], new cxcywh boxes of the kept [k, 4], margins [n, 3]): the distance of each
    box's clipped width and height fractions from 0.001 and of its visible-area ratio from min_visibility"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    H, W = shape
    l, t, cw, ch = (float(v) for v in crop)
    cx, cy, bw, bh = b.T
    x1 = np.clip((cx - 0.5 * bw) * W - l, 0, cw); x2 = np.clip((cx + 0.5 * bw) * W - l, 0, cw)
    y1 = np.clip((cy - 0.5 * bh) * H - t, 0, ch); y2 = np.clip((cy + 0.5 * bh) * H - t, 0, ch)
    fw, fh = (x2 - x1) / cw, (y2 - y1) / ch
    vis = (x2 - x1) * (y2 - y1) / ((bw * W) * (bh * H))
    keep = (x2 > x1) & (y2 > y1) & (fw >= 0.001) & (fh >= 0.001) & (vis >= min_visibility)
    if flip:
        x1, x2 = cw - x2, cw - x1
    out = np.stack([(x1 + x2) / (2 * cw), (y1 + y2) / (2 * ch), (x2 - x1) / cw, (y2 - y1) / ch], axis=1)
    margins = np.stack([np.abs(fw - 0.001), np.abs(fh - 0.001), np.abs(vis - min_visibility) if min_visibility > 0 else np.ones_like(vis)], axis=1)
    return keep, out[keep], margins


def random_boxes(n, seed, shape, crop, min_visibility, margin=1e-4):
    """n normalised cxcywh boxes (float32 values), some outside the crop, some straddling it; none within `margin` of a keep threshold"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        cxcy = rng.uniform(0.0, 1.0, 2)
        wh = rng.uniform(0.002, 0.6, 2)
        b = np.concatenate([cxcy, wh]).astype(np.float32)
        if b[0] - b[2] / 2 < 0 or b[0] + b[2] / 2 > 1 or b[1] - b[3] / 2 < 0 or b[1] + b[3] / 2 > 1:
            continue
        if (targets_f64(b[None], shape, crop, False, min_visibility)[2] >= margin).all():
            out.append(b)
    return np.stack(out)
