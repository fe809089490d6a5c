"""Shared cases and oracles of the composed-canvas tests (tests/test_compose_cpu.py, tests/test_gpu_compose.py): a canvas of a fill
colour with disjoint pieces pasted into it, each piece the chain of tests/augment_cases.py at its own output size.

Two oracles, both built on augment_cases:
  * `pillow_compose`: Image.new + `pillow_chain` per piece + Image.paste;
  * `restated_compose`: a numpy canvas, `restated_chain` per piece written into its dest rect.
The CPU test pins the second against the first on every case, which licenses it as the GPU test's second oracle.
A case is dict(images, pieces, size, fill): pieces is a list per canvas of (src, crop (l, t, w, h), flip, jitter or None,
dest (dx, dy, dw, dh)) -- what `augment.compose_batch` takes.
"""
import functools

import numpy as np

from tests import augment_cases as ac


def _fill_of(fill, n):
    f = np.asarray(fill, dtype=np.uint8)
    return f if f.ndim == 1 else f[n]


def pillow_compose(images, pieces, size, fill):
    """uint8 [N, out_h, out_w, 3], by Pillow"""
    from PIL import Image
    out_h, out_w = size
    out = []
    for n, canvas in enumerate(pieces):
        cv = Image.new("RGB", (out_w, out_h), tuple(int(v) for v in _fill_of(fill, n)))
        for src, crop, flip, jitter, (dx, dy, dw, dh) in canvas:
            cv.paste(Image.fromarray(ac.pillow_chain(images[src], crop, flip, jitter, dh, dw)), (dx, dy))
        out.append(np.array(cv))
    return np.stack(out)


def restated_compose(images, pieces, size, fill):
    """uint8 [N, out_h, out_w, 3], in numpy"""
    out_h, out_w = size
    out = np.empty((len(pieces), out_h, out_w, 3), dtype=np.uint8)
    for n, canvas in enumerate(pieces):
        out[n] = _fill_of(fill, n)
        for src, crop, flip, jitter, (dx, dy, dw, dh) in canvas:
            out[n, dy:dy + dh, dx:dx + dw] = ac.restated_chain(images[src], crop, flip, jitter, dh, dw)
    return out


# ------------------------------------------------------------------------------------------------------------------------ cases
def _case(images, pieces, size, fill=(124, 116, 104)):
    return dict(images=images, pieces=pieces, size=size, fill=fill)


def _noisy(shape, rgb, seed):
    """a flat colour plus noise of +-8"""
    noise = np.random.default_rng(seed).integers(-8, 9, size=(shape[0], shape[1], 3))
    return np.clip(np.array(rgb)[None, None] + noise, 0, 255).astype(np.uint8)


def _ramp(shape):
    """left-right and top-bottom asymmetric: red rises with x, green with y"""
    im = np.zeros((shape[0], shape[1], 3), dtype=np.uint8)
    im[..., 0] = np.linspace(0, 255, shape[1]).astype(np.uint8)[None]
    im[..., 1] = np.linspace(0, 255, shape[0]).astype(np.uint8)[:, None]
    im[..., 2] = 77
    return im


def _mosaic_edges():
    # canvas 56 x 300, centre (cx, cy) = (299, 1): a 1-pixel-high top row, a 1-pixel-wide right column, and two pieces 299 wide that
    # straddle the 256-column block boundary.  Bottom right: a 15 x 800 crop -> 1 x 55, 31 taps both ways, next to the upscaled
    # bottom left (120 x 30 -> 299 x 55).
    imgs = [ac._rand((40, 400), 200), ac._rand((20, 30), 201), ac._rand((50, 150), 202), ac._rand((820, 40), 203)]
    canvas = [(0, (30, 12, 350, 10), True, (1.2, 0.8, 1.1), (0, 0, 299, 1)),
              (1, (11, 9, 7, 5), False, None, (299, 0, 1, 1)),
              (2, (20, 10, 120, 30), True, (1.0, 1.0, 0.4), (0, 1, 299, 55)),
              (3, (13, 7, 15, 800), False, (0.9, 1.3, 1.0), (299, 1, 1, 55))]
    return _case(imgs, [canvas], (56, 300))


def _abutting():
    # a 3 x 3 grid of unequal cells on 42 x 42, each cell another flat colour plus noise: a gap would show the fill, an overlap the
    # neighbour's colour
    xs, ys = [0, 13, 30, 42], [0, 9, 20, 42]
    colours = [(250, 20, 20), (20, 250, 20), (20, 20, 250), (250, 250, 20), (250, 20, 250), (20, 250, 250), (128, 128, 128), (240, 240, 240),
               (15, 15, 15)]
    imgs = [_noisy((30 + 3 * i, 41 - 2 * i), c, 210 + i) for i, c in enumerate(colours)]
    canvas = []
    for r in range(3):
        for c in range(3):
            i = 3 * r + c
            H, W = imgs[i].shape[:2]
            canvas.append((i, (1, 2, W - 3, H - 4), bool(i & 1), None, (xs[c], ys[r], xs[c + 1] - xs[c], ys[r + 1] - ys[r])))
    return _case(imgs, [canvas], (42, 42), fill=(0, 255, 0))


def _sixteen():
    # 16 pieces on one canvas (the cap), next to a canvas without pieces and a canvas with one
    imgs = [ac._rand((25 + i, 33 - i), 230 + i) for i in range(6)]
    xs, ys = [0, 9, 22, 30, 44], [0, 12, 19, 31, 40]
    full = []
    for r in range(4):
        for c in range(4):
            i = 4 * r + c
            s = i % 6
            H, W = imgs[s].shape[:2]
            jit = (1.0 + 0.05 * i, 1.0 - 0.03 * i, 1.0) if i % 3 == 0 else None
            full.append((s, (i % 5, i % 4, W - 6, H - 5), bool(i % 2), jit, (xs[c], ys[r], xs[c + 1] - xs[c], ys[r + 1] - ys[r])))
    one = [(5, (0, 0, 28, 30), True, (0.7, 1.0, 1.4), (3, 5, 30, 21))]
    return _case(imgs, [full, [], one], (40, 44))


def _shared_source():
    # one source under four pieces with different crops and contrast factors: the mean is each piece's own
    img = np.concatenate([ac._rand((30, 40), 240) // 4, 128 + ac._rand((30, 40), 241) // 2], axis=1)      # dark left half, bright right half
    canvas = [(0, (0, 0, 40, 30), False, (1.0, 1.8, 1.0), (0, 0, 24, 20)),
              (0, (40, 0, 40, 30), False, (1.0, 0.3, 1.0), (24, 0, 24, 20)),
              (0, (20, 5, 40, 20), True, (1.0, 1.8, 1.0), (0, 20, 24, 20)),
              (0, (0, 0, 80, 30), False, (1.1, 1.5, 0.9), (24, 20, 24, 20))]
    return _case([img], [canvas], (40, 48))


def _zoom_out():
    # a piece strictly inside its canvas: the fill on all four sides; one fill per canvas
    imgs = [ac._rand((45, 60), 250), ac._rand((33, 41), 251)]
    pieces = [[(0, (0, 0, 60, 45), False, None, (7, 5, 31, 23))],
              [(1, (3, 2, 35, 30), True, (1.2, 0.9, 1.1), (1, 1, 48, 34))]]
    return _case(imgs, pieces, (36, 50), fill=[(1, 2, 3), (200, 100, 50)])


def _flip_inside():
    # an asymmetric piece flipped at dx > 0: it mirrors within its own rect
    return _case([_ramp((40, 90))], [[(0, (5, 3, 80, 30), True, None, (17, 4, 40, 20))]], (30, 64), fill=(1, 2, 3))


def _factors():
    # the FACTORS grid of augment_cases (every factor alone in every enhancer, chains, the hard-edged image under the clip branch) on
    # pieces: four per canvas
    dests = [(0, 0, 25, 19), (25, 0, 23, 19), (0, 19, 25, 21), (25, 19, 23, 21)]
    imgs, flat = [], []
    for k in range(3):
        for i, f in enumerate(ac.FACTORS):
            fs = [1.0, 1.0, 1.0]
            fs[k] = f
            imgs.append(ac._rand((24, 31), 260 + 6 * k + i))
            flat.append((len(imgs) - 1, (2, 1, 27, 22), bool((k + i) & 1), tuple(fs)))
    for i, fs in enumerate([(0.37, 0.999, 0.0), (1.0001, 1.9, 1.0001), (1.9, 0.0, 1.9), (0.999, 1.0001, 0.37)]):
        imgs.append(ac._rand((24, 31), 290 + i))
        flat.append((len(imgs) - 1, (0, 0, 31, 24), bool(i & 1), fs))
    imgs.append(ac._hard((24, 31)))
    flat.append((len(imgs) - 1, (1, 1, 29, 22), True, (1.9, 1.9, 1.9)))
    pieces = [[p + (dests[j],) for j, p in enumerate(flat[i:i + 4])] for i in range(0, len(flat), 4)]
    return _case(imgs, pieces, (40, 48))


CASES = {"mosaic_edges": _mosaic_edges, "abutting": _abutting, "sixteen": _sixteen, "shared_source": _shared_source, "zoom_out": _zoom_out,
         "flip_inside": _flip_inside, "factors": _factors}


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and the restatement's uint8 [N, out_h, out_w, 3] result, computed once (read-only)"""
    c = CASES[name]()
    want = restated_compose(c["images"], c["pieces"], c["size"], c["fill"])
    want.setflags(write=False)
    return c, want


@functools.lru_cache(maxsize=None)
def pillow(name):
    """Pillow's result of the case, computed once (read-only)"""
    c, _ = case(name)
    want = pillow_compose(c["images"], c["pieces"], c["size"], c["fill"])
    want.setflags(write=False)
    return want


# ---------------------------------------------------------------------------------------------------------------------- targets
def targets_f64(boxes, shape, piece, size, min_visibility=0.0):
    """one piece's target transform in float64: (keep mask [n], canvas-normalised cxcywh of the kept [k, 4], margins [n, 3] as
    augment_cases.targets_f64 gives them)"""
    _, crop, flip, _, (dx, dy, dw, dh) = piece
    out_h, out_w = size
    keep, rel, margins = ac.targets_f64(boxes, shape, crop, flip, min_visibility)      # normalised cxcywh of the crop
    cx, cy, w, h = rel.T
    out = np.stack([(dx + cx * dw) / out_w, (dy + cy * dh) / out_h, w * dw / out_w, h * dh / out_h], axis=1)
    return keep, out, margins
