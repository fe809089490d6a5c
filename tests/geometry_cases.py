"""Closed-loop geometry cases (tests/test_geometry_loop_cpu.py, tests/test_gpu_geometry_loop.py): paint objects, push pixels and boxes
through the input pipeline separately, measure the objects in the output pixels and compare with the boxes.  The reference is the
image itself, not a formula: a box that no longer frames the pixels it framed in the source fails, however faithfully a float64
restatement repeats the formula that produced it.  numpy only (and Pillow, where a warp case is drawn), nothing of the project;
tests/geometry_train.py has what reads `TrainAugment`'s plans back.

`paint` draws solid rectangles in six saturated colours (R, G, B, C, M, Y at 0 / 255) on uniform noise in [0, 40); the colour index is
the label, an object is the set of pixels whose channels are >= 128 exactly where its colour's are.  The noise, the default fill
(124, 116, 104) and every blend of an object with them below half coverage are "no object".  `extent` is a mask's bounding box,
`check` holds the boxes to it.

THE BOUND.  A mask thresholded at 128 between a background of at most 39 and an object at 255 switches at a coverage between 0.41
and 0.5, so with Pillow's triangle filter the mask edge sits within 0.5 + 0.09 max(1, s) output pixels of the true edge, s being the
output pixels per source pixel: 0.5 is the pixel quantisation, the rest the threshold bias, which is outward.  `bound(s)` is
0.5 + 0.1 max(1, s) per side, every case keeps s <= 4 (at most 0.9 px), and over the sides of a pipeline that are not clipped at the
output border |mean signed residual| <= 0.25 px: a half-pixel convention error moves the mean by 0.5 px.  For a pipeline of two
resampling stages (a chain or canvas, then a warp) s is max(1, s_chain) max(1, m), m the warp's largest local magnification: the
first stage leaves a ramp at least one of its own pixels wide and the second stretches it.

WHAT A CASE MUST KEEP for the premise to hold (all decided from the case's own integers, never from a result of the project's):
  * two rectangles of one source are at least a filter support (2 x the largest down-scaling + 1 source pixels) apart, so no pixel
    blends two colours (yellow and cyan blend to green);
  * the part of a rectangle that a crop, a dest rect or the canvas leaves visible is either nothing or at least 3 output pixels in
    both axes: a sliver thinner than the filter has no plateau for the threshold to cut;
  * explicit plans down-scale by at most 4 and up-scale by at most 4.
Brightness is the only jitter and stays within [0.9, 1.2]: the object stays above 229 and the noise below 47, so the switching
coverage stays within 0.39 .. 0.56, inside what the 0.1 s term allows.

WARPS.  The box is the hull of the four mapped corners.  A box that touches the output border was clipped by the canvas: the visible
part's hull may be smaller, so such a box is held to containment only (the extent lies inside the box plus the bound); every other box
is held on both sides.

ROTATED CORNERS.  The 0.5 and the 0.09 above are the quantisation and the bias at a straight edge that runs along the pixel grid.
Every side of a rotated rectangle's hull is one of its corners, and a corner loses pixels twice over:
  * the ramps of the two edges multiply, so the thresholded mask is rounded and ends short of the corner: `corner_depth(phi)` ramp
    widths for edges tilted by phi against the grid, -0.09 .. 0 at 0 degrees (the straight edge), 0.13 at 15, 0.25 at 30;
  * the mask ends in a wedge that is (tan phi + cot phi) d wide at depth d, and a wedge narrower than a pixel can pass between two
    pixel centres: only from d = sin(2 phi) / 2 on must a row hold one, so the quantisation is 0.5 + sin(2 phi) / 2, not 0.5.
So Pillow's own pixels are sure to meet 0.5 + 0.1 max(1, s) on a hull side only while sin(2 phi) / 2 + corner_depth(phi) <= 0.1, a
tilt of at most `MAX_TILT` = 3.8 degrees; beyond it they meet it or not by the corner's sub-pixel position (at 30 degrees and s = 1 the
mask can end 1.18 px inside the hull).  The bound stays what it is on every box.  A case that Pillow's own pixels take over it is a
wrong case: a warp is drawn again until Pillow's warp of the painted source frames every mapped rectangle within the bound
(`pillow_frames`, against the hull by the case's own `forward`, nothing of the project), so the committed warps reach 30 degrees at
corner positions where the bound can be met, and every third affine is drawn within MAX_TILT.
"""
import collections
import functools
import math

import numpy as np

from tests import warp_cases as wc

COLOURS = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0)], dtype=np.uint8)
FILL = (124, 116, 104)
SIZES = ((96, 128), (56, 150), (64, 64))
MAX_SCALE = 4.0            # the largest up- and down-scaling of an explicit plan
MIN_SIDE = 12
MIN_VISIBLE = 3.0          # output pixels
MEAN_BOUND = 0.25
MIN_SIDES = 300


class GeometryError(AssertionError):
    pass


Residuals = collections.namedtuple("Residuals", ["res", "free", "contain"])
Residuals.__doc__ = """res float64 [n, 4]: extent - box per side (x1, y1, x2, y2) in output pixels; free bool [n, 4]: the side is not
clipped at the output border and its box is held on both sides (what the mean is taken over); contain bool [n]: containment only"""


def paint(H, W, rects, seed):
    """uint8 [H, W, 3]: uniform grey noise in [0, 40) with the rectangles (x1, y1, x2, y2, colour), far sides exclusive, solid on it.
    The noise is the same in the three channels: with independent channels the edge of a cyan object, blended over a pixel whose
    green is 39 and whose blue is 0, crosses 128 in green before it does in blue, and a line of green pixels frames every cyan one."""
    img = np.repeat(np.random.default_rng(seed).integers(0, 40, size=(H, W, 1), dtype=np.uint8), 3, axis=2)
    for x1, y1, x2, y2, c in rects:
        img[y1:y2, x1:x2] = COLOURS[c]
    return img


def boxes_of(rects, H, W):
    """the rectangles as (normalised cxcywh float32 [n, 4], labels int64 [n])"""
    r = np.asarray(rects, dtype=np.float64).reshape(-1, 5)
    b = np.stack([(r[:, 0] + r[:, 2]) / (2 * W), (r[:, 1] + r[:, 3]) / (2 * H), (r[:, 2] - r[:, 0]) / W, (r[:, 3] - r[:, 1]) / H], axis=1)
    return b.astype(np.float32), r[:, 4].astype(np.int64)


def mask(out_u8, colour):
    return ((np.asarray(out_u8) >= 128) == (COLOURS[int(colour)] >= 128)).all(axis=-1)


def extent(out_u8, colour):
    """(x1, y1, x2, y2) of the colour's mask, max + 1 on the far sides, or None"""
    m = mask(out_u8, colour)
    if not m.any():
        return None
    xs, ys = np.flatnonzero(m.any(axis=0)), np.flatnonzero(m.any(axis=1))
    return int(xs[0]), int(ys[0]), int(xs[-1]) + 1, int(ys[-1]) + 1


def bound(s):
    return 0.5 + 0.1 * max(1.0, float(s))


def corner_depth(phi, coverage=0.5):
    """how far inside a rectangle's corner the mask's hull ends, in ramp widths, when the rectangle's edges are tilted by phi degrees
    against the pixel grid.  Across an edge the bilinear ramp is r(t) = 0.5 + t for |t| <= 0.5 (t inward, in source pixels); near a
    corner the value is r(a) r(b), a and b the depths behind the two edges, and the mask is where it reaches `coverage`.  The hull side
    through the corner has the inward normal (cos phi, sin phi) in (a, b), so the mask's hull ends at the least a cos phi + b sin phi
    over the contour r(a) r(b) = coverage, taken numerically.  The default is the largest switching coverage, the deepest."""
    phi = math.radians(min(abs(float(phi)), 90.0 - abs(float(phi))) if abs(float(phi)) <= 90.0 else 0.0)
    b = np.linspace(-0.5, 0.5, 4001)
    ra = coverage / np.maximum(0.5 + b, 1e-9)
    ok = ra <= 1.0
    return float(((ra - 0.5) * math.cos(phi) + b * math.sin(phi))[ok].min())


MAX_TILT = 3.8             # degrees: sin(2 phi) / 2 + corner_depth(phi) = 0.099, the steepest tilt that fits the bound's 0.1 max(1, s)


def tilt(pts):
    """the largest tilt, in degrees, of the quadrilateral's edges (corners [4, 2] in order) against the nearer axis"""
    v = np.roll(np.asarray(pts, dtype=np.float64), -1, axis=0) - np.asarray(pts, dtype=np.float64)
    lo, hi = np.abs(v).min(axis=1), np.abs(v).max(axis=1)
    return float(np.degrees(np.arctan2(lo, hi)).max())


def xyxy_of(boxes, size):
    """normalised cxcywh -> xyxy in pixels of size = (height, width), float64"""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    h, w = size
    return np.stack([(b[:, 0] - 0.5 * b[:, 2]) * w, (b[:, 1] - 0.5 * b[:, 3]) * h, (b[:, 0] + 0.5 * b[:, 2]) * w, (b[:, 1] + 0.5 * b[:, 3]) * h], axis=1)


def touches_border(boxes, size, eps=1e-3):
    """bool [n, 4]: the side of the normalised cxcywh box lies on the border of the size = (height, width) output"""
    b = xyxy_of(boxes, size)
    h, w = size
    return np.stack([b[:, 0] <= eps, b[:, 1] <= eps, b[:, 2] >= w - eps, b[:, 3] >= h - eps], axis=1)


def check(out_u8, boxes, labels, size, upscale, contain=None, fmt="cxcywh", tol=None):
    """out_u8: uint8 [h, w, 3]; boxes: [n, 4] normalised cxcywh of size = (h, w), or with fmt="xyxy" pixels; labels [n]: colour indices;
    upscale: the case's s; contain: None or bool [n], the boxes held to containment only; tol: None (bound(upscale) on every side) or
    the tolerance per axis (tol_x, tol_y), scalars or [n].  Raises GeometryError unless
      * every box has a non-empty mask of its colour, and no colour has two boxes;
      * every colour without a box has a mask thinner than 2 px in some axis, or none;
      * every side meets its tolerance: |extent - box| <= tol, or for a containment-only box the extent lies inside the box + tol.
    Returns Residuals."""
    out_u8 = np.asarray(out_u8)
    h, w = size
    if out_u8.shape != (h, w, 3) or out_u8.dtype != np.uint8:
        raise GeometryError(f"expected a uint8 [{h}, {w}, 3] image, got {out_u8.dtype} {out_u8.shape}")
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    b = xyxy_of(b, size) if fmt == "cxcywh" else b
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    n = len(b)
    if len(labels) != n:
        raise GeometryError(f"{n} boxes, {len(labels)} labels")
    contain = np.zeros(n, dtype=bool) if contain is None else np.asarray(contain, dtype=bool).reshape(n)
    tx, ty = (bound(upscale),) * 2 if tol is None else tol
    t = np.stack([np.broadcast_to(np.asarray(tx, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(ty, dtype=np.float64), (n,))] * 2, axis=1)
    if ((labels < 0) | (labels >= len(COLOURS))).any():
        raise GeometryError(f"labels outside 0..{len(COLOURS) - 1}: {labels.tolist()}")
    if len(np.unique(labels)) != n:
        raise GeometryError(f"a colour has more than one box: labels {labels.tolist()}")
    for c in range(len(COLOURS)):
        e = extent(out_u8, c)
        if c not in labels and e is not None and e[2] - e[0] >= 2 and e[3] - e[1] >= 2:
            raise GeometryError(f"colour {c} shows at {e} and has no box (labels {labels.tolist()})")
    res = np.full((n, 4), np.nan)
    for i in range(n):
        e = extent(out_u8, labels[i])
        if e is None:
            raise GeometryError(f"box {i} (colour {labels[i]}, {np.round(b[i], 2).tolist()}) has no pixel of its colour")
        res[i] = np.asarray(e, dtype=np.float64) - b[i]
    inward = res * np.array([1.0, 1.0, -1.0, -1.0])                 # > 0: the extent lies inside the box on that side
    bad = (inward < -t) | (~contain[:, None] & (inward > t))
    if bad.any():
        i, k = np.argwhere(bad)[0]
        raise GeometryError(f"box {i} (colour {labels[i]}), side {'x1 y1 x2 y2'.split()[k]}: extent - box = {res[i, k]:+.3f} px, allowed {t[i, k]:.3f}"
                            f"{' (containment)' if contain[i] else ''}; box {np.round(b[i], 2).tolist()}, {int(bad.sum())} sides in all")
    at_border = np.stack([b[:, 0] <= 1e-3, b[:, 1] <= 1e-3, b[:, 2] >= w - 1e-3, b[:, 3] >= h - 1e-3], axis=1)
    return Residuals(res, ~at_border & ~contain[:, None], contain)


class Tally:
    """the residuals of one pipeline: worst side, mean signed residual per side over the free sides, their number"""

    def __init__(self, name):
        self.name, self.res, self.free, self.contain = name, [], [], []

    def add(self, r):
        self.res.append(r.res), self.free.append(r.free), self.contain.append(r.contain)
        return r

    def summary(self):
        res, free, contain = (np.concatenate(x) if x else np.zeros((0, 4)) for x in (self.res, self.free, self.contain))
        free = free.astype(bool)
        two_sided = res[~contain.astype(bool)] if len(res) else res
        return dict(boxes=len(res), sides=int(free.sum()), worst=float(np.abs(two_sided).max()) if two_sided.size else 0.0,
                    mean=[float(res[:, k][free[:, k]].mean()) if free[:, k].any() else 0.0 for k in range(4)],
                    contain_share=float(contain.mean()) if len(contain) else 0.0)

    def report(self):
        s = self.summary()
        line = (f"geometry loop [{self.name}]: {s['boxes']} boxes, {s['sides']} free sides, worst |residual| {s['worst']:.3f} px, mean signed "
                f"residual (x1, y1, x2, y2) " + " ".join(f"{m:+.3f}" for m in s["mean"]) + f", containment-only {100 * s['contain_share']:.0f} %")
        print(line)
        return s

    def hold(self, min_sides=MIN_SIDES):
        """the per-pipeline condition: at least `min_sides` free sides and |mean signed residual| <= 0.25 px on each of the four"""
        s = self.report()
        if s["sides"] < min_sides:
            raise GeometryError(f"{self.name}: only {s['sides']} sides that are not clipped at the output border, need {min_sides}")
        if max(abs(m) for m in s["mean"]) > MEAN_BOUND:
            raise GeometryError(f"{self.name}: mean signed residual per side {np.round(s['mean'], 3).tolist()} px, allowed {MEAN_BOUND}")
        return s


# ------------------------------------------------------------------------------------------------------------------- generators
def place(rng, H, W, colours, lo, hi, gap, region=None, accept=None):
    """disjoint rectangles (x1, y1, x2, y2, colour), one per colour where it fits, sides in [lo, hi], at least `gap` apart, inside
    region = (x1, y1, x2, y2) of the image (all of it by default) and accepted by accept(x1, y1, x2, y2) if given; at least one"""
    rx1, ry1, rx2, ry2 = (0, 0, W, H) if region is None else region
    lo, hi = int(lo), int(max(lo, hi))
    rects = []
    for c in colours:
        for _ in range(200):
            w, h = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
            if w > rx2 - rx1 or h > ry2 - ry1:
                continue
            x, y = int(rng.integers(rx1, rx2 - w + 1)), int(rng.integers(ry1, ry2 - h + 1))
            if accept is not None and not accept(x, y, x + w, y + h):
                continue
            if all(x >= q[2] + gap or q[0] >= x + w + gap or y >= q[3] + gap or q[1] >= y + h + gap for q in rects):
                rects.append((x, y, x + w, y + h, int(c)))
                break
    assert rects, (H, W, lo, hi, gap)
    return rects


def visible(rect, crop):
    """(width, height) in source pixels of the part of the rectangle inside crop = (left, top, width, height)"""
    l, t, cw, ch = crop
    return max(0, min(rect[2], l + cw) - max(rect[0], l)), max(0, min(rect[3], t + ch) - max(rect[1], t))


def crop_ok(rects, crop, dw, dh):
    """every rectangle is either not in the crop at all or shows at least MIN_VISIBLE output pixels in both axes of the dw x dh dest"""
    for r in rects:
        vw, vh = visible(r, crop)
        if vw > 0 and vh > 0 and (vw * dw / crop[2] < MIN_VISIBLE or vh * dh / crop[3] < MIN_VISIBLE):
            return False
    return True


def crop_kind(rects, crop):
    """(rectangles cut by the crop, rectangles it excludes, rectangles whole inside)"""
    cut = out = whole = 0
    for r in rects:
        vw, vh = visible(r, crop)
        if vw == 0 or vh == 0:
            out += 1
        elif vw < r[2] - r[0] or vh < r[3] - r[1]:
            cut += 1
        else:
            whole += 1
    return cut, out, whole


def draw_crop(rng, H, W, rects, dw, dh, want="any", s_max=MAX_SCALE):
    """a crop (left, top, width, height) of an [H, W] source for a dw x dh dest: scaled by at most 4 down and s_max up, `crop_ok`, and
    of the kind asked for: "any" (some rectangle shows), "cut" (one is cut), "exclude" (one is left out, one shows), "none" (none shows)"""
    w_lo, w_hi = max(1, math.ceil(dw / s_max)), min(W, int(MAX_SCALE * dw))
    h_lo, h_hi = max(1, math.ceil(dh / s_max)), min(H, int(MAX_SCALE * dh))
    assert w_lo <= w_hi and h_lo <= h_hi, (H, W, dw, dh)
    for attempt in range(4000):
        cw, ch = int(rng.integers(w_lo, w_hi + 1)), int(rng.integers(h_lo, h_hi + 1))
        crop = (int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1)), cw, ch)
        if not crop_ok(rects, crop, dw, dh):
            continue
        cut, out, whole = crop_kind(rects, crop)
        if {"any": cut + whole > 0, "cut": cut > 0, "exclude": out > 0 and cut + whole > 0, "none": cut + whole == 0}[want]:
            return crop
    raise AssertionError(f"no {want} crop of a {H}x{W} source for a {dh}x{dw} dest")


def _source(rng, seed, lo, hi, colours, n_max=3, region_half=False):
    """(image, rects, (H, W)): a painted source with sides in [lo, hi]; rectangles 14 .. 0.45 x the shorter side, 9 apart (a filter
    support at 4x down-scaling); region_half: all rectangles in the left half, the right half stays background"""
    H, W = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    gap = int(2 * MAX_SCALE) + 1
    side_lo = max(MIN_SIDE, math.ceil(MIN_VISIBLE * MAX_SCALE) + 2)
    rects = place(rng, H, W, list(colours)[:n_max], side_lo, max(side_lo, int(0.45 * min(H, W))), gap, (0, 0, W // 2 - 2, H) if region_half else None)
    return paint(H, W, rects, seed), rects, (H, W)


def _brightness(rng, on):
    return None if not on else (float(np.float32(rng.uniform(0.9, 1.2))), 1.0, 1.0)


def chain_case(seed, size):
    """the plain chain: 5 to 8 ragged sources of 60 .. 260 px, a crop each (by turns: any, one that cuts a rectangle, one that excludes
    one, any), flips alternating with the turn shifted, brightness on every second case"""
    rng = np.random.default_rng(1000 + seed)
    out_h, out_w = size
    B = 5 + seed % 4
    images, rects, shapes, crops, flips, jitter = [], [], [], [], [], []
    for b in range(B):
        colours = rng.permutation(6)
        im, rs, (H, W) = _source(rng, 7 * seed + b, 60, 260, colours, n_max=2 + (b + seed) % 2)
        want = ("any", "cut", "exclude", "any")[b % 4]
        if want == "exclude" and len(rs) < 2:
            want = "cut"
        images.append(im), rects.append(rs), shapes.append((H, W))
        crops.append(draw_crop(rng, H, W, rs, out_w, out_h, want))
        flips.append((b + seed // 2) % 2)
        jitter.append(_brightness(rng, True))
    jit = np.asarray(jitter, dtype=np.float32) if seed % 2 else None
    s = [max(out_w / c[2], out_h / c[3]) for c in crops]
    return dict(images=images, rects=rects, shapes=shapes, crops=np.asarray(crops, dtype=np.int32), flips=np.asarray(flips, dtype=np.uint8), jitter=jit,
                size=size, s=s)


def _piece_s(pieces):
    return [max([max(d[2] / c[2], d[3] / c[3]) for _, c, _, _, d in canvas] or [1.0]) for canvas in pieces]


def _split(rng, lo, hi):
    return int(rng.integers(lo, hi + 1))


def mosaic_case(seed, size, s_max=MAX_SCALE):
    """four-piece mosaics: 5 or 6 canvases, four sources of 60 .. 200 px each with disjoint colours (2 + 2 + 1 + 1), the centre within
    0.3 .. 0.7 of the canvas, every piece its own crop, flip and (on every second case) brightness"""
    rng = np.random.default_rng(2000 + seed)
    out_h, out_w = size
    N = 5 + seed % 2
    images, rects, shapes, pieces = [], [], [], []
    for n in range(N):
        cx, cy = _split(rng, math.ceil(0.3 * out_w), int(0.7 * out_w)), _split(rng, math.ceil(0.3 * out_h), int(0.7 * out_h))
        dests = [(0, 0, cx, cy), (cx, 0, out_w - cx, cy), (0, cy, cx, out_h - cy), (cx, cy, out_w - cx, out_h - cy)]
        colours = rng.permutation(6)
        groups = [colours[:2], colours[2:4], colours[4:5], colours[5:6]]
        canvas = []
        for q in rng.permutation(4):                      # the paste order is not the quadrant order
            dest = dests[q]
            im, rs, (H, W) = _source(rng, 100 * seed + 4 * n + int(q), 60, 200, groups[q], n_max=2)
            images.append(im), rects.append(rs), shapes.append((H, W))
            want = "cut" if (n + q) % 3 == 0 else "any"
            crop = draw_crop(rng, H, W, rs, dest[2], dest[3], want, s_max)
            canvas.append((len(images) - 1, crop, bool(rng.integers(0, 2)), _brightness(rng, seed % 2 == 1), dest))
        pieces.append(canvas)
    return dict(images=images, rects=rects, shapes=shapes, pieces=pieces, size=size, fill=FILL, s=_piece_s(pieces))


def zoom_out_case(seed, size):
    """zoom-out: 5 to 7 canvases of one piece each, 1 / r of the canvas with r in 1 .. 2, anywhere inside it; the rest is the fill"""
    rng = np.random.default_rng(3000 + seed)
    out_h, out_w = size
    N = 5 + seed % 3
    images, rects, shapes, pieces = [], [], [], []
    for n in range(N):
        r = rng.uniform(1.0, 2.0)
        dw, dh = max(1, round(out_w / r)), max(1, round(out_h / r))
        dest = (_split(rng, 0, out_w - dw), _split(rng, 0, out_h - dh), dw, dh)
        im, rs, (H, W) = _source(rng, 100 * seed + n, 60, 160, rng.permutation(6), n_max=3)
        images.append(im), rects.append(rs), shapes.append((H, W))
        crop = draw_crop(rng, H, W, rs, dw, dh, ("any", "cut", "exclude")[n % 3] if len(rs) > 1 else "any")
        pieces.append([(n, crop, bool((n + seed) % 2), _brightness(rng, seed % 2 == 0), dest)])
    return dict(images=images, rects=rects, shapes=shapes, pieces=pieces, size=size, fill=FILL, s=_piece_s(pieces))


def sixteen_case(seed, size):
    """the 16-piece canvas (the cap): a 4 x 4 grid of unequal cells over six sources of one colour each.  A source's rectangle sits in
    its left half; the first piece of a source shows it, the later ones crop the right half, which holds background only, so every
    colour shows once.  A second canvas holds one piece, so the batch is ragged in pieces as well."""
    rng = np.random.default_rng(4000 + seed)
    out_h, out_w = size
    xs = [0] + sorted(int(v) for v in rng.choice(np.arange(out_w // 5, out_w - out_w // 5, 8), 3, replace=False)) + [out_w]
    ys = [0] + sorted(int(v) for v in rng.choice(np.arange(out_h // 5, out_h - out_h // 5, 8), 3, replace=False)) + [out_h]
    images, rects, shapes = [], [], []
    for i, c in enumerate(rng.permutation(6)):
        im, rs, hw = _source(rng, 100 * seed + i, 80, 140, [c], n_max=1, region_half=True)
        images.append(im), rects.append(rs), shapes.append(hw)
    cells = [(xs[c], ys[r], xs[c + 1] - xs[c], ys[r + 1] - ys[r]) for r in range(4) for c in range(4)]
    order = rng.permutation(16)
    full = []
    for k, cell in enumerate(order):
        src, dest = k % 6, cells[cell]
        H, W = shapes[src]
        if k < 6:
            crop = draw_crop(rng, H, W, rects[src], dest[2], dest[3], "any")
        else:                                               # background only: the right half
            cw, ch = min(W - W // 2, 2 * dest[2]), min(H, 2 * dest[3])
            crop = (W // 2 + _split(rng, 0, W - W // 2 - cw), _split(rng, 0, H - ch), cw, ch)
            assert crop_kind(rects[src], crop)[:2] == (0, 1) and cw <= MAX_SCALE * dest[2] and ch <= MAX_SCALE * dest[3]
        full.append((src, crop, bool(rng.integers(0, 2)), None, dest))
    one = [(0, draw_crop(rng, *shapes[0], rects[0], out_w // 2, out_h // 2, "any"), True, None, (out_w // 4, out_h // 4, out_w // 2, out_h // 2))]
    pieces = [full, one]
    return dict(images=images, rects=rects, shapes=shapes, pieces=pieces, size=size, fill=FILL, s=_piece_s(pieces))


# ------------------------------------------------------------------------------------------------------------------------ warps
def forward(coeffs, pts):
    """source points [n, 2] -> the output points that show them: the inverse of the coefficients' 3 x 3 matrix"""
    F = np.linalg.inv(np.append(np.asarray(coeffs, dtype=np.float64), 1.0).reshape(3, 3))
    q = np.concatenate([np.asarray(pts, dtype=np.float64).reshape(-1, 2), np.ones((len(pts), 1))], axis=1) @ F.T
    return q[:, :2] / q[:, 2:3]


def magnification(coeffs, shape, size):
    """the largest local stretch (largest singular value of the forward map's Jacobian, by central differences) over a 9 x 9 grid of the
    [H, W] source, at the grid points shown inside the size = (height, width) output (all of them if none is)"""
    H, W = shape
    g = np.stack(np.meshgrid(np.linspace(0, W, 9), np.linspace(0, H, 9)), axis=-1).reshape(-1, 2)
    p = forward(coeffs, g)
    inside = (p[:, 0] >= 0) & (p[:, 0] <= size[1]) & (p[:, 1] >= 0) & (p[:, 1] <= size[0])
    g = g[inside] if inside.any() else g
    e = 0.25
    jx = (forward(coeffs, g + [e, 0]) - forward(coeffs, g - [e, 0])) / (2 * e)
    jy = (forward(coeffs, g + [0, e]) - forward(coeffs, g - [0, e])) / (2 * e)
    J = np.stack([jx, jy], axis=-1)
    return float(np.linalg.svd(J, compute_uv=False)[:, 0].max())


def compose_coeffs(a, b):
    """warping by a first and by b second as one warp: M(a) M(b), renormalised"""
    M = np.append(np.asarray(a, dtype=np.float64), 1.0).reshape(3, 3) @ np.append(np.asarray(b, dtype=np.float64), 1.0).reshape(3, 3)
    return (M / M[2, 2]).reshape(9)[:8]


def warp_ok(coeffs, rects, size):
    """every rectangle is either shown nowhere -- the hull of its mapped corners misses the output by a pixel -- or shows at least
    MIN_VISIBLE + 1 output pixels in both axes, measured on its points at half-pixel spacing that land inside the output"""
    out_h, out_w = size
    for x1, y1, x2, y2, _ in rects:
        hull = forward(coeffs, [(x1, y1), (x2, y1), (x2, y2), (x1, y2)])
        if hull[:, 0].max() < -1 or hull[:, 0].min() > out_w + 1 or hull[:, 1].max() < -1 or hull[:, 1].min() > out_h + 1:
            continue
        g = np.stack(np.meshgrid(np.arange(x1, x2 + 0.25, 0.5), np.arange(y1, y2 + 0.25, 0.5)), axis=-1).reshape(-1, 2)
        p = forward(coeffs, g)
        p = p[(p[:, 0] >= 0) & (p[:, 0] <= out_w) & (p[:, 1] >= 0) & (p[:, 1] <= out_h)]
        if len(p) == 0 or np.ptp(p[:, 0]) < MIN_VISIBLE + 1 or np.ptp(p[:, 1]) < MIN_VISIBLE + 1:
            return False
    return True


def draw_affine(rng, shape, size, scale=(0.7, 1.3), gentle=False):
    """output -> source coefficients of a random affine about the centres: up to 30 degrees of rotation, scale 0.7 .. 1.3, up to 10
    degrees of shear, a translation of up to a tenth of the output; gentle: up to 2 degrees of rotation and 1.5 of shear, so that every
    edge stays within MAX_TILT of the grid"""
    turn, shear = (2.0, 1.5) if gentle else (30.0, 10.0)
    return wc.inverse_affine(shape, size, angle=rng.uniform(-turn, turn), scale=rng.uniform(*scale), shear_x=rng.uniform(-shear, shear),
                             translate=(round(rng.uniform(-0.1, 0.1) * size[1]), round(rng.uniform(-0.1, 0.1) * size[0])))


def draw_perspective(rng, shape, size, distortion=0.3):
    """the source's corners shown at the output's corners, each moved inward by up to distortion x half the side"""
    (H, W), (oh, ow) = shape, size
    d = rng.uniform(0, distortion * 0.5, 8)
    quad = [(d[0] * ow, d[1] * oh), (ow - d[2] * ow, d[3] * oh), (ow - d[4] * ow, oh - d[5] * oh), (d[6] * ow, oh - d[7] * oh)]
    return wc.quad_coeffs([(0, 0), (W, 0), (W, H), (0, H)], quad)


def pillow_frames(image, coeffs, rects, size, s, fill=FILL):
    """whether Pillow's own warp of `image` keeps every rectangle's mask within bound(s) of the hull of its four mapped corners -- on
    both sides where the hull lies inside the output, else inside the clipped hull plus the bound.  The hull is the case's own
    arithmetic (`forward`); nothing of the project is asked."""
    out_h, out_w = size
    out = wc.pillow_warp(image, coeffs, out_h, out_w, fill)
    b = bound(s) - 1e-3                                  # (the boxes under test are float32: a case is not admitted on the last digit)
    for x1, y1, x2, y2, c in rects:
        p = forward(coeffs, [(x1, y1), (x2, y1), (x2, y2), (x1, y2)])
        hull = np.array([p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()])
        clipped = np.clip(hull, 0.0, [out_w, out_h, out_w, out_h])
        e = extent(out, c)
        if clipped[2] <= clipped[0] or clipped[3] <= clipped[1]:
            if e is not None:
                return False
            continue
        if e is None:
            return False
        inward = (np.asarray(e, dtype=np.float64) - clipped) * [1.0, 1.0, -1.0, -1.0]
        if (inward < -b).any() or ((hull == clipped).all() and (inward > b).any()):
            return False
    return True


def _drawn_warp(rng, draw, image, rects, size, s_of, fill=FILL):
    """the first draw that `warp_ok` admits, that keeps the up-scaling s_of(coefficients) within 4, and whose Pillow pixels frame the mapped
    rectangles within the bound (`pillow_frames`): a draw that Pillow's own pixels take over the bound is a wrong case, not a reason
    for another bound.  A corner of a tilted rectangle loses pixels (see the module docstring), so steep draws are turned down often;
    those kept sit at lucky sub-pixel phases, which takes nothing from what they check."""
    shape = image.shape[:2]
    for _ in range(5000):
        c = draw(rng, shape, size)
        if s_of(c) <= MAX_SCALE and warp_ok(c, rects, size) and pillow_frames(image, c, rects, size, s_of(c), fill):
            return c
    raise AssertionError(f"no admissible warp of a {shape} source onto {size}")


def warp_case(seed, size, kind):
    """warps straight from painted sources: kind "affine" (sources about the output's size, so the scale is the warp's own) or
    "perspective" (sources of 60 .. 160 px, corner to corner: the map scales by output / source as well)"""
    rng = np.random.default_rng((5000 if kind == "affine" else 6000) + seed)
    out_h, out_w = size
    B = 5 + seed % 4
    images, rects, shapes, coeffs = [], [], [], []
    for b in range(B):
        if kind == "affine":
            H, W = int(rng.integers(max(60, out_h - 20), out_h + 41)), int(rng.integers(max(60, out_w - 40), out_w + 41))
        else:
            H, W = int(rng.integers(60, 161)), int(rng.integers(60, 161))
        down = max(1.0, H / out_h, W / out_w) if kind == "perspective" else 1.5
        lo = max(MIN_SIDE, math.ceil((MIN_VISIBLE + 2) * down))
        region = (int(0.15 * W), int(0.15 * H), W - int(0.15 * W), H - int(0.15 * H)) if kind == "affine" else None
        rs = place(rng, H, W, rng.permutation(6)[:2 + b % 2], lo, max(lo, int(0.35 * min(H, W))), math.ceil(2 * down) + 2, region)
        images.append(paint(H, W, rs, 100 * seed + b)), rects.append(rs), shapes.append((H, W))
        draw = draw_perspective if kind == "perspective" else functools.partial(draw_affine, gentle=b % 3 == 2)      # every third one gentle
        coeffs.append(_drawn_warp(rng, draw, images[-1], rs, size, lambda c: magnification(c, (H, W), size)))
    s = [magnification(c, hw, size) for c, hw in zip(coeffs, shapes)]
    return dict(images=images, rects=rects, shapes=shapes, coeffs=np.asarray(coeffs), size=size, fill=FILL, s=s)


def staged_case(seed, size):
    """affine o perspective behind a mosaic: `mosaic_case` with pieces up-scaled by at most 2, then per canvas one warp at the output
    size, an affine composed with a perspective.  What the warp must keep visible is what the mosaic shows: the canvas rectangles."""
    for k in range(20):                                   # the first mosaic no seam of which has two colours within 2 px of each other
        c = mosaic_case(500 + 20 * seed + k, size, s_max=2.0)
        canvases = [shown_rects(c["rects"], canvas) for canvas in c["pieces"]]
        if all(_apart(p, q, 2.0) for shown in canvases for i, p in enumerate(shown) for q in shown[:i]):
            break
    else:
        raise AssertionError("no mosaic without two colours at one seam")
    from tests import compose_cases as cc
    rng = np.random.default_rng(7000 + seed)
    coeffs, s = [], []
    draw = lambda g, shape, sz: compose_coeffs(draw_affine(g, shape, sz, scale=(0.8, 1.2)), draw_perspective(g, shape, sz))
    for n, (shown, canvas) in enumerate(zip(canvases, cc.pillow_compose(c["images"], c["pieces"], size, c["fill"]))):
        s_of = lambda k: max(1.0, c["s"][n]) * max(1.0, magnification(k, size, size))
        coeffs.append(_drawn_warp(rng, draw, canvas, shown, size, s_of, c["fill"]))
        s.append(s_of(coeffs[-1]))
    return dict(c, coeffs=np.asarray(coeffs), s_compose=c["s"], s=s, shown=canvases)


def _apart(p, q, gap):
    return p[0] >= q[2] + gap or q[0] >= p[2] + gap or p[1] >= q[3] + gap or q[1] >= p[3] + gap


def shown_rects(rects, canvas):
    """where a canvas shows the sources' rectangles: (x1, y1, x2, y2, colour) in canvas pixels, from the plan's own integers (the crop
    clips, the flip mirrors inside the dest rect, the dest rect scales and places)"""
    shown = []
    for src, crop, flip, _, (dx, dy, dw, dh) in canvas:
        for r in rects[src]:
            vw, vh = visible(r, crop)
            if vw > 0 and vh > 0:
                x1, x2 = (max(r[0], crop[0]) - crop[0]) * dw / crop[2], (min(r[2], crop[0] + crop[2]) - crop[0]) * dw / crop[2]
                y1, y2 = (max(r[1], crop[1]) - crop[1]) * dh / crop[3], (min(r[3], crop[1] + crop[3]) - crop[1]) * dh / crop[3]
                if flip:
                    x1, x2 = dw - x2, dw - x1
                shown.append((dx + x1, dy + y1, dx + x2, dy + y2, r[4]))
    return shown


@functools.lru_cache(maxsize=None)
def cases(pipeline):
    """the committed cases of a pipeline, built once (read-only by convention): every output size, several seeds"""
    make = {"chain": chain_case, "mosaic": mosaic_case, "zoom_out": zoom_out_case, "sixteen": sixteen_case,
            "affine": lambda s, z: warp_case(s, z, "affine"), "perspective": lambda s, z: warp_case(s, z, "perspective"), "staged": staged_case}[pipeline]
    seeds = {"chain": 8, "mosaic": 2, "zoom_out": 6, "sixteen": 4, "affine": 5, "perspective": 5, "staged": 3}[pipeline]
    return [make(seed, size) for size in SIZES for seed in range(seeds)]


def targets_of(case):
    """the case's target dicts as numpy: [{"boxes" float32 [n, 4], "labels" int64 [n]}] per source"""
    return [dict(zip(("boxes", "labels"), boxes_of(rs, H, W))) for rs, (H, W) in zip(case["rects"], case["shapes"])]


# ------------------------------------------------------------------------------------------------------------ sliced inference
def tile_starts(L, tile, overlap):
    """the tile starts along an axis of length L as the slicing documents them: 0, step, 2 step ... with step = tile - floor(tile x
    overlap), the last tile moved back to end at L; [0] when the axis is no longer than the tile"""
    if L <= tile:
        return [0], L
    step, starts, x = tile - math.floor(tile * overlap), [], 0
    while x + tile < L:
        starts.append(x)
        x += step
    return starts + [L - tile], tile


def whole_in_a_tile(a, b, L, tile, overlap, margin):
    """[a, b) lies in some tile of the axis, `margin` away from each tile border that is not the axis's own end"""
    starts, t = tile_starts(L, tile, overlap)
    return any((a >= x0 + margin or x0 == 0) and (b <= x0 + t - margin or x0 + t == L) for x0 in starts)


def slicing_sources(seed, n=3, lo=200, hi=260, side=(24, 60), tiles=None):
    """(images, rects, shapes) for sliced inference: sources of 200 .. 260 px with up to four rectangles of `side` px, 9 apart; tiles:
    None or (tile, overlap, margin) -- every rectangle then lies whole in some tile, `margin` px away from the tile's inner borders, so
    the tiles alone can return it"""
    rng = np.random.default_rng(8000 + seed)
    images, rects, shapes = [], [], []
    for b in range(n):
        H, W = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        accept = None if tiles is None else (lambda x1, y1, x2, y2: whole_in_a_tile(x1, x2, W, *tiles) and whole_in_a_tile(y1, y2, H, *tiles))
        rs = place(rng, H, W, rng.permutation(6)[:3 + b % 2], side[0], side[1], 9, accept=accept)
        images.append(paint(H, W, rs, 900 + 10 * seed + b)), rects.append(rs), shapes.append((H, W))
    return images, rects, shapes


# ---------------------------------------------------------------------------------------------------------------- holding a case
WARPED = ("affine", "perspective", "staged")


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def hold_images(tally, outs, targets, size, s, warped=False):
    """`check` on every image of a batch: outs uint8 [N, h, w, 3] (or a list), targets the new target dicts, s the up-scaling per
    image.  Behind a warp a box that touches the output border is held to containment only.  The residuals go to `tally`."""
    for n, out in enumerate(outs):
        bx, lb = _np(targets[n]["boxes"]).reshape(-1, 4), _np(targets[n]["labels"]).reshape(-1)
        contain = touches_border(bx, size).any(axis=1) if warped else None
        try:
            tally.add(check(_np(out), bx, lb, size, s[n], contain))
        except GeometryError as e:
            raise GeometryError(f"{tally.name}, image {n} (s = {s[n]:.2f}): {e}") from None


def float_to_u8(x):
    """float32 [N, 3, h, w] in [0, 1] -> uint8 [N, h, w, 3] by round(x * 255)"""
    return np.rint(np.transpose(_np(x), (0, 2, 3, 1)).astype(np.float64) * 255.0).astype(np.uint8)
