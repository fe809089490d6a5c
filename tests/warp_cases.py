"""Shared cases and oracles of the geometric-warp tests (tests/test_warp_cpu.py, tests/test_gpu_warp.py): random affine and perspective
as Pillow's  Image.transform((out_w, out_h), PERSPECTIVE, coeffs, BILINEAR, fillcolor=fill).

Two oracles:
  * `pillow_warp`: Pillow itself;
  * `restated_warp`: numpy in float64, one rounding per operation (numpy never contracts), Pillow's Geometry.c restated: per output pixel
        xin = x + 0.5; yin = y + 0.5; den = a6 xin + a7 yin + 1; sx = (a0 xin + a1 yin + a2) / den; sy = (a3 xin + a4 yin + a5) / den
        outside <=> not (0 <= sx < W and 0 <= sy < H) -> the fill; else sx -= 0.5, sy -= 0.5, ix = floor(sx), iy = floor(sy),
        dx = sx - ix, dy = sy - iy, columns clamp(ix), clamp(ix + 1), row clamp(iy) and row iy + 1 if it exists (else v2 = v1),
        byte = (uint8)(v1 + (v2 - v1) dy) with v = p0 + (p1 - p0) dx.
The CPU test pins the second against the first on every case, which licenses it as the GPU test's oracle.  `restated_pixel` is the same
in scalar Python, with a `fused` switch that evaluates each  a + (b - a) d  exactly and rounds once, as an FMA would: the fma_probe case
gives another byte under it, so the case can tell a kernel compiled with contraction from one without; its `fused_coords` switch does
the same for the coordinate sums  a0 xin + a1 yin + a2  (the fma_coord_probe case).
A case is dict(images, coeffs float64 [B, 8], size (out_h, out_w), fill (3,) or [B, 3]).
"""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import augment_cases as ac

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def _fill_of(fill, b):
    f = np.asarray(fill, dtype=np.uint8)
    return f if f.ndim == 1 else f[b]


def restated_warp(img, coeffs, out_h, out_w, fill):
    """uint8 [out_h, out_w, 3], in numpy float64"""
    H, W = img.shape[:2]
    a = [np.float64(v) for v in coeffs]
    xin = (np.arange(out_w, dtype=np.float64) + 0.5)[None, :]
    yin = (np.arange(out_h, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        den = a[6] * xin + a[7] * yin + 1.0
        sx = (a[0] * xin + a[1] * yin + a[2]) / den
        sy = (a[3] * xin + a[4] * yin + a[5]) / den
        inside = (sx >= 0.0) & (sx < W) & (sy >= 0.0) & (sy < H)
    out = np.empty((out_h, out_w, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    if H < 1 or W < 1 or not inside.any():
        return out
    sx, sy = sx[inside] - 0.5, sy[inside] - 0.5
    fx, fy = np.floor(sx), np.floor(sy)
    dx, dy = (sx - fx)[:, None], (sy - fy)[:, None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, r0 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1)
    p = img.astype(np.float64)
    v1 = p[r0, x0] + (p[r0, x1] - p[r0, x0]) * dx
    has2 = (iy + 1 >= 0) & (iy + 1 < H)
    r1 = np.where(has2, iy + 1, r0)
    v2 = np.where(has2[:, None], p[r1, x0] + (p[r1, x1] - p[r1, x0]) * dx, v1)
    out[inside] = (v1 + (v2 - v1) * dy).astype(np.uint8)
    return out


def pillow_warp(img, coeffs, out_h, out_w, fill, method="PERSPECTIVE"):
    """uint8 [out_h, out_w, 3], by Pillow; method AFFINE takes the first six coefficients"""
    from PIL import Image
    data = [float(v) for v in coeffs]
    m = Image.Transform.PERSPECTIVE if method == "PERSPECTIVE" else Image.Transform.AFFINE
    im = Image.fromarray(img).transform((out_w, out_h), m, data if method == "PERSPECTIVE" else data[:6], Image.Resampling.BILINEAR,
                                        fillcolor=tuple(int(v) for v in fill))
    return np.array(im)


def _lerp(a, b, d, fused):
    if fused:
        return float(Fraction(a) + (Fraction(b) - Fraction(a)) * Fraction(d))       # exact, rounded once
    return a + (b - a) * d


def _line(p, q, r, xin, yin, fused_coords):
    """p xin + q yin + r; fused_coords 1: the first product fused into the sum, fma(p, xin, q yin), 2: the second, fma(q, yin, p xin)"""
    if fused_coords == 1:
        return float(Fraction(p) * Fraction(xin) + Fraction(q * yin)) + r
    if fused_coords == 2:
        return float(Fraction(q) * Fraction(yin) + Fraction(p * xin)) + r
    return p * xin + q * yin + r


def restated_pixel(img, coeffs, x, y, fill, fused=False, fused_coords=0):
    """one output pixel (three bytes) in scalar Python floats; fused: every lerp as a fused multiply-add would round it; fused_coords:
    the coordinate sums with one of their products contracted (`_line`)"""
    H, W = img.shape[:2]
    a = [float(v) for v in coeffs]
    xin, yin = x + 0.5, y + 0.5
    den = a[6] * xin + a[7] * yin + 1.0
    sx, sy = _line(a[0], a[1], a[2], xin, yin, fused_coords) / den, _line(a[3], a[4], a[5], xin, yin, fused_coords) / den
    if not (sx >= 0.0 and sx < W and sy >= 0.0 and sy < H):
        return tuple(int(v) for v in fill)
    sx, sy = sx - 0.5, sy - 0.5
    ix, iy = math.floor(sx), math.floor(sy)
    dx, dy = sx - ix, sy - iy
    x0, x1, r0 = min(max(ix, 0), W - 1), min(max(ix + 1, 0), W - 1), min(max(iy, 0), H - 1)
    out = []
    for c in range(3):
        v1 = _lerp(float(img[r0, x0, c]), float(img[r0, x1, c]), dx, fused)
        v2 = _lerp(float(img[iy + 1, x0, c]), float(img[iy + 1, x1, c]), dx, fused) if 0 <= iy + 1 < H else v1
        out.append(int(_lerp(v1, v2, dy, fused)))
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------------- coefficients
def inverse_affine(src, out, angle=0.0, scale=1.0, shear_x=0.0, translate=(0.0, 0.0)):
    """output -> source coefficients of: rotate by `angle` degrees (clockwise, y down), shear, scale about the centres, then translate.
    Direct algebra, independent of dinov2_od_amd.augment: p_src = c_src + A^-1 (p_out - c_out - t)."""
    (H, W), (oh, ow) = src, out
    r, t = math.radians(angle), math.tan(math.radians(shear_x))
    A = np.array([[math.cos(r), -math.sin(r)], [math.sin(r), math.cos(r)]]) @ np.array([[1.0, -t], [0.0, 1.0]]) * scale
    Ai = np.linalg.inv(A)
    off = np.array([W / 2, H / 2]) - Ai @ (np.array([ow / 2, oh / 2]) + np.asarray(translate, dtype=np.float64))
    return np.array([Ai[0, 0], Ai[0, 1], off[0], Ai[1, 0], Ai[1, 1], off[1], 0.0, 0.0])


def quad_coeffs(src_quad, out_quad):
    """output -> source coefficients showing src_quad[i] at out_quad[i]: the 8 x 8 system, solved directly"""
    A, rhs = [], []
    for (u, v), (X, Y) in zip(src_quad, out_quad):
        A += [[X, Y, 1, 0, 0, 0, -X * u, -Y * u], [0, 0, 0, X, Y, 1, -X * v, -Y * v]]
        rhs += [u, v]
    return np.linalg.solve(np.array(A, dtype=np.float64), np.array(rhs, dtype=np.float64))


def forward_point(coeffs, u, v):
    """the output point that shows source point (u, v): the inverse of the 3 x 3 matrix applied to (u, v, 1)"""
    F = np.linalg.inv(np.append(np.asarray(coeffs, dtype=np.float64), 1.0).reshape(3, 3))
    q = F @ np.array([u, v, 1.0])
    return q[0] / q[2], q[1] / q[2]


# ------------------------------------------------------------------------------------------------------------------------ cases
def _case(images, coeffs, size, fill=(124, 116, 104)):
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(len(images), 8)
    return dict(images=images, coeffs=coeffs, size=size, fill=fill)


def _copies(name):
    # exact copies of a 9 x 13 source (H = 9, W = 13): every sample falls on a pixel centre, dx = dy = 0
    img = ac._rand((9, 13), 500)
    c, size = {"identity": (IDENTITY, (9, 13)),
               "translate_int": ((1, 0, 3, 0, 1, -2, 0, 0), (9, 13)),
               "mirror": ((-1, 0, 13, 0, 1, 0, 0, 0), (9, 13)),
               "transpose": ((0, 1, 0, 1, 0, 0, 0, 0), (13, 9))}[name]
    return _case([img], [c], size, fill=(1, 2, 3))


def _rotate30():
    return _case([ac._rand((40, 50), 510)], [inverse_affine((40, 50), (56, 56), angle=30.0)], (56, 56))


def _shear():
    return _case([ac._rand((40, 50), 511)], [inverse_affine((40, 50), (56, 56), shear_x=20.0, translate=(3.0, -2.0))], (56, 56))


def _scale_down():
    return _case([ac._rand((40, 50), 512)], [inverse_affine((40, 50), (56, 56), angle=-7.0, scale=0.5)], (56, 56))


def _scale_up():
    # 3x on the 0 / 255 column pattern: every lerp spans the full byte range
    return _case([ac._hard((40, 50))], [inverse_affine((40, 50), (56, 56), angle=4.0, scale=3.0)], (56, 56))


def _perspective():
    # a modest corner distortion; next to it an affine handed over as eight coefficients (a6 = a7 = 0)
    H, W, o = 40, 50, 56
    quad = [(4.0, 2.5), (o - 6.5, 5.0), (o - 1.5, o - 3.0), (2.0, o - 7.5)]
    return _case([ac._rand((H, W), 520), ac._rand((H, W), 521)],
                 [quad_coeffs([(0, 0), (W, 0), (W, H), (0, H)], quad), inverse_affine((H, W), (o, o), angle=12.0, scale=1.1, shear_x=5.0)], (o, o))


def _all_fill():
    return _case([ac._rand((20, 30), 530)], [(1, 0, 1000, 0, 1, 0, 0, 0)], (24, 40), fill=(9, 200, 77))


def _partly_outside():
    return _case([ac._rand((30, 40), 531), ac._rand((30, 40), 532)],
                 [inverse_affine((30, 40), (48, 40), angle=25.0, translate=(14.0, -9.0)), inverse_affine((30, 40), (48, 40), scale=0.7, translate=(-20.0, 20.0))],
                 (48, 40), fill=[(1, 2, 3), (200, 100, 50)])


def _boundary():
    # H = 9, W = 13 -> 10 x 14.  Image 0, offsets -0.5: sx is exactly 0.0 at x = 0 (inside; ix = -1 after the -0.5, clamped) and exactly
    # W at x = 13 (fill); the same vertically.  Image 1, offsets +0.25: at the last inside row sy - 0.5 = H - 0.75, so iy + 1 == H and
    # v2 = v1; the last inside column clamps x1.  Image 2, offsets -0.25: ix = iy = -1 with dx = dy = 0.75.
    img = ac._rand((9, 13), 540)
    return _case([img, img, img], [(1, 0, -0.5, 0, 1, -0.5, 0, 0), (1, 0, 0.25, 0, 1, 0.25, 0, 0), (1, 0, -0.25, 0, 1, -0.25, 0, 0)], (10, 14),
                 fill=(255, 0, 255))


def _thin():
    srcs = [(1, 1), (1, 17), (17, 1)]
    return _case([ac._rand(s, 550 + i) for i, s in enumerate(srcs)],
                 [inverse_affine(s, (12, 12), angle=10.0 * i, scale=12.0 / max(s) * 0.9) for i, s in enumerate(srcs)], (12, 12))


FMA_DX = float.fromhex("0x1.2d2d2d2d2d2d4p-2")      # 17 + (0 - 17) dx: 12 rounded twice, 11 rounded once
FMA_DY = float.fromhex("0x1.0e38e38e38e3ap-1")      # 68 + (32 - 68) dy: 49 rounded twice, 48 rounded once


def _fma_probe():
    # image 0: the row [., 17, 0], the output pixel samples between columns 1 and 2 at dx (sx - 0.5 = 1 + dx, exactly); image 1: the
    # column [68, 32], sampled between rows 0 and 1 at dy (sy - 0.5 = dy, exactly; dx = 0, so v1 and v2 are the bytes themselves)
    row = np.array([[[99, 99, 99], [17, 17, 17], [0, 0, 0]]], dtype=np.uint8)
    col = np.array([[[68, 68, 68]], [[32, 32, 32]]], dtype=np.uint8)
    return _case([row, col], [(1, 0, 1.0 + FMA_DX, 0, 1, 0, 0, 0), (1, 0, 0, 0, 1, FMA_DY, 0, 0)], (1, 1), fill=(7, 7, 7))


FMA_COORD = tuple(float.fromhex(h) for h in ("0x1.1bcf024eed30fp-1", "0x1.c12151ccdd66fp-2", "-0x1.6bbf84c1a8dc0p-3"))


def _fma_coord_probe():
    # the row [0, 255] -> 2 x 2; at output pixel (1, 1) (xin = yin = 1.5, so neither product is exact) a0 xin + a1 yin + a2 puts
    # 255 dx one ulp below 207: Pillow writes 206, and 207 if either product is contracted into the sum
    row = np.array([[[0, 0, 0], [255, 255, 255]]], dtype=np.uint8)
    return _case([row], [FMA_COORD + (0.0, 0.0, 0.5, 0.0, 0.0)], (2, 2), fill=(7, 7, 7))


def _two_tiles_wide():
    return _case([ac._rand((40, 50), 560)], [inverse_affine((40, 50), (20, 300), angle=8.0, scale=4.0)], (20, 300))


def _two_tiles_tall():
    return _case([ac._rand((40, 50), 561)], [inverse_affine((40, 50), (37, 70), angle=-33.0, scale=1.2, shear_x=6.0)], (37, 70))


def _ragged():
    shapes = [(61, 47), (33, 90), (50, 50), (7, 31), (20, 120)]
    o = (56, 56)
    quad = [(3.0, 6.0), (50.0, 1.0), (54.0, 52.0), (0.5, 49.0)]
    coeffs = [inverse_affine(shapes[0], o, angle=15.0, scale=0.9),
              inverse_affine(shapes[1], o, angle=-40.0, scale=0.6, shear_x=10.0, translate=(4.0, 2.0)),
              IDENTITY,
              quad_coeffs([(0, 0), (31, 0), (31, 7), (0, 7)], quad),
              inverse_affine(shapes[4], o, angle=90.0, scale=0.5)]
    return _case([ac._rand(s, 570 + i) for i, s in enumerate(shapes)], coeffs, o,
                 fill=[(0, 0, 0), (255, 255, 255), (124, 116, 104), (10, 20, 30), (250, 5, 128)])


CASES = {"identity": lambda: _copies("identity"), "translate_int": lambda: _copies("translate_int"), "mirror": lambda: _copies("mirror"),
         "transpose": lambda: _copies("transpose"), "rotate30": _rotate30, "shear": _shear, "scale_down": _scale_down, "scale_up": _scale_up,
         "perspective": _perspective, "all_fill": _all_fill, "partly_outside": _partly_outside, "boundary": _boundary, "thin": _thin,
         "fma_probe": _fma_probe, "fma_coord_probe": _fma_coord_probe, "two_tiles_wide": _two_tiles_wide, "two_tiles_tall": _two_tiles_tall, "ragged": _ragged}


@functools.lru_cache(maxsize=None)
def case(name):
    """the case and the restatement's uint8 [B, out_h, out_w, 3] result, computed once (read-only)"""
    c = CASES[name]()
    want = np.stack([restated_warp(im, c["coeffs"][b], *c["size"], _fill_of(c["fill"], b)) for b, im in enumerate(c["images"])])
    want.setflags(write=False)
    return c, want


# ---------------------------------------------------------------------------------------------------------------- target cases
def targets_f64(boxes, shape, coeffs, size, min_visibility=0.0):
    """the target transform in float64, box by box: (keep mask [n], output-normalised cxcywh of the kept [k, 4], margins [n, 3]): the
    distance of each box's clipped width and height fractions from 0.001 and of its visible-area ratio from min_visibility"""
    H, W = shape
    out_h, out_w = size
    keep, out, margins = [], [], []
    for cx, cy, bw, bh in np.asarray(boxes, dtype=np.float64).reshape(-1, 4):
        corners = [((cx + sx * 0.5 * bw) * W, (cy + sy * 0.5 * bh) * H) for sx in (-1, 1) for sy in (-1, 1)]
        pts = [forward_point(coeffs, u, v) for u, v in corners]
        ux1, ux2 = min(p[0] for p in pts), max(p[0] for p in pts)
        uy1, uy2 = min(p[1] for p in pts), max(p[1] for p in pts)
        x1, x2 = min(max(ux1, 0.0), out_w), min(max(ux2, 0.0), out_w)
        y1, y2 = min(max(uy1, 0.0), out_h), min(max(uy2, 0.0), out_h)
        fw, fh = (x2 - x1) / out_w, (y2 - y1) / out_h
        vis = (x2 - x1) * (y2 - y1) / ((ux2 - ux1) * (uy2 - uy1))
        k = x2 > x1 and y2 > y1 and fw >= 0.001 and fh >= 0.001 and vis >= min_visibility
        keep.append(k)
        margins.append((abs(fw - 0.001), abs(fh - 0.001), abs(vis - min_visibility) if min_visibility > 0 else 1.0))
        if k:
            out.append(((x1 + x2) / (2 * out_w), (y1 + y2) / (2 * out_h), fw, fh))
    return np.array(keep, dtype=bool), np.array(out, dtype=np.float64).reshape(-1, 4), np.array(margins, dtype=np.float64).reshape(-1, 3)


def random_boxes(n, seed, shape, coeffs, size, min_visibility, margin=1e-4):
    """n normalised cxcywh boxes (float32 values) inside the source, generated like augment_cases.random_boxes: some land outside the
    output, some straddle its edge; none within `margin` of a keep threshold"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        b = np.concatenate([rng.uniform(0.0, 1.0, 2), rng.uniform(0.002, 0.6, 2)]).astype(np.float32)
        if b[0] - b[2] / 2 < 0 or b[0] + b[2] / 2 > 1 or b[1] - b[3] / 2 < 0 or b[1] + b[3] / 2 > 1:
            continue
        if (targets_f64(b[None], shape, coeffs, size, min_visibility)[2] >= margin).all():
            out.append(b)
    return np.stack(out)


def target_cases():
    """(name, source shape, coefficients, output size, min_visibility): rotation, perspective and a warp that pushes boxes over the edge"""
    quad = [(-18.0, -6.0), (50.0, 9.0), (75.0, 66.0), (1.0, 44.0)]
    return [("rotate", (40, 50), inverse_affine((40, 50), (56, 56), angle=30.0, scale=1.7), (56, 56), 0.0),
            ("perspective", (40, 50), quad_coeffs([(0, 0), (50, 0), (50, 40), (0, 40)], quad), (56, 56), 0.3),
            ("clipped", (60, 45), inverse_affine((60, 45), (48, 64), angle=-20.0, scale=1.6, shear_x=8.0, translate=(17.0, -11.0)), (48, 64), 0.5),
            ("clipped_all_kept", (60, 45), inverse_affine((60, 45), (48, 64), angle=-20.0, scale=1.6, translate=(17.0, -11.0)), (48, 64), 0.0)]
