"""dod_roi_embed (include/dinodet.h) restated in numpy, for tests/test_roi_embed_cpu.py and tests/test_gpu_roi_embed.py.

The contract, as the header states it.  The tokens first_token + r * gw + c of an image are a gh x gw map with centres at (c + 0.5, r + 0.5).
A row is valid when it lies below the image's count, its coordinates are finite and x2 > x1, y2 > y1 in fp32.  Its box goes to map units in
double (u = (x * gw) / width, v = (y * gh) / height), is clipped to the map, and is invalid when nothing is left.  grid x grid sample points
at the centres of the box's cells are sampled bilinearly at (u - 0.5, v - 0.5), coordinates clamped to the map, the upper neighbour clamped to
the last index (torchvision's aligned ROIAlign); the pooled vector is their mean and the output its L2 normalisation (zeros when the norm
is 0, zeros for invalid rows).

`literal` is that sentence, sample by sample.  `separable` is what the kernel computes: per axis the samples' weights are summed per token
index (at most 2 * grid non-zero ones), p = sum_r sum_c wy[r] wx[c] f[r, c, :] over the tokens whose fp32 weight product is not zero -- a
token with weight zero is not read, so it may hold anything.  Both work in float64; `separable` also returns what the error bound of the
GPU test needs."""
import numpy as np

F = np.float32
MAX_K, MAX_D, MAX_GRID = 1024, 2048, 8


def valid_rows(boxes, counts):
    """boxes [B, K, 4] f32, counts [B] or None -> bool [B, K]: the tracker's rule"""
    B, K = boxes.shape[:2]
    cnt = np.full(B, K) if counts is None else np.clip(np.asarray(counts, np.int64), 0, K)
    with np.errstate(invalid="ignore"):
        return (np.arange(K)[None, :] < cnt[:, None]) & np.isfinite(boxes).all(axis=2) & (boxes[..., 2] > boxes[..., 0]) & (boxes[..., 3] > boxes[..., 1])


def _clip(x, hi):
    x = 0.0 if x < 0.0 else x                    # as the kernel's conditionals: a NaN passes through both
    return hi if x > hi else x


def map_box(box, size, gh, gw):
    """one valid fp32 box, size = (height, width) -> (u1, v1, u2, v2) in map units, or None when nothing is left after clipping"""
    x1, y1, x2, y2 = (float(v) for v in box)
    hh, ww = (1.0, 1.0) if size is None else (float(F(size[0])), float(F(size[1])))
    with np.errstate(all="ignore"):
        u1, u2 = (_clip(float(np.float64(x) * gw / np.float64(ww)), float(gw)) for x in (x1, x2))
        v1, v2 = (_clip(float(np.float64(y) * gh / np.float64(hh)), float(gh)) for y in (y1, y2))
    if not (u2 > u1 and v2 > v1):
        return None
    return u1, v1, u2, v2


def sample_points(a1, a2, grid):
    step = (a2 - a1) / float(grid)
    return [a1 + (i + 0.5) * step for i in range(grid)]


def axis_weights(a1, a2, n, grid):
    """the weight every one of the n token indices of an axis gets from the samples of [a1, a2]: dense float64 [n], summed in sample order
    (lower neighbour, then upper) and divided by grid once"""
    w = np.zeros(n)
    for a in sample_points(a1, a2, grid):
        x = _clip(a - 0.5, float(n - 1))
        c0 = int(x)
        c1 = min(c0 + 1, n - 1)
        f = x - c0
        w[c0] = w[c0] + (1.0 - f)
        w[c1] = w[c1] + f
    return w / float(grid)


def _bilinear(fmap, x, y):
    """fmap [gh, gw, D] float64 at (x, y) by the clamped rules"""
    gh, gw = fmap.shape[:2]
    x, y = _clip(x, float(gw - 1)), _clip(y, float(gh - 1))
    c0, r0 = int(x), int(y)
    c1, r1 = min(c0 + 1, gw - 1), min(r0 + 1, gh - 1)
    fx, fy = x - c0, y - r0
    return ((1 - fy) * ((1 - fx) * fmap[r0, c0] + fx * fmap[r0, c1]) + fy * ((1 - fx) * fmap[r1, c0] + fx * fmap[r1, c1]))


def _unit(p):
    n = float(np.sqrt(np.sum(p * p)))
    return p / n if n > 0.0 else np.zeros_like(p)


def _maps(features, first_token, gh, gw):
    B, N, D = features.shape
    assert first_token >= 0 and first_token + gh * gw <= N
    return features[:, first_token:first_token + gh * gw].astype(np.float64).reshape(B, gh, gw, D)


def literal(features, first_token, gh, gw, boxes, counts, sizes, grid):
    """the mean of the grid^2 bilinear samples, normalised: float64 [B, K, D].  Reads all four neighbours of a sample, so the map must be
    finite."""
    fm = _maps(features, first_token, gh, gw)
    B, K = boxes.shape[:2]
    out = np.zeros((B, K, features.shape[2]))
    ok = valid_rows(boxes, counts)
    for b in range(B):
        for k in range(K):
            m = map_box(boxes[b, k], None if sizes is None else sizes[b], gh, gw) if ok[b, k] else None
            if m is None:
                continue
            p = np.zeros(features.shape[2])
            for v in sample_points(m[1], m[3], grid):
                for u in sample_points(m[0], m[2], grid):
                    p = p + _bilinear(fm[b], u - 0.5, v - 0.5)
            out[b, k] = _unit(p / float(grid * grid))
    return out


def separable(features, first_token, gh, gw, boxes, counts, sizes, grid):
    """what the kernel computes, in float64 with the exact (double) weights -> (emb [B, K, D], info) with info[b][k] = None for a row that
    comes out as zeros, else dict(wx, wy, tokens = how many tokens have a non-zero fp32 weight product, p = the pooled vector before
    normalisation, a = sum w |f| per channel)"""
    B, K, D = boxes.shape[0], boxes.shape[1], features.shape[2]
    out = np.zeros((B, K, D))
    info = [[None] * K for _ in range(B)]
    ok = valid_rows(boxes, counts)
    for b in range(B):
        for k in range(K):
            m = map_box(boxes[b, k], None if sizes is None else sizes[b], gh, gw) if ok[b, k] else None
            if m is None:
                continue
            wx, wy = axis_weights(m[0], m[2], gw, grid), axis_weights(m[1], m[3], gh, grid)
            p, a, n = np.zeros(D), np.zeros(D), 0
            for r in np.nonzero(wy)[0]:
                for c in np.nonzero(wx)[0]:
                    if F(wy[r]) * F(wx[c]) == 0:                          # the kernel skips (does not read) a token whose fp32 weight is zero
                        continue
                    f = features[b, first_token + r * gw + c].astype(np.float64)
                    p = p + (wy[r] * wx[c]) * f
                    a = a + (wy[r] * wx[c]) * np.abs(f)
                    n += 1
            out[b, k] = _unit(p)
            info[b][k] = dict(wx=wx, wy=wy, tokens=n, p=p, a=a)
    return out, info


def boxes_for(gh, gw, height, width, K=8):
    """the K = 8 rows of the tests, in pixels of a height x width image whose token map is gh x gw: the whole image; strictly inside one
    token; straddling the border; wholly outside; x2 <= x1; a NaN coordinate; a plain box; (with counts = 7) a row beyond the count"""
    tw, th = width / gw, height / gh
    c, r = gw // 2, gh // 2
    rows = [(0.0, 0.0, width, height),
            (c * tw + 0.2 * tw, r * th + 0.3 * th, c * tw + 0.7 * tw, r * th + 0.8 * th),
            (-0.4 * width, 0.1 * height, 0.3 * width, 1.5 * height),
            (1.1 * width, 0.2 * height, 1.6 * width, 0.9 * height),
            (0.6 * width, 0.2 * height, 0.6 * width, 0.9 * height),
            (0.1 * width, float("nan"), 0.5 * width, 0.9 * height),
            (0.13 * width, 0.21 * height, 0.87 * width, 0.66 * height),
            (0.2 * width, 0.2 * height, 0.8 * width, 0.8 * height)]
    assert K == len(rows)
    return np.asarray(rows, np.float32)
