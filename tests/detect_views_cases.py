"""dod_detect_views (include/dinodet.h) restated in numpy, and the seeded inputs of tests/test_detect_views_cpu.py and
tests/test_gpu_detect_views.py.

The restatement follows the header to the letter and reuses the pieces of tests/detect_cases.py that the header reuses from dod_detect
(the key image of a logit, the sigmoid, the clamp, min / max): candidates over all views of an image (class >= first_class, logit not
NaN, threshold rule, edge filter per (view, query)), the stable order on (logit bits descending, flat index (v*Q + q)*C + c ascending),
the first K, boxes in float32 with one rounding per operation in the stated order (corners, mirror, `* extent`, `+ origin`, edge
filter, clamp), greedy NMS with the IoU or the intersection-over-smaller decision, compaction, padding.
"""
import numpy as np

from dinov2_od_amd import synth
from dinov2_od_amd.slicing import NMS_METRICS
from tests import detect_cases as dc

F = np.float32
assert (NMS_METRICS["iou"], NMS_METRICS["ios"]) == (0, 1)      # the nms_metric codes the Python layer passes are the ones dc.nms_keep takes


def view_boxes(rows, rect, flip):
    """rows [n, 4] cxcywh float32 of one view -> xyxy float32 in source pixels, before the edge filter and the clamp"""
    cx, cy, w, h = (np.ascontiguousarray(rows[:, i], dtype=np.float32) for i in range(4))
    vl, vt, vw, vh = (int(x) for x in rect)
    half, one = F(0.5), F(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        x1, y1, x2, y2 = cx - half * w, cy - half * h, cx + half * w, cy + half * h
        if flip:
            t = one - x2
            x2 = one - x1
            x1 = t
        x1, y1, x2, y2 = x1 * F(vw), y1 * F(vh), x2 * F(vw), y2 * F(vh)
        x1, y1, x2, y2 = x1 + F(vl), y1 + F(vt), x2 + F(vl), y2 + F(vt)
    return np.stack([x1, y1, x2, y2], axis=1).astype(np.float32)


def edge_cut(boxes, rect, margin, hw):
    """boolean [n]: the box is cut by a border of its view that is not a border of the hw = (height, width) source image"""
    cut = np.zeros(len(boxes), bool)
    if not margin > 0:
        return cut
    vl, vt, vw, vh = (int(x) for x in rect)
    m, ih, iw = F(margin), F(hw[0]), F(hw[1])
    with np.errstate(invalid="ignore"):
        if vl > 0:
            cut |= boxes[:, 0] < F(vl) + m
        if F(vl + vw) < iw:
            cut |= boxes[:, 2] > F(vl + vw) - m
        if vt > 0:
            cut |= boxes[:, 1] < F(vt) + m
        if F(vt + vh) < ih:
            cut |= boxes[:, 3] > F(vt + vh) - m
    return cut


def detect_views_ref(det, C, K, offsets, rects, flips, sizes, first_class=1, threshold=-1.0, iou=None, metric=0, class_agnostic=False,
                     clamp=True, edge_margin=0.0):
    """the whole call: {"scores" [B,K] f32, "labels", "views", "queries" [B,K] i32, "boxes" [B,K,4] f32, "counts" [B] i32,
    "selected" [B] (candidates taken before NMS), "rows" and "cut" [B] (the (view, query) rows of the image and how many the edge
    filter removed)}"""
    det = np.ascontiguousarray(det, dtype=np.float32)
    V, Q, _ = det.shape
    B = len(offsets) - 1
    hw = dc.size_rows(sizes, B)
    out = {"scores": np.zeros((B, K), np.float32), "labels": np.full((B, K), -1, np.int32), "views": np.full((B, K), -1, np.int32),
           "queries": np.full((B, K), -1, np.int32), "boxes": np.zeros((B, K, 4), np.float32), "counts": np.zeros(B, np.int32),
           "selected": np.zeros(B, np.int32), "rows": np.zeros(B, np.int64), "cut": np.zeros(B, np.int64)}
    for b in range(B):
        v0, v1 = int(offsets[b]), int(offsets[b + 1])
        nv = v1 - v0
        if nv == 0:
            continue
        raw = np.concatenate([view_boxes(det[v, :, C:], rects[v], flips[v]) for v in range(v0, v1)])        # [nv*Q, 4], r = v*Q + q
        cut = np.concatenate([edge_cut(raw[(v - v0) * Q:(v - v0 + 1) * Q], rects[v], edge_margin, hw[b]) for v in range(v0, v1)])
        out["rows"][b], out["cut"][b] = nv * Q, int(cut.sum())
        logits = det[v0:v1, :, :C].reshape(-1)
        sel = dc.select(logits, C, K, first_class, threshold, ~cut)
        r, lab = sel // C, sel % C
        vi, q = r // Q, r % Q
        bx = raw[r]
        if clamp:
            ih, iw = F(hw[b][0]), F(hw[b][1])
            bx = np.stack([dc._clamp(bx[:, 0], iw), dc._clamp(bx[:, 1], ih), dc._clamp(bx[:, 2], iw), dc._clamp(bx[:, 3], ih)], axis=1).astype(np.float32)
        sc = dc.sigmoid32(logits[sel])
        out["selected"][b] = len(sel)
        if iou is not None:
            keep = dc.nms_keep(bx, lab, iou, class_agnostic, metric)
            vi, q, lab, bx, sc = vi[keep], q[keep], lab[keep], bx[keep], sc[keep]
        n = len(q)
        out["counts"][b] = n
        out["scores"][b, :n], out["labels"][b, :n], out["views"][b, :n], out["queries"][b, :n], out["boxes"][b, :n] = sc, lab, vi, q, bx
    return out


# ------------------------------------------------------------------------------------------------ inputs
def offsets_of(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def image_sizes(B):
    """(height, width) per image: integers, as source images have them; odd ones among them"""
    return [(480.0 - 7 * (b % 5), 640.0 - 11 * (b % 3)) for b in range(B)]


def make_views(seed, counts, sizes):
    """rectangles inside their images with odd origins and extents, touching each of the four source borders in turn, and mixed flips.
    View k of an image: 0 the whole image; then by k % 5: the top-left corner, the bottom-right corner, an interior rectangle, a strip of
    the full width, a strip of the full height."""
    rects, flips = [], []
    for b, nv in enumerate(counts):
        H, W = int(sizes[b][0]), int(sizes[b][1])
        u = synth.uniform01(seed, f"dv.views.{b}.{nv}", (max(nv, 1), 5))
        for k in range(nv):
            w, h = 33 + 2 * int(u[k, 0] * (W - 80) / 2), 31 + 2 * int(u[k, 1] * (H - 80) / 2)      # odd extents, at least 40 short of the image
            l, t = 1 + 2 * int(u[k, 2] * (W - w - 2) / 2), 1 + 2 * int(u[k, 3] * (H - h - 2) / 2)  # odd origins, inside
            rect = [(0, 0, W, H), (0, 0, w, h), (W - w, H - h, w, h), (l, t, w, h), (0, t, W, h), (l, 0, w, H)][0 if k == 0 else 1 + k % 5]
            assert rect[0] >= 0 and rect[1] >= 0 and rect[0] + rect[2] <= W and rect[1] + rect[3] <= H
            rects.append(rect)
            flips.append(int(u[k, 4] < 0.5))
    return np.asarray(rects, np.int32).reshape(-1, 4), np.asarray(flips, np.uint8)


def make_case(seed, counts, Q, C, kind="random"):
    """(det [V, Q, C+4], offsets, rects, flips, sizes) for the given view counts per image"""
    V, B = int(sum(counts)), len(counts)
    sizes = image_sizes(B)
    rects, flips = make_views(seed, counts, sizes)
    n = max(V, 1)
    if kind == "random":
        det = dc.random_det(seed, n, Q, C)
    elif kind == "special":
        det = dc.special_det(seed, n, Q, C)
    elif kind == "ties":             # one view's quantised logits replicated over all views: ties that differ only in the view index
        det = np.repeat(dc.quantised_det(seed, 1, Q, C), n, axis=0)
        det[..., C:] = dc.rand_boxes(seed + 1, n, Q)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(det[:V]), offsets_of(counts), rects, flips, sizes


# the clustered multi-view scene: every cluster is seen from several views
NMS_KS = (4, 100, 512, 513, 1024)
NMS_CASES = [(K, iou, metric, agn) for K in NMS_KS for iou in (0.0, 0.5, 0.7) for metric in (0, 1) for agn in (False, True)]
SCENE_HW = (480, 640)
SCENE_VIEWS = [((0, 0, 640, 480), 0), ((0, 0, 400, 300), 0), ((240, 0, 400, 300), 0), ((0, 180, 400, 300), 0), ((240, 180, 400, 300), 0),
               ((0, 0, 640, 480), 1), ((240, 0, 400, 300), 1)]      # the four tiles share x in [240, 400], y in [180, 300]


def clustered_views(K, seed=60, C=5, centres=4):
    """One 480 x 640 image under the 7 views of SCENE_VIEWS, Q = ceil((K + 24) / 7) queries per view.  The (view, query) rows are ranked
    g = q*7 + v, so that neighbouring ranks come from different views.  Every second rank sits on one of `centres` objects of about
    40 x 40 pixels in the region all views share, seen with a jitter of a few pixels and mostly with the object's class; the others
    are small scattered boxes inside their view.  The boxes are laid out in source pixels and written as each view's own normalised
    (and, for a mirrored view, mirrored) cxcywh.  One class per row carries a high logit falling with g, so the top K are roughly the
    first K ranks.  tests/test_detect_views_cpu.py checks that the reference suppresses 20 % .. 80 % of the selected candidates for every
    entry of NMS_CASES.  Returns (det, offsets, rects, flips, sizes)."""
    nv = len(SCENE_VIEWS)
    Q = -(-(K + 24) // nv)
    G = nv * Q
    u = synth.uniform01(seed, f"dv.cl.{K}", (G, 8))
    cen = synth.uniform01(seed + 1, f"dv.cen.{K}", (centres, 2)) * np.array([120.0, 80.0]) + np.array([260.0, 200.0])
    hot = synth.uniform01(seed + 3, f"dv.hot.{K}", (G, 2))
    lg = dc.safe_logits(seed + 2, (nv, Q, C), -7.0, 0.5)
    bx = np.zeros((nv, Q, 4), np.float32)
    for g in range(G):
        q, v = divmod(g, nv)
        (vl, vt, vw, vh), fl = SCENE_VIEWS[v]
        which = (g // 4) % centres
        member = g % 2 == 0
        if member:
            jit = (u[g, 4:8] - 0.5) * (0.8 if g < 8 else 8.0)                      # the first members agree closely: K = 4 sees a suppression
            X, Y, Wp, Hp = cen[which, 0] + jit[0], cen[which, 1] + jit[1], 40.0 + jit[2], 40.0 + jit[3]
        else:
            Wp, Hp = 3.0 + 6.0 * u[g, 2], 3.0 + 6.0 * u[g, 3]
            X, Y = vl + Wp + u[g, 0] * (vw - 2 * Wp), vt + Hp + u[g, 1] * (vh - 2 * Hp)
        xn = (X - vl) / vw
        bx[v, q] = (1.0 - xn if fl else xn, (Y - vt) / vh, Wp / vw, Hp / vh)
        own = member and (g < 8 or hot[g, 0] < 0.75)
        c = 1 + which % (C - 1) if own else 1 + int(hot[g, 0] * 997) % (C - 1)
        lg[v, q, c] = F(4.0 - 3.0 * g / G + (0.0 if g < 8 else 0.2 * (hot[g, 1] - 0.5)))
    rects = np.asarray([r for r, _ in SCENE_VIEWS], np.int32)
    flips = np.asarray([f for _, f in SCENE_VIEWS], np.uint8)
    return dc.pack(lg, bx), offsets_of([nv]), rects, flips, [tuple(float(x) for x in SCENE_HW)]


EDGE_MARGIN = 6.0


def edge_case(seed=70):
    """3 images x (5, 7, 4) views of make_views, random boxes: with EDGE_MARGIN a share of the rows between 10 % and 90 % is cut
    (tests/test_detect_views_cpu.py checks it), at every one of the four kinds of inner border"""
    return make_case(seed, [5, 7, 4], 40, 6)


def ulp_above(x):
    """the spacing of float32 numbers at magnitude x"""
    return float(np.spacing(F(abs(x))))
