"""dod_fuse_views (include/dinodet.h) restated in numpy, and the hand-built inputs of tests/test_fuse_views_cpu.py and
tests/test_gpu_fuse_views.py.

Stages 0 - 4 (edge filter, selection and order, score, label, view, query, box in source pixels) are dod_detect_views' and are taken
from its restatement with NMS off (tests/detect_views_cases.py).  What follows is the header to the letter: one pass over the sorted
candidates, each joining the cluster whose current fused box it overlaps best or founding one; five running fp32 sums per cluster;
the fused box re-divided (and re-clamped) after every member; the coverage count N over the image's views; the "max" and "avg"
scores; the output order.  The loop over clusters is vectorised: numpy's float32 array operations round as the scalar ones do.
"""
import numpy as np

from tests import detect_cases as dc
from tests import detect_views_cases as dv

F = np.float32
MAX, AVG = 0, 1                       # dod_fuse_views' conf, as slicing.FUSE_CONFS names them


def _area(b):
    z = F(0.0)
    return (dc._max(z, b[..., 2] - b[..., 0]) * dc._max(z, b[..., 3] - b[..., 1])).astype(np.float32)


def covering_views(f, rects, margin, hw):
    """how many of the image's views (rects [nv, 4]) cover the fused box f [4]; hw = (height, width) of the source image"""
    n = 0
    with np.errstate(invalid="ignore"):
        for rect in rects:
            vl, vt, vw, vh = (int(x) for x in rect)
            inside = f[0] >= F(vl) and f[1] >= F(vt) and f[2] <= F(vl + vw) and f[3] <= F(vt + vh)
            if inside and not dv.edge_cut(f[None, :], rect, margin, hw)[0]:
                n += 1
    return n


def fuse_image(sc, lab, bx, iou, class_agnostic, clamp, hw, match_box="fused"):
    """The pass over one image's n sorted candidates (scores sc [n], labels lab [n], boxes bx [n, 4], all final).  Returns the
    clusters in founding order: {"box" [m, 4], "sums" [m, 5], "label", "members", "founder" [m], "assign" [n] (the cluster every
    candidate went to), "matches" [n] (how many clusters it matched)}.  match_box="founder" is NOT the contract: it matches against the
    founder's box instead of the evolving fused box, for the tests that show the inputs tell the two apart."""
    n = len(sc)
    kbox, kcmp, ksum = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 5), np.float32)
    karea, klab, kT, kfirst = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assign, matches = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ih, iw = F(hw[0]), F(hw[1])
    can = iou is not None and iou >= 0
    z, m = F(0.0), 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(n):
            s, b, l = F(sc[i]), bx[i], lab[i]
            ab = _area(b)
            j = -1
            if can and m:
                f = kcmp[:m]
                w = dc._max(z, dc._min(f[:, 2], b[2]) - dc._max(f[:, 0], b[0]))
                h = dc._max(z, dc._min(f[:, 3], b[3]) - dc._max(f[:, 1], b[1]))
                inter = (w * h).astype(np.float32)
                uni = ((karea[:m] + ab).astype(np.float32) - inter).astype(np.float32)
                hit = inter > (F(iou) * uni).astype(np.float32)
                if not class_agnostic:
                    hit &= klab[:m] == l
                idx = np.flatnonzero(hit)
                matches[i] = len(idx)
                if len(idx):
                    q = (inter[idx] / uni[idx]).astype(np.float32)
                    assert not np.isnan(q).any()
                    j = int(idx[np.argmax(q)])                         # the first largest: equal quotients go to the lowest cluster
            if j < 0:
                j, m = m, m + 1
                ksum[j, :4], ksum[j, 4] = (s * b).astype(np.float32), s
                kbox[j], kcmp[j], karea[j], klab[j], kT[j], kfirst[j] = b, b, ab, l, 1, i
            else:
                ksum[j, :4] = (ksum[j, :4] + (s * b).astype(np.float32)).astype(np.float32)
                ksum[j, 4] = ksum[j, 4] + s
                f = (ksum[j, :4] / ksum[j, 4]).astype(np.float32)
                if clamp:
                    f = np.stack([dc._clamp(f[0], iw), dc._clamp(f[1], ih), dc._clamp(f[2], iw), dc._clamp(f[3], ih)]).astype(np.float32)
                kbox[j] = f
                kT[j] += 1
                if match_box == "fused":
                    kcmp[j], karea[j] = f, _area(f)
            assign[i] = j
    return {"box": kbox[:m], "sums": ksum[:m], "label": klab[:m], "members": kT[:m], "founder": kfirst[:m], "assign": assign, "matches": matches}


def fused_scores(cl, sc, rects, margin, hw, conf):
    """the clusters' scores and the divisor N of every cluster"""
    m = len(cl["members"])
    N = np.asarray([max(1, covering_views(cl["box"][c], rects, margin, hw)) for c in range(m)], np.int32).reshape(m)
    if conf == MAX:
        return np.asarray(sc, np.float32)[cl["founder"]], N
    out = np.zeros(m, np.float32)
    for c in range(m):
        T = int(cl["members"][c])
        mean = F(cl["sums"][c, 4] / F(T))
        out[c] = mean if T >= N[c] else F(F(mean * F(T)) / F(N[c]))
    return out, N


def fuse_views_ref(det, C, K, offsets, rects, flips, sizes, first_class=1, threshold=-1.0, iou=0.5, class_agnostic=False, clamp=True,
                   edge_margin=0.0, conf=AVG, scores=None, match_box="fused", base=None):
    """the whole call: {"scores" [B,K] f32, "labels", "views", "queries", "members" [B,K] i32, "boxes" [B,K,4] f32, "counts" [B] i32,
    "selected" [B], "divisor" [B,K] i32 (N of every row, 0 in padding) and "info" [B]: per image the candidates (detect_views_ref's
    rows with NMS off) and fuse_image's clusters}.  scores [B, K]: the candidates' scores to fuse in place of this file's sigmoid --
    the device's expf is not numpy's to the last bit, and everything after stage 4 is a function of the scores' bits.  base: the result
    of detect_views_ref(..., iou=None) for the same arguments, if the caller has it."""
    if base is None:
        base = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, first_class, threshold, None, 0, False, clamp, edge_margin)
    B = len(offsets) - 1
    hw = dc.size_rows(sizes, B)
    out = {"scores": np.zeros((B, K), np.float32), "labels": np.full((B, K), -1, np.int32), "views": np.full((B, K), -1, np.int32),
           "queries": np.full((B, K), -1, np.int32), "boxes": np.zeros((B, K, 4), np.float32), "members": np.zeros((B, K), np.int32),
           "counts": np.zeros(B, np.int32), "selected": base["selected"], "divisor": np.zeros((B, K), np.int32), "info": []}
    for b in range(B):
        n = int(base["counts"][b])
        sc = (base["scores"] if scores is None else np.asarray(scores, np.float32))[b, :n]
        lab, bx = base["labels"][b, :n], base["boxes"][b, :n]
        cl = fuse_image(sc, lab, bx, iou, class_agnostic, clamp, hw[b], match_box)
        vr = np.asarray(rects).reshape(-1, 4)[int(offsets[b]):int(offsets[b + 1])]
        fs, N = fused_scores(cl, sc, vr, edge_margin, hw[b], conf)
        m = len(fs)
        order = np.arange(m) if conf == MAX else np.argsort(-fs, kind="stable")          # ties by cluster number
        fo = cl["founder"][order]
        out["counts"][b] = m
        out["scores"][b, :m], out["labels"][b, :m], out["boxes"][b, :m], out["members"][b, :m] = fs[order], cl["label"][order], cl["box"][order], cl["members"][order]
        out["views"][b, :m], out["queries"][b, :m], out["divisor"][b, :m] = base["views"][b, :n][fo], base["queries"][b, :n][fo], N[order]
        out["info"].append({"scores": sc, "labels": lab, "boxes": bx, "views": base["views"][b, :n], "clusters": cl, "order": order})
    return out


# ------------------------------------------------------------------------------------------------ inputs
def scene_from_pixels(hw, views, entries, C=4):
    """One image of hw = (height, width) under `views` = [((left, top, width, height), flip)], Q = the largest number of entries of a
    view.  entries: (view, label, logit, (x1, y1, x2, y2) in source pixels); every box is written as its view's normalised (for a
    mirrored view, mirrored) cxcywh.  With power-of-two extents and integer corners every step is exact in fp32.  Unused rows carry
    logit -30 everywhere.  Returns (det, offsets, rects, flips, sizes)."""
    nv = len(views)
    per = [[e for e in entries if e[0] == v] for v in range(nv)]
    Q = max(1, max(len(p) for p in per))
    lg = np.full((nv, Q, C), -30.0, np.float32)
    bx = np.zeros((nv, Q, 4), np.float32)
    bx[..., :2], bx[..., 2:] = 0.5, 0.25
    for v, p in enumerate(per):
        (vl, vt, vw, vh), fl = views[v]
        for q, (_, lab, logit, (x1, y1, x2, y2)) in enumerate(p):
            cx, cy, w, h = (0.5 * (x1 + x2) - vl) / vw, (0.5 * (y1 + y2) - vt) / vh, (x2 - x1) / vw, (y2 - y1) / vh
            bx[v, q] = (1.0 - cx if fl else cx, cy, w, h)
            lg[v, q, lab] = logit
    rects = np.asarray([r for r, _ in views], np.int32)
    flp = np.asarray([f for _, f in views], np.uint8)
    return dc.pack(lg, bx), dv.offsets_of([nv]), rects, flp, [(float(hw[0]), float(hw[1]))]


def tie_case():
    """founders [0,0,10,10] and [10,0,20,10] of one label and a candidate [5,0,15,10]: both quotients are 50 / 150 in exact fp32, and at
    iou = 0.3 both match (50 > 0.3f * 150)"""
    views = [((0, 0, 64, 64), 0)]
    return scene_from_pixels((64, 64), views, [(0, 1, 3.0, (0, 0, 10, 10)), (0, 1, 2.0, (10, 0, 20, 10)), (0, 1, 1.0, (5, 0, 15, 10))])


# a 128 x 256 image: the whole image, tile A = x 0..128, tile B = x 64..192 (both borders inner), and the mirrored tile M = x 128..256
COVER_HW = (128, 256)
COVER_VIEWS = [((0, 0, 256, 128), 0), ((0, 0, 128, 128), 0), ((64, 0, 128, 128), 0), ((128, 0, 128, 128), 1)]
COVER_MARGIN = 6.0
COVER_BOXES = {"overlap": (80, 40, 112, 72), "one_tile": (8, 8, 40, 40), "near_border": (100, 80, 126, 112), "mirrored": (200, 16, 232, 48),
               "twice": (16, 80, 48, 112)}
# name -> (label, the views that cover the box without / with COVER_MARGIN, the (view, logit) reports)
COVER_EXPECT = {
    "overlap": (1, 3, 3, [(0, 4.0), (1, 3.0), (2, 2.0)]),            # full, A, B cover it; all three report it: T = N
    "one_tile": (2, 2, 2, [(1, 3.5)]),                                # full and A cover it; only A reports it: T = 1 < N = 2
    "near_border": (3, 3, 2, [(0, 2.5), (2, 1.5)]),                   # x2 = 126 is within 6 of A's inner border at 128: A does not count
    "mirrored": (1, 2, 2, [(0, 1.0), (3, 0.5)]),                      # full and the mirrored tile
    "twice": (2, 2, 2, [(0, 0.0), (1, -0.5), (1, -1.0)]),             # A reports it twice: T = 3 > N = 2
}


def coverage_case():
    entries = [(v, lab, logit, COVER_BOXES[name]) for name, (lab, _, _, reports) in COVER_EXPECT.items() for v, logit in reports]
    return scene_from_pixels(COVER_HW, COVER_VIEWS, entries)


def stacked_case(n, C=3):
    """n candidates on one and the same box, from 4 views: a single cluster of n members"""
    views = [((0, 0, 64, 64), 0), ((0, 0, 64, 64), 1), ((0, 0, 32, 64), 0), ((0, 0, 64, 32), 0)]
    entries = [(g % 4, 1, 4.0 - 6.0 * g / n, (4, 4, 28, 28)) for g in range(n)]
    return scene_from_pixels((64, 64), views, entries, C)


def disjoint_case(n, C=3):
    """n candidates on a grid of disjoint 4 x 4 boxes of a 256 x 256 image, from 2 views: n clusters"""
    views = [((0, 0, 256, 256), 0), ((0, 0, 256, 256), 1)]
    entries = [(g % 2, 1, 4.0 - 6.0 * g / n, (8 * (g % 32), 8 * (g // 32), 8 * (g % 32) + 4, 8 * (g // 32) + 4)) for g in range(n)]
    return scene_from_pixels((256, 256), views, entries, C)
