"""The numpy restatement of dod_detect_views (tests/detect_views_cases.py) against what it has a second definition for, and the
conditions on the seeded inputs that keep the GPU tests from passing vacuously."""
import functools

import numpy as np
import pytest

from tests import detect_cases as dc
from tests import detect_views_cases as dv


@functools.lru_cache(maxsize=None)
def _scene(K):
    return dv.clustered_views(K)


@pytest.mark.parametrize("iou,agnostic", [(None, False), (0.5, False), (0.3, True)])
@pytest.mark.parametrize("threshold", [-1.0, 0.05])
def test_one_unflipped_full_view_per_image_is_dod_detect(threshold, iou, agnostic):
    """rect = (0, 0, W, H), no flip: `x * W` then `+ 0.0f` is dod_detect's `x * W` as a value (-0.0 may become +0.0)"""
    B, Q, C, K = 3, 40, 7, 50
    det = dc.random_det(31, B, Q, C)
    sizes = dv.image_sizes(B)
    rects = np.asarray([(0, 0, int(w), int(h)) for h, w in sizes], np.int32)
    for clamp in (True, False):
        for first in (0, 1):
            want = dc.detect_ref(det, C, K, first, sizes, threshold, iou, agnostic, clamp)
            got = dv.detect_views_ref(det, C, K, dv.offsets_of([1] * B), rects, np.zeros(B, np.uint8), sizes, first, threshold, iou, 0, agnostic, clamp, 5.0)
            for k in ("counts", "labels", "queries", "selected"):
                assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(got["boxes"], want["boxes"]) and np.array_equal(got["scores"], want["scores"])      # as values
            assert not got["cut"].any()                                      # every border is the image's own: the margin filters nothing
            n = got["counts"]
            assert all((got["views"][b, :n[b]] == 0).all() and (got["views"][b, n[b]:] == -1).all() for b in range(B))


def test_a_mirrored_view_of_mirrored_boxes_maps_back():
    """Input mirrored in the view (cx' = fl(1 - cx)) and the flip flag set, against the plain input.  The unmirrored x1 is one rounded
    operation, fl(cx - 0.5 w).  The mirrored path takes three: fl(1 - cx), fl(cx' + 0.5 w) and fl(1 - x2').  With cx in [0, 1] and w in
    [0, 1] every operand and result is below 2 in magnitude, so each rounding errs by at most half an ulp of [1, 2) = 2^-24: the two
    normalised x1 differ by at most 4 * 2^-24 = 2^-22, scaled by the view's width.  Each side then rounds `* vw` and `+ vl` once more, on
    results below P = 2^k: four roundings of at most 2^(k-24).  Bound per x coordinate: vw * 2^-22 + 2^(k-22).  y is untouched: bit-equal."""
    Q, C, K = 60, 5, 300
    counts = [4, 3]
    det, offsets, rects, flips, sizes = dv.make_case(32, counts, Q, C)
    u = np.abs(det[..., C:]) % 1.0
    det[..., C:] = u.astype(np.float32)                                     # cx, cy, w, h in [0, 1)
    mir = det.copy()
    mir[..., C] = np.float32(1.0) - det[..., C]
    a = dv.detect_views_ref(det, C, K, offsets, rects, np.zeros(len(rects), np.uint8), sizes, clamp=False)
    b = dv.detect_views_ref(mir, C, K, offsets, rects, np.ones(len(rects), np.uint8), sizes, clamp=False)
    for k in ("counts", "labels", "queries", "views", "scores"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["boxes"][..., 1::2].view(np.uint32), b["boxes"][..., 1::2].view(np.uint32))
    worst = 0.0
    for img in range(len(counts)):
        n = int(a["counts"][img])
        assert n == K
        vw = rects[offsets[img] + a["views"][img, :n], 2].astype(np.float64)
        k = np.ceil(np.log2(np.abs(a["boxes"][img, :n]).max() + 1.0))
        bound = vw * 2.0 ** -22 + 2.0 ** (k - 22)
        err = np.abs(a["boxes"][img, :n, 0::2].astype(np.float64) - b["boxes"][img, :n, 0::2].astype(np.float64)).max(axis=1)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound)
    print(f"worst error / bound {worst:.3g}")
    assert (a["boxes"] != b["boxes"]).any()                                 # the roundings do differ somewhere: the bound is exercised


def test_flip_moves_only_x_and_views_are_local():
    Q, C, K = 9, 4, 30
    det, offsets, rects, flips, sizes = dv.make_case(33, [3, 0, 2], Q, C)
    assert flips.min() == 0 and flips.max() == 1                            # mixed within the case
    r = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, clamp=False)
    assert r["counts"].tolist() == [min(K, 3 * Q * (C - 1)), 0, min(K, 2 * Q * (C - 1))]
    assert r["rows"].tolist() == [3 * Q, 0, 2 * Q]
    for b in (0, 2):
        n = r["counts"][b]
        assert r["views"][b, :n].min() >= 0 and r["views"][b, :n].max() == offsets[b + 1] - offsets[b] - 1
        for j in range(n):
            v, q = offsets[b] + r["views"][b, j], r["queries"][b, j]
            want = dv.view_boxes(det[v, q:q + 1, C:], rects[v], flips[v])[0]
            assert np.array_equal(r["boxes"][b, j], want)
            plain = dv.view_boxes(det[v, q:q + 1, C:], rects[v], 0)[0]
            assert np.array_equal(plain[1::2], want[1::2])
    assert (r["views"][1] == -1).all() and not r["boxes"][1].any()


def test_ties_across_views_go_by_view_then_query_then_class():
    Q, C, K = 7, 5, 4
    det, offsets, rects, flips, sizes = dv.make_case(34, [1, 5, 2], Q, C, "ties")
    r = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes)
    for b in range(3):
        n = int(r["counts"][b])
        v, q, c = r["views"][b, :n], r["queries"][b, :n], r["labels"][b, :n]
        lg = det[offsets[b] + v, q, c]
        assert np.all(np.diff(lg) <= 0)
        flat = (v.astype(np.int64) * Q + q) * C + c
        same = np.diff(lg) == 0
        assert np.all(np.diff(flat)[same] > 0)
    nv = 5
    cand = det[offsets[1]:offsets[2], :, 1:C].reshape(-1)
    last = det[offsets[1] + r["views"][1, K - 1], r["queries"][1, K - 1], r["labels"][1, K - 1]]
    taken = (det[offsets[1] + r["views"][1], r["queries"][1], r["labels"][1]] == last).sum()
    assert (cand == last).sum() > taken > 0 and (cand == last).sum() % nv == 0        # ties straddle the K-th position, view by view


# ------------------------------------------------------------------------- conditions on the inputs the GPU tests use
@pytest.mark.parametrize("K,iou,metric,agnostic", dv.NMS_CASES)
def test_clustered_views_are_suppressed_between_20_and_80_percent(K, iou, metric, agnostic):
    det, offsets, rects, flips, sizes = _scene(K)
    C = det.shape[-1] - 4
    r = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, 1, -1.0, iou, metric, agnostic, True)
    sel, kept = int(r["selected"].sum()), int(r["counts"].sum())
    assert sel == K
    frac = 1.0 - kept / sel
    print(f"K={K} iou={iou} metric={metric} agnostic={agnostic}: suppressed {frac:.2f}")
    assert 0.2 <= frac <= 0.8
    n = int(r["counts"][0])
    assert len(np.unique(r["views"][0, :n])) >= min(5, n)                             # survivors come from several views


def test_clusters_are_seen_from_several_views_and_metrics_differ():
    differ = 0
    for K in dv.NMS_KS:
        det, offsets, rects, flips, sizes = _scene(K)
        C = det.shape[-1] - 4
        a = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, 1, -1.0, 0.5, 0, False, True)
        b = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, 1, -1.0, 0.5, 1, False, True)
        differ += int(a["counts"][0] != b["counts"][0] or not np.array_equal(a["queries"], b["queries"]) or not np.array_equal(a["views"], b["views"]))
        assert b["counts"][0] <= a["counts"][0]                                       # IoS >= IoU: it never suppresses less on this scene
        plain = dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, 1, -1.0, None)
        big = (plain["boxes"][0, :, 2] - plain["boxes"][0, :, 0]) > 20                # the objects, not the scattered boxes
        assert len(np.unique(plain["views"][0][big])) >= min(5, big.sum())
    assert differ >= 1


def test_edge_filter_removes_between_10_and_90_percent_of_the_rows():
    det, offsets, rects, flips, sizes = dv.edge_case()
    C = det.shape[-1] - 4
    r = dv.detect_views_ref(det, C, 50, offsets, rects, flips, sizes, edge_margin=dv.EDGE_MARGIN)
    frac = r["cut"].sum() / r["rows"].sum()
    print(f"edge filter cuts {frac:.2f} of the rows")
    assert 0.1 <= frac <= 0.9
    off = dv.detect_views_ref(det, C, 50, offsets, rects, flips, sizes, edge_margin=0.0)
    assert not off["cut"].any() and not np.array_equal(off["queries"], r["queries"])
    # each of the four inner borders filters something, and a view border on the source border filters nothing
    hits = np.zeros(4, int)
    for b in range(len(sizes)):
        for v in range(offsets[b], offsets[b + 1]):
            bx = dv.view_boxes(det[v, :, C:], rects[v], flips[v])
            l, t, w, h = rects[v].tolist()
            H, W = sizes[b]
            for side, (inner, rect1) in enumerate([(l > 0, (l, 0, W - l, H)), (l + w < W, (0, 0, l + w, H)), (t > 0, (0, t, W, H - t)), (t + h < H, (0, 0, W, t + h))]):
                n = int(dv.edge_cut(bx, rect1, dv.EDGE_MARGIN, sizes[b]).sum())          # a view with this one inner border only
                assert inner or n == 0
                hits[side] += n
    assert hits.min() > 0
    # NaN boxes are never filtered: every comparison is false
    nan = det.copy()
    nan[..., C:] = np.nan
    assert not dv.detect_views_ref(nan, C, 50, offsets, rects, flips, sizes, edge_margin=dv.EDGE_MARGIN)["cut"].any()
