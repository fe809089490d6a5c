"""The numpy restatement of dod_fuse_views (tests/fuse_views_cases.py) against what it has a second definition for -- the merge without
NMS, mirrored views, float64 evaluation of the same clusters, hand-derived tie and coverage cases -- and the conditions the GPU tests
(tests/test_gpu_fuse_views.py) rely on in their inputs: the clustered scene really fuses, really lets the argmax decide, and really
tells the evolving fused box from the founder's.  No GPU."""
import functools
import re
import os

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import detect_cases as dc
from tests import detect_views_cases as dv
from tests import fuse_views_cases as fv

F = np.float32
OUTS = ("scores", "labels", "views", "queries", "boxes", "counts")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


@functools.lru_cache(maxsize=None)
def _scene(K):
    return dv.clustered_views(K)


@functools.lru_cache(maxsize=None)
def _fused(K, iou, agnostic, conf=fv.AVG, match_box="fused"):
    case = _scene(K)
    return fv.fuse_views_ref(case[0], 5, K, *case[1:], iou=iou, class_agnostic=agnostic, conf=conf, match_box=match_box)


def test_binding_and_header_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    assert "int dod_fuse_views(" in hdr and "size_t dod_fuse_views_workspace_bytes(int V, int Q, int C, int K);" in hdr
    decl = re.search(r"int dod_fuse_views\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(nat.SYMBOLS["dod_fuse_views"][1]) == len(nat.SYMBOLS["dod_detect_views"][1]) + 1
    assert "nms_metric" not in decl and "int conf" in decl and "int32_t* members" in decl
    L = nat.lib()
    assert L.dod_fuse_views_workspace_bytes(7, 30, 5, 100) == L.dod_detect_views_workspace_bytes(7, 30, 5, 100) > 0
    assert L.dod_fuse_views_workspace_bytes(7, 30, 5, 1025) == 0


@pytest.mark.parametrize("kind,counts,Q,C,K", [("random", (3, 0, 2), 9, 5, 40), ("ties", (4, 1), 12, 4, 30), ("special", (2, 3), 20, 6, 64)])
def test_no_match_equals_merge_without_nms(kind, counts, Q, C, K):
    """iou = 1.0 can never match (inter <= union): one member per cluster; "max" is the merge without NMS bit for bit, "avg" differs in
    the scores only, by the stated formula, and in the order they induce"""
    case = dv.make_case(51, list(counts), Q, C, kind)
    for clamp, margin in [(True, 0.0), (False, dv.EDGE_MARGIN)]:
        plain = dv.detect_views_ref(case[0], C, K, *case[1:], clamp=clamp, edge_margin=margin)
        mx = fv.fuse_views_ref(case[0], C, K, *case[1:], iou=1.0, clamp=clamp, edge_margin=margin, conf=fv.MAX)
        for k in OUTS:
            assert np.array_equal(_bits(mx[k]), _bits(plain[k])), k
        pad = np.arange(K)[None, :] >= plain["counts"][:, None]
        assert np.all(mx["members"][~pad] == 1) and not mx["members"][pad].any()
        av = fv.fuse_views_ref(case[0], C, K, *case[1:], iou=1.0, clamp=clamp, edge_margin=margin, conf=fv.AVG)
        assert np.array_equal(av["counts"], plain["counts"])
        for b in range(len(counts)):
            n, order = int(plain["counts"][b]), av["info"][b]["order"]
            if not n:
                continue
            vr = case[2][case[1][b]:case[1][b + 1]]
            hw = dc.size_rows(case[4], len(counts))[b]
            N = np.asarray([max(1, fv.covering_views(plain["boxes"][b, i], vr, margin, hw)) for i in range(n)])
            want = np.asarray([F(s / F(1.0)) if 1 >= d else F(F(F(s / F(1.0)) * F(1.0)) / F(d)) for s, d in zip(plain["scores"][b, :n], N)], np.float32)
            assert np.array_equal(av["scores"][b, :n].view(np.uint32), want[order].view(np.uint32))
            assert np.all(np.diff(av["scores"][b, :n]) <= 0)
            for k in ("labels", "views", "queries"):
                assert np.array_equal(av[k][b, :n], plain[k][b, :n][order])
            assert np.array_equal(av["boxes"][b, :n].view(np.uint32), plain["boxes"][b, :n][order].view(np.uint32))


def test_mirrored_views_of_mirrored_boxes_fuse_to_the_same():
    """dyadic boxes and power-of-two views: 1 - x is exact, so the mirrored scene must give the plain scene's bits"""
    views = [((0, 0, 256, 128), 0), ((0, 0, 128, 128), 0), ((128, 0, 128, 128), 0)]
    rng = np.random.default_rng(5)
    entries = []
    for g in range(40):
        v = g % 3
        vl = views[v][0][0]
        x1, y1 = vl + int(rng.integers(0, 24)) * 4, int(rng.integers(0, 24)) * 4
        entries.append((v, 1 + g % 2, 3.0 - 0.1 * g, (x1, y1, x1 + 24 + 4 * int(rng.integers(0, 3)), y1 + 28)))
    plain = fv.scene_from_pixels((128, 256), views, entries)
    mirrored = fv.scene_from_pixels((128, 256), [(r, 1) for r, _ in views], entries)
    assert not np.array_equal(plain[0], mirrored[0])
    for conf in (fv.MAX, fv.AVG):
        a = fv.fuse_views_ref(plain[0], 4, 40, *plain[1:], iou=0.3, conf=conf)
        b = fv.fuse_views_ref(mirrored[0], 4, 40, *mirrored[1:], iou=0.3, conf=conf)
        assert 0 < a["counts"][0] < 40 and a["members"].max() >= 3
        for k in OUTS + ("members",):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("n", [4, 64, 1024])
def test_identical_boxes_fuse_to_that_box(n):
    case = fv.stacked_case(n)
    r = fv.fuse_views_ref(case[0], 3, n, *case[1:], iou=0.5)
    assert r["counts"][0] == 1 and r["members"][0, 0] == n and r["views"][0, 0] == 0 and r["queries"][0, 0] == 0
    box = np.asarray([4, 4, 28, 28], np.float64)
    assert np.all(np.abs(r["boxes"][0, 0] - box) <= (n + 3) * 2.0 ** -24 * box)
    assert r["divisor"][0, 0] == 4 and n >= 4
    s = r["info"][0]["scores"].astype(np.float64)
    assert abs(r["scores"][0, 0] - s.mean()) <= (n + 2) * 2.0 ** -24 * s.mean()


@pytest.mark.parametrize("K,iou,agnostic", [(100, 0.5, False), (512, 0.7, False), (513, 0.5, True), (1024, 0.7, True)])
def test_fused_boxes_against_float64(K, iou, agnostic):
    """the same clusters (the restatement's assignment) summed in float64: per coordinate the fp32 box lies within
    (T + 3) * 2^-24 * sum s|x| / sum s -- T rounded products summed recursively, the denominator's sum, the division"""
    r = _fused(K, iou, agnostic)
    info = r["info"][0]
    s, bx, cl = info["scores"].astype(np.float64), info["boxes"].astype(np.float64), info["clusters"]
    hi = np.asarray([640.0, 480.0, 640.0, 480.0])
    worst = 0.0
    for c in range(len(cl["members"])):
        mem = np.flatnonzero(cl["assign"] == c)
        assert len(mem) == cl["members"][c] and mem[0] == cl["founder"][c]
        want = np.clip((s[mem, None] * bx[mem]).sum(0) / s[mem].sum(), 0.0, hi)
        bound = (len(mem) + 3) * 2.0 ** -24 * (s[mem, None] * np.abs(bx[mem])).sum(0) / s[mem].sum()
        err = np.abs(cl["box"][c].astype(np.float64) - want)
        if len(mem) > 1:
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (c, err, bound)
        else:
            assert np.array_equal(cl["box"][c], info["boxes"][mem[0]])
    print(f"largest error / bound {worst:.3f}")


def test_tie_goes_to_the_earlier_cluster():
    case = fv.tie_case()
    r = fv.fuse_views_ref(case[0], 4, 3, *case[1:], iou=0.3, conf=fv.MAX)
    info = r["info"][0]
    assert np.array_equal(info["boxes"], np.asarray([[0, 0, 10, 10], [10, 0, 20, 10], [5, 0, 15, 10]], np.float32))
    assert F(50.0) > F(0.3) * F(150.0)
    assert info["clusters"]["matches"].tolist() == [0, 0, 2] and info["clusters"]["assign"].tolist() == [0, 1, 0]
    assert r["counts"][0] == 2 and r["members"][0, :2].tolist() == [2, 1]
    assert np.array_equal(r["boxes"][0, 1], np.asarray([10, 0, 20, 10], np.float32)) and 0 < r["boxes"][0, 0, 0] < 5


@pytest.mark.parametrize("margin", [0.0, fv.COVER_MARGIN])
def test_coverage_counts_and_avg_scores(margin):
    case = fv.coverage_case()
    K = sum(len(e[3]) for e in fv.COVER_EXPECT.values())
    r = fv.fuse_views_ref(case[0], 4, K, *case[1:], iou=0.5, edge_margin=margin, conf=fv.AVG)
    assert r["selected"][0] == K and r["counts"][0] == len(fv.COVER_EXPECT)
    seen = {}
    for i in range(r["counts"][0]):
        name = [k for k, b in fv.COVER_BOXES.items() if np.abs(r["boxes"][0, i] - np.asarray(b, np.float32)).max() < 1e-3]
        assert len(name) == 1                                             # identical boxes fuse to themselves within rounding
        seen[name[0]] = i
    assert set(seen) == set(fv.COVER_EXPECT)
    branches = set()
    for name, (lab, n0, n1, reports) in fv.COVER_EXPECT.items():
        i = seen[name]
        N, T = (n1 if margin > 0 else n0), len(reports)
        assert r["labels"][0, i] == lab and r["members"][0, i] == T and r["divisor"][0, i] == N, name
        s = dc.sigmoid32(np.asarray([lg for _, lg in reports], np.float32))
        tot = s[0]
        for x in s[1:]:
            tot = F(tot + x)
        mean = F(tot / F(T))
        want = mean if T >= N else F(F(mean * F(T)) / F(N))
        assert r["scores"][0, i] == want, name
        branches.add("T>N" if T > N else "T=N" if T == N else "T<N")
        assert r["views"][0, i] == reports[0][0], name                  # the founder's: the highest logit
    assert branches == {"T>N", "T=N", "T<N"}
    assert np.all(np.diff(r["scores"][0, :r["counts"][0]]) <= 0)
    mx = fv.fuse_views_ref(case[0], 4, K, *case[1:], iou=0.5, edge_margin=margin, conf=fv.MAX)
    assert np.array_equal(mx["scores"][0, :5], dc.sigmoid32(np.asarray([4.0, 3.5, 2.5, 1.0, 0.0], np.float32)))


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("iou", [0.5, 0.7])
@pytest.mark.parametrize("K", dv.NMS_KS)
def test_clustered_scene_discriminates(K, iou, agnostic):
    """conditions on the GPU tests' inputs, so that the scene cannot silently lose them"""
    r = _fused(K, iou, agnostic)
    cl = r["info"][0]["clusters"]
    n = int(r["selected"][0])
    assert n == K
    in_groups = int(cl["members"][cl["members"] >= 2].sum())
    assert 0.2 * n <= in_groups <= 0.8 * n, in_groups / n
    if K >= 100:
        T, N = r["members"][0, :r["counts"][0]], r["divisor"][0, :r["counts"][0]]
        assert (T > N).any() and (T < N).any()
        views = r["info"][0]["views"]
        assert any(len(set(views[cl["assign"] == c].tolist())) < cl["members"][c] for c in range(len(cl["members"])))
    if iou == 0.7 and K >= 100:
        assert (cl["matches"] >= 2).sum() >= 1                          # the argmax decides
        other = _fused(K, iou, agnostic, fv.AVG, "founder")["info"][0]["clusters"]["assign"]
        assert (other != cl["assign"]).sum() >= 1                       # a kernel that never (or late) updates the fused box fails
    mx = _fused(K, iou, agnostic, fv.MAX)
    assert np.all(np.diff(mx["scores"][0, :mx["counts"][0]]) <= 0)      # founding order is descending in score


def test_restatement_is_quick():
    import time
    t = time.perf_counter()
    case = _scene(1024)
    fv.fuse_views_ref(case[0], 5, 1024, *case[1:], iou=0.6, class_agnostic=True, conf=fv.MAX)
    assert time.perf_counter() - t < 5.0


def test_python_argument_errors_without_a_gpu():
    from dinov2_od_amd import slicing as sl
    counts, Q, C = (2, 1), 6, 4
    det_np, offsets, rects, flips, sizes = dv.make_case(52, list(counts), Q, C)
    det, plan = torch.from_numpy(det_np), sl.ViewPlan(offsets, rects, flips)
    assert issubclass(sl.FusedDetections, sl.SlicedDetections) and sl.FUSE_CONFS == {"max": fv.MAX, "avg": fv.AVG}
    bad = [(dict(merge="wbf"), "merge must"), (dict(merge="fuse", fuse_conf="mean"), "fuse_conf"), (dict(merge="fuse", nms_metric="ios"), "IoU only"),
           (dict(merge="fuse", nms_iou=None), "needs nms_iou"), (dict(merge="fuse", top_k=1025), "top_k")]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            sl.detect_views_packed(det, C, plan, sizes, **kw)
    for kw in (dict(merge="fuse"), dict(merge="fuse", fuse_conf="max"), dict(merge="nms"), dict()):
        with pytest.raises(ValueError, match="no CPU fallback"):          # every argument passed: only the device is missing
            sl.detect_views_packed(det, C, plan, sizes, **kw)
