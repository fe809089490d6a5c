"""GPU parity of weighted boxes fusion across views (dod_fuse_views) against its numpy restatement (tests/fuse_views_cases.py): scores,
labels, views, queries, members, counts and boxes BIT FOR BIT, padding rows exactly as specified, guard rows around every output
untouched.

One thing is taken from the device: the candidates' scores.  The sigmoid of stage 4 is expf on the device and numpy's exp in the
restatement, which agree to detect_cases.SCORE_TOL and not to the last bit, and everything after stage 4 -- sums, fused boxes, which
cluster a later candidate joins, the order of the "avg" scores -- is a function of the scores' bits.  So every comparison first runs
dod_detect_views without NMS on the same inputs, checks its rows against the restatement as tests/test_gpu_detect_views.py does
(labels, views, queries, counts, box bits exact; scores within SCORE_TOL), and hands those scores to the restatement.  Given them, the
fusion is compared bit for bit; a NaN must come out as a NaN in whatever bits the hardware gives it.

The inputs' own conditions (the clustered scene fuses, lets the argmax decide, tells the evolving box from the founder's) are asserted on
the CPU in tests/test_fuse_views_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import cases
from tests import detect_cases as dc
from tests import detect_views_cases as dv
from tests import fuse_views_cases as fv
from tests.guard_rows import buffers as _buffers, same as _same, shaped as _shaped, untouched as _untouched

pytestmark = pytest.mark.gpu
OUTS = ("scores", "labels", "views", "queries", "boxes", "members", "counts")
BASE = ("scores", "labels", "views", "queries", "boxes", "counts")
INVALID = 1                     # DOD_ERR_INVALID (include/dinodet.h)


@pytest.fixture(scope="module")
def sl():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from dinov2_od_amd import slicing
    return slicing


def _device(case):
    det, offsets, rects, flips, sizes = case
    B = len(offsets) - 1
    d = det if isinstance(det, torch.Tensor) else torch.from_numpy(det).cuda()
    return d, [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (offsets, rects.reshape(-1, 4), flips, dc.size_rows(sizes, B))]


def _run(case, C, K, first_class=1, threshold=-1.0, iou=0.5, class_agnostic=False, clamp=True, margin=0.0, conf=fv.AVG, stream=None, fuse=True):
    """dod_fuse_views (fuse=False: dod_detect_views without NMS) through the C ABI into guarded outputs -> dict of numpy arrays"""
    L = nat.lib()
    B, (V, Q, _) = len(case[1]) - 1, case[0].shape
    d, dev = _device(case)
    bufs = _buffers(B, K, OUTS if fuse else BASE)
    ws = torch.empty(L.dod_fuse_views_workspace_bytes(V, Q, C, K), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    s = torch.cuda.current_stream() if stream is None else stream
    head = (nat.ptr(d) if V else None, B, V, Q, C, nat.ptr(dev[0]), nat.ptr(dev[1]) if V else None, nat.ptr(dev[2]) if V else None, nat.ptr(dev[3]),
            first_class, float(threshold), K)
    with torch.cuda.stream(s):
        if fuse:
            nat.check(L.dod_fuse_views(*head, float(iou), int(class_agnostic), int(clamp), float(margin), int(conf), *(nat.ptr(bufs[k][1]) for k in OUTS),
                                       nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        else:
            nat.check(L.dod_detect_views(*head, -1.0, 0, 0, int(clamp), float(margin), *(nat.ptr(bufs[k][1]) for k in BASE), nat.ptr(ws), ws.numel(),
                                         nat.stream_ptr()))
    s.synchronize()
    _untouched(bufs)
    return _shaped(bufs, B, K)


def _eq(got, want, k):
    g, w = got[k], want[k]
    if g.dtype == np.float32:
        gn, wn = np.isnan(g), np.isnan(w)
        assert np.array_equal(gn, wn), f"{k}: NaN rows differ"
        g, w = np.where(gn, np.float32(0), g).view(np.uint32), np.where(wn, np.float32(0), w).view(np.uint32)
    assert np.array_equal(g, w), f"{k}: {int((g != w).sum())} of {g.size} differ"


def _candidate_scores(case, C, K, first_class, threshold, clamp, margin):
    """the device's stage-4 rows, checked against the restatement of dod_detect_views without NMS -> (their scores [B, K], that
    restatement's result)"""
    got = _run(case, C, K, first_class, threshold, clamp=clamp, margin=margin, fuse=False)
    det = case[0].cpu().numpy() if isinstance(case[0], torch.Tensor) else case[0]
    want = dv.detect_views_ref(det, C, K, *case[1:], first_class, threshold, None, 0, False, clamp, margin)
    for k in ("counts", "labels", "views", "queries", "boxes"):
        _eq(got, want, k)
    err = np.abs(got["scores"].astype(np.float64) - want["scores"].astype(np.float64)).max()
    assert err < dc.SCORE_TOL
    print(f"candidate scores: {int((got['scores'].view(np.uint32) != want['scores'].view(np.uint32)).sum())} of {got['scores'].size} differ from numpy's sigmoid in their bits, max {err:.3g}")
    return got["scores"], want


def _check(case, C, K, first_class=1, threshold=-1.0, iou=0.5, class_agnostic=False, clamp=True, margin=0.0, conf=fv.AVG, scores=None):
    """run, restate, compare everything; scores: _candidate_scores' pair for the same first five arguments; returns (got, want)"""
    if scores is None:
        scores = _candidate_scores(case, C, K, first_class, threshold, clamp, margin)
    det = case[0].cpu().numpy() if isinstance(case[0], torch.Tensor) else case[0]
    want = fv.fuse_views_ref(det, C, K, *case[1:], first_class, threshold, iou, class_agnostic, clamp, margin, conf, scores=scores[0], base=scores[1])
    got = _run(case, C, K, first_class, threshold, iou, class_agnostic, clamp, margin, conf)
    for k in ("counts", "members", "labels", "views", "queries", "boxes", "scores"):
        _eq(got, want, k)
    pad = np.arange(K)[None, :] >= want["counts"][:, None]
    assert np.all(got["scores"][pad].view(np.uint32) == 0) and np.all(got["labels"][pad] == -1) and np.all(got["views"][pad] == -1)
    assert np.all(got["queries"][pad] == -1) and not got["members"][pad].any() and not got["boxes"][pad].view(np.uint32).any()
    assert np.all(got["members"][~pad] >= 1)
    return got, want


@functools.lru_cache(maxsize=None)
def _case(seed, counts, Q, C, kind="random"):
    return dv.make_case(seed, list(counts), Q, C, kind)


@functools.lru_cache(maxsize=None)
def _scene(K):
    return dv.clustered_views(K)


@functools.lru_cache(maxsize=None)
def _scene_scores(K):
    return _candidate_scores(_scene(K), 5, K, 1, -1.0, True, 0.0)


@pytest.mark.parametrize("conf", [fv.MAX, fv.AVG])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("iou", [0.5, 0.7])
@pytest.mark.parametrize("K", dv.NMS_KS)
def test_clustered_scene_matches_restatement(sl, K, iou, agnostic, conf):
    """K crosses the wave (64), the 512 / 513 boundary of the NMS instances and reaches the 1024 limit"""
    got, want = _check(_scene(K), 5, K, 1, -1.0, iou, agnostic, True, 0.0, conf, scores=_scene_scores(K))
    n = int(got["members"].sum())
    assert n == K and 0.2 * K <= got["members"][got["members"] >= 2].sum() <= 0.8 * K


# (view counts per image, Q, C, K): test_gpu_detect_views.py's -- one candidate; ragged; images without views first, in the middle and
# last; the documented shape; 16 * 720 * 91 candidates, just under 2^20, at the largest K; more images than a wave has lanes
SHAPES = [((1,), 1, 2, 1), ((1, 5, 2), 7, 5, 4), ((3, 0, 1, 0), 9, 3, 5), ((0, 2, 0), 9, 3, 5), ((13, 13), 100, 91, 300), ((16,), 720, 91, 1024),
          ((1,) * 65, 9, 3, 5), ((2, 3), 37, 11, 257)]


@pytest.mark.parametrize("counts,Q,C,K", SHAPES)
def test_shapes_match_restatement(sl, counts, Q, C, K):
    """random boxes: mostly single-member clusters, up to K of them"""
    case = _case(41, counts, Q, C)
    for first, conf, agn in ((1, fv.AVG, True), (0, fv.MAX, False))[:1 if sum(counts) * Q * C > 500000 else 2]:      # the largest shape once
        got, want = _check(case, C, K, first, iou=0.4, class_agnostic=agn, conf=conf)
        assert np.array_equal(want["counts"] == 0, np.asarray(counts) == 0)
    if K >= 257:
        assert want["counts"].max() > 0.5 * K and want["members"].max() >= 2


@pytest.mark.parametrize("counts,Q,C,K", [((1, 5, 2), 7, 5, 4), ((13, 13), 100, 91, 300), ((3, 2), 40, 7, 33)])
def test_ties_across_views(sl, counts, Q, C, K):
    """quantised logits replicated over the views: equal scores everywhere, in the selection and in the "avg" order"""
    case = _case(42, counts, Q, C, "ties")
    for conf in (fv.MAX, fv.AVG):
        _check(case, C, K, iou=0.3, class_agnostic=True, conf=conf)


@pytest.mark.parametrize("threshold", [-1.0, 0.5])
def test_special_values(sl, threshold):
    """NaN and infinite logits, and NaN boxes: the restatement is the contract for whatever the arithmetic yields"""
    counts, Q, C, K = (3, 2), 50, 9, 120
    case = _case(43, counts, Q, C, "special")
    for first in (0, 1):
        scores = _candidate_scores(case, C, K, first, threshold, True, dv.EDGE_MARGIN)
        for conf in (fv.MAX, fv.AVG):
            _check(case, C, K, first, threshold, 0.3, True, True, dv.EDGE_MARGIN, conf, scores=scores)
    nanbox = (case[0].copy(),) + case[1:]
    nanbox[0][:, ::3, C:] = np.nan
    got, want = _check(nanbox, C, K, 1, threshold, 0.3, True, True, dv.EDGE_MARGIN, fv.AVG)
    assert np.isnan(want["boxes"]).any() and np.all(want["members"][np.isnan(want["boxes"]).any(-1)] == 1)
    infbox = (case[0].copy(),) + case[1:]
    infbox[0][:, ::4, C + 2] = np.inf
    infbox[0][:, 1::4, C] = -np.inf
    _check(infbox, C, K, 1, threshold, 0.3, True, False, 0.0, fv.AVG)


@pytest.mark.parametrize("n", [5, 100, 1024])
def test_one_cluster_of_all_candidates(sl, n):
    case = fv.stacked_case(n)
    for conf in (fv.MAX, fv.AVG):
        got, _ = _check(case, 3, n, iou=0.5, conf=conf)
        assert got["counts"][0] == 1 and got["members"][0, 0] == n


@pytest.mark.parametrize("n", [3, 65, 1024])
def test_all_candidates_disjoint(sl, n):
    case = fv.disjoint_case(n)
    for conf in (fv.MAX, fv.AVG):
        got, _ = _check(case, 3, n, iou=0.0, class_agnostic=True, conf=conf)
        assert got["counts"][0] == n and np.all(got["members"] == 1)


def test_tie_rule_and_coverage_cases(sl):
    got, _ = _check(fv.tie_case(), 4, 3, iou=0.3, conf=fv.MAX)
    assert got["counts"][0] == 2 and got["members"][0].tolist() == [2, 1, 0]
    K = sum(len(e[3]) for e in fv.COVER_EXPECT.values())
    for margin in (0.0, fv.COVER_MARGIN):
        for conf in (fv.MAX, fv.AVG):
            got, want = _check(fv.coverage_case(), 4, K, iou=0.5, margin=margin, conf=conf)
            assert got["counts"][0] == len(fv.COVER_EXPECT) and sorted(got["members"][0, :5].tolist()) == [1, 2, 2, 3, 3]


@pytest.mark.parametrize("margin", [0.0, dv.EDGE_MARGIN, 40.0])
@pytest.mark.parametrize("clamp", [True, False])
def test_clamp_and_edge_margin(sl, clamp, margin):
    case = dv.edge_case()
    C, K = case[0].shape[-1] - 4, 90
    for conf in (fv.MAX, fv.AVG):
        got, want = _check(case, C, K, iou=0.2, class_agnostic=True, clamp=clamp, margin=margin, conf=conf)
        assert want["members"].max() >= 2
    if not clamp and margin == 0.0:
        assert got["boxes"].min() < 0


def test_iou_one_is_the_merge_without_nms(sl):
    """inter <= union: nothing matches, and "max" gives dod_detect_views' own bits, scores included"""
    counts, Q, C, K = (4, 0, 3), 30, 7, 100
    case = _case(48, counts, Q, C)
    plain = _run(case, C, K, margin=dv.EDGE_MARGIN, fuse=False)
    for iou in (1.0, 2.5, -1.0, float("nan")):
        got = _run(case, C, K, iou=iou, margin=dv.EDGE_MARGIN, conf=fv.MAX)
        assert _same({k: got[k] for k in BASE}, plain)
        assert np.array_equal(got["members"], (np.arange(K)[None, :] < plain["counts"][:, None]).astype(np.int32))
    _check(case, C, K, iou=1.0, margin=dv.EDGE_MARGIN, conf=fv.AVG)


def test_repeatable_and_stream_independent(sl):
    big = _scene(1024)
    case = (torch.from_numpy(big[0]).cuda(),) + big[1:]
    for conf in (fv.MAX, fv.AVG):
        a = _run(case, 5, 1024, iou=0.5, conf=conf)
        b = _run(case, 5, 1024, iou=0.5, conf=conf)
        assert _same(a, b)
        torch.cuda.synchronize()
        assert _same(a, _run(case, 5, 1024, iou=0.5, conf=conf, stream=torch.cuda.Stream()))


def test_invalid_arguments_return_invalid_and_write_nothing(sl):
    L = nat.lib()
    counts, Q, C, K = (2, 1), 9, 4, 5
    case = _case(46, counts, Q, C)
    B, V = len(counts), int(sum(counts))
    d, t = _device(case)
    bufs = _buffers(B, K, OUTS)
    ws = torch.empty(L.dod_fuse_views_workspace_bytes(V, Q, C, K), dtype=torch.uint8, device="cuda")
    good = dict(det=nat.ptr(d), B=B, V=V, Q=Q, C=C, offs=nat.ptr(t[0]), rects=nat.ptr(t[1]), flips=nat.ptr(t[2]), sizes=nat.ptr(t[3]), first=1,
                thr=-1.0, K=K, iou=0.5, agn=0, clamp=1, margin=0.0, conf=1, ws=nat.ptr(ws), wsb=ws.numel())
    good.update({k: nat.ptr(bufs[k][1]) for k in OUTS})
    order = ["det", "B", "V", "Q", "C", "offs", "rects", "flips", "sizes", "first", "thr", "K", "iou", "agn", "clamp", "margin", "conf", *OUTS, "ws", "wsb"]

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return L.dod_fuse_views(*(a[k] for k in order), nat.stream_ptr())

    bad = [dict(det=None), dict(offs=None), dict(rects=None), dict(flips=None), dict(sizes=None), dict(ws=None), dict(wsb=ws.numel() - 1), dict(wsb=0),
           dict(B=0), dict(B=-1), dict(V=-1), dict(Q=0), dict(C=0), dict(K=0), dict(K=1025), dict(Q=1 << 11, C=(1 << 9) + 1),
           dict(first=-1), dict(first=C), dict(conf=2), dict(conf=-1), dict(boxes=nat.C.c_void_p(bufs["boxes"][1].data_ptr() + 4))]
    bad += [{k: None} for k in OUTS]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    _untouched(bufs, inside=True)
    W = L.dod_fuse_views_workspace_bytes
    assert W(V, Q, C, 0) == 0 and W(V, Q, C, 1025) == 0 and W(-1, Q, C, K) == 0 and W(0, Q, C, K) > 0
    assert W(16, 720, 91, 1024) == L.dod_detect_views_workspace_bytes(16, 720, 91, 1024)
    assert call() == 0                                                              # the good call, last: the outputs are written now
    torch.cuda.synchronize()
    _untouched(bufs)
    assert int(bufs["counts"][1].min()) > 0


def _named(r):
    return {k: getattr(r, k).cpu().numpy() for k in OUTS}


def test_detect_views_packed_fuse_forms(sl):
    from dinov2_od_amd import postprocess as pp
    counts, Q, C, K = (3, 2), 30, 6, 20
    case = _case(47, counts, Q, C)
    det = torch.from_numpy(case[0]).cuda()
    plan = sl.ViewPlan(*case[1:4])
    sizes = case[4]
    scores, _ = _candidate_scores(case, C, K, 1, 0.05, True, dv.EDGE_MARGIN)
    for p in (plan, sl.plan_to_device(plan, "cuda")):
        for name, conf in sl.FUSE_CONFS.items():
            r = sl.detect_views_packed(det, C, p, sizes, top_k=K, threshold=0.05, nms_iou=0.3, class_agnostic=True, edge_margin=dv.EDGE_MARGIN, merge="fuse",
                                       fuse_conf=name)
            assert isinstance(r, sl.FusedDetections) and isinstance(r, sl.SlicedDetections) and isinstance(r, pp.Detections)
            assert r._fields == ("scores", "labels", "boxes", "queries", "counts") and r.members.dtype == torch.int32 and r.members.is_cuda
            want = fv.fuse_views_ref(case[0], C, K, *case[1:], 1, 0.05, 0.3, True, True, dv.EDGE_MARGIN, conf, scores=scores)
            got = _named(r)
            for k in OUTS:
                _eq(got, want, k)
    lst = pp.detections_to_list(r)
    assert [len(x["scores"]) for x in lst] == want["counts"].tolist()
    nms = sl.detect_views_packed(det, C, plan, sizes, top_k=K, threshold=0.05, nms_iou=0.3, class_agnostic=True, edge_margin=dv.EDGE_MARGIN)
    assert type(nms) is sl.SlicedDetections and not hasattr(nms, "members")          # the default path is what it was
    for kw in (dict(merge="wbf"), dict(merge="fuse", fuse_conf="mean"), dict(merge="fuse", nms_metric="ios"), dict(merge="fuse", nms_iou=None)):
        with pytest.raises(ValueError):
            sl.detect_views_packed(det, C, plan, sizes, **kw)


def test_model_detect_sliced_fuse_end_to_end(sl):
    """model.detect_sliced(..., flip=True, merge="fuse") == the restatement applied to forward_packed_u8's own output"""
    from dinov2_od_amd import postprocess as pp, visualize
    from tests import augment_cases as ac, gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "bf16x3", "facebook/dinov2-small")
    imgs = [ac._rand(s, 140 + i) for i, s in enumerate([(300, 420), (150, 180), (333, 500)])]
    shapes = [im.shape[:2] for im in imgs]
    size, tile, C, Q, K = (224, 224), 200, 91, 25, 100
    plan = sl.plan_views(shapes, tile, 0.2, True, True, size=size, pairs=Q * C)
    with torch.no_grad():
        det = m.forward_packed_u8(sl.extract_views(imgs, plan, size)).clone()
    sizes = [(float(h), float(w)) for h, w in shapes]
    base = sl.detect_views_packed(det, C, plan, sizes, top_k=K, threshold=-1.0, nms_iou=None, edge_margin=4.0)
    ref = dv.detect_views_ref(det.cpu().numpy(), C, K, plan.offsets, plan.rects, plan.flips, sizes, 1, -1.0, None, 0, False, True, 4.0)
    for k in ("labels", "views", "queries"):
        assert np.array_equal(getattr(base, k).cpu().numpy(), ref[k])
    scores = base.scores.cpu().numpy()
    assert np.abs(scores.astype(np.float64) - ref["scores"]).max() < dc.SCORE_TOL
    for name, conf in sl.FUSE_CONFS.items():
        want = fv.fuse_views_ref(det.cpu().numpy(), C, K, plan.offsets, plan.rects, plan.flips, sizes, 1, -1.0, 0.5, True, True, 4.0, conf, scores=scores)
        r = m.detect_sliced(imgs, size=size, tile=tile, overlap=0.2, full_view=True, flip=True, top_k=K, threshold=-1.0, nms_iou=0.5, class_agnostic=True,
                            edge_margin=4.0, merge="fuse", fuse_conf=name)
        got = _named(r)
        for k in OUTS:
            _eq(got, want, k)
        print(f"{name}: clusters {want['counts'].tolist()}, largest {int(want['members'].max())}")
        assert want["counts"].min() > 0 and isinstance(r, sl.FusedDetections)
    canvas = torch.zeros(3, 333, 500, 3, dtype=torch.uint8, device="cuda")
    drawn = visualize.draw_detections(canvas, r, score_threshold=-1.0)
    assert tuple(drawn.shape) == (3, 333, 500, 3) and int(drawn.max()) > 0
    assert [len(d["scores"]) for d in pp.detections_to_list(r)] == want["counts"].tolist()
