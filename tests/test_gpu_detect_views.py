"""GPU parity of the merge of sliced inference (dod_detect_views: top-k over all views of an image, boxes mapped into source pixels,
edge filter, optional NMS across views) against its numpy restatement (tests/detect_views_cases.py).  labels, views, queries, counts
and the padding rows are exact, boxes bit-equal, scores within the project's tolerance for this sigmoid (detect_cases.SCORE_TOL).
Every output sits between guard rows that must stay untouched.  The inputs' own conditions (suppression rates, the edge filter's
share, ties) are asserted on the CPU in tests/test_detect_views_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import cases
from tests import detect_cases as dc
from tests import detect_views_cases as dv
from tests import guard_rows as gr
from tests.guard_rows import same as _same, untouched as _untouched

pytestmark = pytest.mark.gpu
OUTS = ("scores", "labels", "views", "queries", "boxes", "counts")
INVALID = 1                     # DOD_ERR_INVALID (include/dinodet.h)


@pytest.fixture(scope="module")
def sl():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from dinov2_od_amd import slicing
    return slicing


def _run(case, C, K, first_class=1, threshold=-1.0, iou=None, metric=0, class_agnostic=False, clamp=True, margin=0.0, stream=None):
    """dod_detect_views through the C ABI into guarded outputs -> dict of numpy arrays shaped like detect_views_ref's"""
    det, offsets, rects, flips, sizes = case
    L = nat.lib()
    B, (V, Q, _) = len(offsets) - 1, det.shape
    d = det if isinstance(det, torch.Tensor) else torch.from_numpy(det).cuda()
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (offsets, rects.reshape(-1, 4), flips, dc.size_rows(sizes, B))]
    bufs = gr.buffers(B, K, OUTS)
    ws = torch.empty(L.dod_detect_views_workspace_bytes(V, Q, C, K), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        nat.check(L.dod_detect_views(nat.ptr(d) if V else None, B, V, Q, C, nat.ptr(dev[0]), nat.ptr(dev[1]) if V else None,
                                     nat.ptr(dev[2]) if V else None, nat.ptr(dev[3]), first_class, float(threshold), K,
                                     -1.0 if iou is None else float(iou), int(metric), int(class_agnostic), int(clamp), float(margin),
                                     *(nat.ptr(bufs[k][1]) for k in OUTS), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    s.synchronize()
    _untouched(bufs)
    return gr.shaped(bufs, B, K)


def _ref(case, C, K, first_class=1, threshold=-1.0, iou=None, metric=0, class_agnostic=False, clamp=True, margin=0.0):
    det, offsets, rects, flips, sizes = case
    return dv.detect_views_ref(det, C, K, offsets, rects, flips, sizes, first_class, threshold, iou, metric, class_agnostic, clamp, margin)


def _check(got, want, nan_boxes=False):
    """nan_boxes: the input holds NaN box coordinates -- a NaN must come out as a NaN, in whatever bits the hardware gives it"""
    if nan_boxes:
        gn, wn = np.isnan(got["boxes"]), np.isnan(want["boxes"])
        assert wn.any() and np.array_equal(gn, wn)
        got, want = dict(got, boxes=np.where(gn, np.float32(0), got["boxes"])), dict(want, boxes=np.where(wn, np.float32(0), want["boxes"]))
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["views"], want["views"])
    assert np.array_equal(got["queries"], want["queries"])
    assert np.array_equal(got["boxes"].view(np.uint32), want["boxes"].view(np.uint32))
    err = float(np.max(np.abs(got["scores"].astype(np.float64) - want["scores"].astype(np.float64))))
    print(f"max score error {err:.3g}")
    assert err < dc.SCORE_TOL
    K = got["scores"].shape[1]
    pad = np.arange(K)[None, :] >= want["counts"][:, None]
    assert np.all(got["scores"][pad] == 0.0) and np.all(got["labels"][pad] == -1) and np.all(got["views"][pad] == -1) and np.all(got["queries"][pad] == -1)
    assert not got["boxes"][pad].view(np.uint32).any()


@functools.lru_cache(maxsize=None)
def _case(seed, counts, Q, C, kind="random"):
    return dv.make_case(seed, list(counts), Q, C, kind)


@functools.lru_cache(maxsize=None)
def _scene(K):
    return dv.clustered_views(K)


# (view counts per image, Q, C, K): one candidate; ragged; images without views first, in the middle and last; the documented shape;
# 16 * 720 * 91 = 1 048 320 candidates, just under 2^20, at the largest K; more images than a wave has lanes
SHAPES = [((1,), 1, 2, 1), ((1, 5, 2), 7, 5, 4), ((3, 0, 1, 0), 9, 3, 5), ((0, 2, 0), 9, 3, 5), ((13, 13), 100, 91, 300), ((16,), 720, 91, 1024),
          ((1,) * 65, 9, 3, 5)]


@pytest.mark.parametrize("nms", [None, (0.5, 0), (0.5, 1)])
@pytest.mark.parametrize("counts,Q,C,K", SHAPES)
def test_shapes_match_restatement(sl, counts, Q, C, K, nms):
    case = _case(41, counts, Q, C)
    flips = case[3]
    if max(counts) >= 5:
        assert flips.min() == 0 and flips.max() == 1                                              # flips on and off within an image
        assert (case[2][:, :2] % 2 == 1).any() and (case[2][:, 2:] % 2 == 1).any()                # odd origins and extents
    kw = {} if nms is None else dict(iou=nms[0], metric=nms[1])
    for first in (1, 0):
        want = _ref(case, C, K, first, **kw)
        got = _run(case, C, K, first, **kw)
        _check(got, want)
        if nms is None:
            assert np.array_equal(want["counts"], [min(K, n * Q * (C - first)) for n in counts])


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("iou,agnostic", [(None, False), (0.5, False), (0.5, True)])
@pytest.mark.parametrize("B,Q,C,K", [(3, 9, 5, 4), (2, 7, 3, 64)])         # the second: fewer pairs than K, the pass without a select
def test_one_unflipped_full_view_per_image_is_dod_detect(sl, B, Q, C, K, iou, agnostic, clamp):
    """the kernels' statement of tests/test_detect_views_cpu.py's test of this name: both entry points end in the same tail
    (det_finish, csrc/detect_select.h), so with rect = (0, 0, W, H) and no flip counts, labels, queries and the bits of boxes and scores
    are dod_detect's, views is 0 in every valid row and -1 in the padding"""
    L = nat.lib()
    H, W = 37, 53
    det = dc.random_det(48, B, Q, C)
    case = (det, dv.offsets_of([1] * B), np.asarray([(0, 0, W, H)] * B, np.int32), np.zeros(B, np.uint8), [(float(H), float(W))] * B)
    got = _run(case, C, K, 1, -1.0, iou, 0, agnostic, clamp)
    names = ("scores", "labels", "queries", "boxes", "counts")
    bufs = gr.buffers(B, K, names)
    d, st = torch.from_numpy(det).cuda(), torch.from_numpy(dc.size_rows((H, W), B)).cuda()
    ws = torch.empty(L.dod_detect_workspace_bytes(B, Q, C, K), dtype=torch.uint8, device="cuda")
    nat.check(L.dod_detect(nat.ptr(d), B, Q, C, 1, nat.ptr(st), -1.0, K, -1.0 if iou is None else float(iou), int(agnostic), int(clamp),
                           *(nat.ptr(bufs[k][1]) for k in names), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    torch.cuda.synchronize()
    _untouched(bufs)
    want = gr.shaped(bufs, B, K)
    for k in names:
        assert _same({k: want[k]}, {k: got[k]}), k
    n = got["counts"]
    assert n.min() > 0 and (iou is not None or np.all(n == min(K, Q * (C - 1))))
    valid = np.arange(K)[None, :] < n[:, None]
    assert np.all(got["views"][valid] == 0) and np.all(got["views"][~valid] == -1)


@pytest.mark.parametrize("counts,Q,C,K", [((1, 5, 2), 7, 5, 4), ((13, 13), 100, 91, 300), ((3, 2), 40, 7, 33)])
def test_ties_across_views(sl, counts, Q, C, K):
    """quantised logits replicated over the views: the K-th position is straddled by ties that differ only in the view index"""
    case = _case(42, counts, Q, C, "ties")
    det, offsets = case[0], case[1]
    want = _ref(case, C, K)
    b = int(np.argmax(counts))
    sel = det[offsets[b] + want["views"][b], want["queries"][b], want["labels"][b]]
    cand = det[offsets[b]:offsets[b + 1], :, 1:C].reshape(-1)
    assert (cand == sel[-1]).sum() > (sel == sel[-1]).sum() > 0 and (cand == sel[-1]).sum() % counts[b] == 0
    _check(_run(case, C, K), want)
    _check(_run(case, C, K, iou=0.5, metric=1), _ref(case, C, K, iou=0.5, metric=1))
    flat = (det.copy(),) + case[1:]
    flat[0][..., :C] = -1.25                                                                       # every logit equal: pure index order
    want = _ref(flat, C, K)
    idx = (want["views"].astype(np.int64) * Q + want["queries"]) * C + want["labels"]
    assert all(np.all(np.diff(idx[i, :want["counts"][i]]) > 0) for i in range(len(counts)))
    _check(_run(flat, C, K), want)


@pytest.mark.parametrize("threshold", [-1.0, 0.5])
def test_special_values(sl, threshold):
    counts, Q, C, K = (3, 2), 50, 9, 120
    case = _case(43, counts, Q, C, "special")
    lg = case[0][..., :C]
    assert np.isnan(lg).sum() > 10 and np.isposinf(lg).sum() > 3 and np.isneginf(lg).sum() > 3 and (lg == 0).sum() > 6
    for first in (0, 1):
        for margin in (0.0, dv.EDGE_MARGIN):
            got = _run(case, C, K, first, threshold, margin=margin)
            _check(got, _ref(case, C, K, first, threshold, margin=margin))
            for b, n in enumerate(got["counts"]):
                assert not np.isnan(case[0][case[1][b] + got["views"][b, :n], got["queries"][b, :n], got["labels"][b, :n]]).any()
    allnan = (case[0].copy(),) + case[1:]
    allnan[0][..., :C] = np.nan
    got = _run(allnan, C, K, 0)
    assert not got["counts"].any()
    _check(got, _ref(allnan, C, K, 0))
    nanbox = (case[0].copy(),) + case[1:]
    nanbox[0][:, ::3, C:] = np.nan                                                                 # NaN boxes pass the edge filter and the clamp
    _check(_run(nanbox, C, K, 1, -1.0, 0.5, 1, True, True, dv.EDGE_MARGIN), _ref(nanbox, C, K, 1, -1.0, 0.5, 1, True, True, dv.EDGE_MARGIN), nan_boxes=True)


@pytest.mark.parametrize("threshold", [-1.0, 0.05, 0.5, 0.9])
def test_thresholds_and_counts(sl, threshold):
    counts, Q, C, K = (2, 1, 3), 15, 6, 40
    case = (dc.random_det(44, 6, Q, C, mean=-1.0, std=2.0),) + _case(44, counts, Q, C)[1:]
    want = _ref(case, C, K, 1, threshold)
    _check(_run(case, C, K, 1, threshold), want)
    if threshold == 0.9:
        assert np.all(want["counts"] < K) and want["counts"].min() > 0                             # fewer candidates than K: padding appears
    if threshold < 0:
        assert np.all(want["counts"] == K)


@pytest.mark.parametrize("margin", [0.0, dv.EDGE_MARGIN, 40.0])
@pytest.mark.parametrize("clamp", [True, False])
def test_clamp_and_edge_margin(sl, clamp, margin):
    """views touching each of the four source borders (make_views): the filter acts at inner borders only"""
    case = dv.edge_case()
    C, K = case[0].shape[-1] - 4, 90
    rects, sizes = case[2], case[4]
    assert (rects[:, 0] == 0).any() and (rects[:, 1] == 0).any() and (rects[:, 0] > 0).any() and (rects[:, 1] > 0).any()
    assert any(r[0] + r[2] == sizes[0][1] for r in rects[:5]) and any(r[1] + r[3] == sizes[0][0] for r in rects[:5])
    for kw in (dict(), dict(iou=0.5, metric=1, class_agnostic=True)):
        want = _ref(case, C, K, clamp=clamp, margin=margin, **kw)
        got = _run(case, C, K, clamp=clamp, margin=margin, **kw)
        _check(got, want)
    hw = dc.size_rows(sizes, len(sizes))
    if clamp:
        assert got["boxes"].min() >= 0 and np.all(got["boxes"][..., 0::2] <= hw[:, None, 1:2]) and np.all(got["boxes"][..., 1::2] <= hw[:, None, 0:1])
    elif margin == 0.0:
        assert got["boxes"].min() < 0
    if margin > 0:
        assert 0 < want["cut"].sum() < want["rows"].sum()
        assert not _same({k: got[k] for k in OUTS}, {k: _ref(case, C, K, clamp=clamp, **kw)[k] for k in OUTS})


@pytest.mark.parametrize("K,iou,metric,agnostic", dv.NMS_CASES)
def test_nms_across_views_matches_restatement(sl, K, iou, metric, agnostic):
    case = _scene(K)
    C = case[0].shape[-1] - 4
    want = _ref(case, C, K, 1, -1.0, iou, metric, agnostic, True)
    got = _run(case, C, K, 1, -1.0, iou, metric, agnostic, True)
    _check(got, want)
    assert 0.2 * K <= K - got["counts"].sum() <= 0.8 * K


def test_nms_on_random_views_with_threshold_and_margin(sl):
    counts, Q, C, K = (13, 13), 100, 91, 300
    case = _case(41, counts, Q, C)
    for iou, metric, agn, thr, margin in [(0.5, 0, False, -1.0, 0.0), (0.3, 1, True, 0.05, dv.EDGE_MARGIN), (0.0, 0, True, -1.0, 2.5)]:
        _check(_run(case, C, K, 1, thr, iou, metric, agn, True, margin), _ref(case, C, K, 1, thr, iou, metric, agn, True, margin))


def test_nms_identical_boxes_from_different_views(sl):
    """the same source box seen unmirrored and mirrored from two views: only the first survives; a zero-area box neither suppresses nor
    is suppressed under IoU, and under the smaller-box rule `inter > t * 0` is false for it too"""
    C = 3
    det = np.zeros((2, 3, C + 4), np.float32)
    det[..., :C] = -9.0
    det[0, :, 1] = [5.0, 3.0, 1.0]
    det[1, :, 1] = [4.0, 2.0, 0.5]
    det[0, :, C:] = [[.5, .5, .25, .25], [.25, .5, 0.0, .25], [.125, .125, .125, .125]]
    det[1, :, C:] = [[.5, .5, .25, .25], [.75, .5, 0.0, .25], [.875, .125, .125, .125]]         # view 1 mirrors view 0's x: 1 - x
    case = (det, dv.offsets_of([2]), np.asarray([(0, 0, 64, 64), (0, 0, 64, 64)], np.int32), np.asarray([0, 1], np.uint8), [(64.0, 64.0)])
    for iou, metric in [(0.0, 0), (0.5, 0), (0.5, 1)]:
        got = _run(case, C, 6, 1, -1.0, iou, metric)
        _check(got, _ref(case, C, 6, 1, -1.0, iou, metric))
        assert got["counts"][0] == 4
        assert list(zip(got["views"][0, :4].tolist(), got["queries"][0, :4].tolist())) == [(0, 0), (0, 1), (1, 1), (0, 2)]


def test_repeatable_and_stream_independent(sl):
    counts, Q, C, K = (4, 3, 5, 1), 100, 91, 100
    det, offsets, rects, flips, sizes = _case(45, counts, Q, C, "ties")
    case = (torch.from_numpy(det).cuda(), offsets, rects, flips, sizes)
    for kw in (dict(), dict(iou=0.5, metric=1, margin=dv.EDGE_MARGIN)):
        a = _run(case, C, K, 1, 0.05, **kw)
        b = _run(case, C, K, 1, 0.05, **kw)
        assert _same(a, b)
        torch.cuda.synchronize()
        c = _run(case, C, K, 1, 0.05, stream=torch.cuda.Stream(), **kw)
        assert _same(a, c)
    big = _scene(1024)
    a = _run(big, 5, 1024, iou=0.5, metric=1)
    torch.cuda.synchronize()
    assert _same(a, _run(big, 5, 1024, iou=0.5, metric=1, stream=torch.cuda.Stream()))


def test_invalid_arguments_return_invalid_and_write_nothing(sl):
    L = nat.lib()
    counts, Q, C, K = (2, 1), 9, 4, 5
    det, offsets, rects, flips, sizes = _case(46, counts, Q, C)
    B, V = len(counts), int(sum(counts))
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (det, offsets, rects, flips, dc.size_rows(sizes, B))]
    bufs = gr.buffers(B, K, OUTS)
    ws = torch.empty(L.dod_detect_views_workspace_bytes(V, Q, C, K), dtype=torch.uint8, device="cuda")
    good = dict(det=nat.ptr(t[0]), B=B, V=V, Q=Q, C=C, offs=nat.ptr(t[1]), rects=nat.ptr(t[2]), flips=nat.ptr(t[3]), sizes=nat.ptr(t[4]), first=1,
                thr=-1.0, K=K, iou=0.5, metric=0, agn=0, clamp=1, margin=0.0, ws=nat.ptr(ws), wsb=ws.numel())
    good.update({k: nat.ptr(bufs[k][1]) for k in OUTS})
    order = ["det", "B", "V", "Q", "C", "offs", "rects", "flips", "sizes", "first", "thr", "K", "iou", "metric", "agn", "clamp", "margin", *OUTS, "ws", "wsb"]

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return L.dod_detect_views(*(a[k] for k in order), nat.stream_ptr())

    bad = [dict(det=None), dict(offs=None), dict(rects=None), dict(flips=None), dict(sizes=None), dict(ws=None), dict(wsb=ws.numel() - 1), dict(wsb=0),
           dict(B=0), dict(B=-1), dict(V=-1), dict(Q=0), dict(C=0), dict(K=0), dict(K=1025), dict(K=1025, iou=-1.0), dict(Q=1 << 11, C=(1 << 9) + 1),
           dict(first=-1), dict(first=C), dict(metric=2), dict(metric=-1), dict(boxes=nat.C.c_void_p(bufs["boxes"][1].data_ptr() + 4))]
    bad += [{k: None} for k in OUTS]
    for kw in bad:
        assert call(**kw) == INVALID, kw
    torch.cuda.synchronize()
    _untouched(bufs, inside=True)
    W = L.dod_detect_views_workspace_bytes
    assert W(V, Q, C, 0) == 0 and W(V, Q, C, 1025) == 0 and W(-1, Q, C, K) == 0 and W(V, 0, C, K) == 0 and W(V, Q, 0, K) == 0
    assert W(V, 1 << 11, (1 << 9) + 1, K) == 0 and W(0, Q, C, K) > 0 and W(16, 720, 91, 1024) >= 16 * 720 * 91 * 4 + 16 * 720
    assert call() == 0                                                              # the good call, last: the outputs are written now
    torch.cuda.synchronize()
    _untouched(bufs)
    assert int(bufs["counts"][1].min()) > 0


def test_detect_views_packed_forms(sl):
    """the Python entry: a numpy plan and a device plan, sizes in their forms, the metric names, the named result"""
    from dinov2_od_amd import postprocess as pp
    counts, Q, C, K = (3, 2), 30, 6, 20
    det_np, offsets, rects, flips, sizes = case = _case(47, counts, Q, C)
    det = torch.from_numpy(det_np).cuda()
    plan = sl.ViewPlan(offsets, rects, flips)
    for p in (plan, sl.plan_to_device(plan, "cuda")):
        for sz in (sizes, torch.tensor(sizes), torch.tensor(sizes).cuda()):
            r = sl.detect_views_packed(det, C, p, sz, top_k=K, threshold=0.05, nms_iou=0.5, nms_metric="ios", edge_margin=dv.EDGE_MARGIN)
            assert isinstance(r, pp.Detections) and r._fields == ("scores", "labels", "boxes", "queries", "counts") and r.views.is_cuda
            got = {k: getattr(r, k).cpu().numpy() for k in OUTS}
            _check(got, _ref(case, C, K, 1, 0.05, 0.5, 1, False, True, dv.EDGE_MARGIN))
    r = sl.detect_views_packed(det, C, plan, sizes, top_k=K, threshold=-1.0, nms_iou=None, skip_background=False, clamp=False)
    _check({k: getattr(r, k).cpu().numpy() for k in OUTS}, _ref(case, C, K, 0, -1.0, None, 0, False, False))
    lst = pp.detections_to_list(r)
    assert len(lst) == 2 and all(d["boxes"].shape == (K, 4) for d in lst)
    r = sl.detect_views_packed(det, C, plan, sizes, top_k=1024, threshold=-1.0, nms_iou=0.5)       # NMS at 1024 is allowed here
    _check({k: getattr(r, k).cpu().numpy() for k in OUTS}, _ref(case, C, 1024, 1, -1.0, 0.5))
    for kw in (dict(nms_metric="giou"), dict(top_k=1025), dict(top_k=0), dict(nms_iou=-0.5)):
        with pytest.raises(ValueError):
            sl.detect_views_packed(det, C, plan, sizes, **kw)
    with pytest.raises(ValueError):
        sl.detect_views_packed(det, C, plan, None)
    with pytest.raises(ValueError):
        sl.detect_views_packed(det[:4], C, plan, sizes)
    with pytest.raises(ValueError):
        sl.detect_views_packed(det, C, sl.ViewPlan(np.asarray([0, 5, 4], np.int32), rects, flips), sizes)


def test_model_detect_sliced_end_to_end(sl):
    """model.detect_sliced on three ragged raw images with tiles, full view and flip == extract_views -> forward_packed_u8 -> the
    numpy restatement; extract_views == augment_batch(as_uint8=True) per view, byte for byte; the result draws; train() is restored"""
    from dinov2_od_amd import augment, postprocess as pp, visualize
    from tests import augment_cases as ac, gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "bf16x3", "facebook/dinov2-small")
    imgs = [ac._rand(s, 140 + i) for i, s in enumerate([(300, 420), (150, 180), (333, 500)])]
    shapes = [im.shape[:2] for im in imgs]
    size, tile, C, Q = (224, 224), 200, 91, 25
    plan = sl.plan_views(shapes, tile, 0.2, True, True, size=size, pairs=Q * C)
    assert np.diff(plan.offsets).tolist() == [14, 2, 14] and plan.flips.sum() == 15
    u8 = sl.extract_views(imgs, plan, size)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (30, 224, 224, 3)
    for b in range(3):
        for v in range(plan.offsets[b], plan.offsets[b + 1]):
            one, _ = augment.augment_batch([imgs[b]], None, [plan.rects[v]], [plan.flips[v]], None, size, as_uint8=True)
            assert torch.equal(one[0], u8[v]), (b, v)
    with torch.no_grad():
        det = m.forward_packed_u8(u8).clone()
    kw = dict(top_k=100, threshold=-1.0, nms_iou=0.5, nms_metric="ios", edge_margin=4.0)          # no score threshold: nothing hinges on an ulp of expf
    sizes = [(float(h), float(w)) for h, w in shapes]
    want = dv.detect_views_ref(det.cpu().numpy(), C, 100, plan.offsets, plan.rects, plan.flips, sizes, 1, -1.0, 0.5, 1, False, True, 4.0)
    print(f"rows cut {want['cut'].tolist()} of {want['rows'].tolist()}, counts {want['counts'].tolist()}")
    assert want["counts"].min() > 0
    m.train()
    r = m.detect_sliced(imgs, size=size, tile=tile, overlap=0.2, full_view=True, flip=True, **kw)
    assert m.training
    m.eval()
    assert isinstance(r, pp.Detections) and tuple(r.boxes.shape) == (3, 100, 4)
    _check({k: getattr(r, k).cpu().numpy() for k in OUTS}, want)
    r2 = m.detect_sliced(imgs, size=size, tile=tile, flip=True, max_batch=7, **kw)               # chunked forward: the same views
    assert not m.training and np.array_equal(r2.counts.cpu().numpy() > 0, want["counts"] > 0) and 0 <= int(r2.views.max()) <= 13
    canvas = torch.zeros(3, 333, 500, 3, dtype=torch.uint8, device="cuda")
    drawn = visualize.draw_detections(canvas, r, score_threshold=-1.0)
    assert tuple(drawn.shape) == (3, 333, 500, 3) and int(drawn.max()) > 0
    lst = pp.detections_to_list(r)
    assert [len(d["scores"]) for d in lst] == want["counts"].tolist()
    with pytest.raises(ValueError, match="candidates"):
        sl.plan_views(shapes, 16, 0.5, pairs=Q * C)                                              # thousands of views of one image
