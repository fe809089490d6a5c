"""GPU parity of the detection output (dod_detect: top-k, pixel boxes, optional NMS) against its numpy restatement
(tests/detect_cases.py).  labels, queries, counts and the padding rows are exact, boxes bit-equal, scores within the project's
tolerance for this sigmoid (3e-7 absolute).  Every output sits between guard rows that must stay untouched."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, synth
from tests import cases
from tests import detect_cases as dc
from tests import guard_rows as gr
from tests.guard_rows import same as _same

pytestmark = pytest.mark.gpu
OUTS = ("scores", "labels", "queries", "boxes", "counts")


@pytest.fixture(scope="module")
def pp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from dinov2_od_amd import postprocess
    return postprocess


def _run(det, C, K, first_class=1, sizes=None, threshold=-1.0, iou=None, class_agnostic=False, clamp=True, stream=None):
    """dod_detect through the C ABI into guarded outputs -> dict of numpy arrays shaped like detect_cases.detect_ref's"""
    L = nat.lib()
    d = det if isinstance(det, torch.Tensor) else torch.from_numpy(det).cuda()
    B, Q, _ = d.shape
    bufs = gr.buffers(B, K, OUTS)
    st = None if sizes is None else torch.from_numpy(dc.size_rows(sizes, B)).cuda()
    ws = torch.empty(L.dod_detect_workspace_bytes(B, Q, C, K), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        nat.check(L.dod_detect(nat.ptr(d), B, Q, C, first_class, nat.ptr(st), float(threshold), K, -1.0 if iou is None else float(iou),
                               int(class_agnostic), int(clamp), *(nat.ptr(bufs[k][1]) for k in OUTS), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    s.synchronize()
    gr.untouched(bufs)
    return gr.shaped(bufs, B, K)


def _check(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(got["queries"], want["queries"])
    assert np.array_equal(got["boxes"].view(np.uint32), want["boxes"].view(np.uint32))
    err = float(np.max(np.abs(got["scores"].astype(np.float64) - want["scores"].astype(np.float64))))
    print(f"max score error {err:.3g}")
    assert err < dc.SCORE_TOL
    K = got["scores"].shape[1]
    pad = np.arange(K)[None, :] >= want["counts"][:, None]
    assert np.all(got["scores"][pad] == 0.0) and np.all(got["labels"][pad] == -1) and np.all(got["queries"][pad] == -1)
    assert not got["boxes"][pad].view(np.uint32).any()


TOPK_SHAPES = [(1, 1, 2, 1), (3, 7, 5, 4), (2, 113, 19, 100), (2, 100, 91, 100), (2, 300, 91, 300), (1, 300, 91, 1024), (65, 9, 3, 5)]


@pytest.mark.parametrize("skip_background", [True, False])
@pytest.mark.parametrize("B,Q,C,K", TOPK_SHAPES)
def test_topk_matches_restatement(pp, B, Q, C, K, skip_background):
    det = dc.random_det(11, B, Q, C)
    first = 1 if skip_background else 0
    sizes = [(480.0 + 3 * b, 640.0 - 5 * b) for b in range(B)]
    want = dc.detect_ref(det, C, K, first, sizes)
    got = _run(det, C, K, first, sizes)
    _check(got, want)
    assert np.all(want["counts"] == min(K, Q * (C - first)))
    if skip_background:
        assert got["labels"].min() >= -1 and not np.any(got["labels"] == 0)


@pytest.mark.parametrize("B,Q,C,K", [(2, 40, 7, 33), (2, 100, 91, 100), (1, 300, 91, 300), (3, 5, 4, 15)])
def test_ties_are_broken_by_lowest_flat_index(pp, B, Q, C, K):
    det = dc.quantised_det(12, B, Q, C)
    want = dc.detect_ref(det, C, K, 1)
    n0 = int(want["counts"][0])
    lg, cand = det[0, want["queries"][0, :n0], want["labels"][0, :n0]], det[0, :, 1:C].reshape(-1)
    assert K >= cand.size or (cand == lg[-1]).sum() > (lg == lg[-1]).sum() > 0      # ties straddle the K-th position
    _check(_run(det, C, K, 1), want)
    flat = det.copy()
    flat[..., :C] = -1.25                                                            # every logit equal
    want = dc.detect_ref(flat, C, K, 1)
    idx = want["queries"].astype(np.int64) * C + want["labels"]
    n = int(want["counts"][0])
    assert np.all(np.diff(idx[:, :n], axis=1) > 0)
    _check(_run(flat, C, K, 1), want)


@pytest.mark.parametrize("threshold", [-1.0, 0.5])
def test_special_values(pp, threshold):
    B, Q, C, K = 2, 50, 9, 120
    det = dc.special_det(13, B, Q, C)
    lg = det[..., :C]
    assert np.isnan(lg).sum() > 10 and np.isposinf(lg).sum() > 3 and np.isneginf(lg).sum() > 3 and (lg == 0).sum() > 6
    for first in (0, 1):
        want = dc.detect_ref(det, C, K, first, (333.0, 500.0), threshold)
        got = _run(det, C, K, first, (333.0, 500.0), threshold)
        _check(got, want)
        n = got["counts"]
        for b in range(B):
            sel = det[b, got["queries"][b, :n[b]], got["labels"][b, :n[b]]]
            assert not np.isnan(sel).any()
    allnan = det.copy()
    allnan[..., :C] = np.nan
    got = _run(allnan, C, K, 0)
    assert not got["counts"].any()
    _check(got, dc.detect_ref(allnan, C, K, 0))


@pytest.mark.parametrize("threshold", [-1.0, 0.05, 0.5, 0.9])
def test_thresholds_and_counts(pp, threshold):
    B, Q, C, K = 3, 30, 6, 40
    det = dc.random_det(14, B, Q, C, mean=-1.0, std=2.0)
    want = dc.detect_ref(det, C, K, 1, None, threshold)
    _check(_run(det, C, K, 1, None, threshold), want)
    if threshold == 0.9:
        assert np.all(want["counts"] < K) and want["counts"].min() > 0            # fewer candidates than K: padding appears
    if threshold < 0:
        assert np.all(want["counts"] == K)


def test_exactly_k_candidates_and_none(pp):
    B, Q, C, K = 2, 12, 5, 17
    det = dc.random_det(15, B, Q, C)
    det[..., :C] = -9.0
    hot = synth.uniform01(15, "det.exact", (B, Q * (C - 1)))
    for b in range(B):
        pick = np.argsort(hot[b], kind="stable")[:K]
        det[b, pick // (C - 1), 1 + pick % (C - 1)] = 2.0 + hot[b, pick]
    want = dc.detect_ref(det, C, K, 1, None, 0.5)
    assert np.all(want["counts"] == K)
    _check(_run(det, C, K, 1, None, 0.5), want)
    _check(_run(det, C, K + 1, 1, None, 0.5), dc.detect_ref(det, C, K + 1, 1, None, 0.5))
    det[..., :C] = -9.0                                                            # all below the threshold
    got = _run(det, C, K, 1, None, 0.5)
    assert not got["counts"].any()
    _check(got, dc.detect_ref(det, C, K, 1, None, 0.5))


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("sizes", [None, (480.0, 640.0), [(480.0, 640.0), (333.0, 500.0), (1.0, 1.0)]])
def test_boxes_scale_and_clamp(pp, sizes, clamp):
    B, Q, C, K = 3, 64, 4, 90
    det = dc.random_det(16, B, Q, C)
    bx = det[..., C:]
    assert (bx[..., 0] - 0.5 * bx[..., 2] < 0).any() and (bx[..., 0] + 0.5 * bx[..., 2] > 1).any()      # boxes reach outside the image
    assert (bx[..., 2] == 0).any() and (bx[..., 2] < 0).any()                                              # zero and negative widths
    want = dc.detect_ref(det, C, K, 1, sizes, -1.0, None, False, clamp)
    got = _run(det, C, K, 1, sizes, -1.0, None, False, clamp)
    _check(got, want)
    hw = dc.size_rows(sizes, B)
    if clamp:
        assert got["boxes"].min() >= 0 and np.all(got["boxes"][..., 0::2] <= hw[:, None, 1:2]) and np.all(got["boxes"][..., 1::2] <= hw[:, None, 0:1])
    else:
        assert got["boxes"].min() < 0


@pytest.mark.parametrize("K,iou,agnostic", dc.NMS_CASES)
def test_nms_matches_restatement(pp, K, iou, agnostic):
    det = dc.clustered_det(K)
    C = det.shape[-1] - 4
    want = dc.detect_ref(det, C, K, 1, dc.NMS_SIZES, -1.0, iou, agnostic, True)
    got = _run(det, C, K, 1, dc.NMS_SIZES, -1.0, iou, agnostic, True)
    _check(got, want)
    assert 0 < got["counts"].sum() < K * det.shape[0]


def test_nms_on_random_boxes_and_with_threshold(pp):
    B, Q, C, K = 2, 100, 91, 300
    det = dc.random_det(17, B, Q, C)
    for iou, agn, thr in [(0.5, False, -1.0), (0.3, True, 0.05), (0.0, True, -1.0)]:
        want = dc.detect_ref(det, C, K, 1, (480.0, 640.0), thr, iou, agn, True)
        _check(_run(det, C, K, 1, (480.0, 640.0), thr, iou, agn, True), want)


def test_nms_identical_and_degenerate_boxes(pp):
    """identical boxes of one class: only the first survives; a zero-area box is never suppressed and never suppresses"""
    C = 3
    det = np.zeros((1, 6, C + 4), np.float32)
    det[0, :, :C] = -9.0
    det[0, :, 1] = [5.0, 4.0, 3.0, 2.0, 1.0, 0.5]
    det[0, :, C:] = [[.5, .5, .2, .2], [.5, .5, .2, .2], [.5, .5, 0.0, .2], [.5, .5, .2, .2], [.5, .5, 0.0, .2], [.1, .1, .1, .1]]
    for iou in (0.0, 0.5):
        got = _run(det, C, 6, 1, (100.0, 100.0), -1.0, iou, False, True)
        _check(got, dc.detect_ref(det, C, 6, 1, (100.0, 100.0), -1.0, iou, False, True))
        assert got["counts"][0] == 4 and got["queries"][0, :4].tolist() == [0, 2, 4, 5]


def test_repeatable_and_stream_independent(pp):
    B, Q, C, K = 4, 100, 91, 100
    det = torch.from_numpy(dc.quantised_det(18, B, Q, C, levels=64)).cuda()
    for iou in (None, 0.5):
        a = _run(det, C, K, 1, (480.0, 640.0), 0.05, iou)
        b = _run(det, C, K, 1, (480.0, 640.0), 0.05, iou)
        assert _same(a, b)
        torch.cuda.synchronize()
        c = _run(det, C, K, 1, (480.0, 640.0), 0.05, iou, stream=torch.cuda.Stream())
        assert _same(a, c)


def test_detect_packed_forms(pp):
    """the Python entry: sizes as None / one pair / a list of pairs / a tensor, the named result, detections_to_list"""
    B, Q, C, K = 2, 30, 6, 20
    det_np = dc.random_det(19, B, Q, C)
    det = torch.from_numpy(det_np).cuda()
    pairs = [(480.0, 640.0), (333.0, 500.0)]
    for sizes, ref_sizes in [(None, None), ((480, 640), (480.0, 640.0)), (pairs, pairs), (torch.tensor(pairs), pairs), (torch.tensor(pairs).cuda(), pairs)]:
        r = pp.detect_packed(det, C, sizes, top_k=K, threshold=0.05, nms_iou=0.5)
        assert r._fields == ("scores", "labels", "boxes", "queries", "counts") and all(t.is_cuda for t in r)
        got = {k: getattr(r, k).cpu().numpy() for k in r._fields}
        _check(got, dc.detect_ref(det_np, C, K, 1, ref_sizes, 0.05, 0.5, False, True))
    r = pp.detect_packed(det, C, top_k=K, skip_background=False, clamp=False, class_agnostic=True, nms_iou=0.0)
    _check({k: getattr(r, k).cpu().numpy() for k in r._fields}, dc.detect_ref(det_np, C, K, 0, None, -1.0, 0.0, True, False))
    lst = pp.detections_to_list(r)
    assert len(lst) == B
    for b, d in enumerate(lst):
        n = int(r.counts[b])
        assert 0 < n < K and set(d) == {"boxes", "scores", "labels"}
        assert d["boxes"].shape == (n, 4) and d["scores"].shape == (n,) and d["labels"].shape == (n,)
        assert torch.equal(d["labels"], r.labels[b, :n]) and int(d["labels"].min()) >= 0
    with pytest.raises(ValueError):
        pp.detect_packed(det, C, top_k=513, nms_iou=0.5)


def test_model_detect(pp):
    """model.detect(images) == detect_packed(model.forward_packed(images)) with the input's own (H, W) as sizes"""
    from tests import gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "fp32", "facebook/dinov2-small")
    x = G.to_gpu(synth.make_pixels(2, 224, 224, seed=0))
    r = m.detect(x, top_k=50, threshold=0.05, nms_iou=0.5)
    with torch.no_grad():
        det = m.forward_packed(x)
    w = pp.detect_packed(det, 91, (224, 224), top_k=50, threshold=0.05, nms_iou=0.5)
    for a, b in zip(r, w):
        assert torch.equal(a, b)
    assert not m.training
    r2 = m.detect(x, sizes=[(480, 640), (333, 500)], top_k=7)           # no score threshold: nothing hinges on an ulp of expf
    assert r2.boxes.shape == (2, 7, 4) and int(r2.counts.min()) == 7
    _check({k: getattr(r2, k).cpu().numpy() for k in r2._fields}, dc.detect_ref(det.cpu().numpy(), 91, 7, 1, [(480.0, 640.0), (333.0, 500.0)]))
    out = m(x)
    assert set(out) == {"pred_logits", "pred_boxes"}
