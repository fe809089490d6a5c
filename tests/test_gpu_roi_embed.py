"""GPU parity of dod_roi_embed against its float64 restatement (tests/roi_embed_cases.py), element by element, within a bound derived
from the kernel's own arithmetic; the output sits between guard rows; the CLS row, the tokens behind the map and the other image's
tokens are NaN-filled to show that they are never read.  Then reid.roi_embed and model.embed / model.detect_embed on top of it.

The bound.  u = 2^-24.  The kernel narrows the two axis weights to fp32 (relative error u each), multiplies them in fp32 (u more:
(1 + u)^3, 3u to first order) and accumulates p = fmaf(w, f, p) over the n tokens it touches: an fmaf chain of n terms is off by at most
n u sum w |f| to first order.  So every pooled element is within
    delta = (n + 3) u a,   a = sum w |f|                 (+ n 2^-126 max |f| for a weight product that underflows)
of the exact p.  The norm is taken in double from the fp32 p and the quotient is narrowed once, so with d = |delta| (2-norm over the
channels) and e = p / |p|
    |e^ - e| <= delta / (|p| - d) + |p_k| d / (|p| (|p| - d)) + u |e|
All of it times (1 + 2^-10) for the second-order terms (n u is below 2^-15 here), plus 1e-15 for the double arithmetic."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, reid, synth
from tests import cases
from tests import guard_rows as gr
from tests import roi_embed_cases as rc

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SIZES = np.asarray([(70.0, 98.0), (33.0, 51.0)], np.float32)
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    yield
    print(f"\ndod_roi_embed: worst observed error / bound over all cases = {WORST['ratio']:.3f}")


def bound(info, ref):
    """per element [D], for one live row"""
    n, p, a = info["tokens"], info["p"], info["a"]
    delta = (n + 3) * U * a + n * 2.0 ** -126 * float(np.max(a))
    d, norm = float(np.linalg.norm(delta)), float(np.linalg.norm(p))
    assert d < 1e-3 * norm, "the test's features keep the pooled vector well away from zero"
    return (delta / (norm - d) + np.abs(p) * d / (norm * (norm - d)) + U * np.abs(ref)) * (1.0 + 2.0 ** -10) + 1e-15


def launch(feat, first, gh, gw, boxes, counts, sizes, grid):
    """through the C ABI, emb between guard rows -> numpy [B, K, D]"""
    B, N, D = feat.shape
    K = boxes.shape[1]
    f, bx = torch.from_numpy(feat).cuda(), torch.from_numpy(boxes).cuda()
    ct = None if counts is None else torch.from_numpy(counts).cuda()
    sz = None if sizes is None else torch.from_numpy(sizes).cuda()
    bufs = {"emb": gr.guarded(B * K, D, torch.float32, gr.SENT_F)}
    nat.check(nat.lib().dod_roi_embed(nat.ptr(f), B, N, D, first, gh, gw, nat.ptr(bx), nat.ptr(ct), nat.ptr(sz), K, grid, nat.ptr(bufs["emb"][1]),
                                      nat.stream_ptr()))
    torch.cuda.synchronize()
    gr.untouched(bufs)
    assert np.array_equal(f.cpu().numpy().view(np.uint32), feat.view(np.uint32))      # the input is not changed
    return bufs["emb"][1].cpu().numpy().reshape(B, K, D)


def check(got, ref, info):
    live = 0
    for b in range(got.shape[0]):
        for k in range(got.shape[1]):
            if info[b][k] is None:
                assert not got[b, k].view(np.uint32).any(), (b, k)               # +0.0 everywhere
                continue
            live += 1
            bd = bound(info[b][k], ref[b, k])
            err = np.abs(got[b, k].astype(np.float64) - ref[b, k])
            WORST["ratio"] = max(WORST["ratio"], float(np.max(err / bd)))
            assert (err <= bd).all(), (b, k, float(np.max(err / bd)))
    return live


@pytest.mark.parametrize("grid", [1, 2, 4, 8])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("D", [8, 260])
@pytest.mark.parametrize("gh,gw", [(5, 7), (1, 3)])
def test_every_element_against_float64(gh, gw, D, first, grid):
    rng = np.random.default_rng(1000 * gh + 100 * gw + 10 * first + grid + D)
    B, K, M = 2, 8, gh * gw
    N = first + M + 2
    feat = (rng.normal(size=(B, N, D)) + 0.5).astype(np.float32)
    feat[:, :first] = np.nan                                             # CLS
    feat[:, first + M:] = np.nan                                         # behind the map
    boxes = np.stack([rc.boxes_for(gh, gw, float(SIZES[b, 0]), float(SIZES[b, 1])) for b in range(B)])
    counts = np.asarray([7, 8], np.int32)
    ref, info = rc.separable(feat, first, gh, gw, boxes, counts, SIZES, grid)
    got = launch(feat, first, gh, gw, boxes, counts, SIZES, grid)
    live = check(got, ref, info)
    # whole image, inside one token, straddling the border, (outside, x2 <= x1, NaN: zeros), a plain box, the row at the count
    assert [info[0][k] is None for k in range(K)] == [False, False, False, True, True, True, False, True] and info[1][7] is not None
    assert live == 9 and info[0][1]["tokens"] <= 9 and info[0][0]["tokens"] <= min(2 * grid, gh) * min(2 * grid, gw)
    for b in range(B):                                                   # the other image's tokens are never read
        alone = np.full_like(feat, np.nan)
        alone[b, first:first + M] = feat[b, first:first + M]
        again = launch(alone, first, gh, gw, boxes, counts, SIZES, grid)
        assert np.array_equal(again[b].view(np.uint32), got[b].view(np.uint32)), b


def test_normalised_boxes_without_counts_and_sizes():
    rng = np.random.default_rng(7)
    gh, gw, D, B, K = 5, 7, 260, 2, 8
    feat = rng.normal(size=(B, 1 + gh * gw, D)).astype(np.float32)
    feat[:, 0] = np.nan
    boxes = np.stack([rc.boxes_for(gh, gw, 1.0, 1.0) for _ in range(B)])
    ref, info = rc.separable(feat, 1, gh, gw, boxes, None, None, 4)
    got = launch(feat, 1, gh, gw, boxes, None, None, 4)
    assert check(got, ref, info) == 10
    for counts in ([-3, 0], [9, 100]):                                   # counts are clamped to 0..K
        c = np.asarray(counts, np.int32)
        ref, info = rc.separable(feat, 1, gh, gw, boxes, c, None, 4)
        assert check(launch(feat, 1, gh, gw, boxes, c, None, 4), ref, info) == (0 if counts[0] < 0 else 10)
    bad = np.asarray([(0.0, 5.0), (float("nan"), 4.0)], np.float32)       # a size that is not a positive number: every row is zeros
    assert not launch(feat, 1, gh, gw, boxes, None, bad, 4).view(np.uint32).any()
    zero = np.zeros_like(feat)                                            # |p| == 0: zeros, not NaN
    assert not launch(zero, 1, gh, gw, boxes, None, None, 4).view(np.uint32).any()


def test_python_entry_and_the_widest_row():
    rng = np.random.default_rng(9)
    gh, gw, D, B, K = 3, 4, 2048, 1, 8
    feat = rng.normal(size=(B, 1 + gh * gw, D)).astype(np.float32)
    boxes = rc.boxes_for(gh, gw, 30.0, 40.0)[None]
    ref, info = rc.separable(feat, 1, gh, gw, boxes, None, [(30.0, 40.0)], 2)
    got = reid.roi_embed(torch.from_numpy(feat).cuda(), torch.from_numpy(boxes).cuda(), sizes=(30.0, 40.0), grid=2, grid_hw=(gh, gw))
    assert got.shape == (B, K, D) and check(got.cpu().numpy(), ref, info) == 5
    same = reid.roi_embed(torch.from_numpy(feat).cuda(), torch.from_numpy(boxes).cuda(), sizes=torch.tensor([[30.0, 40.0]]), grid=2)      # 12 = 3 x 4
    assert torch.equal(same, got)


def test_model_embed_and_detect_embed():
    from tests import gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "fp32", "facebook/dinov2-small")
    H, W = 70, 98
    x = G.to_gpu(synth.make_pixels(2, H, W, seed=3))
    eng = m._get_engine()
    _, mem = eng.forward_mem(x, m._engine_named())
    boxes = np.stack([rc.boxes_for(5, 7, float(H), float(W)) for _ in range(2)])
    counts = np.asarray([7, 8], np.int32)
    emb = m.embed(x, torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda(), grid=4)
    ref, info = rc.separable(mem.cpu().numpy(), 1, 5, 7, boxes, counts, np.asarray([(H, W)] * 2, np.float32), 4)
    assert emb.shape == (2, 8, dcfg.hidden_dim) and check(emb.cpu().numpy(), ref, info) == 9
    norms = emb.norm(dim=-1).cpu().numpy()
    assert np.allclose(norms[norms > 0], 1.0, atol=1e-6) and (norms > 0).sum() == 9
    det, e2 = m.detect_embed(x, top_k=10, nms_iou=0.5)
    plain = m.detect(x, top_k=10, nms_iou=0.5)
    for p, q in zip(det, plain):
        assert torch.equal(p, q)
    hand = reid.roi_embed(mem, det.boxes, det.counts, (H, W), 4, 1, (5, 7))
    assert torch.equal(e2, hand) and e2.shape == (2, 10, dcfg.hidden_dim) and not m.training
    cnt = det.counts.tolist()
    for b in range(2):
        assert not e2[b, cnt[b]:].any() and cnt[b] > 0
