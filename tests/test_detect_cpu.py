"""CPU-side checks of the detection output (dod_detect): the numpy restatement in tests/detect_cases.py against an independent
formulation (torch.topk + a brute-force NMS in Python floats), the NMS inputs of the GPU test shown not to be vacuous, the ABI entry
and the argument checks of postprocess.detect_packed.  No GPU compute."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import detect_cases as dc

f = np.float32


def _brute_nms(boxes, labels, iou, agnostic):
    """O(K^2) greedy NMS, one Python float operation at a time, each rounded through np.float32"""
    n = len(boxes)
    bx = [[f(v) for v in r] for r in boxes]
    area = [f(max(f(0), f(r[2] - r[0])) * max(f(0), f(r[3] - r[1]))) for r in bx]
    keep = []
    for j in range(n):
        gone = False
        for i in keep:
            if not agnostic and labels[i] != labels[j]:
                continue
            iw = max(f(0), f(min(bx[i][2], bx[j][2]) - max(bx[i][0], bx[j][0])))
            ih = max(f(0), f(min(bx[i][3], bx[j][3]) - max(bx[i][1], bx[j][1])))
            inter = f(iw * ih)
            union = f(f(area[i] + area[j]) - inter)
            if inter > f(f(iou) * union):
                gone = True
                break
        if not gone:
            keep.append(j)
    return keep


@pytest.mark.parametrize("B,Q,C,K", [(2, 40, 7, 25), (1, 113, 19, 100), (2, 9, 3, 18)])
@pytest.mark.parametrize("first_class", [0, 1])
@pytest.mark.parametrize("iou,agnostic", [(None, False), (0.5, False), (0.3, True)])
def test_restatement_matches_topk_and_brute_force_nms(B, Q, C, K, first_class, iou, agnostic):
    det = dc.distinct_det(3, B, Q, C)
    sizes = [(480.0, 640.0), (333.0, 500.0)][:B]
    ref = dc.detect_ref(det, C, K, first_class, sizes, -1.0, iou, agnostic, True)
    for b in range(B):
        lg = torch.from_numpy(det[b, :, first_class:C].copy()).reshape(-1)          # sigmoid is monotone: rank the logits
        k = min(K, lg.numel())
        top = torch.topk(lg, k).indices.numpy()
        q, lab = top // (C - first_class), first_class + top % (C - first_class)
        cx, cy, w, h = (det[b, q, C + i] for i in range(4))
        ih, iw = f(sizes[b][0]), f(sizes[b][1])
        box = np.stack([(cx - f(0.5) * w) * iw, (cy - f(0.5) * h) * ih, (cx + f(0.5) * w) * iw, (cy + f(0.5) * h) * ih], 1).astype(f)
        box = np.stack([np.clip(box[:, 0], 0, iw), np.clip(box[:, 1], 0, ih), np.clip(box[:, 2], 0, iw), np.clip(box[:, 3], 0, ih)], 1).astype(f)
        keep = list(range(k)) if iou is None else _brute_nms(box, lab, iou, agnostic)
        n = len(keep)
        assert ref["selected"][b] == k and ref["counts"][b] == n
        assert np.array_equal(ref["queries"][b, :n], q[keep]) and np.array_equal(ref["labels"][b, :n], lab[keep])
        assert np.array_equal(ref["boxes"][b, :n].view(np.uint32), box[keep].view(np.uint32))
        want = 1.0 / (1.0 + np.exp(-det[b, q[keep], lab[keep]].astype(np.float64)))
        assert np.max(np.abs(ref["scores"][b, :n] - want), initial=0.0) < dc.SCORE_TOL
        assert np.all(ref["labels"][b, n:] == -1) and np.all(ref["queries"][b, n:] == -1)
        assert not ref["scores"][b, n:].any() and not ref["boxes"][b, n:].any()


def test_restatement_orders_ties_and_special_values_by_bits():
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1.0, -np.nan, 40.0, -40.0], np.float32)
    got = dc.select(x, 1, 10, 0, -1.0)
    assert got.tolist() == [2, 8, 5, 6, 0, 1, 9, 3]          # +inf, 40, the two 1.0 by index, +0.0 before -0.0, -40, -inf; no NaN
    assert dc.select(x, 1, 3, 0, 0.5).tolist() == [2, 8, 5]  # sigmoid(0) = 0.5 is not above 0.5
    assert dc.select(np.full(12, -2.0, np.float32), 3, 5, 1, -1.0).tolist() == [1, 2, 4, 5, 7]      # all equal: lowest index, class 0 skipped


@pytest.mark.parametrize("K,iou,agnostic", dc.NMS_CASES)
def test_clustered_nms_inputs_are_not_vacuous(K, iou, agnostic):
    """between 20 % and 80 % of the selected candidates are suppressed: the GPU test can fail in either direction"""
    det = dc.clustered_det(K)
    C = det.shape[-1] - 4
    ref = dc.detect_ref(det, C, K, 1, dc.NMS_SIZES, -1.0, iou, agnostic, True)
    sel, kept = int(ref["selected"].sum()), int(ref["counts"].sum())
    assert sel == K * det.shape[0]
    frac = 1.0 - kept / sel
    print(f"K={K} iou={iou} agnostic={agnostic}: suppressed {frac:.3f}")
    assert 0.2 <= frac <= 0.8, frac


def test_identical_and_degenerate_boxes():
    """identical boxes of one class: only the first survives; a zero-area box is never suppressed and never suppresses"""
    C = 3
    det = np.zeros((1, 6, C + 4), np.float32)
    det[0, :, :C] = -9.0
    det[0, :, 1] = [5.0, 4.0, 3.0, 2.0, 1.0, 0.5]
    det[0, :, C:] = [[.5, .5, .2, .2], [.5, .5, .2, .2], [.5, .5, 0.0, .2], [.5, .5, .2, .2], [.5, .5, 0.0, .2], [.1, .1, .1, .1]]
    for iou in (0.0, 0.5):
        ref = dc.detect_ref(det, C, 6, 1, (100.0, 100.0), -1.0, iou, False, True)
        assert ref["counts"][0] == 4 and ref["queries"][0, :4].tolist() == [0, 2, 4, 5]


def test_abi_entry_is_declared():
    assert "dod_detect" in nat.SYMBOLS and "dod_detect_workspace_bytes" in nat.SYMBOLS


def test_abi_entry_validates_arguments():
    """limits of include/dinodet.h: DOD_ERR_INVALID before any launch (no GPU here: a launch would be DOD_ERR_HIP)"""
    import ctypes as C
    import os
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    L = nat.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ws = L.dod_detect_workspace_bytes
    assert ws(2, 100, 91, 100) >= 2 * 100 * 91 * 4 and ws(1, 1, 1, 1) > 0
    assert ws(2, 100, 91, 0) == 0 and ws(2, 100, 91, 1025) == 0 and ws(1, 1 << 11, 1 << 10, 5) == 0 and ws(0, 1, 1, 1) == 0 and ws(1, 4, 0, 1) == 0
    assert ws(1, 1 << 10, 1 << 10, 1024) == 4 << 20

    def call(B=2, Q=10, C_=5, first=1, K=8, iou=-1.0, nbytes=1 << 20, null=None):
        a = [p, B, Q, C_, first, None, -1.0, K, iou, 0, 1, p, p, p, p, p, p, nbytes, None]
        if null is not None:
            a[null] = None
        return L.dod_detect(*a)
    for bad in (dict(K=0), dict(K=1025), dict(C_=0), dict(first=5), dict(first=-1), dict(B=0), dict(Q=0), dict(Q=1 << 19, nbytes=1 << 40),
                dict(K=513, iou=0.5), dict(nbytes=16)):
        assert call(**bad) == 1, bad
    for i in (0, 11, 12, 13, 14, 15, 16):
        assert call(null=i) == 1, i


def test_detect_packed_rejects_bad_arguments():
    from dinov2_od_amd import postprocess as pp
    good = torch.zeros(2, 3, 9)
    with pytest.raises(ValueError, match="CUDA"):
        pp.detect_packed(good, 5)                                  # a CPU tensor: there is no CPU fallback
    with pytest.raises(ValueError, match="columns"):
        pp.detect_packed(good, 4)                                  # 4 + 4 != 9
    with pytest.raises(ValueError, match="top_k"):
        pp.detect_packed(good, 5, top_k=0)
    with pytest.raises(ValueError, match="top_k"):
        pp.detect_packed(good, 5, top_k=1025)
    with pytest.raises(ValueError, match="top_k"):
        pp.detect_packed(good, 5, top_k=513, nms_iou=0.5)          # the NMS limit
    with pytest.raises(ValueError, match="sizes"):
        pp.detect_packed(good, 5, sizes=[(480, 640)] * 3)          # three pairs for two images
    with pytest.raises(ValueError, match="sizes"):
        pp.detect_packed(good, 5, sizes=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="nms_iou"):
        pp.detect_packed(good, 5, nms_iou=-0.5)
