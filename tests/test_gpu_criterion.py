"""`-m gpu`: the native set criterion (csrc/criterion.hip through dinov2_od_amd.losses) against golden G10 (the reference's own
SetCriterion + autograd, float64) and against the float64 torch composite at training shapes; reading the packed output views
in place, run-to-run bit reproducibility, the upstream gradient arriving through d_losses, our matcher on G10's case 2, and
a real train step (native decoder forward / backward + matcher + native criterion) against the composite criterion."""
import os

import numpy as np
import pytest
import torch

from dinov2_od_amd import losses as L, synth
from tests import cases, criterion_cases as cc, criterion_edge_cases as ce
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
KEYS = ("loss_ce", "loss_bbox", "loss_giou")


@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_criterion.npz"))


def _dev():
    return torch.device("cuda:0")


def _native_case(name, g, packed=True):
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    d = torch.from_numpy(det).to(_dev()).requires_grad_(True)
    out = {"pred_logits": d[..., :C], "pred_boxes": d[..., C:]} if packed else \
        {"pred_logits": d[..., :C].contiguous(), "pred_boxes": d[..., C:].contiguous()}
    tg = cc.targets(labels, gt, offs, to=lambda t: t.to(_dev()))
    ld = L.SetCriterion(cc.FixedMatcher(cc.indices_from(g, name)), C, dict(cc.WEIGHTS), alpha, gamma)(out, tg)
    sum(ld.values()).backward()
    gd = d.grad.detach()
    return np.array([float(ld[k].detach()) for k in KEYS]), gd[..., :C].cpu().numpy(), gd[..., C:].cpu().numpy()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_native_matches_reference_float64(g10, name):
    losses, gl, gb = _native_case(name, g10)
    want = g10[f"{name}.losses64"]
    rel = np.abs(losses - want) / np.maximum(np.abs(want), 1e-30)
    ref32 = np.abs(g10[f"{name}.losses32"] - want) / np.maximum(np.abs(want), 1e-30)
    print(f"{name} losses rel err {rel.max():.2e} (reference fp32 {ref32.max():.2e})")
    assert (rel <= 1e-5).all() or np.abs(losses - want).max() <= 1e-5 * np.abs(want).max(), (losses, want)
    for got, key in ((gl, "dlogits"), (gb, "dboxes")):
        w64, w32 = g10[f"{name}.{key}64"], g10[f"{name}.{key}32"]
        err, err32 = np.abs(got - w64).max(), np.abs(w32 - w64).max()
        scale = np.abs(w64).max()
        print(f"{name} {key}: max|d| {err:.2e} (reference fp32 {err32:.2e}), max|g64| {scale:.2e}")
        assert err <= 1e-5 * scale or scale == 0 and err == 0, (key, err, scale)
    # and element by element (tests/criterion_edge_cases.py); the criterion's weights are the upstream gradient and scale the losses
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    w = np.array([cc.WEIGHTS[k] for k in KEYS], np.float32)
    ref = ce.reference(det.reshape(B * Q, -1)[:, :C], det.reshape(B * Q, -1)[:, C:], labels, gt, L.match_table(cc.indices_from(g10, name), counts, Q).numpy(),
                       float(sum(counts)), alpha, gamma, d_losses=w)
    ref["losses_bound"] = w * ref["losses_bound"] + ce.U * np.abs(w * ref["losses"])
    ref["losses"] = w * ref["losses"]
    r = ce.check({"losses": losses, "d_logits": gl.reshape(B * Q, C), "d_boxes": gb.reshape(B * Q, 4)}, ref, name)
    print(f"{name} worst error / bound per element: {ce.fmt(r)}")


def _synthetic(B, Q, C, seed):
    """training-like outputs and a random one-to-one assignment of 0..min(Q, 40) targets per image"""
    rng = np.random.default_rng(seed)
    counts = [int(rng.integers(0, min(Q, 40) + 1)) for _ in range(B)]
    det, labels, gt, offs = cc.synth_inputs(B, Q, C, counts, seed)
    idx = [(torch.from_numpy(np.sort(rng.permutation(Q)[:n]).astype(np.int64)), torch.from_numpy(rng.permutation(n).astype(np.int64)))
           for n in counts]
    return det, labels, gt, offs, counts, idx


@pytest.mark.parametrize("B,Q,C", [(16, 100, 91), (32, 300, 91)])
def test_native_matches_composite_float64_at_training_shapes(B, Q, C):
    det, labels, gt, offs, counts, idx = _synthetic(B, Q, C, seed=B + Q)
    match = L.match_table(idx, counts, Q)
    nb = torch.tensor([float(sum(counts))])
    d64 = torch.from_numpy(det).double().to(_dev()).requires_grad_(True)
    ref = L.composite_losses(d64[..., :C], d64[..., C:], torch.from_numpy(labels).to(_dev()), torch.from_numpy(gt).double().to(_dev()),
                             match.to(_dev()), nb.double().to(_dev()))
    (ref * torch.tensor([1.0, 5.0, 2.0], dtype=torch.float64, device=_dev())).sum().backward()
    d = torch.from_numpy(det).to(_dev()).requires_grad_(True)
    got = L.native_losses(d[..., :C], d[..., C:], torch.from_numpy(labels).to(_dev()), torch.from_numpy(gt).to(_dev()), match.to(_dev()),
                          nb.to(_dev()))
    (got * torch.tensor([1.0, 5.0, 2.0], device=_dev())).sum().backward()
    r, gr = ref.detach().cpu().numpy(), got.detach().cpu().numpy()
    print(f"B={B} Q={Q}: losses {gr} rel err {np.abs(gr - r).max() / np.abs(r).max():.2e}")
    np.testing.assert_allclose(gr, r, rtol=1e-5)
    g64, g32 = d64.grad.cpu().numpy(), d.grad.cpu().numpy()
    for sl, key in ((np.s_[..., :C], "dlogits"), (np.s_[..., C:], "dboxes")):
        err, scale = np.abs(g32[sl] - g64[sl]).max(), np.abs(g64[sl]).max()
        print(f"B={B} Q={Q} {key}: max|d| {err:.2e}, max|g64| {scale:.2e}")
        assert err <= 1e-5 * scale, key
    ref = ce.reference(det.reshape(B * Q, -1)[:, :C], det.reshape(B * Q, -1)[:, C:], labels, gt, match.numpy(), float(sum(counts)), 0.25, 2.0,
                       d_losses=np.array([1.0, 5.0, 2.0], np.float32))
    r = ce.check({"losses": gr, "d_logits": g32[..., :C].reshape(B * Q, C), "d_boxes": g32[..., C:].reshape(B * Q, 4)}, ref, f"B={B} Q={Q}")
    print(f"B={B} Q={Q} worst error / bound per element: {ce.fmt(r)}")


def _packed_run(det, C, labels, gt, match, nb, views, scale=1.0):
    d = det.clone().requires_grad_(True)
    lg, bx = (d[..., :C], d[..., C:]) if views else (d[..., :C].contiguous(), d[..., C:].contiguous())
    out = L.native_losses(lg, bx, labels, gt, match, nb)
    (scale * out.sum()).backward()
    return out.detach(), d.grad.detach()


def test_packed_views_read_in_place_bit_identical_and_deterministic():
    from dinov2_od_amd.engine import split_detections
    B, Q, C = 8, 100, 91
    det, labels, gt, offs, counts, idx = _synthetic(B, Q, C, seed=5)
    dev = _dev()
    det = torch.from_numpy(det).to(dev)
    labels, gt = torch.from_numpy(labels).to(dev), torch.from_numpy(gt).to(dev)
    match, nb = L.match_table(idx, counts, Q).to(dev), torch.tensor([float(sum(counts))], device=dev)
    o = split_detections(det, C)
    assert o["pred_logits"].data_ptr() == det.data_ptr() and not o["pred_logits"].is_contiguous()
    a_loss, a_grad = _packed_run(det, C, labels, gt, match, nb, views=True)
    b_loss, b_grad = _packed_run(det, C, labels, gt, match, nb, views=False)
    c_loss, c_grad = _packed_run(det, C, labels, gt, match, nb, views=True)
    assert torch.equal(a_loss, b_loss) and torch.equal(a_grad, b_grad)          # strided views == contiguous copies, bit for bit
    assert torch.equal(a_loss, c_loss) and torch.equal(a_grad, c_grad)          # run to run
    # the upstream gradient arrives through d_losses: (2 loss).backward() doubles every gradient exactly
    _, d_grad = _packed_run(det, C, labels, gt, match, nb, views=True, scale=2.0)
    assert torch.equal(d_grad, 2 * a_grad)
    # only the forward under no_grad
    with torch.no_grad():
        n_loss = L.native_losses(o["pred_logits"], o["pred_boxes"], labels, gt, match, nb)
    assert torch.equal(n_loss, a_loss) and n_loss.grad_fn is None


def test_gradient_accumulates_across_backward_calls():
    B, Q, C = 4, 25, 11
    det, labels, gt, offs, counts, idx = _synthetic(B, Q, C, seed=9)
    dev = _dev()
    d = torch.from_numpy(det).to(dev).requires_grad_(True)
    args = (torch.from_numpy(labels).to(dev), torch.from_numpy(gt).to(dev), L.match_table(idx, counts, Q).to(dev),
            torch.tensor([float(sum(counts))], device=dev))
    L.native_losses(d[..., :C], d[..., C:], *args).sum().backward()
    once = d.grad.clone()
    L.native_losses(d[..., :C], d[..., C:], *args).sum().backward()
    assert torch.equal(d.grad, 2 * once)


def test_our_matcher_reproduces_golden_indices(g10):
    from dinov2_od_amd.matching import HungarianMatcher
    name = "c2_coco"
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    d = torch.from_numpy(det).to(_dev())
    idx = HungarianMatcher()({"pred_logits": d[..., :C], "pred_boxes": d[..., C:]}, cc.targets(labels, gt, offs, to=lambda t: t.to(_dev())))
    for (i, j), (wi, wj) in zip(idx, cc.indices_from(g10, name)):
        assert torch.equal(i, wi) and torch.equal(j, wj)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_focal_loss_on_the_criterion_kernel(reduction):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(300, 91, generator=g) * 3
    t = torch.randint(0, 91, (300,), generator=g)
    xc = x.double().requires_grad_(True)
    want = L.FocalLoss(0.25, 2.0, reduction)(xc, t)
    up = torch.rand(want.shape, generator=g, dtype=torch.float64) if reduction == "none" else torch.tensor(1.5, dtype=torch.float64)
    (want * up).sum().backward()
    xg = x.to(_dev()).requires_grad_(True)
    got = L.FocalLoss(0.25, 2.0, reduction)(xg, t.to(_dev()))
    assert got.shape == want.shape
    (got * up.float().to(_dev())).sum().backward()
    assert rel_err(got.detach().cpu().numpy(), want.detach().numpy()) < 1e-5
    assert rel_err(xg.grad.cpu().numpy(), xc.grad.numpy()) < 1e-5
    # element by element: row r's target is t[r]; 'none' is elem_loss / d_elem, 'mean' is num_boxes = N C, 'sum' is num_boxes = NULL
    up32 = up.float().numpy()
    none = reduction == "none"
    ref = ce.reference(x.numpy(), None, t.numpy(), np.zeros((0, 4), np.float32), np.arange(300), 300.0 * 91 if reduction == "mean" else None, 0.25, 2.0,
                       d_losses=None if none else np.array([up32, 0, 0], np.float32), d_elem=up32 if none else None)
    mine = {"elem": got.detach().cpu().numpy()} if none else {"losses": np.array([float(got.detach()), 0.0, 0.0])}
    r = ce.check(dict(mine, d_logits=xg.grad.cpu().numpy()), ref, f"FocalLoss {reduction}")
    print(f"FocalLoss {reduction} worst error / bound per element: {ce.fmt(r)}")
    with pytest.raises(RuntimeError):
        L.FocalLoss()(xg, torch.full((300,), 91, device=_dev()))


def test_train_step_with_the_native_criterion():
    """train.py:1079-1109 with every piece ours: train()-mode forward on the native decoder, our matcher, the native criterion,
    backward into the native decoder backward; decoder gradients agree with the composite criterion's, and AdamW lowers the loss"""
    from dinov2_od_amd import _native as nat
    from dinov2_od_amd.matching import HungarianMatcher
    from tests import gpu_util as G
    torch.manual_seed(0)
    bb, dc = cases.cfg1(25)
    m = G.make_detector(bb, dc, "fp32", "facebook/dinov2-small")
    m.train()
    G.no_dropout(m)
    x = G.to_gpu(synth.make_pixels(2, 224, 224, seed=0))
    rng = np.random.default_rng(0)
    targets = []
    for b in range(2):
        n = int(rng.integers(2, 6))
        cxcy = 0.2 + 0.6 * rng.random((n, 2))
        wh = 0.1 + 0.2 * rng.random((n, 2))
        targets.append({"labels": torch.from_numpy(rng.integers(1, dc.num_classes, n)).cuda(),
                        "boxes": torch.from_numpy(np.concatenate([cxcy, wh], 1).astype(np.float32)).cuda()})
    with torch.no_grad():
        o = m(x)
    idx = HungarianMatcher()(o, targets)
    W = dict(cc.WEIGHTS)
    counts = [len(t["labels"]) for t in targets]

    def grads(native):
        m.zero_grad(set_to_none=True)
        out = m(x)
        if native:
            ld = L.SetCriterion(cc.FixedMatcher(idx), dc.num_classes, W)(out, targets)
            loss = sum(ld.values())
        else:
            lab = torch.cat([t["labels"] for t in targets])
            gt = torch.cat([t["boxes"] for t in targets])
            lc = L.composite_losses(out["pred_logits"], out["pred_boxes"], lab, gt, L.match_table(idx, counts, dc.num_queries).cuda(),
                                    torch.tensor([float(sum(counts))], device="cuda"))
            loss = W["loss_ce"] * lc[0] + W["loss_bbox"] * lc[1] + W["loss_giou"] * lc[2]
        loss.backward()
        return float(loss.detach()), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    nat.set_option("deterministic", 1)
    try:
        l_nat, g_nat = grads(True)
        l_cmp, g_cmp = grads(False)
    finally:
        nat.set_option("deterministic", -1)
    assert abs(l_nat - l_cmp) <= 1e-5 * abs(l_cmp), (l_nat, l_cmp)
    assert set(g_nat) == set(g_cmp) and any(k.startswith("decoder.") for k in g_nat)
    for k in g_nat:
        if k.startswith("decoder."):
            assert rel_err(g_nat[k].cpu().numpy(), g_cmp[k].cpu().numpy()) < 1e-4, k
    crit = L.SetCriterion(HungarianMatcher(), dc.num_classes, W)
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=2e-3)
    hist = []
    for _ in range(6):
        ld = crit(m(x), targets)
        loss = sum(ld.values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    assert all(np.isfinite(hist)) and min(hist[-2:]) < hist[0], hist
