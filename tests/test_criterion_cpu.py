"""CPU checks of dinov2_od_amd.losses (the drop-in for dino_detector.losses): the torch composite of the criterion against
golden G10 (the reference's own SetCriterion + autograd, float64), the reference behaviours the module keeps (empty images,
num_boxes clamp, index errors, class-count mismatch), the documented deviation (repeated prediction index), FocalLoss, and
num_boxes summed across a world-size-2 gloo group."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dinov2_od_amd import losses as L
from tests import criterion_cases as cc

KEYS = ("loss_ce", "loss_bbox", "loss_giou")


@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_criterion.npz"))


def _run(name, g, dtype=torch.float64, matcher=None, targets=None, num_classes=None):
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    d = torch.from_numpy(det).to(dtype)
    logits = d[..., :C].clone().requires_grad_(True)
    boxes = d[..., C:].clone().requires_grad_(True)
    tg = targets if targets is not None else cc.targets(labels, gt, offs, to=lambda t: t.to(dtype) if t.is_floating_point() else t)
    crit = L.SetCriterion(matcher or cc.FixedMatcher(cc.indices_from(g, name)), num_classes or C, dict(cc.WEIGHTS), alpha, gamma)
    ld = crit({"pred_logits": logits, "pred_boxes": boxes}, tg)
    sum(ld.values()).backward()
    return ld, logits.grad, boxes.grad


def test_golden_inputs_regenerate(g10):
    for name, case in cc.CASES.items():
        if case[4] is None:
            det, labels, gt, _ = cc.inputs(name)
            assert np.array_equal(g10[f"{name}.det"], det) and np.array_equal(g10[f"{name}.labels"], labels)
            assert np.array_equal(g10[f"{name}.gt"], gt)
        else:
            assert int(g10[f"{name}.seed"]) == case[4]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_composite_matches_reference_float64(g10, name):
    ld, gl, gb = _run(name, g10)
    assert list(ld) == list(KEYS)
    got = np.array([float(ld[k].detach()) for k in KEYS])
    np.testing.assert_allclose(got, g10[f"{name}.losses64"], rtol=1e-12, atol=1e-12)
    for got, key in ((gl, "dlogits64"), (gb, "dboxes64")):
        want = g10[f"{name}.{key}"]
        assert np.abs(got.numpy() - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), key


@pytest.mark.parametrize("name", list(cc.CASES))
def test_composite_fp32_is_at_the_reference_fp32_distance(g10, name):
    ld, gl, gb = _run(name, g10, torch.float32)
    got = np.array([float(ld[k].detach()) for k in KEYS])
    np.testing.assert_allclose(got, g10[f"{name}.losses64"], rtol=1e-5)
    for got, key in ((gl, "dlogits"), (gb, "dboxes")):
        want = g10[f"{name}.{key}64"]
        ref32 = np.abs(g10[f"{name}.{key}32"] - want).max()
        assert np.abs(got.numpy() - want).max() <= max(4 * ref32, 1e-6 * np.abs(want).max()), key


def test_tie_case_gradients(g10):
    """case 4: the exact pair has zero L1 gradient and the GIoU tie shares; the touching pair keeps the clamp's pass-through"""
    _, _, gb = _run("c4_ties", g10)
    want = g10["c4_ties.dboxes64"]
    assert np.array_equal(gb.numpy(), want)
    assert np.abs(want[0, 1]).max() > 0 and np.abs(want[0, 2:]).max() == 0


def test_empty_image_contributes_background_only(g10):
    """case 1 image 1 has empty target tensors: its rows carry focal gradient only, its box rows none"""
    _, gl, gb = _run("c1_matcher", g10)
    assert gb[1].abs().max() == 0 and gl[1].abs().max() > 0


def test_num_boxes_zero_is_clamped_to_one(g10):
    ld, _, gb = _run("c5_empty", g10)
    B, Q, C, _, _, alpha, gamma = cc.CASES["c5_empty"]
    det, _, _, _ = cc.inputs("c5_empty")
    x = torch.from_numpy(det[..., :C]).double()
    want = L.focal_terms(x, torch.zeros_like(x), alpha, gamma).sum()
    assert float(ld["loss_ce"].detach()) == pytest.approx(float(want), rel=1e-12)
    assert float(ld["loss_bbox"].detach()) == 0 and float(ld["loss_giou"].detach()) == 0 and gb.abs().max() == 0


def test_out_of_range_indices_raise_index_error(g10):
    idx = cc.indices_from(g10, "c1_matcher")
    bad = list(idx)
    bad[0] = (torch.tensor([0, 25]), torch.tensor([0, 1]))              # prediction index >= Q
    with pytest.raises(IndexError):
        _run("c1_matcher", g10, matcher=cc.FixedMatcher(bad))
    bad = list(idx)
    bad[2] = (torch.tensor([0, 1]), torch.tensor([0, 7]))               # target index >= n_b (7 targets)
    with pytest.raises(IndexError):
        _run("c1_matcher", g10, matcher=cc.FixedMatcher(bad))
    bad = list(idx)
    bad[1] = (torch.tensor([3]), torch.tensor([0]))                     # the empty image has no target 0
    with pytest.raises(IndexError):
        _run("c1_matcher", g10, matcher=cc.FixedMatcher(bad))


def test_repeated_prediction_index_raises_value_error(g10):
    bad = list(cc.indices_from(g10, "c1_matcher"))
    bad[0] = (torch.tensor([2, 2]), torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        _run("c1_matcher", g10, matcher=cc.FixedMatcher(bad))


def test_num_classes_mismatch_raises(g10):
    with pytest.raises(RuntimeError):
        _run("c1_matcher", g10, num_classes=12)


def test_label_equal_to_num_classes_is_background():
    """the reference's one-hot has C+1 columns and drops the last: a target labelled C is matched (box losses) but has no
    focal positive"""
    B, Q, C = 1, 4, 3
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, Q, C, generator=g, dtype=torch.float64)
    boxes = 0.3 + 0.2 * torch.rand(B, Q, 4, generator=g, dtype=torch.float64)
    gt = 0.3 + 0.2 * torch.rand(1, 4, generator=g, dtype=torch.float64)
    match = torch.tensor([-1, 0, -1, -1], dtype=torch.int32)
    nb = torch.ones(1)
    bg = L.composite_losses(logits, boxes, torch.tensor([C]), gt, match, nb)
    none = L.composite_losses(logits, boxes, torch.tensor([-5]), gt, match, nb)
    empty = L.composite_losses(logits, boxes, torch.zeros(0, dtype=torch.int64), gt[:0], torch.full((4,), -1, dtype=torch.int32), nb)
    assert torch.equal(bg, none) and bg[0] == empty[0] and bg[1] > 0


def test_weight_dict_and_keys_follow_the_reference(g10):
    """keys missing from weight_dict pass unweighted (losses.py:236-240)"""
    name = "c1_matcher"
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    d = torch.from_numpy(det).double()
    out = {"pred_logits": d[..., :C], "pred_boxes": d[..., C:]}
    tg = cc.targets(labels, gt, offs)
    full = L.SetCriterion(cc.FixedMatcher(cc.indices_from(g10, name)), C, {"loss_ce": 1.0, "loss_bbox": 1.0, "loss_giou": 1.0})(out, tg)
    part = L.build_criterion(cc.FixedMatcher(cc.indices_from(g10, name)), C, {"loss_bbox": 3.0})(out, tg)
    assert float(part["loss_ce"]) == float(full["loss_ce"]) and float(part["loss_giou"]) == float(full["loss_giou"])
    assert float(part["loss_bbox"]) == pytest.approx(3.0 * float(full["loss_bbox"]), rel=1e-15)


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_focal_loss_cpu(reduction):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 5, generator=g, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([0, 4, 2, 2, 1, 3, 0])
    out = L.FocalLoss(0.3, 1.5, reduction)(x, t)
    oh = torch.nn.functional.one_hot(t, 5).double()
    p = x.sigmoid()
    pt = p * oh + (1 - p) * (1 - oh)
    want = (0.3 * oh + 0.7 * (1 - oh)) * (1 - pt) ** 1.5 * -(oh * torch.log(p) + (1 - oh) * torch.log(1 - p))
    want = {"none": want, "mean": want.mean(), "sum": want.sum()}[reduction]
    torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-12)
    with pytest.raises(RuntimeError):
        L.FocalLoss()(x, torch.tensor([0, 5, 0, 0, 0, 0, 0]))


# ------------------------------------------------------------------ world size 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = torch.Generator().manual_seed(10 + rank)
        B, Q, C = 2, 6, 4
        n = (1, 2) if rank == 0 else (3, 0)          # 3 targets on each rank: num_boxes = 6
        logits = torch.randn(B, Q, C, generator=g)
        boxes = 0.3 + 0.3 * torch.rand(B, Q, 4, generator=g)
        tg = [{"labels": torch.randint(0, C, (k,), generator=g), "boxes": 0.3 + 0.3 * torch.rand(k, 4, generator=g)} for k in n]
        idx = [(torch.arange(k), torch.arange(k)) for k in n]
        ld = L.SetCriterion(cc.FixedMatcher(idx), C, {})({"pred_logits": logits, "pred_boxes": boxes}, tg)
        labels = torch.cat([t["labels"] for t in tg])
        gt = torch.cat([t["boxes"] for t in tg])
        match = L.match_table(idx, list(n), Q)
        want = L.composite_losses(logits, boxes, labels, gt, match, torch.tensor([6.0]))
        local = L.composite_losses(logits, boxes, labels, gt, match, torch.tensor([3.0]))
        got = torch.stack([ld[k] for k in KEYS])
        q.put((rank, torch.allclose(got, want, rtol=1e-6), bool(torch.allclose(got * 2, local, rtol=1e-6))))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_num_boxes_is_summed_across_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, halved in res:
        assert ok and halved, rank


def test_native_entry_points_validate_shapes_before_launch():
    """dod_set_criterion_*: bad shapes / strides return DOD_ERR_INVALID on the host, before anything is enqueued (the pointers
    below are never dereferenced)"""
    from dinov2_od_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    lib = nat.lib()
    assert lib.dod_set_criterion_workspace_bytes(2, 100, 91) == 3 * 4 * 13
    assert lib.dod_set_criterion_workspace_bytes(0, 100, 91) == 0
    p = 4096                                              # a stand-in address: validation fails before any launch

    def fwd(ls=95, bs=95, B=2, Q=100, C=91, G=5, M=200, match=p, boxes=p, gamma=2.0, wsb=1 << 20):
        return lib.dod_set_criterion_forward(p, ls, boxes, bs, B, Q, C, p, p, G, match, M, p, 0.25, gamma, p, None, p, wsb, None)

    def bwd(ls=95, bs=95, M=200, d_losses=p):
        return lib.dod_set_criterion_backward(p, ls, p, bs, 2, 100, 91, p, p, 5, p, M, p, 0.25, 2.0, d_losses, None, p, p, None)
    assert fwd(ls=90) == 1 and fwd(bs=3) == 1 and fwd(B=0) == 1 and fwd(C=0) == 1 and fwd(G=-1) == 1
    assert fwd(M=199) == 1 and fwd(match=None, M=0) == 1 and fwd(gamma=-1.0) == 1
    assert fwd(wsb=8) == 3
    assert bwd(ls=90) == 1 and bwd(bs=3) == 1 and bwd(M=7) == 1 and bwd(d_losses=None) == 1
