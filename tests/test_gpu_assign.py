"""`-m gpu`: the device Hungarian assignment (csrc/assign.hip, dod_match_assign) through `matching.assign`,
`HungarianMatcher.match_table` and `SetCriterion(device_assignment=True)`.  The device solver restates scipy's
linear_sum_assignment operation for operation in double precision, so every comparison here is EXACT: the same indices in the
same order, the same status (scipy's exception) image by image, losses and gradients `torch.equal` to the host path's."""
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from dinov2_od_amd import losses as L, synth
from tests import cases, criterion_cases as cc

pytestmark = pytest.mark.gpu
KW2 = dict(cost_class=2.0, cost_bbox=1.0, cost_giou=3.0, focal_alpha=0.4, focal_gamma=1.5)


@pytest.fixture(scope="module")
def mt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import matching
    return matching


def _dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------ host yardstick: scipy, image by image
def _scipy_status(M):
    """(row_ind, col_ind, status): scipy's result, or its exception as the documented status code"""
    try:
        i, j = linear_sum_assignment(M)
        return i, j, 0
    except ValueError as e:
        msg = str(e)
        assert msg in ("matrix contains invalid numeric entries", "cost matrix is infeasible"), msg
        return None, None, 1 if "invalid" in msg else 2


def _flat(mats, Q):
    """list of [Q, n_b] fp32 matrices -> (flat buffer as match_cost lays it out, int32 offsets [B+1])"""
    offs = np.concatenate([[0], np.cumsum([m.shape[1] for m in mats])]).astype(np.int32)
    flat = np.concatenate([np.ascontiguousarray(m, np.float32).reshape(-1) for m in mats] + [np.zeros(0, np.float32)])
    assert flat.size == offs[-1] * Q
    return flat, offs


def _expected(mats, Q, offs):
    """the table losses.match_table builds from scipy's indices (failing images all -1) and the per-image statuses"""
    table = np.full(len(mats) * Q, -1, np.int32)
    status = np.zeros(len(mats), np.int32)
    for b, M in enumerate(mats):
        i, j, st = _scipy_status(M)
        status[b] = st
        if st == 0 and len(i):
            table[b * Q + i] = offs[b] + j
    return table, status


def _pairs(table, offs, Q, b):
    """(row_ind, col_ind) of image b read back from a table: queries ascending, as scipy returns them in both orientations"""
    row = table[b * Q:(b + 1) * Q]
    i = np.nonzero(row >= 0)[0]
    return i, row[i] - offs[b]


def _assign(mt, mats, Q, labels=None, C=None):
    flat, offs = _flat(mats, Q)
    lab = None if labels is None else torch.from_numpy(labels).to(_dev())
    match, status = mt.assign(torch.from_numpy(flat).to(_dev()), torch.from_numpy(offs).to(_dev()), Q, lab, C)
    assert match.dtype == torch.int32 and status.dtype == torch.int32 and match.is_cuda and status.is_cuda
    return match.cpu().numpy(), status.cpu().numpy(), offs


# ------------------------------------------------------------------ 1. golden G6: the reference's own matrices and assignments
@pytest.mark.parametrize("tag,kw", [("default", {}), ("g15", KW2)])
def test_reference_golden_g6(mt, tag, kw):
    g = cases.golden("g6_matcher")
    det, labels, gt, offs = g["det"], g["labels"], g["gt"], g["offs"]
    B, Q = det.shape[:2]
    C = det.shape[-1] - 4
    mats = [g[f"{tag}_cost{b}"] for b in range(B)]
    assert [m.shape for m in mats] == [(Q, offs[b + 1] - offs[b]) for b in range(B)]          # 25x4, 25x0, 25x7, 25x30
    table, status, o2 = _assign(mt, mats, Q)
    assert np.array_equal(o2, offs) and not status.any()
    for b in range(B):
        i, j = _pairs(table, offs, Q, b)
        assert np.array_equal(i, g[f"{tag}_i{b}"]) and np.array_equal(j, g[f"{tag}_j{b}"]), b
    d = torch.from_numpy(det).to(_dev())
    tg = [{"labels": torch.from_numpy(labels[offs[b]:offs[b + 1]]).to(_dev()), "boxes": torch.from_numpy(gt[offs[b]:offs[b + 1]]).to(_dev())}
          for b in range(B)]
    match, st = mt.HungarianMatcher(**kw).match_table({"pred_logits": d[..., :C], "pred_boxes": d[..., C:]}, tg)
    match = match.cpu().numpy()
    assert not st.cpu().numpy().any()
    for b in range(B):
        i, j = _pairs(match, offs, Q, b)
        assert np.array_equal(i, g[f"{tag}_i{b}"]) and np.array_equal(j, g[f"{tag}_j{b}"]), b


# ------------------------------------------------------------------ 2. against scipy on seeded matrices
KINDS = ("uniform", "int012", "const", "decimal", "inf_feasible", "inf_dense", "inf_infeasible", "nan", "neginf")


def _matrix(rng, kind, Q, n):
    if kind == "uniform":
        M = rng.random((Q, n))
    elif kind == "int012":
        M = rng.integers(0, 3, (Q, n)).astype(np.float64)
    elif kind == "const":
        M = np.full((Q, n), rng.choice([0.0, 1.0, -2.5, 7.0]))
    elif kind == "decimal":
        M = np.round(rng.uniform(-1.0, 1.0, (Q, n)), 1)
    elif kind in ("inf_feasible", "inf_dense"):
        M = np.round(rng.uniform(0.0, 2.0, (Q, n)), 1)
        M[rng.random((Q, n)) < (0.4 if kind == "inf_feasible" else 0.8)] = np.inf
        if kind == "inf_feasible":                     # keep one complete matching finite
            k = min(Q, n)
            M[rng.permutation(Q)[:k], rng.permutation(n)[:k]] = rng.random(k)
    elif kind == "inf_infeasible":                     # a whole line of the smaller side is +inf
        M = rng.integers(0, 3, (Q, n)).astype(np.float64)
        if n and n < Q:
            M[:, rng.integers(n)] = np.inf
        elif n:
            M[rng.integers(Q), :] = np.inf
    else:
        M = rng.random((Q, n))
        if n:
            M[rng.integers(Q), rng.integers(n)] = np.nan if kind == "nan" else -np.inf
    return M.astype(np.float32)


def _batch(Q, B, nmax, seed, extra=()):
    rng = np.random.default_rng(seed)
    ns = [0, Q + 1] + list(extra) + [int(x) for x in rng.integers(0, nmax + 1, B - 2 - len(extra))]
    return [_matrix(rng, KINDS[b % len(KINDS)], Q, n) for b, n in enumerate(ns)]


def _check_against_scipy(mt, mats, Q):
    table, status, offs = _assign(mt, mats, Q)
    want, wst = _expected(mats, Q, offs)
    bad = np.nonzero(status != wst)[0]
    assert not bad.size, f"status differs at images {bad[:10]}: {status[bad[:10]]} vs scipy {wst[bad[:10]]}"
    for b in range(len(mats)):
        assert np.array_equal(table[b * Q:(b + 1) * Q], want[b * Q:(b + 1) * Q]), (b, mats[b].shape)
    return wst


# (Q, images, largest n_b, extra n_b values): ragged widths with 0 and widths above Q in every launch
SCIPY_SETS = [(1, 500, 4, ()), (7, 500, 12, ()), (25, 500, 40, ()), (100, 400, 130, ()), (300, 120, 100, (301, 320, 450))]


@pytest.mark.parametrize("Q,B,nmax,extra", SCIPY_SETS)
def test_against_scipy_seeded(mt, Q, B, nmax, extra):
    mats = _batch(Q, B, nmax, seed=1000 + Q, extra=extra)
    wst = _check_against_scipy(mt, mats, Q)
    print(f"Q={Q}: {len(mats)} matrices, statuses {np.bincount(wst, minlength=3)}")
    assert (wst == 0).sum() > B // 2 and (wst == 1).any() and (wst == 2).any()


def test_scipy_sets_cover_at_least_2000_matrices():
    assert sum(B for _, B, _, _ in SCIPY_SETS) >= 2000


def test_square_300_and_state_outside_lds(mt):
    """one 300x300 uniform matrix, plus images whose rows + columns exceed the LDS budget (state in the workspace) in the
    same launch as small ones"""
    rng = np.random.default_rng(7)
    _check_against_scipy(mt, [rng.random((300, 300)).astype(np.float32)], 300)
    mats = [rng.random((25, 1700)).astype(np.float32), _matrix(rng, "int012", 25, 1600), _matrix(rng, "decimal", 25, 9),
            _matrix(rng, "inf_dense", 25, 1650), np.zeros((25, 0), np.float32)]
    _check_against_scipy(mt, mats, 25)
    mats = [rng.random((1700, 3)).astype(np.float32), _matrix(rng, "int012", 1700, 40), _matrix(rng, "nan", 1700, 5)]
    _check_against_scipy(mt, mats, 1700)


def test_b64_q300_50_to_100_targets(mt):
    rng = np.random.default_rng(64)
    mats = [rng.random((300, int(n))).astype(np.float32) for n in rng.integers(50, 101, 64)]
    assert not _check_against_scipy(mt, mats, 300).any()


def test_labels_out_of_range_is_status_3(mt):
    rng = np.random.default_rng(3)
    mats = [rng.random((7, n)).astype(np.float32) for n in (3, 2, 0, 4)]
    labels = np.array([0, 1, 4, 2, 3, 0, 1, 2, 3], np.int64)       # C = 5: all valid
    table, status, offs = _assign(mt, mats, 7, labels, 5)
    want, wst = _expected(mats, 7, offs)
    assert not status.any() and np.array_equal(table, want)
    for k, v in ((3, 5), (4, -1)):                                 # image 1 (targets 3, 4): label == C, then negative
        lab = labels.copy()
        lab[k] = v
        table, status, _ = _assign(mt, mats, 7, lab, 5)
        assert status.tolist() == [0, 3, 0, 0]
        assert (table[7:14] == -1).all()
        keep = np.r_[0:7, 14:28]
        assert np.array_equal(table[keep], want[keep])
    table, status, _ = _assign(mt, [np.zeros((7, 0), np.float32)] * 3, 7)   # no targets anywhere (G = 0)
    assert not status.any() and (table == -1).all()


# ------------------------------------------------------------------ 3. G10 cases and training shapes through the matcher and the criterion
def _outputs(d, C):
    return {"pred_logits": d[..., :C], "pred_boxes": d[..., C:]}


def _host_table(mt, matcher, out, tg, Q):
    counts = [0 if len(t) == 0 else int(t["labels"].numel()) for t in tg]
    return L.match_table(matcher(out, tg), counts, Q).numpy()


def _crit_run(det, C, tg, matcher, device, alpha, gamma):
    d = torch.from_numpy(det).to(_dev()).requires_grad_(True)
    crit = L.SetCriterion(matcher, C, dict(cc.WEIGHTS), alpha, gamma, device_assignment=device)
    ld = crit(_outputs(d, C), tg)
    sum(ld.values()).backward()
    if device:
        crit.check_assignment()
    return torch.stack([ld[k].detach() for k in L.LOSS_KEYS]), d.grad.detach()


def _table_and_criterion_agree(mt, det, C, tg, Q, alpha, gamma, per_image_rows):
    m = mt.HungarianMatcher(focal_alpha=alpha, focal_gamma=gamma, per_image_rows=per_image_rows)
    out = _outputs(torch.from_numpy(det).to(_dev()), C)
    want = _host_table(mt, m, out, tg, Q)
    match, st = m.match_table(out, tg)
    assert not st.cpu().numpy().any()
    assert np.array_equal(match.cpu().numpy(), want)
    lh, gh = _crit_run(det, C, tg, m, False, alpha, gamma)
    ld, gd = _crit_run(det, C, tg, m, True, alpha, gamma)
    assert torch.equal(lh, ld) and torch.equal(gh, gd)
    return want


@pytest.mark.parametrize("per_image_rows", [False, True])
@pytest.mark.parametrize("name", list(cc.CASES))
def test_g10_cases(mt, g10_file, name, per_image_rows):
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    tg = cc.targets(labels, gt, offs, to=lambda t: t.to(_dev()))
    table = _table_and_criterion_agree(mt, det, C, tg, Q, alpha, gamma, per_image_rows)
    if not per_image_rows or B == 1:                  # the reference matcher (recorded in G10) reads image 0's rows for every image
        want = L.match_table(cc.indices_from(g10_file, name), list(counts), Q).numpy()
        assert np.array_equal(table, want)


@pytest.fixture(scope="module")
def g10_file(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_criterion.npz"))


@pytest.mark.parametrize("per_image_rows", [False, True])
@pytest.mark.parametrize("B,Q,C,lo,hi", [(16, 100, 91, 0, 40), (64, 300, 91, 0, 100)])
def test_training_shapes(mt, B, Q, C, lo, hi, per_image_rows):
    rng = np.random.default_rng(B + Q)
    counts = [int(n) for n in rng.integers(lo, hi + 1, B)]
    counts[1] = 0                                      # a zero-box image
    det, labels, gt, offs = cc.synth_inputs(B, Q, C, counts, seed=B * Q)
    tg = cc.targets(labels, gt, offs, to=lambda t: t.to(_dev()))
    _table_and_criterion_agree(mt, det, C, tg, Q, 0.25, 2.0, per_image_rows)
    # an empty target dict short-circuits in forward (matching.py:73-75); match_table follows it
    tg[3] = {}
    m = mt.HungarianMatcher(per_image_rows=per_image_rows)
    out = _outputs(torch.from_numpy(det).to(_dev()), C)
    match, st = m.match_table(out, tg)
    assert not st.cpu().numpy().any() and np.array_equal(match.cpu().numpy(), _host_table(mt, m, out, tg, Q))


# ------------------------------------------------------------------ 4. no host sync in the device-mode criterion
def _sleep_cycles(ms=100.0):
    """torch.cuda._sleep cycles that keep the stream busy for >= 50 ms (calibrated once with events)"""
    cycles = 1 << 20
    for _ in range(8):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        torch.cuda._sleep(cycles)
        e.record()
        e.synchronize()
        t = s.elapsed_time(e)
        if t >= 50.0:
            return cycles
        cycles = int(cycles * min(100.0, 1.2 * ms / max(t, 0.01)))
    raise AssertionError(f"could not calibrate a 50 ms sleep ({t:.2f} ms at {cycles} cycles)")


def test_device_mode_does_not_synchronise(mt):
    B, Q, C = 16, 100, 91
    rng = np.random.default_rng(16)
    counts = [int(n) for n in rng.integers(1, 21, B)]
    det, labels, gt, offs = cc.synth_inputs(B, Q, C, counts, seed=5)
    tg = cc.targets(labels, gt, offs, to=lambda t: t.to(_dev()))    # already on the device, as train.py:1071-1072 puts them
    d = torch.from_numpy(det).to(_dev()).requires_grad_(True)
    cycles = _sleep_cycles()
    res = {}
    for device in (True, False):
        crit = L.SetCriterion(mt.HungarianMatcher(), C, dict(cc.WEIGHTS), device_assignment=device)

        def step():
            d.grad = None
            ld = crit(_outputs(d, C), tg)
            sum(ld.values()).backward()
            return ld

        for _ in range(2):                              # warm-up: settles the device and pinned-host caching allocators
            step()
        torch.cuda.synchronize()
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record()
        ld = step()
        done = ev.query()
        torch.cuda.synchronize()
        print(f"device_assignment={device}: event complete when the call returned: {done}")
        assert done is (not device), "the device path synchronised" if device else "the control did not see the host sync"
        res[device] = (torch.stack([ld[k].detach() for k in L.LOSS_KEYS]), d.grad.detach().clone())
        if device:
            crit.check_assignment()
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


# ------------------------------------------------------------------ 5. deferred errors
def _scipy_rows(mt, det, C, labels, gt, offs, Q, skip):
    """the host table of every image but `skip`, by scipy on the same device costs"""
    cost = mt.match_cost(torch.from_numpy(det).to(_dev()), C, torch.from_numpy(labels).to(_dev()).clamp(0, C - 1),
                         torch.from_numpy(gt).to(_dev()), torch.from_numpy(offs).to(_dev())).cpu().numpy()
    table = np.full((len(offs) - 1) * Q, -1, np.int32)
    for b in range(len(offs) - 1):
        n = offs[b + 1] - offs[b]
        if b in skip or n == 0:
            continue
        i, j = linear_sum_assignment(cost[offs[b] * Q:offs[b + 1] * Q].reshape(Q, n))
        table[b * Q + i] = offs[b] + j
    return table


@pytest.mark.parametrize("fault", ["nan_box", "bad_label", "both"])
def test_deferred_errors(mt, fault):
    B, Q, C = 4, 25, 11
    det, labels, gt, offs = cc.synth_inputs(B, Q, C, (3, 5, 0, 6), seed=77)
    if fault in ("nan_box", "both"):
        gt[offs[1] + 2, 0] = np.nan                    # image 1
    if fault in ("bad_label", "both"):
        labels[offs[3] + 1] = C                        # image 3
    tg = cc.targets(labels, gt, offs, to=lambda t: t.to(_dev()))
    d = torch.from_numpy(det).to(_dev())
    exc = IndexError if fault != "nan_box" else ValueError
    with pytest.raises(exc) as host:
        L.SetCriterion(mt.HungarianMatcher(), C, dict(cc.WEIGHTS))(_outputs(d, C), tg)
    crit = L.SetCriterion(mt.HungarianMatcher(), C, dict(cc.WEIGHTS), device_assignment=True)
    crit(_outputs(d, C), tg)                           # nothing raised yet
    with pytest.raises(exc) as dev:
        crit.check_assignment()
    assert type(dev.value) is type(host.value) and str(dev.value) == str(host.value)
    failing = {"nan_box": {1}, "bad_label": {3}, "both": {1, 3}}[fault]
    st = crit.last_assignment_status.cpu().numpy()
    assert st.tolist() == [0, 1 if 1 in failing else 0, 0, 3 if 3 in failing else 0]
    match, _ = mt.HungarianMatcher().match_table(_outputs(d, C), tg)
    match = match.cpu().numpy()
    want = _scipy_rows(mt, det, C, labels, gt, offs, Q, failing)
    for b in range(B):
        assert np.array_equal(match[b * Q:(b + 1) * Q], want[b * Q:(b + 1) * Q]), b
        if b in failing:
            assert (match[b * Q:(b + 1) * Q] == -1).all()


# ------------------------------------------------------------------ 6. a train step with the device assignment
def test_train_step_with_device_assignment():
    """test_gpu_criterion.py::test_train_step_with_the_native_criterion's setup (cfg1, deterministic option) with
    device_assignment=True: gradients bit-identical to the host mode's, and six AdamW steps lower the loss"""
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
    W = dict(cc.WEIGHTS)

    def grads(device):
        m.zero_grad(set_to_none=True)
        crit = L.SetCriterion(HungarianMatcher(), dc.num_classes, W, device_assignment=device)
        ld = crit(m(x), targets)
        loss = sum(ld.values())
        loss.backward()
        if device:
            crit.check_assignment()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    nat.set_option("deterministic", 1)
    try:
        l_host, g_host = grads(False)
        l_dev, g_dev = grads(True)
    finally:
        nat.set_option("deterministic", -1)
    assert torch.equal(l_host, l_dev), (float(l_host), float(l_dev))
    assert set(g_host) == set(g_dev) and any(k.startswith("decoder.") for k in g_dev)
    for k in g_host:
        assert torch.equal(g_host[k], g_dev[k]), k
    crit = L.SetCriterion(HungarianMatcher(), dc.num_classes, W, device_assignment=True)
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=2e-3)
    hist = []
    for _ in range(6):
        ld = crit(m(x), targets)
        loss = sum(ld.values())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        crit.check_assignment()
        hist.append(float(loss.detach()))
    print("device-assignment train losses", hist)
    assert all(np.isfinite(hist)) and min(hist[-2:]) < hist[0], hist
