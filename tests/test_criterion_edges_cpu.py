"""CPU checks of tests/criterion_edge_cases.py, which the GPU tests of csrc/criterion.hip and csrc/matchcost.hip rely on: its float64
reference against float64 autograd of losses.composite_losses where that is well conditioned, the written-out tie rules against autograd
on all 196 grid pairs, and a numpy fp32 restatement of the kernels' statements inside every bound on every case with no element excluded.
torch's own fp32 composite is printed against the same bounds as a yardstick (its formula rounds differently: not asserted)."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import losses as L
from tests import criterion_edge_cases as ce


def test_ladder_and_grid_are_what_the_issue_lists():
    assert len(ce.LADDER) == 29 and len(set(ce.LADDER.tolist())) == 29
    d = ce.ladder_case()
    pos = np.zeros(d["logits"].shape, bool)
    pos[np.arange(29), d["labels"]] = True
    assert sorted(d["logits"][pos].tolist()) == sorted(ce.LADDER.tolist())                     # each value once as a matched row's target column
    assert all((d["logits"][~pos] == v).sum() >= 1 for v in ce.LADDER)                        # and as a background entry
    g = ce.grid_boxes()
    assert g.shape == (196, 4) and len({tuple(r) for r in g.tolist()}) == 196
    p, t, rejected = ce.random_pairs()
    print(f"random pairs: {rejected} candidates rejected for 512 kept (margin 2^-10)")
    assert len(p) == 512 and (ce._margins(p, t) > ce.MARGIN).all() and rejected > 0


@pytest.mark.parametrize("gamma", [1.0, 1.5, 2.0, 3.0])
def test_reference_is_float64_autograd_of_the_composite_where_well_conditioned(gamma):
    """|x| <= 12 (the composite forms 1 - p_t by subtraction) and gamma >= 1 (autograd of pow at base 0 aside)"""
    d = ce.geometry_case(11, 20)
    d["logits"] = np.clip(d["logits"], -12, 12)
    a = dict(d, nb=2.5, alpha=0.4, gamma=gamma, d_losses=np.array([0.75, 5.0, 2.0], np.float32), d_elem=None)
    ref, want = ce.reference(**a), ce.composite(a, torch.float64)
    for k in ("losses", "d_logits", "d_boxes"):
        err = np.abs(ref[k] - want[k])
        # the composite's 1 - p_t carries an absolute 1.1e-16: S of the bound, times float64's unit roundoff instead of u
        tol = 64 * 2.0 ** -53 * (np.abs(want[k]) + ref[k + "_bound"] / ce.U) if k != "losses" else 1e-13 * np.abs(want[k])
        assert (err <= tol).all(), (k, float((err / np.maximum(tol, 1e-300)).max()))


def test_tie_rules_are_autograd_on_all_grid_pairs():
    g = ce.grid_boxes()
    ar = ce.RunArith()
    one = ce.Run(np.ones(196))
    _, lg, d = ce.box_statements(g.astype(np.float64), np.repeat(ce.GRID_GT[None].astype(np.float64), 196, 0), ce.Run(np.zeros(196)), -one, ar)
    assert not ar.undecided
    src = torch.from_numpy(g).double().requires_grad_(True)
    loss = 1 - L.pair_giou(src, torch.from_numpy(ce.GRID_GT).double().expand(196, 4))
    loss.sum().backward()
    mine = np.stack([c.v for c in d], 1)
    assert np.isfinite(mine).all() and np.isfinite(lg.v).all()
    err = np.abs(mine - src.grad.numpy()).max()
    print(f"tie rules vs float64 autograd of pair_giou on 196 pairs: max |d| {err:.2e}")
    assert err <= 2e-15 and np.abs(lg.v - loss.detach().numpy()).max() <= 2e-15
    bound = np.stack([c.e for c in d], 1)
    print(f"grid: largest box-gradient bound at upstream 1: {bound.max() / ce.U:.1f} u")


@pytest.mark.parametrize("family", ce.FAMILIES)
def test_fp32_restatement_is_inside_every_bound(family):
    worst, yard = {}, {}
    n = 0
    for case in ce.cases(family):
        for l in range(len(case["layers"])):
            a = ce.layer_args(case, l)
            ref = ce.reference(**a)
            got = ce.restate32(**a)
            for k in ce.OUTPUTS:                                                             # nothing excluded: every output present has a finite bound
                if k in got:
                    assert k in ref and np.isfinite(ref[k + "_bound"]).all() and ref[k].shape == np.asarray(got[k]).shape
                    n += np.asarray(got[k]).size
            ce.check(got, ref, f"{case['name']} layer {l}", worst)
            if ce.has_yardstick(a):
                for k, v in ce.ratios(ce.composite(a, torch.float32), ref).items():
                    yard[k] = max(yard.get(k, 0.0), v)
    print(f"{family}: {n} elements; worst error / bound, fp32 restatement: {ce.fmt(worst)} | torch fp32 composite: {ce.fmt(yard)}")
    assert n > 0 and worst


@pytest.mark.parametrize("gamma", [2.0, 1.5, 0.5])
@pytest.mark.parametrize("rows_from", [0, -1])
def test_cost_restatement_is_inside_the_running_bound(gamma, rows_from):
    case = ce.cost_case()
    w = (2.0, 5.0, 3.0)
    ar = ce.RunArith()
    want = ce.cost_expected(case, w, 0.4, gamma, rows_from, ar)
    with np.errstate(all="ignore"):
        got = ce.cost_expected(case, w, 0.4, gamma, rows_from, ce.F32Arith())
    assert not ar.undecided and len(want) == 2
    worst = 0.0
    for g, r in zip(got, want):
        assert np.isfinite(r.v).all() and np.isfinite(r.e).all() and np.isfinite(g).all()
        worst = max(worst, float((np.abs(g.astype(np.float64) - r.v) / r.e).max()))
    print(f"cost gamma={gamma} rows_from={rows_from}: worst error / bound of the fp32 restatement {worst:.3f}")
    assert worst <= 1.0
