"""`-m gpu`: csrc/criterion.hip per element.  Every call of tests/criterion_edge_cases.py (saturated logits, every gamma branch, class
counts and row counts around the 64-lane stride / 4 rows per wave / 16 rows per workgroup, the 196 dyadic box pairs and 512 random ones,
labels and match entries outside their ranges, every num_boxes, elem_loss / d_elem single-layer and layered, three layers with their own
match tables) goes through dod_set_criterion_layers_{forward,backward} on strided NaN-padded inputs into NaN-filled outputs between
canaries; each element of losses, elem_loss, d_logits and d_boxes is held to its float64 reference within the bound derived in DESIGN.md
section 6b, none excluded.  torch's fp32 composite on the same device is printed against the same bounds (not asserted).
The matcher's cost kernel (csrc/matchcost.hip) gets the grid and the saturation ladder entry by entry against its own formula in float64."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import criterion_edge_cases as ce

pytestmark = pytest.mark.gpu
CANARY = 12345.0
PAD, GUARD_ROWS = 5, 8


def _guarded(n, dev):
    """n NaN floats to be written, between two 64-float canaries -> (whole buffer, the view)"""
    buf = torch.full((n + 128,), CANARY, dtype=torch.float32, device=dev)
    buf[64:64 + n] = float("nan")
    return buf, buf[64:64 + n]


def _intact(buf, n):
    return bool((buf[:64] == CANARY).all()) and bool((buf[64 + n:] == CANARY).all())


def run_native(case):
    """one layered forward + backward of a case -> per layer {losses, elem, d_logits, d_boxes} as numpy"""
    dev = torch.device("cuda:0")
    lib, s = nat.lib(), nat.stream_ptr()
    lays = case["layers"]
    nl = len(lays)
    R, Cc = lays[0]["logits"].shape
    B, Q = (3, R // 3) if R % 3 == 0 else (1, R)
    boxed = lays[0]["boxes"] is not None
    W = Cc + PAD + 4                                            # logits | NaN pad | boxes; NaN rows behind the last row
    det = torch.full((nl * R + GUARD_ROWS, W), float("nan"), dtype=torch.float32, device=dev)
    det[:nl * R, :Cc] = torch.from_numpy(np.concatenate([l["logits"] for l in lays])).to(dev)
    if boxed:
        det[:nl * R, Cc + PAD:] = torch.from_numpy(np.concatenate([l["boxes"] for l in lays])).to(dev)
    lg, bx = det[:, :Cc], (det[:, Cc + PAD:] if boxed else None)
    labels = torch.from_numpy(case["labels"]).to(dev)
    gt = torch.from_numpy(case["gt"]).to(dev) if boxed else None
    G = int(labels.numel())
    match = None if case["identity"] else torch.from_numpy(np.concatenate([l["match"] for l in lays]).astype(np.int32)).to(dev)
    nb = None if case["nb"] is None else torch.tensor([case["nb"]], dtype=torch.float32, device=dev)
    dl = None if case["d_losses"] is None else torch.from_numpy(np.ascontiguousarray(case["d_losses"], np.float32)).to(dev)
    de = None if case["d_elem"] is None else torch.from_numpy(np.ascontiguousarray(case["d_elem"], np.float32)).to(dev)
    a, g = float(case["alpha"]), float(case["gamma"])
    M = nl * R if match is not None else 0
    ws = torch.empty(lib.dod_set_criterion_layers_workspace_bytes(nl, B, Q, Cc) // 4, dtype=torch.float32, device=dev)
    lbuf, losses = _guarded(nl * 3, dev)
    ebuf, elem = _guarded(nl * R * Cc, dev)
    nat.check(lib.dod_set_criterion_layers_forward(nat.ptr(lg), W, nat.ptr(bx), W, nl, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G, nat.ptr(match), M,
                                                   nat.ptr(nb), a, g, nat.ptr(losses), nat.ptr(elem), nat.ptr(ws), ws.numel() * 4, s))
    out = {"losses": (lbuf, losses, (nl, 3)), "elem": (ebuf, elem, (nl, R, Cc))}
    if dl is not None or de is not None:
        out["d_logits"] = _guarded(nl * R * Cc, dev) + ((nl, R, Cc),)
        if boxed and dl is not None:
            out["d_boxes"] = _guarded(nl * R * 4, dev) + ((nl, R, 4),)
        nat.check(lib.dod_set_criterion_layers_backward(nat.ptr(lg), W, nat.ptr(bx), W, nl, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G, nat.ptr(match), M,
                                                        nat.ptr(nb), a, g, nat.ptr(dl), nat.ptr(de), nat.ptr(out["d_logits"][1]),
                                                        nat.ptr(out["d_boxes"][1]) if "d_boxes" in out else None, s))
    torch.cuda.synchronize()
    res = {}
    for k, (buf, view, shape) in out.items():
        assert _intact(buf, view.numel()), f"{case['name']}: {k} written outside its extent"
        v = view.cpu().numpy().reshape(shape)
        assert not np.isnan(v).any(), f"{case['name']}: an element of {k} was not written"
        res[k] = v
    return [{k: v[l] for k, v in res.items()} for l in range(nl)]


@pytest.mark.parametrize("family", ce.FAMILIES)
def test_every_element_within_its_float64_bound(family):
    worst, yard = {}, {}
    for case in ce.cases(family):
        got = run_native(case)
        for l, g in enumerate(got):
            a = ce.layer_args(case, l)
            ref = ce.reference(**a)
            if ce.has_yardstick(a):
                for k, v in ce.ratios(ce.composite(a, torch.float32, "cuda:0"), ref).items():
                    yard[k] = max(yard.get(k, 0.0), v)
            r = ce.check(g, ref, f"{case['name']} layer {l}", worst)
            assert set(r) == {k for k in ce.OUTPUTS if k in ref}, (case["name"], sorted(r))      # nothing the reference bounds went unchecked
            # the three summed losses keep the tensor-wide 1e-5 as well
            assert (np.abs(g["losses"] - ref["losses"]) <= 1e-5 * np.abs(ref["losses"])).all(), (case["name"], l, g["losses"], ref["losses"])
    print(f"{family}: worst error / bound, kernel: {ce.fmt(worst)} | torch fp32 composite: {ce.fmt(yard)}")


def test_d_elem_is_the_gradient_of_the_unnormalised_elem_loss():
    """elem_loss does not depend on num_boxes, so neither does d_elem's gradient: the calls at num_boxes = 2.5 and NULL agree bit for bit
    (on top of the per-element check of the "element" family, which a division by num_boxes misses by a factor 2.5)"""
    by_name = {c["name"]: c for c in ce.cases("element")}
    for nl in (1, 3):
        for kind in ("d_elem and d_losses, boxes", "d_elem alone, no boxes, match NULL"):
            a, b = (run_native(by_name[f"{kind}, nl={nl} nb={nb}"]) for nb in (None, 2.5))
            for x, y in zip(a, b):
                for k in ("elem", "d_logits"):
                    assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), (kind, nl, k)


@pytest.mark.parametrize("gamma", [2.0, 1.5, 0.5])
@pytest.mark.parametrize("rows_from", [0, -1])
def test_match_cost_entries_against_the_kernel_formula_in_float64(gamma, rows_from):
    """the 196 grid boxes and the saturation ladder as prediction rows against the one grid target, an image without targets in the middle
    of the offsets; every entry within the running error of the kernel's own statements (1e-8 inside the logs included)"""
    from dinov2_od_amd import matching
    case = ce.cost_case()
    w, alpha = (2.0, 5.0, 3.0), 0.4
    ar = ce.RunArith()
    want = ce.cost_expected(case, w, alpha, gamma, rows_from, ar)
    assert not ar.undecided
    Q = case["det"].shape[1]
    cost = matching.match_cost(torch.from_numpy(case["det"]).cuda(), case["C"], torch.from_numpy(case["labels"]).cuda(), torch.from_numpy(case["gt"]).cuda(),
                               torch.from_numpy(case["offs"]).cuda(), cost_class=w[0], cost_bbox=w[1], cost_giou=w[2], focal_alpha=alpha,
                               focal_gamma=gamma, rows_from=rows_from).cpu().numpy()
    assert cost.shape == (2 * Q,)
    worst = 0.0
    for j, r in enumerate(want):
        got = cost[j * Q:(j + 1) * Q].astype(np.float64)
        assert np.isfinite(got).all() and np.isfinite(r.e).all()
        ratio = np.abs(got - r.v) / r.e
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (j, int(ratio.argmax()), float(ratio.max()))
    print(f"match cost gamma={gamma} rows_from={rows_from}: worst error / bound {worst:.3f}")
