"""Shared cases of the deep-supervision (aux_loss) tests and of golden G11 (tests/golden/make_goldens_aux.py)."""
import numpy as np
import torch

from oracle import matching_oracle as mo
from tests import cases

# the micro decoder of G11: (Dd, Hd, Q, L, F, C, P, B, N) and the number of targets per image
MICRO = (128, 4, 7, 3, 256, 11, 2, 2, 26)
COUNTS = (3, 1)
# the whole detector of G11: cfg1 of cases.G9_CASES (ViT-S/14 lightweight, two decoder layers, dropout 0)
DETECTOR = "g9_grad_cfg1"


def micro_cfg():
    Dd, Hd, Q, L, F, C, P, B, N = MICRO
    return cases.dec_cfg(True, Dd=Dd, Hd=Hd, Q=Q, layers=L, F=F, C=C, P=P)


def targets(C, counts=COUNTS, seed=23, dtype=torch.float32, device="cpu"):
    """per image: labels in [0, C), cxcywh boxes well inside the unit square"""
    rs = np.random.RandomState(seed)
    out = []
    for n in counts:
        lab = rs.randint(0, C, size=n).astype(np.int64)
        box = np.concatenate([rs.uniform(0.3, 0.7, (n, 2)), rs.uniform(0.1, 0.4, (n, 2))], axis=1)
        out.append({"labels": torch.from_numpy(lab).to(device), "boxes": torch.from_numpy(box).to(dtype).to(device)})
    return out


class OracleMatcher:
    """the reference's HungarianMatcher on the CPU, through oracle/matching_oracle.py (cost matrices + scipy)"""

    def __call__(self, outputs, tg):
        det = torch.cat([outputs["pred_logits"], outputs["pred_boxes"]], dim=-1).detach().float().cpu().numpy()
        counts = [len(t["labels"]) for t in tg]
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        labels = np.concatenate([t["labels"].cpu().numpy() for t in tg]) if offs[-1] else np.zeros(0, np.int64)
        gt = np.concatenate([t["boxes"].detach().float().cpu().numpy() for t in tg]) if offs[-1] else np.zeros((0, 4), np.float32)
        C = outputs["pred_logits"].shape[-1]
        return [(torch.from_numpy(i), torch.from_numpy(j)) for i, j in mo.assign(mo.cost_matrices(det, C, labels, gt, offs))]


class RecordingMatcher:
    """wraps a matcher and keeps what it returned, call by call (the criterion calls it once per supervised layer)"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __call__(self, outputs, tg):
        r = self.inner(outputs, tg)
        self.calls.append([(torch.as_tensor(i).cpu().numpy().astype(np.int64), torch.as_tensor(j).cpu().numpy().astype(np.int64)) for i, j in r])
        return r


def golden_indices(g, tag, layer, B):
    return [(g[f"{tag}.l{layer}.src{b}"].astype(np.int64), g[f"{tag}.l{layer}.tgt{b}"].astype(np.int64)) for b in range(B)]


def same_assignment(a, b):
    """two lists of (pred_idx, tgt_idx) per image hold the same pairs"""
    return len(a) == len(b) and all(sorted(zip(i.tolist(), j.tolist())) == sorted(zip(k.tolist(), l.tolist())) for (i, j), (k, l) in zip(a, b))


def grad_check(model, g, tol_probe, tol_norm, metric=None):
    """cases.g9_check's rule on a G11 file (every recorded gradient: probe entries, L2 norm and abs-sum of the whole tensor; the
    tensors the reference's loss does not reach are unreached here too), returning the worst (probe error, name) -- an exact match
    (error 0.0) included, which g9_check's tuple comparison cannot order"""
    metric = metric or cases.rel_err
    params = dict(model.named_parameters())
    worst, bad = (-1.0, ""), []
    for k in map(str, g["trainable_with_grad"]):
        assert k in params and params[k].grad is not None, f"no gradient for {k}"
        pr, st = cases.grad_probe(params[k].grad.detach().cpu().numpy())
        e = metric(pr, g["grad:" + k])
        worst = max(worst, (float(e), k))
        en = abs(st[2] - g["stat:" + k][2]) / max(g["stat:" + k][2], 1e-30)
        ea = abs(st[1] - g["stat:" + k][1]) / max(g["stat:" + k][1], 1e-30)
        if not (e < tol_probe and en <= tol_norm and ea <= tol_norm):
            bad.append((k, float(e), float(en), float(ea)))
    assert not bad, f"{len(bad)} gradients outside (probe {tol_probe:g}, norms {tol_norm:g}): {bad[:6]}"
    want = {str(k) for k in g["trainable_with_grad"]}
    have = {k for k, p in params.items() if p.grad is not None and float(p.grad.abs().sum()) > 0}
    assert have == want, have ^ want
    return worst
