#!/usr/bin/env python3
"""Generate golden G10 (tests/golden/g10_criterion.npz) by running THE REFERENCE's own criterion.

For every case of tests/criterion_cases.py the reference's HungarianMatcher (matching.py) assigns, then the reference's
SetCriterion (losses.py:71-242) with config.py's loss weights {ce: 1, bbox: 5, giou: 2} computes the weighted losses and its
autograd gives d loss / d pred_logits and d loss / d pred_boxes for loss = sum(loss_dict.values()) (train.py:1088-1101),
in fp32 and in float64 (the float64 run reuses the fp32 run's assignment).  Stored: the matched indices, the losses and
gradients of both precisions, and the inputs' synth seeds (case 4's hand-written inputs are stored as arrays).

  python tests/golden/make_goldens_criterion.py

Runs only where the reference is importable (see make_goldens.py, whose loader and _save this script reuses).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_goldens import _save, matcher_inputs  # noqa: E402  (imports the reference)
from tests import criterion_cases as cc  # noqa: E402


def _run(name, dtype, indices=None):
    import dino_detector.losses as rl
    import dino_detector.matching as rm
    B, Q, C, counts, seed, alpha, gamma = cc.CASES[name]
    det, labels, gt, offs = cc.inputs(name)
    d = torch.from_numpy(det).to(dtype)
    logits = d[..., :C].clone().requires_grad_(True)
    boxes = d[..., C:].clone().requires_grad_(True)
    tg = cc.targets(labels, gt, offs, to=lambda t: t.to(dtype) if t.is_floating_point() else t)
    outputs = {"pred_logits": logits, "pred_boxes": boxes}
    if indices is None:
        indices = rm.HungarianMatcher(cost_class=1, cost_bbox=5, cost_giou=2, focal_alpha=alpha, focal_gamma=gamma)(outputs, tg)
    crit = rl.SetCriterion(cc.FixedMatcher(indices), C, dict(cc.WEIGHTS), focal_alpha=alpha, focal_gamma=gamma)
    ld = crit(outputs, tg)
    sum(ld.values()).backward()
    losses = np.array([float(ld[k].detach()) for k in ("loss_ce", "loss_bbox", "loss_giou")], np.float64)
    return indices, losses, logits.grad.numpy(), boxes.grad.numpy()


def g10_criterion():
    # case 1 is G6's matcher_inputs() as is
    for a, b in zip(matcher_inputs(), cc.inputs("c1_matcher")):
        assert np.array_equal(a, b)
    out = {}
    for name, (B, Q, C, counts, seed, alpha, gamma) in cc.CASES.items():
        idx, l32, gl32, gb32 = _run(name, torch.float32)
        _, l64, gl64, gb64 = _run(name, torch.float64, indices=idx)
        for b, (i, j) in enumerate(idx):
            out[f"{name}.src{b}"] = i.numpy().astype(np.int16)
            out[f"{name}.tgt{b}"] = j.numpy().astype(np.int16)
        out[f"{name}.losses32"] = l32
        out[f"{name}.losses64"] = l64
        out[f"{name}.dlogits32"] = gl32.astype(np.float32)
        out[f"{name}.dboxes32"] = gb32.astype(np.float32)
        out[f"{name}.dlogits64"] = gl64
        out[f"{name}.dboxes64"] = gb64
        if seed is None:
            det, labels, gt, offs = cc.inputs(name)
            out[f"{name}.det"], out[f"{name}.labels"], out[f"{name}.gt"] = det, labels, gt
        else:
            out[f"{name}.seed"] = np.array(seed)
        print(name, "losses f64", l64, "matched", sum(len(i) for i, _ in idx))
    # case 4 exercises the ties it was built for
    i0, j0 = (t.tolist() for t in cc.indices_from(out, "c4_ties")[0])
    assert sorted(zip(i0, j0)) == [(0, 0), (1, 1)], (i0, j0)
    _save("g10_criterion", **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    g10_criterion()
