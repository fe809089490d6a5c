"""Inputs of golden G10 (the set criterion, tests/golden/g10_criterion.npz): regenerated from dinov2_od_amd.synth seeds, so
the golden file stores only the seeds of cases 1-3 and 5 (case 4, the exact-tie case, is written out by hand here too)."""
import numpy as np

from dinov2_od_amd import synth

WEIGHTS = {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}      # the reference's config.py loss_weights


def synth_inputs(B, Q, C, counts, seed):
    """packed detections [B,Q,C+4], labels int64 [G], cxcywh boxes fp32 [G,4], offsets int32 [B+1]; the generator of
    tests/golden/make_goldens.py matcher_inputs (G6), restated so the tests need no reference"""
    logits = synth.normal(seed, "mt.logits", (B, Q, C), 2.0).astype(np.float32)
    cxcy = 0.15 + 0.7 * synth.uniform01(seed, "mt.cxcy", (B, Q, 2))
    wh = 0.05 + 0.4 * synth.uniform01(seed, "mt.wh", (B, Q, 2))
    det = np.concatenate([logits, cxcy, wh], axis=-1).astype(np.float32)
    G = int(sum(counts))
    labels = (synth.uniform01(seed, "mt.labels", (G,)) * C).astype(np.int64).clip(0, C - 1)
    gcxcy = 0.15 + 0.7 * synth.uniform01(seed, "mt.gcxcy", (G, 2))
    gwh = 0.05 + 0.4 * synth.uniform01(seed, "mt.gwh", (G, 2))
    gt = np.concatenate([gcxcy, gwh], axis=-1).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return det, labels, gt, offs


def tie_inputs():
    """case 4: query 0 predicts target 0's box exactly (every max / min of the GIoU ties, every L1 difference is 0); query 1's
    box touches target 1's edge to edge (intersection width exactly 0: the clamp's boundary) and shares its y extent.
    Dyadic coordinates, so the ties hold in fp32 and float64 alike.  The other queries sit far away with low scores."""
    B, Q, C = 1, 6, 5
    det, _, _, _ = synth_inputs(B, Q, C, (0,), seed=41)
    det[..., :C] -= 4.0
    det[0, 0, 1] = 6.0
    det[0, 1, 3] = 6.0
    gt = np.array([[0.25, 0.25, 0.125, 0.25], [0.625, 0.5, 0.25, 0.25]], np.float32)
    labels = np.array([1, 3], np.int64)
    det[0, 0, C:] = gt[0]
    det[0, 1, C:] = [0.875, 0.5, 0.25, 0.25]                 # x: [0.75, 1.0] against [0.5, 0.75]
    det[0, 2:, C:] = [0.125, 0.875, 0.0625, 0.0625]
    det[0, 2:, C] += 0.03125 * np.arange(Q - 2)
    offs = np.array([0, 2], np.int32)
    return det, labels, gt, offs


# name -> (B, Q, C, counts, seed, focal_alpha, focal_gamma); seed None = tie_inputs()
CASES = {
    "c1_matcher": (4, 25, 11, (4, 0, 7, 30), 13, 0.25, 2.0),
    "c2_coco": (2, 100, 91, (7, 23), 29, 0.25, 2.0),
    "c3_alpha_gamma": (3, 25, 11, (5, 2, 9), 23, 0.4, 1.5),
    "c4_ties": (1, 6, 5, (2,), None, 0.25, 2.0),
    "c5_empty": (2, 10, 5, (0, 0), 31, 0.25, 2.0),
}


def inputs(name):
    B, Q, C, counts, seed, _, _ = CASES[name]
    if seed is None:
        return tie_inputs()
    return synth_inputs(B, Q, C, counts, seed)


def targets(labels, gt, offs, to=lambda a: a):
    import torch
    return [{"labels": to(torch.from_numpy(labels[offs[b]:offs[b + 1]].copy())),
             "boxes": to(torch.from_numpy(gt[offs[b]:offs[b + 1]].copy()))} for b in range(len(offs) - 1)]


def indices_from(g, name):
    """the matcher's recorded (pred_idx, tgt_idx) pairs of a G10 case, as int64 CPU tensors per image"""
    import torch
    B = CASES[name][0]
    out = []
    for b in range(B):
        out.append((torch.from_numpy(g[f"{name}.src{b}"].astype(np.int64)), torch.from_numpy(g[f"{name}.tgt{b}"].astype(np.int64))))
    return out


class FixedMatcher:
    """a matcher that hands back recorded indices (the assignment is G6's subject; G10 pins what the criterion does with it)"""

    def __init__(self, indices):
        self.indices = indices

    def __call__(self, outputs, targets):
        return self.indices
