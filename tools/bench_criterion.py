#!/usr/bin/env python3
"""Set criterion timing: the native criterion (dinov2_od_amd.losses.SetCriterion: host match table + one async copy, two forward
launches, one backward launch) against the torch composite of the same math on the GPU, driven the way the reference's
losses.py drives it (num_boxes read back with .item(), then the per-term kernels), at B=16/Q=100/C=91 and B=64/Q=300/C=91;
then one ViT-B/14 224x224 batch-16 train step (train()-mode forward, our matcher, criterion, backward) with each criterion.
hipEvent pairs around every step, warm-up first, median and p10 / p90 over --steps steps.  One JSON line on stdout.
    python tools/bench_criterion.py [--steps 30] [--warmup 5]
--aux: instead, the layered criterion (deep supervision: L = 3 layers of a packed [L, B, Q, C+4] buffer through ONE
dod_set_criterion_layers_* call) against L single-layer calls on the same slices, forward + backward, device-resident inputs."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dinov2_od_amd import losses as L  # noqa: E402
from tests import criterion_cases as cc  # noqa: E402

W = dict(cc.WEIGHTS)


class _Fixed:
    def __init__(self, idx):
        self.idx = idx

    def __call__(self, outputs, targets):
        return self.idx


def composite_criterion(matcher, C):
    """the reference criterion's flow on the composite math: host num_boxes -> device -> .item() (losses.py:222-226)"""
    def run(outputs, targets):
        idx = matcher(outputs, targets)
        logits, boxes = outputs["pred_logits"], outputs["pred_boxes"]
        dev = logits.device
        counts = [len(t["labels"]) for t in targets]
        nb = torch.clamp(torch.as_tensor([float(sum(counts))], device=dev), min=1).item()
        lab = torch.cat([t["labels"] for t in targets])
        gt = torch.cat([t["boxes"] for t in targets])
        match = L.match_table(idx, counts, logits.shape[1]).to(dev)
        lc = L.composite_losses(logits, boxes, lab, gt, match, torch.tensor([nb], device=dev))
        return {k: W[k] * lc[n] for n, k in enumerate(L.LOSS_KEYS)}
    return run


def _stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4), "steps": len(ms)}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return _stats(ms)


def criterion_legs(B, Q, C, steps, warmup):
    rng = np.random.default_rng(B * Q)
    counts = [int(rng.integers(1, 21)) for _ in range(B)]           # COCO-like: up to 20 objects per image
    det, labels, gt, offs = cc.synth_inputs(B, Q, C, counts, seed=7)
    idx = [(torch.from_numpy(np.sort(rng.permutation(Q)[:n]).astype(np.int64)), torch.from_numpy(rng.permutation(n).astype(np.int64)))
           for n in counts]
    d = torch.from_numpy(det).cuda().requires_grad_(True)
    out = {"pred_logits": d[..., :C], "pred_boxes": d[..., C:]}
    tg = cc.targets(labels, gt, offs, to=lambda t: t.cuda())
    native = L.SetCriterion(_Fixed(idx), C, W)
    comp = composite_criterion(_Fixed(idx), C)

    def step(crit):
        def f():
            d.grad = None
            sum(crit(out, tg).values()).backward()
        return f
    dev = d.device
    args = (torch.from_numpy(labels).to(dev), torch.from_numpy(gt).to(dev), L.match_table(idx, counts, Q).to(dev),
            torch.tensor([float(sum(counts))], device=dev))

    def kernels():                                   # the three launches alone (plus the .sum()), device-resident inputs
        d.grad = None
        L.native_losses(out["pred_logits"], out["pred_boxes"], *args).sum().backward()
    return {"native": _time(step(native), steps, warmup), "native_kernels_only": _time(kernels, steps, warmup),
            "composite": _time(step(comp), steps, warmup)}


def layered_legs(B, Q, C, nl, steps, warmup):
    rng = np.random.default_rng(B * Q + nl)
    counts = [int(rng.integers(1, 21)) for _ in range(B)]
    det = np.stack([cc.synth_inputs(B, Q, C, counts, seed=7 + l)[0] for l in range(nl)])
    _, labels, gt, offs = cc.synth_inputs(B, Q, C, counts, seed=7)
    tabs = [L.match_table([(torch.from_numpy(np.sort(rng.permutation(Q)[:n]).astype(np.int64)), torch.from_numpy(rng.permutation(n).astype(np.int64)))
                           for n in counts], counts, Q).cuda() for _ in range(nl)]
    d = torch.from_numpy(det).cuda().requires_grad_(True)
    lab, g, nb = torch.from_numpy(labels).cuda(), torch.from_numpy(gt).cuda(), torch.tensor([float(sum(counts))], device="cuda")
    match = torch.cat(tabs)

    def layered():
        d.grad = None
        L.native_losses_layers([d[l, ..., :C] for l in range(nl)], [d[l, ..., C:] for l in range(nl)], lab, g, match, nb).sum().backward()

    def singles():
        d.grad = None
        sum(L.native_losses(d[l, ..., :C], d[l, ..., C:], lab, g, tabs[l], nb).sum() for l in range(nl)).backward()
    return {"layered_call": _time(layered, steps, warmup), f"{nl}_single_layer_calls": _time(singles, steps, warmup)}


def train_step_legs(steps, warmup):
    from bench import build
    from dinov2_od_amd.matching import HungarianMatcher
    m, bb, dc = build("facebook/dinov2-base", 100, "bf16", torch.device("cuda"))
    m.train()
    B = 16
    x = torch.rand(B, 3, 224, 224, device="cuda")
    rng = np.random.default_rng(0)
    tg = []
    for _ in range(B):
        n = int(rng.integers(1, 21))
        tg.append({"labels": torch.from_numpy(rng.integers(1, dc.num_classes, n)).cuda(),
                   "boxes": torch.from_numpy(np.concatenate([0.2 + 0.6 * rng.random((n, 2)), 0.05 + 0.3 * rng.random((n, 2))], 1)
                                             .astype(np.float32)).cuda()})
    matcher = HungarianMatcher()
    crits = {"native": L.SetCriterion(matcher, dc.num_classes, W), "composite": composite_criterion(matcher, dc.num_classes)}
    res = {}
    for name, crit in crits.items():
        def f(crit=crit):
            m.zero_grad(set_to_none=True)
            sum(crit(m(x), tg).values()).backward()
        res[name] = _time(f, steps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--aux", action="store_true")
    a = ap.parse_args()
    assert a.steps >= 20
    out = {"tool": "bench_criterion", "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if a.aux:
        for B, Q, C in ((16, 100, 91), (64, 300, 91)):
            out[f"criterion_layers_fwd_bwd_L3_B{B}_Q{Q}_C{C}"] = layered_legs(B, Q, C, 3, a.steps, a.warmup)
        print(json.dumps(out))
        return
    for B, Q, C in ((16, 100, 91), (64, 300, 91)):
        out[f"criterion_fwd_bwd_B{B}_Q{Q}_C{C}"] = criterion_legs(B, Q, C, a.steps, a.warmup)
    out["train_step_vitb_224_b16"] = train_step_legs(a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
