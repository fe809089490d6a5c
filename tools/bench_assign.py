#!/usr/bin/env python3
"""Hungarian assignment timing: the device solver (matching.assign / HungarianMatcher.match_table / SetCriterion with
device_assignment=True) against the host path it can replace (costs read back, scipy per image, the match table built on the
host and uploaded from pinned memory).  Three legs, each interleaved host, device, host, device ... in one process:
  (a) the assignment alone on a device-resident cost buffer (the matcher's real costs), at B=16/Q=100 with 1-20 targets per
      image, B=64/Q=300 with 1-20 and B=64/Q=300 with 50-100
  (b) SetCriterion forward + backward, host mode against device mode, at B=16/Q=100/C=91 and B=64/Q=300/C=91 (1-20 targets)
  (c) the ViT-B/14 224x224 batch-16 train step of tools/bench_criterion.py in both modes, plus the host-side return time of the
      criterion call (no synchronise)
hipEvent pairs around every step, warm-up first, median and p10 / p90 over --steps steps.  One JSON line on stdout.
    python tools/bench_assign.py [--steps 30] [--warmup 5] [--legs abc] [--host-only]
--host-only runs only the host legs: the code path an earlier commit also has (run from that commit's tree for an A/B check)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

from dinov2_od_amd import losses as L  # noqa: E402
from dinov2_od_amd import matching  # noqa: E402
from tests import criterion_cases as cc  # noqa: E402

W = dict(cc.WEIGHTS)


def _stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4), "steps": len(ms)}


def _interleaved(fns, steps, warmup):
    """fns: name -> callable; each step times every callable once, in order, with its own event pair"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return {k: _stats(v) for k, v in ms.items()}


def _inputs(B, Q, C, lo, hi, seed):
    rng = np.random.default_rng(seed)
    counts = [int(rng.integers(lo, hi + 1)) for _ in range(B)]
    det, labels, gt, offs = cc.synth_inputs(B, Q, C, counts, seed=seed)
    return counts, det, labels, gt, offs


def assign_leg(B, Q, lo, hi, steps, warmup, host_only):
    C = 91
    counts, det, labels, gt, offs = _inputs(B, Q, C, lo, hi, seed=B * Q + hi)
    dev = torch.device("cuda")
    offs_d = torch.from_numpy(offs).to(dev)
    cost = matching.match_cost(torch.from_numpy(det).to(dev), C, torch.from_numpy(labels).to(dev), torch.from_numpy(gt).to(dev),
                               offs_d)

    def host():
        c = cost.cpu().numpy()
        idx = [linear_sum_assignment(c[offs[b] * Q:offs[b + 1] * Q].reshape(Q, n)) for b, n in enumerate(counts)]
        return L.match_table(idx, counts, Q, pin=True).to(dev, non_blocking=True)

    fns = {"host": host}
    if not host_only:
        fns["device"] = lambda: matching.assign(cost, offs_d, Q)[0]
        assert torch.equal(host(), fns["device"]())                  # the same table before anything is timed
    return _interleaved(fns, steps, warmup)


def criterion_leg(B, Q, C, steps, warmup, host_only):
    counts, det, labels, gt, offs = _inputs(B, Q, C, 1, 20, seed=B * Q)
    d = torch.from_numpy(det).cuda().requires_grad_(True)
    out = {"pred_logits": d[..., :C], "pred_boxes": d[..., C:]}
    tg = cc.targets(labels, gt, offs, to=lambda t: t.cuda())
    fns = {}
    for name, device in (("host", False), ("device", True)):
        if device and host_only:
            continue
        crit = L.SetCriterion(matching.HungarianMatcher(), C, W, **({"device_assignment": True} if device else {}))

        def f(crit=crit):
            d.grad = None
            sum(crit(out, tg).values()).backward()
        fns[name] = f
    return _interleaved(fns, steps, warmup)


def train_step_leg(steps, warmup, host_only):
    from bench import build
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
    fns, ret = {}, {}
    for name, device in (("host", False), ("device", True)):
        if device and host_only:
            continue
        crit = L.SetCriterion(matching.HungarianMatcher(), dc.num_classes, W, **({"device_assignment": True} if device else {}))
        ret[name] = []

        def f(crit=crit, name=name):
            m.zero_grad(set_to_none=True)
            o = m(x)
            t0 = time.perf_counter()
            ld = crit(o, tg)
            ret[name].append(1e3 * (time.perf_counter() - t0))
            sum(ld.values()).backward()
        fns[name] = f
    res = _interleaved(fns, steps, warmup)
    for name in fns:
        res[name]["criterion_call_return"] = _stats(ret[name][warmup:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    assert a.steps >= 30
    out = {"tool": "bench_assign", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "host_only": a.host_only}
    if "a" in a.legs:
        for B, Q, lo, hi in ((16, 100, 1, 20), (64, 300, 1, 20), (64, 300, 50, 100)):
            out[f"assign_B{B}_Q{Q}_n{lo}-{hi}"] = assign_leg(B, Q, lo, hi, a.steps, a.warmup, a.host_only)
    if "b" in a.legs:
        for B, Q, C in ((16, 100, 91), (64, 300, 91)):
            out[f"criterion_fwd_bwd_B{B}_Q{Q}_C{C}"] = criterion_leg(B, Q, C, a.steps, a.warmup, a.host_only)
    if "c" in a.legs:
        out["train_step_vitb_224_b16"] = train_step_leg(a.steps, a.warmup, a.host_only)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
