"""The optimizer step of csrc/optim.hip restated in float64 (torch, host): gradient-norm clip, Adam with L2 or decoupled (AdamW) weight
decay, the exponential moving average of the weights and the skip of a step whose norm is not finite.  tests/test_optim_ext_cpu.py pins
the restatement against torch.optim.Adam / AdamW / lerp run in float64; tests/test_gpu_optim_ext.py measures the kernels against it.

A snapshot is what tests/test_gpu_optim.py's Rig.snapshot returns: per parameter dict(p, g or None, m or None, v or None, t), plus an
optional e (the average, None = none).  groups = [(indices, dict(lr, betas, eps, weight_decay))]."""
import math

import torch

F64 = torch.float64


def norm64(snap):
    """the total 2-norm of the gradients (0.0 for none)"""
    total = torch.zeros((), dtype=F64)
    for e in snap:
        if e["g"] is not None:
            g = e["g"].to(F64)
            total = total + (g * g).sum()
    return float(torch.sqrt(total))


def clip_coef64(norm, max_norm):
    """clip_grad_norm_'s coefficient; a NaN norm keeps a NaN coefficient (torch.clamp)"""
    if max_norm is None:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if not c >= 1.0 else 1.0


def ema64(e, p, w):
    """e + (p - e) w in float64"""
    e = e.to(F64)
    return e + (p.to(F64) - e) * w


def ema_weight(decay, tau, updates):
    """w = 1 - d, d = decay (1 - exp(-updates / tau)); tau == 0: d = decay"""
    return 1.0 - (decay * (1.0 - math.exp(-updates / tau)) if tau > 0 else decay)


def step64(snap, groups, max_norm=None, decoupled=False, ema_w=None, skip_nonfinite=False):
    """one step from `snap` -> (out, norm, skipped): out per parameter dict(p, m, v, g, t, e, den, delta, step_size) in float64, g the clipped
    (not decayed) gradient.  A parameter without a gradient keeps p, m, v, t; its average still moves (the standalone launch).  A skipped step
    keeps p, m, v, e of every parameter with a gradient and still advances t: the host's step counter counts calls."""
    hyp_of = {i: hyp for idx, hyp in groups for i in idx}
    norm = norm64(snap)
    coef = clip_coef64(norm, max_norm)
    skipped = bool(skip_nonfinite and not math.isfinite(norm))
    out = []
    for i, s in enumerate(snap):
        p = s["p"].to(F64)
        e = s.get("e")
        e = None if e is None else e.to(F64)
        if s["g"] is None:
            out.append(dict(p=p, m=None if s["m"] is None else s["m"].to(F64), v=None if s["v"] is None else s["v"].to(F64), g=None, t=s["t"],
                            e=e if e is None or ema_w is None else ema64(e, p, ema_w)))
            continue
        hyp = hyp_of[i]
        lr, (b1, b2), eps, wd = hyp["lr"], hyp["betas"], hyp["eps"], hyp.get("weight_decay", 0.0)
        m = torch.zeros_like(p) if s["m"] is None else s["m"].to(F64)
        v = torch.zeros_like(p) if s["v"] is None else s["v"].to(F64)
        t = s["t"] + 1
        g = coef * s["g"].to(F64)
        if skipped:
            out.append(dict(p=p, m=m, v=v, g=g, t=t, e=e))
            continue
        gd = g
        if decoupled:
            p = p * (1 - lr * wd)
        elif wd != 0:
            gd = g + wd * p
        m = m + (gd - m) * (1 - b1)
        v = b2 * v + (1 - b2) * (gd * gd)
        step_size, bc2_sqrt = lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5
        den = v.sqrt() / bc2_sqrt + eps
        delta = step_size * (m / den)
        p = p - delta
        out.append(dict(p=p, m=m, v=v, g=g, gd=gd, t=t, den=den, delta=delta, step_size=step_size,
                        e=e if e is None or ema_w is None else ema64(e, p, ema_w)))
    return out, norm, skipped
