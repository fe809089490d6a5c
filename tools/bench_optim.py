#!/usr/bin/env python3
"""Optimizer step timing on the trainable set of the reference's default model (ViT-B/14, LoRA r = 2, one deformable decoder
layer: 57 tensors, 55 of them with a gradient, 5.6 M fp32 elements; synth weights, random gradients):
    torch       clip_grad_norm_(params, 1.0) + torch.optim.Adam(lr 1e-4, weight_decay 1e-4).step()    what the reference runs
    torch_fused the same with Adam(fused=True)
    native      dinov2_od_amd.optim.Adam(max_grad_norm=1.0).step()                                    two launches (csrc/optim.hip)
and the same with decoupled weight decay and an exponential moving average (decay 0.9999) of the trainable set:
    torch_adamw / torch_adamw_fused          clip_grad_norm_ + torch.optim.AdamW(fused=...).step()
    torch_adamw_ema / torch_adamw_fused_ema  ... followed by torch._foreach_lerp_(shadows, params, 1e-4)
    native_adamw                             optim.AdamW(max_grad_norm=1.0).step()
    native_adamw_ema_fused                   optim.AdamW(max_grad_norm=1.0, ema=ModelEMA(...)).step(): the update launch writes the shadows
    native_adamw_ema_standalone              optim.AdamW(max_grad_norm=1.0).step() + ModelEMA.update(): one more launch
One hipEvent pair per step on the compute stream; the legs alternate step by step, each on its own copy of the parameters;
the gradients are restored from a master copy before every step, outside the events (PyTorch's clip scales them in place).
Median and p10 / p90 over --steps steps after --warmup; for the native legs also the bytes the arithmetic needs (one read of g for
the norm; one read of g, p, m, v and one write of p, m, v for the update; one read and write of e for the average, and a read of p
more where the average is a launch of its own) over the median.  One JSON line on stdout.
    python tools/bench_optim.py [--steps 100] [--warmup 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dinov2_od_amd import DINOv2ObjectDetector, _native, optim, synth  # noqa: E402


def trainable_set(device):
    """[(name, tensor)] of the default model's trainable parameters, synth weights"""
    with torch.device("meta"):
        m = DINOv2ObjectDetector(pretrained=False, precision="bf16")
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    sd = synth.detector_state_dict(m._bb_cfg, m._dc_cfg, seed=1)
    return [(n, torch.from_numpy(np.ascontiguousarray(sd[n])).to(device)) for n in names]


def _stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4), "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert a.steps >= 50 and a.warmup >= 10
    assert torch.cuda.is_available(), "bench_optim needs the GPU"
    dev = torch.device("cuda:0")
    named = trainable_set(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    # the unused decoder.reference_points pair never receives a gradient (its .grad stays None)
    master = [None if n.startswith("decoder.reference_points.") else torch.randn(t.shape, device=dev, generator=gen) * 0.05 for n, t in named]
    hyp = dict(lr=1e-4, weight_decay=1e-4)

    def leg(make, clip):
        """make(params, holder) -> optimizer, or (optimizer, what follows its step inside the timed window)"""
        holder = torch.nn.Module()
        holder.list = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for _, t in named])
        params = list(holder.list)
        for p, g in zip(params, master):
            p.grad = None if g is None else g.clone()
        made = make(params, holder)
        opt, after = made if isinstance(made, tuple) else (made, None)

        def restore():
            for p, g in zip(params, master):
                if g is not None:
                    p.grad.copy_(g)

        def step():
            if clip:
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
            if after is not None:
                after()
        return restore, step, params

    def with_lerp(cls, **kw):
        def make(ps, holder):
            shadows = [p.detach().clone() for p in ps]
            return cls(ps, **kw, **hyp), lambda: torch._foreach_lerp_(shadows, [p.detach() for p in ps], 1e-4)
        return make

    def native_then_update(ps, holder):
        ema = optim.ModelEMA(holder, decay=0.9999)
        return optim.AdamW(ps, max_grad_norm=1.0, **hyp), ema.update

    legs = {"torch": leg(lambda ps, h: torch.optim.Adam(ps, **hyp), True),
            "torch_fused": leg(lambda ps, h: torch.optim.Adam(ps, fused=True, **hyp), True),
            "native": leg(lambda ps, h: optim.Adam(ps, max_grad_norm=1.0, **hyp), False),
            "torch_adamw": leg(lambda ps, h: torch.optim.AdamW(ps, **hyp), True),
            "torch_adamw_fused": leg(lambda ps, h: torch.optim.AdamW(ps, fused=True, **hyp), True),
            "torch_adamw_ema": leg(with_lerp(torch.optim.AdamW), True),
            "torch_adamw_fused_ema": leg(with_lerp(torch.optim.AdamW, fused=True), True),
            "native_adamw": leg(lambda ps, h: optim.AdamW(ps, max_grad_norm=1.0, **hyp), False),
            "native_adamw_ema_fused": leg(lambda ps, h: optim.AdamW(ps, max_grad_norm=1.0, ema=optim.ModelEMA(h, decay=0.9999), **hyp), False),
            "native_adamw_ema_standalone": leg(native_then_update, False)}
    before = _native.lib().dod_test_counter(b"optim_launches")
    ms = {k: [] for k in legs}
    for it in range(a.warmup + a.steps):
        for name, (restore, step, _) in legs.items():
            restore()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            step()
            e.record()
            e.synchronize()
            if it >= a.warmup:
                ms[name].append(s.elapsed_time(e))
    launches = (_native.lib().dod_test_counter(b"optim_launches") - before) / (a.warmup + a.steps)
    n_grad = sum(g.numel() for g in master if g is not None)
    n_all = sum(t.numel() for _, t in named)
    nbytes = 4 * n_grad * (1 + 4 + 3)
    native_bytes = {"native": nbytes, "native_adamw": nbytes, "native_adamw_ema_fused": nbytes + 4 * 2 * n_all,
                    "native_adamw_ema_standalone": nbytes + 4 * 3 * n_all}
    out = {"tool": "bench_optim", "device": torch.cuda.get_device_name(0), "torch_version": torch.__version__, "tensors": len(named),
           "tensors_with_grad": sum(g is not None for g in master), "elements_with_grad": n_grad,
           "native_launches_per_step_all_native_legs": launches, "native_bytes_per_step": nbytes}
    for k in legs:
        out[k] = _stats(ms[k])
    for k, nb in native_bytes.items():
        out[k]["bytes_per_step"] = nb
        out[k]["achieved_GBps"] = round(nb / (out[k]["median_ms"] * 1e-3) / 1e9, 1)
    # the legs of one family saw the same gradients from the same start: their parameters agree to fp32 rounding of the same formula
    ref = legs["torch"][2]
    for k in ("torch_fused", "native"):
        out[k]["max_abs_diff_vs_torch"] = float(max((p.detach() - q.detach()).abs().max() for p, q in zip(legs[k][2], ref)))
    ref = legs["torch_adamw"][2]
    for k in legs:
        if "adamw" in k and k != "torch_adamw":
            out[k]["max_abs_diff_vs_torch_adamw"] = float(max((p.detach() - q.detach()).abs().max() for p, q in zip(legs[k][2], ref)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
