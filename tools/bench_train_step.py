#!/usr/bin/env python3
"""train()-mode step (forward + backward) on the drop-in detector, ViT-B/14 224x224, batch 16: the native step (HIP forward with a
tape + HIP backward; the default) or, with DINODET_NATIVE_TRAIN=0, the native frozen prefix + the PyTorch autograd composite --
against the all-composite evaluation (selected by an input that requires grad).
    python tools/bench_train_step.py [resolution] [batch]
--aux: deep supervision (aux_loss=True, the loss reads every decoder layer's outputs) instead: the native step without aux, the
native step with aux and the composite with aux (DINODET_NATIVE_TRAIN=0), alternated round by round, device events around each step,
median and p10 / p90 over 30 steps per leg after a warm-up of each.
    python tools/bench_train_step.py --aux [resolution] [batch]
--train-precision fp32|bf16x3: what the native step's linears run on (DINOv2ObjectDetector.set_train_precision; default fp32).
    python tools/bench_train_step.py --train-precision bf16x3 [resolution] [batch]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import build
m, bb, dc = build("facebook/dinov2-base", 100, os.environ.get("DINODET_PRECISION", "bf16"), torch.device("cuda"))
m.train()
AUX = "--aux" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--aux"]
TP = "fp32"
if "--train-precision" in argv:
    i = argv.index("--train-precision")
    TP = argv[i + 1]
    del argv[i:i + 2]
m.set_train_precision(TP)
R = int(argv[0]) if len(argv) > 0 else 224
B = int(argv[1]) if len(argv) > 1 else 16
x = torch.rand(B, 3, R, R, device="cuda")
def aux_legs(rounds=6, per=5, warmup=3):
    import numpy as np
    def step(aux, native):
        os.environ["DINODET_NATIVE_TRAIN"] = "1" if native else "0"
        m.decoder.aux_loss = aux
        m.zero_grad(set_to_none=True)
        o = m(x)
        sum(l["pred_logits"].square().mean() + l["pred_boxes"].mean() for l in [o] + list(o.get("aux_outputs", ()))).backward()
    legs = {"native step, no aux": (False, True), "native step, aux": (True, True), "composite, aux": (True, False)}
    ms = {k: [] for k in legs}
    for a in legs.values():
        for _ in range(warmup): step(*a)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, a in legs.items():
            for _ in range(per):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); step(*a); e.record(); e.synchronize()
                ms[k].append(s.elapsed_time(e))
    for k, v in ms.items():
        print(f"{k:24s}: median {np.median(v):7.2f} ms  p10 {np.percentile(v, 10):7.2f}  p90 {np.percentile(v, 90):7.2f} per forward+backward "
              f"({len(v)} steps, batch {B}, {R}x{R}, Q {dc.num_queries}, L {dc.num_layers})")
if AUX:
    aux_legs()
    sys.exit(0)
def step(inp):
    m.zero_grad(set_to_none=True)
    o = m(inp)
    (o["pred_logits"].square().mean() + o["pred_boxes"].mean()).backward()
first = "native prefix + composite" if os.environ.get("DINODET_NATIVE_TRAIN", "1") == "0" else f"native step ({TP})"
for name, mk in ((first, lambda: x), ("all-composite", lambda: x.clone().requires_grad_(True))):
    for _ in range(2): step(mk())
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(5): step(mk())
    torch.cuda.synchronize()
    print(f"{name:24s}: {(time.perf_counter() - t) / 5 * 1e3:7.1f} ms per forward+backward (batch {B}, {R}x{R})")
