#!/usr/bin/env python3
"""Generate golden G11 (tests/golden/g11_aux_*.npz): deep supervision evaluated by THE REFERENCE's own modules.

The reference's decoder returns every layer's state (`DeformableTransformerDecoder.forward` -> (output, intermediate),
deformable_attention.py:286-309) but its detector uses only the last.  Here its `class_embed` / `bbox_embed(...).sigmoid()`
are applied to each `intermediate[j]`, its HungarianMatcher + SetCriterion (config.py's weights {ce: 1, bbox: 5, giou: 2}) to
each layer's outputs, the per-layer sums of `loss_dict.values()` (train.py:1090) are added up and `backward()` runs once.
Recorded per layer: logits, boxes, the three weighted losses, the assignment; and of the whole step: the total loss and, as
G9 keeps them (grad_probe: a strided probe + three checksums per tensor), the gradient of every trainable parameter and of
the decoder's memory.  dropout = 0 (no RNG to reproduce).
  g11_aux_micro      the micro decoder of tests/aux_cases.py (L = 3, N = 26), fp32
  g11_aux_micro_f64  the same in float64, with the fp32 run's assignments
  g11_aux_cfg1       the whole detector: cfg1 of cases.G9_CASES (num_decoder_layers = 2), so the LoRA and projection
                     gradients under deep supervision are pinned too

  python tests/golden/make_goldens_aux.py

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

import make_goldens as mg  # noqa: E402  (imports the reference)
from make_goldens import _load, _save, grad_probe  # noqa: E402
from dinov2_od_amd import synth  # noqa: E402
from dinov2_od_amd.config import BackboneConfig, DecoderConfig  # noqa: E402
from tests import aux_cases as ac  # noqa: E402
from tests import cases  # noqa: E402
from tests import criterion_cases as cc  # noqa: E402

KEYS = ("loss_ce", "loss_bbox", "loss_giou")


def _supervise(dec, memory, tg, dtype, indices=None):
    """reference DETRDecoder `dec` on `memory` -> (total loss, per-layer outputs, per-layer losses, per-layer indices)"""
    import dino_detector.losses as rl
    import dino_detector.matching as rm
    C = dec.class_embed.out_features
    tgt = dec.query_embed.weight.unsqueeze(0).repeat(memory.size(0), 1, 1)
    _, intermediate = dec.decoder(tgt, memory)
    total, outs, losses, idx = 0, [], [], []
    for j, hs in enumerate(intermediate):
        o = {"pred_logits": dec.class_embed(hs), "pred_boxes": dec.bbox_embed(hs).sigmoid()}
        ind = indices[j] if indices is not None else rm.HungarianMatcher(cost_class=1, cost_bbox=5, cost_giou=2)(o, tg)
        ld = rl.SetCriterion(cc.FixedMatcher(ind), C, dict(cc.WEIGHTS))(o, tg)
        total = total + sum(ld.values())
        outs.append(o)
        losses.append(np.array([float(ld[k].detach()) for k in KEYS], np.float64))
        idx.append(ind)
    return total, outs, losses, idx


def _record(tag, out, outs, losses, idx, total):
    for j, (o, l, ind) in enumerate(zip(outs, losses, idx)):
        out[f"{tag}.l{j}.logits"] = o["pred_logits"].detach().numpy()
        out[f"{tag}.l{j}.boxes"] = o["pred_boxes"].detach().numpy()
        out[f"{tag}.l{j}.losses"] = l
        for b, (i, k) in enumerate(ind):
            out[f"{tag}.l{j}.src{b}"] = np.asarray(i).astype(np.int16)
            out[f"{tag}.l{j}.tgt{b}"] = np.asarray(k).astype(np.int16)
    out[f"{tag}.loss"] = np.array(float(total.detach()))


def _grads(module, out):
    names, nograd = [], []
    for k, p in module.named_parameters():
        if not p.requires_grad:
            continue
        if p.grad is None:
            nograd.append(k)
            continue
        out["grad:" + k], out["stat:" + k] = grad_probe(p.grad.numpy())
        names.append(k)
    out["trainable_with_grad"] = np.array(names)
    out["trainable_without_grad"] = np.array(nograd)


def micro():
    Dd, Hd, Q, L, F, C, P, B, N = ac.MICRO
    dc = ac.micro_cfg()
    indices = None
    for name, dtype in (("g11_aux_micro", torch.float32), ("g11_aux_micro_f64", torch.float64)):
        m = mg.DETRDecoder(num_queries=Q, hidden_dim=Dd, nheads=Hd, num_decoder_layers=L, num_classes=C, dim_feedforward=F, dropout=0.0,
                           n_points=P, use_deformable=True)
        _load(m, synth.decoder_state_dict(dc, seed=1, prefix=""))
        m = m.to(dtype).train()
        mem = torch.from_numpy(cases.g1_memory(N, Dd)).to(dtype).requires_grad_(True)
        tg = ac.targets(C, dtype=dtype)
        total, outs, losses, idx = _supervise(m, mem, tg, dtype, indices)
        indices = indices or idx
        total.backward()
        out = {}
        _record("micro", out, outs, losses, idx, total)
        _grads(m, out)
        out["dmem_probe"], out["dmem_stat"] = grad_probe(mem.grad.numpy())
        _save(name, **out)
        print(name, "loss", float(total), "per layer", [l.tolist() for l in losses])


def detector():
    model_name, R, B, kw = cases.G9_CASES[ac.DETECTOR]
    hid = kw["hidden_dim"]
    bb = BackboneConfig.from_name(model_name, lora_r=kw["lora_r"], lora_alpha=1.0, target_dim=hid)
    mg._BB_FOR_PATCH["bb"] = bb
    m = mg.DINOv2ObjectDetector(dino_model_name=model_name, **kw)
    dc = DecoderConfig(num_queries=kw["num_queries"], hidden_dim=hid, nheads=kw["nheads"], num_layers=kw["num_decoder_layers"],
                       num_classes=kw["num_classes"], dim_feedforward=kw["dim_feedforward"], n_points=2, use_deformable=True)
    _load(m, synth.detector_state_dict(bb, dc, seed=1))
    m.train()
    x = torch.from_numpy(synth.make_pixels(B, R, R, seed=0))
    feats = m.backbone(x)
    feats.retain_grad()
    total, outs, losses, idx = _supervise(m.decoder, feats, ac.targets(kw["num_classes"]), torch.float32)
    total.backward()
    out = {}
    _record("cfg1", out, outs, losses, idx, total)
    _grads(m, out)
    out["dmem_probe"], out["dmem_stat"] = grad_probe(feats.grad.numpy())
    _save("g11_aux_cfg1", **out)
    print("g11_aux_cfg1 loss", float(total), "per layer", [l.tolist() for l in losses])


if __name__ == "__main__":
    torch.manual_seed(0)
    micro()
    detector()
