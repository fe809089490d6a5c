"""`-m gpu`: the native training steps with train_precision="bf16x3" -- their linears as bf16 split products on the fp32 operands
(csrc/gemm_f32x3.hip; schedules in dec_train.hip / tail_train.hip) -- against the fp32 native step on the same inputs.

One rule for every step.  Per tensor (each output, d(memory), every parameter gradient)
    e_ref = rel_err(fp32 native step, fp32 autograd composite)          two fp32 evaluations of the same math
    rel_err(x3 step, fp32 native step) <= max(floor, 4 * e_ref)
`floor` is the gate the step's own test applies to two fp32 evaluations (1e-4: tests/test_gpu_train_native.py), the factor 4 is
test_gpu_train_ops.py's _hold.  Each case prints its worst ratio to the bound."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, synth
from tests import cases
from tests.cases import rel_err

pytestmark = pytest.mark.gpu

DEFORM_CASES = [  # Dd, Hd, Q, layers, F, C, P, B, N: CASES[0], [1], [3] of tests/test_gpu_train_native.py
    (128, 4, 7, 2, 256, 11, 2, 2, 26),
    (128, 4, 7, 2, 256, 11, 2, 3, 257),
    (256, 4, 25, 2, 512, 91, 2, 2, 257),
]
DENSE_CASE = (128, 4, 7, 2, 256, 11, 2, 17)      # Dd, Hd, Q, layers, F, C, B, N


def _counter(name):
    return nat.lib().dod_test_counter(name.encode())


def _decoder(dc, deform=True, aux=False, **kw):
    from dinov2_od_amd.models import DETRDecoder
    from tests import gpu_util as G
    m = DETRDecoder(dc.num_queries, dc.hidden_dim, dc.nheads, dc.num_layers, dc.num_classes, dim_feedforward=dc.dim_feedforward,
                    dropout=0.0, n_points=dc.n_points, use_deformable=deform, precision="fp32", aux_loss=aux, **kw)
    G.load_np_state(m, synth.decoder_state_dict(dc, seed=1, prefix=""))
    return m.to(G.dev()).train()


def _run(m, mem, wl, wb, native, tp="fp32"):
    """-> {name: tensor}: every supervised layer's logits and boxes, d(memory), every parameter gradient.  wl / wb: [layers, B, Q, .]"""
    os.environ["DINODET_NATIVE_TRAIN"] = "1" if native else "0"
    m.set_train_precision(tp)
    try:
        m.zero_grad(set_to_none=True)
        x = mem.clone().requires_grad_(True)
        o = m(x)
        ls = list(o.get("aux_outputs", ())) + [o]
        off = wl.shape[0] - len(ls)
        sum((l["pred_logits"] * wl[off + j]).sum() + (l["pred_boxes"] * wb[off + j]).sum() for j, l in enumerate(ls)).backward()
        out = {f"grad:{k}": p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        for j, l in enumerate(ls):
            out[f"logits.{j}"], out[f"boxes.{j}"] = l["pred_logits"].detach().clone(), l["pred_boxes"].detach().clone()
        out["d(memory)"] = x.grad.detach().clone()
        return out
    finally:
        m.set_train_precision("fp32")
        os.environ.pop("DINODET_NATIVE_TRAIN", None)


def _hold(what, x3, f32, comp, floor):
    """the module's rule over every tensor of a step; prints the worst ratio"""
    assert set(x3) == set(f32) == set(comp)
    worst, bad = (0.0, "", 0.0, 0.0), []
    for k in sorted(f32):
        ref = f32[k].cpu().numpy()
        e, e_ref = rel_err(x3[k].cpu().numpy(), ref), rel_err(ref, comp[k].cpu().numpy())
        bound = max(floor, 4 * e_ref)
        worst = max(worst, (e / bound, k, e, e_ref))
        if not e <= bound:
            bad.append((k, e, e_ref))
    print(f"x3 vs fp32 native step, {what}: worst {worst[0]:.3f} of its bound at {worst[1]} (err {worst[2]:.2e}, e_ref {worst[3]:.2e})")
    assert not bad, bad
    return worst


def _weights(B, Q, C, layers, tag):
    from tests import gpu_util as G
    wl = np.stack([synth.normal(5, f"x3.{tag}.wl.{l}", (B, Q, C), 1.0) for l in range(layers)])
    wb = np.stack([synth.normal(5, f"x3.{tag}.wb.{l}", (B, Q, 4), 1.0) for l in range(layers)])
    return G.to_gpu(wl), G.to_gpu(wb)


def _deform_setup(case, aux=False, **kw):
    from tests import gpu_util as G
    Dd, Hd, Q, layers, F, C, P, B, N = case
    m = _decoder(cases.dec_cfg(True, Dd, Hd, Q, layers, F, C, P), aux=aux, **kw)
    mem = G.to_gpu(synth.normal(3, f"memory.train.{N}.{Dd}", (B, N, Dd), 1.0))
    return m, mem, *_weights(B, Q, C, layers, "deform")


@pytest.mark.parametrize("case", DEFORM_CASES, ids=[f"Dd{c[0]}_Q{c[2]}_N{c[8]}" for c in DEFORM_CASES])
def test_x3_deformable_decoder_step(case):
    m, mem, wl, wb = _deform_setup(case)
    comp = _run(m, mem, wl, wb, native=False)
    n0 = _counter("f32x3_launches")
    f32 = _run(m, mem, wl, wb, native=True)
    assert _counter("f32x3_launches") == n0, "the fp32 step launched the split GEMM"
    x3 = _run(m, mem, wl, wb, native=True, tp="bf16x3")
    assert _counter("f32x3_launches") > n0, "the bf16x3 step never launched the split GEMM"
    _hold(f"deformable {case}", x3, f32, comp, 1e-4)
    k = "grad:decoder.layers.0.cross_attn.value_proj.weight"
    assert not torch.equal(x3[k], f32[k]), "value_proj.weight: the bf16x3 gradient is bit-equal to the fp32 one"
    assert len([k for k in x3 if k.startswith("grad:")]) >= 30


def test_x3_aux_decoder_step():
    m, mem, wl, wb = _deform_setup(DEFORM_CASES[1], aux=True)
    comp = _run(m, mem, wl, wb, native=False)
    f32 = _run(m, mem, wl, wb, native=True)
    n0 = _counter("f32x3_launches")
    x3 = _run(m, mem, wl, wb, native=True, tp="bf16x3")
    assert _counter("f32x3_launches") > n0
    assert "logits.1" in x3 and "logits.0" in x3
    _hold(f"deformable, aux {DEFORM_CASES[1]}", x3, f32, comp, 1e-4)


def test_x3_dense_decoder_step():
    from tests import gpu_util as G
    Dd, Hd, Q, layers, F, C, B, N = DENSE_CASE
    m = _decoder(cases.dec_cfg(False, Dd, Hd, Q, layers, F, C), deform=False)
    mem = G.to_gpu(synth.normal(3, f"memory.dense.{N}.{Dd}", (B, N, Dd), 1.0))
    wl, wb = _weights(B, Q, C, 1, "dense")
    comp = _run(m, mem, wl, wb, native=False)
    f32 = _run(m, mem, wl, wb, native=True)
    n0 = _counter("f32x3_launches")
    x3 = _run(m, mem, wl, wb, native=True, tp="bf16x3")
    assert _counter("f32x3_launches") > n0
    assert not torch.equal(x3["logits.0"], f32["logits.0"]), "the k | v projection of the memory rows did not change the forward"
    _hold(f"dense {DENSE_CASE}", x3, f32, comp, 1e-4)


@pytest.mark.parametrize("swiglu", [False, True], ids=["gelu", "swiglu"])
def test_x3_backbone_tail_step(swiglu):
    """the smallest GELU and SwiGLU tails of test_native_backbone_tail_backward_matches_composite_autograd (micro, 70x70, batch 3: 26
    tokens, so that test's tol is 1e-4), batched-GEMM attention adjoint"""
    from dinov2_od_amd.models import DINOv2Backbone
    from tests import gpu_util as G
    bb = cases.micro_bb(swiglu)
    bb.target_dim, bb.layers = 64, 3
    m = DINOv2Backbone("micro", lora_r=bb.lora_r, lora_alpha=bb.lora_alpha, target_dim=bb.target_dim, pretrained=False, precision="fp32", config=bb)
    G.load_np_state(m, synth.backbone_state_dict(bb, seed=1, prefix=""))
    m = m.to(G.dev()).train()
    B, R = 3, 70
    x = G.to_gpu(synth.make_pixels(B, R, R, seed=0))
    N = (R // 14) ** 2 + 1
    wgt = G.to_gpu(synth.normal(7, "tail.w.micro", (B, N, bb.target_dim), 1.0))

    def run(native, tp="fp32"):
        os.environ["DINODET_NATIVE_TRAIN"] = "1" if native else "0"
        m.set_train_precision(tp)
        try:
            nat.set_option("attn_bwd_flash", 0)
            m.zero_grad(set_to_none=True)
            mem = m(x)
            (mem * wgt).sum().backward()
            out = {f"grad:{k}": p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
            out["memory"] = mem.detach().clone()
            return out
        finally:
            nat.set_option("attn_bwd_flash", -1)
            m.set_train_precision("fp32")
            os.environ.pop("DINODET_NATIVE_TRAIN", None)
    comp = run(False)
    n0 = _counter("f32x3_launches")
    f32 = run(True)
    assert _counter("f32x3_launches") == n0
    x3 = run(True, "bf16x3")
    assert _counter("f32x3_launches") > n0
    assert sum("lora_A" in k for k in x3) == 12 and "grad:projection.weight" in x3
    assert not torch.equal(x3["memory"], f32["memory"])
    _hold(f"backbone tail micro {'swiglu' if swiglu else 'gelu'}", x3, f32, comp, 1e-4)


def test_x3_step_is_bit_reproducible_in_deterministic_mode():
    m, mem, wl, wb = _deform_setup(DEFORM_CASES[1])
    nat.set_option("deterministic", 1)
    try:
        a = _run(m, mem, wl, wb, native=True, tp="bf16x3")
        b = _run(m, mem, wl, wb, native=True, tp="bf16x3")
    finally:
        nat.set_option("deterministic", -1)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two deterministic bf16x3 steps differ"


def test_default_train_precision_is_fp32_bit_for_bit():
    """a model built without the argument and one built with train_precision="fp32": the same step, bit for bit (deterministic mode)"""
    m0, mem, wl, wb = _deform_setup(DEFORM_CASES[0])
    m1, _, _, _ = _deform_setup(DEFORM_CASES[0], train_precision="fp32")
    assert m0.train_precision == m1.train_precision == "fp32"

    def run(m):      # not through _run: nothing here may call set_train_precision
        m.zero_grad(set_to_none=True)
        x = mem.clone().requires_grad_(True)
        o = m(x)
        ((o["pred_logits"] * wl[-1]).sum() + (o["pred_boxes"] * wb[-1]).sum()).backward()
        g = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        g["d(memory)"] = x.grad.detach().clone()
        return g
    nat.set_option("deterministic", 1)
    n0 = _counter("f32x3_launches")
    try:
        a, b = run(m0), run(m1)
    finally:
        nat.set_option("deterministic", -1)
    assert _counter("f32x3_launches") == n0
    assert set(a) == set(b) and len(a) >= 31
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_tape_and_workspace_bytes_do_not_depend_on_the_training_precision():
    from dinov2_od_amd.engine import make_config
    L = nat.lib()
    Dd, Hd, Q, layers, F, C, P, B, N = DEFORM_CASES[2]
    bb = cases.micro_bb()
    bb.target_dim, bb.layers = 64, 3
    deform, dense = cases.dec_cfg(True, Dd, Hd, Q, layers, F, C, P), cases.dec_cfg(False, *DENSE_CASE[:6])
    queries = [(deform, lambda c: (L.dod_decoder_train_tape_bytes(c, B, N), L.dod_decoder_train_workspace_bytes(c, B, N))),
               (deform, lambda c: (L.dod_decoder_train_aux_tape_bytes(c, B, N), L.dod_decoder_train_aux_workspace_bytes(c, B, N))),
               (dense, lambda c: (L.dod_dense_decoder_train_tape_bytes(c, DENSE_CASE[6], DENSE_CASE[7]), L.dod_dense_decoder_train_workspace_bytes(c, DENSE_CASE[6], DENSE_CASE[7]))),
               (deform, lambda c: (L.dod_backbone_tail_tape_bytes(c, 3, 26, 2), L.dod_backbone_tail_workspace_bytes(c, 3, 26, 2)))]
    for dc, q in queries:
        f32, x3 = q(ctypes.byref(make_config(bb, dc, "fp32"))), q(ctypes.byref(make_config(bb, dc, "bf16x3")))
        assert f32 == x3 and min(f32) > 0, (f32, x3)


def test_x3_golden_gradients_match_the_reference_backward():
    """G9 (the reference's own loss.backward()) through DINOv2ObjectDetector(..., train_precision="bf16x3"), golden g9_grad_cfg1: the
    inequalities test_train_step_gradients_match_the_reference_backward applies to that golden, constants unchanged -- forward and loss
    within 1e-3, every gradient's probe and norms within 2e-4 (that golden has no float64 companion; the 1.5x / 8x float64 gate of the
    768-wide case needs one)."""
    from tests import gpu_util as G
    from dinov2_od_amd.models import DINOv2ObjectDetector
    name = "g9_grad_cfg1"
    g = cases.golden(name)
    model_name, R, B, kw = cases.G9_CASES[name]
    m = DINOv2ObjectDetector(dino_model_name=model_name, pretrained=False, precision="fp32", train_precision="bf16x3", **kw)
    assert m.backbone.train_precision == m.decoder.train_precision == "bf16x3"
    G.load_np_state(m, synth.detector_state_dict(m._bb_cfg, m._dc_cfg, seed=1))
    m = m.to(G.dev()).train()
    x = G.to_gpu(synth.make_pixels(B, R, R, seed=0))
    gl, gb = cases.g9_loss_weights(B, m._dc_cfg.num_queries, m._dc_cfg.num_classes)
    n0 = _counter("f32x3_launches")
    o = m(x)
    loss = (o["pred_logits"] * G.to_gpu(gl)).sum() + (o["pred_boxes"] * G.to_gpu(gb)).sum()
    loss.backward()
    G.sync()
    assert _counter("f32x3_launches") > n0
    el, eb = rel_err(o["pred_logits"].detach().cpu().numpy(), g["pred_logits"]), rel_err(o["pred_boxes"].detach().cpu().numpy(), g["pred_boxes"])
    assert el < 1e-3 and eb < 1e-3
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-3 * max(1.0, abs(float(g["loss"])))
    worst = cases.g9_check(m, g, 2e-4, 2e-4)
    print(f"{name} bf16x3: forward logits {el:.2e} boxes {eb:.2e}; worst gradient probe {worst[0]:.2e} ({worst[1]})")


def _loss(out, targets, indices, num_classes):
    """tests/test_gpu_train_loop.py's loss: classification (background = class 0 for unmatched queries) + L1 on matched boxes"""
    logits, boxes = out["pred_logits"], out["pred_boxes"]
    tgt_cls = torch.zeros(logits.shape[:2], dtype=torch.int64, device=logits.device)
    l1 = logits.new_zeros(())
    n = 0
    for b, (i, j) in enumerate(indices):
        if len(i) == 0:
            continue
        tgt_cls[b, i] = targets[b]["labels"][j]
        l1 = l1 + (boxes[b, i] - targets[b]["boxes"][j]).abs().sum()
        n += len(i)
    return torch.nn.functional.cross_entropy(logits.flatten(0, 1), tgt_cls.flatten()) + 5.0 * l1 / max(n, 1)


def test_few_x3_training_steps_reduce_the_loss():
    """tests/test_gpu_train_loop.py's loop with train_precision="bf16x3": the loss stays finite and falls"""
    from dinov2_od_amd.matching import HungarianMatcher
    from tests import gpu_util as G
    torch.manual_seed(0)
    bb, dc = cases.cfg1(25)
    m = G.make_detector(bb, dc, "bf16", "facebook/dinov2-small").set_train_precision("bf16x3")
    matcher = HungarianMatcher(per_image_rows=True)
    x = G.to_gpu(synth.make_pixels(4, 112, 112, seed=0))
    rng = np.random.default_rng(0)
    targets = []
    for b in range(4):
        n = int(rng.integers(1, 5))
        cxcy = 0.2 + 0.6 * rng.random((n, 2))
        wh = 0.1 + 0.2 * rng.random((n, 2))
        targets.append({"labels": torch.from_numpy(rng.integers(1, dc.num_classes, n)).cuda(),
                        "boxes": torch.from_numpy(np.concatenate([cxcy, wh], 1).astype(np.float32)).cuda()})
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=2e-3)
    losses = []
    m.train()
    n0 = _counter("f32x3_launches")
    for _ in range(8):
        out = m(x)
        idx = matcher({"pred_logits": out["pred_logits"].detach(), "pred_boxes": out["pred_boxes"].detach()}, targets)
        loss = _loss(out, targets, idx, dc.num_classes)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert _counter("f32x3_launches") > n0
    assert all(np.isfinite(losses))
    assert min(losses[-3:]) < 0.8 * losses[0], losses
