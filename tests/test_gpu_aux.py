"""`-m gpu`: deep supervision (aux_loss=True) on the native kernels -- the decoder step with L outputs (dec_train.hip through
dod_decoder_train_aux_forward / _backward) against the autograd composite and against the plain native step, its dropout
seeding, the layered criterion (criterion.hip, dod_set_criterion_layers_*) against the single-layer entry points and float64,
and a whole detector step through SetCriterion in host and device assignment modes against the composite and golden G11."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, losses as L, synth
from tests import aux_cases as ac
from tests import cases, criterion_cases as cc, criterion_edge_cases as ce
from tests.cases import rel_err, rel_l2

pytestmark = pytest.mark.gpu

CASES = [  # Dd, Hd, Q, layers, F, C, P, B, N
    (128, 4, 7, 3, 256, 11, 2, 2, 26),       # G11's micro decoder
    (128, 4, 7, 2, 256, 11, 2, 3, 257),      # prime token count, three images
    (192, 2, 5, 3, 256, 11, 4, 2, 1370),     # head_dim 96, 4 points
    (768, 8, 100, 3, 1024, 91, 2, 2, 257),   # config.py:21-35 defaults (tied x3)
]
MEM_STD = {768: 0.1}      # as tests/test_gpu_train_native.py: unit-variance memory is ill-conditioned at Dd = 768
_ID = lambda c: f"Dd{c[0]}_Q{c[2]}_L{c[3]}_N{c[8]}"


def _decoder(dc, dropout=0.0, aux=True):
    from dinov2_od_amd.models import DETRDecoder
    from tests import gpu_util as G
    m = DETRDecoder(dc.num_queries, dc.hidden_dim, dc.nheads, dc.num_layers, dc.num_classes, dim_feedforward=dc.dim_feedforward,
                    dropout=dropout, n_points=dc.n_points, use_deformable=True, precision="fp32", aux_loss=aux)
    G.load_np_state(m, synth.decoder_state_dict(dc, seed=1, prefix=""))
    m = m.to(G.dev()).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = dropout
    return m


def _layers(o):
    """decoder layers 0 .. L-1 of an output dict"""
    return list(o.get("aux_outputs", ())) + [o]


def _run(m, mem, wl, wb, native):
    """loss = sum over the supervised layers of <logits_l, wl[l]> + <boxes_l, wb[l]> (wl / wb hold the LAST layers' weights when the
    module supervises fewer) -> per-layer (logits, boxes), d(memory), parameter gradients"""
    os.environ["DINODET_NATIVE_TRAIN"] = "1" if native else "0"
    try:
        m.zero_grad(set_to_none=True)
        x = mem.clone().requires_grad_(True)
        ls = _layers(m(x))
        off = wl.shape[0] - len(ls)
        sum((o["pred_logits"] * wl[off + j]).sum() + (o["pred_boxes"] * wb[off + j]).sum() for j, o in enumerate(ls)).backward()
        g = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        return [(o["pred_logits"].detach().clone(), o["pred_boxes"].detach().clone()) for o in ls], x.grad.detach().clone(), g
    finally:
        os.environ.pop("DINODET_NATIVE_TRAIN", None)


def _inputs(case):
    """the memory and the last layer's loss weights of test_native_decoder_backward_matches_composite_autograd (the inputs its rule was
    stated on: see _grad_rule), and other random weights for every layer below"""
    from tests import gpu_util as G
    Dd, Hd, Q, layers, F, Cc, P, B, N = case
    mem = G.to_gpu(synth.normal(3, f"memory.train.{N}.{Dd}", (B, N, Dd), 1.0) * np.float32(MEM_STD.get(Dd, 1.0)))
    wl = np.stack([synth.normal(5, f"aux.wl.{l}", (B, Q, Cc), 1.0) for l in range(layers - 1)] + [synth.normal(5, "train.wl", (B, Q, Cc), 1.0)])
    wb = np.stack([synth.normal(5, f"aux.wb.{l}", (B, Q, 4), 1.0) for l in range(layers - 1)] + [synth.normal(5, "train.wb", (B, Q, 4), 1.0)])
    return mem, G.to_gpu(wl), G.to_gpu(wb)


def _grad_rule(case):
    """test_native_decoder_backward_matches_composite_autograd's own rule: 1e-4 element-relative, or rel_l2 < 1e-2 for the deep
    768-wide case (its reasons: the sampling gradient is piecewise smooth, a ReLU unit at zero flips a whole row).
    That bound compares two fp32 evaluations of an ill-conditioned gradient and holds on that test's memory tensor, which _inputs
    therefore reuses.  On another draw of the same distribution (synth tag "memory.aux.257.768", unit-normal weights on all three
    layers) the PLAIN step that predates deep supervision is already 5.9e-2 (rel_l2, reference_points_proj.weight) from the
    composite -- with the native step 5.3e-2 and the composite 7.7e-2 from the same math in float64 -- and the aux step 6.9e-2
    (7.1e-1 / 8.4e-1 from float64 on the two-element reference_points_proj.bias), while the aux step with zero upstream on the
    aux slices stays 1.2e-6 from the plain native step: conditioning of the inputs, not the schedule."""
    deep = case[0] >= 768 and case[3] >= 3
    return (rel_l2, 1e-2) if deep else (rel_err, 1e-4)


def _compare(case, a, b, what):
    """every parameter gradient and d(memory) of run a against run b at the rule above"""
    err, gtol = _grad_rule(case)
    assert set(a[2]) == set(b[2]) and len(a[2]) >= 30
    worst = max((float(err(a[2][k].cpu().numpy(), b[2][k].cpu().numpy())), k) for k in a[2])
    e = float(err(a[1].cpu().numpy(), b[1].cpu().numpy()))
    print(f"{what} {case}: worst parameter {worst[1]} {worst[0]:.2e}, d(memory) {e:.2e}")
    assert worst[0] < gtol and e < gtol, (worst, e)


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_native_aux_step_matches_composite_autograd(case):
    from dinov2_od_amd.models import _native_train as nt
    Dd, Hd, Q, layers, F, Cc, P, B, N = case
    m = _decoder(cases.dec_cfg(True, Dd, Hd, Q, layers, F, Cc, P))
    mem, wl, wb = _inputs(case)
    comp = _run(m, mem, wl, wb, native=False)
    natv = _run(m, mem, wl, wb, native=True)
    assert len(comp[0]) == len(natv[0]) == layers
    for j, ((l0, b0), (l1, b1)) in enumerate(zip(comp[0], natv[0])):
        el, eb = rel_err(l1.cpu().numpy(), l0.cpu().numpy()), rel_err(b1.cpu().numpy(), b0.cpu().numpy())
        print(f"layer {j}: forward logits {el:.2e} boxes {eb:.2e}")
        assert el < 1e-4 and eb < 1e-4, j
    _compare(case, natv, comp, "native aux vs composite aux")
    assert not any(k.startswith("reference_points.") for k in natv[2])
    # the last slice against the plain native forward: the class head's K-split may depend on the row count, so fp32-close, not bitwise
    with torch.no_grad():
        plain = nt.decoder_train(m, mem, seed=1, aux=False)
        packed = nt.decoder_train(m, mem, seed=1, aux=True)
    assert packed.shape == (layers, B, Q, Cc + 4)
    print(f"last slice of the aux forward torch.equal to the plain forward: {torch.equal(packed[-1], plain)}")
    assert rel_err(packed[-1, ..., :Cc].cpu().numpy(), plain[..., :Cc].cpu().numpy()) < 1e-4
    assert rel_err(packed[-1, ..., Cc:].cpu().numpy(), plain[..., Cc:].cpu().numpy()) < 1e-4


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=_ID)
def test_zero_upstream_on_the_aux_slices_is_the_plain_step(case):
    from dinov2_od_amd.models import _native_train as nt
    Dd, Hd, Q, layers, F, Cc, P, B, N = case
    dc = cases.dec_cfg(True, Dd, Hd, Q, layers, F, Cc, P)
    m = _decoder(dc)
    mem, wl, wb = _inputs(case)
    wl, wb = wl.clone(), wb.clone()
    wl[:-1] = 0
    wb[:-1] = 0
    aux = _run(m, mem, wl, wb, native=True)
    m.aux_loss = False
    plain = _run(m, mem, wl, wb, native=True)
    assert len(plain[0]) == 1
    _compare(case, aux, plain, "aux step with zero upstream on the aux slices vs plain native step")
    # with dropout the last slice is the plain step's output at the same seed: a mask mismatch would show as O(1)
    md = _decoder(dc, dropout=0.1)
    with torch.no_grad():
        a = nt.decoder_train(md, mem, seed=4321, aux=True)[-1]
        b = nt.decoder_train(md, mem, seed=4321, aux=False)
        c = nt.decoder_train(md, mem, seed=4322, aux=False)
    e = max(rel_err(a[..., :Cc].cpu().numpy(), b[..., :Cc].cpu().numpy()), rel_err(a[..., Cc:].cpu().numpy(), b[..., Cc:].cpu().numpy()))
    print(f"p = 0.1, same seed: last aux slice vs plain forward {e:.2e} (another seed: {rel_err(c.cpu().numpy(), b.cpu().numpy()):.2e})")
    assert e < 1e-4


def test_aux_dropout_masks_are_consistent_and_seeded():
    """as test_native_decoder_dropout_masks_are_consistent_and_seeded, with every layer's output in the loss: the forward is a function
    of the seed, and the backward applies the SAME masks (directional finite difference against the analytic gradient)"""
    from dinov2_od_amd.models import _native_train as nt
    from tests import gpu_util as G
    Ln = 3
    dc = cases.dec_cfg(True, 128, 4, 16, Ln, 256, 11, 2)
    m = _decoder(dc, dropout=0.1)
    B, N = 4, 257
    mem = G.to_gpu(synth.normal(3, "memory.auxdrop", (B, N, 128), 1.0))
    a = nt.decoder_train(m, mem, seed=1234, aux=True).detach().clone()
    b = nt.decoder_train(m, mem, seed=1234, aux=True).detach().clone()
    c = nt.decoder_train(m, mem, seed=99, aux=True).detach().clone()
    assert a.shape == (Ln, B, 16, 15) and torch.equal(a, b) and not torch.equal(a, c)
    assert all(not torch.equal(a[j], c[j]) for j in range(Ln))
    L0 = m.decoder.layers[0]
    with torch.no_grad():      # sampling locations frozen for the finite difference (a bilinear gather is only piecewise smooth)
        L0.reference_points_proj.weight.zero_()
        L0.cross_attn.sampling_offsets.weight.zero_()
    frozen = {id(L0.reference_points_proj.weight), id(L0.reference_points_proj.bias), id(L0.cross_attn.sampling_offsets.weight),
              id(L0.cross_attn.sampling_offsets.bias)}
    params = [q for q in m.parameters() if q.requires_grad and id(q) not in frozen]
    g = torch.Generator(device="cpu").manual_seed(0)
    dirs = [torch.randn(q.shape, generator=g).to(q.device) * (0.03 / max(1.0, q.numel() ** 0.5)) for q in params]
    vx = torch.randn(mem.shape, generator=g).to(mem.device) * (0.03 / mem.numel() ** 0.5)
    wl = G.to_gpu(synth.normal(5, "auxdrop.wl", (Ln, B, 16, 15), 1.0))

    def f(x):
        return (nt.decoder_train(m, x, seed=77, aux=True) * wl).sum()
    x = mem.clone().requires_grad_(True)
    m.zero_grad(set_to_none=True)
    f(x).backward()
    ana = float(sum((q.grad * v).sum() for q, v in zip(params, dirs) if q.grad is not None) + (x.grad * vx).sum())
    with torch.no_grad():
        for q, v in zip(params, dirs):
            q.add_(v)
        lp = float(f(mem + vx))
        for q, v in zip(params, dirs):
            q.sub_(2 * v)
        lm = float(f(mem - vx))
        for q, v in zip(params, dirs):
            q.add_(v)
    num = (lp - lm) / 2
    print(f"aux dropout directional derivative: analytic {ana:.5f}, central difference {num:.5f}")
    assert abs(ana - num) < 2e-2 * abs(num) + 1e-3


def test_eval_has_no_aux_outputs():
    Dd, Hd, Q, Ln, F, Cc, P, B, N = ac.MICRO
    from tests import gpu_util as G
    m = _decoder(ac.micro_cfg()).eval()
    plain = _decoder(ac.micro_cfg(), aux=False).eval()
    mem = G.to_gpu(cases.g1_memory(N, Dd))
    o, p = m(mem), plain(mem)
    assert set(o) == {"pred_logits", "pred_boxes"}
    assert torch.equal(o["pred_logits"], p["pred_logits"]) and torch.equal(o["pred_boxes"], p["pred_boxes"])


# ------------------------------------------------------------------------------------------------ layered criterion
CANARY = 12345.0
_I64 = C.c_int64


def _guarded(n, dev):
    """an output buffer of n floats between two 64-float canaries -> (whole buffer, the view to write)"""
    buf = torch.full((n + 128,), CANARY, dtype=torch.float32, device=dev)
    return buf, buf[64:64 + n]


def _intact(buf, n):
    return bool((buf[:64] == CANARY).all()) and bool((buf[64 + n:] == CANARY).all())


@pytest.mark.parametrize("B,Q,Cc", [(3, 7, 11), (3, 7, 91)], ids=["C11", "C91"])
@pytest.mark.parametrize("nl", [1, 3])
def test_layered_criterion_is_the_single_layer_call_per_layer(nl, B, Q, Cc):
    """21 rows per layer (not a multiple of the 16-row workgroup), one image without targets, 91 classes = more than one wave
    stride; NaN rows behind the last row, canaries around every output"""
    dev = torch.device("cuda:0")
    lib = nat.lib()
    counts = [3, 0, 2]
    R, W = B * Q, Cc + 4
    rng = np.random.default_rng(100 * nl + Cc)
    det_np = np.stack([cc.synth_inputs(B, Q, Cc, counts, seed=31 + l)[0] for l in range(nl)])            # [nl, B, Q, C+4]
    _, labels_np, gt_np, offs = cc.synth_inputs(B, Q, Cc, counts, seed=31)
    idx = [[(torch.from_numpy(np.sort(rng.permutation(Q)[:n]).astype(np.int64)), torch.from_numpy(rng.permutation(n).astype(np.int64)))
            for n in counts] for _ in range(nl)]
    match = torch.cat([L.match_table(i, counts, Q) for i in idx]).to(dev)
    guard = 8
    det = torch.full((nl * R + guard, W), float("nan"), dtype=torch.float32, device=dev)
    det[:nl * R] = torch.from_numpy(det_np).reshape(nl * R, W).to(dev)
    labels, gt = torch.from_numpy(labels_np).to(dev), torch.from_numpy(gt_np).to(dev)
    G_ = int(labels.numel())
    nb = torch.tensor([float(sum(counts))], device=dev)
    dl = torch.from_numpy(rng.uniform(0.5, 2.0, (nl, 3)).astype(np.float32)).to(dev)
    s = nat.stream_ptr()
    lg, bx = det[:, :Cc], det[:, Cc:]

    ws = torch.empty(lib.dod_set_criterion_layers_workspace_bytes(nl, B, Q, Cc) // 4, dtype=torch.float32, device=dev)
    assert ws.numel() == nl * 3 * ((R + 15) // 16)
    lbuf, losses = _guarded(nl * 3, dev)
    glbuf, d_logits = _guarded(nl * R * Cc, dev)
    gbbuf, d_boxes = _guarded(nl * R * 4, dev)
    nat.check(lib.dod_set_criterion_layers_forward(nat.ptr(lg), W, nat.ptr(bx), W, nl, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G_, nat.ptr(match),
                                                   nl * R, nat.ptr(nb), 0.25, 2.0, nat.ptr(losses), None, nat.ptr(ws), ws.numel() * 4, s))
    nat.check(lib.dod_set_criterion_layers_backward(nat.ptr(lg), W, nat.ptr(bx), W, nl, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G_, nat.ptr(match),
                                                    nl * R, nat.ptr(nb), 0.25, 2.0, nat.ptr(dl), None, nat.ptr(d_logits), nat.ptr(d_boxes), s))
    torch.cuda.synchronize()
    assert _intact(lbuf, nl * 3) and _intact(glbuf, nl * R * Cc) and _intact(gbbuf, nl * R * 4)
    assert bool(torch.isfinite(losses).all()) and bool(torch.isfinite(d_logits).all()) and bool(torch.isfinite(d_boxes).all())
    losses, d_logits, d_boxes = losses.view(nl, 3), d_logits.view(nl, R, Cc), d_boxes.view(nl, R, 4)
    # a wrong-sized table or workspace is refused before any launch
    assert lib.dod_set_criterion_layers_forward(nat.ptr(lg), W, nat.ptr(bx), W, nl, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G_, nat.ptr(match),
                                                nl * R + 1, nat.ptr(nb), 0.25, 2.0, nat.ptr(losses), None, nat.ptr(ws), ws.numel() * 4, s) == 1
    assert lib.dod_set_criterion_layers_forward(nat.ptr(lg), W, nat.ptr(bx), W, nl, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G_, nat.ptr(match),
                                                nl * R, nat.ptr(nb), 0.25, 2.0, nat.ptr(losses), None, nat.ptr(ws), ws.numel() * 4 - 4, s) == 3
    ws1 = torch.empty(lib.dod_set_criterion_workspace_bytes(B, Q, Cc) // 4, dtype=torch.float32, device=dev)
    for l in range(nl):
        # bit-identical to the single-layer entry points on the slice
        one, gl1, gb1 = torch.empty(3, device=dev), torch.empty(R, Cc, device=dev), torch.empty(R, 4, device=dev)
        sl, sb, sm = lg[l * R:], bx[l * R:], match[l * R:(l + 1) * R].contiguous()
        nat.check(lib.dod_set_criterion_forward(nat.ptr(sl), W, nat.ptr(sb), W, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G_, nat.ptr(sm), R,
                                                nat.ptr(nb), 0.25, 2.0, nat.ptr(one), None, nat.ptr(ws1), ws1.numel() * 4, s))
        nat.check(lib.dod_set_criterion_backward(nat.ptr(sl), W, nat.ptr(sb), W, B, Q, Cc, nat.ptr(labels), nat.ptr(gt), G_, nat.ptr(sm), R,
                                                 nat.ptr(nb), 0.25, 2.0, nat.ptr(dl[l].contiguous()), None, nat.ptr(gl1), nat.ptr(gb1), s))
        torch.cuda.synchronize()
        assert torch.equal(one, losses[l]) and torch.equal(gl1, d_logits[l]) and torch.equal(gb1, d_boxes[l]), l
        # and within criterion_cases' float64 bounds (tests/test_gpu_criterion.py: 1e-5 on the losses, 1e-5 of max|g| on the gradients)
        d64 = torch.from_numpy(det_np[l]).double().requires_grad_(True)
        ref = L.composite_losses(d64[..., :Cc], d64[..., Cc:], torch.from_numpy(labels_np), torch.from_numpy(gt_np).double(), sm.cpu(), nb.double().cpu())
        (ref * dl[l].double().cpu()).sum().backward()
        r, got = ref.detach().numpy(), losses[l].cpu().numpy()
        assert (np.abs(got - r) <= 1e-5 * np.abs(r)).all() or np.abs(got - r).max() <= 1e-5 * np.abs(r).max(), (l, got, r)
        g64 = d64.grad.numpy().reshape(R, W)
        for mine, want, key in ((d_logits[l].cpu().numpy(), g64[:, :Cc], "dlogits"), (d_boxes[l].cpu().numpy(), g64[:, Cc:], "dboxes")):
            err, scale = np.abs(mine - want).max(), np.abs(want).max()
            assert err <= 1e-5 * scale, (l, key, err, scale)
        # and element by element (tests/criterion_edge_cases.py)
        flat = det_np[l].reshape(R, W)
        ref64 = ce.reference(flat[:, :Cc], flat[:, Cc:], labels_np, gt_np, sm.cpu().numpy(), float(sum(counts)), 0.25, 2.0, d_losses=dl[l].cpu().numpy())
        ce.check({"losses": got, "d_logits": d_logits[l].cpu().numpy(), "d_boxes": d_boxes[l].cpu().numpy()}, ref64, f"nl={nl} C={Cc} layer {l}")
    # the Python layer: packed slices are read in place, separate tensors go through one stacked copy -- same bits either way
    d = det[:nl * R].clone().view(nl, B, Q, W).requires_grad_(True)
    views = L.native_losses_layers([d[l, ..., :Cc] for l in range(nl)], [d[l, ..., Cc:] for l in range(nl)], labels, gt, match, nb)
    (views * dl).sum().backward()
    e = det[:nl * R].clone().view(nl, B, Q, W).requires_grad_(True)
    copies = L.native_losses_layers([e[l, ..., :Cc].contiguous() for l in range(nl)], [e[l, ..., Cc:].contiguous() for l in range(nl)],
                                    labels, gt, match, nb)
    (copies * dl).sum().backward()
    assert torch.equal(views.detach(), losses) and torch.equal(copies.detach(), losses)
    assert torch.equal(d.grad[..., :Cc].reshape(nl, R, Cc), d_logits) and torch.equal(d.grad[..., Cc:].reshape(nl, R, 4), d_boxes)
    assert torch.equal(d.grad, e.grad)


# ------------------------------------------------------------------------------------------------ detector step
class _Recording:
    """our HungarianMatcher, keeping each call's assignment as a [B*Q] table (host mode: from the indices; device mode: the table)"""

    def __init__(self, counts, Q):
        from dinov2_od_amd.matching import HungarianMatcher
        self.inner, self.counts, self.Q, self.tables = HungarianMatcher(), counts, Q, []

    def __call__(self, outputs, tg):
        r = self.inner(outputs, tg)
        self.tables.append(L.match_table(r, self.counts, self.Q).clone())
        return r

    def match_table(self, outputs, tg):
        t, st = self.inner.match_table(outputs, tg)
        self.tables.append(t.cpu())
        return t, st


def test_detector_aux_step_through_the_criterion():
    """cfg1 (two decoder layers) with aux_loss=True through SetCriterion in host and device assignment modes: same keys and
    assignments, gradients against the composite and against the reference's (golden G11), deterministic mode bit-identical"""
    from tests import gpu_util as G
    from dinov2_od_amd.models import DINOv2ObjectDetector
    g = cases.golden("g11_aux_cfg1")
    model_name, R, B, kw = cases.G9_CASES[ac.DETECTOR]
    m = DINOv2ObjectDetector(dino_model_name=model_name, pretrained=False, precision="fp32", aux_loss=True, **kw)
    G.load_np_state(m, synth.detector_state_dict(m._bb_cfg, m._dc_cfg, seed=1))
    m = m.to(G.dev()).train()
    x = G.to_gpu(synth.make_pixels(B, R, R, seed=0))
    Q, Cc = kw["num_queries"], kw["num_classes"]
    tg = ac.targets(Cc, device=G.dev())

    def run(native, device_assignment):
        os.environ["DINODET_NATIVE_TRAIN"] = "1" if native else "0"
        try:
            m.zero_grad(set_to_none=True)
            rec = _Recording(list(ac.COUNTS), Q)
            crit = L.SetCriterion(rec, Cc, dict(cc.WEIGHTS), device_assignment=device_assignment)
            o = m(x)
            ld = crit(o, tg)
            sum(ld.values()).backward()
            crit.check_assignment()
            if device_assignment:
                assert crit.last_assignment_status.shape == (2 * B,)
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
            return {k: float(v.detach()) for k, v in ld.items()}, rec.tables, grads, o
        finally:
            os.environ.pop("DINODET_NATIVE_TRAIN", None)

    comp = run(False, False)
    host = run(True, False)
    # the reference's step (G11), at G9's gate for cfg1
    o = host[3]
    assert [x_["pred_logits"].data_ptr() for x_ in o["aux_outputs"]] == [o["pred_logits"].data_ptr() - B * Q * (Cc + 4) * 4]      # one packed buffer
    for j, oj in enumerate(list(o["aux_outputs"]) + [o]):
        assert rel_err(oj["pred_logits"].detach().cpu().numpy(), g[f"cfg1.l{j}.logits"]) < 1e-3
        assert rel_err(oj["pred_boxes"].detach().cpu().numpy(), g[f"cfg1.l{j}.boxes"]) < 1e-3
        want = L.match_table([(torch.from_numpy(i), torch.from_numpy(k)) for i, k in ac.golden_indices(g, "cfg1", j, B)], list(ac.COUNTS), Q)
        assert torch.equal(host[1][j], want), j
        for n, k in enumerate(L.LOSS_KEYS):
            mine, ref = host[0][k if j == 1 else f"{k}_{j}"], float(g[f"cfg1.l{j}.losses"][n])
            assert abs(mine - ref) < 1e-3 * max(1.0, abs(ref)), (j, k, mine, ref)
    worst = ac.grad_check(m, g, 2e-4, 2e-4)
    print(f"native aux step vs the reference (G11): worst gradient probe {worst[0]:.2e} ({worst[1]})")
    dev_ = run(True, True)
    assert set(host[0]) == set(dev_[0]) == set(comp[0]) == set(L.LOSS_KEYS) | {f"{k}_0" for k in L.LOSS_KEYS}
    assert len(host[1]) == len(dev_[1]) == 2 and all(torch.equal(a, b) for a, b in zip(host[1], dev_[1]))
    for k in host[0]:       # the same assignment on the same forward
        assert abs(host[0][k] - dev_[0][k]) <= 1e-6 * max(1.0, abs(host[0][k])), k
    # against the composite, at the native decoder step's rule
    assert set(comp[2]) == set(host[2]) == set(dev_[2])
    worst = max((rel_err(host[2][k].cpu().numpy(), comp[2][k].cpu().numpy()), k) for k in comp[2])
    print(f"native aux step vs composite aux step: worst gradient {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 1e-4, worst
    nat.set_option("deterministic", 1)
    try:
        d1, d2 = run(True, True), run(True, True)
    finally:
        nat.set_option("deterministic", -1)
    assert d1[0] == d2[0] and set(d1[2]) == set(d2[2]) == set(host[2])
    for k in d1[2]:
        assert torch.equal(d1[2][k], d2[2][k]), f"{k}: not bit-reproducible in deterministic mode"
