"""What the optimizer extensions promise without a GPU: the float64 restatement of tests/optim_cases.py is PyTorch's Adam / AdamW / lerp,
optim.AdamW on CPU parameters is torch.optim.AdamW, ModelEMA shares the frozen parameters and follows its formula, and an engine module
deep-copies and pickles without its engine."""
import copy
import math
import pickle

import pytest
import torch

from dinov2_od_amd import optim
from tests import optim_cases as oc

HYP = dict(betas=(0.9, 0.999), eps=1e-8)
GROUPS = [([0, 2], dict(HYP, lr=1e-3, weight_decay=1e-2)), ([1, 3], dict(HYP, lr=3e-2, weight_decay=0.3))]
SHAPES = [(7,), (3, 5), (1,), (4, 4)]


def _rel(a, b):
    """max |a - b| over max |b|: the error relative to the tensor's scale (an element that cancels to ~0 has no relative accuracy in
    either evaluation order)"""
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam_l2", "adamw"])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_restatement_is_pytorch_in_float64(decoupled, max_norm):
    gen = torch.Generator().manual_seed(11)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in SHAPES]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[ps[i] for i in idx], **hyp) for idx, hyp in GROUPS])
    snap = [dict(p=p.detach().clone(), g=None, m=None, v=None, t=0.0) for p in ps]
    for step in range(3):
        for i, (p, s) in enumerate(zip(ps, snap)):
            none = step == 1 and i == 2                      # one parameter misses a gradient on the second step: its t stays behind
            p.grad = None if none else 3.0 * torch.randn(p.shape, generator=gen, dtype=torch.float64)
            s["g"] = None if none else p.grad.clone()
        out, norm, _ = oc.step64(snap, GROUPS, max_norm, decoupled)
        if max_norm is not None:
            want_norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            assert abs(norm - float(want_norm)) <= 1e-14 * float(want_norm)
        opt.step()
        for i, (p, o) in enumerate(zip(ps, out)):
            st = opt.state[p]
            assert float(st["step"]) == o["t"]
            assert _rel(o["p"], p.detach()) <= 1e-14 and _rel(o["m"], st["exp_avg"]) <= 1e-14 and _rel(o["v"], st["exp_avg_sq"]) <= 1e-14, (step, i)
            snap[i] = dict(p=o["p"], g=None, m=o["m"], v=o["v"], t=o["t"])      # the restatement runs on its own state throughout


def test_restatement_ema_is_a_float64_lerp():
    gen = torch.Generator().manual_seed(12)
    e, p = torch.randn(1000, generator=gen, dtype=torch.float64), torch.randn(1000, generator=gen, dtype=torch.float64)
    for d in (0.9, 0.9999, 0.999999):
        w = 1.0 - d
        assert _rel(oc.ema64(e, p, w), torch.lerp(e, p, w)) <= 1e-15
    assert oc.ema_weight(0.9999, 0, 5) == 1.0 - 0.9999
    assert oc.ema_weight(0.9999, 2000, 5) == 1.0 - 0.9999 * (1.0 - math.exp(-5 / 2000))


def test_restatement_skip_keeps_the_state_and_advances_t():
    snap = [dict(p=torch.ones(3), g=torch.tensor([1.0, float("inf"), 0.0]), m=torch.full((3,), 0.5), v=torch.ones(3), t=4.0, e=torch.zeros(3))]
    groups = [([0], dict(HYP, lr=1e-3, weight_decay=1e-2))]
    out, norm, skipped = oc.step64(snap, groups, 1.0, True, ema_w=0.1, skip_nonfinite=True)
    assert skipped and not math.isfinite(norm) and out[0]["t"] == 5.0
    for k in ("p", "m", "v", "e"):
        assert torch.equal(out[0][k], snap[0][k].double())
    out, _, skipped = oc.step64(snap, groups, 1.0, True, ema_w=0.1, skip_nonfinite=False)
    assert not skipped and torch.isnan(out[0]["p"]).tolist() == [False, True, False]      # coef = 1 / inf = 0, and 0 * inf is NaN


def _cpu_pair(cls_ours, cls_theirs, **kw):
    gen = torch.Generator().manual_seed(13)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    ours, theirs = [torch.nn.Parameter(t.clone()) for t in init], [torch.nn.Parameter(t.clone()) for t in init]
    mk = lambda cls, ps, **more: cls([dict(params=[ps[i] for i in idx], **hyp) for idx, hyp in GROUPS], **more)
    return ours, theirs, mk(cls_ours, ours, **kw), mk(cls_theirs, theirs), gen


def test_adamw_on_cpu_parameters_is_torch_adamw():
    ours, theirs, a, b, gen = _cpu_pair(optim.AdamW, torch.optim.AdamW)
    assert isinstance(a, torch.optim.AdamW) and a.defaults["weight_decay"] == 1e-2 and a.defaults["decoupled_weight_decay"]
    for _ in range(3):
        for p, q in zip(ours, theirs):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        a.step()
        b.step()
    for p, q in zip(ours, theirs):
        assert torch.equal(p.detach(), q.detach())
    # the state interchanges in both directions, and the next step agrees bit for bit again
    c = torch.optim.AdamW([dict(params=[ours[i] for i in idx], **hyp) for idx, hyp in GROUPS])
    c.load_state_dict(a.state_dict())
    d = optim.AdamW([dict(params=[theirs[i] for i in idx], **hyp) for idx, hyp in GROUPS])
    d.load_state_dict(b.state_dict())
    for p, q in zip(ours, theirs):
        p.grad = torch.randn(p.shape, generator=gen)
        q.grad = p.grad.clone()
    c.step()
    d.step()
    for p, q in zip(ours, theirs):
        assert torch.equal(p.detach(), q.detach())
        assert float(c.state[p]["step"]) == float(d.state[q]["step"]) == 4.0


def test_adam_with_the_decoupled_flag_is_adamw_and_clips_on_cpu():
    ours, theirs, a, b, gen = _cpu_pair(optim.Adam, torch.optim.AdamW, decoupled_weight_decay=True, max_grad_norm=1.0)
    for p, q in zip(ours, theirs):
        p.grad = 3.0 * torch.randn(p.shape, generator=gen)
        q.grad = p.grad.clone()
    a.step()
    torch.nn.utils.clip_grad_norm_(theirs, 1.0)
    b.step()
    for p, q in zip(ours, theirs):
        assert torch.equal(p.detach(), q.detach())


def test_skip_nonfinite_raises_on_the_delegated_path():
    ps = [torch.nn.Parameter(torch.ones(3))]
    opt = optim.AdamW(ps, skip_nonfinite=True)
    ps[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="skip_nonfinite"):
        opt.step()


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.frozen = torch.nn.Linear(4, 4)
        self.head = torch.nn.Linear(4, 2)
        self.register_buffer("scale", torch.ones(1))
        for p in self.frozen.parameters():
            p.requires_grad = False


def test_model_ema_shares_the_frozen_parameters_and_follows_its_formula():
    torch.manual_seed(14)
    model = _Tiny().train()
    ema = optim.ModelEMA(model, decay=0.99, tau=3)
    assert not ema.module.training and model.training
    theirs, mine = dict(ema.module.named_parameters()), dict(model.named_parameters())
    for n, p in mine.items():
        assert (theirs[n].data_ptr() == p.data_ptr()) == (not p.requires_grad), n
        assert not theirs[n].requires_grad and theirs[n].dtype == torch.float32
    assert ema.module.scale.data_ptr() != model.scale.data_ptr()             # a buffer is copied, as deepcopy copies it
    want = {n: p.detach().double().clone() for n, p in mine.items() if p.requires_grad}
    for k in (1, 2, 3):
        with torch.no_grad():
            for p in model.head.parameters():
                p.add_(torch.randn_like(p))
        versions = {n: theirs[n]._version for n in want}
        ema.update()
        w = 1.0 - 0.99 * (1.0 - math.exp(-k / 3))
        assert ema.updates == k and ema.weight(k) == w
        for n in want:
            want[n] = oc.ema64(want[n], mine[n].detach(), w).float().double()      # rounded once, as the shadow is stored
            assert torch.equal(theirs[n].detach().double(), want[n]), (k, n)
            assert theirs[n]._version > versions[n]
        assert torch.equal(theirs["frozen.weight"], mine["frozen.weight"])
    # the state round trip
    state = copy.deepcopy(ema.state_dict())
    assert state["updates"] == 3 and state["decay"] == 0.99 and state["tau"] == 3.0 and set(state["shadows"]) == set(want)
    other = optim.ModelEMA(model, decay=0.5)
    other.load_state_dict(state)
    assert (other.updates, other.decay, other.tau) == (3, 0.99, 3.0)
    for n, e in other.module.named_parameters():
        assert torch.equal(e, theirs[n])
    with pytest.raises(KeyError):
        other.load_state_dict(dict(state, shadows={}))


def test_update_raises_when_the_optimizer_drives_the_average():
    torch.manual_seed(15)
    model = _Tiny()
    ema = optim.ModelEMA(model, decay=0.9)
    head = list(model.head.parameters())
    opt = optim.AdamW(head, lr=1e-2, ema=ema)
    ref = [torch.nn.Parameter(p.detach().clone()) for p in head]
    ref_opt = torch.optim.AdamW(ref, lr=1e-2)
    shadow = [p.detach().double().clone() for p in head]
    head[0].grad, ref[0].grad = torch.ones_like(head[0]), torch.ones_like(ref[0])      # the bias has no gradient: its average still moves
    opt.step()
    ref_opt.step()
    assert ema.updates == 1
    for e, p, r, s in zip(ema.module.head.parameters(), head, ref, shadow):
        assert torch.equal(p.detach(), r.detach())
        assert torch.equal(e.detach().double(), oc.ema64(s, p.detach(), 1.0 - 0.9).float().double())
    with pytest.raises(RuntimeError, match="update"):
        ema.update()
    with pytest.raises(RuntimeError, match="already"):
        optim.AdamW(head, ema=ema)


def test_an_engine_module_copies_and_pickles_without_its_engine():
    from dinov2_od_amd.models import DINOv2Backbone
    from tests import cases

    m = DINOv2Backbone(pretrained=False, precision="fp32", config=cases.micro_bb(), lora_r=2)
    named = m._engine_named()
    assert "_named_cache" in m.__dict__ and named
    m.__dict__["_engine"] = lambda: None                     # a stand-in for the Engine: neither copyable state nor picklable
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert "_engine" not in clone.__dict__ and "_named_cache" not in clone.__dict__
        assert clone.precision == m.precision and clone._bb_cfg == m._bb_cfg
        for (n, p), (k, q) in zip(m.state_dict().items(), clone.state_dict().items()):
            assert n == k and torch.equal(p, q) and p.data_ptr() != q.data_ptr()
        assert [k for k, _ in clone._engine_named()] == [k for k, _ in named]      # the copy builds its own cache
    assert "_engine" in m.__dict__                           # the original keeps its engine
