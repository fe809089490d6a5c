"""AdamW, the fused moving average and the non-finite skip of csrc/optim.hip (dod_optim_step, dod_optim_ema_update; dinov2_od_amd.optim's
AdamW, ModelEMA, skip_nonfinite) against the float64 restatement of tests/optim_cases.py.

Bounds, u = 2^-24, from the arithmetic (DESIGN.md section 6b derives them; none comes from what the kernels give):
    |m' - m64| <= 4u (|m| + |g|)              g the clipped gradient, with the L2 term where the decay is L2
    |v' - v64| <= 6u v64 + 2^-149
    |p' - p64| <= u |p64| + 8u |D64| + step_size 4u (|m| + |g|) / den64
    |norm - norm64| <= 2 ulp_fp32(norm64)
    |e' - e64| <= u |e64| + 2^-149            e64 = e + (p' - e) w in float64 from the device's stored p'
The decoupled decay adds nothing to the bound on p: p (1 - lr wd) - delta is evaluated in double (2^-53 relative, inside the slack of
round-to-nearest's u / (1 + u)) and rounded once, the rounding the L2 form's final subtraction already has.
PyTorch's fp32 AdamW on the GPU from the same state is printed beside every figure and not asserted.
Every tensor is carved out of a flat buffer between NaN guard elements that must keep their bits; lengths sit around the 4-wide vector and
the chunk of one workgroup, carved 16-byte aligned, 4-byte aligned, and with the average alone off the 16-byte grid."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import optim
from tests import optim_cases as oc
from tests.test_gpu_optim import _ratio, norm_ratio

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD_BITS = 0x7FC0A5A5                 # a NaN no arithmetic produces
KEYS = ("p", "g", "m", "v", "e")
HYP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
T0 = 3.0                                # the step count every state starts from
LAYOUTS = {"aligned16": (0, 0), "aligned4": (1, 1), "ema_off_grid": (0, 1)}      # element offset of p g m v / of e


def _counter(name):
    return nat.lib().dod_test_counter(name.encode())


def _lengths():
    c = _counter("optim_chunk_elems")
    return [1, 3, 0, 4, 5, c - 1, c, c + 1, 2 * c + 3]


class Rig:
    """p, g, m, v, e of every tensor carved out of one flat device buffer per kind, NaN guards in front of, between and behind them"""

    def __init__(self, lengths, layout="aligned16", seed=0):
        self.n = list(lengths)
        off, e_off = LAYOUTS[layout]
        self.start, at = [], 8
        for n in self.n:
            self.start.append(at)
            at += n + 4 + (-n) % 4          # a gap of 4..7 guard elements; every start keeps the carve's alignment
        self.size = at + 8
        self.off = {k: (e_off if k == "e" else off) for k in KEYS}
        d = torch.device("cuda:0")
        self.flat = {k: torch.full((self.size,), GUARD_BITS, dtype=torch.int32, device=d).view(torch.float32) for k in KEYS}
        for k in KEYS:
            assert self.flat[k].data_ptr() % 16 == 0
        self.gen = torch.Generator().manual_seed(seed)
        self.params = []
        for i, n in enumerate(self.n):
            self.view("p", i).copy_(torch.randn(n, generator=self.gen))
            self.view("m", i).copy_(0.1 * torch.randn(n, generator=self.gen))
            self.view("v", i).copy_((0.1 * torch.randn(n, generator=self.gen)) ** 2)
            self.view("e", i).copy_(torch.randn(n, generator=self.gen))
            self.view("g", i).zero_()
            self.params.append(torch.nn.Parameter(self.view("p", i)))
        self.gap = {}
        for k in KEYS:
            gap = torch.ones(self.size, dtype=torch.bool, device=d)
            for s, n in zip(self.start, self.n):
                gap[self.off[k] + s:self.off[k] + s + n] = False
            self.gap[k] = gap

    def view(self, k, i):
        s = self.off[k] + self.start[i]
        return self.flat[k][s:s + self.n[i]]

    def attach_state(self, opt):
        for i, p in enumerate(self.params):
            opt.state[p] = {"step": torch.tensor(T0), "exp_avg": self.view("m", i), "exp_avg_sq": self.view("v", i)}

    def make_ema(self, decay, tau=0):
        """a ModelEMA over the rig's parameters whose shadows are the rig's carved e tensors"""
        holder = torch.nn.Module()
        holder.list = torch.nn.ParameterList(self.params)
        ema = optim.ModelEMA(holder, decay=decay, tau=tau)
        for i, (e, p) in enumerate(ema._pairs):
            assert p is self.params[i]
            e.data = self.view("e", i)
        return ema

    def set_grads(self, scale=3.0, none=(), poison=None):
        for i, p in enumerate(self.params):
            if i in none:
                p.grad = None
                continue
            self.view("g", i).copy_(scale * torch.randn(self.n[i], generator=self.gen))
            p.grad = self.view("g", i)
        if poison is not None:
            last = max(i for i, n in enumerate(self.n) if n > 0 and i not in none)
            self.view("g", last)[self.n[last] // 2] = poison

    def guards_intact(self):
        return all(bool((self.flat[k].view(torch.int32)[self.gap[k]] == GUARD_BITS).all()) for k in KEYS)

    def bits(self, keys=("p", "m", "v", "e")):
        return {k: self.flat[k].view(torch.int32).clone() for k in keys}

    def snapshot(self, t=None, with_grad=None):
        out = []
        for i, p in enumerate(self.params):
            has = p.grad is not None if with_grad is None else i in with_grad
            out.append(dict(p=self.view("p", i).cpu().clone(), g=self.view("g", i).cpu().clone() if has else None,
                            m=self.view("m", i).cpu().clone(), v=self.view("v", i).cpu().clone(), e=self.view("e", i).cpu().clone(),
                            t=T0 if t is None else t[i]))
        return out

    def state64(self):
        return [{k: self.view(k, i).double().cpu() for k in ("p", "m", "v", "e")} for i in range(len(self.n))]


def same_bits(a, b, keys=("p", "m", "v", "e")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def ratios(snap, want, got, groups, decoupled):
    """worst ratio of |got - want| to the bounds of the docstring, over the parameters that had a gradient"""
    hyp_of = {i: hyp for idx, hyp in groups for i in idx}
    worst = dict(m=0.0, v=0.0, p=0.0)
    for i, (s, w, g) in enumerate(zip(snap, want, got)):
        if s["g"] is None:
            for k in ("p", "m", "v"):
                assert torch.equal(g[k], s[k].double()), (i, k)          # no gradient, nothing moves
            continue
        if w["p"].numel() == 0:
            continue
        bm = 4 * U * (s["m"].double().abs() + w["gd"].abs())
        bv = 6 * U * w["v"] + 2.0 ** -149
        bp = U * w["p"].abs() + 8 * U * w["delta"].abs() + w["step_size"] * bm / w["den"]
        worst["m"] = max(worst["m"], _ratio((g["m"] - w["m"]).abs(), bm))
        worst["v"] = max(worst["v"], _ratio((g["v"] - w["v"]).abs(), bv))
        worst["p"] = max(worst["p"], _ratio((g["p"] - w["p"]).abs(), bp))
    return worst


def ema_ratio(e_before, p_after, e_after, w):
    """worst |e' - e64| / (u |e64| + 2^-149), e64 from the device's stored p'"""
    worst = 0.0
    for e0, p1, e1 in zip(e_before, p_after, e_after):
        if e0.numel():
            e64 = oc.ema64(e0, p1, w)
            worst = max(worst, _ratio((e1 - e64).abs(), U * e64.abs() + 2.0 ** -149))
    return worst


def torch_adamw32(snap, groups, max_norm):
    """PyTorch's own fp32 clip + AdamW on the GPU from `snap`: the yardstick"""
    ps = [torch.nn.Parameter(s["p"].cuda()) for s in snap]
    opt = torch.optim.AdamW([dict(params=[ps[i] for i in idx], **hyp) for idx, hyp in groups])
    for p, s in zip(ps, snap):
        opt.state[p] = {"step": torch.tensor(s["t"]), "exp_avg": s["m"].cuda(), "exp_avg_sq": s["v"].cuda()}
        p.grad = None if s["g"] is None else s["g"].cuda()
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm is not None else None
    opt.step()
    return [dict(p=p.detach().double().cpu(), m=opt.state[p]["exp_avg"].double().cpu(), v=opt.state[p]["exp_avg_sq"].double().cpu()) for p in ps], norm


def one_group(rig, **hyp):
    return [(list(range(len(rig.params))), dict(HYP, **hyp))]


# ------------------------------------------------------------------------------------------------ the C entry, called directly
def abi_step(rig, hyp, decoupled=False, max_norm=0.0, ema=None, ema_w=0.0, skip=False, counter=None, old=False, t=T0 + 1):
    """dod_optim_step (old: dod_optim_adam_step) over every tensor of the rig; ema: the indices whose average travels, None = no list"""
    lib, k = nat.lib(), len(rig.n)
    b1, b2 = hyp["betas"]
    desc = np.zeros(k, dtype=optim._DESC)
    for key in ("p", "g", "m", "v"):
        desc[key] = [rig.view(key, i).data_ptr() for i in range(k)]
    desc["n"], desc["step_size"], desc["bc2_sqrt"] = rig.n, hyp["lr"] / (1 - b1 ** t), (1 - b2 ** t) ** 0.5
    wd = hyp.get("weight_decay", 0.0)
    norm = torch.full((), -1.0, device="cuda:0")
    nbytes = lib.dod_optim_workspace_bytes(k, sum(rig.n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    if old:
        optim._check(lib.dod_optim_adam_step(desc.ctypes.data, k, b1, b2, hyp["eps"], wd, max_norm, nat.ptr(norm), nat.ptr(ws), nbytes, nat.stream_ptr()))
        return norm
    o = nat.DodOptimOptions()
    o.beta1, o.beta2, o.eps, o.weight_decay, o.max_norm = b1, b2, hyp["eps"], 0.0 if decoupled else wd, max_norm
    o.ema_w, o.skip_nonfinite, o.total_norm_dev = ema_w, int(skip), nat.ptr(norm)
    o.skipped_dev = None if counter is None else nat.ptr(counter)
    decay = np.full(k, 1 - hyp["lr"] * wd, dtype=np.float64) if decoupled else None
    shadows = None
    if ema is not None:
        shadows = np.array([rig.view("e", i).data_ptr() if i in ema else 0 for i in range(k)], dtype=np.uint64)
    optim._check(lib.dod_optim_step(desc.ctypes.data, None if shadows is None else shadows.ctypes.data, None if decay is None else decay.ctypes.data,
                                    k, C.byref(o), nat.ptr(ws), nbytes, nat.stream_ptr()))
    return norm


def abi_ema(rig, idx, w):
    d = np.zeros(len(idx), dtype=optim._EMA_DESC)
    d["e"], d["p"], d["n"] = [rig.view("e", i).data_ptr() for i in idx], [rig.view("p", i).data_ptr() for i in idx], [rig.n[i] for i in idx]
    optim._check(nat.lib().dod_optim_ema_update(d.ctypes.data, len(idx), w, nat.stream_ptr()))


# ------------------------------------------------------------------------------------------------ case 1: AdamW against float64
@pytest.mark.parametrize("layout", ["aligned16", "aligned4"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_adamw_against_float64(layout, weight_decay, max_norm):
    rig = Rig(_lengths(), layout, seed=21)
    groups = one_group(rig, weight_decay=weight_decay)
    opt = optim.AdamW(rig.params, max_grad_norm=max_norm, **groups[0][1])
    rig.attach_state(opt)
    rig.set_grads(none=(1,))
    snap = rig.snapshot()
    e_bits = rig.flat["e"].view(torch.int32).clone()
    opt.step()
    got = rig.state64()
    want, norm64, _ = oc.step64(snap, groups, max_norm, decoupled=True)
    ref32, norm32 = torch_adamw32(snap, groups, max_norm)
    ours, theirs = ratios(snap, want, got, groups, True), ratios(snap, want, ref32, groups, True)
    line = f"adamw {layout} wd{weight_decay:g} clip{max_norm}: worst ratio to the bound, native / PyTorch fp32:  " + \
        "  ".join(f"{k} {ours[k]:.3f} / {theirs[k]:.3f}" for k in ("m", "v", "p"))
    if max_norm is not None:
        rn, rn32 = norm_ratio(opt.last_grad_norm, norm64), norm_ratio(norm32, norm64)
        line += f"  norm {rn:.3f} / {rn32:.3f}"
        assert float(opt.last_grad_norm) > max_norm                           # the clip was active
    print(line)
    assert rig.guards_intact(), "a guard element changed"
    assert torch.equal(rig.flat["e"].view(torch.int32), e_bits)              # no average was asked for
    assert all(float(opt.state[p]["step"]) == (T0 if i == 1 else T0 + 1) for i, p in enumerate(rig.params))
    assert ours["m"] <= 1 and ours["v"] <= 1 and ours["p"] <= 1, line
    if max_norm is not None:
        assert rn <= 1, line
    if weight_decay:
        l2, _, _ = oc.step64(snap, groups, max_norm, decoupled=False)
        assert ratios(snap, l2, got, groups, False)["p"] > 1                  # the decay was decoupled: the L2 step is somewhere else


# ------------------------------------------------------------------------------------------------ case 2: zero decay, L2 through the new entry
@pytest.mark.parametrize("layout", ["aligned16", "aligned4"])
def test_zero_decay_and_l2_equal_the_old_entry_bit_for_bit(layout):
    def fresh():
        rig = Rig(_lengths(), layout, seed=22)
        rig.set_grads()
        return rig
    # AdamW with weight_decay = 0 == dod_optim_adam_step with weight_decay = 0
    a, b = fresh(), fresh()
    norm_a = abi_step(a, dict(HYP, weight_decay=0.0), max_norm=1.0, old=True)
    opt = optim.AdamW(b.params, weight_decay=0.0, max_grad_norm=1.0, **HYP)
    b.attach_state(opt)
    opt.step()
    assert same_bits(a.bits(), b.bits()) and torch.equal(norm_a.view(torch.int32), opt.last_grad_norm.view(torch.int32))
    # the C entry itself: a decay list of ones is the old entry too
    c = fresh()
    abi_step(c, dict(HYP, weight_decay=0.0), decoupled=True, max_norm=1.0)
    assert same_bits(a.bits(), c.bits())
    # L2 through the new entry == the old entry
    a, b = fresh(), fresh()
    abi_step(a, dict(HYP, weight_decay=1e-4), max_norm=1.0, old=True)
    abi_step(b, dict(HYP, weight_decay=1e-4), max_norm=1.0)
    assert same_bits(a.bits(), b.bits()) and a.guards_intact() and b.guards_intact()
    assert not torch.equal(a.bits()["p"], Rig(_lengths(), layout, seed=22).bits()["p"])      # and something moved


# ------------------------------------------------------------------------------------------------ case 3: the moving average
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", [0.9, 0.9999, 0.999999])
def test_ema_is_one_rounding_from_float64_fused_and_standalone(layout, d):
    w = 1.0 - d
    hyp = dict(HYP, weight_decay=1e-2)
    fused, alone = Rig(_lengths(), layout, seed=23), Rig(_lengths(), layout, seed=23)
    k = len(fused.n)
    null = 6                                                    # this tensor's entry of the ema list is NULL
    with_ema = [i for i in range(k) if i != null]
    for rig in (fused, alone):
        rig.set_grads()
    e0 = [fused.view("e", i).double().cpu() for i in range(k)]
    e_bits0 = fused.view("e", null).view(torch.int32).clone()
    abi_step(fused, hyp, decoupled=True, max_norm=1.0, ema=with_ema, ema_w=w)
    abi_step(alone, hyp, decoupled=True, max_norm=1.0)
    abi_ema(alone, with_ema, w)
    assert fused.guards_intact() and alone.guards_intact()
    assert same_bits(fused.bits(), alone.bits()), "the fused and the standalone average differ"
    assert torch.equal(fused.view("e", null).view(torch.int32), e_bits0), "the tensor with a NULL entry was touched"
    p1 = [fused.view("p", i).double().cpu() for i in range(k)]
    e1 = [fused.view("e", i).double().cpu() for i in range(k)]
    sel = lambda x: [x[i] for i in with_ema]
    worst = ema_ratio(sel(e0), sel(p1), sel(e1), w)
    w32 = float(np.float32(1.0) - np.float32(d))               # what an fp32 interface would make of it: 1 - (float)0.999999 is 1.3 % off
    as_float = ema_ratio(sel(e0), sel(p1), [oc.ema64(a, b, w32).float().double() for a, b in zip(sel(e0), sel(p1))], w)
    print(f"ema {layout} d={d}: worst |e' - e64| / (u |e64| + 2^-149) = {worst:.3f};  with w = 1 - (float)d it would be {as_float:.1f}")
    assert worst <= 1
    if d == 0.999999:
        assert as_float > 1                                     # the case is sensitive to w crossing as a float


def test_five_steps_two_groups_and_a_parameter_without_gradient_on_odd_steps():
    rig = Rig(_lengths(), "aligned16", seed=24)
    k = len(rig.params)
    lazy = 4                                                    # no gradient on odd steps
    groups = [(list(range(0, k, 2)), dict(HYP, lr=1e-3, weight_decay=1e-2)), (list(range(1, k, 2)), dict(HYP, lr=3e-2, weight_decay=0.1))]
    frozen = torch.nn.Parameter(torch.randn(33, device="cuda:0"), requires_grad=False)
    holder = torch.nn.Module()
    holder.list, holder.frozen = torch.nn.ParameterList(rig.params), frozen
    ema = optim.ModelEMA(holder, decay=0.999, tau=4)
    for i, (e, p) in enumerate(ema._pairs):
        e.data = rig.view("e", i)
    assert ema.module.frozen.data_ptr() == frozen.data_ptr()
    frozen_bits = frozen.detach().view(torch.int32).clone()
    opt = optim.AdamW([dict(params=[rig.params[i] for i in idx], **hyp) for idx, hyp in groups], max_grad_norm=1.0, ema=ema)
    rig.attach_state(opt)
    t = [T0] * k
    before = _counter("optim_launches")
    for step in range(5):
        none = (lazy,) if step % 2 else ()
        rig.set_grads(none=none)
        snap = rig.snapshot(t)
        opt.step()
        w = oc.ema_weight(0.999, 4, step + 1)
        got = rig.state64()
        want, norm64, _ = oc.step64(snap, groups, 1.0, decoupled=True, ema_w=w)
        ours = ratios(snap, want, got, groups, True)
        re = ema_ratio([s["e"].double() for s in snap], [g["p"] for g in got], [g["e"] for g in got], w)
        rn = norm_ratio(opt.last_grad_norm, norm64)
        # against the restatement's OWN p' the average carries the error of p' times w on top of its rounding
        worst_acc = 0.0
        for s, wnt, g in zip(snap, want, got):
            if wnt["p"].numel():
                slack = w * (g["p"] - wnt["p"]).abs()
                worst_acc = max(worst_acc, _ratio((g["e"] - wnt["e"]).abs(), U * wnt["e"].abs() + 2.0 ** -149 + slack * (1 + U)))
        print(f"adamw+ema step {step + 1}: m {ours['m']:.3f} v {ours['v']:.3f} p {ours['p']:.3f} norm {rn:.3f} e {re:.3f} e vs restatement {worst_acc:.3f}")
        assert ours["m"] <= 1 and ours["v"] <= 1 and ours["p"] <= 1 and rn <= 1 and re <= 1 and worst_acc <= 1
        assert rig.guards_intact()
        t = [x if i in none else x + 1 for i, x in enumerate(t)]
    # both groups differ in lr and decoupled decay alone: one norm launch and one update launch per step, one standalone launch on odd steps
    assert _counter("optim_launches") - before == 5 * 2 + 2
    assert ema.updates == 5 and float(opt.state[rig.params[lazy]]["step"]) == T0 + 3
    assert ema.module.frozen.data_ptr() == frozen.data_ptr() and torch.equal(frozen.detach().view(torch.int32), frozen_bits)


# ------------------------------------------------------------------------------------------------ case 4: the skip
@pytest.mark.parametrize("layout", ["aligned16", "aligned4"])
def test_a_nonfinite_norm_skips_the_step(layout):
    rig = Rig(_lengths(), layout, seed=25)
    groups = one_group(rig, weight_decay=1e-2)
    ema = rig.make_ema(0.99)
    opt = optim.AdamW(rig.params, max_grad_norm=1.0, skip_nonfinite=True, ema=ema, **groups[0][1])
    rig.attach_state(opt)
    assert opt.skipped_steps.dtype == torch.int32 and opt.skipped_steps.is_cuda and int(opt.skipped_steps) == 0
    for count, poison in ((1, float("inf")), (2, float("nan"))):
        rig.set_grads(poison=poison)
        bits = rig.bits()
        opt.step()
        assert same_bits(bits, rig.bits()), f"a step with a {poison} gradient wrote something"
        assert int(opt.skipped_steps) == count and not math.isfinite(float(opt.last_grad_norm))
    assert all(float(opt.state[p]["step"]) == T0 + 2 for p in rig.params)        # the host's counter counts calls
    # a finite step after the skips: the restatement with the advanced step
    rig.set_grads()
    snap = rig.snapshot([T0 + 2] * len(rig.n))
    opt.step()
    w = 1.0 - 0.99
    got = rig.state64()
    want, norm64, skipped = oc.step64(snap, groups, 1.0, decoupled=True, ema_w=w, skip_nonfinite=True)
    ours = ratios(snap, want, got, groups, True)
    re = ema_ratio([s["e"].double() for s in snap], [g["p"] for g in got], [g["e"] for g in got], w)
    print(f"adamw after two skips {layout}: m {ours['m']:.3f} v {ours['v']:.3f} p {ours['p']:.3f} e {re:.3f}")
    assert not skipped and int(opt.skipped_steps) == 2 and ema.updates == 3
    assert ours["m"] <= 1 and ours["v"] <= 1 and ours["p"] <= 1 and re <= 1 and norm_ratio(opt.last_grad_norm, norm64) <= 1
    assert rig.guards_intact()


def test_skip_without_clip_and_skip_switched_off():
    # no clip: the norm launch still runs, a finite step equals the plain unclipped one bit for bit
    a, b = Rig(_lengths(), seed=26), Rig(_lengths(), seed=26)
    hyp = dict(HYP, weight_decay=1e-2)
    counter = torch.zeros((), dtype=torch.int32, device="cuda:0")
    for rig in (a, b):
        rig.set_grads()
    norm = abi_step(a, hyp, decoupled=True, skip=True, counter=counter)
    abi_step(b, hyp, decoupled=True)
    g64 = torch.cat([a.view("g", i).double().cpu() for i in range(len(a.n))])
    assert same_bits(a.bits(), b.bits()) and int(counter) == 0 and norm_ratio(norm, float(g64.norm())) <= 1
    a.set_grads(poison=float("inf"))
    bits = a.bits()
    norm = abi_step(a, hyp, decoupled=True, skip=True, counter=counter, ema=list(range(len(a.n))), ema_w=0.5)
    assert same_bits(bits, a.bits()) and int(counter) == 1 and math.isinf(float(norm))
    # switched off: today's behaviour, the NaN coefficient reaches the weights
    rig = Rig(_lengths(), seed=26)
    opt = optim.AdamW(rig.params, max_grad_norm=1.0, weight_decay=1e-2, **HYP)
    rig.attach_state(opt)
    rig.set_grads(poison=float("nan"))
    opt.step()
    assert opt.skipped_steps is None and math.isnan(float(opt.last_grad_norm))
    assert all(bool(torch.isnan(rig.view("p", i)).all()) for i in range(len(rig.n)))
    assert rig.guards_intact()


def test_skip_with_groups_that_need_separate_calls():
    """groups that differ in betas share one norm through the standalone clip; every call reads it and skips"""
    rig = Rig(_lengths(), seed=27)
    k = len(rig.params)
    groups = [(list(range(0, k // 2)), dict(HYP, weight_decay=1e-2)), (list(range(k // 2, k)), dict(HYP, betas=(0.8, 0.99), weight_decay=1e-2))]
    opt = optim.AdamW([dict(params=[rig.params[i] for i in idx], **hyp) for idx, hyp in groups], skip_nonfinite=True)
    rig.attach_state(opt)
    rig.set_grads(poison=float("inf"))
    bits = rig.bits()
    opt.step()
    assert same_bits(bits, rig.bits()) and int(opt.skipped_steps) == 1 and math.isinf(float(opt.last_grad_norm))
    rig.set_grads()
    snap = rig.snapshot([T0 + 1] * k)
    opt.step()
    want, norm64, _ = oc.step64(snap, groups, None, decoupled=True)
    ours = ratios(snap, want, rig.state64(), groups, True)
    assert ours["m"] <= 1 and ours["v"] <= 1 and ours["p"] <= 1 and int(opt.skipped_steps) == 1
    assert norm_ratio(opt.last_grad_norm, norm64) <= 1 and rig.guards_intact()


# ------------------------------------------------------------------------------------------------ case 5: table boundary, determinism
def test_a_list_longer_than_one_table_twice():
    table = _counter("optim_table_tensors")
    res = []
    for _ in range(2):
        rig = Rig([5] * (table + 1), seed=28)
        ema = rig.make_ema(0.9)
        opt = optim.AdamW(rig.params, max_grad_norm=1.0, weight_decay=1e-2, ema=ema, **HYP)
        rig.attach_state(opt)
        rig.set_grads()
        start = rig.bits()
        before = _counter("optim_launches")
        opt.step()
        assert _counter("optim_launches") - before == 1 + 2
        now = rig.bits()
        for key in ("p", "m", "v", "e"):
            moved = (now[key] != start[key]).view(-1)
            assert all(bool(moved[rig.off[key] + s:rig.off[key] + s + 5].all()) for s in rig.start), key      # every tensor was updated
        assert rig.guards_intact()
        res.append(dict(now, norm=opt.last_grad_norm.view(torch.int32).reshape(1).clone()))
    assert same_bits(res[0], res[1], ("p", "m", "v", "e", "norm"))


# ------------------------------------------------------------------------------------------------ case 6: launches of the default model
def test_default_vitb_trainable_set_with_clip_adamw_and_fused_ema():
    from dinov2_od_amd import DINOv2ObjectDetector
    with torch.device("meta"):
        m = DINOv2ObjectDetector(pretrained=False, precision="bf16")
    named = [(n, p.shape) for n, p in m.named_parameters() if p.requires_grad]
    holder = torch.nn.Module()
    holder.list = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(tuple(s), device="cuda:0")) for _, s in named])
    params = list(holder.list)
    ema = optim.ModelEMA(holder)
    opt = optim.AdamW(params, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, ema=ema)
    for (n, _), p in zip(named, params):
        p.grad = None if n.startswith("decoder.reference_points.") else torch.ones_like(p)
    with_grad = sum(p.grad is not None for p in params)
    before = _counter("optim_launches")
    opt.step()
    torch.cuda.synchronize()
    used = _counter("optim_launches") - before
    ceil = lambda a, b: -(-a // b)
    norm_launches = ceil(with_grad, _counter("optim_norm_table_tensors"))
    # the parameters without a gradient take the standalone launch: still no more update launches than the whole set in tables
    assert used == norm_launches + ceil(with_grad, _counter("optim_table_tensors")) + ceil(len(params) - with_grad, _counter("optim_ema_table_tensors"))
    assert used <= norm_launches + ceil(len(params), _counter("optim_table_tensors"))
    total = sum(p.numel() for p in params if p.grad is not None)
    assert abs(float(opt.last_grad_norm) - total ** 0.5) <= 2 * float(np.spacing(np.float32(total ** 0.5)))
    assert all(bool((e != 0).all()) == (p.grad is not None) for e, p in ema._pairs)      # the shadows moved with their parameters


# ------------------------------------------------------------------------------------------------ case 7: version counters and the engines
def test_the_ema_module_and_the_live_model_forward_on_the_new_weights():
    from dinov2_od_amd import synth
    from tests import cases, gpu_util as G
    bb, dc = cases.micro_bb(), cases.dec_cfg(True)
    m = G.make_detector(bb, dc, "bf16")
    x = G.to_gpu(synth.make_pixels(2, 56, 70, seed=0))
    live0 = m.forward_packed(x).clone()                         # both engines now hold weights packed from the initial parameters
    ema = optim.ModelEMA(m, decay=0.5)                          # a deep copy of a module that owns an engine
    assert "_engine" in m.__dict__ and "_engine" not in ema.module.__dict__
    ema0 = ema.module.forward_packed(x).clone()
    assert torch.equal(live0, ema0)
    for n, p in m.named_parameters():
        assert (dict(ema.module.named_parameters())[n].data_ptr() == p.data_ptr()) == (not p.requires_grad), n
    params = [p for p in m.parameters() if p.requires_grad]
    opt = optim.AdamW(params, lr=1e-2, weight_decay=1e-2, max_grad_norm=1.0, ema=ema)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda:0", generator=gen)
    versions = [e._version for e, _ in ema._pairs]
    opt.step()
    assert all(e._version > v for (e, _), v in zip(ema._pairs, versions))
    out = ema.module.forward_packed(x).clone()
    fresh = G.make_detector(bb, dc, "bf16")
    fresh.load_state_dict(ema.module.state_dict())
    assert torch.equal(out, fresh.eval().forward_packed(x)), "the average's forward ran on stale packed weights"
    assert not torch.equal(out, ema0)
    live = m.forward_packed(x).clone()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(live, fresh.eval().forward_packed(x)), "the live model's forward ran on stale packed weights"
    assert not torch.equal(live, live0) and not torch.equal(live, out)
