"""The native optimizer step (dinov2_od_amd.optim over csrc/optim.hip) against the same update in float64.

The arbiter is torch.optim.Adam + torch.nn.utils.clip_grad_norm_ on float64 CPU copies of the state the native step starts from;
PyTorch's own fp32 step on the GPU, from the same state, is measured against the same bounds as a yardstick (printed, not
asserted).  With u = 2^-24, g the clipped-and-decayed gradient, D64 the float64 update and den64 its denominator:
    |m' - m64| <= 4u (|m| + |g|)
    |v' - v64| <= 6u v64 + 2^-149
    |p' - p64| <= u |p64| + 8u |D64| + step_size 4u (|m| + |g|) / den64
    |norm - norm64| <= 2 ulp_fp32(norm64)
    clip_grad_norm_ alone: |g' - g64| <= 2u |g64|
These are worst cases of the roundings involved (DESIGN.md section 6b derives them), not measurements; none had to be widened.
Shapes are the smallest at which the kernels branch: lengths around the 4-wide vector, the 256-thread row and the 4096-element
chunk, a list one longer than an argument table, 4-byte aligned carves (the scalar path).  Every tensor is carved out of a flat
buffer with sentinel gaps that must keep their bits."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import optim

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = 1234.5
HYP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


def _counter(name):
    return nat.lib().dod_test_counter(name.encode())


def _lengths():
    c = _counter("optim_chunk_elems")
    return [1, 3, 4, 5, 255, 256, 257, c - 1, c, c + 1, 2 * c + 1]


class Rig:
    """parameters, gradients and both moments carved out of one flat device buffer each, sentinel gaps between the tensors"""

    def __init__(self, lengths, offset=0, seed=0, carve_state=True):
        self.n = list(lengths)
        self.start, at = [], offset
        for n in self.n:
            self.start.append(at)
            at += n + 4 + (-n) % 4          # a gap of 4..7 elements; every start keeps the carve's alignment (offset mod 4)
        self.size = at + 4
        d = torch.device("cuda:0")
        self.flat = {k: torch.full((self.size,), SENT, device=d) for k in ("p", "g", "m", "v")}
        self.gap = torch.ones(self.size, dtype=torch.bool, device=d)
        for s, n in zip(self.start, self.n):
            self.gap[s:s + n] = False
        self.gen = torch.Generator().manual_seed(seed)
        self.params = []
        for i, (s, n) in enumerate(zip(self.start, self.n)):
            self.view("p", i).copy_(torch.randn(n, generator=self.gen))
            self.params.append(torch.nn.Parameter(self.view("p", i)))
        self.carve_state = carve_state
        self.no_state = set()                 # parameters that start without optimizer state

    def view(self, k, i):
        return self.flat[k][self.start[i]:self.start[i] + self.n[i]]

    def attach_state(self, opt):
        """zero moments inside the flat buffers, step 0: what load_state_dict of a fresh checkpoint leaves"""
        if not self.carve_state:
            return
        for i, p in enumerate(self.params):
            if i in self.no_state:
                continue
            self.view("m", i).zero_()
            self.view("v", i).zero_()
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": self.view("m", i), "exp_avg_sq": self.view("v", i)}

    def set_grads(self, scale=3.0, none=(), fn=None):
        for i, p in enumerate(self.params):
            if i in none:
                p.grad = None
                continue
            g = scale * torch.randn(self.n[i], generator=self.gen)
            if fn is not None:
                g = fn(i, g)
            self.view("g", i).copy_(g)
            p.grad = self.view("g", i)

    def gaps_intact(self, keys=("p", "g", "m", "v")):
        want = torch.tensor(SENT).view(torch.int32).item()
        return all(bool((self.flat[k].view(torch.int32)[self.gap] == want).all()) for k in keys)

    def snapshot(self, opt):
        """the state a step starts from, on the host: per parameter p, g (or None), m, v (or None before the first step), t"""
        out = []
        for p in self.params:
            st = opt.state.get(p) or {}
            out.append(dict(p=p.detach().cpu().clone(), g=None if p.grad is None else p.grad.detach().cpu().clone(),
                            m=st["exp_avg"].cpu().clone() if st else None, v=st["exp_avg_sq"].cpu().clone() if st else None,
                            t=float(st["step"]) if st else 0.0))
        return out


def torch_step(snap, groups, max_norm, dtype, device):
    """PyTorch's clip + Adam from `snap` in the given precision -> per parameter p', m', v', clipped g, t; and the norm"""
    ps = [torch.nn.Parameter(e["p"].to(device=device, dtype=dtype)) for e in snap]
    opt = torch.optim.Adam([dict(params=[ps[i] for i in idx], **hyp) for idx, hyp in groups])
    for p, e in zip(ps, snap):
        if e["m"] is not None:
            opt.state[p] = {"step": torch.tensor(e["t"]), "exp_avg": e["m"].to(device=device, dtype=dtype),
                            "exp_avg_sq": e["v"].to(device=device, dtype=dtype)}
        p.grad = None if e["g"] is None else e["g"].to(device=device, dtype=dtype)
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm is not None else None
    clipped = [None if p.grad is None else p.grad.detach().double().cpu().clone() for p in ps]
    opt.step()
    out = []
    for p, g in zip(ps, clipped):
        st = opt.state.get(p) or {}
        out.append(dict(p=p.detach().double().cpu(), g=g, m=st["exp_avg"].double().cpu() if st else None,
                        v=st["exp_avg_sq"].double().cpu() if st else None, t=float(st["step"]) if st else 0.0))
    return out, None if norm is None else norm.double().cpu()


def _ratio(err, bound):
    """worst err / bound; an element whose bound is 0 must be exact"""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0


def ratios(snap, want, got, groups, g_stored=False):
    """worst ratio to each of the three bounds of `got` (per parameter p, m, v as float64 host tensors) against the arbiter.
    g_stored: the clipped gradient went through an fp32 store before the update (groups that differ in more than lr: the standalone
    clip, then one update per group), so g carries u |coef g_raw| of absolute error -- more than u |g| where the clipped gradient and
    the decay cancel.  Its first-order effect joins the bounds: (1 - beta1) dg on m, (1 - beta2)(2 |g| dg + dg^2) on v."""
    hyp_of = {i: hyp for idx, hyp in groups for i in idx}
    worst = dict(m=0.0, v=0.0, p=0.0)
    for i, (e, w, g) in enumerate(zip(snap, want, got)):
        if e["g"] is None:
            for k in ("p", "m", "v"):      # PyTorch's rule: no gradient, nothing moves
                assert (g[k] is None and w[k] is None) or torch.equal(g[k], e[k].double()), (i, k)
            assert g["t"] == e["t"]
            continue
        hyp = hyp_of[i]
        b1, b2 = hyp["betas"]
        t = w["t"]
        assert g["t"] == t, (i, g["t"], t)
        m0 = e["m"].double() if e["m"] is not None else torch.zeros_like(w["p"])
        gd = w["g"] + hyp.get("weight_decay", 0.0) * e["p"].double()          # clipped and decayed
        step_size, bc2_sqrt = hyp["lr"] / (1 - b1 ** t), (1 - b2 ** t) ** 0.5
        den = w["v"].sqrt() / bc2_sqrt + hyp["eps"]
        delta = step_size * w["m"] / den
        bm = 4 * U * (m0.abs() + gd.abs())
        bv = 6 * U * w["v"] + 2.0 ** -149
        if g_stored:
            dg = U * w["g"].abs()
            bm = bm + (1 - b1) * dg
            bv = bv + (1 - b2) * (2 * gd.abs() * dg + dg * dg)
        worst["m"] = max(worst["m"], _ratio((g["m"] - w["m"]).abs(), bm))
        worst["v"] = max(worst["v"], _ratio((g["v"] - w["v"]).abs(), bv))
        worst["p"] = max(worst["p"], _ratio((g["p"] - w["p"]).abs(), U * w["p"].abs() + 8 * U * delta.abs() + step_size * bm / den))
    return worst


def norm_ratio(got, want64):
    ulp = float(np.spacing(np.float32(want64)))
    return abs(float(got) - float(want64)) / (2 * ulp)


def native_state(rig, opt):
    out = []
    for p in rig.params:
        st = opt.state.get(p) or {}
        out.append(dict(p=p.detach().double().cpu(), m=st["exp_avg"].double().cpu() if st else None,
                        v=st["exp_avg_sq"].double().cpu() if st else None, t=float(st["step"]) if st else 0.0))
    return out


def run(rig, groups, max_norm, steps=1, grads=None, label=""):
    """`steps` native steps; every one is checked against float64 from the native state it started from.  Returns the optimizer."""
    opt = optim.Adam([dict(params=[rig.params[i] for i in idx], **hyp) for idx, hyp in groups], max_grad_norm=max_norm)
    rig.attach_state(opt)
    g_stored = max_norm is not None and len({(h["betas"], h["eps"], h.get("weight_decay", 0.0)) for _, h in groups}) > 1
    for step in range(steps):
        (grads or (lambda s: rig.set_grads()))(step)
        snap = rig.snapshot(opt)
        opt.step()
        got = native_state(rig, opt)
        want, norm64 = torch_step(snap, groups, max_norm, torch.float64, "cpu")
        ref32, norm32 = torch_step(snap, groups, max_norm, torch.float32, "cuda:0")
        ours, theirs = ratios(snap, want, got, groups, g_stored), ratios(snap, want, ref32, groups, g_stored)
        line = f"optim {label} step {step + 1}: worst ratio to the bound, native / PyTorch fp32:  " + \
            "  ".join(f"{k} {ours[k]:.3f} / {theirs[k]:.3f}" for k in ("m", "v", "p"))
        if max_norm is not None:
            rn, rn32 = norm_ratio(opt.last_grad_norm, norm64), norm_ratio(norm32, norm64)
            line += f"  norm {rn:.3f} / {rn32:.3f}"
        print(line)
        assert rig.gaps_intact(), "a sentinel between two tensors changed"
        assert ours["m"] <= 1 and ours["v"] <= 1 and ours["p"] <= 1, line
        if max_norm is not None:
            assert rn <= 1, line
    return opt


def one_group(rig, **hyp):
    return [(list(range(len(rig.params))), dict(HYP, **hyp))]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_step_against_float64(offset, weight_decay, max_norm):
    rig = Rig(_lengths(), offset=offset, seed=1)
    mid = len(rig.params) // 2                # a None gradient in the middle of the list, on every step
    late = 2                                  # a parameter whose first gradient arrives at step 2: its t stays one behind
    rig.no_state = {mid}

    def grads(step):
        rig.set_grads(none=(mid, late) if step == 0 else (mid,))
    opt = run(rig, one_group(rig, weight_decay=weight_decay), max_norm, steps=2, grads=grads,
              label=f"off{offset} wd{weight_decay:g} clip{max_norm}")
    assert rig.params[mid] not in opt.state                                   # no state is created for it
    assert float(opt.state[rig.params[late]]["step"]) == 1 and float(opt.state[rig.params[0]]["step"]) == 2
    if max_norm is not None:
        assert float(opt.last_grad_norm) > max_norm                           # the clip was active


def test_five_steps_and_two_groups_with_their_own_lr():
    rig = Rig(_lengths(), seed=2)
    k = len(rig.params)
    groups = [(list(range(0, k, 2)), dict(HYP, lr=1e-3, weight_decay=1e-4)), (list(range(1, k, 2)), dict(HYP, lr=3e-2, weight_decay=1e-4))]
    before = _counter("optim_launches")
    run(rig, groups, 1.0, steps=5, label="two lr")
    assert _counter("optim_launches") - before == 5 * 2                       # groups that differ in lr alone share both launches


def test_groups_with_different_decay_share_one_norm():
    rig = Rig(_lengths(), seed=3)
    k = len(rig.params)
    groups = [(list(range(0, k // 2)), dict(HYP, weight_decay=0.0)), (list(range(k // 2, k)), dict(HYP, betas=(0.8, 0.99), weight_decay=1e-2))]
    run(rig, groups, 1.0, steps=2, label="two decays")


def test_list_longer_than_one_argument_table():
    table = _counter("optim_table_tensors")
    rig = Rig([1 + i % 7 for i in range(table + 1)] + [300] * (_counter("optim_norm_table_tensors") - table), seed=4, carve_state=False)
    before = _counter("optim_launches")
    run(rig, one_group(rig, weight_decay=1e-4), 1.0, steps=2, label="long list")       # lazily created state, as a fresh optimizer has
    assert rig.gaps_intact(("p", "g"))
    assert _counter("optim_launches") - before == 2 * (2 + 3)                 # one table more than fits, for the norm and for the update


def test_huge_max_norm_equals_the_unclipped_step_bit_for_bit():
    res = []
    for max_norm in (None, 1e9):
        rig = Rig(_lengths(), seed=5)
        opt = run(rig, one_group(rig, weight_decay=1e-4), max_norm, steps=2, label=f"clip{max_norm}")
        res.append({k: rig.flat[k].clone() for k in ("p", "m", "v")})
        if max_norm:
            assert 1.0 < float(opt.last_grad_norm) < 1e9
    for k in ("p", "m", "v"):
        assert torch.equal(res[0][k].view(torch.int32), res[1][k].view(torch.int32)), k


def test_same_inputs_twice_give_the_same_bits():
    res = []
    for _ in range(2):
        rig = Rig(_lengths(), seed=6)
        opt = run(rig, one_group(rig, weight_decay=1e-4), 1.0, steps=2, label="repeat")
        res.append({**{k: rig.flat[k].clone() for k in ("p", "m", "v")}, "norm": opt.last_grad_norm.clone().reshape(1)})
    for k in res[0]:
        assert torch.equal(res[0][k].view(torch.int32), res[1][k].view(torch.int32)), k


@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
def test_all_zero_gradients(weight_decay):
    rig = Rig(_lengths(), seed=7)
    p0 = rig.flat["p"].clone()
    opt = run(rig, one_group(rig, weight_decay=weight_decay), 1.0, grads=lambda s: rig.set_grads(scale=0.0), label=f"zero grads wd{weight_decay:g}")
    assert float(opt.last_grad_norm) == 0.0
    moved = not torch.equal(rig.flat["p"], p0)
    assert moved == (weight_decay != 0.0)                                     # parameters move by the decay alone


def test_infinite_gradient():
    rig = Rig(_lengths(), seed=8)
    opt = optim.Adam(rig.params, weight_decay=1e-4, max_grad_norm=1.0, **HYP)
    rig.attach_state(opt)

    def poison(i, g):
        if i == 5:
            g[g.numel() // 2] = float("inf")
        return g
    rig.set_grads(fn=poison)
    snap = rig.snapshot(opt)
    opt.step()
    _, norm32 = torch_step(snap, one_group(rig, weight_decay=1e-4), 1.0, torch.float32, "cuda:0")
    assert bool(torch.isfinite(opt.last_grad_norm)) == bool(torch.isfinite(norm32)) and not bool(torch.isfinite(norm32))
    assert rig.gaps_intact()


def test_clip_grad_norm_alone():
    for offset in (0, 1):
        rig = Rig(_lengths(), offset=offset, seed=9)
        rig.set_grads(none=(4,))
        g64 = [None if p.grad is None else p.grad.double().cpu() for p in rig.params]
        norm64 = torch.sqrt(sum((g * g).sum() for g in g64 if g is not None))
        versions = [p.grad._version for p in rig.params if p.grad is not None]
        # below max_norm: nothing is written
        g0 = rig.flat["g"].clone()
        norm = optim.clip_grad_norm_(rig.params, 2.0 * float(norm64))
        assert norm.dim() == 0 and norm.is_cuda and norm.dtype == torch.float32
        assert norm_ratio(norm, norm64) <= 1
        assert torch.equal(rig.flat["g"].view(torch.int32), g0.view(torch.int32))
        # above: scaled to within 2u of float64
        norm = optim.clip_grad_norm_(rig.params, 1.0)
        coef = 1.0 / (float(norm64) + 1e-6)
        worst = 0.0
        for p, g in zip(rig.params, g64):
            if g is not None:
                worst = max(worst, _ratio((p.grad.double().cpu() - coef * g).abs(), 2 * U * (coef * g).abs()))
        ref = [torch.nn.Parameter(p.detach().clone()) for p in rig.params]
        for r, g in zip(ref, g64):
            r.grad = None if g is None else g.float().cuda()
        norm32 = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        theirs = max(_ratio((r.grad.double().cpu() - coef * g).abs(), 2 * U * (coef * g).abs()) for r, g in zip(ref, g64) if g is not None)
        print(f"clip_grad_norm_ off{offset}: worst ratio to 2u, native / PyTorch fp32: {worst:.3f} / {theirs:.3f};  norm "
              f"{norm_ratio(norm, norm64):.3f} / {norm_ratio(norm32, norm64):.3f}")
        assert worst <= 1 and norm_ratio(norm, norm64) <= 1
        assert rig.gaps_intact(("p", "g"))
        assert all(p.grad._version > v for p, v in zip([p for p in rig.params if p.grad is not None], versions))
    # PyTorch's other norms are PyTorch's
    rig.set_grads()
    want = max(float(p.grad.abs().max()) for p in rig.params)
    assert float(optim.clip_grad_norm_(rig.params, 1e9, norm_type=float("inf"))) == want


def test_native_step_bumps_the_version_counters():
    rig = Rig([5, 300], seed=10)
    opt = optim.Adam(rig.params, max_grad_norm=1.0, **HYP)
    rig.set_grads()
    before = [p._version for p in rig.params]
    opt.step()
    assert all(p._version > v for p, v in zip(rig.params, before))


def test_default_vitb_trainable_set_takes_at_most_four_launches():
    from dinov2_od_amd import DINOv2ObjectDetector
    with torch.device("meta"):
        m = DINOv2ObjectDetector(pretrained=False, precision="bf16")      # the reference's defaults: ViT-B/14, r = 2, 1 decoder layer
    named = [(n, p.shape) for n, p in m.named_parameters() if p.requires_grad]
    assert len(named) == 57
    params = [torch.nn.Parameter(torch.zeros(tuple(s), device="cuda:0")) for _, s in named]
    opt = optim.Adam(params, lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0)
    for (n, _), p in zip(named, params):
        p.grad = None if n.startswith("decoder.reference_points.") else torch.ones_like(p)      # the unused pair never gets a gradient
    before = _counter("optim_launches")
    opt.step()
    torch.cuda.synchronize()
    used = _counter("optim_launches") - before
    assert 2 <= used <= 4, used
    total = sum(p.numel() for p in params if p.grad is not None)
    assert abs(float(opt.last_grad_norm) - total ** 0.5) <= 2 * float(np.spacing(np.float32(total ** 0.5)))
