"""The fixed-reference softmax of the bf16 flash attention (csrc/attn_bf16.hip), as far as a CPU can show it.  No GPU.

The kernel takes a row's softmax reference from key tile 0 alone (the scaled maximum m0 of keys 0..63) and runs every later tile as
p = exp2(fma(s, c, -m0)), l += sum p, without a running maximum.  A row whose normaliser is not below 2^60, or that holds an accumulator
which is not finite, is computed again with the running maximum.  `emu_fixed_ref` is that, next to attention_cases.emu_bf16's conventions:
fp32 scores, the reference from tile 0, one rounding of the exp2 argument to fp32 (the FMA), fp32 exp2, P rounded to bf16 before P V (the
normaliser sums the unrounded P), the rerun rows taken from attention_cases.emu_bf16, the context rounded to bf16; float64 elsewhere.
It is held to attention_cases.bf16_bound against float64 on the `normal` input, every SOFTMAX_KINDS input and the `mixed` input below.

`mixed` (also the input of tests/test_gpu_attention_ref.py): the `normal` input with one key per spike in a LATER tile set to a u, u = ones(64) / 8,
a = 96.  Query rows r % 4 == 0 get +8 u: their spike score is about a nats above everything else, exp2 overflows, they must rerun.  Rows
r % 4 == 1 get -8 u: about -a, p = 0.  The other rows score a / 64 * sum(q) there, a spread of about +-18 nats: a few of them pass the
threshold, most do not.  `classify` sorts every (image, head, row) by its float64 normaliser relative to the tile-0 maximum: >= 2^61 must
rerun, <= 2^59 must not, in between undecided -- the kernel sums l in fp32 and in another order, one bit either way is far more than
its error.  At most 5 % of the rows may be undecided: a condition on the chosen input, asserted here.

`rising` below N = 201: attention_cases.make_input writes keys 140 and 200, so `make_kind` repeats its recipe on the `normal` seed with the spikes
that fit, keys 64 / 70 / 128 at a = 24 / 40 / 56.  At N = 129 most rows pass 2^60 (asserted: the case must keep exercising the rerun); at N = 65
only key 64 at 24 nats is left, which does not reach 2^60 (41.6 nats): that case shows a reference outgrown WITHOUT a rerun.

`vbig` pins the other half of the check, the accumulator that is not finite: every q gets +8 u, key 70 is 24 u -- about 24 nats, l stays below
2^59 for every row -- and its value row is 2^110 in every column, so p v passes fp32's range for the rows with p >= 2^18 while their normaliser
does not ask for a rerun.  `classify_finite`: p_70 2^110 >= 2^128.5 must rerun, sum_k p_k |v_k| <= 2^127.5 must not -- half a bit either side of fp32's range, against the
2^-9 of P's rounding to bf16 and the 1e-5 of exp2."""
import functools

import numpy as np
import pytest
import torch

from tests import attention_cases as ac

REF_LMAX = 2.0 ** 60             # csrc/attn_bf16.hip AT_REF_LMAX
SPIKE_A = 96.0
UNDECIDED_CAP = 0.05
VBIG_KEY, VBIG_V = 70, 2.0 ** 110
# N -> the spike keys of `mixed`: the one-key half-width tail tile; a full-width tail tile; two reference tiles and a one-key tail; behind the
# ring's wrap; tile 1 and the 26-key tail tile of the fused launch
SPIKES = {1: (), 64: (), 65: (64,), 97: (96,), 129: (70,), 257: (200,), 300: (200,), 346: (100, 330)}
SHAPES = [(2, 300, 2), (2, 129, 1), (2, 65, 1)]
KINDS = ["normal"] + ac.SOFTMAX_KINDS + ["mixed"]


def make_mixed(B, N, heads):
    """fp32 [n_unique(B), N, 3 * heads * 64]"""
    x = ac.make_input(B, N, heads, "normal").numpy().copy()
    D = heads * 64
    u = np.ones(64, dtype=np.float32) / 8.0
    if SPIKES[N]:
        x[:, 0::4, :D] += np.tile(8.0 * u, heads)
        x[:, 1::4, :D] -= np.tile(8.0 * u, heads)
    for key in SPIKES[N]:
        assert 64 <= key < N                 # behind tile 0
        x[:, key, D:2 * D] = np.tile(SPIKE_A * u, heads)
    return torch.from_numpy(x)


def make_kind(B, N, heads, kind):
    if kind == "mixed":
        return make_mixed(B, N, heads)
    if kind == "vbig":
        x = ac.make_input(B, N, heads, "normal").numpy().copy()
        D = heads * 64
        u = np.ones(64, dtype=np.float32) / 8.0
        x[:, :, :D] += np.tile(8.0 * u, heads)
        x[:, VBIG_KEY, D:2 * D] = np.tile(24.0 * u, heads)
        x[:, VBIG_KEY, 2 * D:] = VBIG_V
        return torch.from_numpy(x)
    if kind == "rising" and N <= 200:        # attention_cases' recipe with the spikes that fit (module docstring)
        x = ac.make_input(B, N, heads, "normal").numpy().copy()
        D = heads * 64
        u = np.ones(64, dtype=np.float32) / 8.0
        x[:, :, :D] += np.tile(8.0 * u, heads)
        for key, a in ((64, 24.0), (70, 40.0), (128, 56.0)):
            if key < N:
                x[:, key, D:2 * D] = np.tile(a * u, heads)
        return torch.from_numpy(x)
    return ac.make_input(B, N, heads, kind)


def _qkv(vals, heads):
    D = vals.shape[-1] // 3
    return [ac.heads_view(t.double(), heads) for t in (vals[..., :D], vals[..., D:2 * D], vals[..., 2 * D:])]


def classify(vals_bf16, heads, scale=ac.SCALE):
    """-> (must rerun, must not rerun) bool [n, heads, N] from the float64 normaliser sum_k exp(s_k - max over tile 0)"""
    q, k, _ = _qkv(vals_bf16, heads)
    s = q @ k.transpose(-1, -2) * scale
    l = torch.exp(s - s[..., :64].amax(-1, keepdim=True)).sum(-1)
    return l >= 2.0 * REF_LMAX, l <= 0.5 * REF_LMAX


def later_maximum(vals_bf16, heads, margin=1.0, scale=ac.SCALE):
    """-> bool [n, heads, N]: the row's maximum lies behind key tile 0 by more than `margin` nats, so the two softmax forms round P differently"""
    q, k, _ = _qkv(vals_bf16, heads)
    s = q @ k.transpose(-1, -2) * scale
    if s.shape[-1] <= 64:
        return torch.zeros(s.shape[:-1], dtype=torch.bool)
    return s[..., 64:].amax(-1) > s[..., :64].amax(-1) + margin


def classify_finite(vals_bf16, heads, scale=ac.SCALE):
    """`vbig`: -> (must rerun, must not rerun) bool [n, heads, N] by whether an fp32 accumulator of the fixed-reference pass leaves fp32's range;
    asserts that no row's normaliser comes near the threshold, so that the finite test alone decides"""
    q, k, v = _qkv(vals_bf16, heads)
    s = q @ k.transpose(-1, -2) * scale
    p = torch.exp(s - s[..., :64].amax(-1, keepdim=True))
    assert bool((p.sum(-1) <= 0.5 * REF_LMAX).all())
    return p[..., VBIG_KEY] * VBIG_V >= 2.0 ** 128.5, (p @ v.abs()).amax(-1) <= 2.0 ** 127.5


def emu_fixed_ref(vals_bf16, heads, scale=ac.SCALE):
    """-> (context [n, N, D] float64, rerun [n, heads, N] bool as the emulation's own fp32 normaliser decides it)"""
    q, k, v = _qkv(vals_bf16, heads)
    c = float(np.float32(scale * ac.LOG2E))
    s = (q @ k.transpose(-1, -2)).float()                                        # fp32 scores (the MFMA accumulator)
    m0 = (s[..., :64].amax(-1, keepdim=True) * np.float32(c)).float()            # mx * c in fp32
    arg = (s.double() * c - m0.double()).float()                                 # fma(s, c, -m0): one rounding
    p = torch.exp2(arg)                                                          # fp32; inf above 2^128
    l = p.sum(-1, dtype=torch.float32)
    o = ac.bf(p).double() @ v
    rerun = ~(l < REF_LMAX) | ~torch.isfinite(o.float()).all(-1)                 # the accumulators are fp32
    fast = ac.unheads(o / l.double()[..., None])
    slow = ac.emu_bf16(vals_bf16, heads, scale)
    sel = ac.unheads(rerun[..., None].expand(-1, -1, -1, 64))
    return torch.where(sel, slow, ac.bf(torch.nan_to_num(fast)).double()), rerun


@functools.lru_cache(maxsize=None)
def case(B, N, heads, kind):
    """-> (bf16-valued fp32 input, want, T, must rerun, must not rerun): computed once, shared with the GPU test, never written to"""
    x = ac.bf(make_kind(B, N, heads, kind))
    want, T = ac.ref64_qkv(x.double(), heads)
    must, must_not = classify_finite(x, heads) if kind == "vbig" else classify(x, heads)
    return x, want, T, must, must_not


@pytest.mark.parametrize("B,N,heads", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_fixed_reference_emulation_holds_the_bf16_bound(B, N, heads, kind):
    x, want, T, must, must_not = case(B, N, heads, kind)
    emu, rerun = emu_fixed_ref(x, heads)
    bound = ac.bf16_bound(want, T)
    ratio = float(((emu - want).abs() / bound.clamp(min=1e-300)).max())
    share = float(rerun.double().mean())
    print(f"fixed-reference emulation {B, N, heads, kind}: {ratio:.2f} of the bound, {share:.3f} of the rows rerun")
    assert bool(((emu - want).abs() <= bound).all()), ratio
    # the emulation's own decision agrees with the float64 classification wherever that decides
    assert bool(rerun[must].all()) and not bool(rerun[must_not].any())
    if kind in ("normal", "tile0"):
        assert share == 0.0
    if kind == "rising" and N >= 129:
        assert share > 0.5, "`rising` must keep exercising the rerun"
    if kind == "mixed":
        assert 0.0 < share < 1.0, "the rerun set of `mixed` must be neither empty nor everything"
        assert bool(must[:, :, 0::4].all()), "every +8 u row overflows"
        assert bool(must_not[:, :, 1::4].all()), "every -8 u row stays put"


@pytest.mark.parametrize("B,N,heads", SHAPES + [(2, 97, 1), (2, 257, 1), (64, 346, 8), (2, 346, 8)])
def test_mixed_leaves_few_rows_undecided(B, N, heads):
    _, _, _, must, must_not = case(B, N, heads, "mixed")
    undecided = float((~must & ~must_not).double().mean())
    print(f"mixed {B, N, heads}: {float(must.double().mean()):.3f} must rerun, {undecided:.4f} undecided")
    assert undecided <= UNDECIDED_CAP
    assert bool(must.any()) and bool(must_not.any())


def test_vbig_reruns_by_the_finite_test_alone():
    B, N, heads = 2, 129, 1
    x, want, T, must, must_not = case(B, N, heads, "vbig")
    emu, rerun = emu_fixed_ref(x, heads)
    undecided = float((~must & ~must_not).double().mean())
    print(f"vbig {B, N, heads}: {float(must.double().mean()):.3f} must rerun, {float(must_not.double().mean()):.3f} must not, {undecided:.3f} undecided")
    assert bool(must.any()) and bool(must_not.any()) and undecided <= UNDECIDED_CAP
    assert bool(rerun[must].all()) and not bool(rerun[must_not].any())
    assert bool(((emu - want).abs() <= ac.bf16_bound(want, T)).all())


def test_without_a_rerun_the_overflowing_rows_break_the_bound():
    """the rerun is what keeps `mixed` inside the bound: the fast pass alone leaves its +8 u rows non-finite"""
    x, want, T, must, _ = case(2, 129, 1, "mixed")
    q, k, v = _qkv(x, 1)
    s = (q @ k.transpose(-1, -2)).float()
    c = np.float32(ac.SCALE * ac.LOG2E)
    p = torch.exp2((s.double() * float(c) - (s[..., :64].amax(-1, keepdim=True) * c).double()).float())
    fast = ac.unheads((ac.bf(p).double() @ v) / p.sum(-1, dtype=torch.float32).double()[..., None])
    assert not bool(torch.isfinite(fast)[ac.unheads(must[..., None].expand(-1, -1, -1, 64))].all())
