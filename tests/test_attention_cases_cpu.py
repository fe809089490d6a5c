"""What tests/test_gpu_attention.py relies on and a CPU can show: the inputs are what their names say, the bf16 bound passes an
emulation that rounds where the kernel rounds, a single mis-weighted key breaks it, and the float64 reference alone leaves at most
15 % of the block-scale bytes undecided on every input the block-scaled test uses.  No GPU."""
import numpy as np
import pytest
import torch

from tests import attention_cases as ac


def _qkv_heads(x, heads):
    D = x.shape[-1] // 3
    return [ac.heads_view(t.double(), heads) for t in (x[..., :D], x[..., D:2 * D], x[..., 2 * D:])]


def test_softmax_inputs_are_what_they_claim():
    sc = {}
    for kind in ac.SOFTMAX_KINDS:
        x = ac.bf(ac.make_input(2, 300, 1, kind))            # as the bf16 kernels see them (the x3 kernels see the fp32 values: same structure)
        q, k, _ = _qkv_heads(x, 1)
        sc[kind] = (q @ k.transpose(-1, -2) * ac.SCALE)[:, 0]          # [image, query, key]
    tile_max = lambda s: torch.stack([s[..., 64 * t:64 * t + 64].amax(-1) for t in range(5)], -1)      # [image, query, tile]
    # rising: nearly every row sees a new maximum in tile 1, again in tile 2 and again in tile 3 (three rescales with alpha < 1)
    run = torch.cummax(tile_max(sc["rising"]), -1).values
    rises = (run[..., 1:4] > run[..., 0:3] + 1.0).all(-1)
    assert float(rises.double().mean()) > 0.9, float(rises.double().mean())
    # tile0: every row's maximum is key 5, by a margin: every later alpha is exactly 1
    s = sc["tile0"]
    assert bool((s.argmax(-1) == 5).all())
    assert float((s[..., 5] - torch.cat([s[..., :5], s[..., 6:]], -1).amax(-1)).min()) > 4.0
    # equal: every third row's scores are one number (exact: one product per score), not the same number for every row
    s = sc["equal"][:, ::3]
    assert bool((s == s[..., :1]).all()) and float(s[..., 0].std()) > 1.0
    # pm60: every row has scores near +60 and near -60
    s = sc["pm60"]
    assert 40.0 < float(s.amax(-1).min()) and float(s.amax(-1).max()) < 90.0
    assert -90.0 < float(s.amin(-1).min()) and float(s.amin(-1).max()) < -40.0


@pytest.mark.parametrize("B,N,heads,kind", [(2, 300, 2, "normal"), (1, 17, 2, "normal"), (3, 65, 1, "normal"), (1, 1370, 2, "normal"),
                                            (2, 300, 1, "rising"), (2, 300, 1, "pm60")])
def test_bf16_bound_passes_the_emulation_and_rejects_a_misweighted_key(B, N, heads, kind):
    x = ac.bf(ac.make_input(B, N, heads, kind))
    want, T = ac.ref64_qkv(x.double(), heads)
    bound = ac.bf16_bound(want, T)
    emu = ac.emu_bf16(x, heads)
    ratio = float(((emu - want).abs() / bound.clamp(min=1e-300)).max())
    print(f"bf16 emulation {B, N, heads, kind}: {ac.dist_by_T(emu, want, T):.2e} T, {ratio:.2f} of the bound")
    assert ratio < 0.75                          # RNE rounds within HALF an ulp, the bound allows a whole one at both points
    if N >= 17 and kind == "normal":             # key 3 weighted 1.25 x: the context moves by p_3 v_3 / 4
        q, k, v = _qkv_heads(x, heads)
        p = torch.softmax(q @ k.transpose(-1, -2) * ac.SCALE, -1)
        p[..., 3] *= 1.25
        bad = ac.unheads(p @ v)
        assert not bool(((bad - want).abs() <= bound).all())


@pytest.mark.parametrize("B,N,heads,kind", ac.mx_cases())
def test_mx_scale_bytes_are_decided_by_the_reference(B, N, heads, kind):
    """the float64 reference and the value margin alone fix at least 85 % of the block-scale bytes of every input"""
    x = ac.bf(ac.make_input(B, N, heads, kind))
    want, T = ac.ref64_qkv(x.double(), heads)
    D = heads * 64
    lo, hi = ac.mx_byte_range(want.reshape(-1, D), T.reshape(-1, D))
    assert bool((hi >= lo).all()) and bool((hi - lo <= 1).all())
    share = float((lo != hi).double().mean())
    print(f"mx {B, N, heads, kind}: {share:.3f} of the blocks undecided")
    assert share <= ac.MX_UNDECIDED_CAP


def test_e4m3_half_ulp_and_table():
    t = ac.E4M3_LUT
    assert torch.isnan(t[0x7F]) and torch.isnan(t[0xFF]) and float(t[0x7E]) == 448.0 and float(t[0x01]) == 2.0 ** -9
    fin = t[:0x7F]
    gaps = fin[1:] - fin[:-1]
    mid = 0.5 * (fin[1:] + fin[:-1])
    assert torch.equal(ac.e4m3_half_ulp(mid), 0.5 * gaps)
