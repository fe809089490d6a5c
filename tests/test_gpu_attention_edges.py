"""`-m gpu`: the last key tile and the K/V staging of the bf16 flash attention (csrc/attn_bf16.hip) against their earlier forms.

A last tile of at most 32 keys (N mod 64 in 1..32; N = 1370: 26) computes its first 32-key block only -- the second one is all masked:
scores of -inf, p = +0, +0 into the row sum and into O -- and the K/V tiles are staged through a buffer descriptor whose bound makes the key
rows >= N read as zeros where the per-lane pointers clamped them to row N - 1 (a zero K row is masked like any other, a zero V row meets
p = 0).  Neither changes a bit: test option "attn_diet" = 0 selects the full-width tail tile and the pointer staging, and the outputs must be
`torch.equal`; dod_test_counter("attn_diet") counts the launches whose last tile ran at half width.

Shapes.  (2, N, 2) is the 32-rows-per-wave kernel: N = 1, 26, 31, 32 a half tile alone, 33, 63, 64 not, 65, 90, 96 a full tile and a half
one, 97 not, 129 two full tiles and one key.  (64, N, 8) has B * heads * ceil(N / 256) = 1024 and a remainder of at most 128 rows: the fused
kernel with both bodies; 346 has the remainders of N = 1370 (90 rows, 26 keys), 352 exactly 32 keys in the last tile, 353 one more (full
width), 320 no tail tile.  The 64 images repeat 7 distinct ones (tests/attention_cases.py), so the float64 reference stays small.
Inputs sit between 256 rows of NaN, outputs between 256 guard rows (tests/test_gpu_attention.py): a read past the last key row that reached
a score or a product, or a store past the last row, fails."""
import functools

import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import attention_cases as ac
from tests.test_gpu_attention import BF16, DEV, GUARD, U8, Out, _check_mx, _hold

pytestmark = pytest.mark.gpu

SMALL = [(2, N, 2) for N in (1, 26, 31, 32, 33, 63, 64, 65, 90, 96, 97, 129)]
FUSED = [(64, N, 8) for N in (320, 346, 352, 353)]
MX_CASE = (64, 346, 8)


def _half_tile(N):
    return 1 <= N % 64 <= 32


@functools.lru_cache(maxsize=None)
def _reference(B, N, heads):
    """-> (bf16 values, want, T float64) of the distinct images [n_unique(B), N, .], on the CPU"""
    vals = ac.make_input(B, N, heads).bfloat16()
    return (vals,) + ac.ref64_qkv(vals.double(), heads)


@functools.lru_cache(maxsize=None)
def _case(B, N, heads):
    """-> (input rows [B * N, 3 D] bf16 inside a buffer whose other rows are NaN, that whole buffer, a copy of its bits,
    want, T [B * N, D] float64 on the device); computed once per shape and never written to"""
    vals, want_u, T_u = _reference(B, N, heads)
    idx = torch.from_numpy(ac.image_index(B)).to(DEV)
    tile = lambda u: u.to(DEV)[idx].reshape(B * N, -1)
    full = torch.full((B * N + 2 * GUARD, 3 * heads * 64), float("nan"), dtype=BF16, device=DEV)
    full[GUARD:GUARD + B * N] = tile(vals)
    return full[GUARD:GUARD + B * N], full, full.view(torch.int16).clone(), tile(want_u), tile(T_u)


def _launch(B, N, heads, option, mx=False):
    """one launch with "attn_diet" = option -> (outputs, launches the counter saw)"""
    x, full, bits, _, _ = _case(B, N, heads)
    D, rows, L = heads * 64, B * N, nat.lib()
    nat.check(L.dod_test_set_option(b"attn_diet", option))
    try:
        c0 = L.dod_test_counter(b"attn_diet")
        if mx:
            outs = (Out(rows, D, U8), Out(rows, D // 32, U8, unwritten=0xFF))
            nat.check(L.dod_op_attention_bf16_mx(nat.ptr(x), nat.ptr(outs[0].view), nat.ptr(outs[1].view), B, N, heads, ac.SCALE, nat.stream_ptr()))
        else:
            outs = (Out(rows, D, BF16),)
            nat.check(L.dod_op_attention_bf16(nat.ptr(x), nat.ptr(outs[0].view), B, N, heads, ac.SCALE, nat.stream_ptr()))
        torch.cuda.synchronize()
        counted = L.dod_test_counter(b"attn_diet") - c0
    finally:
        nat.check(L.dod_test_set_option(b"attn_diet", -1))
    for o in outs:
        assert o.guards_intact(), ((B, N, heads), option, "guard rows of the output written")
    assert torch.equal(full.view(torch.int16), bits), ((B, N, heads), option, "the input or its guard rows were written")
    return outs, counted


def _bit_for_bit(B, N, heads, mx=False):
    old, n_old = _launch(B, N, heads, 0, mx)
    new, n_new = _launch(B, N, heads, -1, mx)
    assert n_old == 0, "option 0 must run the last tile at full width"
    assert n_new == (1 if _half_tile(N) else 0), (N, n_new)
    for a, b in zip(old, new):
        assert torch.equal(a.raw, b.raw), ((B, N, heads), "the output bits differ from option 0's")
    forced, n_forced = _launch(B, N, heads, 1, mx)
    assert n_forced == n_new and all(torch.equal(a.raw, b.raw) for a, b in zip(new, forced))


@pytest.mark.parametrize("B,N,heads", SMALL)
def test_32_row_kernel_equals_option_0_bit_for_bit(B, N, heads):
    assert B * heads * ((N + 255) // 256) < 1024
    _bit_for_bit(B, N, heads)


@pytest.mark.parametrize("B,N,heads", FUSED)
def test_fused_kernel_equals_option_0_bit_for_bit(B, N, heads):
    assert B * heads * ((N + 255) // 256) >= 1024 and 0 < N % 256 <= 128 and N > 256
    _bit_for_bit(B, N, heads)


def test_mx_output_equals_option_0_bit_for_bit():
    _bit_for_bit(*MX_CASE, mx=True)


@pytest.mark.parametrize("B,N,heads", SMALL + FUSED)
def test_default_path_against_float64(B, N, heads):
    """bound: attention_cases.bf16_bound -- the context's and P's rounding to bf16 (2^-8 each) and ACC_REL of fp32 accumulation, per element"""
    _, _, _, want, T = _case(B, N, heads)
    outs, _ = _launch(B, N, heads, -1)
    _hold("bf16", f"{(B, N, heads)} edges", outs[0].view.double(), want, ac.bf16_bound(want, T))


def test_mx_default_path_against_float64():
    """the block-scaled form at the timed shape's remainders, held as tests/test_gpu_attention.py holds it"""
    B, N, heads = MX_CASE
    D = heads * 64
    _, _, _, want, T = _case(B, N, heads)
    _, want_u, T_u = _reference(B, N, heads)
    idx = torch.from_numpy(ac.image_index(B)).to(DEV)
    lo, hi = [t.reshape(-1, N, D // 32).to(DEV)[idx].reshape(B * N, -1) for t in ac.mx_byte_range(want_u.reshape(-1, D), T_u.reshape(-1, D))]
    outs, _ = _launch(B, N, heads, -1, mx=True)
    _check_mx(f"{(B, N, heads)} edges", outs, want, T, lo, hi, D)
