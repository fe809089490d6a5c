"""`-m gpu`: the fixed softmax reference of the bf16 flash attention (csrc/attn_bf16.hip) and its rerun.

The kernel takes every row's reference from key tile 0, runs the tiles behind it without a running maximum, and computes again -- with the
running maximum, the arithmetic it had before -- the rows whose normaliser is not below 2^60 or whose accumulators are not finite.  Test option
"attn_fixed_ref" = 0 sends every row through the running-maximum pass; dod_test_counter("attn_rerun") counts the workgroups that reran.

Input `mixed` (tests/test_attention_ref_cpu.py, where its classification is checked on the CPU): one key per spike in a LATER tile; a quarter of
the rows overflow on it, a quarter see p = 0 there, a few of the others pass the threshold.  Shapes, the smallest at which each path can go
wrong: (2, 64, 1) and (2, 1, 1) have no tile behind the first; (2, 65, 1) the spike IS the one-key half-width tail tile; (2, 97, 1) a spike in
a full-width tail tile; (2, 129, 1) two reference tiles and a one-key tail; (2, 257, 1) the three-slot ring wraps before the rerun restages;
(64, 346, 8) the fused launch -- the 64-row body over rows 0..255, the 32-row body over the last 90 -- with spikes in tile 1 and in the 26-key
tail tile, 7 distinct images; the same with the block-scaled output.
Per-row selection: every workgroup of every `mixed` launch holds overflowing rows and reruns, so equality with option 0 on the must-rerun rows
alone would also hold if a rerunning workgroup stored ALL of its rows.  Hence the converse: among the rows that must not rerun and whose maximum
lies behind tile 0 -- where the two forms round P against different references -- some must differ from option 0's bits.
Input `vbig` pins the finite test: no normaliser comes near 2^60, one value row is 2^110, and the rows whose p there passes 2^18 overflow an fp32
accumulator; without the test they would leave as inf or NaN and miss the bound.
Inputs sit between 256 rows of NaN (the rerun stages K/V a second time), outputs between 256 guard rows.  Bounds: attention_cases.bf16_bound
per element against float64, for the default launch and for option 0 alike."""
import functools

import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import attention_cases as ac
from tests import test_attention_ref_cpu as rc
from tests.test_gpu_attention import BF16, DEV, GUARD, U8, Out, _check_mx, _hold

pytestmark = pytest.mark.gpu

NO_LATER_TILE = [(2, 64, 1), (2, 1, 1)]
MIXED = [(2, 65, 1), (2, 97, 1), (2, 129, 1), (2, 257, 1), (64, 346, 8)]
MX_CASE = (64, 346, 8)


@functools.lru_cache(maxsize=None)
def _case(B, N, heads, kind):
    """-> (input rows [B * N, 3 D] bf16 inside a buffer whose other rows are NaN, that buffer, a copy of its bits, want, T [B * N, D] float64
    and the must-rerun / must-not-rerun / maximum-behind-tile-0 masks [B * N, D] on the device); computed once per case and never written to"""
    x, want_u, T_u, must_u, not_u = rc.case(B, N, heads, kind)
    idx = torch.from_numpy(ac.image_index(B)).to(DEV)
    tile = lambda u: u.to(DEV)[idx].reshape(B * N, -1)
    cols = lambda m: ac.unheads(m[..., None].expand(-1, -1, -1, 64))      # [n, heads, N] -> [n, N, D]
    full = torch.full((B * N + 2 * GUARD, 3 * heads * 64), float("nan"), dtype=BF16, device=DEV)
    full[GUARD:GUARD + B * N] = tile(x.bfloat16())
    later_u = rc.later_maximum(x, heads)
    return (full[GUARD:GUARD + B * N], full, full.view(torch.int16).clone(), tile(want_u), tile(T_u), tile(cols(must_u)), tile(cols(not_u)),
            tile(cols(later_u)))


def _run(x, B, N, heads, option, mx=False):
    """one launch of the rows x with "attn_fixed_ref" = option -> (outputs, workgroups that reran)"""
    D, rows, L = heads * 64, B * N, nat.lib()
    nat.check(L.dod_test_set_option(b"attn_fixed_ref", option))
    try:
        torch.cuda.synchronize()
        c0 = L.dod_test_counter(b"attn_rerun")
        if mx:
            outs = (Out(rows, D, U8), Out(rows, D // 32, U8, unwritten=0xFF))
            nat.check(L.dod_op_attention_bf16_mx(nat.ptr(x), nat.ptr(outs[0].view), nat.ptr(outs[1].view), B, N, heads, ac.SCALE, nat.stream_ptr()))
        else:
            outs = (Out(rows, D, BF16),)
            nat.check(L.dod_op_attention_bf16(nat.ptr(x), nat.ptr(outs[0].view), B, N, heads, ac.SCALE, nat.stream_ptr()))
        torch.cuda.synchronize()
        reran = L.dod_test_counter(b"attn_rerun") - c0
    finally:
        nat.check(L.dod_test_set_option(b"attn_fixed_ref", -1))
    assert c0 >= 0
    for o in outs:
        assert o.guards_intact(), ((B, N, heads), option, "guard rows of the output written")
    return outs, reran


def _launch(B, N, heads, kind, option, mx=False):
    x, full, bits = _case(B, N, heads, kind)[:3]
    outs, reran = _run(x, B, N, heads, option, mx)
    assert torch.equal(full.view(torch.int16), bits), ((B, N, heads), option, "the input or its guard rows were written")
    return outs, reran


def _both(B, N, heads, kind):
    """default and option 0, each within the bound of float64 -> (default, option 0, reran)"""
    want, T = _case(B, N, heads, kind)[3:5]
    new, reran = _launch(B, N, heads, kind, -1)
    old, reran_old = _launch(B, N, heads, kind, 0)
    assert reran_old == 0, "option 0 runs no fast pass: nothing to rerun"
    _hold("bf16", f"{(B, N, heads)} {kind} fixed reference", new[0].view.double(), want, ac.bf16_bound(want, T))
    _hold("bf16", f"{(B, N, heads)} {kind} option 0", old[0].view.double(), want, ac.bf16_bound(want, T))
    forced, reran_forced = _launch(B, N, heads, kind, 1)
    assert reran_forced == reran and torch.equal(forced[0].raw, new[0].raw)
    return new, old, reran


@pytest.mark.parametrize("B,N,heads", NO_LATER_TILE)
def test_one_key_tile_is_option_0_bit_for_bit(B, N, heads):
    new, old, reran = _both(B, N, heads, "mixed")
    assert reran == 0 and torch.equal(new[0].raw, old[0].raw)


@pytest.mark.parametrize("B,N,heads", MIXED)
def test_mixed_rows_rerun_and_the_others_do_not(B, N, heads):
    must, must_not, later = _case(B, N, heads, "mixed")[5:8]
    new, old, reran = _both(B, N, heads, "mixed")
    assert reran > 0, "a spike must send workgroups through the rerun"
    assert bool(must.any()) and torch.equal(new[0].view[must], old[0].view[must]), "a row that reran must carry option 0's bits"
    kept = must_not & later                  # rows of rerunning workgroups that keep the fixed-reference bits
    differ = int((new[0].view.view(torch.int16)[kept] != old[0].view.view(torch.int16)[kept]).sum())
    print(f"mixed {(B, N, heads)}: {int(kept.sum())} elements of rows that stay, {differ} of them differ from option 0")
    if B * heads * ((N + 255) // 256) >= 1024:      # enough such rows for the statement to be safe: the fused launch
        assert differ > 0, "rows that must not rerun carry option 0's bits: the rerun selects per workgroup, not per row"


def test_mixed_block_scaled_output():
    B, N, heads = MX_CASE
    D = heads * 64
    _, _, _, want, T, must = _case(B, N, heads, "mixed")[:6]
    _, want_u, T_u, _, _ = rc.case(B, N, heads, "mixed")
    idx = torch.from_numpy(ac.image_index(B)).to(DEV)
    lo, hi = [t.reshape(-1, N, D // 32).to(DEV)[idx].reshape(B * N, -1) for t in ac.mx_byte_range(want_u.reshape(-1, D), T_u.reshape(-1, D))]
    new, reran = _launch(B, N, heads, "mixed", -1, mx=True)
    old, reran_old = _launch(B, N, heads, "mixed", 0, mx=True)
    assert reran > 0 and reran_old == 0
    _check_mx(f"{(B, N, heads)} mixed fixed reference", new, want, T, lo, hi, D)
    _check_mx(f"{(B, N, heads)} mixed option 0", old, want, T, lo, hi, D)
    assert torch.equal(new[0].view[must], old[0].view[must])
    row_must = must.reshape(B * N, D // 32, 32)[..., 0]                     # per (row, 32-column block); scale bytes lie [row][2][D / 64]
    assert torch.equal(ac.mx_block_order(new[1].view, D)[row_must], ac.mx_block_order(old[1].view, D)[row_must])


def test_an_accumulator_that_is_not_finite_reruns_the_row():
    """`vbig` at (2, 129, 1): l stays below 2^59 in every row (asserted by the CPU classification), so only the finite test can ask for the rerun"""
    B, N, heads = 2, 129, 1
    must, must_not = _case(B, N, heads, "vbig")[5:7]
    assert bool(must.any()) and bool(must_not.any())
    new, old, reran = _both(B, N, heads, "vbig")          # a row that overflowed and was stored anyway is inf or NaN: outside the bound
    assert reran > 0
    assert torch.equal(new[0].view[must], old[0].view[must])


@pytest.mark.parametrize("B,N,heads", [(2, 300, 2), (256, 300, 2)])
def test_maxima_in_tile_0_are_option_0_bit_for_bit(B, N, heads):
    """every row's maximum is key 5: alpha was exactly 1 behind tile 0, so the reference form changes no bit and nothing reruns"""
    new, old, reran = _both(B, N, heads, "tile0")
    assert reran == 0 and torch.equal(new[0].raw, old[0].raw)


@pytest.mark.parametrize("B,N,heads", [(2, 300, 2), (2, 129, 1)])
def test_normal_input_does_not_rerun(B, N, heads):
    _, _, reran = _both(B, N, heads, "normal")
    assert reran == 0


def test_a_row_does_not_depend_on_its_launch():
    """two images of the (64, 346, 8) `mixed` launch alone as (2, 346, 8): the 32-row body everywhere, other workgroup mates.  Every row the
    float64 classification decides is bit-identical; an undecided row may fall on either side of the threshold (l is summed per launch form)."""
    B, N, heads = 64, 346, 8
    x, _, _, _, _, must, must_not = _case(B, N, heads, "mixed")[:7]
    decided = (must | must_not)[:2 * N]
    assert float((~decided).double().mean()) <= rc.UNDECIDED_CAP
    big, reran_big = _launch(B, N, heads, "mixed", -1)
    full = torch.full((2 * N + 2 * GUARD, 3 * heads * 64), float("nan"), dtype=BF16, device=DEV)
    full[GUARD:GUARD + 2 * N] = x[:2 * N]
    small, reran_small = _run(full[GUARD:GUARD + 2 * N], 2, N, heads, -1)
    assert reran_big > 0 and reran_small > 0
    assert bool(must[:2 * N].any()) and bool(must_not[:2 * N].any())
    assert torch.equal(big[0].view[:2 * N][decided], small[0].view[decided])
