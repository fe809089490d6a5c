"""`-m gpu`: every forward attention kernel in every output format a forward writes -- attn_bf16.hip (bf16 rows; block-scaled e4m3 bytes
+ e8m0 scale bytes, the fp8 mode's `MX` epilogue), attn_x3.hip (bf16 pair rows; H2 rows, the fp16x2 mode's epilogue), attn_f32m.hip and
attn_f32.hip (fp32) -- through its operator entry point against float64 softmax attention of the values the kernel is given.

One harness (tests/attention_cases.py holds the reference, the emulations and the bounds; tests/test_attention_cases_cpu.py what a CPU
can show of them):
  * every error is normalised per element by T[q, d] = sum_k p[q, k] |v[k, d]|, the size of what is summed there; the tensor-wide
    rel_err bounds that tests/test_gpu_ops.py and tests/test_gpu_x3.py hold the same kernels to are asserted beside it;
  * every output sits between 256 guard rows of a sentinel bit pattern and starts as another one that decodes to NaN: a store past
    the last row, or a missing one, fails; every input sits between 256 rows of NaN (the kernels clamp rows to N - 1: a read past the
    last row turns the output to NaN);
  * two launches of one input are bit-identical, and an image's rows do not change when the other images of the launch do.
Bounds: attn_bf16 from its two rounding points (attention_cases.bf16_bound); the block-scaled form from the same margin plus half an
e4m3 ulp, its scale byte exact wherever the margin decides it; attn_x3 max(2^-16, 4 x the distance of a CPU emulation that splits
where the kernel splits and accumulates in float64), computed per case; the fp32 kernels max(1e-6, 4 x the distance of torch's fp32
CPU attention).  The factor 4 (tests/test_gpu_train_ops.py) covers fp32 accumulation order and the exp2 approximation.
Shapes (attention_cases.SMALL / BIG): N around every key-tile and query-block edge, the XCD pair map with 1, 3, 8 and 9 (image, head)
pairs, and B = 256, heads = 2 at N = 300 / 400 / 512 -- the 64-rows-per-wave body of attn_bf16 as the fused short-tail launch, with a
long remainder and with none.  The large launches repeat 7 distinct images, so that their float64 reference stays small."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import attention_cases as ac
from tests.gpu_util import PATTERN, Out, guarded_input as _guarded_input
from tests.test_gpu_fp8 import ACC_TOL, quant_ref
from tests.test_gpu_h2 import decode as h2_decode, pack as h2_pack

pytestmark = pytest.mark.gpu

GUARD = ac.GUARD
DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
FLASH = ["bf16", "mx", "x3", "h2"]
WORST = {}      # kernel -> (error / bound, where); X3_DIST: kernel -> (largest emulation distance, where)
DIST = {}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    nat.lib()
    yield None
    for k in sorted(WORST):
        print(f"attention worst  {k:<6s} {WORST[k][0]:.3f} of its per-element bound at {WORST[k][1]}")
    for k in sorted(DIST):
        print(f"attention reference distance  {k:<6s} {DIST[k][0]:.3e} T at {DIST[k][1]}")


def _hold(kernel, where, got, want, bound):
    """|got - want| <= bound for every element (an unwritten element is NaN and fails); records the worst share of the bound"""
    err = (got - want).abs()
    ratio = float(torch.nan_to_num(err / bound, nan=0.0, posinf=float("inf")).max())      # 0 / 0: an exact zero, allowed
    print(f"{kernel} {where}: worst element at {ratio:.3f} of its bound")
    if ratio >= WORST.get(kernel, (-1.0,))[0]:
        WORST[kernel] = (ratio, where)
    assert bool((err <= bound).all()), (kernel, where, ratio, int((~(err <= bound)).sum()))


def _rel_err(got, want):
    return float((got - want).abs().max() / want.abs().max())


@functools.lru_cache(maxsize=None)
def _reference(family, B, N, heads, kind):
    """family "b": the bf16 kernels (values = the bf16-rounded input); "x": the x3 kernels (values = hi + lo of the pair layout).
    -> (device rows of the distinct images [nu, N, W] in the kernel's input format, want, T [nu, N, D] float64, emulation distance)"""
    x = ac.make_input(B, N, heads, kind)
    if family == "b":
        dev = x.bfloat16()
        want, T = ac.ref64_qkv(dev.double(), heads)
        return dev, want, T, None
    hi, lo = ac.split_pair(x)
    want, T = ac.ref64_qkv(hi.double() + lo.double(), heads)
    dist = ac.dist_by_T(ac.emu_x3(hi, lo, heads), want, T)
    return torch.cat([hi, lo], -1).bfloat16(), want, T, dist         # [hi(q|k|v) | lo(q|k|v)]


def _launch(kernel, xin, B, N, heads):
    D, rows, L, sp = heads * 64, B * N, nat.lib(), nat.stream_ptr()
    if kernel == "bf16":
        o = (Out(rows, D, BF16),)
        nat.check(L.dod_op_attention_bf16(nat.ptr(xin), nat.ptr(o[0].view), B, N, heads, ac.SCALE, sp))
    elif kernel == "mx":
        o = (Out(rows, D, U8), Out(rows, D // 32, U8, unwritten=0xFF))
        nat.check(L.dod_op_attention_bf16_mx(nat.ptr(xin), nat.ptr(o[0].view), nat.ptr(o[1].view), B, N, heads, ac.SCALE, sp))
    elif kernel == "x3":
        o = (Out(rows, 2 * D, BF16),)
        nat.check(L.dod_op_attention_x3(nat.ptr(xin), nat.ptr(o[0].view), B, N, heads, ac.SCALE, sp))
    else:
        o = (Out(rows, 4 * D, U8),)
        nat.check(L.dod_op_attention_x3_h2(nat.ptr(xin), nat.ptr(o[0].view), B, N, heads, ac.SCALE, sp))
    torch.cuda.synchronize()
    return o


def _check_mx(where, outs, want, T, lo, hi, D):
    q8, bs = outs[0].view, outs[1].view
    rows = q8.shape[0]
    assert not bool((bs == 0xFF).any()), "scale bytes left unwritten"
    eb = ac.mx_block_order(bs, D).long()
    assert bool(((eb == lo) | (eb == hi)).all()), (where, "scale byte outside the rule's range", int(((eb != lo) & (eb != hi)).sum()))
    undecided = float((lo != hi).double().mean())
    print(f"mx {where}: {undecided:.3f} of the scale bytes undecided by the margin, the others exact")
    assert undecided <= ac.MX_UNDECIDED_CAP
    zero = (T.reshape(rows, D // 32, 32) == 0).all(-1)               # an all-zero block: byte 1 and zero bytes
    assert bool((eb[zero] == 1).all()) and bool((q8.reshape(rows, D // 32, 32)[zero] == 0).all())
    sc = torch.exp2((eb - 127).double())[..., None].expand(rows, D // 32, 32).reshape(rows, D)
    got = ac.E4M3_LUT.to(DEV)[q8.long()] * sc
    margin = ac.mx_value_margin(T)
    _hold("mx", where, got, want, margin + ac.e4m3_half_ulp((want.abs() + margin) / sc) * sc)
    return got


def _check_h2(where, outs, want, T, xb, D):
    h, m8, r8 = [t.to(DEV) for t in h2_decode(outs[0].view, D)]
    # the main bytes are a function of the stored fp16 part alone
    assert torch.equal(m8, h.float().clamp(-448, 448).cpu().to(torch.float8_e4m3fn).double().to(DEV)), (where, "e4m3(h) bytes")
    rem = ((want - h).abs() + xb) * 2048.0
    _hold("h2", where, h + r8, want, xb + ac.e4m3_half_ulp(rem) / 2048.0)
    _hold("h2.fp16", where, h, want, xb + 2.0 ** -11 * (want.abs() + xb) + 2.0 ** -25)       # fp16(x): half an ulp, 2^-25 below the normal range


def _check_case(kernel, B, N, heads, kind="normal"):
    D, rows = heads * 64, B * N
    where = f"{(B, N, heads)} {kind}"
    dev_u, want_u, T_u, dist = _reference("b" if kernel in ("bf16", "mx") else "x", B, N, heads, kind)
    idx = torch.from_numpy(ac.image_index(B)).to(DEV)
    tile = lambda u: u.to(DEV)[idx].reshape(rows, -1)
    x_dev = tile(dev_u)
    outs = _launch(kernel, _guarded_input(x_dev), B, N, heads)
    for o in outs:
        assert o.guards_intact(), (kernel, where, "guard rows written")
    want, T = tile(want_u), tile(T_u)
    if kernel == "bf16":
        got = outs[0].view.double()
        _hold("bf16", where, got, want, ac.bf16_bound(want, T))
        assert _rel_err(got, want) < 1e-2
        assert float((got - want).abs().mean() / want.abs().mean()) < 3e-3
    elif kernel == "mx":
        lo, hi = [tile(t.reshape(-1, N, D // 32)) for t in ac.mx_byte_range(want_u.reshape(-1, D), T_u.reshape(-1, D))]
        _check_mx(where, outs, want, T, lo, hi, D)
    else:
        xrel = max(ac.X3_FLOOR, 4.0 * dist)
        print(f"{kernel} {where}: emulation distance {dist:.3e} T, bound {xrel:.3e} T")
        if dist >= DIST.get("x3", (-1.0,))[0]:
            DIST["x3"] = (dist, where)
        if kernel == "x3":
            c = outs[0].view.double()
            got = c[:, :D] + c[:, D:]
            _hold("x3", where, got, want, xrel * T)
            assert _rel_err(got, want) < 3e-5
        else:
            _check_h2(where, outs, want, T, xrel * T, D)
    # bit for bit: the same launch again; and the rows of one image when every other image of the launch holds other data
    again = _launch(kernel, _guarded_input(x_dev), B, N, heads)
    for o, a in zip(outs, again):
        assert torch.equal(o.raw, a.raw), (kernel, where, "two launches differ")
    if B >= 2:
        b0 = B // 2
        other = ac.make_input(B, N, heads, "normal", variant=1)
        other = other.bfloat16() if kernel in ("bf16", "mx") else torch.cat(ac.split_pair(other), -1).bfloat16()
        x2 = tile(other)
        x2[b0 * N:(b0 + 1) * N] = x_dev[b0 * N:(b0 + 1) * N]
        alone = _launch(kernel, _guarded_input(x2), B, N, heads)
        for o, a in zip(outs, alone):
            assert a.guards_intact()
            assert torch.equal(o.raw[GUARD + b0 * N:GUARD + (b0 + 1) * N], a.raw[GUARD + b0 * N:GUARD + (b0 + 1) * N]), (kernel, where, "an image depends on its neighbours")
    return outs


@pytest.mark.parametrize("B,N,heads", ac.SMALL)
@pytest.mark.parametrize("kernel", FLASH)
def test_tile_and_block_edges_and_pair_map(G, kernel, B, N, heads):
    _check_case(kernel, B, N, heads)


@pytest.mark.parametrize("B,N,heads", ac.BIG)
@pytest.mark.parametrize("kernel", ["bf16", "mx"])
def test_attn_bf16_64_row_body_launch_forms(G, kernel, B, N, heads):
    """npairs * ceil(N / 256) >= 1024: 64 query rows per wave.  N = 300: the fused launch whose trailing workgroups run the 32-row body
    over the last 44 rows; 400: one body, the last block's 144 rows leave a wave with 16 rows and one with none; 512: no remainder."""
    assert B * heads * ((N + 255) // 256) >= 1024
    _check_case(kernel, B, N, heads)


@pytest.mark.parametrize("kind", ac.SOFTMAX_KINDS)
@pytest.mark.parametrize("kernel", FLASH)
def test_online_softmax(G, kernel, kind):
    """N = 300, five key tiles: maxima that rise in tiles 1, 2 and 3 (three rescales); maxima in tile 0 (every later alpha is 1); rows
    whose scores are all one number; scores of order +-60 (tests/test_attention_cases_cpu.py shows the inputs are that)"""
    _check_case(kernel, 2, 300, 1, kind)


@pytest.mark.parametrize("kernel", ["bf16", "mx"])
def test_online_softmax_rising_maxima_in_the_64_row_body(G, kernel):
    _check_case(kernel, 256, 300, 2, "rising")


@pytest.mark.parametrize("kernel", FLASH)
def test_all_zero_head(G, kernel):
    """v = 0 for the last head: exact zeros in every format; the block-scaled form writes scale byte 1 and zero bytes there"""
    outs = _check_case(kernel, 2, 65, 2, "vzero")
    if kernel == "mx":
        assert bool((outs[0].view[:, 64:] == 0).all()) and bool((ac.mx_block_order(outs[1].view, 128)[:, 2:] == 1).all())


def test_mx_epilogue_feeds_the_block_scaled_gemm(G):
    """heads = 4 (D = 256, four scale bytes per half): the epilogue's bytes and scale bytes as the A operand of dod_op_linear_fp8_mx against
    the float64 product of the decoded operands -- the byte order as the consumer reads it"""
    B, N, heads, Nout = 2, 150, 4, 128
    D, M = heads * 64, B * N
    outs = _check_case("mx", B, N, heads)
    q8, bs = outs[0].view, outs[1].view
    eb = ac.mx_block_order(bs, D).long()
    a = (ac.E4M3_LUT.to(DEV)[q8.long()].reshape(M, D // 32, 32) * torch.exp2((eb - 127).double())[..., None]).reshape(M, D)
    W = torch.from_numpy(np.random.default_rng(5).standard_normal((Nout, D)).astype(np.float32) * 0.05)
    qw, sw = quant_ref(W)
    qw_d, sw_d = qw.view(torch.uint8).to(DEV), sw.to(DEV)
    out = Out(M, Nout, F32)
    nat.check(nat.lib().dod_op_linear_fp8_mx(nat.ptr(q8), D, nat.ptr(bs), nat.ptr(qw_d), D, nat.ptr(sw_d), M, Nout, D, None, None, None, 0,
                                             nat.ptr(out.view), nat.DOD_F32, Nout, 0, nat.stream_ptr()))
    torch.cuda.synchronize()
    want = a @ (qw.double() * sw.double()[:, None]).t().to(DEV)
    err = _rel_err(out.view.double(), want)
    print(f"mx epilogue -> fp8 mx gemm: rel err vs the decoded operands' product {err:.2e}")
    assert out.guards_intact() and err < ACC_TOL


def test_h2_epilogue_feeds_the_h2_gemm(G):
    """the H2 rows as the A operand of dod_op_linear_h2 against the float64 product of the decoded operands"""
    B, N, heads, Nout = 2, 150, 2, 100
    D, M = heads * 64, B * N
    outs = _check_case("h2", B, N, heads)
    W = torch.from_numpy(np.random.default_rng(6).standard_normal((Nout, D)).astype(np.float32) * 0.05)
    Wb, wexp = h2_pack(W.to(DEV), weight=True)
    ah, am, ar = h2_decode(outs[0].view, D)
    wh, wm, wr = h2_decode(Wb, D, wexp)
    defined = ah @ wh.t() + am @ wr.t() + ar @ wm.t()
    out = Out(M, Nout, F32)
    nat.check(nat.lib().dod_op_linear_h2(nat.ptr(outs[0].view), nat.ptr(Wb), nat.ptr(wexp), M, Nout, D, None, None, None, 0,
                                         nat.ptr(out.view), 0, Nout, 0, nat.stream_ptr()))
    torch.cuda.synchronize()
    err = _rel_err(out.view.double().cpu(), defined)
    print(f"h2 epilogue -> h2 gemm: rel err vs the decoded operands' product {err:.2e}")
    assert out.guards_intact() and err < 2e-6


# ------------------------------------------------------------------------------------------------ fp32 kernels
def _f32_case(where, B, Lq, Lk, heads, dh, q_buf, q_col, ldq, kv_buf, k_col, v_col, ldkv, ldo):
    """q_buf [B * Lq, ldq], kv_buf [B * Lk, ldkv] CUDA fp32 inside NaN rows (pad columns NaN too); q / k / v start at the given columns"""
    E, sc, L = heads * dh, 1.0 / math.sqrt(dh), nat.lib()
    kern = "f32.mfma" if dh in (32, 64, 96) else "f32.valu"
    at = lambda buf, col: C.c_void_p(buf.data_ptr() + 4 * col)

    def launch(qb, kvb):
        o = Out(B * Lq, ldo, F32)
        nat.check(L.dod_op_attention_f32(at(qb, q_col), at(kvb, k_col), at(kvb, v_col), nat.ptr(o.view), ldq, ldkv, ldkv, ldo, Lq, Lk, B, heads, dh,
                                         sc, nat.stream_ptr()))
        torch.cuda.synchronize()
        return o
    o = launch(q_buf, kv_buf)
    assert o.guards_intact(), (where, "guard rows written")
    if ldo > E:
        assert bool((o.raw[GUARD:GUARD + B * Lq, E:] == PATTERN[F32][2]).all()), (where, "columns past the row's width written")
    q = q_buf[:, q_col:q_col + E].cpu().reshape(B, Lq, E)
    k = kv_buf[:, k_col:k_col + E].cpu().reshape(B, Lk, E)
    v = kv_buf[:, v_col:v_col + E].cpu().reshape(B, Lk, E)
    want, T = ac.ref64(q, k, v, heads, sc)
    e_ref = ac.dist_by_T(ac.f32_cpu(q, k, v, heads, sc), want, T)
    rel = max(ac.F32_FLOOR, 4.0 * e_ref)
    print(f"{kern} {where}: torch fp32 CPU distance {e_ref:.3e} T, bound {rel:.3e} T")
    if e_ref >= DIST.get(kern, (-1.0,))[0]:
        DIST[kern] = (e_ref, where)
    got = o.view[:, :E].double().cpu().reshape(B, Lq, E)
    _hold(kern, where, got, want, rel * T)
    assert _rel_err(got, want) < 5e-6
    assert torch.equal(o.raw, launch(q_buf, kv_buf).raw), (where, "two launches differ")
    # image 1 with other data in image 0
    q2, kv2 = q_buf.clone(), kv_buf.clone()
    q2[:Lq] = q_buf[:Lq].flip(0) * 0.5 + 0.25
    kv2[:Lk] = kv_buf[:Lk].flip(0) * 0.5 + 0.25
    o2 = launch(_guarded_input(q2), _guarded_input(kv2))
    assert o2.guards_intact() and torch.equal(o.raw[GUARD + Lq:], o2.raw[GUARD + Lq:]), (where, "an image depends on its neighbours")      # bit patterns: the pad columns hold NaN


def _randn(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("N", [33, 129])
@pytest.mark.parametrize("dh", [32, 64, 96, 48, 128])
def test_attention_f32_self_attention_form(G, dh, N):
    """q, k, v as three views of ONE [B * N, 3E] buffer, ld = 3E, as the forward passes them (head_dim 32 / 64 / 96: the fp32-MFMA
    kernel; 48 / 128: the VALU kernel); N = 33: one ragged query block and key tile, 129: a one-row second block / a one-key third tile"""
    B, heads = 2, 3
    E = heads * dh
    buf = _guarded_input(_randn(dh * 1000 + N, (B * N, 3 * E)).to(DEV))
    _f32_case(f"self {(B, N, heads, dh)}", B, N, N, heads, dh, buf, 0, 3 * E, buf, E, 2 * E, 3 * E, E)


@pytest.mark.parametrize("Lk", [64, 65, 200])
@pytest.mark.parametrize("dh", [96, 48])
def test_attention_f32_cross_attention_form(G, dh, Lk):
    """the decoder's cross-attention: Lq = 5 != Lk, q in a buffer of its own pitch, k and v side by side in another, an output pitch wider
    than E; every pad column of the inputs is NaN"""
    B, Lq, heads = 2, 5, 2
    E = heads * dh
    ldq, ldkv, ldo = E + 4, 2 * E + 8, E + 8
    qb = torch.full((B * Lq, ldq), float("nan"))
    qb[:, :E] = _randn(dh + Lk, (B * Lq, E))
    kvb = torch.full((B * Lk, ldkv), float("nan"))
    kvb[:, :E] = _randn(dh + Lk + 1, (B * Lk, E))
    kvb[:, E + 4:2 * E + 4] = _randn(dh + Lk + 2, (B * Lk, E))
    _f32_case(f"cross {(B, Lq, Lk, heads, dh)}", B, Lq, Lk, heads, dh, _guarded_input(qb.to(DEV)), 0, ldq, _guarded_input(kvb.to(DEV)), 0, E + 4, ldkv, ldo)
