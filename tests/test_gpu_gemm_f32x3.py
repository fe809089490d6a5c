"""`-m gpu`: the fp32-in bf16 split GEMM (csrc/gemm_f32x3.hip) through dod_op_gemm_f32x3 / dod_op_linear_f32x3, against float64.

The kernel reads fp32 operands, splits each x = h + l (h = bf16_rne(x), l = bf16_rne(x - h)) on its way into LDS and accumulates
Ah Wh^T + Ah Wl^T + Al Wh^T in fp32 on the bf16 MFMA.  Two bounds, both the project's own:
    3e-5  against the exact (float64) product of the fp32 inputs -- TOL of tests/test_gpu_x3.py, as rel_err;
    3e-6  against the float64 evaluation of the same three split terms (halves from torch.bfloat16 rounding on the CPU) -- the bound
          test_gemm_f32x_operand_layouts holds the fp32 kernel to: only the fp32 accumulation separates the two.
On these shapes the split evaluation itself sits 3.0e-6 .. 5.2e-6 from exact, a product with one cross term missing >= 1.2e-3 and a
single-pass bf16 product >= 1.7e-3, so both bounds discriminate.
Every output sits between guard rows of a sentinel (NaN where the kernel must write, or the addend where it accumulates), every operand
has a pitch of its width + 4 with NaN in the pad columns: an unmasked tail or a store past the tile shows."""
import functools

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, synth
from tests.cases import rel_err

pytestmark = pytest.mark.gpu

TOL_EXACT, TOL_SPLIT = 3e-5, 3e-6
GUARD, SENT = 64, 777.25
SHAPES = [(1, 4, 64), (100, 50, 768), (257, 64, 257), (333, 95, 130), (70, 768, 4112), (768, 2, 4112), (37, 29, 5)]      # K = 5: less than one k-tile


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from tests import gpu_util
    nat.lib()
    return gpu_util


class _Tile:
    """the "f32x3_tile" test option for the body of a `with`, handed back on exit"""

    def __init__(self, tile):
        self.tile = tile

    def __enter__(self):
        nat.set_option("f32x3_tile", self.tile)

    def __exit__(self, *a):
        nat.set_option("f32x3_tile", -1)


def _n(key, shape, std=1.0):
    return torch.from_numpy(synth.normal(29, key, shape, std))


def _split(x):
    h = x.bfloat16().float()
    return h.double(), (x - h).bfloat16().double()


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """operands, addend, the exact product and the float64 evaluation of the three split terms: computed once per shape, never modified"""
    A, W, C0 = _n(f"x3g.A.{M}.{K}", (M, K)), _n(f"x3g.W.{N}.{K}", (N, K), 0.05), _n(f"x3g.C.{M}.{N}", (M, N))
    exact = A.double() @ W.double().t()
    (ah, al), (wh, wl) = _split(A), _split(W)
    split = ah @ wh.t() + ah @ wl.t() + al @ wh.t()
    return A, W, C0, exact, split


def _operand(G, X, kmajor, pad=4):
    """X [rows, K] on the GPU as the kernel reads it: [rows, K + pad] or, k-major, [K, rows + pad]; NaN in the pad columns"""
    S = X.t() if kmajor else X
    buf = torch.full((S.shape[0], S.shape[1] + pad), float("nan"), dtype=torch.float32)
    buf[:, :S.shape[1]] = S
    return G.to_gpu(buf.numpy()), buf.shape[1]


def _output(G, M, N, init=None):
    """[GUARD + M + GUARD, N + 3]: sentinel everywhere, NaN (or `init`) in the M x N block the kernel owns -> (whole buffer, view of the block's rows)"""
    full = torch.full((M + 2 * GUARD, N + 3), SENT, dtype=torch.float32)
    full[GUARD:GUARD + M, :N] = float("nan") if init is None else init
    full = G.to_gpu(full.numpy())
    return full, full[GUARD:GUARD + M]


def _result(full, M, N, what):
    f = full.cpu()
    assert bool((f[:GUARD] == SENT).all()) and bool((f[GUARD + M:] == SENT).all()), f"{what}: guard rows written"
    assert bool((f[GUARD:GUARD + M, N:] == SENT).all()), f"{what}: columns past the row's width written"
    got = f[GUARD:GUARD + M, :N]
    assert not bool(torch.isnan(got).any()), f"{what}: elements left unwritten, or a pad column read"
    return got.numpy()


def _gemm(A, lda, akm, asb, ash, W, ldw, wkm, wsb, wsh, Cm, ldc, csb, csh, M, N, K, batch, hb, alpha, acc, ksplit):
    nat.check(nat.lib().dod_op_gemm_f32x3(nat.ptr(A), lda, akm, asb, ash, nat.ptr(W), ldw, wkm, wsb, wsh, nat.ptr(Cm), ldc, csb, csh,
                                          M, N, K, batch, hb, alpha, acc, ksplit, nat.stream_ptr()))


def _hold(got, exact, split, what):
    e_exact, e_split = rel_err(got, exact.numpy()), rel_err(got, split.numpy())
    print(f"gemm_f32x3 {what}: {e_exact:.2e} from exact, {e_split:.2e} from the float64 split evaluation")
    assert e_exact < TOL_EXACT and e_split < TOL_SPLIT, (what, e_exact, e_split)


def _layouts(G, M, N, K, akm, wkm, pad, what):
    A, W, C0, exact, split = _case(M, N, K)
    Ad, lda = _operand(G, A, akm, pad)
    Wd, ldw = _operand(G, W, wkm, pad)
    full, out = _output(G, M, N)
    _gemm(Ad, lda, akm, 0, 0, Wd, ldw, wkm, 0, 0, out, N + 3, 0, 0, M, N, K, 1, 1, 1.0, 0, 1)
    _hold(_result(full, M, N, what), exact, split, f"{what} plain")
    full, out = _output(G, M, N, C0)
    _gemm(Ad, lda, akm, 0, 0, Wd, ldw, wkm, 0, 0, out, N + 3, 0, 0, M, N, K, 1, 1, 0.5, 1, 1)
    _hold(_result(full, M, N, what), C0.double() + 0.5 * exact, C0.double() + 0.5 * split, f"{what} alpha 0.5, accumulate")
    for ks in (2, 7):      # K <= 192 has fewer than 7 k-tiles of 32: the launcher clamps the slice count
        full, out = _output(G, M, N, C0)
        _gemm(Ad, lda, akm, 0, 0, Wd, ldw, wkm, 0, 0, out, N + 3, 0, 0, M, N, K, 1, 1, 0.5, 1, ks)
        _hold(_result(full, M, N, what), C0.double() + 0.5 * exact, C0.double() + 0.5 * split, f"{what} ksplit {ks}")


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("akm,wkm", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_f32x3_operand_layouts(G, M, N, K, akm, wkm, tile):
    """either operand k-major, odd sizes, alpha, accumulate and the K slices with their atomic accumulate, under both tile forms"""
    with _Tile(tile):
        _layouts(G, M, N, K, akm, wkm, 4, f"{M}x{N}x{K} akm {akm} wkm {wkm} tile {tile}")


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("akm,wkm", [(0, 0), (1, 1)])
def test_gemm_f32x3_pitches_that_rule_out_vector_loads(G, akm, wkm, tile):
    """pitches of width + 5 floats: no row but the first is 16-byte aligned, so every load is the scalar form"""
    with _Tile(tile):
        _layouts(G, 100, 50, 768, akm, wkm, 5, f"100x50x768 pitch + 5 akm {akm} wkm {wkm} tile {tile}")


def test_gemm_f32x3_shipped_tile_rule(G):
    """128x128 from 256 such tiles up (one per CU): 2051 x 2053 is 17 x 17 of them; 100 x 50 is one"""
    L = nat.lib()
    for (M, N, K), wide in (((2051, 2053, 40), 1), ((100, 50, 768), 0)):
        A, W, _, exact, split = _case(M, N, K)
        Ad, lda = _operand(G, A, 0)
        Wd, ldw = _operand(G, W, 0)
        full, out = _output(G, M, N)
        n0, w0 = L.dod_test_counter(b"f32x3_launches"), L.dod_test_counter(b"f32x3_wide_launches")
        _gemm(Ad, lda, 0, 0, 0, Wd, ldw, 0, 0, 0, out, N + 3, 0, 0, M, N, K, 1, 1, 1.0, 0, 1)
        assert L.dod_test_counter(b"f32x3_launches") - n0 == 1
        assert L.dod_test_counter(b"f32x3_wide_launches") - w0 == wide, (M, N, K)
        _hold(_result(full, M, N, f"{M}x{N}x{K}"), exact, split, f"{M}x{N}x{K} shipped rule")


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("M,N,K", [(100, 50, 768), (333, 95, 130)])
def test_linear_f32x3_epilogue(G, M, N, K, tile):
    """bias with none / ReLU / GELU, and LayerScale + residual (the backbone tail's out-proj / fc2 form), against float64"""
    A, W, _, exact, _s = _case(M, N, K)
    bias, scale, resid = _n("x3g.b", (N,)), 1 + _n("x3g.s", (N,), 0.1), _n("x3g.r", (M, N))
    Ad, lda = _operand(G, A, 0)
    Wd = G.to_gpu(W.numpy())
    bd, sd, rd = G.to_gpu(bias.numpy()), G.to_gpu(scale.numpy()), G.to_gpu(resid.numpy())
    z = exact + bias.double()

    def run(act, scale=None, resid=None):
        full, out = _output(G, M, N)
        nat.check(nat.lib().dod_op_linear_f32x3(nat.ptr(Ad), lda, nat.ptr(Wd), nat.ptr(bd), nat.ptr(scale), nat.ptr(resid), N if resid is not None else 0,
                                                M, N, K, nat.ptr(out), N + 3, nat.ACT[act], nat.stream_ptr()))
        return _result(full, M, N, f"{M}x{N}x{K} {act}")
    with _Tile(tile):
        for act, want in (("none", z), ("relu", torch.relu(z)), ("gelu", torch.nn.functional.gelu(z))):
            e = rel_err(run(act), want.numpy())
            print(f"linear_f32x3 {M}x{N}x{K} tile {tile} bias + {act}: {e:.2e}")
            assert e < TOL_EXACT, (act, e)
        e = rel_err(run("none", sd, rd), (z * scale.double() + resid.double()).numpy())
        print(f"linear_f32x3 {M}x{N}x{K} tile {tile} bias, scale, residual: {e:.2e}")
        assert e < TOL_EXACT, e


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("B,H,Q,dh", [(2, 4, 7, 16), (3, 8, 100, 96)])
def test_gemm_f32x3_batched_attention_views(G, B, H, Q, dh, tile):
    """the three products of test_gemm_f32x_batched_attention_views: the (image, head) batch over strided views of a [B*Q, 3*D] buffer"""
    D = H * dh
    qkv = synth.normal(29, "x3g.qkv", (B * Q, 3 * D), 1.0)
    Qp = (Q + 3) // 4 * 4
    t = torch.from_numpy(qkv).double().view(B, Q, 3, H, dh)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))        # [B, H, Q, dh]
    S_ref = 0.25 * q @ k.transpose(-1, -2)
    qd = G.to_gpu(qkv)
    ld, qs, ss = 3 * D, Q * 3 * D, Q * Qp
    with _Tile(tile):
        S = torch.zeros(B * H, Q, Qp, device=G.dev())
        _gemm(qd, ld, 0, qs, dh, qd[:, D:], ld, 0, qs, dh, S, Qp, ss * H, ss, Q, Q, dh, B * H, H, 0.25, 0, 1)
        assert rel_err(S[:, :, :Q].cpu().numpy().reshape(B, H, Q, Q), S_ref.numpy()) < TOL_EXACT
        assert float(S[:, :, Q:].abs().max()) == 0.0 if Qp > Q else True
        O = torch.full((B * Q, D), float("nan"), device=G.dev())
        _gemm(S, Qp, 0, ss * H, ss, qd[:, 2 * D:], ld, 1, qs, dh, O, D, Q * D, dh, Q, dh, Q, B * H, H, 1.0, 0, 1)
        O_ref = (S_ref @ v).permute(0, 2, 1, 3).reshape(B * Q, D)
        assert rel_err(O.cpu().numpy(), O_ref.numpy()) < TOL_EXACT
        dK = torch.full((B * Q, D), float("nan"), device=G.dev())
        _gemm(S, Qp, 1, ss * H, ss, qd, ld, 1, qs, dh, dK, D, Q * D, dh, Q, dh, Q, B * H, H, 1.0, 0, 1)
        dK_ref = (S_ref.transpose(-1, -2) @ q).permute(0, 2, 1, 3).reshape(B * Q, D)
        assert rel_err(dK.cpu().numpy(), dK_ref.numpy()) < TOL_EXACT
