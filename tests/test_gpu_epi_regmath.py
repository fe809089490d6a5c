"""`-m gpu`: the register epilogue of the 16-wave bf16 GEMM (csrc/gemm_x3.hip EPI >= 1, csrc/gemm_epi.h epi_quad_bf16) against the LDS-staged one.

Plain bf16 output rows (QKV, fc1 of the bf16 mode) do their bias / folded-LayerNorm / GELU math on the accumulators and cross the LDS once,
as bf16; the row statistics and column parameters are fetched at kernel entry.  Per element it is the same fp32 operations in the same
order, so the output BITS equal the staged epilogue's (test option "epi_regmath" = 0), and so do the statistics a consumer publishes.

Shapes (the dispatcher sends M >= 4096, N >= 1536, K < 2048, K % 64 == 0 to this kernel), the smallest at which it can go wrong:
M = 4140 = 16 full m-tiles + 44 ragged rows, M = 4352 = exactly 17; N = 1544 leaves an n-tile of 8 columns; K = 64 is ONE K-tile -- the early
parameter loads meet the first and only wait -- K = 192 three."""
import ctypes as C

import pytest
import torch

from dinov2_od_amd import _native as nat
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
EPS = 1e-6
SPARE = 8            # rows behind row M that no store may touch
SENTINEL = -7.25     # exact in bf16 and fp32
KINDS = ["bias", "bias_gelu", "nobias", "cons_stats", "cons_part", "cons_part_gelu"]
SHAPES = [(M, N, K) for M in (4140, 4352) for N in (1536, 1544) for K in (64, 192)]
_cache = {}


def _inputs(M, N, K):
    """operands and statistics of one shape, computed once and shared by every epilogue kind (never written to)"""
    key = (M, N, K)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(M + 3 * N + 7 * K)
        x = torch.randn(M, K, device="cuda", generator=g)
        x = x * (0.5 + torch.rand(M, 1, device="cuda", generator=g) * 3) + torch.randn(M, 1, device="cuda", generator=g) * 1.5
        W = (torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16().contiguous()
        bias = torch.randn(N, device="cuda", generator=g) * 0.1
        csum = W.double().sum(-1).float()
        xd = x.double()
        mean = xd.mean(-1)
        rstd = 1.0 / torch.sqrt(((xd - mean[:, None]) ** 2).mean(-1) + EPS)
        stats = torch.stack([mean, rstd], -1).float().contiguous()
        # what a producer leaves: per 128-column group (sum, sum of squares) of the row minus a shift near its mean
        shift = torch.zeros(M, 2, device="cuda")
        shift[:, 0] = (mean + 0.05 * torch.randn(M, device="cuda", generator=g).double()).float()
        npart = (K + 127) // 128
        part = torch.zeros(M, npart, 2, device="cuda")
        for p in range(npart):
            d = x[:, 128 * p:128 * (p + 1)] - shift[:, :1]
            part[:, p, 0] = d.sum(-1)
            part[:, p, 1] = (d * d).sum(-1)
        _cache[key] = dict(x=x, xop=x.bfloat16().contiguous(), W=W, bias=bias, csum=csum, stats=stats, shift=shift, part=part, mean=mean, rstd=rstd)
    return _cache[key]


def _run(kind, d, M, N, K, option):
    """one launch with the test option set; -> (out [M + SPARE, N] bf16, stats_out [M + SPARE, 2] or None, launches counted)"""
    L = nat.lib()
    out = torch.full((M + SPARE, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    st_out = None
    act = nat.ACT["gelu" if kind.endswith("gelu") else "none"]
    nat.check(L.dod_test_set_option(b"epi_regmath", option))
    try:
        c0 = L.dod_test_counter(b"epi_regmath")
        if kind.startswith("cons"):
            if kind == "cons_stats":
                ln = nat.DodLnFold(d["stats"].data_ptr(), d["csum"].data_ptr(), None, None, None, None, None, 0.0)
            else:
                st_out = torch.full((M + SPARE, 2), SENTINEL, device="cuda")
                ln = nat.DodLnFold(d["shift"].data_ptr(), d["csum"].data_ptr(), None, None, None, d["part"].data_ptr(), st_out.data_ptr(), EPS)
            nat.check(L.dod_op_linear_ln(1, nat.ptr(d["xop"]), nat.ptr(d["W"]), None, M, N, K, nat.ptr(d["bias"]), None, None, 0, nat.ptr(out), 1, N, act,
                                         C.byref(ln), nat.stream_ptr()))
        else:
            bias = None if kind == "nobias" else d["bias"]
            nat.check(L.dod_op_linear(nat.DOD_BF16, nat.ptr(d["xop"]), K, nat.ptr(d["W"]), K, M, N, K, nat.ptr(bias), None, None, 0, nat.ptr(out),
                                      nat.DOD_BF16, N, act, nat.stream_ptr()))
        torch.cuda.synchronize()
        return out, st_out, L.dod_test_counter(b"epi_regmath") - c0
    finally:
        nat.check(L.dod_test_set_option(b"epi_regmath", -1))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N,K", SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in SHAPES])
def test_register_epilogue_equals_staged_epilogue_bit_for_bit(M, N, K, kind):
    d = _inputs(M, N, K)
    out0, st0, n0 = _run(kind, d, M, N, K, 0)
    out1, st1, n1 = _run(kind, d, M, N, K, 1)
    assert n0 == 0, "option 0 must take the LDS-staged epilogue"
    assert n1 == 1, "option 1: exactly one launch on the register epilogue"
    assert torch.equal(out0, out1)
    spare = torch.full((SPARE, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    assert torch.equal(out0[M:], spare) and torch.equal(out1[M:], spare), "a store went behind row M"
    assert not (out1[:M] == SENTINEL).all(dim=1).any(), "a row was never written"
    if st0 is not None:
        assert torch.equal(st0, st1), "published statistics differ"
        assert bool((st1[M:] == SENTINEL).all()), "a statistics store went behind row M"
        assert not bool((st1[:M, 1] == SENTINEL).any()), "a row's statistics were never published"


@pytest.mark.parametrize("kind", KINDS)
def test_register_epilogue_against_float64(kind):
    """Bound and reference of test_gpu_lnfold.test_folded_consumer_equals_layernorm_then_linear: the exact arithmetic of the rounded operands
    in float64; what remains is the bf16 rounding of the output, 2^-8."""
    M, N, K = 4140, 1544, 192
    d = _inputs(M, N, K)
    out, _, n = _run(kind, d, M, N, K, 1)
    assert n == 1
    acc = d["xop"].double() @ d["W"].double().t()
    if kind.startswith("cons"):
        want = (acc - d["mean"][:, None] * d["csum"].double()) * d["rstd"][:, None] + d["bias"].double()
    else:
        want = acc + (0 if kind == "nobias" else d["bias"].double())
    if kind.endswith("gelu"):
        want = torch.nn.functional.gelu(want)
    err = rel_err(out[:M].double().cpu().numpy(), want.cpu().numpy())
    print(f"register epilogue {kind} M={M} N={N} K={K}: {err:.2e}")
    assert err < 2 ** -8
