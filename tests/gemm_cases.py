"""Float64 references, CPU stand-ins and per-element bounds of the inference GEMM operator tests (tests/test_gpu_gemm_edges.py on the GPU,
tests/test_gemm_cases_cpu.py for what can be shown without one).  Everything here is plain torch on the CPU.

One rule for every kernel family, as in tests/attention_cases.py: the reference is the float64 product of the values the kernel is actually
given (bf16-rounded operands; hi + lo of the pair layout; the decoded H2 parts; dequantised e4m3 with its scales), and every error is
normalised PER ELEMENT by the size of what is summed there,
    T[m, n] = sum_k |a[m, k]| |w[n, k]|,
never by the tensor's maximum.

Bounds on the accumulated product, before the epilogue:
  * fp32 accumulation (every family, against the reference of its own operands): max(2^-22, 4 d32) T, d32 = the largest
    |torch fp32 CPU product - float64| / T of the case.  The factor 4 is tests/test_gpu_train_ops.py's, for accumulation order.  The floor:
    a 32-products-per-step chunked fp32 accumulation (`chunked_f32`, the stand-in kernel) sits at 3.2e-8 .. 5.0e-8 T for K = 64 .. 3072 and
    d32 at 2e-8 .. 3.0e-7 (tests/test_gemm_cases_cpu.py prints both; the largest d32 is the H2 product's), so 2^-22 = 2.4e-7 is about 5 x a
    valid other summation order, and about 4 x under what 3e-6 of the tensor's maximum allows at K = 768.
  * fp8 MFMA kernels: ACC_TOL T (tests/test_gpu_fp8.py: the instruction aligns its 64 products more narrowly than an fp32 chain).
  * x3 and H2 against the exact product of the fp32 inputs: max(2^-16, 4 dist) T, dist = the distance of the float64 "defined" reference
    from the exact product, per case (tests/attention_cases.py's recipe).
Through the epilogue (`epilogue`) the bound is carried by the activation's largest slope and |scale|, and every fp32 operation adds half an
fp32 ulp of its result; a bf16 output adds half a bf16 ulp, a pair output 2^-17 |want|."""
import zlib

import numpy as np
import torch

from tests.attention_cases import bf, dist_by_T, split_pair, E4M3_LUT      # noqa: F401  (re-exported)

ACC_FLOOR = 2.0 ** -22
SPLIT_FLOOR = 2.0 ** -16
HALF_F32 = 2.0 ** -24            # half an fp32 ulp, relative
PAIR_REL = 2.0 ** -17            # hi + lo of a pair row: 16 significant bits
# activation: (largest slope, absolute error of the device function beside one rounding of its result).  GELU (dod_common.h gelu_fast2): erf by
# Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, times |x| / 2, and one v_rcp and one v_exp (1 ulp each) on factors of at most |x| / 2:
# 2^-22 |x| = 2.4e-7 |x| covers 0.75e-7 |x| + 2 x 2^-23 x |x| / 2 with room; the strict kernel's erff is tighter.  Sigmoid: expf to 2 ulp
# moves 1 / (1 + e) by at most 2^-22 of a value <= 1.
ACT_SLOPE = {"none": 1.0, "relu": 1.0, "gelu": 1.13, "sigmoid": 0.25}


def half_ulp_bf16(y):
    """half a bf16 ulp at magnitude y: 8 significant bits, so 2^(e - 8) in the binade [2^e, 2^(e + 1)); subnormal spacing below 2^-126"""
    return torch.exp2(torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -126))) - 8)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def normal(key, shape, std=1.0):
    return torch.from_numpy((np.random.default_rng(seed_of(*key)).standard_normal(shape) * std).astype(np.float32))


def operands(M, N, K, tag=""):
    """fp32 A [M, K] (unit variance) and W [N, K] (std 0.05), seeded by the shape"""
    return normal(("A", M, K, tag), (M, K)), normal(("W", N, K, tag), (N, K), 0.05)


def epi_params(M, N, tag=""):
    """bias [N], LayerScale [N] around 1, residual [M, N]"""
    return normal(("b", N, tag), (N,)), 1.0 + normal(("s", N, tag), (N,), 0.1), normal(("r", M, N, tag), (M, N))


def size_T(a, w):
    return a.double().abs() @ w.double().abs().t()


# ------------------------------------------------------------------------------------------------ references of the values a kernel is given
def ref_plain(a, w):
    """float64 product of the given operand values (bf16-rounded, fp32, or dequantised e4m3) -> (want, T)"""
    return a.double() @ w.double().t(), size_T(a, w)


def ref_x3(ah, al, wh, wl):
    """the split product as the kernels define it: Ah Wh + Al Wh + Ah Wl (lo . lo dropped) -> (defined, T of hi + lo)"""
    ah, al, wh, wl = ah.double(), al.double(), wh.double(), wl.double()
    return ah @ wh.t() + al @ wh.t() + ah @ wl.t(), size_T(ah + al, wh + wl)


def ref_h2(a_parts, w_parts):
    """decoded H2 parts (tests/test_gpu_h2.decode: fp16 part, e4m3 main, e4m3 remainder): fp16 product + both cross terms"""
    (ah, am, ar), (wh, wm, wr) = a_parts, w_parts
    return ah @ wh.t() + am @ wr.t() + ar @ wm.t(), size_T(ah + ar, wh + wr)


def h2_parts_cpu(x, weight=False):
    """the H2 packing in torch on the CPU, as tests/test_gpu_h2.py pins dod_op_split_h2 to it bit for bit -> (h, main, remainder) float64"""
    xc = x.float().clamp(-65504, 65504)
    hh = xc.half()
    if not weight:
        return (hh.double(), hh.float().clamp(-448, 448).to(torch.float8_e4m3fn).double(),
                ((xc - hh.float()) * 2048).clamp(-448, 448).to(torch.float8_e4m3fn).double() / 2048)
    amax = hh.float().abs().amax(1)
    e = torch.where(amax > 0, torch.floor(torch.log2(448.0 / amax.double())), torch.zeros_like(amax, dtype=torch.float64))
    sc = torch.exp2(e)[:, None]
    return (hh.double(), (hh.double() * sc).float().to(torch.float8_e4m3fn).double() / sc,
            ((xc - hh.float()).double() * sc * 2048).float().to(torch.float8_e4m3fn).double() / (sc * 2048))


def dequant_rows(q, scale):
    """per-row scaled e4m3 (tests/test_gpu_fp8.quant_ref) -> float64 values"""
    return q.double() * scale.double()[:, None]


def dequant_mx(q, lay):
    """block-scaled e4m3 with its e8m0 bytes in the kernels' [rows][2][K / 64] layout (tests/test_gpu_fp8.mx_ref) -> float64 values"""
    rows, K = q.shape
    eb = lay.reshape(rows, 2, K // 64).permute(0, 2, 1).reshape(rows, K // 32).double()
    return (q.double().reshape(rows, K // 32, 32) * torch.exp2(eb - 127)[..., None]).reshape(rows, K)


# ------------------------------------------------------------------------------------------------ fp32 stand-ins and distances
def f32_product(terms):
    """torch's fp32 CPU product of the (a, w) operand pairs, summed in fp32: its distance from float64 is d32"""
    out = None
    for a, w in terms:
        p = a.float() @ w.float().t()
        out = p if out is None else out + p
    return out.double()


def chunked_f32(terms, chunk=32, drop=None):
    """the CPU stand-in kernel: fp32 accumulation of the same operands, `chunk` products per step, the terms of one step in order (the
    three-term x3 form: pass [(ah, wl), (al, wh), (ah, wh)]).  drop = (term, step): that term is left out of that one step (a planted defect)"""
    K = terms[0][0].shape[1]
    acc = torch.zeros(terms[0][0].shape[0], terms[0][1].shape[0], dtype=torch.float32)
    for s, k0 in enumerate(range(0, K, chunk)):
        for t, (a, w) in enumerate(terms):
            if drop == (t, s):
                continue
            acc += a[:, k0:k0 + chunk].float() @ w[:, k0:k0 + chunk].float().t()
    return acc.double()


def acc_rel(d32):
    return max(ACC_FLOOR, 4.0 * d32)


def split_rel(dist):
    return max(SPLIT_FLOOR, 4.0 * dist)


# ------------------------------------------------------------------------------------------------ epilogue
def _act64(x, act):
    if act == "none":
        return x
    if act == "relu":
        return torch.relu(x)
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    if act == "sigmoid":
        return torch.sigmoid(x)
    raise ValueError(act)


def epilogue(z, zb, bias=None, scale=None, resid=None, act="none", glu=False, out="f32"):
    """float64 epilogue of the product z whose error is bounded by zb: act(z + bias) * scale + resid, or with glu the SwiGLU gate of the
    interleaved column pairs, silu(x[2i]) * x[2i + 1].  out: "f32", "bf16" or "pair".  -> (want, bound), both float64"""
    x, e = z, zb
    if bias is not None:
        x = z + bias.double()
        e = e + HALF_F32 * x.abs()
    if glu:
        x1, x2, e1, e2 = x[:, 0::2], x[:, 1::2], e[:, 0::2], e[:, 1::2]
        s = x1 / (1.0 + torch.exp(-x1))
        es = 1.1 * e1 + 8 * HALF_F32 * s.abs()            # silu's slope is at most 1.1; expf (2 ulp), the add and the divide
        y = s * x2
        e = es * x2.abs() + s.abs() * e2 + es * e2 + HALF_F32 * y.abs()
    else:
        y = _act64(x, act)
        if act != "none":
            e = ACT_SLOPE[act] * e + HALF_F32 * y.abs() + (2.0 ** -22 * x.abs() if act == "gelu" else (2.0 ** -22 if act == "sigmoid" else 0.0))
        if scale is not None:
            y = y * scale.double()
            e = e * scale.double().abs() + HALF_F32 * y.abs()
        if resid is not None:
            y = y + resid.double()
            e = e + HALF_F32 * y.abs()
    if out == "bf16":
        e = e + half_ulp_bf16(y.abs() + e)          # of the binade the kernel's fp32 value can lie in
    elif out == "pair":
        e = e + PAIR_REL * y.abs()
    elif out != "f32":
        raise ValueError(out)
    return y, e


def h2_row_bounds(want, xb, h, r8):
    """the three tolerances of tests/test_gpu_h2.py for H2 output rows, per element: (got, bound) pairs for h + r8 and for h alone; xb = the
    bound on the fp32 value that was packed"""
    from tests.attention_cases import e4m3_half_ulp
    rem = ((want - h).abs() + xb) * 2048.0
    return ((h + r8, xb + e4m3_half_ulp(rem) / 2048.0), (h, xb + 2.0 ** -11 * (want.abs() + xb) + 2.0 ** -25))


# ------------------------------------------------------------------------------------------------ checks
def ratio(got, want, bound):
    """worst |got - want| / bound; NaN (an unwritten element, a NaN operand that leaked) counts as infinite; 0 / 0 as an exact zero"""
    err = (got.double() - want).abs()
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), torch.nan_to_num(err / bound, nan=0.0, posinf=float("inf")))
    return float(r.max())


def holds(got, want, bound):
    return bool(((got.double() - want).abs() <= bound).all())


def sample_rows(M, tile, cuts=(), every=0):
    """row sample for the float64 reference of a large case: the whole first and last m-tile and 64 rows either side of every internal row
    cut (plus every `every`-th row) -> sorted unique LongTensor"""
    last0 = (M - 1) // tile * tile
    idx = [torch.arange(0, min(tile, M)), torch.arange(last0, M)]
    for c in cuts:
        idx.append(torch.arange(max(0, c - 64), min(M, c + 64)))
    if every:
        idx.append(torch.arange(0, M, every))
    return torch.unique(torch.cat(idx))
