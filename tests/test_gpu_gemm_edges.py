"""`-m gpu`: every inference GEMM kernel form -- gemm_bf16.hip (128x128 on a 2- / 3-slot ring, 256x128 `m16`), gemm_x3.hip (16-wave 256x256:
plain `k64` with register or LDS epilogue, split product), gemm_pp.hip (ping-pong plain and x3, H2, the K-split tail and its reduce launch),
gemm_fp8.hip (per-row, block-scaled A, both block-scaled on either tile), gemm_f32.hip -- and the fused patch embedding (patch_embed.hip),
through the operator entry points (the patch embedding: through the drop-in modules' engine tap 0).

One harness (tests/gemm_cases.py holds the references, the epilogue and the bounds; tests/test_gemm_cases_cpu.py what a CPU can show of them):
  * footprint: every output is a padded `Out` (tests/gpu_util.py): 256 guard rows either side and pad columns N..ld-1 of a sentinel pattern
    that must survive, the rows themselves start as a NaN pattern of which nothing may be left;
  * pitches: lda = K + 8, ldw = K + 16, ldc = N + 8, ldr = N + 4 (in place: ldr = ldc); the operands' pad columns and 256 rows either side of
    them, inside the same allocation, are NaN;
  * every element against float64 of the values the kernel is given, normalised by T[m, n] = sum_k |a||w| (bounds: tests/gemm_cases.py); the
    tensor-wide bounds of the older operator tests are asserted beside them, unchanged;
  * dod_test_counter("form_*") says which kernel form(s) a case ran, and that no other did; a second launch is bit-identical.
The float64 reference and T cover every element (torch float64 on the device); d32, the distance of torch's fp32 CPU product that sets the fp32
bound, is measured on a row sample: the first and last m-tile, 64 rows either side of an internal row cut, and a stride through the rest.
Shapes are the smallest that reach each form on 256 CUs with ragged last tiles in M and N; on another device a case whose form depends on
the CU count does not assert its expected forms; every case holds the launches to dod_test_gemm_plan's steps for the device's own CU count.

Measured margins (MI355X, 256 CUs; the summary this module prints at teardown: worst error / bound per form, largest d32 and dist in T).
A form whose worst case has a bf16 output sits at 1.000 by construction: half a bf16 ulp is the bound and a rounding tie reaches it.
  form              worst   at                                  d32        dist
  bf16_128_r2       1.000   (129, 132, 64) gelu_bf16            1.14e-07
  bf16_128_r3       0.999   (255, 136, 320) gelu_bf16           1.11e-07
  bf16_m16          1.000   (3841, 1292, 64) gelu_bf16          1.48e-07
  k64               1.000   (4097, 1544, 64) gelu_bf16          1.50e-07
  k64+cut           1.000   (11521, 1536, 64) gelu_bf16         1.46e-07
  ppm               0.999   (10753, 768, 2048) gelu_bf16        3.16e-08
  ppm+split         1.000   (21800, 768, 384) bf16              8.09e-08
  f32               0.835   (130, 4, 96) lda=K+4 none           1.46e-07
  f32+ksplit        0.154   (50, 50, 768) sigmoid               6.25e-08
  x3_16w            1.000   (257, 264, 96) gelu_bf16            1.19e-07   6.42e-06
  x3_pp             1.000   (4097, 260, 96) gelu_bf16           1.32e-07   3.90e-06
  x3_pp+split       0.999   (2049, 516, 192) gelu_bf16          1.45e-07   2.95e-06
  h2                0.881   (257, 260, 32) gelu_pair            2.99e-07   1.47e-05
  h2+split          0.722   (2049, 516, 192) gelu_pair          2.90e-07   6.18e-06
  h2.fp16           0.990   (2049, 288, 160) gelu_h2
  fp8_rows          0.999   (257, 132, 64) gelu_bf16
  fp8mx_256x128     0.930   (257, 132, 256) gelu_bf16
  fp8mx2_256x128    0.926   (257, 132, 256) gelu_bf16
  fp8mx2_256x256    0.948   (4097, 516, 256) gelu_bf16
  patch_fused       0.781   (5, 224, 224) D=128 p=14 bf16x3     5.23e-08   1.04e-06
The 146 cases take about 7 s together, none more than 0.6 s."""
import collections
import functools

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from tests import gemm_cases as gc
from tests import gemm_dispatch_cases as dc
from tests.gpu_util import Out, guarded_input
from tests.test_gpu_fp8 import ACC_TOL, mx_ref, quant_ref
from tests.test_gpu_h2 import decode as h2_decode, pack as h2_pack

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
FORMS = ["bf16_128_r2", "bf16_128_r3", "bf16_m16", "k64", "ppm", "x3_16w", "x3_pp", "h2", "fp8_rows", "fp8mx_256x128", "fp8mx2_256x128",
         "fp8mx2_256x256", "f32", "patch_fused"]
COUNTERS = ["form_" + f for f in FORMS] + ["tail_splits", "rem_cuts", "f32_ksplits"]
WORST = {}       # form -> (error / bound, where)
DIST = {}        # (form, "d32" | "dist") -> (largest, where)
Ref = collections.namedtuple("Ref", "ops want T d32 exact dist")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    nat.lib()
    nat.check(nat.lib().dod_reserve_gemm_scratch(64 << 20))
    yield None
    for k in sorted(WORST):
        print(f"gemm worst  {k:<16s} {WORST[k][0]:.3f} of its per-element bound at {WORST[k][1]}")
    for k in sorted(DIST):
        print(f"gemm reference  {k[0]:<16s} largest {k[1]:<4s} {DIST[k][0]:.3e} T at {DIST[k][1]}")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


EXPECT_FORMS = True


@pytest.fixture(autouse=True)
def _expect_forms():
    global EXPECT_FORMS
    EXPECT_FORMS = True
    yield


def _needs_256_cus(what):
    """the forms a case expects are chosen by the CU count and its shapes are for 256: on another device _twice still holds the launches to the
    plan for THAT count (dod_test_gemm_plan), and every value check runs on whatever form that is"""
    global EXPECT_FORMS
    EXPECT_FORMS = _cus() == 256
    if not EXPECT_FORMS:
        print(f"{what} is chosen by the CU count: this device has {_cus()}, the expected forms are for 256 and are not asserted")


def _snap():
    L = nat.lib()
    return {c: L.dod_test_counter(c.encode()) for c in COUNTERS}


def _moved(before):
    after = _snap()
    return {c: after[c] - before[c] for c in COUNTERS if after[c] != before[c]}


def _note(form, kind, value, where):
    if value >= DIST.get((form, kind), (-1.0,))[0]:
        DIST[(form, kind)] = (value, where)


def _hold(form, where, got, want, bound):
    r = gc.ratio(got, want, bound)
    print(f"{form} {where}: worst element at {r:.3f} of its bound")
    if r >= WORST.get(form, (-1.0,))[0]:
        WORST[form] = (r, where)
    assert r <= 1.0, (form, where, r, int((~((got.double() - want).abs() <= bound)).sum()))


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def _footprint(where, out, inplace=False):
    assert out.guards_intact(), (where, "guard rows or pad columns written")
    if not inplace:
        assert out.unwritten() == 0, (where, "elements never written", out.unwritten())


def _twice(where, launch, expect, plan):
    """launch() -> tuple of Outs.  The first launch moves exactly the counters of `expect`, and exactly those that the steps of
    dod_test_gemm_plan for plan = (family, M, N, K, epilogue flags), this device's CU count and the fixture's 64 MiB add up to; the second
    launch is bit-identical"""
    before = _snap()
    outs = launch()
    torch.cuda.synchronize()
    moved = _moved(before)
    if EXPECT_FORMS:
        assert moved == expect, (where, "kernel forms launched", moved, "expected", expect)
    family, M, N, K, flags = plan
    steps = nat.gemm_plan(dc.FAMILY[family], M, N, K, flags, _cus(), 64 << 20)
    planned = {k: v for k, v in dc.counters_of(steps).items() if k in COUNTERS}
    assert planned == moved, (where, "planned", steps, "launched", moved)
    again = launch()
    torch.cuda.synchronize()
    for o, a in zip(outs, again):
        assert torch.equal(o.raw, a.raw), (where, "two launches differ")
    return outs


def _with_tailsplit(mode, fn):
    try:
        nat.set_option("tailsplit", mode)
        return fn()
    finally:
        nat.set_option("tailsplit", -1)


def _sample(M, cuts=()):
    return gc.sample_rows(M, 256, cuts, every=max(1, M // 256)) if M > 1024 else torch.arange(M)


# ================================================================================================ dod_op_linear, bf16 operands
@functools.lru_cache(maxsize=None)
def _ref_bf16(M, N, K, cuts=()):
    A, W = gc.operands(M, N, K)
    a, w = A.bfloat16(), W.bfloat16()
    ad, wd = a.to(DEV), w.to(DEV)
    want, T = gc.ref_plain(ad, wd)
    rows = _sample(M, cuts)
    wc, Tc = gc.ref_plain(a[rows], w)
    d32 = gc.dist_by_T(gc.f32_product([(a[rows], w)]), wc, Tc)
    return Ref((ad, wd), want, T, d32, None, None)


# epilogue -> (gemm_cases.epilogue keywords, output dtype)
EPI = {"none": (dict(), F32), "bf16": (dict(out="bf16"), BF16), "gelu_bf16": (dict(bias=1, act="gelu", out="bf16"), BF16),
       "ls_inplace": (dict(bias=1, scale=1, resid=1), F32), "ls_resid": (dict(bias=1, scale=1, resid=1), F32), "resid": (dict(bias=1, resid=1), F32),
       "inplace": (dict(bias=1, resid=1), F32), "swiglu": (dict(bias=1, glu=True, out="bf16"), BF16), "relu": (dict(bias=1, act="relu"), F32),
       "sigmoid": (dict(bias=1, act="sigmoid", scale=1, resid=1), F32), "gelu": (dict(bias=1, act="gelu", scale=1, resid=1), F32)}


def _epi_args(epi, M, N):
    """-> (keywords for gemm_cases.epilogue with device tensors, output dtype, output width, in place?)"""
    kw, dt = EPI[epi]
    bias, scale, resid = [t.to(DEV) for t in gc.epi_params(M, N)]
    kw = {k: ({"bias": bias, "scale": scale, "resid": resid}[k] if k in ("bias", "scale", "resid") else v) for k, v in kw.items()}
    return kw, dt, (N // 2 if kw.get("glu") else N), epi in ("ls_inplace", "inplace")


def _linear(form, in_dtype, ref, M, N, K, epi, expect, lda, ldw, where=None):
    """one dod_op_linear case: pitched NaN-padded operands, padded Out at ldc = width + 8, the residual at ldr = N + 4 (in place: the output)"""
    L, sp = nat.lib(), nat.stream_ptr()
    where = where or f"{(M, N, K)} {epi}"
    kw, dt, width, inplace = _epi_args(epi, M, N)
    Ad, Wd = guarded_input(ref.ops[0], ld=lda), guarded_input(ref.ops[1], ld=ldw)
    ldc = width + 8
    rd = None if inplace or "resid" not in kw else guarded_input(kw["resid"], ld=N + 4)
    act = "swiglu_pairs" if kw.get("glu") else kw.get("act", "none")

    def launch():
        o = Out(M, width, dt, ld=ldc)
        if inplace:
            o.data.copy_(kw["resid"])
        r = o.view if inplace else rd
        nat.check(L.dod_op_linear(in_dtype, nat.ptr(Ad), lda, nat.ptr(Wd), ldw, M, N, K, nat.ptr(kw.get("bias")), nat.ptr(kw.get("scale")),
                                  nat.ptr(r), (ldc if inplace else N + 4) if r is not None else 0, nat.ptr(o.view),
                                  nat.DOD_BF16 if dt == BF16 else nat.DOD_F32, ldc, nat.ACT[act], sp))
        return (o,)
    out, = _twice(where, launch, expect, ("bf16" if in_dtype == nat.DOD_BF16 else "f32", M, N, K, dc.epi_flags(epi, N, ldc)))
    _footprint(where, out, inplace)
    rel = gc.acc_rel(ref.d32)
    _note(form, "d32", ref.d32, where)
    want, bound = gc.epilogue(ref.want, rel * ref.T, **kw)
    _hold(form, where, out.data, want, bound)
    assert _rel(out.data, want) < (3e-6 if dt == F32 else (2 ** -8 if kw.get("glu") else 2 ** -7)), (where, "tensor-wide bound")
    return out


def _linear_bf16(form, M, N, K, epi, expect, cuts=(), tailsplit=0):
    ref = _ref_bf16(M, N, K, cuts)
    return _with_tailsplit(tailsplit, lambda: _linear(form, nat.DOD_BF16, ref, M, N, K, epi, expect, K + 8, K + 16))


SMALL_EPIS = ["none", "gelu_bf16", "ls_inplace", "resid"]


@pytest.mark.parametrize("epi", SMALL_EPIS)
@pytest.mark.parametrize("M,N,K", [(129, 132, 64), (129, 136, 128)])
def test_bf16_128x128_two_slot_ring(G, M, N, K, epi):
    """one and two K-tiles; N % 8 != 0 keeps the 16-byte bf16 drain off, N % 8 == 0 turns it on"""
    _linear_bf16("bf16_128_r2", M, N, K, epi, {"form_bf16_128_r2": 1})


@pytest.mark.parametrize("epi", SMALL_EPIS)
@pytest.mark.parametrize("M,N,K", [(129, 132, 192), (255, 136, 320)])
def test_bf16_128x128_three_slot_ring(G, M, N, K, epi):
    """three K-tiles = the ring depth; five: an odd count that wraps the ring"""
    _linear_bf16("bf16_128_r3", M, N, K, epi, {"form_bf16_128_r3": 1})


@pytest.mark.parametrize("epi", SMALL_EPIS)
@pytest.mark.parametrize("M,N,K", [(3841, 1292, 64), (3841, 1288, 192)])
def test_bf16_m16_small_path(G, M, N, K, epi):
    """176 tiles of 256x128, the last m-tile holds one row"""
    _linear_bf16("bf16_m16", M, N, K, epi, {"form_bf16_m16": 1})


@pytest.mark.parametrize("epi", SMALL_EPIS)
def test_bf16_m16_round_rule(G, epi):
    _needs_256_cus("the 256x128 tile at M >= 4096")
    _linear_bf16("bf16_m16", 4097, 768, 64, epi, {"form_bf16_m16": 1})


@pytest.mark.parametrize("M,N,K,epi", [(4097, 1544, 64, "gelu_bf16"), (4097, 1544, 64, "bf16"), (4097, 1540, 192, "gelu_bf16"), (4097, 1540, 192, "bf16"),
                                       (4097, 1544, 64, "ls_inplace"), (4097, 1544, 64, "none"), (4097, 1540, 192, "resid")])
def test_bf16_k64_register_and_lds_epilogue(G, M, N, K, epi):
    """16-wave 256x256x64: bf16 rows with N % 8 == 0 take the register epilogue (`epi_regmath` counts it), every other form the LDS-staged one"""
    L = nat.lib()
    c0 = L.dod_test_counter(b"epi_regmath")
    _linear_bf16("k64", M, N, K, epi, {"form_k64": 1})
    assert L.dod_test_counter(b"epi_regmath") - c0 == (2 if N % 8 == 0 and epi in ("gelu_bf16", "bf16") else 0)      # two launches


@pytest.mark.parametrize("epi", ["resid", "ls_inplace", "bf16", "none", "gelu_bf16"])
def test_bf16_k64_rem_cut(G, epi):
    """46 x 6 = 276 tiles: the 20 of the second round are cut off at row 10752 and run as 128x128 tiles; every per-row pointer of the second
    launch is shifted by 10752 rows of ITS pitch (gemm_epi_rows)"""
    _needs_256_cus("the cut-off last round")
    _linear_bf16("k64+cut", 11521, 1536, 64, epi, {"form_k64": 1, "form_bf16_128_r2": 1, "rem_cuts": 1}, cuts=(10752,))


@pytest.mark.parametrize("epi", ["ls_inplace", "bf16", "resid", "none", "gelu_bf16"])
def test_bf16_ping_pong(G, epi):
    _needs_256_cus("the ping-pong kernel for a long-K narrow GEMM")
    _linear_bf16("ppm", 10753, 768, 2048, epi, {"form_ppm": 1})


@pytest.mark.parametrize("epi", ["ls_inplace", "bf16", "resid", "none"])
def test_bf16_tail_split(G, epi):
    """86 x 3 = 258 tiles, two more than one round: the last m-tile's 40 rows (21760..21799) are K-split two ways on the ping-pong kernel and
    reduced; the main rows take the 16-wave kernel"""
    _needs_256_cus("the tail split")
    _linear_bf16("ppm+split", 21800, 768, 384, epi, {"form_k64": 1, "form_ppm": 1, "tail_splits": 1}, cuts=(21760,), tailsplit=2)


@pytest.mark.parametrize("form,M,N,K", [("bf16_128_r2", 129, 136, 128), ("bf16_m16", 3841, 1288, 192), ("k64", 4097, 1544, 64)])
def test_bf16_swiglu_pairs(G, form, M, N, K):
    """N = 2F interleaved (x1, x2) columns -> F gated columns at ldc = F + 8"""
    _linear_bf16(form, M, N, K, "swiglu", {"form_" + form: 1})


def test_bf16_linear_rejects_pitches_it_cannot_honour(G):
    """lda, ldw % 8 and ldc, ldr % 4 are what the kernels' 16-byte loads and float4 stores need: anything else is DOD_ERR_INVALID, not a result"""
    L, sp = nat.lib(), nat.stream_ptr()
    A = torch.zeros(64, 80, device=DEV, dtype=BF16)
    W = torch.zeros(64, 80, device=DEV, dtype=BF16)
    o = Out(64, 64, F32, ld=72)
    r = torch.zeros(64, 72, device=DEV)
    for lda, ldw, ldc, ldr in ((68, 80, 72, 0), (72, 76, 72, 0), (72, 80, 70, 0), (72, 80, 72, 66)):
        before = _snap()
        with pytest.raises(ValueError):
            nat.check(L.dod_op_linear(nat.DOD_BF16, nat.ptr(A), lda, nat.ptr(W), ldw, 64, 64, 64, None, None, nat.ptr(r) if ldr else None, ldr,
                                      nat.ptr(o.view), nat.DOD_F32, ldc, 0, sp))
        assert _moved(before) == {}
    torch.cuda.synchronize()
    assert o.guards_intact() and o.unwritten() == 64 * 64


# ================================================================================================ dod_op_linear, fp32 operands
@functools.lru_cache(maxsize=None)
def _ref_f32(M, N, K):
    A, W = gc.operands(M, N, K)
    ad, wd = A.to(DEV), W.to(DEV)
    want, T = gc.ref_plain(ad, wd)
    wc, Tc = gc.ref_plain(A, W)
    return Ref((ad, wd), want, T, gc.dist_by_T(gc.f32_product([(A, W)]), wc, Tc), None, None)


@pytest.mark.parametrize("epi", ["none", "relu", "gelu", "sigmoid", "ls_inplace"])
@pytest.mark.parametrize("pad", [5, 4], ids=["scalar-loads", "vector-loads"])
@pytest.mark.parametrize("M,N,K", [(65, 68, 17), (130, 4, 96)])
def test_f32_linear(G, M, N, K, pad, epi):
    """gemm_f32.hip: a pitch of K + 5 rules out float4 loads, K + 4 keeps them (K = 17: a ragged last k-tile either way)"""
    _linear("f32", nat.DOD_F32, _ref_f32(M, N, K), M, N, K, epi, {"form_f32": 1}, K + pad, K + pad, where=f"{(M, N, K)} lda=K+{pad} {epi}")


def test_f32_linear_k_split(G):
    try:
        nat.set_option("f32_ksplit", 1)
        _linear("f32+ksplit", nat.DOD_F32, _ref_f32(50, 50, 768), 50, 50, 768, "sigmoid", {"form_f32": 1, "f32_ksplits": 1}, 768 + 4, 768 + 8)
    finally:
        nat.set_option("f32_ksplit", -1)


def test_f32_detector_head_layout(G):
    """class head (N = 91) and box head (N = 4, sigmoid, starting at column 91: 4-byte aligned only) into ONE [M, 95] buffer at ldc = 95, as
    the forward writes `det`: neither launch disturbs the other's columns"""
    L, sp = nat.lib(), nat.stream_ptr()
    M, K, C = 130, 96, 91
    rc, rb = _ref_f32(M, C, K), _ref_f32(M, 4, K)
    bc, bb = gc.normal(("head.bc",), (C,)).to(DEV), gc.normal(("head.bb",), (4,)).to(DEV)
    Ac, Ab = guarded_input(rc.ops[0], ld=K + 4), guarded_input(rb.ops[0], ld=K + 4)
    Wc, Wb = guarded_input(rc.ops[1], ld=K + 4), guarded_input(rb.ops[1], ld=K + 4)

    def cls(o):
        nat.check(L.dod_op_linear(nat.DOD_F32, nat.ptr(Ac), K + 4, nat.ptr(Wc), K + 4, M, C, K, nat.ptr(bc), None, None, 0, nat.ptr(o.view), nat.DOD_F32, C + 4, 0, sp))

    def box(o):
        nat.check(L.dod_op_linear(nat.DOD_F32, nat.ptr(Ab), K + 4, nat.ptr(Wb), K + 4, M, 4, K, nat.ptr(bb), None, None, 0, nat.ptr(o.view[:, C:]), nat.DOD_F32, C + 4,
                                  nat.ACT["sigmoid"], sp))
    o = Out(M, C + 4, F32)
    before = _snap()
    cls(o)
    torch.cuda.synchronize()
    assert _moved(before) == {"form_f32": 1}
    first = o.raw.clone()
    assert o.guards_intact() and o.unwritten() == 4 * M, "the class head wrote (or left) something outside its 91 columns"
    box(o)
    torch.cuda.synchronize()
    assert o.guards_intact() and o.unwritten() == 0
    assert torch.equal(o.raw[:, :C], first[:, :C]), "the box head disturbed the class columns"
    boxes = o.raw[:, C:].clone()
    cls(o)
    torch.cuda.synchronize()
    assert torch.equal(o.raw[:, :C], first[:, :C]) and torch.equal(o.raw[:, C:], boxes), "the class head disturbed the box columns"
    for name, ref, bias, act, got in (("class", rc, bc, "none", o.data[:, :C]), ("box", rb, bb, "sigmoid", o.data[:, C:])):
        want, bound = gc.epilogue(ref.want, gc.acc_rel(ref.d32) * ref.T, bias=bias, act=act)
        _hold("f32", f"head {name}", got, want, bound)
        assert _rel(got, want) < 3e-6


# ================================================================================================ dod_op_linear_x3 / dod_op_linear_h2
@functools.lru_cache(maxsize=None)
def _ref_x3(M, N, K):
    A, W = gc.operands(M, N, K)
    (ah, al), (wh, wl) = gc.split_pair(A), gc.split_pair(W)
    A2, W2 = torch.cat([ah, al], 1).bfloat16().to(DEV), torch.cat([wh, wl], 1).bfloat16().to(DEV)
    defined, T = gc.ref_x3(ah.to(DEV), al.to(DEV), wh.to(DEV), wl.to(DEV))
    exact = A.to(DEV).double() @ W.to(DEV).double().t()
    rows = _sample(M)
    dc, Tc = gc.ref_x3(ah[rows], al[rows], wh, wl)
    d32 = gc.dist_by_T(gc.f32_product([(ah[rows], wl), (al[rows], wh), (ah[rows], wh)]), dc, Tc)
    return Ref((A2, W2), defined, T, d32, exact, gc.dist_by_T(defined, exact, T))


@functools.lru_cache(maxsize=None)
def _ref_h2(M, N, K):
    A, W = gc.operands(M, N, K)
    Ab, _ = h2_pack(A.to(DEV))
    Wb, wexp = h2_pack(W.to(DEV), weight=True)
    ap, wp = h2_decode(Ab, K), h2_decode(Wb, K, wexp)
    defined, T = gc.ref_h2([t.to(DEV) for t in ap], [t.to(DEV) for t in wp])
    exact = A.to(DEV).double() @ W.to(DEV).double().t()
    rows = _sample(M)
    apr = [t[rows] for t in ap]
    dc, Tc = gc.ref_h2(apr, wp)
    d32 = gc.dist_by_T(gc.f32_product([(apr[1], wp[2]), (apr[2], wp[1]), (apr[0], wp[0])]), dc, Tc)
    return Ref((Ab, Wb, wexp), defined, T, d32, exact, gc.dist_by_T(defined, exact, T))


# epilogue -> (gemm_cases.epilogue keywords, output layout: 0 fp32, 1 bf16, 2 bf16 pair, 3 H2 rows)
SPLIT_EPI = {"none": (dict(), 0), "ls_resid": (dict(bias=1, scale=1, resid=1), 0), "gelu_pair": (dict(bias=1, act="gelu", out="pair"), 2),
             "gelu_bf16": (dict(bias=1, act="gelu", out="bf16"), 1), "gelu_h2": (dict(bias=1, act="gelu"), 3)}


def _split_case(family, form, M, N, K, epi, expect, tailsplit=0):
    """dod_op_linear_x3 / dod_op_linear_h2 (the entries fix the operand pitches): padded Out, the residual at ldr = N + 4; against the float64
    "defined" product at the fp32-accumulation bound and against the exact product of the fp32 inputs at the split bound"""
    L, sp = nat.lib(), nat.stream_ptr()
    where = f"{(M, N, K)} {epi}"
    ref = (_ref_x3 if family == "x3" else _ref_h2)(M, N, K)
    kw, layout = SPLIT_EPI[epi]
    bias, scale, resid = [t.to(DEV) for t in gc.epi_params(M, N)]
    kw = {k: ({"bias": bias, "scale": scale, "resid": resid}[k] if k in ("bias", "scale", "resid") else v) for k, v in kw.items()}
    Ad, Wd = guarded_input(ref.ops[0], pad=float("nan") if family == "x3" else 0x7F), ref.ops[1]
    rd = guarded_input(resid, ld=N + 4) if "resid" in kw else None
    dt, width = {0: (F32, N), 1: (BF16, N), 2: (BF16, 2 * N), 3: (U8, 4 * N)}[layout]
    ld = width + (16 if layout == 3 else 8)
    ldc = ld // 2 if layout == 3 else ld            # H2 rows: the pitch counts bf16 elements

    def launch(unwritten=None):
        o = Out(M, width, dt, unwritten, ld=ld)
        if family == "x3":
            nat.check(L.dod_op_linear_x3(nat.ptr(Ad), nat.ptr(Wd), M, N, K, nat.ptr(kw.get("bias")), nat.ptr(kw.get("scale")), nat.ptr(rd), N + 4 if rd is not None else 0,
                                         nat.ptr(o.view), layout, ldc, nat.ACT[kw.get("act", "none")], sp))
        else:
            nat.check(L.dod_op_linear_h2(nat.ptr(Ad), nat.ptr(Wd), nat.ptr(ref.ops[2]), M, N, K, nat.ptr(kw.get("bias")), nat.ptr(kw.get("scale")), nat.ptr(rd),
                                         N + 4 if rd is not None else 0, nat.ptr(o.view), layout, ldc, nat.ACT[kw.get("act", "none")], sp))
        return (o,)
    out, = _with_tailsplit(tailsplit, lambda: _twice(where, launch, expect, (family, M, N, K, dc.epi_flags(epi, N, ldc))))
    _footprint(where, out, inplace=layout == 3)
    if layout == 3:      # any byte is a valid half of an fp16 value: an unwritten one shows when the buffer starts as another pattern
        assert torch.equal(_with_tailsplit(tailsplit, lambda: launch(0x5A))[0].raw, out.raw), (where, "bytes never written")
    _note(form, "d32", ref.d32, where)
    _note(form, "dist", ref.dist, where)
    want_d, bound_d = gc.epilogue(ref.want, gc.acc_rel(ref.d32) * ref.T, **kw)
    want_x, bound_x = gc.epilogue(ref.exact, gc.split_rel(ref.dist) * ref.T, **kw)
    wide_d, wide_x = (3e-5, 3e-5) if family == "x3" else (2e-6, 5e-5)        # tests/test_gpu_x3.py, tests/test_gpu_h2.py
    if layout == 3:
        h, m8, r8 = [t.to(DEV) for t in h2_decode(out.data, N)]
        assert torch.equal(m8, h.float().clamp(-448, 448).to(torch.float8_e4m3fn).double()), (where, "e4m3(h) bytes")
        xb = bound_d                              # the bound on the fp32 value that is packed
        for (got, b), name in zip(gc.h2_row_bounds(want_d, xb, h, r8), ("", ".fp16")):
            _hold(form + name, where, got, want_d, b)
        assert _rel(h, want_x) < 2 ** -11 and _rel(h + r8, want_x) < 5e-5 and _rel(m8, want_x) < 2 ** -3
        return
    got = out.data.double()
    if layout == 2:
        got = got[:, :N] + got[:, N:]
    _hold(form, where + " vs defined", got, want_d, bound_d)
    _hold(form, where + " vs exact", got, want_x, bound_x)
    if layout == 1:
        assert _rel(got, want_x) < 2 ** -7
    else:
        assert _rel(got, want_x) < wide_x and (layout == 2 or _rel(got, want_d) < wide_d)      # a pair row carries 16 bits: 2^-17 > 2e-6


X3_EPIS = ["none", "ls_resid", "gelu_pair", "gelu_bf16"]


@pytest.mark.parametrize("epi", X3_EPIS)
@pytest.mark.parametrize("M,N,K", [(257, 260, 32), (257, 264, 96), (2049, 516, 160)])
def test_x3_16_wave(G, M, N, K, epi):
    """one, three and five 32-wide K-tiles; a one-row last m-tile; ragged second / third n-tile"""
    _split_case("x3", "x3_16w", M, N, K, epi, {"form_x3_16w": 1})


@pytest.mark.parametrize("epi", X3_EPIS)
def test_x3_ping_pong(G, epi):
    _split_case("x3", "x3_pp", 4097, 260, 96, epi, {"form_x3_pp": 1})


@pytest.mark.parametrize("epi", X3_EPIS)
def test_x3_underfilled_k_split(G, epi):
    """9 x 3 = 27 tiles of an underfilled single round: every tile K-split two ways (no main launch) and reduced"""
    _needs_256_cus("the K-split of an underfilled grid")
    _split_case("x3", "x3_pp+split", 2049, 516, 192, epi, {"form_x3_pp": 1, "tail_splits": 1}, tailsplit=1)


H2_EPIS = ["none", "ls_resid", "gelu_pair"]


@pytest.mark.parametrize("epi", H2_EPIS)
@pytest.mark.parametrize("M,N,K", [(257, 260, 32), (257, 264, 96), (2049, 516, 160), (4097, 260, 96)])
def test_h2(G, M, N, K, epi):
    _split_case("h2", "h2", M, N, K, epi, {"form_h2": 1})


@pytest.mark.parametrize("M,N,K", [(257, 288, 96), (2049, 288, 160)])
def test_h2_rows_out(G, M, N, K):
    """layout 3 (N % 32 == 0): H2 operand rows, 4N bytes at a pitch of 4N + 16"""
    _split_case("h2", "h2", M, N, K, "gelu_h2", {"form_h2": 1})


@pytest.mark.parametrize("epi", H2_EPIS)
def test_h2_underfilled_k_split(G, epi):
    _needs_256_cus("the K-split of an underfilled grid")
    _split_case("h2", "h2+split", 2049, 516, 192, epi, {"form_h2": 1, "tail_splits": 1}, tailsplit=1)


def test_split_and_fp8_linears_reject_what_they_cannot_honour(G):
    """an fp32 output or residual pitch that is no multiple of 4 floats, H2 rows out with N % 32 != 0 or a pitch under 2N, fp8 operand
    pitches that are no multiple of 16 bytes: DOD_ERR_INVALID, no launch, nothing written"""
    L, sp = nat.lib(), nat.stream_ptr()
    M, N, K = 64, 64, 64
    o = Out(M, 4 * N, U8, ld=4 * N + 16)
    z = torch.zeros(M, 4 * K + 64, dtype=U8, device=DEV)
    f = torch.ones(M, device=DEV)
    calls = [lambda: L.dod_op_linear_x3(nat.ptr(z), nat.ptr(z), M, N, K, None, None, None, 0, nat.ptr(o.view), 0, N + 2, 0, sp),
             lambda: L.dod_op_linear_x3(nat.ptr(z), nat.ptr(z), M, N, K, None, None, nat.ptr(z), N + 2, nat.ptr(o.view), 0, N + 8, 0, sp),
             lambda: L.dod_op_linear_h2(nat.ptr(z), nat.ptr(z), nat.ptr(z), M, N, K, None, None, None, 0, nat.ptr(o.view), 0, N + 2, 0, sp),
             lambda: L.dod_op_linear_h2(nat.ptr(z), nat.ptr(z), nat.ptr(z), M, 48, K, None, None, None, 0, nat.ptr(o.view), 3, 2 * 48 + 8, 0, sp),
             lambda: L.dod_op_linear_h2(nat.ptr(z), nat.ptr(z), nat.ptr(z), M, N, K, None, None, None, 0, nat.ptr(o.view), 3, 2 * N - 8, 0, sp),
             lambda: L.dod_op_linear_fp8(nat.ptr(z), K + 8, nat.ptr(f), nat.ptr(z), K + 16, nat.ptr(f), M, N, K, None, None, None, 0, nat.ptr(o.view), nat.DOD_F32, N + 8, 0, sp),
             lambda: L.dod_op_linear_fp8(nat.ptr(z), K + 16, nat.ptr(f), nat.ptr(z), K + 8, nat.ptr(f), M, N, K, None, None, None, 0, nat.ptr(o.view), nat.DOD_F32, N + 8, 0, sp),
             lambda: L.dod_op_linear_fp8(nat.ptr(z), K + 16, nat.ptr(f), nat.ptr(z), K + 16, nat.ptr(f), M, N, K, None, None, None, 0, nat.ptr(o.view), nat.DOD_F32, N + 6, 0, sp)]
    for i, call in enumerate(calls):
        before = _snap()
        with pytest.raises(ValueError):
            nat.check(call())
        assert _moved(before) == {}, i
    torch.cuda.synchronize()
    assert o.guards_intact() and o.unwritten() == M * 4 * N


# ================================================================================================ fp8
def _varied(M, N, K):
    """blocks of very different magnitude along K in rows of A and of W (tests/test_gpu_fp8.py)"""
    A, W = gc.operands(M, N, K)
    A[:, :K // 2] *= 40.0
    A[1::3] *= 1e-2
    W[:, K // 4:K // 2] *= 25.0
    W[2::5, :64] *= 1e-3
    return A, W


@functools.lru_cache(maxsize=None)
def _ref_fp8(kind, M, N, K):
    """kind "rows": per-row scales on both; "mx": block-scaled A; "mx2": both block-scaled.  ops = (A bytes, A scales, W bytes, W scales)"""
    A, W = _varied(M, N, K)
    if kind == "rows":
        qa, sa = quant_ref(A)
        a, a_sc = gc.dequant_rows(qa, sa), sa
    else:
        qa, a_sc, _ = mx_ref(A)
        a = gc.dequant_mx(qa, a_sc)
    if kind == "mx2":
        qw, w_sc, _ = mx_ref(W)
        w = gc.dequant_mx(qw, w_sc)
    else:
        qw, w_sc = quant_ref(W)
        w = gc.dequant_rows(qw, w_sc)
    want, T = gc.ref_plain(a.to(DEV), w.to(DEV))
    return Ref((qa.view(U8).to(DEV), a_sc.to(DEV), qw.view(U8).to(DEV), w_sc.to(DEV)), want, T, None, None, None)


def _fp8_case(kind, form, M, N, K, epi):
    L, sp = nat.lib(), nat.stream_ptr()
    where = f"{(M, N, K)} {kind} {epi}"
    ref = _ref_fp8(kind, M, N, K)
    kw, dt, width, inplace = _epi_args(epi, M, N)
    qa, sa, qw, sw = ref.ops
    lda, ldw, ldc = K + 16, K + 32, N + 8
    Ad, Wd = guarded_input(qa, ld=lda, pad=0x7F), guarded_input(qw, ld=ldw, pad=0x7F)
    sad = guarded_input(sa[:, None], pad=float("nan"))[:, 0] if kind == "rows" else guarded_input(sa, pad=0xFF)
    rd = guarded_input(kw["resid"], ld=N + 4) if "resid" in kw else None
    odt = nat.DOD_BF16 if dt == BF16 else nat.DOD_F32

    def launch():
        o = Out(M, N, dt, ld=ldc)
        common = (M, N, K, nat.ptr(kw.get("bias")), nat.ptr(kw.get("scale")), nat.ptr(rd), N + 4 if rd is not None else 0, nat.ptr(o.view), odt, ldc,
                  nat.ACT[kw.get("act", "none")])
        if kind == "rows":
            nat.check(L.dod_op_linear_fp8(nat.ptr(Ad), lda, nat.ptr(sad), nat.ptr(Wd), ldw, nat.ptr(sw), *common, sp))
        elif kind == "mx":
            nat.check(L.dod_op_linear_fp8_mx(nat.ptr(Ad), lda, nat.ptr(sad), nat.ptr(Wd), ldw, nat.ptr(sw), *common, sp))
        else:
            nat.check(L.dod_op_linear_fp8_mx2(nat.ptr(Ad), lda, nat.ptr(sad), nat.ptr(Wd), ldw, nat.ptr(sw), *common, None, sp))
        return (o,)
    out, = _twice(where, launch, {"form_" + form: 1}, ("fp8", M, N, K, dc.epi_flags(kind if epi == "none" else f"{kind}_{epi}", N, ldc)))
    _footprint(where, out)
    want, bound = gc.epilogue(ref.want, ACC_TOL * ref.T, **kw)
    _hold(form, where, out.data, want, bound)
    assert _rel(out.data, want) < (ACC_TOL if dt == F32 else 2 ** -7)


@pytest.mark.parametrize("epi", ["none", "gelu_bf16", "ls_resid"])
@pytest.mark.parametrize("kind,form,M,N,K", [("rows", "fp8_rows", 257, 132, 64), ("mx", "fp8mx_256x128", 257, 132, 256), ("mx2", "fp8mx2_256x128", 257, 132, 256),
                                             ("mx2", "fp8mx2_256x256", 4097, 516, 256)])
def test_fp8(G, kind, form, M, N, K, epi):
    _fp8_case(kind, form, M, N, K, epi)


def test_fp8_glu_quantised_output(G):
    """weights_in of the fp8 SwiGLU MLP through dod_op_linear_fp8_mx2: gated e4m3 byte rows at ldq = F + 16 and their e8m0 bytes, which start as
    0xFF.  Values: the criteria of tests/test_gpu_fp8.py's test of this epilogue, unchanged; here the footprint and the pitch"""
    from oracle import dinodet_oracle as orc
    from tests.cases import rel_l2
    from tests.test_gpu_fp8 import F_silu
    L, sp = nat.lib(), nat.stream_ptr()
    M, F, K = 257, 128, 256
    A, W = gc.operands(M, 2 * F, K, "glu")
    bias = gc.normal(("glu.b",), (2 * F,), 0.1)
    qa, la, _ = mx_ref(A)
    qw, lw, _ = mx_ref(W)
    z = gc.dequant_mx(qa, la) @ gc.dequant_mx(qw, lw).t() + bias.double()
    ref = (F_silu(z[:, 0::2]) * z[:, 1::2]).float()
    Ad, Wd = guarded_input(qa.view(U8).to(DEV), ld=K + 16, pad=0x7F), guarded_input(qw.view(U8).to(DEV), ld=K + 32, pad=0x7F)
    lad, lwd, bd = guarded_input(la.to(DEV), pad=0xFF), lw.to(DEV), bias.to(DEV)

    def launch():
        oq, ob = Out(M, F, U8, ld=F + 16), Out(M, F // 32, U8, unwritten=0xFF)
        nat.check(L.dod_op_linear_fp8_mx2(nat.ptr(Ad), K + 16, nat.ptr(lad), nat.ptr(Wd), K + 32, nat.ptr(lwd), M, 2 * F, K, nat.ptr(bd), None, None, 0,
                                          nat.ptr(oq.view), nat.DOD_BF16, F + 16, 0, nat.ptr(ob.view), sp))
        return oq, ob
    oq, ob = _twice("glu mx2", launch, {"form_fp8mx2_256x128": 1}, ("fp8", M, 2 * F, K, dc.epi_flags("mx2_glu", 2 * F, F + 16)))
    assert oq.guards_intact() and ob.guards_intact() and ob.unwritten() == 0, "scale bytes left at 0xFF, or a guard written"
    eb = ob.data.cpu().reshape(M, 2, F // 64).permute(0, 2, 1).reshape(M, F // 32).long()
    deq = (gc.E4M3_LUT[oq.data.cpu().long()].float().reshape(M, F // 32, 32) * torch.pow(torch.tensor(2.0), (eb - 127).float())[..., None]).reshape(M, F)
    assert bool(torch.isfinite(deq).all()), "a byte row element left at the unwritten pattern (e4m3 NaN)"
    e_ref, e_orc = rel_l2(deq.numpy(), ref.numpy()), rel_l2(deq.numpy(), orc._q8_mx(ref).numpy())
    same = float((eb == orc._mx_scales(ref)).float().mean())
    print(f"glu + mx2 epilogue: vs exact gate {e_ref:.2e}, vs the oracle's quantisation of it {e_orc:.2e}, equal scale bytes {same:.4f}")
    assert e_ref < 4e-2 and e_orc < 1e-2 and same > 0.995


# ================================================================================================ fused patch embedding (patch_embed.hip)
def _pe_cfg(D=128, heads=2, p=14, pos_grid=5):
    from dinov2_od_amd.config import BackboneConfig
    return BackboneConfig(hidden=D, layers=1, heads=heads, swiglu=False, patch=p, pos_grid=pos_grid, lora_r=2, lora_alpha=1.0, target_dim=0)


def _pe_check(where, precision, sd, bb, vals, emb):
    """vals: fp32 pixel values [B, 3, H, W] as the kernel forms them (CPU); emb: the tap [B, N, D].  Against the float64 convolution of the
    bf16-rounded pixels and weights (bf16) or the three-term product of their hi / lo halves (bf16x3), + bias + position row"""
    p, D = bb.patch, bb.hidden
    B, _, H, W = vals.shape
    gh, gw = H // p, W // p
    Np = gh * gw
    a = vals[:, :, :gh * p, :gw * p].reshape(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * Np, 3 * p * p)
    w = torch.from_numpy(sd["dino.embeddings.patch_embeddings.projection.weight"]).reshape(D, 3 * p * p)
    bias = torch.from_numpy(sd["dino.embeddings.patch_embeddings.projection.bias"])
    pos = torch.from_numpy(sd["dino.embeddings.position_embeddings"])[0]
    cls = torch.from_numpy(sd["dino.embeddings.cls_token"])[0, 0]
    if precision == "bf16":
        ab, wb = gc.bf(a), gc.bf(w)
        want, T = gc.ref_plain(ab, wb)
        d32 = gc.dist_by_T(gc.f32_product([(ab, wb)]), want, T)
    else:
        (ah, al), (wh, wl) = gc.split_pair(a), gc.split_pair(w)
        want, T = gc.ref_x3(ah, al, wh, wl)
        d32 = gc.dist_by_T(gc.f32_product([(ah, wl), (al, wh), (ah, wh)]), want, T)
        dist = gc.dist_by_T(want, a.double() @ w.double().t(), T)
        _note("patch_fused", "dist", dist, where)
    _note("patch_fused", "d32", d32, where)
    square = gh == gw == bb.pos_grid and H == W                 # the native grid: the table is used as it is; every other case has pos = 0
    posrows = pos[1:].repeat(B, 1) if square else torch.zeros(B * Np, D)
    assert square or not bool(pos.any())
    want, bound = gc.epilogue(want, gc.acc_rel(d32) * T, bias=bias, resid=posrows)
    got = emb.cpu()
    assert torch.equal(got[:, 0], (cls + pos[0]).expand(B, D)), (where, "CLS rows")
    _hold("patch_fused", where, got[:, 1:].reshape(B * Np, D), want, bound)
    assert _rel(got[:, 1:].reshape(B * Np, D), want) < (3e-6 if precision == "bf16" else 3e-5)
    if precision == "bf16x3":
        exact, xb = gc.epilogue(a.double() @ w.double().t(), gc.split_rel(dist) * T, bias=bias, resid=posrows)
        _hold("patch_fused", where + " vs exact", got[:, 1:].reshape(B * Np, D), exact, xb)


def _pe_state(bb, zero_pos):
    from dinov2_od_amd import synth
    sd = synth.backbone_state_dict(bb, seed=1, prefix="")
    if zero_pos:
        sd["dino.embeddings.position_embeddings"] = np.zeros_like(sd["dino.embeddings.position_embeddings"])      # its bicubic resize is then exactly zero
    return sd


PE_CASES = [(1, 14, 28, 128, 2, 14, 5), (3, 70, 98, 128, 2, 14, 5), (5, 84, 70, 128, 2, 14, 5), (2, 75, 100, 128, 2, 14, 5), (5, 224, 224, 128, 2, 14, 5),
            (3, 70, 98, 192, 3, 14, 5), (2, 64, 96, 128, 2, 16, 4), (2, 70, 70, 128, 2, 14, 5)]


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("B,H,W,D,heads,p,pos_grid", PE_CASES)
def test_patch_embed_fp32_pixels(G, B, H, W, D, heads, p, pos_grid, precision):
    """two patches; non-square and less than one 128-row tile; a tile that straddles images; H and W no multiples of p (the cropped remainder
    must not enter the sum); 10 patch tiles (the second XCD group of 8 partly empty); a ragged second n-tile (D = 192); p = 16; and the square
    native grid, the one case with a non-zero position table"""
    from dinov2_od_amd import synth
    from dinov2_od_amd.models import DINOv2Backbone
    from tests import gpu_util
    bb = _pe_cfg(D, heads, p, pos_grid)
    sd = _pe_state(bb, zero_pos=not (H == W == p * pos_grid))
    m = DINOv2Backbone("micro", lora_r=bb.lora_r, lora_alpha=1.0, target_dim=None, pretrained=False, precision=precision, config=bb)
    gpu_util.load_np_state(m, sd)
    m = m.to(DEV).eval()
    x = torch.from_numpy(synth.make_pixels(B, H, W, seed=3))
    N = (H // p) * (W // p) + 1
    tap = m._get_engine().set_tap(0, (B, N, D), "cuda:0")
    before = _snap()
    m(x.to(DEV))
    torch.cuda.synchronize()
    moved = _moved(before)
    assert moved.get("form_patch_fused") == 1, moved
    first = tap.clone()
    _pe_check(f"{(B, H, W)} D={D} p={p} {precision}", precision, sd, bb, x, first)
    m(x.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(tap, first), "two launches differ"


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
@pytest.mark.parametrize("B,H,W", [(3, 70, 98), (2, 75, 101)])
def test_patch_embed_u8_pixels(G, B, H, W, precision):
    """uint8 HWC through forward_packed_u8 (an odd width: byte loads need no alignment): float64 of fp32(byte) / 255 rounded as the kernel rounds it"""
    from dinov2_od_amd import synth
    from dinov2_od_amd.models import DINOv2ObjectDetector
    from tests import cases, gpu_util
    bb, dc = _pe_cfg(), cases.dec_cfg(True)
    sd = synth.detector_state_dict(bb, dc, seed=1)
    sd["backbone.dino.embeddings.position_embeddings"] = np.zeros_like(sd["backbone.dino.embeddings.position_embeddings"])
    m = DINOv2ObjectDetector(num_classes=dc.num_classes, dino_model_name="custom", lora_r=bb.lora_r, lora_alpha=bb.lora_alpha, hidden_dim=dc.hidden_dim,
                             num_queries=dc.num_queries, nheads=dc.nheads, num_decoder_layers=dc.num_layers, dim_feedforward=dc.dim_feedforward,
                             n_points=dc.n_points, use_deformable=dc.use_deformable, pretrained=False, precision=precision, backbone_config=bb)
    gpu_util.load_np_state(m, sd)
    m = m.to(DEV).eval()
    u8 = torch.from_numpy(np.random.default_rng(gc.seed_of("u8", B, H, W)).integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    N = (H // 14) * (W // 14) + 1
    tap = m._get_engine().set_tap(0, (B, N, 128), "cuda:0")
    before = _snap()
    m.forward_packed_u8(u8.to(DEV))
    torch.cuda.synchronize()
    assert _moved(before).get("form_patch_fused") == 1
    vals = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()          # ToTensor in fp32, as the load stage does it
    bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.dino.embeddings.")}
    _pe_check(f"u8 {(B, H, W)} {precision}", precision, bsd, bb, vals, tap.clone())
