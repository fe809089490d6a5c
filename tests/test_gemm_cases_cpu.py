"""CPU: what can be shown of the GEMM edge harness (tests/gemm_cases.py, tests/gpu_util.Out) without a GPU.  A stand-in kernel -- fp32
accumulation of the same operands, 32 products per step, the three-term form for x3 -- passes every bound; each planted defect fails:
one element off by 2^-12 T, one x3 cross term dropped for ONE 32-wide K-tile at K = 3072, one e8m0 byte off by one on one block, a write
into a pad column, into a guard row, a row left unwritten, and a NaN pad column of A that leaks into the sum."""
import pytest
import torch

from tests import gemm_cases as gc
from tests.gpu_util import GUARD, PATTERN, Out, guarded_input

F32, BF16 = torch.float32, torch.bfloat16


def _bf16_case(M, N, K):
    A, W = gc.operands(M, N, K)
    a, w = gc.bf(A), gc.bf(W)
    want, T = gc.ref_plain(a, w)
    d32 = gc.dist_by_T(gc.f32_product([(a, w)]), want, T)
    return a, w, want, T, d32


def _x3_case(M, N, K):
    A, W = gc.operands(M, N, K)
    (ah, al), (wh, wl) = gc.split_pair(A), gc.split_pair(W)
    terms = [(ah, wl), (al, wh), (ah, wh)]
    defined, T = gc.ref_x3(ah, al, wh, wl)
    exact = A.double() @ W.double().t()
    return terms, defined, exact, T, gc.dist_by_T(gc.f32_product(terms), defined, T), gc.dist_by_T(defined, exact, T)


def _mx(x):
    from tests.test_gpu_fp8 import mx_ref
    q, lay, _ = mx_ref(x)
    return q, lay


@pytest.mark.parametrize("K", [64, 192, 768, 3072])
def test_stand_in_passes_the_fp32_accumulation_bound_and_the_floor_has_room(K):
    a, w, want, T, d32 = _bf16_case(70, 36, K)
    got = gc.chunked_f32([(a, w)])
    d_chunk = gc.dist_by_T(got, want, T)
    print(f"K = {K}: chunked fp32 accumulation {d_chunk:.2e} T, torch fp32 CPU product d32 {d32:.2e} T, floor {gc.ACC_FLOOR:.2e}")
    assert gc.holds(got, want, gc.acc_rel(d32) * T)
    assert d_chunk < gc.ACC_FLOOR / 2 and d32 < 1e-6          # a valid other summation order keeps clear of the floor
    # ... and the epilogues carry the bound: every form on the stand-in's product
    bias, scale, resid = gc.epi_params(70, 36)
    for kw in (dict(bias=bias, act="gelu", out="bf16"), dict(bias=bias, scale=scale, resid=resid), dict(bias=bias, resid=resid), dict(act="relu"),
               dict(bias=bias, act="sigmoid"), dict(bias=bias, glu=True, out="bf16")):
        y_want, bound = gc.epilogue(want, gc.acc_rel(d32) * T, **kw)
        y_got, _ = gc.epilogue(got, 0 * T, **kw)
        y_got = y_got.float()                                   # the kernel's fp32 epilogue value ...
        if kw.get("out") == "bf16":
            y_got = y_got.bfloat16()                            # ... and its stored form
        assert gc.holds(y_got, y_want, bound), kw
        if kw.get("out") != "bf16":                            # a defect of 2^-12 T survives the fp32 epilogues
            bad = got.clone()
            x = want + (kw["bias"].double() if "bias" in kw else 0.0)
            i, j = divmod(int(torch.where(x > 0, x, torch.full_like(x, 1e30)).argmin()), x.shape[1])      # where ReLU passes it on and the sigmoid is steep
            bad[i, j] += 2.0 ** -12 * T[i, j]
            assert not gc.holds(gc.epilogue(bad, 0 * T, **kw)[0].float(), y_want, bound), kw


def test_stand_in_passes_x3_bounds_and_one_dropped_cross_term_tile_fails():
    """K = 3072: 96 K-tiles of 32.  The cross term Al Wh of tile 41 alone moves a typical element by about 3e-6 T: several times the
    per-element bound, and a few 1e-5 of the tensor's maximum, where tests/test_gpu_x3.py's bound is 3e-5"""
    terms, defined, exact, T, d32, dist = _x3_case(48, 40, 3072)
    got = gc.chunked_f32(terms)
    print(f"x3 K = 3072: d32 {d32:.2e} T, defined vs exact {dist:.2e} T")
    assert gc.holds(got, defined, gc.acc_rel(d32) * T) and gc.holds(got, exact, gc.split_rel(dist) * T)
    bad = gc.chunked_f32(terms, drop=(1, 41))
    tensor_wide = float((bad - defined).abs().max() / defined.abs().max())
    print(f"  one cross term dropped for one tile: {gc.ratio(bad, defined, gc.acc_rel(d32) * T):.1f} of the per-element bound, tensor-wide rel err {tensor_wide:.1e}")
    assert not gc.holds(bad, defined, gc.acc_rel(d32) * T)
    off = got.clone()
    off[7, 9] += 2.0 ** -12 * T[7, 9]
    assert not gc.holds(off, defined, gc.acc_rel(d32) * T) and not gc.holds(off, exact, gc.split_rel(dist) * T)


def test_h2_stand_in_passes_its_bounds():
    A, W = gc.operands(40, 36, 192)
    ap, wp = gc.h2_parts_cpu(A), gc.h2_parts_cpu(W, weight=True)
    defined, T = gc.ref_h2(ap, wp)
    terms = [(ap[1], wp[2]), (ap[2], wp[1]), (ap[0], wp[0])]
    exact = A.double() @ W.double().t()
    d32, dist = gc.dist_by_T(gc.f32_product(terms), defined, T), gc.dist_by_T(defined, exact, T)
    got = gc.chunked_f32(terms)
    print(f"h2: d32 {d32:.2e} T, defined vs exact {dist:.2e} T")
    assert gc.holds(got, defined, gc.acc_rel(d32) * T) and gc.holds(got, exact, gc.split_rel(dist) * T)
    # H2 output rows: packing the fp32 result passes the three tolerances of tests/test_gpu_h2.py
    h, m8, r8 = gc.h2_parts_cpu(got.float())
    for g, b in gc.h2_row_bounds(defined, gc.acc_rel(d32) * T, h, r8):
        assert gc.holds(g, defined, b)


def test_fp8_bounds_and_one_scale_byte_off_by_one():
    from tests.test_gpu_fp8 import ACC_TOL, quant_ref
    M, N, K = 33, 36, 256
    A, W = gc.operands(M, N, K)
    A[:, :K // 2] *= 40.0
    qa, lay = _mx(A)
    qw, sw = quant_ref(W)
    a, w = gc.dequant_mx(qa, lay), gc.dequant_rows(qw, sw)
    want, T = gc.ref_plain(a, w)
    got = gc.chunked_f32([(a, w)])
    assert gc.holds(got, want, ACC_TOL * T)
    bad_lay = lay.clone()
    bad_lay[5, 3] += 1                                         # one e8m0 byte off by one on one block: that block's 32 products double
    bad = gc.chunked_f32([(gc.dequant_mx(qa, bad_lay), w)])
    assert gc.holds(bad[torch.arange(M) != 5], want[torch.arange(M) != 5], ACC_TOL * T[torch.arange(M) != 5])
    assert not gc.holds(bad[5:6], want[5:6], ACC_TOL * T[5:6])
    off = got.clone()
    off[2, 2] -= 2.0 ** -12 * T[2, 2]
    assert not gc.holds(off, want, ACC_TOL * T)
    # per-row scales on both operands
    qa2, sa2 = quant_ref(A)
    a2 = gc.dequant_rows(qa2, sa2)
    want2, T2 = gc.ref_plain(a2, w)
    assert gc.holds(gc.chunked_f32([(a2, w)]), want2, ACC_TOL * T2)


@pytest.mark.parametrize("dtype", [F32, BF16, torch.uint8])
def test_out_sees_pad_column_guard_row_and_unwritten_row(dtype):
    rows, width, ld = 5, 12, 20
    fresh = lambda: Out(rows, width, dtype, ld=ld, device="cpu")
    o = fresh()
    assert o.view.shape == (rows, ld) and o.data.shape == (rows, width) and o.guards_intact() and o.unwritten() == rows * width
    assert dtype == torch.uint8 or bool(torch.isnan(o.data.float()).all())          # the unwritten pattern decodes to NaN
    val = torch.ones(rows, width).to(dtype)
    o.data.copy_(val)
    assert o.guards_intact() and o.unwritten() == 0
    o = fresh(); o.data.copy_(val); o.view[2, width] = val[0, 0]                      # a write into a pad column
    assert not o.guards_intact()
    o = fresh(); o.data.copy_(val); o.raw[GUARD + rows, 0] = 0                        # one row past the last
    assert not o.guards_intact()
    o = fresh(); o.data.copy_(val); o.raw[GUARD - 1, ld - 1] = 0                      # one element before the first
    assert not o.guards_intact()
    o = fresh(); o.data[:4].copy_(val[:4])                                            # a row left unwritten
    assert o.guards_intact() and o.unwritten() == width
    if dtype != torch.uint8:
        assert not gc.holds(o.data.double(), val.double(), torch.full((rows, width), 1e30, dtype=torch.float64)), "an unwritten element must fail any bound"
    o = Out(rows, width, dtype, device="cpu")                                         # ld == width: the contiguous form the attention tests use
    assert o.view.shape == (rows, width) and o.view.is_contiguous() and PATTERN[dtype][1] == o.guard


def test_nan_pad_column_of_a_leaking_into_the_sum_fails():
    a, w, want, T, d32 = _bf16_case(9, 8, 64)
    ap = guarded_input(a, ld=64 + 8)
    assert ap.shape == (9, 72) and bool(torch.isnan(ap[:, 64:]).all()) and torch.equal(ap[:, :64], a)
    good = gc.chunked_f32([(ap[:, :64], w)])
    assert gc.holds(good, want, gc.acc_rel(d32) * T) and gc.ratio(good, want, gc.acc_rel(d32) * T) < 1.0
    leak = gc.chunked_f32([(ap[:, :72], torch.cat([w, torch.zeros(8, 8)], 1))])      # a kernel that walks K past the row's width
    assert not gc.holds(leak, want, gc.acc_rel(d32) * T) and gc.ratio(leak, want, gc.acc_rel(d32) * T) == float("inf")


def test_sample_rows_cover_tiles_and_cuts():
    idx = gc.sample_rows(11521, 256, cuts=(10752,))
    s = set(idx.tolist())
    assert set(range(256)) <= s and {11520} <= s and 11519 not in s and set(range(10752 - 64, 10752 + 64)) <= s and len(s) < 1000


def test_every_form_counter_is_known_to_the_library():
    """dod_test_counter("form_*") (include/dinodet.h): host-side, so they read 0 or more without a GPU; an unknown form is -1"""
    from dinov2_od_amd import _native as nat
    forms = ["bf16_128_r2", "bf16_128_r3", "bf16_m16", "k64", "ppm", "x3_16w", "x3_pp", "h2", "fp8_rows", "fp8mx_256x128", "fp8mx2_256x128",
             "fp8mx2_256x256", "f32", "patch_fused"]
    L = nat.lib()
    assert all(L.dod_test_counter(("form_" + f).encode()) >= 0 for f in forms)
    assert L.dod_test_counter(b"form_nope") == -1 and L.dod_test_counter(b"form_") == -1
