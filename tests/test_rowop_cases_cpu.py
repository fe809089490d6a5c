"""What tests/test_gpu_rowops.py relies on and a CPU can show: the inputs of tests/rowop_cases.py are what they claim, the named cases
reach every instance of the two dispatch ladders, every bound passes a CPU emulation that sums and rounds where the kernels do, the
float64 reference alone decides the block-scale bytes, and each of nine seeded defects is rejected by the same checks.  No GPU."""
import pytest
import torch

from oracle import dinodet_oracle as orc
from tests import rowop_cases as rc
from tests.gemm_cases import ACC_FLOOR, h2_parts_cpu, ratio

ALL_D = rc.LN_D + rc.LN_D_FREE
INEXACT_D = [D for D in ALL_D if D % 256 or rc.ln_arm(D)[0] * 256 != D]          # some lane of some chunk is masked


def _ln_case(D, variant):
    x, a, g, b, eps = rc.ln_input(D, variant)
    return (x, a, g, b, eps), rc.ln_reference(x, a, g, b, eps)


def _worst(res):
    return max(res.values())


def test_named_cases_reach_every_dispatch_arm():
    """every (chunk count, exact) instance ln_dispatch and rowstats_dispatch can launch is the arm of a D in the sweep, under its name in
    LN_ARMS / RS_ARMS; the constrained forms (D % 64 == 0) still reach all of them"""
    assert {D: rc.ln_arm(D) for D in ALL_D} == rc.LN_ARMS and {D: rc.ln_arm(D, True) for D in ALL_D} == rc.RS_ARMS
    ln_all = {(1, True), (2, True), (3, True), (4, True), (6, True), (1, False), (2, False), (4, False), (8, False)}
    assert {rc.LN_ARMS[D] for D in rc.LN_D} == ln_all
    assert {rc.RS_ARMS[D] for D in rc.LN_D} == {(3, True), (4, True), (6, True), (2, False), (4, False), (8, False)}
    for D in range(4, 2049, 4):                                     # nothing else exists
        assert rc.ln_arm(D) in ln_all
    assert all(D % 64 == 0 for D in rc.LN_D) and all(D % 4 == 0 and D <= 2048 for D in ALL_D)
    assert {v[1] for v in rc.ln_variants(64)} == {1, 5, 9} and {v[2] for D in ALL_D for v in rc.ln_variants(D)} == {1e-6, 1e-5}
    assert {v[3] for v in rc.ln_variants(64)} == {True, False}
    assert {k for D in ALL_D for v in rc.ln_variants(D) for k in v[5]} == set(rc.ROW_KINDS)


def test_layernorm_inputs_are_what_they_claim():
    for D in (64, 768, 2044):
        for variant in rc.ln_variants(D)[:2]:
            (x, a, g, b, eps), R = _ln_case(D, variant)
            v = x.double() + (a.double() if a is not None else 0.0)
            for r, kind in enumerate(variant[5]):
                if kind == "offset":              # the mean is about a hundred standard deviations away
                    assert 60.0 < float(v[r].mean() / v[r].std()) < 160.0
                elif kind == "normal":
                    assert 1.5 < float(v[r].std()) < 2.9 and abs(float(v[r].mean()) - 0.5) < 1.0
                elif kind == "outlier":
                    assert float(v[r].abs().amax()) > 9e3 and int((v[r].abs() > 100).sum()) == 1
                elif kind == "const":
                    assert bool((v[r] == v[r, 0]).all()) and float(v[r, 0]) != 0.0
                    assert bool((R["want"][r] == b.double()).all()) and bool((R["T"][r] > 0).all())
                else:                             # exact zeros in, beta = 0: exact zeros out, nothing allowed
                    assert bool((v[r] == 0).all()) and bool((b == 0).all())
                    assert bool((R["want"][r] == 0).all()) and bool((R["T"][r] == 0).all()) and bool((R["xb"][r] == 0).all())


def test_layernorm_bounds_pass_the_emulation_of_the_kernels_order():
    """fp32 rows summed lane by lane and through the butterfly as the kernel does, then every output form made from them: inside every bound
    of ln_check, for every form, D and variant.  The emulation's own distance decides whether LN_FLOOR has to be raised: it does not"""
    worst_emu = worst_d32 = 0.0
    worst = {}
    for D in ALL_D:
        for variant in rc.ln_variants(D):
            (x, a, g, b, eps), R = _ln_case(D, variant)
            y = rc.ln_emulate(x, a, g, b, eps)
            worst_emu = max(worst_emu, rc.dist_by_T(y.double(), R["want"], R["T"]))
            worst_d32 = max(worst_d32, R["d32"])
            for form in rc.LN_FORMS:
                if D not in rc.ln_dims(form):
                    continue
                for name, val in rc.ln_check(form, rc.ln_forms_emulate(y, form), R).items():
                    worst[name] = max(worst.get(name, 0.0), val)
                    assert val <= 1.0, (D, variant[0], form, name, val)
    print(f"layernorm: emulation {worst_emu:.3e} T, torch fp32 {worst_d32:.3e} T, floor {rc.LN_FLOOR:.3e}; worst ratios {worst}")
    assert worst_emu <= rc.LN_FLOOR == ACC_FLOOR
    assert 2e-8 < worst_d32 < 2.5e-7


def test_h2_bytes_are_the_shared_packing():
    y = rc.ln_emulate(*rc.ln_input(256, rc.ln_variants(256)[0]))
    for got, want in zip(rc.h2_decode(rc.h2_pack_cpu(y), 256), h2_parts_cpu(y)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("D", rc.LN_D)
def test_block_scale_bytes_are_decided_by_the_reference(D):
    """with the fp32 bound as the value margin, at most 1 % of the 32-column blocks of any launch have a byte the reference leaves open"""
    for variant in rc.ln_variants(D):
        _, R = _ln_case(D, variant)
        share = rc.mx_undecided(R)
        print(f"D = {D} {variant[0]}: {share:.4f} of the blocks undecided")
        assert share <= 0.01


def test_rowstats_bounds_pass_the_emulation():
    worst = {}
    for kind in rc.RS_KINDS:
        for D in rc.rs_dims(kind):
            for variant in rc.ln_variants(D):
                x, _, _, _, eps = rc.ln_input(D, variant)
                mean, rstd = rc.ln_stats_emulate(x, eps, rowstats=True)
                res = rc.rs_check(kind, torch.stack([mean, rstd], 1), rc.rs_operand_cpu(x, kind), x, rc.rs_reference(x, eps))
                for name, val in res.items():
                    worst[name] = max(worst.get(name, 0.0), val)
                    assert val <= 1.0, (kind, D, variant[0], name, val)
    print(f"rowstats: worst ratios {worst}")


# ------------------------------------------------------------------------------------------------ seeded defects, LayerNorm
@pytest.mark.parametrize("D", INEXACT_D)
@pytest.mark.parametrize("defect", ["tail_in_mean", "var_div"])
def test_defect_in_the_statistics_of_a_masked_tail_is_rejected(D, defect):
    """a masked lane's float4 summed into the mean, or the variance divided by the instance's 256 NCH columns instead of D: at every D
    with a masked lane (384, 832, 1280 with three whole chunks masked, 4, 132, 2044) the fp32 bound fails, and the statistics' own too"""
    assert INEXACT_D == [64, 384, 832, 1280, 4, 132, 2044]
    variant = rc.ln_variants(D)[0]
    (x, a, g, b, eps), R = _ln_case(D, variant)
    assert _worst(rc.ln_check("f32", rc.ln_forms_emulate(rc.ln_emulate(x, a, g, b, eps, defect), "f32"), R)) > 1.0
    mean, rstd = rc.ln_stats_emulate(x, eps, defect, rowstats=True)
    res = rc.rs_check("bf16", torch.stack([mean, rstd], 1), rc.rs_operand_cpu(x, "bf16"), x, rc.rs_reference(x, eps))
    assert res["mean" if defect == "tail_in_mean" else "rstd"] > 1.0


@pytest.mark.parametrize("D", [D for D in rc.LN_D if D >= 256])
def test_defect_scale_byte_at_the_plain_block_index_is_rejected(D):
    """D = 64 has two blocks, whose plain and interleaved offsets coincide; from D = 256 on the outlier's block gives it away"""
    for variant in rc.ln_variants(D)[:2]:
        (x, a, g, b, eps), R = _ln_case(D, variant)
        y = rc.ln_emulate(x, a, g, b, eps)
        assert _worst(rc.ln_check("fp8_mx", rc.ln_forms_emulate(y, "fp8_mx", "bs_plain"), R)) > 1.0


@pytest.mark.parametrize("D", ALL_D)
def test_defects_of_the_split_outputs_are_rejected(D):
    """S3 in the weight order [hi | lo | hi]; the pair's lo taken from a truncated instead of the rounded hi"""
    for variant in rc.ln_variants(D)[:2]:
        (x, a, g, b, eps), R = _ln_case(D, variant)
        y = rc.ln_emulate(x, a, g, b, eps)
        res = rc.ln_check("f32_s3", rc.ln_forms_emulate(y, "f32_s3", "s3_weight_order"), R)
        assert res["s3 planes 0 == 1"] > 1.0 and res["s3 == split(f32)"] > 1.0
        res = rc.ln_check("pair", rc.ln_forms_emulate(y, "pair", "pair_lo"), R)
        assert res["pair hi + lo"] > 1.0 and res["pair hi"] <= 1.0


# ------------------------------------------------------------------------------------------------ deformable gather
@pytest.mark.parametrize("case", rc.DF_CASES)
def test_gather_inputs_reference_and_defects(case):
    h, w, Hd, dh, P = case
    proj, values = rc.df_input(case)
    ncat = rc.df_ncat(case)
    assert proj.shape == (rc.DF_B * rc.DF_Q, ncat + 3) and bool(torch.isnan(proj[:, ncat:]).all()) and not bool(torch.isnan(proj[:, :ncat]).any())
    assert 0.25 <= rc.df_clamp_share(proj, case) <= 0.5               # about a third of the points clamp on an axis
    assert {30.0, -30.0, 0.0} <= set(proj[:, :2].reshape(-1).tolist())
    aw = proj[:, 2 + 2 * Hd * P:ncat]
    assert float(aw.max()) == 60.0 and float(aw.min()) == -60.0
    assert (rc.DF_B * rc.DF_Q * Hd) % 4 != 0 or Hd % 2 == 0
    # the float64 restatement is the oracle's
    p = proj[:, :ncat].double()
    o = orc.deformable_sample(values.double().reshape(rc.DF_B, h * w, Hd, dh), torch.sigmoid(p[:, :2]).reshape(rc.DF_B, rc.DF_Q, 2),
                              p[:, 2:2 + 2 * Hd * P].reshape(rc.DF_B, rc.DF_Q, Hd, P, 2),
                              torch.softmax(p[:, 2 + 2 * Hd * P:].reshape(rc.DF_B, rc.DF_Q, Hd, P), -1), h, w).reshape(-1, Hd * dh)
    for shared in (False, True):
        R = rc.df_reference(proj, values, case, shared)
        if not shared:
            assert float((o - R["want"]).abs().max()) < 1e-13
        else:                                     # every image samples with image 0's projections
            want0 = rc.df_reference(proj[:rc.DF_Q].repeat(rc.DF_B, 1), values, case, False)["want"]
            assert torch.equal(R["want"], want0) and not torch.equal(R["want"][rc.DF_Q:], rc.df_reference(proj, values, case, False)["want"][rc.DF_Q:])
        f32 = rc.df_eval(proj, values, case, torch.float32, shared)
        res = rc.df_check(f32, torch.cat([rc.split_pair(f32)[0]] * 2 + [rc.split_pair(f32)[1]], 1).bfloat16(), R)
        print(f"gather {case} shared {shared}: fp32 CPU {R['d32']:.2e} T, ratios {res}")
        assert _worst(res) <= 1.0
        # corners (y1, x0) and (y0, x1) exchanged
        assert _worst(rc.df_check(rc.df_eval(proj, values, case, torch.float32, shared, "swap_corners"), None, R)) > 1.0
    # the shared projections indexed by b Q + q: the rows behind the Q shared ones are NaN
    Rs = rc.df_reference(proj, values, case, True)
    sh = torch.cat([proj[:rc.DF_Q], torch.full_like(proj[rc.DF_Q:], float("nan"))])
    assert _worst(rc.df_check(rc.df_eval(sh, values, case, torch.float32, True), None, Rs)) <= 1.0
    assert _worst(rc.df_check(rc.df_eval(sh, values, case, torch.float32, True, "shared_bq"), None, Rs)) == float("inf")
    if 64 < dh < 128:                             # every lane of the second group stores, whatever dh is
        f32 = rc.df_eval(proj, values, case, torch.float32, False)
        assert _worst(rc.df_check(rc.df_spill_second_half(f32, case), None, rc.df_reference(proj, values, case, False))) > 1.0


# ------------------------------------------------------------------------------------------------ SwiGLU, split3
@pytest.mark.parametrize("rows,Fh", rc.SW_CASES)
@pytest.mark.parametrize("bf16", [False, True])
def test_swiglu_bound_passes_fp32_and_rejects_interleaved_halves(rows, Fh, bf16):
    x = rc.sw_input(rows, Fh, bf16)
    gates = set(x[:, :Fh].float().reshape(-1)[:11].tolist())
    assert gates >= ({0.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0} if rows * Fh >= 11 else {0.0, 20.0, -20.0, 88.0, -88.0})
    if rows * Fh >= 11:
        assert max(gates) > 9e3 and min(gates) < -9e3
    R = rc.sw_reference(x, bf16)
    got = rc.sw_eval(x, torch.float32)
    got = got.bfloat16().double() if bf16 else got.double()
    r = ratio(got, R["want"], R["bound"])
    print(f"swiglu {rows, Fh} bf16 {bf16}: fp32 CPU {R['d32']:.2e}, ratio {r:.3f}")
    assert r <= 1.0 and R["rel"] < 1e-6
    assert bool(torch.isfinite(R["want"]).all())
    bad = rc.sw_eval(x, torch.float32, "interleaved")
    assert ratio(bad.bfloat16().double() if bf16 else bad.double(), R["want"], R["bound"]) > 1.0
    if rows * Fh > 8192 * 256:
        assert rows * Fh < 2 * 8192 * 256         # the grid-stride loop's second pass, not a third


def test_split3_cases_and_orders():
    for rows, K in rc.S3_CASES:
        x = rc.s3_input(rows, K)
        a, wt = rc.s3_cpu(x, 0).float(), rc.s3_cpu(x, 1).float()
        assert torch.equal(a[:, :K], a[:, K:2 * K]) and torch.equal(wt[:, :K], wt[:, 2 * K:]) and torch.equal(a[:, 2 * K:], wt[:, K:2 * K])
        assert torch.equal(a[:, :K], x.bfloat16().float()) and float(((a[:, :K] + a[:, 2 * K:]).double() - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())
    assert rc.S3_CASES[-1][0] * rc.S3_CASES[-1][1] > 4096 * 256
