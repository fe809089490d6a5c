"""The inference GEMM dispatch policy (csrc/gemm_plan.h) interrogated on the host through dod_test_gemm_plan: no device, any CU count.

  * tests/golden/gemm_dispatch_parent.json: what the launchers of the commit BEFORE the planner did at every case of tests/gemm_dispatch_cases.py
    (recorded on an MI355X with tools/record_gemm_dispatch.py from the counters that moved).  The plan, aggregated into counters, must predict
    exactly those movements: no shape is launched differently.
  * what the comments beside the rules promise, as explicit cases with the comment cited;
  * at other CU counts: every plan tiles [0, M), every K-split step meets its kernel's precondition and fits the scratch."""
import json
import os

import pytest

from dinov2_od_amd import _native as nat
from tests import gemm_dispatch_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_dispatch_parent.json")
MIB64 = 64 << 20
F = dc.FORMS.index


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def options():
    """set the test options of a case; hand the shipped behaviour back afterwards"""
    def set_(tailsplit=-1, f32_ksplit=-1, epi_regmath=-1):
        nat.set_option("tailsplit", tailsplit)
        nat.set_option("f32_ksplit", f32_ksplit)
        nat.set_option("epi_regmath", epi_regmath)
    yield set_
    set_()


def plan(family, M, N, K, epi, cus=256, scratch=MIB64):
    return nat.gemm_plan(dc.FAMILY[family], M, N, K, dc.epi_flags(epi, N), cus, scratch)


def test_case_list_is_what_was_recorded(recorded):
    got = [dc.Case(*(r[k] for k in dc.Case._fields)) for r in recorded["cases"]]
    assert got == dc.CASES, "tests/gemm_dispatch_cases.py and the recording differ: record again at the commit the recording stands for"
    assert recorded["cus"] == 256 and recorded["scratch_bytes"] == MIB64


def test_plan_predicts_every_recorded_launch(recorded, options):
    wrong = []
    for r in recorded["cases"]:
        c = dc.Case(*(r[k] for k in dc.Case._fields))
        options(c.tailsplit, c.f32_ksplit)
        steps = plan(c.family, c.M, c.N, c.K, c.epi, recorded["cus"], recorded["scratch_bytes"])
        if dc.counters_of(steps) != r["moved"]:
            wrong.append((c, steps, r["moved"]))
    assert not wrong, (len(wrong), wrong[:5])


# (source comment, family, M, N, K, epilogue, tailsplit, the steps on 256 CUs with 64 MiB reserved: (form, row0, rows, kslices))
COMMENT_FACTS = [
    ("gemm_plan.h tail_split: 1029 tiles (4 rounds + 5: S = 8)", "x3", 87680, 768, 3072, "ls_resid", -1,
     [("x3_pp", 0, 87296, 1), ("x3_pp", 87296, 384, 8), (None, 87296, 384, 8)]),
    ("the same on the H2 kernel", "h2", 87680, 768, 3072, "ls_resid", -1, [("h2", 0, 87296, 1), ("h2", 87296, 384, 8), (None, 87296, 384, 8)]),
    ("the same, plain bf16: fc2 behind its tail split", "bf16", 87680, 768, 3072, "ls_resid", -1,
     [("ppm", 0, 87296, 1), ("ppm", 87296, 384, 8), (None, 87296, 384, 8)]),
    ("gemm_plan.h tail_split: 344 tiles (1 round + 88: S = 2)", "x3", 10960, 2048, 768, "pair", 2,
     [("x3_pp", 0, 8192, 1), ("x3_pp", 8192, 2768, 2), (None, 8192, 2768, 2)]),
    ("gemm_plan.h tail_split: the compensated QKV at 32 images of 224^2, 33 x 9 = 297 tiles, takes the shallow split", "x3", 8224, 2304, 768, "pair", -1,
     [("x3_pp", 0, 7168, 1), ("x3_pp", 7168, 1056, 4), (None, 7168, 1056, 4)]),
    ("the same on the H2 kernel", "h2", 8224, 2304, 768, "pair", -1, [("h2", 0, 7168, 1), ("h2", 7168, 1056, 4), (None, 7168, 1056, 4)]),
    ("gemm_plan.h bf16_rows: QKV = 33 x 9 = 297 = one round + 41 takes the remainder cut", "bf16", 8224, 2304, 768, "bf16", -1,
     [("k64", 0, 7168, 1), ("bf16_128_r3", 7168, 1056, 1)]),
    ("gemm_plan.h bf16_rows: fc1 = 43 x 12 = 516 tiles = two rounds + 4 is BELOW the window and is not cut (tests/test_gpu_lnfold.py says so too; "
     "the comment that listed it as cut was wrong)", "bf16", 10960, 3072, 768, "gelu_bf16", -1, [("k64", 0, 10960, 1)]),
    ("gemm_plan.h bf16_rows: 2 x 4 images of 518^2, fc1 = 264 tiles, is not cut", "bf16", 5480, 3072, 768, "gelu_bf16", -1, [("k64", 0, 5480, 1)]),
    # the window CUs / 16 <= rem <= CUs / 6 from both sides: 6 n-tiles, rem = 14 | 20 | 38 | 44; 8 n-tiles, rem = 8 | 16
    ("remainder-cut window: rem = 14 < CUs / 16", "bf16", 45 * 256, 1536, 64, "bf16", 0, [("k64", 0, 45 * 256, 1)]),
    ("remainder-cut window: rem = 20", "bf16", 46 * 256, 1536, 64, "bf16", 0, [("k64", 0, 42 * 256, 1), ("bf16_128_r2", 42 * 256, 4 * 256, 1)]),
    ("remainder-cut window: rem = 38 <= CUs / 6", "bf16", 49 * 256, 1536, 64, "bf16", 0, [("k64", 0, 42 * 256, 1), ("bf16_128_r2", 42 * 256, 7 * 256, 1)]),
    ("remainder-cut window: rem = 44 > CUs / 6", "bf16", 50 * 256, 1536, 64, "bf16", 0, [("k64", 0, 50 * 256, 1)]),
    ("remainder-cut window: rem = 8 < CUs / 16", "bf16", 33 * 256, 2048, 64, "bf16", 0, [("k64", 0, 33 * 256, 1)]),
    ("remainder-cut window: rem = 16 = CUs / 16", "bf16", 34 * 256, 2048, 64, "bf16", 0, [("k64", 0, 32 * 256, 1), ("bf16_128_r2", 32 * 256, 2 * 256, 1)]),
]


@pytest.mark.parametrize("why,family,M,N,K,epi,tailsplit,want", COMMENT_FACTS, ids=[f"{c[1]}-{c[2]}x{c[3]}x{c[4]}" for c in COMMENT_FACTS])
def test_what_the_comments_promise(recorded, options, why, family, M, N, K, epi, tailsplit, want):
    options(tailsplit)
    steps = plan(family, M, N, K, epi)
    got = [(None if s[0] == dc.FORM_REDUCE else dc.FORMS[s[0]],) + s[1:4] for s in steps]
    assert got == want, why
    # ... and the launchers before the planner did just that, as far as their counters show
    rec = [r for r in recorded["cases"] if (r["family"], r["M"], r["N"], r["K"], r["epi"], r["tailsplit"]) == (family, M, N, K, epi, tailsplit)]
    assert len(rec) == 1 and rec[0]["moved"] == dc.counters_of(steps), (why, rec)


def test_f32_slices_depend_on_n_and_k_until_the_slab_is_full(options):
    """gemm_plan.h GEMM_F32 (the comment gemm_f32.hip used to get wrong): S from (N, K) alone, and the split is dropped when tiles x S exceeds
    F32K_PARTS = 1536 -- the class head (2 n-tiles, S = 6) stops splitting above 128 m-tiles = 8192 rows"""
    options(f32_ksplit=1)
    for M in (100, 400, 3200, 8192):
        assert [s[3] for s in plan("f32", M, 91, 768, "none")] == [6], M
        assert [s[3] for s in plan("f32", M, 4, 768, "none")] == [6], M
    assert [s[3] for s in plan("f32", 8193, 91, 768, "none")] == [1]
    assert [s[3] for s in plan("f32", 1600, 768, 768, "none")] == [3]      # "N = 768 (12 n-tiles) -> 3": 25 x 12 tiles x 3
    assert [s[3] for s in plan("f32", 2731, 768, 768, "none")] == [1]      # 43 x 12 = 516 tiles x 3 > 1536
    assert [s[3] for s in plan("f32", 400, 91, 768, "none", scratch=0)] == [1]      # no slab reserved
    options(f32_ksplit=-1)
    assert [s[3] for s in plan("f32", 400, 91, 768, "none")] == [1]        # the operator's callers do not allow it
    assert [s[3] for s in nat.gemm_plan(dc.FAMILY["f32"], 400, 91, 768, dc.epi_flags("none", 91) | dc.ALLOW_KSPLIT, 256, MIB64)] == [6]      # the forward's do


def test_register_epilogue_follows_its_option(options):
    options(tailsplit=0)
    assert [s[4] for s in plan("bf16", 4097, 1544, 64, "gelu_bf16")] == [1] and [s[4] for s in plan("bf16", 4097, 1540, 192, "gelu_bf16")] == [0]
    assert [s[4] for s in plan("bf16", 4097, 1544, 64, "ls_inplace")] == [0] and [s[4] for s in plan("bf16", 4097, 1544, 64, "swiglu")] == [0]
    options(tailsplit=0, epi_regmath=0)
    assert [s[:5] for s in plan("bf16", 4097, 1544, 64, "gelu_bf16")] == [(F("k64"), 0, 4097, 1, 0)]


KTILE = {"bf16": 64, "x3": 32, "h2": 32}
SHAPES = [("bf16", 87680, 768, 3072, "ls_resid"), ("bf16", 8224, 2304, 768, "bf16"), ("bf16", 10960, 3072, 768, "gelu_bf16"), ("bf16", 21800, 768, 384, "bf16"),
          ("bf16", 11521, 1536, 64, "resid"), ("bf16", 3200, 768, 2304, "none"), ("bf16", 257, 768, 768, "none"),
          ("x3", 87680, 768, 3072, "ls_resid"), ("x3", 8224, 2304, 768, "pair"), ("x3", 8224, 768, 768, "ls_resid"), ("x3", 2049, 516, 192, "gelu_pair"),
          ("x3", 43840, 3072, 768, "gelu_pair"), ("h2", 87680, 768, 3072, "ls_resid"), ("h2", 10960, 2304, 768, "pair"), ("h2", 2740, 768, 768, "ls_resid"),
          ("fp8", 8224, 3072, 768, "mx2"), ("fp8", 257, 768, 768, "rows"), ("f32", 3200, 91, 768, "none"), ("f32", 8193, 91, 768, "none")]


@pytest.mark.parametrize("scratch", [0, 1 << 20, MIB64])
@pytest.mark.parametrize("tailsplit", [-1, 2])
@pytest.mark.parametrize("cus", [64, 128, 240, 256, 304])
def test_plans_at_other_cu_counts_are_sound(options, cus, tailsplit, scratch):
    """properties of every plan, whatever it chooses: the steps tile [0, M) in order without overlap; a K-split step has K divisible by
    S x ktile with at least three K-tiles per slice, its S x tiles fill at most the chip, its R x N x S x 4 bytes of partial slabs fit the
    scratch, and the reduce step that follows covers the same rows with the same S"""
    options(tailsplit, 1)
    split = 0
    for family, M, N, K, epi in SHAPES:
        steps = plan(family, M, N, K, epi, cus, scratch)
        assert 1 <= len(steps) <= 4
        nxt = 0
        for i, (form, row0, rows, S, regmath, gm) in enumerate(steps):
            assert rows > 0 and S >= 1
            if form == dc.FORM_REDUCE:
                assert i > 0 and steps[i - 1][0] != dc.FORM_REDUCE and steps[i - 1][1:4] == (row0, rows, S) and S >= 2
                continue
            assert row0 == nxt, (family, M, N, K, cus, steps)
            nxt += rows
            if family == "f32":
                tiles = -(-rows // 64) * -(-N // 64)
                assert S == 1 or (scratch > 0 and tiles <= 4096 and tiles * S <= 1536 and -(-K // 16) // S >= 8)
            elif S > 1:
                split += 1
                assert dc.FORMS[form] == {"bf16": "ppm", "x3": "x3_pp", "h2": "h2"}[family]
                assert K % (S * KTILE[family]) == 0 and K // (S * KTILE[family]) >= 3
                assert -(-rows // 256) * -(-N // 256) * S <= cus
                assert rows * N * S * 4 <= scratch
                assert i + 1 < len(steps) and steps[i + 1][0] == dc.FORM_REDUCE
            assert regmath in (0, 1) and (not regmath or dc.FORMS[form] == "k64")
        assert nxt == M, (family, M, N, K, cus, steps)
    assert split > 0 or scratch < MIB64 or cus == 64, "no shape of the list took a K split: the properties above were not exercised"


def test_bad_arguments_are_rejected():
    L = nat.lib()
    steps = (nat.DodGemmStep * 4)()
    assert L.dod_test_gemm_plan(5, 64, 64, 64, 0, 256, 0, steps, 4) == -1 and L.dod_test_gemm_plan(0, 0, 64, 64, 0, 256, 0, steps, 4) == -1
    assert L.dod_test_gemm_plan(0, 64, 64, 64, 0, 0, 0, steps, 4) == -1 and L.dod_test_gemm_plan(0, 64, 64, 64, 0, 256, 0, None, 4) == -1
    assert L.dod_test_gemm_plan(0, 64, 64, 64, 0, 256, 0, steps, 0) == -1 and L.dod_test_gemm_plan(0, 64, 64, 64, 0, 256, 0, steps, 1) == 1
