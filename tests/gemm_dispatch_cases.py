"""Inference GEMM dispatch cases: the shapes the project runs, shared by the recorder (tools/record_gemm_dispatch.py, which launches each
case once through the operator entry points and writes the counters that moved to tests/golden/gemm_dispatch_parent.json) and by the CPU test
of the planner (tests/test_gemm_plan_cpu.py, which asks dod_test_gemm_plan for the same case and aggregates its steps into counters).

A case: family ("bf16" / "x3" / "h2" / "fp8" / "f32"), M, N, K, epi (the epilogue kind: what the operator entry point is given), and the
`tailsplit` / `f32_ksplit` test option values (-1 = the shipped behaviour).  EPI maps a kind to the GemmEpi facts the dispatch policy reads."""
import collections

Case = collections.namedtuple("Case", "family M N K epi tailsplit f32_ksplit")
FAMILY = {"bf16": 0, "x3": 1, "h2": 2, "fp8": 3, "f32": 4}            # gemm_plan.h GEMM_*
FORMS = ["bf16_128_r2", "bf16_128_r3", "bf16_m16", "k64", "ppm", "x3_16w", "x3_pp", "h2", "fp8_rows", "fp8mx_256x128", "fp8mx2_256x128",
         "fp8mx2_256x256", "f32", "patch_fused"]                     # dod_common.h FORM_*, in order
FORM_REDUCE = len(FORMS)                                             # gemm_plan.h FORM_KSPLIT_REDUCE: the tail split's reduce launch (no counter)
COUNTERS = ["form_" + f for f in FORMS] + ["tail_splits", "rem_cuts", "f32_ksplits", "epi_regmath"]

# include/dinodet.h DOD_PLAN_*: what the policy reads of an epilogue
GELU, SIGMOID, ROWMAP, A_SCALE, OUT_SPLIT3, KSPLIT, ROWS_OK, REGMATH_OK, A_BS, W_BS, OUT_BS, ALLOW_KSPLIT = [1 << i for i in range(12)]

# kind -> what the operator call sets: out ("f32" / "bf16" / "pair" / "h2"), act, resid, glu, fp8 scale kind
Epi = collections.namedtuple("Epi", "out act resid glu scales", defaults=("f32", "none", False, False, None))
EPI = {"none": Epi(), "bf16": Epi("bf16"), "gelu_bf16": Epi("bf16", "gelu"), "ls_resid": Epi(resid=True), "ls_inplace": Epi(resid=True), "resid": Epi(resid=True),
       "inplace": Epi(resid=True), "relu": Epi(act="relu"), "gelu": Epi(act="gelu", resid=True), "sigmoid": Epi(act="sigmoid", resid=True),
       "swiglu": Epi("bf16", glu=True), "pair": Epi("pair"), "gelu_pair": Epi("pair", "gelu"), "gelu_h2": Epi("h2", "gelu"),
       "rows": Epi(scales="rows"), "mx": Epi(scales="mx"), "mx2": Epi(scales="mx2"), "rows_gelu_bf16": Epi("bf16", "gelu", scales="rows"),
       "mx_gelu_bf16": Epi("bf16", "gelu", scales="mx"), "mx2_gelu_bf16": Epi("bf16", "gelu", scales="mx2"), "mx2_ls_resid": Epi(resid=True, scales="mx2"),
       "mx_ls_resid": Epi(resid=True, scales="mx"), "rows_ls_resid": Epi(resid=True, scales="rows"),
       "mx2_glu": Epi("bf16", glu=True, scales="mx2_glu")}


def epi_flags(kind, N, ldc=None):
    """the planner's flag word for epilogue `kind` of an N-column GEMM whose output pitch is ldc (default: dense rows).  Restates
    gemm_epi_rows_ok (dod_common.h) and epi_regmath_ok (gemm_epi.h) for the epilogues the operator entry points can build: none of them maps
    rows, K-slices or writes the [hi | hi | lo] layout, so ROWMAP, KSPLIT and OUT_SPLIT3 stay clear"""
    e = EPI[kind]
    width = N // 2 if e.glu else (2 * N if e.out == "pair" else N)
    ldc = width if ldc is None else ldc
    f = {"gelu": GELU, "sigmoid": SIGMOID}.get(e.act, 0)
    f |= {None: 0, "rows": A_SCALE, "mx": A_BS, "mx2": A_BS | W_BS, "mx2_glu": A_BS | W_BS | OUT_BS}[e.scales]
    if e.scales is None:
        f |= ROWS_OK
    drain8 = (e.out in ("bf16", "pair", "h2") and not e.resid and e.scales in (None, "mx2") and N % 8 == 0 and ldc % 8 == 0)
    if drain8 and e.out == "bf16" and not e.glu and e.act in ("none", "relu", "gelu"):
        f |= REGMATH_OK
    return f


def counters_of(steps):
    """what executing `steps` [(form, row0, rows, kslices, regmath, gm)] moves: one launch per form, the reduce launch under tail_splits, main
    rows followed by cut rows under rem_cuts, an fp32 launch with K slices under f32_ksplits, a register epilogue under epi_regmath"""
    c = collections.Counter()
    for form, row0, rows, kslices, regmath, gm in steps:
        if form == FORM_REDUCE:
            c["tail_splits"] += 1
            continue
        c["form_" + FORMS[form]] += 1
        if row0 > 0 and kslices <= 1:
            c["rem_cuts"] += 1
        if FORMS[form] == "f32" and kslices > 1:
            c["f32_ksplits"] += 1
        if regmath:
            c["epi_regmath"] += 1
    return dict(c)


TOKENS = [t * b for t in (257, 1370) for b in (1, 2, 4, 8, 16, 32, 64)]
# (N, K, epilogue of the plain bf16 family, of the compensated families) of the four block linears: QKV, out-proj, fc1 / weights_in, fc2 / weights_out
VIT_B = [(2304, 768, "bf16", "pair"), (768, 768, "ls_resid", "ls_resid"), (3072, 768, "gelu_bf16", "gelu_pair"), (768, 3072, "ls_resid", "ls_resid")]
VIT_L = [(3072, 1024, "bf16", "pair"), (1024, 1024, "ls_resid", "ls_resid"), (4096, 1024, "gelu_bf16", "gelu_pair"), (1024, 4096, "ls_resid", "ls_resid")]
VIT_G = [(4608, 1536, "bf16", "pair"), (1536, 1536, "ls_resid", "ls_resid"), (8192, 1536, "swiglu", "pair"), (1536, 4096, "ls_resid", "ls_resid")]


def _cases():
    out = []

    def add(family, M, N, K, epi, tailsplit=-1, f32_ksplit=-1):
        c = Case(family, M, N, K, epi, tailsplit, f32_ksplit)
        if c not in out:
            out.append(c)
    # ---- backbone: token rows x block linears.  ViT-B at every batch; the wider models where their outputs stay under ~1.5 GB
    for M in TOKENS:
        for N, K, eb, ec in VIT_B:
            add("bf16", M, N, K, eb)
            add("x3", M, N, K, ec)
            add("h2", M, N, K, ec)
    for M in (257 * 8, 257 * 32, 1370 * 2, 1370 * 8, 1370 * 16):
        for N, K, eb, ec in VIT_L + VIT_G:
            add("bf16", M, N, K, eb)
            add("x3", M, N, K, ec)
            add("h2", M, N, K, ec)
    # the shards and micro-batches the benchmark times (8 x 10 960, 2 x 43 840) are 1370 x 8 and 1370 x 32 above; the tail split's modes on them
    for M in (8224, 10960, 43840, 87680):
        for N, K, eb, ec in VIT_B:
            for mode in (0, 2):
                add("bf16", M, N, K, eb, tailsplit=mode)
                add("x3", M, N, K, ec, tailsplit=mode)
                add("h2", M, N, K, ec, tailsplit=mode)
    # ---- fp8 scale kinds on the ViT-B linears (K % 256 == 0)
    for M in (257, 2056, 8224, 10960, 43840):
        for N, K, eb, _ in VIT_B:
            for kind in ("rows", "mx", "mx2"):
                add("fp8", M, N, K, kind + {"bf16": "_gelu_bf16", "gelu_bf16": "_gelu_bf16", "ls_resid": "_ls_resid"}[eb])
        add("fp8", M, 8192, 1536, "mx2_glu")
    # ---- decoder: Q x B query rows; plain fp32 operands (K = 768) and the [hi | hi | lo] split operands as a plain bf16 GEMM over K' = 3K
    for M in [q * b for q in (100, 300) for b in (1, 2, 4, 8, 16, 32, 64)]:
        for N in (768, 1024, 2304, 256):                                # self-attn / value / output projections, FFN, fused QKV, a 256-wide projection
            add("f32", M, N, 768, "none", f32_ksplit=1)
            add("bf16", M, N, 2304, "none")
        add("f32", M, 768, 1024, "none", f32_ksplit=1)
        add("bf16", M, 768, 3072, "ls_resid")
        for N in (91, 50, 4):                                            # class head, a 50-wide head, box head
            add("f32", M, N, 768, "sigmoid" if N == 4 else "none", f32_ksplit=1)
    for N in (91, 50, 4):
        add("f32", 400, N, 768, "none")                                  # the operator's default: no split
        add("f32", 400, N, 768, "none", f32_ksplit=0)
    # the class head at and just above the row count where tiles x S crosses the slab's F32K_PARTS = 1536 (gemm_f32.hip): 128 x 2 tiles x 6
    add("f32", 8192, 91, 768, "none", f32_ksplit=1)
    add("f32", 8193, 91, 768, "none", f32_ksplit=1)
    # memory-side projections of the decoder (value-proj over every token) at small batch
    for M in (257, 1370, 2740):
        add("bf16", M, 768, 768, "none")
        add("bf16", M, 256, 768, "none")
    # ---- the edge shapes of tests/test_gpu_gemm_edges.py, test_gpu_lnfold.py and test_gpu_tailsplit.py
    for M, N, K in ((129, 132, 64), (129, 136, 128), (129, 132, 192), (255, 136, 320), (3841, 1292, 64), (3841, 1288, 192), (4097, 768, 64)):
        add("bf16", M, N, K, "gelu_bf16", tailsplit=0)
        add("bf16", M, N, K, "resid", tailsplit=0)
    for epi in ("gelu_bf16", "bf16", "ls_inplace", "none", "swiglu"):
        add("bf16", 4097, 1544, 64, epi, tailsplit=0)
    add("bf16", 4097, 1540, 192, "gelu_bf16", tailsplit=0)
    add("bf16", 4097, 1540, 192, "resid", tailsplit=0)
    for epi in ("resid", "bf16", "gelu_bf16"):
        add("bf16", 11521, 1536, 64, epi, tailsplit=0)
        add("bf16", 10753, 768, 2048, epi, tailsplit=0)
    for epi in ("ls_inplace", "bf16", "none"):
        add("bf16", 21800, 768, 384, epi, tailsplit=2)
        add("bf16", 21800, 768, 384, epi)
    for fam in ("x3", "h2"):
        for M, N, K in ((257, 260, 32), (257, 264, 96), (2049, 516, 160), (4097, 260, 96)):
            add(fam, M, N, K, "gelu_pair", tailsplit=0)
        for mode in (0, 1, 2):
            add(fam, 2049, 516, 192, "gelu_pair", tailsplit=mode)
            add(fam, 2049, 516, 192, "none", tailsplit=mode)
    add("h2", 2049, 288, 160, "gelu_h2", tailsplit=0)
    for kind, M, N, K in (("rows", 257, 132, 64), ("mx", 257, 132, 256), ("mx2", 257, 132, 256), ("mx2", 4097, 516, 256), ("mx2", 4096, 512, 256), ("mx2", 4095, 512, 256)):
        add("fp8", M, N, K, kind)
    for M, N, K in ((65, 68, 17), (130, 4, 96)):
        add("f32", M, N, K, "relu")
    add("f32", 50, 50, 768, "sigmoid", f32_ksplit=1)
    add("bf16", 8224, 2304, 768, "bf16", tailsplit=0)
    add("bf16", 10960, 3072, 768, "gelu_bf16", tailsplit=0)
    # ---- what the comments beside the rules promise (tests/test_gemm_plan_cpu.py COMMENT_FACTS): 43 x 8 = 344 tiles, and the remainder-cut window
    # CUs / 16 <= rem <= CUs / 6 from both sides on 256 CUs (N = 1536: 6 n-tiles, rem = 14 | 20 | 38 | 44; N = 2048: 8 n-tiles, rem = 8 | 16)
    for fam in ("x3", "h2"):
        add(fam, 10960, 2048, 768, "pair", tailsplit=2)
    for M, N in ((45 * 256, 1536), (46 * 256, 1536), (49 * 256, 1536), (50 * 256, 1536), (33 * 256, 2048), (34 * 256, 2048)):
        add("bf16", M, N, 64, "bf16", tailsplit=0)
    return out


CASES = _cases()
