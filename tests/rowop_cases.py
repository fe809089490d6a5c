"""Inputs, float64 references, CPU emulations and per-element bounds of the row and gather operator tests (tests/test_gpu_rowops.py on the
GPU, tests/test_rowop_cases_cpu.py for what can be shown without one): every output form of layernorm_kernel, rowstats_kernel,
deform_sample_kernel with shared projections and the fused operand copy, swiglu_kernel and split3_kernel.  Plain torch on the CPU.

The rule of tests/attention_cases.py and tests/gemm_cases.py: the reference is the float64 value of the statement on the fp32 values the
kernel is given, and every error is normalised PER ELEMENT by the size of what is formed there, never by the tensor's maximum.

LayerNorm:  T = (|x - mu| + max_row|x|) rstd |gamma| + |beta|.  The second term carries the rounding of the mean (a few 2^-24 of the
  row's largest element, multiplied by rstd |gamma| like everything else), which is all there is on constant rows and most of it on
  offset rows.  fp32 rows: |got - want| <= max(LN_FLOOR, 4 d32) T, d32 = the distance per T of torch's fp32 layer_norm on the CPU from
  float64 for that case, 4 = the project's allowance for another accumulation order.  LN_FLOOR = gemm_cases.ACC_FLOOR = 2^-22: the
  emulation of the kernel's own order (`ln_emulate`: lane-strided float4 partial sums, then the 64-lane butterfly) is at most
  1.4e-7 T on the cases here (offset rows at D = 1536; d32 reaches the same 1.4e-7), which the floor holds: it is not raised
  (tests/test_rowop_cases_cpu.py prints both and asserts that the emulation needs no more than the floor).
  Every quantised form is held against the SAME float64 reference with its own rounding added to that bound (`ln_check`).
Deformable gather:  T = sum_p a_p sum_corners w |v|, bound = max(ACC_FLOOR, 4 d32) T + C, C = 2^-21 max(h, w) sum_p a_p (|dv/dx| + |dv/dy|):
  the sampling coordinate is formed in fp32 (sigmoid: expf, an add and a divide, at most 2.5 ulp of a value <= 1; the add of the offset and
  the product with w - 1 half an ulp each: under 4 x 2^-23 (w - 1) in all) and bilinear interpolation is continuous and piecewise linear, so
  a coordinate that is off by that much -- a floor() that lands in the neighbouring cell included -- moves the result by at most the slope
  times it.  No sample is excluded.
SwiGLU:  bound = max(ACC_FLOOR, 4 d32) |want| + 2^-121 |x2|: fp32 expf(-x1) overflows past x1 = -88.73, where the statement as written (and
  as the reference model evaluates it in fp32) gives -0 for a gate of magnitude <= 88.73 e^-88.73 = 2.6e-37 < 2^-121."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.attention_cases import BF16_REL, ACC_REL, dist_by_T, e4m3_half_ulp, mx_block_order, mx_byte_range, split_pair, E4M3_LUT
from tests.gemm_cases import ACC_FLOOR, PAIR_REL, h2_row_bounds, half_ulp_bf16, normal, ratio

LN_FLOOR = ACC_FLOOR
INF = float("inf")

# ------------------------------------------------------------------------------------------------ LayerNorm cases
# D -> the (float4 chunks per lane, exact) arm of ln_dispatch: 64 (1, no) 256 (1, yes) 384 (2, no) 512 (2, yes) 768 (3, yes) 832 (4, no)
# 1024 (4, yes) 1280 (8, no: five chunks, past the switch) 1536 (6, yes) 2048 (8, no: eight full chunks fall through the switch too);
# 4 (one lane), 132 (33 lanes of one chunk) and 2044 (the last lane of the eighth chunk masked) for the forms without a column constraint
LN_D = [64, 256, 384, 512, 768, 832, 1024, 1280, 1536, 2048]
LN_D_FREE = [4, 132, 2044]
LN_FORMS = ["f32", "bf16", "f32_bf16", "pair", "h2", "fp8", "fp8_mx", "f32_s3"]
LN_CONSTRAINED = {"h2": 32, "fp8_mx": 64}
LN_ARMS = {64: (1, False), 256: (1, True), 384: (2, False), 512: (2, True), 768: (3, True), 832: (4, False), 1024: (4, True), 1280: (8, False),
           1536: (6, True), 2048: (8, False), 4: (1, False), 132: (1, False), 2044: (8, False)}
RS_ARMS = {64: (2, False), 256: (2, False), 384: (2, False), 512: (2, False), 768: (3, True), 832: (4, False), 1024: (4, True), 1280: (8, False),
           1536: (6, True), 2048: (8, False), 4: (2, False), 132: (2, False), 2044: (8, False)}
ROW_KINDS = ["normal", "offset", "outlier", "const", "zero"]
CONST, CONST_ADD = 0.3, 0.11


def ln_dims(form):
    return LN_D if form in LN_CONSTRAINED else LN_D + LN_D_FREE


def ln_variants(D):
    """(name, rows, eps, add, beta0, row kinds) of the three launches per D: rows 9, 5 and 1 (rows % 4 != 0: empty waves in the last
    workgroup), both eps, with and without `add`; the all-zero row goes with beta = 0, the constant rows with a beta that is not (with
    beta = 0 a constant row's float64 result is 0 while T is not: its block maxima, and so its scale bytes, would be rounding noise)"""
    i = (LN_D + LN_D_FREE).index(D)
    return [("r9", 9, 1e-6, False, False, [ROW_KINDS[r % 4] for r in range(9)]),
            ("r5", 5, 1e-5, True, True, ["normal", "offset", "outlier", "zero", "normal"]),
            ("r1", 1, 1e-5 if i & 1 else 1e-6, bool(i & 2), False, [ROW_KINDS[i % 4]])]


def ln_input(D, variant):
    """-> (x, add or None, gamma, beta, eps), fp32.  normal: std 2 about 0.5; offset: std 1 about 100; outlier: a normal row with one 1e4;
    const: one number; zero: zeros (with beta = 0 the row's result is exactly zero)"""
    name, rows, eps, add, beta0, kinds = variant
    g = 1.0 + normal(("ln.g", D), (D,), 0.1)
    b = torch.zeros(D) if beta0 else normal(("ln.b", D), (D,), 0.1)
    x = torch.empty(rows, D)
    a = normal(("ln.add", D, name), (rows, D)) if add else None
    for r, kind in enumerate(kinds):
        n = normal(("ln.x", D, name, r), (D,))
        if kind == "normal":
            x[r] = 0.5 + 2.0 * n
        elif kind == "offset":
            x[r] = 100.0 + n
        elif kind == "outlier":
            x[r] = 0.5 + 2.0 * n
            x[r, min(D - 1, D // 2 + 5)] = 1e4
        elif kind == "const":
            x[r] = CONST
            if add:
                a[r] = CONST_ADD
        else:
            x[r] = 0.0
            if add:
                a[r] = 0.0
    return x, a, g, b, eps


def eps32(eps):
    return float(np.float32(eps))


def ln_reference(x, add, g, b, eps):
    """float64 LayerNorm of the fp32 values given -> dict(want, T, d32, rel, xb, mu, rstd, xmax)"""
    v = x.double() + (add.double() if add is not None else 0.0)
    mu = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mu) ** 2).mean(1, keepdim=True) + eps32(eps))
    want = (v - mu) * rstd * g.double() + b.double()
    xmax = v.abs().amax(1, keepdim=True)
    T = ((v - mu).abs() + xmax) * rstd * g.double().abs() + b.double().abs()
    f32 = F.layer_norm(x + add if add is not None else x, (x.shape[1],), g, b, eps32(eps)).double()
    d32 = dist_by_T(f32, want, T)
    rel = max(LN_FLOOR, 4.0 * d32)
    return dict(want=want, T=T, d32=d32, rel=rel, xb=rel * T, mu=mu[:, 0], rstd=rstd[:, 0], xmax=xmax[:, 0], eps=eps32(eps))


# ------------------------------------------------------------------------------------------------ LayerNorm: the kernel's own order on the CPU
def _wave_sum(s):
    """the xor butterfly of dod_common.h wave_sum over the 64 lanes of [rows, 64] fp32 -> [rows]"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lane ^ o]
    return s[:, 0]


def ln_arm(D, rowstats=False):
    """(NCH, EXACT) of the instance ln_dispatch / rowstats_dispatch launch for D (rowops.hip)"""
    nc = D // 4
    nch = (nc + 63) // 64
    if nc == 64 * nch and nch in ((3, 4, 6) if rowstats else (1, 2, 3, 4, 6)):
        return nch, True
    return (2 if nch <= 2 else 4 if nch <= 4 else 8) if rowstats else (1 if nch <= 1 else 2 if nch <= 2 else 4 if nch <= 4 else 8), False


def ln_stats_emulate(v, eps, defect=None, rowstats=False):
    """mean and rstd of fp32 rows v as layernorm_kernel / rowstats_kernel form them: lane l holds the float4 chunks l, l + 64, ... of the
    NCH its instance has; per chunk (x + y) + (z + w), chunks added in order, then the butterfly; the centred squares the same way.
    Defects: "tail_in_mean": the masked lanes are summed too (they hold what follows the row in memory); "var_div": the variance divided
    by 256 NCH"""
    rows, D = v.shape
    nch = ln_arm(D, rowstats)[0]
    W = 256 * nch
    flat = v.reshape(-1)
    idx = (torch.arange(rows)[:, None] * D + torch.arange(W)[None, :]) % flat.numel()        # what a lane without its mask would read
    L = flat[idx].reshape(rows, nch, 64, 4)
    ok = (torch.arange(W) < D).reshape(nch, 64, 4)[None]
    Ls = L if defect == "tail_in_mean" else torch.where(ok, L, torch.zeros(()))
    s = torch.zeros(rows, 64)
    for i in range(nch):
        s = s + ((Ls[:, i, :, 0] + Ls[:, i, :, 1]) + (Ls[:, i, :, 2] + Ls[:, i, :, 3]))
    mean = _wave_sum(s) / torch.tensor(float(D))
    d = torch.where(ok, L - mean[:, None, None, None], torch.zeros(()))
    q = torch.zeros(rows, 64)
    for i in range(nch):
        q = q + ((d[:, i, :, 0] * d[:, i, :, 0] + d[:, i, :, 1] * d[:, i, :, 1]) + (d[:, i, :, 2] * d[:, i, :, 2] + d[:, i, :, 3] * d[:, i, :, 3]))
    var = _wave_sum(q) / torch.tensor(float(W if defect == "var_div" else D))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps32(eps)))
    return mean, rstd


def ln_emulate(x, add, g, b, eps, defect=None):
    """fp32 rows of layernorm_kernel on the CPU"""
    v = x + add if add is not None else x.clone()
    mean, rstd = ln_stats_emulate(v, eps, defect)
    return (v - mean[:, None]) * rstd[:, None] * g + b


def trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def h2_pack_cpu(y):
    """H2 activation rows (dod_common.h) as bytes [rows, 4 D]: fp16 x D | per 16 columns: 16 x e4m3(h), 16 x e4m3((x - h) 2^11)"""
    rows, D = y.shape
    xc = y.float().clamp(-65504, 65504)
    hh = xc.half()
    m8 = hh.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    r8 = ((xc - hh.float()) * 2048).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    grp = torch.stack([m8.reshape(rows, D // 16, 16), r8.reshape(rows, D // 16, 16)], 2).reshape(rows, 2 * D)
    return torch.cat([hh.contiguous().view(torch.uint8).reshape(rows, 2 * D), grp], 1)


def h2_decode(buf, D):
    """bytes [rows, 4 D] -> (fp16 part, e4m3 main, e4m3 remainder / 2^11) float64 (tests/test_gpu_h2.decode)"""
    f8 = lambda t: t.contiguous().view(torch.float8_e4m3fn).double()
    h = buf[:, :2 * D].contiguous().view(torch.float16).double()
    grp = buf[:, 2 * D:].contiguous().view(-1, D // 16, 2, 16)
    return h, f8(grp[:, :, 0, :].reshape(-1, D)), f8(grp[:, :, 1, :].reshape(-1, D)) / 2048.0


def mx_layout(eb):
    """scale bytes in block order [rows, D / 32] -> the kernels' [rows][2][D / 64] layout: block bi at (bi & 1) (D / 64) + (bi >> 1)"""
    rows, nb = eb.shape
    return eb.reshape(rows, nb // 2, 2).permute(0, 2, 1).reshape(rows, nb)


def ln_forms_emulate(y, form, defect=None):
    """the outputs of one launch from its fp32 rows y, as CPU tensors in the device layouts.  Defects: "pair_lo": lo from the truncated
    instead of the rounded hi; "s3_weight_order": [hi | lo | hi]; "bs_plain": the scale byte at the plain block index"""
    from oracle import dinodet_oracle as orc
    rows, D = y.shape
    hi, lo = split_pair(y)
    if defect == "pair_lo":
        lo = (y - trunc_bf16(y)).bfloat16().float()
    out = {}
    if form in ("f32", "f32_bf16", "f32_s3"):
        out["f32"] = y.clone()
    if form in ("bf16", "f32_bf16"):
        out["bf16"] = y.bfloat16()
    if form == "pair":
        out["pair"] = torch.cat([hi, lo], 1).bfloat16()
    if form == "f32_s3":
        out["s3"] = torch.cat([hi, lo, hi] if defect == "s3_weight_order" else [hi, hi, lo], 1).bfloat16()
    if form == "h2":
        out["h2"] = h2_pack_cpu(y)
    if form == "fp8":
        amax = y.abs().amax(1)
        sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        out["scale"] = sc
        out["q8"] = (y * (1.0 / sc)[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    if form == "fp8_mx":
        eb = orc._mx_scales(y)
        inv = torch.exp2((127 - eb).double()).float()
        out["q8"] = (y.reshape(rows, D // 32, 32) * inv[..., None]).reshape(rows, D).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        out["bs"] = (eb if defect == "bs_plain" else mx_layout(eb)).to(torch.uint8)
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm: the checks
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def ln_check(form, out, R):
    """every bound of one launch's outputs against the float64 reference R -> {check name: worst |got - want| / bound}; an exactness
    condition that fails counts as infinite.  A launch passes when no ratio exceeds 1"""
    want, xb = R["want"], R["xb"]
    rows, D = want.shape
    res = {}
    zero = (R["T"] == 0).all(1)                                  # all-zero rows with beta = 0
    if "f32" in out:
        res["f32"] = ratio(out["f32"], want, xb)
    if "bf16" in out:
        res["bf16"] = ratio(out["bf16"].double(), want, xb + half_ulp_bf16(want.abs() + xb))
        if "f32" in out:
            res["bf16 == rne(f32)"] = 0.0 if torch.equal(_bits(out["bf16"]), _bits(out["f32"].bfloat16())) else INF
    if "pair" in out:
        p = out["pair"].double()
        res["pair hi + lo"] = ratio(p[:, :D] + p[:, D:], want, xb + PAIR_REL * want.abs())
        res["pair hi"] = ratio(p[:, :D], want, xb + half_ulp_bf16(want.abs() + xb))
    if "s3" in out:
        s3 = out["s3"]
        res["s3 hi + lo"] = ratio(s3[:, :D].double() + s3[:, 2 * D:].double(), want, xb + PAIR_REL * want.abs())
        res["s3 planes 0 == 1"] = 0.0 if torch.equal(_bits(s3[:, :D]), _bits(s3[:, D:2 * D])) else INF
        hi, lo = split_pair(out["f32"])
        res["s3 == split(f32)"] = 0.0 if torch.equal(_bits(s3), _bits(torch.cat([hi, hi, lo], 1).bfloat16())) else INF
    if "h2" in out:
        h, m8, r8 = h2_decode(out["h2"], D)
        for name, (got, bound) in zip(("h2 h + r", "h2 h"), h2_row_bounds(want, xb, h, r8)):
            res[name] = ratio(got, want, bound)
        res["h2 main == e4m3(h)"] = 0.0 if torch.equal(m8, h.float().clamp(-448, 448).to(torch.float8_e4m3fn).double()) else INF
    if "scale" in out:
        sc = out["scale"].double()
        amax = want.abs().amax(1)
        sc_want = torch.where(zero, torch.ones_like(amax), amax / 448.0)
        sc_b = xb.amax(1) / 448.0 + 2.0 ** -24 * sc_want * (~zero)
        maybe0 = (sc == 1.0) & (amax <= xb.amax(1))                      # a row the bound allows to be all zero may carry the zero row's scale
        res["fp8 scale"] = ratio(torch.where(maybe0, sc_want, sc), sc_want, sc_b)
        scs = sc[:, None]
        res["fp8 values"] = ratio(E4M3_LUT[out["q8"].long()] * scs, want, xb + e4m3_half_ulp((want.abs() + xb) / scs) * scs)
        res["fp8 zero rows"] = 0.0 if bool((out["q8"][zero] == 0).all()) and bool((out["scale"][zero] == 1.0).all()) else INF
    if "bs" in out:
        lo, hi = mx_byte_range(want, xb / (BF16_REL + ACC_REL))           # the fp32 bound as the value margin
        eb = mx_block_order(out["bs"], D).long()
        res["mx scale bytes"] = 0.0 if bool(((eb >= lo) & (eb <= hi)).all()) else INF
        sc = torch.exp2((eb.clamp(1, 253) - 127).double())[..., None].expand(rows, D // 32, 32).reshape(rows, D)
        res["mx values"] = ratio(E4M3_LUT[out["q8"].long()] * sc, want, xb + e4m3_half_ulp((want.abs() + xb) / sc) * sc)
        res["mx zero rows"] = 0.0 if bool((out["q8"][zero] == 0).all()) and bool((eb[zero] == 1).all()) else INF
    return res


def mx_undecided(R):
    """share of the 32-column blocks whose scale byte the reference does not decide within the fp32 bound"""
    lo, hi = mx_byte_range(R["want"], R["xb"] / (BF16_REL + ACC_REL))
    return float((lo != hi).double().mean())


# ------------------------------------------------------------------------------------------------ row statistics (the folded LayerNorm's first block)
RS_KINDS = ["bf16", "pair", "h2"]


def rs_dims(kind):
    return LN_D if kind == "h2" else LN_D + LN_D_FREE


def rs_reference(x, eps):
    """float64 (mean, rstd) with their bounds.  mean: rel max_row|x|.  rstd: rel rstd + rstd^3 / 2 (rel max_row|x|)^2 -- the variance is
    taken about the computed mean, whose allowed error enters it squared (d rstd / d var = -rstd^3 / 2): all there is on a constant row"""
    v = x.double()
    mu = v.mean(1)
    rstd = 1.0 / torch.sqrt(((v - mu[:, None]) ** 2).mean(1) + eps32(eps))
    xmax = v.abs().amax(1)
    var32, mu32 = torch.var_mean(x, 1, unbiased=False)
    r32 = (1.0 / torch.sqrt(var32 + eps32(eps))).double()
    d_mu = dist_by_T(mu32.double(), mu, xmax)
    rel_mu = max(LN_FLOOR, 4.0 * d_mu)

    def rstd_bound(rel):
        return rel * rstd + 0.5 * rstd ** 3 * (rel_mu * xmax) ** 2
    rel_rs = max(LN_FLOOR, 4.0 * float(((r32 - rstd).abs() - rstd_bound(0.0)).clamp(min=0).div(rstd).max()))
    return dict(mu=mu, rstd=rstd, mu_b=rel_mu * xmax, rstd_b=rstd_bound(rel_rs))


def rs_operand_cpu(x, kind):
    """the operand copy of x itself, bit for bit: bf16 rows, [hi | lo] or H2 bytes"""
    if kind == "bf16":
        return x.bfloat16()
    if kind == "pair":
        return torch.cat(split_pair(x), 1).bfloat16()
    return h2_pack_cpu(x)


def rs_check(kind, stats, op, x, R):
    res = {"mean": ratio(stats[:, 0], R["mu"], R["mu_b"]), "rstd": ratio(stats[:, 1], R["rstd"], R["rstd_b"])}
    res["operand == split(x)"] = 0.0 if torch.equal(_bits(op), _bits(rs_operand_cpu(x, kind))) else INF
    return res


# ------------------------------------------------------------------------------------------------ deformable gather
DF_B, DF_Q = 3, 5               # B Q Hd is no multiple of 4 when Hd is odd: the last workgroup has empty waves
# (h, w, Hd, dh, P): one point and a one-row grid; a one-column grid with dh = 65 (one lane of the second group); dh = 96 (half of it);
# dh = 128 and P = 8 (both limits); the decoder's 37 x 37 grid with 8 heads; dh = 1 (one lane)
DF_CASES = [(1, 17, 1, 32, 1), (5, 1, 3, 65, 2), (2, 13, 3, 96, 2), (16, 16, 2, 128, 8), (37, 37, 8, 96, 2), (7, 9, 5, 1, 4)]
DF_PAD = 3
DF_OFF_STD = 0.2
COORD_REL = 2.0 ** -21


def df_ncat(case):
    return 2 + 3 * case[2] * case[4]


def df_input(case):
    """-> (proj [B Q, ncat + 3] with NaN in the pad columns, values [B N, Hd dh]).  Reference logits +-30 and 0 among normal ones, offsets of
    std 0.2 (a third of the points leave [0, 1] on an axis and clamp), weight logits of std 25 cut at +-60 with both ends present"""
    h, w, Hd, dh, P = case
    R, ncat = DF_B * DF_Q, df_ncat(case)
    proj = torch.full((R, ncat + DF_PAD), float("nan"))
    ref = normal(("df.ref", case), (R, 2), 1.5)
    for i in range(R):
        if i % 5 == 0:
            ref[i, 0] = 30.0
        elif i % 5 == 1:
            ref[i, 1] = -30.0
        elif i % 5 == 2:
            ref[i, i % 2] = 0.0
    proj[:, :2] = ref
    proj[:, 2:2 + 2 * Hd * P] = normal(("df.off", case), (R, 2 * Hd * P), DF_OFF_STD)
    awl = normal(("df.aw", case), (R, Hd * P), 25.0).clamp(-60, 60)
    awl[0::3, 0] = 60.0
    awl[1::3, -1] = -60.0
    proj[:, 2 + 2 * Hd * P:ncat] = awl
    values = 0.5 + normal(("df.v", case), (DF_B * h * w, Hd * dh))
    return proj, values


def df_eval(proj, values, case, dtype, shared=False, defect=None, parts=False):
    """the reference statement (deform.hip's header; oracle.deformable_sample) in `dtype`, the kernel's operation order -> out [B Q, Hd dh];
    shared: proj has Q rows used by every image.  parts: also (T, C) in the same dtype.  Defects: "swap_corners": (y1, x0) and (y0, x1)
    exchanged; "shared_bq": the shared projections indexed by b Q + q (proj must then hold B Q rows)"""
    h, w, Hd, dh, P = case
    B, Q, N, ncat = DF_B, DF_Q, h * w, df_ncat(case)
    p = proj[:, :ncat].to(dtype)
    if shared and defect != "shared_bq":
        p = p[:Q].repeat(B, 1)
    ref = 1.0 / (1.0 + torch.exp(-p[:, :2]))
    off = p[:, 2:2 + 2 * Hd * P].reshape(B * Q, Hd, P, 2)
    awl = p[:, 2 + 2 * Hd * P:].reshape(B * Q, Hd, P)
    aw = torch.exp(awl - awl.amax(-1, keepdim=True))
    a = aw / aw.sum(-1, keepdim=True)
    lx = (ref[:, None, None, 0] + off[..., 0]).clamp(0, 1) * (w - 1)
    ly = (ref[:, None, None, 1] + off[..., 1]).clamp(0, 1) * (h - 1)
    x0, y0 = torch.floor(lx).long(), torch.floor(ly).long()
    x1, y1 = (x0 + 1).clamp(0, w - 1), (y0 + 1).clamp(0, h - 1)
    x0, y0 = x0.clamp(0, w - 1), y0.clamp(0, h - 1)
    wx1 = lx - x0.to(dtype)
    wy1 = ly - y0.to(dtype)
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    v = values.to(dtype).reshape(B, N, Hd, dh)
    bI = (torch.arange(B * Q) // Q)[:, None, None]
    hI = torch.arange(Hd)[None, :, None]
    g = lambda yy, xx: v[bI, yy * w + xx, hI]                        # [B Q, Hd, P, dh]
    v00, v01, v10, v11 = g(y0, x0), g(y1, x0), g(y0, x1), g(y1, x1)
    if defect == "swap_corners":
        v01, v10 = v10, v01
    w00, w01, w10, w11 = [t[..., None] for t in (wx0 * wy0, wx0 * wy1, wx1 * wy0, wx1 * wy1)]
    s = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11
    out = torch.zeros(B * Q, Hd, dh, dtype=dtype)
    for pt in range(P):
        out = out + s[:, :, pt] * a[:, :, pt, None]
    out = out.reshape(B * Q, Hd * dh)
    if not parts:
        return out
    T = ((v00.abs() * w00 + v01.abs() * w01 + v10.abs() * w10 + v11.abs() * w11) * a[..., None]).sum(2).reshape(B * Q, Hd * dh)
    sx = (v10 - v00).abs() * wy0[..., None] + (v11 - v01).abs() * wy1[..., None]
    sy = (v01 - v00).abs() * wx0[..., None] + (v11 - v10).abs() * wx1[..., None]
    C = COORD_REL * max(h, w) * ((sx + sy) * a[..., None]).sum(2).reshape(B * Q, Hd * dh)
    return out, T, C


def df_reference(proj, values, case, shared):
    want, T, C = df_eval(proj, values, case, torch.float64, shared, parts=True)
    f32 = df_eval(proj, values, case, torch.float32, shared).double()
    d32 = float((((f32 - want).abs() - C).clamp(min=0) / T.clamp(min=1e-300)).max())
    rel = max(ACC_FLOOR, 4.0 * d32)
    return dict(want=want, T=T, C=C, d32=d32, rel=rel, bound=rel * T + C)


def df_clamp_share(proj, case):
    Hd, P = case[2], case[4]
    p = proj.double()
    ref = torch.sigmoid(p[:, :2])
    loc = ref[:, None, :] + p[:, 2:2 + 2 * Hd * P].reshape(-1, Hd * P, 2)
    return float(((loc < 0) | (loc > 1)).any(-1).double().mean())


def df_spill_second_half(out, case):
    """the defect `lanes 64.. written whatever dh is`: every item stores 128 columns from its head's first one, the items taken last to
    first, so what an item spills (zeros: those lanes accumulate nothing) lands on the item after it"""
    h, w, Hd, dh, P = case
    flat = torch.cat([out.reshape(-1), torch.zeros(128, dtype=out.dtype)])
    res = flat.clone()
    for item in reversed(range(DF_B * DF_Q * Hd)):
        o = item * dh
        res[o:o + dh] = flat[o:o + dh]
        res[o + max(dh, 64):o + 128] = 0.0
    return res[:out.numel()].reshape(out.shape)


def df_check(out, out3, R):
    res = {"out": ratio(out, R["want"], R["bound"])}
    if out3 is not None:
        hi, lo = split_pair(out)
        res["out3 == split(out)"] = 0.0 if torch.equal(_bits(out3), _bits(torch.cat([hi, hi, lo], 1).bfloat16())) else INF
    return res


# ------------------------------------------------------------------------------------------------ SwiGLU gate
# (rows, Fh): one wave's worth, a full row of 64, and 1030 x 2048 > 8192 x 256 elements: the grid-stride loop takes a second pass
SW_CASES = [(3, 5), (7, 64), (1030, 2048)]
SW_GATES = [0.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4]
SW_UNDER = 2.0 ** -121


def sw_input(rows, Fh, bf16):
    """[rows, 2 Fh]: x1 | x2 chunked.  The special gates sit at the head of the flattened x1 (and again at its tail)"""
    x = normal(("sw", rows, Fh), (rows, 2 * Fh), 2.0)
    g = torch.tensor(SW_GATES)
    x1 = x[:, :Fh].reshape(-1).clone()
    n = min(len(g), x1.numel())
    x1[:n] = g[:n]
    if x1.numel() >= 2 * n:
        x1[x1.numel() - n:] = g[:n]
    x[:, :Fh] = x1.reshape(rows, Fh)
    return x.bfloat16() if bf16 else x


def sw_eval(x, dtype, defect=None):
    """silu(x1) * x2 as the kernel writes it, a / (1 + exp(-a)) * b.  Defect "interleaved": the halves taken as adjacent pairs"""
    Fh = x.shape[1] // 2
    t = x.to(dtype)
    a, b = (t[:, 0::2], t[:, 1::2]) if defect == "interleaved" else (t[:, :Fh], t[:, Fh:])
    return a / (1.0 + torch.exp(-a)) * b


def sw_reference(x, bf16):
    want = sw_eval(x, torch.float64)
    under = SW_UNDER * x[:, x.shape[1] // 2:].double().abs()
    f32 = sw_eval(x, torch.float32).double()
    d32 = float((((f32 - want).abs() - under).clamp(min=0) / want.abs().clamp(min=1e-300)).max())
    rel = max(ACC_FLOOR, 4.0 * d32)
    bound = rel * want.abs() + under
    if bf16:
        bound = bound + half_ulp_bf16(want.abs() + bound)
    return dict(want=want, d32=d32, rel=rel, bound=bound)


# ------------------------------------------------------------------------------------------------ bf16x3 split
# (rows, K): one float4, an odd row count with K = 132, and 1100 x 1024 > 4096 x 256 elements (a second pass of the grid-stride loop)
S3_CASES = [(1, 4), (5, 132), (1100, 1024)]
S3_PITCH_PAD = 8


def s3_input(rows, K):
    x = normal(("s3", rows, K), (rows, K), 3.0)
    x.reshape(-1)[:4] = torch.tensor([1e5, -7e4, 3e-6, 0.0])
    return x


def s3_cpu(x, weight_order):
    hi, lo = split_pair(x)
    return torch.cat([hi, lo, hi] if weight_order else [hi, hi, lo], 1).bfloat16()
