"""State dicts, float64 definitions, CPU packers and per-element bounds of the weight packer's tests (tests/test_gpu_pack.py on the GPU, which
reads what dod_finalize_weights stored through dod_test_packed_*; tests/test_pack_cases_cpu.py for what can be shown without one).  Plain torch
on the CPU.

The rule of tests/gemm_cases.py: the reference is the float64 value of the statement on the fp32 values the packer is given, and every error
is normalised PER ELEMENT by the size of what is formed there, never by the tensor's maximum.

What the packer forms (csrc/dod_pack.hip, csrc/rowops.hip):
  merge       W_eff = W + alpha B A                              T = |W| + |alpha| sum_t |B| |A|
  QKV         rows [q | k | v] of W_eff and of b
  fold        W' = W_eff diag(gamma)                             T = T_merge |gamma|
              b' = b + W_eff beta                                T = |b| + sum_k |W_eff| |beta|
              c  = sum_k W' (of bf16-rounded W' in the bf16 mode) T = sum_k |W'|
  SwiGLU      row 2i = x1_i, row 2i + 1 = x2_i of W', b' and so c (after the fold)
  patch       [D, 3 p p] padded with zeros along K; the fused kernel's order: column s 32 + r 16 + j = W[n][c][2 si + r][j], step s = c (p / 2) + si,
              zero for j >= p
  decoder     cat_w rows [reference (2) | offsets (Hd P 2) | weights (Hd P)], split3 copies [hi | lo | hi]
Bound on a merged / folded value: max(ACC_FLOOR, 4 d32) T, d32 = the distance per T of torch's fp32 CPU restatement (`block_linears` in float32)
from float64 for that operand of that case.  The format's own rounding is ADDED to that bound (`check_operand`): half a bf16 ulp; PAIR_REL of
|want| for hi + lo; gemm_cases.h2_row_bounds for H2 weight rows (with the row's 2^e on the remainder); half an e4m3 step at the row's or
block's scale.  Where no arithmetic precedes the format (no LoRA, no fold) the bytes must equal the CPU packers the suite already pins
(bf16 RNE, split_pair, the H2 weight rows of tests/test_gpu_h2.py, test_gpu_fp8.quant_ref / mx_ref)."""
from dataclasses import dataclass

import numpy as np
import torch

from dinov2_od_amd import synth
from dinov2_od_amd.config import DecoderConfig
from tests.attention_cases import BF16_REL, ACC_REL, E4M3_LUT, e4m3_half_ulp, mx_block_order, mx_byte_range, split_pair
from tests.gemm_cases import ACC_FLOOR, PAIR_REL, dequant_mx, dequant_rows, h2_row_bounds, half_ulp_bf16, ratio, seed_of

INF = float("inf")
MODES = ["fp32", "bf16", "bf16x3", "fp16x2", "fp8"]
FAMILIES = ["synth", "ckpt"]
ALPHA = 0.75                     # not 1: a dropped or doubled alpha shows


@dataclass(frozen=True)
class BB:
    """the fields of config.BackboneConfig that synth and the packer read, with the MLP width stated directly"""
    hidden: int
    swiglu: bool
    ffn_hidden: int
    patch: int = 14
    target_dim: int = 0
    layers: int = 2
    lora_layers: int = 1         # block 0 plain, block 1 merged
    lora_r: int = 3
    lora_alpha: float = ALPHA
    pos_grid: int = 3
    ln_eps: float = 1e-6

    @property
    def heads(self):
        return self.hidden // 64


@dataclass(frozen=True)
class Case:
    name: str
    bb: BB
    decoder: str                 # "tied" / "untied" (deformable) or "dense"
    modes: tuple

    @property
    def dc(self):
        return DecoderConfig(num_queries=7, hidden_dim=128, nheads=4, num_layers=2, num_classes=5, dim_feedforward=192, n_points=2,
                             use_deformable=self.decoder != "dense")


ALL = tuple(MODES)
# the smallest configurations that reach each branch of the packer (hidden, MLP, F -> branch):
#   128 GELU 512      plain GELU MLP; fp8: per-row scales, fc2 stays bf16
#   128 SwiGLU 344    F % 32 != 0.  dod_create takes F % 64 != 0 in the fp32 mode only, so the compensated modes' "un-interleaved gate" arm of
#                     dod_pack.hip cannot be reached through the ABI: the case runs in fp32, and the other modes must reject it
#   384 SwiGLU 1024   hidden % 256 != 0: fp8 takes per-row scales
#   768 SwiGLU 2048   fp8 takes block-scaled weights (fp8 and bf16 only: the widest case)
CASES = [
    Case("gelu128", BB(128, False, 512), "tied", ALL),
    Case("gelu128-p16-proj-dense", BB(128, False, 512, patch=16, target_dim=128), "dense", ALL),
    Case("swiglu128-f344", BB(128, True, 344), "tied", ("fp32",)),
    Case("swiglu384-p16-proj-untied", BB(384, True, 1024, patch=16, target_dim=128), "untied", ALL),
    Case("swiglu768-proj-dense", BB(768, True, 2048, target_dim=128), "dense", ("bf16", "fp8")),
]
SMALL_GLU = Case("swiglu128-f192", BB(128, True, 192), "tied", ALL)      # the smallest case with the interleave (the CPU test's planted defects)
REJECTED = [("swiglu128-f344", m) for m in MODES if m != "fp32"]


def case(name):
    return next(c for c in CASES + [SMALL_GLU] if c.name == name)


# ------------------------------------------------------------------------------------------------ state dicts
def _t(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).clone() for k, v in sd.items()}


def state_dict(cs, family):
    """fp32 CPU tensors under the reference's keys.  "synth": synth.detector_state_dict as it is.  "ckpt": the checkpoint-like edit below.
    "untied" decoders get their own value_proj (and output_proj) per layer; "tied" ones share ONE tensor object per key across layers."""
    sd = _t(synth.detector_state_dict(cs.bb, cs.dc, seed=3))
    dp = "decoder.decoder.layers."
    if cs.decoder == "tied":
        for k in [k for k in sd if k.startswith(dp + "1.")]:
            sd[k] = sd[k.replace(dp + "1.", dp + "0.")]
    elif cs.decoder == "untied":
        for k in [k for k in sd if k.startswith(dp + "1.cross_attn.")]:
            sd[k] = sd[k] + torch.from_numpy(synth.normal(5, k, tuple(sd[k].shape), 0.01))
    if family == "ckpt":
        checkpoint_like(sd, cs)
    return sd


def checkpoint_like(sd, cs):
    """in place, seeded by the key: LayerScale log-uniform in [1e-5, 1]; LN gamma with three channels at about 10x and one at exactly 0, LN beta
    with outliers at the same channels; per linear one row at 100x, one all-zero row and one column at 50x; block 1's query LoRA with
    lora_B = 0 (the reference's initial state)"""
    for k in sorted(sd):
        if not k.startswith("backbone."):
            continue
        rng = np.random.default_rng(seed_of("ckpt", k))
        v = sd[k]
        if "layer_scale" in k:
            sd[k] = torch.from_numpy(np.exp(rng.uniform(np.log(1e-5), 0.0, v.shape)).astype(np.float32))
        elif ".norm1." in k or ".norm2." in k or "dino.layernorm." in k:
            D = v.shape[0]
            ch = np.random.default_rng(seed_of("ckpt", k.rsplit(".", 1)[0])).permutation(D)[:4]      # the same channels for weight and bias
            v = v.clone()
            if k.endswith(".weight"):
                v[ch[:3]] *= torch.tensor([10.0, -9.0, 11.0])
                v[ch[3]] = 0.0
            else:
                v[ch[:3]] = torch.tensor([3.0, -2.5, 4.0])
                v[ch[3]] = -1.5
            sd[k] = v
        elif k.endswith(".weight") and v.dim() == 2 and "lora_" not in k:
            v = v.clone()
            r = rng.permutation(v.shape[0])[:2]
            c = int(rng.integers(v.shape[1]))
            v[:, c] *= 50.0
            v[r[0]] *= 100.0
            v[r[1]] = 0.0
            sd[k] = v
        elif k.endswith("layer.1.attention.attention.query.lora_B.weight"):
            sd[k] = torch.zeros_like(v)
    return sd


# ------------------------------------------------------------------------------------------------ the statement, in any dtype
def interleave(x, F):
    """rows [x1 (F) | x2 (F)] -> row 2i = x1_i, row 2i + 1 = x2_i"""
    return torch.stack([x[:F], x[F:]], 1).reshape(x.shape)


def fold_expected(cs, mode, fold_opt):
    return bool(fold_opt) and mode in ("bf16", "bf16x3", "fp16x2") and cs.bb.hidden % 32 == 0


def glu_expected(cs, mode):
    if not cs.bb.swiglu:
        return False
    return cs.bb.ffn_hidden % 32 == 0 if mode in ("bf16x3", "fp16x2") else mode in ("bf16", "fp8")


def linear_format(cs, mode, which):
    if mode == "fp16x2":
        return "h2w"
    if mode == "bf16x3":
        return "pair"
    if mode == "fp8" and not (which == "fc2" and not cs.bb.swiglu):
        mx = cs.bb.hidden % 256 == 0 and (not cs.bb.swiglu or cs.bb.ffn_hidden % 256 == 0)
        return "e4m3_mx" if mx else "e4m3_rows"
    return "bf16" if mode in ("bf16", "fp8") else "f32"


def block_linears(sd, cs, i, fold, glu, dtype, defect=None):
    """the four linears of block i as the packer forms them before any format -> {name: dict(w, b, c, T_w, T_b, T_c, arith)} in `dtype`
    (T_* always float64, from the fp32 inputs).  Defects: "alpha_half", "qk_swap", "beta_after_interleave", "c_without_gamma"."""
    bb = cs.bb
    D, F = bb.hidden, bb.ffn_hidden
    lp = f"backbone.dino.encoder.layer.{i}."
    alpha = bb.lora_alpha * (0.5 if defect == "alpha_half" else 1.0)

    def eff(prefix):
        if prefix + ".linear.weight" in sd:
            W, A, B = sd[prefix + ".linear.weight"], sd[prefix + ".lora_A.weight"], sd[prefix + ".lora_B.weight"]
            w = W.to(dtype) + torch.tensor(alpha, dtype=torch.float32).to(dtype) * (B.to(dtype) @ A.to(dtype))
            T = W.double().abs() + abs(float(np.float32(bb.lora_alpha))) * (B.double().abs() @ A.double().abs())
            return w, sd[prefix + ".linear.bias"].to(dtype), T, True
        W = sd[prefix + ".weight"]
        return W.to(dtype), sd[prefix + ".bias"].to(dtype), W.double().abs(), False

    def folded(w, b, T, arith, norm, F_glu=0):
        out = dict(w=w, b=b, c=None, T_w=T, T_b=b.double().abs(), T_c=None, arith=arith, arith_b=False)
        if fold:
            g, be = sd[lp + norm + ".weight"], sd[lp + norm + ".bias"]
            out["b"] = b + w @ be.to(dtype)
            out["T_b"] = b.double().abs() + w.double().abs() @ be.double().abs()
            out["w"] = w * g.to(dtype)
            out["T_w"] = T * g.double().abs()
            out["arith"] = out["arith_b"] = True
            csrc = w if defect == "c_without_gamma" else out["w"]
            out["c"] = csrc.sum(1)
            out["T_c"] = out["w"].double().abs().sum(1)
        if F_glu:
            bias = out["b"]
            if defect == "beta_after_interleave" and fold:
                bias = interleave(b, F_glu) + w @ sd[lp + norm + ".bias"].to(dtype)
                out["b"] = bias
            else:
                out["b"] = interleave(bias, F_glu)
            for k in ("w", "T_w", "T_b", "c", "T_c"):
                if out[k] is not None:
                    out[k] = interleave(out[k], F_glu)
        return out

    parts = [eff(lp + "attention.attention." + n) for n in (("key", "query", "value") if defect == "qk_swap" else ("query", "key", "value"))]
    res = {"qkv": folded(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
                         any(p[3] for p in parts), "norm1")}
    w, b, T, ar = eff(lp + "attention.output.dense")
    res["o"] = dict(w=w, b=b, c=None, T_w=T, T_b=b.double().abs(), T_c=None, arith=ar, arith_b=False)
    n1, n2 = ("mlp.weights_in", "mlp.weights_out") if bb.swiglu else ("mlp.fc1", "mlp.fc2")
    res["fc1"] = folded(*eff(lp + n1), "norm2", F if glu else 0)
    w, b, T, ar = eff(lp + n2)
    res["fc2"] = dict(w=w, b=b, c=None, T_w=T, T_b=b.double().abs(), T_c=None, arith=ar, arith_b=False)
    return res


def patch_im2col(W, Kp):
    D = W.shape[0]
    out = torch.zeros(D, Kp, dtype=W.dtype)
    out[:, :W[0].numel()] = W.reshape(D, -1)
    return out


def patch_fused_order(W):
    """[D, 3, p, p] -> [D, 3 (p / 2) 32]: column (c (p / 2) + si) 32 + r 16 + j = W[n][c][2 si + r][j], zero for j >= p"""
    D, _, p, _ = W.shape
    out = torch.zeros(D, 3, p // 2, 2, 16, dtype=W.dtype)
    out[..., :p] = W.reshape(D, 3, p // 2, 2, p)
    return out.reshape(D, 3 * (p // 2) * 32)


def rel_of(d32):
    return max(ACC_FLOOR, 4.0 * d32)


def _d32(f32, f64, T):
    err = (f32.double() - f64).abs()
    pos = T > 0
    assert bool((err[~pos] == 0).all())
    return float((err[pos] / T[pos]).max()) if bool(pos.any()) else 0.0


@dataclass
class Spec:
    """one packed operand: its expected format and shape, the float64 value `want` [rows, cols] with the bound `xb` of the fp32 value that is
    then formatted (None: no arithmetic, the bytes must equal the CPU packer's of `src`), and for a block linear the aux arrays"""
    format: str
    rows: int
    cols: int
    want: torch.Tensor = None
    xb: torch.Tensor = None
    src: torch.Tensor = None          # fp32 source where exact
    pad_cols: int = 0                 # zero columns behind `cols` (per plane)
    bias: tuple = None                # (want, bound, None) or, where exact, (want, None, fp32 source)
    csum: tuple = None                # (T_c, rel of the summation)
    d32: dict = None
    glu: bool = False
    fold: bool = False
    vp_alias: int = -1


def reference(sd, cs, mode, fold_opt=True, fused_patch=True):
    """{operand name: Spec} of everything dod_finalize_weights keeps for this case, mode and test option (absent operands: format "absent")"""
    bb, dc = cs.bb, cs.dc
    D, F, p, Dd = bb.hidden, bb.ffn_hidden, bb.patch, dc.hidden_dim
    is16, x3 = mode in ("bf16", "fp8"), mode in ("bf16x3", "fp16x2")
    wfmt = "bf16" if is16 else "f32"
    fold, glu = fold_expected(cs, mode, fold_opt), glu_expected(cs, mode)
    S = {}

    def exact(name, t, fmt="f32", pad=0):
        t = t.reshape(1, -1) if t.dim() == 1 else t.reshape(t.shape[0], -1)
        S[name] = Spec(fmt, t.shape[0], t.shape[1], want=t.double(), src=t.float(), pad_cols=pad)

    def absent(name):
        S[name] = Spec("absent", 0, 0)

    e = "backbone.dino.embeddings."
    Wp = sd[e + "patch_embeddings.projection.weight"]
    K = 3 * p * p
    exact("Wpatch", Wp, wfmt, ((K + 63) // 64 * 64 if is16 else K) - K)
    exact("Wpatch2", Wp, "pair", (K + 31) // 32 * 32 - K) if x3 else absent("Wpatch2")
    exact("Wpe", patch_fused_order(Wp), "pair" if x3 else "bf16") if (is16 or x3) and p in (14, 16) and fused_patch else absent("Wpe")
    exact("bpatch", sd[e + "patch_embeddings.projection.bias"])
    exact("cls", sd[e + "cls_token"].reshape(-1))
    exact("pos", sd[e + "position_embeddings"][0])
    exact("lnfw", sd["backbone.dino.layernorm.weight"])
    exact("lnfb", sd["backbone.dino.layernorm.bias"])
    if bb.target_dim:
        exact("Wproj", sd["backbone.projection.weight"], "pair" if x3 else wfmt)
        exact("bproj", sd["backbone.projection.bias"])
    else:
        absent("Wproj"), absent("bproj")
    for i in range(bb.layers):
        lp = f"backbone.dino.encoder.layer.{i}."
        for short, key in (("ln1w", "norm1.weight"), ("ln1b", "norm1.bias"), ("ln2w", "norm2.weight"), ("ln2b", "norm2.bias"),
                           ("ls1", "layer_scale1.lambda1"), ("ls2", "layer_scale2.lambda1")):
            exact(f"block.{i}.{short}", sd[lp + key])
            S[f"block.{i}.{short}"].glu, S[f"block.{i}.{short}"].fold = glu, fold          # the flags are the block's
        l64, l32 = block_linears(sd, cs, i, fold, glu, torch.float64), block_linears(sd, cs, i, fold, glu, torch.float32)
        for n in ("qkv", "o", "fc1", "fc2"):
            a, b = l64[n], l32[n]
            sp = Spec(linear_format(cs, mode, n), a["w"].shape[0], a["w"].shape[1], want=a["w"], glu=glu, fold=fold, d32={})
            if a["arith"]:
                sp.d32["w"] = _d32(b["w"], a["w"], a["T_w"])
                sp.xb = rel_of(sp.d32["w"]) * a["T_w"]
            else:
                sp.src = b["w"]
            if a["arith_b"]:
                sp.d32["bias"] = _d32(b["b"], a["b"], a["T_b"])
                sp.bias = (a["b"], rel_of(sp.d32["bias"]) * a["T_b"], None)
            else:
                sp.bias = (a["b"], None, b["b"])
            if a["c"] is not None:
                addends = bf(b["w"]) if mode == "bf16" else b["w"]                  # d32 of the summation alone, of the same fp32 addends
                sp.d32["csum"] = _d32(addends.sum(1), addends.double().sum(1), a["T_c"])
                sp.csum = (a["T_c"], rel_of(sp.d32["csum"]))
            S[f"block.{i}.{n}"] = sp
    # ---- decoder: fp32 copies, split3 copies of the query-side weights, the memory-side projections in the operand dtype
    dp = "decoder."
    s3 = is16 or x3
    exact("query", sd[dp + "query_embed.weight"])
    for short, key in (("cls_w", "class_embed.weight"), ("cls_b", "class_embed.bias"), ("bb0_w", "bbox_embed.mlp.0.weight"), ("bb0_b", "bbox_embed.mlp.0.bias"),
                       ("bb2_w", "bbox_embed.mlp.2.weight"), ("bb2_b", "bbox_embed.mlp.2.bias")):
        exact(short, sd[dp + key])
    exact("bb0_w3", sd[dp + "bbox_embed.mlp.0.weight"], "split3w") if s3 else absent("bb0_w3")
    deform_only = ["cat_w", "cat_b", "op_w", "op_b", "op_w3", "vp_w", "vp_w2", "vp_b"]
    dense_only = ["ca_q_w", "ca_q_b", "ca_kv_w", "ca_kv_w2", "ca_kv_b", "ca_out_w", "ca_out_b", "ca_q_w3", "ca_out_w3"]
    for j in range(dc.num_layers):
        lp, o = f"{dp}decoder.layers.{j}.", f"dec.{j}."
        for short, key in (("in_w", "self_attn.in_proj_weight"), ("in_b", "self_attn.in_proj_bias"), ("out_w", "self_attn.out_proj.weight"),
                           ("out_b", "self_attn.out_proj.bias"), ("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("n2w", "norm2.weight"),
                           ("n2b", "norm2.bias"), ("n3w", "norm3.weight"), ("n3b", "norm3.bias"), ("l1w", "linear1.weight"), ("l1b", "linear1.bias"),
                           ("l2w", "linear2.weight"), ("l2b", "linear2.bias")):
            exact(o + short, sd[lp + key])
        for short, key in (("in_w3", "self_attn.in_proj_weight"), ("out_w3", "self_attn.out_proj.weight"), ("l1w3", "linear1.weight"), ("l2w3", "linear2.weight")):
            exact(o + short, sd[lp + key], "split3w") if s3 else absent(o + short)
        if dc.use_deformable:
            names = ("reference_points_proj", "cross_attn.sampling_offsets", "cross_attn.attention_weights")
            exact(o + "cat_w", torch.cat([sd[lp + n + ".weight"] for n in names]))
            exact(o + "cat_b", torch.cat([sd[lp + n + ".bias"] for n in names]))
            exact(o + "op_w", sd[lp + "cross_attn.output_proj.weight"])
            exact(o + "op_b", sd[lp + "cross_attn.output_proj.bias"])
            exact(o + "op_w3", sd[lp + "cross_attn.output_proj.weight"], "split3w") if s3 else absent(o + "op_w3")
            vw, vb = sd[lp + "cross_attn.value_proj.weight"], sd[lp + "cross_attn.value_proj.bias"]
            alias = next((k for k in range(j) if sd[f"{dp}decoder.layers.{k}.cross_attn.value_proj.weight"] is vw
                          and sd[f"{dp}decoder.layers.{k}.cross_attn.value_proj.bias"] is vb), -1)
            if alias < 0:
                exact(o + "vp_w", vw, wfmt)
                exact(o + "vp_b", vb)
                exact(o + "vp_w2", vw, "pair") if x3 else absent(o + "vp_w2")
            else:
                absent(o + "vp_w"), absent(o + "vp_b"), absent(o + "vp_w2")
            for n in dense_only:
                absent(o + n)
        else:
            alias = -1
            iw, ib = sd[lp + "multihead_attn.in_proj_weight"], sd[lp + "multihead_attn.in_proj_bias"]
            exact(o + "ca_q_w", iw[:Dd])
            exact(o + "ca_q_b", ib[:Dd])
            exact(o + "ca_kv_w", iw[Dd:], wfmt)
            exact(o + "ca_kv_w2", iw[Dd:], "pair") if x3 else absent(o + "ca_kv_w2")
            exact(o + "ca_kv_b", ib[Dd:])
            exact(o + "ca_out_w", sd[lp + "multihead_attn.out_proj.weight"])
            exact(o + "ca_out_b", sd[lp + "multihead_attn.out_proj.bias"])
            for short, t in (("ca_q_w3", iw[:Dd]), ("ca_out_w3", sd[lp + "multihead_attn.out_proj.weight"])):
                exact(o + short, t, "split3w") if s3 else absent(o + short)
            for n in deform_only:
                absent(o + n)
        for k in [k for k in S if k.startswith(o)]:
            S[k].vp_alias = alias
    return S


# ------------------------------------------------------------------------------------------------ CPU packers (device layouts as byte tensors)
def bf(x):
    return x.float().bfloat16().float()


def _u8(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)


def _padded(x, pad):
    return torch.cat([x, torch.zeros(x.shape[0], pad, dtype=x.dtype)], 1) if pad else x


def h2w_pack_cpu(x):
    """H2 weight rows (include/dinodet.h dod_op_split_h2 with wexp) -> (bytes [rows, 3 cols] = fp16 x cols | e4m3((x - h) 2^(e + 11)) x cols,
    wexp [rows] = 127 - e), e = floor(log2(448 / max_row |h|)) (0 for a zero row); tests/test_gpu_h2.py pins the kernel to exactly this"""
    xc = x.float().clamp(-65504, 65504)
    hh = xc.half()
    amax = hh.float().abs().amax(1)
    e = torch.where(amax > 0, torch.floor(torch.log2(448.0 / amax.double())), torch.zeros_like(amax, dtype=torch.float64))
    sc = torch.exp2(e)[:, None]
    r8 = ((xc - hh.float()).double() * sc * 2048).float().to(torch.float8_e4m3fn)
    return torch.cat([_u8(hh), _u8(r8)], 1), (127 - e).to(torch.uint8)


def pack_cpu(fmt, x, pad=0, defect=None):
    """fp32 [rows, cols] -> {array name: byte tensor} of the format, as the device lays it out"""
    from tests.test_gpu_fp8 import mx_ref, quant_ref
    x = x.float()
    if fmt == "f32":
        return {"w": _u8(_padded(x, pad))}
    if fmt == "bf16":
        return {"w": _u8(_padded(x, pad).bfloat16())}
    if fmt in ("pair", "split3w"):
        hi, lo = split_pair(_padded(x, pad))
        if defect == "lo_zero":
            lo = torch.zeros_like(lo)
        planes = [hi, lo] if fmt == "pair" else ([hi, hi, lo] if defect == "s3_act_order" else [hi, lo, hi])
        return {"w": _u8(torch.cat(planes, 1).bfloat16())}
    if fmt == "h2w":
        b, wexp = h2w_pack_cpu(x)
        return {"w": b, "wexp": wexp}
    if fmt == "e4m3_rows":
        q, sc = quant_ref(x)
        return {"w": _u8(q), "wscale": sc.contiguous().view(torch.uint8)}
    if fmt == "e4m3_mx":
        q, lay, _ = mx_ref(x)
        return {"w": _u8(q), "wbs": lay.reshape(-1)}
    raise ValueError(fmt)


def decode(fmt, arrays, rows, cols, pitch):
    """byte arrays -> dict(value float64 [rows, cols] = what the MFMAs multiply, planes..., pads: the values behind `cols`)"""
    w = arrays["w"].reshape(rows, pitch)
    if fmt == "f32":
        v = w.contiguous().view(torch.float32).double()
        return dict(value=v[:, :cols], pads=v[:, cols:])
    if fmt == "bf16":
        v = w.contiguous().view(torch.bfloat16).double()
        return dict(value=v[:, :cols], pads=v[:, cols:])
    if fmt in ("pair", "split3w"):
        n = 2 if fmt == "pair" else 3
        v = w.contiguous().view(torch.bfloat16).double().reshape(rows, n, -1)
        d = dict(hi=v[:, 0, :cols], lo=v[:, 1, :cols], value=v[:, 0, :cols] + v[:, 1, :cols], pads=v[:, :, cols:].reshape(rows, -1))
        if n == 3:
            d["hi2"] = v[:, 2, :cols]
        return d
    if fmt == "h2w":
        from tests.test_gpu_h2 import decode as decode_h2
        h, m8, r8 = decode_h2(w, cols, arrays["wexp"])
        return dict(h=h, r8=r8, main=m8, value=h + r8, pads=torch.zeros(rows, 0), sc=torch.exp2(127 - arrays["wexp"].double())[:, None])
    if fmt == "e4m3_rows":
        sc = arrays["wscale"].contiguous().view(torch.float32)
        return dict(value=dequant_rows(E4M3_LUT[w.long()], sc), q=w, sc=sc.double(), pads=torch.zeros(rows, 0))
    if fmt == "e4m3_mx":
        lay = arrays["wbs"].reshape(rows, cols // 32)
        return dict(value=dequant_mx(E4M3_LUT[w.long()], lay), q=w, eb=mx_block_order(lay, cols).long(), pads=torch.zeros(rows, 0))
    raise ValueError(fmt)


def restate(sd, cs, mode, fold_opt=True, defect=None):
    """the whole pack in torch fp32 on the CPU pushed through the CPU packers -> {name: (info dict, arrays)} in the accessor's terms"""
    S = reference(sd, cs, mode, fold_opt)
    fold, glu = fold_expected(cs, mode, fold_opt), glu_expected(cs, mode)
    out = {}
    for name, sp in S.items():
        if sp.format == "absent":
            out[name] = (dict(format="absent", rows=0, cols=0, pitch=0, arrays={}, glu=False, fold=False, vp_alias=sp.vp_alias), {})
            continue
        if name.startswith("block.") and name.rsplit(".", 1)[1] in ("qkv", "o", "fc1", "fc2"):
            i, n = int(name.split(".")[1]), name.rsplit(".", 1)[1]
            L = block_linears(sd, cs, i, fold, glu, torch.float32, defect)[n]
            arrays = pack_cpu(sp.format, L["w"], 0, defect)
            arrays["bias"] = L["b"].contiguous().view(torch.uint8)
            if L["c"] is not None:
                c = bf(L["w"]).sum(1) if mode == "bf16" and defect != "c_without_gamma" else L["c"]
                arrays["csum"] = c.float().contiguous().view(torch.uint8)
        else:
            arrays = pack_cpu(sp.format, sp.src, sp.pad_cols, defect)
            if defect == "pad_1e-6" and sp.pad_cols and sp.format in ("f32", "bf16"):
                v = _padded(sp.src, sp.pad_cols)
                v[:, -1] = 1e-6
                arrays = pack_cpu(sp.format, v)
        per = {"f32": 4, "bf16": 2, "pair": 4, "split3w": 6, "h2w": 3}.get(sp.format, 1)
        info = dict(format=sp.format, rows=sp.rows, cols=sp.cols, pitch=per * (sp.cols + sp.pad_cols), arrays={k: v.numel() for k, v in arrays.items()},
                    glu=sp.glu, fold=sp.fold, vp_alias=sp.vp_alias)
        out[name] = (info, arrays)
    return out


# ------------------------------------------------------------------------------------------------ the checks
def _same(a, b):
    return 0.0 if a.shape == b.shape and torch.equal(a, b) else INF


def check_operand(sp, info, arrays, mode):
    """every bound of one packed operand -> {check name: worst |got - want| / bound, or 0 / inf for an exactness condition}; the operand
    passes when no ratio exceeds 1.  "csum gap" is a measurement, reported beside the ratios under the key "_gap"."""
    res = {}
    want_info = dict(format=sp.format, rows=sp.rows, cols=sp.cols, glu=sp.glu, fold=sp.fold, vp_alias=sp.vp_alias)
    res["info"] = 0.0 if all(info[k] == v for k, v in want_info.items()) else INF
    if sp.format == "absent":
        res["no arrays"] = 0.0 if not info["arrays"] else INF
        return res
    rows, cols, fmt = sp.rows, sp.cols, sp.format
    per = {"f32": 4, "bf16": 2, "pair": 4, "split3w": 6, "h2w": 3}.get(fmt, 1)
    res["pitch"] = 0.0 if info["pitch"] == per * (cols + sp.pad_cols) else INF
    expect_arrays = {"w"} | ({"bias"} if sp.bias else set()) | ({"csum"} if sp.csum else set()) | {"h2w": {"wexp"}, "e4m3_rows": {"wscale"}, "e4m3_mx": {"wbs"}}.get(fmt, set())
    res["arrays"] = 0.0 if set(info["arrays"]) == expect_arrays and info["arrays"]["w"] == rows * info["pitch"] else INF
    if res["pitch"] or res["arrays"]:
        return res
    d = decode(fmt, arrays, rows, cols, info["pitch"])
    want = sp.want
    res["pads == 0"] = 0.0 if bool((d["pads"] == 0).all()) else INF
    if sp.xb is None:                                              # no arithmetic before the format: the CPU packer's bytes
        ref = pack_cpu(fmt, sp.src, sp.pad_cols)
        for k, v in ref.items():
            res[f"{k} bytes == cpu packer"] = _same(arrays[k].reshape(-1), v.reshape(-1))
    xb = sp.xb if sp.xb is not None else torch.zeros_like(want)
    if fmt == "f32":
        res["f32"] = ratio(d["value"], want, xb)
    elif fmt == "bf16":
        res["bf16"] = ratio(d["value"], want, xb + half_ulp_bf16(want.abs() + xb))
    elif fmt in ("pair", "split3w"):
        res["hi + lo"] = ratio(d["value"], want, xb + PAIR_REL * want.abs())
        res["hi"] = ratio(d["hi"], want, xb + half_ulp_bf16(want.abs() + xb))
        if fmt == "split3w":
            res["planes 0 == 2"] = _same(d["hi"], d["hi2"])
    elif fmt == "h2w":
        h, r8, sc = d["h"], d["r8"], d["sc"]
        amax = h.abs().amax(1)
        e = torch.where(amax > 0, torch.floor(torch.log2(448.0 / amax)), torch.zeros_like(amax))
        res["wexp == rule(h)"] = _same(127 - arrays["wexp"].double(), e)
        (got, bound), _ = h2_row_bounds(want * sc, xb * sc, h * sc, r8 * sc)        # the remainder is quantised at the row's 2^e
        res["h2 h + r"] = ratio(got / sc, want, bound / sc)
        _, (got, bound) = h2_row_bounds(want, xb, h, r8)
        res["h2 h"] = ratio(got, want, bound)
    elif fmt == "e4m3_rows":
        sc = d["sc"]
        amax = want.abs().amax(1)
        zero = amax == 0
        sc_want = torch.where(zero, torch.ones_like(amax), amax / 448.0)
        res["fp8 scale"] = ratio(sc, sc_want, xb.amax(1) / 448.0 + 2.0 ** -24 * sc_want)
        scs = sc[:, None]
        # q = rne_e4m3(x * fp32(1 / scale)): the scale, its reciprocal and the product round once each before the e4m3 rounding
        res["fp8 values"] = ratio(d["value"], want, xb + e4m3_half_ulp((want.abs() + xb) / scs) * scs + 3 * 2.0 ** -24 * want.abs())
        res["fp8 zero rows"] = 0.0 if bool((d["q"][zero] == 0).all()) and bool((sc[zero] == 1.0).all()) else INF
    elif fmt == "e4m3_mx":
        lo, hi = mx_byte_range(want, xb / (BF16_REL + ACC_REL))
        eb = d["eb"]
        res["mx scale bytes"] = 0.0 if bool(((eb >= lo) & (eb <= hi)).all()) else INF
        scs = torch.exp2((eb.clamp(1, 253) - 127).double())[..., None].expand(rows, cols // 32, 32).reshape(rows, cols)
        res["mx values"] = ratio(d["value"], want, xb + e4m3_half_ulp((want.abs() + xb) / scs) * scs)
    if sp.bias:
        bw, bb_, bsrc = sp.bias
        got = arrays["bias"].contiguous().view(torch.float32)
        if bb_ is None:
            res["bias == source"] = _same(got, bsrc.float())
        else:
            res["bias"] = ratio(got, bw, bb_)
    if sp.csum:
        T_c, rel = sp.csum
        got = arrays["csum"].contiguous().view(torch.float32).double()
        if mode == "bf16":          # the kernel sums bf16-rounded W': elements whose rounding the fp32 bound does not decide may fall either way
            und = (bf((want + xb).float()).double() - bf((want - xb).float()).double()).abs().sum(1)
            res["csum (definition)"] = ratio(got, bf(want.float()).double().sum(1), rel * T_c + und)
        else:
            res["csum (definition)"] = ratio(got, want.sum(1), rel * T_c + xb.sum(1))
        dec = d["value"]
        widen = (want - dec).abs().sum(1)
        res["csum (decoded)"] = ratio(got, dec.sum(1), rel * T_c + xb.sum(1) + widen)
        res["_gap"] = float(((got - dec.sum(1)).abs() / dec.abs().sum(1).clamp(min=1e-300)).max())
        res["_gap_allowed"] = float((widen / dec.abs().sum(1).clamp(min=1e-300)).max())
    return res


def worst(res):
    return max((v for k, v in res.items() if not k.startswith("_")), default=0.0)
