"""Cases, float64 reference, CPU emulations and bounds of the attention operator tests (tests/test_gpu_attention.py on the GPU,
tests/test_attention_cases_cpu.py for what can be shown without one).  Everything here is plain torch on the CPU.

One rule for every kernel: the reference is float64 softmax attention of the values the kernel is actually given, and every error is
normalised PER ELEMENT by the size of what is summed there,
    T[q, d] = sum_k p[q, k] |v[k, d]|,
never by the tensor's maximum."""
import math
import zlib

import numpy as np
import torch

from oracle import dinodet_oracle as orc

SCALE = 0.125
GUARD = 256                      # guard rows before and after every output and every input
PERIOD = 7                       # the large launches repeat 7 distinct images (coprime with the XCD map's 8 and with the head counts)
LOG2E = 1.44269504088896340736

# key tiles of 64; query blocks of 128 (attn_x3, the 32-rows-per-wave body of attn_bf16): only a tail tile, only full tiles, one full tile
# plus a one-key tail, waves without rows, and four tiles (the three-slot ring of attn_bf16 wraps)
N_SWEEP = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 256, 257, 300]
# the XCD pair map: B * heads = 1 (seven of eight workgroups return at once), 3, 8, 9 (a second group of eight), heads odd and B odd
PAIR_MAP = [(1, 65, 1), (1, 129, 3), (3, 65, 1), (8, 33, 1), (3, 129, 3), (9, 64, 1)]
SMALL = [(2, n, 1) for n in N_SWEEP] + PAIR_MAP
# npairs * ceil(N / 256) >= 1024 selects the 64-rows-per-wave body of attn_bf16: the fused short tail (300 = 256 + 44), one launch with a
# long remainder (400 = 256 + 144) and no remainder (512)
BIG = [(256, 300, 2), (256, 400, 2), (256, 512, 2)]
SOFTMAX_KINDS = ["rising", "tile0", "equal", "pm60"]

BF16_REL = 2.0 ** -8             # one rounding to bf16 (P, and the stored context)
ACC_REL = 1e-5                   # fp32 accumulation and exp2 of the bf16 kernel, relative to T
X3_FLOOR = 2.0 ** -16
F32_FLOOR = 1e-6
MX_UNDECIDED_CAP = 0.15


def n_unique(B):
    return B if B <= 16 else PERIOD


def image_index(B):
    """image b of a launch carries distinct image b % n_unique(B)"""
    return np.arange(B) % n_unique(B)


def make_input(B, N, heads, kind="normal", variant=0):
    """fp32 [n_unique(B), N, 3 * heads * 64] (q | k | v column blocks).  kind: "normal", "vzero", or one of SOFTMAX_KINDS (N = 300: tiles 0..4)"""
    D = heads * 64
    nu = n_unique(B)
    rng = np.random.default_rng(zlib.crc32(repr((B, N, heads, kind, variant)).encode()))
    x = (rng.standard_normal((nu, N, 3 * D)) * 1.5).astype(np.float32)
    u = np.ones(64, dtype=np.float32) / 8.0          # a unit vector: q gets a component 8 u, so a key a * u scores 0.125 * a * (8 + noise)
    if kind == "rising":            # row maxima rise tile by tile: one key spikes in each of tiles 1, 2, 3, each above the last
        x[:, :, :D] += np.tile(8.0 * u, heads)
        for key, a in ((70, 24.0), (140, 40.0), (200, 56.0)):
            x[:, key, D:2 * D] = np.tile(a * u, heads)
    elif kind == "tile0":           # every row's maximum is key 5: all q share a component along u, key 5 is a multiple of u
        x[:, :, :D] += np.tile(8.0 * u, heads)
        x[:, 5, D:2 * D] = np.tile(80.0 * u, heads)
    elif kind == "equal":           # every third row's scores are one number, another for each row: q = a e_0 per head, and k[:, 0] = 2 for every key
        a = 4.0 * x[:, ::3, 0:D:64].copy()
        x[:, ::3, :D] = 0.0
        x[:, ::3, 0:D:64] = a
        x[:, :, D:2 * D:64] = 2.0
    elif kind == "pm60":            # scores of order +-60 after scaling, both signs in every row: dims 0..7 of a head hold a_q in q and +-2 (by key
        a = rng.uniform(24.0, 36.0, (nu, N, heads)) * rng.choice([-1.0, 1.0], (nu, N, heads))       # parity) in k: 0.125 * 8 * (+-2) * a_q = +-2 a_q
        sign = np.where(np.arange(N) % 2 == 0, 2.0, -2.0).astype(np.float32)
        for h in range(heads):      # +-2 is exact in bf16 (its lo half is 0), so the split products attn_x3 drops are not inflated by the offset
            x[:, :, h * 64:h * 64 + 8] = a[:, :, h, None].astype(np.float32)
            x[:, :, D + h * 64:D + h * 64 + 8] = sign[None, :, None]
    elif kind == "vzero":           # v = 0 for the last head: its context is exactly zero
        x[:, :, 3 * D - 64:] = 0.0
    elif kind != "normal":
        raise ValueError(kind)
    return torch.from_numpy(x)


def heads_view(t, heads):
    nu, N, D = t.shape
    return t.reshape(nu, N, heads, D // heads).transpose(1, 2)


def unheads(t):
    nu, h, N, dh = t.shape
    return t.transpose(1, 2).reshape(nu, N, h * dh)


def ref64(q, k, v, heads, scale=SCALE):
    """float64 softmax attention of [n, Lq, E] / [n, Lk, E] values -> (want, T), both [n, Lq, E] float64"""
    qh, kh, vh = heads_view(q.double(), heads), heads_view(k.double(), heads), heads_view(v.double(), heads)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    return unheads(p @ vh), unheads(p @ vh.abs())


def ref64_qkv(vals, heads, scale=SCALE):
    D = vals.shape[-1] // 3
    return ref64(vals[..., :D], vals[..., D:2 * D], vals[..., 2 * D:], heads, scale)


def f32_cpu(q, k, v, heads, scale):
    """the same statement in torch's fp32 on the CPU: its distance from float64 sets the fp32 kernels' bound"""
    qh, kh, vh = heads_view(q.float(), heads), heads_view(k.float(), heads), heads_view(v.float(), heads)
    return unheads(torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).double()


def bf(x):
    return x.float().bfloat16().float()


def split_pair(x):
    """x = hi + lo as dod_op_split_pair writes it (tests/test_gpu_x3.py test_split_pair_layout pins the kernel to exactly this)"""
    hi = bf(x)
    return hi, bf(x.float() - hi)


def emu_bf16(vals_bf16, heads, scale=SCALE):
    """attn_bf16 with its two rounding points and nothing else: P rounded to bf16 before P V (the normaliser sums the unrounded P), the
    context rounded to bf16; float64 everywhere else"""
    D = vals_bf16.shape[-1] // 3
    q, k, v = [heads_view(t.double(), heads) for t in (vals_bf16[..., :D], vals_bf16[..., D:2 * D], vals_bf16[..., 2 * D:])]
    s = q @ k.transpose(-1, -2) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (bf(p).double() @ v) / p.sum(-1, keepdim=True)
    return bf(unheads(o)).double()


def emu_x3(hi, lo, heads, scale=SCALE):
    """attn_x3 split at the kernel's split points, float64 accumulation: S = Kh Qh + Kh Ql + Kl Qh (lo.lo dropped), P in fp32 split
    into two bf16 halves, O = Vh Ph + Vh Pl + Vl Ph, the normaliser from the fp32 P, the context as hi + lo of its fp32 value"""
    D = hi.shape[-1] // 3
    qh, kh, vh = [heads_view(t.double(), heads) for t in (hi[..., :D], hi[..., D:2 * D], hi[..., 2 * D:])]
    ql, kl, vl = [heads_view(t.double(), heads) for t in (lo[..., :D], lo[..., D:2 * D], lo[..., 2 * D:])]
    s = qh @ kh.transpose(-1, -2) + ql @ kh.transpose(-1, -2) + qh @ kl.transpose(-1, -2)
    p = torch.exp2((s - s.amax(-1, keepdim=True)) * (scale * LOG2E)).float()
    ph, pl = split_pair(p)
    o = (ph.double() @ vh + pl.double() @ vh + ph.double() @ vl) / p.double().sum(-1, keepdim=True)
    oh, ol = split_pair(unheads(o).float())
    return oh.double() + ol.double()


def dist_by_T(got, want, T):
    """max over elements of |got - want| / T (elements with T = 0 must be exact)"""
    err = (got - want).abs()
    assert bool((err[T == 0] == 0).all())
    return float((err / T.clamp(min=1e-300))[T > 0].max()) if bool((T > 0).any()) else 0.0


def bf16_bound(want, T):
    """|got - want| <= 2^-8 |want| + 2^-8 T + 1e-5 T: the context's rounding to bf16, P's rounding to bf16 (at most 2^-8 relative per
    term of the sum T bounds), fp32 accumulation.  The normaliser l sums the fp32 P (attn_tile: lsum is formed before pack2bf), so it
    adds nothing of order 2^-8."""
    return BF16_REL * want.abs() + (BF16_REL + ACC_REL) * T


def mx_value_margin(T):
    """what the MX epilogue's fp32 context may differ from float64 by before it is quantised"""
    return (BF16_REL + ACC_REL) * T


def e4m3_half_ulp(y):
    """half an e4m3 ulp at magnitude y (normal from 2^-6 with 3 mantissa bits, subnormal spacing 2^-9 below; the top binade ends at 448)"""
    e = torch.floor(torch.log2(y.clamp(min=2.0 ** -6, max=448.0)))
    return 0.5 * torch.exp2(e - 3)


def _f32_outward(a, up):
    f = a.float()
    inf = torch.tensor(float("inf") if up else float("-inf"))
    wrong = (f.double() < a) if up else (f.double() > a)
    return torch.where(wrong, torch.nextafter(f, inf), f)


def mx_byte_range(want, T):
    """e8m0 bytes the rule (oracle._mx_scales, mirrored from mx_ebyte) gives for the smallest and the largest block maximum the value
    margin allows: [rows, D / 32] each, in block order.  Where they agree the kernel's byte is decided."""
    rows, D = want.shape
    m = mx_value_margin(T)
    a_lo = (want.abs() - m).clamp(min=0).reshape(rows, D // 32, 32).amax(-1)
    a_hi = (want.abs() + m).reshape(rows, D // 32, 32).amax(-1)

    def rule(a):
        t = torch.zeros(rows, D // 32, 32)
        t[..., 0] = a
        return orc._mx_scales(t.reshape(rows, D))
    return rule(_f32_outward(a_lo, False)), rule(_f32_outward(a_hi, True))


def mx_block_order(bs, D):
    """scale bytes [rows][2][D / 64] as the kernels lay them out -> block order [rows, D / 32]"""
    rows = bs.shape[0]
    return bs.reshape(rows, 2, D // 64).permute(0, 2, 1).reshape(rows, D // 32)


E4M3_LUT = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()      # NaN at 0x7f / 0xff


def mx_cases():
    """(B, N, heads, kind) of every block-scaled launch the GPU test makes"""
    return [(B, N, h, "normal") for B, N, h in SMALL + BIG] + [(2, 300, 1, k) for k in SOFTMAX_KINDS] + [(256, 300, 2, "rising"), (2, 65, 2, "vzero"), (2, 150, 4, "normal")]
