"""The yardstick of tests/test_gpu_pack.py shown sound without a GPU (tests/pack_cases.py): a torch-fp32 restatement of the whole pack, pushed
through the CPU packers, stays inside every bound for both weight families in every mode -- the largest ratio per operand kind and mode is
printed -- and each of seven deliberately wrong packs lands outside a bound on at least one element of the smallest case that has the
branch."""
import collections

import pytest
import torch

from tests import pack_cases as pc

RUNS = [(cs.name, mode) for cs in pc.CASES + [pc.SMALL_GLU] for mode in cs.modes]


def _kind(name):
    parts = name.split(".")
    return parts[-1] if parts[0] in ("block", "dec") else name


def _run(cs, family, mode, fold_opt=True, defect=None):
    sd = pc.state_dict(cs, family)
    S = pc.reference(sd, cs, mode, fold_opt)
    got = pc.restate(sd, cs, mode, fold_opt, defect)
    return S, {name: pc.check_operand(sp, *got[name], mode) for name, sp in S.items()}


@pytest.mark.parametrize("family", pc.FAMILIES)
@pytest.mark.parametrize("name,mode", RUNS, ids=[f"{n}-{m}" for n, m in RUNS])
def test_fp32_restatement_is_inside_every_bound(name, mode, family):
    cs = pc.case(name)
    for fold_opt in ([True, False] if pc.fold_expected(cs, mode, True) else [True]):
        S, res = _run(cs, family, mode, fold_opt)
        worst = collections.defaultdict(float)
        d32 = collections.defaultdict(float)
        gap = [0.0, 0.0]
        for op, r in res.items():
            for chk, v in r.items():
                if chk.startswith("_"):
                    continue
                worst[f"{_kind(op)}: {chk}"] = max(worst[f"{_kind(op)}: {chk}"], v)
                assert v <= 1.0, (name, family, mode, fold_opt, op, chk, v)
            gap = [max(gap[0], r.get("_gap", 0.0)), max(gap[1], r.get("_gap_allowed", 0.0))]
            for k, v in (S[op].d32 or {}).items():
                d32[f"{_kind(op)}.{k}"] = max(d32[f"{_kind(op)}.{k}"], v)
        shown = {k: f"{v:.3g}" for k, v in sorted(worst.items()) if v > 0}
        print(f"\n{name} {family} {mode} fold={int(fold_opt)}: largest ratios {shown}")
        print(f"  d32 {({k: f'{v:.2e}' for k, v in sorted(d32.items())})}  csum gap {gap[0]:.2e} (format residual allows {gap[1]:.2e})")


# (defect, mode, the operand it must break): the smallest case with a merged block, a fold, the interleave, a padded patch weight and split3 copies
DEFECTS = [("alpha_half", "bf16x3", "block.1.qkv"), ("qk_swap", "bf16x3", "block.0.qkv"), ("beta_after_interleave", "bf16x3", "block.0.fc1"),
           ("c_without_gamma", "bf16x3", "block.0.qkv"), ("lo_zero", "bf16x3", "block.0.o"), ("pad_1e-6", "bf16", "Wpatch"),
           ("s3_act_order", "bf16x3", "dec.0.in_w3")]


@pytest.mark.parametrize("defect,mode,operand", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_wrong_packs_land_outside_a_bound(defect, mode, operand):
    _, res = _run(pc.SMALL_GLU, "synth", mode, True, defect)
    bad = {op: {c: v for c, v in r.items() if not c.startswith("_") and v > 1.0} for op, r in res.items()}
    bad = {op: r for op, r in bad.items() if r}
    print(f"\n{defect}: {({op: {c: f'{v:.3g}' for c, v in r.items()} for op, r in list(bad.items())[:4]})}")
    assert operand in bad, (defect, sorted(bad))


def test_families_differ_where_they_should():
    """the checkpoint-like edit has what it says: LayerScale down to 1e-5, a zero gamma, a zero row, a zero lora_B"""
    sd = pc.state_dict(pc.case("gelu128"), "ckpt")
    lp = "backbone.dino.encoder.layer.1."
    ls = sd[lp + "layer_scale1.lambda1"]
    assert float(ls.min()) < 1e-3 and float(ls.max()) <= 1.0 and float(ls.min()) >= 1e-5 * 0.999
    g = sd[lp + "norm1.weight"]
    assert int((g == 0).sum()) == 1 and float(g.abs().max()) > 5.0
    w = sd[lp + "attention.attention.key.linear.weight"]
    assert int((w.abs().sum(1) == 0).sum()) == 1 and float(w.abs().amax(1).max() / w.abs().amax(1).median()) > 20
    assert not sd[lp + "attention.attention.query.lora_B.weight"].any() and sd[lp + "attention.attention.key.lora_B.weight"].any()
    tied = pc.state_dict(pc.case("gelu128"), "synth")
    k = "decoder.decoder.layers.%d.cross_attn.value_proj.weight"
    assert tied[k % 0] is tied[k % 1]
    untied = pc.state_dict(pc.case("swiglu384-p16-proj-untied"), "synth")
    assert untied[k % 0] is not untied[k % 1] and not torch.equal(untied[k % 0], untied[k % 1])


def test_h2_weight_bytes_decode_to_the_pinned_parts():
    """the byte packer of H2 weight rows used by the restatement decodes (tests/test_gpu_h2.decode) to gemm_cases.h2_parts_cpu's values"""
    from tests.gemm_cases import h2_parts_cpu
    from tests.test_gpu_h2 import decode
    x = pc.state_dict(pc.case("gelu128"), "ckpt")["backbone.dino.encoder.layer.0.mlp.fc1.weight"]
    b, wexp = pc.h2w_pack_cpu(x)
    for got, want in zip(decode(b, x.shape[1], wexp), h2_parts_cpu(x, weight=True)):
        assert torch.equal(got, want)
    assert int((wexp == 127).sum()) >= 1                     # the all-zero row: e = 0


def test_fused_patch_order_is_the_kernels_map():
    """column s 32 + r 16 + j of the packed row holds W[n][c][2 si + r][j] with s = c (p / 2) + si, zero for j >= p (csrc/patch_embed.hip)"""
    for p in (14, 16):
        W = torch.arange(2 * 3 * p * p, dtype=torch.float32).reshape(2, 3, p, p) + 1
        out = pc.patch_fused_order(W)
        assert out.shape == (2, 3 * (p // 2) * 32)
        for n, c, si, r, j in [(0, 0, 0, 0, 0), (1, 2, p // 2 - 1, 1, p - 1), (0, 1, 3, 1, 5), (1, 0, 2, 0, 13)]:
            assert out[n, (c * (p // 2) + si) * 32 + r * 16 + j] == W[n, c, 2 * si + r, j]
        assert int((out == 0).sum()) == 2 * 3 * (p // 2) * 2 * (16 - p)
