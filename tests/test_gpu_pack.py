"""`-m gpu`: what dod_finalize_weights stores, operand by operand, against the float64 definitions and per-element bounds of
tests/pack_cases.py (shown sound on the CPU by tests/test_pack_cases_cpu.py).  The tests finalize only -- no forward beside the one the
packer itself runs for the decoder's layer-0 constants -- and read every packed array through dod_test_packed_info / dod_test_packed_copy.

Every case has one plain and one LoRA-merged block; the configurations are the smallest that reach each branch of the packer
(pack_cases.CASES), in every precision mode, with the LayerNorm fold on and off, on synth's weights and on checkpoint-like ones."""
import collections
import ctypes as C

import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd.engine import make_config
from tests import pack_cases as pc
from tests.test_gpu_h2 import pack as pack_h2

pytestmark = pytest.mark.gpu

LINEARS = ("qkv", "o", "fc1", "fc2")


class Handle:
    """a dod_handle with `sd` registered (one device tensor per distinct CPU tensor object: tied parameters stay tied) and finalized"""

    def __init__(self, cs, mode, sd, fold_opt=True, dtype=torch.float32):
        self.lib, self.h, self.dev = nat.lib(), C.c_void_p(), {}
        cfg = make_config(cs.bb, cs.dc, mode)
        nat.check(self.lib.dod_create(C.byref(cfg), C.byref(self.h)))
        self.dtype = dtype
        self.finalize(sd, fold_opt)

    def finalize(self, sd, fold_opt=True):
        keep = {}
        for k, t in sd.items():
            if id(t) not in keep:
                keep[id(t)] = t.to(self.dtype).contiguous().cuda()
            d = keep[id(t)]
            shape = (C.c_int64 * max(d.dim(), 1))(*d.shape)
            nat.check(self.lib.dod_set_weight(self.h, k.encode(), nat.ptr(d), shape, d.dim(), nat.DOD_BF16 if self.dtype == torch.bfloat16 else nat.DOD_F32), self.h)
        nat.set_option("ln_fold", 1 if fold_opt else 0)
        try:
            nat.check(self.lib.dod_finalize_weights(self.h, nat.stream_ptr()), self.h)
        finally:
            nat.set_option("ln_fold", -1)
        del keep                                            # the caller's tensors are no longer referenced after finalize

    def read(self, name):
        info = nat.packed_info(self.h, name)
        arrays = {a: nat.packed_array(self.h, name, a, info) for a in info["arrays"]}
        torch.cuda.synchronize()
        return info, {a: t.cpu() for a, t in arrays.items()}

    def read_all(self, names):
        return {n: self.read(n) for n in names}

    def close(self):
        if self.h:
            self.lib.dod_destroy(self.h)
            self.h = C.c_void_p()


def _kind(name):
    parts = name.split(".")
    return parts[-1] if parts[0] in ("block", "dec") else name


def _check_all(hd, S, mode, tag):
    """every operand of S against its Spec; prints the largest ratio per operand kind, the d32 values and the csum gap"""
    worst, d32, gap, bad = collections.defaultdict(float), collections.defaultdict(float), [0.0, 0.0], []
    for name, sp in S.items():
        info, arrays = hd.read(name)
        res = pc.check_operand(sp, info, arrays, mode)
        if sp.format == "h2w" and sp.xb is None and not pc.worst(res):       # exact H2 weight rows: the bytes of the kernel tests/test_gpu_h2.py pins
            b, wexp = pack_h2(sp.src.cuda(), weight=True)
            res["w bytes == dod_op_split_h2"] = 0.0 if torch.equal(b.cpu().reshape(-1), arrays["w"]) and torch.equal(wexp.cpu(), arrays["wexp"]) else pc.INF
        for chk, v in res.items():
            if chk.startswith("_"):
                continue
            worst[f"{_kind(name)}: {chk}"] = max(worst[f"{_kind(name)}: {chk}"], v)
            if not v <= 1.0:
                bad.append((name, chk, v))
        gap = [max(gap[0], res.get("_gap", 0.0)), max(gap[1], res.get("_gap_allowed", 0.0))]
        for k, v in (sp.d32 or {}).items():
            d32[f"{_kind(name)}.{k}"] = max(d32[f"{_kind(name)}.{k}"], v)
    print(f"\n{tag}: largest ratios {({k: f'{v:.3g}' for k, v in sorted(worst.items()) if v > 0})}")
    print(f"  d32 {({k: f'{v:.2e}' for k, v in sorted(d32.items())})}  csum gap {gap[0]:.2e} (format residual allows {gap[1]:.2e})")
    assert not bad, (tag, bad[:8])


RUNS = [(cs.name, mode, fold) for cs in pc.CASES for mode in cs.modes for fold in ([1, 0] if pc.fold_expected(cs, mode, True) else [1])]


@pytest.mark.parametrize("family", pc.FAMILIES)
@pytest.mark.parametrize("name,mode,fold", RUNS, ids=[f"{n}-{m}-fold{f}" for n, m, f in RUNS])
def test_every_packed_operand_is_inside_its_bound(name, mode, fold, family):
    """formats, shapes, pitches, flags and vp_alias as the branch of this configuration has them; every array per element inside its bound;
    bit-equal to the CPU packers where no arithmetic precedes the format; pad columns exactly zero; csum against its definition and against
    the sum of the decoded packed row"""
    cs = pc.case(name)
    sd = pc.state_dict(cs, family)
    S = pc.reference(sd, cs, mode, bool(fold))
    hd = Handle(cs, mode, sd, bool(fold))
    try:
        _check_all(hd, S, mode, f"{name} {family} {mode} fold={fold}")
        if cs.decoder != "dense":
            assert nat.packed_info(hd.h, "dec.1.vp_w")["vp_alias"] == (0 if cs.decoder == "tied" else -1)
            assert ("w" in nat.packed_info(hd.h, "dec.1.vp_w")["arrays"]) == (cs.decoder == "untied")
    finally:
        hd.close()


def test_accessor_rejections_on_a_finalized_handle():
    """an unknown name, a layer past the last, an array the operand does not have, a NULL or short destination: the project's error codes,
    nothing written, and the handle still answers"""
    cs = pc.case("gelu128")
    hd = Handle(cs, "bf16", pc.state_dict(cs, "synth"))
    try:
        L, info = hd.lib, nat.DodPackedInfo()
        err = lambda: L.dod_last_error(hd.h)
        for name in (b"nope", b"block.2.qkv", b"block.0.nope", b"dec.2.in_w", b"dec.0.", b"block.x.qkv", b"block.-1.qkv", b""):
            assert L.dod_test_packed_info(hd.h, name, C.byref(info)) == 1 and b"no packed operand" in err(), name
        assert L.dod_test_packed_info(hd.h, b"cls", None) == 1 and b"null info" in err()
        i = nat.packed_info(hd.h, "block.0.qkv")
        n = i["arrays"]["w"]
        buf = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        assert L.dod_test_packed_copy(hd.h, b"block.0.qkv", 0, None, n, None) == 1 and b"null destination" in err()
        assert L.dod_test_packed_copy(hd.h, b"block.0.qkv", 0, nat.ptr(buf), n - 1, nat.stream_ptr()) == 1 and b"destination" in err()
        assert L.dod_test_packed_copy(hd.h, b"block.0.qkv", 6, nat.ptr(buf), n, nat.stream_ptr()) == 1 and b"dod_packed_array" in err()
        assert L.dod_test_packed_copy(hd.h, b"block.0.qkv", -1, nat.ptr(buf), n, nat.stream_ptr()) == 1
        assert L.dod_test_packed_copy(hd.h, b"block.0.qkv", nat.PK_ARRAY["wexp"], nat.ptr(buf), n, nat.stream_ptr()) == 1 and b"no array" in err()
        assert L.dod_test_packed_copy(hd.h, b"Wpatch2", 0, nat.ptr(buf), n, nat.stream_ptr()) == 1 and b"no array" in err()        # absent in bf16 mode
        torch.cuda.synchronize()
        assert bool((buf == 0x5A).all())
        assert L.dod_test_packed_copy(hd.h, b"block.0.qkv", 0, nat.ptr(buf), n + 64, nat.stream_ptr()) == 0                       # a larger destination is fine
        torch.cuda.synchronize()
        assert bool((buf[n:] == 0x5A).all()) and torch.equal(buf[:n].cpu(), hd.read("block.0.qkv")[1]["w"])
        assert nat.packed_info(hd.h, "Wpatch2")["format"] == "absent" and nat.packed_info(hd.h, "block.0.qkv") == i                # no state changed
    finally:
        hd.close()


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "fp8"])
def test_bf16_state_dict_packs_like_its_widened_copy(mode):
    """tensors registered as DOD_BF16 pack to the same bytes as their fp32 widening; tied tensors are widened once, so the alias survives"""
    cs = pc.case("gelu128")
    sd16 = {}
    src = pc.state_dict(cs, "ckpt")
    seen = {}
    for k, t in src.items():
        if id(t) not in seen:
            seen[id(t)] = t.bfloat16()
        sd16[k] = seen[id(t)]
    wide = {}
    for k, t in sd16.items():
        if id(t) not in wide:
            wide[id(t)] = t.float()
    sd32 = {k: wide[id(t)] for k, t in sd16.items()}
    names = list(pc.reference(sd32, cs, mode))
    a, b = Handle(cs, mode, sd16, dtype=torch.bfloat16), Handle(cs, mode, sd32)
    try:
        ra, rb = a.read_all(names + ["l0_tgt", "l0_proj"]), b.read_all(names + ["l0_tgt", "l0_proj"])
        for n in ra:
            assert ra[n][0] == rb[n][0], n
            for arr in ra[n][1]:
                assert torch.equal(ra[n][1][arr], rb[n][1][arr]), (n, arr)
        assert ra["dec.1.vp_w"][0]["vp_alias"] == 0 and ra["dec.0.vp_w"][0]["vp_alias"] == -1
        _check_all(a, pc.reference(sd32, cs, mode), mode, f"bf16 state dict {mode}")
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "fp16x2"])
def test_second_finalize_repacks_every_view(mode):
    """finalize, change query_embed, one LoRA B and one norm gamma, finalize again: every view -- the decoder's layer-0 constants l0_tgt /
    l0_proj included, which the packer computes by a forward of its own -- equals a fresh handle's for the new weights bit for bit, is inside
    the new weights' bounds, and the views that depend on the changed tensors did change"""
    cs = pc.case("gelu128")
    sd = pc.state_dict(cs, "synth")
    hd = Handle(cs, mode, sd)
    fresh = None
    try:
        names = list(pc.reference(sd, cs, mode)) + ["l0_tgt", "l0_proj"]
        before = hd.read_all(names)
        new = dict(sd)
        lp = "backbone.dino.encoder.layer."
        qk, bk, gk = "decoder.query_embed.weight", lp + "1.attention.attention.key.lora_B.weight", lp + "0.norm2.weight"
        new[qk] = sd[qk] * 1.5 + 0.25
        new[bk] = sd[bk] * -2.0
        new[gk] = sd[gk] * 0.5 + 0.125
        hd.finalize(new)
        after = hd.read_all(names)
        fresh = Handle(cs, mode, new)
        want = fresh.read_all(names)
        for n in names:
            assert after[n][0] == want[n][0], n
            for arr in want[n][1]:
                assert torch.equal(after[n][1][arr], want[n][1][arr]), (n, arr)
        _check_all(hd, pc.reference(new, cs, mode), mode, f"second finalize {mode}")
        changed = {n for n in names if any(not torch.equal(before[n][1][a], after[n][1][a]) for a in after[n][1])}
        assert changed == {"query", "l0_tgt", "l0_proj", "block.1.qkv", "block.0.ln2w", "block.0.fc1"}, sorted(changed)
        D = cs.bb.hidden
        per = after["block.1.qkv"][0]["pitch"]
        rows = lambda r, lo, hi_: r[1]["w"].reshape(3 * D, per)[lo:hi_]
        assert torch.equal(rows(before["block.1.qkv"], 0, D), rows(after["block.1.qkv"], 0, D))            # q rows: their LoRA did not change
        assert not torch.equal(rows(before["block.1.qkv"], D, 2 * D), rows(after["block.1.qkv"], D, 2 * D))
        assert torch.equal(rows(before["block.1.qkv"], 2 * D, 3 * D), rows(after["block.1.qkv"], 2 * D, 3 * D))
    finally:
        hd.close()
        if fresh:
            fresh.close()
