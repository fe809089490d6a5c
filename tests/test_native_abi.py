"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/dinodet.h declares, argument validation returns the documented status codes, and the
Python mirrors expose the reference's state-dict keys.  No GPU compute."""
import ctypes as C
import os
import re

import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import synth
from dinov2_od_amd.engine import make_config
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def test_header_symbols_all_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    declared = set(re.findall(r"\b(dod_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(nat.SYMBOLS), (declared ^ set(nat.SYMBOLS))
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.dod_version()


def test_release_library_has_no_tuning_code(lib):
    """The release library carries no tuning hooks: none of the dod_debug_* entry points of include/dinodet_tuning.h (in-kernel time
    stamps, MFMA probes) is exported, and the only DINODET_* environment variables it reads are the operational ones INTEGRATION.md
    lists (<= 8) -- no variable can make a shipped kernel skip work or pick another tile."""
    tun = open(os.path.join(ROOT, "include", "dinodet_tuning.h")).read()
    names = set(re.findall(r"\b(dod_debug_[a-z0-9_]+)\s*\(", tun))
    assert len(names) >= 5
    raw = open(nat.LIB_PATH, "rb").read()
    for n in names:
        assert not hasattr(lib, n), n
    assert b"dod_debug_" not in raw
    env = set(re.findall(rb"DINODET_[A-Z0-9_]+", raw))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(env) <= 8, env
    for v in env:
        assert v.decode() in doc, f"{v.decode()} is read by the library but not documented in INTEGRATION.md"
    for gone in (b"DINODET_GEMM_ABL", b"DINODET_DEBUG_NOOUT", b"DINODET_DEBUG_LDA0", b"DINODET_GEMM_TILE", b"DINODET_EPI_RB"):
        assert gone not in raw


def test_test_options_validate_names(lib):
    assert lib.dod_test_set_option(b"tailsplit", -1) == 0
    assert lib.dod_test_set_option(b"no_such_option", 1) == 1 and b"unknown" in lib.dod_last_error(None)
    assert lib.dod_test_counter(b"tail_splits") >= 0 and lib.dod_test_counter(b"nope") == -1


def test_config_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    body = re.search(r"typedef struct dod_config \{(.*?)\} dod_config;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in nat.DodConfig._fields_]
    for (ct, _), (_, pt) in zip(fields, nat.DodConfig._fields_):
        assert (ct == "float") == (pt is C.c_float)
    assert C.sizeof(nat.DodConfig) == 4 * len(fields)


def test_dec_train_params_struct_matches_header():
    """struct dod_dec_train_params (native decoder training step): the ctypes mirror lists the header's pointers in order"""
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    body = re.search(r"typedef struct dod_dec_train_params \{(.*?)\} dod_dec_train_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*\s*(\w+)", body)
    assert names == nat.DEC_TRAIN_FIELDS and len(names) == 31
    assert C.sizeof(nat.DodDecTrainParams) == 31 * C.sizeof(C.c_void_p)


def test_decoder_train_entry_points_validate_arguments(lib):
    bb, dc = cases.cfg1(25)
    cfg = make_config(bb, dc, "fp32")
    assert lib.dod_decoder_train_tape_bytes(C.byref(cfg), 2, 257) > 0 and lib.dod_decoder_train_workspace_bytes(C.byref(cfg), 2, 257) > 0
    assert lib.dod_decoder_train_tape_bytes(C.byref(cfg), 0, 257) == 0
    dense = make_config(bb, cases.dec_cfg(False), "fp32")
    assert lib.dod_decoder_train_tape_bytes(C.byref(dense), 2, 257) == 0            # nn.TransformerDecoder branch: not native
    rc = lib.dod_decoder_train_forward(C.byref(cfg), None, None, 2, 257, 0.1, 1, None, None, 0, None, 0, None)
    assert rc == 1 and b"null" in lib.dod_decoder_train_last_error()


def _layout_cases():
    """(name, tape_bytes query, workspace_bytes query, arguments, test option to set around the call or None) of the three training steps"""
    from dinov2_od_amd.config import BackboneConfig, DecoderConfig
    bb0 = cases.cfg1(25)[0]
    out = []

    def dec(deform, Dd, Hd, Q, layers, F, Cn, P, B, N):
        dc = DecoderConfig(num_queries=Q, hidden_dim=Dd, nheads=Hd, num_layers=layers, num_classes=Cn, dim_feedforward=F, n_points=P, use_deformable=deform)
        step = "decoder" if deform else "dense_decoder"
        out.append((f"{step}-Dd{Dd}-Q{Q}-P{P}-B{B}-N{N}", f"dod_{step}_train_tape_bytes", f"dod_{step}_train_workspace_bytes", (make_config(bb0, dc, "fp32"), B, N), None))
    dec(True, 128, 4, 7, 2, 256, 11, 2, 2, 26)            # CASES[0] of test_gpu_train_native.py
    dec(True, 192, 2, 5, 2, 256, 11, 4, 2, 1370)          # CASES[2]: 4 points, head_dim 96
    dec(True, 256, 4, 25, 2, 512, 91, 2, 2, 257)          # CASES[3]
    dec(True, 128, 4, 7, 2, 256, 11, 9, 2, 26)            # not taken: 9 sampling points
    dec(False, 128, 4, 7, 2, 256, 11, 2, 2, 17)           # DENSE_CASES[0]
    dec(False, 256, 4, 25, 2, 512, 91, 2, 2, 257)         # DENSE_CASES[3]: N > Q, the cross-attention sizes the score scratch
    dec(False, 256, 4, 25, 2, 512, 91, 2, 2, 9)           # N < Q: the self-attention does
    dec(False, 128, 4, 7, 2, 256, 11, 2, 2, 1409)         # not taken: more than 1 408 memory tokens

    def tail(name, flash, B=2, N=257, nblocks=2, **kw):
        cfg = make_config(BackboneConfig(**kw), DecoderConfig(), "fp32")
        out.append((f"tail-{name}-flash{flash}", "dod_backbone_tail_tape_bytes", "dod_backbone_tail_workspace_bytes", (cfg, B, N, nblocks), flash))
    tail("vits", 1, hidden=384, heads=6, lora_r=2, target_dim=256)      # ViT-S at 224x224, flash attention adjoint: no score scratch
    tail("vits", 0, hidden=384, heads=6, lora_r=2, target_dim=256)      # the batched-GEMM adjoint
    tail("vitg", -1, hidden=1536, heads=24, swiglu=True, lora_r=2)      # SwiGLU, the shipped rule
    tail("vits-r65", -1, hidden=384, heads=6, lora_r=65)                # not taken: LoRA rank past 64
    return out


# (tape bytes, workspace bytes) as built from commit fafa2de -- the last one with all three schedules in one dec_train.hip
_LAYOUT_PARENT = {
    "decoder-Dd128-Q7-P2-B2-N26": (227840, 151296),
    "decoder-Dd192-Q5-P4-B2-N1370": (2308352, 2247168),
    "decoder-Dd256-Q25-P2-B2-N257": (1946880, 1276160),
    "decoder-Dd128-Q7-P9-B2-N26": (0, 0),
    "dense_decoder-Dd128-Q7-P2-B2-N17": (281600, 158720),
    "dense_decoder-Dd256-Q25-P2-B2-N257": (3617024, 2687744),
    "dense_decoder-Dd256-Q25-P2-B2-N9": (1585408, 792832),
    "dense_decoder-Dd128-Q7-P2-B2-N1409": (0, 0),
    "tail-vits-flash1": (41058048, 7937024),
    "tail-vits-flash0": (41058048, 14351872),
    "tail-vitg-flash-1": (334099712, 70003200),
    "tail-vits-r65-flash-1": (0, 0),
}


def test_training_tape_and_workspace_layouts_are_pinned(lib):
    """*_tape_bytes / *_workspace_bytes of the three training steps return what they returned before the schedules were split over
    dec_train.hip / tail_train.hip and their carve functions moved onto one carver: same buffers, same order, same 256-byte slots.  An
    unsupported configuration still reports 0 from both."""
    got = {}
    for name, ftape, fws, (cfg, *dims), flash in _layout_cases():
        if flash is not None:
            assert lib.dod_test_set_option(b"attn_bwd_flash", flash) == 0
        try:
            got[name] = (getattr(lib, ftape)(C.byref(cfg), *dims), getattr(lib, fws)(C.byref(cfg), *dims))
        finally:
            lib.dod_test_set_option(b"attn_bwd_flash", -1)
    assert got == _LAYOUT_PARENT
    assert sum(v == (0, 0) for v in got.values()) == 3 and all(a > 0 and b > 0 for a, b in got.values() if (a, b) != (0, 0))


def test_training_operators_validate_arguments(lib):
    """dod_op_layernorm_bwd ... dod_op_colsum_add: a null pointer or a shape past a documented limit is DOD_ERR_INVALID before any
    launch (no GPU here: a launch would be DOD_ERR_HIP), a short workspace DOD_ERR_STATE; the workspace queries return 0 for the same
    shapes.  `p` stands in for device pointers that are never dereferenced."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lib.dod_decoder_train_last_error
    big = 1 << 30
    # LayerNorm backward: D <= 2048
    assert lib.dod_op_layernorm_bwd(p, p, p, 1e-6, 4, 2052, p, p, p, None) == 1 and b"2048" in err()
    assert lib.dod_op_layernorm_bwd(p, p, p, 1e-6, 0, 64, p, p, p, None) == 1
    for i in (0, 1, 2, 6, 7, 8):
        a = [p, p, p, 1e-6, 4, 64, p, p, p, None]
        a[i] = None
        assert lib.dod_op_layernorm_bwd(*a) == 1 and b"null" in err(), i
    # attention: form 0 takes Lk <= 1408, form 1 head_dim 64 and no dropout; head_dim <= 128
    ws = lib.dod_op_attention_f32_vjp_workspace_bytes
    assert ws(1, 3, 1408, 1, 64, 0) > 0 and ws(1, 3, 1409, 1, 64, 0) == 0
    assert ws(1, 3, 1409, 1, 64, 1) > 0 and ws(1, 3, 7, 1, 32, 1) == 0 and ws(1, 3, 7, 1, 132, 0) == 0 and ws(1, 3, 7, 1, 64, 2) == 0

    def vjp(B=1, Lq=3, Lk=7, heads=1, dh=64, form=0, drop=0.0, ld=None, nbytes=big, null=None):
        ld = heads * dh if ld is None else ld
        a = [p, ld, p, p, ld, p, p, ld, p, ld, p, p, ld, B, Lq, Lk, heads, dh, 0.125, form, drop, 7, p, nbytes, None]
        if null is not None:
            a[null] = None
        return lib.dod_op_attention_f32_vjp(*a)
    assert vjp(Lk=1409, form=0) == 1 and b"1408" in err()
    assert vjp(dh=32, form=1) == 1 and vjp(dh=96, form=1) == 1 and b"head_dim 64" in err()
    assert vjp(dh=132, form=0) == 1 and vjp(form=2) == 1
    assert vjp(form=1, drop=0.1) == 1 and b"dropout" in err()
    assert vjp(form=0, drop=1.0) == 1
    assert vjp(ld=66) == 1 and vjp(ld=60) == 1 and b"pitch" in err()
    assert vjp(nbytes=16) == 3 and b"workspace" in err()
    for i in (0, 2, 3, 5, 6, 8, 10, 11, 22):
        assert vjp(null=i) == 1 and b"null" in err(), i
    # deformable adjoint: 1 <= P <= 8, head_dim <= 128, h * w == N, pitch >= 2 + 3 Hd P
    def dfm(P=2, dh=32, hh=2, ww=13, ldp=16, null=None):
        a = [p, ldp, p, p, 1, 3, 26, 2, P, dh, hh, ww, p, p, None]
        if null is not None:
            a[null] = None
        return lib.dod_op_deform_sample_bwd(*a)
    assert dfm(P=9, ldp=64) == 1 and b"points" in err()
    assert dfm(P=0) == 1 and dfm(dh=132) == 1
    assert dfm(hh=5, ww=5) == 1 and b"feature map" in err()
    assert dfm(ldp=12) == 1 and b"pitch" in err()
    for i in (0, 2, 3, 12, 13):
        assert dfm(null=i) == 1 and b"null" in err(), i
    # LoRA gradients: 1 <= r <= 64
    assert lib.dod_op_lora_grads_workspace_bytes(130, 64) > 0
    assert lib.dod_op_lora_grads_workspace_bytes(130, 65) == 0 and lib.dod_op_lora_grads_workspace_bytes(130, 0) == 0

    def lora(r=2, ldy=36, nbytes=big, null=None):
        a = [p, 100, p, ldy, 36, p, p, 65, r, 1.0, p, p, p, nbytes, None]
        if null is not None:
            a[null] = None
        return lib.dod_op_lora_grads(*a)
    assert lora(r=0) == 1 and lora(r=65) == 1 and b"1..64" in err()
    assert lora(ldy=32) == 1
    assert lora(nbytes=16) == 3
    for i in (0, 2, 5, 6, 10, 11, 12):
        assert lora(null=i) == 1 and b"null" in err(), i
    # element-wise adjoints and the column sum
    pw = lib.dod_op_train_pointwise
    assert pw(nat.PW["gelu_bwd"], None, p, p, 8, 0, 0.0, 0, None) == 1 and b"null" in err()
    assert pw(nat.PW["dropout_add"], None, None, p, 8, 0, 0.0, 0, None) == 1
    assert pw(nat.PW["dropout_add"], None, p, None, 8, 0, 0.0, 0, None) == 1
    assert pw(nat.PW["relu_drop_bwd"], p, p, p, 8, 0, 1.0, 0, None) == 1
    assert pw(nat.PW["swiglu_bwd"], p, p, p, 8, 0, 0.0, 0, None) == 1
    assert pw(nat.PW["sigmoid_bwd4"], p, p, p, 8, 3, 0.0, 0, None) == 1
    assert pw(17, p, p, p, 8, 0, 0.0, 0, None) == 1 and b"unknown op" in err()
    assert lib.dod_op_colsum_add(None, 4, 4, 4, p, None) == 1 and lib.dod_op_colsum_add(p, 4, 4, 4, None, None) == 1
    assert lib.dod_op_colsum_add(p, 3, 4, 4, p, None) == 1
    # the new test option is known by name
    assert lib.dod_test_set_option(b"attn_bwd_flash", 1) == 0 and lib.dod_test_set_option(b"attn_bwd_flash", -1) == 0


def test_attention_epilogue_operators_validate_arguments(lib):
    """dod_op_attention_bf16_mx / dod_op_attention_x3_h2 (the fp8 and fp16x2 modes' context epilogues): a null pointer, a non-positive
    size or a grid past one launch is DOD_ERR_INVALID with a message before any launch (no GPU here: a launch would be DOD_ERR_HIP)."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.dod_last_error(None)
    mx, h2 = lib.dod_op_attention_bf16_mx, lib.dod_op_attention_x3_h2
    for i in (0, 1, 2):
        a = [p, p, p, 1, 17, 2, 0.125, None]
        a[i] = None
        assert mx(*a) == 1 and b"null" in err(), i
    for i in (0, 1):
        a = [p, p, 1, 17, 2, 0.125, None]
        a[i] = None
        assert h2(*a) == 1 and b"null" in err(), i
    for B, N, heads in [(0, 17, 2), (-1, 17, 2), (1, 0, 2), (1, -5, 2), (1, 17, 0), (1, 17, -3)]:
        assert mx(p, p, p, B, N, heads, 0.125, None) == 1 and b"dod_op_attention_bf16_mx" in err() and b"positive" in err(), (B, N, heads)
        assert h2(p, p, B, N, heads, 0.125, None) == 1 and b"dod_op_attention_x3_h2" in err() and b"positive" in err(), (B, N, heads)
    # 2^20 images x 2^10 heads x 9 query blocks: more workgroups than a launch's int index
    assert mx(p, p, p, 1 << 20, 1000, 1 << 10, 0.125, None) == 1 and b"workgroups" in err()
    assert h2(p, p, 1 << 20, 1000, 1 << 10, 0.125, None) == 1 and b"workgroups" in err()
    assert mx(p, p, p, 1 << 16, 1, 1 << 16, 0.125, None) == 1 and h2(p, p, 1 << 16, 1, 1 << 16, 0.125, None) == 1      # B * heads past an int


def test_row_and_gather_operators_validate_arguments(lib):
    """dod_op_layernorm_form / dod_op_deform_sample_ex / dod_op_swiglu / dod_op_split3: a null pointer, a non-positive size or a shape the
    launcher does not take is DOD_ERR_INVALID with a message before any launch (no GPU here: a launch would be DOD_ERR_HIP)."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.dod_last_error(None)
    F = nat.LN_FORM
    two = {"f32_bf16", "fp8", "fp8_mx", "f32_s3"}

    def ln(form="f32", rows=5, D=64, null=None, out2="auto"):
        a = [p, p, p, p, 1e-6, rows, D, F[form] if isinstance(form, str) else form, p, (p if form in two else None) if out2 == "auto" else out2, None]
        if null is not None:
            a[null] = None
        return lib.dod_op_layernorm_form(*a)
    for form in F:
        for i in (0, 2, 3, 8):                                  # x, gamma, beta, out (add may be NULL)
            assert ln(form, null=i) == 1 and b"null" in err(), (form, i)
        assert ln(form, D=2052) == 1 and b"2048" in err(), form
        assert ln(form, D=66) == 1 and b"multiple of 4" in err(), form
        assert ln(form, rows=0) == 1 and ln(form, rows=-3) == 1 and ln(form, D=0) == 1 and b"positive" in err(), form
        if form in two:
            assert ln(form, out2=None) == 1 and b"null" in err(), form
        else:
            assert ln(form, out2=p) == 1 and b"out2 must be NULL" in err(), form
    assert ln("h2", D=48) == 1 and b"32" in err() and ln("h2", D=2044) == 1
    assert ln("fp8_mx", D=96) == 1 and b"64" in err() and ln("fp8_mx", D=32) == 1 and ln("fp8_mx", D=2016) == 1
    assert ln(-1) == 1 and ln(8) == 1 and b"unknown form" in err()

    def dfm(ldp=20, shared=0, B=3, Q=5, N=26, Hd=3, P=2, dh=32, hh=2, ww=13, null=None):
        a = [p, ldp, shared, p, B, Q, N, Hd, P, dh, hh, ww, p, None, None]
        if null is not None:
            a[null] = None
        return lib.dod_op_deform_sample_ex(*a)
    for i in (0, 3, 12):                                        # proj, values, out (out3 may be NULL)
        assert dfm(null=i) == 1 and b"null" in err(), i
    assert dfm(P=9, ldp=64) == 1 and b"points" in err() and dfm(P=0) == 1
    assert dfm(dh=129) == 1 and b"head_dim" in err() and dfm(dh=0) == 1
    assert dfm(hh=5, ww=5) == 1 and b"feature map" in err()
    assert dfm(ldp=19) == 1 and b"pitch" in err()
    for kw in (dict(B=0), dict(Q=-1), dict(Hd=0), dict(N=0, hh=0, ww=13), dict(N=0, hh=13, ww=0)):
        assert dfm(**kw) == 1 and b"positive" in err(), kw
    assert dfm(B=1 << 15, Q=1 << 15, Hd=3, shared=1) == 1 and b"items" in err()

    sw = lib.dod_op_swiglu
    assert sw(None, p, 0, 3, 5, None) == 1 and b"null" in err() and sw(p, None, 1, 3, 5, None) == 1 and b"null" in err()
    assert sw(p, p, 2, 3, 5, None) == 1 and b"dtype" in err()
    assert sw(p, p, 0, 0, 5, None) == 1 and sw(p, p, 1, 3, -1, None) == 1 and b"positive" in err()
    s3 = lib.dod_op_split3
    assert s3(None, 8, 2, 8, 0, p, None) == 1 and b"null" in err() and s3(p, 8, 2, 8, 0, None, None) == 1 and b"null" in err()
    assert s3(p, 7, 2, 8, 0, p, None) == 1 and b"pitch" in err()
    assert s3(p, 8, 0, 8, 0, p, None) == 1 and s3(p, 8, 2, 0, 1, p, None) == 1 and b"positive" in err()
    assert s3(p, 8, 2, 8, 2, p, None) == 1 and b"weight_order" in err()


def test_create_validates_arguments(lib):
    bb, dc = cases.cfg1(25)
    h = C.c_void_p()
    cfg = make_config(bb, dc, "bf16")
    assert lib.dod_create(C.byref(cfg), C.byref(h)) == 0
    # not finalized -> state error, message available
    assert lib.dod_workspace_bytes(h, 0, 224, 224) == 0
    rc = lib.dod_forward(h, None, 1, 224, 224, None, None, 0, None)
    assert rc == 3 and b"finalize" in lib.dod_last_error(h)
    rc = lib.dod_finalize_weights(h, None)
    assert rc == 2 and b"weights" in lib.dod_last_error(h)      # nothing registered
    lib.dod_destroy(h)
    bad = make_config(bb, dc, "bf16")
    bad.heads = 5                                                # 384 % 5 != 0
    h2 = C.c_void_p()
    assert lib.dod_create(C.byref(bad), C.byref(h2)) == 1
    assert b"backbone dims" in lib.dod_last_error(None)
    bad = make_config(bb, dc, "bf16")
    bad.target_dim = 128                                         # != decoder hidden 256
    assert lib.dod_create(C.byref(bad), C.byref(h2)) == 1
    with pytest.raises(ValueError):
        make_config(bb, dc, "fp4")
    assert make_config(bb, dc, "fp8").precision == 2          # DOD_PREC_FP8


def test_packed_accessor_rejects_bad_arguments_before_any_copy(lib):
    """dod_test_packed_info / dod_test_packed_copy: NULL handle, name, info or destination and a handle that is not finalized, before anything
    is read (an unknown name, an absent array and a short destination need a finalized handle: tests/test_gpu_pack.py)"""
    bb, dc = cases.cfg1(25)
    h = C.c_void_p()
    cfg = make_config(bb, dc, "bf16")
    assert lib.dod_create(C.byref(cfg), C.byref(h)) == 0
    info = nat.DodPackedInfo()
    buf = (C.c_char * 64)()
    assert lib.dod_test_packed_info(None, b"cls", C.byref(info)) == 1 and b"null handle" in lib.dod_last_error(None)
    assert lib.dod_test_packed_copy(None, b"cls", 0, buf, 64, None) == 1 and b"null handle" in lib.dod_last_error(None)
    assert lib.dod_test_packed_info(h, None, C.byref(info)) == 1 and b"null name" in lib.dod_last_error(h)
    assert lib.dod_test_packed_copy(h, None, 0, buf, 64, None) == 1 and b"null name" in lib.dod_last_error(h)
    for name in (b"cls", b"block.0.qkv", b"no.such.operand"):        # not finalized comes before the name is looked at
        assert lib.dod_test_packed_info(h, name, C.byref(info)) == 3 and b"finalize" in lib.dod_last_error(h)
        assert lib.dod_test_packed_copy(h, name, 0, buf, 64, None) == 3 and b"finalize" in lib.dod_last_error(h)
    lib.dod_destroy(h)
    assert C.sizeof(nat.DodPackedInfo) == 88                           # struct dod_packed_info
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    assert "int dod_test_packed_info(" in hdr and "int dod_test_packed_copy(" in hdr
    for name, value in list(nat.PK_ARRAY.items()) + [(v, k) for k, v in nat.PK_FORMAT.items()]:      # the binding's numbering is the header's
        token = {"w": "DOD_PK_W", "absent": "DOD_PK_ABSENT", "h2w": "DOD_PK_H2W", "split3w": "DOD_PK_SPLIT3W"}.get(name, "DOD_PK_" + name.upper())
        assert re.search(rf"{token} = {value}\b", hdr), token


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "fp16x2", "fp8"])
def test_create_rejects_a_swiglu_width_the_fast_modes_cannot_pack(lib, mode):
    """F = 344 (F % 64 != 0) exists in the fp32 mode only: the un-interleaved gate arm of dod_pack.hip for F % 32 != 0 is not reachable
    through dod_create (tests/pack_cases.py REJECTED)"""
    from tests import pack_cases as pc
    cs = pc.case("swiglu128-f344")
    assert (cs.name, mode) in pc.REJECTED
    h = C.c_void_p()
    cfg = make_config(cs.bb, cs.dc, mode)
    assert lib.dod_create(C.byref(cfg), C.byref(h)) == 1 and b"ffn_hidden" in lib.dod_last_error(None)
    cfg = make_config(cs.bb, cs.dc, "fp32")
    assert lib.dod_create(C.byref(cfg), C.byref(h)) == 0
    lib.dod_destroy(h)


@pytest.mark.parametrize("deform", [True, False])
def test_state_dict_keys_match_reference_layout(deform):
    """Keys/shapes equal the synthetic state dict, which tests/golden/make_goldens.py loads
    into the REFERENCE modules with strict=True."""
    from dinov2_od_amd.models import DINOv2ObjectDetector
    m = DINOv2ObjectDetector(dino_model_name="facebook/dinov2-small", hidden_dim=256, nheads=4, num_queries=25,
                             num_decoder_layers=2, dim_feedforward=512, lora_r=1, use_deformable=deform,
                             pretrained=False)
    bb, dc = cases.cfg1(25)
    dc.use_deformable = deform
    ref = synth.detector_state_dict(bb, dc)
    sd = m.state_dict()
    assert set(sd) == set(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == v.shape, k
    # frozen backbone, trainable LoRA / projection / decoder (dinov2_backbone.py:40-51)
    trainable = {k for k, p in m.named_parameters() if p.requires_grad}
    assert all(("lora_" in k) or k.startswith("decoder.") or k.startswith("backbone.projection") for k in trainable)
    assert any("lora_A" in k for k in trainable)
    if deform:   # tied decoder layers alias one storage (deformable_attention.py:284)
        a = m.state_dict(keep_vars=True)
        assert a["decoder.decoder.layers.0.linear1.weight"].data_ptr() == a["decoder.decoder.layers.1.linear1.weight"].data_ptr()


def test_forward_without_gpu_fails_loudly():
    from dinov2_od_amd.models import DINOv2ObjectDetector
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = DINOv2ObjectDetector(dino_model_name="facebook/dinov2-small", hidden_dim=256, nheads=4, num_queries=5,
                             num_decoder_layers=1, dim_feedforward=64, lora_r=1, pretrained=False).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError, match="channel dimension"):
        m(torch.zeros(1, 4, 224, 224))
    m.train()                      # train(): the autograd composite is GPU-only too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 224, 224))


def test_engine_named_cache_follows_replaced_parameters():
    """_engine_named() caches the (key, tensor) list; replacing a Parameter object after the first call (setattr of a block,
    register_parameter, load_state_dict(assign=True) on a child) must be seen -- the engine's (data_ptr, _version) signature of the
    OLD tensors would still match.  Host logic only."""
    from dinov2_od_amd.models import DINOv2ObjectDetector
    m = DINOv2ObjectDetector(dino_model_name="facebook/dinov2-small", hidden_dim=64, num_queries=5, num_decoder_layers=1,
                             dim_feedforward=64, lora_r=1, nheads=4, pretrained=False)
    a = dict(m._engine_named())
    assert m._engine_named() is m._engine_named()                      # cached
    key = "decoder.class_embed.weight"
    new = torch.nn.Parameter(torch.zeros_like(m.decoder.class_embed.weight))
    m.decoder.class_embed.weight = new                                  # no hook of the mixin sees this
    b = dict(m._engine_named())
    assert b[key] is new and a[key] is not new
    sd = {k: v.clone() for k, v in m.decoder.state_dict().items()}
    m.decoder.load_state_dict(sd, assign=True)                          # child-level assign: every tensor object replaced
    c = dict(m._engine_named())
    assert all(c["decoder." + k] is v for k, v in m.decoder.state_dict(keep_vars=True).items())


def test_abi_version_matches_header(lib):
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    assert int(re.search(r"#define DOD_ABI_VERSION (\d+)", hdr).group(1)) == lib.dod_abi_version() == nat.ABI_VERSION


# ---- the calling thread's error slot (include/dinodet.h, Conventions: errors)
# every status-returning entry point of track / criterion / jpeg / draw / detect / detect_views / preproc / roi_embed / warp / postproc /
# assign / matchcost .hip, with the status its all-NULL, all-zero call returns: a null pointer fails each one's first check, before any device call
ENTRY_POINTS = [
    ("dod_track_reset", 1), ("dod_track_update", 1), ("dod_track_update_app", 1), ("dod_track_embed_dots", 1), ("dod_track_embed_commit", 1),
    ("dod_track_export", 1),
    ("dod_set_criterion_forward", 1), ("dod_set_criterion_backward", 1), ("dod_set_criterion_layers_forward", 1),
    ("dod_set_criterion_layers_backward", 1),
    ("dod_jpeg_entropy_host", 1), ("dod_jpeg_entropy_device", 1), ("dod_jpeg_idct", 1), ("dod_jpeg_color", 1),
    ("dod_draw_detections", 1), ("dod_detect", 1), ("dod_detect_views", 1), ("dod_fuse_views", 1),
    ("dod_preprocess", 1), ("dod_preprocess_u8", 1), ("dod_preprocess_aug", 1), ("dod_preprocess_aug_u8", 1), ("dod_preprocess_compose", 1),
    ("dod_preprocess_compose_u8", 1), ("dod_preprocess_warp", 1), ("dod_preprocess_warp_u8", 1),
    ("dod_roi_embed", 1), ("dod_postprocess", 1), ("dod_match_assign", 1), ("dod_match_cost", 1),
]


def _null_args(name):
    """NULL for every pointer argument and zero for every number of entry point `name` (by the binding's argument types)"""
    return [0.0 if t in (C.c_float, C.c_double) else 0 if t in (C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_uint64) else None
            for t in nat.SYMBOLS[name][1]]


def _buf():
    return C.cast((C.c_double * 64)(), C.c_void_p)      # 8-byte aligned host memory: argument checks never read through it


# one more rejecting call per shared checker and per status other than DOD_ERR_INVALID: (entry point, arguments by position over the null
# call, status, a word of the message)
def _shape_cases():
    p = _buf()
    return [
        ("dod_track_update", {0: p, 3: p, 4: p, 5: p, 6: p, 8: C.byref(nat.DodTrackParams()), 9: p, 10: p}, 1, b"outside the limits"),      # S = T = K = 0
        ("dod_track_update_app", {9: C.byref(nat.DodTrackAppParams()), 10: p, 13: p}, 1, b"null argument or misaligned state"),       # its own check passes
        ("dod_set_criterion_forward", {0: p, 1: 4, 4: 1, 5: 1, 6: 4, 7: p, 9: 1}, 1, b"null losses"),                # the shared check passes
        ("dod_set_criterion_layers_forward", {0: p, 1: 4, 4: 1, 5: 1, 6: 1, 7: 4, 8: p, 10: 1, 16: p, 18: p}, 3, b"workspace too small"),
        ("dod_match_assign", {1: p, 2: 1, 3: 1, 7: p, 8: p}, 3, b"workspace"),
        ("dod_detect_views", {13: 2}, 1, b"nms_metric"),
        ("dod_preprocess_warp_u8", {0: p, 1: p, 2: p, 3: p, 4: 70000, 5: p, 6: p, 8: 8, 9: 8, 10: p}, 1, b"B=70000"),
    ]


@pytest.mark.parametrize("name,status", ENTRY_POINTS)
def test_every_rejecting_entry_point_names_itself(lib, name, status):
    assert lib.dod_test_set_option(b"no_such_option", 1) == 1                      # something else's message is in the slot
    assert getattr(lib, name)(*_null_args(name)) == status
    msg = lib.dod_last_error(None)
    assert msg.startswith(name.encode() + b":"), msg


@pytest.mark.parametrize("case", range(7))
def test_shared_checkers_name_the_entry_point_that_called_them(lib, case):
    name, over, status, word = _shape_cases()[case]
    args = _null_args(name)
    for i, v in over.items():
        args[i] = v
    assert getattr(lib, name)(*args) == status
    msg = lib.dod_last_error(None)
    assert msg.startswith(name.encode() + b":") and word in msg, msg


def test_entry_point_table_covers_the_twelve_files():
    """every extern "C" int function of the twelve files is in ENTRY_POINTS, and none of them returns a bare DOD_ERR_* constant or ends on a
    bare launch-error check: every such exit goes through dod_fail / dod_launched"""
    found = set()
    for f in ("track", "criterion", "jpeg", "draw", "detect", "detect_views", "preproc", "roi_embed", "warp", "postproc", "assign", "matchcost"):
        src = open(os.path.join(ROOT, "dinov2_od_amd", "csrc", f + ".hip")).read()
        found |= set(re.findall(r'^extern "C" int (dod_\w+)\(', src, re.M))
        assert not re.search(r"return DOD_ERR_\w+;|\? DOD_OK : DOD_ERR_HIP", src), f
    assert found == {n for n, _ in ENTRY_POINTS}
    csrc = os.path.join(ROOT, "dinov2_od_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in os.listdir(csrc))
    for gone in ("g_err", "g_terr", "g_oerr", "g_tail_owner", "g_f32k_owner"):
        assert not re.search(rf"\b{gone}\b", text), gone


def test_a_rejected_call_replaces_a_stale_message(lib):
    assert lib.dod_test_set_option(b"no_such_option", 1) == 1 and b"unknown test option" in lib.dod_last_error(None)
    assert lib.dod_track_update(*_null_args("dod_track_update")) == 1
    assert lib.dod_last_error(None).startswith(b"dod_track_update:")
    assert lib.dod_test_set_option(b"tailsplit", -1) == 0                          # a successful call leaves the slot alone
    assert lib.dod_last_error(None).startswith(b"dod_track_update:")


def _readers(lib):
    return lib.dod_last_error(None), lib.dod_decoder_train_last_error(), lib.dod_optim_last_error()


def test_the_three_readers_return_one_slot(lib):
    assert lib.dod_optim_ema_update(None, -1, 0.5, None) == 1
    a, b, c = _readers(lib)
    assert a == b == c and a.startswith(b"dod_optim_ema_update:")
    assert lib.dod_op_colsum_add(None, 4, 4, 4, None, None) == 1
    a, b, c = _readers(lib)
    assert a == b == c and a.startswith(b"dod_op_colsum_add:")
    assert lib.dod_detect(*_null_args("dod_detect")) == 1
    a, b, c = _readers(lib)
    assert a == b == c and a.startswith(b"dod_detect:")


def test_each_thread_reads_its_own_message(lib):
    """two threads fail in two different entry points (ctypes releases the GIL around the calls); a barrier holds both until both calls
    have returned, then each reads its own message through all three readers"""
    import threading
    barrier = threading.Barrier(2)
    calls = [lambda: lib.dod_test_set_option(b"no_such_option", 1), lambda: lib.dod_track_update(*_null_args("dod_track_update"))]
    want = [b"unknown test option 'no_such_option'", b"dod_track_update:"]
    got = [None, None]

    def work(i):
        for _ in range(50):
            rc = calls[i]()
            barrier.wait(timeout=30)
            got[i] = (rc, _readers(lib))
            barrier.wait(timeout=30)
            if rc != 1 or not all(m.startswith(want[i]) for m in got[i][1]):
                break
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    for i in range(2):
        assert got[i] is not None and got[i][0] == 1 and all(m.startswith(want[i]) for m in got[i][1]), (i, got[i])


def test_check_maps_each_status_as_its_call_site_did(lib):
    """_native.check: ValueError / KeyError / RuntimeError / RuntimeError for the four statuses, DodError beyond; the training steps'
    mapping (models/_native_train.py) keeps RuntimeError for everything but DOD_ERR_INVALID.  The text is the calling thread's message."""
    from dinov2_od_amd.models import _native_train as nt
    rc = lib.dod_match_cost(*_null_args("dod_match_cost"))
    for status, exc, texc in ((1, ValueError, ValueError), (2, KeyError, RuntimeError), (3, RuntimeError, RuntimeError), (4, RuntimeError, RuntimeError),
                              (9, nat.DodError, RuntimeError)):
        with pytest.raises(exc, match="dod_match_cost") as e:
            nat.check(status)
        assert type(e.value) is exc
        with pytest.raises(texc, match="dod_match_cost") as e:
            nt._check(status)
        assert type(e.value) is texc
    assert rc == 1
    nat.check(0)
    nt._check(0)
    from dinov2_od_amd import optim
    assert optim._check is nat.check


def test_stream_slab_rule_in_a_sanitized_standalone_program(tmp_path):
    """tests/stream_slabs_main.cpp includes only csrc/stream_slabs.h (the slot rule of both GEMM scratch pools); built with the host
    compiler and -fsanitize=address,undefined (a report of either aborts the program) it checks that one stream keeps its slot, four
    streams get four slots, a fifth evicts the least recently used and reset() forgets the owners."""
    import shutil
    import subprocess
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    static = None
    for flags in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        p = subprocess.run([cxx] + sanitize + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            static = flags
            break
    if static is None:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined here: {(p.stderr.strip().splitlines() or ['?'])[-1]}")
    exe = str(tmp_path / "stream_slabs_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + sanitize + static +
                       [os.path.join(ROOT, "tests", "stream_slabs_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.gpu
def test_python_call_sites_raise_what_they_raised_with_the_entry_point_named():
    """tracking, losses, matching and optim each make one call their own Python checks let through and the library rejects: ValueError,
    as before, and the text now names the entry point"""
    from dinov2_od_amd import losses, matching, optim, tracking
    dev = torch.device("cuda")
    trk = tracking.Tracker(num_streams=1, max_tracks=8, device=dev)
    state = trk._ensure(dev)
    trk._state = torch.empty(state.numel() + 8, dtype=torch.uint8, device=dev)[1:1 + state.numel()]      # misaligned: the table holds doubles
    with pytest.raises(ValueError, match="^dod_track_reset:"):
        trk.reset()
    x = torch.zeros(4, 3, device=dev)
    with pytest.raises(ValueError, match="^dod_set_criterion_forward:"):
        losses._FocalFn.apply(x, torch.zeros(4, dtype=torch.int64, device=dev), 0.25, -1.0, "mean")          # a negative gamma
    det = torch.zeros(2, 5, 3 + 4, device=dev)
    labels, gt, offs = torch.zeros(2, dtype=torch.int64, device=dev), torch.full((2, 4), 0.5, device=dev), torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="^dod_match_cost:"):
        matching.match_cost(det, 3, labels, gt, offs, rows_from=2)                                       # rows_from >= B
    w = torch.nn.Parameter(torch.ones(8, device=dev))
    w.grad = torch.ones(8, device=dev)
    with pytest.raises(ValueError, match="^dod_optim_clip_grad_norm:"):
        optim.clip_grad_norm_([w], float("nan"))
