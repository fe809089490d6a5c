"""No GPU: the `train_precision` argument of the drop-in modules, the configuration it puts in front of the native training entry
points, and those entry points' answers to a bf16x3 size query."""
import ctypes

import pytest

from dinov2_od_amd import _native as nat
from dinov2_od_amd.engine import make_config
from tests import cases


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def _detector(**kw):
    from dinov2_od_amd.models import DINOv2ObjectDetector
    bb, dc = cases.cfg1(7)
    return DINOv2ObjectDetector(num_classes=dc.num_classes, dino_model_name="custom", lora_r=bb.lora_r, lora_alpha=bb.lora_alpha, hidden_dim=dc.hidden_dim,
                                num_queries=dc.num_queries, nheads=dc.nheads, num_decoder_layers=dc.num_layers, dim_feedforward=dc.dim_feedforward,
                                n_points=dc.n_points, use_deformable=dc.use_deformable, pretrained=False, precision="fp32", backbone_config=bb, **kw)


def test_constructors_validate_train_precision():
    from dinov2_od_amd.models import DETRDecoder, DINOv2Backbone
    bb = cases.micro_bb()
    m = _detector()
    assert m.train_precision == m.backbone.train_precision == m.decoder.train_precision == "fp32"
    m = _detector(train_precision="bf16x3")
    assert m.train_precision == m.backbone.train_precision == m.decoder.train_precision == "bf16x3"
    assert m.precision == m.backbone.precision == "fp32", "train_precision must not touch precision"
    assert DETRDecoder(7, 128, 4, 2, 11, train_precision="bf16x3").train_precision == "bf16x3"
    assert DINOv2Backbone("micro", pretrained=False, config=bb, train_precision="bf16x3").train_precision == "bf16x3"
    for bad in ("bf16", "fp8", "fp16x2", "", None, 3):
        for make in (lambda: _detector(train_precision=bad), lambda: DETRDecoder(7, 128, 4, 2, 11, train_precision=bad),
                     lambda: DINOv2Backbone("micro", pretrained=False, config=bb, train_precision=bad)):
            with pytest.raises(ValueError) as e:
                make()
            assert "fp32" in str(e.value) and "bf16x3" in str(e.value)


def test_setter_validates_and_reaches_the_children():
    m = _detector()
    assert m.set_train_precision("bf16x3") is m
    assert m.train_precision == m.backbone.train_precision == m.decoder.train_precision == "bf16x3"
    with pytest.raises(ValueError) as e:
        m.set_train_precision("bf16")
    assert "fp32" in str(e.value) and "bf16x3" in str(e.value)
    assert m.train_precision == m.backbone.train_precision == m.decoder.train_precision == "bf16x3", "a rejected value changed the mode"
    m.decoder.set_train_precision("fp32")
    assert (m.backbone.train_precision, m.decoder.train_precision) == ("bf16x3", "fp32")


def test_native_training_configs_carry_the_training_precision():
    from dinov2_od_amd.models import _native_train as nt
    m = _detector(train_precision="bf16x3")
    for mod in (m.backbone, m.decoder):
        cfg = nt.train_config(mod, mod._bb_cfg, mod._dc_cfg)
        assert cfg.precision == nat.PREC["bf16x3"]
    m.set_precision("bf16")             # eval() and the frozen prefix: not the training steps' business
    assert nt.train_config(m.decoder, m._bb_cfg, m._dc_cfg).precision == nat.PREC["bf16x3"]
    m.set_train_precision("fp32")
    assert nt.train_config(m.decoder, m._bb_cfg, m._dc_cfg).precision == nat.PREC["fp32"]
    m.decoder.train_precision = "fp8"   # set behind the setter's back: refused where the configuration is built
    with pytest.raises(ValueError):
        nt.train_config(m.decoder, m._bb_cfg, m._dc_cfg)


def test_library_exports_the_split_product_operators(lib):
    assert hasattr(lib, "dod_op_gemm_f32x3") and hasattr(lib, "dod_op_linear_f32x3")
    assert "dod_op_gemm_f32x3" in nat.SYMBOLS and nat.SYMBOLS["dod_op_gemm_f32x3"] == nat.SYMBOLS["dod_op_gemm_f32x"]
    n0, w0 = lib.dod_test_counter(b"f32x3_launches"), lib.dod_test_counter(b"f32x3_wide_launches")
    assert n0 >= w0 >= 0      # known counters (-1 = unknown name); other tests of the process may have launched the kernel already
    assert lib.dod_test_set_option(b"f32x3_tile", 128) == 0 and lib.dod_test_set_option(b"f32x3_tile", -1) == 0
    assert lib.dod_op_gemm_f32x3(None, 4, 0, 0, 0, None, 4, 0, 0, 0, None, 4, 0, 0, 1, 1, 1, 1, 1, 1.0, 0, 1, None) == 1      # null buffers: DOD_ERR_INVALID
    assert (lib.dod_test_counter(b"f32x3_launches"), lib.dod_test_counter(b"f32x3_wide_launches")) == (n0, w0), "a rejected call counted as a launch"


def test_size_queries_answer_bf16x3_with_the_fp32_numbers(lib):
    bb = cases.micro_bb()
    bb.target_dim, bb.layers = 64, 3
    deform, dense = cases.dec_cfg(True), cases.dec_cfg(False)
    fns = [(deform, "dod_decoder_train_tape_bytes", (2, 26)), (deform, "dod_decoder_train_workspace_bytes", (2, 26)),
           (deform, "dod_decoder_train_aux_tape_bytes", (3, 257)), (deform, "dod_decoder_train_aux_workspace_bytes", (3, 257)),
           (dense, "dod_dense_decoder_train_tape_bytes", (2, 17)), (dense, "dod_dense_decoder_train_workspace_bytes", (2, 17)),
           (deform, "dod_backbone_tail_tape_bytes", (3, 26, 2)), (deform, "dod_backbone_tail_workspace_bytes", (3, 26, 2))]
    for dc, fn, args in fns:
        f32 = getattr(lib, fn)(ctypes.byref(make_config(bb, dc, "fp32")), *args)
        x3 = getattr(lib, fn)(ctypes.byref(make_config(bb, dc, "bf16x3")), *args)
        assert f32 == x3 > 0, (fn, f32, x3)
