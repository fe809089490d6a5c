"""Deep supervision (aux_loss=True) on the CPU: the autograd composite and the criterion's layer loop against golden G11 -- the
reference's own decoder states, heads, matcher and criterion per layer (tests/golden/make_goldens_aux.py) -- and the Python /
C surface the feature adds.  Tolerances are those tests/test_train_composite.py uses for the same quantities."""
import os
import re

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import losses as L
from dinov2_od_amd import synth
from dinov2_od_amd.models import DETRDecoder, DINOv2ObjectDetector
from tests import aux_cases as ac
from tests import cases
from tests import criterion_cases as cc
from tests.cases import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _composite_on_cpu(monkeypatch):
    monkeypatch.setenv("DINODET_COMPOSITE_ON_CPU", "1")


def _micro(dtype=torch.float32, **kw):
    Dd, Hd, Q, Ln, F, C, P, B, N = ac.MICRO
    m = DETRDecoder(num_queries=Q, hidden_dim=Dd, nheads=Hd, num_decoder_layers=Ln, num_classes=C, dim_feedforward=F, dropout=0.0,
                    n_points=P, use_deformable=True, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state_dict(ac.micro_cfg(), seed=1, prefix="").items()}, strict=True)
    return m.to(dtype)


def _layers(o):
    """decoder layers 0 .. L-1 of an output dict"""
    return list(o["aux_outputs"]) + [o]


def _check_step(m, o, g, tag, tg, B, mem=None):
    """outputs, per-layer losses and assignments, total loss and gradients of one supervised step against a G11 file"""
    nl = len(_layers(o))
    for j, oj in enumerate(_layers(o)):
        tol = 1e-4 if mem is not None else 1e-3               # decoder-only / through the backbone (test_train_composite.py)
        assert rel_err(oj["pred_logits"].detach().numpy(), g[f"{tag}.l{j}.logits"]) < tol, j
        assert rel_err(oj["pred_boxes"].detach().numpy(), g[f"{tag}.l{j}.boxes"]) < tol, j
    rec = ac.RecordingMatcher(ac.OracleMatcher())
    ld = L.SetCriterion(rec, o["pred_logits"].shape[-1], dict(cc.WEIGHTS))(o, tg)
    assert set(ld) == set(L.LOSS_KEYS) | {f"{k}_{i}" for k in L.LOSS_KEYS for i in range(nl - 1)}
    # the criterion matches the aux layers first (memory order of the packed detections), the last layer last
    assert len(rec.calls) == nl
    for j in range(nl):
        assert ac.same_assignment(rec.calls[j], ac.golden_indices(g, tag, j, B)), j
        for n, k in enumerate(L.LOSS_KEYS):
            mine = float(ld[k if j == nl - 1 else f"{k}_{j}"].detach())
            want = float(g[f"{tag}.l{j}.losses"][n])
            assert abs(mine - want) < 1e-3 * max(1.0, abs(want)), (j, k, mine, want)
    loss = sum(ld.values())
    assert abs(float(loss.detach()) - float(g[f"{tag}.loss"])) < 1e-3 * max(1.0, abs(float(g[f"{tag}.loss"])))
    loss.backward()
    worst = ac.grad_check(m, g, 2e-4, 2e-4)
    if mem is not None:
        pr, st = cases.grad_probe(mem.grad.numpy())
        assert rel_err(pr, g["dmem_probe"]) < 2e-4 and abs(st[2] - g["dmem_stat"][2]) <= 2e-4 * g["dmem_stat"][2]
    return worst


@pytest.mark.parametrize("name,dtype", [("g11_aux_micro", torch.float32), ("g11_aux_micro_f64", torch.float64)])
def test_composite_aux_step_matches_the_reference(name, dtype):
    Dd, Hd, Q, Ln, F, C, P, B, N = ac.MICRO
    g = cases.golden(name)
    m = _micro(dtype, aux_loss=True).train()
    mem = torch.from_numpy(cases.g1_memory(N, Dd)).to(dtype).requires_grad_(True)
    o = m(mem)
    assert len(o["aux_outputs"]) == Ln - 1
    worst = _check_step(m, o, g, "micro", ac.targets(C, dtype=dtype), B, mem)
    print(f"{name}: worst gradient probe error {worst[0]:.2e} ({worst[1]})")


def test_composite_aux_detector_step_matches_the_reference():
    """cfg1 with two decoder layers: the LoRA and projection gradients under deep supervision"""
    g = cases.golden("g11_aux_cfg1")
    model_name, R, B, kw = cases.G9_CASES[ac.DETECTOR]
    m = DINOv2ObjectDetector(dino_model_name=model_name, pretrained=False, aux_loss=True, **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.detector_state_dict(m._bb_cfg, m._dc_cfg, seed=1).items()}, strict=True)
    m.train()
    o = m(torch.from_numpy(synth.make_pixels(B, R, R, seed=0)))
    assert len(o["aux_outputs"]) == 1
    worst = _check_step(m, o, g, "cfg1", ac.targets(kw["num_classes"]), B)
    print(f"g11_aux_cfg1: worst gradient probe error {worst[0]:.2e} ({worst[1]})")


def test_default_is_unchanged_and_eval_has_no_aux_outputs():
    Dd, Hd, Q, Ln, F, C, P, B, N = ac.MICRO
    mem = torch.from_numpy(cases.g1_memory(N, Dd))
    plain, aux = _micro().train(), _micro(aux_loss=True).train()
    assert plain.aux_loss is False and list(plain.state_dict()) == list(aux.state_dict())
    with torch.no_grad():
        a, b = plain(mem), aux(mem)
    assert set(a) == {"pred_logits", "pred_boxes"}
    assert set(b) == {"pred_logits", "pred_boxes", "aux_outputs"}
    assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
    for o in b["aux_outputs"]:
        assert set(o) == {"pred_logits", "pred_boxes"} and o["pred_logits"].shape == (B, Q, C) and o["pred_boxes"].shape == (B, Q, 4)
    one = DETRDecoder(Q, Dd, Hd, 1, C, dim_feedforward=F, dropout=0.0, n_points=P, aux_loss=True).train()
    with torch.no_grad():
        assert one(mem)["aux_outputs"] == []


def test_aux_loss_is_the_last_keyword_and_the_dense_branch_raises():
    import inspect
    for cls in (DETRDecoder, DINOv2ObjectDetector):
        p = list(inspect.signature(cls.__init__).parameters.values())
        assert p[-1].name == "aux_loss" and p[-1].default is False
        assert [q.name for q in p].index("precision") < len(p) - 1
    with pytest.raises(ValueError, match="use_deformable"):
        DETRDecoder(7, 128, 4, 2, 11, use_deformable=False, aux_loss=True)
    with pytest.raises(ValueError, match="use_deformable"):
        DINOv2ObjectDetector(pretrained=False, backbone_config=cases.micro_bb(), hidden_dim=128, use_deformable=False, aux_loss=True)


def test_criterion_weight_fallback():
    """k_i is weighted by weight_dict[k_i] if present, else weight_dict[k], else 1"""
    Dd, Hd, Q, Ln, F, C, P, B, N = ac.MICRO
    m = _micro(aux_loss=True).train()
    with torch.no_grad():
        o = m(torch.from_numpy(cases.g1_memory(N, Dd)))
    tg = ac.targets(C)
    raw = L.SetCriterion(ac.OracleMatcher(), C, {})(o, tg)
    w = {"loss_ce": 2.0, "loss_bbox": 5.0, "loss_giou_0": 7.0, "loss_ce_1": 3.0}
    got = L.SetCriterion(ac.OracleMatcher(), C, w)(o, tg)
    want = {"loss_ce": 2.0, "loss_ce_0": 2.0, "loss_ce_1": 3.0, "loss_bbox": 5.0, "loss_bbox_0": 5.0, "loss_bbox_1": 5.0,
            "loss_giou": 1.0, "loss_giou_0": 7.0, "loss_giou_1": 1.0}
    assert set(got) == set(want)
    for k, f in want.items():
        assert torch.allclose(got[k], f * raw[k], rtol=1e-6), k
    # without the key the criterion is what it was
    plain = L.SetCriterion(ac.OracleMatcher(), C, w)({k: o[k] for k in ("pred_logits", "pred_boxes")}, tg)
    assert set(plain) == set(L.LOSS_KEYS) and all(torch.equal(plain[k], got[k]) for k in plain)


def test_header_declares_the_new_symbols_at_abi_6():
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    declared = set(re.findall(r"\b(dod_[a-z0-9_]+)\s*\(", hdr))
    new = {f"dod_decoder_train_aux_{k}" for k in ("tape_bytes", "workspace_bytes", "forward", "backward")}
    new |= {f"dod_set_criterion_layers_{k}" for k in ("workspace_bytes", "forward", "backward")}
    assert new <= declared and new <= set(nat.SYMBOLS)
    assert re.search(r"#define DOD_ABI_VERSION 7\b", hdr) and nat.ABI_VERSION == 7
