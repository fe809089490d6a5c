"""CPU-side checks of the ROI embeddings and of the appearance entry points (include/dinodet.h): the separable restatement of
dod_roi_embed (tests/roi_embed_cases.py) against the literal grid^2 bilinear-sample mean, the weights' invariants, the argument errors of
dod_roi_embed, dod_forward_mem, dod_track_update_app, dod_track_embed_dots and dod_track_embed_commit (every call returns before a
launch), the argument checks of reid.roi_embed and of Tracker(appearance=True), and the header.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import reid, tracking
from dinov2_od_amd.engine import make_config
from dinov2_od_amd.postprocess import Detections
from tests import cases
from tests import roi_embed_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def _scene(gh, gw, D, first, seed, B=2):
    rng = np.random.default_rng(seed)
    N = first + gh * gw + 2                                              # two tokens behind the map as well
    feat = rng.normal(size=(B, N, D)).astype(np.float32)
    sizes = np.asarray([(70.0, 98.0), (33.0, 51.0)], np.float32)[:B]
    boxes = np.stack([rc.boxes_for(gh, gw, float(sizes[b, 0]), float(sizes[b, 1])) for b in range(B)])
    extra = rng.uniform(0.0, 0.9, (B, 8, 4)).astype(np.float32) * sizes[:, None, [1, 0, 1, 0]]
    extra = np.concatenate([np.minimum(extra[..., :2], extra[..., 2:]), np.maximum(extra[..., :2], extra[..., 2:]) + 1.0], axis=-1).astype(np.float32)
    return feat, np.concatenate([boxes, extra], axis=1), np.asarray([15, 16], np.int32)[:B], sizes


@pytest.mark.parametrize("gh,gw", [(5, 7), (1, 3), (6, 2)])
@pytest.mark.parametrize("grid", [1, 2, 4, 8])
def test_separable_form_equals_the_literal_sample_mean(gh, gw, grid):
    feat, boxes, counts, sizes = _scene(gh, gw, 12, 1, seed=gh * 100 + gw * 10 + grid)
    want = rc.literal(feat, 1, gh, gw, boxes, counts, sizes, grid)
    got, info = rc.separable(feat, 1, gh, gw, boxes, counts, sizes, grid)
    worst = float(np.max(np.abs(got - want)))
    print(f"{gh} x {gw} grid {grid}: worst difference {worst:.3g}")
    assert worst <= 1e-12
    ok = rc.valid_rows(boxes, counts)
    live = 0
    for b in range(boxes.shape[0]):
        for k in range(boxes.shape[1]):
            i = info[b][k]
            if i is None:
                assert not got[b, k].any()
                continue
            live += 1
            assert ok[b, k] and abs(float(np.linalg.norm(got[b, k])) - 1.0) < 1e-12
            for w in (i["wx"], i["wy"]):
                assert (w >= 0.0).all() and abs(float(w.sum()) - 1.0) < 1e-12 and int((w != 0).sum()) <= 2 * grid
    # of the eight committed rows: wholly outside, x2 <= x1, the NaN coordinate are zeros; of image 0 also the row beyond its count
    assert [info[0][k] is None for k in range(8)] == [False, False, False, True, True, True, False, False]
    assert info[0][15] is None and info[1][15] is not None and live >= 20


def test_constant_map_gives_one_unit_vector_for_every_valid_box():
    gh, gw, D = 4, 6, 8
    feat, boxes, counts, sizes = _scene(gh, gw, D, 1, seed=5)
    v = np.random.default_rng(1).normal(size=D).astype(np.float32)
    feat[:, 1:1 + gh * gw] = v
    for grid in (1, 3, 8):
        got, info = rc.separable(feat, 1, gh, gw, boxes, counts, sizes, grid)
        unit = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64))
        for b in range(2):
            for k in range(boxes.shape[1]):
                if info[b][k] is not None:
                    assert np.max(np.abs(got[b, k] - unit)) < 1e-14


def test_zero_weight_tokens_and_everything_outside_the_map_are_never_read():
    """NaN in CLS, behind the map and in a column no sample touches changes nothing (the literal form would read the upper neighbour)"""
    gh, gw, D = 3, 4, 8
    rng = np.random.default_rng(2)
    feat = rng.normal(size=(1, 1 + gh * gw + 2, D)).astype(np.float32)
    boxes = np.asarray([[[1.0, 1.0, 2.0, 2.0]]], np.float32)              # one sample, exactly on the centre of token (1, 1)
    a, _ = rc.separable(feat, 1, gh, gw, boxes, None, [(float(gh), float(gw))], 1)
    poisoned = np.full_like(feat, np.nan)
    poisoned[0, 1 + 1 * gw + 1] = feat[0, 1 + 1 * gw + 1]
    b, info = rc.separable(poisoned, 1, gh, gw, boxes, None, [(float(gh), float(gw))], 1)
    assert info[0][0]["tokens"] == 1 and np.array_equal(a, b) and np.isfinite(b).all()


def _aligned(nbytes):
    raw = (C.c_char * (nbytes + 16))()
    addr = (C.addressof(raw) + 15) // 16 * 16
    return raw, C.c_void_p(addr)


def test_roi_embed_rejects_bad_arguments_before_any_launch(lib):
    B, N, D, K = 2, 36, 8, 4
    keep_f, feat = _aligned(B * N * D * 4)
    keep_e, emb = _aligned(B * K * D * 4)
    boxes, counts, sizes = (C.c_float * (B * K * 4))(), (C.c_int32 * B)(), (C.c_float * (B * 2))()
    p = lambda a: C.cast(a, C.c_void_p)                                     # noqa: E731
    ok = dict(feat=feat, B=B, N=N, D=D, first=1, gh=5, gw=7, boxes=p(boxes), counts=p(counts), sizes=p(sizes), K=K, grid=4, emb=emb)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dod_roi_embed(a["feat"], a["B"], a["N"], a["D"], a["first"], a["gh"], a["gw"], a["boxes"], a["counts"], a["sizes"], a["K"],
                                 a["grid"], a["emb"], None)

    bads = [dict(feat=None), dict(boxes=None), dict(emb=None), dict(feat=C.c_void_p(feat.value + 4)), dict(emb=C.c_void_p(emb.value + 8)),
            dict(B=0), dict(B=-1), dict(K=0), dict(K=1025), dict(D=0), dict(D=2), dict(D=6), dict(D=2052), dict(grid=0), dict(grid=9),
            dict(gh=0), dict(gw=0), dict(gw=-3), dict(first=-1), dict(first=2), dict(gh=6), dict(N=35), dict(N=0),
            dict(gh=65536, gw=65536)]
    for bad in bads:
        assert call(**bad) == INVALID, bad


def test_forward_mem_rejects_bad_arguments_before_any_launch(lib):
    bb, dc = cases.cfg1(25)
    h = C.c_void_p()
    cfg = make_config(bb, dc, "bf16")
    assert lib.dod_create(C.byref(cfg), C.byref(h)) == 0
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.dod_forward_mem(None, p, 1, 224, 224, p, p, p, 64, None) == INVALID
    assert lib.dod_forward_mem(h, p, 1, 224, 224, p, None, p, 64, None) == INVALID and b"null" in lib.dod_last_error(h)
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert lib.dod_forward_mem(h, a[0], 1, 224, 224, a[1], a[2], a[3], 64, None) == INVALID, k
    assert lib.dod_forward_mem(h, p, 1, 224, 224, p, p, p, 64, None) == 3 and b"finalize" in lib.dod_last_error(h)      # the state error of dod_forward
    lib.dod_destroy(h)


def test_appearance_entry_points_reject_bad_arguments_before_any_launch(lib):
    S, T, K, D = 2, 8, 6, 8
    state = (C.c_double * (lib.dod_track_state_bytes(S, T) // 8))()
    need = lib.dod_track_workspace_bytes(S, T, K)
    ws = (C.c_double * (need // 8))()
    f, i = (C.c_float * (S * max(T, K) * max(K, D)))(), (C.c_int32 * (S * K))()
    p = lambda a: C.cast(a, C.c_void_p)                                     # noqa: E731
    trk = tracking.Tracker(appearance=True)
    par, app = trk.params, trk.app_params
    ok = dict(state=p(state), S=S, T=T, scores=p(f), labels=p(i), boxes=p(f), counts=p(i), K=K, par=C.pointer(par), app=C.pointer(app), dots=p(f),
              ids=p(i), tb=p(f), assoc=p(i), ws=p(ws), n=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dod_track_update_app(a["state"], a["S"], a["T"], a["scores"], a["labels"], a["boxes"], a["counts"], a["K"], a["par"], a["app"],
                                        a["dots"], a["ids"], a["tb"], a["assoc"], a["ws"], a["n"], None)

    bads = [dict(state=None), dict(scores=None), dict(labels=None), dict(boxes=None), dict(counts=None), dict(par=None), dict(app=None),
            dict(dots=None), dict(ids=None), dict(tb=None), dict(assoc=None), dict(ws=None), dict(n=need - 1), dict(S=0), dict(T=0), dict(T=513),
            dict(K=0), dict(K=1025), dict(state=C.c_void_p(p(state).value + 4))]
    for bad in bads:
        assert call(**bad) == INVALID, bad
    nan = float("nan")
    for field, v in (("appearance_thresh", nan), ("proximity_thresh", nan), ("momentum", nan), ("momentum", -0.1), ("momentum", 1.5)):
        q = nat.DodTrackAppParams.from_buffer_copy(app)
        setattr(q, field, v)
        assert call(app=C.pointer(q)) == INVALID, field
    for field, v in (("track_thresh", nan), ("max_age", -1), ("low_thresh", 0.9)):
        q = nat.DodTrackParams.from_buffer_copy(par)
        setattr(q, field, v)
        assert call(par=C.pointer(q)) == INVALID, field
    dots, commit = lib.dod_track_embed_dots, lib.dod_track_embed_commit
    for bad in ((None, p(f), S, T, K, D, p(f)), (p(f), None, S, T, K, D, p(f)), (p(f), p(f), S, T, K, D, None), (p(f), p(f), 0, T, K, D, p(f)),
                (p(f), p(f), S, 0, K, D, p(f)), (p(f), p(f), S, 513, K, D, p(f)), (p(f), p(f), S, T, 0, D, p(f)), (p(f), p(f), S, T, 1025, D, p(f)),
                (p(f), p(f), S, T, K, 0, p(f)), (p(f), p(f), S, T, K, 6, p(f)), (p(f), p(f), S, T, K, 2052, p(f))):
        assert dots(*bad, None) == INVALID, bad[2:6]
    for bad in ((None, p(f), p(i), S, T, K, D, 0.9), (p(f), None, p(i), S, T, K, D, 0.9), (p(f), p(f), None, S, T, K, D, 0.9),
                (p(f), p(f), p(i), 0, T, K, D, 0.9), (p(f), p(f), p(i), S, 513, K, D, 0.9), (p(f), p(f), p(i), S, T, 1025, D, 0.9),
                (p(f), p(f), p(i), S, T, K, 10, 0.9), (p(f), p(f), p(i), S, T, K, D, nan), (p(f), p(f), p(i), S, T, K, D, -0.5),
                (p(f), p(f), p(i), S, T, K, D, 1.25)):
        assert commit(*bad, None) == INVALID, bad[3:]


def test_header_declares_the_entries_and_the_abi_is_still_7(lib):
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    for name in ("dod_forward_mem", "dod_roi_embed", "dod_track_embed_dots", "dod_track_update_app", "dod_track_embed_commit"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in nat.SYMBOLS and hasattr(lib, name), name
    body = re.search(r"typedef struct dod_track_app_params \{(.*?)\} dod_track_app_params;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [f for f, _ in nat.DodTrackAppParams._fields_] and C.sizeof(nat.DodTrackAppParams) == 12
    assert re.search(r"#define DOD_ABI_VERSION 7\b", hdr) and nat.ABI_VERSION == 7 and lib.dod_abi_version() == 7
    assert C.sizeof(nat.DodTrackParams) == 36                              # the plain tracker's struct is untouched
    left = re.search(r"Left out on purpose:(.*?)Two choices differ", hdr, re.S).group(1)
    assert "remove_duplicate_stracks" in left and "camera-motion compensation" in left and "ReID" not in left
    for word in ("appearance_thresh", "proximity_thresh", "slot + 1024 * kind", "torchvision"):
        assert word in hdr, word


def _feat(B=2, N=36, D=8):
    return torch.zeros(B, N, D)


def test_roi_embed_checks_its_arguments_before_the_device():
    bx = torch.zeros(2, 4, 4)
    for kw, msg in ((dict(features=torch.zeros(2, 36, 8, dtype=torch.float64)), "features"), (dict(features=torch.zeros(36, 8)), "features"),
                    (dict(features=_feat(D=6)), "multiple of 4"), (dict(features=_feat(D=2052)), "multiple of 4"),
                    (dict(boxes=torch.zeros(3, 4, 4)), "boxes"), (dict(boxes=torch.zeros(2, 4, 5)), "boxes"), (dict(boxes=torch.zeros(2, 0, 4)), "1024"),
                    (dict(boxes=torch.zeros(2, 1025, 4)), "1024"), (dict(counts=torch.zeros(2, dtype=torch.int64)), "counts"),
                    (dict(counts=torch.zeros(3, dtype=torch.int32)), "counts"), (dict(grid=0), "grid"), (dict(grid=9), "grid"), (dict(grid=2.5), "grid"),
                    (dict(first_token=-1), "first_token"), (dict(first_token=36), "first_token"), (dict(grid_hw=(6, 7)), "does not fit"),
                    (dict(grid_hw=(0, 7)), "does not fit"), (dict(sizes=torch.zeros(3, 2)), "sizes")):
        a = dict(dict(features=_feat(), boxes=bx), **kw)
        with pytest.raises(ValueError, match=msg):
            reid.roi_embed(**a)
    with pytest.raises(ValueError, match="no CPU fallback"):                # the device comes last
        reid.roi_embed(_feat(), bx, grid_hw=(5, 7))
    assert [reid.spatial_factor(n) for n in (1, 35, 36, 37, 256, 1369, 12)] == [(1, 1), (5, 7), (6, 6), (1, 37), (16, 16), (37, 37), (3, 4)]


def _det(S=1, K=4, **over):
    d = dict(scores=torch.zeros(S, K), labels=torch.zeros(S, K, dtype=torch.int32), boxes=torch.zeros(S, K, 4),
             queries=torch.zeros(S, K, dtype=torch.int32), counts=torch.zeros(S, dtype=torch.int32))
    d.update(over)
    return Detections(**d)


def test_appearance_tracker_checks_its_arguments_before_the_device():
    for kw in (dict(appearance_thresh=float("nan")), dict(proximity_thresh=float("nan")), dict(momentum=float("nan")), dict(momentum=-0.1),
               dict(momentum=1.1)):
        with pytest.raises(ValueError):
            tracking.Tracker(appearance=True, **kw)
    plain = tracking.Tracker(num_streams=2)
    assert plain.appearance is False and plain.app_params is None and plain._emb is None
    with pytest.raises(ValueError, match="exactly when"):
        plain.update(_det(2), torch.zeros(2, 4, 8))
    with pytest.raises(ValueError, match="appearance=False"):
        plain.embeddings()
    t = tracking.Tracker(num_streams=2, max_tracks=16, appearance=True)
    assert {k: getattr(t.app_params, k) for k, _ in nat.DodTrackAppParams._fields_} == dict(
        appearance_thresh=np.float32(0.25), proximity_thresh=np.float32(0.5), momentum=np.float32(0.9))
    assert t.embeddings() is None and t.check() == [0, 0]
    t.reset()
    with pytest.raises(ValueError, match="exactly when"):
        t.update(_det(2))
    for e, msg in ((torch.zeros(2, 4, 8, dtype=torch.float64), "embeddings"), (torch.zeros(2, 5, 8), "embeddings"), (torch.zeros(2, 4), "embeddings"),
                   (torch.zeros(2, 4, 6), "multiple of 4"), (torch.zeros(2, 4, 2052), "multiple of 4")):
        with pytest.raises(ValueError, match=msg):
            t.update(_det(2), e)
    with pytest.raises(ValueError, match="no CPU fallback"):                # the device comes last
        t.update(_det(2), torch.zeros(2, 4, 8))
