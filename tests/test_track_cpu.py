"""CPU-side checks of the tracker (dod_track_update, include/dinodet.h): the block-form Kalman filter of the restatement
(tests/track_cases.py) against ByteTrack's full 8 x 8 filter, the scene invariants of the association with ByteTrack's defaults, the
coverage the committed seeds must reach, the entry points' argument errors (every call returns before a launch) and the argument
checks of tracking.Tracker.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import tracking
from dinov2_od_amd.postprocess import Detections
from tests import track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def test_block_filter_equals_full_kalman_filter():
    """200 random tracks x 60 frames: mean and covariance of the block form stay within 1e-9 (relative) of ByteTrack's 8 x 8 filter with
    its Cholesky solve; the 8 x 8 covariance never leaves the four 2 x 2 blocks beyond rounding"""
    rng = np.random.default_rng(0)
    n, frames = 200, 60
    kf = tc.FullKalman()
    pos, vel = rng.uniform(50.0, 900.0, (n, 2)), rng.normal(0.0, 4.0, (n, 2))
    wh = rng.uniform(10.0, 300.0, (n, 2))

    def boxes():
        p, s = pos + rng.normal(0.0, 1.5, pos.shape), wh * rng.uniform(0.95, 1.05, wh.shape)
        return np.concatenate([p - s / 2, p + s / 2], axis=1).astype(np.float32)

    z = tc.measure(boxes())
    mean, cov = tc.initiate(z)
    full = [kf.initiate(z[i]) for i in range(n)]
    worst = off = 0.0
    for f in range(frames):
        pos += vel
        tc.predict(mean, cov)
        full = [kf.predict(m, P) for m, P in full]
        if f % 7 != 5:                                                   # some frames predict only, as a LOST track does
            z = tc.measure(boxes())
            tc.correct(mean, cov, z)
            full = [kf.update(m, P, z[i]) for i, (m, P) in enumerate(full)]
        for i, (m, P) in enumerate(full):
            B = tc.block_to_full(cov[i])
            worst = max(worst, float(np.max(np.abs(mean[i] - m) / np.maximum(np.abs(m), 1.0))), float(np.max(np.abs(B - P)[B != 0] / np.abs(P)[B != 0])))
            off = max(off, float(np.max(np.abs(P[B == 0])) / np.max(np.abs(P))))
    print(f"worst relative difference {worst:.3g}, largest off-block entry {off:.3g} of the largest entry")
    assert worst < 1e-9 and off < 1e-9


def _ids(frames, params=None, T=8):
    return [out[0][0] for out in tc.run(frames, 1, T, params)[1]]


def test_score_dip_keeps_the_id_through_the_second_pass():
    before = tc.BRANCH["hits2"]
    ids = _ids(tc.single_object(8, score=lambda f: 0.3 if f in (4, 5) else 0.9))
    assert [int(i[0]) for i in ids] == [1] * 8
    assert tc.BRANCH["hits2"] == before + 2


def test_five_frame_disappearance_returns_with_the_same_id():
    before = tc.BRANCH["refound"]
    frames = tc.single_object(14, visible=lambda f: not 5 <= f <= 9)
    tab, out = tc.run(frames, 1, 8)
    assert [int(o[0][0, 0]) for o in out] == [1] * 4 + [-1] * 5 + [1] * 5
    assert out[6][2]["state"][0, 0] == tc.LOST and out[9][2]["state"][0, 0] == tc.TRACKED
    assert tc.BRANCH["refound"] == before + 1 and int(tab["next_id"][0]) == 2


def test_one_frame_ghost_consumes_an_id_and_dies_tentative():
    ghost = (0.95, 2, 300.0, 300.0, 320.0, 330.0)
    frames = tc.single_object(6, extra=lambda f: [ghost] if f == 3 else [])
    tab, out = tc.run(frames, 1, 8)
    assert all(int(o[0][0, 0]) == 1 for o in out)
    assert int(out[2][0][0, 1]) == -1                                     # the ghost's own row: tentative, no id reported
    assert out[2][2]["state"][0, 1] == tc.TENTATIVE and out[2][2]["id"][0, 1] == 2
    assert out[3][2]["state"][0, 1] == tc.FREE
    assert int(tab["next_id"][0]) == 3 and int(tab["overflow"][0]) == 0


def test_max_age_expires_and_a_new_id_appears_one_frame_after_reappearance():
    before = tc.BRANCH["expired"]
    frames = tc.single_object(14, visible=lambda f: not 5 <= f <= 9)
    tab, out = tc.run(frames, 1, 8, dict(max_age=3))
    ids = [int(o[0][0, 0]) for o in out]
    assert ids == [1] * 4 + [-1] * 5 + [-1] + [2] * 4                      # frame 10 is the birth (tentative), frame 11 confirms it
    assert tc.BRANCH["expired"] == before + 1
    assert out[6][2]["state"][0, 0] == tc.LOST and out[7][2]["state"][0, 0] == tc.FREE      # last seen at frame 4: 8 - 4 > 3 is the first expiry


def test_committed_seeds_reach_every_branch():
    """a condition on the inputs of tests/test_gpu_track.py: its scenes together hit every branch of the restatement"""
    tc.BRANCH.clear()
    tc.run(tc.crossing_scene(), 2, 8)
    tc.run(tc.births_scene(), 3, 4)
    tc.run(tc.ties_scene(), 1, 8)
    tc.run(tc.invalid_rows_scene(), 1, 8)
    tc.run(tc.random_walk_scene(), 2, 32)
    tc.run(tc.single_object(14, visible=lambda f: not 5 <= f <= 9), 1, 1, dict(max_age=3))
    for k in ("hits1", "hits2", "hits3", "refound", "expired", "overflow", "births", "rows_gt_cols", "rows_lt_cols", "empty_side", "tie", "invalid_row"):
        assert tc.BRANCH[k] > 0, (k, dict(tc.BRANCH))
    assert tc.BRANCH["lsap_workspace"] == 0
    tc.run(tc.large_scene(frames=2), 1, 512)
    assert tc.BRANCH["lsap_workspace"] > 0


def test_random_walk_keeps_identities_apart():
    """sanity of the scene itself: ids are unique within a frame and a stream, and tracks live long"""
    tab, out = tc.run(tc.random_walk_scene(), 2, 32)
    for ids, _, _ in out:
        for row in ids:
            on = row[row >= 0]
            assert len(set(on.tolist())) == len(on)
    assert int(tab["next_id"].max()) < 64 and int(tab["overflow"].sum()) == 0


def test_header_states_the_contract(lib):
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    for name in ("dod_track_state_bytes", "dod_track_workspace_bytes", "dod_track_reset", "dod_track_update", "dod_track_export"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in nat.SYMBOLS and hasattr(lib, name)
    body = re.search(r"typedef struct dod_track_params \{(.*?)\} dod_track_params;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f for f, _ in nat.DodTrackParams._fields_] and C.sizeof(nat.DodTrackParams) == 36
    for word in ("remove_duplicate_stracks", "lapjv", "tentative slots are predicted too", "FREE (0), TENTATIVE (1), TRACKED (2) or LOST (3)"):
        assert word in hdr, word
    assert (tracking.FREE, tracking.TENTATIVE, tracking.TRACKED, tracking.LOST) == (tc.FREE, tc.TENTATIVE, tc.TRACKED, tc.LOST) == (0, 1, 2, 3)


def test_byte_queries(lib):
    sb, wb = lib.dod_track_state_bytes, lib.dod_track_workspace_bytes
    assert sb(1, 1) >= 8 * 8 + 12 * 8 + 5 * 4 + 3 * 4 and sb(2, 128) >= 2 * 128 * (160 + 20) + 2 * 12
    assert wb(1, 1, 1) > 0 and wb(8, 128, 100) >= 8 * (128 * 100 * 4 + 228 * 29) and wb(3, 512, 1024) == 3 * wb(1, 512, 1024)
    for S, T in ((0, 8), (-1, 8), (1, 0), (1, 513), (65536, 8)):
        assert sb(S, T) == 0 and wb(S, T, 8) == 0, (S, T)
    assert wb(1, 8, 0) == 0 and wb(1, 8, 1025) == 0


def test_entry_points_reject_bad_arguments_before_any_launch(lib):
    S, T, K = 2, 8, 6
    state = (C.c_double * (lib.dod_track_state_bytes(S, T) // 8))()
    need = lib.dod_track_workspace_bytes(S, T, K)
    ws = (C.c_double * (need // 8))()
    f, i = (C.c_float * (S * K * 4))(), (C.c_int32 * (S * K))()
    p = lambda a: C.cast(a, C.c_void_p)                                     # noqa: E731
    par = tracking.Tracker().params
    ok = dict(state=p(state), S=S, T=T, scores=p(f), labels=p(i), boxes=p(f), counts=p(i), K=K, par=C.pointer(par), ids=p(i), tb=p(f), ws=p(ws), n=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dod_track_update(a["state"], a["S"], a["T"], a["scores"], a["labels"], a["boxes"], a["counts"], a["K"], a["par"], a["ids"],
                                    a["tb"], a["ws"], a["n"], None)

    bads = [dict(state=None), dict(scores=None), dict(labels=None), dict(boxes=None), dict(counts=None), dict(par=None), dict(ids=None),
            dict(tb=None), dict(ws=None), dict(n=need - 1), dict(S=0), dict(S=-2), dict(T=0), dict(T=513), dict(K=0), dict(K=1025),
            dict(state=C.c_void_p(p(state).value + 4))]
    for bad in bads:
        assert call(**bad) == INVALID, bad
    for field, v in (("track_thresh", float("nan")), ("match_thresh", float("nan")), ("max_age", -1), ("low_thresh", 0.9)):
        q = nat.DodTrackParams.from_buffer_copy(par)
        setattr(q, field, v)
        assert call(par=C.pointer(q)) == INVALID, field
    assert lib.dod_track_reset(None, S, T, None, None) == INVALID and lib.dod_track_reset(p(state), S, 0, None, None) == INVALID
    assert lib.dod_track_reset(p(state), 0, T, None, None) == INVALID
    outs = [p(state)] * 10
    assert lib.dod_track_export(None, S, T, *outs, None) == INVALID and lib.dod_track_export(p(state), S, 600, *outs, None) == INVALID
    for k in range(10):
        a = list(outs)
        a[k] = None
        assert lib.dod_track_export(p(state), S, T, *a, None) == INVALID, k


def _det(S=1, K=4, **over):
    d = dict(scores=torch.zeros(S, K), labels=torch.zeros(S, K, dtype=torch.int32), boxes=torch.zeros(S, K, 4),
             queries=torch.zeros(S, K, dtype=torch.int32), counts=torch.zeros(S, dtype=torch.int32))
    d.update(over)
    return Detections(**d)


def test_tracker_checks_its_arguments_before_the_device():
    for kw in (dict(num_streams=0), dict(num_streams=65536), dict(max_tracks=0), dict(max_tracks=513), dict(track_thresh=float("nan")),
               dict(low_thresh=0.6, track_thresh=0.5), dict(max_age=-1), dict(max_age=2.5)):
        with pytest.raises(ValueError):
            tracking.Tracker(**kw)
    t = tracking.Tracker(num_streams=2, max_tracks=16)
    assert (t.num_streams, t.max_tracks) == (2, 16)
    d = {k: getattr(t.params, k) for k, _ in nat.DodTrackParams._fields_}
    assert d == {k: (np.float32(v) if isinstance(v, float) else int(v)) for k, v in tc.DEFAULTS.items()}
    assert t.check() == [0, 0]
    t.reset()
    with pytest.raises(ValueError, match="streams"):
        t.reset([2])
    for bad, msg in ((_det(1), "per stream"), (_det(2, scores=torch.zeros(2, 4, dtype=torch.float64)), "scores"),
                     (_det(2, labels=torch.zeros(2, 4, dtype=torch.int64)), "labels"), (_det(2, boxes=torch.zeros(2, 4, 5)), "boxes"),
                     (_det(2, counts=torch.zeros(3, dtype=torch.int32)), "counts"), (_det(2, 1025), "1024"),
                     (_det(2, scores=torch.zeros(2, 0), labels=torch.zeros(2, 0, dtype=torch.int32), boxes=torch.zeros(2, 0, 4)), "1024")):
        with pytest.raises(ValueError, match=msg):
            t.update(bad)
    with pytest.raises(ValueError, match="Detections"):
        t.update({"scores": 1})
    with pytest.raises(ValueError, match="no CPU fallback"):                # the device comes last
        t.update(_det(2))
    assert issubclass(tracking.TrackedDetections, Detections)
    td = tracking.TrackedDetections(*_det(1), ids=torch.tensor([[3, -1, 1, -1]], dtype=torch.int32), track_boxes=torch.zeros(1, 4, 4))
    assert td._fields == Detections._fields and len(td) == 5 and td.ids.shape == (1, 4)
    by = td.by_id()
    assert type(by) is Detections and by.labels.tolist() == [[3, -1, 1, -1]] and by.queries.tolist() == [[0, -1, 0, -1]]
    import dinov2_od_amd
    assert dinov2_od_amd.Tracker is tracking.Tracker
