"""GPU parity of the tracker (dod_track_update) against its numpy + scipy restatement (tests/track_cases.py): after every frame the
ids, the track boxes and the whole exported table equal the restatement's bit for bit (doubles viewed as int64, floats as uint32).
ids, track_boxes, the state buffer and the workspace sit between guard rows that must stay untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, synth, tracking
from dinov2_od_amd.postprocess import Detections
from tests import cases
from tests import guard_rows as gr
from tests import track_cases as tc

pytestmark = pytest.mark.gpu
VIEW = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.uint32}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")


def _bits(a):
    return a.view(VIEW[a.dtype]) if a.dtype in VIEW else a


def _same_table(got, want, what=""):
    for k in tc.TABLE:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:4].tolist())


class Dev:
    """a tracker through the C ABI, every buffer it writes between guard rows"""

    def __init__(self, S, T, K, params=None):
        self.L = nat.lib()
        self.S, self.T, self.K = S, T, K
        self.sb, self.wb = self.L.dod_track_state_bytes(S, T), self.L.dod_track_workspace_bytes(S, T, K)
        assert self.sb > 0 and self.wb > 0
        self.bufs = {"state": gr.guarded(-(-self.sb // 256), 64, torch.int32, gr.SENT_I), "ws": gr.guarded(-(-self.wb // 256), 64, torch.int32, gr.SENT_I)}
        self.bufs.update(gr.buffers(S, K, ("ids", "boxes")))
        self.par = tracking.Tracker(**(params or {})).params
        self.reset()

    def _p(self, k):
        return nat.ptr(self.bufs[k][1])

    def reset(self, streams=None):
        mask = None
        if streams is not None:
            m = np.zeros(self.S, np.int32)
            m[list(streams)] = 1
            mask = torch.from_numpy(m).cuda()
        nat.check(self.L.dod_track_reset(self._p("state"), self.S, self.T, nat.ptr(mask), nat.stream_ptr()))
        torch.cuda.synchronize()

    def update(self, frame):
        sc, lb, bx, ct = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in frame)
        nat.check(self.L.dod_track_update(self._p("state"), self.S, self.T, nat.ptr(sc), nat.ptr(lb), nat.ptr(bx), nat.ptr(ct), self.K,
                                          C.byref(self.par), self._p("ids"), self._p("boxes"), self._p("ws"), self.wb, nat.stream_ptr()))
        torch.cuda.synchronize()
        gr.untouched(self.bufs)
        for a, b in zip((sc, lb, bx, ct), frame):                           # nothing of the input is changed
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(np.ascontiguousarray(b)))
        out = gr.shaped({k: self.bufs[k] for k in ("ids", "boxes")}, self.S, self.K)
        return out["ids"], out["boxes"]

    def table(self):
        S, T = self.S, self.T
        out = dict(mean=torch.empty(S, T, 8, dtype=torch.float64, device="cuda"), cov=torch.empty(S, T, 12, dtype=torch.float64, device="cuda"))
        for k in ("state", "id", "label", "last_frame"):
            out[k] = torch.empty(S, T, dtype=torch.int32, device="cuda")
        out["score"] = torch.empty(S, T, dtype=torch.float32, device="cuda")
        for k in ("frame", "next_id", "overflow"):
            out[k] = torch.empty(S, dtype=torch.int32, device="cuda")
        nat.check(self.L.dod_track_export(self._p("state"), S, T, *(nat.ptr(out[k]) for k in tc.TABLE), nat.stream_ptr()))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


def _parity(frames, S, T, params=None, dev=None, tab=None):
    """every frame through the device and the restatement; returns (dev, restatement table, [(ids, boxes)] of the device)"""
    K = frames[0][0].shape[1]
    dev = dev or Dev(S, T, K, params)
    tab = tc.new_table(S, T) if tab is None else tab
    outs = []
    for f, frame in enumerate(frames):
        ids, tb = dev.update(frame)
        want_ids, want_tb = tc.update(tab, frame, params)
        assert np.array_equal(ids, want_ids), (f, ids.tolist(), want_ids.tolist())
        assert np.array_equal(_bits(tb), _bits(want_tb)), f
        assert not tb[ids < 0].view(np.uint32).any()
        _same_table(dev.table(), tab, f"frame {f + 1}")
        outs.append((ids, tb))
    return dev, tab, outs


@pytest.mark.parametrize("fuse_score", [True, False])
@pytest.mark.parametrize("class_aware", [False, True])
def test_crossing_dropout_ghost_scene(class_aware, fuse_score):
    frames = tc.crossing_scene(S=2, K=8, frames=16)
    _, tab, outs = _parity(frames, 2, 8, dict(class_aware=class_aware, fuse_score=fuse_score))
    assert int(tab["next_id"].min()) >= 6 and (outs[-1][0] > 0).sum() >= 8


def test_simultaneous_births_overflow_and_leave_older_tracks_alone():
    _, tab, outs = _parity(tc.births_scene(S=3, K=8), 3, 4)
    assert tab["overflow"].tolist() == [8, 8, 8]                            # four dropped at frame 2 and four at frame 3, per stream
    assert (tab["id"][:, :2] == [1, 2]).all() and (tab["state"][:, :2] == tc.TRACKED).all()
    for ids, _ in outs:
        assert (np.sort(ids[:, :2], axis=1) == [1, 2]).all()


@pytest.mark.parametrize("T,K", [(1, 1), (1, 8), (8, 1)])
def test_one_slot_and_one_row(T, K):
    if K == 1:
        frames = tc.single_object(10, score=lambda f: 0.3 if f == 4 else 0.9, visible=lambda f: f not in (6, 7), K=1)
    else:
        frames = [tuple(a[:1] for a in f) for f in tc.crossing_scene(S=1, K=8, frames=10)]
    _, tab, _ = _parity(frames, 1, T)
    assert int(tab["frame"][0]) == 10 and (T > 1 or int(tab["overflow"][0]) > 0 or K == 1)


def test_empty_frames_and_empty_table():
    frames = tc.crossing_scene(S=2, K=8, frames=8)
    empty = tc.pack([[], []], 8)
    _parity([empty, empty] + frames[:3] + [empty] + frames[3:6] + [empty] * 3 + frames[6:], 2, 8, dict(max_age=2))


def test_duplicate_boxes_and_equal_scores():
    before = tc.BRANCH["tie"]
    _parity(tc.ties_scene(), 1, 8)
    _parity(tc.ties_scene(), 1, 8, dict(fuse_score=False, match_thresh=1.0, second_thresh=1.0, tentative_thresh=1.0))      # every 1.0 cost is kept: ties at the threshold
    assert tc.BRANCH["tie"] > before


def test_invalid_rows_and_nan_padding():
    before = tc.BRANCH["invalid_row"]
    _, tab, outs = _parity(tc.invalid_rows_scene(), 1, 8)
    assert tc.BRANCH["invalid_row"] >= before + 12
    assert int(tab["next_id"][0]) == 3 and all(sorted(ids[0].tolist()) == [-1] * 6 + [1, 2] for ids, _ in outs)


def test_random_walk_scene():
    _, tab, _ = _parity(tc.random_walk_scene(S=2, K=24, frames=64), 2, 32)
    assert int(tab["frame"][0]) == 64 and int(tab["next_id"].min()) > 14


def test_solver_state_in_the_workspace():
    """T + K = 1536 with more than tc.LDS_UNITS rows + columns in the first association of frame 2: the solver runs on the workspace"""
    before = tc.BRANCH["lsap_workspace"]
    _, tab, _ = _parity(tc.large_scene(frames=3), 1, 512)
    assert tc.BRANCH["lsap_workspace"] >= before + 2 and int(tab["overflow"][0]) > 0


def test_streams_are_independent_and_reset_is_per_stream():
    frames = tc.random_walk_scene(S=3, K=12, frames=12, n_obj=8, seed=5)
    dev, tab, outs = _parity(frames, 3, 16)
    for s in range(3):
        alone = [tuple(a[s:s + 1] for a in f) for f in frames]
        _, tab1, outs1 = _parity(alone, 1, 16)
        for k in tc.TABLE:
            assert np.array_equal(_bits(tab1[k][0]), _bits(tab[k][s])), (s, k)
        for (ids, tb), (ids1, tb1) in zip(outs, outs1):
            assert np.array_equal(ids[s], ids1[0]) and np.array_equal(_bits(tb[s]), _bits(tb1[0]))
    dev.reset(streams=[1])
    tc.reset(tab, [1])
    got = dev.table()
    _same_table(got, tab, "after reset")
    assert int(got["frame"][1]) == 0 and int(got["next_id"][1]) == 1 and not got["state"][1].any() and int(got["frame"][0]) == 12
    _parity(frames[:4], 3, 16, dev=dev, tab=tab)                            # stream 1 starts over (frame 1 births are TRACKED), 0 and 2 go on
    dev.reset()
    tc.reset(tab)
    _same_table(dev.table(), tab, "after full reset")


def test_two_runs_are_bit_identical():
    frames = tc.random_walk_scene(S=2, K=24, frames=16)
    a, b = Dev(2, 32, 24), Dev(2, 32, 24)
    for f in frames:
        (ia, ba), (ib, bb) = a.update(f), b.update(f)
        assert np.array_equal(ia, ib) and np.array_equal(_bits(ba), _bits(bb))
    ta, tb = a.table(), b.table()
    _same_table(ta, tb)


def _to_detections(frame):
    sc, lb, bx, ct = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in frame)
    return Detections(sc, lb, bx, torch.zeros_like(lb), ct)


def test_tracker_class_and_by_id_through_draw_detections():
    from dinov2_od_amd.visualize import draw_detections
    frames = tc.crossing_scene(S=2, K=8, frames=6)
    trk = tracking.Tracker(num_streams=2, max_tracks=8)
    tab = tc.new_table(2, 8)
    images = torch.full((2, 360, 360, 3), 40, dtype=torch.uint8, device="cuda")
    for frame in frames:
        det = _to_detections(frame)
        t = trk.update(det)
        want_ids, want_tb = tc.update(tab, frame)
        assert isinstance(t, tracking.TrackedDetections) and t.scores is det.scores and t.boxes is det.boxes and t.counts is det.counts
        assert np.array_equal(t.ids.cpu().numpy(), want_ids) and np.array_equal(_bits(t.track_boxes.cpu().numpy()), _bits(want_tb))
        got = {k: v.cpu().numpy() for k, v in trk.tracks().items()}
        _same_table(got, tab)
        on = want_ids >= 0
        hand = Detections(torch.from_numpy(np.where(on, frame[0], np.float32(0))).cuda(), torch.from_numpy(want_ids).cuda(),
                          torch.from_numpy(np.where(on[..., None], frame[2], np.float32(0))).cuda(),
                          torch.from_numpy(np.where(on, 0, -1).astype(np.int32)).cuda(), det.counts)
        by = t.by_id()
        assert type(by) is Detections
        for a, b in zip(by, hand):
            assert torch.equal(a, b)
        a, b = draw_detections(images, by), draw_detections(images, hand)
        assert torch.equal(a, b) and bool((a != images).any())
    assert trk.check() == [0, 0]
    trk.reset([0])
    tc.reset(tab, [0])
    _same_table({k: v.cpu().numpy() for k, v in trk.tracks().items()}, tab)
    small = tracking.Tracker(num_streams=2, max_tracks=2)
    small.update(_to_detections(frames[0]))
    assert small.check() == [2, 2]
    with pytest.raises(RuntimeError, match="overflow"):
        small.check(strict=True)


def test_model_track_is_detect_then_update():
    from tests import gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "fp32", "facebook/dinov2-small")
    kw = dict(num_streams=2, max_tracks=16, track_thresh=0.0, low_thresh=-1.0, new_thresh=0.0)      # synthetic weights score low: every valid row counts as high
    a, b = tracking.Tracker(**kw), tracking.Tracker(**kw)
    for f in range(3):
        x = G.to_gpu(synth.make_pixels(2, 224, 224, seed=f))
        t = m.track(x, a, top_k=10, nms_iou=0.5)
        d = m.detect(x, top_k=10, nms_iou=0.5)
        u = b.update(d)
        assert isinstance(t, tracking.TrackedDetections) and t.ids.shape == (2, 10)
        for p, q in zip(t, d):
            assert torch.equal(p, q)
        assert torch.equal(t.ids, u.ids) and torch.equal(t.track_boxes, u.track_boxes)
        if f == 0:
            assert bool((t.ids > 0).any())
    ta, tb = a.tracks(), b.tracks()
    for k in ta:
        assert torch.equal(ta[k].view(torch.int64) if ta[k].dtype == torch.float64 else ta[k], tb[k].view(torch.int64) if tb[k].dtype == torch.float64 else tb[k])
    assert not m.training
