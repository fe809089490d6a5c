"""GPU parity of the appearance association (dod_track_embed_dots, dod_track_update_app, dod_track_embed_commit) against its numpy +
scipy restatement (tests/track_app_cases.py), through the C ABI, every buffer the calls write between guard rows.  After every frame:
  dots        for non-FREE slots and valid rows within (D + 2) 2^-24 sum |a b| of the float64 product of the device's own slot_emb and emb:
              the fp32 MFMA accumulates the D products one rounding each (at most D - 1 additions and the product roundings, in any
              order: D u sum |a b| to first order; the two more cover the second-order terms)
  association ids, track boxes, assoc and the whole exported table equal the restatement fed the device's dots, bit for bit
  commit      a touched slot is within one fp32 ulp per element of the float64 commit of the device's previous table, every other slot
              is bit-identical
FREE slots' embedding rows, dots of FREE slots and emb rows beyond the counts are poisoned with NaN between the launches."""
import ctypes as C

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat, reid, synth, tracking
from dinov2_od_amd.postprocess import Detections
from tests import cases
from tests import guard_rows as gr
from tests import track_app_cases as ta
from tests import track_cases as tc

pytestmark = pytest.mark.gpu
VIEW = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.uint32}
U = 2.0 ** -24


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
    """a tracker through the C ABI, every buffer it writes between guard rows; app=None: the plain dod_track_update"""

    def __init__(self, S, T, K, D, params=None, app=None):
        self.L = nat.lib()
        self.S, self.T, self.K, self.D = S, T, K, D
        self.sb, self.wb = self.L.dod_track_state_bytes(S, T), self.L.dod_track_workspace_bytes(S, T, K)
        self.bufs = {"state": gr.guarded(-(-self.sb // 256), 64, torch.int32, gr.SENT_I), "ws": gr.guarded(-(-self.wb // 256), 64, torch.int32, gr.SENT_I),
                     "assoc": gr.guarded(S * K, 1, torch.int32, gr.SENT_I), "dots": gr.guarded(S * T, K, torch.float32, gr.SENT_F),
                     "slot_emb": gr.guarded(S * T, D, torch.float32, gr.SENT_F)}
        self.bufs.update(gr.buffers(S, K, ("ids", "boxes")))
        self.bufs["slot_emb"][1].zero_()
        trk = tracking.Tracker(**dict(params or {}, appearance=app is not None, **(app or {})))
        self.par, self.app = trk.params, trk.app_params
        nat.check(self.L.dod_track_reset(self._p("state"), S, T, None, nat.stream_ptr()))
        torch.cuda.synchronize()

    def _p(self, k):
        return nat.ptr(self.bufs[k][1])

    def slot_emb(self):
        return self.bufs["slot_emb"][1].cpu().numpy().reshape(self.S, self.T, self.D)

    def poison_free_slots(self, state):
        free = torch.from_numpy(state.reshape(-1) == tc.FREE).cuda()
        self.bufs["slot_emb"][1][free] = float("nan")
        return free

    def dots(self, emb):
        nat.check(self.L.dod_track_embed_dots(self._p("slot_emb"), nat.ptr(emb), self.S, self.T, self.K, self.D, self._p("dots"), nat.stream_ptr()))
        torch.cuda.synchronize()
        gr.untouched(self.bufs)
        return self.bufs["dots"][1].cpu().numpy().reshape(self.S, self.T, self.K)

    def update(self, frame):
        sc, lb, bx, ct = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in frame)
        a = (self._p("state"), self.S, self.T, nat.ptr(sc), nat.ptr(lb), nat.ptr(bx), nat.ptr(ct), self.K, C.byref(self.par))
        z = (self._p("ws"), self.wb, nat.stream_ptr())
        if self.app is None:
            nat.check(self.L.dod_track_update(*a, self._p("ids"), self._p("boxes"), *z))
        else:
            nat.check(self.L.dod_track_update_app(*a, C.byref(self.app), self._p("dots"), self._p("ids"), self._p("boxes"), self._p("assoc"), *z))
        torch.cuda.synchronize()
        gr.untouched(self.bufs)
        out = gr.shaped({k: self.bufs[k] for k in ("ids", "boxes")}, self.S, self.K)
        return out["ids"], out["boxes"], self.bufs["assoc"][1].cpu().numpy().reshape(self.S, self.K)

    def commit(self, emb):
        nat.check(self.L.dod_track_embed_commit(self._p("slot_emb"), nat.ptr(emb), self._p("assoc"), self.S, self.T, self.K, self.D, self.app.momentum,
                                                nat.stream_ptr()))
        torch.cuda.synchronize()
        gr.untouched(self.bufs)

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


def _parity(frames, embs, S, T, D, params=None, app=None):
    """every frame through the three launches and the restatement -> [(ids, track_boxes, assoc)] of the device"""
    K = frames[0][0].shape[1]
    dev = Dev(S, T, K, D, params, app or {})
    A = dict(ta.APP_DEFAULTS, **(app or {}))
    tab = tc.new_table(S, T)
    outs, worst = [], 0.0
    for f, (frame, e) in enumerate(zip(frames, embs)):
        counts = frame[3]
        e = e.copy()
        beyond = np.arange(K)[None, :] >= np.clip(counts, 0, K)[:, None]
        e[beyond] = np.nan                                                # emb rows beyond the counts
        emb = torch.from_numpy(e).cuda()
        free = dev.poison_free_slots(tab["state"])                       # FREE slots' embedding rows
        before = dev.slot_emb()
        # (a) the similarity matrix against the float64 product of the device's own operands
        dots = dev.dots(emb)
        want, mag = ta.dots64(before, e)
        live = (tab["state"] != tc.FREE)[:, :, None] & ~beyond[:, None, :]
        err, bd = np.abs(dots.astype(np.float64) - want)[live], ((D + 2) * U * mag)[live]
        if live.any():
            worst = max(worst, float(np.max(err / np.maximum(bd, 1e-300))))
            assert (err <= bd).all(), (f, float(np.max(err / bd)))
        dev.bufs["dots"][1][free] = float("nan")                         # dots of FREE slots
        # (b) the association, fed the device's dots
        ids, tb, assoc = dev.update(frame)
        want_ids, want_tb, want_assoc = ta.update_app(tab, frame, dots, params, A)
        assert np.array_equal(ids, want_ids), (f, ids.tolist(), want_ids.tolist())
        assert np.array_equal(assoc, want_assoc), (f, assoc.tolist(), want_assoc.tolist())
        assert np.array_equal(_bits(tb), _bits(want_tb)), f
        assert not tb[ids < 0].view(np.uint32).any()
        _same_table(dev.table(), tab, f"frame {f + 1}")
        # (c) the commit against float64 on the device's previous table
        dev.commit(emb)
        after = dev.slot_emb()
        want_emb, touched = ta.commit(before, e, assoc, A["momentum"])
        assert np.array_equal(after[~touched].view(np.uint32), before[~touched].view(np.uint32)), f
        if touched.any():
            ulp = np.spacing(np.abs(want_emb[touched]).astype(np.float32)).astype(np.float64)
            assert (np.abs(after[touched].astype(np.float64) - want_emb[touched]) <= ulp).all(), f
            assert np.isfinite(after[touched]).all()
        outs.append((ids, tb, assoc))
    print(f"dots: worst observed error / bound = {worst:.3f}")
    return outs


@pytest.mark.parametrize("D", [8, 260])
def test_swap_scene(D):
    frames, embs, truth = ta.swap_scene(S=2, K=8, frames=14, D=D)
    outs = _parity(frames, embs, 2, 6, D)
    assert ta.id_switches(outs, truth) == 0
    assert ta.id_switches(tc.run(frames, 2, 6)[1], truth) >= 1


@pytest.mark.parametrize("D", [8, 260])
def test_random_walk_scene(D):
    before = dict(ta.BRANCH)
    frames, embs, _ = ta.random_walk_app_scene(S=2, K=8, frames=16, D=D)
    outs = _parity(frames, embs, 2, 6, D)
    _parity(frames[:12], embs[:12], 2, 6, D, dict(fuse_score=False, class_aware=True), dict(appearance_thresh=0.4, proximity_thresh=0.8, momentum=0.5))
    for k in ("appearance_rejected", "proximity_rejected", "app_chosen", "base_chosen", "kind0", "kind1", "kind2"):
        assert ta.BRANCH[k] > before.get(k, 0), k
    kinds = np.concatenate([o[2][o[2] >= 0] // ta.KIND for o in outs])
    assert set(kinds.tolist()) == {0, 1, 2}


def test_closed_gates_equal_the_plain_update_on_the_device():
    frames, embs, _ = ta.random_walk_app_scene(S=2, K=8, frames=16, D=8)
    K, D = 8, 8
    a, b = Dev(2, 6, K, D, None, ta.CLOSED), Dev(2, 6, K, D)
    for frame, e in zip(frames, embs):
        emb = torch.from_numpy(e).cuda()
        a.dots(emb)
        ia, ba, assoc = a.update(frame)
        a.commit(emb)
        ib, bb, _ = b.update(frame)
        assert np.array_equal(ia, ib) and np.array_equal(_bits(ba), _bits(bb))
        _same_table(a.table(), b.table())
        assert ((assoc >= 0) | (ia < 0)).all()
    assert int(a.table()["next_id"].min()) > 5


def _to_detections(frame):
    sc, lb, bx, ct = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in frame)
    return Detections(sc, lb, bx, torch.zeros_like(lb), ct)


def test_tracker_with_appearance_keeps_the_ids_the_default_tracker_switches():
    frames, embs, truth = ta.swap_scene(S=2, K=8, frames=14, D=8)
    plain, app = tracking.Tracker(num_streams=2, max_tracks=6), tracking.Tracker(num_streams=2, max_tracks=6, appearance=True)
    assert plain._emb is None and app.embeddings() is None
    out_p, out_a = [], []
    _, slot_emb, want = ta.run_app(frames, embs, 2, 6)
    for frame, e in zip(frames, embs):
        det = _to_detections(frame)
        p, a = plain.update(det), app.update(det, torch.from_numpy(e).cuda())
        assert isinstance(a, tracking.TrackedDetections) and a.scores is det.scores and a.ids.shape == (2, 8)
        out_p.append((p.ids.cpu().numpy(),))
        out_a.append((a.ids.cpu().numpy(),))
    assert plain._emb is None
    assert ta.id_switches(out_p, truth) >= 1 and ta.id_switches(out_a, truth) == 0
    assert all(np.array_equal(o[0], w[0]) for o, w in zip(out_a, want))    # the restatement's ids (its dots differ from the device's in the last bits only)
    E = app.embeddings()
    assert E.shape == (2, 6, 8) and np.allclose(E.cpu().numpy(), slot_emb, atol=1e-5)
    state = app.tracks()["state"].cpu().numpy()
    assert np.allclose(E.norm(dim=-1).cpu().numpy()[state != tc.FREE], 1.0, atol=1e-6)
    app.reset([1])
    assert not E[1].any() and bool(E[0].any()) and app.tracks()["frame"].tolist() == [14, 0]
    app.reset()
    assert not app.embeddings().any()
    with pytest.raises(ValueError, match="channels"):
        app.update(_to_detections(frames[0]), torch.zeros(2, 8, 12, device="cuda"))


def test_model_track_with_an_appearance_tracker_is_the_pieces_composed_by_hand():
    from tests import gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "fp32", "facebook/dinov2-small")
    kw = dict(num_streams=2, max_tracks=16, track_thresh=0.0, low_thresh=-1.0, new_thresh=0.0, appearance=True)      # synthetic weights score low
    a, b = tracking.Tracker(**kw), tracking.Tracker(**kw)
    H, W = 70, 98
    for f in range(3):
        x = G.to_gpu(synth.make_pixels(2, H, W, seed=f))
        t = m.track(x, a, top_k=10, nms_iou=0.5)
        d = m.detect(x, top_k=10, nms_iou=0.5)
        _, mem = m._get_engine().forward_mem(x, m._engine_named())
        e = reid.roi_embed(mem, d.boxes, d.counts, (H, W), 4, 1, (H // 14, W // 14))
        u = b.update(d, e)
        assert isinstance(t, tracking.TrackedDetections) and t.ids.shape == (2, 10)
        for p, q in zip(t, d):
            assert torch.equal(p, q)
        assert torch.equal(t.ids, u.ids) and torch.equal(t.track_boxes, u.track_boxes)
        if f == 0:
            assert bool((t.ids > 0).any())
    ta_, tb_ = a.tracks(), b.tracks()
    for k in ta_:
        assert torch.equal(ta_[k].view(torch.int64) if ta_[k].dtype == torch.float64 else ta_[k], tb_[k].view(torch.int64) if tb_[k].dtype == torch.float64 else tb_[k])
    assert torch.equal(a.embeddings(), b.embeddings()) and bool(a.embeddings().any()) and not m.training
