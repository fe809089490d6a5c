#!/usr/bin/env python3
"""Tracker timing: dod_track_update (tracking.Tracker.update: one launch per frame for all streams) next to the host leg any host
tracker must at least pay for the same frame, and next to the detect call it follows.
  scenes     S=8 K=100 T=128 with about 40 live tracks per stream, and S=1 K=300 T=256 with about 120: objects on a random walk with
             score dips and dropouts, the other rows clutter below track_thresh (part of it in the low band); 48 frames, played forward
             and backward so that the table stays in its steady state however many calls are timed
  legs       native = Tracker.update (allocates ids and track_boxes per call, as a user calls it); native_c_call = dod_track_update
             alone into preallocated buffers; host_floor = counts / boxes / scores D2H, the SAME three linear_sum_assignment calls per
             stream on the matrices the restatement (tests/track_cases.py) solves for that frame, ids H2D -- no Kalman filter, no IoU, no
             bookkeeping: a floor, not a tracker; detect = postprocess.detect_packed on a packed buffer of the scene's shape (Q = K,
             91 classes, NMS 0.5), the call the update follows
  timing     device legs: hipEvent pairs around `reps` back-to-back calls on consecutive frames; host_floor: wall clock around the same
             number of frames, synchronised; samples of all legs alternating in one process, warm-up first; median / p10 / p90 per call
  agreement  the device ids of the 48 forward frames equal the restatement's (asserted)
One JSON line on stdout.
    python tools/bench_track.py [--steps 30] [--warmup 5]
  --appearance   the appearance tracker's launches instead, on the same two scenes with D = the default decoder width and a 16 x 16 token
             map (224 x 224 input): roi_embed, embed_dots, update_app next to dod_track_update on the same frames (two tables, one
             each), embed_commit, and model.track end to end with and without appearance (the default detector, batch = the scene's
             streams).  Every call is timed on its own with a hipEvent pair, the versions alternating frame by frame, 200 frames a run,
             two runs in the same call: median and p10 / p90 per call and run.  roi_embed's bytes are computed from the shapes (token
             rows read + rows written).
  --roi-only     nothing but 200 roi_embed launches per scene: for a kernel-trace run of its own"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dinov2_od_amd import _native as nat, synth  # noqa: E402
from dinov2_od_amd.postprocess import Detections, detect_packed  # noqa: E402
from dinov2_od_amd.tracking import Tracker  # noqa: E402
from tests import track_cases as tc  # noqa: E402

SCENES = [(8, 100, 128, 40), (1, 300, 256, 120)]      # S, K, T, objects per stream
FRAMES = 48


def scene(S, K, n_obj, frames, seed=0, area=1400.0):
    rng = np.random.default_rng(seed)
    pos, vel = rng.uniform(50.0, area, (S, n_obj, 2)), rng.normal(0.0, 2.0, (S, n_obj, 2))
    wh = rng.uniform(24.0, 80.0, (S, n_obj, 2))
    gone = np.zeros((S, n_obj), np.int64)
    out = []
    for f in range(frames):
        pos += vel + rng.normal(0.0, 0.4, pos.shape)
        per = []
        for s in range(S):
            rows = []
            for o in range(n_obj):
                if gone[s, o] > 0:
                    gone[s, o] -= 1
                    continue
                if f > 0 and rng.random() < 0.03:
                    gone[s, o] = rng.integers(1, 5)
                    continue
                sc = rng.uniform(0.15, 0.45) if rng.random() < 0.1 else rng.uniform(0.55, 0.98)
                rows.append((sc, 1 + o % 5) + tc._box(pos[s, o, 0], pos[s, o, 1], wh[s, o, 0], wh[s, o, 1]))
            while len(rows) < K:                                          # clutter: detect always fills its K rows
                rows.append((rng.uniform(0.01, 0.3), 1) + tc._box(rng.uniform(0, area), rng.uniform(0, area), rng.uniform(10, 60), rng.uniform(10, 60)))
            per.append([rows[i] for i in rng.permutation(K)])
        out.append(tc.pack(per, K))
    return out


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def _wall(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def _stats(ms, reps):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4),
            "samples": len(ms), "calls_per_sample": reps}


def _per_call(fns, frames):
    """every fn once per frame, in turn, each between its own event pair -> name -> [ms]"""
    ev = {k: [] for k, _ in fns}
    for _ in range(frames):
        for k, fn in fns:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            ev[k].append((s, e))
    torch.cuda.synchronize()
    return {k: [s.elapsed_time(e) for s, e in v] for k, v in ev.items()}


def _pcts(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4), "p90_ms": round(float(np.percentile(a, 90)), 4)}


def appearance(a):
    from dinov2_od_amd import reid
    from dinov2_od_amd.config import REF_DEFAULTS
    from dinov2_od_amd.models import DINOv2ObjectDetector
    from tests import roi_embed_cases as rc
    L = nat.lib()
    RUN, GH, GW, AREA = 200, 16, 16, 1450.0
    model = None if a.roi_only else DINOv2ObjectDetector(pretrained=False).cuda().eval()
    D = model._dc_cfg.hidden_dim if model is not None else (REF_DEFAULTS["hidden_dim"] or 768)
    out = {"tool": "bench_track --appearance", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "D": D, "token_map": [GH, GW],
           "frames_per_run": RUN, "runs": 2}
    for S, K, T, n_obj in SCENES:
        frames = scene(S, K, n_obj, FRAMES)
        dets = [Detections(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (f[0], f[1], f[2])), torch.zeros(S, K, dtype=torch.int32, device="cuda"),
                           torch.from_numpy(f[3]).cuda()) for f in frames]
        mem = torch.from_numpy(synth.normal(5, f"bench_track.mem.{S}", (S, 1 + GH * GW, D), 1.0).astype(np.float32)).cuda()
        sizes = torch.full((S, 2), AREA, device="cuda")
        embs = [reid.roi_embed(mem, d.boxes, d.counts, sizes, 4, 1, (GH, GW)) for d in dets]
        # bytes of one roi_embed launch, from the shapes: every touched token row is read once per box, every output row written once
        rows = 0
        for b in frames[0][2].reshape(-1, 4):
            m = rc.map_box(b, (AREA, AREA), GH, GW)
            if m is not None:
                rows += int((rc.axis_weights(m[0], m[2], GW, 4) != 0).sum()) * int((rc.axis_weights(m[1], m[3], GH, 4) != 0).sum())
        roi_bytes = (rows + S * K) * D * 4 + S * K * 16
        order = list(range(FRAMES - 2, 0, -1)) + list(range(FRAMES))
        pos = [0]

        def nxt():
            i = order[pos[0] % len(order)]
            pos[0] += 1
            return i

        emb_out = torch.empty(S, K, D, device="cuda")
        cur = [0]

        def roi():
            d = dets[cur[0]]
            nat.check(L.dod_roi_embed(nat.ptr(mem), S, 1 + GH * GW, D, 1, GH, GW, nat.ptr(d.boxes), nat.ptr(d.counts), nat.ptr(sizes), K, 4, nat.ptr(emb_out),
                                      nat.stream_ptr()))

        key = f"S{S}_K{K}_T{T}"
        if a.roi_only:
            for _ in range(RUN):
                roi()
            torch.cuda.synchronize()
            out[key] = {"roi_embed_bytes": roi_bytes, "token_rows_read": rows, "launches": RUN}
            continue
        plain, app = Tracker(num_streams=S, max_tracks=T), Tracker(num_streams=S, max_tracks=T, appearance=True)
        for d, e in zip(dets, embs):                                        # both tables into their steady state
            plain.update(d), app.update(d, e)
        ids, tb = torch.empty(S, K, dtype=torch.int32, device="cuda"), torch.empty(S, K, 4, device="cuda")
        assoc, dots = torch.empty(S, K, dtype=torch.int32, device="cuda"), torch.empty(S, T, K, device="cuda")
        ws = torch.empty(L.dod_track_workspace_bytes(S, T, K), dtype=torch.uint8, device="cuda")

        def step():
            cur[0] = nxt()

        def f_dots():
            nat.check(L.dod_track_embed_dots(nat.ptr(app._emb), nat.ptr(embs[cur[0]]), S, T, K, D, nat.ptr(dots), nat.stream_ptr()))

        def f_app():
            d = dets[cur[0]]
            nat.check(L.dod_track_update_app(nat.ptr(app._state), S, T, nat.ptr(d.scores), nat.ptr(d.labels), nat.ptr(d.boxes), nat.ptr(d.counts), K,
                                             C.byref(app.params), C.byref(app.app_params), nat.ptr(dots), nat.ptr(ids), nat.ptr(tb), nat.ptr(assoc),
                                             nat.ptr(ws), ws.numel(), nat.stream_ptr()))

        def f_plain():
            d = dets[cur[0]]
            nat.check(L.dod_track_update(nat.ptr(plain._state), S, T, nat.ptr(d.scores), nat.ptr(d.labels), nat.ptr(d.boxes), nat.ptr(d.counts), K,
                                         C.byref(plain.params), nat.ptr(ids), nat.ptr(tb), nat.ptr(ws), ws.numel(), nat.stream_ptr()))

        def f_commit():
            nat.check(L.dod_track_embed_commit(nat.ptr(app._emb), nat.ptr(embs[cur[0]]), nat.ptr(assoc), S, T, K, D, app.app_params.momentum, nat.stream_ptr()))

        x = torch.from_numpy(synth.make_pixels(S, 224, 224, seed=1).astype(np.float32)).cuda()
        kw = dict(top_k=K, threshold=-1.0)
        mp, ma = Tracker(num_streams=S, max_tracks=T), Tracker(num_streams=S, max_tracks=T, appearance=True)
        legs = [("step", step), ("roi_embed", roi), ("embed_dots", f_dots), ("update_app", f_app), ("update_plain", f_plain), ("embed_commit", f_commit)]
        e2e = [("track_plain", lambda: model.track(x, mp, **kw)), ("track_appearance", lambda: model.track(x, ma, **kw))]
        _per_call(legs, a.warmup * 4), _per_call(e2e, a.warmup * 2)
        leg = {"roi_embed_bytes": roi_bytes, "token_rows_read": rows, "dots_bytes_read_by_update_app": S * T * K * 4}
        for run in range(2):
            t = _per_call(legs, RUN)
            t.update(_per_call(e2e, RUN))
            leg[f"run{run + 1}"] = {k: _pcts(v) for k, v in t.items() if k != "step"}
        leg["overflow"] = app.check()
        out[key] = leg
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--appearance", action="store_true")
    ap.add_argument("--roi-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_track needs a GPU"
    if a.appearance or a.roi_only:
        return appearance(a)
    L = nat.lib()
    out = {"tool": "bench_track", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "frames": FRAMES}
    for S, K, T, n_obj in SCENES:
        frames = scene(S, K, n_obj, FRAMES)
        dets = [Detections(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (f[0], f[1], f[2])), torch.zeros(S, K, dtype=torch.int32, device="cuda"),
                           torch.from_numpy(f[3]).cuda()) for f in frames]
        # the restatement's pass: ids to compare with, and the matrices of its linear_sum_assignment calls per frame
        solved, per_frame = [], []
        real = tc.linear_sum_assignment
        tc.linear_sum_assignment = lambda c: (solved.append(c.copy()), real(c))[1]
        try:
            tab, want = tc.new_table(S, T), []
            for f in frames:
                solved.clear()
                want.append(tc.update(tab, f)[0])
                per_frame.append(list(solved))
        finally:
            tc.linear_sum_assignment = real
        trk = Tracker(num_streams=S, max_tracks=T)
        got = [trk.update(d).ids.cpu().numpy() for d in dets]
        agree = all(np.array_equal(g, w) for g, w in zip(got, want))
        assert agree, "device ids differ from the restatement"
        live = float(np.mean((tab["state"] == tc.TRACKED) | (tab["state"] == tc.LOST)) * T)
        order = list(range(FRAMES - 2, 0, -1)) + list(range(FRAMES))        # after the forward pass: back, then forward again, ...
        pos = [0]

        def nxt():
            i = order[pos[0] % len(order)]
            pos[0] += 1
            return i

        ids, tb = torch.empty(S, K, dtype=torch.int32, device="cuda"), torch.empty(S, K, 4, device="cuda")
        ws = torch.empty(L.dod_track_workspace_bytes(S, T, K), dtype=torch.uint8, device="cuda")
        state = trk._state

        def raw():
            d = dets[nxt()]
            nat.check(L.dod_track_update(nat.ptr(state), S, T, nat.ptr(d.scores), nat.ptr(d.labels), nat.ptr(d.boxes), nat.ptr(d.counts), K,
                                         C.byref(trk.params), nat.ptr(ids), nat.ptr(tb), nat.ptr(ws), ws.numel(), nat.stream_ptr()))

        def native():
            return trk.update(dets[nxt()])

        hpos = [0]

        def host():
            i = hpos[0] % FRAMES
            hpos[0] += 1
            d = dets[i]
            d.counts.cpu(), d.boxes.cpu(), d.scores.cpu()
            for c in per_frame[i]:
                real(c)
            torch.from_numpy(want[i]).cuda()

        Q, Cn = K, 91
        logits = synth.normal(3, f"bench_track.{S}.{K}", (S, Q, Cn), 1.5, -4.0)
        u = synth.uniform01(4, f"bench_track.boxes.{S}.{K}", (S, Q, 4)).astype(np.float32)
        packed = torch.from_numpy(np.concatenate([logits, u[..., :2], np.float32(0.02) + np.float32(0.38) * u[..., 2:]], -1).astype(np.float32)).cuda()
        detect = lambda: detect_packed(packed, Cn, (480.0, 640.0), top_k=K, nms_iou=0.5)      # noqa: E731
        reps, hreps = 48, 12
        for _ in range(a.warmup):
            _time(native, reps), _time(raw, reps), _time(detect, reps), _wall(host, hreps)
        tn, tr, td, th = [], [], [], []
        for _ in range(a.steps):
            tn.append(_time(native, reps))
            tr.append(_time(raw, reps))
            td.append(_time(detect, reps))
            th.append(_wall(host, hreps))
        leg = {"native": _stats(tn, reps), "native_c_call": _stats(tr, reps), "host_floor": _stats(th, hreps), "detect": _stats(td, reps),
               "ids_equal_restatement": agree, "live_tracks_per_stream": round(live, 1), "overflow": trk.check(),
               "lsap_calls_per_frame": round(float(np.mean([len(p) for p in per_frame])), 1)}
        leg["host_floor_over_native"] = round(leg["host_floor"]["median_ms"] / leg["native"]["median_ms"], 1)
        out[f"S{S}_K{K}_T{T}"] = leg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
