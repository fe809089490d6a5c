"""dod_track_update_app, dod_track_embed_dots and dod_track_embed_commit (include/dinodet.h) restated in numpy + scipy on top of
tests/track_cases.py, and the scenes of tests/test_track_app_cpu.py and tests/test_gpu_track_app.py.

The filter, the IoU, the classification of the rows and the solver are track_cases'; steps 0..7 are its `update_stream`, repeated here
because two things differ: the cost of the first and the tentative association,
    d_iou = 1 - iou;  base = fuse_score ? 1 - iou * score : d_iou;  d_app = 0.5 * max(0, 1 - dots[slot, row])
    d_app = 1 where d_app > appearance_thresh or d_iou > proximity_thresh;  cost = (float) min(base, d_app)
and the one new output, assoc [K] = -1 or slot + 1024 * kind (0: hit in the second pass, 1: hit in the first or the tentative pass, 2: birth,
at every frame).  `commit` is dod_track_embed_commit in float64: kind 2 stores the row's embedding, kind 1 blends x = m E + (1 - m) e and
normalises.  `dots` is the float64 product the similarity matrix is held against; the restatement is fed either its fp32 narrowing (CPU
tests) or the device's own matrix (GPU tests).

BRANCH counts the gates; tests/test_track_app_cpu.py asserts that the committed seeds reach every one.
"""
import collections

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import track_cases as tc

F = np.float32
KIND = 1024
APP_DEFAULTS = dict(appearance_thresh=0.25, proximity_thresh=0.5, momentum=0.9)
CLOSED = dict(APP_DEFAULTS, appearance_thresh=-1.0)                       # every d_app is 1: the cost is track_cases' cost

BRANCH = collections.Counter()


def cost_matrix_app(tab, s, rows, cols, scores, labels, boxes, fuse, class_aware, dots, A):
    iou = tc.iou_matrix(tc.xyxy(tab["mean"][s, rows]), boxes[cols].astype(np.float64))
    if class_aware:
        iou = np.where(tab["label"][s, rows][:, None] != labels[cols][None, :], 0.0, iou)
    d_iou = 1.0 - iou
    base = 1.0 - iou * scores[cols].astype(np.float64)[None, :] if fuse else d_iou
    gap = 1.0 - dots[np.ix_(rows, cols)].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d_app = 0.5 * np.where(gap > 0.0, gap, 0.0)
        far_app, far_iou = d_app > np.float64(F(A["appearance_thresh"])), d_iou > np.float64(F(A["proximity_thresh"]))
        d_app = np.where(far_app | far_iou, 1.0, d_app)
        take_app = d_app < base
    BRANCH["appearance_rejected"] += int(far_app.sum())
    BRANCH["proximity_rejected"] += int((far_iou & ~far_app).sum())
    BRANCH["app_chosen"] += int(take_app.sum())
    BRANCH["base_chosen"] += int((~take_app).sum())
    return np.where(take_app, d_app, base).astype(np.float32)


def associate_app(tab, s, rows, cols, det, fuse, thresh, P, frame, slot_of, dots, A):
    """track_cases.associate with the fused cost; hits are applied to the table and to slot_of"""
    scores, labels, boxes = det
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if len(rows) == 0 or len(cols) == 0:
        return
    cost = cost_matrix_app(tab, s, rows, cols, scores, labels, boxes, fuse, P["class_aware"], dots, A)
    try:
        ri, ci = linear_sum_assignment(cost)
    except ValueError:
        return
    keep = cost[ri, ci] <= F(thresh)
    ri, ci = ri[keep], ci[keep]
    if len(ri) == 0:
        return
    t, j = rows[ri], cols[ci]
    mean, cov = tab["mean"][s, t], tab["cov"][s, t]
    tc.correct(mean, cov, tc.measure(boxes[j]))
    tab["mean"][s, t], tab["cov"][s, t] = mean, cov
    tab["state"][s, t] = tc.TRACKED
    tab["last_frame"][s, t] = frame
    tab["score"][s, t] = scores[j]
    tab["label"][s, t] = labels[j]
    slot_of[j] = t


def update_stream_app(tab, s, scores, labels, boxes, count, P, A, dots):
    """one frame of stream s with dots [T, K] fp32 -> (ids [K] i32, track_boxes [K, 4] f32, assoc [K] i32)"""
    K = len(scores)
    det = (scores, labels, boxes)
    frame = int(tab["frame"][s]) + 1
    cnt = min(max(int(count), 0), K)
    with np.errstate(invalid="ignore"):
        valid = (np.arange(K) < cnt) & np.isfinite(scores) & np.isfinite(boxes).all(axis=1) & (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
        is_hi = valid & (scores > F(P["track_thresh"]))
        is_lo = valid & ~is_hi & (scores > F(P["low_thresh"]))
    hi, lo = np.nonzero(is_hi)[0], np.nonzero(is_lo)[0]
    slot_of, kind = np.full(K, -1, np.int64), np.full(K, -1, np.int64)

    def mark(k):
        kind[(slot_of >= 0) & (kind < 0)] = k

    st = tab["state"][s]
    lost = np.nonzero(st == tc.LOST)[0]
    tab["mean"][s, lost, 7] = 0.0
    live = np.nonzero(st != tc.FREE)[0]
    mean, cov = tab["mean"][s, live], tab["cov"][s, live]
    tc.predict(mean, cov)
    tab["mean"][s, live], tab["cov"][s, live] = mean, cov
    # 3. first association: fused cost
    associate_app(tab, s, np.nonzero((st == tc.TRACKED) | (st == tc.LOST))[0], hi, det, P["fuse_score"], P["match_thresh"], P, frame, slot_of, dots, A)
    mark(1)
    # 4. second association: pure IoU, track_cases' own
    rows = np.nonzero((st == tc.TRACKED) & (tab["last_frame"][s] != frame))[0]
    tc.associate(tab, s, rows, lo, det, False, P["second_thresh"], P, frame, slot_of, "hits2")
    mark(0)
    st[(st == tc.TRACKED) & (tab["last_frame"][s] != frame)] = tc.LOST
    # 5. tentative: fused cost
    left = hi[slot_of[hi] < 0]
    associate_app(tab, s, np.nonzero(st == tc.TENTATIVE)[0], left, det, P["fuse_score"], P["tentative_thresh"], P, frame, slot_of, dots, A)
    mark(1)
    st[st == tc.TENTATIVE] = tc.FREE
    # 6. expiry
    st[(st == tc.LOST) & (frame - tab["last_frame"][s] > P["max_age"])] = tc.FREE
    # 7. birth: assoc names the slot at every frame, the id only at frame 1
    free = np.nonzero(st == tc.FREE)[0]
    born = left[(slot_of[left] < 0) & (scores[left] >= F(P["new_thresh"]))]
    n = min(len(born), len(free))
    t, j = free[:n], born[:n]
    assoc = np.where(slot_of >= 0, slot_of + KIND * np.maximum(kind, 0), -1)
    if n:
        tab["mean"][s, t], tab["cov"][s, t] = tc.initiate(tc.measure(boxes[j]))
        tab["id"][s, t] = tab["next_id"][s] + np.arange(n, dtype=np.int32)
        tab["label"][s, t] = labels[j]
        tab["score"][s, t] = scores[j]
        tab["last_frame"][s, t] = frame
        st[t] = tc.TRACKED if frame == 1 else tc.TENTATIVE
        assoc[j] = t + 2 * KIND
        if frame == 1:
            slot_of[j] = t
    for k in range(3):
        BRANCH[f"kind{k}"] += int(((assoc >= 0) & (assoc // KIND == k)).sum())
    tab["frame"][s] = frame
    tab["next_id"][s] += n
    tab["overflow"][s] += len(born) - n
    ids, tb = np.full(K, -1, np.int32), np.zeros((K, 4), np.float32)
    on = np.nonzero(slot_of >= 0)[0]
    ids[on] = tab["id"][s, slot_of[on]]
    tb[on] = tc.xyxy(tab["mean"][s, slot_of[on]]).astype(np.float32)
    return ids, tb, assoc.astype(np.int32)


def update_app(tab, frame, dots, params=None, app=None):
    """frame = (scores [S, K], labels, boxes, counts), dots [S, T, K] fp32 -> (ids [S, K], track_boxes [S, K, 4], assoc [S, K])"""
    P, A = dict(tc.DEFAULTS, **(params or {})), dict(APP_DEFAULTS, **(app or {}))
    scores, labels, boxes, counts = frame
    out = [update_stream_app(tab, s, scores[s], labels[s], boxes[s], counts[s], P, A, dots[s]) for s in range(len(counts))]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def dots64(slot_emb, emb):
    """[S, T, D], [S, K, D] -> the float64 product [S, T, K] and sum |a b| [S, T, K] (what its error bound scales with)"""
    a, b = slot_emb.astype(np.float64), emb.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.einsum("std,skd->stk", a, b), np.einsum("std,skd->stk", np.abs(a), np.abs(b))


def commit(slot_emb, emb, assoc, momentum):
    """dod_track_embed_commit in float64: slot_emb [S, T, D] f32, emb [S, K, D] f32, assoc [S, K] -> (the new table in float64 -- rows that
    are not touched hold the old fp32 values exactly --, touched bool [S, T])"""
    out = slot_emb.astype(np.float64)
    touched = np.zeros(slot_emb.shape[:2], bool)
    m = np.float64(F(momentum))
    for s, j in zip(*np.nonzero(assoc >= KIND)):
        k, t = int(assoc[s, j]) // KIND, int(assoc[s, j]) % KIND
        assert not touched[s, t], "the rows of a frame name distinct slots"
        touched[s, t] = True
        if k == 2:
            out[s, t] = emb[s, j].astype(np.float64)
        else:
            x = m * slot_emb[s, t].astype(np.float64) + (1.0 - m) * emb[s, j].astype(np.float64)
            ss = float(np.sum(x * x))
            out[s, t] = x / np.sqrt(ss) if ss > 0.0 else 0.0
    return out, touched


def run_app(frames, embs, S, T, params=None, app=None):
    """every frame through dots -> update_app -> commit, all on the host (dots narrowed to fp32, the committed table narrowed to fp32)
    -> (table, slot_emb, [(ids, track_boxes, assoc, table copy) per frame])"""
    tab = tc.new_table(S, T)
    A = dict(APP_DEFAULTS, **(app or {}))
    slot_emb = np.zeros((S, T, embs[0].shape[2]), np.float32)
    out = []
    for f, e in zip(frames, embs):
        with np.errstate(invalid="ignore"):
            d = dots64(slot_emb, e)[0].astype(np.float32)
        ids, tb, assoc = update_app(tab, f, d, params, app)
        slot_emb = commit(slot_emb, e, assoc, A["momentum"])[0].astype(np.float32)
        out.append((ids, tb, assoc, tc.copy_table(tab)))
    return tab, slot_emb, out


# ---- scenes with appearance: (frames, embs, truth) with truth [frames][S, K] = the object every row shows (-1: none) -------------------
def _appearance(n_obj, D, seed):
    """n_obj near-orthogonal unit vectors [n_obj, D]: random directions made orthogonal, then tilted towards a shared direction so that two
    objects' similarity is about 0.1"""
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.normal(size=(D, min(D, n_obj + 1))))[0].T
    base = [q[1 + i % (len(q) - 1)] + 0.35 * q[0] + (0.2 * rng.normal(size=D) / np.sqrt(D) if i >= len(q) - 1 else 0.0) for i in range(n_obj)]
    return np.stack([b / np.linalg.norm(b) for b in base])


def _observe(app, rng, noise):
    e = app + noise * rng.normal(size=app.shape) / np.sqrt(len(app))
    return (e / np.linalg.norm(e)).astype(np.float32)


def swap_scene(S=2, K=8, frames=14, D=8, seed=3, noise=0.05):
    """per stream two equal-sized objects on one line: object 0 walks right and stops dead at frame 6, object 1 walks left at the same pace
    and passes through it in frames 7..9.  The filter carries object 0's velocity on, so by geometry the passing object is the better
    continuation of track 0 and the two swap ids; their appearance is near-orthogonal.  Rows are shuffled per frame."""
    rng = np.random.default_rng(seed)
    app = _appearance(2, D, seed)
    out_f, out_e, truth = [], [], []
    for f in range(1, frames + 1):
        per, emb, who = [], np.zeros((S, K, D), np.float32), np.full((S, K), -1)
        for s in range(S):
            o = 5.0 * s
            x0 = 40.0 + 12.0 * min(f, 6) + o
            x1 = 196.0 - 12.0 * f + o
            rows = [(0.92, 1) + tc._box(x0, 100.0, 30.0, 60.0), (0.9, 1) + tc._box(x1, 100.0, 30.0, 60.0)]
            rows = [(r[0], r[1]) + tuple(np.float32(x) + np.float32(rng.normal(0, 0.3)) for x in r[2:]) for r in rows]
            order = rng.permutation(2)
            per.append([rows[i] for i in order])
            for j, i in enumerate(order):
                emb[s, j], who[s, j] = _observe(app[i], rng, noise), i
        out_f.append(tc.pack(per, K))
        out_e.append(emb)
        truth.append(who)
    return out_f, out_e, truth


def random_walk_app_scene(S=2, K=8, frames=16, n_obj=5, D=8, seed=11, noise=0.15):
    """track_cases.random_walk_scene's kind of scene (dropouts, score dips into the low band, ghosts) in a small area, every object with
    an appearance of its own; a ghost's embedding is random"""
    rng = np.random.default_rng(seed)
    app = _appearance(n_obj, D, seed)
    pos = rng.uniform(20.0, 140.0, (S, n_obj, 2))
    vel = rng.normal(0.0, 3.0, (S, n_obj, 2))
    wh = rng.uniform(24.0, 60.0, (S, n_obj, 2))
    gone = np.zeros((S, n_obj), np.int64)
    out_f, out_e, truth = [], [], []
    for f in range(frames):
        pos += vel + rng.normal(0.0, 0.5, pos.shape)
        vel += rng.normal(0.0, 0.3, vel.shape)
        per, emb, who = [], np.zeros((S, K, D), np.float32), np.full((S, K), -1)
        for s in range(S):
            rows = []
            for o in range(n_obj):
                if gone[s, o] > 0:
                    gone[s, o] -= 1
                    continue
                if f > 0 and rng.random() < 0.12:
                    gone[s, o] = rng.integers(1, 4)
                    continue
                sc = rng.uniform(0.15, 0.45) if rng.random() < 0.2 else rng.uniform(0.55, 0.98)
                rows.append((o, (sc, 1 + o % 3) + tc._box(pos[s, o, 0], pos[s, o, 1], wh[s, o, 0], wh[s, o, 1])))
            if rng.random() < 0.3:
                rows.append((-1, (rng.uniform(0.6, 0.9), 1) + tc._box(rng.uniform(0, 160.0), rng.uniform(0, 160.0), 20.0, 20.0)))
            rows = rows[:K]
            order = rng.permutation(len(rows))
            per.append([rows[i][1] for i in order])
            for j, i in enumerate(order):
                o = rows[i][0]
                who[s, j] = o
                emb[s, j] = _observe(app[o], rng, noise) if o >= 0 else _observe(rng.normal(size=D), rng, 0.0)
        out_f.append(tc.pack(per, K))
        out_e.append(emb)
        truth.append(who)
    return out_f, out_e, truth


def id_switches(outs, truth):
    """how often an object's reported id changes from one of its reported ids to another one: outs[f][0] = ids [S, K]"""
    last, n = {}, 0
    for o, who in zip(outs, truth):
        ids = o[0]
        for s, j in zip(*np.nonzero((ids >= 0) & (who >= 0))):
            key = (int(s), int(who[s, j]))
            if key in last and last[key] != int(ids[s, j]):
                n += 1
            last[key] = int(ids[s, j])
    return n
