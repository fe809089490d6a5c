"""dod_track_update (include/dinodet.h) restated in numpy + scipy, and the seeded scenes of tests/test_track_cpu.py and
tests/test_gpu_track.py.

The contract, as the header states it.  A tracker owns S streams of T slots (FREE / TENTATIVE / TRACKED / LOST); the table is held
here as the arrays dod_track_export writes (`new_table`).  One `update` of a stream: count the frame and classify the rows (valid,
high, low); predict every live slot (a LOST slot's velocity of h zeroed first); first association of TRACKED + LOST slots against the
high rows (cost 1 - iou * score with fuse_score), second association of the TRACKED slots still without a hit against the low rows
(cost 1 - iou), the rest of them become LOST; tentative slots against the high rows left over, misses freed; LOST slots older than
max_age freed; births into the lowest free slots in row order (TRACKED at frame 1, TENTATIVE later), overflow counted.  Association
is scipy.optimize.linear_sum_assignment on the fp32 cost matrix, then the pairs with cost <= threshold.

The filter is ByteTrack's constant-velocity Kalman filter over (cx, cy, a, h) in its block form -- four independent 2 x 2 blocks
(p, c, v) per slot, a scalar innovation per component -- with every double operation written out in the order the kernel performs it
(numpy's float64 array operations round once each, as the kernel's do without FMA contraction).  `FullKalman` is the same filter as
ByteTrack writes it (8 x 8 covariance, Cholesky solve), which tests/test_track_cpu.py holds the block form against.

BRANCH counts what the scenes exercise; tests/test_track_cpu.py asserts that the committed seeds reach every branch.
"""
import collections

import numpy as np
import scipy.linalg
from scipy.optimize import linear_sum_assignment

F = np.float32
FREE, TENTATIVE, TRACKED, LOST = 0, 1, 2, 3
MAX_TRACKS, MAX_ROWS = 512, 1024
LDS_UNITS = 1024                     # rows + columns of an association problem up to which the kernel keeps the solver state in LDS
STD_POS, STD_VEL = 1.0 / 20, 1.0 / 160
INIT_POS, INIT_VEL = 2.0 * STD_POS, 10.0 * STD_VEL
ASP_INIT, ASP_VEL, ASP_MEAS = 1e-2, 1e-5, 1e-1
DEFAULTS = dict(track_thresh=0.5, low_thresh=0.1, new_thresh=0.6, match_thresh=0.8, second_thresh=0.5, tentative_thresh=0.7,
                max_age=30, fuse_score=True, class_aware=False)
TABLE = ("mean", "cov", "state", "id", "label", "last_frame", "score", "frame", "next_id", "overflow")

BRANCH = collections.Counter()


def new_table(S, T):
    t = dict(mean=np.zeros((S, T, 8)), cov=np.zeros((S, T, 12)), state=np.zeros((S, T), np.int32), id=np.zeros((S, T), np.int32),
             label=np.zeros((S, T), np.int32), last_frame=np.zeros((S, T), np.int32), score=np.zeros((S, T), np.float32),
             frame=np.zeros(S, np.int32), next_id=np.ones(S, np.int32), overflow=np.zeros(S, np.int32))
    return t


def reset(tab, streams=None):
    for s in range(len(tab["frame"])) if streams is None else streams:
        for k in TABLE:
            tab[k][s] = 1 if k == "next_id" else 0


def copy_table(tab):
    return {k: v.copy() for k, v in tab.items()}


# ---- the filter, block form: mean [n, 8], cov [n, 12] = (p, c, v) of cx, cy, a, h ------------------------------------------------
def measure(boxes):
    """fp32 xyxy [n, 4] -> z [n, 4] double (cx, cy, a, h)"""
    b = boxes.astype(np.float64)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    with np.errstate(all="ignore"):
        return np.stack([b[:, 0] + 0.5 * w, b[:, 1] + 0.5 * h, w / h, h], axis=1)


def xyxy(mean):
    w = mean[..., 2] * mean[..., 3]
    return np.stack([mean[..., 0] - 0.5 * w, mean[..., 1] - 0.5 * mean[..., 3], mean[..., 0] + 0.5 * w, mean[..., 1] + 0.5 * mean[..., 3]], axis=-1)


def predict(mean, cov):
    """in place"""
    h = mean[:, 3].copy()
    sp, sv = STD_POS * h, STD_VEL * h
    qp, qv = sp * sp, sv * sv
    for c in range(4):
        qpc, qvc = (ASP_INIT * ASP_INIT, ASP_VEL * ASP_VEL) if c == 2 else (qp, qv)
        p, cc, v = cov[:, 3 * c].copy(), cov[:, 3 * c + 1].copy(), cov[:, 3 * c + 2].copy()
        mean[:, c] = mean[:, c] + mean[:, 4 + c]
        cov[:, 3 * c] = (((p + cc) + cc) + v) + qpc
        cov[:, 3 * c + 1] = cc + v
        cov[:, 3 * c + 2] = v + qvc


def correct(mean, cov, z):
    """in place"""
    sp = STD_POS * mean[:, 3]
    r = sp * sp
    for c in range(4):
        rc = ASP_MEAS * ASP_MEAS if c == 2 else r
        p, cc, v = cov[:, 3 * c].copy(), cov[:, 3 * c + 1].copy(), cov[:, 3 * c + 2].copy()
        s = p + rc
        kp, kv = p / s, cc / s
        y = z[:, c] - mean[:, c]
        mean[:, c] = mean[:, c] + kp * y
        mean[:, 4 + c] = mean[:, 4 + c] + kv * y
        cov[:, 3 * c] = p - (kp * kp) * s
        cov[:, 3 * c + 1] = cc - (kp * kv) * s
        cov[:, 3 * c + 2] = v - (kv * kv) * s


def initiate(z):
    n = len(z)
    mean, cov = np.zeros((n, 8)), np.zeros((n, 12))
    mean[:, :4] = z
    sp, sv = INIT_POS * z[:, 3], INIT_VEL * z[:, 3]
    for c in range(4):
        cov[:, 3 * c] = ASP_INIT * ASP_INIT if c == 2 else sp * sp
        cov[:, 3 * c + 2] = ASP_VEL * ASP_VEL if c == 2 else sv * sv
    return mean, cov


class FullKalman:
    """ByteTrack's KalmanFilter as written there: 8-vector mean, 8 x 8 covariance, Cholesky solve of the projected covariance"""

    def __init__(self):
        self.F = np.eye(8)
        for i in range(4):
            self.F[i, 4 + i] = 1.0
        self.H = np.eye(4, 8)

    def initiate(self, z):
        mean = np.r_[z, np.zeros(4)]
        h = z[3]
        std = [2 * STD_POS * h, 2 * STD_POS * h, 1e-2, 2 * STD_POS * h, 10 * STD_VEL * h, 10 * STD_VEL * h, 1e-5, 10 * STD_VEL * h]
        return mean, np.diag(np.square(std))

    def predict(self, mean, cov):
        h = mean[3]
        std = [STD_POS * h, STD_POS * h, 1e-2, STD_POS * h, STD_VEL * h, STD_VEL * h, 1e-5, STD_VEL * h]
        return self.F @ mean, np.linalg.multi_dot((self.F, cov, self.F.T)) + np.diag(np.square(std))

    def update(self, mean, cov, z):
        h = mean[3]
        std = [STD_POS * h, STD_POS * h, 1e-1, STD_POS * h]
        pm, pc = self.H @ mean, np.linalg.multi_dot((self.H, cov, self.H.T)) + np.diag(np.square(std))
        chol, lower = scipy.linalg.cho_factor(pc, lower=True, check_finite=False)
        gain = scipy.linalg.cho_solve((chol, lower), (cov @ self.H.T).T, check_finite=False).T
        return mean + (z - pm) @ gain.T, cov - np.linalg.multi_dot((gain, pc, gain.T))


def block_to_full(cov12):
    """cov [12] -> the 8 x 8 matrix it stands for"""
    P = np.zeros((8, 8))
    for c in range(4):
        P[c, c], P[c, 4 + c], P[4 + c, c], P[4 + c, 4 + c] = cov12[3 * c], cov12[3 * c + 1], cov12[3 * c + 1], cov12[3 * c + 2]
    return P


# ---- association ---------------------------------------------------------------------------------------------------------------
def _lt(a, b, x, y):
    """a < b ? x : y, element-wise, as the kernel's conditional (a NaN compares false)"""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, x, y)


def iou_matrix(a, b):
    """a [nr, 4], b [nc, 4] double xyxy -> [nr, nc]"""
    a, b = a[:, None, :], b[None, :, :]
    a, b = np.broadcast_arrays(a, b)
    z = np.zeros(a.shape[:2])
    lx, ly = _lt(a[..., 0], b[..., 0], b[..., 0], a[..., 0]), _lt(a[..., 1], b[..., 1], b[..., 1], a[..., 1])
    hx, hy = _lt(a[..., 2], b[..., 2], a[..., 2], b[..., 2]), _lt(a[..., 3], b[..., 3], a[..., 3], b[..., 3])
    pos = lambda x: _lt(z, x, x, z)                                        # noqa: E731   x > 0 ? x : 0
    iw, ih = pos(hx - lx), pos(hy - ly)
    aw, ah, bw, bh = pos(a[..., 2] - a[..., 0]), pos(a[..., 3] - a[..., 1]), pos(b[..., 2] - b[..., 0]), pos(b[..., 3] - b[..., 1])
    inter = iw * ih
    uni = (aw * ah + bw * bh) - inter
    with np.errstate(all="ignore"):
        return _lt(z, uni, inter / uni, z)


def cost_matrix(tab, s, rows, cols, scores, labels, boxes, fuse, class_aware):
    iou = iou_matrix(xyxy(tab["mean"][s, rows]), boxes[cols].astype(np.float64))
    if class_aware:
        iou = np.where(tab["label"][s, rows][:, None] != labels[cols][None, :], 0.0, iou)
    if fuse:
        iou = iou * scores[cols].astype(np.float64)[None, :]
    return (1.0 - iou).astype(np.float32)


def associate(tab, s, rows, cols, det, fuse, thresh, P, frame, slot_of, name):
    """one pass; hits are applied to the table and to slot_of"""
    scores, labels, boxes = det
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if len(rows) == 0 or len(cols) == 0:
        BRANCH["empty_side"] += 1
        return
    cost = cost_matrix(tab, s, rows, cols, scores, labels, boxes, fuse, P["class_aware"])
    BRANCH["rows_gt_cols" if len(rows) > len(cols) else "rows_lt_cols" if len(rows) < len(cols) else "square"] += 1
    if len(rows) + len(cols) > LDS_UNITS:
        BRANCH["lsap_workspace"] += 1
    inside = np.sort(np.where(cost <= F(thresh), cost, np.arange(cost.size, dtype=np.float32).reshape(cost.shape) + F(2)), axis=None)
    if np.any(inside[1:] == inside[:-1]):
        BRANCH["tie"] += 1
    try:
        ri, ci = linear_sum_assignment(cost)
    except ValueError:                                                     # NaN costs: no pair (the kernel's solver reports infeasible)
        return
    keep = cost[ri, ci] <= F(thresh)
    ri, ci = ri[keep], ci[keep]
    if len(ri) == 0:
        return
    t, j = rows[ri], cols[ci]
    BRANCH[name] += len(t)
    BRANCH["refound"] += int((tab["state"][s, t] == LOST).sum())
    mean, cov = tab["mean"][s, t], tab["cov"][s, t]
    correct(mean, cov, measure(boxes[j]))
    tab["mean"][s, t], tab["cov"][s, t] = mean, cov
    tab["state"][s, t] = TRACKED
    tab["last_frame"][s, t] = frame
    tab["score"][s, t] = scores[j]
    tab["label"][s, t] = labels[j]
    slot_of[j] = t


def update_stream(tab, s, scores, labels, boxes, count, P):
    """one frame of stream s: scores [K] f32, labels [K] i32, boxes [K, 4] f32 -> (ids [K] i32, track_boxes [K, 4] f32)"""
    K, T = len(scores), tab["state"].shape[1]
    det = (scores, labels, boxes)
    frame = int(tab["frame"][s]) + 1
    cnt = min(max(int(count), 0), K)
    with np.errstate(invalid="ignore"):
        valid = (np.arange(K) < cnt) & np.isfinite(scores) & np.isfinite(boxes).all(axis=1) & (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])
        BRANCH["invalid_row"] += int(((np.arange(K) < cnt) & ~valid).sum())
        is_hi = valid & (scores > F(P["track_thresh"]))
        is_lo = valid & ~is_hi & (scores > F(P["low_thresh"]))
    hi, lo = np.nonzero(is_hi)[0], np.nonzero(is_lo)[0]
    slot_of = np.full(K, -1, np.int64)
    st = tab["state"][s]
    # 1. predict
    lost = np.nonzero(st == LOST)[0]
    tab["mean"][s, lost, 7] = 0.0
    live = np.nonzero(st != FREE)[0]
    mean, cov = tab["mean"][s, live], tab["cov"][s, live]
    predict(mean, cov)
    tab["mean"][s, live], tab["cov"][s, live] = mean, cov
    # 3. high pass
    associate(tab, s, np.nonzero((st == TRACKED) | (st == LOST))[0], hi, det, P["fuse_score"], P["match_thresh"], P, frame, slot_of, "hits1")
    # 4. low pass
    rows = np.nonzero((st == TRACKED) & (tab["last_frame"][s] != frame))[0]
    associate(tab, s, rows, lo, det, False, P["second_thresh"], P, frame, slot_of, "hits2")
    st[(st == TRACKED) & (tab["last_frame"][s] != frame)] = LOST
    # 5. tentative pass
    left = hi[slot_of[hi] < 0]
    associate(tab, s, np.nonzero(st == TENTATIVE)[0], left, det, P["fuse_score"], P["tentative_thresh"], P, frame, slot_of, "hits3")
    st[st == TENTATIVE] = FREE
    # 6. expiry
    old = (st == LOST) & (frame - tab["last_frame"][s] > P["max_age"])
    BRANCH["expired"] += int(old.sum())
    st[old] = FREE
    # 7. birth
    free = np.nonzero(st == FREE)[0]
    born = left[(slot_of[left] < 0) & (scores[left] >= F(P["new_thresh"]))]
    n = min(len(born), len(free))
    t, j = free[:n], born[:n]
    if n:
        tab["mean"][s, t], tab["cov"][s, t] = initiate(measure(boxes[j]))
        tab["id"][s, t] = tab["next_id"][s] + np.arange(n, dtype=np.int32)
        tab["label"][s, t] = labels[j]
        tab["score"][s, t] = scores[j]
        tab["last_frame"][s, t] = frame
        st[t] = TRACKED if frame == 1 else TENTATIVE
        if frame == 1:
            slot_of[j] = t
    BRANCH["births"] += n
    BRANCH["overflow"] += len(born) - n
    tab["frame"][s] = frame
    tab["next_id"][s] += n
    tab["overflow"][s] += len(born) - n
    ids, tb = np.full(K, -1, np.int32), np.zeros((K, 4), np.float32)
    on = np.nonzero(slot_of >= 0)[0]
    ids[on] = tab["id"][s, slot_of[on]]
    tb[on] = xyxy(tab["mean"][s, slot_of[on]]).astype(np.float32)
    return ids, tb


def update(tab, frame, params=None):
    """frame = (scores [S, K], labels [S, K], boxes [S, K, 4], counts [S]) -> (ids [S, K], track_boxes [S, K, 4])"""
    P = dict(DEFAULTS, **(params or {}))
    scores, labels, boxes, counts = frame
    out = [update_stream(tab, s, scores[s], labels[s], boxes[s], counts[s], P) for s in range(len(counts))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def run(frames, S, T, params=None, tab=None):
    """every frame through `update` -> (table, [(ids, track_boxes, table copy) per frame])"""
    tab = new_table(S, T) if tab is None else tab
    out = []
    for f in frames:
        ids, tb = update(tab, f, params)
        out.append((ids, tb, copy_table(tab)))
    return tab, out


# ---- scenes: lists of frames (scores, labels, boxes, counts) -------------------------------------------------------------------------
def pack(per_stream, K, pad=0.0):
    """per_stream: for every stream a list of (score, label, x1, y1, x2, y2) -> one frame; rows beyond the count hold `pad`"""
    S = len(per_stream)
    scores, boxes = np.full((S, K), pad, np.float32), np.full((S, K, 4), pad, np.float32)
    labels, counts = np.full((S, K), -1, np.int32), np.zeros(S, np.int32)
    for s, rows in enumerate(per_stream):
        assert len(rows) <= K
        counts[s] = len(rows)
        for j, r in enumerate(rows):
            scores[s, j], labels[s, j], boxes[s, j] = r[0], r[1], r[2:6]
    return scores, labels, boxes, counts


def _box(cx, cy, w, h):
    return (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)


def single_object(frames, score=lambda f: 0.9, visible=lambda f: True, extra=lambda f: (), K=4, v=(3.0, 1.0)):
    """one object in linear motion on one stream; score(f) / visible(f) per frame (f = 1 ..), extra(f) more rows"""
    out = []
    for f in range(1, frames + 1):
        rows = [(score(f), 1) + _box(50.0 + v[0] * f, 60.0 + v[1] * f, 30.0, 60.0)] if visible(f) else []
        out.append(pack([rows + list(extra(f))], K))
    return out


def crossing_scene(S=2, K=8, frames=16, seed=7, pad=0.0):
    """per stream: two objects that cross, one that drops out for frames 6..9 and returns, one whose score dips to 0.3 in frames 4..5, a
    one-frame ghost at frame 3, a late arrival at frame 8; rows shuffled per frame"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(1, frames + 1):
        per = []
        for s in range(S):
            o = 7.0 * s
            rows = [(0.92, 1) + _box(40.0 + 6.0 * f + o, 100.0, 30.0, 60.0), (0.88, 2) + _box(150.0 - 6.0 * f + o, 104.0, 32.0, 62.0)]
            if not 6 <= f <= 9:
                rows.append((0.81, 3) + _box(60.0 + 2.0 * f, 220.0 + o, 40.0, 40.0))
            rows.append((0.3 if 4 <= f <= 5 else 0.77, 1) + _box(260.0 + o, 50.0 + 3.0 * f, 24.0, 48.0))
            if f == 3:
                rows.append((0.95, 4) + _box(300.0, 300.0 + o, 20.0, 20.0))
            if f >= 8:
                rows.append((0.7, 2) + _box(20.0 + o, 300.0 - 2.0 * f, 28.0, 50.0))
            rows = [(r[0], r[1]) + tuple(np.float32(x) + np.float32(rng.normal(0, 0.4)) for x in r[2:]) for r in rows]
            per.append([rows[i] for i in rng.permutation(len(rows))])
        out.append(pack(per, K, pad))
    return out


def births_scene(S=3, K=8):
    """two objects at frame 1, then six more at once: T = 4 overflows by four per stream at frame 2 (and again while they stay)"""
    old = [(0.9, 1) + _box(40.0, 40.0, 30.0, 30.0), (0.85, 2) + _box(120.0, 40.0, 30.0, 30.0)]
    new = [(0.8 - 0.01 * i, 3) + _box(30.0 + 45.0 * i, 200.0, 25.0, 25.0) for i in range(6)]
    f1, f2 = pack([old] * S, K), pack([old + new] * S, K)
    return [f1, f2, f2, f1]


def ties_scene(K=8):
    """duplicate boxes with equal scores: equal costs in a row and in a column of the same matrix"""
    a, b = (0.9, 1) + _box(50.0, 50.0, 30.0, 30.0), (0.9, 1) + _box(60.0, 50.0, 30.0, 30.0)
    c = (0.3, 1) + _box(200.0, 50.0, 30.0, 30.0)
    return [pack([[a, b, c]], K), pack([[a, a, b, b, c, c]], K), pack([[b, a, b, a, c]], K), pack([[a, a, a, c, c]], K), pack([[b, b]], K)]


def invalid_rows_scene(K=8):
    """NaN / inf / zero-area / inverted boxes and NaN scores among good rows; padding rows filled with NaN"""
    nan, inf = float("nan"), float("inf")
    good = [(0.9, 1) + _box(50.0, 50.0, 30.0, 30.0), (0.8, 2) + _box(150.0, 60.0, 20.0, 40.0)]
    bad = [(nan, 1) + _box(50.0, 50.0, 30.0, 30.0), (0.9, 1, nan, 10.0, 40.0, 40.0), (0.9, 1, 10.0, 10.0, inf, 40.0),
           (0.9, 1, 10.0, 10.0, 10.0, 40.0), (0.9, 1, 40.0, 10.0, 10.0, 40.0), (inf, 1) + _box(90.0, 90.0, 10.0, 10.0)]
    frames = []
    for f in range(4):
        rows = [(r[0], r[1]) + tuple(x + 2.0 * f for x in r[2:]) for r in good]
        rows = [rows[0], bad[f % 6], rows[1], bad[(f + 3) % 6], bad[(f + 1) % 6]]
        frames.append(pack([rows], K, pad=nan))
    return frames


def random_walk_scene(S=2, K=24, frames=64, n_obj=14, seed=11, p_drop=0.12, p_dip=0.15, p_ghost=0.2, size=(18.0, 60.0), area=400.0, labels=3):
    """n_obj objects per stream on a random walk with dropouts (a few frames long), score dips into the low band and ghosts"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(20.0, area, (S, n_obj, 2))
    vel = rng.normal(0.0, 2.5, (S, n_obj, 2))
    wh = rng.uniform(size[0], size[1], (S, n_obj, 2))
    lab = rng.integers(1, labels + 1, (S, n_obj))
    gone = np.zeros((S, n_obj), np.int64)
    out = []
    for f in range(frames):
        pos += vel + rng.normal(0.0, 0.5, pos.shape)
        vel += rng.normal(0.0, 0.2, vel.shape)
        per = []
        for s in range(S):
            rows = []
            for o in range(n_obj):
                if gone[s, o] > 0:
                    gone[s, o] -= 1
                    continue
                if f > 0 and rng.random() < p_drop:
                    gone[s, o] = rng.integers(1, 6)
                    continue
                sc = rng.uniform(0.15, 0.45) if rng.random() < p_dip else rng.uniform(0.55, 0.98)
                rows.append((sc, int(lab[s, o])) + _box(pos[s, o, 0], pos[s, o, 1], wh[s, o, 0], wh[s, o, 1]))
            if rng.random() < p_ghost:
                rows.append((rng.uniform(0.6, 0.9), 1) + _box(rng.uniform(0, area), rng.uniform(0, area), 20.0, 20.0))
            rows = rows[:K]
            per.append([rows[i] for i in rng.permutation(len(rows))])
        out.append(pack(per, K))
    return out


def large_scene(frames=3, K=1024, n_obj=900, seed=3):
    """a grid of n_obj small objects that jitter, one stream: with T = 512 the table fills at frame 1 (overflow) and the first
    association of frame 2 has 512 + n_obj > LDS_UNITS rows + columns"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(30), np.arange(30))
    c = np.stack([gx.ravel(), gy.ravel()], 1)[:n_obj] * 40.0 + 20.0
    sc = rng.uniform(0.65, 0.95, n_obj)
    out = []
    for f in range(frames):
        p = c + rng.normal(0.0, 1.0, c.shape) + 1.5 * f
        rows = [(sc[i], 1 + i % 3) + _box(p[i, 0], p[i, 1], 24.0, 30.0) for i in range(n_obj)]
        out.append(pack([[rows[i] for i in rng.permutation(n_obj)]], K))
    return out
