"""dod_detect (include/dinodet.h) restated in numpy, and the seeded inputs of tests/test_detect_cpu.py and tests/test_gpu_detect.py.

The restatement follows the header to the letter: candidates (class >= first_class, logit not NaN, threshold < 0 or
sigmoid(logit) > threshold), a stable order on (logit descending, flat index ascending) taken from the logit's BITS, the first K,
boxes and IoU decisions in float32 with one rounding per operation in the stated order, greedy NMS, compaction, padding.

Signed zeros: the order-preserving integer image of a float is `bits | 0x80000000` for a clear sign bit and `~bits` for a set one, so
+0.0 -> 0x80000000 ranks BEFORE -0.0 -> 0x7FFFFFFF, +inf is first and -inf last.  The kernel uses the same image (det_key in
csrc/detect.hip), so both sides agree by construction rather than by how a float comparison treats -0.0 == +0.0.
"""
import numpy as np

from dinov2_od_amd import synth

F = np.float32
SCORE_TOL = 3e-7                      # the project's tolerance for this sigmoid (tests/test_gpu_postprocess.py)
THRESHOLDS = (0.05, 0.5, 0.9)         # the score thresholds the tests use: logits are kept 1e-4 clear of every one of them


def key_image(x):
    """float32 array -> uint32: a larger logit has a larger key"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def sigmoid32(x):
    """1 / (1 + expf(-x)) in float32"""
    with np.errstate(over="ignore"):
        return (F(1.0) / (F(1.0) + np.exp(-np.asarray(x, dtype=np.float32)))).astype(np.float32)


def _clamp(v, hi):
    return np.where(v < F(0.0), F(0.0), np.where(v > hi, hi, v)).astype(np.float32)


def _min(a, b):
    return np.where(a < b, a, b).astype(np.float32)


def _max(a, b):
    return np.where(a > b, a, b).astype(np.float32)


def size_rows(sizes, B):
    """None / one (h, w) / B pairs -> float32 [B, 2] of (height, width); None = 1 x 1"""
    if sizes is None:
        return np.ones((B, 2), np.float32)
    s = np.asarray(sizes, dtype=np.float32)
    return np.broadcast_to(s.reshape(-1, 2), (B, 2)).copy()


def select(logits_flat, C, K, first_class, threshold, row_ok=None):
    """flat indices r*C + c of the first K candidates of one image, in order (r = q for dod_detect, v*Q + q for dod_detect_views);
    row_ok [rows]: None or the edge filter's verdict on every row"""
    x = np.ascontiguousarray(logits_flat, dtype=np.float32)
    idx = np.arange(x.size)
    cand = (idx % C >= first_class) & ~np.isnan(x)
    if row_ok is not None:
        cand &= row_ok[idx // C]
    if not threshold < 0:
        cand &= sigmoid32(x) > F(threshold)
    ci = idx[cand]
    order = np.lexsort((ci, ~key_image(x[ci])))            # last key is primary: key descending, then index ascending
    return ci[order[:K]]


def boxes_of(rows, hw, clamp):
    """rows [n, 4] cxcywh float32 -> xyxy float32 scaled by hw = (height, width)"""
    cx, cy, w, h = (rows[:, i].astype(np.float32) for i in range(4))
    ih, iw = F(hw[0]), F(hw[1])
    half = F(0.5)
    x1, y1, x2, y2 = cx - half * w, cy - half * h, cx + half * w, cy + half * h
    x1, y1, x2, y2 = x1 * iw, y1 * ih, x2 * iw, y2 * ih
    if clamp:
        x1, y1, x2, y2 = _clamp(x1, iw), _clamp(y1, ih), _clamp(x2, iw), _clamp(y2, ih)
    return np.stack([x1, y1, x2, y2], axis=1).astype(np.float32)


def nms_keep(boxes, labels, iou, class_agnostic, metric=0):
    """greedy NMS over boxes in their order -> boolean keep mask; metric 0 = IoU, 1 = intersection over the smaller box (the nms_metric
    codes of dod_detect_views)"""
    n = len(boxes)
    keep = np.ones(n, bool)
    z = F(0.0)
    area = (_max(z, boxes[:, 2] - boxes[:, 0]) * _max(z, boxes[:, 3] - boxes[:, 1])).astype(np.float32)
    for i in range(n):
        if not keep[i]:
            continue
        r = boxes[i + 1:]
        iw = _max(z, _min(boxes[i, 2], r[:, 2]) - _max(boxes[i, 0], r[:, 0]))
        ih = _max(z, _min(boxes[i, 3], r[:, 3]) - _max(boxes[i, 1], r[:, 1]))
        inter = (iw * ih).astype(np.float32)
        if metric == 0:
            ref = ((area[i] + area[i + 1:]).astype(np.float32) - inter).astype(np.float32)
        else:
            assert metric == 1
            ref = _min(np.full(n - i - 1, area[i], np.float32), area[i + 1:])
        sup = inter > (F(iou) * ref).astype(np.float32)
        if not class_agnostic:
            sup &= labels[i + 1:] == labels[i]
        keep[i + 1:] &= ~sup
    return keep


def detect_ref(det, C, K, first_class=1, sizes=None, threshold=-1.0, iou=None, class_agnostic=False, clamp=True):
    """the whole call: {"scores" [B,K] f32, "labels", "queries" [B,K] i32, "boxes" [B,K,4] f32, "counts" [B] i32, "selected" [B]}
    (selected = candidates taken before NMS)"""
    det = np.ascontiguousarray(det, dtype=np.float32)
    B, Q, _ = det.shape
    hw = size_rows(sizes, B)
    out = {"scores": np.zeros((B, K), np.float32), "labels": np.full((B, K), -1, np.int32), "queries": np.full((B, K), -1, np.int32),
           "boxes": np.zeros((B, K, 4), np.float32), "counts": np.zeros(B, np.int32), "selected": np.zeros(B, np.int32)}
    for b in range(B):
        logits = det[b, :, :C].reshape(-1)
        sel = select(logits, C, K, first_class, threshold)
        q, lab = sel // C, sel % C
        bx = boxes_of(det[b, q, C:], hw[b], clamp)
        sc = sigmoid32(logits[sel])
        out["selected"][b] = len(sel)
        if iou is not None:
            keep = nms_keep(bx, lab, iou, class_agnostic)
            q, lab, bx, sc = q[keep], lab[keep], bx[keep], sc[keep]
        n = len(q)
        out["counts"][b] = n
        out["scores"][b, :n], out["labels"][b, :n], out["queries"][b, :n], out["boxes"][b, :n] = sc, lab, q, bx
    return out


# ------------------------------------------------------------------------------------------------ inputs
def safe_logits(seed, shape, mean, std):
    """normal logits whose scores keep 1e-4 clear of every threshold in THRESHOLDS: the keep decision must not hinge on an ulp of expf"""
    x = (synth.normal(seed, f"det.{shape}", shape, std) + mean).astype(np.float32)
    for _ in range(4):
        s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        near = np.zeros(x.shape, bool)
        for t in THRESHOLDS:
            near |= np.abs(s - t) < 1e-4
        if not near.any():
            break
        x[near] -= F(0.05)
    return x


def rand_boxes(seed, B, Q):
    """cxcywh: some boxes reach outside the unit image, some have zero or negative width / height"""
    u = synth.uniform01(seed, f"det.boxes.{B}.{Q}", (B, Q, 4)).astype(np.float32)
    bx = np.empty_like(u)
    bx[..., :2] = u[..., :2] * F(1.2) - F(0.1)
    bx[..., 2:] = u[..., 2:] * F(0.6) - F(0.05)
    bx[:, ::7, 2] = 0.0                                   # exactly zero width
    return bx


def pack(logits, boxes):
    return np.ascontiguousarray(np.concatenate([logits, boxes], axis=-1), dtype=np.float32)


def random_det(seed, B, Q, C, mean=-3.0, std=1.5):
    return pack(safe_logits(seed, (B, Q, C), mean, std), rand_boxes(seed + 1, B, Q))


def distinct_det(seed, B, Q, C):
    """every logit of an image distinct (a permutation of an evenly spaced ladder): top-k has one answer whatever breaks ties"""
    N = Q * C
    lg = np.empty((B, N), np.float32)
    for b in range(B):
        perm = np.argsort(synth.uniform01(seed, f"det.perm.{b}.{N}", (N,)), kind="stable")
        lg[b] = (-8.0 + 12.0 * perm / N).astype(np.float32)
        assert len(np.unique(lg[b])) == N
    return pack(lg.reshape(B, Q, C), rand_boxes(seed + 1, B, Q))


def quantised_det(seed, B, Q, C, levels=8):
    """logits on `levels` distinct values: ties straddle the K-th position whatever K is"""
    u = synth.uniform01(seed, f"det.q.{B}.{Q}.{C}", (B, Q, C))
    lg = (np.floor(u * levels) * 0.75 - 3.0).astype(np.float32)
    return pack(lg, rand_boxes(seed + 1, B, Q))


def special_det(seed, B, Q, C):
    """NaN, +-inf, +-0.0 and saturating logits scattered into normal ones"""
    lg = safe_logits(seed, (B, Q, C), -1.0, 2.0).reshape(-1)
    pick = synth.uniform01(seed, f"det.special.{B}.{Q}.{C}", lg.shape)
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0, 40.0, -40.0, -np.nan]
    for k, v in enumerate(vals):
        lg[(pick >= 0.03 * k) & (pick < 0.03 * (k + 1))] = v
    return pack(lg.reshape(B, Q, C), rand_boxes(seed + 1, B, Q))


NMS_CASES = [(K, iou, agn) for K in (4, 100, 300, 512) for iou in (0.0, 0.5, 0.7) for agn in (False, True)]
NMS_SIZES = [(480.0, 640.0), (333.0, 500.0)]


def clustered_det(K, seed=40, B=2, C=5, centres=4):
    """Q = K + 24 queries per image.  Every second query sits on one of `centres` cluster centres (a box of about 0.1 x 0.1) with a
    jitter of 0.012, so that cluster members overlap at IoU around 0.5 - 0.9 and mostly share their centre's class; the others are small
    scattered boxes that seldom overlap anything.  One class per query carries a high logit, falling with the query index, so the top K
    are roughly the first K queries whatever K is.  tests/test_detect_cpu.py checks that the
    reference suppresses between 20 % and 80 % of the selected candidates for every entry of NMS_CASES."""
    Q = K + 24
    u = synth.uniform01(seed, f"det.cl.{K}.{B}", (B, Q, 8)).astype(np.float32)
    cen = synth.uniform01(seed + 1, f"det.cen.{K}.{B}", (B, centres, 2)).astype(np.float32) * F(0.7) + F(0.15)
    which = (np.arange(Q) // 4) % centres
    clustered = (np.arange(Q) % 2 == 0)
    bx = np.empty((B, Q, 4), np.float32)
    bx[..., :2] = u[..., :2]
    bx[..., 2:] = F(0.01) + F(0.03) * u[..., 2:4]
    jit = (u[..., 4:8] - F(0.5)) * F(0.024)
    jit[:, :8] *= F(0.1)                                  # the first members agree closely: K = 4 sees a suppression at every IoU
    for b in range(B):
        bx[b, clustered, :2] = cen[b, which[clustered]] + jit[b, clustered, :2]
        bx[b, clustered, 2:] = F(0.1) + jit[b, clustered, 2:]
    lg = safe_logits(seed + 2, (B, Q, C), -7.0, 0.5)
    hot = synth.uniform01(seed + 3, f"det.hot.{K}.{B}", (B, Q, 2))
    for b in range(B):
        for q in range(Q):
            own = clustered[q] and (q < 8 or hot[b, q, 0] < 0.75)
            c = 1 + which[q] % (C - 1) if own else 1 + int(hot[b, q, 0] * 997) % (C - 1)
            lg[b, q, c] = F(4.0 - 3.0 * q / Q + (0.0 if q < 8 else 0.2 * (hot[b, q, 1] - 0.5)))      # roughly in query order
    return pack(lg, bx)
