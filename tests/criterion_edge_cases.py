"""What the per-element tests of the set criterion (csrc/criterion.hip) and of the matcher's cost kernel (csrc/matchcost.hip) share:
the edge-case inputs, a float64 reference of every output element, and the bound each fp32 element is held to.  Plain numpy on the CPU.

Reference.  The focal term is written stably in float64 (1 - p_t as sigmoid(-+x), BCE as max(x, 0) - x t + log1p(exp(-|x|))); the box
terms are the kernel's own statement order in float64 with torch autograd's tie rules written out.  None of it goes through
losses.composite_losses: tests/test_criterion_edges_cpu.py pins it to float64 autograd of the composite where that is well conditioned.

Bounds ("Per-element bounds of the criterion"; u = 2^-24).  Worst cases of the roundings, none measured:
  loss element   |l - l64| <= K_LOSS u (|l64| + [pos] |a_t| gamma w^(gamma-1) bce) + K_LOSS 2^-126
  logit gradient |g - g64| <= |s| K_GRAD u (|g64| + S) + K_GRAD 2^-126 max(|s|, 1),   s the upstream factor,
                 S = |a_t| (gamma^2 w^(gamma-1) (1-w) bce + gamma w^gamma bce + (gamma+1) w^gamma) for a positive,
                     |1-alpha| gamma p^gamma bce for a negative
  box terms      the running error of the kernel's statements (class Run): every rounded operation adds u |result| + 2^-126 to what its
                 operands carry, an operation whose exact result is an fp32 number on error-free operands adds nothing (the dyadic grid
                 stays exact up to the first division), a max / min / clamp / sign must be decided beyond the carried error or tie exactly
  summed losses  (sum of the element bounds + n u sum|terms|) / max(num_boxes, 1), n = number of terms + 1
The same running error bounds every entry of the cost matrix, with expf / logf / powf taken as 1 ulp (ASSUMED, as for K_LOSS / K_GRAD)."""
import numpy as np

from dinov2_od_amd import synth

U = 2.0 ** -24
FLOOR = 2.0 ** -126
ULP_FN = 2 * U                  # ASSUMED: expf, log1pf, logf, powf within 1 ulp, i.e. 2u relative
K_LOSS, K_GRAD = 22.0, 30.0     # operation counts for gamma <= 3: DESIGN.md section 6b

LADDER = np.array([0.0] + [s * v for v in (2.0 ** -20, 0.5, 1, 4, 8, 12, 16, 16.7, 17, 20, 30, 87, 88.8, 100) for s in (1, -1)], np.float32)
GAMMAS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
ALPHAS = (0.25, 0.4, 0.0, 1.0, -1.0)
NUM_BOXES = (None, 0.0, 0.5, 1.0, 2.5, 37.0)
GEOM_C = (1, 63, 64, 65, 129)
GEOM_R = (1, 3, 4, 5, 15, 16, 17, 33)


# ------------------------------------------------------------------------------------------------ running error
def _f32_exact(v):
    with np.errstate(over="ignore"):
        return v.astype(np.float32).astype(np.float64) == v


class Run:
    """float64 values with a bound on |fp32 evaluation - value|, carried through the kernel's statements"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def lift(x):
        return x if isinstance(x, Run) else Run(x)

    @staticmethod
    def rounded(v, e, rel=U):
        """the result of one rounded operation whose operands carry e"""
        return Run(v, np.where((e == 0) & _f32_exact(v), 0.0, e + rel * np.abs(v) + FLOOR))

    def __neg__(self):
        return Run(-self.v, self.e)

    def __add__(self, o):
        o = Run.lift(o)
        return Run.rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Run.lift(o)
        return Run.rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Run.lift(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = Run.lift(o)
        return Run.rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Run.lift(o)
        v = self.v / o.v
        den = np.abs(o.v) - o.e
        e = np.where(den > 0, (self.e + np.abs(v) * o.e) / np.where(den > 0, den, 1.0), np.inf)
        return Run.rounded(v, np.where((self.e == 0) & (o.e == 0), 0.0, e))

    def __rtruediv__(self, o):
        return Run.lift(o) / self


class RunArith:
    """the operations the statements below are written in, on Run values; `undecided` collects every comparison that the carried error
    could turn (an exact tie of error-free operands is decided: it is the same tie in fp32)"""

    def __init__(self):
        self.undecided = False

    def num(self, x):
        return Run(np.asarray(x, np.float64))

    def _decide(self, a, b):
        tie = (a.v == b.v) & (a.e == 0) & (b.e == 0)
        self.undecided = self.undecided | bool(np.any((np.abs(a.v - b.v) <= a.e + b.e) & ~tie))

    def scale(self, a, k):                      # k: exact factors (0, 0.5, 1, -1)
        return Run(a.v * k, a.e * np.abs(k))

    def mx(self, a, b):
        self._decide(a, b)
        return Run(np.maximum(a.v, b.v), np.where(a.v > b.v, a.e, np.where(a.v < b.v, b.e, np.maximum(a.e, b.e))))

    def mn(self, a, b):
        self._decide(a, b)
        return Run(np.minimum(a.v, b.v), np.where(a.v < b.v, a.e, np.where(a.v > b.v, b.e, np.maximum(a.e, b.e))))

    def max_share(self, a, b):
        return np.where(a.v > b.v, 1.0, np.where(a.v == b.v, 0.5, 0.0))

    def min_share(self, a, b):
        return np.where(a.v < b.v, 1.0, np.where(a.v == b.v, 0.5, 0.0))

    def ge0(self, a):
        self._decide(a, Run(np.zeros_like(a.v)))
        return a.v >= 0

    def clamp0(self, a):
        keep = self.ge0(a)
        return Run(np.where(keep, a.v, 0.0), np.where(keep, a.e, 0.0))

    def sign(self, a):
        self._decide(a, Run(np.zeros_like(a.v)))
        return np.sign(a.v)

    def abs(self, a):
        return Run(np.abs(a.v), a.e)

    def exp(self, a):
        v = np.exp(a.v)
        return Run.rounded(v, v * np.expm1(a.e), ULP_FN)

    def log(self, a, lo):
        """logf of an fp32 argument known to be >= lo > 0"""
        v = np.log(a.v)
        e = np.maximum(np.log(a.v + a.e) - v, v - np.log(np.maximum(a.v - a.e, lo)))
        return Run.rounded(v, e, ULP_FN)

    def pow(self, a, g):
        v = a.v ** g
        e = np.maximum(np.abs((a.v + a.e) ** g - v), np.abs(np.maximum(a.v - a.e, 0.0) ** g - v))
        return Run.rounded(v, e, ULP_FN)


class F32Arith:
    """the same operations in numpy float32: the restatement of the kernels that the CPU test holds to the bounds"""
    undecided = False

    def num(self, x):
        return np.asarray(x, np.float32)

    def scale(self, a, k):
        return a * np.asarray(k, np.float32)

    def mx(self, a, b):
        return np.maximum(a, b)

    def mn(self, a, b):
        return np.minimum(a, b)

    def max_share(self, a, b):
        return np.where(a > b, 1.0, np.where(a == b, 0.5, 0.0)).astype(np.float32)

    def min_share(self, a, b):
        return np.where(a < b, 1.0, np.where(a == b, 0.5, 0.0)).astype(np.float32)

    def ge0(self, a):
        return a >= 0

    def clamp0(self, a):
        return np.maximum(a, np.float32(0))

    def sign(self, a):
        return np.sign(a).astype(np.float32)

    def abs(self, a):
        return np.abs(a)

    def exp(self, a):
        with np.errstate(over="ignore", under="ignore"):
            return np.exp(a)

    def log(self, a, lo):
        return np.log(a)

    def pow(self, a, g):
        return np.power(a, np.float32(g))


def _giou_state(p, t, ar):
    """giou_pair of criterion.hip / the GIoU lines of matchcost.hip: p, t = four components each"""
    s = {}
    h = lambda a: ar.scale(a, 0.5)
    s["ax1"], s["ay1"], s["ax2"], s["ay2"] = p[0] - h(p[2]), p[1] - h(p[3]), p[0] + h(p[2]), p[1] + h(p[3])
    s["bx1"], s["by1"], s["bx2"], s["by2"] = t[0] - h(t[2]), t[1] - h(t[3]), t[0] + h(t[2]), t[1] + h(t[3])
    s["aw"], s["ah"] = s["ax2"] - s["ax1"], s["ay2"] - s["ay1"]
    area1, area2 = s["aw"] * s["ah"], (s["bx2"] - s["bx1"]) * (s["by2"] - s["by1"])
    s["iwr"] = ar.mn(s["ax2"], s["bx2"]) - ar.mx(s["ax1"], s["bx1"])
    s["ihr"] = ar.mn(s["ay2"], s["by2"]) - ar.mx(s["ay1"], s["by1"])
    s["iw"], s["ih"] = ar.clamp0(s["iwr"]), ar.clamp0(s["ihr"])
    s["inter"] = s["iw"] * s["ih"]
    s["uni"] = area1 + area2 - s["inter"]
    s["ewr"] = ar.mx(s["ax2"], s["bx2"]) - ar.mn(s["ax1"], s["bx1"])
    s["ehr"] = ar.mx(s["ay2"], s["by2"]) - ar.mn(s["ay1"], s["by1"])
    s["ew"], s["eh"] = ar.clamp0(s["ewr"]), ar.clamp0(s["ehr"])
    s["earea"] = s["ew"] * s["eh"]
    s["giou"] = s["inter"] / s["uni"] - (s["earea"] - s["uni"]) / s["earea"]
    return s


def _l1(p, t, ar):
    return ((ar.abs(p[0] - t[0]) + ar.abs(p[1] - t[1])) + ar.abs(p[2] - t[2])) + ar.abs(p[3] - t[3])


def box_statements(pred, tgt, gb, gg, ar):
    """The matched pair's statements of crit_forward_kernel / crit_backward_kernel, [K, 4] boxes: the L1 term, 1 - giou, and
    d(loss) / d(cx, cy, w, h) for gb = d_losses[1] / nb and gg = -(d_losses[2] / nb), with torch autograd's tie rules: half of the
    gradient to each side of an equal maximum / minimum, clamp(min=0) passes at 0, sign(0) = 0."""
    p = [ar.num(pred[:, i]) for i in range(4)]
    t = [ar.num(tgt[:, i]) for i in range(4)]
    s = _giou_state(p, t, ar)
    l1, lg = _l1(p, t, ar), 1.0 - s["giou"]
    g = gg
    N = s["earea"] - s["uni"]
    gT = -g
    gN = gT / s["earea"]
    gE = (-gT) * N / (s["earea"] * s["earea"]) + gN
    gU = -gN - g * s["inter"] / (s["uni"] * s["uni"])
    gI = g / s["uni"] - gU
    mask = lambda raw: np.where(ar.ge0(raw), 1.0, 0.0)
    giw, gih = ar.scale(gI * s["ih"], mask(s["iwr"])), ar.scale(gI * s["iw"], mask(s["ihr"]))
    gew, geh = ar.scale(gE * s["eh"], mask(s["ewr"])), ar.scale(gE * s["ew"], mask(s["ehr"]))
    gdx, gdy = gU * s["ah"], gU * s["aw"]
    sc = ar.scale
    gx2 = gdx + sc(giw, ar.min_share(s["ax2"], s["bx2"])) + sc(gew, ar.max_share(s["ax2"], s["bx2"]))
    gx1 = -gdx - sc(giw, ar.max_share(s["ax1"], s["bx1"])) - sc(gew, ar.min_share(s["ax1"], s["bx1"]))
    gy2 = gdy + sc(gih, ar.min_share(s["ay2"], s["by2"])) + sc(geh, ar.max_share(s["ay2"], s["by2"]))
    gy1 = -gdy - sc(gih, ar.max_share(s["ay1"], s["by1"])) - sc(geh, ar.min_share(s["ay1"], s["by1"]))
    d = [gx1 + gx2, gy1 + gy2, sc(gx2 - gx1, 0.5), sc(gy2 - gy1, 0.5)]
    d = [d[i] + sc(gb, ar.sign(p[i] - t[i])) for i in range(4)]
    return l1, lg, d


def cost_statements(x, pred, tgt, w_class, w_bbox, w_giou, alpha, gamma, ar):
    """match_cost_kernel's entry for logit x [K] (of the target's label column), boxes [K, 4]: the kernel's own formula, the 1e-8 inside
    the logs included"""
    f = lambda c: float(np.float32(c))
    eps = f(1e-8)
    xx = ar.num(x)
    pr = 1.0 / (1.0 + ar.exp(-xx))
    q = 1.0 - pr
    pg, qg = (pr * pr, q * q) if gamma == 2.0 else (ar.pow(pr, f(gamma)), ar.pow(q, f(gamma)))
    one_minus_alpha = ar.num(1.0) - ar.num(f(alpha))
    neg = one_minus_alpha * pg * (-ar.log(q + eps, eps))
    pos = f(alpha) * qg * (-ar.log(pr + eps, eps))
    cc = pos - neg
    p = [ar.num(pred[:, i]) for i in range(4)]
    t = [ar.num(tgt[:, i]) for i in range(4)]
    cb = _l1(p, t, ar)
    giou = _giou_state(p, t, ar)["giou"]
    return f(w_class) * cc + f(w_bbox) * cb + f(w_giou) * (-giou)


# ------------------------------------------------------------------------------------------------ focal term
def focal64(x, pos, alpha, gamma):
    """float64: the loss element, its x-derivative and the two sensitivities of the bounds.  alpha / gamma as the fp32 the kernel gets."""
    x = np.asarray(x, np.float64)
    a, g = float(np.float32(alpha)), float(np.float32(gamma))
    with np.errstate(over="ignore"):
        en = np.exp(-np.abs(x))
    big, small = 1.0 / (1.0 + en), en / (1.0 + en)
    p, q = np.where(x >= 0, big, small), np.where(x >= 0, small, big)          # sigmoid(x), sigmoid(-x)
    w = np.where(pos, q, p)                                                    # 1 - p_t
    at = np.where(pos, a, 1.0 - a)
    bce = np.maximum(x, 0.0) - x * pos + np.log1p(en)
    wg = w ** g if g != 0 else np.ones_like(w)
    wg1 = w ** (g - 1.0) if g != 0 else np.zeros_like(w)                       # only ever multiplied by gamma
    sgn = np.where(pos, -1.0, 1.0)                                             # d(1 - p_t)/dx = sgn p (1 - p);  p - t = sgn (1 - p_t) ... for a positive -q
    loss = at * wg * bce
    grad = at * (g * wg1 * sgn * p * q * bce + wg * np.where(pos, -q, p))
    s_loss = np.where(pos, np.abs(at) * g * wg1 * bce, 0.0)
    s_grad = np.where(pos, np.abs(at) * (g * g * wg1 * (1.0 - w) * bce + g * wg * bce + (g + 1.0) * wg), np.abs(1.0 - a) * g * p ** g * bce)
    return loss, grad, s_loss, s_grad


def focal32(x, pos, alpha, gamma):
    """focal_elem / focal_grad of criterion.hip, statement by statement in numpy float32"""
    f = np.float32
    x, one, a, g = np.asarray(x, f), f(1), f(alpha), f(gamma)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        p = one / (one + np.exp(-x))
        t = pos.astype(f)
        w = np.where(pos, one - p, p)
        at = np.where(pos, a, one - a)
        bce = np.maximum(x, f(0)) - x * t + np.log1p(np.exp(-np.abs(x)))
        pw = w * w if g == 2 else np.power(w, g)
        loss = at * pw * bce
        wg1 = w if g == 2 else np.power(w, g - one)
        dpow = np.where((g != 0) & (w != 0), g * wg1 * (-(f(2) * t - one) * p * (one - p)) * bce, f(0)).astype(f)
        grad = at * (dpow + pw * (p - t))
    return loss.astype(f), grad.astype(f)


# ------------------------------------------------------------------------------------------------ the whole criterion, one layer
def _targets(R, C, labels, G, match):
    m = np.asarray(match, np.int64).reshape(R)
    valid = (m >= 0) & (m < G)
    lab = np.full(R, -1, np.int64)
    if G:
        lab[valid] = np.asarray(labels, np.int64)[m[valid]]
    tc = np.where((lab >= 0) & (lab < C), lab, -1)
    pos = tc[:, None] == np.arange(C)[None, :]
    return m, valid, pos


def _norm(nb):
    return 1.0 if nb is None else max(float(np.float32(nb)), 1.0)


def reference(logits, boxes, labels, gt, match, nb, alpha, gamma, d_losses=None, d_elem=None):
    """One layer in float64 with the bound of every element.  logits fp32 [R, C], boxes fp32 [R, 4] or None, labels int64 [G], gt fp32 [G, 4],
    match int [R] (global target rows; the identity for the kernel's match == NULL), nb a number or None, d_losses [3] / d_elem [R, C] the
    upstream gradients (either may be None).  -> dict of arrays `name` and `name + "_bound"`, and `undecided` (must be False)."""
    R, C = logits.shape
    G = len(labels)
    m, valid, pos = _targets(R, C, labels, G, match)
    n = _norm(nb)
    loss, grad, s_loss, s_grad = focal64(logits, pos, alpha, gamma)
    out = {"elem": loss, "elem_bound": K_LOSS * U * (np.abs(loss) + s_loss) + K_LOSS * FLOOR, "undecided": False}
    sums, sum_bounds = [loss.sum()], [out["elem_bound"].sum() + (loss.size + 1) * U * np.abs(loss).sum()]
    if d_elem is not None:
        s = np.asarray(d_elem, np.float64).reshape(R, C)
    elif d_losses is not None:
        s = np.full((R, C), float(np.float32(d_losses[0])) / n)
    else:
        s = None
    if s is not None:
        out["d_logits"] = s * grad
        out["d_logits_bound"] = np.abs(s) * K_GRAD * U * (np.abs(grad) + s_grad) + K_GRAD * FLOOR * np.maximum(np.abs(s), 1.0)
    if boxes is not None:
        ar = RunArith()
        k = int(valid.sum())
        d1, d2 = (0.0, 0.0) if d_losses is None else (float(np.float32(d_losses[1])), float(np.float32(d_losses[2])))
        gb, gg = Run.rounded(np.full(k, d1 / n), 0.0), -Run.rounded(np.full(k, d2 / n), 0.0)
        l1, lg, d = box_statements(np.asarray(boxes, np.float64)[valid], np.asarray(gt, np.float64).reshape(-1, 4)[m[valid]], gb, gg, ar)
        out["undecided"] = ar.undecided
        for term in (l1, lg):
            sums.append(term.v.sum())
            sum_bounds.append(term.e.sum() + (k + 1) * U * np.abs(term.v).sum())
        if d_losses is not None:
            out["d_boxes"], out["d_boxes_bound"] = np.zeros((R, 4)), np.zeros((R, 4))             # unmatched rows: exactly +0.0
            out["d_boxes"][valid] = np.stack([c.v for c in d], 1)
            out["d_boxes_bound"][valid] = np.stack([c.e for c in d], 1) + FLOOR
    else:
        sums += [0.0, 0.0]
        sum_bounds += [0.0, 0.0]
    out["losses"] = np.array(sums) / n
    out["losses_bound"] = np.array(sum_bounds) / n + FLOOR
    return out


def restate32(logits, boxes, labels, gt, match, nb, alpha, gamma, d_losses=None, d_elem=None):
    """the kernels' statements in numpy float32 (sums in numpy's order: any order is inside the bound), same arguments as `reference`"""
    f = np.float32
    R, C = logits.shape
    G = len(labels)
    m, valid, pos = _targets(R, C, labels, G, match)
    n = f(_norm(nb))
    loss, grad = focal32(logits, pos, alpha, gamma)
    out = {"elem": loss}
    sums = [loss.sum(dtype=f)]
    if d_elem is not None:
        out["d_logits"] = np.asarray(d_elem, f).reshape(R, C) * grad
    elif d_losses is not None:
        out["d_logits"] = (f(d_losses[0]) / n) * grad
    if boxes is not None:
        k = int(valid.sum())
        d1, d2 = (f(0), f(0)) if d_losses is None else (f(d_losses[1]), f(d_losses[2]))
        with np.errstate(all="ignore"):
            l1, lg, d = box_statements(np.asarray(boxes, f)[valid], np.asarray(gt, f).reshape(-1, 4)[m[valid]], np.full(k, d1 / n, f),
                                       -np.full(k, d2 / n, f), F32Arith())
        sums += [l1.sum(dtype=f), lg.sum(dtype=f)]
        if d_losses is not None:
            out["d_boxes"] = np.zeros((R, 4), f)
            out["d_boxes"][valid] = np.stack(d, 1)
    else:
        sums += [f(0), f(0)]
    out["losses"] = np.array(sums, f) / n
    return out


OUTPUTS = ("losses", "elem", "d_logits", "d_boxes")


def ratios(got, ref):
    """name -> worst |got - ref| / bound over the outputs both hold (an element with a zero bound must be equal: inf otherwise);
    a NaN anywhere in `got` gives inf"""
    out = {}
    for k in OUTPUTS:
        if k in got and k in ref and got[k] is not None:
            g, w, b = np.asarray(got[k], np.float64), ref[k], ref[k + "_bound"]
            assert g.shape == w.shape, (k, g.shape, w.shape)
            err = np.abs(g - w)
            r = np.where(err == 0, 0.0, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.inf))
            r = np.where(np.isfinite(g), r, np.inf)
            out[k] = float(r.max()) if r.size else 0.0
    return out


def check(got, ref, what, worst=None):
    """every element of every output inside its bound, zero excluded; unmatched rows of d_boxes exactly +0.0.  `worst` (a dict) keeps
    the largest ratio per output across calls."""
    assert not ref["undecided"], f"{what}: a box comparison of the reference is not decided beyond the carried rounding error"
    for k in OUTPUTS:
        if k in ref:
            assert np.isfinite(ref[k]).all() and np.isfinite(ref[k + "_bound"]).all(), f"{what}: {k} has a non-finite reference or bound"
    r = ratios(got, ref)
    if worst is not None:
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound {bad}"
    if "d_boxes" in r:
        g = np.asarray(got["d_boxes"])
        zero = ref["d_boxes_bound"] == 0
        assert not np.signbit(g[zero]).any() and (g[zero] == 0).all(), f"{what}: d_boxes of an unmatched row is not +0.0"
    return r


def composite(a, dtype, device="cpu"):
    """losses [3], d_logits, d_boxes of losses.composite_losses + autograd for one layer's `reference` arguments (d_losses path): float64
    pins the reference, fp32 is the yardstick printed beside the kernel"""
    import torch
    from dinov2_od_amd import losses as L
    lg = torch.from_numpy(a["logits"]).to(device, dtype).requires_grad_(True)
    bx = torch.from_numpy(a["boxes"]).to(device, dtype).requires_grad_(True)
    nb = torch.tensor([1.0 if a["nb"] is None else a["nb"]], dtype=dtype, device=device)
    out = L.composite_losses(lg[None], bx[None], torch.from_numpy(a["labels"]).to(device), torch.from_numpy(a["gt"]).to(device, dtype),
                             torch.from_numpy(a["match"]).to(device), nb, float(np.float32(a["alpha"])), a["gamma"])
    (out * torch.from_numpy(np.asarray(a["d_losses"])).to(device, dtype)).sum().backward()
    return {"losses": out.detach().cpu().numpy(), "d_logits": lg.grad.cpu().numpy(), "d_boxes": bx.grad.cpu().numpy()}


def has_yardstick(a):
    return a["boxes"] is not None and a["d_elem"] is None and a["d_losses"] is not None and a["gamma"] > 0


def fmt(worst):
    return " ".join(f"{k} {v:.3f}" for k, v in worst.items())


# ------------------------------------------------------------------------------------------------ inputs
def _boxes(seed, key, n):
    cxcy = 0.15 + 0.7 * synth.uniform01(seed, key + ".cxcy", (n, 2))
    wh = 0.05 + 0.4 * synth.uniform01(seed, key + ".wh", (n, 2))
    return np.concatenate([cxcy, wh], 1).astype(np.float32)


def ladder_case(C=32):
    """29 matched rows: row i's target column i % C holds LADDER[i], column j the value LADDER[(i + j) % 29], so every value is a positive
    once and a background entry C - 1 times; 3 unmatched rows behind them"""
    n = len(LADDER)
    R = n + 3
    idx = (np.arange(R)[:, None] + np.arange(C)[None, :]) % n
    logits = LADDER[idx]
    labels = (np.arange(n) % C).astype(np.int64)
    for i in range(n):
        logits[i, labels[i]] = LADDER[i]
    match = np.full(R, -1, np.int32)
    match[:n] = np.arange(n)
    return dict(logits=logits, boxes=_boxes(71, "ladder.pred", R), labels=labels, gt=_boxes(71, "ladder.gt", n), match=match)


def geometry_case(C, R):
    """N(0, 2) logits with a few saturated entries; matched rows on the first and last row of a wave, the last row overall and the first
    row of the last (partial) workgroup; two targets"""
    logits = synth.normal(73, f"geom.{C}.{R}", (R, C), 2.0).astype(np.float32)
    logits[R // 2, C // 2] = 18.0
    logits[0, C - 1] = -30.0
    rows = sorted({0, 3, R - 1, 16 * ((R - 1) // 16)} & set(range(R)))
    labels = np.array([C - 1, C // 3], np.int64)
    match = np.full(R, -1, np.int32)
    for k, r in enumerate(rows):
        match[r] = k % 2
    logits[R - 1, labels[match[R - 1]]] = 17.0                    # a saturated positive on the last row
    return dict(logits=logits, boxes=_boxes(73, f"geom.pred.{R}", R), labels=labels, gt=_boxes(73, "geom.gt", 2), match=match)


GRID_GT = np.array([0.375, 0.375, 0.25, 0.25], np.float32)       # [0.25, 0.5]^2
GRID_INTERVALS = [(lo, hi) for lo in (0.125, 0.25, 0.375) for hi in (0.4375, 0.5, 0.625)] + \
    [(0.5625, 0.75), (0.5, 0.75), (0.0625, 0.25), (0.0, 0.125), (0.3125, 0.3125)]


def grid_boxes():
    """the 14 x 14 dyadic predictions against GRID_GT: one- and two-sided ties, nesting either way, touching, disjoint, zero width"""
    iv = np.array(GRID_INTERVALS, np.float64)
    c, w = (iv[:, 0] + iv[:, 1]) / 2, iv[:, 1] - iv[:, 0]
    ix, iy = np.meshgrid(np.arange(14), np.arange(14), indexing="ij")
    b = np.stack([c[ix.ravel()], c[iy.ravel()], w[ix.ravel()], w[iy.ravel()]], 1)
    assert np.array_equal(b.astype(np.float32).astype(np.float64), b)
    return b.astype(np.float32)


def grid_case(extra=12, C=5):
    g = grid_boxes()
    R = len(g) + extra
    boxes = np.concatenate([g, _boxes(75, "grid.unmatched", extra)])
    match = np.full(R, -1, np.int32)
    match[:len(g)] = 0
    return dict(logits=synth.normal(75, "grid.logits", (R, C), 2.0).astype(np.float32), boxes=boxes, labels=np.array([2], np.int64),
                gt=GRID_GT[None].copy(), match=match)


MARGIN = 2.0 ** -10


def _margins(p, t):
    """the smallest |a - b| among the pairs that decide a max / min / clamp / L1 sign of criterion.hip, per pair (float64 on fp32 inputs)"""
    p, t = p.astype(np.float64), t.astype(np.float64)
    c = lambda b: (b[:, 0] - 0.5 * b[:, 2], b[:, 1] - 0.5 * b[:, 3], b[:, 0] + 0.5 * b[:, 2], b[:, 1] + 0.5 * b[:, 3])
    ax1, ay1, ax2, ay2 = c(p)
    bx1, by1, bx2, by2 = c(t)
    iwr, ihr = np.minimum(ax2, bx2) - np.maximum(ax1, bx1), np.minimum(ay2, by2) - np.maximum(ay1, by1)
    d = [ax1 - bx1, ay1 - by1, ax2 - bx2, ay2 - by2, iwr, ihr] + [p[:, i] - t[:, i] for i in range(4)]
    return np.abs(np.stack(d, 1)).min(1)


def random_pairs(n=512):
    """n prediction / target pairs of criterion_cases' box distribution, drawn until every deciding difference exceeds MARGIN
    -> (pred [n, 4], gt [n, 4], number rejected)"""
    pool = 4 * n
    p, t = _boxes(77, "pairs.pred", pool), _boxes(77, "pairs.gt", pool)
    keep = np.flatnonzero(_margins(p, t) > MARGIN)
    assert len(keep) >= n
    keep = keep[:n]
    return p[keep], t[keep], int(keep[-1] + 1 - n)


def pairs_case(n=512, extra=5, C=5):
    p, t, rejected = random_pairs(n)
    R = n + extra
    perm = np.argsort(synth.uniform01(77, "pairs.perm", (n,)), kind="stable")
    match = np.full(R, -1, np.int32)
    match[:n] = perm
    gt = np.empty_like(t)
    gt[perm] = t                                               # row i is matched to target perm[i], which holds pair i's box
    return dict(logits=synth.normal(77, "pairs.logits", (R, C), 2.0).astype(np.float32), boxes=np.concatenate([p, _boxes(77, "pairs.un", extra)]),
                labels=(np.arange(n) % C).astype(np.int64), gt=gt, match=match), rejected


def background_cases(C=11, R=20):
    """labels outside [0, C) on matched rows (class terms all background, box terms present), and match entries outside [0, G)"""
    base = geometry_case(C, R)
    G = 4
    labels = np.array([C, -5, C + 7, 2 ** 40], np.int64)
    gt = _boxes(79, "bg.gt", G)
    m1 = np.full(R, -1, np.int32)
    m1[[0, 3, 16, R - 1]] = [0, 1, 2, 3]
    m2 = np.full(R, -1, np.int32)
    m2[[1, 7, R - 1]] = [G, -7, 2 ** 31 - 1]
    return {"labels_outside": dict(base, labels=labels, gt=gt, match=m1),
            "match_outside": dict(base, labels=np.array([1, 2, 3, 4], np.int64), gt=gt, match=m2)}


def layered_case(nl=3, B=3, Q=7, C=11):
    """21 rows per layer, another match table and other predictions per layer, one set of targets"""
    R, G = B * Q, 5
    layers = []
    for l in range(nl):
        order = np.argsort(synth.uniform01(81, f"layered.rows.{l}", (R,)), kind="stable")[:G]
        match = np.full(R, -1, np.int32)
        match[order] = np.argsort(synth.uniform01(81, f"layered.tg.{l}", (G,)), kind="stable")
        logits = synth.normal(81, f"layered.logits.{l}", (R, C), 2.0).astype(np.float32)
        logits[order[0], 0] = 16.7
        layers.append(dict(logits=logits, boxes=_boxes(81, f"layered.pred.{l}", R), match=match))
    return dict(layers=layers, labels=(np.arange(G) * 2 % C).astype(np.int64), gt=_boxes(81, "layered.gt", G))


def upstream(seed, key, shape):
    """an upstream gradient in [0.5, 2), some entries negative"""
    v = 0.5 + 1.5 * synth.uniform01(seed, key, shape)
    return (v * np.where(synth.uniform01(seed, key + ".sign", shape) < 0.25, -1.0, 1.0)).astype(np.float32)


FAMILIES = ("ladder", "geometry", "grid", "pairs", "background", "element", "layered")


def _case(name, layers, labels, gt, nb=None, alpha=0.25, gamma=2.0, d_losses=None, d_elem=None, identity=False):
    """One call of the (layered) criterion.  layers: dicts of logits [R, C], boxes [R, 4] or None, match [R]; d_losses [nl, 3] / d_elem
    [nl, R, C] or None; identity: the device gets match == NULL and `match` must be each row's global index."""
    return dict(name=name, layers=layers, labels=labels, gt=gt, nb=nb, alpha=alpha, gamma=gamma, d_losses=d_losses, d_elem=d_elem,
                identity=identity)


def layer_args(case, l):
    """the arguments of `reference` / `restate32` for layer l of a case"""
    lay = case["layers"][l]
    return dict(logits=lay["logits"], boxes=lay["boxes"], labels=case["labels"], gt=case["gt"], match=lay["match"], nb=case["nb"],
                alpha=case["alpha"], gamma=case["gamma"], d_losses=None if case["d_losses"] is None else case["d_losses"][l],
                d_elem=None if case["d_elem"] is None else case["d_elem"][l])


def _one(d):
    return [dict(logits=d["logits"], boxes=d["boxes"], match=d["match"])]


def cases(family):
    """the calls of one family, the same list for the CPU restatement and the device"""
    out = []
    if family == "ladder":
        d = ladder_case()
        for i, (g, a) in enumerate((g, a) for g in GAMMAS for a in ALPHAS):
            out.append(_case(f"ladder gamma={g} alpha={a}", _one(d), d["labels"], d["gt"], NUM_BOXES[i % 6], a, g, upstream(83, f"ladder.{i}", (1, 3))))
    elif family == "geometry":
        for i, (C, R) in enumerate((C, R) for C in GEOM_C for R in GEOM_R):
            d = geometry_case(C, R)
            out.append(_case(f"geometry C={C} R={R}", _one(d), d["labels"], d["gt"], NUM_BOXES[i % 6], ALPHAS[i % 2], GAMMAS[(i // 2) % 6],
                             upstream(85, f"geom.{i}", (1, 3))))
    elif family == "grid":
        d = grid_case()
        out.append(_case("grid, upstream 1", _one(d), d["labels"], d["gt"], None, d_losses=np.ones((1, 3), np.float32)))
        out.append(_case("grid, weighted", _one(d), d["labels"], d["gt"], 2.5, d_losses=np.array([[0.75, 5.0, 2.0]], np.float32)))
    elif family == "pairs":
        d, _ = pairs_case()
        out.append(_case("512 random pairs", _one(d), d["labels"], d["gt"], 37.0, d_losses=np.array([[1.0, 5.0, 2.0]], np.float32)))
    elif family == "background":
        for i, (k, d) in enumerate(background_cases().items()):
            out.append(_case(k, _one(d), d["labels"], d["gt"], (2.5, None)[i], d_losses=upstream(87, f"bg.{i}", (1, 3))))
    elif family == "element":
        lc = layered_case()
        R, C = lc["layers"][0]["logits"].shape
        for nl in (1, 3):
            for nb in (None, 2.5):
                lays = lc["layers"][:nl]
                de = upstream(89, f"elem.{nl}", (nl, R, C))                           # the same for both num_boxes: it must not matter
                out.append(_case(f"d_elem and d_losses, boxes, nl={nl} nb={nb}", lays, lc["labels"], lc["gt"], nb, 0.4, 1.5,
                                 upstream(89, f"elem.dl.{nl}.{nb}", (nl, 3)), de))
                ident = [dict(logits=lay["logits"], boxes=None, match=np.arange(l * R, (l + 1) * R, dtype=np.int32)) for l, lay in enumerate(lays)]
                labels = (np.argsort(synth.uniform01(89, f"elem.labels.{nl}", (nl * R,)), kind="stable") % C).astype(np.int64)
                out.append(_case(f"d_elem alone, no boxes, match NULL, nl={nl} nb={nb}", ident, labels, np.zeros((0, 4), np.float32), nb, 0.25, 2.0,
                                 None, de, identity=True))
    elif family == "layered":
        lc = layered_case()
        for i, nb in enumerate((5.0, None)):
            out.append(_case(f"layered nl=3 nb={nb}", lc["layers"], lc["labels"], lc["gt"], nb, (0.25, 0.4)[i], (2.0, 0.5)[i], upstream(91, f"lay.{i}", (3, 3))))
    else:
        raise KeyError(family)
    return out


# ------------------------------------------------------------------------------------------------ matcher cost
def cost_case():
    """B = 3 images of Q = 196 predictions (the grid boxes; every class column of row q holds LADDER[(q + 7 b) % 29]), the one grid target
    in images 0 and 2, no target in image 1"""
    Q, C, B = 196, 5, 3
    det = np.zeros((B, Q, C + 4), np.float32)
    for b in range(B):
        det[b, :, :C] = LADDER[(np.arange(Q) + 7 * b) % len(LADDER)][:, None]
        det[b, :, C:] = np.roll(grid_boxes(), 5 * b, axis=0)
    return dict(det=det, C=C, labels=np.array([1, 3], np.int64), gt=np.stack([GRID_GT, GRID_GT]), offs=np.array([0, 1, 1, 2], np.int32))


def cost_expected(case, w, alpha, gamma, rows_from, ar):
    """the flat cost buffer [G * Q] (image b's [Q, n_b] matrix at offs[b] * Q) through cost_statements"""
    det, C, offs = case["det"], case["C"], case["offs"]
    B, Q = det.shape[:2]
    out = []
    for b in range(B):
        for g in range(offs[b], offs[b + 1]):                 # n_b <= 1 here: the matrix is a column
            rows = det[rows_from if rows_from >= 0 else b]
            out.append(cost_statements(rows[:, case["labels"][g]], rows[:, C:], np.repeat(case["gt"][g][None], Q, 0), *w, alpha, gamma, ar))
    return out
