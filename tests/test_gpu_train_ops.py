"""`-m gpu`: the training step's adjoint kernels (train_ops.hip, the second half of attn_f32m.hip), one at a time through their
operator entry points (include/dinodet.h "training-step operators"), against the same operation in float64 on the CPU: plain torch
ops under autograd on the float32-rounded inputs.

Every comparison follows one rule.  For each case and each logical output GROUP (never one tensor-wide maximum over several)
    e_ref = rel_err(float32 CPU evaluation of the same reference code, float64 evaluation)
    rel_err(kernel, float64) <= max(floor, 4 * e_ref)
The factor 4 covers a different summation order (wave trees, MFMA k-chains, float atomics against the CPU's lanes); `floor` is the
bound test_gpu_ops.py holds the forward of the same operation class to: 2e-6 row ops, 3e-6 GEMM-like, 5e-6 attention, 1e-5
deformable.  Written outputs sit between 64 guard rows of a sentinel and start as NaN; accumulated outputs start from a seeded
non-zero tensor; every case runs in the fast and in the deterministic mode, each held to float64 on its own, and two deterministic
runs must be bit-identical.  Each comparison prints its measured error next to e_ref."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import synth
from oracle import dinodet_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 777.25
F_ROW, F_GEMM, F_ATTN, F_DEFORM = 2e-6, 3e-6, 5e-6, 1e-5
WORST = {}      # kernel -> (error / bound, error, e_ref, where) of the comparison closest to its bound: printed at the end of the module


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from tests import gpu_util
    nat.lib()
    yield gpu_util
    for k in sorted(WORST):
        print(f"train-op worst  {k:<14s} {WORST[k][0]:.2f} of its bound: err {WORST[k][1]:.2e}  e_ref {WORST[k][2]:.2e}  at {WORST[k][3]}")


def _n(key, shape, std=1.0):
    return synth.normal(23, key, shape, std)


def _tcheck(rc):
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {nat.lib().dod_decoder_train_last_error().decode()}")


def _err(a, b, zero_scale=None):
    """max|a - b| / max|b| over ONE output group.  zero_scale: the denominator for a group whose float64 reference is identically zero
    (the metric has none then): the magnitude of the terms that cancel to that zero, worked out by the caller from the inputs"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.abs(b).max()
    if den == 0.0 and zero_scale:
        den = zero_scale
    return float(np.abs(a - b).max() / max(den, 1e-300))


def _hold(kernel, where, group, got, ref64, ref32, floor, zero_scale=None):
    e, e_ref = _err(got, ref64, zero_scale), _err(ref32, ref64, zero_scale)
    bound = max(floor, 4 * e_ref)
    print(f"{kernel} {where} {group}: err {e:.2e}  e_ref {e_ref:.2e}  bound {bound:.2e}")
    if e / bound >= WORST.get(kernel, (-1.0,))[0]:
        WORST[kernel] = (e / bound, e, e_ref, f"{where} {group}")
    assert e <= bound, (kernel, where, group, e, e_ref)


def _guarded(G, rows, pitch, cols=None):
    """[GUARD + rows + GUARD, pitch]: sentinel everywhere, NaN in the `cols` real columns of the real rows -> (whole buffer, real rows)"""
    full = torch.full((rows + 2 * GUARD, pitch), SENT, device=G.dev(), dtype=torch.float32)
    full[GUARD:GUARD + rows, :pitch if cols is None else cols] = float("nan")
    return full, full[GUARD:GUARD + rows]


def _guards_intact(full, rows, cols=None, what=""):
    f = full.cpu()
    assert bool((f[:GUARD] == SENT).all()) and bool((f[GUARD + rows:] == SENT).all()), f"{what}: guard rows written"
    if cols is not None and cols < f.shape[1]:
        assert bool((f[GUARD:GUARD + rows, cols:] == SENT).all()), f"{what}: columns past the row's width written"
    assert not bool(torch.isnan(f).any()), f"{what}: elements left unwritten"


class _Mode:
    """the "deterministic" test option for the body of a `with`, handed back on exit"""

    def __init__(self, det):
        self.det = det

    def __enter__(self):
        nat.set_option("deterministic", 1 if self.det else 0)

    def __exit__(self, *a):
        nat.set_option("deterministic", -1)


def _u01(key, idx):
    """train_ops.hip u01(key, idx) in numpy uint64: the splitmix64 finaliser of key + idx * golden, top 24 bits as a float in [0, 1)"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(key) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def _keep(key, n, p):
    """keep mask of elements 0..n-1 (all ones for p == 0, where the kernels draw nothing)"""
    if p == 0.0:
        return np.ones(n, dtype=bool)
    return _u01(key, np.arange(n, dtype=np.uint64)) >= np.float32(p)


def _binomial_ok(keep, p):
    n = keep.size
    if p == 0.0 or n < 200:
        return
    dropped = float(n - keep.sum()) / n
    assert abs(dropped - p) <= 4.0 * math.sqrt(p * (1 - p) / n), (dropped, p, n)


def test_u01_restatement_matches_the_header_formula():
    """the numpy restatement itself: 64-bit wrap-around, range, and a hand-computed value (key 0, index 0 hashes to 0)"""
    assert float(_u01(0, [0])[0]) == 0.0
    u = _u01(0xDEADBEEFCAFEF00D, np.arange(100000, dtype=np.uint64) + np.uint64(2 ** 40))
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(float(u.mean()) - 0.5) < 0.01
    z = (0x9E3779B97F4A7C15 + 5) % 2 ** 64      # key 5, index 1, in Python integers
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert float(_u01(5, [1])[0]) == (z >> 40) / 16777216.0


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_ref(x, g, dy, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    gt = torch.from_numpy(g).to(dtype).requires_grad_()
    bt = torch.zeros(g.shape[0], dtype=dtype, requires_grad=True)
    mu = xt.mean(-1, keepdim=True)
    var = ((xt - mu) ** 2).mean(-1, keepdim=True)
    y = (xt - mu) / torch.sqrt(var + 1e-6) * gt + bt
    y.backward(torch.from_numpy(dy).to(dtype))
    return xt.grad.numpy(), gt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("rows,D", [(1, 64), (3, 100), (7, 128), (257, 384), (513, 1024), (130, 1028), (65, 1536), (5, 2048), (9000, 192), (1100, 128)])
def test_layernorm_bwd(G, rows, D):
    """ln_bwd_kernel<16> up to D = 1024, <32> above; more rows than the 8 192 waves of the largest grid (the stride loop), more than the
    256 workgroups of the deterministic grid; dgamma and dbeta on their own normalisation (in the backbone tail they go to a dump).
    From 512 workgroups (2 048 rows) up the fast mode merges the workgroups' partials through 16 interleaved accumulators (ln_bwd in
    train_ops.hip): one float atomic per column and workgroup straight into dgamma / dbeta is a chain of up to 2 048 roundings at the
    size of the running sum, whose order-dependent random walk reaches the 2e-6 floor at (9000, 192)."""
    x = 2.0 * _n(f"ln.x.{rows}.{D}", (rows, D)) + 0.5
    g = 1.0 + 0.1 * _n(f"ln.g.{D}", (D,))
    dy = _n(f"ln.dy.{rows}.{D}", (rows, D))
    pre_g, pre_b = 0.05 * _n(f"ln.pg.{D}", (D,)) + 0.01, 0.05 * _n(f"ln.pb.{D}", (D,)) - 0.01
    r64, r32 = _ln_ref(x, g, dy, torch.float64), _ln_ref(x, g, dy, torch.float32)
    L = nat.lib()
    xd, gd, dyd = G.to_gpu(x), G.to_gpu(g), G.to_gpu(dy)

    def run():
        full, dx = _guarded(G, rows, D)
        dg, db = G.to_gpu(pre_g), G.to_gpu(pre_b)
        _tcheck(L.dod_op_layernorm_bwd(nat.ptr(xd), nat.ptr(gd), nat.ptr(dyd), 1e-6, rows, D, nat.ptr(dx), nat.ptr(dg), nat.ptr(db), nat.stream_ptr()))
        G.sync()
        _guards_intact(full, rows, what="dx")
        return dx.cpu().numpy().copy(), dg.cpu().numpy(), db.cpu().numpy()
    for det in (False, True):
        with _Mode(det):
            dx, dg, db = run()
            if det:
                again = run()
                assert all(np.array_equal(a, b) for a, b in zip((dx, dg, db), again)), "deterministic mode is not bit-reproducible"
        where = f"({rows}, {D}) {'det' if det else 'fast'}"
        _hold("ln_bwd", where, "dx", dx, r64[0], r32[0], F_ROW)
        _hold("ln_bwd", where, "dgamma", dg.astype(np.float64) - pre_g, r64[1], r32[1], F_ROW)
        _hold("ln_bwd", where, "dbeta", db.astype(np.float64) - pre_b, r64[2], r32[2], F_ROW)


# ------------------------------------------------------------------------------------------------ attention
def _attn_ref(q, k, v, dO, scale, keep, p, dtype):
    """q [B, H, Lq, dh], k / v [B, H, Lk, dh], dO [B, H, Lq, dh]; keep [B, H, Lq, Lk] bool or None -> o, dq, dk, dv"""
    qt, kt, vt = (torch.from_numpy(a).to(dtype).requires_grad_() for a in (q, k, v))
    s = (qt @ kt.transpose(-1, -2)) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    pr = e / e.sum(-1, keepdim=True)
    if keep is not None:
        pr = pr * torch.from_numpy(keep).to(dtype) / (1.0 - p)
    o = pr @ vt
    o.backward(torch.from_numpy(dO).to(dtype))
    return o.detach().numpy(), qt.grad.numpy(), kt.grad.numpy(), vt.grad.numpy()


def _attn_cancel(q, k, v, dO, scale):
    """With ONE key the softmax is constant: dq and dk are exactly zero in exact arithmetic, and a kernel that forms dS = P (dP - delta)
    from two differently ordered sums of the same 64 products (the flash form: dP on the MFMA, delta = <dO, O>) leaves their rounding
    difference there.  Such a group is held to the same floor, relative to the largest single term of the sum that cancels:
    scale * max|dO v^T| * max(|q|, |k|)."""
    dP = np.abs(dO.astype(np.float64) @ v.astype(np.float64).transpose(0, 1, 3, 2)).max()
    return float(scale * dP * max(np.abs(q).max(), np.abs(k).max()))


def _heads_in(a, B, L, H, dh):       # [B, H, L, dh] -> rows [B*L, H*dh]
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3).reshape(B * L, H * dh))


def _heads_out(a, B, L, H, dh):      # rows [B*L, H*dh] -> [B, H, L, dh]
    return np.asarray(a).reshape(B, L, H, dh).transpose(0, 2, 1, 3)


def _attn_case(B, H, Lq, Lk, dh, tag, big_keys=()):
    q, k, v, dO = (1.5 * _n(f"at.{n}.{tag}.{B}.{H}.{Lq}.{Lk}.{dh}", (B, H, L, dh)) for n, L in (("q", Lq), ("k", Lk), ("v", Lk), ("do", Lq)))
    dO = dO / 1.5
    for j, f in big_keys:
        k[:, :, j] *= f
    return q, k, v, dO


def _attn_run(G, q, k, v, dO, scale, form, p, key, packed):
    """one dod_op_attention_f32_vjp call on guarded outputs -> (o, dq, dk, dv) as [B, H, L, dh] arrays"""
    L = nat.lib()
    B, H, Lq, dh = q.shape
    Lk, D = k.shape[2], H * dh
    qr, kr, vr, dor = _heads_in(q, B, Lq, H, dh), _heads_in(k, B, Lk, H, dh), _heads_in(v, B, Lk, H, dh), _heads_in(dO, B, Lq, H, dh)
    if packed:
        assert Lq == Lk
        qkv = G.to_gpu(np.concatenate([qr, kr, vr], axis=1))
        qd, kd, vd, ldq, ldkv = qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, 3 * D
        gfull, gq = _guarded(G, B * Lq, 3 * D)
        dqd, dkd, dvd, lddq, lddkv = gq, gq[:, D:], gq[:, 2 * D:], 3 * D, 3 * D
        ldo = D
        dod = G.to_gpu(dor)
    else:       # five different pitches, every operand a view into a wider buffer
        ldq, ldkv, ldo, lddq, lddkv = D + 4, D + 12, D + 8, D + 16, D + 20

        def wide(a, ld):
            t = torch.full((a.shape[0], ld), 3.0e4, device=G.dev(), dtype=torch.float32)
            t[:, :D] = G.to_gpu(a)
            return t
        qd, kd, vd, dod = wide(qr, ldq), wide(kr, ldkv), wide(vr, ldkv), wide(dor, ldo)
        gfull, dqd = _guarded(G, B * Lq, lddq, D)
        kfull, dkd = _guarded(G, B * Lk, lddkv, D)
        vfull, dvd = _guarded(G, B * Lk, lddkv, D)
    ofull, od = _guarded(G, B * Lq, ldo, D)
    nbytes = L.dod_op_attention_f32_vjp_workspace_bytes(B, Lq, Lk, H, dh, form)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=G.dev())
    _tcheck(L.dod_op_attention_f32_vjp(nat.ptr(qd), ldq, nat.ptr(kd), nat.ptr(vd), ldkv, nat.ptr(dod), nat.ptr(od), ldo, nat.ptr(dqd), lddq,
                                       nat.ptr(dkd), nat.ptr(dvd), lddkv, B, Lq, Lk, H, dh, scale, form, p, key, nat.ptr(ws), nbytes, nat.stream_ptr()))
    G.sync()
    _guards_intact(ofull, B * Lq, D, "o")
    if packed:
        _guards_intact(gfull, B * Lq, None, "dq | dk | dv")
    else:
        _guards_intact(gfull, B * Lq, D, "dq")
        _guards_intact(kfull, B * Lk, D, "dk")
        _guards_intact(vfull, B * Lk, D, "dv")
    out = (od[:, :D], dqd[:, :D], dkd[:, :D], dvd[:, :D])
    return tuple(_heads_out(t.cpu().numpy(), B, Lx, H, dh).copy() for t, Lx in zip(out, (Lq, Lq, Lk, Lk)))


def _attn_hold(kernel, where, got, r64, r32, cancel=None):
    """o, dq, dk, dv: each on its own normalisation, over the whole tensor AND over every (image, head) slice.  cancel: see _attn_cancel"""
    for name, a, b64, b32 in zip(("o", "dq", "dk", "dv"), got, r64, r32):
        zs = cancel if name in ("dq", "dk") else None      # o and dv are never identically zero: the plain rule
        _hold(kernel, where, name, a, b64, b32, F_ATTN, zs)
        B, H = a.shape[:2]
        worst = (-1.0, 0.0, None)
        for b in range(B):
            for h in range(H):
                e, e_ref = _err(a[b, h], b64[b, h], zs), _err(b32[b, h], b64[b, h], zs)
                worst = max(worst, (e / max(F_ATTN, 4 * e_ref), e, (b, h)), key=lambda t: t[0])
                assert e <= max(F_ATTN, 4 * e_ref), (kernel, where, name, (b, h), e, e_ref)
        if B * H > 1:
            print(f"{kernel} {where} {name}: worst (image, head) slice {worst[2]} err {worst[1]:.2e} = {worst[0]:.2f} of its bound")


FLASH_CASES = [(1, 1, 1, 1), (2, 2, 31, 31), (1, 2, 64, 64), (1, 2, 128, 128), (2, 3, 65, 129), (2, 1, 200, 90), (1, 2, 90, 200), (1, 6, 257, 257),
               (1, 2, 1370, 1370)]


@pytest.mark.parametrize("B,H,Lq,Lk", FLASH_CASES)
def test_attention_flash_vjp(G, B, H, Lq, Lk):
    """attn_f32m_kernel with the log-sum-exp output, then attn_f32m_delta / bwd_kv / bwd_q: one row, below one 32-row wave, exact tile
    multiples (64, 128), rectangular both ways, several workgroups, and the workload's 1 370 = 10 x 128 + 90 tokens.  Packed q | k | v
    (square cases) and five differing pitches."""
    dh = 64
    q, k, v, dO = _attn_case(B, H, Lq, Lk, dh, "fl")
    scale = 1.0 / math.sqrt(dh)
    r64, r32 = _attn_ref(q, k, v, dO, scale, None, 0.0, torch.float64), _attn_ref(q, k, v, dO, scale, None, 0.0, torch.float32)
    for packed in ((True, False) if Lq == Lk else (False,)):
        for det in (False, True):
            with _Mode(det):
                got = _attn_run(G, q, k, v, dO, scale, 1, 0.0, 0, packed)
                if det:
                    again = _attn_run(G, q, k, v, dO, scale, 1, 0.0, 0, packed)
                    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "deterministic mode is not bit-reproducible"
            _attn_hold("attn_flash", f"({B}, {H}, {Lq}, {Lk}) {'packed' if packed else 'pitched'} {'det' if det else 'fast'}", got, r64, r32,
                       _attn_cancel(q, k, v, dO, scale) if Lk == 1 else None)


def test_attention_flash_vjp_forced_rescale(G):
    """keys 70 and 150 scaled by 8 and 16 (as test_attention_bf16_forced_rescale): the row maxima are large and move from tile to tile"""
    B, H, L, dh = 1, 2, 200, 64
    q, k, v, dO = _attn_case(B, H, L, L, dh, "flr", big_keys=((70, 8.0), (150, 16.0)))
    scale = 1.0 / math.sqrt(dh)
    r64, r32 = _attn_ref(q, k, v, dO, scale, None, 0.0, torch.float64), _attn_ref(q, k, v, dO, scale, None, 0.0, torch.float32)
    for packed in (True, False):
        for det in (False, True):
            with _Mode(det):
                got = _attn_run(G, q, k, v, dO, scale, 1, 0.0, 0, packed)
                if det:
                    again = _attn_run(G, q, k, v, dO, scale, 1, 0.0, 0, packed)
                    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "deterministic mode is not bit-reproducible"
            _attn_hold("attn_flash", f"rescale ({B}, {H}, {L}, {L}) {'packed' if packed else 'pitched'} {'det' if det else 'fast'}", got, r64, r32)


BATCHED_CASES = [(2, 4, 7, 7, 32, 0), (1, 2, 100, 100, 96, 0), (2, 3, 33, 70, 128, 0), (1, 1, 5, 1370, 64, 0), (1, 1, 3, 1408, 64, 0), (3, 2, 17, 17, 64, 2)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,Lq,Lk,dh,chunk", BATCHED_CASES)
def test_attention_batched_vjp(G, B, H, Lq, Lk, dh, chunk, p):
    """launch_mha_fwd_rect + launch_mha_bwd_rect: the softmax row kernels between batched fp32 GEMMs.  With dropout the reference
    applies the documented keep mask u01(key, item * Lk + j) >= p to its float64 probabilities, so a wrong counter on ANY element
    (the item_base of a later image chunk -- chunk = 2 runs 2 + 1 images --, a padded column) shows as a wrong o / dq / dk / dv."""
    q, k, v, dO = _attn_case(B, H, Lq, Lk, dh, "bt")
    scale = 1.0 / math.sqrt(dh)
    key = 0x5DEECE66D1234567
    keep = None
    if p > 0.0:
        keep = _keep(key, B * H * Lq * Lk, p).reshape(B, H, Lq, Lk)
        _binomial_ok(keep, p)
    r64, r32 = _attn_ref(q, k, v, dO, scale, keep, p, torch.float64), _attn_ref(q, k, v, dO, scale, keep, p, torch.float32)
    try:
        if chunk:
            nat.set_option("mha_chunk_images", chunk)
        for packed in ((True, False) if Lq == Lk else (False,)):
            for det in (False, True):
                with _Mode(det):
                    got = _attn_run(G, q, k, v, dO, scale, 0, p, key, packed)
                    if det:
                        again = _attn_run(G, q, k, v, dO, scale, 0, p, key, packed)
                        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "deterministic mode is not bit-reproducible"
                _attn_hold("attn_batched", f"({B}, {H}, {Lq}, {Lk}) dh {dh} p {p} {'packed' if packed else 'pitched'} {'det' if det else 'fast'}",
                           got, r64, r32)
    finally:
        nat.set_option("mha_chunk_images", -1)


# ------------------------------------------------------------------------------------------------ deformable gather adjoint
DEFORM_CASES = [(17, 4, 32, 2, 2, 9, False), (26, 2, 96, 2, 2, 9, False), (257, 8, 96, 2, 1, 5, False), (256, 2, 128, 1, 2, 7, False),
                (36, 2, 64, 8, 1, 9, False), (1370, 4, 64, 4, 2, 9, False), (26, 3, 32, 2, 1, 9, False), (26, 2, 96, 2, 2, 9, True)]


def _deform_inputs(N, Hd, dh, P, B, Q, same_cell):
    """proj [B*Q, ldp] whose every sample lands strictly inside a cell (fractional pixel coordinate in [0.15, 0.85] along every axis
    longer than one pixel), then a few rows overwritten with exact edges.  -> proj, ldp, (h, w), edge bookkeeping"""
    h, w = orc.spatial_factor(N)
    ncat = 2 + 3 * Hd * P
    ldp = (ncat + 3) // 4 * 4
    tag = f"{N}.{Hd}.{dh}.{P}.{B}.{Q}.{int(same_cell)}"
    rng = np.random.RandomState(N * 131 + Hd * 17 + P)
    ref = 0.3 + 0.4 * rng.rand(B * Q, 2)
    logit = np.log(ref / (1.0 - ref)).astype(np.float32)
    ref32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-logit))).astype(np.float64)        # what a float32 sigmoid of the stored logit gives
    shape = (B * Q, Hd, P)
    if same_cell:       # every sample of an image in one cell: the heaviest contention of the scatter's atomics
        cx = np.broadcast_to(np.repeat(rng.randint(0, max(w - 1, 1), B), Q)[:, None, None], shape)
        cy = np.broadcast_to(np.repeat(rng.randint(0, max(h - 1, 1), B), Q)[:, None, None], shape)
    else:
        cx, cy = rng.randint(0, max(w - 1, 1), shape), rng.randint(0, max(h - 1, 1), shape)
    fx, fy = 0.15 + 0.7 * rng.rand(*shape), 0.15 + 0.7 * rng.rand(*shape)
    locx = (cx + fx) / (w - 1) if w > 1 else np.full(shape, 0.5)
    locy = (cy + fy) / (h - 1) if h > 1 else np.full(shape, 0.5)
    off = np.stack([locx - ref32[:, 0, None, None], locy - ref32[:, 1, None, None]], axis=-1)      # [BQ, Hd, P, 2]
    proj = np.zeros((B * Q, ldp), dtype=np.float32)
    proj[:, :2] = logit
    proj[:, 2:2 + 2 * Hd * P] = off.reshape(B * Q, -1).astype(np.float32)
    proj[:, 2 + 2 * Hd * P:ncat] = _n(f"df.aw.{tag}", (B * Q, Hd * P))
    edges = {}
    if not same_cell:
        # rows with reference logits 0 (sigmoid = 0.5 exactly in both precisions) and offsets that put the location exactly ON, and beyond, the clamp
        def put(row, ox, oy):
            proj[row, 0:2] = 0.0
            proj[row, 2:2 + 2 * Hd * P] = np.tile(np.array([ox, oy], dtype=np.float32), Hd * P)
        put(0, -0.5, -0.5)                 # location (0, 0): the gradient passes
        put(1, 0.5, 0.5)                   # location (1, 1): passes; last column and last row, the four corners coincide
        put(2, 0.9, -0.8)                  # beyond both ends: offset gradients exactly 0
        put(3, 0.5, -0.8)                  # x on the clamp (passes), y beyond (0)
        edges = {"zero_xy": [2], "zero_y": [3], "rows": [0, 1, 2, 3]}
    return proj, ldp, (h, w), edges


def _deform_cells(proj, Hd, P, h, w, dtype):
    """cell indices (x0, y0) and fractional parts of every sample, evaluated in `dtype`"""
    pr = proj.astype(dtype)
    one = dtype(1.0)
    ref = one / (one + np.exp(-pr[:, :2]))
    off = pr[:, 2:2 + 2 * Hd * P].reshape(-1, Hd, P, 2)
    loc = np.clip(ref[:, None, None, :] + off, dtype(0.0), dtype(1.0))
    lx, ly = loc[..., 0] * dtype(w - 1), loc[..., 1] * dtype(h - 1)
    return np.floor(lx).astype(np.int64), np.floor(ly).astype(np.int64), lx - np.floor(lx), ly - np.floor(ly)


def _deform_ref(proj, values, dout, B, Q, N, Hd, P, dh, h, w, dtype):
    pt = torch.from_numpy(proj).to(dtype).requires_grad_()
    vt = torch.from_numpy(values).to(dtype).requires_grad_()
    ref = torch.sigmoid(pt[:, :2]).view(B, Q, 2)
    off = pt[:, 2:2 + 2 * Hd * P].reshape(B, Q, Hd, P, 2)
    wts = torch.softmax(pt[:, 2 + 2 * Hd * P:2 + 3 * Hd * P].reshape(B, Q, Hd, P), dim=-1)
    out = orc.deformable_sample(vt.view(B, N, Hd, dh), ref, off, wts, h, w)
    out.backward(torch.from_numpy(dout).to(dtype).view(B, Q, Hd, dh))
    return pt.grad.numpy(), vt.grad.numpy()


@pytest.mark.parametrize("N,Hd,dh,P,B,Q,same_cell", DEFORM_CASES)
def test_deform_sample_bwd(G, N, Hd, dh, P, B, Q, same_cell):
    """deform_bwd_kernel<DET>, deform_bwd_values_det_kernel, deform_dref_det_kernel: head_dim 32 / 64 / 96 / 128 (the `lane + 64` half
    at full width), 1 / 2 / 4 / 8 points, h = 1, a ragged last workgroup (27 items).  No sample sits near a cell border -- asserted: a
    float32 and a float64 evaluation of the locations give identical cells -- so NO element is excluded; the exact clamp edges are
    set by hand.  The two shared reference-logit columns, the offsets, the point weights and dvalues each on their own scale."""
    proj, ldp, (h, w), edges = _deform_inputs(N, Hd, dh, P, B, Q, same_cell)
    x32, y32, fx32, fy32 = _deform_cells(proj, Hd, P, h, w, np.float32)
    x64, y64, fx64, fy64 = _deform_cells(proj, Hd, P, h, w, np.float64)
    assert np.array_equal(x32, x64) and np.array_equal(y32, y64), "precondition: a sample changes cell between float32 and float64"
    inner = np.ones(B * Q, dtype=bool)
    inner[edges.get("rows", [])] = False
    for f, n in ((fx64, w), (fy64, h)):
        if n > 1:
            assert f[inner].min() >= 0.149 and f[inner].max() <= 0.851, "precondition: a sample within 0.15 of a cell border"
    Dd, HP = Hd * dh, Hd * P
    values, dout = _n(f"df.v.{N}.{Dd}.{B}", (B * N, Dd)), _n(f"df.g.{Q}.{Dd}.{B}", (B * Q, Dd))
    pre_v = 0.05 * _n(f"df.pv.{N}.{Dd}.{B}", (B * N, Dd)) + 0.01
    r64 = _deform_ref(proj, values, dout, B, Q, N, Hd, P, dh, h, w, torch.float64)
    r32 = _deform_ref(proj, values, dout, B, Q, N, Hd, P, dh, h, w, torch.float32)
    for row in edges.get("zero_xy", []):      # the reference itself: beyond the clamp nothing flows
        assert not r64[0][row, 2:2 + 2 * HP].any()
    L = nat.lib()
    pd, vd, gd = G.to_gpu(proj), G.to_gpu(values), G.to_gpu(dout)

    def run():
        full, dproj = _guarded(G, B * Q, ldp)
        dv = G.to_gpu(pre_v)
        _tcheck(L.dod_op_deform_sample_bwd(nat.ptr(pd), ldp, nat.ptr(vd), nat.ptr(gd), B, Q, N, Hd, P, dh, h, w, nat.ptr(dproj), nat.ptr(dv), nat.stream_ptr()))
        G.sync()
        _guards_intact(full, B * Q, what="dproj")
        return dproj.cpu().numpy().copy(), dv.cpu().numpy()
    for det in (False, True):
        with _Mode(det):
            dproj, dv = run()
            if det:
                again = run()
                assert np.array_equal(dproj, again[0]) and np.array_equal(dv, again[1]), "deterministic mode is not bit-reproducible"
        where = f"(N {N}, Hd {Hd}, dh {dh}, P {P}, B {B}, Q {Q}{', one cell' if same_cell else ''}) {'det' if det else 'fast'}"
        assert not dproj[:, 2 + 3 * HP:].any(), "padding columns of dproj must stay zero"
        for row in edges.get("zero_xy", []):
            assert not dproj[row, 2:2 + 2 * HP].any(), "offset gradient beyond the clamp must be exactly 0"
        for row in edges.get("zero_y", []):
            assert not dproj[row, 3:2 + 2 * HP:2].any(), "y-offset gradient beyond the clamp must be exactly 0"
        _hold("deform_bwd", where, "dproj[:, 0:2]", dproj[:, :2], r64[0][:, :2], r32[0][:, :2], F_DEFORM)
        _hold("deform_bwd", where, "offsets", dproj[:, 2:2 + 2 * HP], r64[0][:, 2:2 + 2 * HP], r32[0][:, 2:2 + 2 * HP], F_DEFORM)
        _hold("deform_bwd", where, "point weights", dproj[:, 2 + 2 * HP:2 + 3 * HP], r64[0][:, 2 + 2 * HP:2 + 3 * HP], r32[0][:, 2 + 2 * HP:2 + 3 * HP], F_DEFORM)
        _hold("deform_bwd", where, "dvalues", dv.astype(np.float64) - pre_v, r64[1], r32[1], F_DEFORM)


# ------------------------------------------------------------------------------------------------ LoRA gradients
def _lora_ref(X, dY, A, Bm, alpha, dtype):
    X, dY, A, Bm = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in (X, dY, A, Bm))
    return (alpha * (dY @ Bm).t() @ X).numpy(), (alpha * dY.t() @ (X @ A.t())).numpy()


# every rank and every M with at least two feature pairs; the strided dY (a column block of a buffer three times as wide) with r = 2, 8, 9
LORA_CASES = [(1, 1, 128, 128, False), (1, 130, 100, 36, False), (2, 63, 128, 128, True), (2, 65, 384, 1152, False), (2, 1, 100, 36, True),
              (3, 65, 100, 36, False), (3, 130, 128, 128, False), (5, 63, 100, 36, False), (5, 1, 384, 1152, False),
              (8, 130, 384, 1152, True), (8, 65, 100, 36, False), (8, 63, 128, 128, True), (9, 130, 384, 1152, True), (9, 63, 100, 36, False),
              (9, 65, 128, 128, True), (12, 130, 100, 36, False), (12, 1, 128, 128, False), (64, 63, 384, 1152, False), (64, 130, 128, 128, False),
              (64, 65, 100, 36, True)]


@pytest.mark.parametrize("r,M,in_f,out_f,strided", LORA_CASES)
def test_lora_grads(G, r, M, in_f, out_f, strided):
    """lora_down_kernel / lora_up_kernel up to rank 8 (the last of the fast path; ranks that are no multiple of 4), the fp32 GEMMs from
    rank 9; M below and just past one 64-row chunk; out_f no multiple of the 256 columns of a workgroup; dY as the middle column
    block of a [M, 3 out_f] buffer (the q / k / v gradients of the packed dqkv)."""
    alpha = 0.75
    X, dY = _n(f"lo.x.{M}.{in_f}", (M, in_f)), _n(f"lo.dy.{M}.{out_f}", (M, out_f))
    A, Bm = _n(f"lo.a.{r}.{in_f}", (r, in_f), 0.3), _n(f"lo.b.{r}.{out_f}", (out_f, r), 0.3)
    pre_a, pre_b = 0.05 * _n(f"lo.pa.{r}.{in_f}", (r, in_f)) + 0.01, 0.05 * _n(f"lo.pb.{r}.{out_f}", (out_f, r)) - 0.01
    r64, r32 = _lora_ref(X, dY, A, Bm, alpha, torch.float64), _lora_ref(X, dY, A, Bm, alpha, torch.float32)
    L = nat.lib()
    Xd, Ad, Bd = G.to_gpu(X), G.to_gpu(A), G.to_gpu(Bm)
    if strided:
        wide = torch.full((M, 3 * out_f), 3.0e4, device=G.dev(), dtype=torch.float32)
        wide[:, out_f:2 * out_f] = G.to_gpu(dY)
        dYd, ldy = wide[:, out_f:], 3 * out_f
    else:
        dYd, ldy = G.to_gpu(dY), out_f
    nbytes = L.dod_op_lora_grads_workspace_bytes(M, r)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=G.dev())

    def run():
        dA, dB = G.to_gpu(pre_a), G.to_gpu(pre_b)
        _tcheck(L.dod_op_lora_grads(nat.ptr(Xd), in_f, nat.ptr(dYd), ldy, out_f, nat.ptr(Ad), nat.ptr(Bd), M, r, alpha, nat.ptr(dA), nat.ptr(dB),
                                    nat.ptr(ws), nbytes, nat.stream_ptr()))
        G.sync()
        return dA.cpu().numpy(), dB.cpu().numpy()
    for det in (False, True):
        with _Mode(det):
            dA, dB = run()
            if det:
                again = run()
                assert np.array_equal(dA, again[0]) and np.array_equal(dB, again[1]), "deterministic mode is not bit-reproducible"
        where = f"(r {r}, M {M}, {in_f} -> {out_f}{', strided dY' if strided else ''}) {'det' if det else 'fast'}"
        _hold("lora_grads", where, "dA", dA.astype(np.float64) - pre_a, r64[0], r32[0], F_GEMM)
        _hold("lora_grads", where, "dB", dB.astype(np.float64) - pre_b, r64[1], r32[1], F_GEMM)


# ------------------------------------------------------------------------------------------------ element-wise adjoints, column sums
PW_N = 600001       # past 2048 workgroups x 256 threads: the grid-stride loops of the 2048-workgroup launches run


def _pointwise(G, op, a, b, out_shape, n, cols=0, p=0.0, key=0):
    L = nat.lib()
    rows = int(np.prod(out_shape))
    full = torch.full((rows + 2 * GUARD * 64,), SENT, device=G.dev(), dtype=torch.float32)
    full[GUARD * 64:GUARD * 64 + rows] = float("nan")
    out = full[GUARD * 64:GUARD * 64 + rows]
    ad = G.to_gpu(a) if a is not None else None
    _tcheck(L.dod_op_train_pointwise(nat.PW[op], nat.ptr(ad), nat.ptr(G.to_gpu(b)), nat.ptr(out), n, cols, p, key, nat.stream_ptr()))
    G.sync()
    f = full.cpu()
    assert bool((f[:GUARD * 64] == SENT).all()) and bool((f[GUARD * 64 + rows:] == SENT).all()) and not bool(torch.isnan(f).any()), op
    return out.cpu().numpy().reshape(out_shape)


def _spread(key, n, lim=6.0):
    """normal values stretched so that the tails reach +-lim, with the end points present"""
    x = 2.0 * _n(key, (n,))
    x = np.clip(x, -lim, lim)
    x[:4] = (-lim, lim, 0.0, -0.0)
    return x.astype(np.float32)


@pytest.mark.parametrize("n", [PW_N, 1100003])       # 1 100 003: past the 4096 workgroups the GELU / SwiGLU launches are capped at
def test_gelu_bwd(G, n):
    pre, dy = _spread(f"pw.gelu.{n}", n), _n(f"pw.gelu.dy.{n}", (n,))

    def ref(dtype):
        x = torch.from_numpy(pre).to(dtype).requires_grad_()
        y = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
        y.backward(torch.from_numpy(dy).to(dtype))
        return x.grad.numpy()
    _hold("gelu_bwd", f"n {n}", "g", _pointwise(G, "gelu_bwd", dy, pre, (n,), n), ref(torch.float64), ref(torch.float32), F_ROW)


@pytest.mark.parametrize("rows,F", [(31579, 19), (4099, 260)])       # 600 001 and 1 065 740 elements
def test_swiglu_bwd(G, rows, F):
    pre = _spread(f"pw.swi.{rows}.{F}", rows * 2 * F).reshape(rows, 2 * F)
    dh = _n(f"pw.swi.dh.{rows}.{F}", (rows, F))

    def ref(dtype):
        x = torch.from_numpy(pre).to(dtype).requires_grad_()
        x1, x2 = x[:, :F], x[:, F:]
        (x1 * torch.sigmoid(x1) * x2).backward(torch.from_numpy(dh).to(dtype))
        return x.grad.numpy()
    got = _pointwise(G, "swiglu_bwd", dh, pre, (rows, 2 * F), rows, cols=F)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    _hold("swiglu_bwd", f"({rows}, {F})", "d x1", got[:, :F], r64[:, :F], r32[:, :F], F_ROW)
    _hold("swiglu_bwd", f"({rows}, {F})", "d x2", got[:, F:], r64[:, F:], r32[:, F:], F_ROW)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_relu_drop_bwd_and_dropout_add(G, p):
    """the mask of element i is u01(key, i) >= p in the forward's dropout_add and in the backward's relu_drop_bwd alike: both against the
    numpy restatement, element by element (the values are products of one rounding each: 2e-6 is far above what they need)"""
    n, key = PW_N, 0x0123456789ABCDEF
    keep = _keep(key, n, p)
    _binomial_ok(keep, p)
    y = np.maximum(_n("pw.relu.y", (n,)), 0.0).astype(np.float32)       # a ReLU output: about half exact zeros
    y[:3] = (0.0, -0.0, 1e-30)
    assert (y == 0).sum() > n // 3
    dy, a = _n("pw.relu.dy", (n,)), _n("pw.drop.a", (n,))

    def ref_relu(dtype):
        return np.where((y > 0) & keep, dy.astype(dtype) / dtype(1.0 - p), dtype(0.0))

    def ref_add(dtype, with_a):
        v = np.where(keep, dy.astype(dtype) / dtype(1.0 - p), dtype(0.0))
        return a.astype(dtype) + v if with_a else v
    got = _pointwise(G, "relu_drop_bwd", dy, y, (n,), n, p=p, key=key)
    assert np.array_equal(got != 0, (y > 0) & keep & (dy != 0)), "relu_drop_bwd: the pattern of zeros is not mask AND (y > 0)"
    _hold("relu_drop_bwd", f"p {p}", "g", got, ref_relu(np.float64), ref_relu(np.float32), F_ROW)
    got = _pointwise(G, "dropout_add", a, dy, (n,), n, p=p, key=key)
    _hold("dropout_add", f"p {p}", "a + drop(b)", got, ref_add(np.float64, True), ref_add(np.float32, True), F_ROW)
    got = _pointwise(G, "dropout_add", None, dy, (n,), n, p=p, key=key)
    assert np.array_equal(got != 0, keep & (dy != 0)), "dropout_add: the pattern of zeros is not the mask"
    _hold("dropout_add", f"p {p}", "drop(b)", got, ref_add(np.float64, False), ref_add(np.float32, False), F_ROW)


def test_sigmoid_bwd4(G):
    rows, ld = 150001, 95          # dbox is the last four columns of the [B*Q, C + 4] detections' gradient
    z, wide = _spread("pw.sig.z", rows * 4).reshape(rows, 4), _n("pw.sig.d", (rows, ld))
    box = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)      # the taped forward output
    dbox = np.ascontiguousarray(wide[:, ld - 4:])

    def ref(dtype):
        s = torch.from_numpy(box).to(dtype)
        return (torch.from_numpy(dbox).to(dtype) * s * (1.0 - s)).numpy()
    L = nat.lib()
    full, dz = _guarded(G, rows, 4)
    wd = G.to_gpu(wide)
    _tcheck(L.dod_op_train_pointwise(nat.PW["sigmoid_bwd4"], nat.ptr(wd[:, ld - 4:]), nat.ptr(G.to_gpu(box)), nat.ptr(dz), rows, ld, 0.0, 0, nat.stream_ptr()))
    G.sync()
    _guards_intact(full, rows, what="dz")
    _hold("sigmoid_bwd4", f"rows {rows}", "dz", dz.cpu().numpy(), ref(torch.float64), ref(torch.float32), F_ROW)


@pytest.mark.parametrize("rows,cols,ld", [(1, 1, 1), (63, 65, 65), (8200, 200, 200), (8200, 200, 212), (63, 65, 77)])
def test_colsum_add(G, rows, cols, ld):
    """the bias gradient: 4 waves x up to 128 workgroups per 64 columns merged by atomics, or one workgroup per 64 columns walking every row"""
    wide = _n(f"cs.{rows}.{ld}", (rows, ld))
    pre = 0.05 * _n(f"cs.pre.{cols}", (cols,)) + 0.01
    r64 = wide[:, :cols].astype(np.float64).sum(0)
    r32 = torch.from_numpy(np.ascontiguousarray(wide[:, :cols])).sum(0).numpy()
    L = nat.lib()
    src = G.to_gpu(wide)

    def run():
        full = torch.full((cols + 2 * GUARD,), SENT, device=G.dev(), dtype=torch.float32)
        full[GUARD:GUARD + cols] = G.to_gpu(pre)
        _tcheck(L.dod_op_colsum_add(nat.ptr(src), ld, rows, cols, nat.ptr(full[GUARD:]), nat.stream_ptr()))
        G.sync()
        f = full.cpu().numpy()
        assert (f[:GUARD] == SENT).all() and (f[GUARD + cols:] == SENT).all(), "colsum_add wrote past its columns"
        return f[GUARD:GUARD + cols].copy()
    for det in (False, True):
        with _Mode(det):
            got = run()
            if det:
                assert np.array_equal(got, run()), "deterministic mode is not bit-reproducible"
        _hold("colsum_add", f"({rows}, {cols}, ld {ld}) {'det' if det else 'fast'}", "dst", got.astype(np.float64) - pre, r64, r32, F_ROW)
