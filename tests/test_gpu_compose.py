"""GPU parity of the composed canvases (dod_preprocess_compose, dinov2_od_amd/augment.py compose_batch): a fill colour with disjoint
pieces pasted into it, each piece crop -> colour jitter -> resize -> flip at its own size.  Bit-exact against Pillow's paste chain and
against the numpy restatement (tests/compose_cases.py, itself pinned against Pillow by tests/test_compose_cpu.py), for the uint8 HWC and
the fp32 CHW output; every output byte written exactly once and nothing outside; a single full-canvas piece against `augment_batch`;
pieces the kernels must ignore; the entry's own argument check; run-to-run equality; the uint8 bytes into the model; one training step
on a mosaic batch."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as ppo
from tests import augment_cases as ac
from tests import compose_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aug():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import augment
    return augment


# --------------------------------------------------------------------------------------------------------- 1. bit-exact parity
@pytest.mark.parametrize("name", list(cc.CASES))
def test_composed_batch_is_bit_exact_against_pillow_and_the_restatement(aug, name):
    c, want = cc.case(name)
    pil = cc.pillow(name)
    N, (out_h, out_w) = len(c["pieces"]), c["size"]
    u8, none = aug.compose_batch(c["images"], None, c["pieces"], c["size"], c["fill"], as_uint8=True)
    f32, _ = aug.compose_batch(c["images"], None, c["pieces"], c["size"], c["fill"])
    assert none is None and u8.dtype == torch.uint8 and u8.shape == (N, out_h, out_w, 3) and u8.is_cuda
    assert f32.dtype == torch.float32 and f32.shape == (N, 3, out_h, out_w) and f32.is_cuda
    u8, f32 = u8.cpu().numpy(), f32.cpu().numpy()
    for n in range(N):
        assert np.array_equal(u8[n], pil[n]), (name, n, "uint8 vs Pillow")
        assert np.array_equal(u8[n], want[n]), (name, n, "uint8 vs the restatement")
        assert np.array_equal(f32[n].view(np.uint32), ppo.to_tensor(pil[n]).view(np.uint32)), (name, n, "fp32 vs Pillow")
        assert np.array_equal(f32[n].view(np.uint32), ppo.to_tensor(want[n]).view(np.uint32)), (name, n, "fp32 vs the restatement")


# ----------------------------------------------------------------------------------------------- 2. exactly once, and in bounds
def _stage_case(aug, c):
    from dinov2_od_amd import preprocess as pre
    shapes = [im.shape[:2] for im in c["images"]]
    rows, offs, jitter = aug._check_pieces(shapes, c["pieces"], *c["size"])
    fill, per_canvas = aug._check_fill(c["fill"], len(c["pieces"]))
    src, src_offs, hs, ws = pre._stage(c["images"], torch.device("cuda"))
    return (src, src_offs, hs, ws, rows, offs, jitter, fill, per_canvas) + tuple(c["size"])


@pytest.mark.parametrize("name", ["sixteen", "zoom_out"])
@pytest.mark.parametrize("as_uint8", [True, False])
def test_every_output_byte_is_written_once_and_nothing_outside(aug, name, as_uint8):
    """through the C entry into the middle of a buffer pre-filled with a sentinel: the guards before and after stay intact and the
    inside equals the oracle under two different sentinels -- a byte the kernels left alone would differ from it under one of them
    (fp32: neither sentinel word is a value ToTensor can produce)"""
    c, want = cc.case(name)
    N, (out_h, out_w) = len(c["pieces"]), c["size"]
    args = _stage_case(aug, c)
    guard, nbytes = 4096, N * out_h * out_w * 3 * (1 if as_uint8 else 4)
    expect = torch.from_numpy(want.copy() if as_uint8 else np.stack([ppo.to_tensor(w) for w in want]))
    for sentinel in (0xA5, 0x5A):
        buf = torch.full((guard + nbytes + guard,), sentinel, dtype=torch.uint8, device="cuda")
        inner = buf[guard:guard + nbytes]
        out = inner.view(N, out_h, out_w, 3) if as_uint8 else inner.view(torch.float32).view(N, 3, out_h, out_w)
        got = aug._launch_compose(*args, as_uint8, out=out)
        assert got.data_ptr() == buf.data_ptr() + guard
        torch.cuda.synchronize()
        assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + nbytes:] == sentinel).all()), "a guard byte was written"
        if as_uint8:
            assert torch.equal(out.cpu(), expect), sentinel
        else:
            word = int.from_bytes(bytes([sentinel] * 4), "little")
            assert not bool((out.view(torch.int32) == (word - (1 << 32) if word >= 1 << 31 else word)).any()), "a sentinel word survived"
            assert torch.equal(out.cpu().view(torch.int32), expect.view(torch.int32)), sentinel


# ----------------------------------------------------------------------------------- 3. one full-canvas piece = augment_batch
@pytest.mark.parametrize("jittered", [False, True])
def test_a_single_full_canvas_piece_is_augment_batch(aug, jittered):
    imgs = [ac._rand(s, 400 + i) for i, s in enumerate([(48, 64), (33, 50), (100, 80), (57, 300)])]
    crops, flips = [(3, 2, 50, 40), (0, 0, 50, 33), (10, 20, 60, 70), (20, 1, 270, 50)], [1, 0, 0, 1]
    jit = [(0.8, 1.3, 1.1), (1.0, 1.0, 1.0), (1.2, 1.0, 0.4), (1.0, 0.6, 1.0)] if jittered else None
    for size in ((56, 56), (20, 300)):
        pieces = [[(b, crops[b], flips[b], None if jit is None else jit[b], (0, 0, size[1], size[0]))] for b in range(4)]
        for as_uint8 in (False, True):
            got, _ = aug.compose_batch(imgs, None, pieces, size, as_uint8=as_uint8)
            want, _ = aug.augment_batch(imgs, None, crops, flips, jit, size, as_uint8=as_uint8)
            assert torch.equal(got, want), (size, as_uint8)


# --------------------------------------------------------------------------------------- 4. pieces the kernels must not touch
def test_pieces_that_are_invalid_at_the_c_level_take_the_fill(aug):
    """the host wrapper refuses these; handed to the entry directly (wrong, but every array in bounds) the pieces are absent: the
    canvas that holds only such pieces is pure fill, its neighbour is untouched by them"""
    from dinov2_od_amd import preprocess as pre
    imgs = [ac._rand((40, 50), 410), ac._rand((30, 45), 411)]
    good = [(1, (2, 3, 40, 25), True, (1.1, 0.8, 1.2), (4, 6, 30, 20)), (0, (0, 0, 50, 40), False, None, (34, 6, 20, 40))]
    rows = np.array([[0, 45, 0, 10, 10, 0, 0, 0, 10, 10],        # crop beyond the right edge of its 50-wide source
                     [1, 0, 25, 10, 10, 0, 10, 0, 10, 10],       # crop beyond the bottom edge of its 30-high source
                     [0, -1, 0, 10, 10, 0, 20, 0, 10, 10],       # negative crop offset
                     [2, 0, 0, 10, 10, 0, 30, 0, 10, 10],        # no such source
                     [0, 0, 0, 10, 10, 0, 50, 10, 10, 10],       # dest rect beyond the right edge of the 56-wide canvas
                     [0, 0, 0, 10, 10, 0, 0, 50, 10, 10],        # dest rect beyond the bottom edge
                     [0, 0, 0, 40, 10, 0, 0, 20, 2, 10],         # 40 -> 2 columns: 41 taps
                     [0, 0, 0, 10, 10, 0, 40, 20, 0, 10]] +      # empty dest rect
                    [[s, l, t, w, h, int(f), dx, dy, dw, dh] for s, (l, t, w, h), f, _, (dx, dy, dw, dh) in good], dtype=np.int32)
    offs = np.array([0, 8, 10], dtype=np.int32)
    jitter = np.array([[1.3, 0.7, 1.1]] * 8 + [[1.1, 0.8, 1.2], [1.0, 1.0, 1.0]], dtype=np.float32)
    src, src_offs, hs, ws = pre._stage(imgs, torch.device("cuda"))
    fill = np.array([[9, 8, 7], [1, 2, 3]], dtype=np.uint8)
    want = cc.restated_compose(imgs, [[], good], (56, 56), fill)
    for jit in (jitter, None):
        ref = want if jit is not None else cc.restated_compose(imgs, [[], [g[:3] + (None,) + g[4:] for g in good]], (56, 56), fill)
        got = aug._launch_compose(src, src_offs, hs, ws, rows, offs, jit, fill, True, 56, 56, True).cpu().numpy()
        assert (got[0] == fill[0]).all(), "an invalid piece was drawn"
        assert np.array_equal(got[1], ref[1])
        f32 = aug._launch_compose(src, src_offs, hs, ws, rows, offs, jit, fill, True, 56, 56, False).cpu().numpy()
        assert np.array_equal(f32[0].view(np.uint32), ppo.to_tensor(ref[0]).view(np.uint32)) and np.array_equal(f32[1], ppo.to_tensor(ref[1]))


def test_bad_arguments_raise_before_anything_is_staged_and_the_entry_checks_its_bounds(aug):
    from dinov2_od_amd import _native as nat
    from dinov2_od_amd import preprocess as pre
    imgs = [ac._rand((40, 500), 420)]
    aug.compose_batch(imgs, None, [[(0, (0, 0, 480, 40), False, None, (0, 0, 32, 28))]], (28, 32))          # exactly 15x: 31 taps
    staged = pre._STAGE_BUSY
    for pieces in ([[(0, (0, 0, 481, 40), False, None, (0, 0, 32, 28))]],                                       # 33 taps
                   [[(0, (0, 0, 100, 40), False, None, (0, 0, 6, 28))]],                                        # 35 taps in a small piece
                   [[(0, (0, 0, 100, 40), False, None, (0, 0, 20, 28)), (0, (0, 0, 100, 40), False, None, (19, 0, 13, 28))]]):      # overlap
        with pytest.raises(ValueError):
            aug.compose_batch(imgs, None, pieces, (28, 32))
    assert pre._STAGE_BUSY is staged                                       # nothing was copied, so nothing was launched
    # the C entry refuses host-known bounds beyond 32 taps by itself (DOD_ERR_INVALID), before it launches anything; so it does N or P
    # <= 0 and a missing pointer
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")
    L, p = nat.lib(), nat.ptr(z)

    def call(fn, N=1, P=1, max_ch=40, max_cw=480, max_dw=32, fills=p):
        return fn(p, p, p, p, 1, p, p, N, P, None, None, fills, 0, max_ch, max_cw, max_dw, 28, 32, p, p, p, nat.stream_ptr())
    for fn in (L.dod_preprocess_compose, L.dod_preprocess_compose_u8):
        assert call(fn, max_cw=481) == 1 and call(fn, max_ch=421) == 1          # 33 taps horizontally / vertically
        assert call(fn, N=0) == 1 and call(fn, P=0) == 1 and call(fn, fills=None) == 1 and call(fn, max_dw=33) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 5. run to run
def test_two_calls_give_equal_bytes(aug):
    c, _ = cc.case("sixteen")
    a = [aug.compose_batch(c["images"], None, c["pieces"], c["size"], c["fill"], as_uint8=u)[0].clone() for u in (False, True)]
    b = [aug.compose_batch(c["images"], None, c["pieces"], c["size"], c["fill"], as_uint8=u)[0] for u in (False, True)]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------------------------------------------------------------------- 6. uint8 into the model
def test_uint8_mosaic_feeds_the_fused_patch_embed_bit_exactly(aug):
    from tests import cases, gpu_util as G
    imgs = [ac._rand(s, 430 + i) for i, s in enumerate([(90, 120), (64, 64), (120, 80), (77, 101)])]
    plan = aug.sample_mosaic([im.shape[:2] for im in imgs], torch.Generator().manual_seed(3), (56, 70), brightness=0.4, contrast=0.4,
                             saturation=0.4)
    u8, _ = aug.compose_batch(imgs, None, plan, (56, 70), as_uint8=True)
    f32, _ = aug.compose_batch(imgs, None, plan, (56, 70))
    assert np.array_equal(u8.cpu().numpy(), cc.pillow_compose(imgs, plan, (56, 70), (124, 116, 104)))
    m = G.make_detector(cases.micro_bb(), cases.dec_cfg(True), "bf16x3")
    with torch.no_grad():
        assert torch.equal(m.forward_packed(f32).clone(), m.forward_packed_u8(u8).clone())


# ---------------------------------------------------------------------------------------------------------- 7. a training step
def test_mosaic_batch_feeds_a_training_step(aug):
    from dinov2_od_amd import losses as L
    from dinov2_od_amd.matching import HungarianMatcher
    from tests import aux_cases, cases, gpu_util as G
    bb, dc = cases.micro_bb(), aux_cases.micro_cfg()
    bb.target_dim, bb.layers = dc.hidden_dim, 3
    m = G.make_detector(bb, dc, "fp32").train()
    imgs = [ac._rand(s, 440 + i) for i, s in enumerate([(90, 120), (64, 64), (120, 80), (77, 101)])]
    rng = np.random.default_rng(0)
    targets = []
    for b in range(4):
        box = np.concatenate([rng.uniform(0.3, 0.7, (3, 2)), rng.uniform(0.1, 0.3, (3, 2))], 1).astype(np.float32)
        targets.append({"boxes": torch.from_numpy(box), "labels": torch.from_numpy(rng.integers(1, dc.num_classes, 3)), "size": torch.as_tensor([56, 56])})
    kw = dict(crop_prob=1.0, crop_frac=(0.6, 0.9), hflip_prob=0.5, brightness=0.4, contrast=0.4, saturation=0.4, min_visibility=0.25,
              mosaic_prob=1.0, mosaic_center=(0.4, 0.6))
    x, new = aug.TrainAugment((56, 56), generator=torch.Generator().manual_seed(5), **kw)(imgs, targets)
    assert x.shape == (4, 3, 56, 56) and x.dtype == torch.float32 and x.is_cuda and len(new) == 4
    # the same plan on the host (the sampler is host-side and seeded), and its targets
    plan = aug.TrainAugment((56, 56), generator=torch.Generator().manual_seed(5), **kw).sample_plan([im.shape[:2] for im in imgs])
    assert all(len(c) == 4 for c in plan)
    host = aug.compose_targets(targets, [im.shape[:2] for im in imgs], plan, (56, 56), 0.25)
    assert [len(tg["boxes"]) for tg in new] == [len(tg["boxes"]) for tg in host] and sum(len(tg["boxes"]) for tg in new) > 4
    assert np.array_equal(x.cpu().numpy(), np.stack([ppo.to_tensor(w) for w in cc.restated_compose(imgs, plan, (56, 56), (124, 116, 104))]))
    for tg, h in zip(new, host):
        assert torch.equal(tg["boxes"], h["boxes"]) and torch.equal(tg["labels"], h["labels"])
        assert tg["boxes"].shape[1:] == (4,) and tg["labels"].shape == (len(tg["boxes"]),) and tg["size"].tolist() == [56, 56]
        assert bool((tg["boxes"] >= 0).all()) and bool((tg["boxes"] <= 1).all())
    new = [{k: (v.cuda() if k in ("boxes", "labels") else v) for k, v in tg.items()} for tg in new]
    crit = L.SetCriterion(HungarianMatcher(), dc.num_classes, {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0})
    ld = crit(m(x), new)
    loss = sum(ld.values())
    loss.backward()
    assert all(bool(torch.isfinite(v)) for v in ld.values()) and bool(torch.isfinite(loss))
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    assert float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads))) > 0.0
