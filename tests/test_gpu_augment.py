"""GPU parity of the train-time augmentation (dod_preprocess_aug, dinov2_od_amd/augment.py): crop -> colour jitter -> resize ->
horizontal flip, bit-exact against Pillow and against the numpy restatement (tests/augment_cases.py, itself pinned against Pillow by
tests/test_augment_cpu.py), for the fp32 CHW and the uint8 HWC output; the identity against `preprocess_batch`; the uint8 bytes
into the model; bad arguments; run-to-run equality; one training step on a `TrainAugment` batch."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as ppo
from tests import augment_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aug():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import augment
    return augment


# --------------------------------------------------------------------------------------------------------- 1. bit-exact parity
@pytest.mark.parametrize("name", list(ac.CASES))
def test_augmented_batch_is_bit_exact_against_pillow_and_the_restatement(aug, name):
    c, want = ac.case(name)
    B = len(c["images"])
    u8, none = aug.augment_batch(c["images"], None, c["crops"], c["flips"], c["jitter"], c["size"], as_uint8=True)
    f32, _ = aug.augment_batch(c["images"], None, c["crops"], c["flips"], c["jitter"], c["size"])
    assert none is None and u8.dtype == torch.uint8 and u8.shape == (B, c["size"][0], c["size"][1], 3)
    assert f32.dtype == torch.float32 and f32.shape == (B, 3, c["size"][0], c["size"][1]) and f32.is_cuda
    u8, f32 = u8.cpu().numpy(), f32.cpu().numpy()
    for b, im in enumerate(c["images"]):
        pil = ac.pillow_chain(im, c["crops"][b], c["flips"][b], None if c["jitter"] is None else c["jitter"][b], *c["size"])
        assert np.array_equal(u8[b], pil), (name, b, "uint8 vs Pillow")
        assert np.array_equal(u8[b], want[b]), (name, b, "uint8 vs the restatement")
        assert np.array_equal(f32[b].view(np.uint32), ppo.to_tensor(pil).view(np.uint32)), (name, b, "fp32 vs Pillow")
        assert np.array_equal(f32[b], ppo.to_tensor(want[b])), (name, b, "fp32 vs the restatement")


def test_flat_image_under_contrast_is_unchanged(aug):
    c, want = ac.case("flat_contrast")
    got, _ = aug.augment_batch(c["images"], None, c["crops"], c["flips"], c["jitter"], c["size"], as_uint8=True)
    assert (got[0].cpu().numpy() == 137).all() and (c["images"][0] == 137).all() and c["jitter"][0][1] != 1.0


# --------------------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("jitter", [None, 1.0])
def test_full_crop_without_flip_or_jitter_is_preprocess_batch(aug, jitter):
    from dinov2_od_amd import preprocess as pre
    imgs = [ac._rand(s, 100 + i) for i, s in enumerate([(48, 64), (33, 50), (100, 80), (57, 300)])]
    crops = [(0, 0, im.shape[1], im.shape[0]) for im in imgs]
    jit = None if jitter is None else np.full((len(imgs), 3), jitter, dtype=np.float32)
    for size in ((56, 56), (20, 300)):
        for as_uint8 in (False, True):
            got, _ = aug.augment_batch(imgs, None, crops, [0] * len(imgs), jit, size, as_uint8=as_uint8)
            assert torch.equal(got, pre.preprocess_batch(imgs, size, as_uint8=as_uint8)), (size, as_uint8)


# --------------------------------------------------------------------------------------------------- 3. uint8 into the model
def test_augmented_uint8_batch_feeds_the_fused_patch_embed_bit_exactly(aug):
    from tests import cases, gpu_util as G
    imgs = [ac._rand(s, 110 + i) for i, s in enumerate([(480, 640), (333, 500), (300, 280)])]
    crops, flips = [(100, 40, 500, 400), (0, 0, 500, 333), (11, 7, 260, 290)], [1, 0, 1]
    jit = [(0.8, 1.3, 1.1), (1.0, 1.0, 1.0), (1.2, 1.0, 0.4)]
    u8, _ = aug.augment_batch(imgs, None, crops, flips, jit, (224, 224), as_uint8=True)
    f32, _ = aug.augment_batch(imgs, None, crops, flips, jit, (224, 224))
    for b in (0, 2):
        assert np.array_equal(u8[b].cpu().numpy(), ac.pillow_chain(imgs[b], crops[b], flips[b], jit[b], 224, 224))
    bb, dc = cases.cfg1(25)
    m = G.make_detector(bb, dc, "bf16x3", "facebook/dinov2-small")
    assert torch.equal(m.forward_packed(f32).clone(), m.forward_packed_u8(u8).clone())


# ----------------------------------------------------------------------------------------------------------- 4. bad arguments
def test_bad_arguments_raise_before_anything_is_launched(aug):
    from dinov2_od_amd import _native as nat
    imgs = [ac._rand((40, 50), 120), ac._rand((30, 30), 121)]
    ok_c, ok_f, ok_j = [(0, 0, 50, 40), (5, 5, 20, 20)], [0, 1], [(1.0, 1.0, 1.0), (1.2, 0.8, 1.0)]
    from dinov2_od_amd import preprocess as pre
    aug.augment_batch(imgs, None, ok_c, ok_f, ok_j, (28, 28))              # the good call
    staged = pre._STAGE_BUSY                                               # the event every staging copy replaces
    bad = [
        dict(crops=[(1, 0, 50, 40), (5, 5, 20, 20)]),                     # left + width > W
        dict(crops=[(0, 0, 50, 40), (5, 11, 20, 20)]),                    # top + height > H
        dict(crops=[(-1, 0, 50, 40), (5, 5, 20, 20)]),                    # negative offset
        dict(crops=[(0, 0, 0, 40), (5, 5, 20, 20)]),                      # zero width
        dict(crops=[(0, 0, 50, 0), (5, 5, 20, 20)]),                      # zero height
        dict(crops=[(0, 0, 50, 40)]),                                      # wrong lengths
        dict(flips=[0, 1, 0]),
        dict(jitter=[(1.0, 1.0, 1.0)]),
        dict(jitter=[(1.0, 1.0), (1.0, 1.0)]),
        dict(jitter=[(-0.1, 1.0, 1.0), (1.0, 1.0, 1.0)]),                 # negative factor
        dict(jitter=[(1.0, float("nan"), 1.0), (1.0, 1.0, 1.0)]),         # non-finite factors
        dict(jitter=[(1.0, 1.0, float("inf")), (1.0, 1.0, 1.0)]),
        dict(targets=[{}]),
    ]
    for kw in bad:
        a = dict(targets=None, crops=ok_c, flips=ok_f, jitter=ok_j)
        a.update(kw)
        with pytest.raises(ValueError):
            aug.augment_batch(imgs, a["targets"], a["crops"], a["flips"], a["jitter"], (28, 28))
    big = [np.zeros((40, 500, 3), np.uint8)]
    with pytest.raises(ValueError, match="15x"):
        aug.augment_batch(big, None, [(0, 0, 481, 40)], [0], None, (28, 32))      # 481 / 32 > 15: 33 taps
    assert pre._STAGE_BUSY is staged                                       # nothing was copied, so nothing was launched
    aug.augment_batch(big, None, [(0, 0, 480, 40)], [0], None, (28, 32))          # exactly 15x: 31 taps
    # the C entry point refuses the same bound by itself (DOD_ERR_INVALID), before it launches anything
    z = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rc = nat.lib().dod_preprocess_aug(nat.ptr(z), nat.ptr(z), nat.ptr(z), nat.ptr(z), 1, nat.ptr(z), nat.ptr(z), None, None, 40, 481, 28, 32,
                                      nat.ptr(z), nat.ptr(z), nat.ptr(z), nat.stream_ptr())
    assert rc == 1


# ------------------------------------------------------------------------------------------------------------- 5. run to run
def test_two_calls_give_equal_bytes(aug):
    c, _ = ac.case("all_differ")
    a = [aug.augment_batch(c["images"], None, c["crops"], c["flips"], c["jitter"], c["size"], as_uint8=u)[0].clone() for u in (False, True)]
    b = [aug.augment_batch(c["images"], None, c["crops"], c["flips"], c["jitter"], c["size"], as_uint8=u)[0] for u in (False, True)]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------- 6. a training step
def test_train_augment_feeds_a_training_step(aug):
    from dinov2_od_amd import losses as L
    from dinov2_od_amd.matching import HungarianMatcher
    from tests import aux_cases, cases, gpu_util as G
    bb, dc = cases.micro_bb(), aux_cases.micro_cfg()
    bb.target_dim, bb.layers = dc.hidden_dim, 3
    m = G.make_detector(bb, dc, "fp32").train()
    imgs = [ac._rand(s, 130 + i) for i, s in enumerate([(90, 120), (64, 64), (120, 80), (77, 101)])]
    # image 1's only box sits in the bottom right corner; the crop this seed draws for it (host-side, so the same everywhere) misses it
    rng = np.random.default_rng(0)
    targets = []
    for b in range(4):
        n = 1 if b == 1 else 3
        box = np.concatenate([rng.uniform(0.3, 0.7, (n, 2)), rng.uniform(0.1, 0.3, (n, 2))], 1).astype(np.float32)
        if b == 1:
            box[:] = (0.9, 0.9, 0.1, 0.1)
        targets.append({"boxes": torch.from_numpy(box), "labels": torch.from_numpy(rng.integers(1, dc.num_classes, n)),
                        "size": torch.as_tensor([56, 56])})
    t = aug.TrainAugment((56, 56), crop_prob=1.0, crop_frac=(0.5, 0.6), hflip_prob=0.5, brightness=0.4, contrast=0.4, saturation=0.4,
                         generator=torch.Generator().manual_seed(5), min_visibility=0.25)
    x, new = t(imgs, targets)
    assert x.shape == (4, 3, 56, 56) and x.dtype == torch.float32 and x.is_cuda and len(new) == 4
    assert [len(tg["boxes"]) for tg in new] == [3, 0, 3, 3] and new[1]["labels"].shape == (0,)
    for tg in new:
        assert tg["boxes"].shape[1:] == (4,) and tg["labels"].shape == (len(tg["boxes"]),) and tg["size"].tolist() == [56, 56]
    new = [{k: (v.cuda() if k in ("boxes", "labels") else v) for k, v in tg.items()} for tg in new]
    crit = L.SetCriterion(HungarianMatcher(), dc.num_classes, {"loss_ce": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0})
    ld = crit(m(x), new)
    loss = sum(ld.values())
    loss.backward()
    assert all(bool(torch.isfinite(v)) for v in ld.values()) and bool(torch.isfinite(loss))
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    assert float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads))) > 0.0
