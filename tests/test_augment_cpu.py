"""Host side of the train-time augmentation (dinov2_od_amd/augment.py): the numpy restatement of the image chain against Pillow,
the float32 target transform against its float64 evaluation, the parameter sampler, the bindings."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import augment as aug
from tests import augment_cases as ac


# ------------------------------------------------------------------------------------------ 1. the restatement against Pillow
@pytest.mark.parametrize("name", list(ac.CASES))
def test_restated_chain_is_bit_exact_against_pillow(name):
    c, want = ac.case(name)
    for b, im in enumerate(c["images"]):
        got = ac.pillow_chain(im, c["crops"][b], c["flips"][b], None if c["jitter"] is None else c["jitter"][b], *c["size"])
        assert got.shape == want[b].shape and np.array_equal(got, want[b]), (name, b)


def test_each_enhancer_is_bit_exact_against_pillow():
    """every factor of FACTORS in every enhancer alone, on random, flat and hard-edged images"""
    from PIL import Image, ImageEnhance
    imgs = [ac._rand((19, 23), 7), ac._rand((8, 40), 8), ac._flat((9, 9), (3, 250, 128)), ac._hard((10, 11))]
    for im in imgs:
        for k, enh in enumerate((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)):
            for f in ac.FACTORS + (1.23, 1.4, 0.6):
                fs = [1.0, 1.0, 1.0]
                fs[k] = f
                want = np.array(enh(Image.fromarray(im)).enhance(float(np.float32(f))))
                assert np.array_equal(ac.jitter_u8(im, fs), want), (k, f)


# --------------------------------------------------------------------------------------------------- 2. the target transform
# The crops are at least a quarter of their image in each direction (the sampler's default is a half): a float32 pixel coordinate
# cx * W carries about 3 roundings of 2^-24 relative, i.e. (W / width) * 3 * 6e-8 once normalised by the crop -- within the 1e-6 bound
# up to W / width of about 5.  (A 1-pixel-wide crop of an 80-pixel image is at 3e-6 in float32 whatever the order of operations.)
TARGET_CASES = [  # (H, W), crop, flip, min_visibility
    ((480, 640), (100, 50, 400, 300), False, 0.0),
    ((480, 640), (100, 50, 400, 300), True, 0.3),
    ((333, 500), (0, 0, 500, 333), True, 0.0),
    ((100, 80), (20, 0, 40, 100), False, 0.0),
    ((427, 640), (13, 200, 611, 227), True, 0.5),
]


def _tg(boxes, n_classes=11):
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return {"boxes": torch.from_numpy(boxes.copy()), "labels": torch.arange(len(boxes), dtype=torch.int64) % n_classes}


@pytest.mark.parametrize("shape,crop,flip,mv", TARGET_CASES)
def test_float32_targets_match_the_float64_evaluation(shape, crop, flip, mv):
    boxes = ac.random_boxes(40, 5, shape, crop, mv)
    keep, want, margins = ac.targets_f64(boxes, shape, crop, flip, mv)
    assert (margins >= 1e-4).all()                       # no borderline box: the kept sets must agree exactly
    tg = _tg(boxes)
    got = aug.transform_targets([tg], [shape], [crop], [flip], (56, 56), mv)[0]
    assert got["boxes"].dtype == torch.float32 and got["labels"].dtype == torch.int64
    assert torch.equal(got["labels"], tg["labels"][torch.from_numpy(keep)])          # same kept set, order preserved
    assert got["boxes"].shape == (int(keep.sum()), 4)
    assert np.abs(got["boxes"].numpy().astype(np.float64) - want).max(initial=0.0) <= 1e-6


def test_each_keep_rule_by_construction():
    H, W, crop = 400, 600, (150, 100, 300, 200)           # the crop spans x 150..450, y 100..300

    def norm(x1, y1, x2, y2):
        return [(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H]
    boxes = [norm(10, 10, 100, 90),            # 0 entirely outside the crop
             norm(100, 150, 150.2, 250),       # 1 clipped to a 0.2-pixel sliver: 0.2 / 300 < 0.001
             norm(50, 150, 190, 250),          # 2 40 of 140 pixels visible: 0.29 < min_visibility 0.5
             norm(120, 150, 200, 250),         # 3 straddles the left edge, 50 of 80 visible
             norm(400, 150, 480, 250),         # 4 straddles the right edge, 50 of 80
             norm(200, 60, 300, 160),          # 5 straddles the top edge, 60 of 100
             norm(200, 240, 300, 340),         # 6 straddles the bottom edge, 60 of 100
             norm(250, 150, 350, 250)]         # 7 untouched
    tg = _tg(boxes)
    got = aug.transform_targets([tg], [(H, W)], [crop], [False], (56, 56), 0.5)[0]
    assert got["labels"].tolist() == [3, 4, 5, 6, 7]
    want = np.array([[25 / 300, 0.5, 50 / 300, 0.5], [275 / 300, 0.5, 50 / 300, 0.5], [1 / 3, 30 / 200, 100 / 300, 60 / 200],
                     [1 / 3, 170 / 200, 100 / 300, 60 / 200], [0.5, 0.5, 100 / 300, 0.5]])
    assert np.abs(got["boxes"].numpy() - want).max() <= 1e-6
    keep, w64, _ = ac.targets_f64(np.array(boxes, dtype=np.float32), (H, W), crop, False, 0.5)
    assert keep.tolist() == [False, False, False, True, True, True, True, True]
    # without the visibility rule the 40-of-140 box stays; flipped, left and right swap
    got = aug.transform_targets([tg], [(H, W)], [crop], [True], (56, 56), 0.0)[0]
    assert got["labels"].tolist() == [2, 3, 4, 5, 6, 7]
    assert np.abs(got["boxes"].numpy()[1] - np.array([275 / 300, 0.5, 50 / 300, 0.5])).max() <= 1e-6


def test_flip_is_an_involution_and_the_identity_passes_tensors_through():
    H, W = 333, 500
    full = (0, 0, W, H)
    tg = _tg(ac.random_boxes(12, 9, (H, W), full, 0.0))
    tg.update(image_id=7, size=torch.as_tensor([H, W]), orig_size=torch.as_tensor([H, W]), area=torch.arange(5), filename="x.jpg")
    once = aug.transform_targets([tg], [(H, W)], [full], [True], (56, 64))[0]
    twice = aug.transform_targets([once], [(H, W)], [full], [True], (56, 64))[0]
    assert len(once["boxes"]) == 12 and not torch.equal(once["boxes"], tg["boxes"])
    assert (twice["boxes"] - tg["boxes"]).abs().max() <= 1e-6 and torch.equal(twice["labels"], tg["labels"])
    same = aug.transform_targets([tg], [(H, W)], [full], [False], (56, 64))[0]
    assert torch.equal(same["boxes"], tg["boxes"]) and torch.equal(same["labels"], tg["labels"])
    # size becomes the output size; every other key is passed through untouched
    assert same["size"].tolist() == [56, 64] and once["size"].tolist() == [56, 64] and same["size"].dtype == tg["size"].dtype
    for k in ("image_id", "orig_size", "area", "filename"):
        assert once[k] is tg[k] and same[k] is tg[k]
    assert tg["size"].tolist() == [H, W]                   # the input dict is not modified


def test_zero_boxes_in_and_out():
    empty = {"boxes": torch.zeros((0, 4)), "labels": torch.zeros((0,), dtype=torch.int64)}
    got = aug.transform_targets([empty], [(50, 60)], [(5, 5, 20, 20)], [True], (56, 56))[0]
    assert got["boxes"].shape == (0, 4) and got["labels"].shape == (0,) and got["labels"].dtype == torch.int64
    far = _tg([[0.9, 0.9, 0.1, 0.1]])
    got = aug.transform_targets([far], [(50, 60)], [(5, 5, 20, 20)], [False], (56, 56))[0]
    assert got["boxes"].shape == (0, 4) and got["boxes"].dtype == torch.float32 and got["labels"].shape == (0,)


# ----------------------------------------------------------------------------------------------------------- 3. sample_params
SHAPES = [(480, 640), (333, 500), (1, 1), (37, 1000), (2, 3), (224, 224)] * 20


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sample_params_is_seeded_and_stays_inside():
    kw = dict(crop_prob=0.7, crop_frac=(0.3, 0.9), hflip_prob=0.4, brightness=0.4, contrast=1.5, saturation=0.2)
    a = aug.sample_params(SHAPES, _gen(3), **kw)
    b = aug.sample_params(SHAPES, _gen(3), **kw)
    c = aug.sample_params(SHAPES, _gen(4), **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
    crops, flips, jitter = a
    assert crops.dtype == np.int32 and crops.shape == (len(SHAPES), 4) and flips.dtype == np.uint8 and jitter.dtype == np.float32
    full = 0
    for (H, W), (l, t, w, h) in zip(SHAPES, crops.tolist()):
        assert w >= 1 and h >= 1 and l >= 0 and t >= 0 and l + w <= W and t + h <= H
        if (l, t, w, h) == (0, 0, W, H):
            full += 1
        else:
            assert int(np.ceil(0.3 * W)) <= w <= max(1, int(np.floor(0.9 * W))) and int(np.ceil(0.3 * H)) <= h <= max(1, int(np.floor(0.9 * H)))
    assert 0 < full < len(SHAPES) and 0 < int(flips.sum()) < len(SHAPES) and set(flips.tolist()) <= {0, 1}
    j = jitter.astype(np.float64)
    for k, x in enumerate((0.4, 1.5, 0.2)):
        assert (j[:, k] >= max(0.0, 1.0 - x)).all() and (j[:, k] <= 1.0 + x).all() and j[:, k].std() > 0
    assert len({tuple(r) for r in crops.tolist()}) > 20           # offsets and sizes do vary


def test_sample_params_probabilities_and_zero_ranges():
    never = aug.sample_params(SHAPES, _gen(1), crop_prob=0.0, hflip_prob=0.0)
    assert all((l, t, w, h) == (0, 0, W, H) for (H, W), (l, t, w, h) in zip(SHAPES, never[0].tolist())) and not never[1].any()
    assert (never[2] == np.float32(1.0)).all()                    # zero ranges: exactly 1.0
    always = aug.sample_params(SHAPES, _gen(1), crop_prob=1.0, crop_frac=(0.5, 0.5), hflip_prob=1.0, contrast=0.3)
    assert always[1].all()
    for (H, W), (l, t, w, h) in zip(SHAPES, always[0].tolist()):
        assert w == max(1, int(np.ceil(0.5 * W))) and h == max(1, int(np.ceil(0.5 * H)))
    assert (always[2][:, 0] == 1.0).all() and (always[2][:, 2] == 1.0).all() and (always[2][:, 1] != 1.0).any()


def test_collate_raw_stacks_nothing():
    batch = [(np.zeros((4, 5, 3), np.uint8), {"labels": torch.zeros(0)}), (np.zeros((7, 2, 3), np.uint8), {"labels": torch.ones(2)})]
    images, targets = aug.collate_raw(batch)
    assert isinstance(images, list) and isinstance(targets, list) and images[1] is batch[1][0] and targets[0] is batch[0][1]


# ---------------------------------------------------------------------------------------------------------------- 4. bindings
def test_bindings_resolve_and_the_abi_revision_stays():
    import os
    from dinov2_od_amd import _native as nat
    assert nat.ABI_VERSION == 7 and len(nat.SYMBOLS["dod_preprocess_aug"][1]) == 17 and len(nat.SYMBOLS["dod_preprocess_aug_u8"][1]) == 17
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dinodet.h")) as f:
        header = f.read()
    assert "#define DOD_ABI_VERSION 7" in header and "int dod_preprocess_aug(" in header and "int dod_preprocess_aug_u8(" in header
    if os.path.exists(nat.LIB_PATH):
        L = nat.lib()
        assert L.dod_abi_version() == 7
        assert L.dod_preprocess_aug.argtypes == nat.SYMBOLS["dod_preprocess_aug"][1] and L.dod_preprocess_aug_u8.restype is not None
