"""Host side of the composed canvases (dinov2_od_amd/augment.py: compose_batch, compose_targets, sample_mosaic, sample_zoom_out,
TrainAugment's mosaic / zoom-out options): the numpy restatement against Pillow's paste chain, the argument checks, the float32 target
transform against its float64 evaluation, the samplers, the bindings."""
import os

import numpy as np
import pytest
import torch

from dinov2_od_amd import augment as aug
from tests import augment_cases as ac
from tests import compose_cases as cc


# ------------------------------------------------------------------------------------------ 1. the restatement against Pillow
@pytest.mark.parametrize("name", list(cc.CASES))
def test_restated_composition_is_bit_exact_against_pillow(name):
    c, want = cc.case(name)
    got = cc.pillow(name)
    assert got.shape == want.shape == (len(c["pieces"]), c["size"][0], c["size"][1], 3) and np.array_equal(got, want)


def test_the_cases_hold_what_they_are_for():
    c, want = cc.case("mosaic_edges")
    rects = [p[4] for p in c["pieces"][0]]
    assert (0, 0, 299, 1) in rects and (299, 1, 1, 55) in rects and c["size"] == (56, 300)
    assert sorted(max(aug._taps(p[1][2], p[4][2]), aug._taps(p[1][3], p[4][3])) for p in c["pieces"][0])[-1] == 31
    assert any(p[1][2] < p[4][2] and p[1][3] < p[4][3] for p in c["pieces"][0])                  # an upscaled piece
    c, want = cc.case("sixteen")
    assert [len(x) for x in c["pieces"]] == [16, 0, 1] and (want[1] == np.array(c["fill"], np.uint8)).all()
    c, want = cc.case("zoom_out")
    for n, fill in enumerate(c["fill"]):                                                         # the fill on all four sides
        dx, dy, dw, dh = c["pieces"][n][0][4]
        assert dx > 0 and dy > 0 and dx + dw < c["size"][1] and dy + dh < c["size"][0]
        for border in (want[n, :dy], want[n, dy + dh:], want[n, :, :dx], want[n, :, dx + dw:]):
            assert border.size and (border == np.array(fill, np.uint8)).all()
    c, want = cc.case("flip_inside")
    dx, dy, dw, dh = c["pieces"][0][0][4]
    inside = want[0, dy:dy + dh, dx:dx + dw, 0].astype(int)
    assert dx > 0 and (np.diff(inside, axis=1) <= 0).all() and inside[:, 0].min() > inside[:, -1].max()      # red falls left to right
    c, want = cc.case("abutting")                          # no gap: the fill's pure green appears nowhere
    assert not ((want[0] == np.array(c["fill"], np.uint8)).all(axis=-1)).any()
    c, want = cc.case("shared_source")                     # the same crop-independent factor 1.8 on a dark and on a mixed crop
    assert len(c["images"]) == 1 and len({p[3][1] for p in c["pieces"][0]}) >= 3


# ------------------------------------------------------------------------------------------------------- 2. the argument checks
def _ok():
    imgs = [ac._rand((40, 50), 300), ac._rand((30, 30), 301), ac._rand((20, 120), 302)]
    pieces = [[(0, (0, 0, 50, 40), False, None, (0, 0, 28, 28)), (1, (5, 5, 20, 20), True, (1.2, 0.8, 1.0), (28, 0, 28, 28))],
              [(2, (0, 0, 100, 20), False, None, (10, 10, 30, 20))]]
    return imgs, pieces


BAD_PIECES = {
    "overlapping dest rects": lambda p: p[0].__setitem__(1, (1, (5, 5, 20, 20), True, None, (27, 0, 28, 28))),
    "a rect beyond the right edge": lambda p: p[0].__setitem__(1, (1, (5, 5, 20, 20), True, None, (29, 0, 28, 28))),
    "a rect beyond the bottom edge": lambda p: p[1].__setitem__(0, (2, (0, 0, 100, 20), False, None, (10, 37, 30, 20))),
    "a rect at a negative offset": lambda p: p[1].__setitem__(0, (2, (0, 0, 100, 20), False, None, (-1, 10, 30, 20))),
    "an empty rect": lambda p: p[1].__setitem__(0, (2, (0, 0, 100, 20), False, None, (10, 10, 0, 20))),
    "a crop outside its source": lambda p: p[0].__setitem__(0, (0, (1, 0, 50, 40), False, None, (0, 0, 28, 28))),
    "a crop of another source's size": lambda p: p[0].__setitem__(1, (1, (0, 0, 50, 40), True, None, (28, 0, 28, 28))),
    "an empty crop": lambda p: p[0].__setitem__(0, (0, (0, 0, 0, 40), False, None, (0, 0, 28, 28))),
    "more than 16 pieces": lambda p: p.__setitem__(1, [(2, (0, 0, 100, 20), False, None, (3 * i, 0, 3, 20)) for i in range(17)]),
    # a 100-wide crop would pass for the 56-wide canvas (5 taps); in a 6-wide piece it needs ceil(100 / 6) * 2 + 1 = 35
    "more than 32 taps in a small piece": lambda p: p[1].__setitem__(0, (2, (0, 0, 100, 20), False, None, (10, 10, 6, 20))),
    "a source index past the batch": lambda p: p[1].__setitem__(0, (3, (0, 0, 10, 10), False, None, (10, 10, 30, 20))),
    "a negative source index": lambda p: p[1].__setitem__(0, (-1, (0, 0, 10, 10), False, None, (10, 10, 30, 20))),
    "a jitter of two factors": lambda p: p[0].__setitem__(1, (1, (5, 5, 20, 20), True, (1.0, 1.0), (28, 0, 28, 28))),
    "a negative jitter factor": lambda p: p[0].__setitem__(1, (1, (5, 5, 20, 20), True, (1.0, -0.1, 1.0), (28, 0, 28, 28))),
    "a jitter factor that is not finite": lambda p: p[0].__setitem__(1, (1, (5, 5, 20, 20), True, (1.0, 1.0, float("nan")), (28, 0, 28, 28))),
    "a fractional box": lambda p: p[0].__setitem__(0, (0, (0, 0, 49.5, 40), False, None, (0, 0, 28, 28))),
    "no piece at all": lambda p: (p.__setitem__(0, []), p.__setitem__(1, [])),
}


@pytest.mark.parametrize("what", list(BAD_PIECES))
def test_bad_pieces_raise_before_anything_is_staged(what):
    from dinov2_od_amd import preprocess as pre
    imgs, pieces = _ok()
    aug._check_pieces([im.shape[:2] for im in imgs], pieces, 56, 56)          # the good plan passes
    BAD_PIECES[what](pieces)
    staged = pre._STAGE_BUSY
    with pytest.raises(ValueError):
        aug.compose_batch(imgs, None, pieces, (56, 56))
    assert pre._STAGE_BUSY is staged


@pytest.mark.parametrize("kw", [dict(fill=(1, 2)), dict(fill=(1, 2, 256)), dict(fill=(-1, 2, 3)), dict(fill=(1.5, 2, 3)),
                                dict(fill=[(1, 2, 3)] * 3), dict(fill="grey"), dict(targets=[{}]), dict(targets=[{}, {}])])
def test_bad_fill_and_wrong_number_of_targets_raise_before_anything_is_staged(kw):
    from dinov2_od_amd import preprocess as pre
    imgs, pieces = _ok()
    staged = pre._STAGE_BUSY
    with pytest.raises(ValueError):
        aug.compose_batch(imgs, kw.get("targets"), pieces, (56, 56), **{k: v for k, v in kw.items() if k == "fill"})
    assert pre._STAGE_BUSY is staged
    assert aug._check_fill([(1, 2, 3), (4, 5, 6)], 2)[1] and not aug._check_fill((1, 2, 3), 2)[1]


# --------------------------------------------------------------------------------------------------- 3. the target transform
# Bound.  With u = 2^-24 (float32, round to nearest) a canvas corner  X = dx + x * dw / cw,  x = clamp((cx -+ bw / 2) * W - l),  carries:
# cx -+ bw / 2 within u (it is <= 1); times W within 2 W u; minus l within 3 W u (source pixels; the clamp and, when flipped, cw - x add
# at most cw u <= W u more: 4 W u).  Scaled into the canvas that is 4 (W / cw) dw u, the product and the quotient round by dw u each and
# the sum with dx by out_w u:  E <= u (4 (W / cw) dw + 2 dw + out_w) <= u out_w (4 W / cw + 3)  since dw <= out_w.  The centre
# (X1 + X2) / (2 out_w) is within E / out_w + 2 u, the width (X2 - X1) / out_w within 2 E / out_w + 2 u <= u (8 r + 8), r = max(W / cw,
# H / ch).  Every coordinate is held to that last figure.
def _bound(shape, crop):
    return 2.0 ** -24 * (8 * max(shape[1] / crop[2], shape[0] / crop[3]) + 8)


def _tg(boxes, first_label=0):
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    return {"boxes": torch.from_numpy(boxes.copy()), "labels": torch.arange(first_label, first_label + len(boxes), dtype=torch.int64)}


@pytest.mark.parametrize("mv", [0.0, 0.3])
def test_float32_targets_match_the_float64_evaluation_in_piece_order(mv):
    shapes = [(480, 640), (333, 500), (100, 80), (427, 640), (300, 400)]
    size = (224, 320)
    pieces = [[(0, (100, 50, 400, 300), False, None, (0, 0, 150, 100)), (1, (0, 0, 500, 333), True, None, (150, 0, 170, 100)),
               (2, (20, 0, 40, 100), False, None, (0, 100, 150, 124)), (3, (13, 200, 611, 227), True, None, (150, 100, 170, 124))],
              [],
              [(4, (50, 30, 300, 200), True, None, (40, 30, 200, 150))]]
    # every source is seen by one crop; its boxes are drawn away from that crop's keep thresholds (augment_cases.random_boxes)
    targets = [_tg(ac.random_boxes(25, 11 + p[0], shapes[p[0]], p[1], mv), 100 * p[0]) for p in pieces[0] + pieces[2]]
    got = aug.compose_targets(targets, shapes, pieces, size, mv)
    assert len(got) == 3 and got[1]["boxes"].shape == (0, 4) and got[1]["labels"].shape == (0,) and got[1]["labels"].dtype == torch.int64
    for n in (0, 2):
        want_boxes, want_labels, bounds = [], [], []
        for p in pieces[n]:
            keep, out, margins = cc.targets_f64(targets[p[0]]["boxes"].numpy(), shapes[p[0]], p, size, mv)
            assert (margins >= 1e-4).all()                 # no borderline box: the kept sets must agree exactly
            want_boxes.append(out); want_labels.append(targets[p[0]]["labels"].numpy()[keep]); bounds += [_bound(shapes[p[0]], p[1])] * len(out)
        want_boxes, want_labels = np.concatenate(want_boxes), np.concatenate(want_labels)
        assert got[n]["boxes"].dtype == torch.float32 and got[n]["boxes"].shape == want_boxes.shape and len(want_boxes) > 10
        assert got[n]["labels"].tolist() == want_labels.tolist()                       # same kept set, in piece order
        err = np.abs(got[n]["boxes"].numpy().astype(np.float64) - want_boxes).max(axis=1)
        assert (err <= np.array(bounds)).all(), (err / np.array(bounds)).max()


def test_boxes_are_clipped_at_quadrant_borders_and_dropped_outside():
    H, W = 100, 200
    size = (50, 80)

    def norm(x1, y1, x2, y2):
        return [(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H]
    # piece 0 shows the left half of the image in the canvas's left half, piece 1 the right half, mirrored, in the right half
    pieces = [[(0, (0, 0, 100, 100), False, None, (0, 0, 40, 50)), (0, (100, 0, 100, 100), True, None, (40, 0, 40, 50))]]
    tg = _tg([norm(80, 20, 120, 60),        # 0 straddles the border between the crops: clipped in both
              norm(10, 10, 50, 90),         # 1 wholly in the left crop
              norm(150, 40, 190, 80)])      # 2 wholly in the right crop
    tg.update(image_id=7, size=torch.as_tensor([H, W]), orig_size=torch.as_tensor([H, W]))
    got = aug.compose_targets([tg], [(H, W)], pieces, size)[0]
    assert got["labels"].tolist() == [0, 1, 0, 2]                                   # piece order, then box order
    want = np.array([[(32 + 40) / 2 / 80, 0.4, 8 / 80, 0.4],                       # x 80..100 -> 32..40
                     [(4 + 20) / 2 / 80, 0.5, 16 / 80, 0.8],
                     [(72 + 80) / 2 / 80, 0.4, 8 / 80, 0.4],                       # x 100..120 of the right crop, mirrored: 80..100 -> 72..80
                     [(44 + 60) / 2 / 80, 0.6, 16 / 80, 0.4]])                     # x 150..190 -> 50..90 -> mirrored 10..50 -> 44..60
    assert np.abs(got["boxes"].numpy() - want).max() <= 1e-6
    assert got["size"].tolist() == [50, 80] and got["image_id"] == 7 and got["orig_size"] is tg["orig_size"] and tg["size"].tolist() == [H, W]
    # min_visibility 0.6: the straddling box is half visible in each crop and goes
    got = aug.compose_targets([tg], [(H, W)], pieces, size, 0.6)[0]
    assert got["labels"].tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------------------ 4. the samplers
RAGGED = [(480, 640), (333, 500), (1, 1), (37, 1000), (2, 3), (224, 224), (840, 840), (900, 1300), (2000, 17)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


KW = dict(crop_prob=0.7, crop_frac=(0.3, 1.0), hflip_prob=0.4, brightness=0.4, contrast=0.5, saturation=0.2)


def test_the_same_seed_gives_the_same_plan():
    for fn in (aug.sample_mosaic, aug.sample_zoom_out):
        a, b, c = fn(RAGGED, _gen(3), (56, 72), **KW), fn(RAGGED, _gen(3), (56, 72), **KW), fn(RAGGED, _gen(4), (56, 72), **KW)
        assert a == b and a != c and len(a) == len(RAGGED)
    g = _gen(5)
    aug.sample_mosaic(RAGGED, g, (56, 72), **KW)
    h = _gen(5)
    aug.sample_mosaic(RAGGED, h, (56, 72), crop_prob=0.0, hflip_prob=1.0)      # other outcomes, the same count of numbers drawn
    assert torch.equal(g.get_state(), h.get_state())


def test_every_sampled_plan_is_valid_and_mosaics_tile_the_canvas():
    """a few hundred seeded draws on ragged shapes, down to 1 x 1 and up to sources that are more than 15x the canvas"""
    shapes_hw = [im for im in RAGGED]
    shrunk = 0
    for seed in range(40):
        for size in ((56, 56), (28, 300)):
            mosaic = aug.sample_mosaic(shapes_hw, _gen(seed), size, center=(0.0, 1.0), **KW)
            zoom = aug.sample_zoom_out(shapes_hw, _gen(seed), size, ratio=(1.0, 4.0), **KW)
            for plan in (mosaic, zoom):
                rows, offs, _ = aug._check_pieces(shapes_hw, plan, *size)          # compose_batch's own validation
                assert offs[-1] == len(rows)
            for n, canvas in enumerate(mosaic):
                assert len(canvas) == 4 and canvas[0][0] == n
                assert len({p[0] for p in canvas[1:]} | {n}) == 4                   # B >= 4: partners without replacement, never n
                cover = np.zeros(size, dtype=np.int32)
                for _, crop, _, _, (dx, dy, dw, dh) in canvas:
                    assert dw >= 1 and dh >= 1
                    cover[dy:dy + dh, dx:dx + dw] += 1
                assert (cover == 1).all()                                           # the quadrants tile the canvas exactly
                shrunk += sum(p[1][2] == 15 * p[4][2] or p[1][3] == 15 * p[4][3] for p in canvas)
            for n, canvas in enumerate(zoom):
                assert len(canvas) == 1 and canvas[0][0] == n
    assert shrunk > 0                                                               # the tap rule did engage


def test_small_batches_draw_partners_with_replacement():
    plan = aug.sample_mosaic(RAGGED[:2], _gen(0), (56, 56))
    assert all(len(c) == 4 and c[0][0] == n and all(0 <= p[0] < 2 for p in c) for n, c in enumerate(plan))
    aug._check_pieces(RAGGED[:2], plan, 56, 56)


def test_zoom_out_at_ratio_one_covers_the_canvas():
    plan = aug.sample_zoom_out(RAGGED, _gen(2), (56, 72), ratio=(1.0, 1.0), **KW)
    assert all(len(c) == 1 and c[0][4] == (0, 0, 72, 56) for c in plan)
    plan = aug.sample_zoom_out(RAGGED, _gen(2), (56, 72), ratio=(2.0, 2.0), **KW)
    assert all(c[0][4][2:] == (36, 28) and 0 <= c[0][4][0] <= 36 and 0 <= c[0][4][1] <= 28 for c in plan)
    assert len({c[0][4][:2] for c in plan}) > 3                                      # the offsets vary
    with pytest.raises(ValueError):
        aug.sample_zoom_out(RAGGED, _gen(2), (56, 72), ratio=(0.5, 2.0))
    with pytest.raises(ValueError):
        aug.sample_mosaic(RAGGED, _gen(2), (56, 72), center=(0.6, 0.4))


def test_train_augment_without_mosaic_or_zoom_out_is_the_call_it_was(monkeypatch):
    seen = {}
    monkeypatch.setattr(aug, "augment_batch", lambda *a: seen.setdefault("args", a) and ("batch", "targets"))
    monkeypatch.setattr(aug, "compose_batch", lambda *a, **k: pytest.fail("the composed path was taken"))
    imgs = [np.zeros((h, w, 3), np.uint8) for h, w in RAGGED]
    g = _gen(9)
    t = aug.TrainAugment((56, 72), generator=g, **KW)
    assert t.mosaic_prob == 0.0 and t.zoom_out_prob == 0.0 and t.fill == (124, 116, 104)
    t(imgs, None)
    h = _gen(9)
    crops, flips, jitter = aug.sample_params(RAGGED, h, **KW)
    a = seen["args"]
    assert np.array_equal(a[2], crops) and np.array_equal(a[3], flips) and np.array_equal(a[4], jitter) and a[5] == (56, 72)
    assert torch.equal(g.get_state(), h.get_state())                                # not one number more was drawn


def test_train_augment_mixes_the_three_kinds(monkeypatch):
    t = aug.TrainAugment((56, 72), generator=_gen(1), mosaic_prob=0.4, zoom_out_prob=0.5, zoom_out_ratio=(1.5, 3.0), **KW)
    plan = t.sample_plan(RAGGED * 4)
    aug._check_pieces(RAGGED * 4, plan, 56, 72)
    kinds = [4 if len(c) == 4 else (1 if c[0][4] == (0, 0, 72, 56) else 2) for c in plan]
    assert {1, 2, 4} == set(kinds)
    only = aug.TrainAugment((56, 72), generator=_gen(1), mosaic_prob=1.0).sample_plan(RAGGED)
    assert all(len(c) == 4 for c in only)
    with pytest.raises(ValueError):
        aug.TrainAugment(mosaic_prob=1.5)


# ---------------------------------------------------------------------------------------------------------------- 5. bindings
def test_bindings_resolve_and_the_abi_revision_stays():
    from dinov2_od_amd import _native as nat
    assert nat.ABI_VERSION == 7
    for name in ("dod_preprocess_compose", "dod_preprocess_compose_u8"):
        assert len(nat.SYMBOLS[name][1]) == 22
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dinodet.h")) as f:
        header = f.read()
    assert "#define DOD_ABI_VERSION 7" in header and "int dod_preprocess_compose(" in header and "int dod_preprocess_compose_u8(" in header
    if os.path.exists(nat.LIB_PATH):
        L = nat.lib()
        assert L.dod_abi_version() == 7
        assert L.dod_preprocess_compose.argtypes == nat.SYMBOLS["dod_preprocess_compose"][1] and L.dod_preprocess_compose_u8.restype is not None
