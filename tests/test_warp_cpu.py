"""CPU checks of the geometric warp (dinov2_od_amd/augment.py warp_batch and its helpers): the numpy restatement of Pillow's
Image.transform(PERSPECTIVE, BILINEAR, fillcolor) that serves as the GPU test's oracle is pinned against Pillow itself on every case of
tests/warp_cases.py, contraction probes included; the coefficient builders, the argument check, the target transform and the samplers
are pure host code and are tested here in full.  No GPU."""
import math

import numpy as np
import pytest
import torch

from dinov2_od_amd import augment as aug
from tests import augment_cases as ac
from tests import warp_cases as wc


# ------------------------------------------------------------------------------------------------ 1. the restatement is Pillow's
@pytest.mark.parametrize("name", list(wc.CASES))
def test_restatement_equals_pillow_bit_for_bit(name):
    c, want = wc.case(name)
    for b, im in enumerate(c["images"]):
        pil = wc.pillow_warp(im, c["coeffs"][b], *c["size"], wc._fill_of(c["fill"], b))
        assert np.array_equal(want[b], pil), (name, b, int((want[b] != pil).sum()))
        if c["coeffs"][b][6] == 0.0 and c["coeffs"][b][7] == 0.0:       # an affine through PERSPECTIVE gives AFFINE's bytes
            assert np.array_equal(pil, wc.pillow_warp(im, c["coeffs"][b], *c["size"], wc._fill_of(c["fill"], b), method="AFFINE")), (name, b)


def test_cases_do_what_their_names_say():
    img = wc.case("identity")[0]["images"][0]
    assert np.array_equal(wc.case("identity")[1][0], img)
    assert np.array_equal(wc.case("mirror")[1][0], img[:, ::-1])
    assert np.array_equal(wc.case("transpose")[1][0], img.transpose(1, 0, 2))
    t = wc.case("translate_int")[1][0]
    assert np.array_equal(t[2:, :10], img[:7, 3:]) and (t[:2] == (1, 2, 3)).all() and (t[:, 10:] == (1, 2, 3)).all()
    c, w = wc.case("all_fill")
    assert (w == np.array(c["fill"], dtype=np.uint8)).all()
    c, w = wc.case("partly_outside")
    for b in range(2):
        is_fill = (w[b] == np.array(c["fill"][b], dtype=np.uint8)).all(-1)
        assert 0.1 < is_fill.mean() < 0.9, (b, is_fill.mean())
    # boundary: sx == 0.0 is inside (pixel (0, 0) of image 0 is the clamped source pixel (0, 0); column 0 and row 0 are samples), sx == W
    # is the fill (its last column and row)
    c, w = wc.case("boundary")
    img = c["images"][0]
    assert np.array_equal(w[0][0, 0], img[0, 0]) and not (w[0][:9, :13] == (255, 0, 255)).all(-1).any()
    assert (w[0][:, 13] == (255, 0, 255)).all() and (w[0][9] == (255, 0, 255)).all()
    assert not (w[1][8, :12] == (255, 0, 255)).all(-1).any()            # the iy + 1 == H row is sampled, not filled
    for name in ("two_tiles_wide", "two_tiles_tall", "rotate30", "scale_up", "thin"):
        c, w = wc.case(name)
        assert ((w != np.array(c["fill"], dtype=np.uint8)).any(-1)).mean() > 0.2, name


def test_fma_probes_tell_a_contracted_lerp_from_pillows():
    """on the probe pixels a lerp rounded once (as a fused multiply-add rounds it) gives another byte than Pillow's two roundings: a
    kernel compiled with contraction cannot pass the case"""
    c, want = wc.case("fma_probe")
    for b, (im, byte, fused_byte) in enumerate(zip(c["images"], (12, 49), (11, 48))):
        fill = wc._fill_of(c["fill"], b)
        plain = wc.restated_pixel(im, c["coeffs"][b], 0, 0, fill)
        fused = wc.restated_pixel(im, c["coeffs"][b], 0, 0, fill, fused=True)
        assert plain == (byte,) * 3 == tuple(int(v) for v in want[b, 0, 0]), (b, plain)
        assert fused == (fused_byte,) * 3 and fused != plain, (b, fused)
        assert tuple(int(v) for v in wc.pillow_warp(im, c["coeffs"][b], 1, 1, fill)[0, 0]) == plain
    # the coordinate sums: with either product of a0 xin + a1 yin contracted into the sum the probe pixel is 207, Pillow writes 206
    c, want = wc.case("fma_coord_probe")
    im, cf = c["images"][0], c["coeffs"][0]
    assert wc.restated_pixel(im, cf, 1, 1, c["fill"]) == (206,) * 3 == tuple(int(v) for v in want[0, 1, 1])
    assert wc.restated_pixel(im, cf, 1, 1, c["fill"], fused_coords=1) == (207,) * 3 == wc.restated_pixel(im, cf, 1, 1, c["fill"], fused_coords=2)
    assert tuple(int(v) for v in wc.pillow_warp(im, cf, 2, 2, c["fill"])[1, 1]) == (206,) * 3
    # the scalar restatement is the vectorised one elsewhere too
    c, want = wc.case("perspective")
    for b in range(2):
        for x, y in [(0, 0), (17, 30), (55, 55), (40, 3)]:
            assert wc.restated_pixel(c["images"][b], c["coeffs"][b], x, y, c["fill"]) == tuple(int(v) for v in want[b, y, x])


# ---------------------------------------------------------------------------------------------------- 2. coefficient builders
def _apply(coeffs, X, Y):
    a = coeffs
    den = a[6] * X + a[7] * Y + 1.0
    return (a[0] * X + a[1] * Y + a[2]) / den, (a[3] * X + a[4] * Y + a[5]) / den


def test_affine_coeffs_invert_the_forward_map():
    rng = np.random.default_rng(0)
    for angle, translate, scale, shear, src, out, center in [(30.0, (0.0, 0.0), 1.0, 0.0, (40, 50), (56, 56), None),
                                                             (-75.0, (5.0, -3.0), 0.6, 12.0, (33, 90), (224, 224), None),
                                                             (170.0, (-20.0, 8.0), 2.5, (8.0, -6.0), (480, 640), (518, 518), None),
                                                             (10.0, (0.0, 0.0), 1.3, 0.0, (60, 60), (60, 60), (12.5, 40.0))]:
        c = aug.affine_coeffs(src, out, angle, translate, scale, shear, center)
        assert c.shape == (8,) and c.dtype == np.float64 and c[6] == 0.0 and c[7] == 0.0
        # the forward map, written out: p_out = c_out + t + R . ShY . ShX . s (p_src - c_src)
        r = math.radians(angle)
        sx, sy = (shear, 0.0) if np.isscalar(shear) else shear
        cs = np.array([src[1] / 2, src[0] / 2]) if center is None else np.array(center)
        for u, v in rng.uniform(0, 1, (8, 2)) * (src[1], src[0]):
            p = scale * (np.array([u, v]) - cs)
            p = np.array([p[0] - math.tan(math.radians(sx)) * p[1], p[1]])
            p = np.array([p[0], p[1] - math.tan(math.radians(sy)) * p[0]])
            p = np.array([math.cos(r) * p[0] - math.sin(r) * p[1], math.sin(r) * p[0] + math.cos(r) * p[1]])
            X, Y = p + (out[1] / 2 + translate[0], out[0] / 2 + translate[1])
            bu, bv = _apply(c, X, Y)
            assert abs(bu - u) <= 1e-9 and abs(bv - v) <= 1e-9, (angle, u, v, bu, bv)
    # a positive angle turns the picture clockwise on the screen: the source's top middle is shown right of the centre
    X, Y = wc.forward_point(aug.affine_coeffs((40, 40), (40, 40), 90.0), 20.0, 0.0)
    assert abs(X - 40.0) < 1e-9 and abs(Y - 20.0) < 1e-9
    assert tuple(aug.affine_coeffs((40, 50), (40, 50)).tolist()) == aug.IDENTITY_COEFFS
    with pytest.raises(ValueError):
        aug.affine_coeffs((40, 50), (40, 50), scale=0.0)


def test_perspective_coeffs_show_each_source_point_at_its_output_point():
    src = [(0.0, 0.0), (50.0, 0.0), (50.0, 40.0), (0.0, 40.0)]
    dst = [(4.0, 2.5), (49.5, 5.0), (54.5, 53.0), (2.0, 48.5)]
    c = aug.perspective_coeffs(src, dst)
    assert c.shape == (8,) and c.dtype == np.float64 and (c[6] != 0.0 or c[7] != 0.0)
    for (u, v), (X, Y) in zip(src, dst):
        bu, bv = _apply(c, X, Y)
        assert abs(bu - u) <= 1e-9 and abs(bv - v) <= 1e-9
        fx, fy = wc.forward_point(c, u, v)
        assert abs(fx - X) <= 1e-9 and abs(fy - Y) <= 1e-9
    assert np.allclose(c, wc.quad_coeffs(src, dst), rtol=0, atol=1e-12)
    # corners onto corners is the identity; four points of which three are on a line determine nothing
    assert np.allclose(aug.perspective_coeffs(src, src), aug.IDENTITY_COEFFS, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        aug.perspective_coeffs(src, [(0.0, 0.0), (10.0, 10.0), (20.0, 20.0), (30.0, 30.0)])


def test_compose_coeffs_is_one_warp_after_the_other():
    a = aug.affine_coeffs((40, 50), (56, 56), 25.0, (3.0, 1.0), 0.8, 5.0)
    p = aug.perspective_coeffs([(0, 0), (56, 0), (56, 56), (0, 56)], [(4.0, 2.5), (49.5, 5.0), (54.5, 53.0), (2.0, 48.5)])
    c = aug.compose_coeffs(a, p)
    assert c.shape == (8,)
    for X, Y in [(0.5, 0.5), (55.5, 0.5), (20.0, 33.0), (55.5, 55.5)]:
        mid = _apply(p, X, Y)                     # output -> the intermediate image
        want = _apply(a, *mid)                    # -> the source
        got = _apply(c, X, Y)
        assert abs(got[0] - want[0]) <= 1e-9 and abs(got[1] - want[1]) <= 1e-9
    ident = np.array(aug.IDENTITY_COEFFS)
    assert np.array_equal(aug.compose_coeffs(a, ident), a) and np.array_equal(aug.compose_coeffs(ident, p), p)      # bit for bit
    both = aug.compose_coeffs(np.stack([a, ident]), np.stack([p, p]))
    assert both.shape == (2, 8) and np.array_equal(both[0], c) and np.array_equal(both[1], p)


# ------------------------------------------------------------------------------------------------------------ 3. _check_coeffs
def test_check_coeffs_refuses_what_the_kernel_or_the_boxes_must_not_see():
    shapes, ident = [(40, 50), (40, 50)], np.array(aug.IDENTITY_COEFFS)
    good = np.stack([ident, aug.affine_coeffs((40, 50), (56, 56), 30.0)])
    out = aug._check_coeffs(good.tolist(), shapes, 56, 56)
    assert out.dtype == np.float64 and out.shape == (2, 8) and out.flags["C_CONTIGUOUS"] and np.array_equal(out, good)

    def bad(row, shapes=shapes, size=(56, 56)):
        c = good.copy()
        c[1] = row
        with pytest.raises(ValueError):
            aug._check_coeffs(c, shapes, *size)
    for wrong in (good[:1], good[:, :6], good.reshape(-1), np.zeros((2, 9))):        # a wrong shape
        with pytest.raises(ValueError):
            aug._check_coeffs(wrong, shapes, 56, 56)
    bad([1, 0, float("nan"), 0, 1, 0, 0, 0])                                              # a NaN
    bad([1, 0, 0, 0, float("inf"), 0, 0, 0])
    bad([1, 0, 2e9, 0, 1, 0, 0, 0])                                                       # beyond 1e9
    bad([1, 2, 0, 2, 4, 0, 0, 0])                                                         # a singular matrix
    bad([0, 0, 5, 0, 0, 5, 0, 0])
    bad([1, 0, 0, 0, 1, 0, -1.0 / 28, 0])                                                 # the horizon inside the output: den = 0 at x = 28
    bad([1, 0, 0, 0, 1, 0, 0, -1.0 / 55.5])                                               # den = 0 exactly at the last pixel centre
    bad([1, 2, 0, 2, 4 + 1e-12, 0, 0, 0])                                                 # singular to working precision
    # badly scaled but sound maps pass: the verdict is a condition number in unit-square coordinates, not an absolute residual
    for row, shape in (([100, 0, 3000, 0, 100, 2000, 0, 0], (4000, 6000)),               # a 56 x 56 window of a large source, 100x down
                       ([1e-3, 0, 25, 0, 1e-3, 20, 0, 0], (40, 50)),                      # 1000x up
                       ([1, 0, 1e6, 0, 1, -1e6, 0, 0], (40, 50)),                         # a million pixels off: all fill, but a map
                       ([3e-3, 4e-3, 1e5, -4e-3, 3e-3, -1e5, 0, 0], (40, 50))):           # a tiny scale and a large offset together
        aug._check_coeffs(np.stack([ident, np.array(row, dtype=np.float64)]), [(40, 50), shape], 56, 56)
    # a horizon outside the output but inside the source: den > 0 on all of the 56 x 56 output, but the forward map's third component
    # changes sign between the source's corners
    c = np.array([1, 0, 0, 0, 1, 0, 0.01, 0], dtype=np.float64)       # sx = x / (0.01 x + 1) < 100 for every x: column 100 is the horizon
    aug._check_coeffs(np.stack([ident, c]), [(40, 50), (40, 90)], 56, 56)
    bad(c, shapes=[(40, 50), (40, 120)])
    bad(c, shapes=[(40, 50), (40, 100)])                                                  # a corner exactly on it


# ------------------------------------------------------------------------------------------------------------------ 4. targets
@pytest.mark.parametrize("case", wc.target_cases(), ids=lambda c: c[0])
def test_warp_targets_equals_the_float64_transform(case):
    name, shape, coeffs, size, vis = case
    boxes = wc.random_boxes(40, 7, shape, coeffs, size, vis)
    keep, want, margins = wc.targets_f64(boxes, shape, coeffs, size, vis)
    assert (margins >= 1e-4).all()
    if name != "clipped_all_kept":
        assert 0 < keep.sum() < len(keep), (name, keep.sum())
    labels = torch.arange(len(boxes))
    for dtype, tol in ((torch.float32, 2.4e-7), (torch.float64, 1e-12)):      # two float32 ulps at 1.0: one rounding apart after the cast
        tg = {"boxes": torch.from_numpy(boxes).to(dtype), "labels": labels, "size": torch.as_tensor([shape[0], shape[1]]), "image_id": 17}
        (new,) = aug.warp_targets([tg], [shape], coeffs[None], size, vis)
        assert new["boxes"].dtype == dtype and new["boxes"].shape == (int(keep.sum()), 4)
        assert torch.equal(new["labels"], labels[torch.from_numpy(keep)])
        assert new["size"].tolist() == list(size) and new["image_id"] == 17
        assert np.abs(new["boxes"].numpy().astype(np.float64) - want).max() <= tol, name
        assert tg["boxes"].shape == (40, 4)                                   # the input is left alone
    # a rotated box's bounding box grows
    if name == "rotate":
        tg = {"boxes": torch.tensor([[0.5, 0.5, 0.2, 0.2]], dtype=torch.float64)}
        (new,) = aug.warp_targets([tg], [shape], coeffs[None], size)
        w, h = 1.7 * 0.2 * 50, 1.7 * 0.2 * 40          # the case scales by 1.7
        c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
        assert np.allclose(new["boxes"][0, 2:].numpy() * 56, [w * c + h * s, w * s + h * c], rtol=0, atol=1e-9)


def test_identity_warp_passes_boxes_through():
    boxes, labels = torch.rand(5, 4), torch.arange(5)
    tg = {"boxes": boxes, "labels": labels, "size": torch.as_tensor([40, 50])}
    (new,) = aug.warp_targets([tg], [(40, 50)], np.array([aug.IDENTITY_COEFFS]), (40, 50))
    assert new["boxes"] is boxes and new["labels"] is labels
    (new,) = aug.warp_targets([tg], [(40, 50)], np.array([aug.IDENTITY_COEFFS]), (40, 56))      # another size: not the identity
    assert new["boxes"] is not boxes and new["size"].tolist() == [40, 56]


# ----------------------------------------------------------------------------------------------------------------- 5. samplers
def _state_after(n, seed=11):
    g = torch.Generator().manual_seed(seed)
    if n:
        torch.rand(n, generator=g, dtype=torch.float64)
    return g.get_state()


def test_samplers_draw_a_fixed_count_of_numbers_per_image():
    shapes = [(40, 50), (33, 90), (56, 56)]
    for kw in (dict(), dict(degrees=15.0, translate=(0.1, 0.2), scale=(0.8, 1.2), shear=10.0), dict(degrees=(-5, 40), shear=(0, 5, -3, 3), prob=0.5),
               dict(degrees=15.0, prob=0.0), dict(degrees=15.0, size=(64, 48))):
        g = torch.Generator().manual_seed(11)
        c = aug.sample_affine(shapes, g, **kw)
        assert c.shape == (3, 8) and c.dtype == np.float64 and (c[:, 6:] == 0).all()
        assert torch.equal(g.get_state(), _state_after(7 * 3)), kw
        for b, shape in enumerate(shapes):
            aug._check_coeffs(c[b:b + 1], [shape], *kw.get("size", shape))
    for kw in (dict(distortion=0.0), dict(distortion=0.5), dict(distortion=0.9, prob=0.5), dict(distortion=0.5, prob=0.0), dict(distortion=0.3, size=(64, 48))):
        g = torch.Generator().manual_seed(11)
        c = aug.sample_perspective(shapes, g, **kw)
        assert c.shape == (3, 8) and c.dtype == np.float64
        assert torch.equal(g.get_state(), _state_after(9 * 3)), kw
        for b, shape in enumerate(shapes):                       # size = None: every image at its own size
            aug._check_coeffs(c[b:b + 1], [shape], *kw.get("size", shape))
    # the parameter meanings: the angle within its range; not drawn = the identity; every corner moves inward by at most d x half a side
    g = torch.Generator().manual_seed(3)
    c = aug.sample_affine([(56, 56)] * 200, g, degrees=15.0, scale=(0.5, 2.0))
    ang = np.degrees(np.arctan2(-c[:, 1], c[:, 0]))          # the inverse rotates by -angle
    s = 1.0 / np.hypot(c[:, 0], c[:, 1])
    assert np.abs(ang).max() <= 15.0 + 1e-9 and np.abs(ang).max() > 10.0 and s.min() >= 0.5 - 1e-9 and s.max() <= 2.0 + 1e-9 and s.max() > 1.5
    assert (aug.sample_affine([(56, 56)] * 4, g, degrees=15.0, prob=0.0) == np.array(aug.IDENTITY_COEFFS)).all()
    assert (aug.sample_perspective([(56, 56)] * 4, g, 0.5, prob=0.0) == np.array(aug.IDENTITY_COEFFS)).all()
    c = aug.sample_perspective([(40, 50)] * 50, g, 0.5)
    for row in c:
        for (u, v), (X0, Y0) in zip([(0, 0), (50, 0), (50, 40), (0, 40)], [(0, 0), (50, 0), (50, 40), (0, 40)]):
            X, Y = wc.forward_point(row, u, v)
            assert abs(X - X0) <= 0.5 * 25 + 1e-9 and abs(Y - Y0) <= 0.5 * 20 + 1e-9 and -1e-9 <= X <= 50 + 1e-9 and -1e-9 <= Y <= 40 + 1e-9
    for bad in (dict(degrees=-1.0), dict(scale=(0.0, 1.0)), dict(translate=(2.0, 0.0)), dict(prob=1.5)):
        with pytest.raises(ValueError):
            aug.sample_affine(shapes, g, **bad)
    with pytest.raises(ValueError):
        aug.sample_perspective(shapes, g, 1.0)


STRONG = [dict(degrees=30.0, translate=(0.2, 0.2), scale=(1.0, 2.0), shear=5.0, distortion=0.6),
          dict(degrees=30.0, translate=(0.2, 0.2), scale=(1.5, 2.0), shear=5.0, distortion=0.9),
          dict(degrees=180.0, translate=(1.0, 1.0), scale=(0.01, 100.0), shear=(-80.0, 80.0, -80.0, 80.0), distortion=0.99),
          dict(degrees=180.0, translate=(0.5, 0.0), scale=(20.0, 100.0), shear=60.0, distortion=0.99),
          dict(degrees=45.0, translate=(0.0, 1.0), scale=(0.01, 0.05), shear=(0.0, 0.0, -80.0, 80.0), distortion=0.5)]


@pytest.mark.parametrize("kw", STRONG, ids=lambda kw: f"d{kw['degrees']:g}-s{kw['scale'][1]:g}-p{kw['distortion']:g}")
@pytest.mark.parametrize("size", [(224, 224), (56, 300)])
def test_every_composed_draw_is_one_warp_batch_accepts(kw, size):
    """`TrainAugment.sample_warp` at strong parameters, up to the limits of every range, over 60 batches of 64: the composition of the
    affine and the perspective passes `_check_coeffs` for every image (a refusal here would be a ValueError in the middle of
    training); so does every affine and every perspective alone; and 16 numbers per image are drawn whatever had to be halved"""
    g = torch.Generator().manual_seed(123)
    t = aug.TrainAugment(size, generator=g, affine_prob=1.0, perspective_prob=1.0, **kw)
    shapes = [size] * 64
    for _ in range(60):
        aug._check_coeffs(t.sample_warp(64), shapes, *size)
    assert torch.equal(g.get_state(), _state_after(60 * 64 * 16, seed=123))
    affine = {k: v for k, v in kw.items() if k != "distortion"}
    for _ in range(10):
        aug._check_coeffs(aug.sample_affine(shapes, g, **affine), shapes, *size)
        aug._check_coeffs(aug.sample_perspective(shapes, g, kw["distortion"]), shapes, *size)
    # the halving leaves the perspective in place where it can: most images of a strong batch still have one
    c = t.sample_warp(64)
    assert ((c[:, 6] != 0) | (c[:, 7] != 0)).mean() > 0.5
    # ranges beyond the limits are refused when the transform is built, not at some batch
    for bad in (dict(scale=(0.001, 1.0)), dict(scale=(1.0, 1000.0)), dict(shear=85.0), dict(distortion=1.0), dict(degrees=-3.0)):
        with pytest.raises(ValueError):
            aug.TrainAugment(size, affine_prob=0.5, **bad)


def test_train_augment_without_a_warp_consumes_the_generator_as_before(monkeypatch):
    """with affine_prob = perspective_prob = 0 a call draws what `sample_params` / `sample_plan` draw and nothing more, and launches
    what it launched: `warp_batch` is not reached (the launch entry points are stubbed: no GPU here)"""
    imgs = [ac._rand(s, 600 + i) for i, s in enumerate([(40, 50), (33, 90), (56, 56)])]
    shapes = [im.shape[:2] for im in imgs]
    calls = []
    monkeypatch.setattr(aug, "augment_batch", lambda *a, **k: calls.append("augment") or ("batch", None))
    monkeypatch.setattr(aug, "compose_batch", lambda *a, **k: calls.append("compose") or ("batch", None))
    monkeypatch.setattr(aug, "warp_batch", lambda *a, **k: calls.append("warp") or ("warped", None))
    kw = dict(crop_prob=0.7, brightness=0.3, contrast=0.2, saturation=0.1)
    for extra, want_calls in ((dict(), ["augment"]), (dict(mosaic_prob=0.5, zoom_out_prob=0.5), ["compose"])):
        g = torch.Generator().manual_seed(5)
        t = aug.TrainAugment((56, 56), generator=g, degrees=15.0, distortion=0.5, **kw, **extra)      # ranges without a probability: no warp
        del calls[:]
        assert t(imgs) == ("batch", None) and calls == want_calls
        g2 = torch.Generator().manual_seed(5)
        t2 = aug.TrainAugment((56, 56), generator=g2, **kw, **extra)
        if extra:
            t2.sample_plan(shapes)
        else:
            aug.sample_params(shapes, g2, **kw)
        assert torch.equal(g.get_state(), g2.get_state())
        # with a warp: the same draws first, then 16 numbers per image, then one warp_batch call
        g3 = torch.Generator().manual_seed(5)
        del calls[:]
        t3 = aug.TrainAugment((56, 56), generator=g3, affine_prob=0.5, degrees=15.0, **kw, **extra)
        monkeypatch.setattr(aug, "augment_batch", lambda *a, **k: calls.append("augment") or (torch.zeros(3, 56, 56, 3, dtype=torch.uint8), None))
        monkeypatch.setattr(aug, "compose_batch", lambda *a, **k: calls.append("compose") or (torch.zeros(3, 56, 56, 3, dtype=torch.uint8), None))
        assert t3(imgs) == ("warped", None) and calls == want_calls + ["warp"]
        torch.rand(3 * 16, generator=g2, dtype=torch.float64)
        assert torch.equal(g3.get_state(), g2.get_state())
        monkeypatch.setattr(aug, "augment_batch", lambda *a, **k: calls.append("augment") or ("batch", None))
        monkeypatch.setattr(aug, "compose_batch", lambda *a, **k: calls.append("compose") or ("batch", None))
    for bad in (dict(affine_prob=1.5), dict(perspective_prob=-0.1)):
        with pytest.raises(ValueError):
            aug.TrainAugment((56, 56), **bad)
