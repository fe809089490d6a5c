"""plan_views (dinov2_od_amd/slicing.py) is pure host code: for image sizes around the tile size, several overlaps and both aspect
orientations every view lies inside its image, every pixel is covered, neighbouring tiles overlap by at least floor(t * overlap), the
order (whole image, tiles row-major, the same list mirrored) and the dedupe rule hold, and both limits raise before anything runs."""
import math

import numpy as np
import pytest

from dinov2_od_amd import slicing

T = 32
LENGTHS = [T - 1, T, T + 1, 2 * T - 1, 101]          # around the tile, just under two tiles, a prime
OVERLAPS = [0.0, 0.2, 0.33, 0.5, 0.9]


@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("L", LENGTHS + [3 * T, 7 * T + 5])
def test_axis_starts_cover_the_axis_and_overlap(L, overlap):
    starts, extent = slicing.axis_starts(L, T, overlap)
    if L <= T:
        assert starts == [0] and extent == L
        return
    assert extent == T and starts[0] == 0 and starts[-1] == L - T
    assert all(b > a for a, b in zip(starts, starts[1:]))
    step = T - math.floor(T * overlap)
    assert starts[:-1] == [k * step for k in range(len(starts) - 1)]
    assert starts[-2] + T < L <= starts[-2] + step + T                                        # the moved start is the first that reaches the end
    for a, b in zip(starts, starts[1:]):
        assert a + T - b >= math.floor(T * overlap)                                           # neighbours share at least the asked overlap
    covered = np.zeros(L, bool)
    for s in starts:
        covered[s:s + T] = True
    assert covered.all()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("full_view", [False, True])
@pytest.mark.parametrize("overlap", [0.0, 0.2, 0.5])
def test_views_lie_inside_cover_every_pixel_and_keep_the_order(overlap, full_view, flip):
    shapes = [(h, w) for h in LENGTHS for w in LENGTHS]                                       # both aspect orientations of every pair
    tile = (T, T)
    plan = slicing.plan_views(shapes, tile, overlap, full_view, flip)
    assert plan.offsets.dtype == np.int32 and plan.rects.dtype == np.int32 and plan.flips.dtype == np.uint8
    assert plan.offsets[0] == 0 and plan.offsets[-1] == len(plan.rects) == len(plan.flips) and len(plan.offsets) == len(shapes) + 1
    for b, (H, W) in enumerate(shapes):
        rects = plan.rects[plan.offsets[b]:plan.offsets[b + 1]].tolist()
        flips = plan.flips[plan.offsets[b]:plan.offsets[b + 1]].tolist()
        half = len(rects) // 2 if flip else len(rects)
        assert flips == [0] * half + ([1] * half if flip else [])
        if flip:
            assert rects[:half] == rects[half:]                                               # the same list again, mirrored
        rects = rects[:half]
        ys, eh = slicing.axis_starts(H, T, overlap)
        xs, ew = slicing.axis_starts(W, T, overlap)
        tiles = [[x, y, ew, eh] for y in ys for x in xs]                                      # row-major
        full = [0, 0, W, H]
        if full_view:
            assert rects[0] == full
            assert rects[1:] == [r for r in tiles if r != full]                               # a tile equal to the whole image is not listed twice
            assert rects.count(full) == 1
        else:
            assert rects == tiles
        assert len({tuple(r) for r in rects}) == len(rects)
        covered = np.zeros((H, W), bool)
        for l, t, w, h in rects:
            assert 0 <= l and 0 <= t and w >= 1 and h >= 1 and l + w <= W and t + h <= H
            covered[t:t + h, l:l + w] = True
        assert covered.all()


def test_a_rectangular_tile_and_a_scalar_tile():
    a = slicing.plan_views([(100, 300)], (50, 120), 0.25, full_view=False)
    assert a.rects.tolist() == [[x, y, 120, 50] for y in (0, 38, 50) for x in (0, 90, 180)]
    b = slicing.plan_views([(40, 90)], 40, 0.5)
    assert b.rects.tolist() == [[0, 0, 90, 40], [0, 0, 40, 40], [20, 0, 40, 40], [40, 0, 40, 40], [50, 0, 40, 40]]
    c = slicing.plan_views([(30, 30)], 40, 0.5, flip=True)                                    # the image fits the tile: one view, and its mirror
    assert c.rects.tolist() == [[0, 0, 30, 30]] * 2 and c.flips.tolist() == [0, 1]


def test_limits_raise():
    assert len(slicing.plan_views([(5, 5)], 1, 0.999, full_view=False).rects) == 25           # floor(1 * .999) = 0: a step of 1 is fine ...
    with pytest.raises(ValueError, match="step"):
        slicing.axis_starts(100, 10, 1.0)                                                     # ... a step of 0 is not
    with pytest.raises(ValueError):
        slicing.plan_views([(100, 100)], 10, 1.0)
    with pytest.raises(ValueError):
        slicing.plan_views([(100, 100)], 0, 0.2)
    # the resize filter: ceil(extent / out) * 2 + 1 <= 32 taps
    slicing.plan_views([(40, 480)], 480, 0.2, size=(28, 32))                                  # exactly 15x: 31 taps
    with pytest.raises(ValueError, match="taps"):
        slicing.plan_views([(40, 481)], 481, 0.2, size=(28, 32))                              # 33 taps, from the whole-image view
    with pytest.raises(ValueError, match="taps"):
        slicing.plan_views([(40, 600)], 481, 0.2, full_view=False, size=(28, 32))             # ... and from a tile
    slicing.plan_views([(40, 600)], 481, 0.2, full_view=False)                                # no size given: nothing to check
    # the merge: views * Q * C <= 2^20
    shapes, pairs = [(64, 64), (100, 164)], 100 * 91
    plan = slicing.plan_views(shapes, 32, 0.0, pairs=pairs)
    per_image = np.diff(plan.offsets)
    assert per_image.tolist() == [5, 25] and per_image.max() * pairs <= slicing.MAX_CANDIDATES
    with pytest.raises(ValueError, match="candidates"):
        slicing.plan_views(shapes, 32, 0.0, pairs=720 * 91)                                   # 25 views x 65520 pairs
    slicing.plan_views(shapes[:1], 32, 0.0, flip=True, pairs=(1 << 20) // 10)                 # 10 views: exactly at the limit
    with pytest.raises(ValueError, match="candidates"):
        slicing.plan_views(shapes[:1], 32, 0.0, flip=True, pairs=(1 << 20) // 10 + 1)
