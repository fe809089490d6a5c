"""`TrainAugment` in the closed geometry loop (tests/geometry_cases.py): the class draws its own plans, so the loop reads each plan
back from a twin generator -- to know the up-scaling s of every canvas and whether the canvas meets the premise of `check` -- and
holds the images and boxes of one call to the bound.  Shared by tests/test_geometry_loop_cpu.py (Pillow's pixels from the plan) and
tests/test_gpu_geometry_loop.py (`TrainAugment.__call__` itself).

Three configurations: the plain chain; mosaic / zoom-out; the same behind an affine o perspective warp.  The warp's ranges are gentle
-- 1.5 degrees of rotation, 1 of shear, a distortion of 0.04 -- so that every edge stays within `geometry_cases.MAX_TILT` of the pixel
grid, where Pillow's own pixels are sure to meet the bound at a corner: drawn plans cannot be turned down one by one as the
committed warp cases are, and steep rotations are theirs to cover.  Two more things this configuration gives up: it fills with a grey
inside the noise's range, not with the class's default (124, 116, 104) -- behind a zoom-out the warp blends a cut rectangle with the
fill next to it, and against the default the three channels cross 128 at coverages of 0.03 .. 0.16 instead of 0.41 .. 0.5, so the
default fill behind a warp is not looped -- and it leaves the brightness alone, which would move the switching coverage to 0.56."""
import numpy as np
import torch

from tests import compose_cases as cc
from tests import geometry_cases as gc

TRAIN = {"chain": dict(size=(56, 150), brightness=0.1),
         "compose": dict(size=(96, 128), brightness=0.1, mosaic_prob=0.5, zoom_out_prob=0.5),
         "warp": dict(size=(96, 128), mosaic_prob=0.5, zoom_out_prob=0.5, affine_prob=1.0, perspective_prob=0.5, degrees=1.5, translate=(0.1, 0.1),
                      scale=(0.7, 1.3), shear=1.0, distortion=0.04, fill=(20, 20, 20))}
TRAIN_COMMON = dict(crop_prob=0.7, hflip_prob=0.5)
TRAIN_BATCHES = {"chain": 20, "compose": 12, "warp": 24}
MAX_SKIPPED = 0.05         # the share of drawn canvases that may miss the premise and go unmeasured
MAX_CONTAIN = 0.30         # the share of warp boxes that may be held to containment only


def train_batch(seed, B=6):
    """sources for `TrainAugment`: B <= 6 ragged sources of 80 .. 160 px, one colour each (so whichever partners a mosaic draws, its
    colours are disjoint), one rectangle each over the middle -- from 0.25 .. 0.35 to 0.65 .. 0.75 of either side, so that every crop of
    at least half the source shows at least a seventh of the source's side of it"""
    rng = np.random.default_rng(9000 + seed)
    images, rects, shapes = [], [], []
    for b, c in enumerate(rng.permutation(6)[:B]):
        H, W = int(rng.integers(80, 161)), int(rng.integers(80, 161))
        r = (int(rng.uniform(0.25, 0.35) * W), int(rng.uniform(0.25, 0.35) * H), int(rng.uniform(0.65, 0.75) * W), int(rng.uniform(0.65, 0.75) * H), int(c))
        images.append(gc.paint(H, W, [r], 50 * seed + b)), rects.append([r]), shapes.append((H, W))
    return images, rects, shapes


def train_plan(aug, cfg, generator_state, shapes):
    """what a TrainAugment built from `cfg` draws for sources of these shapes from a generator in `generator_state`: (pieces,
    coeffs or None, the generator's state afterwards), the plain chain written as one piece over the whole canvas.  A twin built from
    the same `cfg` over a generator of its own calls the samplers `TrainAugment.__call__` calls, in its order; `train_loop` checks that
    the caller's generator ends in the same state."""
    g = torch.Generator()
    g.set_state(generator_state)
    twin = aug.TrainAugment(generator=g, **cfg)
    out_h, out_w = cfg["size"]
    if twin.mosaic_prob == 0.0 and twin.zoom_out_prob == 0.0:
        crops, flips, jitter = aug.sample_params(shapes, g, **twin.sampler)
        pieces = [[(n, tuple(int(v) for v in crops[n]), bool(flips[n]), tuple(float(f) for f in jitter[n]), (0, 0, out_w, out_h))] for n in range(len(shapes))]
    else:
        pieces = twin.sample_plan(shapes)
    coeffs = twin.sample_warp(len(pieces)) if twin.affine_prob > 0.0 or twin.perspective_prob > 0.0 else None
    return pieces, coeffs, g.get_state()


def plan_admissible(images, rects, canvas, size, coeffs=None, fill=gc.FILL):
    """what `check`'s premise needs of one drawn canvas, from the plan's own numbers: every piece shows each rectangle of its source
    not at all or by at least 3 output pixels (`crop_ok`); no two colours within 2 px of each other; an up-scaling of at most 4; and
    under a warp `warp_ok`, every mapped edge within MAX_TILT of the grid, the up-scaling being that of both stages, and -- as for the
    committed warp cases -- Pillow's own pixels of this plan within the bound of the mapped rectangles (`pillow_frames`: two
    resampling stages leave a wider ramp than one, and one canvas in about 140 ends 0.01 px over).  Returns (admissible, s, shown
    rectangles)."""
    ok = all(gc.crop_ok(rects[src], crop, dw, dh) for src, crop, _, _, (_, _, dw, dh) in canvas)
    shown = gc.shown_rects(rects, canvas)
    ok &= all(gc._apart(p, q, 2.0) for i, p in enumerate(shown) for q in shown[:i])
    s = gc._piece_s([canvas])[0]
    if coeffs is not None:
        s = max(1.0, s) * max(1.0, gc.magnification(coeffs, size, size))
        ok &= gc.warp_ok(coeffs, shown, size)
        ok &= all(gc.tilt(gc.forward(coeffs, [(x1, y1), (x2, y1), (x2, y2), (x1, y2)])) <= gc.MAX_TILT for x1, y1, x2, y2, _ in shown)
        ok = ok and s <= gc.MAX_SCALE and gc.pillow_frames(cc.pillow_compose(images, [canvas], size, fill)[0], coeffs, shown, size, s, fill)
    return bool(ok and s <= gc.MAX_SCALE), s, shown


def train_loop(aug, kind, run):
    """`TrainAugment`'s configuration `kind` over its committed batches: run(ta, images, targets, pieces, coeffs, state) -> (uint8
    [N, h, w, 3], new targets), leaving ta.generator in `state`, where the call itself would leave it.  Canvases whose drawn plan does
    not meet the premise (`plan_admissible`) are counted and not measured: at most 5 %.  Holds both conditions, and behind a warp the
    30 % limit on containment-only boxes."""
    cfg = dict(TRAIN_COMMON, as_uint8=True, **TRAIN[kind])
    size = cfg["size"]
    g = torch.Generator().manual_seed(77)
    ta = aug.TrainAugment(generator=g, **cfg)
    tally, skipped, total = gc.Tally(f"TrainAugment {kind}"), 0, 0
    for k in range(TRAIN_BATCHES[kind]):
        images, rects, shapes = train_batch(k)
        targets = [{"boxes": torch.from_numpy(b), "labels": torch.from_numpy(l)} for b, l in (gc.boxes_of(r, *hw) for r, hw in zip(rects, shapes))]
        pieces, coeffs, after = train_plan(aug, cfg, g.get_state(), shapes)
        outs, new = run(ta, images, targets, pieces, coeffs, after)
        if not torch.equal(g.get_state(), after):
            raise gc.GeometryError("the plan read back is not the plan that was drawn")
        for n, canvas in enumerate(pieces):
            ok, s, _ = plan_admissible(images, rects, canvas, size, None if coeffs is None else coeffs[n], ta.fill)
            total += 1
            if not ok:
                skipped += 1
                continue
            gc.hold_images(tally, outs[n:n + 1], new[n:n + 1], size, [s], warped=coeffs is not None)
    print(f"TrainAugment {kind}: {skipped} of {total} drawn canvases do not meet the premise and are not measured")
    if skipped > MAX_SKIPPED * total:
        raise gc.GeometryError(f"{kind}: {skipped} of {total} drawn canvases do not meet the premise, at most {MAX_SKIPPED:.0%} may")
    summary = tally.hold()
    if summary["contain_share"] > MAX_CONTAIN:
        raise gc.GeometryError(f"{kind}: {summary['contain_share']:.0%} of the boxes are held to containment only, at most {MAX_CONTAIN:.0%} may be")
    return summary
