"""The closed geometry loop without a GPU (tests/geometry_cases.py has the method and the bound): Pillow's own pixels next to the boxes
of `transform_targets`, `compose_targets` and `warp_targets`.  Four things are shown here:
  1. the reference meets both conditions on every committed case (so a GPU failure is the kernel's or the boxes', not the method's),
     the presence rules hold, and the cases do hold what they claim (cut and excluded rectangles, s <= 4, <= 30 % containment-only);
  2. `check` notices each of six deliberate corruptions of the boxes that a same-formula float64 reference would restate faithfully;
  3. `TrainAugment`'s own samplers, which the GPU test runs on the device, give plans whose boxes frame Pillow's pixels;
  4. the inverse direction on the host: a mask measured in a Pillow-extracted view of `plan_views`, mapped back through the view's
     rectangle and mirror flag (tests/detect_views_cases.py `view_boxes`), frames the painted rectangle in source pixels.
Every pipeline prints its worst side, its mean signed residual per side and its number of sides (DESIGN.md 6b has the table)."""
import numpy as np
import pytest
import torch

from dinov2_od_amd import augment as A
from dinov2_od_amd import slicing
from tests import augment_cases as ac
from tests import compose_cases as cc
from tests import detect_views_cases as dv
from tests import geometry_cases as gc
from tests import geometry_train as gt
from tests import warp_cases as wc

PIPELINES = ("chain", "mosaic", "zoom_out", "sixteen", "affine", "perspective", "staged")


def _targets(case):
    return [{"boxes": torch.from_numpy(t["boxes"]), "labels": torch.from_numpy(t["labels"])} for t in gc.targets_of(case)]


def pillow_pixels(pipeline, c):
    """the case's output images by Pillow: list of uint8 [h, w, 3]"""
    size = c["size"]
    if pipeline == "chain":
        return [ac.pillow_chain(im, c["crops"][b], c["flips"][b], None if c["jitter"] is None else c["jitter"][b], *size) for b, im in enumerate(c["images"])]
    if pipeline in ("affine", "perspective"):
        return [wc.pillow_warp(im, c["coeffs"][b], *size, c["fill"]) for b, im in enumerate(c["images"])]
    out = cc.pillow_compose(c["images"], c["pieces"], size, c["fill"])
    return [wc.pillow_warp(o, c["coeffs"][n], *size, c["fill"]) for n, o in enumerate(out)] if pipeline == "staged" else list(out)


def project_boxes(pipeline, c, targets=None, pieces=None, coeffs=None):
    """the case's new targets by the project's host functions; pieces / coeffs: what the boxes are told instead of the case's own"""
    size = c["size"]
    tg = _targets(c) if targets is None else targets
    if pipeline == "chain":
        return A.transform_targets(tg, c["shapes"], c["crops"], c["flips"], size)
    coeffs = c.get("coeffs") if coeffs is None else coeffs
    if pipeline in ("affine", "perspective"):
        return A.warp_targets(tg, c["shapes"], coeffs, size)
    new = A.compose_targets(tg, c["shapes"], c["pieces"] if pieces is None else pieces, size)
    return A.warp_targets(new, [size] * len(new), coeffs, size) if pipeline == "staged" else new


def hold(tally, pipeline, c, outs, new):
    gc.hold_images(tally, outs, new, c["size"], c["s"], warped=pipeline in gc.WARPED)


# ------------------------------------------------------------------------------------------ 1. the reference meets its own bound
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_pillow_pixels_meet_both_bounds_on_every_committed_case(pipeline):
    tally = gc.Tally(f"pillow {pipeline}")
    for c in gc.cases(pipeline):
        assert max(c["s"]) <= gc.MAX_SCALE + 1e-9, max(c["s"])
        hold(tally, pipeline, c, pillow_pixels(pipeline, c), project_boxes(pipeline, c))
    s = tally.hold()
    if pipeline in gc.WARPED:
        assert s["contain_share"] <= 0.30, s["contain_share"]
        assert s["contain_share"] > 0.02 or pipeline == "perspective"      # (corner to corner, inward moves only: nothing leaves the canvas)


def test_the_committed_cases_hold_what_they_claim():
    """rectangles cut and rectangles left out by a crop, in the chain and in the canvases; flips both ways; brightness on and off; batches
    of 5 to 8; every output size; warps gentle enough for the plain bound next to steep ones"""
    for pipeline in ("chain", "mosaic", "zoom_out"):
        cut = out = 0
        for c in gc.cases(pipeline):
            plans = [[(b, tuple(c["crops"][b]), c["flips"][b], None, None)] for b in range(len(c["images"]))] if pipeline == "chain" else c["pieces"]
            for canvas in plans:
                for src, crop, *_ in canvas:
                    k = gc.crop_kind(c["rects"][src], crop)
                    cut, out = cut + k[0], out + k[1]
        assert cut >= 10 and out >= 10, (pipeline, cut, out)
    chain = gc.cases("chain")
    assert {len(c["images"]) for c in chain} == {5, 6, 7, 8} and {c["size"] for c in chain} == set(gc.SIZES)
    assert {int(f) for c in chain for f in c["flips"]} == {0, 1} and {c["jitter"] is None for c in chain} == {True, False}
    assert any(len(canvas) == 16 for c in gc.cases("sixteen") for canvas in c["pieces"])
    tilts = [gc.tilt(gc.forward(c["coeffs"][b], [(r[0], r[1]), (r[2], r[1]), (r[2], r[3]), (r[0], r[3])]))
             for c in gc.cases("affine") for b in range(len(c["images"])) for r in c["rects"][b]]
    assert min(tilts) < gc.MAX_TILT < 25 < max(tilts) and np.mean(np.asarray(tilts) <= gc.MAX_TILT) > 0.2


def test_an_excluded_rectangle_has_neither_box_nor_pixels():
    n = 0
    for c in gc.cases("chain"):
        outs, new = pillow_pixels("chain", c), project_boxes("chain", c)
        for b, rs in enumerate(c["rects"]):
            for r in rs:
                if 0 in gc.visible(r, c["crops"][b]):
                    assert r[4] not in new[b]["labels"].tolist() and gc.extent(outs[b], r[4]) is None
                    n += 1
    assert n >= 10


def test_the_corner_terms():
    """at a straight edge the model gives the bound's own 0.09 outward; the tilt limit is where the two corner terms reach the bound's 0.1"""
    assert abs(gc.corner_depth(0.0, 0.41) + 0.09) < 1e-3 and abs(gc.corner_depth(0.0, 0.5)) < 1e-3
    f = lambda phi: 0.5 * np.sin(2 * np.radians(phi)) + gc.corner_depth(phi)
    assert f(gc.MAX_TILT) <= 0.1 < f(gc.MAX_TILT + 0.2)
    assert abs(gc.corner_depth(30.0) - 0.248) < 2e-3 and abs(gc.corner_depth(60.0) - gc.corner_depth(30.0)) < 1e-12


# ------------------------------------------------------------------------------------------------------------- 2. sensitivity
def _outcome(pipeline, corrupt):
    """run the pipeline's cases with `corrupt(case, new_targets) -> new_targets` applied to the boxes: (images that fail `check`,
    images, whether the per-pipeline mean condition fails on the images that pass)"""
    tally, failed, total = gc.Tally(f"corrupted {pipeline}"), 0, 0
    for c in gc.cases(pipeline):
        outs, new = pillow_pixels(pipeline, c), corrupt(c, project_boxes(pipeline, c))
        for n in range(len(outs)):
            one = dict(c, s=[c["s"][n]])
            total += 1
            try:
                hold(tally, pipeline, one, outs[n:n + 1], new[n:n + 1])
            except gc.GeometryError:
                failed += 1
    try:
        tally.hold(min_sides=0)
        mean_fails = False
    except gc.GeometryError:
        mean_fails = True
    return failed, total, mean_fails


def _with_boxes(t, boxes):
    return dict(t, boxes=boxes.to(t["boxes"].dtype))


def test_check_passes_uncorrupted():
    for pipeline in ("chain", "mosaic", "affine"):
        assert _outcome(pipeline, lambda c, new: new)[::2] == (0, False)


def test_a_half_pixel_shift_in_x_is_noticed():
    """every box 0.5 output px to the right: the mean signed residual moves by half a pixel, which the per-pipeline condition is for"""
    def corrupt(c, new):
        return [_with_boxes(t, t["boxes"] + torch.tensor([0.5 / c["size"][1], 0, 0, 0])) for t in new]
    failed, total, mean_fails = _outcome("chain", corrupt)
    print(f"x + 0.5 px: {failed} of {total} images fail a side; the mean condition fails: {mean_fails}")
    assert mean_fails and failed > total // 4


def test_a_mirror_about_cw_minus_1_is_noticed():
    def corrupt(c, new):
        return [_with_boxes(t, t["boxes"] - torch.tensor([1.0 / c["crops"][b][2], 0, 0, 0])) if c["flips"][b] else t for b, t in enumerate(new)]
    failed, total, _ = _outcome("chain", corrupt)
    flipped = sum(int(f) for c in gc.cases("chain") for f in c["flips"])
    print(f"mirror about cw - 1: {failed} of {flipped} flipped images fail")
    assert failed >= flipped // 2


def test_a_dropped_dx_is_noticed():
    def corrupt(c, new):
        pieces = [[(s, crop, fl, j, (0, dy, dw, dh)) for s, crop, fl, j, (dx, dy, dw, dh) in canvas] for canvas in c["pieces"]]
        return project_boxes("mosaic", c, pieces=pieces)
    failed, total, _ = _outcome("mosaic", corrupt)
    print(f"dx zeroed: {failed} of {total} canvases fail")
    assert failed >= 0.9 * total


def test_piece_targets_in_another_order_than_the_pieces_are_noticed():
    """the boxes concatenated over the pieces in reverse, the labels in paste order"""
    def corrupt(c, new):
        out = []
        for n, canvas in enumerate(c["pieces"]):
            per_piece = project_boxes("mosaic", c, pieces=[[p] for p in canvas])
            out.append(dict(new[n], boxes=torch.cat([t["boxes"] for t in reversed(per_piece)]), labels=torch.cat([t["labels"] for t in per_piece])))
        return out
    failed, total, _ = _outcome("mosaic", corrupt)
    print(f"reversed piece order: {failed} of {total} canvases fail")
    assert failed >= 0.9 * total


@pytest.mark.parametrize("pipeline", ["affine", "perspective"])
def test_a_box_sent_through_the_coefficients_instead_of_their_inverse_is_noticed(pipeline):
    def corrupt(c, new):
        inv = np.stack([(lambda F: (F / F[2, 2]).reshape(9)[:8])(np.linalg.inv(A._matrix(k))) for k in c["coeffs"]])
        return project_boxes(pipeline, c, coeffs=inv)                      # `warp_targets` inverts them back: the boxes go through M
    failed, total, _ = _outcome(pipeline, corrupt)
    print(f"{pipeline}, M for its inverse: {failed} of {total} images fail")
    assert failed >= 0.9 * total


def test_targets_of_neighbouring_images_swapped_are_noticed():
    def corrupt(c, new):
        new = list(new)
        new[0], new[1] = new[1], new[0]
        return new
    failed, total, _ = _outcome("chain", corrupt)
    print(f"targets 0 and 1 swapped: {failed} images fail in {len(gc.cases('chain'))} cases")
    assert failed >= 1.8 * len(gc.cases("chain"))


# ------------------------------------------------------------------------------------------- 3. TrainAugment's plans, Pillow's pixels
@pytest.mark.parametrize("kind", list(gt.TRAIN))
def test_train_augment_plans_with_pillow_pixels(kind):
    """the samplers and the host target functions as `TrainAugment.__call__` chains them, the pixels by Pillow from the same plan; the
    generator is advanced as the call would advance it"""
    def run(ta, images, targets, pieces, coeffs, after):
        size, fill = ta.size, ta.fill
        shapes = [im.shape[:2] for im in images]
        ta.generator.set_state(after)
        outs = cc.pillow_compose(images, pieces, size, fill)
        if kind == "chain":
            new = A.transform_targets(targets, shapes, [p[0][1] for p in pieces], [p[0][2] for p in pieces], size)
        else:
            new = A.compose_targets(targets, shapes, pieces, size)
        if coeffs is not None:
            outs = np.stack([wc.pillow_warp(o, coeffs[n], *size, fill) for n, o in enumerate(outs)])
            new = A.warp_targets(new, [size] * len(new), coeffs, size)
        return outs, new
    gt.train_loop(A, kind, run)


# ------------------------------------------------------------------------------------------------- 4. the inverse direction, host
SLICE = dict(size=(96, 96), tile=128, overlap=0.25)


def test_a_mask_measured_in_a_view_maps_back_onto_the_painted_rectangle():
    """`plan_views` + the numpy restatement of the view mapping: for every view (whole image, tiles, mirrored copies) and every rectangle
    the view shows whole, the mask's extent in the Pillow-extracted view, written as the normalised cxcywh a model would answer and sent
    through `view_boxes`, frames the rectangle in source pixels within the per-side bound times rect_w / out_w (rect_h / out_h in y)"""
    out_h, out_w = SLICE["size"]
    worst, sides, mirrored, tiles = 0.0, 0, 0, 0
    for seed in range(3):
        images, rects, shapes = gc.slicing_sources(seed)
        plan = slicing.plan_views(shapes, SLICE["tile"], SLICE["overlap"], True, True, size=SLICE["size"])
        assert (np.diff(plan.offsets) > 2).all()
        for b, im in enumerate(images):
            for v in range(plan.offsets[b], plan.offsets[b + 1]):
                l, t, w, h = (int(x) for x in plan.rects[v])
                view = ac.pillow_chain(im, plan.rects[v], plan.flips[v], None, out_h, out_w)
                s = max(out_w / w, out_h / h)
                tol = np.array([gc.bound(s) * w / out_w, gc.bound(s) * h / out_h] * 2)
                for r in rects[b]:
                    if gc.visible(r, (l, t, w, h)) != (r[2] - r[0], r[3] - r[1]):
                        continue                                     # cut or left out by this view
                    e = gc.extent(view, r[4])
                    assert e is not None, (seed, b, v, r)
                    row = np.array([[(e[0] + e[2]) / (2 * out_w), (e[1] + e[3]) / (2 * out_h), (e[2] - e[0]) / out_w, (e[3] - e[1]) / out_h]], np.float32)
                    back = dv.view_boxes(row, plan.rects[v], int(plan.flips[v]))[0].astype(np.float64)
                    res = back - np.asarray(r[:4], dtype=np.float64)
                    assert (np.abs(res) <= tol + 1e-4).all(), (seed, b, v, r, res.tolist(), tol.tolist())
                    worst, sides = max(worst, float(np.abs(res / tol).max())), sides + 4
                    mirrored, tiles = mirrored + int(plan.flips[v]), tiles + int((w, h) != shapes[b][::-1])
    print(f"inverse direction, host: {sides} sides, worst residual / tolerance {worst:.3f}")
    assert sides >= 300 and mirrored >= 30 and tiles >= 30
