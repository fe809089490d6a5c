"""The closed geometry loop on the device (tests/geometry_cases.py has the method and the bound; tests/test_geometry_loop_cpu.py shows
that Pillow's pixels meet it and that `check` notices the mistakes looked for): the same `check`, on what the device writes and what
the public entries return together.
  1. `augment_batch`, `compose_batch` and `warp_batch` on the committed ragged cases, both `as_uint8` forms;
  2. `TrainAugment.__call__` for the plain chain, for mosaic / zoom-out, and for the same behind affine o perspective, the boxes through
     both stages exactly as the class returns them;
  3. `detect_sliced` (nms and fuse merges, flip on and off, with and without the whole-image view), the whole-image path
     `preprocess_batch` -> `detect_packed`, and `draw_detections`, with a stub in place of the model that answers, per view and colour,
     the box of the colour's mask: every painted rectangle comes back once, in source pixels, where it was painted.
Every pipeline prints its worst side, its mean signed residual per side and its number of sides."""
import types

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import geometry_train as gt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aug():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import augment
    return augment


def _targets(case):
    return [{"boxes": torch.from_numpy(t["boxes"]), "labels": torch.from_numpy(t["labels"])} for t in gc.targets_of(case)]


def _bytes(out, as_uint8):
    return out.cpu().numpy() if as_uint8 else gc.float_to_u8(out)


# --------------------------------------------------------------------------------------------------------- 1. the direct entries
@pytest.mark.parametrize("pipeline", ["chain", "mosaic", "zoom_out", "sixteen", "affine", "perspective", "staged"])
def test_direct_entries_on_the_committed_cases(aug, pipeline):
    """cases take the two output forms by turns; parameters differ per image, so a row mix-up between pixels and targets shows"""
    tally = gc.Tally(f"device {pipeline}")
    forms = set()
    for k, c in enumerate(gc.cases(pipeline)):
        as_uint8 = k % 2 == 0
        forms.add(as_uint8)
        size, tg = c["size"], _targets(c)
        warped = pipeline in gc.WARPED
        if pipeline == "chain":
            out, new = aug.augment_batch(c["images"], tg, c["crops"], c["flips"], c["jitter"], size, as_uint8=as_uint8)
        elif pipeline in ("affine", "perspective"):
            out, new = aug.warp_batch(c["images"], tg, c["coeffs"], size, c["fill"], as_uint8=as_uint8)
        else:
            out, new = aug.compose_batch(c["images"], tg, c["pieces"], size, c["fill"], as_uint8=as_uint8 or pipeline == "staged")
            if pipeline == "staged":
                out, new = aug.warp_batch(out, new, c["coeffs"], size, c["fill"], as_uint8=as_uint8)
        gc.hold_images(tally, _bytes(out, as_uint8), new, size, c["s"], warped=warped)
    assert forms == {True, False}
    s = tally.hold()
    if pipeline in gc.WARPED:
        assert s["contain_share"] <= 0.30, s["contain_share"]


# ------------------------------------------------------------------------------------------------------ 2. TrainAugment.__call__
@pytest.mark.parametrize("kind", list(gt.TRAIN))
def test_train_augment_call(aug, kind):
    """images and targets from one `__call__`; the plan is read back from a twin generator, which must end where the call's ended"""
    def run(ta, images, targets, pieces, coeffs, after):
        out, new = ta(images, targets)
        return out.cpu().numpy(), new
    gt.train_loop(aug, kind, run)


# ------------------------------------------------------------------------------------------------------------- 3. inference
class MaskBoxes(torch.nn.Module):
    """in place of the model: query k answers colour k.  Per view and colour the normalised cxcywh box of the colour's mask and a logit
    of +8 in class k + 1 where the mask is not empty, -8 everywhere else (class 0 is the background).  With equal logits the merge keeps
    the first view that shows an object, the whole unmirrored image; prefer_late adds 0.01 per row of the batch to the +8, so that the
    last view that shows it whole wins instead: a tile, and with flip a mirrored one."""

    def __init__(self, prefer_late=False):
        super().__init__()
        self.prefer_late = prefer_late
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self._dc_cfg = types.SimpleNamespace(num_queries=len(gc.COLOURS), num_classes=len(gc.COLOURS) + 1)

    def forward_packed_u8(self, u8):
        V, H, W, _ = u8.shape
        dev = u8.device
        pattern = torch.from_numpy(gc.COLOURS >= 128).to(dev)                                   # [6, 3]
        m = ((u8 >= 128)[:, None] == pattern[None, :, None, None, :]).all(-1)                   # [V, 6, H, W]

        def span(a):                                                                            # [V, 6, L] -> first, last + 1
            L = a.shape[-1]
            idx = torch.arange(L, device=dev)
            return torch.where(a, idx, L).amin(-1).float(), torch.where(a, idx + 1, 0).amax(-1).float()
        (x1, x2), (y1, y2) = span(m.any(2)), span(m.any(3))
        present = m.any(3).any(2)                                                               # [V, 6]
        box = torch.stack([(x1 + x2) / (2 * W), (y1 + y2) / (2 * H), (x2 - x1) / W, (y2 - y1) / H], -1)
        box = torch.where(present[..., None], box, torch.zeros_like(box))
        Q = len(gc.COLOURS)
        logits = torch.full((V, Q, Q + 1), -8.0, device=dev)
        k = torch.arange(Q, device=dev)
        high = 8.0 + (0.01 * torch.arange(V, device=dev, dtype=torch.float32)[:, None] if self.prefer_late else torch.zeros(V, 1, device=dev))
        logits[:, k, k + 1] = torch.where(present, high.expand(V, Q), torch.full((V, Q), -8.0, device=dev))
        return torch.cat([logits, box], -1).float().contiguous()


SLICE = dict(size=(96, 96), tile=128, overlap=0.25)
EDGE = 2.0


def _plan(shapes, full_view, flip):
    from dinov2_od_amd import slicing
    return slicing.plan_views(shapes, SLICE["tile"], SLICE["overlap"], full_view, flip, size=SLICE["size"])


def _view_tol(rect):
    """the per-side bound in source pixels of a view (left, top, width, height) resized to SLICE's size: (tol_x, tol_y)"""
    out_h, out_w = SLICE["size"]
    b = gc.bound(max(out_w / rect[2], out_h / rect[3]))
    return b * rect[2] / out_w, b * rect[3] / out_h


def _sliced(model, images, **kw):
    from dinov2_od_amd import slicing
    with torch.no_grad():
        return slicing.detect_sliced(model, images, threshold=0.5, edge_margin=EDGE, **SLICE, **kw)


def _rows(r, b):
    n = int(r.counts[b])
    return n, r.boxes[b, :n].cpu().numpy().astype(np.float64), r.labels[b, :n].cpu().numpy()


@pytest.mark.parametrize("prefer_late", [False, True])
@pytest.mark.parametrize("full_view", [True, False])
@pytest.mark.parametrize("flip", [False, True])
def test_sliced_inference_nms_returns_every_rectangle_once_where_it_was_painted(aug, flip, full_view, prefer_late):
    """without the whole-image view only tiles can answer: the sources then keep every rectangle whole inside some tile, clear of the
    edge margin.  A detection displaced by its tile's offset would miss by 96 px or more."""
    model = MaskBoxes(prefer_late).cuda().eval()
    tally = gc.Tally(f"sliced nms flip={int(flip)} full_view={int(full_view)} prefer_late={int(prefer_late)}")
    from_tiles = mirrored = 0
    for seed in range(3):
        tiles = None if full_view else (SLICE["tile"], SLICE["overlap"], EDGE + 2)
        images, rects, shapes = gc.slicing_sources(seed, side=(24, 60) if full_view else (24, 27), tiles=tiles)
        plan = _plan(shapes, full_view, flip)
        assert (np.diff(plan.offsets) >= 4).all()                                               # multi-tile plans
        r = _sliced(model, images, flip=flip, full_view=full_view, merge="nms")
        for b, (H, W) in enumerate(shapes):
            n, boxes, labels = _rows(r, b)
            assert sorted(labels.tolist()) == sorted(q[4] + 1 for q in rects[b]), (seed, b, labels.tolist(), rects[b])
            kept = plan.offsets[b] + r.views[b, :n].cpu().numpy()
            views = plan.rects[kept]
            from_tiles, mirrored = from_tiles + int((views[:, 2] < W).sum()), mirrored + int(plan.flips[kept].sum())
            tol = np.array([_view_tol(v) for v in views])
            tally.add(gc.check(images[b], boxes, labels - 1, (H, W), 1.0, fmt="xyxy", tol=(tol[:, 0], tol[:, 1])))
    tally.report()
    assert from_tiles >= 9 or (full_view and not prefer_late)
    assert mirrored >= 9 or not (flip and prefer_late)


def test_sliced_inference_fuse(aug):
    model = MaskBoxes().cuda().eval()
    tally = gc.Tally("sliced fuse")
    fused = 0
    for flip in (False, True):
        images, rects, shapes = gc.slicing_sources(5)
        plan = _plan(shapes, True, flip)
        r = _sliced(model, images, flip=flip, merge="fuse", nms_iou=0.5)
        for b, (H, W) in enumerate(shapes):
            n, boxes, labels = _rows(r, b)
            members = r.members[b, :n].cpu().numpy()
            assert sorted(labels.tolist()) == sorted(q[4] + 1 for q in rects[b]) and (members >= 1).all(), (b, labels.tolist(), members.tolist())
            fused += int((members > 1).sum())
            tol = np.array([_view_tol(v) for v in plan.rects[plan.offsets[b]:plan.offsets[b + 1]]]).max(axis=0)      # the largest scale among the views
            tally.add(gc.check(images[b], boxes, labels - 1, (H, W), 1.0, fmt="xyxy", tol=(tol[0], tol[1])))
    tally.report()
    assert fused >= 6


def test_whole_image_path_and_drawing(aug):
    """`preprocess_batch` -> the stub -> `detect_packed(sizes=source shapes)`: boxes in source pixels within the bound times W / out_w
    (H / out_h in y).  Then `draw_detections` into each source, the painted rectangles as ground truth below: every detection-coloured
    pixel lies within that tolerance plus the thickness of its rectangle's border, every ground-truth-coloured one within the thickness."""
    from dinov2_od_amd import preprocess, visualize
    from dinov2_od_amd.postprocess import Detections, detect_packed
    model = MaskBoxes().cuda().eval()
    out_h, out_w = 56, 150                                                                      # three 64-column blocks
    Cn = model._dc_cfg.num_classes
    tally = gc.Tally("whole image")
    white, grey, thickness = (255, 255, 255), (128, 128, 128), 2
    names = ["background", "red", "green", "blue", "cyan", "magenta", "yellow"]
    for seed in range(4):
        images, rects, shapes = gc.slicing_sources(20 + seed, n=5 + seed % 4, lo=80, hi=220, side=(24, 40))
        u8 = preprocess.preprocess_batch(images, (out_h, out_w), as_uint8=True)
        if seed % 2:                                                                            # the float form, through round(x * 255)
            f32 = preprocess.preprocess_batch(images, (out_h, out_w))
            assert np.array_equal(gc.float_to_u8(f32), u8.cpu().numpy())
        with torch.no_grad():
            det = model.forward_packed_u8(u8)
        r = detect_packed(det, Cn, sizes=torch.tensor(shapes, dtype=torch.float32), threshold=0.5)
        for b, (H, W) in enumerate(shapes):
            n, boxes, labels = _rows(r, b)
            assert sorted(labels.tolist()) == sorted(q[4] + 1 for q in rects[b]), (seed, b, labels.tolist())
            b_out = gc.bound(max(out_w / W, out_h / H))
            tol = (b_out * W / out_w, b_out * H / out_h)
            tally.add(gc.check(images[b], boxes, labels - 1, (H, W), 1.0, fmt="xyxy", tol=tol))
            # drawing, one source at a time (the batch is ragged)
            gt_boxes, gt_labels = gc.boxes_of(rects[b], H, W)
            targets = [{"boxes": torch.from_numpy(gt_boxes).cuda(), "labels": torch.from_numpy(gt_labels + 1).cuda()}]
            one = Detections(*(t[b:b + 1] for t in r))
            drawn = visualize.draw_detections(torch.from_numpy(images[b][None]).cuda(), one, targets, names, score_threshold=0.5, thickness=thickness,
                                              fill_alpha=0, font_scale=0, palette=[white], gt_color=grey)[0].cpu().numpy()
            changed = (drawn != images[b]).any(-1)
            is_white, is_grey = (drawn == white).all(-1) & changed, (drawn == grey).all(-1) & changed
            assert (changed == (is_white | is_grey)).all()
            ys, xs = np.mgrid[0:H, 0:W] + 0.5
            near_w, near_g = np.zeros((H, W), bool), np.zeros((H, W), bool)
            for x1, y1, x2, y2, _ in rects[b]:
                for near, ax, ay in ((near_w, tol[0] + thickness + 0.5, tol[1] + thickness + 0.5), (near_g, thickness + 0.5, thickness + 0.5)):
                    outer = (xs >= x1 - ax) & (xs <= x2 + ax) & (ys >= y1 - ay) & (ys <= y2 + ay)
                    inner = (xs > x1 + ax) & (xs < x2 - ax) & (ys > y1 + ay) & (ys < y2 - ay)
                    near |= outer & ~inner
                # every rectangle got its outline: at least half its perimeter in detection-coloured pixels around it
                band = (xs >= x1 - tol[0] - 3) & (xs <= x2 + tol[0] + 3) & (ys >= y1 - tol[1] - 3) & (ys <= y2 + tol[1] + 3)
                assert (is_white & band).sum() >= (x2 - x1) + (y2 - y1), (seed, b, (x1, y1, x2, y2))
            assert not (is_white & ~near_w).any(), (seed, b, np.argwhere(is_white & ~near_w)[:4].tolist())
            assert not (is_grey & ~near_g).any(), (seed, b, np.argwhere(is_grey & ~near_g)[:4].tolist())
    tally.report()
