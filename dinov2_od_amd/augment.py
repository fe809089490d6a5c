"""Train-time augmentation on the GPU: the host side of `dod_preprocess_aug` (include/dinodet.h).

The reference trains on `Resize((224, 224)) + ToTensor()` alone (dino_detector/train.py:584-587).  This module adds what every
DETR recipe adds -- a random crop before the resize, a colour jitter, a random horizontal flip -- where the resize already
lives (preprocess.py), with the boxes transformed alongside.  The image semantics are Pillow's, in this order per image:

    img.crop(box) -> ImageEnhance.Brightness -> ImageEnhance.Contrast -> ImageEnhance.Color -> resize(size, BILINEAR)
                  -> transpose(FLIP_LEFT_RIGHT) -> ToTensor (or the uint8 bytes for `forward_packed_u8`)

bit for bit.  `augment_batch` takes the parameters explicitly; `sample_params` draws them on the host from a CPU
`torch.Generator`; `TrainAugment` is the two together, the training counterpart of `ResizeToTensor`.  The targets (the
reference's dicts, dataset.py:101-111: normalised cxcywh `boxes`, `labels`) are transformed on the host in float32: they are a
few hundred bytes and their output shape depends on the data.  No CPU fallback for the images.

Mosaic and zoom-out are composed canvases (`dod_preprocess_compose`): `compose_batch` pastes disjoint pieces, each the chain above at
its own output size, onto a fill colour; `sample_mosaic` and `sample_zoom_out` draw the plans; `TrainAugment(mosaic_prob=...,
zoom_out_prob=...)` mixes them with the plain chain.

Random affine (rotation, scale, shear, translation) and perspective are a geometric warp (`dod_preprocess_warp`): `warp_batch` is
Pillow's `Image.transform(size, PERSPECTIVE, coeffs, BILINEAR, fillcolor=fill)` bit for bit, one inverse-map gather per batch behind
the chain or the canvas; `affine_coeffs`, `perspective_coeffs` and `compose_coeffs` build the eight coefficients, `warp_targets` sends
the boxes through the forward map, `sample_affine` / `sample_perspective` draw them, and `TrainAugment(affine_prob=...,
perspective_prob=...)` adds the stage to either pipeline.
"""
import math

import numpy as np
import torch

from . import _native as nat
from . import preprocess as _pre

MIN_BOX = 0.001        # the reference dataset's own minimum normalised width / height (dataset.py:90)
MAX_TAPS = 32          # csrc/preproc.hip PP_MAXK: the filter taps at most (down-scaling up to 15x)


def _taps(crop, dest):
    """the filter taps of resizing `crop` pixels to `dest` (csrc/preproc.hip pp_taps_ok): ceil(crop / dest) * 2 + 1"""
    return -(-int(crop) // int(dest)) * 2 + 1


def _check_params(shapes, crops, flips, jitter, out_h, out_w):
    """the parameters as (int32 [B, 4], uint8 [B], float32 [B, 3] or None); ValueError for anything the kernels must not see"""
    B = len(shapes)
    crops = np.asarray(crops)
    if crops.shape != (B, 4) or crops.dtype.kind not in "iu":
        raise ValueError(f"crops: expected {B} integer boxes (left, top, width, height), got {crops.dtype} {crops.shape}")
    crops = crops.astype(np.int64)
    flips = np.asarray(flips)
    if flips.shape != (B,):
        raise ValueError(f"flips: expected {B} flags, got shape {flips.shape}")
    flips = (flips != 0).astype(np.uint8)
    for b, ((H, W), (l, t, w, h)) in enumerate(zip(shapes, crops)):
        if w < 1 or h < 1 or l < 0 or t < 0 or l + w > W or t + h > H:
            raise ValueError(f"crop {b}: box (left {l}, top {t}, width {w}, height {h}) is empty or not inside its {H}x{W} image")
    if jitter is not None:
        jitter = np.asarray(jitter, dtype=np.float32)
        if jitter.shape != (B, 3):
            raise ValueError(f"jitter: expected [{B}, 3] factors (brightness, contrast, saturation), got shape {jitter.shape}")
        if not np.isfinite(jitter).all() or (jitter < 0).any():
            raise ValueError("jitter: factors must be finite and >= 0")
    k = max(_taps(crops[:, 2].max(), out_w), _taps(crops[:, 3].max(), out_h))
    if k > MAX_TAPS:
        raise ValueError(f"a crop is more than 15x the output {out_h}x{out_w}: the filter would need {k} taps (> {MAX_TAPS})")
    return crops.astype(np.int32), flips, jitter


def _boxes_in_crop(boxes, H, W, crop, flip, min_visibility):
    """normalised cxcywh boxes of an [H, W] image under crop (left, top, width, height) and flip, on the host in float32 ->
    (x1, y1, x2, y2, keep): the corners in crop pixels, clamped to the crop and mirrored if flipped, and the keep rule of
    `transform_targets` (decided before the mirror, which changes none of its terms)"""
    l, t, cw, ch = crop
    cx, cy, bw, bh = boxes.detach().to("cpu", torch.float32).reshape(-1, 4).unbind(1)
    x1 = ((cx - 0.5 * bw) * W - l).clamp(0, cw)
    x2 = ((cx + 0.5 * bw) * W - l).clamp(0, cw)
    y1 = ((cy - 0.5 * bh) * H - t).clamp(0, ch)
    y2 = ((cy + 0.5 * bh) * H - t).clamp(0, ch)
    keep = (x2 > x1) & (y2 > y1) & ((x2 - x1) / cw >= MIN_BOX) & ((y2 - y1) / ch >= MIN_BOX) \
        & ((x2 - x1) * (y2 - y1) >= min_visibility * ((bw * W) * (bh * H)))
    if flip:
        x1, x2 = cw - x2, cw - x1
    return x1, y1, x2, y2, keep


def transform_targets(targets, shapes, crops, flips, size, min_visibility=0.0):
    """the reference's target dicts under the crops and flips, on the host in float32.  Per box of an image [H, W] and its crop
    (left, top, width, height): the corners in crop pixels, clamped to the crop; kept iff it is not empty, its clipped width /
    height are >= 0.001 of the crop's (dataset.py:90) and its clipped area >= min_visibility x its area; mirrored if flipped;
    written back as normalised cxcywh of the crop.  `labels` follow the same mask, `size` becomes the output size, every other key
    passes through.  A full-image crop without a flip returns `boxes` and `labels` as they are."""
    out_h, out_w = _pre._out_size(size)
    new = []
    for tg, (H, W), (l, t, cw, ch), fl in zip(targets, shapes, np.asarray(crops).tolist(), np.asarray(flips).tolist()):
        nt = dict(tg)
        if "size" in nt:
            nt["size"] = torch.as_tensor([out_h, out_w]).to(torch.as_tensor(tg["size"]))
        if "boxes" in nt and not (l == 0 and t == 0 and cw == W and ch == H and not fl):
            src = tg["boxes"]
            x1, y1, x2, y2, keep = _boxes_in_crop(src, H, W, (l, t, cw, ch), fl, min_visibility)
            out = torch.stack([(x1 + x2) / (2 * cw), (y1 + y2) / (2 * ch), (x2 - x1) / cw, (y2 - y1) / ch], dim=1)[keep]
            nt["boxes"] = out.to(src.device)
            if "labels" in nt:
                nt["labels"] = tg["labels"][keep.to(tg["labels"].device)]
        new.append(nt)
    return new


def augment_batch(images, targets, crops, flips, jitter=None, size=(224, 224), device="cuda", as_uint8=False, min_visibility=0.0):
    """images: as `preprocess_batch` takes them; targets: the reference's target dicts, one per image, or None; crops: integer
    [B, 4] boxes (left, top, width, height), each inside its image; flips: [B] flags; jitter: None or [B, 3] factors (brightness,
    contrast, saturation; finite, >= 0, 1.0 = identity).  Returns (batch, new_targets): the batch is float32 [B, 3, height, width]
    on `device`, or with as_uint8 the uint8 [B, height, width, 3] bytes for `model.forward_packed_u8`.  Anything wrong with the
    parameters raises ValueError before anything is copied or launched."""
    out_h, out_w = _pre._out_size(size)
    srcs = _pre._sources(images)
    B = len(srcs)
    shapes = srcs.shapes
    crops, flips, jitter = _check_params(shapes, crops, flips, jitter, out_h, out_w)
    if targets is not None and len(targets) != B:
        raise ValueError(f"targets: expected {B} dicts, got {len(targets)}")
    if jitter is not None and (jitter == 1.0).all():
        jitter = None                                   # the geometric-only kernel
    src, src_offs, hs, ws = srcs.stage(torch.device(device))
    out = _launch_aug(src, src_offs, hs, ws, crops, flips, jitter, out_h, out_w, as_uint8)
    new_targets = transform_targets(targets, shapes, crops, flips, (out_h, out_w), min_visibility) if targets is not None else None
    return out, new_targets


def _launch_aug(src, src_offs, hs, ws, crops, flips, jitter, out_h, out_w, as_uint8, staged=None):
    """`dod_preprocess_aug*` on staged sources: src on the device, the rest host arrays with one row per output image -- src_offs / hs /
    ws name its source (outputs may share one), crops / flips / jitter are as `_check_params` returns them.  staged: the (crops, flips)
    tensors of a caller that has them on the device already."""
    dev = src.device
    B = len(crops)
    tmp_offs, tmp_bytes = _pre._tmp_layout(crops[:, 3], out_w, crops[:, 2] if jitter is not None else None)
    meta = _pre._upload(dev, src_offs, hs, ws, tmp_offs, jitter)
    crops_t, flips_t = staged if staged is not None else _pre._upload(dev, crops, flips)
    lsum = _pre._luma_sums(jitter, B, dev)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    out = _pre._out_buffer(B, out_h, out_w, as_uint8, dev)
    nat.check(_pre._entry("dod_preprocess_aug", as_uint8)(
        nat.ptr(src), nat.ptr(meta[0]), nat.ptr(meta[1]), nat.ptr(meta[2]), B, nat.ptr(crops_t), nat.ptr(flips_t), nat.ptr(meta[4]), nat.ptr(lsum),
        int(crops[:, 3].max()), int(crops[:, 2].max()), out_h, out_w, nat.ptr(tmp), nat.ptr(meta[3]), nat.ptr(out), nat.stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------------------------ composed canvases
# Mosaic and zoom-out are one primitive (`dod_preprocess_compose`, include/dinodet.h): a canvas of a fill colour with disjoint
# rectangular pieces pasted into it, each piece the chain above at its own output size.  Pillow's semantics, per canvas:
#     canvas = Image.new("RGB", (out_w, out_h), fill)
#     for (src, crop, flip, jitter, dest) in pieces:  canvas.paste(chain(images[src], crop, jitter, (dw, dh), flip), (dx, dy))
MAX_PIECES = 16        # csrc/preproc.hip PP_MAXP: pieces per canvas


def _check_fill(fill, N):
    """the fill as (uint8 [3] or [N, 3], per-canvas flag)"""
    f = np.asarray(fill)
    if f.dtype.kind not in "iuf" or f.shape not in ((3,), (N, 3)) or not np.isfinite(f).all() or (f != np.floor(f)).any() \
            or (f < 0).any() or (f > 255).any():
        raise ValueError(f"fill: expected (r, g, b) integers in 0..255, or one such triple per canvas ({N}), got {fill!r}")
    return np.ascontiguousarray(f.astype(np.uint8)), f.ndim == 2


def _check_pieces(shapes, pieces, out_h, out_w):
    """the plan as (int32 [P, 10] rows (src, l, t, cw, ch, flip, dx, dy, dw, dh), int32 [N + 1] offsets, float32 [P, 3] or None);
    ValueError for anything the kernels must not see"""
    S = len(shapes)
    rows, jit, offs, any_jitter = [], [], [0], False
    for n, canvas in enumerate(pieces):
        canvas = list(canvas)
        if len(canvas) > MAX_PIECES:
            raise ValueError(f"canvas {n}: {len(canvas)} pieces, at most {MAX_PIECES}")
        rects = []
        for i, piece in enumerate(canvas):
            where = f"canvas {n}, piece {i}"
            try:
                src, crop, flip, jitter, dest = piece
                vals = [src] + list(crop) + list(dest)
                if len(crop) != 4 or len(dest) != 4 or any(int(v) != v for v in vals):
                    raise TypeError
                src, (l, t, cw, ch), (dx, dy, dw, dh) = int(src), (int(v) for v in crop), (int(v) for v in dest)
            except (TypeError, ValueError):
                raise ValueError(f"{where}: expected (src, (left, top, width, height), flip, jitter or None, (dx, dy, dw, dh)) with integer "
                                 f"boxes, got {piece!r}") from None
            if not 0 <= src < S:
                raise ValueError(f"{where}: source index {src} is not in 0..{S - 1}")
            H, W = shapes[src]
            if cw < 1 or ch < 1 or l < 0 or t < 0 or l + cw > W or t + ch > H:
                raise ValueError(f"{where}: crop (left {l}, top {t}, width {cw}, height {ch}) is empty or not inside its {H}x{W} image")
            if dw < 1 or dh < 1 or dx < 0 or dy < 0 or dx + dw > out_w or dy + dh > out_h:
                raise ValueError(f"{where}: dest rect (x {dx}, y {dy}, width {dw}, height {dh}) is empty or not inside the {out_h}x{out_w} canvas")
            k = max(_taps(cw, dw), _taps(ch, dh))
            if k > MAX_TAPS:
                raise ValueError(f"{where}: the {ch}x{cw} crop is more than 15x its {dh}x{dw} dest rect: the filter would need {k} taps "
                                 f"(> {MAX_TAPS})")
            if jitter is None:
                fs = (1.0, 1.0, 1.0)
            else:
                fs = np.asarray(jitter, dtype=np.float32)
                if fs.shape != (3,) or not np.isfinite(fs).all() or (fs < 0).any():
                    raise ValueError(f"{where}: jitter: expected three finite factors >= 0 (brightness, contrast, saturation) or None, "
                                     f"got {jitter!r}")
                any_jitter = True
            for j, (ox, oy, ow, oh) in enumerate(rects):
                if dx < ox + ow and ox < dx + dw and dy < oy + oh and oy < dy + dh:
                    raise ValueError(f"{where}: its dest rect overlaps piece {j}'s: the pieces of a canvas must be disjoint")
            rects.append((dx, dy, dw, dh))
            rows.append((src, l, t, cw, ch, 1 if flip else 0, dx, dy, dw, dh))
            jit.append(fs)
        offs.append(len(rows))
    if not rows:
        raise ValueError("no canvas has a piece: nothing to compose")
    jitter = np.asarray(jit, dtype=np.float32).reshape(-1, 3) if any_jitter else None
    return np.asarray(rows, dtype=np.int32).reshape(-1, 10), np.asarray(offs, dtype=np.int32), jitter


def compose_targets(targets, shapes, pieces, size, min_visibility=0.0):
    """the target dicts of composed canvases, on the host in float32: one dict per canvas.  Per piece (src, crop, flip, _, dest) the
    boxes of targets[src] go through `transform_targets`' steps relative to the crop -- corners in crop pixels clamped to the crop,
    the same keep rule (0.001 of the crop, min_visibility of the box's area), mirrored if flipped -- and are then mapped into the
    canvas, x = dx + x_crop * dw / cw and y = dy + y_crop * dh / ch, and normalised by the canvas (cxcywh).  A canvas's boxes and
    labels are the concatenation over its pieces in piece order.  `size` becomes the canvas size; every other key is taken from the
    target of the canvas's FIRST piece (image_id, orig_size ... then name that source only: a canvas mixes several).  A canvas without
    pieces gives empty [0, 4] boxes and [0] int64 labels."""
    out_h, out_w = _pre._out_size(size)
    new = []
    for canvas in pieces:
        canvas = list(canvas)
        if not canvas:
            new.append({"boxes": torch.zeros((0, 4), dtype=torch.float32), "labels": torch.zeros((0,), dtype=torch.int64),
                        "size": torch.as_tensor([out_h, out_w])})
            continue
        first = targets[int(canvas[0][0])]
        nt = dict(first)
        if "size" in nt:
            nt["size"] = torch.as_tensor([out_h, out_w]).to(torch.as_tensor(first["size"]))
        boxes, labels = [], []
        for src, (l, t, cw, ch), fl, _, (dx, dy, dw, dh) in canvas:
            tg = targets[int(src)]
            if "boxes" not in tg:
                continue
            H, W = shapes[int(src)]
            x1, y1, x2, y2, keep = _boxes_in_crop(tg["boxes"], H, W, (l, t, cw, ch), fl, min_visibility)
            x1, x2, y1, y2 = dx + x1 * dw / cw, dx + x2 * dw / cw, dy + y1 * dh / ch, dy + y2 * dh / ch
            boxes.append(torch.stack([(x1 + x2) / (2 * out_w), (y1 + y2) / (2 * out_h), (x2 - x1) / out_w, (y2 - y1) / out_h], dim=1)[keep])
            if "labels" in tg:
                labels.append(tg["labels"][keep.to(tg["labels"].device)])
        if "boxes" in first:
            nt["boxes"] = torch.cat(boxes).to(first["boxes"].device)
        if "labels" in first:
            nt["labels"] = torch.cat([lb.to(first["labels"].device) for lb in labels]) if labels else first["labels"][:0]
        new.append(nt)
    return new


def _launch_compose(src, src_offs, hs, ws, rows, offs, jitter, fill, per_canvas, out_h, out_w, as_uint8, out=None):
    """`dod_preprocess_compose*` on staged sources: src on the device, the rest host arrays as `_check_pieces` / `_check_fill` return
    them.  Nothing is validated here (the tests hand the kernels plans that the host would refuse); out: None or the buffer to write."""
    dev = src.device
    S, P, N = len(hs), len(rows), len(offs) - 1
    cw, ch, dw = (rows[:, k].astype(np.int64) for k in (3, 4, 8))
    tmp_offs, tmp_bytes = _pre._tmp_layout(np.maximum(ch, 0), np.maximum(dw, 0), np.maximum(cw, 0) if jitter is not None else None)
    meta = _pre._upload(dev, src_offs, hs, ws, rows, offs, tmp_offs, fill, jitter)
    lsum = _pre._luma_sums(jitter, P, dev)
    tmp = torch.empty(max(1, tmp_bytes), dtype=torch.uint8, device=dev)
    if out is None:
        out = _pre._out_buffer(N, out_h, out_w, as_uint8, dev)
    nat.check(_pre._entry("dod_preprocess_compose", as_uint8)(
        nat.ptr(src), nat.ptr(meta[0]), nat.ptr(meta[1]), nat.ptr(meta[2]), S, nat.ptr(meta[3]), nat.ptr(meta[4]), N, P, nat.ptr(meta[7]), nat.ptr(lsum),
        nat.ptr(meta[6]), int(per_canvas), int(ch.max()), int(cw.max()), int(dw.max()), out_h, out_w, nat.ptr(tmp), nat.ptr(meta[5]), nat.ptr(out),
        nat.stream_ptr()))
    return out


def compose_batch(images, targets, pieces, size, fill=(124, 116, 104), device="cuda", as_uint8=False, min_visibility=0.0):
    """images: the sources, as `preprocess_batch` takes them; targets: one target dict per source, or None; pieces: per canvas a list
    of (src, crop, flip, jitter, dest): the source index, the crop (left, top, width, height) inside that source, the flip flag, None
    or the three jitter factors, and the dest rect (dx, dy, dw, dh) inside the canvas the piece is resized into.  The dest rects of a
    canvas are pairwise disjoint; a canvas holds at most 16 pieces (none: it is all fill) and some canvas must hold one; a piece may be
    down-scaled by at most 15x in each direction (32 filter taps).  The contrast mean is that of the piece's crop, the flip mirrors
    inside the dest rect, and pieces may share a source.  fill: (r, g, b) bytes, or one triple per canvas.  Returns (batch,
    new_targets): float32 [N, 3, height, width] on `device`, or with as_uint8 the uint8 [N, height, width, 3] bytes for
    `model.forward_packed_u8`; the targets as `compose_targets` documents them.  Only the sources some piece names are staged, each
    once.  Anything wrong with the arguments raises ValueError before anything is copied or launched."""
    out_h, out_w = _pre._out_size(size)
    srcs = _pre._sources(images)
    shapes = srcs.shapes
    pieces = [list(c) for c in pieces]
    rows, offs, jitter = _check_pieces(shapes, pieces, out_h, out_w)
    fill, per_canvas = _check_fill(fill, len(pieces))
    if targets is not None and len(targets) != len(srcs):
        raise ValueError(f"targets: expected {len(srcs)} dicts (one per source), got {len(targets)}")
    if jitter is not None and (jitter == 1.0).all():
        jitter = None                                   # the geometric-only kernels
    used = np.unique(rows[:, 0])
    remap = np.full(len(srcs), -1, dtype=np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    staged = rows.copy()
    staged[:, 0] = remap[rows[:, 0]]
    src, src_offs, hs, ws = srcs.stage(torch.device(device), used)
    out = _launch_compose(src, src_offs, hs, ws, staged, offs, jitter, fill, per_canvas, out_h, out_w, as_uint8)
    new_targets = compose_targets(targets, shapes, pieces, (out_h, out_w), min_visibility) if targets is not None else None
    return out, new_targets


# --------------------------------------------------------------------------------------------------------------- geometric warp
# Random affine and perspective are one primitive (`dod_preprocess_warp`, include/dinodet.h): an inverse-map bilinear gather with
# eight coefficients per image.  Pillow's semantics, per image:
#     img.transform((out_w, out_h), Image.PERSPECTIVE, coeffs, Image.BILINEAR, fillcolor=fill)
# (an affine is coeffs[6] = coeffs[7] = 0 and gives Image.AFFINE's bytes).  The coefficients map an OUTPUT point to the SOURCE point it
# shows, on continuous coordinates where pixel i covers [i, i + 1):  with M = [[a0, a1, a2], [a3, a4, a5], [a6, a7, 1]],
# (sx, sy, 1) ~ M (x, y, 1).  The builders below work on the forward map (source -> output), which is what a user thinks in and what
# the boxes follow, and invert it.
IDENTITY_COEFFS = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
MAX_COEFF = 1e9
_EYE3 = np.eye(3)


def _matrix(coeffs):
    """eight coefficients -> the 3 x 3 matrix (output -> source)"""
    return np.append(np.asarray(coeffs, dtype=np.float64).reshape(8), 1.0).reshape(3, 3)


def _shear_pair(shear):
    s = np.atleast_1d(np.asarray(shear, dtype=np.float64))
    if s.shape not in ((1,), (2,)):
        raise ValueError(f"shear: expected an x shear in degrees or an (x, y) pair, got {shear!r}")
    return (float(s[0]), 0.0) if s.shape == (1,) else (float(s[0]), float(s[1]))


def _affine_coeffs_batch(H, W, out_h, out_w, angle, tx, ty, scale, shear_x, shear_y, cx=None, cy=None):
    """`affine_coeffs` for arrays of parameters -> float64 [B, 8], in closed form: the forward 2 x 2 block is A = scale . R(angle) .
    [[1, 0], [-tan y, 1]] . [[1, -tan x], [0, 1]] with determinant scale^2, and p_src = c_src + A^-1 (p_out - c_out - translate)"""
    H, W, out_h, out_w, angle, tx, ty, scale, shear_x, shear_y = (np.asarray(v, dtype=np.float64).reshape(-1) for v in
                                                                  (H, W, out_h, out_w, angle, tx, ty, scale, shear_x, shear_y))
    cx = 0.5 * W if cx is None else np.asarray(cx, dtype=np.float64).reshape(-1)
    cy = 0.5 * H if cy is None else np.asarray(cy, dtype=np.float64).reshape(-1)
    r, tnx, tny = np.radians(angle), np.tan(np.radians(shear_x)), np.tan(np.radians(shear_y))
    c, s = np.cos(r), np.sin(r)
    a, b = scale * (c + s * tny), scale * (-c * tnx - s * (1.0 + tny * tnx))
    d, e = scale * (s - c * tny), scale * (-s * tnx + c * (1.0 + tny * tnx))
    det = scale * scale
    with np.errstate(all="ignore"):
        i00, i01, i10, i11 = e / det, -b / det, -d / det, a / det
        ox, oy = 0.5 * out_w + tx, 0.5 * out_h + ty
        out = np.stack([i00, i01, cx - (i00 * ox + i01 * oy), i10, i11, cy - (i10 * ox + i11 * oy), np.zeros_like(det), np.zeros_like(det)], axis=1)
    if not (np.isfinite(out).all() and (det > 0.0).all()):
        raise ValueError("affine_coeffs: the map is not invertible (a scale that is not positive and finite, or a shear of 90 degrees)")
    return out + 0.0                      # (-0.0 -> 0.0)


def affine_coeffs(src_size, out_size, angle=0.0, translate=(0.0, 0.0), scale=1.0, shear=0.0, center=None):
    """the eight coefficients (the last two 0) of the affine warp whose forward map, source -> output, is
        T(center_out + translate) . R(angle) . Shear . S(scale) . T(-center_src)
    in float64.  src_size / out_size: (height, width); center_out is the middle of the output, center_src the middle of the source
    or `center` (x, y) in source pixels; angle in degrees, positive = clockwise on the screen (the y axis points down), as
    torchvision's `RandomAffine`; translate (x, y) in output pixels; scale > 0 magnifies; shear: an x shear in degrees or (x, y),
    Shear = [[1, 0], [-tan y, 1]] . [[1, -tan x], [0, 1]] (torchvision's).  The coefficients are the inverse, output -> source."""
    (H, W), (out_h, out_w) = _pre._out_size(src_size), _pre._out_size(out_size)
    sx, sy = _shear_pair(shear)
    cx, cy = (None, None) if center is None else (float(center[0]), float(center[1]))
    return _affine_coeffs_batch(H, W, out_h, out_w, float(angle), float(translate[0]), float(translate[1]), float(scale), sx, sy, cx, cy)[0]


def perspective_coeffs(src_quad, out_quad):
    """the eight coefficients of the projective warp that shows source point src_quad[i] at output point out_quad[i], i = 0..3
    (points as (x, y) on continuous coordinates): per pair  u = (a0 X + a1 Y + a2) / (a6 X + a7 Y + 1),  v = (a3 X + a4 Y + a5) /
    (a6 X + a7 Y + 1)  with (X, Y) = out_quad[i], (u, v) = src_quad[i]; the 8 x 8 system is solved in float64."""
    src, dst = np.asarray(src_quad, dtype=np.float64), np.asarray(out_quad, dtype=np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2) or not (np.isfinite(src).all() and np.isfinite(dst).all()):
        raise ValueError("perspective_coeffs: expected two lists of four finite (x, y) points")
    try:
        return _perspective_coeffs_batch(src[None], dst[None])[0]
    except np.linalg.LinAlgError:
        raise ValueError("perspective_coeffs: the point pairs do not determine a projective map (three of them on a line?)") from None


def _perspective_coeffs_batch(src, dst):
    """`perspective_coeffs` for [B, 4, 2] point lists -> float64 [B, 8]: B systems of 8 x 8, solved in one call"""
    B = len(src)
    (u, v), (X, Y) = (src[..., 0], src[..., 1]), (dst[..., 0], dst[..., 1])
    A = np.zeros((B, 4, 2, 8))
    A[:, :, 0, 0], A[:, :, 0, 1], A[:, :, 0, 2], A[:, :, 0, 6], A[:, :, 0, 7] = X, Y, 1.0, -X * u, -Y * u
    A[:, :, 1, 3], A[:, :, 1, 4], A[:, :, 1, 5], A[:, :, 1, 6], A[:, :, 1, 7] = X, Y, 1.0, -X * v, -Y * v
    return np.linalg.solve(A.reshape(B, 8, 8), src.reshape(B, 8, 1))[..., 0]


def _matrices(coeffs):
    """[B, 8] coefficients -> [B, 3, 3] matrices (output -> source)"""
    c = np.asarray(coeffs, dtype=np.float64)
    return np.concatenate([c, np.ones((len(c), 1))], axis=1).reshape(-1, 3, 3)


def compose_coeffs(a, b):
    """the coefficients of warping by `a` first and by `b` second as ONE warp (one resampling instead of two): an output point goes
    through b into the intermediate image and through a into the source, so the matrix is M(a) . M(b), renormalised to [2][2] = 1.
    a, b: [8] or [B, 8] (broadcast against each other).  Composing with the identity changes no bit."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    single = a.ndim == 1 and b.ndim == 1
    a, b = np.broadcast_arrays(np.atleast_2d(a), np.atleast_2d(b))
    M = _matrices(a) @ _matrices(b)
    if not (np.isfinite(M).all() and (M[:, 2, 2] != 0.0).all()):
        raise ValueError("the map has no representation with a[8] = 1 (its third row vanishes at the origin)")
    out = (M / M[:, 2:3, 2:3]).reshape(-1, 9)[:, :8].copy()
    return out[0] if single else out


MAX_COND = 1e10


def _coeff_faults(c, shapes, out_h, out_w):
    """float64 [B, 8] finite coefficients -> int [B]: 0 = fine; 1 = the matrix is not invertible to working precision: its condition
    number exceeds 1e10 once output and source are each scaled to the unit square (the forward map, which the boxes need, would keep
    fewer than six digits; the scaling makes the verdict independent of the image sizes, and a tiny scale or a huge offset counts
    the same as a nearly dependent row); 2 = the denominator is not positive at one of the four corner pixel centres of the output;
    3 = the forward map's third component is not positive at one of the four corners of the source.  Also the forward matrices."""
    B = len(c)
    M = _matrices(c)
    hw = np.maximum(np.asarray(shapes, dtype=np.float64).reshape(B, 2), 1.0)
    H, W = hw[:, 0], hw[:, 1]
    s_out = np.array([out_w, out_h, 1.0])
    s_src = np.stack([W, H, np.ones(B)], axis=1)
    with np.errstate(all="ignore"):
        cond = np.linalg.cond(M * s_out[None, None, :] / s_src[:, :, None])
    fault = np.where(cond <= MAX_COND, 0, 1)
    F = np.linalg.inv(np.where(fault[:, None, None] > 0, _EYE3[None], M))
    fault[~np.isfinite(F).all(axis=(1, 2))] = 1
    X = np.array([0.5, out_w - 0.5, 0.5, out_w - 0.5])
    Y = np.array([0.5, 0.5, out_h - 0.5, out_h - 0.5])
    den_ok = (c[:, 6:7] * X[None] + c[:, 7:8] * Y[None] + 1.0 > 0.0).all(axis=1)
    u, v = np.stack([0 * W, W, 0 * W, W], axis=1), np.stack([0 * H, 0 * H, H, H], axis=1)
    fwd_ok = (F[:, 2, 0:1] * u + F[:, 2, 1:2] * v + F[:, 2, 2:3] > 0.0).all(axis=1)
    fault[(fault == 0) & ~den_ok] = 2
    fault[(fault == 0) & ~fwd_ok] = 3
    return fault, F


def _check_coeffs(coeffs, shapes, out_h, out_w):
    """the coefficients as contiguous float64 [B, 8]; ValueError for anything the boxes or the kernel must not see: a wrong shape, a
    value that is not finite or beyond 1e9, a matrix that is not invertible to working precision (`_coeff_faults` has the rule), a
    denominator that is not positive at one of the four corner pixel centres of the output (it is linear, so it is then positive at
    every pixel), or a forward map whose third component is not positive at one of the four corners of the source (a box corner
    would cross the horizon)."""
    B = len(shapes)
    try:
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"coeffs: expected float64 [{B}, 8], got {type(coeffs).__name__}") from None
    if c.shape != (B, 8):
        raise ValueError(f"coeffs: expected [{B}, 8] (eight coefficients per image), got shape {c.shape}")
    if not np.isfinite(c).all() or (np.abs(c) > MAX_COEFF).any():
        raise ValueError(f"coeffs: every coefficient must be finite and at most {MAX_COEFF:g} in magnitude")
    fault, _ = _coeff_faults(c, shapes, out_h, out_w)
    if fault.any():
        b = int(np.argmax(fault > 0))
        H, W = shapes[b]
        raise ValueError(f"coeffs {b}: " + {1: f"the 3 x 3 matrix is not invertible to working precision (condition number above {MAX_COND:g} in "
                                               "unit-square coordinates)",
                                            2: f"the denominator a6 x + a7 y + 1 is not positive at every pixel centre: the horizon crosses the "
                                               f"{out_h}x{out_w} output",
                                            3: f"the forward map sends a corner of the {H}x{W} source to or beyond the horizon"}[int(fault[b])])
    return c


def warp_targets(targets, src_shapes, coeffs, size, min_visibility=0.0):
    """the reference's target dicts under the warps, on the host in float64 (the result is cast to the boxes' dtype).  Per box of an
    image [H, W]: its four corners in source pixels go through the FORWARD map (the inverse of the 3 x 3 matrix of the coefficients);
    the box becomes the axis-aligned bounding box of the four, clipped to [0, out_w] x [0, out_h]; it is kept iff it is not empty,
    its clipped width / out_w and height / out_h are >= 0.001 (dataset.py:90) and its clipped area >= min_visibility x the area of
    the unclipped bounding box; written back as normalised cxcywh of the output.  `labels` follow the same mask, `size` becomes the
    output size, every other key passes through.  An identity warp at unchanged size returns `boxes` and `labels` as they are.
    The bounding box of a rotated or sheared box is larger than the object it framed -- by up to |sin| + |cos| per side for a
    rotation: that is the standard behaviour of every box-level affine augmentation, there is no tighter answer without masks."""
    out_h, out_w = _pre._out_size(size)
    coeffs = np.asarray(coeffs, dtype=np.float64).reshape(-1, 8)
    new = []
    for tg, (H, W), c in zip(targets, src_shapes, coeffs):
        nt = dict(tg)
        if "size" in nt:
            nt["size"] = torch.as_tensor([out_h, out_w]).to(torch.as_tensor(tg["size"]))
        identity = tuple(c.tolist()) == IDENTITY_COEFFS and (int(H), int(W)) == (out_h, out_w)
        if "boxes" in nt and not identity:
            src = tg["boxes"]
            F = np.linalg.inv(_matrix(c))
            bx = src.detach().to("cpu", torch.float64).reshape(-1, 4).numpy()
            x1, x2 = (bx[:, 0] - 0.5 * bx[:, 2]) * W, (bx[:, 0] + 0.5 * bx[:, 2]) * W
            y1, y2 = (bx[:, 1] - 0.5 * bx[:, 3]) * H, (bx[:, 1] + 0.5 * bx[:, 3]) * H
            px = np.stack([x1, x2, x1, x2], axis=1)
            py = np.stack([y1, y1, y2, y2], axis=1)
            w = F[2, 0] * px + F[2, 1] * py + F[2, 2]
            qx = (F[0, 0] * px + F[0, 1] * py + F[0, 2]) / w
            qy = (F[1, 0] * px + F[1, 1] * py + F[1, 2]) / w
            ux1, ux2, uy1, uy2 = qx.min(1), qx.max(1), qy.min(1), qy.max(1)
            cx1, cx2 = np.clip(ux1, 0.0, out_w), np.clip(ux2, 0.0, out_w)
            cy1, cy2 = np.clip(uy1, 0.0, out_h), np.clip(uy2, 0.0, out_h)
            keep = (cx2 > cx1) & (cy2 > cy1) & ((cx2 - cx1) / out_w >= MIN_BOX) & ((cy2 - cy1) / out_h >= MIN_BOX) \
                & ((cx2 - cx1) * (cy2 - cy1) >= min_visibility * ((ux2 - ux1) * (uy2 - uy1)))
            out = np.stack([(cx1 + cx2) / (2 * out_w), (cy1 + cy2) / (2 * out_h), (cx2 - cx1) / out_w, (cy2 - cy1) / out_h], axis=1)[keep]
            nt["boxes"] = torch.from_numpy(out).to(src.dtype).to(src.device)
            if "labels" in nt:
                nt["labels"] = tg["labels"][torch.from_numpy(keep).to(tg["labels"].device)]
        new.append(nt)
    return new


def _launch_warp(src, src_offs, hs, ws, coeffs, fill, per_image, out_h, out_w, as_uint8, out=None):
    """`dod_preprocess_warp*` on staged sources: src on the device, the rest host arrays (coeffs float64 [B, 8], fill as `_check_fill`
    returns it).  Nothing is validated here (the tests hand the kernel what the host would refuse); out: None or the buffer to write."""
    dev = src.device
    B = len(hs)
    meta = _pre._upload(dev, src_offs, hs, ws, coeffs, fill)
    if out is None:
        out = _pre._out_buffer(B, out_h, out_w, as_uint8, dev)
    nat.check(_pre._entry("dod_preprocess_warp", as_uint8)(nat.ptr(src), nat.ptr(meta[0]), nat.ptr(meta[1]), nat.ptr(meta[2]), B, nat.ptr(meta[3]),
                                                           nat.ptr(meta[4]), int(per_image), out_h, out_w, nat.ptr(out), nat.stream_ptr()))
    return out


def warp_batch(images_u8, targets, coeffs, size, fill=(124, 116, 104), device="cuda", as_uint8=False, min_visibility=0.0):
    """images_u8: a uint8 [B, h, w, 3] tensor on the device -- the output of `augment_batch` / `compose_batch` with as_uint8, read where
    it is, not staged again -- or anything `preprocess_batch` takes (ragged sources); targets: one target dict per image, or None;
    coeffs: float64 [B, 8], output -> source, as `affine_coeffs` / `perspective_coeffs` / `compose_coeffs` build them; size: the output
    (height, width); fill: (r, g, b) bytes for every output pixel that shows no source pixel, or one triple per image.  Returns
    (batch, new_targets): float32 [B, 3, height, width] on `device`, or with as_uint8 the uint8 [B, height, width, 3] bytes for
    `model.forward_packed_u8`; the targets as `warp_targets` documents them.  The bytes are Pillow's
    `Image.transform((width, height), PERSPECTIVE, coeffs[b], BILINEAR, fillcolor=fill)`.  Anything wrong with the arguments raises
    ValueError before anything is copied or launched."""
    out_h, out_w = _pre._out_size(size)
    if out_h < 1 or out_w < 1:
        raise ValueError(f"size: expected a positive (height, width), got {size}")
    resident = isinstance(images_u8, torch.Tensor) and images_u8.is_cuda
    if resident:
        if images_u8.dtype != torch.uint8 or images_u8.ndim != 4 or images_u8.shape[3] != 3 or 0 in images_u8.shape:
            raise ValueError(f"expected a uint8 [B, h, w, 3] batch on the device, got {images_u8.dtype} {tuple(images_u8.shape)}")
        B, h, w = (int(v) for v in images_u8.shape[:3])
        shapes = [(h, w)] * B
    else:
        srcs = _pre._sources(images_u8)
        B = len(srcs)
        shapes = srcs.shapes
    coeffs = _check_coeffs(coeffs, shapes, out_h, out_w)
    fill, per_image = _check_fill(fill, B)
    if targets is not None and len(targets) != B:
        raise ValueError(f"targets: expected {B} dicts, got {len(targets)}")
    if resident:
        src = images_u8.contiguous().reshape(-1)
        src_offs = np.arange(B, dtype=np.int64) * (h * w * 3)
        hs, ws = np.full(B, h, dtype=np.int32), np.full(B, w, dtype=np.int32)
    else:
        src, src_offs, hs, ws = srcs.stage(torch.device(device))
    out = _launch_warp(src, src_offs, hs, ws, coeffs, fill, per_image, out_h, out_w, as_uint8)
    new_targets = warp_targets(targets, shapes, coeffs, (out_h, out_w), min_visibility) if targets is not None else None
    return out, new_targets


def _range_of(x, name, symmetric=True):
    """a number x -> (-x, x); a pair -> itself"""
    v = np.atleast_1d(np.asarray(x, dtype=np.float64))
    if v.shape == (1,) and symmetric:
        if not (math.isfinite(v[0]) and v[0] >= 0):
            raise ValueError(f"{name}: expected a finite number >= 0 or a (lo, hi) pair, got {x!r}")
        return -float(v[0]), float(v[0])
    if v.shape != (2,) or not (np.isfinite(v).all() and v[0] <= v[1]):
        raise ValueError(f"{name}: expected a (lo, hi) pair with lo <= hi, got {x!r}")
    return float(v[0]), float(v[1])


def sample_affine(shapes, generator, degrees=0.0, translate=(0.0, 0.0), scale=(1.0, 1.0), shear=0.0, prob=1.0, size=None):
    """one random affine per image, with `RandomAffine`'s parameter meanings -> float64 [B, 8] for `warp_batch`.  shapes: (H, W) per
    source; size: the output (height, width), None = each image's own.  With probability prob: the angle is uniform in [-degrees,
    degrees] (or in the (lo, hi) pair given), clockwise; the translation is uniform in [-tx W_out, tx W_out] x [-ty H_out, ty H_out]
    for translate = (tx, ty), rounded to whole pixels; the scale is uniform in [lo, hi] (within 0.01 .. 100); shear is an x shear
    uniform in [-shear, shear] degrees, or (x_lo, x_hi), or (x_lo, x_hi, y_lo, y_hi) (within -80 .. 80: with these limits every
    draw is a map `warp_batch` accepts); all about the image centre (`affine_coeffs`).  Otherwise the
    centred unit map -- the identity when the size does not change.  Seven numbers are drawn per image whatever the outcomes."""
    a_lo, a_hi = _range_of(degrees, "degrees")
    tx, ty = float(translate[0]), float(translate[1])
    if not (0.0 <= tx <= 1.0 and 0.0 <= ty <= 1.0):
        raise ValueError(f"translate: expected two fractions in [0, 1], got {translate}")
    s_lo, s_hi = _range_of(scale, "scale", symmetric=False)
    if not 0.01 <= s_lo <= s_hi <= 100.0:
        raise ValueError(f"scale: expected 0.01 <= lo <= hi <= 100, got {scale}")
    sh = np.atleast_1d(np.asarray(shear, dtype=np.float64))
    if sh.shape == (4,):
        (x_lo, x_hi), (y_lo, y_hi) = _range_of(sh[:2], "shear"), _range_of(sh[2:], "shear")
    else:
        (x_lo, x_hi), (y_lo, y_hi) = _range_of(shear, "shear"), (0.0, 0.0)
    if max(abs(x_lo), abs(x_hi), abs(y_lo), abs(y_hi)) > 80.0:
        raise ValueError(f"shear: expected angles within [-80, 80] degrees, got {shear}")
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"prob: expected a probability, got {prob}")
    u = torch.rand(len(shapes), 7, generator=generator, dtype=torch.float64).numpy()
    hw = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    out_hw = hw if size is None else np.broadcast_to(np.asarray(_pre._out_size(size), dtype=np.int64), hw.shape)
    H, W, out_h, out_w = hw[:, 0], hw[:, 1], out_hw[:, 0], out_hw[:, 1]
    drawn = u[:, 0] < prob
    pick = lambda k, lo, hi, neutral: np.where(drawn, lo + u[:, k] * (hi - lo), neutral)
    out = _affine_coeffs_batch(H, W, out_h, out_w, pick(1, a_lo, a_hi, 0.0), np.where(drawn, np.round((2.0 * u[:, 2] - 1.0) * tx * out_w), 0.0),
                               np.where(drawn, np.round((2.0 * u[:, 3] - 1.0) * ty * out_h), 0.0), pick(4, s_lo, s_hi, 1.0), pick(5, x_lo, x_hi, 0.0),
                               pick(6, y_lo, y_hi, 0.0))
    out[~drawn & (hw == out_hw).all(axis=1)] = IDENTITY_COEFFS
    return out


def sample_perspective(shapes, generator, distortion=0.5, prob=1.0, size=None, before=None):
    """one random perspective per image, as `RandomPerspective` -> float64 [B, 8] for `warp_batch`.  With probability prob the four
    corners of the source are shown at the four corners of the output, each moved INWARD by up to distortion x half the side:
    horizontally uniform in [0, distortion W_out / 2], vertically in [0, distortion H_out / 2], independently per corner (0 <=
    distortion < 1, so every corner stays inside its own quadrant and the quadrilateral is convex).  Where the moves are so uneven that the
    map's horizon would cross the output frame -- pixels beyond it would show the source mirrored, and `warp_batch` refuses such
    coefficients -- all eight moves of that image are halved until it does not (deterministic, no further draws; moves of zero are the
    corner-to-corner map, which always passes).  before: None, or the [B, 8] coefficients of a warp at unchanged size that runs
    before this one (`TrainAugment`'s affine): the halving then looks at the composed warp `compose_coeffs(before, result)`, whose
    horizon must clear the source's corners as the affine placed them, so the composition is always one `warp_batch` accepts.
    Otherwise the corner-to-corner map -- the identity when the size does not change.  Nine numbers are drawn per image whatever the
    outcomes."""
    if not 0.0 <= distortion < 1.0:
        raise ValueError(f"distortion: expected 0 <= distortion < 1, got {distortion}")
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"prob: expected a probability, got {prob}")
    u = torch.rand(len(shapes), 9, generator=generator, dtype=torch.float64).numpy()
    B = len(shapes)
    hw = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    out_hw = hw if size is None else np.broadcast_to(np.asarray(_pre._out_size(size), dtype=np.int64), hw.shape)
    H, W, out_h, out_w = (x.astype(np.float64) for x in (hw[:, 0], hw[:, 1], out_hw[:, 0], out_hw[:, 1]))
    drawn = (u[:, 0] < prob) & (distortion > 0.0)
    zero = np.zeros(B)
    src = np.stack([np.stack([zero, zero], 1), np.stack([W, zero], 1), np.stack([W, H], 1), np.stack([zero, H], 1)], axis=1)
    d = u[:, 1:9] * np.where(drawn, distortion * 0.5, 0.0)[:, None]          # the eight moves as fractions of the sides
    if before is not None:
        before = np.asarray(before, dtype=np.float64).reshape(B, 8)
    out = np.empty((B, 8), dtype=np.float64)
    todo = np.arange(B)
    for _ in range(64):
        m, (ow, oh) = d[todo], (out_w[todo], out_h[todo])
        quad = np.stack([np.stack([m[:, 0] * ow, m[:, 1] * oh], 1), np.stack([ow - m[:, 2] * ow, m[:, 3] * oh], 1),
                         np.stack([ow - m[:, 4] * ow, oh - m[:, 5] * oh], 1), np.stack([m[:, 6] * ow, oh - m[:, 7] * oh], 1)], axis=1)
        out[todo] = _perspective_coeffs_batch(src[todo], quad)
        # each output size on its own (in TrainAugment there is one); the check is on what `warp_batch` will be handed
        whole = out[todo] if before is None else compose_coeffs(before[todo], out[todo])
        bad = np.zeros(len(todo), dtype=bool)
        for size_ in {tuple(r) for r in out_hw[todo].tolist()}:
            sel = (out_hw[todo] == size_).all(axis=1)
            bad[sel] = _coeff_faults(whole[sel], hw[todo][sel], *size_)[0] > 0
        todo = todo[bad]
        if not len(todo):
            break
        d[todo] *= 0.5                    # halve every move of the images whose horizon crosses a frame
    out[~drawn & (hw == out_hw).all(axis=1)] = IDENTITY_COEFFS
    return out


def _uniform_int(u, lo, hi):
    """u in [0, 1) -> an integer uniform in [lo, hi]"""
    return min(hi, lo + int(u * (hi - lo + 1)))


def _check_sampler(crop_frac, brightness, contrast, saturation):
    f_lo, f_hi = float(crop_frac[0]), float(crop_frac[1])
    if not (0.0 < f_lo <= f_hi <= 1.0):
        raise ValueError(f"crop_frac: expected 0 < lo <= hi <= 1, got {crop_frac}")
    for name, x in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        if not (math.isfinite(x) and x >= 0):
            raise ValueError(f"{name}: expected a finite range >= 0, got {x}")
    return f_lo, f_hi


def _draw_one(u, H, W, crop_prob, f_lo, f_hi, hflip_prob, ranges):
    """one image's (crop (l, t, w, h), flip, three float32 factors) from its nine uniform numbers u"""
    H, W = int(H), int(W)
    w, h, l, t = W, H, 0, 0
    if u[0] < crop_prob:
        w_lo, h_lo = max(1, math.ceil(f_lo * W)), max(1, math.ceil(f_lo * H))
        w = _uniform_int(u[1], w_lo, max(w_lo, math.floor(f_hi * W)))
        h = _uniform_int(u[2], h_lo, max(h_lo, math.floor(f_hi * H)))
        l, t = _uniform_int(u[3], 0, W - w), _uniform_int(u[4], 0, H - h)
    fs = []
    for k, x in enumerate(ranges):
        lo, hi = max(0.0, 1.0 - x), 1.0 + x
        f = np.float32(lo + u[6 + k] * (hi - lo))
        if float(f) > hi:                     # float32 rounding must not leave the range
            f = np.nextafter(f, np.float32(0))
        elif float(f) < lo:
            f = np.nextafter(f, np.float32(2))
        fs.append(f)
    return (l, t, w, h), bool(u[5] < hflip_prob), fs


def sample_params(shapes, generator, crop_prob=0.5, crop_frac=(0.5, 1.0), hflip_prob=0.5, brightness=0.0, contrast=0.0, saturation=0.0):
    """shapes: (H, W) per image; generator: a CPU torch.Generator, the only source of randomness.  With probability crop_prob the
    crop's width is uniform in [ceil(f_lo W), floor(f_hi W)], its height likewise, its offset uniform over what fits; otherwise the
    whole image.  Flip with probability hflip_prob.  Each jitter factor is uniform in [max(0, 1 - x), 1 + x] (torchvision's
    convention; x = 0 gives exactly 1.0).  Returns (crops int32 [B, 4], flips uint8 [B], jitter float32 [B, 3]); every call draws
    the same nine numbers per image, so the same seed and shapes give the same parameters whatever the outcomes."""
    B = len(shapes)
    f_lo, f_hi = _check_sampler(crop_frac, brightness, contrast, saturation)
    u = torch.rand(B, 9, generator=generator, dtype=torch.float64).numpy()
    crops = np.zeros((B, 4), dtype=np.int32)
    flips = np.zeros(B, dtype=np.uint8)
    jitter = np.ones((B, 3), dtype=np.float32)
    for b, (H, W) in enumerate(shapes):
        crops[b], flips[b], jitter[b] = _draw_one(u[b], H, W, crop_prob, f_lo, f_hi, hflip_prob, (brightness, contrast, saturation))
    return crops, flips, jitter


def _fit_taps(crop, dw, dh):
    """the crop (l, t, w, h) shrunk, about its own centre, until a dw x dh dest rect needs at most 32 taps: a width above 15 dw
    becomes 15 dw and the left edge moves right by half the difference (rounded down); likewise vertically.  Deterministic; a crop
    within the bound comes back unchanged."""
    l, t, w, h = crop
    lim = (MAX_TAPS - 1) // 2
    if w > lim * dw:
        l, w = l + (w - lim * dw) // 2, lim * dw
    if h > lim * dh:
        t, h = t + (h - lim * dh) // 2, lim * dh
    return l, t, w, h


def _piece(src, u, shape, dest, crop_prob, f_lo, f_hi, hflip_prob, ranges):
    crop, flip, fs = _draw_one(u, shape[0], shape[1], crop_prob, f_lo, f_hi, hflip_prob, ranges)
    jitter = None if all(x == 0 for x in ranges) else tuple(float(f) for f in fs)
    return src, _fit_taps(crop, dest[2], dest[3]), flip, jitter, dest


def sample_mosaic(shapes, generator, size=(224, 224), center=(0.25, 0.75), crop_prob=0.5, crop_frac=(0.5, 1.0), hflip_prob=0.5,
                  brightness=0.0, contrast=0.0, saturation=0.0):
    """one four-piece mosaic per image of the batch, as `compose_batch` takes it: a list per canvas of (src, crop, flip, jitter,
    dest).  Per canvas n of size (out_h, out_w): the centre cx is uniform over the integers of [c_lo out_w, c_hi out_w] clamped to
    1 .. out_w - 1, cy likewise, so every quadrant is at least one pixel wide; the quadrants (top left, top right, bottom left,
    bottom right) tile the canvas.  The top left one shows image n; the other three show partners drawn from the batch: without
    replacement from the other images when the batch has at least four, else with replacement from all of it.  Every piece draws its
    crop, flip and jitter by `sample_params`' rules on its own image; a crop that would need more than 32 filter taps for its
    quadrant is shrunk about its centre to 15x the quadrant (`_fit_taps`), so every plan is valid.  41 numbers are drawn per canvas
    whatever the outcomes: the same seed and shapes give the same plan."""
    out_h, out_w = _pre._out_size(size)
    B = len(shapes)
    f_lo, f_hi = _check_sampler(crop_frac, brightness, contrast, saturation)
    c_lo, c_hi = float(center[0]), float(center[1])
    if not (0.0 <= c_lo <= c_hi <= 1.0):
        raise ValueError(f"center: expected 0 <= lo <= hi <= 1, got {center}")
    if out_h < 2 or out_w < 2:
        raise ValueError(f"a mosaic needs a canvas of at least 2x2, got {out_h}x{out_w}")
    ranges = (brightness, contrast, saturation)
    u = torch.rand(B, 41, generator=generator, dtype=torch.float64).numpy()
    plan = []
    for n in range(B):
        cs = []
        for k, o in enumerate((out_w, out_h)):
            lo = min(o - 1, max(1, math.ceil(c_lo * o)))
            cs.append(_uniform_int(u[n, k], lo, min(o - 1, max(lo, math.floor(c_hi * o)))))
        cx, cy = cs
        if B >= 4:
            pool = [i for i in range(B) if i != n]
            partners = [pool.pop(_uniform_int(u[n, 2 + k], 0, len(pool) - 1)) for k in range(3)]
        else:
            partners = [_uniform_int(u[n, 2 + k], 0, B - 1) for k in range(3)]
        dests = [(0, 0, cx, cy), (cx, 0, out_w - cx, cy), (0, cy, cx, out_h - cy), (cx, cy, out_w - cx, out_h - cy)]
        plan.append([_piece(s, u[n, 5 + 9 * q:14 + 9 * q], shapes[s], dests[q], crop_prob, f_lo, f_hi, hflip_prob, ranges)
                     for q, s in enumerate([n] + partners)])
    return plan


def sample_zoom_out(shapes, generator, size=(224, 224), ratio=(1.0, 2.0), crop_prob=0.5, crop_frac=(0.5, 1.0), hflip_prob=0.5,
                    brightness=0.0, contrast=0.0, saturation=0.0):
    """one zoom-out (SSD "expand") per image, as `compose_batch` takes it: canvas n holds one piece of image n, of size
    round(out / r) (at least one pixel) with r uniform in [r_lo, r_hi] (1 <= r_lo), at an offset uniform over what fits; the rest of
    the canvas is the fill.  Crop, flip and jitter by `sample_params`' rules, the crop shrunk by `_fit_taps` where the piece would
    need more than 32 taps.  12 numbers per canvas."""
    out_h, out_w = _pre._out_size(size)
    f_lo, f_hi = _check_sampler(crop_frac, brightness, contrast, saturation)
    r_lo, r_hi = float(ratio[0]), float(ratio[1])
    if not (1.0 <= r_lo <= r_hi and math.isfinite(r_hi)):
        raise ValueError(f"ratio: expected 1 <= lo <= hi, got {ratio}")
    u = torch.rand(len(shapes), 12, generator=generator, dtype=torch.float64).numpy()
    plan = []
    for n, shape in enumerate(shapes):
        r = r_lo + u[n, 0] * (r_hi - r_lo)
        dw, dh = min(out_w, max(1, round(out_w / r))), min(out_h, max(1, round(out_h / r)))
        dest = (_uniform_int(u[n, 1], 0, out_w - dw), _uniform_int(u[n, 2], 0, out_h - dh), dw, dh)
        plan.append([_piece(n, u[n, 3:12], shape, dest, crop_prob, f_lo, f_hi, hflip_prob, (brightness, contrast, saturation))])
    return plan


class TrainAugment:
    """Training counterpart of `ResizeToTensor`: `TrainAugment((224, 224), brightness=0.4, ...)(images, targets)` draws one crop,
    flip flag and jitter per image (`sample_params`) and returns `augment_batch`'s (batch, new_targets).

    With mosaic_prob or zoom_out_prob above 0 every output image is a composed canvas: per canvas a mosaic (`sample_mosaic`) with
    probability mosaic_prob, else a zoom-out (`sample_zoom_out`) with probability zoom_out_prob, else the plain chain as a single
    piece covering the canvas; the whole batch is one `compose_batch` call on the `fill` colour.  With both at 0 the call is the
    one above: the same random numbers, the same `augment_batch`.

    With affine_prob or perspective_prob above 0 a geometric warp follows as a last stage, at the output size: the chain or the
    composed canvas above is produced as uint8 bytes on the device, then every image draws a random affine (`sample_affine`: degrees,
    translate, scale, shear) with probability affine_prob and a random perspective (`sample_perspective`: distortion) with probability
    perspective_prob -- both drawn AFTER all the draws above, composed into one warp when both come out, the identity (a bit-for-bit
    copy) when neither does -- and one `warp_batch` call writes the final batch, exposed pixels in the `fill` colour.  Per image that
    is Pillow's  chain(...).transform((w, h), PERSPECTIVE, coeffs, BILINEAR, fillcolor=fill): the antialiased resize stays Pillow's
    and the fill is never jittered.  With both at 0 nothing of this happens: the same random numbers, the same launches as before."""

    def __init__(self, size=(224, 224), crop_prob=0.5, crop_frac=(0.5, 1.0), hflip_prob=0.5, brightness=0.0, contrast=0.0, saturation=0.0,
                 generator=None, device="cuda", as_uint8=False, min_visibility=0.0, mosaic_prob=0.0, mosaic_center=(0.25, 0.75),
                 zoom_out_prob=0.0, zoom_out_ratio=(1.0, 2.0), fill=(124, 116, 104), affine_prob=0.0, degrees=0.0, translate=(0.0, 0.0),
                 scale=(1.0, 1.0), shear=0.0, perspective_prob=0.0, distortion=0.0):
        self.size, self.device, self.as_uint8, self.min_visibility = size, device, as_uint8, min_visibility
        self.sampler = dict(crop_prob=crop_prob, crop_frac=crop_frac, hflip_prob=hflip_prob, brightness=brightness, contrast=contrast,
                            saturation=saturation)
        self.generator = generator if generator is not None else torch.default_generator
        for name, p in (("mosaic_prob", mosaic_prob), ("zoom_out_prob", zoom_out_prob), ("affine_prob", affine_prob),
                        ("perspective_prob", perspective_prob)):
            if not 0.0 <= p <= 1.0:
                raise ValueError(f"{name}: expected a probability, got {p}")
        self.mosaic_prob, self.mosaic_center, self.zoom_out_prob, self.zoom_out_ratio, self.fill = \
            mosaic_prob, mosaic_center, zoom_out_prob, zoom_out_ratio, fill
        self.affine_prob, self.perspective_prob, self.distortion = affine_prob, perspective_prob, distortion
        self.affine = dict(degrees=degrees, translate=translate, scale=scale, shear=shear)
        if affine_prob > 0.0 or perspective_prob > 0.0:      # a bad range raises here, not at the first batch (nothing is drawn for no image)
            sample_affine([], self.generator, **self.affine)
            sample_perspective([], self.generator, distortion)

    def sample_warp(self, B):
        """the warp coefficients of one batch, float64 [B, 8] at the output size: a fixed count of numbers per call (16 per image),
        whichever warps come out; an image that draws neither gets the identity"""
        shapes = [_pre._out_size(self.size)] * B
        a = sample_affine(shapes, self.generator, prob=self.affine_prob, **self.affine)
        p = sample_perspective(shapes, self.generator, self.distortion, prob=self.perspective_prob, before=a)
        return compose_coeffs(a, p)

    def sample_plan(self, shapes):
        """the pieces of one batch (`compose_batch`'s `pieces`): a fixed count of numbers per call, whichever kinds come out"""
        B = len(shapes)
        kind = torch.rand(B, 2, generator=self.generator, dtype=torch.float64).numpy()
        mosaic = sample_mosaic(shapes, self.generator, self.size, self.mosaic_center, **self.sampler)
        zoom = sample_zoom_out(shapes, self.generator, self.size, self.zoom_out_ratio, **self.sampler)
        crops, flips, jitter = sample_params(shapes, self.generator, **self.sampler)
        out_h, out_w = _pre._out_size(self.size)
        # (a plain crop beyond 15x the canvas is shrunk like any other piece; `augment_batch` would refuse it)
        plain = [[(n, _fit_taps(tuple(int(v) for v in crops[n]), out_w, out_h), bool(flips[n]), tuple(float(f) for f in jitter[n]),
                   (0, 0, out_w, out_h))] for n in range(B)]
        return [mosaic[n] if kind[n, 0] < self.mosaic_prob else zoom[n] if kind[n, 1] < self.zoom_out_prob else plain[n] for n in range(B)]

    def __call__(self, images, targets=None):
        arrs = _pre._sources(images)
        shapes = arrs.shapes
        warp = self.affine_prob > 0.0 or self.perspective_prob > 0.0
        as_uint8 = self.as_uint8 or warp                    # the warp reads the bytes
        if self.mosaic_prob == 0.0 and self.zoom_out_prob == 0.0:
            crops, flips, jitter = sample_params(shapes, self.generator, **self.sampler)
            out = augment_batch(arrs, targets, crops, flips, jitter, self.size, self.device, as_uint8, self.min_visibility)
        else:
            out = compose_batch(arrs, targets, self.sample_plan(shapes), self.size, self.fill, self.device, as_uint8, self.min_visibility)
        if not warp:
            return out
        return warp_batch(out[0], out[1], self.sample_warp(len(out[0])), self.size, self.fill, self.device, self.as_uint8, self.min_visibility)


def collate_raw(batch):
    """collate_fn of a DataLoader over undecorated (uint8 image, target) pairs: (list of images, list of targets), nothing
    stacked -- the images are ragged until `TrainAugment` has resized them"""
    images, targets = zip(*batch)
    return list(images), list(targets)
