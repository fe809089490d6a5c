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
"""
import math

import numpy as np
import torch

from . import _native as nat
from . import preprocess as _pre

MIN_BOX = 0.001        # the reference dataset's own minimum normalised width / height (dataset.py:90)
MAX_TAPS = 32          # csrc/preproc.hip PP_MAXK: ceil(crop / out) * 2 + 1 filter taps at most (down-scaling up to 15x)


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
    kh, kv = -(-int(crops[:, 2].max()) // out_w) * 2 + 1, -(-int(crops[:, 3].max()) // out_h) * 2 + 1
    if kh > MAX_TAPS or kv > MAX_TAPS:
        raise ValueError(f"a crop is more than 15x the output {out_h}x{out_w}: the filter would need {max(kh, kv)} taps (> {MAX_TAPS})")
    return crops.astype(np.int32), flips, jitter


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
            bx = src.detach().to("cpu", torch.float32).reshape(-1, 4)
            cx, cy, bw, bh = bx.unbind(1)
            x1 = ((cx - 0.5 * bw) * W - l).clamp(0, cw)
            x2 = ((cx + 0.5 * bw) * W - l).clamp(0, cw)
            y1 = ((cy - 0.5 * bh) * H - t).clamp(0, ch)
            y2 = ((cy + 0.5 * bh) * H - t).clamp(0, ch)
            keep = (x2 > x1) & (y2 > y1) & ((x2 - x1) / cw >= MIN_BOX) & ((y2 - y1) / ch >= MIN_BOX) \
                & ((x2 - x1) * (y2 - y1) >= min_visibility * ((bw * W) * (bh * H)))
            if fl:
                x1, x2 = cw - x2, cw - x1
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
    arrs = _pre._as_arrays(images)
    B = len(arrs)
    shapes = [a.shape[:2] for a in arrs]
    crops, flips, jitter = _check_params(shapes, crops, flips, jitter, out_h, out_w)
    if targets is not None and len(targets) != B:
        raise ValueError(f"targets: expected {B} dicts, got {len(targets)}")
    if jitter is not None and (jitter == 1.0).all():
        jitter = None                                   # the geometric-only kernel
    dev = torch.device(device)
    src, src_offs, hs, ws = _pre._stage(arrs, dev)
    # per image: the horizontal pass's rows and, with jitter, the jittered crop behind them
    tsz = crops[:, 3].astype(np.int64) * (out_w + (crops[:, 2].astype(np.int64) if jitter is not None else 0)) * 3
    tmp_offs = np.concatenate([[0], np.cumsum(tsz)[:-1]]).astype(np.int64)
    meta = [torch.from_numpy(x).to(dev) for x in (src_offs, hs, ws, tmp_offs, crops, flips)]
    jit = torch.from_numpy(jitter).to(dev) if jitter is not None else None
    # the luma sums of the contrast step: only when some image has a contrast factor != 1 (the reduction is not launched otherwise)
    lsum = torch.empty(B, dtype=torch.int64, device=dev) if jitter is not None and (jitter[:, 1] != 1.0).any() else None
    tmp = torch.empty(int(tsz.sum()), dtype=torch.uint8, device=dev)
    if as_uint8:
        out = torch.empty(B, out_h, out_w, 3, dtype=torch.uint8, device=dev)
        fn = nat.lib().dod_preprocess_aug_u8
    else:
        out = torch.empty(B, 3, out_h, out_w, dtype=torch.float32, device=dev)
        fn = nat.lib().dod_preprocess_aug
    nat.check(fn(nat.ptr(src), nat.ptr(meta[0]), nat.ptr(meta[1]), nat.ptr(meta[2]), B, nat.ptr(meta[4]), nat.ptr(meta[5]), nat.ptr(jit),
                 nat.ptr(lsum), int(crops[:, 3].max()), int(crops[:, 2].max()), out_h, out_w, nat.ptr(tmp), nat.ptr(meta[3]), nat.ptr(out),
                 nat.stream_ptr()))
    new_targets = transform_targets(targets, shapes, crops, flips, (out_h, out_w), min_visibility) if targets is not None else None
    return out, new_targets


def _uniform_int(u, lo, hi):
    """u in [0, 1) -> an integer uniform in [lo, hi]"""
    return min(hi, lo + int(u * (hi - lo + 1)))


def sample_params(shapes, generator, crop_prob=0.5, crop_frac=(0.5, 1.0), hflip_prob=0.5, brightness=0.0, contrast=0.0, saturation=0.0):
    """shapes: (H, W) per image; generator: a CPU torch.Generator, the only source of randomness.  With probability crop_prob the
    crop's width is uniform in [ceil(f_lo W), floor(f_hi W)], its height likewise, its offset uniform over what fits; otherwise the
    whole image.  Flip with probability hflip_prob.  Each jitter factor is uniform in [max(0, 1 - x), 1 + x] (torchvision's
    convention; x = 0 gives exactly 1.0).  Returns (crops int32 [B, 4], flips uint8 [B], jitter float32 [B, 3]); every call draws
    the same nine numbers per image, so the same seed and shapes give the same parameters whatever the outcomes."""
    B = len(shapes)
    f_lo, f_hi = float(crop_frac[0]), float(crop_frac[1])
    if not (0.0 < f_lo <= f_hi <= 1.0):
        raise ValueError(f"crop_frac: expected 0 < lo <= hi <= 1, got {crop_frac}")
    for name, x in (("brightness", brightness), ("contrast", contrast), ("saturation", saturation)):
        if not (math.isfinite(x) and x >= 0):
            raise ValueError(f"{name}: expected a finite range >= 0, got {x}")
    u = torch.rand(B, 9, generator=generator, dtype=torch.float64).numpy()
    crops = np.zeros((B, 4), dtype=np.int32)
    flips = np.zeros(B, dtype=np.uint8)
    jitter = np.ones((B, 3), dtype=np.float32)
    for b, (H, W) in enumerate(shapes):
        H, W = int(H), int(W)
        w, h, l, t = W, H, 0, 0
        if u[b, 0] < crop_prob:
            w_lo, h_lo = max(1, math.ceil(f_lo * W)), max(1, math.ceil(f_lo * H))
            w = _uniform_int(u[b, 1], w_lo, max(w_lo, math.floor(f_hi * W)))
            h = _uniform_int(u[b, 2], h_lo, max(h_lo, math.floor(f_hi * H)))
            l, t = _uniform_int(u[b, 3], 0, W - w), _uniform_int(u[b, 4], 0, H - h)
        crops[b] = (l, t, w, h)
        flips[b] = u[b, 5] < hflip_prob
        for k, x in enumerate((brightness, contrast, saturation)):
            lo, hi = max(0.0, 1.0 - x), 1.0 + x
            f = np.float32(lo + u[b, 6 + k] * (hi - lo))
            if float(f) > hi:                     # float32 rounding must not leave the range
                f = np.nextafter(f, np.float32(0))
            elif float(f) < lo:
                f = np.nextafter(f, np.float32(2))
            jitter[b, k] = f
    return crops, flips, jitter


class TrainAugment:
    """Training counterpart of `ResizeToTensor`: `TrainAugment((224, 224), brightness=0.4, ...)(images, targets)` draws one crop,
    flip flag and jitter per image (`sample_params`) and returns `augment_batch`'s (batch, new_targets)."""

    def __init__(self, size=(224, 224), crop_prob=0.5, crop_frac=(0.5, 1.0), hflip_prob=0.5, brightness=0.0, contrast=0.0, saturation=0.0,
                 generator=None, device="cuda", as_uint8=False, min_visibility=0.0):
        self.size, self.device, self.as_uint8, self.min_visibility = size, device, as_uint8, min_visibility
        self.sampler = dict(crop_prob=crop_prob, crop_frac=crop_frac, hflip_prob=hflip_prob, brightness=brightness, contrast=contrast,
                            saturation=saturation)
        self.generator = generator if generator is not None else torch.default_generator

    def __call__(self, images, targets=None):
        arrs = _pre._as_arrays(images)
        crops, flips, jitter = sample_params([a.shape[:2] for a in arrs], self.generator, **self.sampler)
        return augment_batch(arrs, targets, crops, flips, jitter, self.size, self.device, self.as_uint8, self.min_visibility)


def collate_raw(batch):
    """collate_fn of a DataLoader over undecorated (uint8 image, target) pairs: (list of images, list of targets), nothing
    stacked -- the images are ragged until `TrainAugment` has resized them"""
    images, targets = zip(*batch)
    return list(images), list(targets)
