"""Input pipeline on the GPU: the host side of `dod_preprocess` (include/dinodet.h).

The reference prepares every image on the host with `transforms.Compose([Resize((224, 224)), ToTensor()])`
(dino_detector/train.py:584-587: Pillow's antialiased bilinear resample, then uint8 -> float32 / 255 in CHW order) inside the
DataLoader workers.  `preprocess_batch` does the same for a ragged batch of decoded uint8 images in two kernels, bit-exact
against Pillow, and returns the `[B, 3, R, R]` fp32 batch already resident on the device for `model(images)`.
No CPU fallback: without the HIP library this module raises.
"""
import numpy as np
import torch

from . import _native as nat


_STAGE = None
_STAGE_BUSY = None      # event recorded after the last async copy out of the staging buffer


def _staging(nbytes):
    global _STAGE
    if _STAGE_BUSY is not None:
        _STAGE_BUSY.synchronize()          # the previous batch's DMA must have left the buffer before it is refilled
    if _STAGE is None or _STAGE.numel() < nbytes:
        _STAGE = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    return _STAGE


def _staging_sent():
    """after the last async copy out of the staging buffer has been queued: `_staging` waits for this event before the next refill"""
    global _STAGE_BUSY
    _STAGE_BUSY = torch.cuda.Event()
    _STAGE_BUSY.record()


def _as_arrays(images):
    """the batch as contiguous uint8 [H, W, 3] numpy arrays"""
    arrs = []
    for im in images:
        a = im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"expected uint8 RGB images [H, W, 3], got {a.dtype} {a.shape}")
        arrs.append(np.ascontiguousarray(a))
    if not arrs:
        raise ValueError("empty batch")
    return arrs


def _stage(arrs, dev):
    """the raw bytes gathered straight into a (cached) pinned staging buffer: one host copy, one DMA to the device.
    Returns (src on the device, src_offs, heights, widths) -- the last three on the host."""
    hs = np.array([a.shape[0] for a in arrs], dtype=np.int32)
    ws = np.array([a.shape[1] for a in arrs], dtype=np.int32)
    sizes = hs.astype(np.int64) * ws * 3
    src_offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    total = int(sizes.sum())
    stage = _staging(total)
    sv = stage.numpy()
    for a, o in zip(arrs, src_offs):
        sv[o:o + a.size] = a.reshape(-1)
    src = stage[:total].to(dev, non_blocking=True)
    _staging_sent()
    return src, src_offs, hs, ws


class Staged:
    """A batch of ragged uint8 RGB sources that already sits on the device in `_stage`'s layout: `src` (uint8, the images' HWC bytes
    back to back) with `src_offs` (int64), `heights` and `widths` (int32) on the host.  Every entry point that takes `images`
    takes one of these instead and then copies nothing: `jpeg.decode_jpeg_batch` returns one (`DecodedBatch`)."""

    def __init__(self, src, src_offs, heights, widths):
        self.src = src
        self.src_offs = np.ascontiguousarray(src_offs, dtype=np.int64)
        self.heights = np.ascontiguousarray(heights, dtype=np.int32)
        self.widths = np.ascontiguousarray(widths, dtype=np.int32)

    def __len__(self):
        return len(self.heights)

    @property
    def shapes(self):
        return [(int(h), int(w)) for h, w in zip(self.heights, self.widths)]

    def stage(self, dev, used=None):
        """(src, src_offs, heights, widths) of the images `used` (all of them by default), as `_stage` returns them"""
        d = torch.device(dev)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())      # a bare "cuda" is where the caller's metadata will go
        if d != self.src.device:
            raise ValueError(f"the batch was decoded on {self.src.device}, not on {dev}")
        if used is None:
            return self.src, self.src_offs, self.heights, self.widths
        return self.src, self.src_offs[used], self.heights[used], self.widths[used]


class _HostImages:
    """the same two questions -- shapes, stage -- for images that are still on the host"""

    def __init__(self, images):
        self.arrs = _as_arrays(images)

    def __len__(self):
        return len(self.arrs)

    @property
    def shapes(self):
        return [a.shape[:2] for a in self.arrs]

    def stage(self, dev, used=None):
        return _stage(self.arrs if used is None else [self.arrs[i] for i in used], dev)


def _sources(images):
    """what an entry point does with its `images` argument: a `Staged` batch (or what an outer entry point already opened) passes
    through, anything else is validated as host images"""
    return images if isinstance(images, (Staged, _HostImages)) else _HostImages(images)


def _out_size(size):
    return (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))


def _tmp_layout(rows, out_w, jitter_w=None):
    """the temporary of the two-pass resize as (byte offsets int64 [n], total bytes): per output the horizontal pass's `rows` rows of
    out_w RGB pixels and, with jitter, the jittered crop of jitter_w pixels a row behind them"""
    tsz = rows.astype(np.int64) * (out_w + (0 if jitter_w is None else jitter_w.astype(np.int64))) * 3
    return np.concatenate([[0], np.cumsum(tsz)[:-1]]).astype(np.int64), int(tsz.sum())


def _out_buffer(n, out_h, out_w, as_uint8, dev):
    """the batch every entry point of the input pipeline returns: the bytes [n, height, width, 3] or float32 [n, 3, height, width]"""
    if as_uint8:
        return torch.empty(n, out_h, out_w, 3, dtype=torch.uint8, device=dev)
    return torch.empty(n, 3, out_h, out_w, dtype=torch.float32, device=dev)


def _entry(name, as_uint8):
    """the C entry `name` for the float32 CHW output, or its `_u8` twin for the uint8 HWC bytes"""
    return getattr(nat.lib(), name + "_u8" if as_uint8 else name)


def _upload(dev, *arrays):
    """host metadata arrays -> device tensors, one copy each (None stays None)"""
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays]


def _luma_sums(jitter, n, dev):
    """the luma sums of the contrast step: only when some item has a contrast factor != 1 (the reduction is not launched otherwise)"""
    return torch.empty(n, dtype=torch.int64, device=dev) if jitter is not None and (jitter[:, 1] != 1.0).any() else None


def preprocess_batch(images, size=(224, 224), device="cuda", as_uint8=False):
    """images: sequence of uint8 RGB images [H_i, W_i, 3] (numpy arrays, torch tensors or PIL images), or a `Staged` batch that is on
    the device already (`jpeg.decode_jpeg_batch`); size: (height, width) as torchvision's Resize takes it.  Returns float32 [B, 3, height, width] on `device` -- or, with as_uint8, the resampled
    bytes uint8 [B, height, width, 3] (before ToTensor) for `model.forward_packed_u8`, whose patch-embedding kernel divides by 255
    in its load stage: the fp32 batch then never goes through HBM."""
    out_h, out_w = _out_size(size)
    srcs = _sources(images)
    B = len(srcs)
    dev = torch.device(device)
    src, src_offs, hs, ws = srcs.stage(dev)
    tmp_offs, tmp_bytes = _tmp_layout(hs, out_w)
    meta = _upload(dev, src_offs, hs, ws, tmp_offs)
    tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
    out = _out_buffer(B, out_h, out_w, as_uint8, dev)
    nat.check(_entry("dod_preprocess", as_uint8)(nat.ptr(src), nat.ptr(meta[0]), nat.ptr(meta[1]), nat.ptr(meta[2]), B, int(hs.max()), int(ws.max()),
                                                 out_h, out_w, nat.ptr(tmp), nat.ptr(meta[3]), nat.ptr(out), nat.stream_ptr()))
    return out


class ResizeToTensor:
    """Batch counterpart of `transforms.Compose([transforms.Resize(size), transforms.ToTensor()])` (train.py:584-587)."""

    def __init__(self, size=(224, 224), device="cuda", as_uint8=False):
        self.size, self.device, self.as_uint8 = size, device, as_uint8

    def __call__(self, images):
        return preprocess_batch(images, self.size, self.device, self.as_uint8)
