"""ROI embeddings from the backbone tokens: the host side of `dod_roi_embed` (include/dinodet.h).

Every forward leaves the DINOv2 patch tokens -- the decoder's memory -- in HBM.  `roi_embed` pools one unit vector per box from them by
torchvision's aligned ROIAlign rules (the mean of grid x grid bilinear samples, then L2 normalisation): the appearance feature of
`tracking.Tracker(appearance=True)`, and as boxes -> unit vectors also the building block for retrieval and few-shot labelling on the
same backbone.

    det, emb = model.detect_embed(frames, top_k=100)           # Detections and [B, K, D] unit vectors, one forward
    emb = model.embed(frames, boxes)                            # caller-supplied pixel boxes [B, K, 4]
    emb = roi_embed(memory, boxes, sizes=(H, W), grid_hw=(H // 14, W // 14))

One launch on the current stream, no host sync.  tests/roi_embed_cases.py restates the arithmetic in numpy.  No CPU fallback: without the
HIP library and a GPU this module raises.
"""
import math

import torch

from . import _native as nat
from .postprocess import MAX_TOP_K, _sizes_rows

MAX_DIM = 2048                          # include/dinodet.h dod_roi_embed: channels (a multiple of 4)
MAX_GRID = 8                            # samples per axis


def spatial_factor(hw):
    """hw tokens -> (h, w): the square when hw is one, else the factorisation closest to it (h <= w) -- what the decoder's deformable
    attention assumes about its memory"""
    s = math.isqrt(hw)
    if s * s != hw:
        for i in range(s, 0, -1):
            if hw % i == 0:
                return i, hw // i
    return s, s


def roi_embed(features, boxes, counts=None, sizes=None, grid=4, first_token=1, grid_hw=None):
    """features [B, N, D] fp32 CUDA (Engine.forward_mem's memory, or backbone features), boxes [B, K, 4] fp32 xyxy in the frame `sizes`
    gives (one (height, width), one pair per image, a [B, 2] tensor; None = normalised boxes), counts [B] int32 or None (= every row) ->
    [B, K, D] fp32: the L2-normalised mean of grid x grid bilinear samples of the token map under every box.  The tokens first_token ..
    first_token + gh * gw - 1 of an image are its gh x gw map (first_token = 1 skips CLS); grid_hw = (gh, gw), None = the near-square
    factorisation of N - first_token.  Rows at and beyond counts, boxes with a non-finite coordinate or without area and boxes wholly
    outside the image come out as zeros."""
    if not (isinstance(features, torch.Tensor) and features.dtype == torch.float32 and features.dim() == 3):
        raise ValueError("features must be a CUDA fp32 tensor [B, N, D]")
    B, N, D = (int(v) for v in features.shape)
    if B < 1 or not 4 <= D <= MAX_DIM or D % 4:
        raise ValueError(f"features must hold at least one image and 4..{MAX_DIM} channels, a multiple of 4, got {tuple(features.shape)}")
    if not (isinstance(boxes, torch.Tensor) and boxes.dtype == torch.float32 and boxes.dim() == 3 and boxes.shape[0] == B and boxes.shape[2] == 4):
        raise ValueError(f"boxes must be a fp32 tensor [{B}, K, 4]")
    K = int(boxes.shape[1])
    if not 1 <= K <= MAX_TOP_K:
        raise ValueError(f"boxes must hold 1..{MAX_TOP_K} rows per image, got {K}")
    if counts is not None and not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int32 and tuple(counts.shape) == (B,)):
        raise ValueError(f"counts must be None or an int32 tensor [{B}]")
    if int(grid) != grid or not 1 <= int(grid) <= MAX_GRID:
        raise ValueError(f"grid must be an integer in 1..{MAX_GRID}, got {grid}")
    first = int(first_token)
    if first != first_token or not 0 <= first < N:
        raise ValueError(f"first_token must be an integer in 0..{N - 1}, got {first_token}")
    gh, gw = spatial_factor(N - first) if grid_hw is None else (int(grid_hw[0]), int(grid_hw[1]))
    if gh < 1 or gw < 1 or first + gh * gw > N:
        raise ValueError(f"grid_hw {gh} x {gw} from token {first} does not fit {N} tokens")
    st = _sizes_rows(sizes, B)
    if not (features.is_cuda and boxes.is_cuda and (counts is None or counts.is_cuda)):      # last: every argument is checked whether or not a GPU is present
        raise ValueError("features, boxes and counts must be on the GPU (there is no CPU fallback)")
    dev = features.device
    if boxes.device != dev or (counts is not None and counts.device != dev):
        raise ValueError(f"features are on {dev}, boxes on {boxes.device}")
    f, bx = features.contiguous(), boxes.contiguous()
    ct = None if counts is None else counts.contiguous()
    if st is not None:
        st = st.to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        emb = torch.empty(B, K, D, dtype=torch.float32, device=dev)
        nat.check(nat.lib().dod_roi_embed(nat.ptr(f), B, N, D, first, gh, gw, nat.ptr(bx), nat.ptr(ct), nat.ptr(st), K, int(grid), nat.ptr(emb),
                                          nat.stream_ptr()))
    return emb
