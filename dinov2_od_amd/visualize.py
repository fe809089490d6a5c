"""Detections and ground truth drawn into the image batch on the GPU: the host side of `dod_draw_detections` (include/dinodet.h).

The reference has two surfaces for looking at results and draws boxes in neither on the device: `log_images(writer, images, targets,
predictions, global_step, tag)` (dino_detector/utils.py:360-384), whose body logs bare images under a TODO, and
`visualize_predictions` (analyze_results.py:81-203), which re-reads files on the host and draws with matplotlib.  Here
`draw_detections` renders outlined, optionally filled and captioned boxes into a fresh uint8 [B, H, W, 3] batch in one launch with no
host sync, `log_images` is the reference's signature with the TODO filled in, and `save_images` writes PNG files (the one function
here that syncs).  No CPU fallback: without the HIP library and a GPU this module raises.

FONT_5X7 below is the one copy of the caption font: it goes to the kernel as a device buffer, and tests/draw_cases.py reads the same
table.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _native as nat

MAX_BOXES = 1024          # per layer (include/dinodet.h dod_draw_detections)
NAME_LEN = 24             # bytes per row of the class-name table; longer names are cut
MAX_LOGGED = 8            # log_images: as the reference (utils.py:373)

# twenty well-separated colours; predictions take PALETTE[label % len(PALETTE)]
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
           (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
           (128, 128, 0), (255, 215, 180), (0, 0, 128), (128, 128, 128))

# 5 x 7 glyphs, top row first, '#' = set.  Every byte of 0x20..0x7F without an entry here is a solid cell, as is any byte outside that range.
_GLYPHS = {
    " ": "..... ..... ..... ..... ..... ..... .....",
    "%": "##... ##..# ...#. ..#.. .#... #..## ...##",
    ".": "..... ..... ..... ..... ..... .##.. .##..",
    ":": "..... .##.. .##.. ..... .##.. .##.. .....",
    "-": "..... ..... ..... ##### ..... ..... .....",
    "_": "..... ..... ..... ..... ..... ..... #####",
    "0": ".###. #...# #..## #.#.# ##..# #...# .###.",
    "1": "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",
    "2": ".###. #...# ....# ...#. ..#.. .#... #####",
    "3": "##### ...#. ..#.. ...#. ....# #...# .###.",
    "4": "...#. ..##. .#.#. #..#. ##### ...#. ...#.",
    "5": "##### #.... ####. ....# ....# #...# .###.",
    "6": "..##. .#... #.... ####. #...# #...# .###.",
    "7": "##### ....# ...#. ..#.. .#... .#... .#...",
    "8": ".###. #...# #...# .###. #...# #...# .###.",
    "9": ".###. #...# #...# .#### ....# ...#. .##..",
    "A": ".###. #...# #...# ##### #...# #...# #...#",
    "B": "####. #...# #...# ####. #...# #...# ####.",
    "C": ".###. #...# #.... #.... #.... #...# .###.",
    "D": "###.. #..#. #...# #...# #...# #..#. ###..",
    "E": "##### #.... #.... ####. #.... #.... #####",
    "F": "##### #.... #.... ####. #.... #.... #....",
    "G": ".###. #...# #.... #.### #...# #...# .####",
    "H": "#...# #...# #...# ##### #...# #...# #...#",
    "I": ".###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",
    "J": "..### ...#. ...#. ...#. ...#. #..#. .##..",
    "K": "#...# #..#. #.#.. ##... #.#.. #..#. #...#",
    "L": "#.... #.... #.... #.... #.... #.... #####",
    "M": "#...# ##.## #.#.# #.#.# #...# #...# #...#",
    "N": "#...# #...# ##..# #.#.# #..## #...# #...#",
    "O": ".###. #...# #...# #...# #...# #...# .###.",
    "P": "####. #...# #...# ####. #.... #.... #....",
    "Q": ".###. #...# #...# #...# #.#.# #..#. .##.#",
    "R": "####. #...# #...# ####. #.#.. #..#. #...#",
    "S": ".#### #.... #.... .###. ....# ....# ####.",
    "T": "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",
    "U": "#...# #...# #...# #...# #...# #...# .###.",
    "V": "#...# #...# #...# #...# #...# .#.#. ..#..",
    "W": "#...# #...# #...# #.#.# #.#.# #.#.# .#.#.",
    "X": "#...# #...# .#.#. ..#.. .#.#. #...# #...#",
    "Y": "#...# #...# #...# .#.#. ..#.. ..#.. ..#..",
    "Z": "##### ....# ...#. ..#.. .#... #.... #####",
    "a": "..... ..... .###. ....# .#### #...# .####",
    "b": "#.... #.... #.##. ##..# #...# #...# ####.",
    "c": "..... ..... .###. #.... #.... #...# .###.",
    "d": "....# ....# .##.# #..## #...# #...# .####",
    "e": "..... ..... .###. #...# ##### #.... .###.",
    "f": "..##. .#..# .#... ###.. .#... .#... .#...",
    "g": "..... .#### #...# #...# .#### ....# .###.",
    "h": "#.... #.... #.##. ##..# #...# #...# #...#",
    "i": "..#.. ..... .##.. ..#.. ..#.. ..#.. .###.",
    "j": "...#. ..... ..##. ...#. ...#. #..#. .##..",
    "k": "#.... #.... #..#. #.#.. ##... #.#.. #..#.",
    "l": ".##.. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",
    "m": "..... ..... ##.#. #.#.# #.#.# #...# #...#",
    "n": "..... ..... #.##. ##..# #...# #...# #...#",
    "o": "..... ..... .###. #...# #...# #...# .###.",
    "p": "..... ####. #...# #...# ####. #.... #....",
    "q": "..... .#### #...# #...# .#### ....# ....#",
    "r": "..... ..... #.##. ##..# #.... #.... #....",
    "s": "..... ..... .###. #.... .###. ....# ####.",
    "t": ".#... .#... ###.. .#... .#... .#..# ..##.",
    "u": "..... ..... #...# #...# #...# #..## .##.#",
    "v": "..... ..... #...# #...# #...# .#.#. ..#..",
    "w": "..... ..... #...# #...# #.#.# #.#.# .#.#.",
    "x": "..... ..... #...# .#.#. ..#.. .#.#. #...#",
    "y": "..... #...# #...# #...# .#### ....# .###.",
    "z": "..... ..... ##### ...#. ..#.. .#... #####",
}


def _font_table():
    t = np.full((96, 7), 0x1F, np.uint8)
    for ch, art in _GLYPHS.items():
        rows = art.split()
        assert len(rows) == 7 and all(len(r) == 5 and set(r) <= {"#", "."} for r in rows), ch
        t[ord(ch) - 0x20] = [int(r.replace("#", "1").replace(".", "0"), 2) for r in rows]
    t.setflags(write=False)
    return t


FONT_5X7 = _font_table()      # uint8 [96, 7] for 0x20..0x7F: 5 low bits per row, bit 4 the leftmost column

_tables = {}                  # (kind, device, key) -> device tensor: the font, palettes and name tables last used


def _device_table(kind, device, key, make):
    k = (kind, str(device))
    hit = _tables.get(k)
    if hit is None or hit[0] != key:
        hit = (key, torch.from_numpy(np.array(make())).to(device))
        _tables[k] = hit
    return hit[1]


def names_table(class_names):
    """list of str -> uint8 [n, NAME_LEN], zero padded; a name longer than NAME_LEN is cut, a non-ASCII character becomes '?'"""
    t = np.zeros((len(class_names), NAME_LEN), np.uint8)
    for i, nm in enumerate(class_names):
        raw = str(nm).encode("ascii", "replace")[:NAME_LEN]
        t[i, :len(raw)] = np.frombuffer(raw, np.uint8)
    return t


def _rgb(c, what):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f"{what} must be three integers in 0..255, got {c}")
    return c


def _pad_targets(targets, B, device):
    """the train loop's list of {"boxes" [n, 4] normalised cxcywh, "labels" [n]} -> (boxes [B, G, 4] f32, labels [B, G] i32, counts [B] i32),
    by copies only; or a dict of such tensors already padded ({"boxes", "labels"} and optionally "counts")"""
    if isinstance(targets, dict):
        boxes, labels, counts = targets["boxes"], targets["labels"], targets.get("counts")
        if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or tuple(labels.shape) != tuple(boxes.shape[:2]):
            raise ValueError(f"targets must hold boxes [B, G, 4] and labels [B, G] for B={B}, got {tuple(boxes.shape)} and {tuple(labels.shape)}")
        if counts is not None and tuple(counts.shape) != (B,):
            raise ValueError(f"targets['counts'] must have shape ({B},), got {tuple(counts.shape)}")
        return boxes, labels, counts
    if len(targets) != B:
        raise ValueError(f"targets must have one entry per image ({B}), got {len(targets)}")
    ns = []
    for t in targets:
        bx, lb = t["boxes"], t["labels"]
        if bx.dim() != 2 or bx.shape[1] != 4 or lb.dim() != 1 or lb.shape[0] != bx.shape[0]:
            raise ValueError(f"a target needs boxes [n, 4] and labels [n], got {tuple(bx.shape)} and {tuple(lb.shape)}")
        ns.append(int(bx.shape[0]))
    G = max(ns) if ns else 0
    if G > MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} ground-truth boxes per image, got {G}")
    if device is None:
        return ns, None, None
    boxes = torch.zeros(B, max(G, 1), 4, dtype=torch.float32, device=device)
    labels = torch.zeros(B, max(G, 1), dtype=torch.int32, device=device)
    for i, t in enumerate(targets):
        if ns[i]:
            boxes[i, :ns[i]].copy_(t["boxes"], non_blocking=True)
            labels[i, :ns[i]].copy_(t["labels"], non_blocking=True)
    counts = torch.tensor(ns, dtype=torch.int32).to(device, non_blocking=True)
    return boxes, labels, counts


def _layer(boxes, labels, scores, counts, fmt, threshold, use_palette, color, device, keep):
    """tensors -> DodDrawLayer; `keep` collects what must outlive the call"""
    if boxes.dim() != 3 or boxes.shape[2] != 4 or tuple(labels.shape) != tuple(boxes.shape[:2]):
        raise ValueError(f"a layer needs boxes [B, K, 4] and labels [B, K], got {tuple(boxes.shape)} and {tuple(labels.shape)}")
    K = int(boxes.shape[1])
    if K > MAX_BOXES:
        raise ValueError(f"at most {MAX_BOXES} boxes per image and layer, got {K}")
    if scores is not None and tuple(scores.shape) != tuple(labels.shape):
        raise ValueError(f"scores must have the labels' shape, got {tuple(scores.shape)}")
    L = nat.DodDrawLayer()
    L.K, L.format, L.score_threshold, L.use_palette = K, fmt, float(threshold), int(use_palette)
    L.color[0], L.color[1], L.color[2] = color
    if device is not None and K > 0:
        bt = boxes.to(device=device, dtype=torch.float32).contiguous()
        lt = labels.to(device=device, dtype=torch.int32).contiguous()
        st = None if scores is None else scores.to(device=device, dtype=torch.float32).contiguous()
        ct = None if counts is None else counts.to(device=device, dtype=torch.int32).contiguous()
        keep += [bt, lt, st, ct]
        L.boxes, L.labels, L.scores, L.counts = bt.data_ptr(), lt.data_ptr(), None if st is None else st.data_ptr(), None if ct is None else ct.data_ptr()
    return L


def draw_detections(images, detections=None, targets=None, class_names=None, score_threshold=0.0, thickness=2, fill_alpha=0,
                    font_scale=1, palette=None, gt_color=(255, 255, 255)):
    """images: uint8 [B, H, W, 3] (what forward_packed_u8 takes) or fp32 [B, 3, H, W] in [0, 1], on the GPU.  detections: a
    postprocess.Detections whose boxes are pixels of `images` (model.detect(x) with sizes=None); rows with score <= score_threshold are
    left out (a threshold < 0 keeps all).  targets: the train loop's list of {"boxes" normalised cxcywh, "labels"}, or a dict of padded
    tensors {"boxes" [B, G, 4], "labels" [B, G], "counts" [B]}; drawn below the detections in gt_color.  class_names: list of str
    indexed by label (captions show the decimal label without it, and the score as a percentage for detections).  thickness 1..8,
    fill_alpha 0..255 (0: outline only), font_scale 0..4 (0: no captions), palette: sequence of (r, g, b) for label % len(palette).
    Returns a fresh uint8 CUDA tensor [B, H, W, 3].  One launch on the current stream, no host sync."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError("images must be a uint8 [B, H, W, 3] or fp32 [B, 3, H, W] tensor")
    if images.dtype == torch.uint8 and images.shape[3] == 3:
        fp32, (B, H, W) = 0, images.shape[:3]
    elif images.dtype == torch.float32 and images.shape[1] == 3:
        fp32, B, (H, W) = 1, images.shape[0], images.shape[2:]
    else:
        raise ValueError(f"images must be a uint8 [B, H, W, 3] or fp32 [B, 3, H, W] tensor, got {images.dtype} {tuple(images.shape)}")
    B, H, W = int(B), int(H), int(W)
    if B < 1 or H < 1 or W < 1 or B > 65535 or H > 16384 or W > 16384:
        raise ValueError(f"need 1..65535 images of 1..16384 pixels a side, got B={B} H={H} W={W}")
    if not 1 <= int(thickness) <= 8:
        raise ValueError(f"thickness must be in 1..8, got {thickness}")
    if not 0 <= int(fill_alpha) <= 255:
        raise ValueError(f"fill_alpha must be in 0..255, got {fill_alpha}")
    if not 0 <= int(font_scale) <= 4:
        raise ValueError(f"font_scale must be in 0..4, got {font_scale}")
    pal = tuple(_rgb(c, "a palette colour") for c in (PALETTE if palette is None else palette))
    if not pal:
        raise ValueError("palette must not be empty")
    gt = _rgb(gt_color, "gt_color")
    names = None if class_names is None else tuple(str(n) for n in class_names)
    if names is not None and not names:
        raise ValueError("class_names must not be empty")
    device = images.device if images.is_cuda else None
    keep = []
    below = above = None
    if targets is not None:
        bx, lb, ct = _pad_targets(targets, B, device)
        if device is not None or isinstance(targets, dict):
            below = _layer(bx, lb, None, ct, 1, -1.0, 0, gt, device, keep)
    if detections is not None:
        if tuple(detections.boxes.shape[:1]) != (B,) or tuple(detections.counts.shape) != (B,):
            raise ValueError(f"detections must hold {B} images, got boxes {tuple(detections.boxes.shape)} and counts {tuple(detections.counts.shape)}")
        above = _layer(detections.boxes, detections.labels, detections.scores, detections.counts, 0, score_threshold, 1, (0, 0, 0), device, keep)
    if device is None:                                        # last: every argument is checked whether or not a GPU is present
        raise ValueError("images must be on the GPU (there is no CPU fallback)")
    lib = nat.lib()
    images = images.contiguous()
    st = nat.DodDrawStyle()
    st.thickness, st.fill_alpha, st.font_scale, st.palette_size = int(thickness), int(fill_alpha), int(font_scale), len(pal)
    st.palette = _device_table("palette", device, pal, lambda: np.asarray(pal, np.uint8)).data_ptr()
    st.font = _device_table("font", device, 0, lambda: FONT_5X7).data_ptr()
    if names is not None:
        st.names = _device_table("names", device, names, lambda: names_table(names)).data_ptr()
        st.n_names, st.name_len = len(names), NAME_LEN
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=device)
    nat.check(lib.dod_draw_detections(nat.ptr(images), fp32, B, H, W, None if below is None else C.byref(below),
                                      None if above is None else C.byref(above), C.byref(st), nat.ptr(out), nat.stream_ptr()))
    return out      # `keep` and the tables were allocated on this stream: freeing them after the launch is ordered behind it


def _predictions_to_detections(predictions, H, W, top_k=100):
    """a Detections passes through; the model's output dict goes through detect_packed with sizes = (H, W)"""
    from .postprocess import Detections, detect_packed
    if predictions is None or isinstance(predictions, Detections):
        return predictions
    if isinstance(predictions, dict) and "pred_logits" in predictions and "pred_boxes" in predictions:
        lg, bx = predictions["pred_logits"], predictions["pred_boxes"]
        det = torch.cat([lg, bx], dim=-1).float()
        return detect_packed(det, lg.shape[-1], (H, W), top_k=min(top_k, MAX_BOXES))
    raise ValueError("predictions must be a postprocess.Detections or a dict with 'pred_logits' and 'pred_boxes'")


def _first(x, n):
    from .postprocess import Detections
    if x is None:
        return None
    if isinstance(x, Detections):
        return Detections(*(t[:n] for t in x))
    if isinstance(x, dict):
        return {k: (v[:n] if isinstance(v, torch.Tensor) else v) for k, v in x.items()}
    return x[:n]


def log_images(writer, images, targets=None, predictions=None, global_step=0, tag="images", **style):
    """The reference's log_images (utils.py:360-384) with its box drawing filled in: at most 8 images of the batch, ground truth and
    predictions drawn on the device, logged through writer.add_images(tag, drawn, global_step, dataformats="NHWC").  predictions: a
    postprocess.Detections in pixels of `images`, or the model's output dict {"pred_logits", "pred_boxes"}.  A single 3-dim image
    (fp32 [3, H, W] or uint8 [H, W, 3]) goes to writer.add_image(..., dataformats="HWC").  `style`: draw_detections' keyword arguments.
    Any object with add_images / add_image will do as the writer.  Returns the drawn batch."""
    single = images.dim() == 3
    if single:
        images = images[None]
        if isinstance(targets, dict) and targets["boxes"].dim() == 2:          # one image's own target dict
            targets = [targets]
        if isinstance(predictions, dict) and predictions["pred_logits"].dim() == 2:
            predictions = {k: v[None] for k, v in predictions.items() if isinstance(v, torch.Tensor)}
    n = min(int(images.shape[0]), MAX_LOGGED)
    images, targets, predictions = images[:n], _first(targets, n), _first(predictions, n)
    H, W = (images.shape[1:3] if images.dtype == torch.uint8 else images.shape[2:4])
    drawn = draw_detections(images, _predictions_to_detections(predictions, int(H), int(W)), targets, **style)
    if single:
        writer.add_image(tag, drawn[0], global_step, dataformats="HWC")
    else:
        writer.add_images(tag, drawn, global_step, dataformats="NHWC")
    return drawn


def save_images(directory, images, detections=None, targets=None, names=None, **style):
    """The counterpart of the reference's visualize_predictions (analyze_results.py:81-203): draws on the device and writes one PNG per
    image into `directory` -- names[i] + ".png", or 000000.png, 000001.png ... without names.  The one function here that syncs (it
    copies the drawn batch to the host).  Returns the list of paths."""
    from PIL import Image
    B = int(images.shape[0])
    if names is not None and len(names) != B:
        raise ValueError(f"names must have one entry per image ({B}), got {len(names)}")
    drawn = draw_detections(images, detections, targets, **style).cpu().numpy()
    os.makedirs(directory, exist_ok=True)
    paths = []
    for i in range(B):
        stem = f"{i:06d}" if names is None else os.path.splitext(os.path.basename(str(names[i])))[0]
        paths.append(os.path.join(directory, stem + ".png"))
        Image.fromarray(drawn[i], "RGB").save(paths[-1])
    return paths
