"""CPU checks of the drawing feature (dod_draw_detections, dinov2_od_amd/visualize.py): the numpy restatement (tests/draw_cases.py)
against Pillow, which pins it to something outside this repository; the font table; the caption's scaling rule; the entry's argument
checks through the C ABI; and the Python layer's argument handling with a recording writer.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from dinov2_od_amd import _native as nat
from dinov2_od_amd import visualize as V
from tests import draw_cases as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 40, 52
# integer rectangles (xa, ya, xb, yb), sides >= 16 = 2 * the largest thickness: inside, over each edge, over a corner, covering the image, outside
RECTS = [(5, 6, 30, 27), (-7, 10, 12, 30), (40, 3, 60, 22), (10, -9, 33, 9), (8, 30, 28, 55), (-5, -5, 14, 13), (-3, -3, 55, 43),
         (60, 10, 80, 30), (-40, 5, -20, 25), (5, -30, 25, -10), (5, 45, 25, 65)]
COL = (200, 30, 120)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def _as_box(r):
    """the xyxy box whose pixel rectangle is r"""
    return [r[0], r[1], r[2] + 1, r[3] + 1]


def _one(rects, color=COL):
    boxes = np.asarray([[_as_box(r) for r in rects]], np.float32)
    return dw.layer(boxes, np.zeros((1, len(rects)), np.int32), color=color)


@pytest.mark.parametrize("t", [1, 2, 3, 8])
def test_outline_equals_pillow(t):
    img = dw.rand_images_u8(1, 1, H, W)
    for r in RECTS:
        pil = Image.fromarray(img[0].copy(), "RGB")
        ImageDraw.Draw(pil).rectangle(list(r), outline=COL, width=t)
        got = dw.draw_ref(img, None, _one([r]), dw.style(t, 0, 0))
        assert np.array_equal(got[0], np.asarray(pil)), (t, r)
    assert np.array_equal(dw.draw_ref(img, None, _one(RECTS[-4:]), dw.style(t, 0, 0)), img)      # wholly outside: nothing drawn


@pytest.mark.parametrize("a", [0, 1, 127, 128, 254, 255])
def test_fill_equals_pillow_rgba(a):
    img = dw.rand_images_u8(2, 1, H, W)
    for r in RECTS[:7]:
        t = 2
        pil = Image.fromarray(img[0].copy(), "RGB")
        ImageDraw.Draw(pil, "RGBA").rectangle(list(r), fill=COL + (a,))
        want = np.asarray(pil)
        got = dw.draw_ref(img, None, _one([r]), dw.style(t, a, 0))[0]
        ys, xs = np.mgrid[0:H, 0:W]
        inner = (xs >= r[0] + t) & (xs <= r[2] - t) & (ys >= r[1] + t) & (ys <= r[3] - t)
        assert inner.any()
        assert np.array_equal(got[inner], want[inner]), (a, r)                                    # the fill is Pillow's blend
        ImageDraw.Draw(pil, "RGBA").rectangle(list(r), outline=COL + (255,), width=t)             # and with the outline over it, every byte
        assert np.array_equal(got, np.asarray(pil)), (a, r)
    if a == 0:
        ys, xs = np.mgrid[0:H, 0:W]
        r = RECTS[0]
        inner = (xs >= r[0] + 2) & (xs <= r[2] - 2) & (ys >= r[1] + 2) & (ys <= r[3] - 2)
        assert np.array_equal(dw.draw_ref(img, None, _one([r]), dw.style(2, 0, 0))[0][inner], img[0][inner])      # a = 0 draws nothing


def test_overlapping_boxes_follow_painters_order():
    img = dw.rand_images_u8(3, 1, H, W)
    r0, r1 = (5, 6, 30, 27), (18, 14, 47, 36)
    pal = [(250, 10, 10), (10, 10, 250)]
    ly = dw.layer(np.asarray([[_as_box(r0), _as_box(r1)]], np.float32), np.asarray([[0, 1]], np.int32), use_palette=True)
    got = dw.draw_ref(img, None, ly, dw.style(3, 128, 0, palette=pal))
    pil = Image.fromarray(img[0].copy(), "RGB")
    d = ImageDraw.Draw(pil, "RGBA")
    for r, c in ((r1, pal[1]), (r0, pal[0])):                      # row 1 first: row 0 ends on top
        d.rectangle(list(r), fill=c + (128,))
        d.rectangle(list(r), outline=c + (255,), width=3)
    assert np.array_equal(got[0], np.asarray(pil))
    swapped = dw.layer(ly["boxes"][:, ::-1], ly["labels"][:, ::-1], use_palette=True)
    assert not np.array_equal(dw.draw_ref(img, None, swapped, dw.style(3, 128, 0, palette=pal)), got)
    # the layer below is painted first whatever its rows are
    lo, hi = dw.layer(ly["boxes"][:, 1:], ly["labels"][:, 1:], use_palette=True), dw.layer(ly["boxes"][:, :1], ly["labels"][:, :1], use_palette=True)
    assert np.array_equal(dw.draw_ref(img, lo, hi, dw.style(3, 128, 0, palette=pal)), got)


def test_fractional_boxes_round_outwards():
    assert dw.pixel_rect([2.5, 3.0, 7.0, 9.25], 0, H, W) == (2, 3, 6, 9)
    assert dw.pixel_rect([2.0, 3.0, 2.0, 9.0], 0, H, W) is None                       # empty
    assert dw.pixel_rect([5.0, 3.0, 2.0, 9.0], 0, H, W) is None                       # inverted
    assert dw.pixel_rect([np.nan, 3.0, 7.0, 9.0], 0, H, W) is None
    assert dw.pixel_rect([-np.inf, -1e30, np.inf, 1e30], 0, H, W) == (-32768, -32768, 32766, 32766)
    assert dw.pixel_rect([0.5, 0.5, 0.25, 0.5], 1, 40, 52) == (19, 10, 32, 29)         # cxcywh: x 0.375..0.625 * 52, y 0.25..0.75 * 40


def test_font_table():
    f = V.FONT_5X7
    assert f.shape == (96, 7) and f.dtype == np.uint8 and int(f.max()) <= 0x1F
    required = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz%.:-_"
    assert len(set(required)) == 68
    glyphs = {c: f[ord(c) - 0x20].tobytes() for c in required}
    for c, g in glyphs.items():
        assert c == " " or any(g), f"glyph {c!r} is empty"
        assert g != bytes([0x1F] * 7), f"glyph {c!r} is the solid cell"
    assert len(set(glyphs.values())) == len(required), "two required glyphs are equal"
    assert not any(glyphs[" "])
    for code in range(0x20, 0x80):                                                      # every byte the font does not design is solid
        if chr(code) not in required:
            assert f[code - 0x20].tobytes() == bytes([0x1F] * 7), hex(code)
    assert not f.flags.writeable


def test_caption_scales_by_pixel_doubling():
    text = b"car 87%"
    one = dw.caption_bitmap(text, 1)
    assert one.shape == (9, 6 * len(text) + 1) and one.any()
    for s in (2, 3, 4):
        assert np.array_equal(dw.caption_bitmap(text, s), np.repeat(np.repeat(one, s, 0), s, 1))
    # a margin of one pixel, a blank column after every glyph and a blank row under it
    assert not one[0].any() and not one[:, 0].any() and not one[8].any() and not one[:, 6::6].any()
    # bit 4 is the leftmost column: 'L' has its stem at the left
    L = dw.caption_bitmap(b"L", 1)
    assert L[1:8, 1].all() and not L[1:7, 2:6].any()
    # bytes outside 0x20..0x7F and undesigned ones are solid cells
    for raw in (b"\x01", b"\xe9", b"?", b"\x7f"):
        assert dw.caption_bitmap(raw, 1)[1:8, 1:6].all()


def test_caption_text_and_placement():
    names = dw.names_array()
    assert dw.caption_text(3, None, names) == b"car" and dw.caption_text(3, np.float32(0.874), names) == b"car 87%"
    assert dw.caption_text(7, None, names) == b"7"                                    # an empty name falls back to the label
    assert dw.caption_text(8, None, names) == b"x" * V.NAME_LEN                       # cut at NAME_LEN
    assert dw.caption_text(len(names), np.float32(1.0), names) == b"%d 100%%" % len(names)
    assert dw.caption_text(-12, np.float32(0.004), None) == b"-12 0%" and dw.caption_text(5, np.float32(np.nan), None) == b"5 0%"
    assert dw.caption_text(5, np.float32(0.005), None) == b"5 1%" and dw.caption_text(5, np.float32(1e9), None) == b"5 999%"
    assert dw.caption_rect(10, 20, 3, 1, 40, 52) == (10, 11, 19, 9)                    # above the box
    assert dw.caption_rect(10, 8, 3, 1, 40, 52) == (10, 8, 19, 9)                      # no room above: inside, at the box's top
    assert dw.caption_rect(45, 20, 3, 1, 40, 52) == (33, 11, 19, 9)                    # shifted left
    assert dw.caption_rect(-6, 20, 3, 1, 40, 52) == (0, 11, 19, 9)
    assert dw.caption_rect(10, 20, 30, 2, 40, 52) == (0, 2, 52, 18)                    # wider than the image: cut
    assert dw.caption_rect(0, 3, 2, 4, 20, 30) == (0, 0, 30, 20)                       # higher than the image too


def test_header_documents_the_entry():
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    assert "int dod_draw_detections(" in hdr and "typedef struct dod_draw_layer {" in hdr and "typedef struct dod_draw_style {" in hdr
    for struct, mirror in (("dod_draw_layer", nat.DodDrawLayer), ("dod_draw_style", nat.DodDrawStyle)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = re.findall(r"(\w+)(?:\[\d+\])?;", body)
        assert names == [f for f, _ in mirror._fields_], struct
    assert "dod_draw_detections" in nat.SYMBOLS and len(nat.SYMBOLS["dod_draw_detections"][1]) == 10


def test_entry_validates_arguments(lib):
    """every documented invalid argument is DOD_ERR_INVALID (1) before any launch; the valid call reaches the launch, which without a GPU
    is DOD_ERR_HIP (4).  `p`, `q` stand in for device pointers that are never dereferenced."""
    buf, buf2 = (C.c_float * 64)(), (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)

    def call(images=p, fp32=0, B=1, H=8, W=8, below=None, above=None, style="default", out=q, **kw):
        st = nat.DodDrawStyle()
        st.thickness, st.fill_alpha, st.font_scale, st.palette_size = 2, 0, 1, 4
        st.palette, st.font = p.value, p.value
        for k, v in kw.items():
            setattr(st, k, v)
        return lib.dod_draw_detections(images, fp32, B, H, W, below, above, None if style is None else C.byref(st), out, None)

    def lay(**kw):
        ly = nat.DodDrawLayer()
        ly.boxes, ly.labels, ly.counts, ly.K, ly.format = p.value, p.value, p.value, 4, 0
        for k, v in kw.items():
            setattr(ly, k, v)
        return C.byref(ly)

    ok = 4 if not torch.cuda.is_available() else 0
    if not torch.cuda.is_available():
        assert call() == ok and call(above=lay(), below=lay(format=1)) == ok
    assert call(images=None) == 1 and call(out=None) == 1 and call(style=None) == 1 and call(out=p) == 1
    assert call(fp32=2) == 1 and call(fp32=-1) == 1
    for dims in ({"B": 0}, {"H": 0}, {"W": 0}, {"B": -1}, {"H": -3}, {"W": -2}, {"B": 65536}, {"H": 16385}, {"W": 16385}):
        assert call(**dims) == 1, dims
    for bad in ({"thickness": 0}, {"thickness": 9}, {"thickness": -1}, {"fill_alpha": -1}, {"fill_alpha": 256}, {"font_scale": -1}, {"font_scale": 5},
                {"font": None}, {"names": p.value, "n_names": 0, "name_len": 8}, {"names": p.value, "n_names": 3, "name_len": 0},
                {"names": p.value, "n_names": 3, "name_len": 65}):
        assert call(**bad) == 1, bad
    for bad in ({"K": -1}, {"K": 1025}, {"format": 2}, {"format": -1}, {"labels": None}, {"boxes": p.value + 4}):
        assert call(above=lay(**bad)) == 1 and call(below=lay(**bad)) == 1, bad
    assert call(above=lay(use_palette=1), palette=None) == 1 and call(above=lay(use_palette=1), palette_size=0) == 1
    if not torch.cuda.is_available():
        assert call(font=None, font_scale=0) == ok                                   # no captions: no font needed
        assert call(above=lay(K=0, boxes=None, labels=None)) == ok and call(above=lay(boxes=None, labels=None)) == ok      # absent layers
        assert call(above=lay(K=1024), below=lay(K=1024, counts=None)) == ok


class _Writer:
    def __init__(self):
        self.calls = []

    def add_images(self, tag, img, global_step=None, dataformats="NCHW"):
        self.calls.append(("add_images", tag, img, global_step, dataformats))

    def add_image(self, tag, img, global_step=None, dataformats="CHW"):
        self.calls.append(("add_image", tag, img, global_step, dataformats))


def test_log_images_caps_at_eight_and_logs_nhwc(monkeypatch):
    seen = {}

    def fake_draw(images, detections=None, targets=None, **style):
        seen.update(images=images, detections=detections, targets=targets, style=style)
        B, (Hh, Ww) = images.shape[0], images.shape[2:]
        return torch.zeros(B, Hh, Ww, 3, dtype=torch.uint8)

    monkeypatch.setattr(V, "draw_detections", fake_draw)
    from dinov2_od_amd.postprocess import Detections
    x = torch.rand(11, 3, 16, 20)
    targets = [{"boxes": torch.rand(i % 3, 4), "labels": torch.zeros(i % 3, dtype=torch.int64)} for i in range(11)]
    det = Detections(torch.rand(11, 5), torch.zeros(11, 5, dtype=torch.int32), torch.rand(11, 5, 4), torch.zeros(11, 5, dtype=torch.int32),
                     torch.full((11,), 5, dtype=torch.int32))
    w = _Writer()
    out = V.log_images(w, x, targets, det, global_step=7, tag="val", thickness=3)
    assert len(w.calls) == 1
    kind, tag, img, step, fmt = w.calls[0]
    assert (kind, tag, step, fmt) == ("add_images", "val", 7, "NHWC") and img is out and tuple(img.shape) == (8, 16, 20, 3) and img.dtype == torch.uint8
    assert seen["images"].shape[0] == 8 and len(seen["targets"]) == 8 and seen["style"] == {"thickness": 3}
    assert all(t.shape[0] == 8 for t in seen["detections"]) and isinstance(seen["detections"], Detections)
    w = _Writer()
    V.log_images(w, x[:3])                                                            # fewer than eight: all of them, nothing to draw
    assert w.calls[0][2].shape[0] == 3 and seen["targets"] is None and seen["detections"] is None and w.calls[0][3] == 0 and w.calls[0][1] == "images"
    w = _Writer()
    V.log_images(w, x[0], targets[2], None, 3)                                        # a single image goes to add_image, as in the reference
    assert w.calls[0][0] == "add_image" and w.calls[0][4] == "HWC" and tuple(w.calls[0][2].shape) == (16, 20, 3) and len(seen["targets"]) == 1
    with pytest.raises(ValueError, match="predictions"):
        V.log_images(_Writer(), x, None, "nonsense")


def test_draw_detections_checks_arguments_before_asking_for_a_gpu():
    from dinov2_od_amd.postprocess import Detections
    x = torch.zeros(2, 3, 16, 20)
    u = torch.zeros(2, 16, 20, 3, dtype=torch.uint8)
    det = Detections(torch.rand(2, 5), torch.zeros(2, 5, dtype=torch.int32), torch.rand(2, 5, 4), torch.zeros(2, 5, dtype=torch.int32),
                     torch.full((2,), 5, dtype=torch.int32))
    tg = [{"boxes": torch.rand(2, 4), "labels": torch.zeros(2, dtype=torch.int64)}] * 2
    for bad in (dict(thickness=0), dict(thickness=9), dict(fill_alpha=256), dict(fill_alpha=-1), dict(font_scale=5), dict(font_scale=-1),
                dict(palette=[]), dict(palette=[(1, 2)]), dict(palette=[(1, 2, 300)]), dict(gt_color=(1, 2)), dict(class_names=[])):
        with pytest.raises(ValueError) as e:
            V.draw_detections(u, det, tg, **bad)
        assert "no CPU fallback" not in str(e.value), bad
    for imgs in (torch.zeros(2, 16, 20, 3), torch.zeros(2, 4, 16, 20), torch.zeros(16, 20, 3, dtype=torch.uint8), torch.zeros(2, 16, 20, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="images must be"):
            V.draw_detections(imgs)
    with pytest.raises(ValueError, match="one entry per image"):
        V.draw_detections(x, None, tg[:1])
    with pytest.raises(ValueError, match="boxes \\[n, 4\\]"):
        V.draw_detections(x, None, [{"boxes": torch.rand(2, 5), "labels": torch.zeros(2)}] * 2)
    with pytest.raises(ValueError, match="at most 1024"):
        V.draw_detections(x, None, [{"boxes": torch.rand(1025, 4), "labels": torch.zeros(1025)}] * 2)
    with pytest.raises(ValueError, match="must hold 2 images"):
        V.draw_detections(x, Detections(*(t[:1] for t in det)))
    with pytest.raises(ValueError, match="at most 1024"):
        V.draw_detections(x, Detections(torch.rand(2, 1025), torch.zeros(2, 1025, dtype=torch.int32), torch.rand(2, 1025, 4), None, torch.zeros(2, dtype=torch.int32)))
    if not torch.cuda.is_available():
        for imgs in (x, u):
            with pytest.raises(ValueError, match="no CPU fallback"):
                V.draw_detections(imgs, det, tg, class_names=["a", "b"])
    import dinov2_od_amd
    assert dinov2_od_amd.draw_detections is V.draw_detections and dinov2_od_amd.log_images is V.log_images and dinov2_od_amd.save_images is V.save_images
