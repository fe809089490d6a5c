"""GPU parity of dod_draw_detections against its numpy restatement (tests/draw_cases.py): bit-equal on every byte.  The output sits
between guard bytes that must stay untouched; with the odd guard length the output (and, where a case asks for it, the uint8 input)
starts at an address that is no multiple of 4, which takes the rows' byte-wise edges instead of whole dwords."""
import ctypes as C

import numpy as np
import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import visualize as V
from tests import detect_cases as dc
from tests import draw_cases as dw

pytestmark = pytest.mark.gpu
GUARDS = (64, 37)
SENT = 0xA5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return nat.lib()


def _c_layer(ly, keep):
    if ly is None:
        return None
    L = nat.DodDrawLayer()
    L.K, L.format, L.score_threshold, L.use_palette = ly["boxes"].shape[1], ly["format"], ly["threshold"], int(ly["use_palette"])
    L.color[0], L.color[1], L.color[2] = ly["color"]
    for k in ("boxes", "labels", "counts", "scores"):
        if ly[k] is not None and ly[k].size:
            t = torch.from_numpy(ly[k]).cuda()
            keep.append(t)
            setattr(L, k, t.data_ptr())
    return C.byref(L)


def _run(images, below, above, st, guard=64, stream=None, in_offset=0):
    """dod_draw_detections through the C ABI into a guarded output -> uint8 [B, H, W, 3]"""
    L = nat.lib()
    fp32 = int(images.dtype == np.float32)
    B, H, W = (images.shape[0], images.shape[2], images.shape[3]) if fp32 else images.shape[:3]
    keep = []
    if fp32:
        img = torch.from_numpy(images).cuda()
    else:                                                    # the uint8 input may start at any byte
        raw_in = torch.zeros(images.size + in_offset, dtype=torch.uint8, device="cuda")
        img = raw_in[in_offset:]
        img.copy_(torch.from_numpy(images.reshape(-1)))
    n = B * H * W * 3
    raw = torch.full((n + 2 * guard,), SENT, dtype=torch.uint8, device="cuda")
    out = raw[guard:guard + n]
    S = nat.DodDrawStyle()
    S.thickness, S.fill_alpha, S.font_scale = st["thickness"], st["fill_alpha"], st["font_scale"]
    pal, font = torch.from_numpy(st["palette"]).cuda(), torch.from_numpy(np.array(V.FONT_5X7)).cuda()
    S.palette, S.palette_size, S.font = pal.data_ptr(), len(st["palette"]), font.data_ptr()
    if st["names"] is not None:
        nm = torch.from_numpy(np.ascontiguousarray(st["names"])).cuda()
        S.names, S.n_names, S.name_len = nm.data_ptr(), nm.shape[0], nm.shape[1]
    lo, hi = _c_layer(below, keep), _c_layer(above, keep)
    s = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        nat.check(L.dod_draw_detections(nat.ptr(img), fp32, B, H, W, lo, hi, C.byref(S), nat.ptr(out), nat.stream_ptr()))
    s.synchronize()
    assert bool((raw[:guard] == SENT).all()) and bool((raw[guard + n:] == SENT).all()), "guard bytes written"
    return out.cpu().numpy().reshape(B, H, W, 3)


def _check(images, below, above, st, **kw):
    want = dw.draw_ref(images, below, above, st)
    got = _run(images, below, above, st, **kw)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at (b, y, x, c) = {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    return got


@pytest.mark.parametrize("guard", GUARDS)
@pytest.mark.parametrize("font_scale,fill", [(0, 0), (1, 0), (2, 96)])
def test_small_odd_batch(gpu, guard, font_scale, fill):
    """B = 2, 37 x 45: 3 W is no multiple of 4, H and W are no multiples of the tile"""
    img, gt, pred = dw.rand_scene(20, 2, 37, 45, 12, 5)
    got = _check(img, gt, pred, dw.style(2, fill, font_scale, names=dw.names_array()), guard=guard, in_offset=guard % 4)
    assert (got != img).any()


@pytest.mark.parametrize("guard", GUARDS)
def test_uint8_form_two_tiles_a_side(gpu, guard):
    img, gt, pred = dw.rand_scene(21, 1, 70, 70, 20, 6)
    _check(img, gt, pred, dw.style(3, 40, 1, names=dw.names_array()), guard=guard, in_offset=(guard + 2) % 4)


def test_fp32_form_and_its_rounding_edges(gpu):
    x = dw.fp32_edges(22, 70, 70)
    assert np.isnan(x).sum() > 50 and (x == 1).sum() > 50 and (x == 0).sum() > 50 and (x == -1).sum() > 50 and (x == 2).sum() > 50 and np.isinf(x).sum() > 50
    b = dw.to_bytes(x)
    assert b[np.isnan(x).transpose(0, 2, 3, 1)].max() == 0 and len(np.unique(b)) == 256
    _, gt, pred = dw.rand_scene(22, 1, 70, 70, 20, 6)
    assert np.array_equal(_check(x, None, None, dw.style(2, 0, 0)), b)                  # nothing to draw: the conversion alone
    _check(x, gt, pred, dw.style(2, 64, 1), guard=37)


@pytest.mark.parametrize("font_scale,fp32", [(1, False), (2, True)])
def test_both_layers_lists_longer_than_a_wave(gpu, font_scale, fp32):
    """224 x 224, 100 predictions and 20 ground-truth boxes, captions, fill 64: a tile's list holds more than 64 rows"""
    img, gt, pred = dw.rand_scene(23, 1, 224, 224, 100, 20)
    pred["counts"][:] = 100
    gt["counts"][:] = 20
    pred["threshold"] = -1.0
    u = dw.synth.uniform01(24, "draw.big", (80, 4)).astype(np.float32)                  # 80 large boxes that all hold the pixel (50, 75)
    pred["boxes"][0, :80] = np.stack([u[:, 0] * 40, 40 + u[:, 1] * 30, 100 + u[:, 2] * 100, 100 + u[:, 3] * 100], -1)
    if fp32:
        img = np.ascontiguousarray(img.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    st = dw.style(2, 64, font_scale, names=dw.names_array())
    rects = [dw.pixel_rect(r, 0, 224, 224) for r in pred["boxes"][0]]
    assert sum(r is not None and r[0] < 64 and r[2] >= 0 and r[1] < 80 and r[3] >= 64 for r in rects) > 64
    _check(img, gt, pred, st)


def test_list_at_capacity(gpu):
    """32 x 32, K = 1024 in both layers, every box over the one tile: 2048 records"""
    B, H, W, K = 1, 32, 32, 1024
    img = dw.rand_images_u8(25, B, H, W)
    u = dw.synth.uniform01(25, "draw.cap", (2, K, 4)).astype(np.float32)
    bx = np.stack([u[..., 0] * 12 - 2, u[..., 1] * 12 - 2, 18 + u[..., 2] * 16, 18 + u[..., 3] * 16], -1).astype(np.float32)
    lab = (dw.synth.uniform01(26, "draw.cap.l", (2, K)) * 1000).astype(np.int32)
    sc = dw.synth.uniform01(27, "draw.cap.s", (1, K))
    above = dw.layer(bx[:1], lab[:1], np.asarray([K], np.int32), sc, 0, -1.0, True)
    cx = np.stack([(bx[1, :, 0] + bx[1, :, 2]) / 2 / W, (bx[1, :, 1] + bx[1, :, 3]) / 2 / H, (bx[1, :, 2] - bx[1, :, 0]) / W, (bx[1, :, 3] - bx[1, :, 1]) / H], -1)
    below = dw.layer(cx[None].astype(np.float32), lab[1:], np.asarray([K], np.int32), None, 1, -1.0, False, (255, 255, 0))
    for st in (dw.style(1, 16, 1), dw.style(1, 255, 0)):
        _check(img, below, above, st, guard=37)


def test_counts_and_absent_layers(gpu):
    img, gt, pred = dw.rand_scene(28, 2, 37, 45, 6, 4)
    st = dw.style(2, 32, 1)
    pred["threshold"] = -1.0
    for counts in ([0, 0], [0, 6], [9, 100], [-3, 2]):                                  # 0: nothing, > K: clamped to K, < 0: clamped to 0
        pred["counts"] = np.asarray(counts, np.int32)
        got = _check(img, gt, pred, st)
    pred["counts"] = np.asarray([0, 0], np.int32)
    assert np.array_equal(_check(img, None, pred, st), img)
    pred["counts"] = None                                                               # no counts: K rows everywhere
    full = _check(img, None, pred, st)
    pred["counts"] = np.asarray([6, 6], np.int32)
    assert np.array_equal(_check(img, None, pred, st), full)
    empty = dw.layer(np.zeros((2, 0, 4), np.float32), np.zeros((2, 0), np.int32))       # K = 0
    assert np.array_equal(_check(img, empty, empty, st), img)
    assert np.array_equal(_check(img, None, None, st), img)                             # both layers absent: a straight copy
    only_gt, only_pred = _check(img, gt, None, st), _check(img, None, pred, st)
    assert (only_gt != img).any() and (only_pred != img).any() and (got != only_gt).any()


def test_skipped_rows_and_edges(gpu):
    H, W = 37, 45
    img = dw.rand_images_u8(29, 1, H, W)
    nan = np.float32(np.nan)
    skipped = np.asarray([[[nan, 5, 20, 20], [5, nan, 20, 20], [5, 5, nan, 20], [5, 5, 20, nan], [20, 5, 5, 20], [5, 20, 20, 5], [7, 7, 7, 9],
                           [-30, 5, -0.5, 20], [45, 5, 60, 20], [5, -20, 20, 0], [5, 37, 20, 50], [50, 50, 60, 60], [-1e30, -1e30, -1e20, -1e20]]], np.float32)
    st = dw.style(2, 80, 1)
    assert np.array_equal(_check(img, None, dw.layer(skipped, np.arange(13)[None]), st), img)
    # a box over each edge, over each corner, and one holding the whole image (infinite corners saturate)
    over = np.asarray([[[-6.5, 10, 9.25, 22], [38.5, 8, 51, 30], [12, -7.75, 30, 6.5], [12, 30.5, 30, 44], [-3, -3, 6, 6], [40, 31, 1e9, 1e9],
                        [-np.inf, -np.inf, np.inf, np.inf], [-0.5, 5, 0.5, 20]]], np.float32)
    for t in (1, 3, 8):
        got = _check(img, None, dw.layer(over, np.arange(8)[None], use_palette=True), dw.style(t, 80, 0), guard=37)
        assert (got != img).any()


def test_caption_placement(gpu):
    H, W = 37, 45
    img = dw.rand_images_u8(30, 1, H, W)
    names = dw.names_array()
    bx = np.asarray([[[5, 20, 30, 34],          # room above
                      [3, 4, 30, 18],           # no room above: inside the box
                      [38, 22, 44, 36],         # shifted left
                      [-9, 15, 12, 30],         # box starts left of the image: the caption starts at x = 0
                      [10, 30, 20, 36.5]]], np.float32)
    lab = np.asarray([[1, 4, 2, 3, 5]], np.int32)
    for s in (1, 2, 3, 4):                      # at scale 3 and 4 "traffic_light 100%" is wider than the image, at 4 the caption is 36 of 37 rows
        for rows in ([0], [1], [2], [3], [4], [0, 1, 2, 3, 4]):
            ly = dw.layer(bx[:, rows], lab[:, rows], None, np.ones((1, len(rows)), np.float32), 0, -1.0, True)
            _check(img, None, ly, dw.style(1, 0, s, names=names))
    assert dw.caption_rect(5, 20, 10, 1, H, W)[1] == 11 and dw.caption_rect(3, 4, 18, 1, H, W)[1] == 4 and dw.caption_rect(38, 22, 12, 1, H, W)[0] < 38
    # a tiny image: the caption is cut in both directions
    tiny = dw.rand_images_u8(31, 1, 7, 9)
    _check(tiny, None, dw.layer(np.asarray([[[1, 1, 8, 6]]], np.float32), np.asarray([[1]], np.int32)), dw.style(1, 0, 2, names=names), guard=37)


def test_score_threshold(gpu):
    img = dw.rand_images_u8(32, 1, 37, 45)
    bx = np.asarray([[[2, 2, 14, 14], [16, 2, 28, 14], [30, 2, 42, 14], [2, 20, 14, 32]]], np.float32)
    thr = np.float32(0.3)
    sc = np.asarray([[thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), np.nan]], np.float32)
    ly = dw.layer(bx, np.zeros((1, 4), np.int32), None, sc, 0, float(thr), True)
    got = _check(img, None, ly, dw.style(1, 255, 0))
    same = lambda r: np.array_equal(got[0, int(r[1]):int(r[3]), int(r[0]):int(r[2])], img[0, int(r[1]):int(r[3]), int(r[0]):int(r[2])])
    assert same(bx[0, 0]) and not same(bx[0, 1]) and same(bx[0, 2]) and not same(bx[0, 3])      # at the threshold: skipped; a NaN score is kept
    ly["threshold"] = -1.0
    got = _check(img, None, ly, dw.style(1, 255, 1))
    assert not same(bx[0, 0]) and not same(bx[0, 2])
    ly["threshold"] = 0.0
    ly["scores"] = np.asarray([[0.0, -0.0, 1e-30, -1.0]], np.float32)
    _check(img, None, ly, dw.style(1, 255, 0))


def test_labels_beyond_names_and_palette(gpu):
    img = dw.rand_images_u8(33, 1, 45, 70)
    names = dw.names_array()
    names[9, 3] = 0xE9                                                                  # a byte past 0x7F inside a name: a solid cell
    labs = [0, 1, 5, 6, 7, 8, 9, len(names) - 1, len(names), 19, 20, 21, 1000, 123456789, 2147483647, -1, -21, -2147483648]
    u = dw.synth.uniform01(33, "draw.lab", (len(labs), 2))
    bx = np.asarray([[[x * 50, 10 + y * 30, x * 50 + 18, 10 + y * 30 + 9] for x, y in u]], np.float32)
    ly = dw.layer(bx, np.asarray([labs], np.int32), None, None, 0, -1.0, True)
    for nm in (names, None):
        _check(img, None, ly, dw.style(1, 0, 1, names=nm))
    _check(img, None, ly, dw.style(1, 0, 1, palette=[(0, 0, 0), (255, 255, 255), (10, 200, 10)], names=names[:2]))      # black and white boxes: both text colours


def test_normalised_format_equals_pixel_format(gpu):
    B, H, W, G = 2, 37, 45, 9
    img = dw.rand_images_u8(34, B, H, W)
    cx = dw.rand_cxcywh(34, B, G)
    lab = np.arange(B * G, dtype=np.int32).reshape(B, G)
    px = np.stack([dc.boxes_of(cx[b], (np.float32(H), np.float32(W)), False) for b in range(B)])
    st = dw.style(2, 50, 1)
    a = _check(img, dw.layer(cx, lab, fmt=1), None, st)
    b = _check(img, dw.layer(px, lab, fmt=0), None, st)
    assert np.array_equal(a, b) and (a != img).any()


def test_pixels_outside_every_rectangle_keep_the_input(gpu):
    img, gt, pred = dw.rand_scene(35, 2, 70, 90, 8, 3)
    st = dw.style(2, 128, 1, names=dw.names_array())
    want, touched = dw.draw_ref(img, gt, pred, st, return_touched=True)
    got = _run(img, gt, pred, st, guard=37)
    assert np.array_equal(got, want)
    assert 0.02 < touched.mean() < 0.98
    assert np.array_equal(got[~touched], img[~touched])
    x = np.ascontiguousarray(img.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))      # the fp32 form of the same bytes
    assert np.array_equal(dw.to_bytes(x), img)
    assert np.array_equal(_run(x, gt, pred, st), got)


def test_repeatable_and_stream_independent(gpu):
    img, gt, pred = dw.rand_scene(36, 2, 70, 90, 40, 10)
    st = dw.style(2, 77, 1, names=dw.names_array())
    a = _run(img, gt, pred, st)
    assert np.array_equal(a, _run(img, gt, pred, st))
    assert np.array_equal(a, _run(img, gt, pred, st, stream=torch.cuda.Stream()))
    assert np.array_equal(a, dw.draw_ref(img, gt, pred, st))


def test_python_entry_end_to_end(gpu):
    """seeded packed detections -> detect_packed(sizes=(H, W), nms_iou=0.5) -> draw_detections, against the restatement fed with
    detect_cases.detect_ref's output; targets as the train loop's list of dicts"""
    from dinov2_od_amd.postprocess import detect_packed
    B, Q, Cn, K, H, W = 2, 40, 11, 25, 70, 90
    det_np = dc.random_det(37, B, Q, Cn, mean=-2.5, std=1.5)      # about 15 of an image's 25 best score above 0.5
    img = dw.rand_images_u8(37, B, H, W)
    gtb = dw.rand_cxcywh(38, B, 4)
    gtl = np.asarray([[1, 2, 3, 4], [5, 6, 7, 8]], np.int64)
    ns = [3, 0]
    targets = [{"boxes": torch.from_numpy(gtb[b, :ns[b]]).cuda(), "labels": torch.from_numpy(gtl[b, :ns[b]]).cuda()} for b in range(B)]
    r = detect_packed(torch.from_numpy(det_np).cuda(), Cn, (H, W), top_k=K, nms_iou=0.5)
    names = [f"class_{i}" for i in range(Cn)]
    pal = [(250, 10, 10), (10, 250, 10), (10, 10, 250)]
    got = V.draw_detections(torch.from_numpy(img).cuda(), r, targets, names, score_threshold=0.5, thickness=1, fill_alpha=40, font_scale=1,
                            palette=pal, gt_color=(255, 255, 0))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
    ref = dc.detect_ref(det_np, Cn, K, 1, (float(H), float(W)), -1.0, 0.5, False, True)
    assert np.array_equal(r.counts.cpu().numpy(), ref["counts"]) and np.array_equal(r.labels.cpu().numpy(), ref["labels"])
    # the restatement draws detect_ref's boxes and labels; the scores are the kernel's own (they agree to 3e-7, the caption shows whole percents)
    above = dw.layer(ref["boxes"], ref["labels"], ref["counts"], r.scores.cpu().numpy(), 0, 0.5, True)
    below = dw.layer(gtb, gtl, np.asarray(ns, np.int32), None, 1, -1.0, False, (255, 255, 0))
    st = dw.style(1, 40, 1, palette=pal, names=V.names_table(names))
    want = dw.draw_ref(img, below, above, st)
    assert np.array_equal(got.cpu().numpy(), want) and (want != img).any()
    kept = (r.scores.cpu().numpy() > 0.5).sum()
    assert 0 < kept < ref["counts"].sum()                                                # the threshold removes some rows and keeps some
    # the fp32 form through Python, the padded-tensor form of the targets, defaults
    x = torch.from_numpy(np.ascontiguousarray(img.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))).cuda()
    padded = {"boxes": torch.from_numpy(gtb).cuda(), "labels": torch.from_numpy(gtl).cuda(), "counts": torch.tensor(ns, dtype=torch.int32).cuda()}
    got2 = V.draw_detections(x, r, padded, names, score_threshold=0.5, thickness=1, fill_alpha=40, font_scale=1, palette=pal, gt_color=(255, 255, 0))
    assert torch.equal(got, got2)
    d = V.draw_detections(x, r)
    assert np.array_equal(d.cpu().numpy(), dw.draw_ref(img, None, dw.layer(ref["boxes"], ref["labels"], ref["counts"], r.scores.cpu().numpy(), 0, 0.0, True), dw.style()))


def test_log_images_and_save_images(gpu, tmp_path):
    from PIL import Image
    from dinov2_od_amd.postprocess import detect_packed
    B, Q, Cn, H, W = 10, 12, 6, 37, 45
    det_np = dc.random_det(39, B, Q, Cn, mean=0.0, std=2.0)
    det = torch.from_numpy(det_np).cuda()
    x = torch.from_numpy(dw.rand_images_u8(39, B, H, W)).cuda()

    class Writer:
        calls = []

        def add_images(self, tag, img, step, dataformats="NCHW"):
            self.calls.append((tag, img, step, dataformats))

    out = {"pred_logits": det[..., :Cn].contiguous(), "pred_boxes": det[..., Cn:].contiguous()}
    w = Writer()
    V.log_images(w, x, None, out, 5, "train", score_threshold=0.3, font_scale=2)
    tag, drawn, step, fmt = w.calls[0]
    assert (tag, step, fmt) == ("train", 5, "NHWC") and tuple(drawn.shape) == (8, H, W, 3)
    want = V.draw_detections(x[:8], detect_packed(det[:8], Cn, (H, W), top_k=100), score_threshold=0.3, font_scale=2)
    assert torch.equal(drawn, want) and not torch.equal(drawn, x[:8])
    paths = V.save_images(str(tmp_path), x[:3], detect_packed(det[:3], Cn, (H, W), top_k=100), names=["a.jpg", "dir/b.png", "c"], score_threshold=0.3, font_scale=2)
    assert [p.split("/")[-1] for p in paths] == ["a.png", "b.png", "c.png"]
    for i, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), want[i].cpu().numpy())
