"""GPU parity of the device input pipeline (dod_preprocess): bit-exact against Pillow's BILINEAR resize + ToTensor
(what the reference's transform, train.py:584-587, computes) and against the numpy oracle, for ragged batches."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as ppo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pre():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import preprocess
    return preprocess


def _imgs(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]


def _pillow(img, out_h, out_w):
    from PIL import Image
    r = np.array(Image.fromarray(img, "RGB").resize((out_w, out_h), Image.BILINEAR))
    return (np.transpose(r, (2, 0, 1)).astype(np.float32) / np.float32(255.0))


@pytest.mark.parametrize("size", [(224, 224), (518, 518)])
def test_ragged_batch_is_bit_exact_against_pillow(pre, size):
    shapes = [(480, 640), (427, 640), (640, 480), (333, 500), (224, 224), (100, 80), (518, 700), (225, 223), (1000, 37), (37, 1000)]
    imgs = _imgs(shapes, 1)
    imgs[3][:, ::2] = 255
    imgs[3][:, 1::2] = 0                     # hard edges: rounding / clipping
    got = pre.preprocess_batch(imgs, size).cpu().numpy()
    assert got.shape == (len(imgs), 3, size[0], size[1]) and got.dtype == np.float32
    for i, im in enumerate(imgs):
        want = _pillow(im, *size)
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), shapes[i]
        assert np.array_equal(got[i], ppo.preprocess([im], *size)[0])


def test_coco_sized_batch_and_non_square_target(pre):
    """the bench batch's worth of COCO-sized images (64 x 480x640) and a non-square target"""
    imgs = _imgs([(480, 640)] * 8 + [(640, 427)] * 8, 2)
    got = pre.preprocess_batch(imgs, (224, 320)).cpu().numpy()
    for i in (0, 7, 8, 15):
        assert np.array_equal(got[i], _pillow(imgs[i], 224, 320))
    t = pre.ResizeToTensor((224, 224))(imgs[:2])
    assert t.is_cuda and t.shape == (2, 3, 224, 224) and float(t.min()) >= 0.0 and float(t.max()) <= 1.0


def test_accepts_torch_and_pil_inputs_and_rejects_bad_ones(pre):
    from PIL import Image
    im = _imgs([(50, 60)], 3)[0]
    a = pre.preprocess_batch([im, torch.from_numpy(im), Image.fromarray(im, "RGB")], (32, 32)).cpu().numpy()
    assert np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2])
    with pytest.raises(ValueError):
        pre.preprocess_batch([im.astype(np.float32)], (32, 32))
    with pytest.raises(ValueError):
        pre.preprocess_batch([im[:, :, :1]], (32, 32))
    with pytest.raises(ValueError):
        pre.preprocess_batch([np.zeros((4000, 4000, 3), np.uint8)], (32, 32))       # > 15x down-scaling: filter wider than PP_MAXK


def test_uint8_pipeline_feeds_the_fused_patch_embed_bit_exactly(pre):
    """f4 fused into K1: the resampled bytes (uint8 HWC, Pillow-exact) go straight into the patch-embedding kernel, which applies
    ToTensor's / 255 in its load stage -- same detections, bit for bit, as the fp32 CHW batch through the same model"""
    from PIL import Image
    from dinov2_od_amd import synth
    from tests import cases, gpu_util as G
    imgs = _imgs([(480, 640), (333, 500), (100, 80)], 5)
    u8 = pre.preprocess_batch(imgs, (224, 224), as_uint8=True)
    assert u8.dtype == torch.uint8 and u8.shape == (3, 224, 224, 3)
    for i, im in enumerate(imgs):
        assert np.array_equal(u8[i].cpu().numpy(), np.array(Image.fromarray(im, "RGB").resize((224, 224), Image.BILINEAR)))
    f32 = pre.preprocess_batch(imgs, (224, 224))
    bb, dc = cases.cfg1(25)
    for precision in ("bf16x3", "bf16"):
        m = G.make_detector(bb, dc, precision, "facebook/dinov2-small")
        a = m.forward_packed(f32).clone()
        b = m.forward_packed_u8(u8).clone()
        assert torch.equal(a, b), precision
    m = G.make_detector(bb, dc, "fp32", "facebook/dinov2-small")
    with pytest.raises(ValueError, match="fused patch embed"):
        m.forward_packed_u8(u8)                          # exact-fp32 mode keeps the explicit im2col + fp32 GEMM


# ------------------------------------------------------------------------------------------- the plain entry on edge shapes
EDGE_SHAPES = [(1, 1), (1, 700), (17, 3), (33, 513), (75, 4500)]


@pytest.mark.parametrize("size,transposed", [((5, 300), False), ((300, 5), True)])
def test_edge_shapes_are_bit_exact_against_pillow_and_the_oracle(pre, size, transposed):
    """what one ragged batch hits at these two sizes: a window clipped at both ends (1x1), two 256-column blocks of which the second is
    partial (300 = 256 + 44), one row past a 16-row block (17), up-scaling, 31 taps on both axes at once (4500 -> 300 and 75 -> 5, the
    most the 32-tap bound admits here), and max_h / max_w that come from different images"""
    from PIL import Image
    shapes = [(w, h) for h, w in EDGE_SHAPES] if transposed else EDGE_SHAPES
    imgs = _imgs(shapes, 7)
    f32 = pre.preprocess_batch(imgs, size).cpu().numpy()
    u8 = pre.preprocess_batch(imgs, size, as_uint8=True).cpu().numpy()
    assert f32.shape == (len(imgs), 3) + size and u8.shape == (len(imgs),) + size + (3,) and u8.dtype == np.uint8
    for i, im in enumerate(imgs):
        pil = np.array(Image.fromarray(im, "RGB").resize((size[1], size[0]), Image.BILINEAR))
        assert np.array_equal(u8[i], pil), (shapes[i], "uint8 vs Pillow")
        assert np.array_equal(u8[i], ppo.resize_bilinear_u8(im, *size)), (shapes[i], "uint8 vs the oracle")
        assert np.array_equal(f32[i].view(np.uint32), _pillow(im, *size).view(np.uint32)), (shapes[i], "fp32 vs Pillow")
        assert np.array_equal(f32[i].view(np.uint32), ppo.preprocess([im], *size)[0].view(np.uint32)), (shapes[i], "fp32 vs the oracle")


@pytest.mark.parametrize("as_uint8", [False, True])
def test_empty_images_in_a_batch_come_out_all_zero(pre, as_uint8):
    """an image without rows or without columns has no filter taps: every output byte is clip8(1 << 21) = 0 (fp32: +0.0), and the
    image next to it in the batch is Pillow's"""
    from PIL import Image
    imgs = _imgs([(0, 5), (4, 0), (6, 7)], 8)
    got = pre.preprocess_batch(imgs, (3, 9), as_uint8=as_uint8).cpu().numpy()
    assert got.shape == ((3, 3, 9, 3) if as_uint8 else (3, 3, 3, 9))
    zero = got[:2].view(np.uint8 if as_uint8 else np.uint32)
    assert not zero.any(), "an empty image gave something other than zero bytes"
    pil = np.array(Image.fromarray(imgs[2], "RGB").resize((9, 3), Image.BILINEAR))
    assert np.array_equal(got[2], pil if as_uint8 else ppo.to_tensor(pil))


# ------------------------------------------------------------------------------- the three entries refuse the same arguments
# One valid call per entry (an 8x8 source, a 4x4 output), then one argument wrong at a time.  "taps33" is the smallest width the
# 32-tap bound refuses (15 * out_w + 1: ceil -> 16, 33 taps), "taps35" is 16 * out_w + 1.  Rows that other files already assert
# through the same entries are not repeated here: dod_preprocess_aug with 33 taps (test_gpu_augment.py,
# test_bad_arguments_raise_before_anything_is_launched), dod_preprocess_compose with 33 taps and with N = 0 / P = 0
# (test_gpu_compose.py, test_bad_arguments_raise_before_anything_is_staged_and_the_entry_checks_its_bounds).
REFUSALS = {"null_src": dict(src=None), "count_0": dict(count=0), "count_65536": dict(count=65536), "no_output": dict(out=None),
            "taps33": dict(max_w=15 * 4 + 1), "taps35": dict(max_w=16 * 4 + 1)}
REFUSED = [(e, r) for e in ("plain", "aug", "compose") for r in REFUSALS
           if (e, r) not in (("aug", "taps33"), ("compose", "taps33"), ("compose", "count_0"))] + [("compose", "pieces_65536")]


def _entry_call(nat, entry, as_uint8, a):
    L, p, i = nat.lib(), nat.ptr, int
    fn = getattr(L, {"plain": "dod_preprocess", "aug": "dod_preprocess_aug", "compose": "dod_preprocess_compose"}[entry] + ("_u8" if as_uint8 else ""))
    head = (p(a["src"]), p(a["src_offs"]), p(a["hs"]), p(a["ws"]))
    tail = (4, 4, p(a["tmp"]), p(a["tmp_offs"]), p(a["out"]), nat.stream_ptr())
    if entry == "plain":
        return fn(*head, i(a["count"]), 8, i(a["max_w"]), *tail)
    if entry == "aug":
        return fn(*head, i(a["count"]), p(a["crops"]), p(a["flips"]), None, None, 8, i(a["max_w"]), *tail)
    return fn(*head, 1, p(a["pieces"]), p(a["piece_offs"]), i(a["count"]), i(a["pieces_n"]), None, None, p(a["fill"]), 0, 8, i(a["max_w"]), 4, *tail)


@pytest.mark.parametrize("as_uint8", [False, True])
@pytest.mark.parametrize("entry,refusal", REFUSED)
def test_the_entries_refuse_bad_arguments_and_launch_nothing(pre, entry, refusal, as_uint8):
    from dinov2_od_amd import _native as nat
    dev = torch.device("cuda")
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=dev)
    nbytes = 4 * 4 * 3 * (1 if as_uint8 else 4)
    a = dict(src=torch.from_numpy(_imgs([(8, 8)], 9)[0].reshape(-1)).to(dev), src_offs=t([0], torch.int64), hs=t([8], torch.int32),
             ws=t([8], torch.int32), count=1, max_w=8, crops=t([0, 0, 8, 8], torch.int32), flips=t([0], torch.uint8),
             pieces=t([0, 0, 0, 8, 8, 0, 0, 0, 4, 4], torch.int32), piece_offs=t([0, 1], torch.int32), pieces_n=1,
             fill=t([1, 2, 3], torch.uint8), tmp=torch.full((8 * 4 * 3,), 0xA5, dtype=torch.uint8, device=dev), tmp_offs=t([0], torch.int64),
             out=torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev))
    bad = dict(a, **(dict(pieces_n=65536) if refusal == "pieces_65536" else REFUSALS[refusal]))
    with pytest.raises(ValueError):                       # DOD_ERR_INVALID
        nat.check(_entry_call(nat, entry, as_uint8, bad))
    torch.cuda.synchronize()
    assert bool((a["out"] == 0xA5).all()) and bool((a["tmp"] == 0xA5).all()), "a refused call wrote something"
    nat.check(_entry_call(nat, entry, as_uint8, a))       # the same arguments without the mistake are a valid call
    want = ppo.resize_bilinear_u8(a["src"].cpu().numpy().reshape(8, 8, 3), 4, 4)
    got = a["out"].cpu().numpy()
    assert np.array_equal(got.reshape(4, 4, 3), want) if as_uint8 else np.array_equal(got.view(np.float32).reshape(3, 4, 4), ppo.to_tensor(want))
