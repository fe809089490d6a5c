"""GPU parity of the JPEG decode (dod_jpeg_*, dinov2_od_amd/jpeg.py decode_jpeg_batch): bit for bit the numpy restatement of
tests/jpeg_cases.py (itself pinned against Pillow by tests/test_jpeg_cpu.py) and the stored fixture pixels, on every case of the grid
and through both entropy paths; guard bytes around the output, plane and coefficient buffers; the two entropy paths' coefficient
buffers against each other; the Pillow fallback inside a mixed batch; and the entry points that take a `DecodedBatch` against the same
calls on Pillow-decoded arrays.  Only well-formed streams reach the device: the malformed ones are test_jpeg_cpu.py's, on the host."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_cases as jc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096          # bytes in front of and behind every buffer of a decode
SENT = 0xA5


@pytest.fixture(scope="module")
def jpeg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))


class _Ref(dict):
    """name -> the restatement's pixels of a grid case, decoded when a test first asks for it and kept, read-only, for the others"""

    def __missing__(self, name):
        self[name] = px = jc.decode(jc.grid()[name])
        px.setflags(write=False)
        return px


@pytest.fixture(scope="module")
def ref():
    return _Ref()


@pytest.fixture(scope="module")
def turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


class Guarded:
    """stands in for jpeg._device_buffer: every buffer of the decode sits between GUARD sentinel bytes"""

    def __init__(self):
        self.raw = {}

    def __call__(self, name, nbytes, dev):
        raw = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.raw[name] = (raw, nbytes)
        return raw[GUARD:GUARD + nbytes]

    def view(self, name):
        raw, n = self.raw[name]
        return raw[GUARD:GUARD + n]

    def intact(self):
        torch.cuda.synchronize()
        for name, (raw, n) in self.raw.items():
            assert bool((raw[:GUARD] == SENT).all()) and bool((raw[GUARD + n:] == SENT).all()), f"a guard byte of {name} was written"


def _decode(jpeg, monkeypatch, files, **kw):
    g = Guarded()
    monkeypatch.setattr(jpeg, "_device_buffer", g)
    batch = jpeg.decode_jpeg_batch(files, **kw)
    g.intact()
    batch.check()
    return batch, g


def _compare(batch, names, ref, golden, turbo):
    assert len(batch) == len(names) and [tuple(i.shape) for i in batch.images()] == [ref[n].shape for n in names]
    host = batch.src.cpu().numpy()
    g = jc.grid()
    for n, o, h, w in zip(names, batch.src_offs, batch.heights, batch.widths):
        got = host[o:o + int(h) * int(w) * 3].reshape(int(h), int(w), 3)
        assert np.array_equal(got, ref[n]), (n, int((got != ref[n]).sum()))
        if "p_" + n in golden.files and np.array_equal(golden["f_" + n], np.frombuffer(g[n], np.uint8)):
            assert np.array_equal(got, golden["p_" + n]), n
        if turbo:
            assert np.array_equal(got, jc.pillow_decode(g[n])), n


def test_device_entropy_on_every_case_with_restart_markers(jpeg, monkeypatch, ref, golden, turbo):
    g = jc.grid()
    names = [n for n in g if jc.has_restart(g[n])]
    assert len(names) == 361
    batch, _ = _decode(jpeg, monkeypatch, [g[n] for n in names], entropy="device")
    assert set(batch.routes) == {"device"}
    _compare(batch, names, ref, golden, turbo)


def test_host_entropy_on_every_case(jpeg, monkeypatch, ref, golden, turbo):
    g = jc.grid()
    names = list(g)
    batch, _ = _decode(jpeg, monkeypatch, [g[n] for n in names], entropy="host")
    assert set(batch.routes) == {"host"}
    _compare(batch, names, ref, golden, turbo)


def test_fixture_files_decode_to_the_fixture_pixels(jpeg, monkeypatch, golden):
    """the stored files themselves (whatever encoder the Pillow here has): both entropy paths give the stored pixels"""
    names = [k[2:] for k in golden.files if k.startswith("f_") and k != "f_progressive"]
    for entropy, pick in (("host", names), ("device", [n for n in names if jc.has_restart(golden["f_" + n].tobytes())])):
        assert len(pick) >= 61
        batch, _ = _decode(jpeg, monkeypatch, [golden["f_" + n] for n in pick], entropy=entropy)
        for n, img in zip(pick, batch.images()):
            assert np.array_equal(img.cpu().numpy(), golden["p_" + n]), (entropy, n)


def test_auto_on_a_mixed_batch_with_fallback(jpeg, monkeypatch, ref, golden):
    g = jc.grid()
    names = ["w37h53_s0_q90_plain_n60", "w37h53_s2_q90_rows1_n60", "grey_w37h53"]
    files = [g[n] for n in names] + [golden["f_progressive"]]
    batch, _ = _decode(jpeg, monkeypatch, files)
    assert batch.routes == ["host", "device", "host", None]
    imgs = [i.cpu().numpy() for i in batch.images()]
    for n, got in zip(names, imgs):
        assert np.array_equal(got, ref[n]), n
    assert np.array_equal(imgs[3], jc.pillow_decode(golden["f_progressive"].tobytes()))       # the fallback IS Pillow's decode
    assert imgs[3].shape == golden["p_progressive"].shape
    assert int(batch.status.abs().sum()) == 0
    with pytest.raises(jpeg.UnsupportedJpeg, match="file 3: progressive") as e:
        jpeg.decode_jpeg_batch(files, fallback=False)
    assert e.value.index == 3 and e.value.reason == "progressive"
    with pytest.raises(ValueError, match="no restart markers"):
        jpeg.decode_jpeg_batch(files[:1], entropy="device")
    # a batch that is all fallback launches nothing and still returns the pixels
    only = jpeg.decode_jpeg_batch([golden["f_progressive"]])
    assert np.array_equal(only.images()[0].cpu().numpy(), imgs[3])


def test_fill_bytes_in_front_of_markers_change_nothing(jpeg, monkeypatch, ref):
    """FF FF Dn / FF FF D9: legal fill bytes in front of every marker behind the scan header; both paths, same pixels, no flag"""
    data = jc.with_fill_bytes()
    for entropy in ("device", "host"):
        batch, _ = _decode(jpeg, monkeypatch, [data], entropy=entropy)             # _decode runs check()
        assert np.array_equal(batch.images()[0].cpu().numpy(), ref["w37h53_s2_q90_rows1_n60"]), entropy


def test_device_and_host_entropy_give_identical_coefficients_and_planes(jpeg, monkeypatch):
    g = jc.grid()
    names = [n for n in g if jc.has_restart(g[n])][::5] + ["every_mcu"]
    files = [g[n] for n in names]
    _, dev = _decode(jpeg, monkeypatch, files, entropy="device")
    _, host = _decode(jpeg, monkeypatch, files, entropy="host")
    for name in ("coef", "planes", "out"):
        assert torch.equal(dev.view(name), host.view(name)), name
    want = np.concatenate([np.concatenate([c.reshape(-1) for c in jc.coefficients(f)[1]]) for f in files])
    assert np.array_equal(dev.view("coef").view(torch.int16).cpu().numpy(), want)
    assert dev.view("planes").numel() == want.size and dev.view("out").numel() == sum(3 * jc.parse(f)["width"] * jc.parse(f)["height"] for f in files)


def _pick(golden, *parts):
    """the fixture case whose name holds all of `parts`"""
    return next(k[2:] for k in golden.files if k.startswith("f_") and all(p in k for p in parts))


def test_consumers_read_a_decoded_batch_like_pillow_arrays(jpeg, golden):
    """preprocess_batch, augment_batch, compose_batch, warp_batch, extract_views and TrainAugment on a DecodedBatch == the same calls on
    the Pillow-decoded arrays, bit for bit (the files and pixels are the fixture's)"""
    from dinov2_od_amd import augment, preprocess, slicing
    names = [_pick(golden, "w37h53_s2", "rows1"), _pick(golden, "w17h33_s1", "opt"), "grey_w40h3", "every_mcu", _pick(golden, "w37h53_s0", "plain")]
    files = [golden["f_" + n] for n in names] + [golden["f_progressive"]]
    arrs = [golden["p_" + n] for n in names] + [golden["p_progressive"]]
    B = len(files)
    batch = jpeg.decode_jpeg_batch(files).check()
    for as_u8 in (False, True):
        assert torch.equal(preprocess.preprocess_batch(batch, (32, 48), as_uint8=as_u8), preprocess.preprocess_batch(arrs, (32, 48), as_uint8=as_u8))
    crops = np.array([[0, 0, a.shape[1], a.shape[0]] if i % 2 else [a.shape[1] // 4, a.shape[0] // 4, max(a.shape[1] // 2, 1), max(a.shape[0] // 2, 1)]
                      for i, a in enumerate(arrs)])
    flips = np.arange(B) % 2 == 0
    jit = np.tile([1.2, 0.8, 1.1], (B, 1))
    a, _ = augment.augment_batch(batch, None, crops, flips, jit, (24, 40), as_uint8=True)
    b, _ = augment.augment_batch(arrs, None, crops, flips, jit, (24, 40), as_uint8=True)
    assert torch.equal(a, b)
    pieces = [[(0, (0, 0, arrs[0].shape[1], arrs[0].shape[0]), False, None, (0, 0, 20, 16)), (B - 1, (1, 1, 8, 8), True, None, (20, 16, 12, 16))]]
    a, _ = augment.compose_batch(batch, None, pieces, (32, 32), as_uint8=True)
    b, _ = augment.compose_batch(arrs, None, pieces, (32, 32), as_uint8=True)
    assert torch.equal(a, b)
    coeffs = np.stack([augment.affine_coeffs(x.shape[:2], (24, 24), angle=10.0 * i) for i, x in enumerate(arrs)])
    a, _ = augment.warp_batch(batch, None, coeffs, (24, 24), as_uint8=True)
    b, _ = augment.warp_batch(arrs, None, coeffs, (24, 24), as_uint8=True)
    assert torch.equal(a, b)
    plan = slicing.plan_views(batch.shapes, 24, 0.2, True, True, size=(32, 32), pairs=25 * 91)
    assert torch.equal(slicing.extract_views(batch, plan, (32, 32)), slicing.extract_views(arrs, plan, (32, 32)))
    outs = []
    for images in (batch, arrs):
        gen = torch.Generator().manual_seed(11)
        ta = augment.TrainAugment((32, 32), brightness=0.3, contrast=0.3, generator=gen, as_uint8=True, mosaic_prob=0.5, affine_prob=0.5, degrees=15.0)
        outs.append(ta(images, None)[0])
    assert torch.equal(outs[0], outs[1])
    files2, targets = jpeg.collate_encoded([(f, {"i": i}) for i, f in enumerate(files)])
    assert len(files2) == B and targets[2] == {"i": 2}


def test_detect_sliced_reads_a_decoded_batch(jpeg, golden):
    from tests import cases, gpu_util as G
    names = [k[2:] for k in golden.files if k.startswith("f_w37h53_s2")][:2]
    files, arrs = [golden["f_" + n] for n in names], [golden["p_" + n] for n in names]
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "bf16", "facebook/dinov2-small").eval()
    kw = dict(size=(224, 224), tile=32, overlap=0.2, full_view=True, flip=False, top_k=20, threshold=-1.0, nms_iou=0.5)
    a = m.detect_sliced(jpeg.decode_jpeg_batch(files, entropy="host"), **kw)
    b = m.detect_sliced(arrs, **kw)
    for k in ("scores", "labels", "boxes", "counts", "views"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
