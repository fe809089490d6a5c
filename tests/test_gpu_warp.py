"""GPU parity of the geometric warp (dod_preprocess_warp, dinov2_od_amd/augment.py warp_batch): random affine and perspective as one
inverse-map bilinear gather.  Bit-exact against the numpy restatement of Pillow's Image.transform (tests/warp_cases.py, itself pinned
against Pillow by tests/test_warp_cpu.py) for the uint8 HWC and the fp32 CHW output, contraction probes included; every output element
written exactly once and nothing outside; run-to-run equality; a resident batch against staged arrays; `TrainAugment` with a warp
behind the plain chain and behind a mosaic, images and targets; coefficients and sizes the kernel must survive; the entry's own
argument check."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as ppo
from tests import augment_cases as ac
from tests import compose_cases as cc
from tests import guard_rows as gr
from tests import warp_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aug():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import augment
    return augment


def _stage_case(aug, c):
    from dinov2_od_amd import preprocess as pre
    fill, per_image = aug._check_fill(c["fill"], len(c["images"]))
    src, src_offs, hs, ws = pre._stage(c["images"], torch.device("cuda"))
    return src, src_offs, hs, ws, c["coeffs"], fill, per_image, c["size"][0], c["size"][1]


def _f32_of(want):
    return np.stack([ppo.to_tensor(w) for w in want])


# ------------------------------------------------------------------------- 1. bit-exact, exactly once, in bounds, run to run
@pytest.mark.parametrize("name", list(wc.CASES))
def test_every_case_is_bit_exact_and_written_once_between_intact_guards(aug, name):
    """through the C entries into the middle of a buffer pre-filled with a sentinel (tests/guard_rows.py): the bytes equal the
    restatement under two different sentinels -- a byte the kernel left alone would differ under one of them -- the fp32 output equals
    bytes / 255 in float32 and holds no sentinel word, the guard rows stay intact, and a second call gives the same bits"""
    c, want = wc.case(name)
    B, (out_h, out_w) = len(c["images"]), c["size"]
    args = _stage_case(aug, c)
    for sentinel in (0xA5, 0x5A):
        raw, view = gr.guarded(B * out_h, out_w * 3, torch.uint8, sentinel)
        out = view.view(B, out_h, out_w, 3)
        got = aug._launch_warp(*args, True, out=out)
        assert got.data_ptr() == raw.data_ptr() + gr.GUARD * out_w * 3
        torch.cuda.synchronize()
        assert bool((raw[:gr.GUARD] == sentinel).all()) and bool((raw[gr.GUARD + B * out_h:] == sentinel).all()), "a guard byte was written"
        u8 = out.cpu().numpy()
        for b in range(B):
            assert np.array_equal(u8[b], want[b]), (name, b, sentinel, int((u8[b] != want[b]).sum()))
    # the fp32 output between float32 guard rows.  One sentinel is enough here: SENT_F = -77.25 is no value ToTensor can produce, so an
    # element the kernel left alone shows as the sentinel itself (a byte can take any value, hence the two sentinels above)
    bufs = {"out_f32": gr.guarded(B * 3 * out_h, out_w, torch.float32, gr.SENT_F)}
    raw, view = bufs["out_f32"]
    out = view.view(B, 3, out_h, out_w)
    aug._launch_warp(*args, False, out=out)
    torch.cuda.synchronize()
    gr.untouched(bufs)
    f32 = out.cpu().numpy().copy()
    assert not (f32 == gr.SENT_F).any(), "an element was not written"
    assert np.array_equal(f32.view(np.uint32), _f32_of(want).view(np.uint32)), name
    again = aug._launch_warp(*args, False).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), f32.view(np.uint32))
    assert np.array_equal(aug._launch_warp(*args, True).cpu().numpy(), want)


# -------------------------------------------------------------------------------------------------- 2. the public entry point
def test_warp_batch_on_a_resident_batch_equals_the_staged_call(aug):
    c, want = wc.case("perspective")
    boxes = [torch.from_numpy(wc.random_boxes(6, 20 + b, (40, 50), c["coeffs"][b], c["size"], 0.2)) for b in range(2)]
    targets = [{"boxes": bx, "labels": torch.arange(6), "size": torch.as_tensor([40, 50])} for bx in boxes]
    dev = torch.from_numpy(np.stack(c["images"])).cuda()
    for as_uint8 in (True, False):
        a, ta = aug.warp_batch(dev, targets, c["coeffs"], c["size"], c["fill"], as_uint8=as_uint8, min_visibility=0.2)
        b, tb = aug.warp_batch(c["images"], targets, c["coeffs"], c["size"], c["fill"], as_uint8=as_uint8, min_visibility=0.2)
        assert a.is_cuda and a.shape == ((2, 56, 56, 3) if as_uint8 else (2, 3, 56, 56)) and a.dtype == (torch.uint8 if as_uint8 else torch.float32)
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), want) if as_uint8 else np.array_equal(a.cpu().numpy(), _f32_of(want))
        for x, y, bx, (cf) in zip(ta, tb, boxes, c["coeffs"]):
            keep, ref, _ = wc.targets_f64(bx.numpy(), (40, 50), cf, c["size"], 0.2)
            assert torch.equal(x["boxes"], y["boxes"]) and torch.equal(x["labels"], y["labels"]) and x["size"].tolist() == [56, 56]
            assert torch.equal(x["labels"], torch.arange(6)[torch.from_numpy(keep)])
            assert np.abs(x["boxes"].numpy().astype(np.float64) - ref).max(initial=0.0) <= 2.4e-7
    # a per-image fill, a non-contiguous resident batch, and the refusals: nothing is launched for them
    flipped = torch.from_numpy(np.stack(c["images"])).cuda().flip(0)
    got, none = aug.warp_batch(flipped, None, c["coeffs"][::-1].copy(), c["size"], [(1, 2, 3), (4, 5, 6)], as_uint8=True)
    assert none is None
    for b in range(2):
        assert np.array_equal(got[b].cpu().numpy(), wc.restated_warp(c["images"][1 - b], c["coeffs"][1 - b], 56, 56, (1, 2, 3) if b == 0 else (4, 5, 6)))
    for bad in (dict(coeffs=c["coeffs"][:1]), dict(coeffs=np.full((2, 8), np.nan)), dict(fill=(1, 2)), dict(size=(0, 56)), dict(targets=targets[:1]),
                dict(coeffs=np.array([[1, 2, 0, 2, 4, 0, 0, 0]] * 2, dtype=np.float64)), dict(images=dev.float()), dict(images=dev[..., :2])):
        kw = dict(images=dev, targets=None, coeffs=c["coeffs"], size=c["size"], fill=c["fill"])
        kw.update(bad)
        with pytest.raises(ValueError):
            aug.warp_batch(kw["images"], kw["targets"], kw["coeffs"], kw["size"], kw["fill"])


# ------------------------------------------------------------------------------------------------------------ 3. TrainAugment
def _sources():
    imgs = [ac._rand(s, 700 + i) for i, s in enumerate([(48, 64), (33, 50), (70, 60), (57, 90)])]
    rng = np.random.default_rng(1)
    targets = []
    for b in range(4):
        box = np.concatenate([rng.uniform(0.3, 0.7, (5, 2)), rng.uniform(0.05, 0.5, (5, 2))], 1).astype(np.float32)
        targets.append({"boxes": torch.from_numpy(box), "labels": torch.from_numpy(rng.integers(1, 9, 5)), "size": torch.as_tensor([56, 56])})
    return imgs, targets


JITTER = dict(crop_prob=1.0, crop_frac=(0.6, 0.9), hflip_prob=0.5, brightness=0.3, contrast=0.3, saturation=0.3, min_visibility=0.2)
WARP = dict(affine_prob=1.0, degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=5.0)


def _restated_train_augment(aug, imgs, targets, seed, **kw):
    """the same draws on the host (the samplers are host code and seeded): (uint8 [4, 56, 56, 3] of the chain or canvas before the
    warp, its targets, the coefficients drawn)"""
    t = aug.TrainAugment((56, 56), generator=torch.Generator().manual_seed(seed), **kw)
    shapes = [im.shape[:2] for im in imgs]
    if t.mosaic_prob == 0.0 and t.zoom_out_prob == 0.0:
        crops, flips, jitter = aug.sample_params(shapes, t.generator, **t.sampler)
        chain = np.stack([ac.restated_chain(im, crops[b], flips[b], jitter[b], 56, 56) for b, im in enumerate(imgs)])
        tg = aug.transform_targets(targets, shapes, crops, flips, (56, 56), t.min_visibility)
    else:
        plan = t.sample_plan(shapes)
        chain = cc.restated_compose(imgs, plan, (56, 56), t.fill)
        tg = aug.compose_targets(targets, shapes, plan, (56, 56), t.min_visibility)
    return chain, tg, t.sample_warp(len(imgs))


@pytest.mark.parametrize("mosaic", [False, True])
def test_train_augment_with_a_warp_is_the_restated_chain_then_the_restated_warp(aug, mosaic):
    imgs, targets = _sources()
    kw = dict(JITTER, **WARP, **(dict(mosaic_prob=1.0, mosaic_center=(0.4, 0.6)) if mosaic else {}))
    chain, chain_tg, coeffs = _restated_train_augment(aug, imgs, targets, 5, **kw)
    assert not (coeffs == np.array(aug.IDENTITY_COEFFS)).all(1).any()
    want = np.stack([wc.restated_warp(chain[b], coeffs[b], 56, 56, (124, 116, 104)) for b in range(4)])
    want_tg = aug.warp_targets(chain_tg, [(56, 56)] * 4, coeffs, (56, 56), 0.2)
    for as_uint8 in (True, False):
        x, new = aug.TrainAugment((56, 56), generator=torch.Generator().manual_seed(5), as_uint8=as_uint8, **kw)(imgs, targets)
        assert x.is_cuda and len(new) == 4
        assert np.array_equal(x.cpu().numpy(), want if as_uint8 else _f32_of(want)), (mosaic, as_uint8)
        for tg, h in zip(new, want_tg):
            assert torch.equal(tg["boxes"], h["boxes"]) and torch.equal(tg["labels"], h["labels"]) and tg["size"].tolist() == [56, 56]
            assert tg["boxes"].dtype == torch.float32 and tg["boxes"].shape[1:] == (4,) and tg["labels"].shape == (len(tg["boxes"]),)
            assert bool((tg["boxes"] >= 0).all()) and bool((tg["boxes"] <= 1).all())
    assert 0 < sum(len(tg["boxes"]) for tg in want_tg) and any((w == (124, 116, 104)).all(-1).any() for w in want)      # some fill shows


def test_an_image_that_draws_no_warp_keeps_the_plain_chains_bytes(aug):
    imgs, targets = _sources()
    kw = dict(JITTER, **dict(WARP, affine_prob=0.5), perspective_prob=0.5, distortion=0.4)
    for seed in range(50):          # host only: the first seed with a warped and an unwarped image in the batch
        chain, chain_tg, coeffs = _restated_train_augment(aug, imgs, targets, seed, **kw)
        plain = (coeffs == np.array(aug.IDENTITY_COEFFS)).all(1)
        if plain.any() and not plain.all() and (coeffs[:, 6] != 0).any():
            break
    else:
        raise AssertionError("no seed gives a mixed batch")
    x, new = aug.TrainAugment((56, 56), generator=torch.Generator().manual_seed(seed), as_uint8=True, **kw)(imgs, targets)
    no_warp = {k: v for k, v in kw.items() if k in JITTER}
    y, old = aug.TrainAugment((56, 56), generator=torch.Generator().manual_seed(seed), as_uint8=True, **no_warp)(imgs, targets)
    x, y = x.cpu().numpy(), y.cpu().numpy()
    assert np.array_equal(y, chain)
    for b in range(4):
        if plain[b]:
            assert np.array_equal(x[b], y[b]) and torch.equal(new[b]["boxes"], old[b]["boxes"]) and torch.equal(new[b]["labels"], old[b]["labels"])
        else:
            assert np.array_equal(x[b], wc.restated_warp(chain[b], coeffs[b], 56, 56, (124, 116, 104))) and not np.array_equal(x[b], y[b])


# ------------------------------------------------------------------------------------ 4. what the kernel must survive, and refuse
def test_coefficients_and_sizes_the_host_would_refuse_take_the_fill_without_a_fault(aug):
    """the host wrapper refuses these; handed to the entry directly (wrong, but every array in bounds) a NaN or infinite coordinate is
    the fill, a denominator of the wrong sign samples or fills as the arithmetic says, and an image without pixels is all fill: the
    coordinates become indices only after the inside test.  What is proved is the fill, on arguments that stay in bounds by design:
    every pointer covers what its sizes say (the images without pixels have their heights / widths lowered, never raised), so no
    read or write can leave its buffer whatever the kernel does with the numbers.  Keep it so: no variant of this test may hand the
    entry sizes or offsets beyond its buffers."""
    from dinov2_od_amd import preprocess as pre
    img = ac._rand((20, 30), 710)
    coeffs = np.array([[np.nan] * 8, [np.inf, 0, 0, 0, 1, 0, 0, 0], [1e300, 1e300, -1e300, 1, 1, 1, 0, 0], [1, 0, 0, 0, 1, 0, -1, 0],
                       [1, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, 0, -2.0, 0], [1, 0, 0, 0, 1, 0, 1e308, 1e308]], dtype=np.float64)
    B = len(coeffs)
    src, src_offs, hs, ws = pre._stage([img] * B, torch.device("cuda"))
    hs, ws = hs.copy(), ws.copy()
    hs[4], ws[5] = 0, -3                                    # no pixels
    fill = np.array([[b, 100 + b, 200 + b] for b in range(B)], dtype=np.uint8)
    with np.errstate(all="ignore"):
        want = np.stack([wc.restated_warp(img, coeffs[b], 24, 40, fill[b]) for b in range(B)])
    assert all((want[b] == fill[b]).all() for b in (0, 1, 6))
    want[4], want[5] = fill[4], fill[5]                     # the images without pixels
    got = aug._launch_warp(src, src_offs, hs, ws, coeffs, fill, True, 24, 40, True).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[3] != fill[3]).any() and (got[3] == fill[3]).all(-1).any()
    got = aug._launch_warp(src, src_offs, hs, ws, coeffs, fill, True, 24, 40, False).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), _f32_of(want).view(np.uint32))


def test_the_entries_refuse_invalid_arguments_without_launching(aug):
    from dinov2_od_amd import _native as nat
    z = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    L, p, o = nat.lib(), nat.ptr(z), nat.ptr(out)
    for fn in (L.dod_preprocess_warp, L.dod_preprocess_warp_u8):
        def call(B=1, out_h=4, out_w=4, null=None):
            a = [p, p, p, p, B, p, p, 0, out_h, out_w, o, nat.stream_ptr()]
            if null is not None:
                a[null] = None
            return fn(*a)
        for i in (0, 1, 2, 3, 5, 6, 10):                    # src, src_offs, heights, widths, coeffs, fills, out
            assert call(null=i) == 1, i
        assert call(B=0) == 1 and call(B=-1) == 1 and call(B=65536) == 1
        assert call(out_h=0) == 1 and call(out_w=0) == 1 and call(out_h=-4) == 1 and call(out_w=-1) == 1
        assert call(out_h=524281) == 1
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
