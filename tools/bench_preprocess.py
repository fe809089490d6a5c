#!/usr/bin/env python3
"""Device input pipeline (dod_preprocess) vs Pillow on the host: 64 COCO-sized images (480x640) -> 224^2 and 518^2.
--augment: on the same images, the plain call against the augmented one (dod_preprocess_aug) with a crop + flip, with a crop +
flip + all three jitters, and the same chain in Pillow on one host core; the device calls are timed interleaved in one process.
--mosaic: 64 composed canvases from the same images (dod_preprocess_compose): mosaics of four with and without jitter, zoom-out,
against dod_preprocess_aug writing as many output bytes and Pillow's paste chain on one host core; interleaved likewise.
--warp: the geometric warp (dod_preprocess_warp) on 64 resident images: alone (rotation, perspective; uint8 and fp32 out, with its
achieved GB/s) next to the geometric-only dod_preprocess_aug, behind the chain and behind a mosaic, `TrainAugment` end to end with and
without affine_prob = 1, and the same chains with Image.transform in Pillow on one host core."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from PIL import Image, ImageEnhance
from dinov2_od_amd import _native as nat, preprocess as pre

rng = np.random.default_rng(0)
imgs = [rng.integers(0, 256, size=(480, 640, 3), dtype=np.uint8) for _ in range(64)]


def timed(runs, rounds=20):
    """median and min microseconds of each callable, the callables alternating round by round"""
    for r in runs:
        for _ in range(3): r()
    torch.cuda.synchronize()
    t = [[] for _ in runs]
    for _ in range(rounds):
        for i, r in enumerate(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5): r()
            b.record(); torch.cuda.synchronize()
            t[i].append(a.elapsed_time(b) / 5 * 1e3)
    return [(float(np.median(x)), float(np.min(x))) for x in t]


def augment_leg(R):
    from dinov2_od_amd import augment as aug
    L = nat.lib(); B = len(imgs)
    crops, flips, jitter = aug.sample_params([(480, 640)] * B, torch.Generator().manual_seed(0), crop_prob=1.0, crop_frac=(0.5, 1.0), hflip_prob=0.5,
                                             brightness=0.4, contrast=0.4, saturation=0.4)
    full = np.array([(0, 0, 640, 480)] * B, np.int32)
    hs = np.full(B, 480, np.int32); ws = np.full(B, 640, np.int32)
    so = (np.arange(B, dtype=np.int64) * 480 * 640 * 3)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).cuda()
    out = torch.empty(B, 3, R, R, device="cuda")
    lsum = torch.empty(B, dtype=torch.int64, device="cuda")

    def setup(c, jittered):
        to, nbytes = pre._tmp_layout(c[:, 3], R, c[:, 2] if jittered else None)
        return [torch.from_numpy(x).cuda() for x in (so, hs, ws, to, c)], torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mp, tp = setup(full, False)
    mc, tc = setup(crops, False)
    mpj, tpj = setup(full, True)
    mcj, tcj = setup(crops, True)
    fl, no_fl, jit = torch.from_numpy(flips).cuda(), torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.from_numpy(jitter).cuda()

    def call(m, tmp, f, j, ls, c):
        return lambda: nat.check(L.dod_preprocess_aug(nat.ptr(src), nat.ptr(m[0]), nat.ptr(m[1]), nat.ptr(m[2]), B, nat.ptr(m[4]), nat.ptr(f), nat.ptr(j), nat.ptr(ls),
                                                      int(c[:, 3].max()), int(c[:, 2].max()), R, R, nat.ptr(tmp), nat.ptr(m[3]), nat.ptr(out), nat.stream_ptr()))
    plain = lambda: nat.check(L.dod_preprocess(nat.ptr(src), nat.ptr(mp[0]), nat.ptr(mp[1]), nat.ptr(mp[2]), B, 480, 640, R, R, nat.ptr(tp), nat.ptr(mp[3]), nat.ptr(out), nat.stream_ptr()))
    names = ["dod_preprocess", "aug, full image, no flip, no jitter", "aug, crop + flip", "aug, crop + flip + 3 jitters", "aug, full image + 3 jitters"]
    res = timed([plain, call(mp, tp, no_fl, None, None, full), call(mc, tc, fl, None, None, crops), call(mcj, tcj, fl, jit, lsum, crops), call(mpj, tpj, no_fl, jit, lsum, full)])
    t0 = time.perf_counter()
    for im, (l, t, w, h), f, fs in zip(imgs, crops.tolist(), flips.tolist(), jitter.tolist()):
        p = Image.fromarray(im).crop((l, t, l + w, t + h))
        for enh, x in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), fs):
            p = enh(p).enhance(x)
        p = p.resize((R, R), Image.BILINEAR)
        if f:
            p = p.transpose(Image.FLIP_LEFT_RIGHT)
        np.transpose(np.array(p), (2, 0, 1)).astype(np.float32) / 255
    t_cpu = time.perf_counter() - t0
    frac = float((crops[:, 2].astype(np.int64) * crops[:, 3]).sum()) / (B * 480 * 640)
    print(f"augment, 64 x 480x640 -> {R}^2 (crops cover {frac:.2f} of the pixels), median / min us over 20 interleaved rounds:")
    for n, (med, mn) in zip(names, res):
        print(f"  {n:40s} {med:7.1f} / {mn:7.1f}")
    print(f"  {'Pillow, crop + flip + 3 jitters, one core':40s} {t_cpu*1e3:7.0f} ms")


def mosaic_leg(R):
    """64 composed canvases from the 64 sources (dod_preprocess_compose): mosaic without jitter, mosaic with all three jitters, zoom-out;
    against dod_preprocess_aug writing the same number of output bytes (64 images, crop + flip, without and with jitter) and
    dod_preprocess on the full images; and the Pillow paste chain of the jittered mosaic on one host core"""
    from dinov2_od_amd import augment as aug
    L = nat.lib(); B = len(imgs)
    shapes = [(480, 640)] * B
    kw = dict(crop_prob=1.0, crop_frac=(0.5, 1.0), hflip_prob=0.5)
    jkw = dict(brightness=0.4, contrast=0.4, saturation=0.4)
    hs = np.full(B, 480, np.int32); ws = np.full(B, 640, np.int32)
    so = (np.arange(B, dtype=np.int64) * 480 * 640 * 3)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).cuda()
    out = torch.empty(B, 3, R, R, device="cuda")
    fill = torch.tensor([124, 116, 104], dtype=torch.uint8, device="cuda")
    base = [torch.from_numpy(x).cuda() for x in (so, hs, ws)]
    keep = []

    def compose(plan):
        rows, offs, jitter = aug._check_pieces(shapes, plan, R, R)
        if jitter is not None and (jitter == 1.0).all():
            jitter = None
        cw, ch, dw = (rows[:, k].astype(np.int64) for k in (3, 4, 8))
        to, nbytes = pre._tmp_layout(ch, dw, cw if jitter is not None else None)
        d = [torch.from_numpy(x).cuda() for x in (rows, offs, to)] + [torch.from_numpy(jitter).cuda() if jitter is not None else None,
                                                                      torch.empty(len(rows), dtype=torch.int64, device="cuda") if jitter is not None else None,
                                                                      torch.empty(nbytes, dtype=torch.uint8, device="cuda")]
        keep.append(d)
        frac = float((cw * ch).sum()) / (B * 480 * 640)
        return frac, lambda: nat.check(L.dod_preprocess_compose(nat.ptr(src), nat.ptr(base[0]), nat.ptr(base[1]), nat.ptr(base[2]), B, nat.ptr(d[0]), nat.ptr(d[1]),
                                                                B, len(rows), nat.ptr(d[3]), nat.ptr(d[4]), nat.ptr(fill), 0, int(ch.max()), int(cw.max()), int(dw.max()),
                                                                R, R, nat.ptr(d[5]), nat.ptr(d[2]), nat.ptr(out), nat.stream_ptr()))

    def single(c, f, j):
        to, nbytes = pre._tmp_layout(c[:, 3], R, c[:, 2] if j is not None else None)
        d = [torch.from_numpy(x).cuda() for x in (to, c, f)] + [torch.from_numpy(j).cuda() if j is not None else None,
                                                                torch.empty(B, dtype=torch.int64, device="cuda") if j is not None else None,
                                                                torch.empty(nbytes, dtype=torch.uint8, device="cuda")]
        keep.append(d)
        frac = float((c[:, 2].astype(np.int64) * c[:, 3]).sum()) / (B * 480 * 640)
        return frac, lambda: nat.check(L.dod_preprocess_aug(nat.ptr(src), nat.ptr(base[0]), nat.ptr(base[1]), nat.ptr(base[2]), B, nat.ptr(d[1]), nat.ptr(d[2]), nat.ptr(d[3]),
                                                            nat.ptr(d[4]), int(c[:, 3].max()), int(c[:, 2].max()), R, R, nat.ptr(d[5]), nat.ptr(d[0]), nat.ptr(out), nat.stream_ptr()))
    gen = lambda: torch.Generator().manual_seed(0)
    plan_j = aug.sample_mosaic(shapes, gen(), (R, R), **kw, **jkw)
    crops, flips, jitter = aug.sample_params(shapes, gen(), **kw, **jkw)
    full = np.array([(0, 0, 640, 480)] * B, np.int32)
    legs = [("aug, full image, no flip, no jitter", single(full, np.zeros(B, np.uint8), None)),
            ("aug, crop + flip", single(crops, flips, None)),
            ("aug, crop + flip + 3 jitters", single(crops, flips, jitter)),
            ("mosaic of 4, crop + flip", compose(aug.sample_mosaic(shapes, gen(), (R, R), **kw))),
            ("mosaic of 4, crop + flip + 3 jitters", compose(plan_j)),
            ("mosaic of 4 quarter-image crops + flip", compose(aug.sample_mosaic(shapes, gen(), (R, R), crop_prob=1.0, crop_frac=(0.5, 0.5), hflip_prob=0.5))),
            ("mosaic of 4 full images, no flip", compose(aug.sample_mosaic(shapes, gen(), (R, R), crop_prob=0.0, hflip_prob=0.0))),
            ("zoom-out 1..2, crop + flip", compose(aug.sample_zoom_out(shapes, gen(), (R, R), (1.0, 2.0), **kw))),
            ("one full-canvas piece per canvas, crop + flip", compose([[(n, tuple(int(v) for v in crops[n]), bool(flips[n]), None, (0, 0, R, R))] for n in range(B)]))]
    res = timed([run for _, (_, run) in legs])
    t0 = time.perf_counter()
    for canvas in plan_j:
        cv = Image.new("RGB", (R, R), (124, 116, 104))
        for s, (l, t, w, h), f, fs, (dx, dy, dw, dh) in canvas:
            p = Image.fromarray(imgs[s]).crop((l, t, l + w, t + h))
            for enh, x in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), fs):
                p = enh(p).enhance(x)
            p = p.resize((dw, dh), Image.BILINEAR)
            cv.paste(p.transpose(Image.FLIP_LEFT_RIGHT) if f else p, (dx, dy))
        np.transpose(np.array(cv), (2, 0, 1)).astype(np.float32) / 255
    t_cpu = time.perf_counter() - t0
    print(f"mosaic, 64 canvases from 64 x 480x640 -> {R}^2, median / min us over 20 interleaved rounds (source pixels read, in full images' worth of the 64):")
    for (n, (frac, _)), (med, mn) in zip(legs, res):
        print(f"  {n:48s} {med:7.1f} / {mn:7.1f}   ({frac:.2f})")
    print(f"  {'Pillow paste chain, mosaic + 3 jitters, one core':48s} {t_cpu*1e3:7.0f} ms")


def warp_leg(R):
    """the geometric warp (dod_preprocess_warp) on 64 resident uint8 images of R x R -- what the chain or the canvas hands it: a 15 degree
    rotation and a perspective, to uint8 and to fp32, with the GB/s of B R R (3 read-equivalent + 3 or 12 written) bytes, next to the
    geometric-only dod_preprocess_aug (crop + flip) at the same output; then the kernels of the pipelines with the warp as their last
    stage (chain -> uint8 -> warp -> fp32, mosaic -> uint8 -> warp -> fp32) against the same without it; `TrainAugment` end to end
    (sampling, staging and H2D of the raw bytes included) with and without affine_prob = 1; and the Pillow chains on one host core"""
    from dinov2_od_amd import augment as aug
    L = nat.lib(); B = len(imgs)
    shapes = [(480, 640)] * B
    kw = dict(crop_prob=1.0, crop_frac=(0.5, 1.0), hflip_prob=0.5)
    jkw = dict(brightness=0.4, contrast=0.4, saturation=0.4)
    akw = dict(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=5.0)
    gen = lambda: torch.Generator().manual_seed(0)
    hs = np.full(B, 480, np.int32); ws = np.full(B, 640, np.int32)
    so = (np.arange(B, dtype=np.int64) * 480 * 640 * 3)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).cuda()
    base = [torch.from_numpy(x).cuda() for x in (so, hs, ws)]
    fill = torch.tensor([124, 116, 104], dtype=torch.uint8, device="cuda")
    out_f, out_f2 = torch.empty(B, 3, R, R, device="cuda"), torch.empty(B, 3, R, R, device="cuda")
    out_u, mid_u = torch.empty(B, R, R, 3, dtype=torch.uint8, device="cuda"), torch.empty(B, R, R, 3, dtype=torch.uint8, device="cuda")
    keep = []
    # the warp's own source: a resized batch, as the chain leaves it
    mid, _ = aug.augment_batch(imgs, None, np.array([(0, 0, 640, 480)] * B, np.int32), np.zeros(B, np.uint8), None, (R, R), as_uint8=True)
    wmeta = [torch.from_numpy(x).cuda() for x in (np.arange(B, dtype=np.int64) * R * R * 3, np.full(B, R, np.int32), np.full(B, R, np.int32))]

    def warp(coeffs, source, dst):
        c = torch.from_numpy(np.ascontiguousarray(coeffs)).cuda()
        keep.append(c)
        fn = L.dod_preprocess_warp_u8 if dst.dtype == torch.uint8 else L.dod_preprocess_warp
        return lambda: nat.check(fn(nat.ptr(source), nat.ptr(wmeta[0]), nat.ptr(wmeta[1]), nat.ptr(wmeta[2]), B, nat.ptr(c), nat.ptr(fill), 0, R, R,
                                    nat.ptr(dst), nat.stream_ptr()))

    def chain(c, f, j, dst):
        to, nbytes = pre._tmp_layout(c[:, 3], R, c[:, 2] if j is not None else None)
        d = [torch.from_numpy(x).cuda() for x in (to, c, f)] + [torch.from_numpy(j).cuda() if j is not None else None,
                                                                torch.empty(B, dtype=torch.int64, device="cuda") if j is not None else None,
                                                                torch.empty(nbytes, dtype=torch.uint8, device="cuda")]
        keep.append(d)
        fn = L.dod_preprocess_aug_u8 if dst.dtype == torch.uint8 else L.dod_preprocess_aug
        return lambda: nat.check(fn(nat.ptr(src), nat.ptr(base[0]), nat.ptr(base[1]), nat.ptr(base[2]), B, nat.ptr(d[1]), nat.ptr(d[2]), nat.ptr(d[3]), nat.ptr(d[4]),
                                    int(c[:, 3].max()), int(c[:, 2].max()), R, R, nat.ptr(d[5]), nat.ptr(d[0]), nat.ptr(dst), nat.stream_ptr()))

    def compose(plan, dst):
        rows, offs, jitter = aug._check_pieces(shapes, plan, R, R)
        cw, ch, dw = (rows[:, k].astype(np.int64) for k in (3, 4, 8))
        to, nbytes = pre._tmp_layout(ch, dw, cw if jitter is not None else None)
        d = [torch.from_numpy(x).cuda() for x in (rows, offs, to)] + [torch.from_numpy(jitter).cuda() if jitter is not None else None,
                                                                      torch.empty(len(rows), dtype=torch.int64, device="cuda") if jitter is not None else None,
                                                                      torch.empty(nbytes, dtype=torch.uint8, device="cuda")]
        keep.append(d)
        fn = L.dod_preprocess_compose_u8 if dst.dtype == torch.uint8 else L.dod_preprocess_compose
        return lambda: nat.check(fn(nat.ptr(src), nat.ptr(base[0]), nat.ptr(base[1]), nat.ptr(base[2]), B, nat.ptr(d[0]), nat.ptr(d[1]), B, len(rows), nat.ptr(d[3]),
                                    nat.ptr(d[4]), nat.ptr(fill), 0, int(ch.max()), int(cw.max()), int(dw.max()), R, R, nat.ptr(d[5]), nat.ptr(d[2]), nat.ptr(dst),
                                    nat.stream_ptr()))

    def both(first, second):
        def run():
            first(); second()
        return run
    rot = np.stack([aug.affine_coeffs((R, R), (R, R), 15.0)] * B)
    q = 0.15 * R
    per = np.stack([aug.perspective_coeffs([(0, 0), (R, 0), (R, R), (0, R)], [(q, 0.5 * q), (R - 0.3 * q, q), (R - q, R - 0.2 * q), (0.4 * q, R - q)])] * B)
    drawn = aug.sample_affine([(R, R)] * B, gen(), **akw)
    crops, flips, jitter = aug.sample_params(shapes, gen(), **kw, **jkw)
    plan = aug.sample_mosaic(shapes, gen(), (R, R), **kw, **jkw)
    px = B * R * R
    legs = [("warp alone, rotation 15 deg -> uint8", warp(rot, mid, out_u), px * 6),
            ("warp alone, rotation 15 deg -> fp32", warp(rot, mid, out_f), px * 15),
            ("warp alone, perspective -> uint8", warp(per, mid, out_u), px * 6),
            ("warp alone, perspective -> fp32", warp(per, mid, out_f), px * 15),
            ("warp alone, identity -> fp32", warp(np.array([aug.IDENTITY_COEFFS] * B), mid, out_f), px * 15),
            ("aug, crop + flip (geometric only) -> fp32", chain(crops, flips, None, out_f2), px * 15),
            ("chain: crop + flip + 3 jitters -> fp32", chain(crops, flips, jitter, out_f2), 0),
            ("chain -> uint8, random affine -> fp32", both(chain(crops, flips, jitter, mid_u), warp(drawn, mid_u, out_f)), 0),
            ("mosaic of 4 + 3 jitters -> fp32", compose(plan, out_f2), 0),
            ("mosaic -> uint8, random affine -> fp32", both(compose(plan, mid_u), warp(drawn, mid_u, out_f)), 0)]
    for r in [run for _, run, _ in legs]:
        for _ in range(3): r()
    torch.cuda.synchronize()
    t = [[] for _ in legs]
    for _ in range(20):
        for i, (_, r, _) in enumerate(legs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5): r()
            b.record(); torch.cuda.synchronize()
            t[i].append(a.elapsed_time(b) / 5 * 1e3)
    print(f"warp, 64 images -> {R}^2, median (min .. max) us over 20 interleaved rounds of 5 calls:")
    for (n, _, nbytes), x in zip(legs, t):
        med = float(np.median(x))
        rate = f"   {nbytes / med / 1e3:6.0f} GB/s of {nbytes / 1e6:.0f} MB (3 B read-equivalent + the bytes written per output pixel)" if nbytes else ""
        print(f"  {n:44s} {med:7.1f} ({min(x):7.1f} .. {max(x):7.1f}){rate}")

    def e2e(**extra):
        ta = aug.TrainAugment((R, R), generator=gen(), **kw, **jkw, **extra)
        x = []
        for _ in range(7):
            torch.cuda.synchronize(); t0 = time.perf_counter(); ta(imgs); torch.cuda.synchronize(); x.append((time.perf_counter() - t0) * 1e3)
        return f"{float(np.median(x[2:])):6.1f} ({min(x[2:]):6.1f} .. {max(x[2:]):6.1f}) ms"
    print("  TrainAugment end to end from host arrays (sampling, staging, H2D of 59 MB, kernels), median (min .. max) of 5 calls:")
    print(f"    {'chain':42s} {e2e()}")
    print(f"    {'chain, affine_prob = 1':42s} {e2e(affine_prob=1.0, **akw)}")
    print(f"    {'mosaic_prob = 1':42s} {e2e(mosaic_prob=1.0)}")
    print(f"    {'mosaic_prob = 1, affine_prob = 1':42s} {e2e(mosaic_prob=1.0, affine_prob=1.0, **akw)}")

    def pil_chain(im, crop, f, fs, size):
        l, t, w, h = crop
        p = Image.fromarray(im).crop((l, t, l + w, t + h))
        for enh, x in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), fs):
            p = enh(p).enhance(x)
        p = p.resize(size, Image.BILINEAR)
        return p.transpose(Image.FLIP_LEFT_RIGHT) if f else p

    def pil_warp(p, c):
        p = p.transform((R, R), Image.PERSPECTIVE, [float(v) for v in c], Image.BILINEAR, fillcolor=(124, 116, 104))
        return np.transpose(np.array(p), (2, 0, 1)).astype(np.float32) / 255
    t0 = time.perf_counter()
    for b in range(B):
        pil_warp(Image.fromarray(imgs[b][:R, :R] if R <= 480 else np.resize(imgs[b], (R, R, 3))), rot[b])
    t_warp = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b in range(B):
        pil_warp(pil_chain(imgs[b], crops[b].tolist(), flips[b], jitter[b].tolist(), (R, R)), drawn[b])
    t_chain = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b, canvas in enumerate(plan):
        cv = Image.new("RGB", (R, R), (124, 116, 104))
        for s, crop, f, fs, (dx, dy, dw, dh) in canvas:
            cv.paste(pil_chain(imgs[s], crop, f, fs, (dw, dh)), (dx, dy))
        pil_warp(cv, drawn[b])
    t_mosaic = time.perf_counter() - t0
    print(f"  Pillow on one host core: transform alone (rotation) {t_warp*1e3:.0f} ms, chain + 3 jitters + transform {t_chain*1e3:.0f} ms, "
          f"mosaic + 3 jitters + transform {t_mosaic*1e3:.0f} ms")


if "--warp" in sys.argv:
    for R in (224, 518):
        warp_leg(R)
    sys.exit(0)

if "--mosaic" in sys.argv:
    for R in (224, 518):
        mosaic_leg(R)
    sys.exit(0)

if "--augment" in sys.argv:
    for R in (224, 518):
        augment_leg(R)
    sys.exit(0)

for R in (224, 518):
    L = nat.lib(); B = len(imgs)
    hs = np.array([a.shape[0] for a in imgs], np.int32); ws = np.array([a.shape[1] for a in imgs], np.int32)
    so = np.concatenate([[0], np.cumsum(hs.astype(np.int64) * ws * 3)[:-1]]).astype(np.int64)
    to, nbytes = pre._tmp_layout(hs, R)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).cuda()
    m = [torch.from_numpy(x).cuda() for x in (so, hs, ws, to)]
    tmp = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, 3, R, R, device="cuda")
    run = lambda: nat.check(L.dod_preprocess(nat.ptr(src), nat.ptr(m[0]), nat.ptr(m[1]), nat.ptr(m[2]), B, 480, 640, R, R, nat.ptr(tmp), nat.ptr(m[3]), nat.ptr(out), nat.stream_ptr()))
    for _ in range(3): run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20): run()
    b.record(); torch.cuda.synchronize()
    t_k = a.elapsed_time(b) / 20 * 1e-3
    t0 = time.perf_counter(); o = pre.preprocess_batch(imgs, (R, R)); torch.cuda.synchronize(); t_e2e = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = [np.transpose(np.array(Image.fromarray(im, "RGB").resize((R, R), Image.BILINEAR)), (2, 0, 1)).astype(np.float32) / 255 for im in imgs]
    t_cpu = time.perf_counter() - t0
    alg = src.numel() + tmp.numel() * 2 + out.numel() * 4
    print(f"64 x 480x640 -> {R}^2: kernels {t_k*1e6:.0f} us ({alg/t_k/1e9:.0f} GB/s of {alg/1e6:.0f} MB algorithmic: source + temp write/read + fp32 out), "
          f"incl. H2D of the raw bytes {t_e2e*1e3:.1f} ms, Pillow on one host core {t_cpu*1e3:.0f} ms")
