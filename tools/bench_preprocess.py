#!/usr/bin/env python3
"""Device input pipeline (dod_preprocess) vs Pillow on the host: 64 COCO-sized images (480x640) -> 224^2 and 518^2.
--augment: on the same images, the plain call against the augmented one (dod_preprocess_aug) with a crop + flip, with a crop +
flip + all three jitters, and the same chain in Pillow on one host core; the device calls are timed interleaved in one process."""
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
        # tmp per image: crop height x out_w x 3, and with jitter the jittered crop behind it (include/dinodet.h)
        sz = c[:, 3].astype(np.int64) * (R + (c[:, 2].astype(np.int64) if jittered else 0)) * 3
        to = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.int64)
        return [torch.from_numpy(x).cuda() for x in (so, hs, ws, to, c)], torch.empty(int(sz.sum()), dtype=torch.uint8, device="cuda")
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


if "--augment" in sys.argv:
    for R in (224, 518):
        augment_leg(R)
    sys.exit(0)

for R in (224, 518):
    L = nat.lib(); B = len(imgs)
    hs = np.array([a.shape[0] for a in imgs], np.int32); ws = np.array([a.shape[1] for a in imgs], np.int32)
    so = np.concatenate([[0], np.cumsum(hs.astype(np.int64) * ws * 3)[:-1]]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(hs.astype(np.int64) * R * 3)[:-1]]).astype(np.int64)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).cuda()
    m = [torch.from_numpy(x).cuda() for x in (so, hs, ws, to)]
    tmp = torch.empty(int((hs.astype(np.int64) * R * 3).sum()), dtype=torch.uint8, device="cuda")
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
