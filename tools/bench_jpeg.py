#!/usr/bin/env python3
"""JPEG decode (dinov2_od_amd/jpeg.py decode_jpeg_batch) against Pillow on the host: 64 COCO-sized images (480 x 640, quality 90,
4:2:0), encoded once with restart_marker_rows=1 and once without.  Per batch of 64, median and range over the rounds, the variants
alternating round by round in one process:

  (a) device entropy: decode_jpeg_batch(entropy="device") on the files with restart markers -- parse, one DMA, three launches
  (b) host entropy:   decode_jpeg_batch(entropy="host") on the files without, on 1 thread and on 16
  (c) Pillow:         Image.open(f).convert("RGB") + np.asarray + preprocess._stage, on one core and over 16 worker processes
                      (the workers return the arrays to the parent, as DataLoader workers do)
  (d) the kernels alone (device events around 5 launches): entropy, IDCT, upsample + colour, with the GB/s of the bytes each must move

Every time is a host clock around work that ends in a device synchronise, except (d).  Needs a GPU; prints a table and one JSON line.
"""
import io
import json
import multiprocessing as mp
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

B, H, W = 64, 480, 640


def _pillow_one(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _files():
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = {"restart": [], "plain": []}
    for i in range(B):
        # smooth structure plus noise: about the bytes per pixel of a photograph at quality 90
        base = np.stack([127 + 100 * np.sin(x / (20 + i) + i), 127 + 100 * np.cos(y / (15 + i)), 255 * (x + y) / (W + H)], axis=2)
        pic = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        for name, kw in (("restart", {"restart_marker_rows": 1}), ("plain", {})):
            buf = io.BytesIO()
            Image.fromarray(pic).save(buf, "JPEG", quality=90, subsampling=2, **kw)
            out[name].append(buf.getvalue())
    return out


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    files = _files()
    pool = mp.get_context("spawn").Pool(16)                  # before the GPU is initialised: the workers never see it
    pool.map(_pillow_one, files["plain"][:16])
    import torch
    from dinov2_od_amd import _native as nat, jpeg, preprocess as pre
    assert torch.cuda.is_available(), "bench_jpeg.py measures on the GPU"
    dev = torch.device("cuda")
    want = [_pillow_one(f) for f in files["plain"]]

    def device_entropy():
        return jpeg.decode_jpeg_batch(files["restart"], entropy="device")

    def host_entropy(threads):
        return lambda: jpeg.decode_jpeg_batch(files["plain"], entropy="host", threads=threads)

    def pillow_1():
        return pre._stage([_pillow_one(f) for f in files["plain"]], dev)

    def pillow_16():
        return pre._stage(pool.map(_pillow_one, files["plain"], chunksize=4), dev)

    variants = {"a_device_entropy": device_entropy, "b_host_entropy_1": host_entropy(1), "b_host_entropy_16": host_entropy(16),
                "c_pillow_1": pillow_1, "c_pillow_16": pillow_16}
    # results first: every variant gives Pillow's pixels
    for name in ("a_device_entropy", "b_host_entropy_16"):
        got = variants[name]().check()
        assert all(np.array_equal(i.cpu().numpy(), w) for i, w in zip(got.images(), want)), name      # (restart markers change no pixel)
    times = {k: [] for k in variants}
    for k, fn in variants.items():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: _stats(v) for k, v in times.items()}
    # the host entropy stage by itself (no parse, no copies): what the threads do
    infos = [jpeg.parse_jpeg(f) for f in files["plain"]]
    offs = np.concatenate([[0], np.cumsum([len(f) for f in files["plain"]])[:-1]]).astype(np.int64)
    t = jpeg.build_tables(infos, ["host"] * B, offs, np.zeros(B, np.int64))
    allbytes = np.frombuffer(b"".join(files["plain"]), np.uint8)
    coef_np = np.zeros(t["n_blocks"] * 64, np.int16)
    for th in (1, 16):
        ms = []
        for _ in range(rounds):
            st = np.zeros(B, np.int32)
            t0 = time.perf_counter()
            jpeg.entropy_host(allbytes, t["images"], t["htabs"], coef_np, st, th)
            ms.append((time.perf_counter() - t0) * 1e3)
        res[f"b_entropy_stage_only_{th}"] = _stats(ms)
    t0 = time.perf_counter()
    for f in files["plain"]:
        jpeg.parse_jpeg(f)
    res["parse_64_files_ms"] = (time.perf_counter() - t0) * 1e3
    # (d) the kernels alone, on the restart-marker files
    infos = [jpeg.parse_jpeg(f) for f in files["restart"]]
    offs = np.concatenate([[0], np.cumsum([len(f) for f in files["restart"]])[:-1]]).astype(np.int64)
    src_offs = np.arange(B, dtype=np.int64) * H * W * 3
    t = jpeg.build_tables(infos, ["device"] * B, offs, src_offs)
    d = {k: torch.from_numpy(t[k].view(np.int16) if t[k].dtype == np.uint16 else t[k]).to(dev) for k in ("images", "intervals", "htabs", "qtabs", "comps")}
    d_bytes = torch.from_numpy(np.frombuffer(b"".join(files["restart"]), np.uint8).copy()).to(dev)
    coef = torch.zeros(t["n_blocks"] * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(t["plane_bytes"], dtype=torch.uint8, device=dev)
    out = torch.empty(B * H * W * 3, dtype=torch.uint8, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    L = nat.lib()
    kernels = {
        "entropy": lambda: nat.check(L.dod_jpeg_entropy_device(nat.ptr(d_bytes), d_bytes.numel(), nat.ptr(d["images"]), B, nat.ptr(d["intervals"]), len(t["intervals"]),
                                                               nat.ptr(d["htabs"]), len(t["htabs"]), nat.ptr(coef), t["n_blocks"], nat.ptr(status), nat.stream_ptr())),
        "idct": lambda: nat.check(L.dod_jpeg_idct(nat.ptr(coef), t["n_blocks"], nat.ptr(d["comps"]), len(t["comps"]), nat.ptr(d["qtabs"]), len(t["qtabs"]),
                                                  nat.ptr(planes), nat.stream_ptr())),
        "color": lambda: nat.check(L.dod_jpeg_color(nat.ptr(planes), nat.ptr(d["images"]), B, t["n_items"], nat.ptr(out), nat.stream_ptr())),
    }
    moved = {"entropy": d_bytes.numel() + t["n_blocks"] * 128, "idct": t["n_blocks"] * (128 + 64), "color": B * H * W * (1 + 2 / 4 + 3)}
    for fn in kernels.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    assert int(status.sum()) == 0 and all(np.array_equal(out[o:o + H * W * 3].view(H, W, 3).cpu().numpy(), _pillow_one(f)) for o, f in zip(src_offs[:4], files["restart"]))
    kt = {k: [] for k in kernels}
    for _ in range(rounds):
        for k, fn in kernels.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                fn()
            b.record()
            torch.cuda.synchronize()
            kt[k].append(a.elapsed_time(b) / 5)
    for k, v in kt.items():
        res["d_kernel_" + k] = dict(_stats(v), bytes=int(moved[k]), gb_per_s=float(moved[k] / (np.median(v) * 1e-3) / 1e9))
    pool.close()
    pool.join()
    res["file_bytes"] = {k: int(sum(len(f) for f in v)) for k, v in files.items()}
    res["host_threads"] = jpeg.host_threads()
    print(f"{B} images {H} x {W}, quality 90, 4:2:0; file bytes {res['file_bytes']}; {rounds} rounds; host threads {res['host_threads']}")
    for k, v in res.items():
        if isinstance(v, dict) and "median_ms" in v:
            extra = f"   {v['gb_per_s']:.0f} GB/s of {v['bytes']} bytes" if "gb_per_s" in v else f"   {B / v['median_ms'] * 1e3:.0f} images/s"
            print(f"  {k:28s} median {v['median_ms']:9.3f} ms   range {v['min_ms']:9.3f} .. {v['max_ms']:9.3f}{extra}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
