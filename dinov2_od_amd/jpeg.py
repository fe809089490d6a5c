"""Baseline JPEG decode on the GPU: the host side of `dod_jpeg_*` (include/dinodet.h).

The reference opens every image on the host with `Image.open(path).convert("RGB")` inside the DataLoader workers (dino_detector/
train.py: the dataset's __getitem__).  `decode_jpeg_batch` takes the FILES as bytes and returns the packed uint8 RGB source buffer
`preprocess._stage` produces -- `src` on the device, `src_offs`, heights, widths -- bit for bit what Pillow (libjpeg-turbo, JDCT_ISLOW,
fancy upsampling) decodes, so `preprocess_batch`, `augment_batch`, `compose_batch`, `warp_batch`, `extract_views`, `TrainAugment` and
`detect_sliced` read it where it is and the pixels never exist on the host.

    header parse      here, per file: markers, DQT, DHT, SOF, DRI, SOS, the scan's byte range; with DRI the byte range of every restart
                      interval from one vectorised search for FF D0..D7
    entropy decode    csrc/jpeg_entropy.h, one function with two callers: the device kernel, one thread per restart interval (files
                      with DRI), or the host entry on up to 16 threads into pinned memory (files without)
    dequantise+IDCT   csrc/jpeg.hip
    upsample+colour   csrc/jpeg.hip

A stream the device path does not take (progressive, arithmetic, 12-bit, CMYK, other sampling factors, ...) is decoded by Pillow
into its slot of the same buffer (fallback=True) or raises `UnsupportedJpeg`.  No CPU fallback for the pipeline itself: without the
HIP library this module raises.
"""
import ctypes as C
import io
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _native as nat
from . import preprocess as _pre

# csrc/jpeg_entropy.h: DOD_JI_* (int64 per image), DOD_JV_* (int64 per interval), DOD_JH_* (int32 per Huffman table), flags
JI_WIDTH, JI_HEIGHT, JI_NCOMP, JI_HS, JI_VS, JI_MCUS_X, JI_MCUS_Y, JI_RESTART, JI_SCAN_BEGIN, JI_SCAN_END = range(10)
JI_BLOCK0, JI_BLOCKS_W, JI_PLANE, JI_OUT, JI_QT, JI_DC, JI_AC, JI_ITEM0, JI_STRIDE = 10, 13, 16, 19, 20, 23, 26, 29, 32
JV_STRIDE = 5
JH_LOOK, JH_MAXCODE, JH_VALOFF, JH_VAL, JH_STRIDE = 0, 512, 529, 546, 802
FLAGS = {1: "the scan ran out of bytes", 2: "undefined Huffman code", 4: "coefficient run past the block", 8: "restart marker missing",
         16: "descriptor out of range", 32: "bytes left over behind the last MCU"}
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
MAX_HOST_THREADS = 16


class UnsupportedJpeg(ValueError):
    """a stream the device path does not take, with fallback=False: `.index` is the file's position in the batch, `.reason` says why"""

    def __init__(self, index, reason):
        super().__init__(f"file {index}: {reason}")
        self.index, self.reason = index, reason


class JpegInfo:
    """What `parse_jpeg` found: width, height, mode ("RGB" | "L" | "CMYK" | None), sampling (the luma factors (h, v), None when the
    frame was not read), restart_interval (MCUs, 0 = none), supported, reason (why not, else None)."""

    def __init__(self):
        self.width = self.height = 0
        self.mode = self.sampling = self.reason = None
        self.restart_interval = 0
        self.supported = False
        # what the batch assembly needs
        self.ncomp = 0
        self.qt = self.dc = self.ac = ()         # per component: table payloads (bytes)
        self.scan = (0, 0)                        # byte range of the entropy-coded data
        self._restarts = None                     # positions of the scan's restart markers (files with a restart interval)

    def __repr__(self):
        return (f"JpegInfo({self.width}x{self.height} {self.mode} sampling={self.sampling} restart={self.restart_interval} "
                f"{'supported' if self.supported else 'unsupported: ' + str(self.reason)})")


_SOF_REASON = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "hierarchical", 0xC6: "hierarchical progressive", 0xC7: "hierarchical lossless",
               0xC9: "arithmetic coding", 0xCA: "progressive, arithmetic coding", 0xCB: "lossless, arithmetic coding",
               0xCD: "hierarchical, arithmetic coding", 0xCE: "hierarchical, arithmetic coding", 0xCF: "hierarchical, arithmetic coding"}


def _as_bytes(f):
    if isinstance(f, (bytes, bytearray, memoryview)):
        return np.frombuffer(f, dtype=np.uint8)
    if isinstance(f, np.ndarray):
        if f.dtype != np.uint8 or f.ndim != 1:
            raise ValueError(f"expected the file's bytes as a uint8 vector, got {f.dtype} {f.shape}")
        return np.ascontiguousarray(f)
    if isinstance(f, torch.Tensor):
        return _as_bytes(f.cpu().numpy())
    if isinstance(f, (str, os.PathLike)):
        with open(f, "rb") as fh:
            return np.frombuffer(fh.read(), dtype=np.uint8)
    raise ValueError(f"expected bytes, a uint8 array or a path, got {type(f).__name__}")


def parse_jpeg(data):
    """data: a JPEG file as bytes / bytearray / uint8 array (or a path).  Reads the markers up to the one scan the device path takes
    and returns a `JpegInfo`; a stream outside that path comes back with supported = False and the reason, never an exception (a
    header that ends early is "truncated header")."""
    a = _as_bytes(data)
    info = JpegInfo()
    try:
        _parse(a, info)
    except IndexError:
        info.supported, info.reason = False, "truncated header"
    return info


def _parse(a, info):
    def no(reason):
        info.supported, info.reason = False, reason

    d = a.tobytes() if len(a) < (1 << 16) else bytes(a[:1 << 16])      # the headers: markers in front of the scan (beyond 64 KiB: below)
    if len(a) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return no("not a JPEG file (no SOI)")
    qt, ht = {}, {}
    comps = None
    adobe = None
    jfif = False
    pos = 2
    while True:
        if pos + 4 > len(d):
            if len(d) < len(a):
                d = a.tobytes()                   # a header segment (an ICC profile, a thumbnail) reaches past the first 64 KiB
                continue
            raise IndexError
        if d[pos] != 0xFF:
            return no(f"marker expected at byte {pos}")
        m = d[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if m == 0xD9:
            return no("no scan")
        length = (d[pos + 2] << 8) | d[pos + 3]
        if length < 2:
            return no(f"bad segment length at byte {pos}")
        if pos + 2 + length > len(d):
            if len(d) < len(a):
                d = a.tobytes()
                continue
            raise IndexError
        seg = d[pos + 4:pos + 2 + length]
        if m in (0xC0, 0xC1) or m in _SOF_REASON:
            if comps is not None:
                return no("two frames")
            info.height, info.width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            n = seg[5]
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(n)]
            info.ncomp = n
            info.mode = {1: "L", 3: "RGB", 4: "CMYK"}.get(n)
            info.sampling = (comps[0][1], comps[0][2]) if n else None
            if m in _SOF_REASON:
                return no(_SOF_REASON[m])
            if seg[0] != 8:
                return no(f"{seg[0]}-bit precision")
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                if seg[i] >> 4:
                    return no("16-bit quantisation table")
                qt[seg[i] & 15] = seg[i + 1:i + 65]
                if len(qt[seg[i] & 15]) != 64:
                    raise IndexError
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                n = sum(seg[i + 1:i + 17])
                if i + 17 + n > len(seg):
                    raise IndexError
                ht[(seg[i] >> 4, seg[i] & 15)] = seg[i + 1:i + 17 + n]
                i += 17 + n
        elif m == 0xDD:
            info.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            break
        pos += 2 + length
    # the scan header
    if comps is None:
        return no("scan before the frame")
    n = info.ncomp
    if n == 4:
        return no("4 components (CMYK / YCCK)")
    if n not in (1, 3):
        return no(f"{n} components")
    if info.width < 1 or info.height < 1:
        return no("empty frame (height by DNL)")
    if seg[0] != n:
        return no("multi-scan: the first scan holds %d of %d components" % (seg[0], n))
    if len(seg) < 4 + 2 * n:
        raise IndexError
    if (seg[1 + 2 * n], seg[2 + 2 * n], seg[3 + 2 * n]) != (0, 63, 0):
        return no("spectral selection / successive approximation in a sequential scan")
    if n == 3:
        if adobe == 0:
            return no("Adobe APP14 transform 0 (RGB components)")
        if adobe not in (None, 1):
            return no(f"Adobe APP14 transform {adobe}")
        if adobe is None and not jfif and tuple(c[0] for c in comps) == (82, 71, 66):
            return no("components named R, G, B without a JFIF header (RGB components)")
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return no("sampling factors " + " ".join(f"{c[1]}x{c[2]}" for c in comps))
    else:
        info.sampling = (1, 1)                   # one component: its factors mean nothing (one block per MCU)
    sel = []
    for c in range(n):
        if seg[1 + 2 * c] != comps[c][0]:
            return no("scan components out of frame order")
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if comps[c][3] not in qt or (0, td) not in ht or (1, ta) not in ht:
            return no("a table the scan names is not defined")
        sel.append((qt[comps[c][3]], ht[(0, td)], ht[(1, ta)]))
    for _, dc, ac in sel:
        if _huffman_table(dc) is None or _huffman_table(ac) is None:
            return no("bad Huffman table")
    # the entropy-coded bytes: up to the first marker that is neither a stuffed FF 00, a fill FF FF nor a restart marker
    begin = pos + 2 + length
    ff = np.flatnonzero(a[begin:-1] == 0xFF) + begin if len(a) > begin + 1 else np.zeros(0, dtype=np.int64)
    nxt = a[ff + 1]
    real = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    end = int(real[0]) if len(real) else len(a)
    if len(real) and a[end + 1] != 0xD9:
        return no("multi-scan: marker 0x%02X behind the first scan" % a[end + 1])
    info.scan = (begin, end)
    info._restarts = ff[(nxt >= 0xD0) & (nxt <= 0xD7) & (ff < end)] if info.restart_interval else None
    info.qt, info.dc, info.ac = (tuple(s[i] for s in sel) for i in range(3))
    info.supported, info.reason = True, None


_HT_CACHE = {}


def _huffman_table(payload):
    """DHT payload (16 counts + symbols) -> int32 [JH_STRIDE] (csrc/jpeg_entropy.h), or None when the counts are no prefix code"""
    if payload in _HT_CACHE:
        return _HT_CACHE[payload]
    counts, symbols = payload[:16], payload[16:]
    t = np.zeros(JH_STRIDE, dtype=np.int32)
    t[JH_MAXCODE:JH_MAXCODE + 17] = -1
    ok = len(symbols) == sum(counts) and len(symbols) <= 256
    code = k = 0
    for l in range(1, 17):
        n = counts[l - 1]
        if ok and n:
            if code + n > (1 << l):
                ok = False
                break
            t[JH_VALOFF + l] = k - code
            t[JH_MAXCODE + l] = code + n - 1
            if l <= 9:
                for i in range(n):
                    t[(code + i) << (9 - l):(code + i + 1) << (9 - l)] = (l << 8) | symbols[k + i]
            code += n
            k += n
        code <<= 1
    if ok:
        t[JH_VAL:JH_VAL + len(symbols)] = np.frombuffer(symbols, dtype=np.uint8)
    if len(_HT_CACHE) > 4096:
        _HT_CACHE.clear()
    _HT_CACHE[payload] = t if ok else None
    return _HT_CACHE[payload]


class _Pinned:
    """a cached pinned buffer: refilled only after the last DMA out of it has left (`preprocess._staging`'s rule)"""

    def __init__(self):
        self.buf = self.busy = None

    def get(self, nbytes):
        if self.busy is not None:
            self.busy.synchronize()
            self.busy = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
        return self.buf

    def sent(self):
        self.busy = torch.cuda.Event()
        self.busy.record()


_PIN_BYTES, _PIN_COEF = _Pinned(), _Pinned()
_POOL = None


def host_threads():
    return max(1, min(MAX_HOST_THREADS, len(os.sched_getaffinity(0))))


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=host_threads())
    return _POOL


def _device_buffer(name, nbytes, dev):
    """every device buffer of a decode ("out", "planes", "coef") is allocated here (the tests put guard bytes around them)"""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _align(n, a=256):
    return (n + a - 1) // a * a


def entropy_host(bytes_np, images, htabs, coef_np, status, threads=None):
    """dod_jpeg_entropy_host over all images of the table on `threads` threads (default: `host_threads()`), each a contiguous run
    of images.  Everything is host memory (numpy); status is ORed into."""
    fn = nat.lib().dod_jpeg_entropy_host
    n = len(images)
    threads = max(1, min(host_threads() if threads is None else int(threads), n))
    args = (bytes_np.ctypes.data_as(C.c_void_p), bytes_np.size, images.ctypes.data_as(C.c_void_p))
    tail = (htabs.ctypes.data_as(C.c_void_p), len(htabs), coef_np.ctypes.data_as(C.c_void_p), coef_np.size // 64, status.ctypes.data_as(C.c_void_p))
    # equal shares of the BLOCKS, not of the images: a batch is ragged
    work = np.cumsum(images[:, JI_MCUS_X] * images[:, JI_MCUS_Y] * (images[:, JI_HS] * images[:, JI_VS] + np.where(images[:, JI_NCOMP] == 3, 2, 0)))
    cuts = sorted({0, n} | {int(np.searchsorted(work, work[-1] * t / threads, side="right")) for t in range(1, threads)})
    runs = [(lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    if len(runs) == 1:
        rcs = [fn(*args, runs[0][0], runs[0][1], *tail)]
    else:
        rcs = list(_pool().map(lambda r: fn(*args, r[0], r[1], *tail), runs))
    for rc in rcs:
        nat.check(rc)


def build_tables(infos, routes, byte_offs, out_offs):
    """The integer tables of a batch (include/dinodet.h, dod_jpeg_*).  infos: `parse_jpeg` results; routes: per image "host" |
    "device" | None (not decoded here); byte_offs: where each file starts in the byte buffer; out_offs: where its pixels go.
    Coefficient blocks are laid out host images first, device images behind them.  Returns a dict: images int64 [B, 32], intervals
    int64 [V, 5], htabs int32 [T, 802], qtabs uint16 [Q, 64], comps int64 [C, 4], n_host_blocks, n_blocks, plane_bytes, n_items."""
    B = len(infos)
    images = np.zeros((B, JI_STRIDE), dtype=np.int64)
    hts, qts = {}, {}
    comps, intervals = [], []
    order = [b for b in range(B) if routes[b] == "host"] + [b for b in range(B) if routes[b] == "device"]
    n_host = sum(r == "host" for r in routes)
    block = plane = 0
    n_host_blocks = 0
    for pos, b in enumerate(order):
        info, row = infos[b], images[b]
        hs, vs = info.sampling
        mx, my = -(-info.width // (8 * hs)), -(-info.height // (8 * vs))
        row[:10] = (info.width, info.height, info.ncomp, hs, vs, mx, my, info.restart_interval, byte_offs[b] + info.scan[0], byte_offs[b] + info.scan[1])
        for c in range(info.ncomp):
            bw, bh = (mx * hs, my * vs) if c == 0 else (mx, my)
            row[JI_BLOCK0 + c], row[JI_BLOCKS_W + c], row[JI_PLANE + c] = block, bw, plane
            row[JI_QT + c] = qts.setdefault(info.qt[c], len(qts))
            row[JI_DC + c] = hts.setdefault(info.dc[c], len(hts))
            row[JI_AC + c] = hts.setdefault(info.ac[c], len(hts))
            comps.append((block, bw, plane, row[JI_QT + c]))
            block += bw * bh
            plane += bw * bh * 64
        if pos == n_host - 1:
            n_host_blocks = block
        if routes[b] == "device":
            ri, mcus = info.restart_interval, mx * my
            marks = info._restarts.astype(np.int64) + byte_offs[b]
            n = -(-mcus // ri)
            begins = np.concatenate([[row[JI_SCAN_BEGIN]], marks + 2])[:n]
            ends = np.concatenate([marks, [row[JI_SCAN_END]]])[:n]
            if len(begins) < n:                    # fewer markers than intervals: the missing ones are empty (flagged on the device)
                begins = np.concatenate([begins, np.full(n - len(begins), row[JI_SCAN_END])])
                ends = np.concatenate([ends, np.full(n - len(ends), row[JI_SCAN_END])])
            first = np.arange(n, dtype=np.int64) * ri
            intervals.append(np.stack([np.full(n, b, dtype=np.int64), begins, ends, first, np.minimum(ri, mcus - first)], axis=1))
    items = np.array([info.height * -(-info.width // 4) if routes[b] else 0 for b, info in enumerate(infos)], dtype=np.int64)
    images[:, JI_ITEM0] = np.concatenate([[0], np.cumsum(items)[:-1]])
    images[:, JI_OUT] = out_offs
    for b in range(B):                             # an image decoded elsewhere owns no items: give it a size so that nothing divides by 0
        if not routes[b]:
            images[b, JI_WIDTH] = images[b, JI_HEIGHT] = 1
    qtabs = np.zeros((max(len(qts), 1), 64), dtype=np.uint16)
    for payload, i in qts.items():
        qtabs[i, ZIGZAG] = np.frombuffer(payload, dtype=np.uint8)
    htabs = np.stack([_huffman_table(p) for p in hts]) if hts else np.zeros((1, JH_STRIDE), dtype=np.int32)
    return dict(images=images, intervals=np.concatenate(intervals) if intervals else np.zeros((0, JV_STRIDE), dtype=np.int64), htabs=htabs, qtabs=qtabs,
                comps=np.array(comps, dtype=np.int64).reshape(-1, 4), n_host_blocks=n_host_blocks, n_blocks=block, plane_bytes=plane,
                n_items=int(items.sum()))


class DecodedBatch(_pre.Staged):
    """`decode_jpeg_batch`'s result: the `Staged` fields (src on the device; src_offs, heights, widths on the host) plus `status`,
    int32 [B] on the device -- the flags of every stream's entropy decode (0 = clean).  Nothing has been synchronised: the pixels of a
    flagged image are still a function of its bytes (the rest of the flagged interval decodes as zeros), and `check()` is where a
    training loop learns of it, in the manner of `SetCriterion.check_assignment()`."""

    def __init__(self, src, src_offs, heights, widths, status, routes):
        super().__init__(src, src_offs, heights, widths)
        self.status, self.routes = status, routes

    def images(self):
        """per image a uint8 [H, W, 3] view of `src` on the device"""
        return [self.src[o:o + int(h) * int(w) * 3].view(int(h), int(w), 3) for o, h, w in zip(self.src_offs.tolist(), self.heights, self.widths)]

    def check(self):
        """one synchronisation; raises ValueError naming every image whose stream was flagged"""
        st = self.status.cpu().numpy()
        bad = [f"image {b}: " + ", ".join(text for bit, text in FLAGS.items() if st[b] & bit) for b in np.flatnonzero(st)]
        if bad:
            raise ValueError("malformed JPEG stream: " + "; ".join(bad))
        return self


def _route(infos, entropy, fallback):
    if entropy not in ("auto", "device", "host"):
        raise ValueError(f"entropy must be 'auto', 'device' or 'host', got {entropy!r}")
    routes = []
    for b, info in enumerate(infos):
        if not info.supported:
            if not fallback:
                raise UnsupportedJpeg(b, info.reason)
            routes.append(None)
        elif entropy == "device":
            if not info.restart_interval:
                raise ValueError(f"file {b}: entropy='device' decodes one restart interval per thread and this file has no restart markers")
            routes.append("device")
        elif entropy == "host":
            routes.append("host")
        else:
            # "auto": a file without restart markers takes the host entropy path, which beat Pillow at equal core count
            routes.append("device" if info.restart_interval else "host")
    return routes


def _pillow_rgb(a):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(a.tobytes())).convert("RGB")))


def decode_jpeg_batch(files, device="cuda", entropy="auto", fallback=True, threads=None):
    """files: a sequence of JPEG files, each as bytes / bytearray / a uint8 array, or a path to read.  Returns a `DecodedBatch` whose
    pixels are Pillow's `Image.open(f).convert("RGB")` bit for bit, on `device`.

    entropy: "device" = one GPU thread per restart interval (every file must carry restart markers, else ValueError); "host" =
    `dod_jpeg_entropy_host` on up to min(16, usable CPUs) threads (`threads` lowers that) into pinned memory; "auto" = "device" for
    the files with restart markers, "host" for the others.  fallback: a stream outside the device path (see
    `parse_jpeg(...).reason`) is decoded by Pillow on the host into its slot of the same buffer; with fallback=False it raises
    `UnsupportedJpeg`.  Launches go to the current stream and nothing waits for them: a malformed scan is reported by
    `DecodedBatch.check()`."""
    datas = [_as_bytes(f) for f in files]
    if not datas:
        raise ValueError("empty batch")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("decode_jpeg_batch needs a GPU device (there is no CPU fallback)")
    infos = [parse_jpeg(d) for d in datas]
    routes = _route(infos, entropy, fallback)
    B = len(datas)
    pixels = {b: _pillow_rgb(datas[b]) for b in range(B) if routes[b] is None}
    hs = np.array([pixels[b].shape[0] if b in pixels else infos[b].height for b in range(B)], dtype=np.int32)
    ws = np.array([pixels[b].shape[1] if b in pixels else infos[b].width for b in range(B)], dtype=np.int32)
    sizes = hs.astype(np.int64) * ws * 3
    src_offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    # the byte buffer: the files the device reads first (they leave in the DMA), the host's behind them
    byte_offs = np.zeros(B, dtype=np.int64)
    n_dev_bytes = n_bytes = 0
    for want in ("device", "host"):
        for b in range(B):
            if routes[b] == want:
                byte_offs[b] = n_bytes
                n_bytes += len(datas[b])
        if want == "device":
            n_dev_bytes = n_bytes
    t = build_tables(infos, routes, byte_offs, src_offs)
    out = _device_buffer("out", int(sizes.sum()), dev)
    status_host = np.zeros(B, dtype=np.int32)
    if t["n_blocks"]:
        # one pinned block = [tables | status | file bytes]; the tables' scan offsets are relative to the file bytes.  The status
        # words leave in a copy of their own: the batch keeps them, and must not keep the tables and file bytes alive with them
        parts = [t["images"], t["intervals"], t["htabs"], t["qtabs"], t["comps"], status_host]
        offs, n = [], 0
        for p in parts:
            offs.append(n)
            n = _align(n + p.nbytes)
        head = n
        pin = _PIN_BYTES.get(head + n_bytes + 16)
        pv = pin.numpy()
        for b in range(B):
            if routes[b]:
                pv[head + byte_offs[b]:head + byte_offs[b] + len(datas[b])] = datas[b]
        n_host_blocks, n_blocks = t["n_host_blocks"], t["n_blocks"]
        coef_raw = _device_buffer("coef", n_blocks * 128, dev)
        coef = coef_raw.view(torch.int16)
        if n_host_blocks:
            cpin = _PIN_COEF.get(n_host_blocks * 128)
            host_rows = np.flatnonzero([r == "host" for r in routes])
            st = np.zeros(len(host_rows), dtype=np.int32)
            entropy_host(pv[head:head + n_bytes], np.ascontiguousarray(t["images"][host_rows]), t["htabs"],
                         cpin.numpy()[:n_host_blocks * 128].view(np.int16), st, threads)
            status_host[host_rows] = st
            coef_raw[:n_host_blocks * 128].copy_(cpin[:n_host_blocks * 128], non_blocking=True)
            _PIN_COEF.sent()
        for p, o in zip(parts, offs):
            pv[o:o + p.nbytes] = p.reshape(-1).view(np.uint8)
        blob = pin[:head + n_dev_bytes].to(dev, non_blocking=True)
        status = pin[offs[-1]:offs[-1] + status_host.nbytes].to(dev, non_blocking=True).view(torch.int32)
        _PIN_BYTES.sent()
        d_images, d_intervals, d_htabs, d_qtabs, d_comps = (blob[o:o + p.nbytes].view(_TORCH[p.dtype.type]) for p, o in zip(parts[:-1], offs))
        L = nat.lib()
        if n_blocks > n_host_blocks:
            coef[n_host_blocks * 64:].zero_()
            nat.check(L.dod_jpeg_entropy_device(nat.ptr(blob[head:]), n_dev_bytes, nat.ptr(d_images), B, nat.ptr(d_intervals),
                                                len(t["intervals"]), nat.ptr(d_htabs), len(t["htabs"]), nat.ptr(coef), n_blocks, nat.ptr(status),
                                                nat.stream_ptr()))
        planes = _device_buffer("planes", t["plane_bytes"], dev)
        nat.check(L.dod_jpeg_idct(nat.ptr(coef), n_blocks, nat.ptr(d_comps), len(t["comps"]), nat.ptr(d_qtabs), len(t["qtabs"]), nat.ptr(planes),
                                  nat.stream_ptr()))
        nat.check(L.dod_jpeg_color(nat.ptr(planes), nat.ptr(d_images), B, t["n_items"], nat.ptr(out), nat.stream_ptr()))
    else:
        status = torch.zeros(B, dtype=torch.int32, device=dev)
    if pixels:
        total = sum(p.size for p in pixels.values())
        pin = _pre._staging(total)
        pv, n = pin.numpy(), 0
        run = None                                 # (first output byte, first staged byte) of a run of neighbouring fallback images
        for b in sorted(pixels):
            p = pixels[b]
            pv[n:n + p.size] = p.reshape(-1)
            if run is None:
                run = (int(src_offs[b]), n)
            n += p.size
            if b + 1 not in pixels:                # the run ends here: one copy for all of it
                out[run[0]:run[0] + n - run[1]].copy_(pin[run[1]:n], non_blocking=True)
                run = None
        _pre._staging_sent()
    return DecodedBatch(out, src_offs, hs, ws, status, routes)


_TORCH = {np.int64: torch.int64, np.int32: torch.int32, np.uint16: torch.int16, np.uint8: torch.uint8}


def collate_encoded(batch):
    """collate_fn of a DataLoader over (file bytes, target) pairs -- the counterpart of `augment.collate_raw` for a dataset whose
    __getitem__ READS the file and never decodes it: (list of files, list of targets), for `decode_jpeg_batch` in the training loop"""
    files, targets = zip(*batch)
    return list(files), list(targets)
