"""The JPEG decoder's specification and its cases.

`decode(data)` restates in numpy what Pillow's `Image.open(f).convert("RGB")` computes for a baseline / extended-sequential Huffman
JPEG through libjpeg-turbo (third-party, restated here from the format's definition and the library's documented arithmetic):
Huffman decode of one interleaved scan (jdhuff.c), dequantisation + the slow integer IDCT (jidctint.c jpeg_idct_islow), fancy
h2v1 / h2v2 upsampling (jdsample.c) and the YCbCr -> RGB tables (jdcolor.c).  It shares no code with dinov2_od_amd/jpeg.py or the
kernels: its own header walk, its own Huffman tables (a 16-bit look-up), its own coefficient layout.  test_jpeg_cpu.py pins it
against Pillow on the whole grid; everything else is pinned against it.

`grid()` is the case list: Pillow encodings of a deterministic gradient-plus-noise image.
"""
import io

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

SIZES = [(1, 1), (5, 5), (7, 9), (8, 8), (16, 16), (17, 33), (33, 4), (3, 40), (40, 3), (37, 53)]      # (width, height)
SUBSAMPLINGS = (0, 1, 2)                    # Pillow's: 4:4:4, 4:2:2, 4:2:0
QUALITIES = (30, 90, 100)
OPTIONS = {"plain": {}, "rows1": {"restart_marker_rows": 1}, "blocks3": {"restart_marker_blocks": 3}, "opt": {"optimize": True}}
NOISES = (0, 60)


# ------------------------------------------------------------------------------------------------------------------- the cases
def picture(width, height, noise, seed=0):
    """uint8 [height, width, 3]: three different gradients plus uniform noise of the given amplitude"""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    base = np.stack([255.0 * x / max(width - 1, 1), 255.0 * y / max(height - 1, 1), 255.0 * (x + y) / max(width + height - 2, 1)], axis=2)
    rng = np.random.default_rng(1000 * seed + 7 * width + 13 * height + noise)
    return np.clip(base + rng.uniform(-noise, noise, base.shape), 0, 255).astype(np.uint8)


def encode(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)      # [H, W, 3] -> RGB, [H, W] -> L
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


_GRID = None


def grid():
    """name -> file bytes of every case.  Names: w{W}h{H}_s{subsampling}_q{quality}_{option}_n{noise}, grey_w{W}h{H}, every_mcu, big"""
    global _GRID
    if _GRID is None:
        g = {}
        for (w, h) in SIZES:
            for noise in NOISES:
                pic = picture(w, h, noise)
                for s in SUBSAMPLINGS:
                    for q in QUALITIES:
                        for oname, okw in OPTIONS.items():
                            g[f"w{w}h{h}_s{s}_q{q}_{oname}_n{noise}"] = encode(pic, quality=q, subsampling=s, **okw)
            g[f"grey_w{w}h{h}"] = encode(picture(w, h, 60)[:, :, 1].copy(), quality=90)
        g["every_mcu"] = encode(picture(48, 64, 60), quality=90, subsampling=2, restart_marker_blocks=1)
        g["big"] = encode(picture(640, 480, 60), quality=90, subsampling=2)
        _GRID = g
    return _GRID


def fixture_names():
    """the subset of the grid stored in tests/golden/jpeg_cases.npz: every size, sampling and option, both noise levels and all three
    qualities spread over them, the grey files, the one-MCU intervals and the large file"""
    names = []
    for i, (w, h) in enumerate(SIZES):
        for s in SUBSAMPLINGS:
            for j, oname in enumerate(OPTIONS):
                n = i + s + j
                names.append(f"w{w}h{h}_s{s}_q{QUALITIES[n % 3]}_{oname}_n{NOISES[n % 2]}")
        names.append(f"grey_w{w}h{h}")
    return names + ["every_mcu", "big"]


def has_restart(data):
    return parse(data)["ri"] > 0


def with_fill_bytes():
    """a valid file with restart markers in which every marker behind the scan header (restart markers and EOI) is preceded by
    one or two fill bytes FF, as the format allows: the same pixels, no flag"""
    d = grid()["w37h53_s2_q90_rows1_n60"]
    s = _scan_start(d)
    a = np.frombuffer(d, dtype=np.uint8)
    marks = [int(p) for p in np.flatnonzero((a[:-1] == 0xFF) & (((a[1:] >= 0xD0) & (a[1:] <= 0xD7)) | (a[1:] == 0xD9))) if p >= s]
    out, last = [], 0
    for n, p in enumerate(marks):
        out.append(d[last:p] + b"\xff" * (1 + n % 2))
        last = p
    return b"".join(out) + d[last:]


def progressive():
    return encode(picture(37, 53, 60), quality=90, progressive=True)


# --------------------------------------------------------------------------------------------------------------- header walk
def parse(data):
    """the segments of a single-scan Huffman JPEG: frame, tables, restart interval and the scan's bytes"""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8", "no SOI"
    pos = 2
    out = {"qt": {}, "ht": {}, "ri": 0}
    while True:
        assert d[pos] == 0xFF, f"marker expected at {pos}"
        m = d[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        length = (d[pos + 2] << 8) | d[pos + 3]
        seg = d[pos + 4:pos + 2 + length]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                assert pq == 0
                out["qt"][tq] = np.frombuffer(seg[i + 1:i + 65], dtype=np.uint8).astype(np.int64)      # zigzag order
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                n = sum(counts)
                out["ht"][(tc, th)] = (counts, list(seg[i + 17:i + 17 + n]))
                i += 17 + n
        elif m in (0xC0, 0xC1):
            assert seg[0] == 8
            out["height"], out["width"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            out["comps"] = [dict(id=seg[6 + 3 * c], h=seg[7 + 3 * c] >> 4, v=seg[7 + 3 * c] & 15, tq=seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xDD:
            out["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            ns = seg[0]
            assert ns == len(out["comps"])
            for c in range(ns):
                assert seg[1 + 2 * c] == out["comps"][c]["id"]
                out["comps"][c]["td"], out["comps"][c]["ta"] = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
            out["scan"] = d[pos + 2 + length:]
            return out
        else:
            assert m not in (0xC2, 0xC9, 0xCA), "not a sequential Huffman stream"
        pos += 2 + length


# ----------------------------------------------------------------------------------------------------------------- entropy
def _lookup16(counts, symbols):
    """16-bit look-up: for every 16-bit window the (length, symbol) of the code it starts with; length 0 = no code"""
    length = np.zeros(65536, dtype=np.int64)
    symbol = np.zeros(65536, dtype=np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            lo = code << (16 - l)
            length[lo:lo + (1 << (16 - l))] = l
            symbol[lo:lo + (1 << (16 - l))] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return length.tolist(), symbol.tolist()


def _intervals(scan):
    """the entropy-coded bytes split at the restart markers, stuffing removed, up to the first other marker"""
    a = np.frombuffer(scan, dtype=np.uint8)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nxt = a[ff + 1]
    end = ff[(nxt != 0) & ~((nxt >= 0xD0) & (nxt <= 0xD7))]
    end = int(end[0]) if len(end) else len(a)
    cuts = [int(p) for p in ff[(nxt >= 0xD0) & (nxt <= 0xD7)] if p < end]
    parts, begin = [], 0
    for c in cuts + [end]:
        parts.append(bytes(scan[begin:c]).replace(b"\xff\x00", b"\xff"))
        begin = c + 2
    return parts


def coefficients(data):
    """(info, list per component of int16 [blocks_y, blocks_x, 64] in natural order)"""
    info = parse(data)
    comps = info["comps"]
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    W, H = info["width"], info["height"]
    if len(comps) == 1:
        comps[0]["h"] = comps[0]["v"] = hmax = vmax = 1
    mcus_x, mcus_y = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    info.update(hmax=hmax, vmax=vmax, mcus_x=mcus_x, mcus_y=mcus_y)
    planes = [np.zeros((mcus_y * c["v"], mcus_x * c["h"], 64), dtype=np.int16) for c in comps]
    luts = {k: _lookup16(*v) for k, v in info["ht"].items()}
    parts = _intervals(info["scan"])
    ri = info["ri"] or mcus_x * mcus_y
    assert len(parts) == -(-mcus_x * mcus_y // ri), (len(parts), mcus_x * mcus_y, ri)
    zz = ZIGZAG.tolist()
    for n, part in enumerate(parts):
        b = part + b"\x00\x00\x00\x00"
        win = [(b[i] << 24) | (b[i + 1] << 16) | (b[i + 2] << 8) | b[i + 3] for i in range(len(part))] + [0]
        pos = 0
        pred = [0] * len(comps)
        for m in range(n * ri, min((n + 1) * ri, mcus_x * mcus_y)):
            my, mx = divmod(m, mcus_x)
            for ci, c in enumerate(comps):
                dl, ds = luts[(0, c["td"])]
                al, as_ = luts[(1, c["ta"])]
                for j in range(c["v"]):
                    for i in range(c["h"]):
                        blk = planes[ci][my * c["v"] + j, mx * c["h"] + i]
                        w16 = (win[pos >> 3] >> (16 - (pos & 7))) & 0xFFFF
                        assert dl[w16], "undefined DC code"
                        pos += dl[w16]
                        s = ds[w16]
                        if s:
                            v = (win[pos >> 3] >> (32 - (pos & 7) - s)) & ((1 << s) - 1)
                            pos += s
                            pred[ci] += v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            w16 = (win[pos >> 3] >> (16 - (pos & 7))) & 0xFFFF
                            assert al[w16], "undefined AC code"
                            pos += al[w16]
                            rs = as_[w16]
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            v = (win[pos >> 3] >> (32 - (pos & 7) - s)) & ((1 << s) - 1)
                            pos += s
                            blk[zz[k]] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                            k += 1
        assert pos <= 8 * len(part), "ran past the interval"
    return info, planes


# ------------------------------------------------------------------------------------------------------------------- IDCT
def _idct8(d, shift):
    """one pass of jpeg_idct_islow on int64 d[..., 8] (last axis), descaled by `shift`"""
    d = [d[..., i] for i in range(8)]
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (d[0] + d[4]) << 13
    tmp1 = (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + half) >> shift for o in out], axis=-1)


def idct_plane(coef, qt_zigzag):
    """int16 [by, bx, 64] natural-order coefficients -> uint8 [8 by, 8 bx] samples"""
    q = np.zeros(64, dtype=np.int64)
    q[ZIGZAG] = qt_zigzag
    blocks = (coef.astype(np.int64) * q).reshape(coef.shape[0], coef.shape[1], 8, 8)        # [.., row, col]
    ws = _idct8(blocks.swapaxes(-1, -2), 11).swapaxes(-1, -2)                                # columns: along the row index
    ws = ws.astype(np.int32).astype(np.int64)                                                # the library's int workspace
    px = _idct8(ws, 18)                                                                      # rows
    px = (((px & 1023) ^ 512) - 512) + 128                                                   # range_limit[x & RANGE_MASK]
    px = np.clip(px, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(coef.shape[0] * 8, coef.shape[1] * 8)


# --------------------------------------------------------------------------------------------------------- upsample + colour
def _h2v1(c):
    """fancy horizontal doubling of int64 [h, w] (w > 2) -> [h, 2 w]"""
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int64)
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out


def _h2v2(c):
    """fancy doubling in both directions of int64 [h, w] (w > 2) -> [2 h, 2 w]"""
    above = np.concatenate([c[:1], c[:-1]], axis=0)
    below = np.concatenate([c[1:], c[-1:]], axis=0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), dtype=np.int64)
    for phase, far in ((0, above), (1, below)):
        s = 3 * c + far
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        row = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int64)
        row[:, 0::2] = (3 * s + left + 8) >> 4
        row[:, 1::2] = (3 * s + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[phase::2] = row
    return out


def upsample(plane, W, H, h, v, hmax, vmax):
    """a component's padded plane -> int64 [H, W] at full resolution"""
    dw, dh = -(-W * h // hmax), -(-H * v // vmax)
    c = plane[:dh, :dw].astype(np.int64)
    fx, fy = hmax // h, vmax // v
    if (fx, fy) == (1, 1):
        up = c
    elif dw <= 2:
        up = np.repeat(np.repeat(c, fy, axis=0), fx, axis=1)
    elif (fx, fy) == (2, 1):
        up = _h2v1(c)
    elif (fx, fy) == (2, 2):
        up = _h2v2(c)
    else:
        raise AssertionError((fx, fy))
    return up[:H, :W]


def decode_stages(data):
    """(coefficient planes, sample planes, pixels uint8 [H, W, 3])"""
    info, coefs = coefficients(data)
    W, H = info["width"], info["height"]
    planes = [idct_plane(cf, info["qt"][c["tq"]]) for cf, c in zip(coefs, info["comps"])]
    full = [upsample(p, W, H, c["h"], c["v"], info["hmax"], info["vmax"]) for p, c in zip(planes, info["comps"])]
    if len(full) == 1:
        rgb = np.stack([full[0]] * 3, axis=2)
    else:
        y, cb, cr = full[0], full[1] - 128, full[2] - 128
        rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=2)
    return coefs, planes, np.clip(rgb, 0, 255).astype(np.uint8)


def decode(data):
    return decode_stages(data)[2]


# --------------------------------------------------------------------------------------------------------- malformed streams
def _scan_start(data):
    d = bytes(data)
    i = d.index(b"\xff\xda")
    return i + 2 + ((d[i + 2] << 8) | d[i + 3])


def malformed():
    """name -> bytes of streams whose HEADER parses and whose scan is broken: for the host entropy entry and the stand-alone
    sanitizer program only, never for the device"""
    g = grid()
    out = {}
    for base in ("w37h53_s2_q90_plain_n60", "w37h53_s0_q90_rows1_n60", "every_mcu"):
        d = g[base]
        s = _scan_start(d)
        for cut in (0, 1, 2, 7, (len(d) - s) // 2, len(d) - s - 3):
            out[f"trunc{cut}_{base}"] = d[:s + cut] + b"\xff\xd9"
        # random bytes, byte-stuffed as an encoder would (FF -> FF 00) so that the header parse still sees one scan
        rnd = np.random.default_rng(5).integers(0, 256, len(d) - s - 2, dtype=np.uint8).tobytes().replace(b"\xff", b"\xff\x00")
        out[f"random_{base}"] = d[:s] + rnd + b"\xff\xd9"
    # a Huffman table that defines a single 1-bit code: nearly every pattern of the scan is undefined
    d = bytearray(g["w37h53_s2_q90_plain_n60"])
    i = bytes(d).index(b"\xff\xc4")
    length = (d[i + 2] << 8) | d[i + 3]
    payload = bytes([d[i + 4]]) + bytes([1] + [0] * 15) + bytes([0])
    out["undefined_code"] = bytes(d[:i]) + b"\xff\xc4" + (2 + len(payload)).to_bytes(2, "big") + payload + bytes(d[i + 2 + length:])
    # a restart marker taken out of the middle of the scan
    d = g["w37h53_s0_q90_rows1_n60"]
    s = _scan_start(d)
    a = np.frombuffer(d, dtype=np.uint8)
    marks = [int(p) for p in np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)) if p >= s]
    p = marks[len(marks) // 2]
    out["missing_marker"] = d[:p] + d[p + 2:]
    return out
