"""JPEG decode, host side (no GPU): the numpy restatement of tests/jpeg_cases.py against Pillow and the stored fixture, the header
parse's classification, the host entropy entry against the restatement's coefficients, and the shared decode function on malformed
streams -- through the library's host entry with guard words around its buffers, and through a stand-alone program built with the
host compiler's address and undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dinov2_od_amd import _native as nat
from dinov2_od_amd import jpeg
from tests import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
GUARD = 4096                # int16 guard words in front of and behind the coefficients
SENT = 0x5A5A


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_restatement_equals_pillow_on_the_whole_grid():
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its decoder is not the arithmetic the restatement states")
    g = jc.grid()
    assert len(g) == 10 * 2 * 3 * 3 * 4 + 10 + 2
    assert sum(jc.has_restart(d) for d in g.values()) == 10 * 2 * 3 * 3 * 2 + 1
    for name, data in g.items():
        assert np.array_equal(jc.decode(data), jc.pillow_decode(data)), name


def test_restatement_equals_fixture_pixels(golden):
    names = [k[2:] for k in golden.files if k.startswith("f_") and k != "f_progressive"]
    assert set(names) == set(jc.fixture_names()) - {"big"} and len(names) == 131
    for name in names:
        got = jc.decode(golden["f_" + name].tobytes())
        assert got.shape == golden["p_" + name].shape and np.array_equal(got, golden["p_" + name]), name


def test_fixture_covers_every_size_sampling_and_option(golden):
    seen = set()
    for k in golden.files:
        if k.startswith("f_w"):
            size, s, q, opt, n = k[2:].split("_")
            seen.add((size, s, opt))
    assert len(seen) == 10 * 3 * 4
    assert os.path.getsize(GOLDEN) < (1 << 20)


def _cmyk():
    from PIL import Image
    import io
    buf = io.BytesIO()
    Image.fromarray(jc.picture(19, 11, 60)).convert("CMYK").save(buf, "JPEG", quality=90)
    return buf.getvalue()


def _twelve_bit():
    d = bytearray(jc.grid()["w17h33_s0_q90_plain_n60"])
    i = bytes(d).index(b"\xff\xc0")
    d[i + 4] = 12
    return bytes(d)


def test_parse_classifies_streams(golden):
    info = jpeg.parse_jpeg(jc.grid()["w37h53_s2_q90_rows1_n60"])
    assert info.supported and info.reason is None
    assert (info.width, info.height, info.mode, info.sampling) == (37, 53, "RGB", (2, 2)) and info.restart_interval == 3
    info = jpeg.parse_jpeg(jc.grid()["w37h53_s1_q90_plain_n60"])
    assert info.supported and info.sampling == (2, 1) and info.restart_interval == 0
    info = jpeg.parse_jpeg(bytearray(jc.grid()["grey_w17h33"]))
    assert info.supported and info.mode == "L" and (info.width, info.height) == (17, 33)
    for data, word in ((jc.progressive(), "progressive"), (golden["f_progressive"], "progressive"), (_cmyk(), "CMYK"), (_twelve_bit(), "12-bit")):
        info = jpeg.parse_jpeg(data)
        assert not info.supported and word in info.reason, (word, info)
    d = jc.grid()["w17h33_s0_q90_plain_n60"]
    assert jpeg.parse_jpeg(d[:40]).reason == "truncated header"
    assert "SOI" in jpeg.parse_jpeg(b"\x89PNG\r\n\x1a\n").reason


def _decode_host(data, threads=1):
    """(flags, coefficients, guards intact) of the library's host entry on one file"""
    info = jpeg.parse_jpeg(data)
    assert info.supported, info
    t = jpeg.build_tables([info], ["host"], np.zeros(1, np.int64), np.zeros(1, np.int64))
    n = t["n_blocks"] * 64
    raw = np.full(n + 2 * GUARD, SENT, dtype=np.int16)
    status = np.array([SENT, 0, SENT], dtype=np.int32)
    jpeg.entropy_host(np.frombuffer(data, np.uint8), t["images"], t["htabs"], raw[GUARD:GUARD + n], status[1:2], threads)
    intact = bool((raw[:GUARD] == SENT).all() and (raw[GUARD + n:] == SENT).all() and status[0] == SENT and status[2] == SENT)
    return int(status[1]), raw[GUARD:GUARD + n].copy(), intact, t


def test_host_entropy_equals_restatement_coefficients(lib):
    g = jc.grid()
    for name, data in g.items():
        flags, coef, intact, _ = _decode_host(data)
        want = np.concatenate([c.reshape(-1) for c in jc.coefficients(data)[1]])
        assert flags == 0 and intact and np.array_equal(coef, want), name


def test_host_entropy_threads_share_a_batch(lib):
    """several images over several threads: every image's blocks are what the single decode gave"""
    g = jc.grid()
    names = ["big", "grey_w37h53", "every_mcu", "w37h53_s1_q30_opt_n60", "w17h33_s0_q100_blocks3_n0"]
    infos = [jpeg.parse_jpeg(g[n]) for n in names]
    offs = np.concatenate([[0], np.cumsum([len(g[n]) for n in names])[:-1]]).astype(np.int64)
    t = jpeg.build_tables(infos, ["host"] * len(names), offs, np.zeros(len(names), np.int64))
    coef = np.full(t["n_blocks"] * 64, SENT, dtype=np.int16)
    status = np.zeros(len(names), dtype=np.int32)
    jpeg.entropy_host(np.frombuffer(b"".join(g[n] for n in names), np.uint8), t["images"], t["htabs"], coef, status, threads=3)
    assert not status.any()
    want = np.concatenate([_decode_host(g[n])[1] for n in names])
    assert np.array_equal(coef, want)


def test_fill_bytes_in_front_of_markers_are_not_flagged(lib):
    """FF FF Dn is a legal way to write a restart marker: the host walk skips the fill bytes, the coefficients are the plain file's"""
    data = jc.with_fill_bytes()
    plain = jc.grid()["w37h53_s2_q90_rows1_n60"]
    assert len(data) == len(plain) + 6 and data.count(b"\xff\xff") >= 4 and np.array_equal(jc.pillow_decode(data), jc.pillow_decode(plain))
    flags, coef, intact, _ = _decode_host(data)
    assert flags == 0 and intact and np.array_equal(coef, _decode_host(plain)[1])


def _expected_flag(name):
    return {"undefined_code": 2, "missing_marker": 8}.get(name)


def test_malformed_streams_are_flagged_and_contained(lib):
    m = jc.malformed()
    assert len(m) == 3 * 7 + 2
    for name, data in m.items():
        flags, coef, intact, _ = _decode_host(data)
        again = _decode_host(data)
        assert intact and again[2], f"{name}: a guard word was written"
        assert flags != 0, f"{name}: not flagged"
        assert flags == again[0] and np.array_equal(coef, again[1]), f"{name}: two runs differ"
        want = _expected_flag(name)
        if want is not None:
            assert flags & want, (name, flags)
        if name.startswith("trunc"):
            assert flags & 1, (name, flags)


def _fnv1a(b):
    h = 1469598103934665603
    for x in np.frombuffer(b, dtype=np.uint8).tolist():
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_sanitized_standalone_program_on_malformed_and_valid_streams(lib, tmp_path):
    """tests/jpeg_entropy_main.cpp includes only csrc/jpeg_entropy.h; built with the host compiler and -fsanitize=address,undefined it
    decodes the malformed corpus and the WHOLE valid grid out of heap blocks of exactly the buffers' sizes.  A report of either sanitizer
    aborts the program (-fno-sanitize-recover).  Its flags and coefficient digests are those of the library's host entry."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "jpeg_entropy_main")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # probe first: does this compiler link a sanitized program at all, and can it link the runtimes INTO the program (gcc's and
    # clang's spelling) so that it is self-contained?
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    static = None
    for flags in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
        p = subprocess.run([cxx] + sanitize + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            static = flags
            break
    if static is None:
        pytest.skip(f"{cxx} cannot link a program with -fsanitize=address,undefined here: {(p.stderr.strip().splitlines() or ['?'])[-1]}")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"] + sanitize + static +
                       [os.path.join(ROOT, "tests", "jpeg_entropy_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = jc.grid()
    corpus = dict(jc.malformed())
    corpus.update(g)                                                           # the whole valid grid, the large file included
    assert len(corpus) == len(jc.malformed()) + len(g)
    want, blob = [], [struct.pack("<q", len(corpus))]
    for name, data in corpus.items():
        flags, coef, _, t = _decode_host(data)
        want.append((flags, _fnv1a(coef.tobytes()) if len(coef) < 200000 else None))
        blob.append(struct.pack("<3q", len(data), len(t["htabs"]), t["n_blocks"]) + t["images"][0].tobytes() + t["htabs"].tobytes() + bytes(data))
    path = tmp_path / "corpus.bin"
    path.write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(corpus)
    for line, (flags, digest), name in zip(lines, want, corpus):
        _, f, h = line.split()
        assert int(f) == flags, (name, line)
        if digest is not None:
            assert int(h, 16) == digest, (name, line)
