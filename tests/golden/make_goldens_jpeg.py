"""Writes tests/golden/jpeg_cases.npz: for a subset of the case grid (tests/jpeg_cases.py fixture_names) the JPEG file's bytes
("f_<name>") and the pixels Pillow decoded from it ("p_<name>", uint8 [H, W, 3]), so that the GPU tests do not depend on which JPEG
library the Pillow next to them was built with.  Needs a Pillow built on libjpeg-turbo (the arbiter); the large 480 x 640 file is
left out -- its pixels alone are close to the size limit of a committed file -- and is checked against the numpy restatement.

    python -m tests.golden.make_goldens_jpeg
"""
import os

import numpy as np
from PIL import features

from tests import jpeg_cases as jc

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_cases.npz")


def main():
    assert features.check_feature("libjpeg_turbo"), "the fixture's pixels must come from libjpeg-turbo"
    g = jc.grid()
    arrays = {}
    for name in jc.fixture_names():
        if name == "big":
            continue
        arrays["f_" + name] = np.frombuffer(g[name], dtype=np.uint8)
        arrays["p_" + name] = jc.pillow_decode(g[name])
    prog = jc.progressive()
    arrays["f_progressive"], arrays["p_progressive"] = np.frombuffer(prog, dtype=np.uint8), jc.pillow_decode(prog)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(arrays) // 2} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
