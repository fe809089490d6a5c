"""CPU-side checks of the device Hungarian assignment's boundary (dod_match_assign, include/dinodet.h): the entry points are
exported at ABI revision 6, argument errors return the documented codes before any HIP call, and SetCriterion refuses
device_assignment with a matcher that has no match_table.  No GPU compute: every call below returns before a launch."""
import ctypes as C
import os
import re

import pytest

from dinov2_od_amd import _native as nat
from dinov2_od_amd import losses as L
from dinov2_od_amd.matching import HungarianMatcher
from tests import criterion_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = 1, 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def test_assign_symbols_exported_at_abi_6(lib):
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    assert int(re.search(r"#define DOD_ABI_VERSION (\d+)", hdr).group(1)) == 7 == nat.ABI_VERSION == lib.dod_abi_version()
    for name in ("dod_match_assign", "dod_match_assign_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in nat.SYMBOLS and hasattr(lib, name)


def test_workspace_bytes(lib):
    assert lib.dod_match_assign_workspace_bytes(4, 25, 41) == lib.dod_match_assign_workspace_bytes(4, 25, 0) + 41 * 32
    assert lib.dod_match_assign_workspace_bytes(64, 300, 6400) >= 29 * (64 * 300 + 6400)     # 29 bytes of state per row + column
    for B, Q, G in ((0, 25, 4), (4, 0, 4), (4, 25, -1), (-1, 25, 4)):
        assert lib.dod_match_assign_workspace_bytes(B, Q, G) == 0


def test_assign_rejects_bad_arguments_before_any_launch(lib):
    B, Q, G = 2, 5, 3
    need = lib.dod_match_assign_workspace_bytes(B, Q, G)
    cost, offs, lab = (C.c_float * (G * Q))(), (C.c_int32 * (B + 1))(0, 1, 3), (C.c_int64 * G)()
    match, status, ws = (C.c_int32 * (B * Q))(), (C.c_int32 * B)(), (C.c_uint8 * need)()
    p = lambda a: C.cast(a, C.c_void_p)                                     # noqa: E731
    ok = dict(cost=p(cost), offs=p(offs), B=B, Q=Q, G=G, lab=p(lab), C=4, match=p(match), status=p(status), ws=p(ws))

    def call(nbytes=need, **kw):
        a = dict(ok, **kw)
        return lib.dod_match_assign(a["cost"], a["offs"], a["B"], a["Q"], a["G"], a["lab"], a["C"], a["match"], a["status"], a["ws"],
                                    nbytes, None)

    for bad in (dict(offs=None), dict(match=None), dict(status=None), dict(cost=None), dict(B=0), dict(B=-3), dict(Q=0),
                dict(Q=-1), dict(G=-1), dict(C=0), dict(C=-5)):
        assert call(**bad) == INVALID, bad
    assert call(need - 1) == STATE                                          # short workspace
    assert call(0, ws=None) == STATE
    assert call(ws=None) == STATE


def test_device_assignment_needs_match_table():
    with pytest.raises(TypeError, match="match_table"):
        L.SetCriterion(cc.FixedMatcher([]), 5, dict(cc.WEIGHTS), device_assignment=True)
    crit = L.SetCriterion(HungarianMatcher(), 5, dict(cc.WEIGHTS), device_assignment=True)
    assert crit.device_assignment and crit.last_assignment_status is None
    crit.check_assignment()                                                 # nothing assigned yet: nothing to raise
    host = L.SetCriterion(HungarianMatcher(), 5, dict(cc.WEIGHTS))
    assert not host.device_assignment
