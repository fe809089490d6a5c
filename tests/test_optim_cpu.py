"""CPU-side checks of the native optimizer step (dinov2_od_amd.optim, dod_optim_* of include/dinodet.h): on CPU parameters the
step is PyTorch's bit for bit (the delegated path), the state interchanges with torch.optim.Adam, the entry points are exported
at ABI revision 6 and every argument error returns DOD_ERR_INVALID with a message before any HIP call."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

from dinov2_od_amd import _native as nat
from dinov2_od_amd import optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NAMES = ("dod_optim_workspace_bytes", "dod_optim_clip_grad_norm", "dod_optim_adam_step", "dod_optim_last_error")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


def test_module_is_exported():
    import dinov2_od_amd
    assert dinov2_od_amd.optim is optim
    assert issubclass(optim.Adam, torch.optim.Adam) and callable(optim.clip_grad_norm_)


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (7,), (1,), (2, 2, 2))]


def _grads(ps, step):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(ps):
        p.grad = None if (i == 2 and step == 0) else 3.0 * torch.randn(p.shape, generator=g)      # one parameter joins at step 2


@pytest.mark.parametrize("max_norm", [None, 1.0])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
def test_cpu_parameters_take_pytorchs_step_bit_for_bit(max_norm, weight_decay):
    a, b = _params(0), _params(0)
    oa = torch.optim.Adam(a, lr=1e-2, weight_decay=weight_decay)
    ob = optim.Adam(b, lr=1e-2, weight_decay=weight_decay, max_grad_norm=max_norm)
    for step in range(3):
        _grads(a, step)
        _grads(b, step)
        if max_norm is not None:
            want = torch.nn.utils.clip_grad_norm_(a, max_norm)
        oa.step()
        ob.step()
        if max_norm is not None:
            assert torch.equal(ob.last_grad_norm, want)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(ob.state[b[2]]["step"]) == 2 and float(ob.state[b[0]]["step"]) == 3
    for x, y in zip(a, b):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[x][k], ob.state[y][k])


def test_clip_grad_norm_defers_on_cpu():
    a, b = _params(1), _params(1)
    _grads(a, 1)
    _grads(b, 1)
    for kw in ({}, {"norm_type": float("inf")}, {"norm_type": 1}):
        want = torch.nn.utils.clip_grad_norm_(a, 0.5, **kw)
        got = optim.clip_grad_norm_(b, 0.5, **kw)
        assert torch.equal(got, want)
        for x, y in zip(a, b):
            assert torch.equal(x.grad, y.grad)
    assert torch.equal(optim.clip_grad_norm_(b[0], 0.5), torch.nn.utils.clip_grad_norm_(a[0], 0.5))      # a single tensor
    for p in b:
        p.grad = None
    assert float(optim.clip_grad_norm_(b, 1.0)) == 0.0


def test_step_hooks_run_once_and_closure_is_evaluated():
    p = _params(2)
    torch.optim.Adam(_params(3))      # makes torch.optim.Adam.step a hooked function before ours delegates to it
    o = optim.Adam(p, lr=1e-3, max_grad_norm=1.0)
    calls = []
    o.register_step_post_hook(lambda *a: calls.append(1))

    def closure():
        _grads(p, 1)
        return torch.tensor(3.5)
    assert float(o.step(closure)) == 3.5
    assert calls == [1]


def test_state_dict_round_trips_with_torch_adam():
    a, b = _params(0), _params(0)
    ours = optim.Adam(b, lr=1e-2, weight_decay=1e-4, max_grad_norm=1.0)
    for step in range(2):
        _grads(b, step)
        ours.step()
    sd = copy.deepcopy(ours.state_dict())      # as a checkpoint file would: load_state_dict keeps tensors that need no cast
    theirs = torch.optim.Adam(a, lr=5e-1)
    theirs.load_state_dict(sd)
    assert set(theirs.state_dict()["param_groups"][0]) == set(sd["param_groups"][0])
    assert theirs.param_groups[0]["lr"] == 1e-2
    back = optim.Adam(_params(0), lr=5e-1, max_grad_norm=1.0)
    back.load_state_dict(theirs.state_dict())
    s0, s1 = sd["state"], back.state_dict()["state"]
    assert s0.keys() == s1.keys()
    for k in s0:
        assert set(s0[k]) == {"step", "exp_avg", "exp_avg_sq"}
        for f in s0[k]:
            assert torch.equal(s0[k][f], s1[k][f])
        assert s0[k]["step"].device.type == "cpu"
    # and the resumed optimizers go on identically
    for x, y in zip(a, b):
        x.data.copy_(y.data)
    _grads(a, 2)
    _grads(b, 2)
    torch.nn.utils.clip_grad_norm_(a, 1.0)
    theirs.step()
    ours.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_symbols_in_header_and_binding(lib):
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    assert int(re.search(r"#define DOD_ABI_VERSION (\d+)", hdr).group(1)) == 7 == nat.ABI_VERSION == lib.dod_abi_version()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in nat.SYMBOLS and hasattr(lib, name)
    assert "typedef struct dod_optim_tensor" in hdr and C.sizeof(nat.DodOptimTensor) == 48


def test_workspace_bytes_is_monotone(lib):
    f = lib.dod_optim_workspace_bytes
    chunk = lib.dod_test_counter(b"optim_chunk_elems")
    assert chunk > 0 and lib.dod_test_counter(b"optim_table_tensors") > 0
    sizes = [0, 1, chunk - 1, chunk, chunk + 1, 57 * chunk, 5_700_000, 1 << 31, 1 << 36]
    for nt in (0, 1, 57, 1000):
        vals = [f(nt, n) for n in sizes]
        assert all(x <= y for x, y in zip(vals, vals[1:])) and vals[0] > 0
    for n in sizes:
        vals = [f(nt, n) for nt in (0, 1, 2, 57, 58, 1000)]
        assert all(x <= y for x, y in zip(vals, vals[1:]))
    assert f(57, 1 << 36) > f(57, 5_700_000) and f(58, 5_700_000) > f(57, 5_700_000)
    assert f(-1, 10) == 0 and f(1, -10) == 0


def _tensors(n=2, count=8):
    """descriptors whose pointers are plausible but never dereferenced: every call below returns before a launch"""
    arr = (nat.DodOptimTensor * n)()
    for d in arr:
        d.p, d.g, d.m, d.v, d.n, d.step_size, d.bc2_sqrt = 0x1000, 0x2000, 0x3000, 0x4000, count, 1e-3, 1.0
    return arr


def _adam(lib, arr, n, *, betas=(0.9, 0.999), eps=1e-8, wd=0.0, max_norm=1.0, norm=0x5000, ws=0x6000, ws_bytes=1 << 20):
    return lib.dod_optim_adam_step(arr, n, betas[0], betas[1], eps, wd, max_norm, norm, ws, ws_bytes, None)


def _clip(lib, arr, n, *, max_norm=1.0, norm=0x5000, ws=0x6000, ws_bytes=1 << 20):
    return lib.dod_optim_clip_grad_norm(arr, n, max_norm, norm, ws, ws_bytes, None)


def _bad(field, value):
    arr = _tensors()
    setattr(arr[1], field, value)
    return arr


ADAM_ERRORS = {
    "negative n_tensors": lambda lib: _adam(lib, _tensors(), -1),
    "null list": lambda lib: _adam(lib, None, 2),
    "negative n": lambda lib: _adam(lib, _bad("n", -1), 2),
    "null p": lambda lib: _adam(lib, _bad("p", None), 2),
    "null g": lambda lib: _adam(lib, _bad("g", None), 2),
    "null m": lambda lib: _adam(lib, _bad("m", None), 2),
    "null v": lambda lib: _adam(lib, _bad("v", None), 2),
    "null total_norm": lambda lib: _adam(lib, _tensors(), 2, norm=None),
    "null workspace": lambda lib: _adam(lib, _tensors(), 2, ws=None),
    "short workspace": lambda lib: _adam(lib, _tensors(), 2, ws_bytes=lib.dod_optim_workspace_bytes(2, 16) - 1),
    "beta1 = 1": lambda lib: _adam(lib, _tensors(), 2, betas=(1.0, 0.999)),
    "negative eps": lambda lib: _adam(lib, _tensors(), 2, eps=-1.0),
}
CLIP_ERRORS = {
    "negative n_tensors": lambda lib: _clip(lib, _tensors(), -1),
    "null list": lambda lib: _clip(lib, None, 2),
    "negative n": lambda lib: _clip(lib, _bad("n", -1), 2),
    "null g": lambda lib: _clip(lib, _bad("g", None), 2),
    "null total_norm": lambda lib: _clip(lib, _tensors(), 2, norm=None),
    "null workspace": lambda lib: _clip(lib, _tensors(), 2, ws=None),
    "short workspace": lambda lib: _clip(lib, _tensors(), 2, ws_bytes=lib.dod_optim_workspace_bytes(2, 16) - 1),
}


@pytest.mark.parametrize("case", sorted(ADAM_ERRORS))
def test_adam_step_argument_errors(lib, case):
    _adam(lib, _bad("n", -1), 2)
    first = lib.dod_optim_last_error()
    assert ADAM_ERRORS[case](lib) == INVALID
    msg = lib.dod_optim_last_error()
    assert msg and msg.startswith(b"dod_optim_adam_step") and (case == "negative n" or msg != first)


@pytest.mark.parametrize("case", sorted(CLIP_ERRORS))
def test_clip_grad_norm_argument_errors(lib, case):
    assert CLIP_ERRORS[case](lib) == INVALID
    msg = lib.dod_optim_last_error()
    assert msg and msg.startswith(b"dod_optim_clip_grad_norm")


def test_launch_counter_is_known_and_untouched_by_errors(lib):
    before = lib.dod_test_counter(b"optim_launches")
    assert before >= 0
    _adam(lib, _tensors(), -1)
    assert lib.dod_test_counter(b"optim_launches") == before
