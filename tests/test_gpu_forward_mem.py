"""dod_forward_mem (include/dinodet.h): the forward that also hands out the decoder's memory.  On the smallest detector tests/cases.py
builds, in every precision mode: detections bit-identical to dod_forward's, memory bit-identical to what tap 1000 copies, both outputs
between guard rows; and Engine.forward_mem against forward_packed with the micro-batches forced on and off."""
import pytest
import torch

from dinov2_od_amd import _native as nat, synth
from tests import cases
from tests import guard_rows as gr

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "bf16x3", "fp16x2", "bf16", "fp8"]
H, W = 70, 98                                                            # a 5 x 7 token map: 36 tokens with CLS


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from tests import gpu_util
    return gpu_util


def _bits(t):
    return t.contiguous().view(torch.int32)


def _model(G, precision):
    bb, dc = cases.cfg1(25)
    m = G.make_detector(bb, dc, precision, "facebook/dinov2-small")
    eng = m._get_engine()
    eng.micro_streams = 1
    return m, eng, dc


def _tapped(m, eng, dc, x):
    """(dod_forward's detections, tap 1000's copy of the memory)"""
    want = m.forward_packed(x).clone()
    N = nat.lib().dod_num_tokens(eng._h, x.shape[-2], x.shape[-1])
    tap = eng.set_tap(1000, (x.shape[0], N, dc.hidden_dim), "cuda:0")
    again = m.forward_packed(x).clone()
    torch.cuda.synchronize()
    eng.clear_taps()
    assert torch.equal(_bits(again), _bits(want))
    return want, tap.clone()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_c_entry_equals_forward_and_tap_1000_bit_for_bit(G, precision):
    m, eng, dc = _model(G, precision)
    x = G.to_gpu(synth.make_pixels(2, H, W, seed=0))
    want, mem_want = _tapped(m, eng, dc, x)
    L = nat.lib()
    B, N, Q, Wd = 2, mem_want.shape[1], dc.num_queries, dc.num_classes + 4
    assert N == 36
    bufs = {"det": gr.guarded(B * Q, Wd, torch.float32, gr.SENT_F), "mem": gr.guarded(B * N, dc.hidden_dim, torch.float32, gr.SENT_F)}
    nbytes = L.dod_workspace_bytes(eng._h, B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    nat.check(L.dod_forward_mem(eng._h, nat.ptr(x), B, H, W, nat.ptr(bufs["det"][1]), nat.ptr(bufs["mem"][1]), nat.ptr(ws), nbytes, nat.stream_ptr()),
              eng._h)
    torch.cuda.synchronize()
    gr.untouched(bufs)
    assert torch.equal(_bits(bufs["det"][1].reshape(B, Q, Wd)), _bits(want))
    assert torch.equal(_bits(bufs["mem"][1].reshape(B, N, dc.hidden_dim)), _bits(mem_want))
    assert bool(torch.isfinite(mem_want).all()) and float(mem_want.abs().max()) > 0
    # the same workspace again through dod_forward: the extra copy left nothing behind
    det2 = torch.empty_like(want)
    nat.check(L.dod_forward(eng._h, nat.ptr(x), B, H, W, nat.ptr(det2), nat.ptr(ws), nbytes, nat.stream_ptr()), eng._h)
    torch.cuda.synchronize()
    assert torch.equal(_bits(det2), _bits(want))
    with pytest.raises(ValueError):
        nat.check(L.dod_forward_mem(eng._h, nat.ptr(x), B, H, W, nat.ptr(det2), None, nat.ptr(ws), nbytes, nat.stream_ptr()), eng._h)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_engine_forward_mem_with_micro_batches_on_and_off(G, precision):
    m, eng, dc = _model(G, precision)
    named = m._engine_named()
    for B in (3, 4):
        x = G.to_gpu(synth.make_pixels(B, H, W, seed=B))
        eng.micro_streams = 1
        want, mem_want = _tapped(m, eng, dc, x)
        det, mem = eng.forward_mem(x, named)
        torch.cuda.synchronize()
        assert det.shape == want.shape and mem.shape == mem_want.shape and mem.dtype == torch.float32
        assert torch.equal(_bits(det), _bits(want)) and torch.equal(_bits(mem), _bits(mem_want)), ("single launch", B)
        eng.micro_streams, eng.micro_min_batch, eng.micro_min_rows = 2, 2, 0
        assert eng._micro_ok(B, H, W)
        det, mem = eng.forward_mem(x, named)
        torch.cuda.synchronize()
        assert torch.equal(_bits(det), _bits(want)) and torch.equal(_bits(mem), _bits(mem_want)), ("micro-batches", B)
        assert torch.equal(_bits(m.forward_packed(x)), _bits(want))
    eng.use_graph = True                                                 # this entry stays eager: nothing is captured for it
    det, mem = eng.forward_mem(x, named)
    torch.cuda.synchronize()
    assert torch.equal(_bits(det), _bits(want)) and torch.equal(_bits(mem), _bits(mem_want)) and not eng._graphs
    eng.use_graph = False
