"""What the GPU tests of dod_detect, dod_detect_views and dod_fuse_views share: every output of a call sits between guard rows filled with
a sentinel, which the call must leave untouched, and two results are the same when they agree bit for bit (floats by their bits)."""
import numpy as np
import torch

GUARD = 8                       # rows in front of and behind every output
SENT_F, SENT_I = -77.25, -777


def guarded(rows, width, dtype, sentinel):
    raw = torch.full((rows + 2 * GUARD, width), sentinel, dtype=dtype, device="cuda")
    return raw, raw[GUARD:GUARD + rows]


def buffers(B, K, names):
    """name -> (raw, view): "boxes" [B*K, 4] and "scores" [B*K, 1] float32, "counts" [B, 1] int32, every other name [B*K, 1] int32"""
    shape = {"boxes": (B * K, 4, torch.float32, SENT_F), "scores": (B * K, 1, torch.float32, SENT_F), "counts": (B, 1, torch.int32, SENT_I)}
    return {k: guarded(*shape.get(k, (B * K, 1, torch.int32, SENT_I))) for k in names}


def untouched(bufs, inside=False):
    """the guard rows -- with `inside` the outputs between them as well -- still hold the sentinel"""
    for k, (raw, view) in bufs.items():
        sent = SENT_F if raw.dtype == torch.float32 else SENT_I
        part = raw if inside else torch.cat([raw[:GUARD], raw[GUARD + view.shape[0]:]])
        assert bool((part == sent).all()), f"{'outputs' if inside else 'guard rows'} of {k} written"


def shaped(bufs, B, K):
    """the outputs as numpy arrays: "counts" [B], "boxes" [B, K, 4], every other name [B, K]"""
    out = {k: view.cpu().numpy() for k, (raw, view) in bufs.items()}
    return {k: v.reshape(B) if k == "counts" else v.reshape(B, K, 4) if k == "boxes" else v.reshape(B, K) for k, v in out.items()}


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)
