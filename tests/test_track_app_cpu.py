"""CPU-side checks of the appearance association (dod_track_update_app, dod_track_embed_commit, include/dinodet.h) on its numpy + scipy
restatement (tests/track_app_cases.py): with the gates closed it is the plain tracker's restatement bit for bit, the committed swap scene
switches ids without appearance and never with it, and the committed seeds reach every gate.  No GPU compute."""
import numpy as np

from tests import track_app_cases as ta
from tests import track_cases as tc

VIEW = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.uint32}


def _bits(a):
    return a.view(VIEW[a.dtype]) if a.dtype in VIEW else a


def _embs(frames, D, seed):
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        e = rng.normal(size=f[0].shape + (D,))
        out.append((e / np.linalg.norm(e, axis=-1, keepdims=True)).astype(np.float32))
    return out


def test_closed_gates_equal_the_plain_restatement_bit_for_bit():
    for frames, S, T in ((tc.crossing_scene(), 2, 8), (tc.random_walk_scene(), 2, 32)):
        for params in (None, dict(fuse_score=False, class_aware=True)):
            _, plain = tc.run(frames, S, T, params)
            _, slot_emb, app = ta.run_app(frames, _embs(frames, 8, 1), S, T, params, ta.CLOSED)
            for f, (p, a) in enumerate(zip(plain, app)):
                assert np.array_equal(p[0], a[0]) and np.array_equal(_bits(p[1]), _bits(a[1])), f
                for k in tc.TABLE:
                    assert np.array_equal(_bits(p[2][k]), _bits(a[3][k])), (f, k)
                ids, assoc = a[0], a[2]
                assert ((assoc >= 0) | (ids < 0)).all()                      # a row with an id has a slot
                kind, slot = assoc // ta.KIND, assoc % ta.KIND
                assert ((assoc < 0) | ((kind >= 0) & (kind <= 2) & (slot < T))).all()
                late_birth = (assoc >= 2 * ta.KIND) & (ids < 0)
                assert not late_birth.any() or int(a[3]["frame"][0]) > 1
            norms = np.linalg.norm(slot_emb.astype(np.float64), axis=-1)
            assert (np.abs(norms[norms > 0] - 1.0) < 1e-6).all()


def test_swap_scene_switches_ids_without_appearance_and_never_with_it():
    for D in (8, 260):
        frames, embs, truth = ta.swap_scene(D=D)
        _, plain = tc.run(frames, 2, 6)
        _, _, closed = ta.run_app(frames, embs, 2, 6, app=ta.CLOSED)
        _, slot_emb, app = ta.run_app(frames, embs, 2, 6)
        n_plain, n_closed, n_app = ta.id_switches(plain, truth), ta.id_switches(closed, truth), ta.id_switches(app, truth)
        print(f"D = {D}: id switches plain {n_plain}, gates closed {n_closed}, appearance {n_app}")
        assert n_plain >= 1 and n_closed == n_plain and n_app == 0
        for o, who in zip(app, truth):                                      # every object is reported at every frame, under one id
            ids = o[0]
            assert ((ids >= 0) == (who >= 0)).all()
        assert {int(i) for o in app for i in o[0][o[0] >= 0]} == {1, 2}    # and no third id was ever spent on them


def test_committed_seeds_reach_every_gate():
    """a condition on the inputs of tests/test_gpu_track_app.py: its two scenes together hit every branch of the fused cost and every kind"""
    ta.BRANCH.clear()
    frames, embs, _ = ta.swap_scene()
    ta.run_app(frames, embs, 2, 6)
    frames, embs, _ = ta.random_walk_app_scene()
    ta.run_app(frames, embs, 2, 6)
    for k in ("appearance_rejected", "proximity_rejected", "app_chosen", "base_chosen", "kind0", "kind1", "kind2"):
        assert ta.BRANCH[k] > 0, (k, dict(ta.BRANCH))


def test_commit_blends_and_normalises():
    rng = np.random.default_rng(0)
    S, T, K, D = 1, 4, 3, 8
    E = rng.normal(size=(S, T, D)).astype(np.float32)
    e = rng.normal(size=(S, K, D)).astype(np.float32)
    assoc = np.asarray([[2 + 2 * ta.KIND, 0 + 0 * ta.KIND, 1 + 1 * ta.KIND]], np.int32)
    out, touched = ta.commit(E, e, assoc, 0.9)
    assert touched.tolist() == [[False, True, True, False]]
    assert np.array_equal(out[0, 0], E[0, 0].astype(np.float64)) and np.array_equal(out[0, 3], E[0, 3].astype(np.float64))      # kind 0 and unnamed slots
    assert np.array_equal(out[0, 2], e[0, 0].astype(np.float64))                                                               # kind 2 stores
    x = np.float64(np.float32(0.9)) * E[0, 1].astype(np.float64) + (1.0 - np.float64(np.float32(0.9))) * e[0, 2].astype(np.float64)
    assert np.allclose(out[0, 1], x / np.linalg.norm(x), rtol=0, atol=1e-15) and abs(np.linalg.norm(out[0, 1]) - 1.0) < 1e-15
    zero, _ = ta.commit(np.zeros((1, 1, D), np.float32), np.zeros((1, 1, D), np.float32), np.asarray([[ta.KIND]], np.int32), 0.5)
    assert not zero.any()
