"""CPU-side checks of the detection-output evaluation: the yardsticks of tests/eval_detections_cases.py against the COCOeval
restatement (tests/cocoeval_ref.py) and against properties that follow from the definition, `per_category_metrics`, and the
argument errors of the new Python entry points that need no GPU.  The device code is compared with these yardsticks in
tests/test_gpu_eval_detections.py."""
import numpy as np
import pytest
import torch

from tests import cocoeval_ref as ref
from tests import eval_detections_cases as edc


@pytest.fixture(scope="module")
def ce():
    from dinov2_od_amd import cocoeval
    return cocoeval


@pytest.fixture(scope="module")
def scene0():
    ds, res = ref.make_scene(0)
    return ds, res, ref.evaluate(ds, res)


def _valid_mean(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def test_per_category_metrics_relate_to_the_summary_as_the_definition_implies(ce, scene0):
    """stats[0] / [1] / [8] are means over ALL valid entries, so they are the per-category means weighted by each category's number
    of valid entries (counted from the arrays) -- not the plain mean of the per-category values, which counts a category without
    ground truth as -1"""
    ds, _, want = scene0
    per = ce.per_category_metrics(want, ds)
    cats = sorted(c["id"] for c in ds["categories"])
    assert list(per) == cats and all(set(v) == {"AP", "AP50", "AR100"} and all(type(x) is float for x in v.values()) for v in per.values())
    prec, rec = want["precision"], want["recall"]
    slices = {"AP": lambda k: prec[:, :, k, 0, 2], "AP50": lambda k: prec[0, :, k, 0, 2], "AR100": lambda k: rec[:, k, 0, 2]}
    for name, stat in (("AP", 0), ("AP50", 1), ("AR100", 8)):
        n = np.array([np.count_nonzero(slices[name](k) > -1) for k in range(len(cats))])
        v = np.array([per[c][name] for c in cats])
        for k, c in enumerate(cats):
            assert per[c][name] == _valid_mean(slices[name](k))
        assert ((n == 0) == (v == -1.0)).all() and (n == 0).any() and (n > 0).sum() >= 2
        weighted = float((v[n > 0] * n[n > 0]).sum() / n.sum())
        assert abs(weighted - want["stats"][stat]) <= 1e-12, name
    with pytest.raises(ValueError):
        ce.per_category_metrics({"precision": prec[:, :, :-1], "recall": rec[:, :-1]}, ds)


def _one_category_scene():
    """make_scene(5, crowded=False) reduced to one category that has ground truth, at most 100 detections per image"""
    ds, res = ref.make_scene(seed=5, crowded=False)
    cats = sorted(c["id"] for c in ds["categories"])
    n_gt = {c: sum(a["category_id"] == c for a in ds["annotations"]) for c in cats}
    n_dt = {c: sum(r["category_id"] == c for r in res) for c in cats}
    cat = max(cats, key=lambda c: (min(n_gt[c], n_dt[c]), c))
    assert not any(a.get("iscrowd", 0) for a in ds["annotations"])
    per_image, kept = {}, []
    for r in res:
        if r["category_id"] == cat and per_image.get(r["image_id"], 0) < 100:
            per_image[r["image_id"]] = per_image.get(r["image_id"], 0) + 1
            kept.append(r)
    return dict(ds, annotations=[a for a in ds["annotations"] if a["category_id"] == cat]), kept, cats.index(cat)


@pytest.mark.parametrize("t", [0, 5])
def test_confusion_ref_equals_coco_matching_on_a_one_category_scene(t):
    """without crowds, for area range 'all' and at most 100 detections per image, evaluateImg's greedy loop IS the confusion match of
    a one-category scene: the diagonal cell, the unmatched and the missed counts follow from the restatement's own decisions"""
    ds, res, k = _one_category_scene()
    want = ref.evaluate(ds, res)
    K = len(ds["categories"])
    groups = {key: g for key, g in want["groups"].items() if key[0] == k}
    matched = sum(int(g["matched"][0, t].sum()) for g in groups.values() if len(g["dt_index"]))
    n_dt = sum(len(g["dt_index"]) for g in groups.values())
    npig = sum(int(g["npig"][0]) for g in groups.values())
    assert n_dt == len(res) and npig == len(ds["annotations"])
    assert matched > 0 and n_dt - matched > 0 and npig - matched > 0           # all three outcomes occur, or this shows nothing
    M = edc.confusion_ref(ds, res, -np.inf, float(ref.IOU_THRS[t]))
    assert M[k, k] == matched and M[k, K] == n_dt - matched and M[K, k] == npig - matched
    assert M.sum() == M[k, k] + M[k, K] + M[K, k]


@pytest.mark.parametrize("scene", [dict(seed=0), dict(seed=1, n_images=16, n_cats=8), dict(seed=2, n_images=7, n_cats=4)], ids=lambda s: "seed%d" % s["seed"])
def test_confusion_ref_structure_on_multi_class_scenes(scene):
    ds, res = ref.make_scene(**scene)
    cats = {c["id"] for c in ds["categories"]}
    K = len(cats)
    N = sum(1 for a in ds["annotations"] if not a.get("iscrowd", 0))
    rows_before = None
    for thr in (-np.inf, 0.25, 0.5, 0.75):
        M = edc.confusion_ref(ds, res, thr, 0.5)
        cand = sum(1 for r in res if r["category_id"] in cats and r["score"] >= thr)
        assert M.dtype == np.int64 and M.shape == (K + 1, K + 1) and (M >= 0).all()
        assert M[:K].sum() == cand and M[:, :K].sum() == N and M[K, K] == 0
        rows = M[:K].sum(1)
        assert rows_before is None or (rows <= rows_before).all()               # a higher score threshold never adds a candidate
        rows_before = rows
    assert np.trace(edc.confusion_ref(ds, res, -np.inf, 0.5)[:K, :K]) > 0       # and something does match


def test_scene_packing_round_trips_and_pads():
    ds, res = ref.make_scene(2, n_images=7, n_cats=4)
    d = edc.scene_to_detections(ds, res, 200)
    assert d["image_ids"].tolist() == [im["id"] for im in ds["images"]] and int(d["counts"].sum()) == len(res)
    assert d["category_ids"][0] not in {r["category_id"] for r in res}
    rec = edc.detections_to_records(d["boxes"], d["scores"], d["labels"], d["counts"], d["image_ids"], d["category_ids"])
    by_image = sorted(range(len(res)), key=lambda n: d["image_ids"].tolist().index(res[n]["image_id"]))      # stable: list order inside an image
    assert [(r["image_id"], r["category_id"], r["score"]) for r in rec] == [(res[n]["image_id"], res[n]["category_id"], res[n]["score"]) for n in by_image]
    assert all(a["bbox"][:2] == res[n]["bbox"][:2] and abs(a["bbox"][2] - res[n]["bbox"][2]) <= 1e-4 for a, n in zip(rec, by_image))
    for b, n in enumerate(d["counts"]):
        assert np.isnan(d["boxes"][b, n:]).all() and np.isnan(d["scores"][b, n:]).all() and (d["labels"][b, n:] == -1).all()
        assert np.isfinite(d["boxes"][b, :n]).all() and (d["labels"][b, :n] > 0).all()
    with pytest.raises(ValueError):
        edc.scene_to_detections(ds, res, 3)


# ------------------------------------------------------------------------------------------------ argument errors, no GPU
def _cpu_result(B=2, Kd=3):
    from dinov2_od_amd.postprocess import Detections
    return Detections(torch.zeros(B, Kd), torch.zeros(B, Kd, dtype=torch.int32), torch.zeros(B, Kd, 4), torch.zeros(B, Kd, dtype=torch.int32),
                      torch.zeros(B, dtype=torch.int32))


def test_check_detections_raises_value_error_before_the_device_is_looked_at(ce):
    r = _cpu_result()
    bad = [
        (object(), [1, 2], None),                                             # not a Detections
        (r._replace(scores=r.scores.double()), [1, 2], None),
        (r._replace(scores=torch.zeros(2, 0)), [1, 2], None),                 # Kd < 1
        (r._replace(labels=r.labels.long()), [1, 2], None),
        (r._replace(labels=r.labels[:, :2]), [1, 2], None),
        (r._replace(boxes=torch.zeros(2, 3, 5)), [1, 2], None),
        (r._replace(counts=torch.zeros(3, dtype=torch.int32)), [1, 2], None),
        (r._replace(counts=r.counts.float()), [1, 2], None),
        (r, [1], None),                                                       # one id per image
        (r, torch.tensor([1, 2, 3]), None),
        (r, torch.tensor([1.0, 2.0]), None),
        (r, torch.tensor([[1, 2]]), None),
        (r, 7, None),
        (r, [1, 2], []),                                                      # an empty table
        (r, [1, 2], torch.zeros(0, dtype=torch.int64)),
        (r, [1, 2], torch.zeros(2, 2, dtype=torch.int64)),
    ]
    for n, (res, ids, table) in enumerate(bad):
        with pytest.raises(ValueError) as e:
            ce.check_detections(res, ids, table)
        assert "CUDA" not in str(e.value), n                                  # the argument's own message, not the device's
    for ids, table in (([1, 2], None), (torch.tensor([1, 2]), [5, 6, 7]), ((1, 2), torch.tensor([5, 6], dtype=torch.int32))):
        with pytest.raises(ValueError, match="CUDA"):                         # all arguments fine: only now the device
            ce.check_detections(r, ids, table)


def test_confusion_limits_and_per_image_counts(ce):
    ds, _ = ref.make_scene(3)
    ann = ce.load_annotations(ds)
    imgs = sorted(im["id"] for im in ds["images"])
    cats = {c["id"] for c in ds["categories"]}
    want = [sum(1 for a in ds["annotations"] if a["image_id"] == i and a["category_id"] in cats and not a.get("iscrowd", 0)) for i in imgs]
    assert ann.gt_per_image().tolist() == want and any(a.get("iscrowd", 0) for a in ds["annotations"])
    ce.check_confusion_limits(2048, 1024)
    with pytest.raises(ValueError, match="2048"):
        ce.check_confusion_limits(2049, 5)
    with pytest.raises(ValueError, match="1024"):
        ce.check_confusion_limits(80, 1025)
    many = [dict(ds["annotations"][0], id=10 ** 6 + n, category_id=sorted(cats)[n % 2], iscrowd=0) for n in range(1100)]
    big = ce.load_annotations(dict(ds, annotations=many))                     # 550 per (image, category) group: the evaluator takes it
    with pytest.raises(ValueError, match="1024"):
        ce.check_confusion_limits(len(cats), int(big.gt_per_image().max()))


def test_entry_points_return_invalid_before_any_hip_call():
    """a NULL required pointer, B or Kd < 1, an empty map, a NULL matrix, a NaN threshold, K past 2048: DOD_ERR_INVALID with a message
    (no GPU here: a HIP call would be DOD_ERR_HIP).  `p` stands in for device pointers that are never dereferenced"""
    import ctypes as C
    from dinov2_od_amd import _native as nat
    L = nat.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 40
    head = [p, big, 16, 2, 3, 5]
    good = [p, p, p, p, 2, 4, p, p, 7]
    for i, v in [(0, None), (1, None), (2, None), (3, None), (6, None), (4, 0), (4, -1), (4, (1 << 16) + 1), (5, 0), (8, 0), (8, -2)]:
        a = list(good)
        a[i] = v
        assert L.dod_coco_eval_append_detections(*head, *a, None) == 1 and b"coco_eval_append_detections" in L.dod_last_error(None), (i, v)
    assert L.dod_coco_eval_append_detections(p, 16, *head[2:], *good, None) == 3                 # a short workspace: DOD_ERR_STATE
    conf = L.dod_coco_eval_confusion
    assert conf(*head, 0.25, 0.5, None, None) == 1 and b"null" in L.dod_last_error(None)
    assert conf(*head, float("nan"), 0.5, p, None) == 1 and conf(*head, 0.25, float("nan"), p, None) == 1 and b"NaN" in L.dod_last_error(None)
    assert conf(p, big, 16, 2, 2049, 5, 0.25, 0.5, p, None) == 1 and b"2048" in L.dod_last_error(None)
    assert conf(p, 16, *head[2:], 0.25, 0.5, p, None) == 3
    n0, n1 = (L.dod_coco_eval_workspace_bytes(16, i, 3, 5) for i in (2, 1002))
    assert n1 - n0 >= 4000 and n0 > 0                                          # the per-image lists are part of the workspace


def test_validate_coco_refuses_contradicting_keywords_before_anything_runs(ce):
    ds, _ = ref.make_scene(3)

    class Never:
        def __getattr__(self, name):
            raise AssertionError("the model must not be touched")
    for kw in (dict(detect={}, sliced={}), dict(category_ids=[1, 2]), dict(detect=[("top_k", 5)]), dict(sliced=5),
               dict(detect=dict(sizes=(2, 2))), dict(detect={}, category_ids=[]), dict(sliced={}, category_ids=torch.zeros(2, 2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ce.validate_coco(Never(), [], "cuda", ds, **kw)
