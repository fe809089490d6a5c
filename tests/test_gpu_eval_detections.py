"""`-m gpu`: `COCOEvaluator.add_detections` / `.confusion_matrix` (dod_coco_eval_append_detections / dod_coco_eval_confusion in
csrc/cocoeval.hip) and `validate_coco(detect=...)` against the yardsticks of tests/eval_detections_cases.py and the COCOeval
restatement of tests/cocoeval_ref.py.  The device performs the same double operations on the same values in the same order, so
`precision`, `recall` and every cell of the confusion matrix are compared EXACTLY; the 12 means within test_gpu_cocoeval's
STATS_TOL (summation order)."""
import functools

import numpy as np
import pytest
import torch

from tests import cocoeval_ref as ref
from tests import eval_detections_cases as edc
from tests.test_gpu_cocoeval import SCENES, STATS_TOL

pytestmark = pytest.mark.gpu
IDS = ["seed%d" % s["seed"] for s in SCENES]
POINTS = [(-np.inf, 0.5), (0.25, 0.5), (0.5, float(ref.IOU_THRS[5]))]
KEYS = ("boxes", "scores", "labels", "counts")


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import cocoeval
    return cocoeval


@functools.lru_cache(maxsize=None)
def _scene(n, pad="nan"):
    """(dataset, packed arrays, the records they stand for, the restatement's evaluation of those records): computed once, read only"""
    ds, res = ref.make_scene(**SCENES[n])
    per_image = {}
    for r in res:
        per_image[r["image_id"]] = per_image.get(r["image_id"], 0) + 1
    d = edc.scene_to_detections(ds, res, max(per_image.values()) + 3, pad)
    rec = edc.detections_to_records(*(d[k] for k in KEYS), d["image_ids"], d["category_ids"])
    return ds, d, rec, ref.evaluate(ds, rec)


def _result(d, b0=0, b1=None):
    """images b0 .. b1-1 of the packed arrays as a postprocess.Detections of CUDA tensors, and their ids"""
    from dinov2_od_amd.postprocess import Detections
    t = {k: torch.from_numpy(np.ascontiguousarray(d[k][b0:b1])).cuda() for k in KEYS}
    return Detections(t["scores"], t["labels"], t["boxes"], torch.full_like(t["labels"], -1), t["counts"]), d["image_ids"][b0:b1].tolist()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check_against_ref(out, want):
    assert _same_bits(out["precision"], want["precision"])
    assert _same_bits(out["recall"], want["recall"])
    err = np.abs(np.array(out["stats"]) - np.array(want["stats"])).max()
    print("max |stats - restatement| =", err)
    assert err <= STATS_TOL


def _check_order(ev, ds, rec, want):
    """matches()['index'] are positions in append order: per (category, image) group they must be the restatement's, whose
    positions are those of the record list"""
    m = ev.matches()
    ann = ev.ann
    img = np.searchsorted(ann.image_ids, [rec[i]["image_id"] for i in m["index"]])
    cat = np.searchsorted(ann.category_ids, [rec[i]["category_id"] for i in m["index"]])
    got = {}
    for j in np.nonzero(m["rank"] < 100)[0]:
        got.setdefault((int(cat[j]), int(img[j])), []).append(int(m["index"][j]))
    assert got == {k: g["dt_index"].tolist() for k, g in want["groups"].items() if len(g["dt_index"])}


# ------------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("n", range(len(SCENES)), ids=IDS)
def test_add_detections_equals_the_record_list(ce, n):
    ds, d, rec, want = _scene(n)
    table = d["category_ids"].tolist()
    B = len(d["counts"])
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    ev.add_detections(*_result(d), table)
    _check_against_ref(ev.evaluate(), want)
    _check_order(ev, ds, rec, want)
    two = ce.COCOEvaluator(ds, max_detections=len(rec))                                       # exactly full
    for b0, b1 in ((0, B // 2), (B // 2, B)):                                                 # the second call starts at a non-zero base
        res, ids = _result(d, b0, b1)
        two.add_detections(res, torch.tensor(ids), torch.tensor(table, device="cuda"))
    _check_against_ref(two.evaluate(), want)
    _check_order(two, ds, rec, want)
    mixed = ce.COCOEvaluator(ds, max_detections=4096)
    first = int(d["counts"][: B // 2].sum())
    mixed.add_records(rec[:first])
    mixed.add_detections(*_result(d, B // 2, B), table)
    _check_against_ref(mixed.evaluate(), want)
    _check_order(mixed, ds, rec, want)


def test_smallest_shape_empty_batch_and_a_full_image(ce):
    one = {"images": [{"id": 9}], "categories": [{"id": 4}],
           "annotations": [{"id": 1, "image_id": 9, "category_id": 4, "bbox": [10.0, 10.0, 20.0, 20.0], "area": 400.0, "iscrowd": 0}]}
    d = edc.scene_to_detections(one, [{"image_id": 9, "category_id": 4, "bbox": [11.0, 9.0, 20.0, 21.0], "score": 0.5}], 1)      # B = 1, Kd = 1
    rec = edc.detections_to_records(*(d[k] for k in KEYS), d["image_ids"], d["category_ids"])
    ev = ce.COCOEvaluator(one, max_detections=1)
    ev.add_detections(*_result(d), d["category_ids"])
    _check_against_ref(ev.evaluate(), ref.evaluate(one, rec))
    assert ev.confusion_matrix(0.25, 0.5).tolist() == edc.confusion_ref(one, rec, 0.25, 0.5).tolist() == [[1, 0], [0, 0]]
    ds, full, rec, want = _scene(2)
    empty = dict(full, counts=np.zeros_like(full["counts"]))                                  # every row is padding
    ev = ce.COCOEvaluator(ds, max_detections=64)
    ev.add_detections(*_result(empty), full["category_ids"])
    _check_against_ref(ev.evaluate(), ref.evaluate(ds, []))
    assert np.array_equal(ev.confusion_matrix(-np.inf, 0.5), edc.confusion_ref(ds, [], -np.inf, 0.5))
    kd = int(full["counts"].max())                                                            # one image fills its Kd rows
    tight = {k: (full[k][:, :kd] if k != "counts" else full[k]) for k in KEYS}
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    ev.add_detections(*_result(dict(full, **tight)), full["category_ids"])
    _check_against_ref(ev.evaluate(), want)


def test_nan_padding_changes_nothing_against_zero_padding(ce):
    ds, d, rec, want = _scene(0)
    _, z, zrec, _ = _scene(0, "zero")
    assert np.isnan(d["boxes"]).any() and not np.isnan(z["boxes"]).any() and zrec == rec
    outs = []
    for arrays in (d, z):
        ev = ce.COCOEvaluator(ds, max_detections=4096)
        ev.add_detections(*_result(arrays), arrays["category_ids"])
        outs.append((ev.evaluate(), ev.confusion_matrix(0.25, 0.5), ev.matches()))
    (a, ca, ma), (b, cb, mb) = outs
    assert _same_bits(a["precision"], b["precision"]) and _same_bits(a["recall"], b["recall"]) and a["stats"] == b["stats"]
    assert np.array_equal(ca, cb) and all(np.array_equal(ma[k], mb[k]) for k in ma)
    _check_against_ref(a, want)


# ------------------------------------------------------------------------------------------------ errors
def test_bad_labels_counts_and_overflow_raise_at_evaluate_and_reset_clears_them(ce):
    ds, d, rec, want = _scene(2)
    table = d["category_ids"]
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    b = int(np.argmax(d["counts"]))
    for lab in (len(table), -1):                                                              # a label outside the table, in a valid row
        bad = dict(d, labels=d["labels"].copy())
        bad["labels"][b, 0] = lab
        ev.add_detections(*_result(bad), table)
        with pytest.raises(ValueError, match="label"):
            ev.evaluate()
        with pytest.raises(ValueError, match="label"):
            ev.confusion_matrix()
        ev.reset()
    ev.add_detections(*_result(bad))                                                          # without a table any label is an id
    ev.evaluate()
    ev.reset()
    for c in (d["boxes"].shape[1] + 1, -2):                                                   # counts outside [0, Kd]
        bad = dict(d, counts=d["counts"].copy())
        bad["counts"][b] = c
        ev.add_detections(*_result(bad), table)
        with pytest.raises(ValueError, match="truncated"):
            ev.evaluate()
        with pytest.raises(ValueError, match="truncated"):
            ev.confusion_matrix()
        ev.reset()
    ev.add_detections(*_result(d), table)                                                     # reset cleared both bits
    _check_against_ref(ev.evaluate(), want)
    small = ce.COCOEvaluator(ds, max_detections=len(rec) - 1)                                  # one row too many: not written, but counted
    small.add_detections(*_result(d), table)
    with pytest.raises(ValueError, match="max_dets"):
        small.evaluate()
    with pytest.raises(ValueError, match="max_dets"):
        small.confusion_matrix()
    small.reset()
    res, ids = _result(d, 0, 1)
    small.add_detections(res, ids, table)
    small.evaluate()
    with pytest.raises(ValueError, match="image id"):
        other = ce.COCOEvaluator(ds, max_detections=4096)
        other.add_detections(res, [max(d["image_ids"].tolist()) + 1], table)
        other.confusion_matrix()


def test_entry_points_refuse_null_and_short_arguments(ce):
    from dinov2_od_amd import _native as nat
    L = nat.lib()
    ds, d, _, _ = _scene(2)
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    res, ids = _result(d)
    B, Kd = res.scores.shape
    ids_t = torch.tensor(ids, device="cuda")
    table = torch.from_numpy(d["category_ids"]).cuda()
    head = [nat.ptr(ev._ws), ev._ws.numel(), ev.max_detections, ev.I, ev.K, ev.G]
    good = [nat.ptr(res.boxes), nat.ptr(res.scores), nat.ptr(res.labels), nat.ptr(res.counts), B, Kd, nat.ptr(ids_t), nat.ptr(table), table.numel()]

    def append(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.dod_coco_eval_append_detections(*head, *a, nat.stream_ptr())
    for i in (0, 1, 2, 3, 6):
        assert append(**{f"a{i}": None}) == 1 and b"null" in L.dod_last_error(None), i
    assert append(a4=0) == 1 and append(a4=-3) == 1 and append(a4=(1 << 16) + 1) == 1 and append(a5=0) == 1
    assert append(a8=0) == 1 and append(a8=-1) == 1 and b"map" in L.dod_last_error(None)
    short = [nat.ptr(ev._ws), ev._ws.numel() - 1] + head[2:]
    assert L.dod_coco_eval_append_detections(*short, *good, nat.stream_ptr()) == 3
    m = torch.zeros((ev.K + 1, ev.K + 1), dtype=torch.int64, device="cuda")
    conf = L.dod_coco_eval_confusion
    assert conf(*head, 0.25, 0.5, None, nat.stream_ptr()) == 1 and b"null" in L.dod_last_error(None)
    assert conf(*head, float("nan"), 0.5, nat.ptr(m), nat.stream_ptr()) == 1 and conf(*head, 0.25, float("nan"), nat.ptr(m), nat.stream_ptr()) == 1
    assert conf(*short, 0.25, 0.5, nat.ptr(m), nat.stream_ptr()) == 3
    torch.cuda.synchronize()
    assert int(m.sum()) == 0                                                                  # nothing ran
    assert append() == 0 and append(a7=None, a8=0) == 0 and conf(*head, 0.25, 0.5, nat.ptr(m), nat.stream_ptr()) == 0
    with pytest.raises(ValueError, match="1024"):                                             # the limit, before any launch
        big = dict(ds, annotations=[dict(ds["annotations"][0], id=10 ** 6 + n, category_id=ds["categories"][n % 2]["id"], iscrowd=0) for n in range(1100)])
        ce.COCOEvaluator(big, max_detections=8).confusion_matrix()


# ------------------------------------------------------------------------------------------------ confusion matrix
@pytest.mark.parametrize("n", range(len(SCENES)), ids=IDS)
def test_confusion_matrix_equals_the_restatement_before_and_after_evaluate(ce, n):
    ds, d, rec, want = _scene(n)
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    ev.add_detections(*_result(d), d["category_ids"])
    refs = [edc.confusion_ref(ds, rec, s, t) for s, t in POINTS]
    assert all(np.trace(r[:-1, :-1]) > 0 and r[-1].sum() > 0 and r[:, -1].sum() > 0 for r in refs)      # matched, missed and left over
    for (s, t), r in zip(POINTS, refs):                                                       # needs no evaluate before it
        got = ev.confusion_matrix(s, t)
        assert got.dtype == np.int64 and np.array_equal(got, r), (s, t)
    _check_against_ref(ev.evaluate(), want)                                                   # ... and leaves a later one alone
    before = ev.matches()
    for (s, t), r in zip(POINTS, refs):
        assert np.array_equal(ev.confusion_matrix(s, t), r), (s, t)
    after = ev.matches()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    _check_against_ref(ev.evaluate(), want)


def _crowded_image(seed, n_extra):
    """scene 1 with n_extra more ground truths of random categories on one image and a jittered detection, tied scores among them, for
    each: more ground truths than a wave has lanes (and, past 256, than the workgroup has threads), more candidates than one chunk"""
    ds, res = ref.make_scene(**SCENES[1])
    rng = np.random.default_rng(seed)
    img = res[0]["image_id"]
    cats = [c["id"] for c in ds["categories"]]
    anns, dts = [], []
    for n in range(n_extra):
        x, y, w, h = (float(v) for v in np.concatenate([rng.uniform(0, 500, 2), rng.uniform(8, 90, 2)]))
        anns.append({"id": 10 ** 6 + n, "image_id": img, "category_id": cats[int(rng.integers(len(cats)))], "bbox": [x, y, w, h], "area": w * h,
                     "iscrowd": int(n % 37 == 0)})
        j = rng.normal(0, 0.1, 4) * [w, h, w, h]
        dts.append({"image_id": img, "category_id": cats[int(rng.integers(len(cats)))], "bbox": [float(np.float32(v)) for v in (x + j[0], y + j[1], w + j[2], h + j[3])],
                    "score": float(np.float32(rng.choice([0.25, 0.5, 0.75, rng.uniform(0.05, 1)])))})
    return dict(ds, annotations=ds["annotations"] + anns), res + dts


@pytest.mark.parametrize("n_extra", [70, 300])
def test_confusion_matrix_with_more_ground_truths_than_lanes_and_threads(ce, n_extra):
    ds, res = _crowded_image(n_extra, n_extra)
    d = edc.scene_to_detections(ds, res, 520)
    rec = edc.detections_to_records(*(d[k] for k in KEYS), d["image_ids"], d["category_ids"])
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    assert ev.max_gt_per_image > (64 if n_extra == 70 else 256) and int(d["counts"].max()) > (64 if n_extra == 70 else 256)
    ev.add_detections(*_result(d), d["category_ids"])
    wants = [edc.confusion_ref(ds, rec, s, t) for s, t in POINTS]
    assert wants[0][:-1, :-1].sum() - np.trace(wants[0][:-1, :-1]) > n_extra // 2 and all(w[-1].sum() > 0 and w[:, -1].sum() > 0 for w in wants)
    for (s, t), want in zip(POINTS, wants):
        assert np.array_equal(ev.confusion_matrix(s, t), want), (s, t)


def test_confusion_matrix_ties_go_to_the_later_ground_truth(ce):
    """identical ground-truth boxes: every IoU of a candidate ties, so the cells say which ground truth each one took.  70 copies
    spread the tie over two waves; the copies' categories cycle, so taking an earlier one instead would move counts between columns"""
    cats = [3, 5, 8]
    box = [20.0, 30.0, 40.0, 50.0]
    anns = [{"id": n + 1, "image_id": 1, "category_id": cats[n % 3], "bbox": box, "area": 2000.0, "iscrowd": 0} for n in range(70)]
    anns += [{"id": 100 + n, "image_id": 2, "category_id": cats[(2 * n) % 3], "bbox": box, "area": 2000.0, "iscrowd": 0} for n in range(4)]
    ds = {"images": [{"id": 1}, {"id": 2}], "categories": [{"id": c} for c in cats], "annotations": anns}
    res = [{"image_id": 1, "category_id": 5, "bbox": [20.0, 30.0, 40.0, 48.0 - n % 2], "score": 0.5} for n in range(9)]      # tied scores too
    res += [{"image_id": 2, "category_id": cats[n % 3], "bbox": box, "score": 0.9 - 0.1 * n} for n in range(6)]           # two more than ground truths
    d = edc.scene_to_detections(ds, res, 12)
    rec = edc.detections_to_records(*(d[k] for k in KEYS), d["image_ids"], d["category_ids"])
    ev = ce.COCOEvaluator(ds, max_detections=32)
    ev.add_detections(*_result(d), d["category_ids"])
    want = edc.confusion_ref(ds, rec, 0.25, 0.5)
    # image 1: ground truths by category 24 of 3, 23 of 5, 23 of 8; the nine candidates of category 5 take the last nine, all of category 8.
    # image 2: ground truths 3, 3, 5, 8; the candidates 3, 5, 8, 3, 5, 8 by score take 8, 5, the second 3, the first 3, nothing, nothing.
    assert want.tolist() == [[1, 0, 1, 0], [0, 1, 9, 1], [1, 0, 0, 1], [24, 23, 14, 0]]
    assert np.array_equal(ev.confusion_matrix(0.25, 0.5), want)
    assert np.array_equal(ev.confusion_matrix(0.25, 1.0), edc.confusion_ref(ds, rec, 0.25, 1.0))      # the 1 - 1e-10 cap: IoU 1 still matches


# ------------------------------------------------------------------------------------------------ validate_coco(detect=...)
def test_validate_coco_detect_equals_the_host_route(ce):
    """model.detect -> add_detections inside validate_coco == model.detect -> detections_to_list -> dict records on the host ->
    add_records; and validate_coco without a new keyword is what it was: the packed route of the normalised records"""
    from dinov2_od_amd.postprocess import detections_to_list, evaluate_coco
    from tests import cases, gpu_util as G
    m = G.make_detector(cases.micro_bb(), cases.dec_cfg(True), "bf16x3")
    rng = np.random.default_rng(31)
    ids = [int(v) for v in rng.choice(np.arange(1, 900), 4, replace=False)]
    sizes = [(480, 640), (333, 500), None, (56, 70)]
    targets = [dict({"image_id": i}, **({} if s is None else {"orig_size": torch.tensor(s)})) for i, s in zip(ids, sizes)]
    loader = [(torch.from_numpy(rng.uniform(0, 1, (2, 3, 56, 70)).astype(np.float32)), targets[b: b + 2]) for b in (0, 2)]
    kw = dict(top_k=20, threshold=0.05, nms_iou=0.6)
    table = [0] + [3 * c + 2 for c in range(1, 11)]                                           # label -> category id
    records = []
    for images, tg in loader:
        r = m.detect(images.cuda(), sizes=[tuple(float(v) for v in t["orig_size"]) if "orig_size" in t else (56.0, 70.0) for t in tg], **kw)
        for t, one in zip(tg, detections_to_list(r)):
            for box, score, label in zip(one["boxes"].cpu().numpy(), one["scores"].cpu().numpy(), one["labels"].cpu().numpy()):
                x1, y1, x2, y2 = (float(v) for v in box)
                records.append({"image_id": t["image_id"], "category_id": table[int(label)], "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(score)})
    assert len(records) > 20
    anns = [{"id": n + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": [v * s for v, s in zip(r["bbox"], (1.0, 1.0, 0.9, 1.1))],
             "area": r["bbox"][2] * r["bbox"][3], "iscrowd": 0} for n, r in enumerate(records[::3])]
    ds = {"images": [{"id": i} for i in ids], "categories": [{"id": c} for c in table[1:]], "annotations": anns}
    host = ce.COCOEvaluator(ds, max_detections=len(records))
    host.add_records(records)
    want = host.evaluate()
    got = ce.validate_coco(m, loader, G.dev(), ds, detect=kw, category_ids=table)
    assert _same_bits(got["precision"], want["precision"]) and _same_bits(got["recall"], want["recall"]) and got["stats"] == want["stats"]
    assert {k: got[k] for k in ce.METRIC_KEYS} == ce.metrics_from_stats(want["stats"]) and got["AP"] > 0.0
    _check_against_ref(got, ref.evaluate(ds, records))
    per = ce.per_category_metrics(got, ds)
    assert set(per) == set(table[1:]) and max(v["AP"] for v in per.values()) > 0.0
    old = ce.validate_coco(m, loader, G.dev(), ds)                                             # no new keyword: today's answer
    assert set(old) == set(ce.METRIC_KEYS) | {"stats"}
    assert {k: old[k] for k in ce.METRIC_KEYS} == ce.compute_coco_metrics(evaluate_coco(m, loader, G.dev()), ds)


def test_validate_coco_sliced_fused_equals_the_host_route(ce):
    """sliced=dict(..., merge="fuse"): raw ragged uint8 images -> model.detect_sliced -> FusedDetections -> add_detections, against the
    same call's rows carried through detections_to_list and dict records; without category_ids the label is the id"""
    from dinov2_od_amd import slicing
    from dinov2_od_amd.postprocess import detections_to_list
    from tests import augment_cases as ac, cases, gpu_util as G
    bb, dcfg = cases.cfg1(25)
    m = G.make_detector(bb, dcfg, "bf16x3", "facebook/dinov2-small")
    imgs = [ac._rand(s, 140 + i) for i, s in enumerate([(300, 420), (150, 180), (333, 500)])]
    ids = [41, 7, 19]
    loader = [(imgs[:2], [{"image_id": i} for i in ids[:2]]), (imgs[2:], [{"image_id": ids[2]}])]
    kw = dict(size=(224, 224), tile=200, overlap=0.2, full_view=True, flip=True, top_k=60, threshold=-1.0, nms_iou=0.5, edge_margin=4.0, merge="fuse")
    records = []
    for batch, tg in loader:
        r = m.detect_sliced(batch, **kw)
        assert isinstance(r, slicing.FusedDetections)
        for t, one in zip(tg, detections_to_list(r)):
            for box, score, label in zip(one["boxes"].cpu().numpy(), one["scores"].cpu().numpy(), one["labels"].cpu().numpy()):
                x1, y1, x2, y2 = (float(v) for v in box)
                records.append({"image_id": t["image_id"], "category_id": int(label), "bbox": [x1, y1, x2 - x1, y2 - y1], "score": float(score)})
    assert len(records) > 30
    anns = [{"id": n + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": [v * s for v, s in zip(r["bbox"], (1.0, 1.0, 0.9, 1.1))],
             "area": r["bbox"][2] * r["bbox"][3], "iscrowd": 0} for n, r in enumerate(records[::4])]
    ds = {"images": [{"id": i} for i in ids], "categories": [{"id": c} for c in range(1, 91)], "annotations": anns}
    host = ce.COCOEvaluator(ds, max_detections=len(records))
    host.add_records(records)
    want = host.evaluate()
    got = ce.validate_coco(m, loader, G.dev(), ds, sliced=kw, max_detections=4096)
    assert _same_bits(got["precision"], want["precision"]) and _same_bits(got["recall"], want["recall"]) and got["stats"] == want["stats"]
    assert got["AP"] > 0.0
    with pytest.raises(ValueError):
        ce.validate_coco(m, loader, G.dev(), ds, sliced=kw, detect=dict(top_k=5))
