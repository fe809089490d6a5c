"""CPU-side checks of the COCO evaluator.  First the yardstick itself (tests/cocoeval_ref.py, the numpy restatement of
pycocotools' COCOeval) on cases whose answer follows by hand; then the product's host side (dinov2_od_amd/cocoeval.py:
annotation loading and grouping, input errors, record ingestion) and the C boundary's argument checks, which return before any
HIP call.  The device evaluation is compared with the restatement in tests/test_gpu_cocoeval.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests import cocoeval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tp / (fp + tp + eps) is one ulp below 1 for a perfect detector: hand values hold to rounding, not to the bit
APPROX = dict(rel=0, abs=1e-12)


def _ds(gts, images=(1,), cats=(1,)):
    """gts: (image, category, bbox, area, iscrowd) tuples"""
    return {"images": [{"id": i} for i in images], "categories": [{"id": c} for c in cats],
            "annotations": [{"id": n + 1, "image_id": i, "category_id": c, "bbox": list(b), "area": a, "iscrowd": w}
                            for n, (i, c, b, a, w) in enumerate(gts)]}


def _dt(img, cat, bbox, score):
    return {"image_id": img, "category_id": cat, "bbox": list(bbox), "score": score}


# ------------------------------------------------------------------------------------------------ the yardstick, by hand
def test_perfect_detections_give_ap_ar_one_where_gt_exists():
    boxes = {(1, 1): [10, 10, 50, 50], (1, 2): [100, 20, 40, 60], (2, 1): [5, 80, 60, 45]}      # all medium: 1024 < area < 9216
    ds = _ds([(i, c, b, float(b[2] * b[3]), 0) for (i, c), b in boxes.items()], images=(1, 2), cats=(1, 2, 3))
    out = ref.evaluate(ds, [_dt(i, c, b, 0.5) for (i, c), b in boxes.items()])
    want = [1, 1, 1, -1, 1, -1, 1, 1, 1, -1, 1, -1]
    assert out["stats"] == pytest.approx(want, **APPROX)
    assert (out["precision"][:, :, 2] == -1).all() and (out["recall"][:, 2] == -1).all()      # category 3 has no ground truth
    assert (out["precision"][:, :, :2, 1] == -1).all() and (out["precision"][:, :, :2, 3] == -1).all()


def test_tp_fp_tp_average_precision():
    ds = _ds([(1, 1, [0, 0, 50, 50], 2500.0, 0), (1, 1, [200, 200, 50, 50], 2500.0, 0)])
    dts = [_dt(1, 1, [0, 0, 50, 50], 0.9), _dt(1, 1, [400, 400, 50, 50], 0.8), _dt(1, 1, [200, 200, 50, 50], 0.7)]
    out = ref.evaluate(ds, dts)
    ap = (51 + 50 * (2 / 3)) / 101               # recall <= .5 at precision 1; recall in (.5, 1] at precision 2/3
    assert out["stats"][0] == pytest.approx(ap, **APPROX)
    assert out["stats"][1] == pytest.approx(ap, **APPROX) and out["stats"][2] == pytest.approx(ap, **APPROX)
    assert out["stats"][6] == pytest.approx(0.5, **APPROX) and out["stats"][8] == pytest.approx(1.0, **APPROX)      # AR@1, AR@100
    g = out["groups"][0, 0]
    assert g["dt_index"].tolist() == [0, 1, 2] and g["matched"][0, 0].tolist() == [True, False, True]


def test_crowd_absorbs_detections_without_false_positives():
    ds = _ds([(1, 1, [0, 0, 50, 50], 2500.0, 0), (1, 1, [100, 100, 100, 100], 10000.0, 1)])
    dts = [_dt(1, 1, [110, 110, 20, 20], 0.95), _dt(1, 1, [150, 150, 20, 20], 0.85), _dt(1, 1, [0, 0, 50, 50], 0.5)]
    out = ref.evaluate(ds, dts)
    g = out["groups"][0, 0]
    assert g["npig"].tolist() == [1, 0, 1, 0]                                   # the crowd is never counted
    assert g["matched"][0].all() and g["ignored"][0, :, :2].all() and not g["ignored"][0, :, 2].any()
    assert out["stats"][0] == pytest.approx(1.0, **APPROX)                      # both crowd hits ignored: no false positive
    ds["annotations"][1]["iscrowd"] = 0                                         # the same box as a regular object
    out = ref.evaluate(ds, dts)
    assert out["stats"][1] < 0.5 and out["groups"][0, 0]["npig"].tolist() == [2, 0, 1, 1]


def test_area_bounds_are_inclusive():
    ds = _ds([(1, 1, [0, 0, 32, 32], 1024.0, 0), (1, 2, [0, 0, 96, 96], 9216.0, 0)], cats=(1, 2))
    out = ref.evaluate(ds, [_dt(1, 1, [0, 0, 32, 32], 0.9), _dt(1, 2, [0, 0, 96, 96], 0.9)])
    assert out["groups"][0, 0]["npig"].tolist() == [1, 1, 1, 0] and out["groups"][1, 0]["npig"].tolist() == [1, 0, 1, 1]
    assert not out["groups"][0, 0]["ignored"][:3].any() and out["groups"][0, 0]["ignored"][3].all()
    assert out["stats"][3:6] == pytest.approx([1, 1, 1], **APPROX)


def test_iou_exactly_half_matches_at_the_first_threshold_only():
    assert ref.bb_iou([[0, 0, 2, 1]], [[0, 0, 2, 2]], [0])[0, 0] == 0.5
    out = ref.evaluate(_ds([(1, 1, [0, 0, 2, 2], 4.0, 0)]), [_dt(1, 1, [0, 0, 2, 1], 0.9)])
    assert out["groups"][0, 0]["matched"][0, :, 0].tolist() == [True] + [False] * 9
    assert out["stats"][1] == pytest.approx(1.0, **APPROX) and out["stats"][2] == 0.0
    assert out["stats"][0] == pytest.approx(0.1, **APPROX)


def test_scene_generator_holds_the_required_cases():
    ds, res = ref.make_scene(0)
    areas = [a["area"] for a in ds["annotations"]]
    assert 1024.0 in areas and 9216.0 in areas
    assert any(a.get("iscrowd") for a in ds["annotations"]) and any("iscrowd" not in a for a in ds["annotations"])
    groups = {}
    for r in res:
        groups.setdefault((r["image_id"], r["category_id"]), []).append(r["score"])
        assert all(v == float(np.float32(v)) for v in r["bbox"]) and r["score"] == float(np.float32(r["score"]))
    assert max(len(v) for v in groups.values()) > 100
    assert any(len(set(v)) < len(v) for v in groups.values())                   # tied scores inside a group
    gt_imgs, dt_imgs = {a["image_id"] for a in ds["annotations"]}, {r["image_id"] for r in res}
    assert gt_imgs - dt_imgs and dt_imgs - gt_imgs
    gt_cats, cats = {a["category_id"] for a in ds["annotations"]}, {c["id"] for c in ds["categories"]}
    assert len(cats - gt_cats) >= 2 and {r["category_id"] for r in res} - gt_cats
    assert any(r["bbox"] == [0.0, 0.0, 2.0, 1.0] for r in res) and any(a["bbox"] == [0.0, 0.0, 2.0, 2.0] for a in ds["annotations"])


# ------------------------------------------------------------------------------------------------ the product's host side
def test_load_annotations_groups_like_the_restatement(tmp_path):
    from dinov2_od_amd import cocoeval as ce
    ds, res = ref.make_scene(3)
    ds["annotations"].append(dict(ds["annotations"][0], id=99991, image_id=999999))          # unknown image: not evaluated
    ds["annotations"].append(dict(ds["annotations"][0], id=99992, category_id=999))          # unknown category
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(ds))
    for src in (ds, str(path)):
        a = ce.load_annotations(src)
        r = ref.RefCOCOeval(ds, res)
        assert a.image_ids.tolist() == r.img_ids and a.category_ids.tolist() == r.cat_ids
        assert (np.diff(a.gt_group) >= 0).all() and a.gt_group.size == len(ds["annotations"]) - 2
        I = a.image_ids.size
        for key in np.unique(a.gt_group):
            sel = a.gt_group == key
            want = r.gts[r.img_ids[key % I], r.cat_ids[key // I]]                            # the file's order inside a group
            assert a.gt_bbox[sel].tolist() == [g["bbox"] for g in want]
            assert a.gt_area[sel].tolist() == [g["area"] for g in want]
            assert a.gt_iscrowd[sel].tolist() == [g["iscrowd"] for g in want]                # a missing iscrowd counts as 0
        assert a.num_groups == sum(1 for v in r.gts.values() if v)


def test_input_errors():
    from dinov2_od_amd import cocoeval as ce
    ds, res = ref.make_scene(1)
    ann = ce.load_annotations(ds)
    assert ce.to_coco_dets(res, ann).shape == (len(res),)
    with pytest.raises(ValueError, match="image id"):
        ce.to_coco_dets(res + [dict(res[0], image_id=10 ** 9)], ann)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ce.to_coco_dets(res + [dict(res[0], score=bad)], ann)
    for bad_id in (0, -4):
        with pytest.raises(ValueError, match="not positive"):
            ce.load_annotations(dict(ds, annotations=ds["annotations"] + [dict(ds["annotations"][0], id=bad_id)]))
    many = [dict(ds["annotations"][0], id=10 ** 6 + n) for n in range(ce.MAX_GT_PER_GROUP + 1)]
    with pytest.raises(ValueError, match="1024"):
        ce.load_annotations(dict(ds, annotations=many))
    ce.load_annotations(dict(ds, annotations=many[:-1]))                                     # exactly 1024 is inside the limit
    assert ce.to_coco_dets([], ann).shape == (0,)                                            # empty results are accepted


def test_record_dtype_ingestion():
    from dinov2_od_amd import cocoeval as ce
    from dinov2_od_amd.postprocess import RECORD_DTYPE, records_to_coco
    ds, res = ref.make_scene(2)
    ann = ce.load_annotations(ds)
    rec = np.zeros(len(res), RECORD_DTYPE)
    for j, r in enumerate(res):
        rec[j] = (r["image_id"], r["category_id"], j, tuple(r["bbox"]), r["score"], 0)
    a, b = ce.to_coco_dets(rec, ann), ce.to_coco_dets(records_to_coco(rec), ann)
    assert a.dtype == ce.COCO_DET_DTYPE and a.tobytes() == b.tobytes() == ce.to_coco_dets(res, ann).tobytes()
    with pytest.raises(ValueError):
        ce.to_coco_dets(np.zeros(3, np.float32), ann)
    assert np.array_equal(ce.IOU_THRS, ref.IOU_THRS) and np.array_equal(ce.REC_THRS, ref.REC_THRS)


# ------------------------------------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    from dinov2_od_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from dinov2_od_amd._build import build
        build(verbose=False)
    return nat.lib()


NAMES = ("dod_coco_eval_workspace_bytes", "dod_coco_eval_set_gt", "dod_coco_eval_reset", "dod_coco_eval_append", "dod_coco_eval_append_host",
         "dod_coco_eval_evaluate", "dod_coco_eval_matches", "dod_op_sort_pairs_workspace_bytes", "dod_op_sort_pairs_u64")


def test_entry_points_are_declared_bound_and_exported(lib):
    from dinov2_od_amd import _native as nat
    hdr = open(os.path.join(ROOT, "include", "dinodet.h")).read()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in nat.SYMBOLS and hasattr(lib, name)
    assert C.sizeof(C.c_double) * 7 == 56 and "dod_coco_det" in hdr


def test_workspace_bytes_cover_the_limits_and_refuse_beyond(lib):
    ws = lib.dod_coco_eval_workspace_bytes
    assert ws(1 << 24, 5000, 80, 40000) > (1 << 24) * 56                  # 2^24 detections are inside the limits
    assert 0 < ws(1, 1, 1, 0) < ws(1000, 1, 1, 0) < ws(1000, 1, 80, 0)
    for bad in ((0, 10, 10, 5), ((1 << 24) + 1, 10, 10, 5), (100, 0, 10, 5), (100, 10, 0, 5), (100, 10, 10, -1), (-5, 10, 10, 5)):
        assert ws(*bad) == 0, bad
    assert lib.dod_op_sort_pairs_workspace_bytes(1 << 24) > 0 and lib.dod_op_sort_pairs_workspace_bytes(0) == 0
    assert lib.dod_op_sort_pairs_workspace_bytes((1 << 24) + 1) == 0


def test_set_gt_rejects_bad_arguments_before_any_hip_call(lib):
    INVALID, STATE = 1, 3
    I, K, G = 3, 2, 4
    img, cat = np.array([2, 5, 9], np.int64), np.array([1, 4], np.int64)
    key = np.array([0, 0, 2, 5], np.int64)
    box, area, crowd = np.ones((G, 4)), np.ones(G), np.zeros(G, np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)                               # noqa: E731

    def call(img=img, cat=cat, key=key, G=G, box=box, area=area, crowd=crowd, cap=64):
        return lib.dod_coco_eval_set_gt(None, 0, cap, len(img), len(cat), G, p(img), p(cat), p(key), p(box), p(area), p(crowd), p(ref.IOU_THRS),
                                        p(ref.REC_THRS), None)

    assert call() == STATE                                                # everything valid but the (absent) workspace
    assert call(img=np.array([2, 9, 5], np.int64)) == INVALID             # ids must be sorted
    assert call(cat=np.array([4, 4], np.int64)) == INVALID                # ... and unique
    assert call(key=np.array([0, 2, 1, 5], np.int64)) == INVALID          # groups must arrive sorted
    assert call(key=np.array([0, 0, 2, 6], np.int64)) == INVALID          # key outside categories * images
    assert call(cap=(1 << 24) + 1) == INVALID
    n = 1025
    assert lib.dod_coco_eval_set_gt(None, 0, 64, I, K, n, p(img), p(cat), p(np.zeros(n, np.int64)), p(np.ones((n, 4))), p(np.ones(n)),
                                    p(np.zeros(n, np.uint8)), p(ref.IOU_THRS), p(ref.REC_THRS), None) == INVALID      # 1025 in one group
    assert b"1024" in lib.dod_last_error(None)
