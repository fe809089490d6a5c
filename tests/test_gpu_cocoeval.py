"""`-m gpu`: the device COCO evaluator (csrc/cocoeval.hip through dinov2_od_amd/cocoeval.py) against the numpy restatement of
pycocotools' COCOeval (tests/cocoeval_ref.py).  The device code performs the same double operations on the same values, so the
matching decisions, `precision` and `recall` are compared EXACTLY; only the 12 means may differ, by summation order: at most
n * 2^-53 ~ 9e-12 for n <= 80 800 values in [0, 1], hence 1e-10."""
import json

import numpy as np
import pytest
import torch

from tests import cocoeval_ref as ref

pytestmark = pytest.mark.gpu
STATS_TOL = 1e-10
SCENES = [dict(seed=0), dict(seed=1, n_images=16, n_cats=8), dict(seed=2, n_images=7, n_cats=4), dict(seed=5, n_images=12, crowded=False)]


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dinov2_od_amd import cocoeval
    return cocoeval


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check_against_ref(out, want):
    assert _same_bits(out["precision"], want["precision"])
    assert _same_bits(out["recall"], want["recall"])
    err = np.abs(np.array(out["stats"]) - np.array(want["stats"])).max()
    print("max |stats - restatement| =", err)
    assert err <= STATS_TOL


# ------------------------------------------------------------------------------------------------ the sort operator
def _sort(keys, begin=0, end=64):
    from dinov2_od_amd import _native as nat
    L = nat.lib()
    n = keys.size
    dev = torch.device("cuda:0")
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = torch.arange(n, dtype=torch.int32, device=dev)
    k2, v2 = torch.empty_like(k), torch.empty_like(v)
    ws = torch.empty(max(1, L.dod_op_sort_pairs_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    nat.check(L.dod_op_sort_pairs_u64(nat.ptr(k), nat.ptr(v), nat.ptr(k2), nat.ptr(v2), n, begin, end, nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    torch.cuda.synchronize()
    return k.cpu().numpy().view(np.uint64), v.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 2048, 2049, 3 * 2048 + 17, 50000])
def test_sort_pairs_is_numpy_stable_argsort(ce, n):
    rng = np.random.default_rng(n)
    for keys in (rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64),
                 rng.integers(0, 7, n).astype(np.uint64),                                      # heavy ties
                 rng.integers(0, 3, n).astype(np.uint64) << np.uint64(56),                     # ties in the top digit
                 np.full(n, 0xdeadbeefcafe, np.uint64)):                                       # all equal: the identity
        order = np.argsort(keys, kind="stable")
        k, v = _sort(keys)
        assert np.array_equal(v, order.astype(np.int32)) and np.array_equal(k, keys[order])
    keys = rng.integers(0, 2 ** 40, n, dtype=np.int64).astype(np.uint64)                       # a digit window: bits [8, 24)
    order = np.argsort((keys >> np.uint64(8)) & np.uint64(0xffff), kind="stable")
    k, v = _sort(keys, 8, 24)
    assert np.array_equal(v, order.astype(np.int32)) and np.array_equal(k, keys[order])


def test_sort_descending_doubles_through_the_bit_map(ce):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.choice(np.arange(1, 16) / 16, 3000), rng.uniform(-2, 2, 3000), [0.0, -0.0, 1e-300, -1e-300]])
    x = x[rng.permutation(x.size)]
    b = x.view(np.uint64)
    asc = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    k, v = _sort(~asc)
    nz = x != 0                                      # the plain map orders -0.0 after +0.0; the evaluator canonicalises zeros
    order = np.argsort(-x, kind="stable")
    assert np.array_equal(v[nz[v]], order[nz[order]].astype(np.int32))


# ------------------------------------------------------------------------------------------------ evaluation vs the restatement
def _device_groups(ev, m, results):
    """the device's per-group decisions in the restatement's form, from COCOEvaluator.matches()"""
    ann = ev.ann
    I = ann.image_ids.size
    img = np.searchsorted(ann.image_ids, [results[i]["image_id"] for i in m["index"]])
    cat_id = np.array([results[i]["category_id"] for i in m["index"]], np.int64)
    cat = np.searchsorted(ann.category_ids, cat_id)
    known = (cat < ann.category_ids.size) & (ann.category_ids[np.minimum(cat, ann.category_ids.size - 1)] == cat_id)
    groups = {}
    for j in np.nonzero(known & (m["rank"] < 100))[0]:
        g = groups.setdefault((int(cat[j]), int(img[j])), {"dt_index": [], "matched": [], "ignored": []})
        assert m["rank"][j] == len(g["dt_index"])                                             # positions of a group come in rank order
        g["dt_index"].append(int(m["index"][j]))
        for name in ("matched", "ignored"):
            bits = int(m[name][j])
            g[name].append([[(bits >> (a * 10 + t)) & 1 for t in range(10)] for a in range(4)])
    npig = {divmod(int(k), I): row for k, row in zip(m["group_key"], m["npig"])}
    return groups, npig


@pytest.mark.parametrize("scene", SCENES, ids=lambda s: "seed%d" % s["seed"])
def test_matches_precision_recall_and_stats_equal_the_restatement(ce, scene):
    ds, res = ref.make_scene(**scene)
    want = ref.evaluate(ds, res)
    ev = ce.COCOEvaluator(ds, max_detections=4096)
    ev.add_records(res)
    out = ev.evaluate()
    groups, npig = _device_groups(ev, ev.matches(), res)
    assert set(groups) | set(npig) == set(want["groups"])                                     # every group counts, none is invented
    imgs, cats = sorted(i["id"] for i in ds["images"]), sorted(c["id"] for c in ds["categories"])
    assert set(npig) == {(cats.index(a["category_id"]), imgs.index(a["image_id"])) for a in ds["annotations"]}
    for key, w in want["groups"].items():
        assert npig.get(key, np.zeros(4)).tolist() == w["npig"].tolist(), key
        g = groups.get(key, {"dt_index": [], "matched": [], "ignored": []})
        assert g["dt_index"] == w["dt_index"].tolist(), key
        if g["dt_index"]:
            assert np.array_equal(np.array(g["matched"], bool).transpose(1, 2, 0), w["matched"]), key
            assert np.array_equal(np.array(g["ignored"], bool).transpose(1, 2, 0), w["ignored"]), key
    _check_against_ref(out, want)
    again = ev.evaluate()                                                                     # the same input twice: the same bits
    assert _same_bits(again["precision"], out["precision"]) and _same_bits(again["recall"], out["recall"]) and again["stats"] == out["stats"]
    fresh = ce.COCOEvaluator(ds, max_detections=len(res))
    fresh.add_records(res[: len(res) // 2])
    fresh.add_records(res[len(res) // 2:])
    got = fresh.evaluate()
    assert _same_bits(got["precision"], out["precision"]) and got["stats"] == out["stats"]


def test_empty_results_unknown_categories_and_reset(ce):
    ds, res = ref.make_scene(4)
    ev = ce.COCOEvaluator(ds, max_detections=2048)
    out = ev.evaluate()                                                                       # no detections: AP = AR = 0 where ground truth exists
    _check_against_ref(out, ref.evaluate(ds, []))
    assert out["stats"][0] == 0.0 and out["stats"][8] == 0.0
    extra = [dict(res[n], category_id=977 + n) for n in range(5)]                             # categories the annotations lack: not evaluated
    ev.add_records(res[:40] + extra + res[40:])
    want = ref.evaluate(ds, res)
    _check_against_ref(ev.evaluate(), want)
    ev.reset()
    ev.add_records(res)
    _check_against_ref(ev.evaluate(), want)
    m = ce.compute_coco_metrics(res, ds)
    assert list(m) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and all(type(v) is float for v in m.values())
    assert np.abs(np.array(list(m.values())) - np.array(want["stats"][:6])).max() <= STATS_TOL


# ------------------------------------------------------------------------------------------------ the three input paths
def _packed_scene(seed, B=6, Q=40, Cn=7):
    """packed detections [B, Q, Cn+4] and annotations in the detector's own conventions (normalised boxes, class index as id)"""
    rng = np.random.default_rng(seed)
    logits = rng.normal(-2.0, 2.0, (B, Q, Cn)).astype(np.float32)
    logits[:, ::5, 1:] = np.round(logits[:, ::5, 1:])                                         # tied scores
    boxes = np.concatenate([rng.uniform(0.2, 0.8, (B, Q, 2)), rng.uniform(0.05, 0.4, (B, Q, 2))], -1).astype(np.float32)
    det = np.concatenate([logits, boxes], -1)
    ids = [int(v) for v in rng.choice(np.arange(10, 900), B, replace=False)]
    anns = []
    for b in range(B - 1):                                                                    # the last image has no ground truth
        for q in rng.choice(Q, 6, replace=False):
            cx, cy, w, h = (float(v) for v in boxes[b, q] * rng.uniform(0.9, 1.1, 4))
            anns.append({"id": len(anns) + 1, "image_id": ids[b], "category_id": int(rng.integers(1, Cn)), "bbox": [cx - w / 2, cy - h / 2, w, h],
                         "area": w * h, "iscrowd": int(rng.random() < 0.15)})
    ds = {"images": [{"id": i} for i in ids] + [{"id": 5}], "categories": [{"id": c} for c in range(1, Cn)], "annotations": anns}
    return torch.from_numpy(det).cuda(), ids, ds


def test_dict_record_and_packed_paths_agree(ce):
    from dinov2_od_amd.postprocess import postprocess_packed, records_to_coco
    det, ids, ds = _packed_scene(11)
    rec = postprocess_packed(det, det.shape[-1] - 4, ids, 0.05)
    dicts = records_to_coco(rec)
    assert len(dicts) > 200
    outs = []
    for feed in ("dicts", "records", "packed", "packed_tensor_ids"):
        ev = ce.COCOEvaluator(ds, max_detections=det.shape[0] * det.shape[1] * (det.shape[2] - 5))
        if feed == "dicts":
            ev.add_records(dicts)
        elif feed == "records":
            ev.add_records(rec)
        elif feed == "packed":
            ev.add_packed(det[:2], ids[:2], 0.05)                                             # two appends, no sync in between
            ev.add_packed(det[2:], ids[2:], 0.05)
        else:
            ev.add_packed(det, torch.tensor(ids), 0.05)
        outs.append(ev.evaluate())
    for o in outs[1:]:
        assert _same_bits(o["precision"], outs[0]["precision"]) and _same_bits(o["recall"], outs[0]["recall"]) and o["stats"] == outs[0]["stats"]
    _check_against_ref(outs[0], ref.evaluate(ds, dicts))
    assert outs[0]["stats"][0] > 0.0


class _Detector(torch.nn.Module):
    """a synthetic detector: its outputs are a fixed function of the pixels"""
    Q, Cn = 30, 6

    def forward(self, images):
        x = images.flatten(1)
        B = x.shape[0]
        logits = (x[:, : self.Q * self.Cn].reshape(B, self.Q, self.Cn) - 0.6) * 6.0
        boxes = x[:, self.Q * self.Cn: self.Q * (self.Cn + 4)].reshape(B, self.Q, 4) * 0.5 + 0.1
        return {"pred_logits": logits, "pred_boxes": boxes}


def test_validate_coco_equals_evaluate_then_metrics(ce, tmp_path):
    from dinov2_od_amd.postprocess import evaluate_coco
    rng = np.random.default_rng(21)
    dev = torch.device("cuda:0")
    model = _Detector().to(dev)
    ids = [int(v) for v in rng.choice(np.arange(1, 500), 8, replace=False)]
    loader = [(torch.from_numpy(rng.uniform(0, 1, (4, 3, 10, 10)).astype(np.float32)), [{"image_id": i} for i in ids[b: b + 4]]) for b in (0, 4)]
    results = evaluate_coco(model, loader, dev)
    assert len(results) > 100
    anns = [{"id": n + 1, "image_id": r["image_id"], "category_id": r["category_id"], "bbox": [v * s for v, s in zip(r["bbox"], (1.0, 1.0, 0.9, 1.1))],
             "area": r["bbox"][2] * r["bbox"][3], "iscrowd": 0} for n, r in enumerate(results[::7])]
    ds = {"images": [{"id": i} for i in ids], "categories": [{"id": c} for c in range(1, _Detector.Cn)], "annotations": anns}
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(ds))
    want = ce.compute_coco_metrics(results, str(path))
    got = ce.validate_coco(model, loader, dev, str(path))
    assert {k: got[k] for k in ce.METRIC_KEYS} == want and len(got["stats"]) == 12
    full = ref.evaluate(ds, results)
    assert np.abs(np.array(got["stats"]) - np.array(full["stats"])).max() <= STATS_TOL
    assert want["AP"] > 0.0


# ------------------------------------------------------------------------------------------------ limits and errors
def test_limit_overflow_and_bad_input_raise_value_error(ce):
    ds, res = ref.make_scene(6)
    ev = ce.COCOEvaluator(ds, max_detections=8)
    with pytest.raises(ValueError, match="max_dets"):
        ev.add_records(res[:20])
    det, ids, pds = _packed_scene(12)
    ev = ce.COCOEvaluator(pds, max_detections=16)                                             # the device path cannot know before evaluate
    ev.add_packed(det, ids, 0.05)
    with pytest.raises(ValueError, match="max_dets"):
        ev.evaluate()
    ev = ce.COCOEvaluator(pds, max_detections=1 << 14)
    ev.add_packed(det, [1234567] + ids[1:], 0.05)                                             # an image id the annotations lack
    with pytest.raises(ValueError, match="image id"):
        ev.evaluate()
    with pytest.raises(ValueError):
        ce.COCOEvaluator(ds, max_detections=(1 << 24) + 1)
    many = [dict(ds["annotations"][0], id=10 ** 6 + n) for n in range(1025)]
    with pytest.raises(ValueError, match="1024"):
        ce.COCOEvaluator(dict(ds, annotations=many))


def test_a_group_of_a_thousand_ground_truths(ce):
    """groups of more than 64 ground truths run in the large instance of the match kernel"""
    ds, res = ref.make_scene(8, n_images=6, n_cats=4)
    rng = np.random.default_rng(8)
    half = next(a for a in ds["annotations"] if a["bbox"] == [0.0, 0.0, 2.0, 2.0])           # the group of the exact-0.5 pair
    crowd = [dict(half, id=10 ** 6 + n, bbox=[float(v) for v in rng.uniform(0, 300, 2)] + [float(v) for v in rng.uniform(5, 120, 2)],
                  area=float(rng.uniform(100, 20000)), iscrowd=int(n % 50 == 0)) for n in range(1000)]
    dts = [{"image_id": half["image_id"], "category_id": half["category_id"], "bbox": [float(np.float32(v)) for v in g["bbox"]],
            "score": float(np.float32(rng.choice([0.25, 0.5, 0.75, rng.uniform(0.1, 1)])))} for g in crowd[::25]]
    big = dict(ds, annotations=ds["annotations"] + crowd)
    ev = ce.COCOEvaluator(big, max_detections=4096)
    ev.add_records(res + dts)
    _check_against_ref(ev.evaluate(), ref.evaluate(big, res + dts))
