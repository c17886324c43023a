"""GPU tests of the COCO evaluation on the device (csrc/coco_eval.hip, yolov3_amd/coco_eval.py): `precision`, `recall` and `scores` bit for bit against the tests' literal
restatement of pycocotools' COCOeval (tests/coco_eval_cases.py; recorded whole for the fixture scene in tests/golden/coco_eval.pt), the three input forms, and
`run_batches(save_json=True, anno_json=...)` end to end.  Equality is exact: every quantity is one IEEE fp64 operation in a fixed order or an integer count."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import coco_eval_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "coco_eval.pt", weights_only=True)


@pytest.fixture(scope="module")
def scenes():
    """every seeded scene with the restatement's result, computed once (left unchanged by the tests)"""
    out = {}
    for name in cc.SCENES:
        anno, dets, img_ids = cc.scene(name)
        out[name] = (anno, dets, img_ids, cc.evaluate(anno, dets, img_ids))
    return out


def _same(res, want, what):
    for k in ("precision", "recall", "scores"):
        got = getattr(res, k)
        assert got.dtype == np.float64 and got.shape == want[k].shape, (what, k)
        if not np.array_equal(got, want[k]):
            bad = np.argwhere(got != want[k])
            raise AssertionError(f"{what}: {k} differs in {len(bad)} cells, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[k][tuple(bad[0])]!r}")
    assert np.array_equal(res.stats, want["stats"]), (what, res.stats, want["stats"])


def _evaluate(dev, anno, dets, img_ids=None, **kw):
    from yolov3_amd import CocoEval, CocoGroundTruth

    return CocoEval(CocoGroundTruth(anno, dev), img_ids, **kw).evaluate(dets)


def test_fixture_scene_equals_the_recorded_arrays(dev, gold):
    g = gold["fixture"]
    res = _evaluate(dev, json.loads(g["anno"]), json.loads(g["dets"]))
    _same(res, {k: g[k].numpy() for k in ("precision", "recall", "scores", "stats")}, "fixture")
    assert res.summarize() == g["lines"] and res.precision.shape == (10, 101, 2, 4, 3) and res.recall.shape == (10, 2, 4, 3)


@pytest.mark.parametrize("name", list(cc.SCENES))
def test_seeded_scenes_equal_the_restatement(dev, gold, scenes, name):
    """each scene: a pair with 130 detections (the cap of 100, maxDets 1 / 10), a pair with 300 ground truths, score ties inside a pair and across images, crowds under many
    detections, areas on the 32^2 / 96^2 boundaries, images with detections only and with ground truth only, a category without ground truth, one outside the file, and
    ("crowded", "ties") detections of an image left out of img_ids"""
    anno, dets, img_ids, want = scenes[name]
    s = gold["scenes"][name]
    assert all(hashlib.sha256(np.ascontiguousarray(want[k]).tobytes()).hexdigest() == s["sha256"][k] for k in ("precision", "recall", "scores")), "the restatement drifted"
    res = _evaluate(dev, anno, dets, img_ids)
    _same(res, want, name)
    assert res.summarize() == cc.summarize(want["precision"], want["recall"])[1]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_hand_cases(dev, name):
    anno, dets, _ = cc.hand_case(name)
    _same(_evaluate(dev, anno, dets), cc.evaluate(anno, dets), name)


def test_more_than_one_chunk_of_rows_in_a_category(dev):
    anno, dets = cc.long_scene()
    assert min(sum(d["category_id"] == c for d in dets) for c in (1, 2)) > 1024
    _same(_evaluate(dev, anno, dets), cc.evaluate(anno, dets), "long")


def test_other_parameters(dev, scenes):
    """a cap below the pairs' sizes, three thresholds that are not pycocotools' (one of them 1.0: min(t, 1 - 1e-10)), two area ranges, five recall samples"""
    anno, dets, img_ids, _ = scenes["crowded"]
    kw = dict(iou_thrs=[0.3, 0.77, 1.0], rec_thrs=[0.0, 0.25, 0.5, 0.99, 1.0], max_dets=(20, 2, 5), area_rng=[[0, 1e10], [500, 5000]])
    res = _evaluate(dev, anno, dets, img_ids, **kw)
    p, r, s = cc.coco_eval(anno, dets, img_ids, kw["iou_thrs"], kw["rec_thrs"], sorted(kw["max_dets"]), kw["area_rng"])
    assert res.precision.shape == (3, 5, 4, 2, 3) and res.stats is None
    assert np.array_equal(res.precision, p) and np.array_equal(res.recall, r) and np.array_equal(res.scores, s)
    with pytest.raises(ValueError, match="summarize"):
        res.summarize()


def test_empty_detection_list(dev, scenes):
    """every cell with ground truth to find has precision 0 and recall 0, every other stays -1"""
    anno, _, img_ids, _ = scenes["mixed"]
    want = cc.evaluate(anno, [], img_ids)
    for dets in ([], np.zeros((0, 7))):
        res = _evaluate(dev, anno, dets, img_ids)
        _same(res, want, "empty")
        assert set(np.unique(res.precision)) == {-1.0, 0.0} and set(np.unique(res.recall)) == {-1.0, 0.0}
        assert (res.recall[:, 3] == -1).all() and (res.recall[:, :3, 0] == 0).all()   # category 9 has no ground truth; the others have some in the "all" range
        assert ((res.precision == -1).all(axis=1) == (res.recall == -1)).all()


def test_input_forms_and_unknown_image(dev, scenes, tmp_path):
    from yolov3_amd import CocoEval, CocoGroundTruth

    anno, dets, img_ids, want = scenes["ties"]
    (tmp_path / "anno.json").write_text(json.dumps(anno))
    (tmp_path / "predictions.json").write_text(json.dumps(dets))
    gt = CocoGroundTruth(tmp_path / "anno.json", dev)
    ev = CocoEval(gt, img_ids)
    for form in (dets, tmp_path / "predictions.json", str(tmp_path / "predictions.json"), cc.dets_array(dets)):
        _same(ev.evaluate(form), want, type(form).__name__)
    _same(ev.evaluate(dets), want, "a second call on the same evaluator")
    with pytest.raises(ValueError, match="correspond"):
        ev.evaluate(dets + [dict(dets[0], image_id=4242)])
    with pytest.raises(ValueError, match="correspond"):
        ev.evaluate(np.array([[4242, 1, 0, 0, 5, 5, 0.5]]))
    # an image of the file that is outside img_ids takes no part, and neither does an unknown category: no error
    assert any(d["image_id"] == 105 for d in dets) and any(d["category_id"] == 5 for d in dets)


def _tiny(dev, golden_dir):
    from yolov3_amd import DetectMultiBackend, compat

    m = DetectMultiBackend(str(golden_dir / "ref_tiny_w025_fp16.pt"), device=dev, fp16=False)
    compat.uninstall_aliases()
    return m


def _batches():
    """two batches of three 64x64 images, numeric stems"""
    shapes = [((64, 64), ((1.0, 1.0), (0.0, 0.0)))] * 3
    out = []
    for b in range(2):
        g = torch.Generator().manual_seed(70 + b)
        im = torch.rand(3, 3, 64, 64, generator=g)
        targets = torch.tensor([[0, 1, 0.5, 0.5, 0.3, 0.4], [0, 2, 0.3, 0.6, 0.2, 0.2], [2, 0, 0.6, 0.4, 0.5, 0.5]])
        out.append((im, targets, [f"/data/val/{(11 + 3 * b + i):012d}.jpg" for i in range(3)], shapes))
    return out


def test_run_batches_end_to_end(dev, golden_dir, tmp_path):
    from yolov3_amd import CocoGroundTruth, run_batches

    m = _tiny(dev, golden_dir)
    nc, conf = 80, 1e-4   # (the random-weight checkpoint scores obj x cls around 2e-4)
    batches = _batches()
    with torch.no_grad():
        plain = run_batches(m, batches, nc, conf_thres=conf, save_json=True, save_dir=tmp_path / "plain")
        jdict = json.loads((tmp_path / "plain" / "predictions.json").read_text())
        assert len(jdict) > 100
        # a synthetic annotation file from the run's own detections: every 7th box, nudged, is a ground truth (every 10th of those a crowd, twice the size)
        rng = np.random.default_rng(3)
        anns = []
        for i, d in enumerate(jdict[::7]):
            x, y, w, h = (float(v) for v in d["bbox"])
            crowd = int(i % 10 == 0)
            box = [round(x + float(rng.normal(0, 1)), 2), round(y + float(rng.normal(0, 1)), 2), max(round(w * (2 if crowd else 1) + float(rng.normal(0, 1)), 2), 1.0), max(h * (2 if crowd else 1), 1.0)]
            anns.append(dict(id=i + 1, image_id=d["image_id"], category_id=d["category_id"], bbox=box, area=box[2] * box[3], iscrowd=crowd))
        ids = sorted({d["image_id"] for d in jdict})
        assert ids == list(range(11, 17))
        anno = dict(images=[dict(id=i) for i in ids + [99]], categories=[dict(id=c) for c in range(nc)], annotations=anns)
        anno["annotations"].append(dict(id=len(anns) + 1, image_id=99, category_id=0, bbox=[1.0, 1.0, 20.0, 20.0], area=400.0, iscrowd=0))   # an image the run never sees
        (tmp_path / "anno.json").write_text(json.dumps(anno))
        seen = run_batches(m, batches, nc, conf_thres=conf, save_json=True, save_dir=tmp_path / "seen", anno_json=tmp_path / "anno.json", coco_img_ids="seen")
        every = run_batches(m, batches, nc, conf_thres=conf, save_json=True, save_dir=tmp_path / "all", anno_json=CocoGroundTruth(anno, dev))
        again = run_batches(m, batches, nc, conf_thres=conf, save_json=True, save_dir=tmp_path / "again")
    assert (tmp_path / "seen" / "predictions.json").read_bytes() == (tmp_path / "plain" / "predictions.json").read_bytes()
    written = json.loads((tmp_path / "seen" / "predictions.json").read_text())
    for got, img_ids in ((seen, ids), (every, None)):
        want = cc.evaluate(anno, written, img_ids)
        res, maps, stats = got
        _same(stats.coco, want, "run_batches")
        assert res[3] == want["stats"][0] and res[2] == want["stats"][1] and res[:2] == plain[0][:2] and 0 < res[3] <= res[2] <= 1
        base = np.zeros(nc) + want["stats"][0]   # val.py:486-488
        labelled = plain[1] != plain[0][3]
        assert np.array_equal(maps[~labelled], base[~labelled]) and np.array_equal(maps[labelled], plain[1][labelled])
    assert seen[0][3] != every[0][3]   # image 99's ground truth is never found
    # without anno_json nothing changes: the results, maps and ValStats of two runs
    assert plain[0] == again[0] and np.array_equal(plain[1], again[1]) and plain[2].n == again[2].n == seen[2].n and not hasattr(plain[2], "coco")
    assert all(np.array_equal(a, b) for a, b in zip(plain[2].compute()[:6], seen[2].compute()[:6]))
