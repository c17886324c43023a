"""CPU tests of the device-side COCO evaluation (csrc/coco_eval.hip, yolov3_amd/coco_eval.py): the public surface, the symbols declared / bound / exported at ABI 6, the
C ABI's argument validation without a GPU, the host half of the module, and the tests' own restatement of pycocotools' COCOeval (tests/coco_eval_cases.py) against cases
worked by hand and against the recorded fixture."""
import hashlib
import inspect
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import coco_eval_cases as cc  # noqa: E402

NEW_SYMBOLS = ["y3_coco_eval_workspace_bytes", "y3_coco_match", "y3_coco_accumulate"]
P = cc.P1


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "coco_eval.pt", weights_only=True)   # data only


def test_public_names_import():
    import yolov3_amd
    from yolov3_amd import CocoEval, CocoGroundTruth, CocoResult, coco_eval, ops, run_batches

    assert coco_eval.CocoEval is CocoEval and coco_eval.CocoGroundTruth is CocoGroundTruth and coco_eval.CocoResult is CocoResult
    assert callable(yolov3_amd.CocoEval) and callable(ops.coco_match) and callable(ops.coco_accumulate)
    sig = inspect.signature(CocoEval.__init__).parameters
    assert list(sig)[1:] == ["gt", "img_ids", "iou_thrs", "rec_thrs", "max_dets", "area_rng"] and sig["max_dets"].default == (1, 10, 100) and sig["img_ids"].default is None
    rb = inspect.signature(run_batches).parameters
    assert list(rb)[-2:] == ["anno_json", "coco_img_ids"] and rb["anno_json"].default is None and rb["coco_img_ids"].default is None


def test_new_symbols_are_declared_bound_and_exported_at_abi_6(lib):
    from yolov3_amd import _lib

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols()) and declared == set(_lib.exported_symbols())
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    assert ("coco_eval.hip", ["-ffp-contract=off"]) in __import__("yolov3_amd.build", fromlist=["SOURCES"]).SOURCES
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS)
    source = (ROOT / "yolov3_amd" / "coco_eval.py").read_text()
    assert "_lib" not in source and "ctypes" not in source   # the module marshals no C call itself
    assert not re.search(r"torch\.(sort|argsort|cumsum|cummax|searchsorted|maximum|minimum|where)\b", source)   # no torch compute stands in for a kernel


def _match_args(P_, **over):
    """a valid argument list of y3_coco_match on fake, aligned device addresses (validation never dereferences them)"""
    a = dict(det_img=P_, det_cat=P_, det_box=P_, det_score=P_, n_det=10, img_ids=P_, n_img=6, cat_ids=P_, K=3, gt_box=P_, gt_area=P_, gt_crowd=P_, gt_cat=P_, n_gt=5,
             gt_offsets=P_, iou_thrs=P_, T=10, area_rng=P_, A=4, max_det=100, row_score=P_, row_rank=P_, row_match=P_, row_ignore=P_, cat_begin=P_, cat_end=P_, npig=P_,
             workspace=P_, workspace_bytes=1 << 40, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return list(a.values())


def _acc_args(P_, **over):
    a = dict(row_score=P_, row_rank=P_, row_match=P_, row_ignore=P_, n_det=10, cat_begin=P_, cat_end=P_, npig=P_, K=3, T=10, rec_thrs=P_, R=101, max_dets=P_, M=3, A=4,
             precision=P_, scores=P_, recall=P_, stream=None)
    assert set(over) <= set(a), over
    a.update(over)
    return list(a.values())


def test_new_exports_reject_bad_arguments_without_a_gpu(lib):
    P_ = 1 << 20

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    for name in ("det_img", "det_cat", "det_box", "det_score", "img_ids", "cat_ids", "gt_box", "gt_area", "gt_crowd", "gt_cat", "gt_offsets", "iou_thrs", "area_rng", "row_score",
                 "row_rank", "row_match", "row_ignore", "cat_begin", "cat_end", "npig", "workspace"):
        fails(lib.y3_coco_match(*_match_args(P_, **{name: None})), b"y3_coco_match", b"null")
    for over in (dict(n_det=-1), dict(n_gt=-1), dict(n_det=1 << 31), dict(n_gt=1 << 31)):
        fails(lib.y3_coco_match(*_match_args(P_, **over)), b"y3_coco_match", b"counts")
    for over in (dict(n_img=0), dict(n_img=-2), dict(K=0), dict(K=-1), dict(n_img=1 << 20, K=1 << 11)):
        fails(lib.y3_coco_match(*_match_args(P_, **over)), b"y3_coco_match", b"geometry")
    for t in (0, -1, 17):
        fails(lib.y3_coco_match(*_match_args(P_, T=t)), b"y3_coco_match", b"IoU thresholds")
    for a in (0, -1, 9):
        fails(lib.y3_coco_match(*_match_args(P_, A=a)), b"y3_coco_match", b"area ranges")
    for m in (0, -5):
        fails(lib.y3_coco_match(*_match_args(P_, max_det=m)), b"y3_coco_match", b"max_det")
    fails(lib.y3_coco_match(*_match_args(P_, workspace=P_ + 8)), b"y3_coco_match", b"aligned")
    need = lib.y3_coco_eval_workspace_bytes(10, 5, 10, 4)
    assert need > 10 * (8 * 4 + 2 * 8) + 5 * 40
    fails(lib.y3_coco_match(*_match_args(P_, workspace_bytes=need - 1)), b"y3_coco_match", b"workspace needs")
    assert lib.y3_coco_eval_workspace_bytes(0, 0, 1, 1) > 0 and lib.y3_coco_eval_workspace_bytes(1000, 0, 16, 8) > 0
    assert lib.y3_coco_eval_workspace_bytes(10, 1000, 16, 8) - lib.y3_coco_eval_workspace_bytes(10, 1000, 1, 1) == 1000 * 128 - 1024   # one matched flag per ground truth and pass (256-byte steps)
    for bad in ((-1, 5, 10, 4), (10, -1, 10, 4), (1 << 31, 5, 10, 4), (10, 5, 17, 4), (10, 5, 0, 4), (10, 5, 10, 9), (10, 5, 10, 0)):
        assert lib.y3_coco_eval_workspace_bytes(*bad) == 0 and b"y3_coco_eval_workspace_bytes" in lib.y3_last_error() and b"geometry" in lib.y3_last_error()

    for name in ("row_score", "row_rank", "row_match", "row_ignore", "cat_begin", "cat_end", "npig", "rec_thrs", "max_dets", "precision", "scores", "recall"):
        fails(lib.y3_coco_accumulate(*_acc_args(P_, **{name: None})), b"y3_coco_accumulate", b"null")
    fails(lib.y3_coco_accumulate(*_acc_args(P_, n_det=-1)), b"y3_coco_accumulate", b"count")
    fails(lib.y3_coco_accumulate(*_acc_args(P_, n_det=1 << 31)), b"y3_coco_accumulate", b"count")
    fails(lib.y3_coco_accumulate(*_acc_args(P_, K=0)), b"y3_coco_accumulate", b"geometry")
    for t in (0, 17):
        fails(lib.y3_coco_accumulate(*_acc_args(P_, T=t)), b"y3_coco_accumulate", b"IoU thresholds")
    for a in (0, 9):
        fails(lib.y3_coco_accumulate(*_acc_args(P_, A=a)), b"y3_coco_accumulate", b"area ranges")
    for m in (0, 9):
        fails(lib.y3_coco_accumulate(*_acc_args(P_, M=m)), b"y3_coco_accumulate", b"maxDets")
    for r in (0, 1025):
        fails(lib.y3_coco_accumulate(*_acc_args(P_, R=r)), b"y3_coco_accumulate", b"recall samples")


def test_cpu_tensors_and_wrong_calls_are_refused(tmp_path):
    from yolov3_amd import CocoEval, CocoGroundTruth, ops, run_batches

    anno = cc.hand_case("A")[0]
    for call in (lambda: CocoGroundTruth(anno, "cpu"), lambda: CocoGroundTruth(anno, torch.device("cpu"))):
        with pytest.raises(RuntimeError, match="no CPU"):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU"):
            CocoGroundTruth(anno)
    with pytest.raises(TypeError, match="CocoGroundTruth"):
        CocoEval(anno)
    z64, zf = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.coco_match(z64, z64, torch.zeros(4, 4, dtype=torch.float64), zf, z64[:1], z64[:1], torch.zeros(0, 4, dtype=torch.float64), zf[:0], torch.zeros(0, dtype=torch.uint8),
                       torch.zeros(0, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), zf[:1], zf[:2], 100)
    rows = dict(score=zf, rank=torch.zeros(4, dtype=torch.int32), match=torch.zeros(4, 1, dtype=torch.uint16), ignore=torch.zeros(4, 1, dtype=torch.uint16),
                cat_begin=torch.zeros(1, dtype=torch.int32), cat_end=torch.zeros(1, dtype=torch.int32), npig=torch.zeros(1, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.coco_accumulate(rows, 1, zf[:3], torch.ones(1, dtype=torch.int32))
    # anno_json without save_json: refused before any device work (the model is never touched)
    with pytest.raises(ValueError, match="anno_json needs save_json"):
        run_batches(None, [], 80, anno_json=tmp_path / "instances.json")
    with pytest.raises(ValueError, match="anno_json needs save_json"):
        run_batches(None, [], 80, anno_json=anno, save_txt=True, save_dir=tmp_path)
    with pytest.raises(FileNotFoundError, match="anno_json"):
        run_batches(None, [], 80, anno_json=tmp_path / "missing.json", save_json=True, save_dir=tmp_path)


def test_host_half_groups_the_ground_truth_and_parses_the_three_forms(tmp_path, monkeypatch):
    from yolov3_amd import CocoEval, CocoGroundTruth, coco_eval

    # the host half alone: the module's two device hooks stand still (nothing is launched: evaluate() is not reached past its host checks)
    monkeypatch.setattr(coco_eval, "_device", lambda device, what: torch.device("cpu"))
    monkeypatch.setattr(coco_eval, "_upload", lambda a, device: torch.from_numpy(np.ascontiguousarray(a)))
    anno, dets, img_ids = cc.scene("ties")
    gt = CocoGroundTruth(anno)
    assert gt.img_ids.tolist() == list(range(101, 108)) and gt.cat_ids.tolist() == [1, 3, 7, 9] and gt.ann_crowd.dtype == np.uint8
    assert gt.ann_crowd.tolist() == [int(a.get("iscrowd", 0)) for a in anno["annotations"]]   # missing: 0; `ignore` is not read
    ev = CocoEval(gt, img_ids)
    assert ev.img_ids.tolist() == [101, 102, 103, 104, 106, 107] and ev.max_dets == [1, 10, 100]
    assert np.array_equal(ev.iou_thrs, cc.IOU_THRS) and np.array_equal(ev.rec_thrs, cc.REC_THRS) and np.array_equal(ev.area_rng, np.array(cc.AREA_RNG, dtype=np.float64))
    offs = ev._gt_offsets.numpy()
    want = [[a for a in anno["annotations"] if a["image_id"] == i and a["category_id"] == c] for i in ev.img_ids for c in gt.cat_ids]
    assert offs.size == 6 * 4 + 1 and np.diff(offs).tolist() == [len(w) for w in want] and ev.n_gt == sum(len(w) for w in want) < len(anno["annotations"])
    flat = [a for w in want for a in w]   # file order inside a pair
    assert ev._gt_area.tolist() == [a["area"] for a in flat] and ev._gt_box.tolist() == [a["bbox"] for a in flat]
    assert ev._gt_cat.tolist() == [gt.cat_ids.tolist().index(a["category_id"]) for a in flat]
    assert CocoEval(gt).img_ids.tolist() == gt.img_ids.tolist()
    # the three forms of `dets` give the same columns
    (tmp_path / "p.json").write_text(json.dumps(dets))
    a, b, c = ev._columns(dets), ev._columns(tmp_path / "p.json"), ev._columns(cc.dets_array(dets))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z) and x.dtype == y.dtype == z.dtype
    assert a[0].dtype == np.int64 and a[2].shape == (len(dets), 4) and a[3].dtype == np.float64
    with pytest.raises(ValueError, match="integers"):
        ev._columns([dict(dets[0], image_id="frame_0")])
    with pytest.raises(ValueError, match="correspond"):
        ev.evaluate([dict(dets[0], image_id=999)])   # raised on the host, before anything is uploaded
    for bad in (dict(max_dets=(0, 10)), dict(iou_thrs=np.linspace(0.1, 0.9, 17)), dict(area_rng=[[0, 1]] * 9), dict(max_dets=range(1, 10)), dict(img_ids=[])):
        with pytest.raises(ValueError):
            CocoEval(gt, **bad)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_restatement_on_the_cases_worked_by_hand(name):
    """The issue's hand values treat the mean of equal numbers as exact; NumPy's pairwise sum of n copies of p = 1 - 2^-52 is not (n p needs more than 53 bits), so a
    stat of a case whose cells all equal p is np.mean of that many copies of p -- within one unit in the last place of p -- and every CELL is p exactly."""
    anno, dets, want = cc.hand_case(name)
    r = cc.evaluate(anno, dets)
    assert P == 0.9999999999999998
    cells = [1010, 101, 101, 1010, 1010, 1010]
    for i, (got, w) in enumerate(zip(r["stats"], want)):
        if w == P:
            assert got == np.mean(np.full(cells[i], P)) and abs(got - P) <= 2.0 ** -52, (name, i, got)
        else:
            assert got == w, (name, i, got)
    p = r["precision"]
    if name == "A":
        assert (p[:, :, 0, 0, :] == P).all() and (p[:, :, 0, 2, :] == P).all() and (p[:, :, 0, 1, :] == -1).all() and (p[:, :, 0, 3, :] == -1).all()
        assert (r["scores"][:, :, 0, 0, :] == 0.9).all() and (r["recall"][:, 0, 0, :] == 1).all()
    if name == "B":   # maxDets 1: the false positive alone -- the sample at recall 0 is 0 (the envelope of [0]), the others are past the end
        assert (p[:, :, 0, 0, 0] == 0).all() and (p[:, :, 0, 0, 1:] == 0.5).all() and (r["scores"][:, 0, 0, 0, 2] == 0.9).all() and (r["scores"][:, 1:, 0, 0, 2] == 0.8).all()
    if name == "C":
        assert (p[:, :, 0, 0, 1:] == P).all() and (p[:, :, 0, 1, 1:] == P).all() and (p[:, :, 0, 2:, :] == -1).all()
        assert (p[:, 0, 0, 0, 0] == 0).all() and (r["recall"][:, 0, 0, 0] == 0).all()   # top-1 is the ignored detection: pr = 0 / (0 + 0 + spacing) = 0, recall 0
        assert (r["scores"][:, 0, 0, 0, 2] == 0.9).all() and (r["scores"][:, 1:, 0, 0, 2] == 0.7).all()   # rc = [0, 0, 1]: recall 0 is met by the first row, any other by the third


def _stats(anno, dets, img_ids=None):
    return cc.evaluate(anno, dets, img_ids)


def test_stop_rule_keeps_a_plain_match_over_a_better_ignored_one():
    """a detection overlaps a plain ground truth at IoU 0.6 and a crowd (visited last) at IoU 1: it stays matched to the plain one -- a true positive at 0.5 .. 0.6"""
    det = [0.0, 0.0, 100.0, 60.0]
    anno = cc._anno([(1, 1, [0.0, 0.0, 100.0, 100.0], 10000.0, 0), (1, 1, det, 6000.0, 1)])
    assert cc.box_iou(det, [0.0, 0.0, 100.0, 100.0], 0) == 0.6 and cc.box_iou(det, det, 1) == 1.0
    r = _stats(anno, [cc._det(1, 1, det, 0.9)])
    assert r["recall"][:, 0, 0, 2].tolist() == [1, 1, 1] + [0] * 7   # 0.5, 0.55, 0.6 (0.6 >= min(t, 1 - 1e-10) holds at t = 0.6 only if linspace gives 0.6 or less)
    assert cc.IOU_THRS[2] <= 0.6
    assert (r["precision"][:3, :, 0, 0, 2] == P).all()
    # above 0.6 the plain one is out of reach and the crowd takes the detection: ignored, neither true nor false positive
    assert (r["precision"][3:, :, 0, 0, 2] == 0).all() and (r["scores"][3:, 0, 0, 0, 2] == 0.9).all()
    # without the stop rule the crowd (IoU 1) would have taken it at every threshold
    e = cc.evaluate_img([dict(bbox=[0.0, 0.0, 100.0, 100.0], area=10000.0, iscrowd=0), dict(bbox=det, area=6000.0, iscrowd=1)], [dict(bbox=det, score=0.9)], cc.AREA_RNG[0], 100, cc.IOU_THRS)
    assert e["dtm"][:, 0].all() and e["dtIg"][:, 0].tolist() == [False] * 3 + [True] * 7 and e["npig"] == 1


def test_area_exactly_1024_counts_as_small_and_as_medium():
    box = [0.0, 0.0, 32.0, 32.0]
    r = _stats(cc._anno([(1, 1, box, 1024.0, 0)]), [cc._det(1, 1, box, 0.5)])
    assert (r["recall"][:, 0, 1, 2] == 1).all() and (r["recall"][:, 0, 2, 2] == 1).all() and (r["recall"][:, 0, 3, :] == -1).all()
    assert r["stats"][3] == r["stats"][4] == r["stats"][0] and r["stats"][5] == -1 and r["stats"][9] == r["stats"][10] == 1
    # the area is the annotation's field, not w * h: the same box with area 1025 is medium only
    r = _stats(cc._anno([(1, 1, box, 1025.0, 0)]), [cc._det(1, 1, box, 0.5)])
    assert (r["recall"][:, 0, 1, :] == -1).all() and (r["recall"][:, 0, 2, 2] == 1).all()


def test_category_with_detections_and_no_ground_truth_stays_minus_one():
    box = [0.0, 0.0, 50.0, 50.0]
    r = _stats(cc._anno([(1, 1, box, 2500.0, 0)], cats=(1, 2)), [cc._det(1, 1, box, 0.5), cc._det(1, 2, box, 0.9), cc._det(1, 3, box, 0.9)])
    assert r["precision"].shape == (10, 101, 2, 4, 3) and (r["precision"][:, :, 1] == -1).all() and (r["recall"][:, 1] == -1).all() and (r["scores"][:, :, 1] == -1).all()
    assert (r["recall"][:, 0, 0, :] == 1).all()


def test_score_ties_across_images_resolve_by_image_order():
    """two images, equal scores: image 1 holds a false positive, image 2 a true positive.  In imgIds order the false positive comes first (precision 1/2 everywhere);
    the other way round the samples would be p"""
    box, far = [0.0, 0.0, 50.0, 50.0], [300.0, 300.0, 50.0, 50.0]
    anno = cc._anno([(2, 1, box, 2500.0, 0), (1, 1, box, 2500.0, 0)], n_img=2)
    dets = [cc._det(2, 1, box, 0.5), cc._det(1, 1, far, 0.5)]   # arrival order is the other one
    r = _stats(anno, dets)
    assert (r["precision"][:, :51, 0, 0, 2] == 0.5).all() and (r["precision"][:, 51:, 0, 0, 2] == 0).all() and (r["recall"][:, 0, 0, 2] == 0.5).all()
    assert r["stats"][0] == np.mean(np.r_[np.full(510, 0.5), np.zeros(500)])


def test_case_builders_and_restatement_reproduce_the_golden(gold):
    anno, dets = cc.fixture_scene()
    g = gold["fixture"]
    assert json.loads(g["anno"]) == anno and json.loads(g["dets"]) == dets
    r = cc.evaluate(anno, dets)
    for k in ("precision", "recall", "scores", "stats"):
        assert np.array_equal(r[k], g[k].numpy()), k
    assert cc.summarize(r["precision"], r["recall"])[1] == g["lines"] and len(g["lines"]) == 12
    assert g["lines"][0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % r["stats"][0]
    assert list(gold["scenes"]) == list(cc.SCENES)
    anno, dets, img_ids = cc.scene("ties")   # (one scene here; the GPU tests recompute all of them and check the digests too)
    r = cc.evaluate(anno, dets, img_ids)
    s = gold["scenes"]["ties"]
    assert (len(anno["annotations"]), len(dets)) == (s["n_gt"], s["n_det"]) and np.array_equal(r["stats"], s["stats"].numpy())
    assert all(hashlib.sha256(np.ascontiguousarray(r[k]).tobytes()).hexdigest() == s["sha256"][k] for k in ("precision", "recall", "scores"))
    # what the scenes promise
    pairs = {}
    for d in dets:
        pairs.setdefault((d["image_id"], d["category_id"]), []).append(d["score"])
    gts = {}
    for a in anno["annotations"]:
        gts.setdefault((a["image_id"], a["category_id"]), []).append(a)
    assert max(len(v) for v in pairs.values()) >= 130 and max(len(v) for v in gts.values()) >= cc.BIG_G
    assert any(len(set(v)) < len(v) for v in pairs.values()) and any(a["area"] in (1024.0, 9216.0) for a in anno["annotations"])
    assert any(k[0] == 104 for k in pairs) and not any(k[0] == 104 for k in gts) and any(k[0] == 106 for k in gts) and not any(k[0] == 106 for k in pairs)
    assert any(k[1] == 9 for k in pairs) and any(k[1] == 5 for k in pairs) and any(k[0] == 105 for k in pairs) and 105 not in img_ids
    assert sum(1 for a in anno["annotations"] if a.get("iscrowd")) >= 5 and any("iscrowd" not in a for a in anno["annotations"])
