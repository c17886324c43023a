"""GPU tests of the output writers: y3_export_rows (csrc/val_edge.hip) bit for bit against the tables of the unmodified reference (tests/golden/val_outputs.pt),
the reference-signature functions and the batched writers of yolov3_amd.outputs against its file bytes / jdict / target array, Detections' strings from the export's class
histogram, and `run_batches(save_txt=, save_json=)` / `detect_batches` end to end against this package's own per-image writers."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import val_outputs_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "val_outputs.pt", weights_only=False)


@pytest.fixture(scope="module")
def cases(dev):
    """every case once, on the device (left unchanged by the tests)"""
    out = {}
    for name in oc.CASES:
        c = oc.case(name)
        c["dev_rows"] = c["rows"].to(dev)
        c["dev_counts"] = torch.tensor(c["counts"], dtype=torch.int32, device=dev)
        c["sizes"] = torch.tensor([[float(w), float(h)] for h, w in c["shapes"]], dtype=torch.float32, device=dev)
        out[name] = c
    return out


def _export(c, form, rows=None, **kw):
    from yolov3_amd import ops

    rows = c["dev_rows"] if rows is None else rows
    limit = kw.get("limit", 0)
    total = sum(min(n, limit) if limit else n for n in c["counts"])
    return ops.export_rows(rows, rows.stride(0), rows.stride(1), c["dev_counts"], rows.shape[0], rows.shape[1], form, total, sizes=c["sizes"] if form == "txt" else None, **kw)


def _read_dir(folder):
    return {f.name: f.read_bytes() for f in sorted(Path(folder).iterdir())} if Path(folder).exists() else {}


@pytest.mark.parametrize("name", list(oc.CASES))
def test_export_rows_equals_the_reference_tables_bit_for_bit(cases, gold, name):
    c, g = cases[name], gold["cases"][name]
    before = c["dev_rows"].clone()
    for limit in (c["limits"] or (300,)):
        table, offs, _ = _export(c, "target", limit=limit)
        assert torch.equal(table.cpu(), g[f"target_{limit}"]) and torch.equal(offs.cpu(), g[f"target_{limit}_offsets"]), (name, "target", limit)
    for form, key, kw in (("target", "target_300", {}), ("txt", "txt", {}), ("json", "json", {}), ("txt", "detect", dict(round_boxes=True, reverse=True))):
        table, offs, hist = _export(c, form, nc=c["nc"], **kw)
        assert torch.equal(table.cpu(), g[key]), (name, key, (table.cpu() != g[key]).nonzero()[:4])
        assert torch.equal(offs.cpu(), g["offsets"]), (name, key)
        want = torch.stack([torch.bincount(c["rows"][i, :n, 5].long(), minlength=c["nc"]) for i, n in enumerate(c["counts"])]).int()
        assert torch.equal(hist.cpu(), want), (name, key)
    # the flags one at a time: rounding without the reversal is the detect table image by image back to front, and image0 moves the image column alone
    table, offs, _ = _export(c, "txt", round_boxes=True)
    back = torch.cat([g["detect"][a:b].flip(0) for a, b in zip(g["offsets"][:-1].tolist(), g["offsets"][1:].tolist())]) if table.shape[0] else g["detect"]
    assert torch.equal(table.cpu(), back), name
    table, _, _ = _export(c, "json", image0=1000)
    want = g["json"].clone()
    want[:, 0] += 1000
    assert torch.equal(table.cpu(), want), name
    assert torch.equal(c["dev_rows"], before)   # the rows are read, never written


@pytest.mark.parametrize("name", list(oc.CASES))
def test_export_rows_on_a_view_equals_the_contiguous_case(cases, gold, name):
    c, g = cases[name], gold["cases"][name]
    view = oc.as_view(c["dev_rows"])
    assert view.stride(1) == 7 and view.stride(0) > view.shape[1] * 7 and not view.is_contiguous()
    for form, key, kw in (("target", "target_300", {}), ("txt", "txt", {}), ("json", "json", {}), ("txt", "detect", dict(round_boxes=True, reverse=True))):
        table, offs, hist = _export(c, form, rows=view, nc=c["nc"], **kw)
        flat = _export(c, form, nc=c["nc"], **kw)
        assert torch.equal(table, flat[0]) and torch.equal(offs, flat[1]) and torch.equal(hist, flat[2]) and torch.equal(table.cpu(), g[key]), (name, key)


def test_export_rows_without_counts_and_with_a_short_table(cases, dev):
    """counts == NULL exports max_rows rows of every image; a table shorter than the counts say drops the rows past it and nothing else is written"""
    from yolov3_amd import _lib, ops

    c = cases["small"]
    rows = c["dev_rows"]
    bs, m = rows.shape[:2]
    table, offs, _ = ops.export_rows(rows, rows.stride(0), rows.stride(1), None, bs, m, "target", bs * m)
    assert offs.tolist() == [i * m for i in range(bs + 1)]
    r = c["rows"]
    want = torch.stack((torch.arange(bs).repeat_interleave(m).float(), r[..., 5].reshape(-1), ((r[..., 0] + r[..., 2]) / 2).reshape(-1), ((r[..., 1] + r[..., 3]) / 2).reshape(-1),
                        (r[..., 2] - r[..., 0]).reshape(-1), (r[..., 3] - r[..., 1]).reshape(-1), r[..., 4].reshape(-1)), 1)
    assert torch.equal(table.cpu(), want)
    with pytest.raises(_lib.Y3Error, match="capacity"):
        ops.export_rows(rows, rows.stride(0), rows.stride(1), None, bs, m, "target", bs * m - 1)
    total = sum(c["counts"])
    full, _, _ = ops.export_rows(rows, rows.stride(0), rows.stride(1), c["dev_counts"], bs, m, "target", total)
    guard = torch.full((total + 4, 7), -1.0, device=dev)
    short = guard[: total - 3]
    check = ops._lib.lib().y3_export_rows(rows.data_ptr(), rows.stride(0), rows.stride(1), c["dev_counts"].data_ptr(), bs, m, 0, 0, 0, 0, 0, None, short.data_ptr(), total - 3,
                                          torch.empty(bs + 1, dtype=torch.int32, device=dev).data_ptr(), None, 0, ops.stream_ptr())
    assert check == 0
    assert torch.equal(guard[: total - 3], full[: total - 3]) and bool((guard[total - 3:] == -1.0).all())


@pytest.mark.parametrize("name", list(oc.CASES))
def test_output_to_target_both_input_forms(cases, gold, name, dev):
    from yolov3_amd import outputs

    c, g = cases[name], gold["cases"][name]
    views = [c["dev_rows"][i, :n] for i, n in enumerate(c["counts"])]                 # the list non_max_suppression returns: views of one buffer
    copies = [v.clone() for v in views]                                                # any other list: gathered first
    for limit in (c["limits"] or (300,)):
        want = g[f"target_{limit}"].numpy()
        for out in (views, copies, (c["dev_rows"], c["dev_counts"]), (c["dev_rows"], c["counts"]), (c["dev_rows"], c["dev_counts"], c["counts"])):
            got = outputs.output_to_target(out, max_det=limit)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, want), (name, limit)
    block = outputs._padded(views)
    assert block[0].data_ptr() == c["dev_rows"].data_ptr() and block[1:3] == (c["dev_rows"].stride(0), 6)   # used where it lies


def test_list_form_is_one_launch_and_one_copy(cases, gold, monkeypatch):
    from yolov3_amd import ops, outputs

    c = cases["wide"]
    views = [c["dev_rows"][i, :n] for i, n in enumerate(c["counts"])]
    log = []
    real = ops.export_rows
    monkeypatch.setattr(ops, "export_rows", lambda *a, **k: (log.append("launch"), real(*a, **k))[1])
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                log.append(_name)
            return _orig(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, counted)
    got = outputs.output_to_target(views, max_det=7)
    monkeypatch.undo()
    assert log == ["launch", "cpu"], log
    assert np.array_equal(got, gold["cases"]["wide"]["target_7"].numpy())


@pytest.mark.parametrize("name", oc.TXT_CASES)
def test_txt_writers_reproduce_the_reference_bytes(cases, gold, name, tmp_path):
    from yolov3_amd import outputs

    c, g = cases[name], gold["cases"][name]
    for save_conf in (False, True):
        want = g[f"files_conf{int(save_conf)}"]
        one = tmp_path / f"one{int(save_conf)}"
        one.mkdir()
        for i, n in enumerate(c["counts"]):   # the per-image function, on the (n, 6) view val.py hands it; called for empty images too: no file
            outputs.save_one_txt(c["dev_rows"][i, :n], save_conf, c["shapes"][i], one / f"{Path(c['paths'][i]).stem}.txt")
        assert _read_dir(one) == want, (name, save_conf)
        for counts in (c["counts"], (c["dev_counts"], c["counts"]), c["dev_counts"]):
            folder = tmp_path / f"batched{int(save_conf)}_{type(counts).__name__}"
            written = outputs.save_txt_batched(c["dev_rows"], counts, c["shapes"], c["paths"], folder, save_conf)
            assert _read_dir(folder) == want and sorted(f.name for f in written) == sorted(want), (name, save_conf)
        if name == "detect":
            folder = tmp_path / f"detect{int(save_conf)}"
            outputs.save_txt_batched(c["dev_rows"], c["counts"], c["shapes"], c["paths"], folder, save_conf, detect=True)
            assert _read_dir(folder) == g[f"detect_files_conf{int(save_conf)}"] and _read_dir(folder) != want
    # append mode: a second call doubles every file
    folder = tmp_path / "twice"
    for _ in range(2):
        outputs.save_txt_batched(c["dev_rows"], c["counts"], c["shapes"], c["paths"], folder, True)
    assert _read_dir(folder) == {k: v + v for k, v in g["files_conf1"].items()}


@pytest.mark.parametrize("name", oc.JSON_CASES)
def test_json_writers_reproduce_the_reference_jdict(cases, gold, name):
    from yolov3_amd import outputs

    c, g = cases[name], gold["cases"][name]
    class_map = outputs.coco80_to_coco91_class() if c["nc"] == 80 else list(range(1000))
    one = []
    for i, n in enumerate(c["counts"]):
        outputs.save_one_json(c["dev_rows"][i, :n], one, Path(c["paths"][i]), class_map)
    batched = [{"kept": True}]
    assert outputs.save_json_batched(c["dev_rows"], (c["dev_counts"], c["counts"]), c["paths"], batched, class_map) is batched
    assert one == g["jdict"] and batched == [{"kept": True}] + g["jdict"]
    assert json.loads(json.dumps(one)) == g["jdict"]


def test_detections_strings_from_the_export_histogram(cases, gold, dev, monkeypatch):
    from yolov3_amd import Detections, outputs

    c = cases["detect"]
    ims = [np.zeros((*s, 3), np.uint8) for s in c["shapes"]]
    pred = [c["dev_rows"][i, :n] for i, n in enumerate(c["counts"])]
    d = Detections(ims, pred, [Path(p).name for p in c["paths"]], oc.TIMES, dict(enumerate(oc.NAMES)), oc.DETECTIONS_SHAPE)
    calls = []
    real = outputs.export_table
    monkeypatch.setattr(outputs, "export_table", lambda *a, **k: (calls.append(k.get("nc")), real(*a, **k))[1])
    assert str(d) == gold["detections"]["str"] and calls == [80]
    monkeypatch.undo()
    frames = d.pandas()
    for k, want in gold["detections"]["pandas"].items():
        for df, (columns, values) in zip(getattr(frames, k), want):
            assert list(df.columns) == columns and df.values.tolist() == values, k


def _tiny(dev, golden_dir):
    from yolov3_amd import DetectMultiBackend, compat

    m = DetectMultiBackend(str(golden_dir / "ref_tiny_w025_fp16.pt"), device=dev, fp16=False)   # the checkpoint whose eval output ref_tiny_w025_eval.pt records
    compat.uninstall_aliases()
    return m


def _e2e_batches():
    """two batches of three 96x160 letterboxed images whose native sizes differ (ratio / pad as the dataloader reports them)"""
    shapes = [((180, 320), ((0.5, 0.5), (0.0, 3.0))), ((96, 160), ((1.0, 1.0), (0.0, 0.0))), ((135, 240), ((2 / 3, 2 / 3), (0.0, 3.0)))]
    out = []
    for b in range(2):
        g = torch.Generator().manual_seed(40 + b)
        im = torch.rand(3, 3, 96, 160, generator=g)
        targets = torch.tensor([[0, 1, 0.5, 0.5, 0.3, 0.4], [0, 2, 0.3, 0.6, 0.2, 0.2], [2, 0, 0.6, 0.4, 0.5, 0.5]])
        out.append((im, targets, [f"/data/val/{(7 + 3 * b + i):012d}.jpg" if i != 1 else f"/data/val/frame_{b}.jpg" for i in range(3)], shapes))
    return out


def test_run_batches_writes_what_the_per_image_writers_write(dev, golden_dir, tmp_path):
    from yolov3_amd import coco80_to_coco91_class, non_max_suppression, outputs, run_batches, scale_boxes

    m = _tiny(dev, golden_dir)
    nc, conf = 80, 1e-4   # (the random-weight checkpoint scores obj x cls around 2e-4: nothing passes val.py's 0.001)
    batches = _e2e_batches()
    class_map = list(range(1000))
    caller = [{"mine": 1}]
    with torch.no_grad():
        plain = run_batches(m, [(im, t, s) for im, t, _, s in batches], nc, conf_thres=conf)
        again = run_batches(m, batches, nc, conf_thres=conf)                                # a 4-tuple without the flags: the paths are ignored
        saved = run_batches(m, batches, nc, conf_thres=conf, save_txt=True, save_conf=True, save_json=True, save_dir=tmp_path / "run", class_map=class_map, jdict=caller)
        run_batches(m, batches, nc, conf_thres=conf, save_txt=True, save_json="mine.json", save_dir=tmp_path / "run2", single_cls=True)
        # the per-image loop of val.py:379-413 with this package's reference-signature functions
        want_dir, jdict = tmp_path / "want", []
        want_dir.mkdir()
        total = 0
        for im, targets, paths, shapes in batches:
            pred = m(im.to(dev))[0]
            for si, det in enumerate(non_max_suppression(pred, conf, 0.6, multi_label=True, max_det=300)):
                if det.shape[0] == 0:
                    continue
                predn = det.clone()
                scale_boxes(im.shape[2:], predn[:, :4], shapes[si][0], shapes[si][1])
                outputs.save_one_txt(predn, True, shapes[si][0], want_dir / f"{Path(paths[si]).stem}.txt")
                outputs.save_one_json(predn, jdict, Path(paths[si]), class_map)
                total += det.shape[0]
    assert total > 0 and len(jdict) == total
    assert plain[0] == again[0] == saved[0] and all(np.array_equal(a, b) for a, b in ((plain[1], again[1]), (plain[1], saved[1])))
    assert saved[2].n == plain[2].n == total
    assert _read_dir(tmp_path / "run" / "labels") == _read_dir(want_dir) and len(_read_dir(want_dir)) > 0
    assert caller[0] == {"mine": 1} and caller[1:] == jdict
    assert (tmp_path / "run" / "predictions.json").read_bytes() == json.dumps(caller).encode()
    assert sorted(p.name for p in (tmp_path / "run").iterdir()) == ["labels", "predictions.json"]
    # single_cls: the class column is zeroed before the writers (val.py:394-395); save_conf off: five numbers per line; the named file
    lines = b"".join(_read_dir(tmp_path / "run2" / "labels").values()).decode().splitlines()
    assert lines and all(ln.startswith("0 ") and len(ln.split()) == 5 for ln in lines)
    assert {e["category_id"] for e in json.loads((tmp_path / "run2" / "mine.json").read_text())} == {0}
    assert coco80_to_coco91_class()[0] == 1


def test_detect_batches_output_through_the_detect_writer(dev, golden_dir, tmp_path):
    """detect.py:196-236 for a batch: detect_batches -> scale_boxes -> save_txt_batched(detect=True), against that loop's own order of operations on the
    host (round half to even, last row first, xywh / gn in fp32) built from torch tensor operations"""
    from yolov3_amd import detect_batches, outputs, scale_boxes

    m = _tiny(dev, golden_dir)
    (im, _, paths, shapes), _ = _e2e_batches()
    with torch.no_grad():
        dets = next(iter(detect_batches(m, [im.to(dev)], conf_thres=1e-4, iou_thres=0.6, max_det=40)))
    counts = [int(d.shape[0]) for d in dets]
    assert sum(counts) > 0
    for d, (shape, ratio_pad) in zip(dets, shapes):
        scale_boxes(im.shape[2:], d[:, :4], shape, ratio_pad)   # in place on the views, as detect.py:223 does
    block, step, rs, _, most = outputs._padded(dets)
    assert block.data_ptr() == dets[0].data_ptr() and step == 40 * 6   # NMS's own buffer, where it lies
    outputs.save_txt_batched(block, counts, [s[0] for s in shapes], paths, tmp_path / "labels", save_conf=True, detect=True)
    want = {}
    for d, (shape, _), p in zip(dets, shapes, paths):
        d = d.cpu()
        if d.shape[0] == 0:
            continue
        box = d[:, :4].round().flip(0)
        xywh = torch.stack(((box[:, 0] + box[:, 2]) / 2, (box[:, 1] + box[:, 3]) / 2, box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]), 1) / torch.tensor(shape)[[1, 0, 1, 0]]
        rows = torch.cat((d[:, 5:6].flip(0), xywh, d[:, 4:5].flip(0)), 1).tolist()
        want[f"{Path(p).stem}.txt"] = "".join(("%g " * 6).rstrip() % tuple(r) + "\n" for r in rows).encode()
    assert _read_dir(tmp_path / "labels") == want
