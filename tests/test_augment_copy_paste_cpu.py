"""CPU tests of copy-paste in the train-mode dataset (yolov3_amd/augment.py, csrc/augment.hip): the NumPy statement of tests/augment_copy_paste_cases.py against the
fixture of the unmodified reference (tests/golden/make_augment_copy_paste_golden.py) and, where the reference tree is present, against the live reference; the fill
rule against properties that do not depend on it and against Pillow; the draws; the keyword and its default; the table the host sends; the header."""
import random
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import augment_cases as ac  # noqa: E402
import augment_copy_paste_cases as cpc  # noqa: E402
import augment_polygon_cases as apc  # noqa: E402

NEW_SYMBOLS = ["y3_augment_copy_paste_select", "y3_augment_copy_paste_raster", "y3_augment_batch_paste", "y3_augment_polygons_paste", "y3_augment_targets_paste"]
CASES = cpc.cases()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "augment_copy_paste.pt", weights_only=True)   # data only


@pytest.fixture(scope="module")
def data():
    labels, segments = apc.make_polygons()
    return SimpleNamespace(images=ac.make_images(), labels=labels, segments=segments, counts=[len(sg) for sg in segments])


@pytest.fixture(autouse=True)
def _generators_left_alone():
    state = random.getstate(), np.random.get_state()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])


def _seed(seed):
    random.seed(seed)
    np.random.seed(seed)


def test_the_cases_are_what_the_issue_lists():
    assert list(CASES) == [f"{b}_{p}" for b in ("exact", "low", "wild") for p in (0.1, 0.5, 1.0)]
    for name, c in CASES.items():
        base = apc.CASES[c["base"]]
        assert c["hyp"] == dict(base["hyp"], copy_paste=float(name.split("_")[1])) and c["indices"] == base["indices"]
    assert CASES["wild_0.5"]["hyp"]["mixup"] > 0


@pytest.mark.parametrize("case", list(CASES))
def test_the_statement_and_the_draws_reproduce_the_fixture(gold, data, case):
    """draw_item makes copy_paste's random.sample at the reference's place (both generators end where the reference left them), and the statement over those draws
    gives the reference's targets, accepted lists, masks and images"""
    from yolov3_amd import draw_item

    c, g = CASES[case], gold["cases"][case]
    epoch = c["indices"] if c["indices"] is not None else list(range(len(ac.IMAGES)))
    assert g["indices"] == epoch
    _seed(c["seed"])
    for k, want in enumerate(g["batches"]):
        items = [draw_item(i, ac.hw(), c["hyp"], ac.IMG_SIZE, epoch, len(ac.IMAGES), True, data.counts) for i in epoch[k * ac.BATCH : (k + 1) * ac.BATCH]]
        assert [list(it.mosaics[m].paste) if m < len(it.mosaics) else [] for it in items for m in range(2)] == want["pastes"]
        st = cpc.batch_statement(items, data.images, data.labels, data.segments, ac.hw(), ac.IMG_SIZE)
        assert np.array_equal(st["targets"].view(np.int32), want["targets"].numpy().view(np.int32)), f"{case}: targets of batch {k}"
        assert cpc.crc(st["im"]) == want["im_crc"] and np.array_equal(st["words"], want["words"].numpy())
        assert [[(e, j) for e, j, _ in a] for a in st["accepted"]] == [[(e, j) for e, j, _ in a] for a in want["accepted"]]
        assert all(np.array_equal(b.view(np.int32), wb.numpy().view(np.int32)) for a, wa in zip(st["accepted"], want["accepted"]) for (_, _, b), (_, _, wb) in zip(a, wa))
        assert [-1 if m is None else cpc.crc(np.packbits(m, axis=1, bitorder="little")) for m in st["masks"]] == want["mask_crc"]
    assert random.random() == g["batches"][-1]["next_random"] and float(np.random.random()) == g["batches"][-1]["next_np_random"]


def test_the_fixture_holds_every_situation(gold, data):
    """the generator's counters, stored with the fixture, name all eight situations of its check_situations and none is zero; they are counted again here from the
    draws and the statement (no reference needed), and three of them once more from the stored lists alone"""
    from yolov3_amd import draw_item

    SITUATIONS, examine, new_stats = cpc.SITUATIONS, cpc.examine, cpc.new_stats
    assert set(gold["situations"]) == set(SITUATIONS) and len(SITUATIONS) == 9 and all(v > 0 for v in gold["situations"].values())   # (the survivor pair counts as two)
    stats = new_stats()
    for c in CASES.values():
        epoch = c["indices"] if c["indices"] is not None else list(range(len(ac.IMAGES)))
        _seed(c["seed"])
        for i in epoch:
            item = draw_item(i, ac.hw(), c["hyp"], ac.IMG_SIZE, epoch, len(ac.IMAGES), True, data.counts)
            examine(item, cpc.paste_labels(item, data.labels, data.segments, ac.hw(), ac.IMG_SIZE), data.labels, data.segments, ac.hw(), stats)
    assert stats == gold["situations"]
    mixed = k_zero = both = 0
    for g in gold["cases"].values():
        for b in g["batches"]:
            for js, acc in zip(b["pastes"], b["accepted"]):
                mixed += int(0 < len(acc) < len(js))
            k_zero += sum(int(not js) for js in b["pastes"][0::2])
            both += sum(int(len(a) > 0 and len(c) > 0) for a, c in zip(b["accepted"][0::2], b["accepted"][1::2]))
    assert mixed and k_zero and both


def test_the_statement_reproduces_the_live_reference(gold):
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("the reference tree is not readable here")
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import tempfile

    import make_augment_copy_paste_golden as gen
    import make_augment_polygons_golden as pgen

    with tempfile.TemporaryDirectory() as tmp:   # run_case asserts, per item, statement == reference: draws, appended rows, pasted canvas, image, targets
        pgen.write_tree(Path(tmp))
        live = gen.run_case(gen.reference(), Path(tmp), "exact_0.5", gen.new_stats())
    g = gold["cases"]["exact_0.5"]
    assert live["indices"] == g["indices"] and len(live["batches"]) == len(g["batches"])
    for a, b in zip(live["batches"], g["batches"]):
        assert torch.equal(a["targets"], b["targets"]) and a["im_crc"] == b["im_crc"] and a["mask_crc"] == b["mask_crc"] and a["pastes"] == b["pastes"] and a["next_random"] == b["next_random"]


def test_bbox_ioa_is_the_published_definition():
    box = np.array([[10, 10, 30, 20]], dtype=np.float32)
    rows = np.array([[10, 10, 30, 20], [20, 15, 40, 25], [0, 0, 5, 5], [30, 20, 50, 40], [12, 12, 14, 14], [7, 7, 7, 7]], dtype=np.float32)
    got = cpc.bbox_ioa(box, rows)
    assert got.dtype == np.float32 and got.shape == (1, 6)
    want = [200 / (200 + 1e-7), 50 / 200, 0.0, 0.0, 1.0, 0.0]   # over the area of the ROW: a small row inside the box is fully covered
    assert np.allclose(got[0], want, rtol=1e-6, atol=0)


def _even_odd(pts, xs, ys):
    """the exact even-odd test of pixel centres (no rule of the statement's is used)"""
    inside = np.zeros(xs.shape, dtype=bool)
    p = np.asarray(pts, dtype=np.float64)
    for (x0, y0), (x1, y1) in zip(np.roll(p, 1, 0), p):
        if y0 == y1:
            continue
        cross = ((y0 <= ys) != (y1 <= ys)) & (xs < x0 + (ys - y0) * (x1 - x0) / (y1 - y0))
        inside ^= cross
    return inside


def _edge_distance(pts, xs, ys):
    p = np.asarray(pts, dtype=np.float64)
    best = np.full(xs.shape, np.inf)
    for a, b in zip(np.roll(p, 1, 0), p):
        ab = b - a
        t = np.zeros(xs.shape) if not ab.any() else np.clip(((xs - a[0]) * ab[0] + (ys - a[1]) * ab[1]) / (ab @ ab), 0, 1)
        best = np.minimum(best, np.hypot(xs - (a[0] + t * ab[0]), ys - (a[1] + t * ab[1])))
    return best


def _random_polygons(n, w):
    rs = np.random.RandomState(7)
    return [rs.randint(0, w + 1, (int(rs.randint(3, 10)), 2)) for _ in range(n)]   # vertices on 0 and on w (outside the canvas) included


def test_the_fill_rule_has_the_properties_that_do_not_depend_on_it():
    for x1, y1, x2, y2 in ((3, 4, 20, 17), (0, 0, 31, 31), (5, 5, 5, 9), (2, 30, 29, 31)):   # an axis-aligned integer rectangle fills its inclusive pixel rectangle
        want = np.zeros((32, 32), dtype=bool)
        want[y1 : y2 + 1, x1 : x2 + 1] = True
        assert np.array_equal(cpc.fill_mask(32, 32, [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]), want)
    w = 48
    ys, xs = np.mgrid[0:w, 0:w].astype(np.float64)
    for pts in _random_polygons(150, w):
        m, inside, dist = cpc.fill_mask(w, w, pts), _even_odd(pts, xs, ys), _edge_distance(pts, xs, ys)
        assert m[inside & (dist > 1)].all() and not m[~inside & (dist > 1)].any(), pts.tolist()
    # degenerate polygons set exactly their line pixels
    assert np.argwhere(cpc.fill_mask(16, 16, [[5, 7]])).tolist() == [[7, 5]]
    assert np.argwhere(cpc.fill_mask(16, 16, [[0, 0]] * 3)).tolist() == [[0, 0]]
    line = cpc.fill_mask(16, 16, [[2, 3], [10, 9]])
    assert np.array_equal(np.argwhere(line)[:, ::-1].tolist(), sorted(cpc.line_pixels(16, 16, (2, 3), (10, 9)), key=lambda p: (p[1], p[0]))) and line.sum() == 9
    assert not cpc.fill_mask(16, 16, [[16, 5]]).any() and not cpc.fill_mask(16, 16, [[16, 2], [16, 9], [16, 16]]).any()   # a vertex at 2 S lies outside the canvas


def test_the_fill_rule_agrees_with_pillow_away_from_the_edges():
    Image, ImageDraw = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageDraw")
    w = 48
    ys, xs = np.mgrid[0:w, 0:w].astype(np.float64)
    for pts in _random_polygons(150, w):
        im = Image.new("L", (w, w), 0)
        ImageDraw.Draw(im).polygon([tuple(int(v) for v in p) for p in pts], fill=1, outline=1)
        differ = cpc.fill_mask(w, w, pts) != np.array(im).astype(bool)
        assert not (differ & (_edge_distance(pts, xs, ys) > 1)).any(), pts.tolist()


def test_a_box_only_set_makes_no_draw_and_packs_the_same_records(data):
    from yolov3_amd import augment

    hyp = dict(ac.CASES["wild"]["hyp"], copy_paste=0.5)
    _seed(4)
    plain = [augment.draw_item(i, ac.hw(), dict(hyp, copy_paste=0.0), ac.IMG_SIZE, None, 12, True) for i in range(12)]
    after = random.getstate(), np.random.get_state()
    _seed(4)
    keyed = [augment.draw_item(i, ac.hw(), hyp, ac.IMG_SIZE, None, 12, True, [0] * 12) for i in range(12)]
    now = random.getstate(), np.random.get_state()
    assert now[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(now[1], after[1]))
    assert not any(mo.paste for it in keyed for mo in it.mosaics) and augment.pack_items(keyed).tobytes() == augment.pack_items(plain).tobytes()
    # a letterbox item never pastes, whatever the set holds; and the draw consumes nothing when k == 0
    _seed(4)
    single = [augment.draw_item(i, ac.hw(), dict(hyp, mosaic=0.0), ac.IMG_SIZE, None, 12, True, data.counts) for i in range(12)]
    assert not any(it.mosaic or mo.paste for it in single for mo in it.mosaics)
    _seed(4)
    none = [augment.draw_item(i, ac.hw(), dict(hyp, copy_paste=0.01), ac.IMG_SIZE, None, 12, True, data.counts) for i in range(12)]   # round(0.01 n) == 0
    now = random.getstate(), np.random.get_state()
    assert now[0] == after[0] and not any(mo.paste for it in none for mo in it.mosaics)


def test_the_paste_table(data):
    from yolov3_amd import augment

    c = CASES["wild_0.5"]
    _seed(c["seed"])
    items = [augment.draw_item(i, ac.hw(), c["hyp"], ac.IMG_SIZE, c["indices"], 12, True, data.counts) for i in c["indices"][:4]]
    table, nk, masks = augment.pack_paste(items)
    ks = [len(it.mosaics[m].paste) if m < len(it.mosaics) else 0 for it in items for m in range(2)]
    assert table.dtype == np.int32 and table.shape == (4 * 4 + 1 + sum(ks),) and nk == sum(ks) > 0 and masks == sum(k > 0 for k in ks)
    assert table[:9].tolist() == [0] + np.cumsum(ks).tolist()
    idx = table[9:17].tolist()
    assert [i for i in idx if i >= 0] == list(range(masks)) and [i >= 0 for i in idx] == [k > 0 for k in ks]
    assert table[17:].tolist() == [j for it in items for mo in it.mosaics for j in mo.paste]
    for it in items:
        for mo in it.mosaics:
            n = sum(data.counts[j] for j in mo.indices)
            assert len(mo.paste) == round(0.5 * n) and len(set(mo.paste)) == len(mo.paste) and all(0 <= j < n for j in mo.paste)


def _ds(data, hyp, cls=None, **kw):
    from yolov3_amd import DeviceRectTrainDataset, DeviceTrainDataset

    args = dict(img_size=ac.IMG_SIZE, batch_size=ac.BATCH, stride=ac.STRIDE, shapes0=ac.hw0(), paths=ac.paths(), device="cpu")
    args.update(kw)
    return (DeviceRectTrainDataset if cls == "rect" else DeviceTrainDataset)(data.images, data.labels, hyp, **args)


def test_the_keyword_and_its_default(data, monkeypatch):
    from yolov3_amd import DeviceTrainDataset, dataset

    def no_upload(*a, **k):
        raise AssertionError("an upload was attempted")

    monkeypatch.setattr(dataset, "_upload", no_upload)
    monkeypatch.setattr(dataset, "_upload_arena", no_upload)
    hyp = dict(ac.CASES["low"]["hyp"], copy_paste=0.1)
    for kw in (dict(), dict(segments=data.segments), dict(copy_paste=False)):   # the default still refuses, with the same text
        with pytest.raises(ValueError, match=r"DeviceTrainDataset: hyp\['copy_paste'\] = 0.1; copy-paste is not built"):
            _ds(data, hyp, **kw)
    with pytest.raises(ValueError, match=r"DeviceRectTrainDataset: hyp\['copy_paste'\] = 0.1; copy-paste is not built"):
        _ds(data, hyp, "rect", stride=16)
    for kw in (dict(), dict(segments=data.segments)):   # with the keyword the hyp is accepted: the device is what is missing
        with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
            _ds(data, hyp, copy_paste=True, **kw)
    with pytest.raises(ValueError, match="perspective"):   # the other refusals stand
        _ds(data, dict(hyp, perspective=0.001), copy_paste=True)
    ref = SimpleNamespace(ims=data.images, im_hw0=ac.hw0(), im_hw=ac.hw(), labels=data.labels, segments=data.segments, im_files=ac.paths(), rect=False, img_size=64, stride=32,
                          augment=True, mosaic=True, hyp=hyp, indices=range(12))
    with pytest.raises(ValueError, match="copy-paste is not built"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU"):
        DeviceTrainDataset.from_dataset(ref, batch_size=4, device="cpu", copy_paste=True)


def test_the_header_declares_the_new_exports_at_abi_6():
    from yolov3_amd import _lib, augment, ops

    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and declared == set(_lib.exported_symbols()) and not set(NEW_SYMBOLS) & set(_lib._QUERIES)
    assert "#define Y3_ABI_VERSION 6" in re.sub(r"[ \t]+", " ", header) and _lib.ABI_VERSION == 6
    assert (augment.TILE.itemsize, augment.MOSAIC.itemsize, augment.ITEM.itemsize) == (40, 280, 1360) and len(re.findall(r"typedef\s+struct", header)) == 10   # no new record
    assert len(_lib._SIGNATURES["y3_augment_batch"][1]) == 10 and len(_lib._SIGNATURES["y3_augment_polygons"][1]) == 15 and len(_lib._SIGNATURES["y3_augment_targets_polygons"][1]) == 14
    assert callable(ops.augment_copy_paste)
    assert all(s in (ROOT / "INTEGRATION.md").read_text() for s in NEW_SYMBOLS)
    source = (ROOT / "yolov3_amd" / "csrc" / "augment.hip").read_text()
    assert all(f'extern "C" int {s}(' in source for s in NEW_SYMBOLS)
    assert all("copy_paste" in (ROOT / f).read_text() for f in ("README.md", "DESIGN.md", "INTEGRATION.md", "tools/README.md"))


def test_the_new_exports_reject_bad_arguments_without_a_gpu():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.lib()
    P = 1 << 20   # a fake, aligned device address: validation never dereferences it

    def fails(status, *needles):
        msg = lib.y3_last_error()
        assert status != 0 and all(n in msg for n in needles), (status, msg)

    def select(labels=P, loff=P, voff=P, nv=100, rows=26, images=P, n=12, items=P, count=4, S=64, paste=P, nk=5, sel_i=P, sel_f=P):
        return lib.y3_augment_copy_paste_select(labels, loff, voff, nv, rows, images, n, items, count, S, paste, nk, sel_i, sel_f, None)

    for null in ("labels", "loff", "voff", "images", "items", "paste", "sel_i", "sel_f"):
        fails(select(**{null: None}), b"y3_augment_copy_paste_select", b"null")
    fails(select(nk=0), b"y3_augment_copy_paste_select", b"candidates")
    fails(select(S=72), b"y3_augment_copy_paste_select", b"72 is not a multiple of 16")
    fails(select(paste=P + 2), b"y3_augment_copy_paste_select", b"aligned")
    fails(select(count=1025), b"y3_augment_copy_paste_select", b"geometry")

    def raster(verts=P, nv=100, voff=P, rows=26, loff=P, images=P, n=12, items=P, count=4, S=64, paste=P, nk=5, sel_i=P, masks=P, n_masks=2):
        return lib.y3_augment_copy_paste_raster(verts, nv, voff, rows, loff, images, n, items, count, S, paste, nk, sel_i, masks, n_masks, None)

    for null in ("verts", "voff", "loff", "images", "items", "paste", "sel_i", "masks"):
        fails(raster(**{null: None}), b"y3_augment_copy_paste_raster", b"null")
    fails(raster(n_masks=9), b"y3_augment_copy_paste_raster", b"geometry")   # more masks than mosaics
    fails(raster(n_masks=0), b"y3_augment_copy_paste_raster", b"geometry")
    fails(raster(masks=P + 2), b"y3_augment_copy_paste_raster", b"aligned")

    def batch(arena=P, nbytes=4096, images=P, n=12, items=P, count=4, dst=P, dt=3, S=64, paste=P, masks=P, n_masks=2):
        return lib.y3_augment_batch_paste(arena, nbytes, images, n, items, count, dst, dt, S, paste, masks, n_masks, None)

    for null in ("arena", "images", "items", "dst", "paste", "masks"):
        fails(batch(**{null: None}), b"y3_augment_batch_paste", b"null")
    fails(batch(n_masks=9), b"y3_augment_batch_paste", b"geometry")
    fails(batch(dt=7), b"y3_augment_batch_paste", b"dtype")

    def polygons(verts=P, nv=100, voff=P, rows=26, loff=P, images=P, n=12, items=P, count=4, S=64, paste=P, nk=5, sel_i=P, sel_f=P, boxes=P, inside=P, paths=P, n_rows=30):
        return lib.y3_augment_polygons_paste(verts, nv, voff, rows, loff, images, n, items, count, S, paste, nk, sel_i, sel_f, boxes, inside, paths, n_rows, None)

    for null in ("verts", "voff", "loff", "images", "items", "paste", "sel_i", "sel_f", "boxes", "inside", "paths"):
        fails(polygons(**{null: None}), b"y3_augment_polygons_paste", b"null")
    fails(polygons(n_rows=-1), b"y3_augment_polygons_paste", b"geometry")
    fails(polygons(boxes=P + 4), b"y3_augment_polygons_paste", b"aligned")

    def targets(labels=P, loff=P, images=P, n=12, items=P, count=4, S=64, paste=P, nk=5, sel_i=P, sel_f=P, boxes=P, inside=P, paths=P, out=P, rows=9, out_offsets=P):
        return lib.y3_augment_targets_paste(labels, loff, images, n, items, count, S, paste, nk, sel_i, sel_f, boxes, inside, paths, out, rows, out_offsets, None)

    for null in ("labels", "loff", "images", "items", "paste", "sel_i", "sel_f", "boxes", "inside", "paths", "out", "out_offsets"):
        fails(targets(**{null: None}), b"y3_augment_targets_paste", b"null")
    fails(targets(rows=-1), b"y3_augment_targets_paste", b"geometry")
    fails(targets(sel_f=P + 2), b"y3_augment_targets_paste", b"aligned")


def test_cpu_tensors_are_refused():
    from yolov3_amd import ops

    z, items = torch.zeros(32 * 12, dtype=torch.uint8), torch.zeros(4 * 1360, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_copy_paste(torch.zeros(4, 5), torch.zeros(13, dtype=torch.int64), torch.zeros(8, 2), torch.zeros(5, dtype=torch.int64), torch.zeros(64, dtype=torch.uint8), z, 12,
                               items, 4, 64, 9, torch.zeros(22, dtype=torch.int32), 5, 2)
