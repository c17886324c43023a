"""GPU tests of the device-side apply_classifier (yolov3_amd/crops.py, csrc/crops.hip) against the fixture the unmodified reference wrote
(tests/golden/classifier_crops.pt) and the NumPy statement of tests/classifier_crops_cases.py, which is computed once per module on the host.  Everything is
compared with torch.equal: the boxes and the crops are integer arithmetic and one IEEE division, the filter a comparison of integers."""
import numpy as np
import pytest
import torch

import classifier_crops_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "classifier_crops.pt", weights_only=True)


@pytest.fixture(scope="module")
def case():
    ims, x = cc.build_case()
    st = cc.statement(ims, x)
    live = [i for i, d in enumerate(x) if d is not None and len(d)]
    want = torch.cat([cc.to_float(st["crops"][i]) for i in live], 0)
    return dict(ims=ims, x=x, st=st, live=live, crops=want)


@pytest.fixture(scope="module")
def device_images(case):
    from yolov3_amd import DeviceImages

    return DeviceImages(case["ims"], DEV)


def pack(x, fill=float("nan")):
    """a list of (n, 6) / empty / None entries -> (rows (bs, max, 6) on the device with `fill` beyond every count, counts_t, counts)"""
    counts = [0 if d is None else len(d) for d in x]
    rows = torch.full((len(x), max(max(counts), 1), 6), fill, dtype=torch.float32)
    for i, d in enumerate(x):
        if counts[i]:
            rows[i, : counts[i]] = d
    return rows.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), counts


def test_boxes_and_crops_equal_the_fixture_and_the_statement(gold, case, device_images):
    from yolov3_amd import classifier_crops

    rows, counts_t, counts = pack(case["x"])   # NaN beyond the counts: those rows are not read
    before = rows.clone()
    crops, boxes, prefix, status = classifier_crops(rows, counts_t, counts, cc.IMG1, device_images)
    assert torch.equal(rows.nan_to_num(-1.0), before.nan_to_num(-1.0))   # `rows` is not written
    assert prefix.tolist() == [0, 7, 15, 24, 24] and status.tolist() == [0]
    for i, n in enumerate(counts):
        assert torch.equal(boxes[i, n:].cpu(), torch.zeros(boxes.shape[1] - n, 4))
        if n:
            assert torch.equal(boxes[i, :n].cpu(), gold["boxes"][i]) and torch.equal(boxes[i, :n].cpu(), case["st"]["boxes"][i])
    assert crops.dtype == torch.float32 and crops.shape == (24, 3, cc.SIZE, cc.SIZE) and torch.equal(crops.cpu(), case["crops"])
    for key, u8 in gold["full"].items():   # the crops the fixture holds whole
        i, j = (int(v) for v in key.split(","))
        assert torch.equal(crops[int(prefix[i]) + j].cpu(), cc.to_float(u8.numpy()[None])[0])
    for dtype in (torch.float16, torch.bfloat16):
        low = classifier_crops(rows, counts_t, counts, cc.IMG1, device_images, dtype=dtype)[0]
        assert low.dtype == dtype and torch.equal(low, crops.to(dtype))
    from_list = classifier_crops(rows, counts_t, counts, cc.IMG1, case["ims"])   # plain arrays, uploaded for the call
    assert torch.equal(from_list[0], crops) and torch.equal(from_list[1], boxes)


def test_apply_classifier_end_to_end(gold, case, device_images):
    from yolov3_amd import apply_classifier, apply_classifier_batched

    model = cc.ToyClassifier().to(DEV)
    x = [None if d is None else d.to(DEV) for d in case["x"]]
    out = apply_classifier(x, model, torch.empty(1, 3, *cc.IMG1), device_images)
    assert len(model.seen) == 1 and model.seen[0].dtype == torch.float32 and torch.equal(model.seen[0].cpu(), case["crops"])   # one call, on the crops
    assert out[4] is None and out[3].shape == (0, 6)
    for i in case["live"]:
        assert torch.equal(out[i].cpu(), gold["kept"][i]) and torch.equal(out[i].cpu(), case["st"]["kept"][i])
    assert [len(d) for d in x if d is not None] == [7, 8, 9, 0]   # the caller's list is not changed
    # a list of arrays and an (h, w) pair in place of the batch
    again = apply_classifier(x, model, cc.IMG1, case["ims"])
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(again, out))
    # the batched convention; a half-precision classifier gets half-precision crops
    rows, counts_t, counts = pack(case["x"])
    half = cc.ToyClassifier().to(DEV).half()
    kept, kept_t, kept_n = apply_classifier_batched(rows, counts_t, counts, half, cc.IMG1, device_images)
    assert half.seen[0].dtype == torch.float16 and torch.equal(half.seen[0], model.seen[0].half())
    assert kept_n == [5, 5, 6, 0, 0] == kept_t.tolist() and kept.shape == rows.shape
    for i, n in enumerate(kept_n):
        assert torch.equal(kept[i, n:].cpu(), torch.zeros(kept.shape[1] - n, 6))
        if n:
            assert torch.equal(kept[i, :n].cpu(), gold["kept"][i])


@pytest.fixture(scope="module")
def hand(case):
    """tables made by hand over the 300 x 260 image and a 20 x 20 one: the whole image, a 1 x 1 cutout, a sliver; the second image's one cutout"""
    ims = [case["ims"][2], case["ims"][4]]
    boxes = torch.full((2, 4, 4), float("nan"))
    boxes[0, :3] = torch.tensor([[0.0, 0.0, 260.0, 300.0], [5.7, 7.2, 6.9, 8.1], [250.2, 3.9, 260.0, 297.5]])
    boxes[1, :1] = torch.tensor([[3.0, 2.0, 20.0, 19.9]])
    counts = [3, 1]
    want = {S: torch.cat([cc.to_float(cc.crops_u8(im, boxes[i, :n], S)) for i, (im, n) in enumerate(zip(ims, counts))], 0) for S in (8, 20, 224)}
    assert cc.cutouts(ims[0], boxes[0, :3])[1].shape == (1, 1, 3) and cc.cutouts(ims[0], boxes[0, :3])[0].shape == (300, 260, 3)
    return ims, boxes, counts, want


@pytest.mark.parametrize("S", [8, 20, 224])
def test_hand_made_tables(hand, S):
    from yolov3_amd import DeviceImages, ops

    ims, boxes, counts, want = hand
    di = DeviceImages(ims, DEV)
    b, counts_t, prefix = boxes.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), torch.tensor([0, 3], device=DEV)
    crops, status = ops.crop_resize(di.arena, di.records, b, counts_t, prefix, 4, S)
    assert status.tolist() == [0] and torch.equal(crops.cpu(), want[S][:4])
    assert torch.equal(crops[1].cpu(), cc.to_float(np.broadcast_to(ims[0][7:8, 5:6], (1, S, S, 3)))[0])   # the 1 x 1 cutout: its pixel everywhere
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(ops.crop_resize(di.arena, di.records, b, counts_t, prefix, 4, S, dtype)[0], crops.to(dtype))
    # an output that is not 16-byte aligned takes the element stores: the same values, and nothing outside it is written
    buf = torch.full((4 * 3 * S * S + 2,), -7.0, device=DEV)
    ops.crop_resize(di.arena, di.records, b, counts_t, prefix, 4, S, out=buf[1:-1].view(4, 3, S, S))
    assert torch.equal(buf[1:-1].view(4, 3, S, S), crops) and buf[0].item() == -7.0 and buf[-1].item() == -7.0


def test_counts_all_zero_launch_nothing(case, device_images):
    from yolov3_amd import apply_classifier_batched, classifier_crops, ops

    rows, counts_t, counts = pack([None] * 5)
    crops, boxes, prefix, status = classifier_crops(rows, counts_t, counts, cc.IMG1, device_images, size=20, dtype=torch.float16)
    assert crops.shape == (0, 3, 20, 20) and crops.dtype == torch.float16 and boxes.shape == (5, 1, 4) and not boxes.any() and prefix.tolist() == [0] * 5 and status.tolist() == [0]
    model = cc.ToyClassifier().to(DEV)
    kept, kept_t, kept_n = apply_classifier_batched(rows, counts_t, counts, model, cc.IMG1, device_images)
    assert kept_n == [0] * 5 and kept_t.tolist() == [0] * 5 and not model.seen
    out, st = ops.crop_resize(device_images.arena, device_images.records, torch.zeros(5, 1, 4, device=DEV), counts_t, prefix, 0, 20)
    assert out.shape == (0, 3, 20, 20) and st.tolist() == [0]


def test_a_crop_that_cannot_be_cut_is_zeros_and_counted(hand, case):
    from yolov3_amd import DeviceImages, apply_classifier, ops

    ims, boxes, counts, want = hand
    di = DeviceImages(ims, DEV)
    counts_t, prefix = torch.tensor(counts, dtype=torch.int32, device=DEV), torch.tensor([0, 3], device=DEV)
    bad = boxes.clone()
    bad[0, 1] = torch.tensor([10.0, 10.0, 10.9, 20.0])   # an empty cutout: w = 0
    crops, status = ops.crop_resize(di.arena, di.records, bad.to(DEV), counts_t, prefix, 4, 20)
    assert status.tolist() == [1] and not crops[1].any() and torch.equal(crops[[0, 2, 3]].cpu(), want[20][[0, 2, 3]])
    bad[0, 2] = torch.tensor([250.0, 3.0, 261.0, 297.0])   # a box outside its image (no clip was applied to it), and a NaN
    bad[1, 0, 0] = float("nan")
    crops, status = ops.crop_resize(di.arena, di.records, bad.to(DEV), counts_t, prefix, 4, 20, status=status)   # the word accumulates
    assert status.tolist() == [4] and not crops[1:].any() and torch.equal(crops[0].cpu(), want[20][0])
    # a record that points outside the arena: every crop of that image, and only those
    rec = di.records.clone()
    rec.view(torch.int64)[4] = di.arena.numel() - 64   # the second image's offset: 20 x 20 x 3 bytes do not fit behind it
    crops, status = ops.crop_resize(di.arena, rec, boxes.to(DEV), counts_t, prefix, 4, 8)
    assert status.tolist() == [1] and not crops[3].any() and torch.equal(crops[:3].cpu(), want[8][:3])
    kept, kept_t = ops.keep_matching(torch.ones(2, 4, 6, device=DEV), counts_t, prefix, torch.ones(4, dtype=torch.int64, device=DEV), boxes.to(DEV), di.arena, rec)
    assert kept_t.tolist() == [3, 0]   # a crop the status word counted never matches
    # the public call raises, naming the count: a detection far outside the letterboxed image has an empty cutout after the clip
    x = [torch.tensor([[100.0, 100.0, 140.0, 150.0, 0.9, 0.0], [5000.0, 100.0, 5040.0, 150.0, 0.8, 0.0]], device=DEV), None]
    with pytest.raises(ValueError, match="1 of 2 crops"):
        apply_classifier(x, cc.ToyClassifier().to(DEV), cc.IMG1, di)


def test_keep_matching_keeps_the_order_and_zeroes_the_rest(hand):
    from yolov3_amd import DeviceImages, ops

    ims = hand[0]
    di = DeviceImages(ims, DEV)
    g = torch.Generator().manual_seed(5)
    n, counts = 600, [600, 257]   # more than one pass of 256 rows, a count that ends one lane into a pass
    rows = torch.rand(2, n, 6, generator=g) * 100
    rows[..., 5] = torch.randint(0, 3, (2, n), generator=g).float() + 0.75   # (long) 2.75 == 2: truncation
    rows[1, 257:] = float("nan")
    classes = torch.randint(0, 3, (sum(counts),), generator=g)
    boxes = torch.tensor([0.0, 0.0, 10.0, 10.0]).repeat(2, n, 1)
    counts_t, prefix = torch.tensor(counts, dtype=torch.int32, device=DEV), torch.tensor([0, 600], device=DEV)
    kept, kept_t = ops.keep_matching(rows.to(DEV), counts_t, prefix, classes.to(DEV), boxes.to(DEV), di.arena, di.records)
    for i, (c, p) in enumerate(zip(counts, [0, 600])):
        want = rows[i, :c][rows[i, :c, 5].long() == classes[p : p + c]]
        assert 0 < len(want) < c and int(kept_t[i]) == len(want)
        assert torch.equal(kept[i, : len(want)].cpu(), want) and not kept[i, len(want) :].any()
    # a strided view of wider rows, as y3_scale_boxes takes it
    wide = torch.zeros(2, n, 8)
    wide[..., :6] = rows
    again = ops.keep_matching(wide.to(DEV)[..., :6], counts_t, prefix, classes.to(DEV), boxes.to(DEV), di.arena, di.records)
    assert torch.equal(again[0], kept) and torch.equal(again[1], kept_t)


def test_detections_crop(case, tmp_path):
    from PIL import Image

    from yolov3_amd import Detections

    ims = case["ims"][:4]
    g = np.random.RandomState(9)
    pred = []
    for im, n in zip(ims, (5, 3, 4, 0)):   # native pixels; some boxes reach over the edge so that the clip acts
        h, w = im.shape[:2]
        xy = np.stack([g.uniform(-5, w - 20, n), g.uniform(-5, h - 20, n)], 1)
        wh = np.stack([g.uniform(4, 60, n), g.uniform(4, 60, n)], 1)
        pred.append(torch.from_numpy(np.concatenate([xy, xy + wh, g.uniform(0.3, 0.9, (n, 1)), g.randint(0, 3, (n, 1))], 1).astype(np.float32)).reshape(n, 6).to(DEV))
    det = Detections(ims, pred, [f"image{i}.jpg" for i in range(4)], names=["ant", "bee", "cat"])
    crops = det.crop(save=False)
    assert len(crops) == 12 and not (tmp_path / "crops").exists()
    k = 0
    for im, p in zip(ims, pred):
        for row in reversed(p.cpu()):
            want, box = cc.save_one_box(row[:4].numpy(), im)
            c = crops[k]
            assert sorted(c) == ["box", "cls", "conf", "im", "label"] and np.array_equal(c["im"], want) and c["im"].shape[:2] == (box[3] - box[1], box[2] - box[0])
            assert torch.equal(torch.stack(c["box"]).cpu(), row[:4]) and float(c["conf"]) == float(row[4]) and float(c["cls"]) == float(row[5])
            assert c["label"] == f"{['ant', 'bee', 'cat'][int(row[5])]} {float(row[4]):.2f}"
            k += 1
    saved = det.crop(save=True, save_dir=tmp_path / "exp")
    files = sorted((tmp_path / "exp" / "crops").rglob("*.jpg"))
    assert len(files) == len(saved) == 12 and {f.parent.name for f in files} <= {"ant", "bee", "cat"}
    sizes = sorted(Image.open(f).size for f in files)
    assert sizes == sorted((c["im"].shape[1], c["im"].shape[0]) for c in saved)
    assert (tmp_path / "exp2").exists() is False and det.crop(save=True, save_dir=tmp_path / "exp") and (tmp_path / "exp2" / "crops").exists()   # increment_path
