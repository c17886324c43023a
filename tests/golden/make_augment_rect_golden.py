"""Generate tests/golden/augment_rect.pt from the UNMODIFIED reference: utils.dataloaders.LoadImagesAndLabels with augment=True, rect=True, stride=16, pad=0.0 (train.py
--rect), driven through the helpers of make_augment_golden.py (reference(), seed_all, write_tree): its real __init__ (the aspect-ratio sort, batch_shapes), __getitem__
(letterbox to the batch shape, random_perspective, augment_hsv, the flips) and collate_fn for every batch of every case of tests/augment_rect_cases.py.

    python tests/golden/make_augment_rect_golden.py            # writes the fixture
    python tests/golden/make_augment_rect_golden.py --search   # looks for a seed under which every situation listed in check_situations occurs

Only where the reference tree is present.  The file holds tensors, tuples, numbers and names only.

The cached images are injected as make_dataset_golden.py injects them, permuted (with im_hw0 and im_hw) by the dataset's own aspect-ratio order; cv2.resize of the stub is
replaced by a recorder that raises, and the generator asserts it was never called (every image fits its batch shape with r = 1).  Asserted before anything is stored:
the reference's order, batch index and batch_shapes are those of yolov3_amd.dataset.rect_batch_shapes and the values written down in tests/augment_rect_cases.py; per
item the matrix, the letterboxed image handed to warpAffine, the tables, the flips and the shapes tuple are those of yolov3_amd.augment.draw_item replayed from the same
generator state, both leave `random` and `np.random` in the same state, the labels are those of augment_rect_cases.item_labels bit for bit and the image is that of
augment_rect_cases.item_image; no box_candidates comparison lies within 1e-9 relative of its threshold.

What the images rest on: case `rect_exact` on the reference alone (M is the identity, the reference calls neither warpAffine nor cvtColor, and the generator asserts
the image equal to the plain letterbox paste, flipped); the other cases on the reference plus the sampler and colour statements of tests/augment_cases.py.  What
the labels rest on: the reference (and the restated xywhn2xyxy / xyxy2xywhn, as before)."""
import random
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import augment_cases as ac  # noqa: E402
import augment_rect_cases as arc  # noqa: E402
import make_augment_golden as gen  # noqa: E402  (the reference under the shim with the cv2 statements bound, seed_all, write_tree, _peek, plain, REC)
from yolov3_amd import augment  # noqa: E402
from yolov3_amd.dataset import rect_batch_shapes  # noqa: E402

SITUATIONS = ("wide_batch", "tall_batch", "ud_on", "ud_off", "lr_on", "lr_off", "cut_left", "cut_right", "cut_top", "cut_bottom", "dropped", "no_labels")
RESIZES = []


def new_stats():
    return dict.fromkeys(SITUATIONS, 0)


def check_situations(stats):
    """every situation the (H, W) form of the kernels can get wrong occurs under the seeds of the cases: a wide batch and a tall batch; each flip both on and off in a
    non-square batch; a kept label cut by each of the four edges of a non-square batch; a label dropped by box_candidates; an item without labels"""
    missing = [k for k, v in stats.items() if not v]
    assert not missing, f"situations that do not occur: {missing} ({stats})"


def tally(item, H, W, stats):
    stats["wide_batch"] += int(W > H)
    stats["tall_batch"] += int(H > W)
    if H != W:
        stats["ud_on" if item.flipud else "ud_off"] += 1
        stats["lr_on" if item.fliplr else "lr_off"] += 1


def no_resize(*a, **k):
    RESIZES.append(a)
    raise AssertionError("cv2.resize was called: an image does not fit its batch shape with r = 1")


def build_dataset(d, root: Path, case: str):
    import cv2  # the shim's stub

    cv2.resize = no_resize
    c = arc.CASES[case]
    ds = d.LoadImagesAndLabels(str(root / "images"), img_size=arc.IMG_SIZE, batch_size=arc.BATCH, augment=True, hyp=dict(c["hyp"]), rect=True, cache_images=False, stride=arc.STRIDE,
                               pad=0.0)
    assert ds.rect and not ds.mosaic and ds.albumentations.transform is None and list(ds.indices) == list(range(len(ac.IMAGES)))
    stems = [Path(f).stem for f in ds.im_files]
    fi = [[s for s, _, _ in ac.IMAGES].index(s) for s in stems]   # dataset position -> file-order position: the dataset's own aspect-ratio order
    # the project's layout, run here, and the values written down in the cases file
    order, batch, shapes = rect_batch_shapes([(w0, h0) for h0, w0 in ac.hw0()], arc.IMG_SIZE, arc.BATCH, arc.STRIDE, 0.0)
    assert fi == [int(i) for i in order] == arc.file_index() and stems == arc.ORDER, (stems, order)
    assert np.array_equal(ds.batch, batch) and np.array_equal(ds.batch_shapes, shapes) and [tuple(int(v) for v in s) for s in ds.batch_shapes] == arc.BATCH_SHAPES
    images, labels, hw, hw0, paths = arc.sorted_set()
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(ds.labels, labels)) and not any(len(sg) for sg in ds.segments)
    assert all(tuple(ds.shapes[j]) == hw0[j][::-1] for j in range(len(fi)))
    ds.ims, ds.im_hw0, ds.im_hw, ds.im_files = images, hw0, hw, paths
    # r = 1 for every image, letterbox halves ending in .5 on both axes, the label-less image in batch 0
    halves = [((W - w) / 2, (H - h) / 2) for (h, w), (H, W) in zip(hw, (arc.BATCH_SHAPES[b] for b in batch))]
    assert all(min(H / h, W / w) == 1.0 for (h, w), (H, W) in zip(hw, (arc.BATCH_SHAPES[b] for b in batch)))
    assert {5.5, 1.5} <= {dh for _, dh in halves} and {3.5, 7.5, 12.5} <= {dw for dw, _ in halves} and [len(lb) for lb in labels[:4]].count(0) == 1
    return ds


def run_case(d, root: Path, case: str, stats):
    c = arc.CASES[case]
    ds = build_dataset(d, root, case)
    images, labels, hw, n = ds.ims, ds.labels, ds.im_hw, len(ds.ims)
    gen.seed_all(c["seed"])
    orig = dict(flipud=np.flipud, fliplr=np.fliplr)
    np.flipud = lambda m: (gen.REC["flips"].append("ud"), orig["flipud"](m))[1]
    np.fliplr = lambda m: (gen.REC["flips"].append("lr"), orig["fliplr"](m))[1]
    batches = []
    try:
        for k in range((n + arc.BATCH - 1) // arc.BATCH):
            H, W = arc.BATCH_SHAPES[k]
            got, items = [], []
            for i in range(k * arc.BATCH, min(n, (k + 1) * arc.BATCH)):
                state = random.getstate(), np.random.get_state()
                item = augment.draw_item(i, hw, c["hyp"], (H, W), None, n, False)
                after = random.getstate(), np.random.get_state()
                random.setstate(state[0])
                np.random.set_state(state[1])
                gen._clear()
                got.append(ds[i])
                now = random.getstate(), np.random.get_state()
                assert now[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(now[1], after[1])), f"{case}: item {i} leaves the generators elsewhere"
                mo = item.mosaics[0]
                assert not item.mosaic and len(item.mosaics) == 1 and item.ratio is None and mo.indices == [i] and not gen.REC["beta"]
                identity = bool((mo.M == np.eye(3)).all())
                assert len(gen.REC["warps"]) == (0 if identity else 1) and identity == (case == "rect_exact")
                for M, canvas in gen.REC["warps"]:   # what the reference handed to warpAffine against what draw_item formed
                    assert M.tobytes() == mo.M[:2].tobytes(), f"{case}: item {i}: M differs\n{M}\n{mo.M}"
                    assert np.array_equal(canvas, arc.paste(mo, images, H, W)), f"{case}: item {i}: the letterboxed image is not the one pasted from draw_item's rectangle"
                assert (item.luts is None and not gen.REC["luts"]) or all(np.array_equal(a, b) for a, b in zip(gen.REC["luts"], item.luts))
                assert gen.REC["flips"] == ["ud"] * item.flipud + ["lr"] * item.fliplr
                (h, w), (h0, w0) = hw[i], ds.im_hw0[i]
                assert got[-1][3] == ((h0, w0), ((h / h0, w / w0), mo.pad[0])) and mo.pad[0] == ((W - w) / 2, (H - h) / 2)
                want = arc.item_labels(item, labels, hw, H, W, stats, check=True)
                assert np.array_equal(got[-1][1][:, 1:].numpy().view(np.int32), want.view(np.int32)), f"{case}: item {i}: the label model differs\n{got[-1][1]}\n{want}"
                assert tuple(got[-1][0].shape) == (3, H, W) and np.array_equal(got[-1][0].numpy(), arc.item_image(item, images, H, W)), f"{case}: item {i}: the image statement differs"
                if case == "rect_exact":   # no cv2 statement involved: the plain letterbox paste, flipped
                    plain_im = arc.paste(mo, images, H, W)
                    plain_im = plain_im[::-1] if item.flipud else plain_im
                    plain_im = plain_im[:, ::-1] if item.fliplr else plain_im
                    assert item.luts is None and np.array_equal(got[-1][0].numpy(), plain_im.transpose(2, 0, 1)[::-1]), "rect_exact: the image is not the plain letterbox paste"
                tally(item, H, W, stats)
                items.append(item)
            im, targets, paths, shapes = d.LoadImagesAndLabels.collate_fn(got)
            assert im.dtype == torch.uint8 and targets.dtype == torch.float32 and tuple(im.shape) == (len(got), 3, H, W)
            assert np.array_equal(targets.numpy().view(np.int32), arc.batch_targets(items, labels, hw, H, W).view(np.int32))
            b = dict(targets=targets.clone(), paths=list(paths), shapes=gen.plain(shapes), next_random=gen._peek()[0], next_np_random=gen._peek()[1], items=[
                dict(index=it.index, flipud=it.flipud, fliplr=it.fliplr, luts=None if it.luts is None else torch.from_numpy(it.luts.copy()), M=torch.from_numpy(it.mosaics[0].M.copy()),
                     scale=float(it.mosaics[0].scale), rect=gen.plain(it.mosaics[0].rects[0]), pad=gen.plain(it.mosaics[0].pad[0])) for it in items])
            if case not in arc.IMAGES_OF:
                b["im"] = im.clone()
            else:
                assert torch.equal(im, arc.expected_images({"cases": STORED}, case, k))
            batches.append(b)
    finally:
        np.flipud, np.fliplr = orig["flipud"], orig["fliplr"]
    assert not RESIZES, "cv2.resize was called"
    return dict(batches=batches, order=arc.file_index(), batch=[int(v) for v in ds.batch], batch_shapes=[tuple(int(v) for v in s) for s in ds.batch_shapes])


STORED: dict = {}


def search(limit=400):
    """a seed, used for every case, under which all situations occur and no assertion of item_labels refuses (put it into augment_rect_cases.SEED, then generate)"""
    _, labels, hw, _, _ = arc.sorted_set()
    for seed in range(limit):
        stats = new_stats()
        try:
            for case, c in arc.CASES.items():
                gen.seed_all(seed)
                for i in range(len(hw)):
                    H, W = arc.BATCH_SHAPES[i // arc.BATCH]
                    item = augment.draw_item(i, hw, c["hyp"], (H, W), None, len(hw), False)
                    tally(item, H, W, stats)
                    arc.item_labels(item, labels, hw, H, W, stats, check=True)
        except AssertionError as e:
            print(seed, "refused:", e)
            continue
        missing = [k for k, v in stats.items() if not v]
        print(seed, "missing", missing)
        if not missing:
            return seed
    return None


def main():
    if "--search" in sys.argv:
        print("seed:", search())
        return
    d = gen.reference()
    images, labels = ac.make_images(), ac.make_labels()
    gold = {"meta": {"numpy": np.__version__, "torch": str(torch.__version__), "python": sys.version.split()[0]}, "checksum": ac.checksum(images, labels), "cases": STORED}
    stats = new_stats()
    for case in arc.CASES:
        with tempfile.TemporaryDirectory() as tmp:
            gen.write_tree(Path(tmp))
            STORED[case] = run_case(d, Path(tmp), case, stats)
        print(case, [tuple(b["im"].shape) if "im" in b else None for b in STORED[case]["batches"]], [len(b["targets"]) for b in STORED[case]["batches"]])
    check_situations(stats)
    print(stats)
    path = ROOT / "tests" / "golden" / "augment_rect.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only: tensors, numbers, strings
    print(path, path.stat().st_size, "bytes", gold["meta"])


if __name__ == "__main__":
    main()
