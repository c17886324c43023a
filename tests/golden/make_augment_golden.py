"""Generate tests/golden/augment.pt from the UNMODIFIED reference: utils.dataloaders.LoadImagesAndLabels with augment=True, rect=False (through oracle/ref_shim.py) --
its real __init__, __getitem__ (load_mosaic, random_perspective, mixup, augment_hsv, the flips) and collate_fn for every batch of every case of tests/augment_cases.py.

    python tests/golden/make_augment_golden.py            # writes the fixture
    python tests/golden/make_augment_golden.py --search   # looks for seeds under which every situation listed in check_situations occurs

Only where the reference tree is present.  The file holds tensors, tuples, numbers and names only.

The reference is driven as make_dataset_golden.py drives it; in addition the stub cv2 gets warpAffine, cvtColor, split / merge / LUT and getRotationMatrix2D, bound
to the statements of tests/augment_cases.py (or trivial indexing).  warpAffine and LUT also RECORD what the reference handed them (M, the canvas, the tables);
np.random.beta, np.flipud / np.fliplr and load_image are wrapped to record the ratio, the flips and the chosen images.  The paste rectangles are not visible from
outside load_mosaic: the fixture stores those of yolov3_amd.augment.draw_item, replayed from the same generator state, after asserting that the canvas pasted
from them IS the canvas the reference handed to warpAffine, and that both leave `random` and `np.random` in the same state.

What the images rest on: case `exact` on the reference alone (the generator asserts that the sampler returns the plain crop of the canvas and no HSV runs); the
other cases on the reference plus the two statements.  What the labels rest on: the reference (and the restated xywhn2xyxy / xyxy2xywhn, as before).
"""
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
import make_dataset_golden as base  # noqa: E402  (the restated xywhn2xyxy / xyxy2xywhn, img2label_paths, the progress stub, copyMakeBorder)
from oracle import ref_shim  # noqa: E402
from yolov3_amd import augment  # noqa: E402

COLOR_BGR2HSV, COLOR_HSV2BGR = 40, 54
REC = dict(warps=[], luts=[], beta=[], flips=[], loads=[])


def _clear():
    for v in REC.values():
        v.clear()


def warp_affine(im, M, dsize, borderValue=(0, 0, 0)):
    assert len(set(borderValue)) == 1 and M.shape == (2, 3) and M.dtype == np.float64
    REC["warps"].append((M.copy(), im.copy()))
    return ac.warp_affine_u8(im, M, dsize, border=borderValue[0])


def cvt_color(im, code, dst=None):
    out = ac.bgr2hsv_u8(im) if code == COLOR_BGR2HSV else ac.hsv2bgr_u8(im)
    assert code in (COLOR_BGR2HSV, COLOR_HSV2BGR)
    if dst is not None:
        dst[...] = out
        return dst
    return out


def lut(src, table):
    REC["luts"].append(table.copy())
    return table[src]


def reference():
    ref_shim.install()
    import cv2  # the shim's stub
    import utils.dataloaders as d  # type: ignore

    cv2.copyMakeBorder, cv2.warpAffine, cv2.cvtColor, cv2.LUT = base.copy_make_border, warp_affine, cvt_color, lut
    cv2.split, cv2.merge = (lambda im: tuple(im[..., c] for c in range(im.shape[2]))), (lambda planes: np.stack(planes, -1))
    cv2.getRotationMatrix2D = lambda angle, center, scale: ac.get_rotation_matrix_2d(angle, center, scale)
    cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = COLOR_BGR2HSV, COLOR_HSV2BGR
    d.xywhn2xyxy, d.xyxy2xywhn, d.img2label_paths, d.get_hash, d.TQDM = base.xywhn2xyxy, base.xyxy2xywhn, base.img2label_paths, (lambda paths: "augment-golden"), base._Progress
    return d


def write_tree(root: Path):
    from PIL import Image

    (root / "images").mkdir()
    (root / "labels").mkdir()
    for (stem, _, (h0, w0)), lb in zip(ac.IMAGES, ac.make_labels()):
        Image.new("RGB", (w0, h0), (90, 120, 150)).save(root / "images" / f"{stem}.png")
        (root / "labels" / f"{stem}.txt").write_text("".join(" ".join([str(int(r[0]))] + [repr(float(v)) for v in r[1:]]) + "\n" for r in lb))


def build_dataset(d, root: Path, case: str):
    c = ac.CASES[case]
    ds = d.LoadImagesAndLabels(str(root / "images"), img_size=ac.IMG_SIZE, batch_size=ac.BATCH, augment=True, hyp=dict(c["hyp"]), rect=False, cache_images=False, stride=ac.STRIDE)
    assert [Path(f).stem for f in ds.im_files] == [s for s, _, _ in ac.IMAGES] and ds.mosaic and ds.albumentations.transform is None
    images, labels = ac.make_images(), ac.make_labels()
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(ds.labels, labels)) and not any(len(sg) for sg in ds.segments)
    ds.ims, ds.im_hw0, ds.im_hw, ds.im_files = images, ac.hw0(), ac.hw(), ac.paths()
    if c["indices"] is not None:
        ds.indices = list(c["indices"])
    return ds


def plain(v):
    if v is None:
        return None
    return tuple(plain(x) for x in v) if isinstance(v, (tuple, list, np.ndarray)) else (float(v) if isinstance(v, (float, np.floating)) else int(v))


def paste(mo, images):
    """the canvas of a drawn Mosaic, or the letterboxed image"""
    canvas = np.full((mo.canvas, mo.canvas, 3), 114, dtype=np.uint8)
    for j, (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b) in zip(mo.indices, mo.rects):
        canvas[y1a:y2a, x1a:x2a] = images[j][y1b:y2b, x1b:x2b]
    return canvas


def model_labels(item, labels, hw, s, stats):
    """The label path as csrc/augment.hip computes it (fp32 / fp64 as the reference's arrays are, the corner transform as a plain left-to-right sum) -> (nl, 5) fp32;
    `stats` collects what check_situations asks about."""
    out = []
    for mo in item.mosaics:
        rows = []
        for j, (padw, padh) in zip(mo.indices, mo.pad):
            lb = labels[j].copy()
            if lb.size:
                lb[:, 1:] = base.xywhn2xyxy(lb[:, 1:], hw[j][1], hw[j][0], padw, padh)
            rows.append(lb)
        t = np.concatenate(rows, 0)
        if item.mosaic:
            np.clip(t[:, 1:], 0, 2 * s, out=t[:, 1:])
        n = len(t)
        if n:
            M = mo.M
            p = t[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2).astype(np.float64)
            x = (p[:, 0] * M[0, 0] + p[:, 1] * M[0, 1] + M[0, 2]).reshape(n, 4)
            y = (p[:, 0] * M[1, 0] + p[:, 1] * M[1, 1] + M[1, 2]).reshape(n, 4)
            blas = (np.concatenate([p, np.ones((n * 4, 1))], 1) @ M.T)[:, :2].reshape(n, 8)
            raw = np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], 1)
            raw_blas = np.stack([blas[:, 0::2].min(1), blas[:, 1::2].min(1), blas[:, 0::2].max(1), blas[:, 1::2].max(1)], 1)
            new = np.stack([raw[:, 0].clip(0, s), raw[:, 1].clip(0, s), raw[:, 2].clip(0, s), raw[:, 3].clip(0, s)], 1)
            assert np.array_equal(new.astype(np.float32), raw_blas.clip(0, s).astype(np.float32)), "the plain fp64 sum and xy @ M.T round to different fp32 boxes"
            box1 = t[:, 1:5].T * mo.scale
            assert box1.dtype == np.float32
            w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
            w2, h2 = new[:, 2] - new[:, 0], new[:, 3] - new[:, 1]
            eps = 1e-16
            ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
            area = w2 * h2 / (w1 * h1 + eps)
            keep = (w2 > 2) & (h2 > 2) & (area > 0.1) & (ar < 100)
            for v, thr in ((w2, 2.0), (h2, 2.0), (area, 0.1), (ar, 100.0)):
                assert (np.abs(v - thr) > 1e-9 * thr).all(), "a box_candidates comparison lies at its threshold"
            stats["clipped"] += int(((raw != new).any(1) & keep).sum())
            t = t[keep]
            t[:, 1:5] = new[keep]
        out.append(t)
    t = np.concatenate(out, 0)
    stats["dropped_all"] += int(sum(len(labels[j]) for mo in item.mosaics for j in mo.indices) > 0 and len(t) == 0)
    if len(t):
        t[:, 1:5] = base.xyxy2xywhn(t[:, 1:5], w=s, h=s, clip=True, eps=1e-3)
        if item.flipud:
            t[:, 2] = 1 - t[:, 2]
        if item.fliplr:
            t[:, 1] = 1 - t[:, 1]
    return t


def new_stats():
    return dict(mixup=0, ud=0, lr=0, both=0, dropped_all=0, clipped=0, gap=0, lo=0, hi=0, mixed_tap=0, left=0, right=0, top=0, bottom=0, negative=0, small=0, large=0)


def tally(item, s, stats):
    """the situations of check_situations that the draws decide"""
    stats["mixup"] += item.ratio is not None
    stats["ud"] += item.flipud and not item.fliplr
    stats["lr"] += item.fliplr and not item.flipud
    stats["both"] += item.flipud and item.fliplr
    for mo in item.mosaics:
        stats["small"] += mo.scale < 0.6
        stats["large"] += mo.scale > 1.4
        X, Y = ac.warp_coordinates(mo.M[:2], s, s)
        sx, sy = X >> 5, Y >> 5
        stats["negative"] += int((X < 0).any() or (Y < 0).any())
        stats["left"] += int((sx < 0).any())
        stats["top"] += int((sy < 0).any())
        stats["right"] += int((sx + 1 >= mo.canvas).any())
        stats["bottom"] += int((sy + 1 >= mo.canvas).any())
        if item.mosaic:
            yc, xc = mo.center
            stats["lo"] += int(min(yc, xc) <= s // 2 + 2)
            stats["hi"] += int(max(yc, xc) >= 3 * s // 2 - 3)
            x1a, y1a = mo.rects[0][:2]
            stats["gap"] += int(x1a > 0 or y1a > 0)
            owner = np.full((mo.canvas + 2, mo.canvas + 2), -1)
            for t, (x1a, y1a, x2a, y2a, *_) in enumerate(mo.rects):
                owner[y1a + 1 : y2a + 1, x1a + 1 : x2a + 1] = t
            cx, cy = np.clip(sx + 1, 0, mo.canvas + 1), np.clip(sy + 1, 0, mo.canvas + 1)
            a, b = owner[cy, cx], owner[np.clip(cy + 1, 0, mo.canvas + 1), np.clip(cx + 1, 0, mo.canvas + 1)]
            stats["mixed_tap"] += int(((a >= 0) & (b >= 0) & (a != b) & ((X & 31) > 0) & ((Y & 31) > 0)).any())


def check_situations(stats):
    """every situation the kernels can get wrong occurs under the seeds of the cases: an item with mixup; flipud alone, fliplr alone, both; an item whose labels are
    all dropped by box_candidates; a kept label clipped by the image edge; a tile smaller than its quadrant (a 114 gap inside the canvas); a mosaic centre within 2
    pixels of each end of its range; a tap that mixes two tiles; a tap outside the canvas on each of the four sides; a negative source coordinate; a scale below 0.6
    and one above 1.4"""
    missing = [k for k, v in stats.items() if not v]
    assert not missing, f"situations that do not occur: {missing} ({stats})"


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def run_case(d, root: Path, case: str, stats):
    c = ac.CASES[case]
    ds = build_dataset(d, root, case)
    images, labels, hw, s = ds.ims, ds.labels, ac.hw(), ac.IMG_SIZE
    epoch = list(ds.indices)
    seed_all(c["seed"])
    orig = dict(beta=np.random.beta, flipud=np.flipud, fliplr=np.fliplr, load=d.LoadImagesAndLabels.load_image)

    def beta(a, b):
        r = orig["beta"](a, b)
        REC["beta"].append(r)
        return r

    def load_image(self, i):
        REC["loads"].append(int(i))
        return orig["load"](self, i)

    np.random.beta = beta
    np.flipud = lambda m: (REC["flips"].append("ud"), orig["flipud"](m))[1]
    np.fliplr = lambda m: (REC["flips"].append("lr"), orig["fliplr"](m))[1]
    d.LoadImagesAndLabels.load_image = load_image
    batches = []
    try:
        for k in range((len(epoch) + ac.BATCH - 1) // ac.BATCH):
            got, items = [], []
            for i in range(k * ac.BATCH, min(len(epoch), (k + 1) * ac.BATCH)):
                state = random.getstate(), np.random.get_state()
                item = augment.draw_item(epoch[i], hw, c["hyp"], s, epoch, len(hw), True)
                after = random.getstate(), np.random.get_state()
                random.setstate(state[0])
                np.random.set_state(state[1])
                _clear()
                got.append(ds[i])
                now = random.getstate(), np.random.get_state()
                assert now[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(now[1], after[1])), f"{case}: item {i} leaves the generators elsewhere"
                # what the reference handed out against what draw_item formed
                assert len(REC["warps"]) == len(item.mosaics) and REC["loads"] == [j for mo in item.mosaics for j in mo.indices]
                for (M, canvas), mo in zip(REC["warps"], item.mosaics):
                    assert np.array_equal(M, mo.M[:2]) and M.tobytes() == mo.M[:2].tobytes(), f"{case}: item {i}: M differs\n{M}\n{mo.M}"
                    assert np.array_equal(canvas, paste(mo, images)), f"{case}: item {i}: the canvas is not the one pasted from draw_item's rectangles"
                    if case == "exact":
                        assert np.array_equal(ac.warp_affine_u8(canvas, M, (s, s)), canvas[s // 2 : s // 2 + s, s // 2 : s // 2 + s]), "exact: the warp is not the plain crop"
                assert (item.ratio is None and not REC["beta"]) or [item.ratio] == REC["beta"]
                assert (item.luts is None and not REC["luts"]) or all(np.array_equal(a, b) for a, b in zip(REC["luts"], item.luts))
                assert REC["flips"] == ["ud"] * item.flipud + ["lr"] * item.fliplr and item.mosaic == (got[-1][3] is None)
                want = model_labels(item, labels, hw, s, stats)
                assert np.array_equal(got[-1][1][:, 1:].numpy().view(np.int32), want.view(np.int32)), f"{case}: item {i}: the label model differs\n{got[-1][1]}\n{want}"
                tally(item, s, stats)
                items.append(item)
            im, targets, paths, shapes = d.LoadImagesAndLabels.collate_fn(got)
            assert im.dtype == torch.uint8 and targets.dtype == torch.float32 and tuple(im.shape) == (len(got), 3, s, s)
            b = dict(targets=targets.clone(), paths=list(paths), shapes=plain(shapes), next_random=_peek()[0], next_np_random=_peek()[1], items=[
                dict(index=it.index, mosaic=it.mosaic, flipud=it.flipud, fliplr=it.fliplr, ratio=it.ratio, luts=None if it.luts is None else torch.from_numpy(it.luts.copy()),
                     mosaics=[dict(indices=list(mo.indices), rects=plain(mo.rects), M=torch.from_numpy(mo.M.copy()), scale=float(mo.scale), center=plain(mo.center)) for mo in it.mosaics])
                for it in items])
            if case not in ac.IMAGES_OF:
                b["im"] = im.clone()
            else:
                assert torch.equal(im, ac.expected_images({"cases": STORED}, case, k))
            batches.append(b)
    finally:
        np.random.beta, np.flipud, np.fliplr, d.LoadImagesAndLabels.load_image = orig["beta"], orig["flipud"], orig["fliplr"], orig["load"]
    return dict(batches=batches, indices=epoch)


STORED: dict = {}


def _peek():
    """the next random.random() and np.random.random(), the generators left where they were"""
    state = random.getstate(), np.random.get_state()
    out = random.random(), float(np.random.random())
    random.setstate(state[0])
    np.random.set_state(state[1])
    return out


def search(limit=400):
    """seeds of `exact` and `wild` under which the draw-decided situations occur (run it, put the seeds into augment_cases.CASES, then generate)"""
    hw, s, labels = ac.hw(), ac.IMG_SIZE, ac.make_labels()
    for seed in range(limit):
        stats = new_stats()
        try:
            for case, c in ac.CASES.items():
                epoch = list(c["indices"]) if c["indices"] is not None else list(range(len(hw)))
                seed_all(seed)
                for i in epoch:
                    item = augment.draw_item(i, hw, c["hyp"], s, epoch, len(hw), True)
                    tally(item, s, stats)
                    model_labels(item, labels, hw, s, stats)
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
    d = reference()
    images, labels = ac.make_images(), ac.make_labels()
    gold = {"meta": {"numpy": np.__version__, "torch": str(torch.__version__), "python": sys.version.split()[0]}, "checksum": ac.checksum(images, labels), "cases": STORED}
    stats = new_stats()
    for case in ac.CASES:
        with tempfile.TemporaryDirectory() as tmp:
            write_tree(Path(tmp))
            STORED[case] = run_case(d, Path(tmp), case, stats)
        print(case, [len(b["targets"]) for b in STORED[case]["batches"]])
    check_situations(stats)
    print(stats)
    path = ROOT / "tests" / "golden" / "augment.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only: tensors, numbers, strings
    print(path, path.stat().st_size, "bytes", gold["meta"])


if __name__ == "__main__":
    main()
