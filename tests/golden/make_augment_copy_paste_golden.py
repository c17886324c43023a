"""Generate tests/golden/augment_copy_paste.pt from the UNMODIFIED reference: LoadImagesAndLabels with augment=True, rect=False and hyp["copy_paste"] > 0 over the
polygon label files of make_augment_polygons_golden.py (whose helpers are imported), so that load_mosaic runs copy_paste (utils/augmentations.py:219-240): its
random.sample, its pairing of label row j with polygon j, its acceptance loop, its pixels.

    python tests/golden/make_augment_copy_paste_golden.py            # writes the fixture
    python tests/golden/make_augment_copy_paste_golden.py --search   # looks for a seed under which every situation of check_situations occurs

Only where the reference tree is present.  The file holds tensors, numbers and names only.  oracle/ref_shim.py is not touched: this script binds, on the stub cv2 and
on utils.augmentations, the three names copy_paste needs and the shim lacks -- cv2.drawContours and cv2.flip to the statement of
tests/augment_copy_paste_cases.py (fill_mask restates drawContours(FILLED); NOT compared with a cv2 build), and bbox_ioa to the restatement of the ultralytics
definition in the same file.

Cases: `exact`, `low` and `wild` of augment_polygon_cases.CASES, each with copy_paste 0.1, 0.5 and 1.0.  Per batch the file stores the reference's targets, the
accepted (slot, j, box) lists per mosaic and the generator states, and once the counters of check_situations; images and masks as CRC-32 (the nine cases' images exceed the size limit of a committed file),
after asserting per item: the image the reference returned equals item_image of the statement bit for bit; the canvas the reference handed to warpAffine equals
canvas_of with the statement's mask; the rows and polygons the reference's copy_paste appended equal the statement's; the statement's targets are the reference's;
draw_item leaves both generators where the reference leaves them.  `exact` (the warp is the plain crop, no HSV) pins the pasted pixels on the reference's own canvas
arithmetic, given the mask.  No ioa comparison lies within 1e-6 of 0.30.
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
import augment_copy_paste_cases as cpc  # noqa: E402
import augment_polygon_cases as apc  # noqa: E402
import make_augment_golden as gen  # noqa: E402  (the reference under the shim with the cv2 statements bound, seed_all, _peek, REC)
import make_augment_polygons_golden as pgen  # noqa: E402  (write_tree)
from yolov3_amd import augment  # noqa: E402

PASTES = []
SITUATIONS, new_stats, check_situations, examine = cpc.SITUATIONS, cpc.new_stats, cpc.check_situations, cpc.examine   # (in the cases module: the CPU test counts them too)


def reference():
    """the reference of make_augment_golden.py plus the three names copy_paste needs"""
    d = gen.reference()
    import cv2  # the shim's stub

    cv2.drawContours, cv2.flip, cv2.FILLED = cpc.draw_contours, cpc.flip, -1
    sys.modules["utils.augmentations"].bbox_ioa = cpc.bbox_ioa
    return d


def build_dataset(d, root: Path, case: str):
    c = cpc.cases()[case]
    ds = d.LoadImagesAndLabels(str(root / "images"), img_size=ac.IMG_SIZE, batch_size=ac.BATCH, augment=True, hyp=dict(c["hyp"]), rect=False, cache_images=False, stride=ac.STRIDE)
    assert [Path(f).stem for f in ds.im_files] == [s for s, _, _ in ac.IMAGES] and ds.mosaic and ds.albumentations.transform is None and ds.hyp["copy_paste"] == c["hyp"]["copy_paste"]
    labels, segments = apc.make_polygons()
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(ds.labels, labels)), "the labels are not the reference's parse of the label files"
    assert all(len(a) == len(b) and all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(ds.segments, segments)), "the segments differ"
    ds.ims, ds.im_hw0, ds.im_hw, ds.im_files = ac.make_images(), ac.hw0(), ac.hw(), ac.paths()
    ds.segments = [list(sg) for sg in ds.segments]
    if c["indices"] is not None:
        ds.indices = list(c["indices"])
    return ds


def run_case(d, root: Path, case: str, stats):
    c = cpc.cases()[case]
    ds = build_dataset(d, root, case)
    labels, segments = apc.make_polygons()
    images, hw, s = ac.make_images(), ac.hw(), ac.IMG_SIZE
    counts = [len(sg) for sg in segments]
    epoch = list(ds.indices)
    gen.seed_all(c["seed"])
    orig = d.copy_paste

    def copy_paste(im, lb, sg, p=0.5):
        n0, s0 = len(lb), len(sg)
        out = orig(im, lb, sg, p)
        PASTES.append(dict(rows=out[1][n0:].copy(), polys=[x.copy() for x in out[2][s0:]], dtype=out[1].dtype))
        return out

    d.copy_paste = copy_paste
    batches = []
    try:
        for k in range((len(epoch) + ac.BATCH - 1) // ac.BATCH):
            got, items = [], []
            for i in range(k * ac.BATCH, min(len(epoch), (k + 1) * ac.BATCH)):
                state = random.getstate(), np.random.get_state()
                item = augment.draw_item(epoch[i], hw, c["hyp"], s, epoch, len(hw), True, counts)
                after = random.getstate(), np.random.get_state()
                random.setstate(state[0])
                np.random.set_state(state[1])
                gen._clear()
                PASTES.clear()
                got.append(ds[i])
                now = random.getstate(), np.random.get_state()
                assert now[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(now[1], after[1])), f"{case}: item {i} leaves the generators elsewhere"
                st = cpc.paste_labels(item, labels, segments, hw, s)
                examine(item, st, labels, segments, hw, stats)
                assert len(gen.REC["warps"]) == len(item.mosaics) and len(PASTES) == len(item.mosaics)
                for (M, canvas), mo, mask, acc, rows, pasted in zip(gen.REC["warps"], item.mosaics, st["masks"], st["accepted"], st["rows"], PASTES):
                    assert M.tobytes() == mo.M[:2].tobytes() and np.array_equal(canvas, cpc.canvas_of(mo, images, mask)), f"{case}: item {i}: the pasted canvas differs"
                    assert pasted["dtype"] == np.float32 and len(pasted["rows"]) == len(acc) == len(pasted["polys"])
                    assert np.array_equal(pasted["rows"].view(np.int32), rows[len(rows) - len(acc) :].view(np.int32)), f"{case}: item {i}: the appended rows differ"
                    assert all(np.array_equal(r[1:].view(np.int32), box.view(np.int32)) for r, (_, _, box) in zip(pasted["rows"], acc))
                    assert all(p.dtype == np.float32 for p in pasted["polys"])
                    if case.startswith("exact"):
                        assert np.array_equal(ac.warp_affine_u8(canvas, M, (s, s)), canvas[s // 2 : s // 2 + s, s // 2 : s // 2 + s]), "exact: the warp is not the plain crop"
                assert np.array_equal(got[-1][1][:, 1:].numpy().view(np.int32), st["targets"].view(np.int32)), f"{case}: item {i}: the statement differs\n{got[-1][1]}\n{st['targets']}"
                assert np.array_equal(got[-1][0].numpy(), cpc.item_image(item, images, st["masks"], s)), f"{case}: item {i}: the image statement differs"
                items.append(item)
            im, targets, paths_, _ = d.LoadImagesAndLabels.collate_fn(got)
            bs = cpc.batch_statement(items, images, labels, segments, hw, s)
            assert np.array_equal(bs["targets"].view(np.int32), targets.numpy().view(np.int32)) and np.array_equal(bs["im"], im.numpy())
            batches.append(dict(targets=targets.clone(), paths=list(paths_), im_crc=cpc.crc(im.numpy()), words=torch.from_numpy(bs["words"].copy()),
                                pastes=[[int(j) for j in (it.mosaics[m].paste if m < len(it.mosaics) else ())] for it in items for m in range(2)],
                                accepted=[[(int(e), int(j), torch.from_numpy(box.copy())) for e, j, box in acc] for acc in bs["accepted"]],
                                mask_crc=[-1 if m is None else cpc.crc(np.packbits(m, axis=1, bitorder="little")) for m in bs["masks"]],
                                next_random=gen._peek()[0], next_np_random=gen._peek()[1]))
    finally:
        d.copy_paste = orig
    return dict(batches=batches, indices=epoch)


def search(limit=400):
    """a seed, used for every case, under which all situations occur and no assertion of examine refuses (put it into augment_copy_paste_cases.SEEDS, then generate)"""
    hw, s = ac.hw(), ac.IMG_SIZE
    labels, segments = apc.make_polygons()
    counts = [len(sg) for sg in segments]
    for seed in range(limit):
        stats = new_stats()
        try:
            for case, c in cpc.cases().items():
                epoch = list(c["indices"]) if c["indices"] is not None else list(range(len(hw)))
                gen.seed_all(seed)
                for i in epoch:
                    item = augment.draw_item(i, hw, c["hyp"], s, epoch, len(hw), True, counts)
                    examine(item, cpc.paste_labels(item, labels, segments, hw, s), labels, segments, hw, stats)
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
    labels, segments = apc.make_polygons()
    gold = {"meta": {"numpy": np.__version__, "torch": str(torch.__version__), "python": sys.version.split()[0]},
            "checksum": float(sum(float(l.astype(np.float64).sum()) for l in labels) + sum(float(p.astype(np.float64).sum()) + len(p) for sg in segments for p in sg)), "cases": {}}
    stats = new_stats()
    for case in cpc.cases():
        with tempfile.TemporaryDirectory() as tmp:
            pgen.write_tree(Path(tmp))
            gold["cases"][case] = run_case(d, Path(tmp), case, stats)
        print(case, [len(b["targets"]) for b in gold["cases"][case]["batches"]], [sum(len(a) for a in b["accepted"]) for b in gold["cases"][case]["batches"]])
    check_situations(stats)
    print(stats)
    gold["situations"] = {k: int(v) for k, v in stats.items()}   # how often each situation of check_situations occurred: the CPU test asserts them without the reference
    path = ROOT / "tests" / "golden" / "augment_copy_paste.pt"
    torch.save(gold, path)
    torch.load(path, weights_only=True)   # data only: tensors, numbers, strings
    print(path, path.stat().st_size, "bytes", gold["meta"])


if __name__ == "__main__":
    main()
