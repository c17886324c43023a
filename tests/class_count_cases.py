"""Seeded inputs shared by tests/golden/make_class_counts_golden.py (the unmodified reference), tests/test_oracle_vs_reference_live.py (the oracle) and
tests/test_gpu_class_counts.py (the HIP kernels): target sets for heads of any class count."""
import torch

from oracle import yolo_oracle as yo

HYP = dict(box=0.05, cls=0.5, cls_pw=1.0, obj=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)


def scaled_hyp(nl, nc, hw, over=()):
    """the hyper-parameters as the reference's train.py:327-329 scales them to the head (levels, classes, image size)"""
    hyp = dict(HYP, **dict(over))
    hyp["box"] *= 3 / nl
    hyp["cls"] *= nc / 80 * 3 / nl
    hyp["obj"] *= (hw / 640) ** 2 * 3 / nl
    return hyp


def matched_cells(shapes, tg, anchors_grid):
    """matched rows per level (oracle.build_targets: the anchor-ratio test and the neighbour offsets)"""
    return [int(t[0].shape[0]) for t in yo.build_targets(shapes, tg, anchors_grid.float().cpu(), HYP["anchor_t"])]


def pick_targets(bs, nc, shapes, anchors_grid, seed0):
    """(seed, targets): yo.synth_targets(bs, nc, seed) of the first seed >= seed0 whose targets match at least one cell on EVERY level and, for nc <= 4, name every
    class 0 .. nc-1; for larger nc the last class nc-1 is given to the first target (the labels are otherwise the generator's)."""
    for seed in range(seed0, seed0 + 200):
        tg = yo.synth_targets(bs, nc, seed=seed)
        if not tg.shape[0]:
            continue
        if nc > 4:
            tg[0, 1] = nc - 1
        if all(matched_cells(shapes, tg, anchors_grid)) and (nc > 4 or set(tg[:, 1].long().tolist()) == set(range(nc))):
            return seed, tg
    raise AssertionError(f"no seed in [{seed0}, {seed0 + 200}) gives targets on every level for nc {nc}")
