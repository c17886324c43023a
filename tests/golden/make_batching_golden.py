"""Generate tests/golden/batching.pt from the UNMODIFIED reference: the --multi-scale size draws of train.py:395-398 and the outputs of
utils/dataloaders.py::collate_fn4 (--quad).

    python tests/golden/make_batching_golden.py

Only where the reference tree is present.  Neither file can be imported here (utils/dataloaders.py imports cv2, train.py the whole training stack), and this script
holds none of their statements: it reads the four lines of train.py and the body of collate_fn4 from the reference tree when it runs (linecache / ast), checks
that they are still the lines it means, and executes that text with torch, F, random and math in its namespace.  The file written holds data only:

  draws     per (seed 0..3, (imgsz, batch shape)) eight consecutive draws: the new size [h, w] or None where the reference does not resize, and the value of the
            next random.random() afterwards (the state the generator is left in)
  quad      a seeded batch of 8 uint8 images (3, 6, 10) with 0 to 5 labels each (one image has none), and per seed collate_fn4's images and labels; the two seeds
            are the first that take different branches in each group, so that both groups see both branches
  quad_big  collate_fn4's images for the 12 images (3, 32, 40) of `big_batch()` below (three groups, mixed branches); the input is rebuilt from its formula
"""
import ast
import linecache
import math
import random
import sys
import textwrap
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import ref_shim  # noqa: E402

SEEDS = (0, 1, 2, 3)
DRAW_CASES = ((640, (640, 640)), (640, (384, 640)), (416, (416, 416)), (128, (128, 128)))   # (imgsz, spatial shape of the batch); the last is the GPU end-to-end test's
DRAWS = 8
GS = 32


def big_batch():
    """12 uint8 images (3, 32, 40) from integer arithmetic alone (no random stream whose implementation could change)"""
    n = 12 * 3 * 32 * 40
    return (((torch.arange(n, dtype=torch.int64) * 1103515245 + 12345) >> 8) % 256).to(torch.uint8).reshape(12, 3, 32, 40)


def small_batch():
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (8, 3, 6, 10), generator=g, dtype=torch.uint8)
    counts = [3, 0, 5, 1, 2, 4, 1, 3]
    labels = []
    for n in counts:
        lb = torch.zeros(n, 6)
        lb[:, 1] = torch.randint(0, 80, (n,), generator=g).float()
        lb[:, 2:] = torch.rand(n, 4, generator=g)
        labels.append(lb)
    return imgs, labels


def multi_scale_lines():
    path = str(ref_shim.REFERENCE_ROOT / "train.py")
    text = textwrap.dedent("".join(linecache.getline(path, n) for n in range(395, 399)))
    assert "random.randrange" in text and text.count("\n") == 4, "train.py:395-398 are no longer the multi-scale size draw"
    return compile(text, path, "exec")


def collate_fn4():
    path = ref_shim.REFERENCE_ROOT / "utils" / "dataloaders.py"
    source = path.read_text()
    node = next(n for n in ast.walk(ast.parse(source)) if isinstance(n, ast.FunctionDef) and n.name == "collate_fn4")
    text = textwrap.dedent("\n".join(source.splitlines()[node.lineno - 1:node.end_lineno]))   # from the `def` line: the decorator stays behind
    assert text.startswith("def collate_fn4") and "random.random()" in text
    ns = {"torch": torch, "F": F, "random": random, "math": math}
    exec(compile(text, str(path), "exec"), ns)
    return ns["collate_fn4"]


def run_collate(fn, imgs, labels):
    batch = [(imgs[i], labels[i].clone(), f"im{i}", None) for i in range(len(imgs))]
    im4, lb4, paths, shapes = fn(batch)
    return im4, lb4


def main():
    assert ref_shim.available(), "the reference tree is not readable here"
    code = multi_scale_lines()
    draws = {}
    for seed in SEEDS:
        for imgsz, shape in DRAW_CASES:
            random.seed(seed)
            sizes = []
            for _ in range(DRAWS):
                class imgs:   # the lines read imgs.shape[2:]
                    pass
                imgs.shape = (16, 3, *shape)
                ns = {"random": random, "math": math, "imgsz": imgsz, "gs": GS, "imgs": imgs}
                exec(code, ns)
                sizes.append([int(v) for v in ns["ns"]] if "ns" in ns else None)
                assert ("ns" in ns) == (ns["sf"] != 1)
            draws[(seed, imgsz, shape)] = {"sizes": sizes, "next_random": random.random()}
    assert draws[(0, 640, (640, 640))]["sizes"][:3] == [[704, 704], [736, 736], [352, 352]]
    assert draws[(0, 640, (384, 640))]["sizes"][:3] == [[448, 704], [448, 736], [224, 352]]
    assert draws[(0, 416, (416, 416))]["sizes"][:4] == [[640, 640], [384, 384], [576, 576], None]

    fn = collate_fn4()
    imgs, labels = small_batch()
    assert sorted(len(lb) for lb in labels)[0] == 0
    quad, seen = {}, []
    for seed in range(64):
        random.seed(seed)
        flags = [random.random() < 0.5 for _ in range(2)]
        if flags[0] != flags[1] and flags not in seen:
            seen.append(flags)
            random.seed(seed)
            im4, lb4 = run_collate(fn, imgs, labels)
            quad[seed] = {"flags": flags, "imgs": im4, "labels": lb4, "next_random": random.random()}
        if len(seen) == 2:
            break
    assert len(quad) == 2
    big = big_batch()
    for seed in range(64):
        random.seed(seed)
        flags = [random.random() < 0.5 for _ in range(3)]
        if len(set(flags)) == 2:
            random.seed(seed)
            im4, _ = run_collate(fn, big, [torch.zeros(0, 6)] * 12)
            quad_big = {"seed": seed, "flags": flags, "imgs": im4, "input_sum": int(big.long().sum())}
            break
    out = {"gs": GS, "draws": draws, "quad_in": {"imgs": imgs, "labels": labels}, "quad": quad, "quad_big": quad_big}
    path = ROOT / "tests" / "golden" / "batching.pt"
    torch.save(out, path)
    torch.load(path, weights_only=True)   # data only
    print(path, path.stat().st_size, "bytes; quad seeds", {s: q["flags"] for s, q in quad.items()}, "big", quad_big["seed"], quad_big["flags"])


if __name__ == "__main__":
    main()
