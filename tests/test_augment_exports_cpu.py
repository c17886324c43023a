"""One table over the eleven augment exports of csrc/augment.hip (include/yolov3_hip.h): every export refuses every bad argument it can be given without a GPU, under
its own name, in the category the fault belongs to and with exactly the text recorded below.  The argument names are read from the header; a call changes exactly one
argument of a valid set, so no call here launches.  The texts are what the library answered before the exports were given one argument check and one launch path; a
reworded or reordered refusal fails here."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
P = 1 << 20   # a fake, aligned device address: validation never dereferences it

EXPORTS = ["y3_augment_batch", "y3_augment_batch_hw", "y3_augment_targets", "y3_augment_targets_hw", "y3_augment_polygons", "y3_augment_targets_polygons",
           "y3_augment_copy_paste_select", "y3_augment_copy_paste_raster", "y3_augment_batch_paste", "y3_augment_polygons_paste", "y3_augment_targets_paste"]

# a valid value per argument name (every other name is a device pointer: P); the sets of the four tests/test_augment*_cpu.py
VALID = {"arena_bytes": 4096, "n_images": 12, "count": 4, "dst_dtype": 3, "S": 64, "H": 48, "W": 64, "n_vertices": 100, "n_label_rows": 26, "n_rows": 30, "n_paste": 5,
         "n_masks": 2, "stream": None}

# (argument, value, category): applied to every export that has the argument; "S" stands for H and for W of the _hw pair, each on its own
FAULTS = [
    ("images", None, b"null"), ("items", None, b"null"),
    ("n_images", 0, b"geometry"), ("count", -1, b"geometry"), ("count", 1025, b"geometry"), ("S", 4112, b"geometry"),
    ("S", 72, b"72 is not a multiple of 16"),
    ("images", P + 4, b"aligned"), ("items", P + 4, b"aligned"),
    # the groups an export has of its own
    ("label_offsets", P + 4, b"aligned"), ("vertex_offsets", P + 4, b"aligned"),
    ("n_rows", -1, b"geometry"), ("n_vertices", -1, b"geometry"), ("n_paste", 0, b"geometry"),
    ("n_masks", 0, b"geometry"), ("n_masks", 2 * VALID["count"] + 1, b"geometry"),
    ("dst_dtype", 7, b"dtype"), ("arena_bytes", 4098, b"multiple of 4"),
]

# where an export answers in another category than the fault's: it tests 2 S % 32 in its own line ahead of the shared check
OTHER_CATEGORY = {("y3_augment_batch_paste", "S=72"): b"geometry"}

MESSAGES = {
    "y3_augment_batch": {
        "images=None": b'y3_augment_batch: null argument',
        "items=None": b'y3_augment_batch: null argument',
        "n_images=0": b'y3_augment_batch: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_batch: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_batch: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_batch: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_batch: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_batch: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_batch: the record table and the items must be 8-byte aligned',
        "dst_dtype=7": b'y3_augment_batch: unsupported output dtype 7 (uint8 / float16 / bfloat16 / float32)',
        "arena_bytes=4098": b"y3_augment_batch: the arena's 4098 bytes are not a positive multiple of 4",
    },
    "y3_augment_batch_hw": {
        "images=None": b'y3_augment_batch_hw: null argument',
        "items=None": b'y3_augment_batch_hw: null argument',
        "n_images=0": b'y3_augment_batch_hw: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 48 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_batch_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 48 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_batch_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 48 x 64 in 16 .. 4096)',
        "H=4112": b'y3_augment_batch_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 64 in 16 .. 4096)',
        "W=4112": b'y3_augment_batch_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 48 x 4112 in 16 .. 4096)',
        "H=72": b'y3_augment_batch_hw: the image size 72 is not a multiple of 16',
        "W=72": b'y3_augment_batch_hw: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_batch_hw: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_batch_hw: the record table and the items must be 8-byte aligned',
        "dst_dtype=7": b'y3_augment_batch_hw: unsupported output dtype 7 (uint8 / float16 / bfloat16 / float32)',
        "arena_bytes=4098": b"y3_augment_batch_hw: the arena's 4098 bytes are not a positive multiple of 4",
    },
    "y3_augment_targets": {
        "images=None": b'y3_augment_targets: null argument',
        "items=None": b'y3_augment_targets: null argument',
        "n_images=0": b'y3_augment_targets: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_targets: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_targets: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_targets: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_targets: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_targets: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_targets: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_targets: the offsets must be 8-byte, the fp32 tables 4-byte aligned',
        "n_rows=-1": b'y3_augment_targets: bad geometry (-1 rows)',
    },
    "y3_augment_targets_hw": {
        "images=None": b'y3_augment_targets_hw: null argument',
        "items=None": b'y3_augment_targets_hw: null argument',
        "n_images=0": b'y3_augment_targets_hw: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 48 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_targets_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 48 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_targets_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 48 x 64 in 16 .. 4096)',
        "H=4112": b'y3_augment_targets_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 64 in 16 .. 4096)',
        "W=4112": b'y3_augment_targets_hw: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 48 x 4112 in 16 .. 4096)',
        "H=72": b'y3_augment_targets_hw: the image size 72 is not a multiple of 16',
        "W=72": b'y3_augment_targets_hw: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_targets_hw: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_targets_hw: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_targets_hw: the offsets must be 8-byte, the fp32 tables 4-byte aligned',
        "n_rows=-1": b'y3_augment_targets_hw: bad geometry (-1 rows)',
    },
    "y3_augment_polygons": {
        "images=None": b'y3_augment_polygons: null argument',
        "items=None": b'y3_augment_polygons: null argument',
        "n_images=0": b'y3_augment_polygons: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_polygons: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_polygons: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_polygons: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_polygons: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_polygons: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_polygons: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_polygons: the offsets and the boxes must be 8-byte, the vertices and the int32 words 4-byte aligned',
        "vertex_offsets=P+4": b'y3_augment_polygons: the offsets and the boxes must be 8-byte, the vertices and the int32 words 4-byte aligned',
        "n_rows=-1": b'y3_augment_polygons: bad geometry (100 vertices, 26 label rows, a workspace of -1 rows)',
        "n_vertices=-1": b'y3_augment_polygons: bad geometry (-1 vertices, 26 label rows, a workspace of 30 rows)',
    },
    "y3_augment_targets_polygons": {
        "images=None": b'y3_augment_targets_polygons: null argument',
        "items=None": b'y3_augment_targets_polygons: null argument',
        "n_images=0": b'y3_augment_targets_polygons: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_targets_polygons: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_targets_polygons: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_targets_polygons: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_targets_polygons: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_targets_polygons: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_targets_polygons: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_targets_polygons: the offsets and the boxes must be 8-byte, the fp32 tables and the int32 words 4-byte aligned',
        "n_rows=-1": b'y3_augment_targets_polygons: bad geometry (-1 rows)',
    },
    "y3_augment_copy_paste_select": {
        "images=None": b'y3_augment_copy_paste_select: null argument',
        "items=None": b'y3_augment_copy_paste_select: null argument',
        "n_images=0": b'y3_augment_copy_paste_select: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_copy_paste_select: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_copy_paste_select: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_copy_paste_select: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_copy_paste_select: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_copy_paste_select: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_copy_paste_select: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_copy_paste_select: the offsets must be 8-byte, the label table 4-byte aligned',
        "vertex_offsets=P+4": b'y3_augment_copy_paste_select: the offsets must be 8-byte, the label table 4-byte aligned',
        "n_vertices=-1": b'y3_augment_copy_paste_select: bad geometry (-1 vertices, 26 label rows)',
        "n_paste=0": b'y3_augment_copy_paste_select: bad geometry (0 candidates)',
    },
    "y3_augment_copy_paste_raster": {
        "images=None": b'y3_augment_copy_paste_raster: null argument',
        "items=None": b'y3_augment_copy_paste_raster: null argument',
        "n_images=0": b'y3_augment_copy_paste_raster: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_copy_paste_raster: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_copy_paste_raster: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_copy_paste_raster: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_copy_paste_raster: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_copy_paste_raster: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_copy_paste_raster: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_copy_paste_raster: the offsets must be 8-byte, the vertices and the masks 4-byte aligned',
        "vertex_offsets=P+4": b'y3_augment_copy_paste_raster: the offsets must be 8-byte, the vertices and the masks 4-byte aligned',
        "n_vertices=-1": b'y3_augment_copy_paste_raster: bad geometry (-1 vertices, 26 label rows, 2 masks for 4 items)',
        "n_paste=0": b'y3_augment_copy_paste_raster: bad geometry (0 candidates)',
        "n_masks=0": b'y3_augment_copy_paste_raster: bad geometry (100 vertices, 26 label rows, 0 masks for 4 items)',
        "n_masks=9": b'y3_augment_copy_paste_raster: bad geometry (100 vertices, 26 label rows, 9 masks for 4 items)',
    },
    "y3_augment_batch_paste": {
        "images=None": b'y3_augment_batch_paste: null argument',
        "items=None": b'y3_augment_batch_paste: null argument',
        "n_images=0": b'y3_augment_batch_paste: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_batch_paste: bad geometry (2 masks for -1 items of 64) or alignment',
        "count=1025": b'y3_augment_batch_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_batch_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_batch_paste: bad geometry (2 masks for 4 items of 72) or alignment',
        "images=P+4": b'y3_augment_batch_paste: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_batch_paste: the record table and the items must be 8-byte aligned',
        "n_masks=0": b'y3_augment_batch_paste: bad geometry (0 masks for 4 items of 64) or alignment',
        "n_masks=9": b'y3_augment_batch_paste: bad geometry (9 masks for 4 items of 64) or alignment',
        "dst_dtype=7": b'y3_augment_batch_paste: unsupported output dtype 7 (uint8 / float16 / bfloat16 / float32)',
        "arena_bytes=4098": b"y3_augment_batch_paste: the arena's 4098 bytes are not a positive multiple of 4",
    },
    "y3_augment_polygons_paste": {
        "images=None": b'y3_augment_polygons_paste: null argument',
        "items=None": b'y3_augment_polygons_paste: null argument',
        "n_images=0": b'y3_augment_polygons_paste: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_polygons_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_polygons_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_polygons_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_polygons_paste: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_polygons_paste: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_polygons_paste: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_polygons_paste: the offsets and the boxes must be 8-byte, the vertices and the int32 words 4-byte aligned',
        "vertex_offsets=P+4": b'y3_augment_polygons_paste: the offsets and the boxes must be 8-byte, the vertices and the int32 words 4-byte aligned',
        "n_rows=-1": b'y3_augment_polygons_paste: bad geometry (100 vertices, 26 label rows, a workspace of -1 rows)',
        "n_vertices=-1": b'y3_augment_polygons_paste: bad geometry (-1 vertices, 26 label rows, a workspace of 30 rows)',
        "n_paste=0": b'y3_augment_polygons_paste: bad geometry (0 candidates)',
    },
    "y3_augment_targets_paste": {
        "images=None": b'y3_augment_targets_paste: null argument',
        "items=None": b'y3_augment_targets_paste: null argument',
        "n_images=0": b'y3_augment_targets_paste: bad geometry (0 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=-1": b'y3_augment_targets_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of -1 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "count=1025": b'y3_augment_targets_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 1025 in 0 .. 1024 items of 64 x 64 in 16 .. 4096)',
        "S=4112": b'y3_augment_targets_paste: bad geometry (12 images in 1 .. 2^31 - 1, a batch of 4 in 0 .. 1024 items of 4112 x 4112 in 16 .. 4096)',
        "S=72": b'y3_augment_targets_paste: the image size 72 is not a multiple of 16',
        "images=P+4": b'y3_augment_targets_paste: the record table and the items must be 8-byte aligned',
        "items=P+4": b'y3_augment_targets_paste: the record table and the items must be 8-byte aligned',
        "label_offsets=P+4": b'y3_augment_targets_paste: the offsets and the boxes must be 8-byte, the fp32 tables and the int32 words 4-byte aligned',
        "n_rows=-1": b'y3_augment_targets_paste: bad geometry (-1 rows)',
        "n_paste=0": b'y3_augment_targets_paste: bad geometry (0 candidates)',
    },
}


def _parameters():
    header = re.sub(r"\s+", " ", (ROOT / "include" / "yolov3_hip.h").read_text())
    out = {}
    for name in EXPORTS:
        (args,) = re.findall(rf"\bint {name}\(([^)]*)\);", header)
        out[name] = [a.split()[-1].lstrip("*") for a in args.split(",")]
    return out


PARAMETERS = _parameters()


def _rows():
    for name in EXPORTS:
        for arg, value, category in FAULTS:
            for a in ("H", "W") if arg == "S" and "S" not in PARAMETERS[name] else (arg,):
                if a in PARAMETERS[name]:
                    fault = f"{a}={'P+4' if value == P + 4 else value}"
                    yield name, fault, a, value, OTHER_CATEGORY.get((name, fault), category)


ROWS = list(_rows())


@pytest.fixture(scope="module")
def lib():
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    return _lib.lib()


def test_the_table_covers_every_export_and_every_shared_fault():
    assert len(EXPORTS) == 11 and all(len(PARAMETERS[name]) >= 10 for name in EXPORTS)
    assert {(name, fault) for name, fault, *_ in ROWS} == {(name, fault) for name in MESSAGES for fault in MESSAGES[name]} and len(ROWS) == len(set(ROWS))
    for name in EXPORTS:
        faults = {fault for n, fault, *_ in ROWS if n == name}
        sides = ("H", "W") if name.endswith("_hw") else ("S",)
        shared = {"images=None", "items=None", "n_images=0", "count=-1", "count=1025", "images=P+4", "items=P+4"} | {f"{s}={v}" for s in sides for v in (4112, 72)}
        assert faults >= shared and len(faults - shared) >= 2   # and the groups of its own


@pytest.mark.parametrize("name,fault,arg,value,category", ROWS, ids=[f"{r[0]}-{r[1]}" for r in ROWS])
def test_an_export_refuses_one_bad_argument(lib, name, fault, arg, value, category):
    args = [value if p == arg else VALID.get(p, P) for p in PARAMETERS[name]]   # exactly one argument differs from the valid set
    status = getattr(lib, name)(*args)
    msg = lib.y3_last_error()
    assert status != 0 and msg.startswith(name.encode() + b":") and category in msg, (status, msg)
    assert msg == MESSAGES[name][fault]
