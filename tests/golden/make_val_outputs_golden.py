"""Generate tests/golden/val_outputs.pt by running the UNMODIFIED reference (through oracle/ref_shim.py) on the seeded inputs of tests/val_outputs_cases.py:
`save_one_txt` / `save_one_json` of val.py, `output_to_target` of utils/plots.py and `Detections` of models/common.py.  The `--save-txt` loop of detect.py:223-236 is
inline code of that file's run() and cannot be called: its files are save_one_txt's (the same per-box statements) fed the rows rounded by `.round()` and last to first.  (`coco80_to_coco91_class` is imported by the reference from a package it does not vendor: the class map of the COCO case is
val_outputs_cases.coco_map().)  Run where the reference tree is present:

    python tests/golden/make_val_outputs_golden.py

The fixture stores reference OUTPUTS and input checksums only; the tests regenerate the inputs from their seeds."""
from __future__ import annotations

import importlib
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import val_outputs_cases as oc  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = Path(__file__).resolve().parent


def table(parts):
    """(N, 7) fp32 [image, cls, box, conf] from per-image (box (n, 4), det (n, 6)) pairs + offsets, put together with the reference's torch.cat as output_to_target does"""
    rows, offs = [], [0]
    for i, (box, d) in enumerate(parts):
        rows.append(torch.cat((torch.full((d.shape[0], 1), i), d[:, 5:6], box, d[:, 4:5]), 1))
        offs.append(offs[-1] + d.shape[0])
    return torch.cat(rows, 0).float(), torch.tensor(offs, dtype=torch.int32)


def main():
    ref_shim.load()
    val = importlib.import_module("val")
    plots = importlib.import_module("utils.plots")
    general = importlib.import_module("utils.general")
    common = importlib.import_module("models.common")
    xyxy2xywh = general.xyxy2xywh
    coco = oc.coco_map()
    out = {"cases": {}}
    for name in oc.CASES:
        c = oc.case(name)
        dets, shapes, paths = oc.dets(c), c["shapes"], [Path(p) for p in c["paths"]]
        rec = {"in_sum": oc.checksum(c), "counts": list(c["counts"])}
        # output_to_target itself, at every cap of the case
        for limit in (c["limits"] or (300,)):
            rec[f"target_{limit}"] = torch.from_numpy(plots.output_to_target(dets, max_det=limit))
            rec[f"target_{limit}_offsets"] = torch.tensor([0] + list(np.cumsum([min(n, limit) for n in c["counts"]])), dtype=torch.int32)
        # the compact tables of the other forms, with the reference's own tensor operations (val.py:98-100, 134-135; detect.py:223,231-233)
        txt, js, det = [], [], []
        for d, shape in zip(dets, shapes):
            gn = torch.tensor(shape)[[1, 0, 1, 0]]
            txt.append((xyxy2xywh(d[:, :4]) / gn, d))
            box = xyxy2xywh(d[:, :4])
            box[:, :2] -= box[:, 2:] / 2
            js.append((box, d))
            r = d.clone()
            r[:, :4] = r[:, :4].round()
            r = r.flip(0)   # reversed(det)
            det.append((xyxy2xywh(r[:, :4]) / gn, r))
        rec["txt"], rec["offsets"] = table(txt)
        rec["json"], _ = table(js)
        rec["detect"], _ = table(det)
        if name == "detect":
            ties = sum(int(((d[:, :4] - d[:, :4].floor()) == 0.5).sum()) for d in dets)
            changed = sum(int((d[:, :4].round() != (d[:, :4] + 0.5).floor()).sum()) for d in dets)
            assert ties >= 4 and changed >= 2, (ties, changed)   # exact ties, and half-to-even differs from half-up on some of them
        if name in oc.JSON_CASES:
            x1 = torch.cat([d[:, 0] for d in dets])
            differ = float((rec["json"][:, 2] != x1).float().mean())
            assert differ >= 0.25, differ   # cx - w / 2 is not x1: a shortcut cannot pass
            jdict, class_map = [], (coco if c["nc"] == 80 else list(range(1000)))
            for d, p in zip(dets, paths):
                if d.shape[0]:   # val.py:386-391: an image without predictions is skipped before the writers
                    val.save_one_json(d.clone(), jdict, p, class_map)
            rec["jdict"] = jdict
            print(name, "json rows whose corner is not x1:", differ)
        if name in oc.TXT_CASES:
            with tempfile.TemporaryDirectory() as tmp:
                for save_conf in (False, True):
                    folder = Path(tmp) / f"val{int(save_conf)}"
                    folder.mkdir()
                    for d, shape, p in zip(dets, shapes, paths):
                        if d.shape[0]:
                            val.save_one_txt(d.clone(), save_conf, shape, file=folder / f"{p.stem}.txt")
                    rec[f"files_conf{int(save_conf)}"] = {f.name: f.read_bytes() for f in sorted(folder.iterdir())}
                if name == "detect":   # detect.py:223-236 is inline code of its run(): its per-box body is save_one_txt's, fed the rounded rows last to first
                    for save_conf in (False, True):
                        folder = Path(tmp) / f"detect{int(save_conf)}"
                        folder.mkdir()
                        for (_, r), shape, p in zip(det, shapes, paths):
                            if r.shape[0]:
                                val.save_one_txt(r.clone(), save_conf, shape, file=folder / f"{p.stem}.txt")
                        rec[f"detect_files_conf{int(save_conf)}"] = {f.name: f.read_bytes() for f in sorted(folder.iterdir())}
        out["cases"][name] = rec
        print(name, "bs", len(dets), "rows", int(rec["offsets"][-1]), {k: (tuple(v.shape) if hasattr(v, "shape") else len(v)) for k, v in rec.items() if k not in ("in_sum", "counts")})
    # Detections: the strings and the DataFrame values of the detect case (an image with one row, one with two rows of one class, one without detections)
    c = oc.case("detect")
    dets = oc.dets(c)
    ims = [np.zeros((*s, 3), np.uint8) for s in c["shapes"]]
    files = [Path(p).name for p in c["paths"]]
    times = tuple(types.SimpleNamespace(t=t) for t in oc.TIMES)   # Detections reads `.t` of the three profilers
    d = common.Detections(ims, dets, files, times, dict(enumerate(oc.NAMES)), oc.DETECTIONS_SHAPE)
    frames = d.pandas()
    out["detections"] = {"str": str(d), "repr": repr(d),
                         "pandas": {k: [(list(df.columns), df.values.tolist()) for df in getattr(frames, k)] for k in ("xyxy", "xyxyn", "xywh", "xywhn")}}
    print(str(d))
    torch.save(out, OUT / "val_outputs.pt")
    print("val_outputs.pt", (OUT / "val_outputs.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
