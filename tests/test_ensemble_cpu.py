"""Host-side tests of model ensembles (reference models/experimental.py:74-136) and of the row-window arithmetic behind them: no GPU needed."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def test_attempt_load_of_two_checkpoints_is_the_reference_ensemble(golden_dir):
    from yolov3_amd import DetectionModel, Ensemble, attempt_load

    gold = torch.load(golden_dir / "ensemble.pt")
    a, b = golden_dir / "ref_tiny_w025_fp16.pt", golden_dir / "ref_tiny_w025_b_fp16.pt"
    ens = attempt_load([str(a), str(b)], device="cpu")
    assert isinstance(ens, Ensemble) and len(ens) == 2 and all(type(m) is DetectionModel for m in ens)
    assert not any(m.training for m in ens) and not any(".bn." in k for k in ens.state_dict())      # fused, eval
    assert all(p.dtype == torch.float32 for p in ens.parameters())
    assert dict(ens.names) == gold["names"] and ens.nc == gold["nc"] and [float(s) for s in ens.stride] == gold["stride"]
    assert ens.yaml == ens[0].yaml and ens.names[3] == "c3" and ens[1].names[3] == "b3"
    assert ens.pred_rows(96, 160) == sum(gold["rows"]) == gold["pred"].shape[1]
    with pytest.raises(RuntimeError, match="no CPU"):       # there is no CPU forward, for an ensemble as for a model
        ens(torch.zeros(1, 3, 64, 64))
    ens.train()
    with pytest.raises(RuntimeError, match="eval-mode"):
        ens._check()


def test_attempt_load_of_a_one_element_list_is_the_model_itself(golden_dir):
    from yolov3_amd import DetectionModel, attempt_load

    a = str(golden_dir / "ref_tiny_w025_fp16.pt")
    for w in ([a], (a,), a):
        assert type(attempt_load(w, device="cpu")) is DetectionModel


def test_members_with_different_class_counts_raise_the_reference_message(golden_dir, tmp_path):
    from yolov3_amd import DetectionModel, attempt_load

    other = DetectionModel("yolov3-tiny.yaml", nc=3)
    torch.save({"model": other, "ema": None}, tmp_path / "nc3.pt")
    with pytest.raises(AssertionError, match=re.escape("Models have different class counts: [80, 3]")):
        attempt_load([str(golden_dir / "ref_tiny_w025_fp16.pt"), str(tmp_path / "nc3.pt")], device="cpu")


def test_ensemble_is_in_the_unpickling_table():
    from yolov3_amd import Ensemble, compat

    assert compat._class_map()[("models.experimental", "Ensemble")] is Ensemble


@pytest.mark.parametrize("name", ["yolov3-tiny", "yolov3"])
@pytest.mark.parametrize("hw", [(96, 160), (64, 64)])
def test_pred_rows_equals_the_reference_row_counts(name, hw, golden_dir):
    """plain: na * sum of the Detect levels' maps (the oracle's own shape walk); augmented: the reference's _clip_augmented arithmetic on those counts, and the shape
    of the reference's own model(x, augment=True) where the TTA fixture has this model and size"""
    import yaml

    from oracle import yolo_oracle as yo
    from yolov3_amd import DetectionModel, engine

    h, w = hw
    m = DetectionModel(f"{name}.yaml", nc=80).eval()
    d = yaml.safe_load(open(ROOT / "yolov3_amd" / "cfg" / f"{name}.yaml"))
    layers, save, anchors, nc = yo.parse_cfg(d, 3, 80)
    strides = [int(s) for s in yo.model_strides(layers)]
    na, nl = 3, len(strides)

    def rows(hh, ww):   # the reference's Detect: one (ny, nx) map per level, na anchors each
        return na * sum((hh // s) * (ww // s) for s in strides)

    assert engine.pred_rows(m, h, w) == rows(h, w)
    gs, g = max(strides), sum(4**k for k in range(nl))
    sizes = [(h, w)] + [tuple(math.ceil(v * s / gs) * gs for v in (h, w)) for s in (0.83, 0.67)]     # upstream scale_img: padded up to the largest stride
    per = [rows(*s) for s in sizes]
    want = (per[0] - per[0] // g) + per[1] + (per[2] - (per[2] // g) * 4 ** (nl - 1))     # models/yolo.py:268-276
    assert engine.pred_rows(m, h, w, augment=True) == want
    if name == "yolov3-tiny" and hw == (96, 160):
        gold = torch.load(golden_dir / "tta.pt")["yolov3-tiny-nc20-96x160-bs2"]
        assert gold["pred"].shape[1] == want


def test_label_rows_is_exported_and_the_abi_version_stays(golden_dir):
    from yolov3_amd import _lib, build

    build.build(verbose=False)
    header = (ROOT / "include" / "yolov3_hip.h").read_text()
    assert re.search(r"\bint y3_label_rows\s*\(", header)
    assert "y3_label_rows" in _lib.exported_symbols() and len(_lib._SIGNATURES["y3_label_rows"][1]) == 13
    nm = subprocess.check_output(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], text=True)
    assert re.search(r" T y3_label_rows\b", nm)
    lib = _lib.lib()
    assert lib.y3_abi_version() == 6 == _lib.ABI_VERSION
    P = 1 << 20
    assert lib.y3_label_rows(P, 4, None, 2, 1.0, 1.0, P, _lib.Y3_F16, 100, 85, 90, 10, None) != 0 and b"null" in lib.y3_last_error()
    assert lib.y3_label_rows(P, 4, P, 2, 1.0, 1.0, P, _lib.Y3_F16, 100, 85, 95, 10, None) != 0 and b"geometry" in lib.y3_last_error()
    assert lib.y3_label_rows(P, 4, P, 2, 1.0, 1.0, P, 7, 100, 85, 90, 10, None) != 0 and b"dtype" in lib.y3_last_error()
    # the decode refuses a window that does not fit its buffer before it launches anything
    t = _lib.Y3Tensor(P, 2, 2, 2, 256, 256)
    anchors = (C.c_float * 6)(*[1.0] * 6)
    assert lib.y3_detect_decode(C.byref(t), _lib.Y3_F16, 3, 85, anchors, 32.0, None, P, 90, 100, None) != 0 and b"do not fit" in lib.y3_last_error()
