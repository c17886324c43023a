"""What a validation or detection run writes: ``labels/*.txt`` (reference val.py:98-103 save_one_txt, detect.py:231-236), the COCO-JSON entries (val.py:134-144
save_one_json) and the plotting targets (utils/plots.py:69-78 output_to_target).  The reference builds a tensor, converts and opens a file per detection; here the boxes of
a whole batch are converted by ONE launch (y3_export_rows, csrc/val_edge.hip) into a compact (N, 7) table -- bit for bit the reference's fp32 values -- that reaches the host in
ONE copy; the rest is the reference's string formatting on NumPy rows (`txt_lines`, `json_entries`: pure functions, no device).  The JSON is evaluated by
`coco_eval.CocoEval` (pycocotools' bbox AP / AR on the device), not here."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import ops


def coco80_to_coco91_class():
    """reference utils/general.py coco80_to_coco91_class: the 80 ids of the 2014 / 2017 detection classes among the 91 of the COCO paper, ascending"""
    unused = {12, 26, 29, 30, 45, 66, 68, 69, 71, 83}
    return [i for i in range(1, 91) if i not in unused]


# ---- host formatting -------------------------------------------------------------------------------------------------------------------------------------------
def txt_lines(table, offsets, save_conf=False):
    """Compact "txt" table (N, 7) [image, cls, x, y, w, h, conf] + offsets (bs + 1) -> per image the text of its label file ("" for an image without rows):
    one ``("%g " * len(line)).rstrip() % line + "\\n"`` per row with line = (cls, x, y, w, h[, conf]) (val.py:101-103)."""
    fmt = ("%g " * (6 if save_conf else 5)).rstrip() + "\n"
    rows = np.asarray(table, dtype=np.float32).reshape(-1, 7)[:, 1:].tolist()   # Python floats of the fp32 values, as `.tolist()` gives the reference
    offs = [int(o) for o in offsets]
    return ["".join(fmt % (tuple(r) if save_conf else tuple(r[:5])) for r in rows[a:b]) for a, b in zip(offs[:-1], offs[1:])]


def json_entries(table, offsets, paths, class_map):
    """Compact "json" table (N, 7) [image, cls, left, top, w, h, conf] + offsets -> the dicts save_one_json appends (val.py:133-144), image by image"""
    rows = np.asarray(table, dtype=np.float32).reshape(-1, 7).tolist()
    offs = [int(o) for o in offsets]
    out = []
    for path, a, b in zip(paths, offs[:-1], offs[1:]):
        stem = Path(path).stem
        image_id = int(stem) if stem.isnumeric() else stem
        out.extend({"image_id": image_id, "category_id": class_map[int(r[1])], "bbox": [round(x, 3) for x in r[2:6]], "score": round(r[6], 5)} for r in rows[a:b])
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------------------------------------------
def _xyxy2xywh(x):
    y = x.clone()
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def _host_table(dets, form, sizes0=None, limit=0, round_boxes=False, reverse=False):
    """the table for detections that already are on the CPU: the reference's own tensor operations, image by image (no device, nothing to launch)"""
    parts, offs = [], [0]
    for i, d in enumerate(dets):
        d = d[: limit if limit > 0 else None, :6].float()
        box = d[:, :4].round() if round_boxes else d[:, :4]
        box = _xyxy2xywh(box)
        if form == "txt":
            box = box / torch.tensor(sizes0[i])[[1, 0, 1, 0]]   # gn = (w0, h0, w0, h0)
        elif form == "json":
            box[:, :2] -= box[:, 2:] / 2
        t = torch.cat((torch.full((d.shape[0], 1), i), d[:, 5:6], box, d[:, 4:5]), 1)
        parts.append(t.flip(0) if reverse else t)
        offs.append(offs[-1] + d.shape[0])
    table = torch.cat(parts, 0).numpy() if parts else np.zeros((0, 7), np.float32)
    return table.astype(np.float32, copy=False), np.asarray(offs, np.int32)


def _padded(dets):
    """a list of (n, 6+) fp32 device tensors as one padded block (base, img_stride, row_stride, counts, max_rows): the list `non_max_suppression` returns is views of one
    (bs, max_det, 6) buffer, which is used where it lies; any other list is gathered into a new block"""
    counts = [int(d.shape[0]) for d in dets]
    bs, most = len(dets), max(counts)
    d0 = dets[0]
    rs = d0.stride(0)
    same = all(d.dim() == 2 and d.dtype == torch.float32 and d.shape[1] >= 6 and d.stride(1) == 1 and d.stride(0) == rs and d.device == d0.device
               and d.untyped_storage().data_ptr() == d0.untyped_storage().data_ptr() for d in dets)
    if same and rs >= 6:
        offs = [d.storage_offset() for d in dets]
        step = offs[1] - offs[0] if bs > 1 else most * rs
        fits = offs[0] + (bs - 1) * step + (most - 1) * rs + 6 <= d0.untyped_storage().nbytes() // 4   # (the strided view below must lie inside the buffer)
        if fits and step >= most * rs and all(o == offs[0] + i * step for i, o in enumerate(offs)):
            return d0.as_strided((bs, most, 6), (step, rs, 1), offs[0]), step, rs, counts, most
    block = torch.zeros(bs, most, 6, dtype=torch.float32, device=d0.device)
    for i, d in enumerate(dets):
        if counts[i]:
            block[i, : counts[i]] = d[:, :6]
    return block, most * 6, 6, counts, most


def _counts(counts, bs, dev):
    """`counts` as (device int32 tensor, host list): the (tensor, list) pair `non_max_suppression_batched` returns costs nothing; a host sequence is uploaded (no
    synchronisation); a device tensor alone is read back (one more synchronisation: pass the host list NMS already produced instead)"""
    if isinstance(counts, (tuple, list)) and len(counts) == 2 and isinstance(counts[0], torch.Tensor) and not isinstance(counts[1], torch.Tensor):
        dev_counts, host = counts[0], [int(c) for c in counts[1]]
    elif isinstance(counts, torch.Tensor):
        host = [int(c) for c in counts.tolist()]
        dev_counts = counts if counts.is_cuda else None
    else:
        host, dev_counts = [int(c) for c in counts], None
    if len(host) != bs:
        raise ValueError(f"{len(host)} counts for a batch of {bs}")
    if dev_counts is None:
        dev_counts = torch.tensor(host, dtype=torch.int32).to(dev, non_blocking=True)
    return dev_counts.to(torch.int32).contiguous(), host


def export_table(rows, counts, form, sizes0=None, limit=0, round_boxes=False, reverse=False, image0=0, nc=0):
    """(bs, max_rows, 6+) fp32 device rows + counts -> (table (N, 7) float32 NumPy, offsets (bs + 1) NumPy[, class histogram (bs, nc) NumPy]): one launch, one
    device->host copy (table, offsets and histogram travel as one block).  `sizes0`: per image (h0, w0), the "txt" form's divisor."""
    ops.require_gpu(rows, "export_table")
    if rows.dim() != 3 or rows.dtype != torch.float32 or rows.shape[2] < 6 or rows.stride(2) != 1:
        raise TypeError("export_table expects (bs, max_rows, 6) fp32 rows [x1, y1, x2, y2, conf, cls]")
    bs, max_rows = rows.shape[0], rows.shape[1]
    dev = rows.device
    dev_counts, host = _counts(counts, bs, dev)
    total = sum(min(c, max_rows, limit) if limit > 0 else min(c, max_rows) for c in host)
    sizes = None
    if form == "txt":
        if sizes0 is None or len(sizes0) != bs:
            raise ValueError("the txt form needs the native (h0, w0) of every image")
        sizes = torch.tensor([[float(s[1]), float(s[0])] for s in sizes0], dtype=torch.float32).to(dev, non_blocking=True)
    table, offsets, hist = ops.export_rows(rows, rows.stride(0), rows.stride(1), dev_counts, bs, max_rows, form, total, limit, round_boxes, reverse, image0, sizes, nc)
    parts = [table.view(-1).view(torch.int32), offsets] + ([hist.view(-1)] if hist is not None else [])   # (bit patterns: one block, one copy)
    host_block = torch.cat(parts).cpu().numpy()
    t = host_block[: total * 7].view(np.float32).reshape(total, 7)
    o = host_block[total * 7 : total * 7 + bs + 1]
    return (t, o, host_block[total * 7 + bs + 1 :].reshape(bs, nc)) if hist is not None else (t, o)


def _list_table(dets, form, sizes0=None, limit=0, round_boxes=False, reverse=False):
    """export_table for a list of per-image (n, 6) tensors: device tensors go through the kernel (one launch, one copy), CPU tensors through the host path"""
    dets = list(dets)
    if not dets or max(int(d.shape[0]) for d in dets) == 0:
        return np.zeros((0, 7), np.float32), np.zeros(len(dets) + 1, np.int32)
    if not dets[0].is_cuda:
        return _host_table(dets, form, sizes0, limit, round_boxes, reverse)
    block, _, _, counts, _ = _padded(dets)
    return export_table(block, counts, form, sizes0, limit, round_boxes, reverse)


# ---- the reference's signatures --------------------------------------------------------------------------------------------------------------------------------
def output_to_target(output, max_det=300):
    """Drop-in for reference utils/plots.py:69: `output` is the list of (n, 6) detections of a batch, or the (rows, counts) pair of `non_max_suppression_batched`
    (its whole 3-tuple works too); returns the (N, 7) float32 NumPy array [batch_id, class_id, x, y, w, h, conf] of at most `max_det` rows per image."""
    if isinstance(output, (tuple, list)) and len(output) in (2, 3) and isinstance(output[0], torch.Tensor) and output[0].dim() == 3:
        counts = output[1] if len(output) == 2 else (output[1], output[2])
        return export_table(output[0], counts, "target", limit=max_det)[0]
    return _list_table(output, "target", limit=max_det)[0]


def _append(file, text):
    if text:   # no file for an image without detections: the reference opens it per line
        with open(file, "a") as f:
            f.write(text)


def save_one_txt(predn, save_conf, shape, file):
    """Drop-in for reference val.py:60: append one `cls x y w h [conf]` line per row of predn (n, 6) [x1, y1, x2, y2, conf, cls] in native pixels, normalised by
    shape = (h0, w0)"""
    table, offs = _list_table([predn], "txt", sizes0=[shape])
    _append(file, txt_lines(table, offs, save_conf)[0])


def save_one_json(predn, jdict, path, class_map):
    """Drop-in for reference val.py:106: append {"image_id", "category_id", "bbox" [left, top, w, h], "score"} per row of predn to `jdict`"""
    table, offs = _list_table([predn], "json")
    jdict.extend(json_entries(table, offs, [path], class_map))


# ---- a batch at a time -----------------------------------------------------------------------------------------------------------------------------------------
def save_txt_batched(rows, counts, shapes0, paths, labels_dir, save_conf=False, detect=False):
    """save_one_txt for every image of a batch: rows (bs, max_det, 6) fp32 on the device in native pixels (after `scale_boxes_batched`), counts as `_counts` takes them
    (pass the host list, or the (tensor, list) pair, NMS produced), shapes0[i] = (h0, w0), paths[i] the image file; appends to ``labels_dir / (stem + ".txt")``.
    `detect`: the writer of detect.py:223-236 -- corners rounded half to even first, rows last to first.  Returns the files written to."""
    table, offs = export_table(rows, counts, "txt", sizes0=shapes0, round_boxes=detect, reverse=detect)
    labels_dir = Path(labels_dir)
    labels_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for path, text in zip(paths, txt_lines(table, offs, save_conf)):
        if text:
            written.append(labels_dir / f"{Path(path).stem}.txt")
            _append(written[-1], text)
    return written


def save_json_batched(rows, counts, paths, jdict, class_map):
    """save_one_json for every image of a batch, appended to `jdict` in image order"""
    table, offs = export_table(rows, counts, "json")
    jdict.extend(json_entries(table, offs, paths, class_map))
    return jdict


# ---- Detections: the text half (reference models/common.py:908-913, 951-952, 990-998) ---------------------------------------------------------------------------
def class_histograms(pred, nc):
    """per image {class: rows} in ascending class order, what `for c in pred[:, -1].unique(): n = (pred[:, -1] == c).sum()` gives: device predictions through the
    histogram of one export launch, CPU predictions through torch.unique"""
    pred = list(pred)
    if not pred or max(int(p.shape[0]) for p in pred) == 0:
        return [{} for _ in pred]
    if not pred[0].is_cuda:
        out = []
        for p in pred:
            c, n = (p[:, 5].unique(return_counts=True)) if p.shape[0] else ((), ())
            out.append({int(a): int(b) for a, b in zip(c, n)})
        return out
    block, _, _, counts, _ = _padded(pred)
    hist = export_table(block, counts, "target", nc=nc)[2]
    return [{int(c): int(h[c]) for c in np.nonzero(h)[0]} for h in hist]
