"""Precision / recall / AP accumulation and the confusion matrix, the last step of a validation run.

On the device (csrc/val_stats.hip): `ValStats` keeps the rows of a run (confidence, class, one bit per IoU threshold) in dense device buffers --
the replacement of val.py's `stats` list -- and `compute()` orders them, builds the fp64 curves and the summary there; only the reference's
7-tuple crosses to the host.  `ap_per_class_device` is the same computation for rows that are already concatenated, `ConfusionMatrix` the
reference's class with its matching in one launch per batch.  Score ties are ordered by arrival (the rule `ap_per_class(..., stable=True)` states
on the host).

On the host (NumPy): `process_batch` (csrc/val_edge.hip) yields one row of IoU-threshold hits per detection.  `ap_per_class` turns the
concatenated rows of a run into the numbers reference val.py:417-421 prints, with the call contract of reference
utils/metrics.py:22 (`ap_per_class`, positional 7-tuple) and :89 (`compute_ap`) so a `val.py`-style loop can call it unchanged; it is the CPU
expectation of the device path.  It is written from the definitions, not from the reference's code:

  * detections are ranked once by confidence; for a class c the k-th ranked detection of that class has
        recall_k = TP_k / n_labels(c),   precision_k = TP_k / k            (TP_k = hits among the first k)
    per IoU threshold -- all thresholds at once as a (k, T) array;
  * AP is COCO's 101-point interpolation: area under the monotone precision envelope sampled at recall 0, 0.01, ..., 1;
  * the reported P / R / F1 are read at the confidence where the class-mean F1 curve, box-filtered over 10 % of its 1000 samples
    (upstream ultralytics.utils.metrics.smooth, un-vendored), peaks.

Pinned to the unmodified reference by tests/golden/metrics.pt (the golden-vector tests, 1e-12).  No plotting."""
from __future__ import annotations

import numpy as np

_CONF_GRID = np.linspace(0.0, 1.0, 1000)     # confidence axis of the P(conf) / R(conf) curves
_RECALL_GRID = np.linspace(0.0, 1.0, 101)    # COCO recall samples


def fitness(x):
    """model-selection score of reference utils/metrics.py:15: 0.1 * mAP@0.5 + 0.9 * mAP@0.5:0.95 of rows [P, R, mAP50, mAP, ...]"""
    x = np.asarray(x)
    return 0.1 * x[:, 2] + 0.9 * x[:, 3]


def smooth(y, f=0.05):
    """moving average over a window of ~2 f len(y) samples (odd length), edges extended by their end values"""
    win = round(len(y) * f * 2) // 2 + 1
    half = win // 2
    padded = np.concatenate((np.full(half, y[0], dtype=float), y, np.full(half, y[-1], dtype=float)))
    return np.convolve(padded, np.full(win, 1.0 / win), mode="valid")


def compute_ap(recall, precision):
    """101-point interpolated average precision of one curve (recall ascending).  Returns (ap, envelope, recall) with the
    sentinels (recall 0 / precision 1 in front, recall 1 / precision 0 behind) included, like reference utils/metrics.py:89."""
    rec = np.concatenate(([0.0], recall, [1.0]))
    env = np.concatenate(([1.0], precision, [0.0]))
    env = np.maximum.accumulate(env[::-1])[::-1]            # best precision at this recall or beyond
    samples = np.interp(_RECALL_GRID, rec, env)
    area = float(((samples[1:] + samples[:-1]) * np.diff(_RECALL_GRID)).sum() * 0.5)   # trapezoid rule on the 101 samples
    return area, env, rec


def _class_curves(hits, conf, n_labels, eps):
    """hits (k, T) 0/1 in rank order, conf (k,) descending.  -> recall (k, T), precision (k, T), and both sampled on the
    confidence grid at the FIRST threshold (what the reference reports as P / R)."""
    tp_run = np.cumsum(hits, axis=0)
    fp_run = np.cumsum(1 - hits, axis=0)
    recall = tp_run / (n_labels + eps)
    precision = tp_run / (tp_run + fp_run)
    # np.interp wants ascending abscissae: walk the confidence axis downwards
    r_of_conf = np.interp(-_CONF_GRID, -conf, recall[:, 0], left=0)
    p_of_conf = np.interp(-_CONF_GRID, -conf, precision[:, 0], left=1)
    return recall, precision, r_of_conf, p_of_conf


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir=".", names=(), eps=1e-16, prefix="", stable=False):
    """Per-class statistics of a validation run; call contract of reference utils/metrics.py:22 (`plot`, `save_dir`, `names`,
    `prefix` accepted and ignored).  tp (n, T) from process_batch, conf / pred_cls (n,), target_cls (n_labels,).
    Returns (tp_count, fp_count, p, r, f1, ap (classes, T), classes) over the classes that have labels.
    stable=True ranks equal confidences by arrival (np.argsort(kind="stable")): the tie rule of the device path; the default is the reference's."""
    order = np.argsort(-conf, kind="stable") if stable else np.argsort(-conf)
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, label_counts = np.unique(target_cls, return_counts=True)
    n_cls, n_thr = classes.shape[0], tp.shape[1]
    ap = np.zeros((n_cls, n_thr))
    p_curve = np.zeros((n_cls, _CONF_GRID.size))
    r_curve = np.zeros((n_cls, _CONF_GRID.size))
    for row, (cls, n_lab) in enumerate(zip(classes, label_counts)):
        mine = pred_cls == cls
        if not mine.any() or n_lab == 0:
            continue
        recall, precision, r_curve[row], p_curve[row] = _class_curves(tp[mine], conf[mine], n_lab, eps)
        ap[row] = [compute_ap(recall[:, t], precision[:, t])[0] for t in range(n_thr)]
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    best = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, best], r_curve[:, best], f1_curve[:, best]
    tp_count = (r * label_counts).round()
    fp_count = (tp_count / (p + eps) - tp_count).round()
    return tp_count, fp_count, p, r, f1, ap, classes.astype(int)


def mean_results(stats):
    """[(correct, conf, pred_cls, target_cls), ...] per image (NumPy) -> (mean P, mean R, mAP@0.5, mAP@0.5:0.95), the summary line
    of reference val.py:416-421."""
    cols = [np.concatenate(c, 0) for c in zip(*stats)]
    if not cols or not cols[0].any():
        return 0.0, 0.0, 0.0, 0.0
    _, _, p, r, _, ap, _ = ap_per_class(*cols)
    return float(p.mean()), float(r.mean()), float(ap[:, 0].mean()), float(ap.mean(1).mean())


# ------------------------------------------------------------------------------------------------ device path (csrc/val_stats.hip)
def _unpack_result(block, n_thr):
    """the result block of y3_val_stats_compute (one device->host copy) -> (7-tuple, any row has a hit)"""
    h = block.cpu().numpy()
    present = int(h[0])
    rows = h[4:4 + present * (n_thr + 6)].reshape(present, n_thr + 6)
    out = (rows[:, 1].copy(), rows[:, 2].copy(), rows[:, 3].copy(), rows[:, 4].copy(), rows[:, 5].copy(), rows[:, 6:].copy(), rows[:, 0].astype(int))
    return out, bool(h[2]), int(h[1]), int(h[3])


def ap_per_class_device(tp, conf, pred_cls, target_cls, eps=1e-16, nc=1024):
    """`ap_per_class` on the MI355X: tp (n, T) bool / uint8, conf (n,), pred_cls (n,), target_cls (n_labels,) DEVICE tensors (what a val.py loop has
    before its `.cpu()`), the reference's 7-tuple out (NumPy fp64, shapes and order of `ap_per_class`).  Equal confidences rank by arrival.  Classes are
    integers in [0, nc); a label class outside that range raises."""
    from . import ops

    ops.require_gpu(conf, "ap_per_class_device")
    ops.require_gpu(target_cls, "ap_per_class_device")
    st = ValStats(nc, int(tp.shape[1]), conf.device)
    st.append_rows(tp, conf, pred_cls)
    st.add_labels(target_cls)
    return st.compute(eps=eps)


class ValStats:
    """The `stats` list of reference val.py:349,388,407 kept on the device: `update` appends a batch's rows where the batched NMS /
    matching left them, without a synchronisation (buffer sizes follow the NMS counts the host already holds; growth is geometric),
    `compute()` is val.py:424-426 (`ap_per_class` on the device, one read-back of classes x (T + 5) doubles and the class ids).
    `iouv`: the IoU thresholds (a tensor / sequence, at most 16) or their number."""

    def __init__(self, nc, iouv, device):
        import torch

        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"ValStats: device {self.device}; the yolov3_amd hot path runs only on an MI355X (HIP) device. There is no CPU / PyTorch fallback.")
        self.nc = int(nc)
        self.niou = int(iouv) if isinstance(iouv, int) else int(len(iouv))
        if not 1 <= self.niou <= 16:
            raise ValueError("ValStats: 1 .. 16 IoU thresholds")
        self.n = 0
        self._cap = 0
        self._conf = self._cls = self._mask = None
        self._nt = torch.zeros(self.nc, dtype=torch.int32, device=self.device)
        self._result = None
        self._labels = 0

    def _reserve(self, extra):
        import torch

        need = self.n + extra
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 4096)
        new = (torch.empty(cap, dtype=torch.float32, device=self.device), torch.empty(cap, dtype=torch.int32, device=self.device),
               torch.empty(cap, dtype=torch.int16, device=self.device))
        if self.n:
            for dst, src in zip(new, (self._conf, self._cls, self._mask)):
                dst[:self.n].copy_(src[:self.n])
        self._conf, self._cls, self._mask = new
        self._cap = cap

    def update(self, rows, counts, counts_list, correct, labels, label_offsets=None):
        """one batch: rows (bs, max_det, 6) fp32 + counts (device int32) + counts_list (the same counts on the host) of
        `non_max_suppression_batched`, correct (bs, max_det, T) of `process_batch_batched`, labels (nl, 5) [cls, ...] of the batch (every label
        counts, val.py:388,407).  No device->host copy."""
        from . import ops

        ops.require_gpu(rows, "ValStats.update")
        if rows.dim() != 3 or rows.shape[2] < 6 or rows.dtype.is_floating_point is False or rows.stride(2) != 1:
            raise TypeError("ValStats.update expects the (bs, max_det, 6) fp32 NMS output")
        bs, max_det = rows.shape[0], rows.shape[1]
        if correct.shape[-1] != self.niou:
            raise ValueError(f"ValStats.update: correct has {correct.shape[-1]} thresholds, the statistics {self.niou}")
        total = int(sum(min(max(int(c), 0), max_det) for c in counts_list))
        if total:
            self._reserve(total)
            ops.val_stats_append(rows[0, 0, 4:], rows[0, 0, 5:], rows.stride(0), rows.stride(1), counts, bs, max_det, correct, self._conf, self._cls, self._mask, self.n)
            self.n += total
        if labels is not None and labels.shape[0]:
            self.add_labels(labels)
        self._result = None

    def append_rows(self, tp, conf, pred_cls):
        """concatenated rows (what val.py holds after torch.cat): tp (n, T), conf (n,), pred_cls (n,) device tensors"""
        import torch

        from . import ops

        n = int(conf.shape[0])
        if n:
            ops.require_gpu(tp, "ValStats")
            self._reserve(n)
            c32 = conf if conf.dtype == torch.float32 and conf.is_contiguous() else conf.float().contiguous()
            k32 = pred_cls if pred_cls.dtype == torch.float32 and pred_cls.is_contiguous() else pred_cls.float().contiguous()
            ops.val_stats_append(c32, k32, 0, 1, None, 1, n, tp.contiguous(), self._conf, self._cls, self._mask, self.n)
            self.n += n
        self._result = None

    def add_labels(self, labels):
        """label classes into the per-class histogram: a (nl, k) tensor whose column 0 is the class, or a class vector"""
        import torch

        from . import ops

        if labels.shape[0] == 0:
            return
        ops.require_gpu(labels, "ValStats")
        lab = labels if labels.dtype == torch.float32 else labels.float()
        ops.val_stats_count_labels(lab, lab.stride(0), lab.shape[0], self._nt)
        self._labels += int(lab.shape[0])
        self._result = None

    @property
    def nt(self):
        """labels per class (val.py:429), NumPy int64 -- a device->host copy"""
        return self._nt.cpu().numpy().astype(np.int64)

    def compute(self, eps=1e-16):
        """val.py:426: (tp, fp, p, r, f1, ap (classes, T), classes) over the classes that have labels"""
        from . import ops

        if self._result is None:
            block = ops.val_stats_compute(self._conf, self._cls, self._mask, self.n, self._nt, self.niou, eps)
            self._result = _unpack_result(block, self.niou)
            if self._result[3] != self._labels:
                raise ValueError(f"ValStats: {self._labels - self._result[3]} label classes lie outside [0, {self.nc})")
        return self._result[0]

    def results(self):
        """(mp, mr, map50, map) of val.py:425-428; zeros for an empty run and for a run without a correct detection"""
        tp, fp, p, r, f1, ap, classes = self.compute()
        if self.n == 0 or not self._result[1] or classes.size == 0:
            return 0.0, 0.0, 0.0, 0.0
        return float(p.mean()), float(r.mean()), float(ap[:, 0].mean()), float(ap.mean(1).mean())

    def maps(self, nc=None):
        """per-class mAP@0.5:0.95 with the mean for classes without labels (val.py:485-488)"""
        nc = self.nc if nc is None else nc
        out = np.zeros(nc) + self.results()[3]
        if self.n and self._result[1]:
            ap, classes = self._result[0][5], self._result[0][6]
            for i, c in enumerate(classes):
                out[c] = ap[i].mean()
        return out


class ConfusionMatrix:
    """reference utils/metrics.py:124 with the matching on the device (csrc/val_stats.hip::confusion_kernel): the matrix is a device int64
    (nc + 1, nc + 1) accumulator, rows = predicted class, columns = true class, index nc = background.  `.matrix` reads it back (the one
    synchronising access) as the reference's float64 array."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.nc = nc
        self.conf = conf
        self.iou_thres = iou_thres
        self._matrix = None

    def _acc(self, like):
        import torch

        from . import ops

        ops.require_gpu(like, "ConfusionMatrix")
        if self._matrix is None:
            self._matrix = torch.zeros(self.nc + 1, self.nc + 1, dtype=torch.int64, device=like.device)
        return self._matrix

    def process_batch(self, detections, labels):
        """one image, reference signature: detections (N, 6) [x1, y1, x2, y2, conf, cls] or None, labels (M, 5) [cls, x1, y1, x2, y2]
        (with detections=None: the class vector, val.py:390)"""
        import torch

        from . import ops

        m = self._acc(labels)
        if labels.shape[0] == 0:
            return
        lab = labels.to(torch.float32).contiguous()
        offs = torch.tensor([0, lab.shape[0]], dtype=torch.int32).to(m.device, non_blocking=True)
        if detections is None:
            ops.confusion_matrix_raw(None, 0, 6, None, 1, 0, lab, 1 if lab.dim() == 1 else lab.stride(0), offs, self.nc, self.conf, self.iou_thres, m)
            return
        ops.require_gpu(detections, "ConfusionMatrix")
        n = detections.shape[0]
        if n > 4096:
            raise ValueError("ConfusionMatrix: more than 4096 detections per image is not supported")
        dets = detections if (detections.dtype == torch.float32 and detections.stride(1) == 1) else detections.float().contiguous()
        ops.confusion_matrix_raw(dets if n else None, 0, max(dets.stride(0), 6) if n else 6, None, 1, n, lab, lab.stride(0) if n else max(lab.stride(0), 1), offs, self.nc, self.conf,
                                 self.iou_thres, m)

    def process_batch_batched(self, rows, counts, labels, label_offsets):
        """a whole batch in one launch: the inputs of `val.process_batch_batched`"""
        import torch

        from . import ops

        m = self._acc(rows)
        if rows.dtype != torch.float32 or rows.dim() != 3 or not rows.is_contiguous():
            raise TypeError("ConfusionMatrix.process_batch_batched expects the contiguous (bs, max_det, 6) fp32 NMS output")
        lab = labels.to(m.device, torch.float32).contiguous()
        offs = label_offsets.to(m.device, torch.int32).contiguous()
        if offs.numel() != rows.shape[0] + 1:
            raise ValueError("label_offsets must hold bs + 1 entries")
        ops.confusion_matrix_raw(rows, rows.stride(0), rows.stride(1), counts, rows.shape[0], rows.shape[1], lab, 5, offs, self.nc, self.conf, self.iou_thres, m)

    @property
    def matrix(self):
        if self._matrix is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        return self._matrix.cpu().numpy().astype(np.float64)

    def tp_fp(self):
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]

    def plot(self, normalize=True, save_dir="", names=()):
        raise NotImplementedError("plots are out of scope of yolov3_amd (DESIGN.md section 8)")

    def print(self):
        for row in self.matrix:
            print(" ".join(map(str, row)))
