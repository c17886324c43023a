"""Host-side mirror of reference models/experimental.py ``Ensemble`` (:74-86): several detection models on one batch, their decoded predictions concatenated along
the row axis in front of ONE non_max_suppression (``detect.py`` / ``val.py --weights a.pt b.pt``; the list branch of ``attempt_load`` is in compat.py).

The reference runs every member, keeps element 0 of its eval output and ``torch.cat``s the predictions: a full copy, and every member's raw head tensors are
computed and dropped.  Here the concatenated prediction is allocated once and every member decodes straight into its row window of it (engine.run_model's
``out=``); the raw tensors are not written at all."""
from __future__ import annotations

import torch
from torch import nn


class Ensemble(nn.ModuleList):
    """reference models/experimental.py:74-86.  ``forward`` returns (y (bs, sum of the members' rows, no), None)."""

    def _member_dtype(self, m):
        from .engine import _engine_dtype

        return getattr(m, "infer_dtype", None) or _engine_dtype(m)

    def pred_rows(self, h, w, augment=False) -> int:
        """rows of ``self(x, augment)[0]`` for an (h, w) batch (host arithmetic only)"""
        from .engine import pred_rows

        return sum(pred_rows(m, h, w, augment) for m in self)

    def _check(self):
        """the members' agreement, before anything is launched: one row width, one inference dtype, eval mode"""
        if len(self) == 0:
            raise ValueError("Ensemble has no members")
        for m in self:
            if not hasattr(m, "_predict_into"):
                raise TypeError(f"Ensemble members are yolov3_amd detection models, not {type(m).__name__}")
            if m.training:
                raise RuntimeError("Ensemble.forward is an eval-mode path (the reference indexes the decoded prediction of eval mode)")
        nos = [m.model[-1].no for m in self]
        if len(set(nos)) != 1:
            raise ValueError(f"Ensemble members disagree on the prediction row width (nc + 5): {nos}")
        dts = [self._member_dtype(m) for m in self]
        if len(set(dts)) != 1:
            raise TypeError(f"Ensemble members disagree on the inference dtype: {dts}")
        return nos[0], dts[0]

    def _predict_into(self, x, out, augment=False, profile=False):
        """every member's prediction into consecutive row windows of out = (buffer, row_offset); returns the rows written.  All windows are checked before the first
        member runs."""
        from .engine import check_window

        self._check()
        buf, off = out
        spans, at = [], int(off)
        for m in self:
            rows = check_window(m, x, (buf, at), augment)[2]
            spans.append(at)
            at += rows
        for m, o in zip(self, spans):
            m._predict_into(x, (buf, o), augment, profile)
        return at - int(off)

    def forward(self, x, augment=False, profile=False, visualize=False):
        if visualize:
            raise NotImplementedError("feature visualisation is outside the accelerated hot path")
        from . import ops

        ops.require_gpu(x, "Ensemble.forward")
        if x.dim() != 4:
            raise ValueError(f"expected a (bs, ch, h, w) image batch, got shape {tuple(x.shape)}")
        no, dtype = self._check()
        y = torch.empty(x.shape[0], self.pred_rows(x.shape[2], x.shape[3], augment), no, dtype=dtype, device=x.device)
        self._predict_into(x, (y, 0), augment, profile)
        return y, None  # inference, train output
