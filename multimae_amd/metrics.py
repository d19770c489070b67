"""Semantic-segmentation evaluation on the device (the reference: ``evaluate()`` of run_finetuning_semseg.py moves every prediction
and label map to the host, pickles them across ranks and runs numpy histograms, utils/semseg_metrics.py).

``seg_argmax`` takes the class map straight from the ConvNeXt head's low-resolution logits (functions.SegHandle), ``SegMetric``
keeps the four histograms of ``intersect_and_union`` (utils/semseg_metrics.py:49-59) in one int64 [4, K] device buffer, exchanges
them with one all-reduce and evaluates the ratios of ``eval_metrics`` (:216-222).  np.histogram's closed last bin (a value equal
to K counted into class K - 1) is not reproduced: predictions and labels outside [0, K) are dropped.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .criterion import _seg_handle


def seg_argmax(pred: torch.Tensor, num_classes: int) -> torch.Tensor:
    """``pred[:, :num_classes].argmax(dim=1)`` (int64, the lowest index on ties).  On an unmodified prediction of the ConvNeXt head
    the interpolation and the argmax run in one kernel on the head's logits and the (B, K, H, W) image is not written."""
    h = _seg_handle(pred)
    if h is None or not 0 < num_classes <= h.K:
        return pred[:, :num_classes].argmax(dim=1)
    out = torch.empty((h.B, h.H, h.W), device=h.logits.device, dtype=torch.int64)
    return ops.seg_argmax(h.logits, h.ld, out, h.B, h.h, h.w, h.K, int(num_classes), h.H, h.W, h.mode)


class SegMetric:
    """Running intersection / union / prediction / label histograms over the pixels with ``target != ignore_index``.

    update(pred_or_map, target)   a (B, K', H, W) prediction (its argmax over the first num_classes channels is taken, fused when
                                  it is the head's own output) or an integer class map of the target's shape
    sync()                        one all_reduce of the [4, K] buffer when torch.distributed is initialised
    compute()                     (all_acc, acc, iou) with eval_metrics' arithmetic; a class absent from labels and predictions is NaN"""

    def __init__(self, num_classes: int, ignore_index: int = 255, device=None):
        if not 0 < num_classes <= ops.SEG_HIST_MAX_K:
            raise ValueError(f'SegMetric: num_classes must be in [1, {ops.SEG_HIST_MAX_K}]')
        self.num_classes, self.ignore_index = int(num_classes), int(ignore_index)
        self.hist = None if device is None else torch.zeros((4, self.num_classes), device=device, dtype=torch.int64)

    def reset(self) -> None:
        if self.hist is not None:
            self.hist.zero_()

    @torch.no_grad()
    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        if pred.dim() == target.dim() + 1:
            pred = seg_argmax(pred, self.num_classes)
        if pred.shape != target.shape:
            raise ValueError(f'SegMetric.update: class map {tuple(pred.shape)} against target {tuple(target.shape)}')
        ops._require_gpu(target, 'segmentation labels')
        if self.hist is None:
            self.hist = torch.zeros((4, self.num_classes), device=target.device, dtype=torch.int64)
        ops.seg_hist(pred.contiguous().long(), target.contiguous().long(), self.num_classes, self.ignore_index, self.hist)

    def sync(self) -> None:
        if self.hist is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(self.hist)

    def compute(self):
        return ratios(self.hist.cpu().numpy())


def ratios(hist: np.ndarray):
    """eval_metrics' mIoU branch (utils/semseg_metrics.py:216-222) on the [4, K] histograms: overall accuracy, per-class accuracy,
    per-class IoU; 0 / 0 is NaN as there."""
    inter, union, _, label = (hist[i].astype(np.int64) for i in range(4))
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter.sum() / label.sum(), inter / label, inter / union
