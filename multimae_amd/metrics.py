"""Semantic-segmentation evaluation on the device (the reference: ``evaluate()`` of run_finetuning_semseg.py moves every prediction
and label map to the host, pickles them across ranks and runs numpy histograms, utils/semseg_metrics.py).

``seg_argmax`` takes the class map straight from the ConvNeXt head's low-resolution logits (functions.SegHandle), ``SegMetric``
keeps the four histograms of ``intersect_and_union`` (utils/semseg_metrics.py:49-59) in one int64 [4, K] device buffer, exchanges
them with one all-reduce and evaluates the ratios of ``eval_metrics`` (:216-222).  np.histogram's closed last bin (a value equal
to K counted into class K - 1) is not reproduced: predictions and labels outside [0, K) are dropped.

Depth evaluation (``masked_nyu_metrics``, run_finetuning_depth.py:86-117, about thirty small launches and -- through
``MetricLogger.update`` -- one ``.item()`` per metric and step): ``depth_metrics`` computes the seven values in one pass over the
ConvNeXt head's low-resolution map or over the DPT head's image, ``DepthMetric`` keeps MetricLogger's running means on the device and
reads them back once.

Classification evaluation (``evaluate()`` of run_finetuning_cls.py:580-613: ``nn.CrossEntropyLoss``, ``accuracy``'s topk sort and three
``.item()`` read-backs per batch): ``cls_accuracy`` and ``ClsMetric`` take the top-k correctness of a row from the rank of its target's
logit, counted in the pass that computes the log-sum-exp (csrc/clseval.hip, two launches), keep MetricLogger's totals in one f64 device
buffer and read it back once.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .criterion import _image_fused_ok, _refuse_under_capture, _seg_handle


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


# ------------------------------------------------------------------------------------------
# NYU depth metrics (run_finetuning_depth.py:86-117)
# ------------------------------------------------------------------------------------------
NYU_MEAN, NYU_STD = 2070.7764, 777.5723          # utils/data_constants.py:29-30
DEPTH_METRIC_KEYS = ('rmse', 'rel', 'srel', 'log10', 'delta_1', 'delta_2', 'delta_3')


def _depth_fused_ok(h, pred, target, mask_valid) -> bool:
    if h is None or h.K != 1 or not torch.is_tensor(target):
        return False
    dev = h.logits.device
    if target.dtype != torch.float32 or tuple(target.shape) != tuple(pred.shape) or target.device != dev:
        return False
    return mask_valid is None or (torch.is_tensor(mask_valid) and mask_valid.dtype == torch.bool and mask_valid.device == dev
                                  and tuple(mask_valid.shape) == tuple(pred.shape))


def _depth_metrics_eager(pred, target, mask_valid, mean, std) -> torch.Tensor:
    """the seven values on the image itself as one f32 [7] tensor: sums over torch.where instead of boolean indexing, so nothing is
    read back to the host"""
    p, t = pred * std + mean, target * std + mean
    if mask_valid is None:
        valid = torch.ones_like(p, dtype=torch.bool)
    else:
        valid = mask_valid.bool() if mask_valid.shape[1] == p.shape[1] else mask_valid.bool().repeat_interleave(p.shape[1], 1)
    n = valid.sum()
    tc, pc = t.clamp_min(1e-6), p.clamp_min(1e-6)
    over = lambda v: torch.where(valid, v, torch.zeros((), dtype=v.dtype, device=v.device)).sum() / n
    d = (p - t).abs()
    r = torch.maximum(p / tc, t / pc)
    lg = pc.log() - tc.log()
    return torch.stack([over(d * d).sqrt(), over(d / tc), over(d * d / tc), over(lg * lg).sqrt()]
                       + [over((r < th).to(p.dtype)) for th in (1.25, 1.25 ** 2, 1.25 ** 3)])


@torch.no_grad()
def _depth_values(pred, target, mask_valid, mean, std, acc=None) -> torch.Tensor:
    _refuse_under_capture(pred, 'depth_metrics')
    h = _seg_handle(pred)
    if _depth_fused_ok(h, pred, target, mask_valid):
        mask = None if mask_valid is None else mask_valid.contiguous()
        return ops.depth_metrics(h.logits, h.ld, target.contiguous(), mask, mean, std, h.B, h.h, h.w, h.H, h.W, h.mode, acc=acc)
    if _image_fused_ok(pred, target, mask_valid, channels=1):
        mask = None if mask_valid is None else mask_valid.contiguous()       # the DPT head's own one-channel prediction
        return ops.depth_metrics_img(pred, target.contiguous(), mask, mean, std, acc=acc)
    out = _depth_metrics_eager(pred, target, mask_valid, mean, std).float()
    if acc is not None:
        acc[:7] += out
        acc[7] += 1
    return out


def depth_metrics(pred: torch.Tensor, target: torch.Tensor, mask_valid=None, mean: float = NYU_MEAN, std: float = NYU_STD):
    """``masked_nyu_metrics(preds, target, mask_valid)``: rmse, rel, srel, log10 (the natural logarithm, as the reference's key),
    delta_1, delta_2, delta_3 of pred std + mean against target std + mean over the valid pixels, as a dict of 0-dim device tensors;
    nothing is read back.  On an unmodified one-channel prediction of the ConvNeXt head with an f32 target and a torch.bool mask of
    its shape the values come from one pass over the head's low-resolution map (csrc/regloss.hip) and the image is not written.
    On the DPT head's own one-channel f32 prediction (functions.ImageMark) under the same conditions they come from one pass over
    the image (mmae_depth_metrics_img); every other prediction -- more channels, ``y * 1``, modified in place -- is evaluated by
    _depth_metrics_eager.  A ConvNeXt-head prediction inside a graph capture raises RuntimeError (criterion._refuse_under_capture)."""
    out = _depth_values(pred, target, mask_valid, mean, std)
    return {k: out[i] for i, k in enumerate(DEPTH_METRIC_KEYS)}


class DepthMetric:
    """What ``MetricLogger`` keeps for the depth loop, on the device: the mean over the update() calls of each per-batch metric
    (``global_avg = total / count`` -- not a sum pooled over pixels) and of any extra 0-dim device tensor such as the loss.

    update(pred, target, mask_valid, **scalars)   adds the batch's seven values and the scalars to the totals; no read-back
    sync()                                        one all_reduce of totals and count when torch.distributed is initialised
    compute()                                     {name: total / count} as Python floats -- the only read-back"""

    def __init__(self, device=None, mean: float = NYU_MEAN, std: float = NYU_STD):
        self.mean, self.std = float(mean), float(std)
        self.names = list(DEPTH_METRIC_KEYS)
        self.acc = None if device is None else torch.zeros((8,), device=device, dtype=torch.float32)      # seven totals, count
        self.extra = None                                                                                 # the scalars' totals

    def reset(self) -> None:
        if self.acc is not None:
            self.acc.zero_()
        self.extra, self.names = None, list(DEPTH_METRIC_KEYS)

    @torch.no_grad()
    def update(self, pred: torch.Tensor, target: torch.Tensor, mask_valid=None, **scalars) -> None:
        if self.acc is None:
            self.acc = torch.zeros((8,), device=target.device, dtype=torch.float32)
        if self.extra is None:
            self.names = list(DEPTH_METRIC_KEYS) + list(scalars)
            self.extra = torch.zeros((len(scalars),), device=self.acc.device, dtype=torch.float32)
        if list(scalars) != self.names[7:]:
            raise ValueError(f'DepthMetric.update: scalars {list(scalars)} differ from the first call\'s {self.names[7:]}')
        _depth_values(pred, target, mask_valid, self.mean, self.std, acc=self.acc)
        if scalars:
            self.extra += torch.stack([v.detach().float().reshape(()) for v in scalars.values()])

    def sync(self) -> None:
        if self.acc is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            buf = self.acc if self.extra is None or not self.extra.numel() else torch.cat([self.acc, self.extra])
            torch.distributed.all_reduce(buf)
            if buf is not self.acc:
                self.acc.copy_(buf[:8])
                self.extra.copy_(buf[8:])

    def compute(self):
        tot = self.acc if self.extra is None else torch.cat([self.acc, self.extra])
        v = tot.double().cpu()
        vals = torch.cat([v[:7], v[8:]]) / v[7]
        return {k: float(x) for k, x in zip(self.names, vals)}


# ------------------------------------------------------------------------------------------
# Classification evaluation (run_finetuning_cls.py:580-613, utils/metrics.py:31-38)
# ------------------------------------------------------------------------------------------
def _topk_arg(topk):
    ks = tuple(int(k) for k in topk)
    if not ks or min(ks) < 1:
        raise ValueError(f'topk must hold at least one threshold, each >= 1, got {tuple(topk)}')
    return ks


def _cls_args(output, target):
    if not (torch.is_tensor(output) and output.dim() == 2 and torch.is_tensor(target) and target.dim() == 1
            and target.shape[0] == output.shape[0]):
        raise ValueError('classification metrics take (B, K) logits and B class indices')
    if target.dtype.is_floating_point or target.dtype == torch.bool:
        raise ValueError(f'classification metrics take integer class indices, got {target.dtype}')


def _cls_fused_ok(output, target, ks) -> bool:
    B, K = output.shape
    if not (output.dtype in (torch.float32, torch.bfloat16) and ops._device_ok(output) and B > 0 and K > 0):
        return False
    if not ((K == 1 or output.stride(1) == 1) and (B == 1 or output.stride(0) >= K)):
        return False
    return target.dtype == torch.int64 and target.device == output.device and len(ks) <= ops.CLS_TOPK_MAX


def _cls_rank_eager(z, target):
    """(valid [B], z_t [B], rank int64 [B]) by the kernel's rule: rank = #{k: z_k > z_t} + #{k < t: z_k == z_t} through comparisons
    (no topk: its order among equal logits is unspecified), K for a target outside [0, K)"""
    K = z.shape[1]
    t = target.long()
    valid = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1)
    zt = z.gather(1, tc[:, None])
    idx = torch.arange(K, device=z.device)
    rank = (z > zt).sum(1) + ((z == zt) & (idx[None, :] < tc[:, None])).sum(1)
    return valid, zt.squeeze(1), torch.where(valid, rank, torch.full_like(rank, K))


def _cls_eval_eager(output, target, ks) -> torch.Tensor:
    """mmae_cls_eval's out (f32 [1 + len(ks)] = loss, percentages) restated in torch without a sort or a read-back: the loss is the
    mean of lse - z_t over the valid targets (0 without one), summed in double; the percentages are accuracy()'s f32 operations"""
    B, K = output.shape
    z = output if output.dtype in (torch.float32, torch.float64) else output.float()
    valid, zt, rank = _cls_rank_eager(z, target)
    nll = torch.where(valid, torch.logsumexp(z, 1) - zt, torch.zeros_like(zt))
    nv = valid.sum()
    loss = torch.where(nv > 0, nll.double().sum() / nv.clamp_min(1), torch.zeros((), dtype=torch.float64, device=z.device)).float()
    accs = [(rank < min(k, K)).float().sum(0) * 100. / B for k in ks]
    return torch.stack([loss] + accs)


@torch.no_grad()
def _cls_values(output, target, ks, acc=None) -> torch.Tensor:
    _cls_args(output, target)
    output = output.detach()
    B, K = output.shape
    if _cls_fused_ok(output, target, ks) and (acc is None or acc.device == output.device):
        ldx = output.stride(0) if B > 1 else K
        return ops.cls_eval(output, ldx, B, K, target.contiguous(), ks, acc=acc)[3]
    out = _cls_eval_eager(output, target, ks)
    if acc is not None:
        acc[0] += out[0].double()
        acc[1] += 1
        acc[2] += B
        acc[3:] += out[1:].double() * B
    return out


def cls_accuracy(output: torch.Tensor, target: torch.Tensor, topk=(1,)):
    """``utils.metrics.accuracy(output, target, topk)``: the percentage of rows whose target is among the k largest logits, as a list of
    0-dim f32 device tensors; nothing is read back.  A row is correct at k iff fewer than min(k, K) logits rank before its target's,
    equal logits ranking by index (the lower first) -- where the reference's topk leaves ties unspecified.  A target outside [0, K)
    is incorrect at every k and B stays the denominator.  2-D f32 / bf16 GPU logits with unit inner stride, an int64 target and at
    most four thresholds run in two launches (csrc/clseval.hip, beside the cross-entropy); anything else takes _cls_eval_eager."""
    ks = _topk_arg(topk)
    out = _cls_values(output, target, ks)
    return [out[1 + j] for j in range(len(ks))]


class ClsMetric:
    """What ``MetricLogger`` keeps in ``evaluate()`` of run_finetuning_cls.py (:600-607), on the device: the plain cross-entropy of
    every batch (``update(loss=loss.item())``: total += loss, count += 1) and the top-k accuracies weighted by the batch size
    (``meters['acc1'].update(acc1.item(), n=batch_size)``) in one f64 buffer [3 + len(topk)] = loss total, batches, samples, acc totals.

    update(output, target)   adds the batch; two launches on the fused path, no read-back on either path
    sync()                   one all_reduce of the buffer when torch.distributed is initialised
    compute()                {'loss': ..., 'acc1': ..., 'acc5': ...} (keys f'acc{k}') as Python floats, MetricLogger's global_avg --
                             the only read-back
    A target outside [0, K) (ignore_index -100 included) is left out of the loss and counts as incorrect; a batch without a valid
    target has loss 0 (torch: NaN) and still counts as a batch."""

    def __init__(self, topk=(1, 5), device=None):
        self.topk = _topk_arg(topk)
        self.acc = None if device is None else torch.zeros((3 + len(self.topk),), device=device, dtype=torch.float64)

    def reset(self) -> None:
        if self.acc is not None:
            self.acc.zero_()

    @torch.no_grad()
    def update(self, output: torch.Tensor, target: torch.Tensor) -> None:
        if self.acc is None:
            self.acc = torch.zeros((3 + len(self.topk),), device=target.device, dtype=torch.float64)
        _cls_values(output, target, self.topk, acc=self.acc)

    def sync(self) -> None:
        if self.acc is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(self.acc)

    def compute(self):
        v = self.acc.cpu()
        res = {'loss': float(v[0] / v[1])}
        res.update({f'acc{k}': float(v[3 + j] / v[2]) for j, k in enumerate(self.topk)})
        return res


def ratios(hist: np.ndarray):
    """eval_metrics' mIoU branch (utils/semseg_metrics.py:216-222) on the [4, K] histograms: overall accuracy, per-class accuracy,
    per-class IoU; 0 / 0 is NaN as there."""
    inter, union, _, label = (hist[i].astype(np.int64) for i in range(4))
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter.sum() / label.sum(), inter / label, inter / union
