"""Masked losses (mirror of the reference's ``multimae/criterion.py`` API) on HIP kernels.

Reference: MaskedCrossEntropyLoss criterion.py:23-57, MaskedMSELoss :60-114, MaskedL1Loss
:117-171.  Semantics reproduced: per-sample masked mean of the
channel-mean error, then the mean over samples that have at least one masked token (nanmean);
norm_pix uses the unbiased patch variance with eps 1e-6 inside the sqrt.

Deliberate deviation (documented in DESIGN.md): when NO token of the batch is masked the
reference returns ``torch.tensor(0)`` (int64, after a host sync); this engine returns a float32
zero with zero gradient and never synchronises.  SegCrossEntropyLoss does the same for a batch without
a valid pixel, where ``nn.CrossEntropyLoss`` returns NaN, and masked_l1_loss / masked_mse_loss / masked_berhu_loss for a mask without a
valid element on their fused path, where the reference divides 0 by 0.
"""
from __future__ import annotations

import torch
from torch import nn

from . import engine, ops
from .functions import MaskedCEFn, MaskedCEPatFn, MaskedPixelLossFn, MaskedPixelLossPatFn, RegImageLossFn, RegLossFn, SegCEFn, SoftCEFn
from .lazy import materialize as _materialize


def _pat_handle(x: torch.Tensor, patch: int, ce: bool = False):
    """The adapter's patch rows behind prediction x (functions.PatHandle), if x is exactly what an output adapter returned
    (``preds[task].float()`` of an f32 tensor is the same object) and the loss's patch grid is the adapter's.  Anything else --
    a modified prediction, a copy made any other way than ``clone()`` -- takes the image-domain loss (same value, gradient rows
    through the f32 image instead of the adapter's activation dtype).  The CLONES torch DDP's output sink returns with
    find_unused_parameters=True keep the side channel (lazy.LazyPrediction.clone), so the reference loop under DDP runs the same
    loss kernels as the native loop (tests/test_reference_loop_gpu.py)."""
    h = getattr(x, '_mmae_pat', None)
    if h is None or not h.matches(x, patch) or not getattr(x, 'unmodified', True):
        return None
    if ce and (patch * patch > 64 or (patch * patch) & (patch * patch - 1)):
        return None
    return h


def _ones_mask(x: torch.Tensor, scale: int) -> torch.Tensor:
    H, W = x.shape[-2:]
    return torch.ones((x.shape[0], (H // scale) * (W // scale)), device=x.device, dtype=torch.int64)


class MaskedCrossEntropyLoss(nn.Module):
    """Cross-entropy loss with masking (patch_size, stride, label_smoothing)."""

    def __init__(self, patch_size: int = 16, stride: int = 1, label_smoothing: float = 0.0):
        super().__init__()
        self.patch_size = patch_size
        self.stride = stride
        self.scale_factor = patch_size // stride
        self.label_smoothing = label_smoothing

    def forward(self, input, target, mask=None):
        if mask is None:
            mask = _ones_mask(input, self.scale_factor)      # plain mean == masked mean with an all-ones mask
        h = _pat_handle(input, self.scale_factor, ce=True)
        if h is not None:
            return MaskedCEPatFn.apply(h.token, h, target, mask, self.scale_factor, float(self.label_smoothing))
        _materialize(input)                                 # image-domain loss: the kernels read the image itself
        return MaskedCEFn.apply(input, target, mask, self.scale_factor, float(self.label_smoothing))


class _MaskedPixelLoss(nn.Module):
    kind = 0

    def __init__(self, patch_size: int = 16, stride: int = 1, norm_pix=False):
        super().__init__()
        self.patch_size = patch_size
        self.stride = stride
        self.scale_factor = patch_size // stride
        self.norm_pix = norm_pix

    def forward(self, input, target, mask=None):
        if mask is None:
            mask = _ones_mask(input, self.scale_factor)
        h = _pat_handle(input, self.scale_factor)
        if h is not None:
            return MaskedPixelLossPatFn.apply(h.token, h, target, mask, self.kind, bool(self.norm_pix), self.scale_factor)
        _materialize(input)
        return MaskedPixelLossFn.apply(input, target, mask, self.kind, bool(self.norm_pix), self.scale_factor)


class MaskedMSELoss(_MaskedPixelLoss):
    """MSE loss with masking (patch_size, stride, norm_pix)."""
    kind = 0


class MaskedL1Loss(_MaskedPixelLoss):
    """L1 loss with masking (patch_size, stride, norm_pix)."""
    kind = 1


def _seg_handle(x: torch.Tensor):
    """The ConvNeXt head's low-resolution logits behind prediction x (functions.SegHandle), if x is exactly what the head returned
    (or a ``clone()`` of it) and has not been modified; None otherwise."""
    h = getattr(x, '_mmae_seg', None)
    if h is None or not h.matches(x) or not getattr(x, 'unmodified', True):
        return None
    return h


class SegCrossEntropyLoss(nn.CrossEntropyLoss):
    """``nn.CrossEntropyLoss`` (same constructor) for the semantic-segmentation fine-tuning loop (run_finetuning_semseg.py:483).  On a
    prediction of the ConvNeXt head with an integer target map of the image's size, no class weights, no label smoothing and
    reduction='mean', the loss and its gradient are computed from the head's low-resolution logits (functions.SegCEFn): the
    (B, K, H, W) image is neither written nor read.  Anything else is ``nn.CrossEntropyLoss`` on the image itself.  Deviations on
    the fused path: a target outside [0, K) other than ignore_index counts as ignored (torch: device assert), and a batch without
    a valid pixel gives 0 with a zero gradient (torch: NaN)."""

    def forward(self, input, target):
        h = _seg_handle(input)
        if (h is not None and self.weight is None and self.label_smoothing == 0 and self.reduction == 'mean'
                and not target.is_floating_point() and not target.is_complex() and target.dtype != torch.bool
                and tuple(target.shape) == (h.B, h.H, h.W) and target.device == h.logits.device):
            return SegCEFn.apply(h.token, h, target, int(self.ignore_index))
        return super().forward(input, target)


# ------------------------------------------------------------------------------------------
# Dense regression fine-tuning (run_finetuning_depth.py:49-84, also used by run_finetuning_taskonomy.py)
# ------------------------------------------------------------------------------------------
def _reg_fused_ok(h, preds: torch.Tensor, target, mask_valid) -> bool:
    """The conditions of the fused regression path: the head's own prediction with at most ops.REG_MAX_K channels, an f32 target of
    its shape on its device, and no mask or a torch.bool mask [B, 1 or K, H, W] on that device."""
    if h is None or h.K > ops.REG_MAX_K or not torch.is_tensor(target):
        return False
    dev = h.logits.device
    if target.dtype != torch.float32 or tuple(target.shape) != tuple(preds.shape) or target.device != dev:
        return False
    if mask_valid is None:
        return True
    return (torch.is_tensor(mask_valid) and mask_valid.dtype == torch.bool and mask_valid.device == dev and mask_valid.dim() == 4
            and mask_valid.shape[1] in (1, h.K) and (mask_valid.shape[0],) + tuple(mask_valid.shape[2:]) == (h.B, h.H, h.W))


def _valid_like(preds: torch.Tensor, mask_valid):
    """the mask in the prediction's shape (one channel is repeated over the channels, as the reference's repeat_interleave) as
    torch.bool (non-zero = valid); None = all"""
    if mask_valid is None:
        return None
    if mask_valid.dtype != torch.bool:
        mask_valid = mask_valid.bool()
    if mask_valid.shape[1] != preds.shape[1]:
        mask_valid = mask_valid.repeat_interleave(preds.shape[1], 1)
    return mask_valid


def _reg_loss_eager(preds: torch.Tensor, target: torch.Tensor, mask_valid, kind: str) -> torch.Tensor:
    """The three formulas on the image itself, for everything the fused path does not take.  sum(e(d)) / count with d = preds - target
    set to 0 where the mask is false: e = |d| (l1), d^2 (mse), or berHu's |d| below c = max(0.2 max|d|, 1e-5) and (d^2 + c^2) / (2 c) from
    c on, c a constant of the graph.  Written with torch.where, so nothing is read back to the host; an empty mask gives 0 / 0 = NaN, as
    the reference does."""
    valid = _valid_like(preds, mask_valid)
    d = preds - target                                       # reads -- and so writes -- a lazy prediction
    if valid is None:
        count = d.numel()
    else:
        d = torch.where(valid, d, torch.zeros((), dtype=d.dtype, device=d.device))
        count = valid.sum()
    a = d.abs()
    if kind == 'l1':
        e = a
    elif kind == 'mse':
        e = d * d
    else:
        with torch.no_grad():
            c = (a.max() * 0.2).clamp_min(1e-5)
        e = torch.where(a < c, a, (d * d + c * c) / 2. / c)
    return e.sum() / count


def _refuse_under_capture(pred, what: str) -> None:
    """Capturing a step of the ConvNeXt head with a regression loss or the depth metrics -- in graph.StepGraph or a plain
    torch.cuda.graph -- is unsupported and untested: the one attempt ended in a fault of the runtime when the capture ended, and its
    cause is not known.  Refused for every prediction that carries the head's side channel, whichever path it would take."""
    if getattr(pred, '_mmae_seg', None) is None:
        return
    if engine.capturing() is not None or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        raise RuntimeError(f'{what}: capturing a ConvNeXt-head + regression-loss / depth-metrics step in a graph is unsupported and '
                           'untested; run this step uncaptured')


def _image_fused_ok(preds, target, mask_valid, channels=None) -> bool:
    """The conditions of the fused path on a prediction that is the image itself: the DPT head's own output, still carrying its mark
    (functions.ImageMark: same shape, not modified in place since) with engine.patch_domain_loss() on, f32 and contiguous (with
    `channels` channels when given); an f32 target of its shape on its device; no mask or a torch.bool mask [B, 1 or K, H, W] on that
    device; no graph capture running (the head runs uncaptured only: anything met inside a capture takes the eager path)."""
    mark = getattr(preds, '_mmae_img', None) if torch.is_tensor(preds) else None
    if mark is None or not engine.patch_domain_loss() or not mark.matches(preds):
        return False
    if preds.dim() != 4 or preds.dtype != torch.float32 or not preds.is_contiguous() or (channels is not None and preds.shape[1] != channels):
        return False
    if engine.capturing() is not None or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        return False
    dev = preds.device
    if not torch.is_tensor(target) or target.dtype != torch.float32 or tuple(target.shape) != tuple(preds.shape) or target.device != dev:
        return False
    if mask_valid is None:
        return True
    B, K, H, W = preds.shape
    return (torch.is_tensor(mask_valid) and mask_valid.dtype == torch.bool and mask_valid.device == dev and mask_valid.dim() == 4
            and mask_valid.shape[1] in (1, K) and (mask_valid.shape[0],) + tuple(mask_valid.shape[2:]) == (B, H, W))


def _reg_loss(preds, target, mask_valid, kind: str) -> torch.Tensor:
    _refuse_under_capture(preds, f'masked_{kind}_loss')
    h = _seg_handle(preds)
    if _reg_fused_ok(h, preds, target, mask_valid):
        return RegLossFn.apply(h.token, h, target, mask_valid, kind)
    if _image_fused_ok(preds, target, mask_valid):
        return RegImageLossFn.apply(preds, target, mask_valid, kind)
    return _reg_loss_eager(preds, target, mask_valid, kind)


def masked_l1_loss(preds, target, mask_valid=None):
    """``masked_l1_loss`` of run_finetuning_depth.py:59-66: mean |preds - target| over the valid elements.  On an unmodified f32
    prediction of the ConvNeXt head (``preds[task].float()`` is the same object) with an f32 target of its shape and a torch.bool mask
    of 1 or K channels, the loss and its gradient come from the head's low-resolution map (functions.RegLossFn) and the image is
    neither written nor read.  On the DPT head's own f32 prediction (it carries functions.ImageMark; ``preds[task].float()`` is the
    same object) under the same conditions on target and mask, the loss and its gradient come from the fused kernels on the image
    (functions.RegImageLossFn, any number of channels).  On both fused paths a mask without a valid element gives 0 with a zero
    gradient (the reference: NaN).  Anything else -- ``y * 1``, ``y.clone()`` of a DPT prediction, a prediction modified in place,
    more than 16 channels of the ConvNeXt head, another dtype, a non-bool mask, engine.set_patch_domain_loss(False), a CPU tensor --
    is evaluated on the image by _reg_loss_eager.  Not inside a graph capture: a ConvNeXt-head prediction met while a
    graph.StepGraph or torch.cuda.graph capture runs raises RuntimeError (_refuse_under_capture); a DPT prediction takes the eager
    path there."""
    return _reg_loss(preds, target, mask_valid, 'l1')


def masked_mse_loss(preds, target, mask_valid=None):
    """``masked_mse_loss`` of run_finetuning_depth.py:49-56: mean (preds - target)^2 over the valid elements; paths as masked_l1_loss."""
    return _reg_loss(preds, target, mask_valid, 'mse')


def masked_berhu_loss(preds, target, mask_valid=None):
    """``masked_berhu_loss`` of run_finetuning_depth.py:69-84: |d| below c = max(0.2 max|d|, 1e-5), (d^2 + c^2) / (2 c) from c on, mean
    over the valid elements; c is a constant of the graph and never leaves the device (the reference takes a Python ``max()`` of it and
    indexes with boolean masks: three host synchronisations).  Paths as masked_l1_loss."""
    return _reg_loss(preds, target, mask_valid, 'berhu')


def _cls_logits(x) -> torch.Tensor:
    if not (torch.is_tensor(x) and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16)):
        raise ValueError('classification loss: the input is a (B, K) tensor of float32 or bfloat16 logits')
    return x


class SoftTargetCrossEntropy(nn.Module):
    """``utils.SoftTargetCrossEntropy`` (utils/cross_entropy.py:36-43) for the classification fine-tuning loop: mean over the batch of
    ``sum_k -target_k log_softmax(x)_k`` on logits (B, K) and a dense float32 target (B, K) -- what ``Mixup`` returns.  One autograd
    node (functions.SoftCEFn): the forward saves the rows' log-sum-exp, the backward recomputes the softmax from it."""

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        x = _cls_logits(x)
        if not (torch.is_tensor(target) and target.dtype == torch.float32 and tuple(target.shape) == tuple(x.shape)):
            raise ValueError(f'SoftTargetCrossEntropy: the target is a float32 tensor of the logits\' shape {tuple(x.shape)} '
                             '(class probabilities, as Mixup returns them)')
        return SoftCEFn.apply(x, target.to(x.device).contiguous(), None, 0.0)


class LabelSmoothingCrossEntropy(nn.Module):
    """``utils.LabelSmoothingCrossEntropy`` (utils/cross_entropy.py:17-33): ``(1 - smoothing) nll + smoothing mean_k(-log_softmax)`` on
    logits (B, K) and int64 class indices (B,), mean over the batch.  Same kernels as SoftTargetCrossEntropy, the target row
    ``smoothing / K + (1 - smoothing) [k == label]`` formed on the fly.  A label outside [0, K) contributes the smoothing term only
    (torch: device assert in the gather)."""

    def __init__(self, smoothing: float = 0.1):
        super().__init__()
        if not smoothing < 1.0:
            raise ValueError('LabelSmoothingCrossEntropy: smoothing must be below 1')
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        x = _cls_logits(x)
        if not (torch.is_tensor(target) and target.dtype == torch.int64 and tuple(target.shape) == (x.shape[0],)):
            raise ValueError(f'LabelSmoothingCrossEntropy: the target is an int64 tensor of {x.shape[0]} class indices')
        return SoftCEFn.apply(x, None, target.to(x.device).contiguous(), float(self.smoothing))
