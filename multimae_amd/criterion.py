"""Masked losses (mirror of the reference's ``multimae/criterion.py`` API) on HIP kernels.

Reference: MaskedCrossEntropyLoss criterion.py:23-57, MaskedMSELoss :60-114, MaskedL1Loss
:117-171.  Semantics reproduced: per-sample masked mean of the
channel-mean error, then the mean over samples that have at least one masked token (nanmean);
norm_pix uses the unbiased patch variance with eps 1e-6 inside the sqrt.

Deliberate deviation (documented in DESIGN.md): when NO token of the batch is masked the
reference returns ``torch.tensor(0)`` (int64, after a host sync); this engine returns a float32
zero with zero gradient and never synchronises.  SegCrossEntropyLoss does the same for a batch without
a valid pixel, where ``nn.CrossEntropyLoss`` returns NaN.
"""
from __future__ import annotations

import torch
from torch import nn

from .functions import MaskedCEFn, MaskedCEPatFn, MaskedPixelLossFn, MaskedPixelLossPatFn, SegCEFn, SoftCEFn
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
