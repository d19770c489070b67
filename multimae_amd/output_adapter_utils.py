"""Building blocks of the DPT head (mirror of the reference's ``multimae/output_adapter_utils.py``, the RefineNet part: lines
60-290): ``ResidualConvUnit_custom``, ``FeatureFusionBlock_custom``, ``make_fusion_block``, ``make_scratch``, ``Interpolate``, plus a
plain ``Conv3x3`` module.  Same constructor arguments, parameter names, shapes and registration order as the reference -- the
parameter holders are real ``nn.Conv2d`` modules, so a seeded construction draws the same numbers and a reference DPT checkpoint's
``scratch.*`` sub-dict loads with ``load_state_dict`` -- but every forward and backward is a hand-written HIP kernel sequence
(functions.Conv3x3Fn, ResidualConvUnitFn, FusionBlockFn on csrc/conv3x3.hip and the engine's GEMMs): a dense 3 x 3 convolution is an
im2col gather + mmae_gemm, the x2 upsample an NHWC kernel of its own.

Modules take and return (B, C, H, W)-shaped f32 GPU tensors.  Inside, a map is channels-last [B][H][W][C]: an input that is
contiguous in ``torch.channels_last`` is used in place, anything else costs one conversion on entry, and outputs are channels-last
strided, so chained blocks never transpose.  Each residual unit and each fusion block is ONE autograd node.

Not built (NotImplementedError naming the argument): ``bn=True``, ``groups > 1``, ``expand=True``, ``deconv=True`` -- nothing
``make_fusion_block`` or the DPT head asks for.  bf16 mode needs channel counts that are multiples of 8 (ValueError); fp32 mode
takes any.  The blocks run uncaptured only: they are untested under graph capture.

The ConvNeXt block of the same reference file lives in output_adapters.py (ConvNeXtBlock) with the head that uses it.
"""
from __future__ import annotations

import torch
from torch import nn

from .functions import Conv3x3Fn, FusionBlockFn, ResidualConvUnitFn, Upsample2xFn
from .multimae_utils import _cfg

# Bytes of gathered rows (the im2col buffer, and the dY x W rows of the data gradient) one chunk of samples may take: a convolution
# runs over the batch in chunks of as many samples as fit (one at least), the last chunk possibly short.  One 56 x 56 x 256
# convolution gathers 14 MB per sample in bf16.
COL_WORKSPACE_BYTES = [256 << 20]


def set_col_workspace_bytes(nbytes: int) -> int:
    """Set the cap on the gathered-rows buffer (returns the previous value).  A tiny cap forces several chunks at a tiny shape."""
    old = COL_WORKSPACE_BYTES[0]
    if int(nbytes) < 1:
        raise ValueError('the gathered-rows cap must be at least one byte')
    COL_WORKSPACE_BYTES[0] = int(nbytes)
    return old


def _conv_cfg(module: nn.Module, **kw):
    return _cfg(module, cap=COL_WORKSPACE_BYTES[0], **kw)


def _not_built(cls: str, **args) -> None:
    for name, bad in args.items():
        if bad:
            raise NotImplementedError(f'{cls}: {name} is not built in multimae_amd (the DPT head never asks for it)')


class Conv3x3(nn.Conv2d):
    """nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1 | 2, padding=1, bias=bias) as a parameter holder (same names,
    shapes and seeded values); forward = im2col gather + GEMM (functions.Conv3x3Fn)."""

    def __init__(self, in_channels: int, out_channels: int, stride: int = 1, bias: bool = True, groups: int = 1):
        _not_built('Conv3x3', **{'groups > 1': groups != 1})
        if stride not in (1, 2):
            raise NotImplementedError(f'Conv3x3: stride = {stride} is not built in multimae_amd (1 or 2)')
        super().__init__(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=bias, groups=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return Conv3x3Fn.apply(_conv_cfg(self, stride=self.stride[0]), x, self.weight, self.bias)


class ResidualConvUnit_custom(nn.Module):
    """Residual convolution module (output_adapter_utils.py:60-123): conv2(act(conv1(act(x)))) + x with two biased 3 x 3
    convolutions.  `activation` must be a ReLU (the gathers apply it on the fly; the input is not modified, as with nn.ReLU(False))."""

    def __init__(self, features, activation, bn):
        super().__init__()
        _not_built('ResidualConvUnit_custom', **{'bn=True': bn})
        if not isinstance(activation, nn.ReLU):
            raise NotImplementedError(f'ResidualConvUnit_custom: activation {type(activation).__name__} is not built in multimae_amd (nn.ReLU)')
        self.bn = bn
        self.groups = 1
        self.conv1 = Conv3x3(features, features, stride=1, bias=True)
        self.conv2 = Conv3x3(features, features, stride=1, bias=True)
        self.activation = activation

    def _params(self):
        return [self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ResidualConvUnitFn.apply(_conv_cfg(self), x, *self._params())


class FeatureFusionBlock_custom(nn.Module):
    """Feature fusion block (output_adapter_utils.py:184-247): xs[0] (+ resConfUnit1(xs[1])) -> resConfUnit2 -> bilinear x2 with
    align_corners=True -> the 1 x 1 out_conv.  Parameters in the reference's order: out_conv, resConfUnit1, resConfUnit2."""

    def __init__(self, features, activation, deconv=False, bn=False, expand=False, align_corners=True):
        super().__init__()
        _not_built('FeatureFusionBlock_custom', **{'deconv=True': deconv, 'bn=True': bn, 'expand=True': expand,
                                                   'align_corners=False': not align_corners})
        self.deconv = deconv
        self.align_corners = align_corners
        self.groups = 1
        self.expand = expand
        self.out_conv = nn.Conv2d(features, features, kernel_size=1, stride=1, padding=0, bias=True, groups=1)
        self.resConfUnit1 = ResidualConvUnit_custom(features, activation, bn)
        self.resConfUnit2 = ResidualConvUnit_custom(features, activation, bn)

    def _params(self):
        return [self.out_conv.weight, self.out_conv.bias, *self.resConfUnit1._params(), *self.resConfUnit2._params()]

    def forward(self, *xs: torch.Tensor) -> torch.Tensor:
        if len(xs) not in (1, 2):
            raise ValueError(f'FeatureFusionBlock_custom takes one or two inputs, got {len(xs)}')
        if len(xs) == 2 and xs[0].shape != xs[1].shape:
            raise ValueError(f'FeatureFusionBlock_custom: the two inputs differ in shape ({tuple(xs[0].shape)}, {tuple(xs[1].shape)})')
        return FusionBlockFn.apply(_conv_cfg(self), xs[0], xs[1] if len(xs) == 2 else None, *self._params())


def make_fusion_block(features, use_bn):
    """the fusion block as the DPT head builds it (output_adapter_utils.py:249-257)"""
    return FeatureFusionBlock_custom(features, nn.ReLU(False), deconv=False, bn=use_bn, expand=False, align_corners=True)


def make_scratch(in_shape, out_shape, groups=1, expand=False):
    """scratch.layer{1..4}_rn: four bias-free 3 x 3 convolutions in_shape[i] -> out_shape, also listed in scratch.layer_rn
    (output_adapter_utils.py:125-182; both sets of keys appear in a state_dict, as in the reference)."""
    _not_built('make_scratch', **{'groups > 1': groups != 1, 'expand=True': expand})
    scratch = nn.Module()
    scratch.layer1_rn = Conv3x3(in_shape[0], out_shape, stride=1, bias=False)
    scratch.layer2_rn = Conv3x3(in_shape[1], out_shape, stride=1, bias=False)
    scratch.layer3_rn = Conv3x3(in_shape[2], out_shape, stride=1, bias=False)
    scratch.layer4_rn = Conv3x3(in_shape[3], out_shape, stride=1, bias=False)
    scratch.layer_rn = nn.ModuleList([scratch.layer1_rn, scratch.layer2_rn, scratch.layer3_rn, scratch.layer4_rn])
    return scratch


class Interpolate(nn.Module):
    """Interpolation module (output_adapter_utils.py:259-290).  Built: what the DPT heads use, scale_factor=2, mode='bilinear',
    align_corners=True."""

    def __init__(self, scale_factor, mode, align_corners=False):
        super().__init__()
        _not_built('Interpolate', **{f'scale_factor={scale_factor}': scale_factor != 2, f'mode={mode!r}': mode != 'bilinear',
                                     'align_corners=False': not align_corners})
        self.scale_factor = scale_factor
        self.mode = mode
        self.align_corners = align_corners

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return Upsample2xFn.apply(x)
