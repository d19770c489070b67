"""RandAugment for the classification fine-tuning loop (mirror of the reference's ``utils/auto_augment.py`` ``rand_augment_transform``
/ ``RandAugment`` / ``AugmentOp``) with the image operations on HIP kernels, bit for bit what PIL computes.

Reference: rand_augment_transform utils/auto_augment.py:639-694, RandAugment.__call__ :630-636, AugmentOp.__call__ :341-356, the level
functions :183-260; in the reference it sits between the crop / flip and the tensor conversion of the training transform
(utils/transforms_factory.py:78-119).  Division of labour, as in ``random_erasing.py``:

  host    every random draw, in the reference's call order, sample 0 first: ``np.random.choice`` of the sample's layer ops, then per
          op ``random.random()`` against ``prob``, ``random.gauss`` / ``random.uniform`` for ``mstd``, the level function's
          ``random.random()`` (``_randomly_negate``) and, for a geometric op when the interpolation is a tuple, ``random.choice`` of
          it.  The level functions run in Python floats.  ``draw()`` packs the *results* -- op code, interpolation, integer argument,
          the enhancement factor as f32 bits, the six f64 affine coefficients as PIL builds them, the fill colour -- into the int32
          table of include/mmae.h ("RandAugment").  What PIL would return unchanged never reaches the device: an op skipped by
          ``prob``, posterize with 8 or more bits, a rotation by 0 mod 360 degrees.
  device  ``mmae_rand_augment_u8`` (``data_ops.rand_augment_u8``, ``staging.ClsStager(rand_augment=...)``) applies a table to a
          uint8 (B, 3, H, W) batch.

Contract: after the same ``random.seed`` / ``np.random.seed`` the table describes exactly what the reference's
``RandAugment.__call__`` does to B images one after the other, and both generators end where the reference leaves them.  This is the
reference run in ONE process over the batch; it says nothing about how a multi-worker DataLoader interleaves its workers' generators.

Not supported (``NotImplementedError``): AutoAugment policies, AugMix, the ``*Abs`` translations, interpolations other than
bilinear / bicubic, and rotations by a multiple of 90 degrees other than 0 (PIL transposes there; out of reach of any ``m`` <= 29).
"""
from __future__ import annotations

import math
import random
import re
import struct

import numpy as np

from . import _lib

MAX_LAYERS, ROW_WORDS = _lib.RA_MAX_LAYERS, _lib.RA_ROW
LAYER_WORDS = 16
# device op codes (include/mmae.h)
NOOP, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE = range(12)
BILINEAR, BICUBIC = 2, 3          # PIL's own codes
_LEVEL_DENOM = 10.

RAND_TRANSFORMS = ['AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast',
                   'Brightness', 'Sharpness', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel']
RAND_INCREASING_TRANSFORMS = ['AutoContrast', 'Equalize', 'Invert', 'Rotate', 'PosterizeIncreasing', 'SolarizeIncreasing', 'SolarizeAdd',
                              'ColorIncreasing', 'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing', 'ShearX',
                              'ShearY', 'TranslateXRel', 'TranslateYRel']
_RAND_CHOICE_WEIGHTS_0 = {'Rotate': 0.3, 'ShearX': 0.2, 'ShearY': 0.2, 'TranslateXRel': 0.1, 'TranslateYRel': 0.1, 'Color': .025,
                          'Sharpness': 0.025, 'AutoContrast': 0.025, 'Solarize': .005, 'SolarizeAdd': .005, 'Contrast': .005,
                          'Brightness': .005, 'Equalize': .005, 'Posterize': 0, 'Invert': 0}
_ENHANCE = {'Color': COLOR, 'Contrast': CONTRAST, 'Brightness': BRIGHTNESS, 'Sharpness': SHARPNESS}
_GEOMETRIC = ('Rotate', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
_INTERP_NAMES = {'bilinear': BILINEAR, 'bicubic': BICUBIC}


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def _interp_code(v):
    if isinstance(v, str):
        v = _INTERP_NAMES.get(v.lower(), v)
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and int(v) in (BILINEAR, BICUBIC):
        return int(v)
    raise NotImplementedError(f'RandAugment: interpolation {v!r} is not bilinear ({BILINEAR}) or bicubic ({BICUBIC})')


def rotate_matrix(degrees: float, W: int, H: int):
    """The six coefficients ``Image.rotate(degrees)`` hands to ``Image.transform(AFFINE)`` (utils/auto_augment.py:98-119 is the same
    formula); None where PIL returns a copy."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    if angle in (90, 180, 270):
        raise NotImplementedError(f'RandAugment: a rotation by {degrees} degrees is a transpose in PIL')
    cx, cy = W / 2.0, H / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    a, b, c, d, e, f = m
    m[2], m[5] = a * -cx + b * -cy + c, d * -cx + e * -cy + f
    m[2] += cx
    m[5] += cy
    return tuple(m)


def pack_layer(row: np.ndarray, op: int, interp: int = 0, iarg: int = 0, factor: float = 0.0, matrix=None) -> None:
    """Appends one layer to a sample's table row (include/mmae.h, "RandAugment")."""
    n = int(row[0])
    if n >= MAX_LAYERS:
        raise ValueError(f'RandAugment: a table row holds {MAX_LAYERS} layers')
    w = row[4 + LAYER_WORDS * n:4 + LAYER_WORDS * (n + 1)]
    w[0], w[1], w[2] = op, interp, iarg
    w[3:4] = np.array([factor], dtype=np.float32).view(np.int32)
    if matrix is not None:
        w[4:16] = np.frombuffer(struct.pack('<6d', *[float(v) for v in matrix]), dtype=np.int32)
    row[0] = n + 1


class RandAugment:
    """``rand_augment_transform(config_str, hparams)`` as a table generator: ``draw((B, 3, H, W))`` is one batch's table."""

    def __init__(self, config_str: str, hparams=None):
        if not isinstance(config_str, str) or not config_str.startswith('rand'):
            raise NotImplementedError(f'RandAugment: config {config_str!r}: only rand-* policies run on the device '
                                      f'(AutoAugment and AugMix are not built)')
        hparams = dict(hparams or {})
        magnitude, num_layers, weight_idx, names = _LEVEL_DENOM, 2, None, RAND_TRANSFORMS
        config = config_str.split('-')
        if config[0] != 'rand':
            raise ValueError(f'RandAugment: config {config_str!r} does not begin with the section "rand"')
        for c in config[1:]:
            cs = re.split(r'(\d.*)', c)
            if len(cs) < 2:
                continue
            key, val = cs[:2]
            if key == 'mstd':
                mstd = float(val)
                hparams.setdefault('magnitude_std', float('inf') if mstd > 100 else mstd)
            elif key == 'mmax':
                hparams.setdefault('magnitude_max', int(val))
            elif key == 'inc':
                if bool(val):                     # the reference tests the string: 'inc0' selects the increasing set as well
                    names = RAND_INCREASING_TRANSFORMS
            elif key == 'm':
                magnitude = int(val)
            elif key == 'n':
                num_layers = int(val)
            elif key == 'w':
                weight_idx = int(val)
            else:
                raise ValueError(f'RandAugment: unknown config section {c!r} in {config_str!r}')
        if num_layers > MAX_LAYERS:
            raise ValueError(f'RandAugment: n = {num_layers} exceeds the {MAX_LAYERS} layers a table row holds')
        if num_layers < 0:
            raise ValueError(f'RandAugment: n = {num_layers}')
        if weight_idx not in (None, 0):
            raise ValueError(f'RandAugment: w{weight_idx}: the reference has one set of choice weights, w0')
        self.config_str = config_str
        self.names = list(names)
        self.magnitude, self.num_layers, self.prob = magnitude, num_layers, 0.5
        self.choice_weights = None
        if weight_idx is not None:                # _select_rand_weights: always over the non-increasing names, position by position
            probs = [_RAND_CHOICE_WEIGHTS_0[k] for k in RAND_TRANSFORMS]
            self.choice_weights = probs / np.sum(probs)
        self.magnitude_std = hparams.get('magnitude_std', 0)
        self.magnitude_max = hparams.get('magnitude_max', None)
        self.translate_pct = hparams.get('translate_pct', 0.45)
        self.translate_const = hparams.get('translate_const', 250)       # the *Abs translations' only: kept, not used
        fill = hparams.get('img_mean', (128, 128, 128))
        if isinstance(fill, (int, np.integer)):
            fill = (int(fill),) * 3
        fill = tuple(int(v) for v in fill)
        if len(fill) != 3 or any(v < 0 or v > 255 for v in fill):
            raise ValueError(f'RandAugment: img_mean {fill} is not three values in [0, 255]')
        self.fill = fill
        interp = hparams.get('interpolation', (BILINEAR, BICUBIC))
        if isinstance(interp, str) and interp.lower() == 'random':
            interp = (BILINEAR, BICUBIC)
        self.interpolation = tuple(_interp_code(v) for v in interp) if isinstance(interp, (list, tuple)) else _interp_code(interp)
        if isinstance(self.interpolation, tuple) and not self.interpolation:
            raise ValueError('RandAugment: an empty interpolation tuple')

    # -- AugmentOp.__call__ for one op of one sample ------------------------------------------------------------------------------
    def _draw_op(self, row: np.ndarray, name: str, H: int, W: int) -> None:
        if self.prob < 1.0 and random.random() > self.prob:
            return
        magnitude = self.magnitude
        if self.magnitude_std > 0:
            if self.magnitude_std == float('inf'):
                magnitude = random.uniform(0, magnitude)
            else:
                magnitude = random.gauss(magnitude, self.magnitude_std)
        magnitude = max(0., min(magnitude, self.magnitude_max or _LEVEL_DENOM))
        level = magnitude / _LEVEL_DENOM
        base = name[:-len('Increasing')] if name.endswith('Increasing') else name
        increasing = base != name
        if name in _GEOMETRIC:
            if name == 'Rotate':
                matrix = rotate_matrix(_randomly_negate(level * 30.), W, H)
            elif name in ('ShearX', 'ShearY'):
                f = _randomly_negate(level * 0.3)
                matrix = (1, f, 0, 0, 1, 0) if name == 'ShearX' else (1, 0, 0, f, 1, 0)
            else:
                pct = _randomly_negate(level * self.translate_pct)
                matrix = (1, 0, pct * W, 0, 1, 0) if name == 'TranslateXRel' else (1, 0, 0, 0, 1, pct * H)
            interp = random.choice(self.interpolation) if isinstance(self.interpolation, tuple) else self.interpolation
            if matrix is not None:
                pack_layer(row, AFFINE, interp=interp, matrix=matrix)
        elif base in _ENHANCE:
            factor = max(0.1, 1.0 + _randomly_negate(level * .9)) if increasing else level * 1.8 + 0.1
            pack_layer(row, _ENHANCE[base], factor=factor)
        elif base == 'Posterize':
            bits = int(level * 4)
            bits = 4 - bits if increasing else bits
            if bits < 8:
                pack_layer(row, POSTERIZE, iarg=max(bits, 0))
        elif base == 'Solarize':
            thresh = int(level * 256)
            pack_layer(row, SOLARIZE, iarg=256 - thresh if increasing else thresh)
        elif name == 'SolarizeAdd':
            pack_layer(row, SOLARIZE_ADD, iarg=int(level * 110))
        else:
            pack_layer(row, {'AutoContrast': AUTOCONTRAST, 'Equalize': EQUALIZE, 'Invert': INVERT}[name])

    def draw(self, shape, chosen=None) -> np.ndarray:
        """One batch's table for a uint8 batch of ``shape`` (B, 3, H, W): int32 [B, 68], the layout of include/mmae.h.  ``chosen``: a
        list that receives, per sample, the names ``np.random.choice`` picked (before ``prob``)."""
        shape = tuple(int(v) for v in shape)
        if len(shape) != 4 or shape[1] != 3 or any(v <= 0 for v in shape):
            raise ValueError(f'RandAugment: expected a non-empty (B, 3, H, W) batch, got shape {shape}')
        B, _, H, W = shape
        table = np.zeros((B, ROW_WORDS), dtype=np.int32)
        table[:, 1:4] = self.fill
        ids = np.arange(len(self.names))
        for b in range(B):
            if self.choice_weights is None:       # what np.random.choice(ops, n, replace=True) draws, without its argument checks
                picks = np.random.randint(0, len(ids), size=self.num_layers)
            else:
                picks = np.random.choice(ids, self.num_layers, replace=False, p=self.choice_weights)
            names = [self.names[int(i)] for i in picks]
            if chosen is not None:
                chosen.append(names)
            for name in names:
                self._draw_op(table[b], name, H, W)
        return table
