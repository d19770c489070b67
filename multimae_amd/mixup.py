"""Mixup / CutMix for the classification fine-tuning loop (mirror of the reference's ``utils/mixup.py`` ``Mixup``) on HIP kernels.

Reference: Mixup utils/mixup.py:96-225, mixup_target :23-33, the box helpers :36-93.  Division of labour:

  host    every random draw, through ``np.random`` in the reference's call order (so the same ``np.random.seed`` gives the same
          parameters and leaves the generator in the same state), expanded into ONE per-sample block (``draw()``): blend weights of
          the pixels, blend weights of the target rows, the CutMix box.  The three modes ('batch', 'pair', 'elem') differ only in
          how the rows are filled.  The block reaches the device through ``engine.host_input``: pinned, non-blocking, and re-drawn
          before every replay of a captured step.
  device  ``mmae_mixup_pairs`` mixes the batch in place (samples i and B - 1 - i in one work item: read once, written once, no
          clone / flip), ``mmae_mix_target`` writes the soft target.  Both are bit-identical to the reference's eager f32
          expressions; the weights are therefore formed exactly as each mode of the reference forms them (batch mode rounds the
          Python doubles ``lam`` and ``1. - lam``; pair / elem modes subtract in float32).

Deviations: a label outside [0, num_classes) raises ValueError when the labels live on the host; labels already on the device are
not read back (no synchronisation) -- such a label matches no class and its row holds ``off_value`` everywhere (the reference's
scatter writes out of bounds).  ``FastCollateMixup`` (uint8 mixing inside the collate function) is not provided.
"""
from __future__ import annotations

import numpy as np
import torch

from . import engine, ops


def _box_from_lam(h: int, w: int, lam):
    """the square-ish box whose area share is 1 - lam around a uniformly drawn centre, clipped to the image (utils/mixup.py:36-57,
    margin 0): two randint draws, the row first"""
    r = np.sqrt(1 - lam)
    ch, cw = int(h * r), int(w * r)
    cy = np.random.randint(0, h, size=None)
    cx = np.random.randint(0, w, size=None)
    return (int(np.clip(cy - ch // 2, 0, h)), int(np.clip(cy + ch // 2, 0, h)),
            int(np.clip(cx - cw // 2, 0, w)), int(np.clip(cx + cw // 2, 0, w)))


def _box_from_minmax(h: int, w: int, minmax):
    """a box whose sides are drawn between the two ratios of the image's (utils/mixup.py:60-80): four randint draws -- height, width,
    top, left"""
    ch = np.random.randint(int(h * minmax[0]), int(h * minmax[1]), size=None)
    cw = np.random.randint(int(w * minmax[0]), int(w * minmax[1]), size=None)
    yl = np.random.randint(0, h - ch, size=None)
    xl = np.random.randint(0, w - cw, size=None)
    return int(yl), int(yl + ch), int(xl), int(xl + cw)


class Mixup:
    """``utils.Mixup`` (same constructor, same ``__call__(x, target) -> (x, soft_target)``) for an f32 batch on the GPU."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5,
                 mode='batch', correct_lam=True, label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if cutmix_minmax is not None:
            if len(cutmix_minmax) != 2:
                raise ValueError('Mixup: cutmix_minmax is a (min, max) pair of image ratios')
            self.cutmix_alpha = 1.0                       # the min / max box replaces the beta-drawn one (utils/mixup.py:116-119)
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True                         # the training loop may switch mixing off

    # -- the reference's draws, in its order ---------------------------------------------------------------------------------
    def _no_alpha(self):
        raise AssertionError('One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.')

    def _params_per_elem(self, n: int):
        lam = np.ones(n, dtype=np.float32)
        cut = np.zeros(n, dtype=bool)
        if not self.mixup_enabled:
            return lam, cut
        both = self.mixup_alpha > 0. and self.cutmix_alpha > 0.
        if both:
            cut = np.random.rand(n) < self.switch_prob
            on_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            on_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            mixed = np.where(cut, on_cut, on_mix)
        elif self.mixup_alpha > 0.:
            mixed = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
        elif self.cutmix_alpha > 0.:
            cut = np.ones(n, dtype=bool)
            mixed = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
        else:
            self._no_alpha()
        lam = np.where(np.random.rand(n) < self.mix_prob, mixed.astype(np.float32), lam)
        return lam, cut

    def _params_per_batch(self):
        lam, cut = 1., False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                cut = np.random.rand() < self.switch_prob
                a = self.cutmix_alpha if cut else self.mixup_alpha
            elif self.mixup_alpha > 0.:
                a = self.mixup_alpha
            elif self.cutmix_alpha > 0.:
                cut, a = True, self.cutmix_alpha
            else:
                self._no_alpha()
            lam = float(np.random.beta(a, a))
        return lam, cut

    def _box_and_lam(self, h: int, w: int, lam):
        """cutmix_bbox_and_lam (utils/mixup.py:83-93): the box, and lam corrected to the area actually replaced"""
        if self.cutmix_minmax is not None:
            box = _box_from_minmax(h, w, self.cutmix_minmax)
        else:
            box = _box_from_lam(h, w, lam)
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1. - (box[1] - box[0]) * (box[3] - box[2]) / float(h * w)
        return box, lam

    # -- the per-sample block --------------------------------------------------------------------------------------------------
    def draw(self, shape) -> np.ndarray:
        """One call's parameters for a batch of ``shape`` (B, C, H, W): int32 [B, 8], the rows of ``mmae_mixup_pairs`` /
        ``mmae_mix_target`` (include/mmae.h) -- words 0-3 hold the bits of the f32 weights w_self, w_other, t_self, t_other, words 4-7
        the box (yl, yh, xl, xh), yl = MIX_BLEND for a blend, MIX_KEEP for a sample that stays as it is."""
        B, _, H, W = shape
        if B % 2:
            raise ValueError('Mixup: the batch size must be even')
        wts = np.zeros((B, 4), dtype=np.float32)
        wts[:, 0] = wts[:, 2] = 1.
        box = np.zeros((B, 4), dtype=np.int32)
        box[:, 0] = ops.MIX_KEEP
        if self.mode in ('elem', 'pair'):
            n = B if self.mode == 'elem' else B // 2
            lam_batch, cut = self._params_per_elem(n)
            one = np.float32(1.)
            for i in range(n):
                lam = lam_batch[i]
                if lam != 1.:
                    if cut[i]:
                        box[i], lam = self._box_and_lam(H, W, lam)
                        lam_batch[i] = lam                   # rounded to float32, as the reference's array assignment does
                    else:
                        box[i, 0] = ops.MIX_BLEND
                        wts[i, 0], wts[i, 1] = lam, one - lam
                wts[i, 2], wts[i, 3] = lam_batch[i], one - lam_batch[i]
            if self.mode == 'pair':
                wts[B // 2:] = wts[:B // 2][::-1]
                box[B // 2:] = box[:B // 2][::-1]
        else:
            lam, cut = self._params_per_batch()
            if lam != 1.:
                if cut:
                    box[:], lam = self._box_and_lam(H, W, lam)
                else:
                    box[:, 0] = ops.MIX_BLEND
                    wts[:, 0], wts[:, 1] = np.float32(lam), np.float32(1. - lam)
                wts[:, 2], wts[:, 3] = np.float32(lam), np.float32(1. - lam)
        return np.concatenate([wts.view(np.int32), box], axis=1)

    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        if not (torch.is_tensor(x) and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous() and ops._device_ok(x)):
            raise ValueError('Mixup: x must be a contiguous float32 (B, C, H, W) batch on the GPU')
        B, K = x.shape[0], int(self.num_classes)
        if B % 2:
            raise ValueError('Mixup: the batch size must be even')
        if target.dim() != 1 or target.shape[0] != B or target.is_floating_point() or target.dtype == torch.bool:
            raise ValueError('Mixup: target must be an integer tensor of B class indices')
        if target.device.type == 'cpu' and B and (int(target.min()) < 0 or int(target.max()) >= K):
            raise ValueError(f'Mixup: a label lies outside [0, {K})')
        labels = target.to(device=x.device, dtype=torch.int64, non_blocking=True).contiguous()
        shape = tuple(x.shape)
        rows = engine.host_input(lambda: torch.from_numpy(self.draw(shape)), x.device)
        ops.mixup_pairs(x, rows)
        off = self.label_smoothing / K
        on = 1. - self.label_smoothing + off
        return x, ops.mix_target(labels, rows, K, on, off)
