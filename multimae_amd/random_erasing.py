"""Random erasing for the classification fine-tuning loop (mirror of the reference's ``utils/random_erasing.py`` ``RandomErasing``)
on HIP kernels.

Reference: RandomErasing.__call__ / _erase utils/random_erasing.py:74-103; in the reference it ends the CPU training transform,
ToTensor -> Normalize -> RandomErasing(device='cpu') (utils/transforms_factory.py:117-129).  Division of labour, as in ``mixup.py``:

  host    every random draw, through Python's ``random`` module in the reference's call order -- the ``num_splits`` skip, the
          probability test, the count, up to 10 attempts of (area, aspect) per rectangle, top and left -- and, in 'rand' mode, the
          colour ``torch.empty((C, 1, 1)).normal_()`` on torch's CPU generator exactly where the reference draws it.  The same seeds
          give the same rectangles and colours and leave both generators where the reference's batch-mode call leaves them.
          ``draw()`` packs one call into the int32 table of include/mmae.h ("Random erasing"), which reaches the device through
          ``engine.host_input``: pinned, non-blocking, and re-drawn before every replay of a captured step.
  device  ``mmae_random_erase`` erases the batch in place, touching erased pixels only; ``mmae_ingest_rgb_u8_chw_erase``
          (``data_ops.ingest_rgb_u8_chw``, ``staging.ClsStager``) decodes a uint8 batch and erases it in one pass.

Deviations:
  1. 'pixel' mode.  The reference draws ``torch.empty((C, h, w)).normal_()`` per rectangle; here the noise is a counter-based
     generator on the device (Philox4x32-10 + Box-Muller), keyed by ``noise_seed`` and ``noise_calls`` and indexed by the element's
     position in the batch.  The rectangles and the distribution are the same, the values differ, and torch's generator is not
     advanced.
  2. The draws are made per batch in the main process (the reference's own batch mode), not per sample in the loader workers.
  3. The output is float32 only.
"""
from __future__ import annotations

import math
import random

import numpy as np
import torch

from . import _lib, data_ops, engine, ops

MAX_RECTS, ROW_WORDS = _lib.ERASE_MAX_RECTS, _lib.ERASE_ROW
MODES = {'const': 0, 'rand': 1, 'pixel': 2}


class RandomErasing:
    """``utils.RandomErasing`` (same constructor, same ``__call__(x) -> x``) for an f32 batch or image on the GPU."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None,
                 mode='const', min_count=1, max_count=None, num_splits=0, device='cuda'):
        self.probability = probability
        self.min_area = min_area
        self.max_area = max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count = min_count
        self.max_count = max_count or min_count
        self.num_splits = num_splits
        mode = (mode or 'const').lower()
        if mode not in MODES:
            raise ValueError(f'RandomErasing: mode {mode!r} is not one of {sorted(MODES)}')
        if self.max_count > MAX_RECTS:
            raise ValueError(f'RandomErasing: max_count {self.max_count} exceeds the {MAX_RECTS} rectangles a table row holds')
        if self.min_count < 0 or self.min_count > self.max_count:
            raise ValueError(f'RandomErasing: need 0 <= min_count <= max_count, got {self.min_count}, {self.max_count}')
        self.mode = mode
        self.rand_color = mode == 'rand'
        self.per_pixel = mode == 'pixel'
        self.device = device
        self.noise_seed = None       # 'pixel' mode: key of the device generator, torch.initial_seed() at the first call unless set
        self.noise_calls = 0         # ... and its call counter, incremented once per draw(); a resumed run may set both

    # -- the reference's draws, in its order -------------------------------------------------------------------------------------
    def _draw_sample(self, row: np.ndarray, chan: int, img_h: int, img_w: int) -> None:
        """_erase (utils/random_erasing.py:74-92) for one sample: its rectangles into ``row``"""
        if random.random() > self.probability:
            return
        area = img_h * img_w
        count = self.min_count if self.min_count == self.max_count else random.randint(self.min_count, self.max_count)
        n = 0
        for _ in range(count):
            for _attempt in range(10):
                target_area = random.uniform(self.min_area, self.max_area) * area / count
                aspect_ratio = math.exp(random.uniform(*self.log_aspect_ratio))
                h = int(round(math.sqrt(target_area * aspect_ratio)))
                w = int(round(math.sqrt(target_area / aspect_ratio)))
                if w < img_w and h < img_h:
                    top = random.randint(0, img_h - h)
                    left = random.randint(0, img_w - w)
                    row[4 + 8 * n:8 + 8 * n] = (top, left, h, w)
                    if self.rand_color:
                        colour = torch.empty((chan, 1, 1), dtype=torch.float32).normal_()
                        row[8 + 8 * n:8 + 8 * n + chan] = colour.view(-1).numpy().view(np.int32)
                    n += 1
                    break
        row[0] = n

    def draw(self, shape) -> np.ndarray:
        """One call's table for a batch of ``shape`` (B, C, H, W), or an image (C, H, W) as a batch of one without the split skip:
        int32 [B + 1, 68], the layout of include/mmae.h."""
        shape = tuple(int(v) for v in shape)
        if len(shape) == 3:
            B, (C, H, W), start = 1, shape, 0
        elif len(shape) == 4:
            B, C, H, W = shape
            start = B // self.num_splits if self.num_splits > 1 else 0
        else:
            raise ValueError(f'RandomErasing: expected a (B, C, H, W) batch or a (C, H, W) image, got shape {shape}')
        if self.rand_color and C > 4:
            raise ValueError(f"RandomErasing: mode 'rand' holds 4 colours per rectangle, the input has {C} channels")
        if self.noise_seed is None:
            self.noise_seed = torch.initial_seed()
        table = np.zeros((B + 1, ROW_WORDS), dtype=np.int32)
        seed, calls = int(self.noise_seed) & (2 ** 64 - 1), int(self.noise_calls) & (2 ** 64 - 1)
        table[0, :4] = np.array([seed & 0xffffffff, seed >> 32, calls & 0xffffffff, calls >> 32], dtype=np.uint32).view(np.int32)
        table[0, 4] = MODES[self.mode]
        self.noise_calls += 1
        for i in range(start, B):
            self._draw_sample(table[1 + i], C, H, W)
        return table

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not (torch.is_tensor(x) and x.dim() in (3, 4) and x.dtype == torch.float32 and x.is_contiguous() and ops._device_ok(x)):
            raise ValueError('RandomErasing: x must be a contiguous float32 (B, C, H, W) batch or (C, H, W) image on the GPU')
        if x.numel() == 0:
            raise ValueError(f'RandomErasing: x is empty (shape {tuple(x.shape)})')
        shape = tuple(x.shape)
        if self.rand_color and shape[-3] > 4:
            raise ValueError(f"RandomErasing: mode 'rand' holds 4 colours per rectangle, the input has {shape[-3]} channels")
        table = engine.host_input(lambda: torch.from_numpy(self.draw(shape)), x.device)
        data_ops.random_erase_(x if x.dim() == 4 else x.unsqueeze(0), table)
        return x
