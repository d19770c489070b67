"""The pre-training transform with its last step left to the device: ``CompactAugmentation`` is DataAugmentationForMultiMAE
(utils/datasets.py:66-111) up to the point where it converts to tensors, and returns the decoded arrays instead --

  rgb     uint8 (H, W, 3)                    (to_tensor + normalize: multimae_amd.staging on the device)
  depth   uint16 (Pillow 'I;16') or int32 ('I') (H, W)   (/ 2**16)
  semseg  uint8 (h, w), after the 0.25x resize           (.to(torch.long))

The library calls and their order are the reference's, so the Python / torch RNG sequence is unchanged: ``random.random()``
for the flip, ``RandomResizedCrop.get_params`` once for the first image task, then per image task crop, resize to
``input_size``, horizontal flip; the semseg map is resized to a quarter afterwards.  The default collate stacks the arrays
into the compact batch ``multimae_amd.BatchStager`` decodes ("Batch staging").
"""
from __future__ import annotations

import random

import numpy as np
from PIL import Image

IMAGE_TASKS = ('rgb', 'depth', 'semseg', 'semseg_coco')      # utils/data_constants.py:27
CROP_SCALE, CROP_RATIO = (0.2, 1.0), (0.75, 1.3333)          # the values the reference passes to get_params


def _torchvision_get_params(img, scale, ratio):
    from torchvision import transforms                       # only this call needs torchvision
    return transforms.RandomResizedCrop.get_params(img, scale=scale, ratio=ratio)


class CompactAugmentation:
    """``DataAugmentationForMultiMAE(args)`` without the tensor conversion.  ``get_params(img, scale, ratio) -> (i, j, h, w)``
    replaces ``torchvision.transforms.RandomResizedCrop.get_params`` (tests inject fixed crops)."""

    def __init__(self, args, get_params=None):
        self.input_size = args.input_size
        self.hflip = args.hflip
        self.get_params = get_params or _torchvision_get_params

    def __call__(self, task_dict):
        flip = random.random() < self.hflip
        ijhw = None
        for task in task_dict:
            if task not in IMAGE_TASKS:
                continue
            img = task_dict[task]
            if ijhw is None:
                ijhw = self.get_params(img, CROP_SCALE, CROP_RATIO)
            i, j, h, w = ijhw
            img = img.crop((j, i, j + w, i + h))                  # TF.crop(img, top=i, left=j, height=h, width=w) on a PIL image
            img = img.resize((self.input_size, self.input_size))
            if flip:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)        # TF.hflip on a PIL image
            task_dict[task] = img
        for task in task_dict:
            img = task_dict[task]
            if task in ('semseg', 'semseg_coco'):
                side = int(self.input_size * 0.25)
                img = img.resize((side, side))
            if task in ('rgb', 'depth', 'semseg', 'semseg_coco'):
                task_dict[task] = np.array(img)
        return task_dict

    def __repr__(self):
        return f'CompactAugmentation(input_size={self.input_size}, hflip={self.hflip})'
