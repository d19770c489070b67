"""CPU: batch staging's host side -- batch validation, byte counts, the prefetch order of StagedLoader, and the compact
transform (dropin/amd_data.py) against a restatement of the reference's DataAugmentationForMultiMAE (utils/datasets.py:66-111)."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimae_amd import data_ops, staging  # noqa: E402
from dropin.amd_data import CompactAugmentation  # noqa: E402


def _cfg3(B, compact, meta=True):
    dev = 'meta' if meta else 'cpu'
    if compact:
        return {'rgb': torch.empty(B, 224, 224, 3, dtype=torch.uint8, device=dev),
                'depth': torch.empty(B, 224, 224, dtype=torch.uint16, device=dev),
                'semseg': torch.empty(B, 56, 56, dtype=torch.uint8, device=dev)}
    return {'rgb': torch.empty(B, 3, 224, 224, device=dev), 'depth': torch.empty(B, 1, 224, 224, device=dev),
            'semseg': torch.empty(B, 56, 56, dtype=torch.int64, device=dev)}


def test_bytes_per_batch_at_cfg3():
    c, r = staging.bytes_per_batch(_cfg3(256, True)), staging.bytes_per_batch(_cfg3(256, False))
    assert c['h2d'] == 65_028_096 and r['h2d'] == 211_943_424
    assert c['device'] == r['device'] == 211_943_424
    assert c['hbm'] == 65_028_096 + 211_943_424 and r['hbm'] == 0
    assert staging.bytes_per_batch(_cfg3(256, False), standardize_depth=True)['hbm'] == 2 * 51_380_224
    i32 = dict(_cfg3(256, True), depth=torch.empty(256, 1, 224, 224, dtype=torch.int32, device='meta'))
    assert staging.bytes_per_batch(i32)['h2d'] == 65_028_096 + 25_690_112


def test_forms_and_malformed_batches_rejected():
    assert staging.batch_forms(_cfg3(2, True)) == {'rgb': 'compact', 'depth': 'compact', 'semseg': 'compact'}
    assert staging.batch_forms(_cfg3(2, False)) == {'rgb': 'reference', 'depth': 'reference', 'semseg': 'reference'}
    assert staging.batch_form('semseg_coco', torch.empty(2, 56, 56, dtype=torch.uint8)) == 'compact'
    bad = [
        ('rgb', torch.empty(2, 224, 224, 3, dtype=torch.float32)),    # HWC float
        ('rgb', torch.empty(2, 3, 224, 224, dtype=torch.uint8)),      # CHW uint8
        ('rgb', torch.empty(2, 224, 224, 4, dtype=torch.uint8)),      # RGBA
        ('depth', torch.empty(2, 224, 224, dtype=torch.float64)),
        ('depth', torch.empty(2, 2, 224, 224, dtype=torch.uint16)),
        ('depth', torch.empty(2, 224, 224, dtype=torch.int16)),
        ('depth', torch.empty(2, 224, 224, dtype=torch.float32)),     # fp32 without the channel axis
        ('semseg', torch.empty(2, 1, 56, 56, dtype=torch.uint8)),
        ('semseg', torch.empty(2, 56, 56, dtype=torch.int32)),
        ('rgb', torch.empty(0, 224, 224, 3, dtype=torch.uint8)),      # empty
        ('normal', torch.empty(2, 3, 224, 224)),                      # a task the stager does not know
    ]
    for task, t in bad:
        with pytest.raises(ValueError) as e:
            staging.batch_forms({task: t})
        msg = str(e.value)
        assert repr(task) in msg and str(tuple(t.shape)) in msg and str(t.dtype) in msg, msg
    with pytest.raises(ValueError):
        staging.batch_forms({'rgb': torch.empty(2, 224, 224, 3, dtype=torch.uint8), 'semseg': torch.empty(3, 56, 56, dtype=torch.uint8)})
    with pytest.raises(ValueError):
        staging.batch_forms({})


class _RecordingStager:
    def __init__(self):
        self.log = []

    def stage(self, batch):
        self.log.append(('stage', batch['i']))
        return batch['i']

    def get(self, staged):
        self.log.append(('get', staged))
        return {'i': staged}


def test_staged_loader_stages_one_batch_ahead():
    st = _RecordingStager()
    loader = staging.StagedLoader([({'i': k}, k * 10) for k in range(4)], st)
    assert len(loader) == 4
    got = []
    for x, target in loader:
        got.append((x['i'], target))
        st.log.append(('step', x['i']))
    assert got == [(k, k * 10) for k in range(4)]
    # batch k + 1 is staged before batch k is handed out
    assert st.log == [('stage', 0), ('stage', 1), ('get', 0), ('step', 0), ('stage', 2), ('get', 1), ('step', 1),
                      ('stage', 3), ('get', 2), ('step', 2), ('get', 3), ('step', 3)]
    assert [x['i'] for x in staging.StagedLoader([{'i': 7}], _RecordingStager())] == [7]
    assert list(staging.StagedLoader([], _RecordingStager())) == []
    with pytest.raises(ValueError):
        list(staging.StagedLoader([torch.zeros(2)], _RecordingStager()))


# ---- the compact transform against the reference transform ---------------------------------------------------------------

MEANS = {'default': (staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD),
         'inception': (staging.IMAGENET_INCEPTION_MEAN, staging.IMAGENET_INCEPTION_STD)}


def _images(seed, size=(173, 141), depth_mode='I;16'):
    g = np.random.default_rng(seed)
    H, W = size
    rgb = Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8), 'RGB')
    if depth_mode == 'I;16':
        depth = Image.fromarray(g.integers(0, 65536, (H, W), dtype=np.uint16))
    else:
        depth = Image.fromarray(g.integers(-3000, 70000, (H, W), dtype=np.int32))
    sem = Image.fromarray(g.integers(0, 140, (H, W), dtype=np.uint8), 'L').convert('P')
    assert depth.mode == depth_mode
    return {'rgb': rgb, 'depth': depth, 'semseg': sem}


def _reference_transform(task_dict, ijhw, flip, input_size, mean, std):
    """DataAugmentationForMultiMAE.__call__ restated with PIL + torch (to_tensor / normalize / pil_to_tensor as torchvision
    computes them), the crop parameters given."""
    i, j, h, w = ijhw
    out = {}
    for task, img in task_dict.items():
        img = img.crop((j, i, j + w, i + h)).resize((input_size, input_size))
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        if task == 'depth':
            out[task] = torch.Tensor(np.array(img) / 2 ** 16).unsqueeze(0)
        elif task == 'rgb':
            t = torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous().float().div(255)
            out[task] = t.sub(torch.as_tensor(mean).view(3, 1, 1)).div(torch.as_tensor(std).view(3, 1, 1))
        else:
            s = int(input_size * 0.25)
            out[task] = torch.from_numpy(np.array(img.resize((s, s)))).to(torch.long)
    return out


def _decode_on_cpu(arrays, mean, std):
    """the device decode's arithmetic (csrc/ingest.hip) on the CPU: table gather, float(v) * 2^-16, widening"""
    tab = data_ops.rgb_table(mean, std)
    rgb = torch.from_numpy(arrays['rgb'])
    out = {'rgb': torch.stack([tab[c][rgb[..., c].long()] for c in range(3)])}
    d = torch.from_numpy(arrays['depth'].astype(np.int64) if arrays['depth'].dtype == np.uint16 else arrays['depth'])
    out['depth'] = (d.float() * 2.0 ** -16).unsqueeze(0)
    out['semseg'] = torch.from_numpy(arrays['semseg']).to(torch.long)
    return out


@pytest.mark.parametrize('depth_mode', ['I;16', 'I'])
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('norm', ['default', 'inception'])
def test_compact_augmentation_matches_the_reference_transform(depth_mode, flip, norm):
    mean, std = MEANS[norm]
    ijhw = (11, 7, 120, 97)
    calls = []

    def get_params(img, scale, ratio):
        calls.append((img.size, scale, ratio))
        return ijhw

    args = types.SimpleNamespace(input_size=64, hflip=1.0 if flip else 0.0)
    aug = CompactAugmentation(args, get_params=get_params)
    src = _images(3, depth_mode=depth_mode)
    arrays = aug({k: v.copy() for k, v in src.items()})
    assert calls == [((141, 173), (0.2, 1.0), (0.75, 1.3333))]            # once, on the first image task
    assert arrays['rgb'].dtype == np.uint8 and arrays['rgb'].shape == (64, 64, 3)
    assert arrays['depth'].dtype == (np.uint16 if depth_mode == 'I;16' else np.int32) and arrays['depth'].shape == (64, 64)
    assert arrays['semseg'].dtype == np.uint8 and arrays['semseg'].shape == (16, 16)
    ref = _reference_transform(src, ijhw, flip, 64, mean, std)
    got = _decode_on_cpu(arrays, mean, std)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert torch.equal(got[k], ref[k]), (k, float((got[k].double() - ref[k].double()).abs().max()))


def test_rgb_table_is_to_tensor_then_normalize_for_every_byte():
    u8 = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 256, 3)       # every value in every channel
    for mean, std in MEANS.values():
        ref = torch.from_numpy(u8).permute(2, 0, 1).float().div(255).sub(torch.as_tensor(mean).view(3, 1, 1)).div(torch.as_tensor(std).view(3, 1, 1))
        assert torch.equal(data_ops.rgb_table(mean, std), ref[:, 0, :])


def test_compact_augmentation_draws_the_flip_once_per_sample():
    args = types.SimpleNamespace(input_size=32, hflip=0.5)
    aug = CompactAugmentation(args, get_params=lambda img, scale, ratio: (0, 0, 40, 40))
    random.seed(5)
    for _ in range(3):
        aug(_images(1, size=(48, 48)))
    after = random.random()
    random.seed(5)
    for _ in range(3):
        random.random()
    assert after == random.random()


def test_rng_sequence_equals_the_reference_class():
    """with torchvision: the crop parameters and flips drawn by CompactAugmentation are the reference transform's (same seeds)"""
    tv = pytest.importorskip('torchvision')
    from torchvision import transforms
    import torchvision.transforms.functional as TF
    assert tv is not None

    def reference(task_dict, input_size, hflip):                      # utils/datasets.py:74-91, the geometric part
        flip = random.random() < hflip
        ijhw = None
        for task in task_dict:
            if ijhw is None:
                ijhw = transforms.RandomResizedCrop.get_params(task_dict[task], scale=(0.2, 1.0), ratio=(0.75, 1.3333))
            i, j, h, w = ijhw
            task_dict[task] = TF.crop(task_dict[task], i, j, h, w).resize((input_size, input_size))
            if flip:
                task_dict[task] = TF.hflip(task_dict[task])
        return task_dict

    args = types.SimpleNamespace(input_size=48, hflip=0.5)
    aug = CompactAugmentation(args)
    for seed in range(6):
        src = _images(seed)
        random.seed(seed)
        torch.manual_seed(seed)
        ref = reference({k: v.copy() for k, v in src.items()}, 48, 0.5)
        random.seed(seed)
        torch.manual_seed(seed)
        got = aug({k: v.copy() for k, v in src.items()})
        assert np.array_equal(got['rgb'], np.array(ref['rgb'])) and np.array_equal(got['depth'], np.array(ref['depth']))
