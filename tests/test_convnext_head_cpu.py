"""CPU: the ConvNeXt semantic-segmentation head (ConvNeXtAdapter, output_adapters.py:481-573) -- the semseg fine-tuning script's import
line through dropin/, the name-only DPT / Segmenter heads, the state-dict contract against the reference's seeded build
(tests/golden/convnext_head.npz, make_golden_convnext.py) and the host control flow of forward + backward against the C ABI stub."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import output_adapters as OA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'convnext_head.npz')
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_convnext import HEADS, VIT, perturb  # noqa: E402


def test_semseg_script_import_line_through_dropin(tmp_path):
    """run_finetuning_semseg.py:36-39 imports ConvNeXtAdapter, DPTOutputAdapter, SegmenterMaskTransformerAdapter from
    multimae.output_adapters; with dropin/ first on sys.path they resolve to the engine."""
    (tmp_path / 'utils').mkdir()
    (tmp_path / 'utils' / '__init__.py').write_text('')
    (tmp_path / 'utils' / 'registry.py').write_text('_model_entrypoints = {}\n')
    code = (
        'import utils.registry\n'
        'from multimae import multimae\n'
        'from multimae.input_adapters import PatchedInputAdapter, SemSegInputAdapter\n'
        'from multimae.output_adapters import (ConvNeXtAdapter, DPTOutputAdapter,\n'
        '                                      SegmenterMaskTransformerAdapter)\n'
        'assert ConvNeXtAdapter.__module__ == "multimae_amd.output_adapters"\n'
        'h = ConvNeXtAdapter(num_classes=150, embed_dim=6144, preds_per_patch=16, main_tasks=("rgb",), patch_size=16, depth=4)\n'
        'h.init(dim_tokens_enc=768)\n'
        'assert h.blocks[0].dwconv.weight.shape == (384, 1, 7, 7) and h.final_layer.weight.shape == (150, 384, 1, 1)\n'
        'print("ok")\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'dropin'), str(tmp_path)]))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize('cls', [OA.DPTOutputAdapter, OA.SegmenterMaskTransformerAdapter])
def test_unbuilt_heads_raise(cls):
    with pytest.raises(NotImplementedError, match=cls.__name__):
        cls(num_classes=150)


def test_constructor_rejects_what_the_reference_cannot_run():
    with pytest.raises(ValueError, match='perfect square'):
        OA.ConvNeXtAdapter(num_classes=3, embed_dim=96, preds_per_patch=8)
    with pytest.raises(ValueError, match='multiple'):
        OA.ConvNeXtAdapter(num_classes=3, embed_dim=100, preds_per_patch=16)
    head = OA.ConvNeXtAdapter(num_classes=3, embed_dim=64, preds_per_patch=16, main_tasks=('rgb', 'depth'), depth=1)
    head.init(8)
    info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': 6}, 'depth': {'start_idx': 6, 'end_idx': 10}}, 'image_size': (32, 48)}
    with pytest.raises(ValueError, match='grid'):
        head(torch.zeros(1, 11, 8), info)


def _assert_sd_equal(sd, gold, prefix):
    keys = [k[len(prefix):] for k in gold.files if k.startswith(prefix)]
    assert list(sd.keys()) == keys
    for k in keys:
        g = gold[prefix + k]
        assert tuple(sd[k].shape) == g.shape, k
        assert np.array_equal(sd[k].detach().cpu().numpy(), g), k


@pytest.mark.parametrize('name', list(HEADS))
def test_head_state_dict_matches_reference_seeded_build(name):
    gold = np.load(GOLD)
    seed = list(HEADS).index(name)
    tasks, mode, p, C, K, depth, _, D, _ = HEADS[name]
    torch.manual_seed(100 + seed)
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                              interpolate_mode=mode)
    head.init(dim_tokens_enc=D)
    perturb(head, 200 + seed)
    _assert_sd_equal(head.state_dict(), gold, f'{name}/sd/')


def build_vit():
    """the engine twin of make_golden_convnext.build_vit"""
    torch.manual_seed(7)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=(VIT['H'], VIT['W']))}
    outs = {'semseg': OA.ConvNeXtAdapter(num_classes=VIT['K'], embed_dim=VIT['E'], preds_per_patch=VIT['p'], main_tasks=('rgb',),
                                         patch_size=16, depth=VIT['head_depth'])}
    return M.MultiViT(input_adapters=ins, output_adapters=outs, num_global_tokens=1, dim_tokens=VIT['D'], depth=VIT['depth'],
                      num_heads=VIT['heads'])


def test_multivit_with_head_state_dict_matches_reference():
    """MultiMAE.__init__'s xavier walk re-initialises proj_dec and the pointwise convolutions as the reference's does"""
    _assert_sd_equal(build_vit().state_dict(), np.load(GOLD), 'vit/sd/')


@pytest.fixture()
def stubbed():
    from multimae_amd import _lib, ops
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('direct', [False, True])
def test_head_control_flow(stubbed, mode, direct):
    """forward + backward of the head alone and under MultiViT run their host code in both precisions and gradient modes; every
    parameter and the encoder tokens receive a gradient of the right shape."""
    head = OA.ConvNeXtAdapter(num_classes=5, embed_dim=256, preds_per_patch=16, main_tasks=('rgb', 'depth'), depth=2,
                              interpolate_mode='nearest')
    head.init(16)
    info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': 6}, 'depth': {'start_idx': 6, 'end_idx': 12}}, 'image_size': (32, 48)}
    x = torch.randn(2, 13, 16, requires_grad=True)
    with M.engine.precision(mode):
        y = head(x, info)
        assert y.shape == (2, 5, 32, 48) and y.dtype == torch.float32
        y.sum().backward()
    assert x.grad.shape == x.shape
    assert all(p.grad is not None and p.grad.shape == p.shape for p in head.parameters())
    model = build_vit()
    model.build_arena()
    M.engine.set_direct_grads(direct)
    try:
        with M.engine.precision(mode):
            out = model({'rgb': torch.randn(2, 3, VIT['H'], VIT['W'])})['semseg']
            assert out.shape == (2, VIT['K'], VIT['H'], VIT['W'])
            out.sum().backward()
    finally:
        M.engine.set_direct_grads(False)
