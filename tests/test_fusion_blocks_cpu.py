"""CPU: the RefineNet pieces of the DPT head (multimae_amd/output_adapter_utils.py; reference output_adapter_utils.py:60-290) -- the
state-dict contract against the reference's seeded build (tests/golden/fusion_blocks.npz, make_golden_fusion.py), what the
constructors refuse, the import through dropin/, the tests' own torch restatement (tests/fusion_oracle.py) against the recorded f32
results bit for bit, and the host control flow of forward + backward against the C ABI stub."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

from multimae_amd import output_adapter_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'fusion_blocks.npz')
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from make_golden_fusion import CASES, SCRATCH, case_seed  # noqa: E402
import fusion_oracle as FO  # noqa: E402


def gold_sd(gold, prefix):
    return {k[len(prefix):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(prefix)}


def build(name):
    """the engine twins of the fixture's seeded residual unit and fusion block"""
    f = CASES[name][0]
    torch.manual_seed(case_seed(name))
    rcu = U.ResidualConvUnit_custom(f, nn.ReLU(False), False)
    torch.manual_seed(case_seed(name) + 1)
    ffb = U.make_fusion_block(f, False)
    return rcu, ffb


def _assert_sd_equal(sd, gold, prefix):
    keys = [k[len(prefix):] for k in gold.files if k.startswith(prefix)]
    assert keys and list(sd.keys()) == keys
    for k in keys:
        g = gold[prefix + k]
        assert tuple(sd[k].shape) == g.shape, k
        assert np.array_equal(sd[k].detach().cpu().numpy(), g), k


def test_scratch_state_dict_matches_reference_seeded_build():
    gold = np.load(GOLD)
    torch.manual_seed(SCRATCH['seed'])
    scratch = U.make_scratch(SCRATCH['in_shape'], SCRATCH['out_shape'], groups=1, expand=False)
    _assert_sd_equal(scratch.state_dict(), gold, 'scratch/sd/')
    assert [n for n, _ in scratch.named_parameters()] == [f'layer{i}_rn.weight' for i in (1, 2, 3, 4)]
    assert scratch.layer_rn[2] is scratch.layer3_rn and scratch.layer2_rn.weight.shape == (16, 16, 3, 3)


@pytest.mark.parametrize('name', list(CASES))
def test_block_state_dicts_match_reference_seeded_build(name):
    gold = np.load(GOLD)
    rcu, ffb = build(name)
    _assert_sd_equal(rcu.state_dict(), gold, f'{name}/rcu/sd/')
    _assert_sd_equal(ffb.state_dict(), gold, f'{name}/ffb/sd/')
    assert list(rcu.state_dict()) == ['conv1.weight', 'conv1.bias', 'conv2.weight', 'conv2.bias']
    assert list(ffb.state_dict())[:2] == ['out_conv.weight', 'out_conv.bias']


@pytest.mark.parametrize('name', list(CASES))
def test_load_state_dict_of_the_reference_parameters(name):
    gold = np.load(GOLD)
    f = CASES[name][0]
    torch.manual_seed(1)
    rcu, ffb = U.ResidualConvUnit_custom(f, nn.ReLU(False), False), U.make_fusion_block(f, False)
    for m, key in ((rcu, 'rcu'), (ffb, 'ffb')):
        sd = gold_sd(gold, f'{name}/{key}/sd/')
        missing, unexpected = m.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    scratch = U.make_scratch(SCRATCH['in_shape'], SCRATCH['out_shape'])
    # a DPT checkpoint's scratch.* sub-dict: both the layerN_rn and the layer_rn.N keys
    scratch.load_state_dict(gold_sd(gold, 'scratch/sd/'), strict=True)
    assert torch.equal(scratch.layer_rn[3].weight, torch.from_numpy(gold['scratch/sd/layer4_rn.weight']))


def test_constructors_refuse_what_is_not_built():
    relu = nn.ReLU(False)
    with pytest.raises(NotImplementedError, match='bn'):
        U.ResidualConvUnit_custom(8, relu, True)
    with pytest.raises(NotImplementedError, match='bn'):
        U.make_fusion_block(8, True)
    with pytest.raises(NotImplementedError, match='expand'):
        U.FeatureFusionBlock_custom(8, relu, expand=True)
    with pytest.raises(NotImplementedError, match='deconv'):
        U.FeatureFusionBlock_custom(8, relu, deconv=True)
    with pytest.raises(NotImplementedError, match='groups'):
        U.make_scratch([8, 8, 8, 8], 8, groups=2)
    with pytest.raises(NotImplementedError, match='expand'):
        U.make_scratch([8, 8, 8, 8], 8, expand=True)
    with pytest.raises(NotImplementedError, match='groups'):
        U.Conv3x3(8, 8, groups=2)
    with pytest.raises(NotImplementedError, match='stride'):
        U.Conv3x3(8, 8, stride=3)
    with pytest.raises(NotImplementedError, match='activation'):
        U.ResidualConvUnit_custom(8, nn.GELU(), False)
    with pytest.raises(NotImplementedError, match='mode'):
        U.Interpolate(scale_factor=2, mode='nearest', align_corners=True)
    ip = U.Interpolate(scale_factor=2, mode='bilinear', align_corners=True)
    assert (ip.scale_factor, ip.mode, ip.align_corners) == (2, 'bilinear', True)
    with pytest.raises(ValueError, match='one or two'):
        U.make_fusion_block(8, False)()
    with pytest.raises(ValueError, match='cap'):
        U.set_col_workspace_bytes(0)


def test_no_cpu_fallback():
    rcu, ffb = build('c8')
    x = torch.randn(2, 8, 3, 4)
    for fn in (lambda: rcu(x), lambda: ffb(x), lambda: ffb(x, x), lambda: U.Conv3x3(8, 8)(x),
               lambda: U.Interpolate(2, 'bilinear', True)(x)):
        with pytest.raises(RuntimeError, match='no CPU'):
            fn()


def test_import_through_dropin(tmp_path):
    """`from multimae.output_adapter_utils import ...` (the reference's output_adapters.py:28 imports these names) resolves to the engine"""
    (tmp_path / 'utils').mkdir()
    (tmp_path / 'utils' / '__init__.py').write_text('')
    (tmp_path / 'utils' / 'registry.py').write_text('_model_entrypoints = {}\n')
    code = (
        'import utils.registry\n'
        'from multimae.output_adapter_utils import (ResidualConvUnit_custom, FeatureFusionBlock_custom, make_fusion_block,\n'
        '                                           make_scratch, Interpolate, Conv3x3)\n'
        'assert FeatureFusionBlock_custom.__module__ == "multimae_amd.output_adapter_utils"\n'
        'b = make_fusion_block(256, False)\n'
        'assert b.resConfUnit2.conv1.weight.shape == (256, 256, 3, 3) and b.out_conv.weight.shape == (256, 256, 1, 1)\n'
        's = make_scratch([96, 192, 384, 768], 256, groups=1, expand=False)\n'
        'assert s.layer4_rn.weight.shape == (256, 768, 3, 3) and s.layer4_rn.bias is None\n'
        'print("ok")\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'dropin'), str(tmp_path)]))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('which', ['rcu', 'ffb1', 'ffb2'])
def test_oracle_restatement_reproduces_the_reference_bit_for_bit(name, which):
    gold = np.load(GOLD)
    x0, x1 = torch.from_numpy(gold[f'{name}/x0']), torch.from_numpy(gold[f'{name}/x1'])
    sd = gold_sd(gold, f'{name}/{"rcu" if which == "rcu" else "ffb"}/sd/')
    xs = [x0, x1] if which == 'ffb2' else [x0]
    y, dxs, grads = FO.run(FO.rcu if which == 'rcu' else FO.fusion, xs, sd)
    pre = f'{name}/{which}/f32/'
    assert np.array_equal(y.numpy(), gold[pre + 'y'])
    for i, d in enumerate(dxs):
        assert np.array_equal(d.numpy(), gold[pre + f'dx{i}']), i
    names = [k[len(pre) + 5:] for k in gold.files if k.startswith(pre + 'grad/')]
    assert sorted(names) == sorted(grads) and (which != 'ffb1' or not any('resConfUnit1' in n for n in names))
    for n in names:
        assert np.array_equal(grads[n].numpy(), gold[pre + 'grad/' + n]), n
    # the f64 evaluation of the fixture is the same computation widened
    y64, _, g64 = FO.run(FO.rcu if which == 'rcu' else FO.fusion, xs, sd, torch.float64)
    assert np.allclose(y64.numpy(), gold[f'{name}/{which}/f64/y'], rtol=1e-12, atol=1e-13)
    for n in names:
        assert np.allclose(g64[n].numpy(), gold[f'{name}/{which}/f64/grad/{n}'], rtol=1e-11, atol=1e-12), n


@pytest.fixture()
def stubbed():
    from multimae_amd import _lib, ops
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()
    from multimae_amd import functions
    functions.ops._require_gpu = ops._require_gpu


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('direct', [False, True])
def test_blocks_control_flow(stubbed, mode, direct):
    """forward + backward of every module run their host code in both precisions and gradient modes, with the batch in three chunks;
    every parameter and input receives a gradient of the right shape, and outputs are channels-last strided."""
    from multimae_amd import engine
    rcu, ffb = build('c8')
    conv = U.Conv3x3(8, 16, stride=2, bias=True)
    mods = nn.ModuleList([rcu, ffb, conv])
    if direct:
        engine.ParamArena(mods)
    B, h, w = 5, 3, 4
    old = U.set_col_workspace_bytes(2 * h * w * 72 * 4)               # two samples of f32 rows per chunk
    engine.set_direct_grads(direct)
    try:
        with engine.precision(mode):
            x0 = torch.randn(B, 8, h, w, requires_grad=True)
            x1 = torch.randn(B, 8, h, w).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            y = ffb(rcu(x0), x1)
            assert y.shape == (B, 8, 2 * h, 2 * w) and y.dtype == torch.float32 and y.is_contiguous(memory_format=torch.channels_last)
            z = conv(U.Interpolate(2, 'bilinear', True)(y))
            assert z.shape == (B, 16, 2 * h, 2 * w)
            z.sum().backward()
            y1 = ffb(x0.detach())
            assert y1.shape == y.shape
            y1.sum().backward()
    finally:
        engine.set_direct_grads(False)
        U.set_col_workspace_bytes(old)
    assert x0.grad.shape == x0.shape and x1.grad.shape == x1.shape
    assert all(p.grad is not None and p.grad.shape == p.shape for p in mods.parameters())
    if mode == 'bf16':
        with engine.precision(mode), pytest.raises(ValueError, match='multiples of 8'):
            U.Conv3x3(3, 8)(torch.randn(1, 3, 4, 4))


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_wrong_geometry_is_refused_before_any_launch(stubbed, mode):
    """the gathered rows are sized from the weight: an input with another channel count, or one that is not (B, C, H, W), gets the
    ValueError nn.Conv2d's own check would give -- in every module, before a kernel is launched -- and the launchers refuse rows that
    do not fit their buffers"""
    from multimae_amd import _lib, engine, ops
    launched = []
    stub = _lib._lib

    class Spy:
        def __getattr__(self, name):
            if name.startswith(('mmae_conv3x3', 'mmae_upsample2x', 'mmae_gemm')):
                launched.append(name)
            return getattr(stub, name)
    _lib._lib = Spy()
    try:
        rcu, ffb = build('c8')
        conv = U.Conv3x3(8, 16)
        scratch = U.make_scratch([8, 16, 8, 16], 16)
        with engine.precision(mode):
            for fn in (lambda: conv(torch.randn(2, 16, 3, 4)),            # more channels than the weight: the gather would overrun its rows
                       lambda: conv(torch.randn(2, 4, 3, 4)), lambda: conv(torch.randn(8, 3, 4)), lambda: conv(torch.randn(0, 8, 3, 4)),
                       lambda: scratch.layer2_rn(torch.randn(2, 8, 3, 4)),  # a wrong entry of in_shape
                       lambda: rcu(torch.randn(2, 16, 3, 4)), lambda: rcu(torch.randn(2, 8, 12)),
                       lambda: ffb(torch.randn(2, 16, 3, 4)), lambda: ffb(torch.randn(2, 8, 3, 4), torch.randn(2, 16, 3, 4)),
                       lambda: ffb(torch.randn(2, 8, 3, 4), torch.randn(2, 8, 4, 3)), lambda: ffb(torch.randn(2, 8, 3)),
                       lambda: U.Interpolate(2, 'bilinear', True)(torch.randn(8, 3, 4))):
                with pytest.raises(ValueError, match='shape'):
                    fn()
        assert launched == []
        x, small = torch.zeros(2, 3, 4, 8), torch.zeros(2 * 3 * 4 * 9 * 8 - 1)
        with pytest.raises(ValueError, match='gathered rows'):
            ops.conv3x3_im2col(x, small, 2, 3, 4, 8, 1, False)
        with pytest.raises(ValueError, match='gathered rows'):
            ops.conv3x3_im2col(x, torch.zeros(2 * 3 * 4 * 9 * 8), 2, 3, 4, 16, 1, False)
        with pytest.raises(ValueError, match='rows'):
            ops.conv3x3_col2im(small, None, None, torch.zeros(2, 3, 4, 8), 2, 3, 4, 8, 1)
        with pytest.raises(ValueError, match='rows'):
            ops.conv3x3_col2im(torch.zeros(2 * 3 * 4 * 72), x[:1], None, torch.zeros(2, 3, 4, 8), 2, 3, 4, 8, 1)
        assert launched == []
        ops.conv3x3_im2col(x, torch.zeros(2 * 3 * 4 * 72), 2, 3, 4, 8, 1, False)
        assert launched == ['mmae_conv3x3_im2col']
    finally:
        _lib._lib = stub


def test_header_declares_the_entry_points():
    from multimae_amd import _lib
    import ctypes
    I, V = ctypes.c_int, ctypes.c_void_p
    want = {'mmae_conv3x3_im2col': [V, V, I, I, I, I, I, I, I, V], 'mmae_conv3x3_col2im': [V, V, V, V, I, I, I, I, I, V],
            'mmae_conv3x3_weight_pack': [V, V, I, I, I, V], 'mmae_conv3x3_weight_unpack': [V, V, I, I, I, V],
            'mmae_upsample2x_fwd': [V, V, I, I, I, I, V], 'mmae_upsample2x_bwd': [V, V, I, I, I, I, V]}
    for name, args in want.items():
        assert name in _lib.declared_symbols() and _lib._PROTOS[name] == (I, args), name
