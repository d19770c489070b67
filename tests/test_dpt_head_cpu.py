"""CPU: DPTOutputAdapter with the regression head (multimae_amd/output_adapters.py; reference output_adapters.py:576-759) -- the
state-dict contract against the reference's seeded build (tests/golden/dpt_head_<case>.npz, make_golden_dpt.py), what the constructor
and forward refuse, the import through dropin/, the new entry points of the C ABI, and the host control flow of forward + backward
against the C ABI stub in both precisions and gradient modes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multimae_amd import output_adapters as OA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dpt_fixture as DF  # noqa: E402
from dpt_fixture import B, CASES, GEOM, UNUSED  # noqa: E402


# ------------------------------------------------------------------------------------------------------ state_dict --
@pytest.mark.parametrize('case', list(CASES))
def test_seeded_construction_reproduces_the_reference_state_dict(case):
    """keys, order, shapes and values bit for bit; the names the reference lists twice are the same tensors here too"""
    sd, ref = DF.seeded_head(case).state_dict(), DF.gold_sd(case)
    assert list(sd) == list(ref) and len(sd) == 82
    for k, v in ref.items():
        assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
        assert np.array_equal(sd[k].numpy(), v.numpy()), k
    assert sd['act_postprocess.0.1.weight'].data_ptr() == sd['act_1_postprocess.1.weight'].data_ptr()
    assert sd['scratch.layer_rn.3.weight'].data_ptr() == sd['scratch.layer4_rn.weight'].data_ptr()
    assert all(float(v.abs().min()) > 0 for k, v in ref.items() if k.endswith('bias'))


@pytest.mark.parametrize('case', list(CASES))
def test_load_state_dict_strict_of_the_reference_checkpoint(case):
    K, tasks, D, _ = CASES[case]
    torch.manual_seed(1)
    head = OA.DPTOutputAdapter(num_classes=K, main_tasks=tasks, dim_tokens_enc=D, **GEOM)       # init() through the constructor
    ref = DF.gold_sd(case)
    missing, unexpected = head.load_state_dict(ref, strict=True)
    assert not missing and not unexpected
    assert all(torch.equal(v, ref[k]) for k, v in head.state_dict().items())


def test_default_geometry_has_the_82_keys_of_the_reference():
    head = OA.DPTOutputAdapter(num_classes=3)
    assert not hasattr(head, 'act_postprocess') and head.dim_tokens_enc is None
    head.init(dim_tokens_enc=768)
    sd = head.state_dict()
    assert len(sd) == 82 and list(sd) == DF.gold('r1')['r1/keys'].tolist()
    assert list(sd)[:3] == ['scratch.layer1_rn.weight', 'scratch.layer2_rn.weight', 'scratch.layer3_rn.weight']
    assert [k for k in sd if k.startswith('head.')] == ['head.0.weight', 'head.0.bias', 'head.2.weight', 'head.2.bias', 'head.4.weight',
                                                        'head.4.bias']
    assert sd['head.0.weight'].shape == (128, 256, 3, 3) and sd['head.2.weight'].shape == (32, 128, 3, 3)
    assert sd['head.4.weight'].shape == (3, 32, 1, 1) and sd['act_4_postprocess.1.weight'].shape == (768, 768, 3, 3)
    assert (head.num_channels, head.stride_level, head.patch_size, head.main_tasks, head.hooks, head.layer_dims, head.feature_dim,
            head.dim_tokens_enc, head.head_type, head.P_H, head.P_W) == (3, 1, (16, 16), ('rgb',), [2, 5, 8, 11], [96, 192, 384, 768],
                                                                           256, 768, 'regression', 16, 16)
    two = OA.DPTOutputAdapter(num_classes=1, main_tasks=('rgb', 'depth'), dim_tokens_enc=768, stride_level=2, some_extra_kwarg=1)
    assert two.dim_tokens_enc == 1536 and (two.P_H, two.P_W) == (8, 8) and two.act_1_postprocess[0].weight.shape == (96, 1536, 1, 1)


# ----------------------------------------------------------------------------------------------------------- raises --
def test_constructor_refuses_what_is_not_built():
    with pytest.raises(NotImplementedError, match='DPTOutputAdapter: num_classes = 150 > 16'):
        OA.DPTOutputAdapter(num_classes=150)
    with pytest.raises(NotImplementedError, match='DPTOutputAdapter: num_classes = 17'):
        OA.DPTOutputAdapter(num_classes=17)
    assert OA.DPTOutputAdapter(num_classes=16).head[4].weight.shape == (16, 32, 1, 1)
    assert OA.DPTOutputAdapter(num_classes=3).num_channels == 3
    with pytest.raises(NotImplementedError, match='DPTOutputAdapter: use_bn'):
        OA.DPTOutputAdapter(num_classes=3, use_bn=True)
    with pytest.raises(NotImplementedError, match="DPTOutputAdapter: head_type = 'semseg'"):
        OA.DPTOutputAdapter(num_classes=3, head_type='semseg')
    with pytest.raises(ValueError, match='DPTOutputAdapter: head_type must be "regression" or "semseg"'):
        OA.DPTOutputAdapter(num_classes=3, head_type='classification')


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


def test_forward_refuses_wrong_inputs_before_any_launch(stubbed):
    from multimae_amd import _lib, engine
    launched = []
    stub = _lib._lib

    class Spy:
        def __getattr__(self, name):
            launched.append(name)
            return getattr(stub, name)
    _lib._lib = Spy()
    try:
        K, tasks, D, (NH, NW) = CASES['r1']
        head = DF.seeded_head('r1')
        toks, info = DF.tokens('r1'), DF.case_info('r1')
        with engine.precision('fp32'):
            with pytest.raises(ValueError, match=r'DPTOutputAdapter: init\(dim_tokens_enc\)'):
                OA.DPTOutputAdapter(num_classes=1, **GEOM)(toks, info)
            with pytest.raises(ValueError, match='DPTOutputAdapter: encoder_tokens must list'):
                head(toks[:3], info)
            with pytest.raises(ValueError, match='DPTOutputAdapter: encoder_tokens must list'):
                head(toks[0], info)
            with pytest.raises(ValueError, match='DPTOutputAdapter: the main_tasks'):
                head(toks, DF.input_info(tasks, NH * NW - 1, 16 * NH, 16 * NW))
            with pytest.raises(ValueError, match='DPTOutputAdapter: encoder width 12'):
                head([t[..., :12].contiguous() for t in toks], info)
            with pytest.raises(ValueError, match='DPTOutputAdapter: the token grid N_H x N_W = 3 x 4 must be even'):
                head([torch.randn(B, 13, D) for _ in range(4)], DF.input_info(tasks, 12, 48, 64))
            with pytest.raises(ValueError, match='DPTOutputAdapter: the token grid N_H x N_W = 2 x 3 must be even'):
                head([torch.randn(B, 7, D) for _ in range(4)], DF.input_info(tasks, 6, 32, 48))
        odd = OA.DPTOutputAdapter(num_classes=1, hooks=[0, 1, 2, 3], layer_dims=[8, 16, 24, 36], feature_dim=16, dim_tokens_enc=16)
        with engine.precision('bf16'), pytest.raises(ValueError, match='DPTOutputAdapter: the bf16 gathers and GEMMs need channel counts'):
            odd(toks, info)
        assert launched == []
    finally:
        _lib._lib = stub


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match='no CPU'):
        DF.seeded_head('r1')(DF.tokens('r1'), DF.case_info('r1'))


# ---------------------------------------------------------------------------------------------- host control flow --
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('direct', [False, True])
def test_head_control_flow(stubbed, case, mode, direct):
    """forward + backward run the whole host code against the C ABI stub: the output is the (B, K, H, W) image, every parameter but
    the four of refinenet4.resConfUnit1 gets a gradient of its own shape, the four token gradients have the tokens' shape"""
    from multimae_amd import engine, output_adapter_utils as OU
    K, tasks, D, (NH, NW) = CASES[case]
    head = DF.seeded_head(case)
    if direct:
        engine.ParamArena(head)
    toks = [t.clone().requires_grad_(True) for t in DF.tokens(case)]
    old = OU.set_col_workspace_bytes(4096)                                # several chunks per convolution
    engine.set_direct_grads(direct)
    try:
        with engine.precision(mode):
            y = head(toks, DF.case_info(case))
            assert y.shape == (B, K, 16 * NH, 16 * NW) and y.dtype == torch.float32 and y.is_contiguous()
            assert type(y) is torch.Tensor and getattr(y, '_mmae_seg', None) is None
            y.sum().backward()
    finally:
        engine.set_direct_grads(False)
        OU.set_col_workspace_bytes(old)
    for t in toks:
        assert t.grad is not None and t.grad.shape == t.shape
    for n, p in head.named_parameters():
        if n in UNUSED and not direct:
            assert p.grad is None, n
        else:
            assert p.grad is not None and p.grad.shape == p.shape, n


def test_launcher_argument_checks(stubbed):
    from multimae_amd import ops
    x, w, b = torch.zeros(2, 3, 5, 32), torch.zeros(3, 32), torch.zeros(3)
    assert ops.dpt_tail_fwd(x, w, b).shape == (2, 3, 3, 5)
    dx, part = ops.dpt_tail_bwd(torch.zeros(2, 3, 3, 5), x, w)
    assert dx.shape == x.shape and part.shape == (1, 3 * 32 + 3)          # the stub answers 0 rows: one at least
    for fn in (lambda: ops.dpt_tail_fwd(torch.zeros(2, 3, 5, 6), torch.zeros(3, 6), b),
               lambda: ops.dpt_tail_fwd(torch.zeros(2, 3, 5, 68), torch.zeros(3, 68), b),
               lambda: ops.dpt_tail_fwd(x, torch.zeros(17, 32), torch.zeros(17)),
               lambda: ops.dpt_tail_fwd(x, torch.zeros(3, 16), b),
               lambda: ops.dpt_tail_fwd(x.permute(0, 2, 1, 3), w, b),
               lambda: ops.dpt_tail_fwd(x, w, b, out=torch.zeros(2, 3, 3, 4)),
               lambda: ops.dpt_tail_bwd(torch.zeros(2, 3, 5, 3), x, w),
               lambda: ops.dpt_tail_bwd(torch.zeros(2, 3, 3, 5), x, w, dx=torch.zeros(5)),
               lambda: ops.deconv_weight_pack(torch.zeros(8, 8, 4, 4), None, 2, torch.float32),
               lambda: ops.deconv_weight_pack(torch.zeros(8, 8, 2, 2), torch.zeros(7), 2, torch.float32),
               lambda: ops.deconv_weight_unpack(torch.zeros(32, 8), None, torch.zeros(8, 8, 2, 2), torch.zeros(8), 2, False),
               lambda: ops.deconv_weight_unpack(torch.zeros(31, 8), None, torch.zeros(8, 8, 2, 2), None, 2, False),
               lambda: ops.deconv_weight_unpack(None, torch.zeros(31), None, torch.zeros(8), 2, False)):
        with pytest.raises(ValueError):
            fn()
    wp, bp = ops.deconv_weight_pack(torch.zeros(8, 24, 2, 2), torch.zeros(24), 2, torch.bfloat16)
    assert wp.shape == (96, 8) and wp.dtype == torch.bfloat16 and bp.shape == (96,)


# --------------------------------------------------------------------------------------------------------- the C ABI --
def test_new_entry_points_of_the_library():
    """declared, exported, the version unchanged; the partial-row query answers on the host, and the tail refuses a geometry outside
    its limits before anything touches a device"""
    from multimae_amd import _lib
    lib = _lib.load()
    assert lib.mmae_abi_version() == 7
    I, V = ctypes.c_int, ctypes.c_void_p
    want = {'mmae_dpt_tail_fwd': [V, V, V, V, I, I, I, I, I, V], 'mmae_dpt_tail_bwd_nblk': [I, I, I],
            'mmae_dpt_tail_bwd': [V, V, V, V, V, I, I, I, I, I, V], 'mmae_deconv_weight_pack': [V, V, V, I, V, I, I, I, V],
            'mmae_deconv_weight_unpack': [V, V, V, V, I, I, I, I, V]}
    for name, args in want.items():
        assert name in _lib.declared_symbols() and _lib._PROTOS[name] == (I, args), name
        assert getattr(lib, name).argtypes == args
    for B_, H, W in ((1, 1, 1), (2, 5, 7), (3, 37, 29), (64, 256, 256)):
        n = lib.mmae_dpt_tail_bwd_nblk(B_, H, W)
        assert 1 <= n <= B_ * H * W
    assert lib.mmae_dpt_tail_bwd_nblk(3, 37, 29) >= 3                     # the GPU tests' largest map: several workgroups
    assert lib.mmae_dpt_tail_bwd_nblk(0, 4, 4) == 0
    EINVAL = -1                                                           # MMAE_EINVAL
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    for K, C in ((17, 32), (3, 6), (3, 68), (0, 32), (3, 0)):
        assert lib.mmae_dpt_tail_fwd(p, p, p, p, 1, 2, 2, C, K, None) == EINVAL, (K, C)
        assert b'dpt_tail_fwd' in lib.mmae_last_error()
        assert lib.mmae_dpt_tail_bwd(p, p, p, p, p, 1, 2, 2, C, K, None) == EINVAL, (K, C)
        assert b'dpt_tail_bwd' in lib.mmae_last_error()


def test_import_through_dropin(tmp_path):
    """the import line of run_finetuning_depth.py:39 resolves to the engine, and the depth recipe's adapter constructs"""
    (tmp_path / 'utils').mkdir()
    (tmp_path / 'utils' / '__init__.py').write_text('')
    (tmp_path / 'utils' / 'registry.py').write_text('_model_entrypoints = {}\n')
    code = (
        'import utils.registry\n'
        'from multimae.output_adapters import ConvNeXtAdapter, DPTOutputAdapter\n'
        'assert DPTOutputAdapter.__module__ == "multimae_amd.output_adapters"\n'
        'a = DPTOutputAdapter(num_classes=1, stride_level=1, patch_size=16, main_tasks=("rgb",))\n'
        'a.init(768)\n'
        'sd = a.state_dict()\n'
        'assert len(sd) == 82 and sd["act_postprocess.0.1.weight"].shape == (96, 96, 4, 4)\n'
        'assert sd["act_postprocess.1.1.weight"].shape == (192, 192, 2, 2) and sd["head.4.weight"].shape == (1, 32, 1, 1)\n'
        'print("ok")\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'dropin'), str(tmp_path)]))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr[-2000:]
