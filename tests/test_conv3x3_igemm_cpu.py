"""CPU: the implicit-GEMM 3 x 3 convolution's host side -- the C ABI of its three entry points, the eligibility rule
(ops.conv3x3_igemm_ok), what the wrappers refuse before a launch, the public switch (engine.set_conv3x3_impl) and the library calls a
residual unit makes under either setting, against the C ABI stub."""
import ctypes
import os
import re
import sys

import pytest
import torch
from torch import nn

from multimae_amd import _lib, engine, ops, output_adapter_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
BF = torch.bfloat16


def test_header_declares_the_entry_points():
    I, V = ctypes.c_int, ctypes.c_void_p
    want = {'mmae_conv3x3_igemm_fwd': [V, V, V, V, V, I, I, I, I, I, I, V], 'mmae_conv3x3_igemm_dgrad': [V, V, V, V, V, I, I, I, I, I, V],
            'mmae_conv3x3_weight_pack_t': [V, V, I, I, V]}
    for name, args in want.items():
        assert name in _lib.declared_symbols() and _lib._PROTOS[name] == (I, args), name


def test_tile_constants_match_the_kernel():
    src = open(os.path.join(ROOT, 'multimae_amd', 'csrc', 'conv3x3_igemm.hip')).read()
    m = re.search(r'constexpr int TH = (\d+), TW = (\d+);', src)
    assert m and (int(m.group(1)), int(m.group(2))) == ops.CONV3X3_IGEMM_TILE
    assert 'conv3x3_igemm.hip' in open(os.path.join(ROOT, 'multimae_amd', 'csrc', 'Makefile')).read()


def test_the_default_is_the_gather_path():
    assert engine.conv3x3_impl() == 'gather'
    engine.set_conv3x3_impl('implicit')
    try:
        assert engine.conv3x3_impl() == 'implicit'
        with pytest.raises(ValueError, match='gather'):
            engine.set_conv3x3_impl('winograd')
        assert engine.conv3x3_impl() == 'implicit'
    finally:
        engine.set_conv3x3_impl('gather')


def test_eligibility_rule():
    ok = ops.conv3x3_igemm_ok
    x = torch.zeros(2, 5, 7, 32)
    assert x.data_ptr() % 16 == 0
    assert ok(x, 32, 32, 1, BF) and ok(x, 32, 96, 1, BF) and ok(torch.zeros(1, 1, 1, 768), 768, 256, 1, BF)
    assert ok(torch.zeros(1, 4, 4, 256), 256, 128, 1, BF) and ok(torch.zeros(1, 4, 4, 128), 128, 32, 1, BF)
    assert not ok(x, 32, 32, 2, BF), 'stride 2'
    assert not ok(x, 32, 32, 1, torch.float32), 'the fp32 mode'
    assert not ok(torch.zeros(2, 5, 7, 8), 8, 8, 1, BF) and not ok(x, 32, 8, 1, BF) and not ok(x, 32, 48, 1, BF), 'channels off the grid of 32'
    assert not ok(torch.zeros(2, 5, 7, 16), 16, 32, 1, BF)
    assert not ok(x, 64, 32, 1, BF), 'a map with another channel count'
    off = torch.zeros(x.numel() + 1)[1:].view(x.shape)
    assert off.data_ptr() % 16 == 4 and not ok(off, 32, 32, 1, BF), 'a view 4 bytes off the 16-byte grid'
    assert not ok(torch.zeros(2, 5, 7, 64)[..., :32], 32, 32, 1, BF), 'a strided view'
    assert not ok(x.double(), 32, 32, 1, BF) and not ok(torch.zeros(0, 5, 7, 32), 32, 32, 1, BF)


@pytest.fixture()
def stubbed():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    rec = dryrun_harness.RecordingLib()
    _lib._lib = rec
    yield rec
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()
    from multimae_amd import functions
    functions.ops._require_gpu = ops._require_gpu


def test_wrappers_refuse_before_any_launch(stubbed):
    B, h, w, Ci, Co = 2, 3, 4, 32, 64
    x, y = torch.zeros(B, h, w, Ci), torch.zeros(B, h, w, Co)
    wp, bias = torch.zeros(Co, 9 * Ci, dtype=BF), torch.zeros(Co)
    bad_fwd = [
        lambda: ops.conv3x3_igemm_fwd(x, wp, bias, None, y, B, h, w, Ci + 32, Co, False),                    # a map shorter than the geometry
        lambda: ops.conv3x3_igemm_fwd(x, wp, bias, None, torch.zeros(B * h * w * Co - 1), B, h, w, Ci, Co, False),
        lambda: ops.conv3x3_igemm_fwd(x, wp[:-1], bias, None, y, B, h, w, Ci, Co, False),
        lambda: ops.conv3x3_igemm_fwd(x, wp, bias[:-1], None, y, B, h, w, Ci, Co, False),
        lambda: ops.conv3x3_igemm_fwd(x, wp, bias, y[:1], y, B, h, w, Ci, Co, False),                        # a short residual
        lambda: ops.conv3x3_igemm_fwd(x, wp.float(), bias, None, y, B, h, w, Ci, Co, False),
        lambda: ops.conv3x3_igemm_fwd(x.double(), wp, bias, None, y, B, h, w, Ci, Co, False),
        lambda: ops.conv3x3_igemm_fwd(torch.zeros(B, h, w, 8), torch.zeros(Co, 72, dtype=BF), bias, None, y, B, h, w, 8, Co, False),
        lambda: ops.conv3x3_igemm_fwd(torch.zeros(x.numel() + 1)[1:].view(x.shape), wp, bias, None, y, B, h, w, Ci, Co, False),
        lambda: ops.conv3x3_igemm_fwd(torch.zeros(B, h, w, 2 * Ci)[..., :Ci], wp, bias, None, y, B, h, w, Ci, Co, False),
    ]
    dy, dx, wpt = y, torch.zeros(B, h, w, Ci), torch.zeros(Ci, 9 * Co, dtype=BF)
    bad_dgrad = [
        lambda: ops.conv3x3_igemm_dgrad(dy, wpt, None, None, torch.zeros(B * h * w * Ci - 1), B, h, w, Co, Ci),
        lambda: ops.conv3x3_igemm_dgrad(dy[:1], wpt, None, None, dx, B, h, w, Co, Ci),
        lambda: ops.conv3x3_igemm_dgrad(dy, wpt, x[:1], None, dx, B, h, w, Co, Ci),                          # a short mask
        lambda: ops.conv3x3_igemm_dgrad(dy, wpt, None, x[:1], dx, B, h, w, Co, Ci),                          # a short addend
        lambda: ops.conv3x3_igemm_dgrad(dy, wpt[:-1], None, None, dx, B, h, w, Co, Ci),
        lambda: ops.conv3x3_igemm_dgrad(dy, wpt, None, torch.zeros(x.numel() + 1)[1:].view(x.shape), dx, B, h, w, Co, Ci),
    ]
    bad_pack = [lambda: ops.conv3x3_weight_pack_t(wp.float()), lambda: ops.conv3x3_weight_pack_t(torch.zeros(Co, 9 * Ci + 1, dtype=BF)),
                lambda: ops.conv3x3_weight_pack_t(torch.zeros(Co * 9 * Ci, dtype=BF)),
                lambda: ops.conv3x3_weight_pack_t(torch.zeros(Co, 18 * Ci, dtype=BF)[:, ::2])]
    for fn in bad_fwd + bad_dgrad + bad_pack:
        with pytest.raises(ValueError, match='conv3x3_'):
            fn()
    assert stubbed.calls == []
    ops.conv3x3_igemm_fwd(x, wp, bias, y, y.clone(), B, h, w, Ci, Co, True)
    ops.conv3x3_igemm_dgrad(dy, wpt, x, x, dx, B, h, w, Co, Ci)
    assert ops.conv3x3_weight_pack_t(wp).shape == (Ci, 9 * Co)
    assert [n for n, _ in stubbed.calls] == ['mmae_conv3x3_igemm_fwd', 'mmae_conv3x3_igemm_dgrad', 'mmae_conv3x3_weight_pack_t']
    assert stubbed.calls[0][1] == ['ptr', 'ptr', 'ptr', 'ptr', 'ptr', B, h, w, Ci, Co, 1, 'NULL']
    assert stubbed.calls[1][1] == ['ptr', 'ptr', 'ptr', 'ptr', 'ptr', B, h, w, Co, Ci, 'NULL']
    assert stubbed.calls[2][1] == ['ptr', 'ptr', Co, Ci, 'NULL']


CONV = ('mmae_conv3x3_igemm_fwd', 'mmae_conv3x3_igemm_dgrad', 'mmae_conv3x3_weight_pack_t', 'mmae_conv3x3_im2col', 'mmae_conv3x3_col2im',
        'mmae_conv3x3_weight_pack', 'mmae_conv3x3_weight_unpack')


def _rcu_calls(rec, which, C, B=4, h=3, w=4, chunks=2):
    """the library calls of one forward + backward of ResidualConvUnit_custom(C) with the batch in `chunks` chunks of gathered rows"""
    torch.manual_seed(0)
    rcu = U.ResidualConvUnit_custom(C, nn.ReLU(False), False)
    old_cap = U.set_col_workspace_bytes((B // chunks) * h * w * 9 * C * 4)       # B / chunks samples of f32 rows per chunk
    engine.set_conv3x3_impl(which)
    try:
        with engine.precision('bf16'):
            x = torch.randn(B, C, h, w, requires_grad=True)
            del rec.calls[:]
            y = rcu(x)
            n_fwd = len(rec.calls)
            y.sum().backward()
    finally:
        engine.set_conv3x3_impl('gather')
        U.set_col_workspace_bytes(old_cap)
    assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in rcu.parameters())
    names = [n for n, _ in rec.calls]
    return names[:n_fwd], names[n_fwd:]


def _is_gemm(n):
    return n == 'mmae_gemm'                                          # every product of the path: forward, dY x W (linear_dx), dY^T x col (linear_dw)


def test_residual_unit_calls_under_implicit(stubbed):
    """eligible (32 channels): two igemm_fwd; two weight_pack_t and two igemm_dgrad; per convolution one im2col + one weight-gradient
    product per chunk; no col2im, and no GEMM in the forward"""
    fwd, bwd = _rcu_calls(stubbed, 'implicit', 32)
    assert [n for n in fwd if n in CONV] == ['mmae_conv3x3_weight_pack'] * 2 + ['mmae_conv3x3_igemm_fwd'] * 2
    assert not any(_is_gemm(n) for n in fwd)
    conv = [n for n in bwd if n in CONV]
    per_conv = ['mmae_conv3x3_weight_pack_t', 'mmae_conv3x3_igemm_dgrad'] + ['mmae_conv3x3_im2col'] * 2 + ['mmae_conv3x3_weight_unpack']
    assert conv == per_conv * 2
    assert 'mmae_conv3x3_col2im' not in bwd
    # the weight-gradient products: the same calls the gather path makes for them, one per chunk and convolution
    g_fwd, g_bwd = _rcu_calls(stubbed, 'gather', 32)
    dw_of = lambda names: [tuple(names[i + 1:i + 3]) for i, n in enumerate(names) if n == 'mmae_conv3x3_im2col']
    assert dw_of(bwd) == [('mmae_gemm_plan', 'mmae_gemm')] * 4 and dw_of(bwd) == dw_of(g_bwd)
    # of the gather path's products the backward keeps exactly those four: its dY x W products (one per chunk and convolution) are gone
    gemms = lambda names: sum(_is_gemm(n) for n in names)
    assert gemms(bwd) == 4 and gemms(g_bwd) == 8
    rest = lambda names: [n for n in names if n not in CONV and not n.startswith('mmae_gemm')]
    assert rest(bwd) == rest(g_bwd)                                  # casts and bias sums: unchanged


def _gather_sequence(rec, C):
    fwd, bwd = _rcu_calls(rec, 'gather', C)
    assert not any('igemm' in n or n == 'mmae_conv3x3_weight_pack_t' for n in fwd + bwd)
    assert [n for n in fwd if n in CONV] == ['mmae_conv3x3_weight_pack'] * 2 + ['mmae_conv3x3_im2col'] * 2         # bf16 rows: one chunk each
    per_conv = ['mmae_conv3x3_im2col', 'mmae_conv3x3_col2im'] * 2 + ['mmae_conv3x3_weight_unpack']
    assert [n for n in bwd if n in CONV] == per_conv * 2
    return fwd, bwd


def test_residual_unit_calls_under_gather(stubbed):
    """the default makes the gather path's sequence, and an ineligible unit (8 channels) makes exactly the same calls, with the same
    arguments, under either setting"""
    _gather_sequence(stubbed, 32)
    _gather_sequence(stubbed, 8)
    _rcu_calls(stubbed, 'gather', 8)
    a = list(stubbed.calls)
    _rcu_calls(stubbed, 'implicit', 8)
    assert stubbed.calls == a
