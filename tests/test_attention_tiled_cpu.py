"""CPU: the host side of the tiled bf16 attention (sequences beyond 256 tokens) -- the C ABI declares and the built library exports
the two entry points, ops routes bf16 operands of any length to the fused kernels, and the encoder stack goes through the one-call
composite at a fine-tuning sequence length.  The C ABI is the type-checking stub of dryrun_harness, which here also records the
names it is asked for."""
import ctypes
import os

import pytest
import torch

import dryrun_harness
from dryrun_harness import RecordingLib

NEW = ('mmae_attn_fwd_tiled', 'mmae_attn_bwd_tiled')


@pytest.fixture()
def stub():
    from multimae_amd import _lib, ops
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    rec = RecordingLib()
    _lib._lib = rec
    yield rec
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()
    ops.set_fused_attention(True)
    ops.set_composite_blocks(True)
    ops.set_stack_composites(True)


def test_header_declares_and_library_exports_tiled_entry_points():
    from multimae_amd import _lib
    n_fwd = len(_lib._PROTOS['mmae_attn_fwd'][1])
    n_bwd = len(_lib._PROTOS['mmae_attn_bwd'][1])
    assert set(NEW) <= set(_lib.declared_symbols())
    assert len(_lib._PROTOS['mmae_attn_fwd_tiled'][1]) == n_fwd                     # same operands as the LDS-resident forward
    assert len(_lib._PROTOS['mmae_attn_bwd_tiled'][1]) == n_bwd + 1                 # + the delta scratch
    assert os.path.exists(_lib.LIB_PATH), 'libmmae_hip.so is not built'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), f'{name} is not exported'
    assert lib.mmae_abi_version() == 7


@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('N', [257, 1025, 3201])
def test_fusable_bf16_any_length(N, hd):
    from multimae_amd import ops
    from multimae_amd.ops import AttnView
    t = torch.empty(1, dtype=torch.bfloat16)
    assert ops._fusable(AttnView(t, 0, 8, N), AttnView(t, 0, 8, N), hd)
    assert ops._fusable(AttnView(t, 0, 8, 100), AttnView(t, 0, 8, N), hd)           # cross-attention: either side may be short
    assert ops._fusable(AttnView(t, 0, 8, N), AttnView(t, 0, 8, 100), hd)
    ops.set_fused_attention(False)
    try:
        assert not ops._fusable(AttnView(t, 0, 8, N), AttnView(t, 0, 8, N), hd)     # the A/B switch still selects the GEMM path
    finally:
        ops.set_fused_attention(True)


def test_fusable_unchanged_for_other_dtypes_and_widths():
    from multimae_amd import ops
    from multimae_amd.ops import AttnView
    for dt in (torch.float32, torch.float16):
        t = torch.empty(1, dtype=dt)
        for N in (257, 1025):
            for hd in (32, 64):
                assert not ops._fusable(AttnView(t, 0, 8, N), AttnView(t, 0, 8, N), hd), (dt, N, hd)
                assert not ops._fusable(AttnView(t, 0, 8, 64), AttnView(t, 0, 8, N), hd), (dt, N, hd)
    h = torch.empty(1, dtype=torch.float16)
    assert ops._fusable(AttnView(h, 0, 8, 256), AttnView(h, 0, 8, 256), 64)
    b = torch.empty(1, dtype=torch.bfloat16)
    for N in (64, 256, 257, 1025):
        assert not ops._fusable(AttnView(b, 0, 8, N), AttnView(b, 0, 8, N), 48)


def test_block_composite_ok_drops_the_limit_for_bf16_only(stub):
    from multimae_amd import ops
    x = torch.empty(4, 128)
    assert ops.block_composite_ok(x, torch.bfloat16, 2, 1025)
    assert ops.block_composite_ok(x, torch.bfloat16, 2, 256)
    assert not ops.block_composite_ok(x, torch.float32, 2, 257)
    assert not ops.block_composite_ok(x, torch.float16, 2, 257)
    assert not ops.block_composite_ok(x, torch.bfloat16, 1, 1025)                   # head_dim 128


def _attn_calls(rec, N):
    from multimae_amd import ops
    from multimae_amd.ops import AttnView
    B, H, hd = 1, 2, 64
    D = H * hd
    qkv = torch.zeros(B * N, 3 * D, dtype=torch.bfloat16)
    o, do, dqkv = torch.zeros(B * N, D, dtype=torch.bfloat16), torch.zeros(B * N, D, dtype=torch.bfloat16), torch.zeros_like(qkv)
    v = lambda t, c: AttnView(t, c, t.shape[1], N)
    rec.names.clear()
    st = ops.attention_fwd(v(qkv, 0), v(qkv, D), v(qkv, 2 * D), v(o, 0), B, H, hd, hd ** -0.5)
    assert st[0] == 'fused' and st[1].shape == (B, H, N)
    ops.attention_bwd(v(qkv, 0), v(qkv, D), v(qkv, 2 * D), st, v(o, 0), v(do, 0), v(dqkv, 0), v(dqkv, D), v(dqkv, 2 * D), B, H, hd, hd ** -0.5)
    return list(rec.names)


def test_dispatch_tiled_above_256_and_resident_at_256(stub):
    assert _attn_calls(stub, 300) == ['mmae_attn_fwd_tiled', 'mmae_attn_bwd_tiled']
    assert _attn_calls(stub, 256) == ['mmae_attn_fwd', 'mmae_attn_bwd']
    assert _attn_calls(stub, 257) == ['mmae_attn_fwd_tiled', 'mmae_attn_bwd_tiled']


def test_dropout_and_switch_keep_the_gemm_path(stub):
    from multimae_amd import ops
    from multimae_amd.ops import AttnView
    B, H, hd, N = 1, 2, 64, 300
    D = H * hd
    qkv = torch.zeros(B * N, 3 * D, dtype=torch.bfloat16)
    o = torch.zeros(B * N, D, dtype=torch.bfloat16)
    v = lambda t, c: AttnView(t, c, t.shape[1], N)
    stub.names.clear()
    st = ops.attention_fwd(v(qkv, 0), v(qkv, D), v(qkv, 2 * D), v(o, 0), B, H, hd, hd ** -0.5, drop_p=0.1)
    assert st[0] == 'gemm' and 'mmae_softmax_fwd' in stub.names and not set(NEW) & set(stub.names)
    ops.set_fused_attention(False)
    stub.names.clear()
    st = ops.attention_fwd(v(qkv, 0), v(qkv, D), v(qkv, 2 * D), v(o, 0), B, H, hd, hd ** -0.5)
    assert st[0] == 'gemm' and 'mmae_softmax_fwd' in stub.names and not set(NEW) & set(stub.names)


def test_encoder_stack_at_300_tokens_is_one_call_per_direction(stub):
    """A 2-block encoder stack at N = 300, bf16: forward + backward reach mmae_stack_fwd / mmae_stack_bwd and nothing per kernel."""
    import multimae_amd as M
    from multimae_amd.multimae_utils import Block, run_blocks
    blocks = torch.nn.ModuleList([Block(128, 2, qkv_bias=True) for _ in range(2)])
    x = torch.randn(2, 300, 128, requires_grad=True)
    stub.names.clear()
    with M.engine.precision('bf16'):
        y = run_blocks(blocks, x)
        y.sum().backward()
    names = list(stub.names)
    print('library calls:', names)
    assert names.count('mmae_stack_fwd') == 1 and names.count('mmae_stack_bwd') == 1, names
    per_kernel = [n for n in names if n in ('mmae_softmax_fwd', 'mmae_softmax_bwd', 'mmae_gemm', 'mmae_attn_fwd', 'mmae_attn_bwd', 'mmae_block_fwd',
                                            'mmae_block_bwd', 'mmae_layernorm_fwd', 'mmae_layernorm_bwd') or n in NEW]
    assert per_kernel == [], per_kernel
    assert x.grad is not None and x.grad.shape == x.shape
    for p in blocks.parameters():
        assert p.grad is not None and p.grad.shape == p.shape
