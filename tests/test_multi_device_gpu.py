"""GPU: one process, two devices.  A kernel's dynamic-LDS limit belongs to the kernel ON A DEVICE, so the opt-in every launch above 64 KiB
needs has to happen on each device the process launches on (csrc/common.h, mmae_launch_lds)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pingpong_product(dev):
    """the smallest product the planner gives the ping-pong kernel (132 KiB of LDS): M = 2048, N = 256, K = 128, bf16 operands, f32 C"""
    from multimae_amd import ops
    M, N, K = 2048, 256, 128
    g = torch.Generator().manual_seed(1)
    A = torch.randn(M, K, generator=g).to(dev, torch.bfloat16)
    B = torch.randn(N, K, generator=g).to(dev, torch.bfloat16)
    C = torch.full((M, N), float('nan'), device=dev)
    ops.gemm(A, B, C, M, N, K, lda=K, ldb=K, ldc=N)
    return [C]


def _fused_attention(dev):
    """mmae_attn_fwd / mmae_attn_bwd, B = 1, H = 2, N = 64, head_dim 64, bf16: o, lse, dq, dk, dv"""
    from multimae_amd import _lib, ops
    lib = _lib.load()
    B, H, N, hd = 1, 2, 64, 64
    D = H * hd
    g = torch.Generator().manual_seed(2)
    q, k, v, do = (torch.randn(B * N, D, generator=g).to(dev, torch.bfloat16) for _ in range(4))
    o, dq, dk, dv = (torch.full((B * N, D), float('nan'), device=dev, dtype=torch.bfloat16) for _ in range(4))
    lse = torch.full((B, H, N), float('nan'), device=dev)
    sb, sc = N * D, hd ** -0.5
    _lib.check(lib.mmae_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, N, N, hd,
                                 sb, D, sb, D, sb, D, sb, D, sc, ops._stream()), 'attn_fwd')
    _lib.check(lib.mmae_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                 dk.data_ptr(), dv.data_ptr(), B, H, N, N, hd, sb, D, sb, D, sb, D, sb, D, sb, D, sb, D, sb, D, sc,
                                 ops._stream()), 'attn_bwd')
    return [o, lse, dq, dk, dv]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two devices')
def test_dynamic_lds_kernels_run_on_a_second_device():
    """device 0, then device 1, in this one process: the same calls must succeed on both and give the same bits (same inputs, same
    kernels, no atomics)"""
    results = []
    for d in (0, 1):
        with torch.cuda.device(d):
            outs = _pingpong_product(f'cuda:{d}') + _fused_attention(f'cuda:{d}')
            torch.cuda.synchronize()
        results.append([t.cpu() for t in outs])
    names = ('gemm C', 'attention o', 'lse', 'dq', 'dk', 'dv')
    for name, r0, r1 in zip(names, *results):
        assert torch.isfinite(r0.float()).all(), f'{name}: device 0 left its output unwritten'
        assert torch.equal(r0.view(torch.int32 if r0.element_size() == 4 else torch.int16),
                           r1.view(torch.int32 if r1.element_size() == 4 else torch.int16)), f'{name}: device 1 differs from device 0'
