"""The dense 3 x 3 convolution and the RefineNet fusion block of the DPT head (multimae_amd/output_adapter_utils.py) at the head's
geometry for 224 x 224 images, feature_dim 256, B = 16: one convolution on the 56 x 56 and on the 112 x 112 map, one whole fusion block
28 -> 56, forward and forward + backward, in the engine's bf16 and fp32 modes -- beside the same blocks as eager PyTorch on the same
GPU (the tests' restatement, tests/fusion_oracle.py: channels-last, bf16 autocast and f32), which is the yardstick.  The convolution's
forward and backward are also timed piece by piece (gather kernels against GEMMs): that share decides whether an implicit-GEMM kernel
is worth writing.  Writes profiles/fusion_block_bench.json.

    python tools/bench_fusion.py [--rounds 20] [--calls 10] [--ratios-from LOG] [--out profiles/fusion_block_bench.json]

--ratios-from: the output of `pytest tests/test_fusion_blocks_gpu.py -s`, whose FUSION_RATIO lines (engine deviation from f64 against the
reference's own) are copied into the result.  Times: a device-event pair around `calls` back-to-back calls is one round; engine and eager alternate
round by round for `rounds` rounds after three warm-up rounds of the same shapes; the median and the range of the rounds are kept.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import multimae_amd as M  # noqa: E402
from multimae_amd import functions as Fn, ops, output_adapter_utils as OU  # noqa: E402
import fusion_oracle as FO  # noqa: E402

C, B = 256, 16
CL = torch.channels_last


def _rounds(fns, rounds, calls, warm=3):
    """{name: fn} -> {name: (median, min, max)} of ms per call: every variant is warmed up `warm` rounds, then the variants ALTERNATE for
    `rounds` rounds, each round one device-event pair around `calls` back-to-back calls of one variant"""
    for _ in range(warm):
        for fn in fns.values():
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in evs.items():
        t = sorted(a.elapsed_time(b) / calls for a, b in pairs)
        out[k] = (statistics.median(t), t[0], t[-1])
    return out


def _put(row, res):
    for k, (med, lo, hi) in res.items():
        row[k + '_ms'] = med
        row[k + '_ms_minmax'] = [lo, hi]


def _time(fn, a):
    return _rounds({'x': fn}, a.rounds, a.calls)['x'][0]


def _map(h, w, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(B, C, h, w, device='cuda', generator=g).contiguous(memory_format=CL)


def conv_rows(hw, a):
    """one biased 3 x 3 convolution C -> C on a hw x hw map"""
    x, gy = _map(hw, hw, 1).requires_grad_(True), _map(hw, hw, 2)
    gy16 = gy.to(torch.bfloat16)
    row = {'map': [hw, hw], 'B': B, 'C': C, 'gflop_fwd': 2.0 * B * hw * hw * 9 * C * C / 1e9}
    torch.manual_seed(0)
    conv = OU.Conv3x3(C, C).cuda()
    ref = nn.Conv2d(C, C, 3, padding=1).cuda().to(memory_format=CL)
    for mode in ('bf16', 'fp32'):
        def eager(t):
            if mode == 'bf16':
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    return ref(t)
            return ref(t)

        def eager_fwd():
            with torch.no_grad():
                eager(x)
        with M.engine.precision(mode):                                # engine and eager alternate round by round
            _put(row, _rounds({f'engine_{mode}_fwd': lambda: conv(x.detach()), f'eager_{mode}_fwd': eager_fwd}, a.rounds, a.calls))
            _put(row, _rounds({f'engine_{mode}_fwd_bwd': lambda: conv(x).backward(gy),
                               f'eager_{mode}_fwd_bwd': lambda: eager(x).backward(gy16 if mode == 'bf16' else gy)}, a.rounds, a.calls))
        # the pieces, on one chunk of the size the forward uses
        act = torch.bfloat16 if mode == 'bf16' else torch.float32
        xn, R1, K9 = x.detach().permute(0, 2, 3, 1), hw * hw, 9 * C
        esz = 2 if mode == 'bf16' else 4
        nb = Fn._col_rows(B, R1, K9, esz, OU.COL_WORKSPACE_BYTES[0])
        nb4 = Fn._col_rows(B, R1, K9, 4, OU.COL_WORKSPACE_BYTES[0])
        wp = ops.conv3x3_weight_pack(conv.weight.detach(), act)
        col = torch.empty((nb * R1, K9), device='cuda', dtype=act)
        y = torch.empty((nb * R1, C), device='cuda')
        dya = torch.randn(nb * R1, C, device='cuda').to(act)
        dcol = torch.empty((nb4 * R1, K9), device='cuda')
        dx = torch.empty((nb4, hw, hw, C), device='cuda')
        dwp = torch.empty((C, K9), device='cuda')
        per = lambda t, n: t * B / n                                  # a chunk's time scaled to the batch
        p = {'samples_per_chunk_fwd': nb, 'samples_per_chunk_bwd': nb4}
        p['im2col_ms'] = per(_time(lambda: ops.conv3x3_im2col(xn, col, nb, hw, hw, C, 1, False), a), nb)
        p['gemm_fwd_ms'] = per(_time(lambda: ops.gemm(col, wp, y, nb * R1, C, K9, lda=K9, ldb=K9, ldc=C, bias=conv.bias.detach()), a), nb)
        p['gemm_dw_ms'] = per(_time(lambda: ops.linear_dw(dya, col, dwp, False), a), nb)
        p['gemm_dx_ms'] = per(_time(lambda: ops.linear_dx(dya[:nb4 * R1], wp, dcol), a), nb4)
        p['col2im_ms'] = per(_time(lambda: ops.conv3x3_col2im(dcol, None, None, dx, nb4, hw, hw, C, 1), a), nb4)
        p['gather_share_fwd'] = p['im2col_ms'] / (p['im2col_ms'] + p['gemm_fwd_ms'])
        gather = 2 * p['im2col_ms'] + p['col2im_ms']                   # im2col runs again in the backward (col is not saved)
        p['gather_share_fwd_bwd'] = gather / (gather + p['gemm_fwd_ms'] + p['gemm_dw_ms'] + p['gemm_dx_ms'])
        row[f'pieces_{mode}'] = p
        del col, y, dya, dcol, dx
        torch.cuda.empty_cache()
    return row


def block_rows(hw, a):
    """one fusion block with two inputs: hw x hw -> 2 hw x 2 hw"""
    x0, x1 = _map(hw, hw, 3).requires_grad_(True), _map(hw, hw, 4).requires_grad_(True)
    gy = _map(2 * hw, 2 * hw, 5)
    gy16 = gy.to(torch.bfloat16)
    torch.manual_seed(0)
    blk = OU.make_fusion_block(C, False).cuda()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    row = {'map': [hw, hw], 'B': B, 'C': C, 'gflop_fwd': 2.0 * B * hw * hw * C * C * (4 * 9 + 4) / 1e9}
    for mode in ('bf16', 'fp32'):
        def eager(a, b):
            if mode == 'bf16':
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    return FO.fusion([a, b], sd)
            return FO.fusion([a, b], sd)

        def eager_fwd():
            with torch.no_grad():
                eager(x0, x1)
        with M.engine.precision(mode):
            _put(row, _rounds({f'engine_{mode}_fwd': lambda: blk(x0.detach(), x1.detach()), f'eager_{mode}_fwd': eager_fwd}, a.rounds, a.calls))
            _put(row, _rounds({f'engine_{mode}_fwd_bwd': lambda: blk(x0, x1).backward(gy),
                               f'eager_{mode}_fwd_bwd': lambda: eager(x0, x1).backward(gy16 if mode == 'bf16' else gy)}, a.rounds, a.calls))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--ratios-from', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fusion_block_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fusion.py measures on the GPU: no device found')
    res = {'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'calls_per_round': a.calls,
           'timing': 'device events around `calls_per_round` back-to-back calls; engine and eager alternate round by round after 3 warm-up rounds; *_ms = median over the rounds, *_ms_minmax = their range; pieces: median', 'col_workspace_bytes': OU.COL_WORKSPACE_BYTES[0],
           'yardstick': 'eager PyTorch on the same GPU, channels-last (nn.Conv2d; tests/fusion_oracle.py), bf16 autocast and f32',
           'conv3x3': {}, 'fusion_block': {}}
    for hw in (56, 112):
        res['conv3x3'][f'{hw}x{hw}'] = conv_rows(hw, a)
        print('conv3x3', hw, json.dumps(res['conv3x3'][f'{hw}x{hw}']), flush=True)
    res['fusion_block']['28->56'] = block_rows(28, a)
    print('fusion_block', json.dumps(res['fusion_block']['28->56']), flush=True)
    if a.ratios_from:
        rows = [json.loads(l.split('FUSION_RATIO ', 1)[1]) for l in open(a.ratios_from) if 'FUSION_RATIO ' in l]
        res['deviation_ratios'] = {'what': 'per tensor: max|engine - f64| / max|f64| against the same for the reference (f32; autocast bf16 in bf16 mode)',
                                   'allowed': {'fp32': 4.0, 'bf16': 2.0},
                                   'worst': {m: max(r['ratio'] for r in rows if r['mode'] == m and r['ratio'] is not None) for m in ('fp32', 'bf16')},
                                   'rows': rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
