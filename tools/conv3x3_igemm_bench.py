"""The implicit-GEMM 3 x 3 convolution (csrc/conv3x3_igemm.hip, engine.set_conv3x3_impl('implicit')) against the gather path it can
replace (im2col + GEMM, the default) and against eager PyTorch (channels-last nn.Conv2d under bf16 autocast), three sides in one process:

    conv     one biased convolution, forward and forward + backward: 256 -> 256 at B = 16 on 56 x 56 and 112 x 112 (the shapes of
             profiles/fusion_block_bench.json) and the DPT head's two convolutions at the depth recipe's geometry, B = 64: 256 -> 128 on
             128 x 128 and 128 -> 32 on 256 x 256; FLOP and the least bytes the shapes need, what the implicit side achieves of each,
             and which of the two bounds it
    block    one fusion block 28 -> 56, 256 channels, B = 16
    head     the whole DPT head at tools/dpt_head_bench.py's geometry, forward and forward + backward, and the peak memory of a
             forward + backward under either setting
    step     the whole fine-tuning step of tools/dpt_head_bench.py with the switch off and on

    python tools/conv3x3_igemm_bench.py [--rounds 20] [--calls 5] [--batch 64] [--parts conv,block,head,step] [--out profiles/conv3x3_igemm_bench.json]

Times: a device-event pair around `calls` back-to-back calls is one round; after three warm-up rounds the sides ALTERNATE round by round
for `rounds` rounds; the median and the min-max range of each side's rounds are kept.  A difference between two sides counts only
where it exceeds the range of the rounds of one side ('verdict').  An existing result file is updated part by part."""
import argparse
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import multimae_amd as M  # noqa: E402
from multimae_amd import engine, output_adapter_utils as OU  # noqa: E402
import fusion_oracle as FO  # noqa: E402
import dpt_head_bench as HB  # noqa: E402

CL = torch.channels_last
PEAK_FLOPS = 2.5e15          # dense bf16 MFMA peak of the MI355X
PEAK_BYTES = 6.0e12          # HBM bandwidth a streaming kernel reaches on it
SHAPES = [(16, 56, 56, 256, 256), (16, 112, 112, 256, 256), (64, 128, 128, 256, 128), (64, 256, 256, 128, 32)]


def _side(which, fn):
    def run():
        engine.set_conv3x3_impl(which)
        try:
            return fn()
        finally:
            engine.set_conv3x3_impl('gather')
    return run


def verdict(row, a, b, key):
    """a against b on row[...'_ms']: 'faster' / 'slower' only where the medians differ by more than the range of either side's rounds"""
    ma, mb = row[f'{a}_{key}_ms'], row[f'{b}_{key}_ms']
    spread = max(row[f'{a}_{key}_ms_minmax'][1] - row[f'{a}_{key}_ms_minmax'][0], row[f'{b}_{key}_ms_minmax'][1] - row[f'{b}_{key}_ms_minmax'][0])
    return 'level' if abs(ma - mb) <= spread else ('faster' if ma < mb else 'slower')


def _verdicts(row):
    row['verdict'] = {f'implicit_vs_{o}_{k}': verdict(row, 'implicit', o, k) for o in ('gather', 'eager') for k in ('fwd', 'fwd_bwd')
                      if f'{o}_{k}_ms' in row}


def _map(B, C, h, w, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(B, C, h, w, device='cuda', generator=g).contiguous(memory_format=CL)


def part_conv(a, res):
    for B, h, w, Cin, Cout in SHAPES:
        x, gy = _map(B, Cin, h, w, 1).requires_grad_(True), _map(B, Cout, h, w, 2)
        gy16 = gy.to(torch.bfloat16)
        torch.manual_seed(0)
        conv = OU.Conv3x3(Cin, Cout).cuda()
        ref = nn.Conv2d(Cin, Cout, 3, padding=1).cuda().to(memory_format=CL)
        pix = B * h * w
        flop = 2.0 * pix * 9 * Cin * Cout
        byt = 4.0 * pix * (Cin + Cout) + 2.0 * 9 * Cin * Cout                  # x read and y written once (f32), the bf16 weight
        row = {'B': B, 'map': [h, w], 'Cin': Cin, 'Cout': Cout, 'gflop_fwd': flop / 1e9, 'mbytes_fwd': byt / 1e6,
               'gflop_fwd_bwd': 3 * flop / 1e9, 'mbytes_fwd_bwd': (3 * byt + 4.0 * 9 * Cin * Cout) / 1e6,
               'note_fwd_bwd_bytes': 'forward, data gradient and weight gradient each reading and writing their maps once; under '
                                     "'implicit' the weight gradient still gathers 9 Cin wide bf16 rows on top of that"}

        def eager(t):
            with torch.autocast('cuda', dtype=torch.bfloat16):
                return ref(t)

        def eager_fwd():
            with torch.no_grad():
                eager(x)
        with M.engine.precision('bf16'):
            HB._put(row, HB._rounds({'implicit_fwd': _side('implicit', lambda: conv(x.detach())), 'gather_fwd': _side('gather', lambda: conv(x.detach())),
                                     'eager_fwd': eager_fwd}, a.rounds, a.calls))
            HB._put(row, HB._rounds({'implicit_fwd_bwd': _side('implicit', lambda: conv(x).backward(gy)),
                                     'gather_fwd_bwd': _side('gather', lambda: conv(x).backward(gy)),
                                     'eager_fwd_bwd': lambda: eager(x).backward(gy16)}, a.rounds, a.calls))
        for k, f, m in (('fwd', flop, byt), ('fwd_bwd', 3 * flop, 3 * byt)):
            t = row[f'implicit_{k}_ms'] / 1e3
            row[f'implicit_{k}_tflops'], row[f'implicit_{k}_gbs'] = f / t / 1e12, m / t / 1e9
            row[f'implicit_{k}_of_peak'] = {'flop': f / t / PEAK_FLOPS, 'bytes': m / t / PEAK_BYTES}
            row[f'bound_{k}'] = 'compute' if f / PEAK_FLOPS > m / PEAK_BYTES else 'memory'
            row[f'floor_{k}_ms'] = max(f / PEAK_FLOPS, m / PEAK_BYTES) * 1e3
        _verdicts(row)
        print('conv', json.dumps(row), flush=True)
        res.setdefault('conv3x3', {})[f'B{B}_{h}x{w}_{Cin}to{Cout}'] = row
        del x, gy, gy16, conv, ref
        torch.cuda.empty_cache()


def part_block(a, res):
    B, C, hw = 16, 256, 28
    x0, x1 = _map(B, C, hw, hw, 3).requires_grad_(True), _map(B, C, hw, hw, 4).requires_grad_(True)
    gy = _map(B, C, 2 * hw, 2 * hw, 5)
    gy16 = gy.to(torch.bfloat16)
    torch.manual_seed(0)
    blk = OU.make_fusion_block(C, False).cuda()
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in blk.state_dict().items()}
    row = {'map': [hw, hw], 'B': B, 'C': C, 'gflop_fwd': 2.0 * B * hw * hw * C * C * (4 * 9 + 4) / 1e9}

    def eager(p, q):
        with torch.autocast('cuda', dtype=torch.bfloat16):
            return FO.fusion([p, q], sd)

    def eager_fwd():
        with torch.no_grad():
            eager(x0, x1)
    with M.engine.precision('bf16'):
        fwd = lambda: blk(x0.detach(), x1.detach())
        both = lambda: blk(x0, x1).backward(gy)
        HB._put(row, HB._rounds({'implicit_fwd': _side('implicit', fwd), 'gather_fwd': _side('gather', fwd), 'eager_fwd': eager_fwd}, a.rounds, a.calls))
        HB._put(row, HB._rounds({'implicit_fwd_bwd': _side('implicit', both), 'gather_fwd_bwd': _side('gather', both),
                                 'eager_fwd_bwd': lambda: eager(x0, x1).backward(gy16)}, a.rounds, a.calls))
    _verdicts(row)
    print('block', json.dumps(row), flush=True)
    res.setdefault('fusion_block', {})['28->56'] = row


def part_head(a, res):
    K, B = 1, a.batch
    head = HB._head(K)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in head.state_dict().items()}
    toks = HB._tokens(B)
    full = [None] * (max(HB.HOOKS) + 1)
    for h, t in zip(HB.HOOKS, toks):
        full[h] = t
    gy = torch.randn(B, K, HB.IMG, HB.IMG, device='cuda')
    row = {'B': B, 'K': K}

    def eager(ts):
        with torch.autocast('cuda', dtype=torch.bfloat16):
            return HB.eager_head(ts, sd, HB.NH, HB.NW).float()

    def eager_fwd():
        with torch.no_grad():
            eager(toks)

    def engine_fwd():
        with torch.no_grad():
            head(full, HB.info(B))
    both = lambda: head(full, HB.info(B)).backward(gy)
    with M.engine.precision('bf16'):
        HB._put(row, HB._rounds({'implicit_fwd': _side('implicit', engine_fwd), 'gather_fwd': _side('gather', engine_fwd), 'eager_fwd': eager_fwd},
                                a.rounds, a.calls))
        HB._put(row, HB._rounds({'implicit_fwd_bwd': _side('implicit', both), 'gather_fwd_bwd': _side('gather', both),
                                 'eager_fwd_bwd': lambda: eager(toks).backward(gy)}, a.rounds, a.calls))
        for which in ('gather', 'implicit'):                          # peak memory of one forward + backward above what is resident before it
            for p in head.parameters():
                p.grad = None
            for t in toks:
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            _side(which, both)()
            torch.cuda.synchronize()
            row[f'{which}_fwd_bwd_peak_mb'] = (torch.cuda.max_memory_allocated() - base) / 1e6
    _verdicts(row)
    print('head', json.dumps(row), flush=True)
    res.setdefault('head', {})[f'K={K}'] = row
    del head, sd, toks, full
    torch.cuda.empty_cache()


def part_step(a, res):
    """tools/dpt_head_bench.py's fine-tuning step (MultiViT-B + DPT head + berHu + depth_metrics + fused AdamW) under either setting"""
    from multimae_amd import output_adapters as OA
    from multimae_amd.multimae import multivit_base
    from multimae_amd.optim import FusedAdamW
    B, IMG, P = a.batch, HB.IMG, HB.P
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(B, 3, IMG, IMG, device='cuda', generator=g)
    target = torch.randn(B, 1, IMG, IMG, device='cuda', generator=g)
    mask = torch.rand(B, 1, IMG, IMG, device='cuda', generator=g) > 0.1
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=P, image_size=IMG)}
    outs = {'depth': OA.DPTOutputAdapter(num_classes=1, stride_level=1, patch_size=P, main_tasks=('rgb',), hooks=HB.HOOKS)}
    model = multivit_base(input_adapters=ins, output_adapters=outs, num_global_tokens=1).cuda()
    model.build_arena()
    opt = FusedAdamW(model, lr=1e-4, weight_decay=0.05)

    def step():
        opt.zero_grad()
        y = model({'rgb': x}, return_all_layers=True)['depth']
        loss = M.masked_berhu_loss(y, target, mask)
        loss.backward()
        M.depth_metrics(y.detach(), target, mask)
        opt.step(loss)
    row = {'B': B}
    with M.engine.precision('bf16'):
        HB._put(row, HB._rounds({'implicit_step': _side('implicit', step), 'gather_step': _side('gather', step)}, a.rounds, a.calls))
    row['verdict'] = {'implicit_vs_gather_step': verdict(row, 'implicit', 'gather', 'step')}
    print('step', json.dumps(row), flush=True)
    res['finetuning_step_bf16'] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--parts', default='conv,block,head,step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv3x3_igemm_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('conv3x3_igemm_bench.py measures on the GPU: no device found')
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.update({'device': torch.cuda.get_device_name(),
                'sides': {'implicit': "engine.set_conv3x3_impl('implicit'): csrc/conv3x3_igemm.hip for forward and data gradient",
                          'gather': "engine.set_conv3x3_impl('gather'), the default: im2col + GEMM, GEMM + col2im",
                          'eager': 'eager PyTorch on the same GPU, channels-last, bf16 autocast'},
                'timing': 'device events around `calls` back-to-back calls; the sides alternate round by round after 3 warm-up rounds; *_ms = median '
                          'over the rounds, *_ms_minmax = their range; verdict: faster / slower only where the medians differ by more than the '
                          'range of either side, level otherwise',
                'peaks': {'flops': PEAK_FLOPS, 'bytes_per_s': PEAK_BYTES}, 'col_workspace_bytes': OU.COL_WORKSPACE_BYTES[0]})
    for p in [p for p in a.parts.split(',') if p]:
        res.setdefault('runs', {})[p] = {'batch': a.batch, 'rounds': a.rounds, 'calls_per_round': a.calls}
        {'conv': part_conv, 'block': part_block, 'head': part_head, 'step': part_step}[p](a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
