"""DPTOutputAdapter (multimae_amd/output_adapters.py) at the depth recipe's geometry -- ViT-B width 768, hooks [2, 5, 8, 11],
256 x 256 images, K = 1 (depth) and K = 3 (Taskonomy normals) -- beside an eager PyTorch restatement of the same head on the same GPU
(channels-last, bf16 autocast and f32), which is the yardstick.  Writes profiles/dpt_head_bench.json.

    python tools/dpt_head_bench.py [--batch 64] [--rounds 20] [--calls 10] [--parts head,stages,tail,step] [--modes bf16,fp32]
                                   [--ratios-from LOG] [--out profiles/dpt_head_bench.json]

parts:  head    the head alone, forward and forward + backward, engine against eager
        stages  the engine's ten autograd nodes one by one, forward + backward: reassemble x 4, fusion x 4, the head node; and the
                head node's two convolutions without the tail
        tail    mmae_dpt_tail_fwd / _bwd against the route they replace.  Forward: ReLU + cast, a GEMM into an 8-padded row, a
                transposing copy.  Backward: dY x W, the ReLU mask, dY^T x rows + bias column sum -- the saved bf16 rows, the mask and
                the transposed, padded bf16 gradient are prepared outside the timed region
        step    the whole fine-tuning step -- MultiViT-B + head + berHu + depth_metrics + fused AdamW -- with the DPT head and with
                a ConvNeXt head (embed_dim 6144, preds_per_patch 16, depth 4)
--ratios-from: the output of `pytest tests/test_dpt_head_gpu.py -s`, whose DPT_RATIO lines are copied into the result.
Times: a device-event pair around `calls` back-to-back calls is one round; the variants of a row alternate round by round for `rounds`
rounds after three warm-up rounds; the median and the range of the rounds are kept.  An existing result file is updated part by part.
"""
import argparse
import json
import os
import re
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import multimae_amd as M  # noqa: E402
from multimae_amd import functions as Fn, ops, output_adapter_utils as OU, output_adapters as OA  # noqa: E402
from multimae_amd.optim import FusedAdamW  # noqa: E402
import fusion_oracle as FO  # noqa: E402

D, HOOKS, IMG, P = 768, [2, 5, 8, 11], 256, 16
NH = NW = IMG // P
CL = torch.channels_last


def _rounds(fns, rounds, calls, warm=3):
    """{name: fn} -> {name: (median, min, max)} ms per call; the variants alternate round by round after `warm` warm-up rounds"""
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


def info(B):
    return {'tasks': {'rgb': {'num_tokens': NH * NW, 'has_2d_posemb': True, 'start_idx': 0, 'end_idx': NH * NW}}, 'image_size': (IMG, IMG),
            'num_task_tokens': NH * NW, 'num_global_tokens': 1}


def eager_head(toks, sd, nh, nw):
    """the reference's DPTOutputAdapter.forward (output_adapters.py:728-759) for main_tasks=('rgb',) as functions of a state dict"""
    maps = []
    for i, t in enumerate(toks):
        x = t[:, :nh * nw].transpose(1, 2).reshape(t.shape[0], -1, nh, nw).contiguous(memory_format=CL)
        pre = f'act_{i + 1}_postprocess.'
        x = F.conv2d(x, sd[pre + '0.weight'], sd[pre + '0.bias'])
        if i < 2:
            x = F.conv_transpose2d(x, sd[pre + '1.weight'], sd[pre + '1.bias'], stride=4 >> i)
        elif i == 3:
            x = F.conv2d(x, sd[pre + '1.weight'], sd[pre + '1.bias'], stride=2, padding=1)
        maps.append(F.conv2d(x, sd[f'scratch.layer{i + 1}_rn.weight'], None, padding=1))
    p = FO.fusion([maps[3]], sd, 'scratch.refinenet4.')
    p = FO.fusion([p, maps[2]], sd, 'scratch.refinenet3.')
    p = FO.fusion([p, maps[1]], sd, 'scratch.refinenet2.')
    p = FO.fusion([p, maps[0]], sd, 'scratch.refinenet1.')
    x = F.conv2d(p, sd['head.0.weight'], sd['head.0.bias'], padding=1)
    x = FO.upsample2x(x)
    x = F.conv2d(x, sd['head.2.weight'], sd['head.2.bias'], padding=1)
    return F.conv2d(F.relu(x), sd['head.4.weight'], sd['head.4.bias'])


def _head(K):
    torch.manual_seed(0)
    head = OA.DPTOutputAdapter(num_classes=K, stride_level=1, patch_size=P, main_tasks=('rgb',), hooks=HOOKS)
    head.init(D)
    return head.cuda()


def _tokens(B, grad=True):
    g = torch.Generator(device='cuda').manual_seed(1)
    return [torch.randn(B, NH * NW + 1, D, device='cuda', generator=g).requires_grad_(grad) for _ in range(4)]


def part_head(a, res):
    for K in (1, 3):
        head = _head(K)
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in head.state_dict().items()}
        toks = _tokens(a.batch)
        full = [None] * (max(HOOKS) + 1)
        for h, t in zip(HOOKS, toks):
            full[h] = t
        gy = torch.randn(a.batch, K, IMG, IMG, device='cuda')
        row = {'B': a.batch, 'K': K}
        for mode in a.modes:
            def eager(ts):
                if mode == 'bf16':
                    with torch.autocast('cuda', dtype=torch.bfloat16):
                        return eager_head(ts, sd, NH, NW).float()
                return eager_head(ts, sd, NH, NW)

            def eager_fwd():
                with torch.no_grad():
                    eager(toks)

            def engine_fwd():
                with torch.no_grad():
                    head(full, info(a.batch))
            with M.engine.precision(mode):
                _put(row, _rounds({f'engine_{mode}_fwd': engine_fwd, f'eager_{mode}_fwd': eager_fwd}, a.rounds, a.calls))
                _put(row, _rounds({f'engine_{mode}_fwd_bwd': lambda: head(full, info(a.batch)).backward(gy),
                                   f'eager_{mode}_fwd_bwd': lambda: eager(toks).backward(gy)}, a.rounds, a.calls))
            print('head', K, mode, json.dumps(row), flush=True)
        res.setdefault('head', {})[f'K={K}'] = row
        del head, sd, toks, full
        torch.cuda.empty_cache()


def part_stages(a, res):
    """every autograd node of the engine's head by itself, forward + backward, on inputs of the shapes it sees in the head"""
    head = _head(1)
    B = a.batch
    inf = info(B)
    for mode in a.modes:
        row = {'B': B}
        with M.engine.precision(mode):
            toks = _tokens(B)
            maps = []
            for i, t in enumerate(toks):
                cfg = OU._conv_cfg(head, layer=i, starts=[0], N=NH * NW, NH=NH, NW=NW)
                run = lambda i=i, t=t, cfg=cfg: Fn.DPTReassembleFn.apply(cfg, t, *head._layer_params(i))
                y = run().detach()
                maps.append(y)
                gy = torch.randn_like(y)
                _put(row, _rounds({f'reassemble_{i + 1}': lambda: run().backward(gy)}, a.rounds, a.calls))
            path = None
            for n in (4, 3, 2, 1):
                blk = getattr(head.scratch, f'refinenet{n}')
                xs = [maps[n - 1].requires_grad_(True)] if path is None else [path.requires_grad_(True), maps[n - 1].requires_grad_(True)]
                y = blk(*xs).detach()
                gy = torch.randn_like(y)
                _put(row, _rounds({f'refinenet{n}': lambda: blk(*xs).backward(gy)}, a.rounds, a.calls))
                path = y
            h = head.head
            params = [h[0].weight, h[0].bias, h[2].weight, h[2].bias, h[4].weight, h[4].bias]
            x = path.requires_grad_(True)
            gy = torch.randn(B, 1, IMG, IMG, device='cuda')
            _put(row, _rounds({'head_node': lambda: Fn.DPTHeadFn.apply(OU._conv_cfg(head), x, *params).backward(gy)}, a.rounds, a.calls))
            g32 = torch.randn(B, 32, IMG, IMG, device='cuda').contiguous(memory_format=CL)
            _put(row, _rounds({'head_convolutions': lambda: h[2](h[1](h[0](x))).backward(g32)}, a.rounds, a.calls))
        print('stages', mode, json.dumps(row), flush=True)
        res.setdefault('stages_fwd_bwd', {})[mode] = row
        del toks, maps, path, x
        torch.cuda.empty_cache()


def part_tail(a, res):
    B, C = a.batch, 32
    x = torch.randn(B, IMG, IMG, C, device='cuda')
    R = B * IMG * IMG
    for K in (1, 3):
        w, b = torch.randn(K, C, device='cuda'), torch.randn(K, device='cuda')
        g = torch.randn(B, K, IMG, IMG, device='cuda')
        w16 = w.bfloat16()
        logits = torch.empty(R, 8, device='cuda')

        def plain_fwd():
            xa = torch.relu(x).to(torch.bfloat16).view(R, C)
            ops.gemm(xa, w16, logits, R, K, C, lda=C, ldb=C, ldc=8, bias=b)
            return logits[:, :K].view(B, IMG, IMG, K).permute(0, 3, 1, 2).contiguous()

        # what the plain backward keeps from its forward (the ReLU'd bf16 rows) and the gradient as 8-padded bf16 rows are made
        # outside the timed region: timed are dY x W, the ReLU mask and dY^T x rows with the bias column sum
        xa_saved = torch.relu(x).to(torch.bfloat16).view(R, C)
        gp = torch.zeros(R, 8, device='cuda', dtype=torch.bfloat16)
        gp[:, :K] = g.permute(0, 2, 3, 1).reshape(R, K).to(torch.bfloat16)
        pos = x.view(R, C) > 0

        def plain_bwd():
            dx = ops.linear_dx(gp[:, :K], w16, torch.empty(R, C, device='cuda'))
            dx = dx * pos
            ops.linear_dw(gp[:, :K], xa_saved, torch.empty(K, C, device='cuda'), False, db=torch.empty(K, device='cuda'))
            return dx

        def kernel_bwd():
            dx, part = ops.dpt_tail_bwd(g, x, w)
            ops.reduce_partials(part, torch.empty(K * C + K, device='cuda'), False)
        row = {'B': B, 'K': K, 'C': C, 'map_mb': x.numel() * 4 / 1e6}
        _put(row, _rounds({'kernel_fwd': lambda: ops.dpt_tail_fwd(x, w, b), 'plain_route_fwd': plain_fwd}, a.rounds, a.calls))
        _put(row, _rounds({'kernel_bwd': kernel_bwd, 'plain_route_bwd': plain_bwd}, a.rounds, a.calls))
        row['kernel_fwd_gbs'] = (x.numel() + B * K * IMG * IMG) * 4 / row['kernel_fwd_ms'] / 1e6
        row['kernel_bwd_gbs'] = (2 * x.numel() + B * K * IMG * IMG) * 4 / row['kernel_bwd_ms'] / 1e6
        print('tail', K, json.dumps(row), flush=True)
        res.setdefault('tail', {})[f'K={K}'] = row


def part_step(a, res):
    """MultiViT-B, one rgb input, B x 256 x 256: forward, berHu, backward, depth_metrics, fused AdamW -- per head"""
    from multimae_amd.multimae import multivit_base
    B = a.batch
    g = torch.Generator(device='cuda').manual_seed(2)
    x = torch.randn(B, 3, IMG, IMG, device='cuda', generator=g)
    target = torch.randn(B, 1, IMG, IMG, device='cuda', generator=g)
    mask = torch.rand(B, 1, IMG, IMG, device='cuda', generator=g) > 0.1
    row = {'B': B}
    for name in ('dpt', 'convnext'):
        torch.manual_seed(0)
        ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=P, image_size=IMG)}
        if name == 'dpt':
            outs = {'depth': OA.DPTOutputAdapter(num_classes=1, stride_level=1, patch_size=P, main_tasks=('rgb',), hooks=HOOKS)}
        else:
            outs = {'depth': OA.ConvNeXtAdapter(num_classes=1, embed_dim=6144, preds_per_patch=16, main_tasks=('rgb',), patch_size=P, depth=4)}
        model = multivit_base(input_adapters=ins, output_adapters=outs, num_global_tokens=1).cuda()
        model.build_arena()
        opt = FusedAdamW(model, lr=1e-4, weight_decay=0.05)

        def step():
            opt.zero_grad()
            y = model({'rgb': x}, return_all_layers=(name == 'dpt'))['depth']
            loss = M.masked_berhu_loss(y, target, mask)
            loss.backward()
            M.depth_metrics(y.detach() if name == 'dpt' else y, target, mask)
            opt.step(loss)
        with M.engine.precision('bf16'):
            _put(row, _rounds({f'step_{name}': step}, a.rounds, a.calls))
        print('step', name, json.dumps(row), flush=True)
        del model, opt
        torch.cuda.empty_cache()
    res['finetuning_step_bf16'] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--parts', default='head,stages,tail,step')
    ap.add_argument('--modes', default='bf16,fp32')
    ap.add_argument('--ratios-from', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dpt_head_bench.json'))
    a = ap.parse_args()
    a.modes = a.modes.split(',')
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    parts = [p for p in a.parts.split(',') if p]
    if parts and not torch.cuda.is_available():
        raise SystemExit('dpt_head_bench.py measures on the GPU: no device found')
    if parts:
        res.update({'device': torch.cuda.get_device_name(), 'geometry': {'width': D, 'hooks': HOOKS, 'image': IMG, 'patch': P},
                    'timing': 'device events around `calls` back-to-back calls; the variants of a row alternate round by round after 3 warm-up '
                              'rounds; *_ms = median over the rounds, *_ms_minmax = their range',
                    'yardstick': 'eager PyTorch on the same GPU, channels-last (F.conv2d / F.conv_transpose2d / F.interpolate), bf16 autocast and f32',
                    'col_workspace_bytes': OU.COL_WORKSPACE_BYTES[0]})
    for p in parts:
        res.setdefault('runs', {})[p] = {'batch': a.batch, 'rounds': a.rounds, 'calls_per_round': a.calls, 'modes': a.modes}
        {'head': part_head, 'stages': part_stages, 'tail': part_tail, 'step': part_step}[p](a, res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    if a.ratios_from:
        rows = {}
        for line in open(a.ratios_from):
            m = re.search(r'DPT_RATIO (\{"case".*\})', line)
            if m:
                r = json.loads(m.group(1))
                rows[r['case'], r['mode'], r['tensor']] = r
        rows = list(rows.values())
        worst = {}
        for m in ('fp32', 'bf16'):
            rs = [r for r in rows if r['mode'] == m and r['ratio'] is not None]
            if rs:
                w = max(rs, key=lambda r: r['ratio'])
                worst[m] = {'ratio': w['ratio'], 'case': w['case'], 'tensor': w['tensor']}
        res['deviation_ratios'] = {
            'what': 'per tensor: max|engine - f64| / max|f64| against the same for the reference (f32; torch.autocast(bfloat16) in bf16 mode)',
            'allowed': {'fp32': 4.0, 'bf16': 5.0}, 'worst': worst,
            'bf16_reason': 'the placement of the roundings: the reference head on the CPU with the engine\'s rounding points (bf16 convolution operands, '
                           'f32 maps between the convolutions; make_golden_dpt.py --emulate) deviates from f64 by the same amounts tensor by tensor; on '
                           '2 x 4-token maps a few ReLU sign flips decide these tensors under either placement',
            'rows': rows}
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
