"""mmae_opt_step (one group) against mmae_opt_step_groups (the fine-tuning recipe's groups) on the same parameter arena.

Shapes: multivit_base (rgb, LinearOutputAdapter(1000), ~86.4 M trainable values, 28 groups at layer decay 0.65) and the
multivit_large equivalent (52 groups).  Both optimisers step the same arena (parameters and a fixed gradient); each has its own
moments.  Per alternation and mode: --warmup untimed steps, then --steps steps between two device events, no host
synchronisation in between (max_steps_in_flight = 0).  Prints one JSON line (ms per optimiser step, every alternation, medians,
grouped / single - 1); --out also writes it to a file.

    python tools/opt_groups_bench.py [--shapes base,large] [--steps 50] [--warmup 10] [--alternations 5] [--out FILE]
    rocprofv3 --kernel-trace --stats -d out -- python tools/opt_groups_bench.py --alternations 1 --steps 20

Estimate, not measured: the step streams p, g, m, v in and p, m, v out (28 B per value) plus the gradient once more for the
norm (4 B), about 2.8 GB per ViT-B step, 0.44 ms at a practical 6.3 TB/s; the group map adds 2 B per 64 values.
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimae_amd as M  # noqa: E402
from dropin import amd_loop  # noqa: E402
from multimae_amd.optim import FusedAdamW  # noqa: E402


def build(shape):
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=224)}
    outs = {'cls': M.LinearOutputAdapter(num_classes=1000)}
    model = getattr(M, f'multivit_{shape}')(input_adapters=ins, output_adapters=outs, num_global_tokens=1).to('cuda')
    L = model.get_num_layers()
    ld = 0.65 if shape == 'base' else 0.75
    values = [ld ** (L + 1 - i) for i in range(L + 2)]

    def layer_id(name):
        if name == 'global_tokens' or name.startswith('input_adapters'):
            return 0
        return int(name.split('.')[1]) + 1 if name.startswith('encoder') else L + 1

    single = FusedAdamW(model, lr=1e-6, weight_decay=0.05, clip_grad=5.0)
    args = types.SimpleNamespace(opt='adamw', lr=1e-6, weight_decay=0.05)
    grouped = amd_loop.create_optimizer_groups(args, model, skip_list=model.no_weight_decay(), get_num_layer=layer_id,
                                               get_layer_scale=lambda k: values[k])
    grouped.clip_grad = 5.0
    for g in grouped.param_groups:
        g['lr'] = 1e-6 * g['lr_scale']
    single.max_steps_in_flight = grouped.max_steps_in_flight = 0
    a = single.arena
    assert grouped.arena is a
    gen = torch.Generator(device='cuda').manual_seed(1)
    a.grad.normal_(generator=gen).mul_(1e-3)
    return a, {'single': single, 'grouped': grouped}


def time_mode(opt, steps, warmup):
    for _ in range(warmup):
        opt.step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        opt.step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='base,large')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, alternations=args.alternations)
    for shape in args.shapes.split(','):
        a, opts = build(shape)
        ms = {k: [] for k in opts}
        for alt in range(args.alternations):
            order = list(opts) if alt % 2 == 0 else list(opts)[::-1]
            for k in order:
                ms[k].append(round(time_mode(opts[k], args.steps, args.warmup), 4))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res[shape] = dict(n_trainable=a.n_trainable, groups=len(opts['grouped'].param_groups), ms_per_step=ms,
                          median_ms=med, grouped_over_single=round(med['grouped'] / med['single'] - 1, 4),
                          est_hbm_ms_at_6p3TBps=round(a.n_trainable * 32 / 6.3e9, 3),
                          counters=dict(single=opts['single'].counters(), grouped=opts['grouped'].counters()))
        del a, opts
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
