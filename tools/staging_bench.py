"""What a host batch costs the cfg3 step (B = 256), in four modes alternated in one process:

  a  resident    the batch already in HBM (bench.py's contract)
  b  to()        reference form (fp32 CHW rgb, fp32 depth, int64 semseg: 212 MB) moved with .to(device, non_blocking=True) on
                 the compute stream, then truncated_depth_standardize -- the drop-in loop today (run_pretraining_multimae.py:482-492)
  c  staged ref  the same batches through multimae_amd.StagedLoader (copy stream, one batch ahead, standardised there)
  d  staged      compact form (uint8 HWC rgb, uint16 depth, uint8 semseg: 65 MB) through the stager, decoded on the device
  i  (not in the default set) the compact batch staged and waited for with no step: copy + decode alone, for the kernel trace

Every step of b-d copies a real pinned host batch, cycling through a pool of --pool distinct ones, and every step ends in
torch.cuda.synchronize() as the reference loop's does.  Prints one JSON line (ms/step per mode, spread over the alternations,
delta from a, bytes_per_batch); --out also writes it to a file.

    python tools/staging_bench.py [--steps 10] [--alternations 3] [--out FILE]
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d out -- python tools/staging_bench.py --modes bcdi --alternations 1 --steps 5
"""
import argparse
import itertools
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import multimae_amd as M  # noqa: E402
from multimae_amd import staging  # noqa: E402
from multimae_amd.optim import FusedAdamW  # noqa: E402

STD = (0.1, 0.9, 1e-6)


def host_pool(n, B, seed=0):
    """n distinct pinned host batches in compact form and the same batches in reference form"""
    compact, ref = [], []
    mean = torch.tensor(staging.IMAGENET_DEFAULT_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(staging.IMAGENET_DEFAULT_STD).view(1, 3, 1, 1)
    for k in range(n):
        g = torch.Generator().manual_seed(seed + k)
        c = {'rgb': torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g),
             'depth': torch.randint(0, 65536, (B, 224, 224), dtype=torch.int32, generator=g).to(torch.uint16),
             'semseg': torch.randint(0, 133, (B, 56, 56), dtype=torch.uint8, generator=g)}
        r = {'rgb': c['rgb'].permute(0, 3, 1, 2).float().div(255).sub(mean).div(std).contiguous(),     # as collated: contiguous CHW
             'depth': (c['depth'].to(torch.int32).float() * 2.0 ** -16).unsqueeze(1),
             'semseg': c['semseg'].to(torch.long)}
        compact.append({t: v.pin_memory() for t, v in c.items()})
        ref.append({t: v.pin_memory() for t, v in r.items()})
    return compact, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10, help='timed steps per mode per alternation')
    ap.add_argument('--warmup', type=int, default=3, help='untimed steps before each timed block')
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--pool', type=int, default=3, help='distinct pinned host batches cycled through (>= 3)')
    ap.add_argument('--modes', default='abcd')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'staging_bench.py measures on the GPU'
    assert args.pool >= 3
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    B = args.batch

    torch.manual_seed(0)
    model, doms = bench.build_model('cfg3')
    model.to(dev)
    model.build_arena()
    M.engine.set_precision('bf16')
    M.engine.set_direct_grads(True)
    M.engine.set_adapter_streams(True)
    M.engine.set_wgrad_stream(True)
    opt = FusedAdamW(model, lr=1e-4 * B / 256, betas=(0.9, 0.95), weight_decay=0.05)
    fns = bench.loss_fns()

    def step(x):
        opt.zero_grad()
        preds, masks = model(x, num_encoded_tokens=98, alphas=1.0, sample_tasks_uniformly=False, fp32_output_adapters=['semseg'])
        mk = dict(masks, norm_rgb=masks['rgb'])
        tgt = dict(x, norm_rgb=x['rgb'])
        loss = sum(fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds)
        loss.backward()
        opt.step(loss)
        torch.cuda.synchronize()                                       # run_pretraining_multimae.py: end of every step

    compact, ref = host_pool(args.pool, B)
    resident = {t: v.to(dev) for t, v in ref[0].items()}
    resident['depth'] = M.truncated_depth_standardize(resident['depth'])
    stager = M.BatchStager(dev, standardize_depth=STD)

    def feed(mode, n):
        if mode == 'a':
            return itertools.repeat(resident, n)
        if mode == 'b':
            def to_device():
                for hb in itertools.islice(itertools.cycle(ref), n):
                    x = {t: v.to(dev, non_blocking=True) for t, v in hb.items()}
                    x['depth'] = M.truncated_depth_standardize(x['depth'])
                    yield x
            return to_device()
        pool = ref if mode == 'c' else compact      # 'd', 'i'
        return iter(M.StagedLoader(list(itertools.islice(itertools.cycle(pool), n)), stager))

    def run(mode, x):
        if mode == 'i':
            torch.cuda.synchronize()
        else:
            step(x)

    def block(mode):
        it = feed(mode, args.warmup + args.steps)
        for _ in range(args.warmup):
            run(mode, next(it))
        t0 = time.perf_counter()
        for x in it:
            run(mode, x)
        return (time.perf_counter() - t0) * 1e3 / args.steps

    ms = {m: [] for m in args.modes}
    for _ in range(args.alternations):
        for m in args.modes:
            ms[m].append(block(m))
    mean = {m: sum(v) / len(v) for m, v in ms.items()}
    res = {
        'tool': 'tools/staging_bench.py', 'config': 'cfg3', 'batch': B, 'steps_per_block': args.steps, 'warmup': args.warmup,
        'alternations': args.alternations, 'host_pool': args.pool, 'device': torch.cuda.get_device_name(dev),
        'modes': {'a': 'resident batch', 'b': 'reference form, .to() on the compute stream + truncated_depth_standardize',
                  'c': 'reference form through BatchStager / StagedLoader', 'd': 'compact form through BatchStager / StagedLoader',
                  'i': 'compact form staged with no step (copy + decode alone)'},
        'ms_per_step': {m: round(v, 3) for m, v in mean.items()},
        'spread_ms': {m: round(max(v) - min(v), 3) for m, v in ms.items()},
        'per_alternation_ms': {m: [round(x, 3) for x in v] for m, v in ms.items()},
        'delta_from_a_ms': {m: round(v - mean['a'], 3) for m, v in mean.items()} if 'a' in mean else None,
        'bytes_per_batch': {'compact': stager.bytes_per_batch(compact[0]), 'reference': stager.bytes_per_batch(ref[0])},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
