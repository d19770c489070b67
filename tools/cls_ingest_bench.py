"""uint8 batch ingest + random erasing for classification fine-tuning (csrc/erase.hip, staging.ClsStager) against the float32 feed of
run_finetuning_cls.py, the variants alternating in one process on one device, medians of --rounds rounds after --warmup rounds.

  (a) kernel   B = 128 and B = 1024, 3 x 224 x 224, erase table of the default recipe (--reprob 0.25 --remode pixel), device events:
                 fused     mmae_ingest_rgb_u8_chw_erase: uint8 CHW -> normalised, erased f32, one launch
                 composed  mmae_ingest_rgb_u8 (uint8 HWC) + mmae_random_erase in place, two launches
                 eager     x.float().sub_(255 mean).div_(255 std), the arithmetic a prefetcher would run (no erasing)
               with the bytes/s over the algorithmic bytes (uint8 read + f32 written) beside the HBM streaming rate of the MI355X
  (b) step     the whole bf16 fine-tuning step at B = 128 (MultiViT-B + linear head, mixup, soft-target loss, grouped fused AdamW) fed
               from pinned host batches, wall clock per step over a round of --steps steps:
                 reference feed  float32 batches, ``.to(device, non_blocking=True)`` on the compute stream, RandomErasing in place
                 staged feed     uint8 batches through ClsStagedLoader (copy + decode + erase on the copy stream, one batch ahead)
               with the H2D bytes per batch and the launches of one step of each (torch.profiler's device events)

The yardstick is the reference feed on the same commit and machine.  Results go to profiles/cls_ingest_bench.json.

    python tools/cls_ingest_bench.py [--rounds 20] [--warmup 5] [--steps 6] [--only kernel|step|all] [--out profiles/cls_ingest_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimae_amd as M  # noqa: E402
from multimae_amd import data_ops, engine, staging  # noqa: E402
from dropin import amd_loop  # noqa: E402

HBM_STREAM_TBS = 6.29
DEV = 'cuda'
MEAN, STD = staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD


def _stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'spread_ms': max(ts) - min(ts), 'n': len(ts)}


def _alternate_events(variants, rounds, warmup):
    times = {n: [] for n in variants}
    for it in range(warmup + rounds):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[n].append(e0.elapsed_time(e1))
    return times


def _launches(fn):
    """device events (kernels and copies) of one call, by torch.profiler; a profiler that records none fails the run, so the file
    never carries an empty count"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = len([e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')])
    if n == 0:
        raise RuntimeError('torch.profiler recorded no device event: the launch counts cannot be taken')
    return n


def _recipe_erasing():
    era = M.RandomErasing(probability=0.25, mode='pixel')
    era.noise_seed = 0
    return era


def bench_kernel(a, res):
    out = {}
    lut = data_ops.rgb_table(MEAN, STD).to(DEV)
    m255 = (torch.tensor(MEAN, device=DEV) * 255).view(1, 3, 1, 1)
    s255 = (torch.tensor(STD, device=DEV) * 255).view(1, 3, 1, 1)
    for B in (128, 1024):
        try:
            u8 = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, device=DEV)
            hwc = u8.permute(0, 2, 3, 1).contiguous()
            y = torch.empty(B, 3, 224, 224, device=DEV)
        except torch.OutOfMemoryError:
            out[f'B{B}'] = 'not measured: out of memory'
            continue
        random.seed(B)
        table_host = _recipe_erasing().draw(tuple(u8.shape))
        table = torch.from_numpy(table_host).to(DEV)
        rects = table_host[1:, 4:].reshape(B, 8, 8)
        erased = float((rects[:, :, 2] * rects[:, :, 3]).sum()) / (B * 224 * 224)

        def fused():
            data_ops.ingest_rgb_u8_chw(u8, lut, table, out=y)

        def decode_only():
            data_ops.ingest_rgb_u8_chw(u8, lut, None, out=y)

        def composed():
            data_ops.ingest_rgb_u8(hwc, lut, out=y)
            data_ops.random_erase_(y, table)

        def eager():
            u8.float().sub_(m255).div_(s255)

        variants = {'fused': fused, 'composed': composed, 'eager': eager, 'decode_only': decode_only}
        r = {n: _stats(t) for n, t in _alternate_events(variants, a.rounds, a.warmup).items()}
        nbytes = u8.numel() * 5
        r['algorithmic_bytes'] = nbytes
        r['erased_fraction'] = erased
        for n in variants:
            r[n]['tb_per_s'] = nbytes / (r[n]['median_ms'] * 1e-3) / 1e12
            r[n]['fraction_of_hbm_stream_rate'] = r[n]['tb_per_s'] / HBM_STREAM_TBS
            r[n]['launches'] = _launches(variants[n])
        r['fused_over_composed'] = r['composed']['median_ms'] / r['fused']['median_ms']
        r['fused_over_eager'] = r['eager']['median_ms'] / r['fused']['median_ms']
        out[f'B{B}'] = r
        del u8, hwc, y
        torch.cuda.empty_cache()
    res['kernel'] = out
    print('kernel', json.dumps(out), flush=True)


def _vit_b():
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=224)}
    outs = {'cls': M.LinearOutputAdapter(num_classes=1000, use_mean_pooling=True)}
    model = M.multivit_base(input_adapters=ins, output_adapters=outs, num_global_tokens=1).to(DEV)
    model.build_arena()
    return model


def bench_step(a, res):
    B, K, n_steps = 128, 1000, a.steps
    model = _vit_b()
    args = types.SimpleNamespace(opt='adamw', lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, mixup=0.8, cutmix=1.0, cutmix_minmax=None,
                                 mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode='batch', smoothing=0.1, nb_classes=K,
                                 reprob=0.25, remode='pixel', recount=1, imagenet_default_mean_and_std=True)
    L = model.get_num_layers()
    values = [0.65 ** (L + 1 - i) for i in range(L + 2)]

    def layer_id(name):
        if name == 'global_tokens' or name.startswith('input_adapters'):
            return 0
        return int(name.split('.')[1]) + 1 if name.startswith('encoder') else L + 1
    opt = amd_loop.create_optimizer_groups(args, model, skip_list=model.no_weight_decay(), get_num_layer=layer_id, get_layer_scale=lambda k: values[k])
    scaler = amd_loop.LossScaler()
    mixup_fn = amd_loop.mixup(args)
    crit = amd_loop.cls_criterion(args, mixup_fn)
    era = amd_loop.random_erasing(args)

    g = torch.Generator().manual_seed(0)
    u8 = [torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=g).pin_memory() for _ in range(3)]
    lut = data_ops.rgb_table(MEAN, STD)
    f32 = [torch.stack([lut[c][b[:, c].long()] for c in range(3)], dim=1).contiguous().pin_memory() for b in u8]
    labels = [torch.randint(0, K, (B,), generator=g).pin_memory() for _ in range(3)]
    feed_f32 = [(f32[i % 3], labels[i % 3]) for i in range(n_steps)]
    feed_u8 = [(u8[i % 3], labels[i % 3]) for i in range(n_steps)]
    loader = amd_loop.cls_staged_loader(feed_u8, args, device=DEV, train=True)

    def step(x, y):
        xs, ts = mixup_fn(x, y)
        opt.zero_grad()
        loss = crit(model({'rgb': xs})['cls'], ts)
        scaler(loss, opt, clip_grad=None, parameters=model.parameters())

    def reference_feed(feed=feed_f32):
        for xh, yh in feed:
            x = xh.to(DEV, non_blocking=True)
            y = yh.to(DEV, non_blocking=True)
            era(x)
            step(x, y)

    def staged_feed():
        for x, y in loader:
            step(x, y)

    variants = {'reference_feed': reference_feed, 'staged_feed': staged_feed}
    times = {n: [] for n in variants}
    engine.set_direct_grads(True)
    try:
        with engine.precision('bf16'):
            random.seed(0)
            np.random.seed(0)
            for it in range(a.warmup + a.rounds):
                for n, fn in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        times[n].append((time.perf_counter() - t0) * 1e3 / n_steps)
            launches = {'reference_feed': _launches(lambda: reference_feed(feed_f32[:1])),
                        'staged_feed': _launches(lambda: [step(x, y) for x, y in amd_loop.cls_staged_loader(feed_u8[:1], args, device=DEV)])}
    finally:
        engine.set_direct_grads(False)
    out = {n: _stats(t) for n, t in times.items()}
    out['staged_over_reference_feed'] = out['reference_feed']['median_ms'] / out['staged_feed']['median_ms']
    out['reference_feed']['h2d_bytes_per_batch'] = f32[0].numel() * 4 + labels[0].numel() * 8
    out['staged_feed']['h2d_bytes_per_batch'] = loader.stager.bytes_per_batch(feed_u8[0])['h2d'] + (B + 1) * 68 * 4
    for n in variants:
        out[n]['device_events_of_one_step'] = launches[n]
    out['geometry'] = dict(B=B, K=K, model='multivit_base', precision='bf16', steps_per_round=n_steps, timing='wall clock per step, host batches pinned')
    res['finetune_step'] = out
    print('step', json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--only', choices=['kernel', 'step', 'all'], default='all')
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cls_ingest_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'warmup': a.warmup, 'hbm_stream_tb_per_s': HBM_STREAM_TBS}
    if a.only in ('kernel', 'all'):
        bench_kernel(a, res)
    if a.only in ('step', 'all'):
        bench_step(a, res)
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
