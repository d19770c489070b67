"""RandAugment on the device (csrc/randaug.hip, staging.ClsStager(rand_augment=...)) for classification fine-tuning: what the augment
launches cost, whether the step notices them, and what the host transform they replace costs.  Medians of --rounds rounds after
--warmup rounds, the variants alternating in one process on one device.

  (a) kernel   B = 128, 3 x 224 x 224, a table of the default policy (rand-m9-mstd0.5-inc1, bicubic), device events around one
               ``data_ops.rand_augment_u8`` call (two layer passes, a stats and an apply launch each):
                 augment    the drawn table
                 without_stats_ops  the same table with AutoContrast / Equalize / Contrast turned into no-ops
                 copy_only  a table without layers: the same launches, every sample copied
               with the bytes the passes move (each pass reads and writes the batch once; the stats launch re-reads the samples whose
               op needs the whole image) beside the HBM streaming rate of the MI355X
  (b) step     the whole bf16 fine-tuning step at B = 128 (MultiViT-B + linear head, mixup, soft-target loss, grouped fused AdamW) fed
               from pinned uint8 host batches through ClsStagedLoader, wall clock per step over a round of --steps steps, with the
               policy on and off.  The augment runs on the copy stream under the previous step, so the expectation is a difference
               inside the run-to-run spread this run records.
  (c) host     the transform the launches replace: the reference's RandAugment on PIL images, per image, one thread.  Needs PIL and
               ``--reference-auto-augment PATH`` (the reference's utils/auto_augment.py, loaded by path); no GPU.  ``--only host``
               merges the figure into an existing result file and names the machine it was taken on.

Results go to profiles/rand_augment_bench.json.

    python tools/rand_augment_bench.py [--rounds 20] [--warmup 5] [--steps 6] [--only kernel|step|host|all] [--out ...]
"""
import argparse
import importlib.util
import json
import os
import platform
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
POLICY = 'rand-m9-mstd0.5-inc1'
STATS_OPS = (1, 2, 8)             # AutoContrast, Equalize, Contrast


def _stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'spread_ms': max(ts) - min(ts), 'n': len(ts)}


def _args():
    return types.SimpleNamespace(opt='adamw', lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, mixup=0.8, cutmix=1.0,
                                 cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode='batch', smoothing=0.1,
                                 nb_classes=1000, reprob=0.25, remode='pixel', recount=1, imagenet_default_mean_and_std=True,
                                 aa=POLICY, input_size=224, train_interpolation='bicubic')


def bench_kernel(a, res):
    B, H, W = 128, 224, 224
    ra = amd_loop.rand_augment(_args())
    random.seed(0)
    np.random.seed(0)
    table_host = ra.draw((B, 3, H, W))
    table = torch.from_numpy(table_host).to(DEV)
    empty = torch.zeros_like(table)
    no_stats_host = table_host.copy()
    for l in range(4):                                          # AutoContrast, Equalize, Contrast -> no-op: what the stats launches cost
        col = no_stats_host[:, 4 + 16 * l]
        col[np.isin(col, STATS_OPS)] = 0
    no_stats = torch.from_numpy(no_stats_host).to(DEV)
    u8 = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, device=DEV)
    y = torch.empty_like(u8)
    variants = {'augment': lambda: data_ops.rand_augment_u8(u8, table, out=y, layers=ra.num_layers),
                'without_stats_ops': lambda: data_ops.rand_augment_u8(u8, no_stats, out=y, layers=ra.num_layers),
                'copy_only': lambda: data_ops.rand_augment_u8(u8, empty, out=y, layers=ra.num_layers)}
    times = {n: [] for n in variants}
    for it in range(a.warmup + a.rounds):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[n].append(e0.elapsed_time(e1))
    out = {n: _stats(t) for n, t in times.items()}
    img = u8.numel()
    ops = [[int(table_host[b, 4 + 16 * l]) for l in range(int(table_host[b, 0]))] for b in range(B)]
    stats_samples = sum(1 for o in ops for v in o if v in STATS_OPS)
    moved = {'augment': 2 * ra.num_layers * img + stats_samples * 3 * H * W, 'copy_only': 2 * ra.num_layers * img,
             'without_stats_ops': 2 * ra.num_layers * img}
    for n in variants:
        out[n]['bytes_moved'] = moved[n]
        out[n]['tb_per_s'] = moved[n] / (out[n]['median_ms'] * 1e-3) / 1e12
        out[n]['fraction_of_hbm_stream_rate'] = out[n]['tb_per_s'] / HBM_STREAM_TBS
    out['geometry'] = dict(B=B, H=H, W=W, policy=POLICY, interpolation='bicubic', layer_passes=ra.num_layers, launches=2 * ra.num_layers,
                           layers_per_sample=float(np.mean([len(o) for o in ops])), samples_with_a_stats_op=stats_samples,
                           ops_drawn={str(k): sum(o.count(k) for o in ops) for k in range(1, 12)}, timing='device events around one call')
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
    args = _args()
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
    g = torch.Generator().manual_seed(0)
    u8 = [torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=g).pin_memory() for _ in range(3)]
    labels = [torch.randint(0, K, (B,), generator=g).pin_memory() for _ in range(3)]
    feed = [(u8[i % 3], labels[i % 3]) for i in range(n_steps)]
    loaders = {'rand_augment_off': amd_loop.cls_staged_loader(feed, args, device=DEV, train=True),
               'rand_augment_on': amd_loop.cls_staged_loader(feed, args, device=DEV, train=True, rand_augment=amd_loop.rand_augment(args))}

    def step(x, y):
        xs, ts = mixup_fn(x, y)
        opt.zero_grad()
        loss = crit(model({'rgb': xs})['cls'], ts)
        scaler(loss, opt, clip_grad=None, parameters=model.parameters())

    times = {n: [] for n in loaders}
    draw = []
    engine.set_direct_grads(True)
    try:
        with engine.precision('bf16'):
            random.seed(0)
            np.random.seed(0)
            for it in range(a.warmup + a.rounds):
                for n, loader in loaders.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for x, y in loader:
                        step(x, y)
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        times[n].append((time.perf_counter() - t0) * 1e3 / n_steps)
    finally:
        engine.set_direct_grads(False)
    ra = loaders['rand_augment_on'].stager.rand_augment
    for _ in range(a.rounds):                                   # what the host pays per batch for the policy's draws
        t0 = time.perf_counter()
        ra.draw((B, 3, 224, 224))
        draw.append((time.perf_counter() - t0) * 1e3)
    out = {n: _stats(t) for n, t in times.items()}
    d = out['rand_augment_on']['median_ms'] - out['rand_augment_off']['median_ms']
    out['on_minus_off_ms'] = d
    out['within_run_to_run_spread'] = bool(abs(d) <= max(out['rand_augment_on']['spread_ms'], out['rand_augment_off']['spread_ms']))
    out['host_draw_per_batch'] = _stats(draw)
    out['geometry'] = dict(B=B, K=K, model='multivit_base', precision='bf16', steps_per_round=n_steps, policy=POLICY,
                           timing='wall clock per step, host batches pinned, ClsStagedLoader both ways')
    res['finetune_step'] = out
    print('step', json.dumps(out), flush=True)


def bench_host(a, res):
    """the reference's own transform on PIL images, one thread"""
    try:
        from PIL import Image
        import PIL
    except ImportError:
        res['host_reference'] = 'not measured: PIL is not importable here'
        return
    if not a.reference_auto_augment or not os.path.exists(a.reference_auto_augment):
        res['host_reference'] = 'not measured: --reference-auto-augment was not given (the reference is not part of this repository)'
        return
    spec = importlib.util.spec_from_file_location('ref_auto_augment', a.reference_auto_augment)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.set_num_threads(1)
    tf = ref.rand_augment_transform(POLICY, dict(translate_const=100, img_mean=(124, 116, 104), interpolation=Image.BICUBIC))
    rng = np.random.RandomState(0)
    imgs = [Image.fromarray(rng.randint(0, 256, (224, 224, 3)).astype(np.uint8)) for _ in range(64)]
    random.seed(0)
    np.random.seed(0)
    per = []
    for it in range(a.warmup + a.rounds):
        t0 = time.perf_counter()
        for im in imgs:
            tf(im)
        if it >= a.warmup:
            per.append((time.perf_counter() - t0) * 1e3 / len(imgs))
    out = _stats(per)
    out['images_per_s_one_thread'] = 1e3 / out['median_ms']
    out['per_batch_of_128_ms'] = 128 * out['median_ms']
    out['machine'] = f'{platform.processor() or platform.machine()}, {os.cpu_count()} CPUs, PIL {PIL.__version__} (the machine that ran --only host, not the GPU host of the other entries)'
    out['what'] = f'utils/auto_augment.py rand_augment_transform({POLICY!r}, bicubic) on 224 x 224 RGB PIL images, ms per image'
    res['host_reference'] = out
    print('host', json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--only', choices=['kernel', 'step', 'host', 'all'], default='all')
    ap.add_argument('--reference-auto-augment', default=None)
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rand_augment_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(0)
    res = {}
    if a.only == 'host' and os.path.exists(a.out):               # merged into the GPU run's file
        with open(a.out) as f:
            res = json.load(f)
    if a.only != 'host':
        res.update({'device': torch.cuda.get_device_name(), 'rounds': a.rounds, 'warmup': a.warmup, 'hbm_stream_tb_per_s': HBM_STREAM_TBS})
    if a.only in ('kernel', 'all'):
        bench_kernel(a, res)
    if a.only in ('step', 'all'):
        bench_step(a, res)
    if a.only in ('host', 'all'):
        bench_host(a, res)
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
