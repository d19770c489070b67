"""The per-batch work of ``evaluate()`` in run_finetuning_cls.py (:600-607) after the forward pass, at (B, K) = (128, 1000) and
(1024, 1000), f32 and bf16 logits; three variants alternating in one process, each round timed with device events after a warm-up:

  eager_items  the reference's lines restated: nn.CrossEntropyLoss, utils.metrics.accuracy (topk(5), t, eq, two reductions) and the three
               .item() read-backs into Python totals
  eager        the same without the read-backs (the values stay on the device)
  fused        ClsMetric.update: mmae_cls_eval, two launches into the f64 accumulator (csrc/clseval.hip)

Medians and the min-max spread of each variant, and the kernel launches and host synchronisations of one round of each (counted as
tools/reg_loss_bench.py counts them), go to profiles/cls_eval_bench.json.  Refuses to run without a GPU.

    python tools/cls_eval_bench.py [--iters 20] [--warmup 5] [--out profiles/cls_eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimae_amd as M  # noqa: E402

SHAPES = ((128, 1000), (1024, 1000))
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def accuracy(output, target, topk=(1,)):
    """the operations of utils/metrics.py:31-38 in their order: a sorted topk, a transpose, an eq against the expanded target, and per
    threshold a float sum, a product and a division"""
    kmax = min(max(topk), output.shape[1])
    top = output.topk(kmax, dim=1, largest=True, sorted=True).indices.t()
    hit = top.eq(target.reshape(1, -1).expand_as(top))
    return [hit[:min(k, kmax)].reshape(-1).float().sum(0) * 100. / target.shape[0] for k in topk]


def _alternate(variants, iters, warmup):
    times = {n: [] for n in variants}
    for it in range(warmup + iters):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[n].append(e0.elapsed_time(e1))
    return times


def _stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'spread_ms': max(ts) - min(ts), 'n': len(ts)}


def _counts(fn):
    """kernel launches (torch.profiler's device kernel events) of one call and host synchronisations (torch's synchronisation check in
    'warn' mode) of two consecutive calls; a count that could not be taken is None"""
    syncs = []
    for _ in range(2):
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode('default')
        syncs.append(sum('synchroniz' in str(x.message) for x in ws))
    torch.cuda.synchronize()
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        launches = n or None
    except Exception as e:                                     # the profiler is optional: the timings do not depend on it
        print('launch count not taken:', repr(e), flush=True)
    return {'launches': launches, 'host_syncs': syncs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cls_eval_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('cls_eval_bench: needs a GPU (the engine has no CPU path)')
    if a.iters < 5:
        sys.exit('cls_eval_bench: at least 5 timed rounds')
    dev = 'cuda'
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(), 'iters': a.iters, 'warmup': a.warmup, 'topk': [1, 5]}
    pending = []
    crit = torch.nn.CrossEntropyLoss()
    for B, K in SHAPES:
        target = torch.randint(0, K, (B,), device=dev)
        for tag, dt in DTYPES.items():
            x = (torch.randn(B, K, device=dev) * 2).to(dt)
            metric = M.ClsMetric(topk=(1, 5), device=dev)
            totals = {'loss': 0.0, 'acc1': 0.0, 'acc5': 0.0, 'n': 0}
            dev_tot = torch.zeros(3, device=dev)

            def eager_items(x=x, target=target, totals=totals, B=B):
                loss = crit(x, target)
                acc1, acc5 = accuracy(x, target, topk=(1, 5))
                totals['loss'] += loss.item()
                totals['acc1'] += acc1.item() * B
                totals['acc5'] += acc5.item() * B
                totals['n'] += B

            def eager(x=x, target=target, dev_tot=dev_tot):
                loss = crit(x, target)
                acc1, acc5 = accuracy(x, target, topk=(1, 5))
                dev_tot.add_(torch.stack([loss.float(), acc1, acc5]))

            def fused(x=x, target=target, metric=metric):
                metric.update(x, target)

            variants = {'eager_items': eager_items, 'eager': eager, 'fused': fused}
            key = f'{B}x{K}_{tag}'
            t = _alternate(variants, a.iters, a.warmup)
            res[key] = {n: _stats(v) for n, v in t.items()}
            res[key]['eager_items_over_fused_medians'] = res[key]['eager_items']['median_ms'] / res[key]['fused']['median_ms']
            res[key]['eager_over_fused_medians'] = res[key]['eager']['median_ms'] / res[key]['fused']['median_ms']
            print(key, json.dumps(res[key]), flush=True)
            pending.append((key, variants))

    def write():
        if not a.no_write:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
    write()                                                    # the timings are kept even if the profiler below gives up
    for key, variants in pending:
        res[key]['per_round'] = {n: _counts(fn) for n, fn in variants.items()}
        print(key, json.dumps(res[key]['per_round']), flush=True)
    write()


if __name__ == '__main__':
    main()
