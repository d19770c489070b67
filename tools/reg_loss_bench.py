"""The dense regression losses and the depth metrics at the depth recipe's geometry (run_finetuning_depth.py: --batch_size 64,
256 x 256, one channel, --output_adapter convnext with preds_per_patch = 64: a 128 x 128 map, bilinear), two variants alternating in
one process, each round timed with device events after a warm-up:

  eager  the path without the fused kernels: mmae_resize_fwd writes the f32 (B, 1, H, W) image, the eager restatement of the loss
         (criterion._reg_loss_eager) forward + backward on it, mmae_resize_bwd gathers the image gradient back to the map; the metrics
         as metrics._depth_metrics_eager on the written image
  fused  mmae_reg_loss_fwd + mmae_reg_loss_bwd and mmae_depth_metrics on the map (csrc/regloss.hip)

for each loss kind (map in, d_map out), for the metrics, and inside the whole head + berHu + metrics step (ConvNeXtAdapter forward,
loss, metrics, backward; bf16).  Medians and the min-max spread of each variant, and the kernel launches and host synchronisations of
one round of each, go to profiles/reg_loss_bench.json.  Refuses to run without a GPU.

    python tools/reg_loss_bench.py [--iters 10] [--warmup 3] [--out profiles/reg_loss_bench.json]
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
from multimae_amd import criterion, metrics, ops, output_adapters as OA  # noqa: E402

B, H, W, K, h, w = 64, 256, 256, 1, 128, 128
D, E, P, DEPTH = 768, 6144, 64, 4
KINDS = ('l1', 'mse', 'berhu')


def _alternate(variants, iters, warmup):
    """variants: name -> thunk.  Runs them in turn, `warmup` untimed rounds first; returns name -> list of ms."""
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
    for _ in range(2):                                         # two rounds, both recorded: a count in the first only is a first-call effect
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


_PENDING = []                  # (key, variants) whose launches and synchronisations are counted after every timing is done


def _pair(res, key, variants, a):
    t = _alternate(variants, a.iters, a.warmup)
    res[key] = {n: _stats(v) for n, v in t.items()}
    res[key]['eager_over_fused_medians'] = res[key]['eager']['median_ms'] / res[key]['fused']['median_ms']
    print(key, json.dumps(res[key]), flush=True)
    _PENDING.append((key, variants))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=['loss', 'step', 'both'], default='both')
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reg_loss_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('reg_loss_bench: needs a GPU (the engine has no CPU path)')
    if a.iters < 5:
        sys.exit('reg_loss_bench: at least 5 timed rounds')
    dev = 'cuda'
    torch.manual_seed(0)
    ld = ops.round_up(K, 8)
    target = torch.randn(B, K, H, W, device=dev)
    mask = torch.rand(B, 1, H, W, device=dev) < 0.8
    geom = (B, h, w, K, H, W, 'bilinear')
    res = {'device': torch.cuda.get_device_name(), 'geometry': dict(B=B, H=H, W=W, K=K, h=h, w=w, ld=ld, mode='bilinear'),
           'iters': a.iters, 'warmup': a.warmup}

    if a.only in ('loss', 'both'):
        x = torch.zeros(B * h * w, ld, device=dev)
        x[:, :K] = torch.randn(B * h * w, K, device=dev)
        up = torch.ones(1, device=dev)
        for kind in KINDS:
            def eager(kind=kind):
                img = ops.resize_fwd(x, ld, torch.empty(B, K, H, W, device=dev), *geom).requires_grad_(True)
                criterion._reg_loss_eager(img, target, mask, kind).backward()
                return ops.resize_bwd(img.grad, torch.empty_like(x), ld, *geom)

            def fused(kind=kind):
                diff, out = ops.reg_loss_fwd(x, ld, target, mask, kind, *geom)
                return ops.reg_loss_bwd(diff, out, up, kind, *geom, torch.empty_like(x), ld)
            _pair(res, f'loss_fwd_bwd_{kind}', {'eager': eager, 'fused': fused}, a)
        img = ops.resize_fwd(x, ld, torch.empty(B, K, H, W, device=dev), *geom)
        _pair(res, 'depth_metrics', {
            'eager': lambda: metrics._depth_metrics_eager(img, target, mask, metrics.NYU_MEAN, metrics.NYU_STD),
            'fused': lambda: ops.depth_metrics(x, ld, target, mask, metrics.NYU_MEAN, metrics.NYU_STD, B, h, w, H, W, 'bilinear')}, a)

    if a.only in ('step', 'both'):
        N = (H // 16) * (W // 16)
        head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=E, preds_per_patch=P, depth=DEPTH)
        head.init(D)
        head = head.to(dev)
        info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': N, 'num_tokens': N}}, 'image_size': (H, W)}
        xt = (torch.randn(B, N + 1, D, device=dev) * 0.5).requires_grad_(True)

        def step(which):
            def run():
                M.engine.set_lazy_predictions(which == 'fused')
                try:
                    y = head(xt, info)
                    p = y if which == 'fused' else y * 1       # a modified prediction takes the eager restatement
                    loss = M.masked_berhu_loss(p, target, mask)
                    M.depth_metrics(p, target, mask)
                    loss.backward()
                finally:
                    M.engine.set_lazy_predictions(True)
            return run
        with M.engine.precision('bf16'):
            _pair(res, 'head_berhu_metrics_step_bf16', {'eager': step('eager'), 'fused': step('fused')}, a)

    res['image_bytes'] = B * K * H * W * 4

    def write():
        if not a.no_write:
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
    write()                                                    # the timings are kept even if the profiler below gives up
    with M.engine.precision('bf16'):
        for key, variants in _PENDING:
            res[key]['per_round'] = {n: _counts(fn) for n, fn in variants.items()}
            print(key, json.dumps(res[key]['per_round']), flush=True)
    write()


if __name__ == '__main__':
    main()
