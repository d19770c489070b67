"""The dense regression losses and the depth metrics on the DPT head's prediction at the depth and Taskonomy recipes' geometry
(--batch_size 64, 256 x 256, one channel for depth and three for normals / rgb; --output_adapter dpt: the prediction is the f32
(B, K, H, W) image itself), two variants alternating in one process, each round timed with device events after a warm-up:

  eager  the same call on ``y * 1``: a derived tensor carries no functions.ImageMark and takes the eager restatement
         (criterion._reg_loss_eager, metrics._depth_metrics_eager) -- what ran before the fused kernels on the image existed
  fused  mmae_reg_img_fwd + mmae_reg_img_bwd and mmae_depth_metrics_img on the image (csrc/regloss.hip)
  fused_launches_only (losses)  ops.reg_img_fwd + ops.reg_img_bwd called directly, without the autograd node and backward() around them

for each loss kind forward + backward (image in, d_image out) at K = 1 and K = 3, for the metrics (K = 1), and inside the whole head
+ berHu + metrics step (DPTOutputAdapter at ViT-B width forward, loss, metrics, backward; bf16).  Medians and the min-max spread of
each variant, and the kernel launches and host synchronisations of one round of each, go to profiles/reg_image_bench.json.  Refuses
to run without a GPU.

    python tools/reg_image_bench.py [--iters 10] [--warmup 3] [--out profiles/reg_image_bench.json]
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
from multimae_amd import functions, ops, output_adapters as OA  # noqa: E402

B, H, W = 64, 256, 256
D, P, HOOKS = 768, 16, [2, 5, 8, 11]
KINDS = {'l1': M.masked_l1_loss, 'mse': M.masked_mse_loss, 'berhu': M.masked_berhu_loss}


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


def _marked(y):
    """a leaf image that carries the mark DPTOutputAdapter.forward leaves on its output"""
    y = y.requires_grad_(True)
    y._mmae_img = functions.ImageMark(y.shape, y._version)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=['loss', 'step', 'both'], default='both')
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reg_image_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('reg_image_bench: needs a GPU (the engine has no CPU path)')
    if a.iters < 5:
        sys.exit('reg_image_bench: at least 5 timed rounds')
    dev = 'cuda'
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(), 'geometry': dict(B=B, H=H, W=W, K=[1, 3]), 'iters': a.iters, 'warmup': a.warmup}
    mask = torch.rand(B, 1, H, W, device=dev) < 0.8
    up = torch.ones(1, device=dev)

    if a.only in ('loss', 'both'):
        for K in (1, 3):
            y = _marked(torch.randn(B, K, H, W, device=dev))
            target = torch.randn(B, K, H, W, device=dev)
            for kind, fn in KINDS.items():
                def run(fused, fn=fn, y=y, target=target):
                    y.grad = None
                    loss = fn(y if fused else y * 1, target, mask)
                    assert (type(loss.grad_fn).__name__ == 'RegImageLossFnBackward') == fused
                    loss.backward()
                    return y.grad

                def launches(kind=kind, y=y, target=target):               # the fused pair without the autograd node around it
                    diff, out = ops.reg_img_fwd(y.detach(), target, mask, kind)
                    return ops.reg_img_bwd(diff, out, up, kind)
                _pair(res, f'loss_fwd_bwd_{kind}_K{K}', {'eager': lambda run=run: run(False), 'fused': lambda run=run: run(True),
                                                         'fused_launches_only': launches}, a)
            if K == 1:
                with torch.no_grad():
                    _pair(res, 'depth_metrics_K1', {'eager': lambda y=y, t=target: M.depth_metrics(y * 1, t, mask),
                                                    'fused': lambda y=y, t=target: M.depth_metrics(y, t, mask)}, a)
            res[f'image_bytes_K{K}'] = B * K * H * W * 4
            del y, target

    if a.only in ('step', 'both'):
        N = (H // P) * (W // P)
        torch.manual_seed(0)
        head = OA.DPTOutputAdapter(num_classes=1, stride_level=1, patch_size=P, main_tasks=('rgb',), hooks=HOOKS)
        head.init(D)
        head = head.to(dev)
        info = {'tasks': {'rgb': {'num_tokens': N, 'has_2d_posemb': True, 'start_idx': 0, 'end_idx': N}}, 'image_size': (H, W),
                'num_task_tokens': N, 'num_global_tokens': 1}
        toks = [None] * (max(HOOKS) + 1)
        for hk in HOOKS:
            toks[hk] = (torch.randn(B, N + 1, D, device=dev) * 0.5).requires_grad_(True)
        target = torch.randn(B, 1, H, W, device=dev)

        def step(which):
            def run():
                y = head(toks, info)
                p = y if which == 'fused' else y * 1           # a derived tensor takes the eager restatement
                loss = M.masked_berhu_loss(p, target, mask)
                M.depth_metrics(p, target, mask)
                loss.backward()
                M.engine.join_wgrad_streams()
            return run
        with M.engine.precision('bf16'):
            _pair(res, 'dpt_head_berhu_metrics_step_bf16', {'eager': step('eager'), 'fused': step('fused')}, a)

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
