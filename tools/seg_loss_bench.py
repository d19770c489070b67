"""The semantic-segmentation loss at the ADE20K geometry (B = 4, 512 x 512, 150 classes on 128 x 128 logits, the geometry of
tools/convnext_head_bench.py), two variants alternating in one process, each iteration timed with device events after a warm-up:

  eager  the path without the fused loss: mmae_resize_fwd writes the f32 (B, K, H, W) image, nn.CrossEntropyLoss(ignore_index=255)
         forward + backward on it, mmae_resize_bwd gathers the image gradient back to the low-resolution logits
  fused  criterion.SegCrossEntropyLoss on the logits: mmae_seg_ce_fwd + mmae_seg_ce_bwd (csrc/segloss.hip)

first on the loss alone (logits in, d_logits out), then inside the whole head + loss step (ConvNeXtAdapter forward, loss, backward;
bf16).  Medians, the min-max spread of each variant and the algorithmic bytes of both go to profiles/seg_loss_bench.json.

    python tools/seg_loss_bench.py [--iters 30] [--warmup 5] [--out profiles/seg_loss_bench.json]

Per-kernel times come from a run of its own under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d out -- python tools/seg_loss_bench.py --iters 5 --only loss --no-write
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
import multimae_amd as M  # noqa: E402
from multimae_amd import ops, output_adapters as OA  # noqa: E402

B, H, W, K, h, w = 4, 512, 512, 150, 128, 128
D, E, P, DEPTH = 768, 6144, 16, 4
IGN = 255


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=['loss', 'step', 'both'], default='both')
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seg_loss_bench.json'))
    a = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    ld = ops.round_up(K, 8)
    target = torch.randint(0, K, (B, H, W), device=dev)
    target[torch.rand(B, H, W, device=dev) < 0.1] = IGN
    res = {'device': torch.cuda.get_device_name(), 'geometry': dict(B=B, H=H, W=W, K=K, h=h, w=w, ld=ld), 'iters': a.iters, 'warmup': a.warmup}

    if a.only in ('loss', 'both'):
        logits = torch.zeros(B * h * w, ld, device=dev)
        logits[:, :K] = torch.randn(B * h * w, K, device=dev) * 3
        ce = nn.CrossEntropyLoss(ignore_index=IGN)
        up = torch.ones(1, device=dev)

        def eager():
            img = ops.resize_fwd(logits, ld, torch.empty(B, K, H, W, device=dev), B, h, w, K, H, W, 'bilinear').requires_grad_(True)
            ce(img, target).backward()
            return ops.resize_bwd(img.grad, torch.empty_like(logits), ld, B, h, w, K, H, W, 'bilinear')

        def fused():
            lse, out = ops.seg_ce_fwd(logits, ld, target, IGN, B, h, w, K, H, W, 'bilinear')
            return ops.seg_ce_bwd(logits, ld, target, IGN, B, h, w, K, H, W, 'bilinear', lse, out, up, torch.empty_like(logits))
        t = _alternate({'eager': eager, 'fused': fused}, a.iters, a.warmup)
        res['loss_only'] = {n: _stats(v) for n, v in t.items()}
        res['loss_only']['speedup_of_medians'] = res['loss_only']['eager']['median_ms'] / res['loss_only']['fused']['median_ms']
        print('loss only', json.dumps(res['loss_only']), flush=True)

    if a.only in ('step', 'both'):
        N = (H // 16) * (W // 16)
        head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=E, preds_per_patch=P, depth=DEPTH)
        head.init(D)
        head = head.to(dev)
        info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': N, 'num_tokens': N}}, 'image_size': (H, W)}
        x = (torch.randn(B, N + 1, D, device=dev) * 0.5).requires_grad_(True)
        crit = {'eager': nn.CrossEntropyLoss(ignore_index=IGN), 'fused': M.SegCrossEntropyLoss(ignore_index=IGN)}

        def step(which):
            def run():
                M.engine.set_lazy_predictions(which == 'fused')
                try:
                    crit[which](head(x, info), target).backward()
                finally:
                    M.engine.set_lazy_predictions(True)
            return run
        with M.engine.precision('bf16'):
            t = _alternate({'eager': step('eager'), 'fused': step('fused')}, a.iters, a.warmup)
        res['head_and_loss_step_bf16'] = {n: _stats(v) for n, v in t.items()}
        res['head_and_loss_step_bf16']['speedup_of_medians'] = (res['head_and_loss_step_bf16']['eager']['median_ms']
                                                                / res['head_and_loss_step_bf16']['fused']['median_ms'])
        print('head + loss step', json.dumps(res['head_and_loss_step_bf16']), flush=True)

    img, low, px = B * K * H * W * 4, B * h * w * ld * 4, B * H * W
    res['algorithmic_bytes'] = {
        # resize_fwd (read logits, write image), log-softmax forward (read + write), NLL forward (gather: the targets), NLL backward
        # (write), log-softmax backward (two reads + one write), resize_bwd (read image gradient, write d_logits)
        'eager': 2 * low + 8 * img + 2 * px * 8,
        # forward: logits + targets in, lse out; backward: logits + targets + lse in, d_logits out
        'fused': 3 * low + 2 * px * 8 + 2 * px * 4,
        'image_bytes': img, 'logits_bytes': low}
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
