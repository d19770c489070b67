"""The classification fine-tuning recipe (csrc/clsrecipe.hip) against eager torch restatements of the reference's own lines, the two
variants alternating in one process on one device, every iteration timed with device events after a warm-up.  The baseline is never
the code under test: it is what utils/mixup.py, utils/cross_entropy.py and utils/model_ema.py execute, restated below.

  (a) mix      B = 128, 3 x 224 x 224 f32, batch mode: a blend (x.flip(0).mul_, mul_, add_) and a CutMix box (flip + slice copy);
               the engine side is ONE mmae_mixup_pairs launch, with the same parameters
  (b) loss     SoftTargetCrossEntropy forward + backward at (128, 1000) and (1024, 1000): log_softmax, mul, sum, mean + autograd
               against mmae_soft_ce_fwd + mmae_soft_ce_bwd; launched from Python, and each variant replayed from a hipGraph of its
               own (the device's share of the time: both are a few microsecond-sized kernels, so the eager figure is host work)
  (c) ema      ModelEma.update on the ViT-B classification model: the per-tensor loop over two state_dict()s against one
               mmae_ema_update over the two arenas
  (d) step     the whole bf16 fine-tuning step at B = 128 (mixup, forward, soft-target loss, backward, grouped fused AdamW, EMA) with
               the recipe's kernels against the same step with the eager restatements of (a)-(c)

Medians and the min-max spread of each variant go to profiles/cls_recipe_bench.json, with the algorithmic bytes of (a) and (c) and
the bytes/s they imply beside the HBM streaming rate of the MI355X (6.29 TB/s measured for a float4 copy).

    python tools/cls_recipe_bench.py [--iters 30] [--warmup 5] [--only mix|loss|ema|step|all] [--out profiles/cls_recipe_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimae_amd as M  # noqa: E402
from multimae_amd import engine, ops  # noqa: E402
from dropin import amd_loop  # noqa: E402

HBM_STREAM_TBS = 6.29
DEV = 'cuda'


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


def _pair(times):
    r = {n: _stats(v) for n, v in times.items()}
    r['speedup_of_medians'] = r['eager']['median_ms'] / r['fused']['median_ms']
    return r


# ---- eager restatements of the reference ------------------------------------------------------------------------------------------
def eager_mix_batch(x, lam, box):
    """Mixup._mix_batch, utils/mixup.py:203-214"""
    if box is not None:
        yl, yh, xl, xh = box
        x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    else:
        x_flipped = x.flip(0).mul_(1. - lam)
        x.mul_(lam).add_(x_flipped)
    return x


def eager_mix_target(target, K, lam, smoothing):
    """mixup_target, utils/mixup.py:23-33"""
    off = smoothing / K
    on = 1. - smoothing + off
    hot = lambda t: torch.full((t.shape[0], K), off, device=t.device).scatter_(1, t.long().view(-1, 1), on)
    return hot(target) * lam + hot(target.flip(0)) * (1. - lam)


def eager_soft_ce(x, target):
    """SoftTargetCrossEntropy.forward, utils/cross_entropy.py:41-43"""
    return torch.sum(-target * F.log_softmax(x, dim=-1), dim=-1).mean()


def eager_ema_update(ema_model, model, decay):
    """ModelEma.update, utils/model_ema.py:72-83"""
    with torch.no_grad():
        msd = model.state_dict()
        for k, ema_v in ema_model.state_dict().items():
            ema_v.copy_(ema_v * decay + (1. - decay) * msd[k].detach())


def _rows(B, lam, box):
    r = np.zeros((B, 8), dtype=np.int32)
    r[:, :4] = np.array([lam, 1. - lam, lam, 1. - lam], dtype=np.float32).view(np.int32)
    r[:, 4:] = (ops.MIX_BLEND, 0, 0, 0) if box is None else box
    return torch.from_numpy(r).to(DEV)


def bench_mix(a, res):
    B, C, H, W = 128, 3, 224, 224
    x = torch.randn(B, C, H, W, device=DEV)
    nbytes = x.numel() * 4
    out = {'geometry': dict(B=B, C=C, H=H, W=W), 'batch_bytes': nbytes}
    for name, lam, box in (('blend', 0.37, None), ('cutmix', 0.5, (40, 198, 33, 191))):
        rows = _rows(B, lam, box)
        t = _alternate({'eager': lambda: eager_mix_batch(x, lam, box), 'fused': lambda: ops.mixup_pairs(x, rows)}, a.iters, a.warmup)
        r = _pair(t)
        frac = 1.0 if box is None else (box[1] - box[0]) * (box[3] - box[2]) / (H * W)
        r['fused_algorithmic_bytes'] = int(nbytes * frac * 2)      # every touched pixel of the batch read once and written once
        r['fused_tb_per_s'] = r['fused_algorithmic_bytes'] / (r['fused']['median_ms'] * 1e-3) / 1e12
        r['fraction_of_hbm_stream_rate'] = r['fused_tb_per_s'] / HBM_STREAM_TBS
        out[name] = r
        x.copy_(torch.randn_like(x))                               # blends shrink the values: fresh data for the next case
    res['mix'] = out
    print('mix', json.dumps(out), flush=True)


def _graphed(fn):
    """fn captured in a hipGraph after a warm-up on a side stream: what the device does, without the host between the launches"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def bench_loss(a, res):
    out = {}
    for B, K in ((128, 1000), (1024, 1000)):
        x = (torch.randn(B, K, device=DEV) * 2).requires_grad_(True)
        t = eager_mix_target(torch.randint(0, K, (B,), device=DEV), K, 0.3, 0.1)
        crit = M.SoftTargetCrossEntropy()

        def eager():
            x.grad = None
            eager_soft_ce(x, t).backward()

        def fused():
            x.grad = None
            crit(x, t).backward()
        out[f'{B}x{K}'] = _pair(_alternate({'eager': eager, 'fused': fused}, a.iters, a.warmup))
        out[f'{B}x{K}']['graph_replay'] = _pair(_alternate({'eager': _graphed(eager), 'fused': _graphed(fused)}, a.iters, a.warmup))
    res['soft_target_loss_fwd_bwd'] = out
    print('loss', json.dumps(out), flush=True)


def _vit_b():
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=224)}
    outs = {'cls': M.LinearOutputAdapter(num_classes=1000, use_mean_pooling=True)}
    model = M.multivit_base(input_adapters=ins, output_adapters=outs, num_global_tokens=1).to(DEV)
    model.build_arena()
    return model


def bench_ema(a, res, model):
    import copy
    fused = M.ModelEma(model, decay=0.9999)
    ref = copy.deepcopy(fused.ema, {id(engine.arena_of(fused.ema)): None})      # plain tensors: the reference's deepcopy of the model
    n = engine.arena_of(model).numel
    out = _pair(_alternate({'eager': lambda: eager_ema_update(ref, model, 0.9999), 'fused': lambda: fused.update(model)}, a.iters, a.warmup))
    out.update(tensors=len(model.state_dict()), arena_elements=n, fused_algorithmic_bytes=3 * n * 4)       # read ema, read p, write ema
    out['fused_tb_per_s'] = out['fused_algorithmic_bytes'] / (out['fused']['median_ms'] * 1e-3) / 1e12
    out['fraction_of_hbm_stream_rate'] = out['fused_tb_per_s'] / HBM_STREAM_TBS
    res['ema_update_vit_b'] = out
    print('ema', json.dumps(out), flush=True)


def bench_step(a, res, model):
    import copy
    B, K = 128, 1000
    args = types.SimpleNamespace(opt='adamw', lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, mixup=0.8, cutmix=1.0, cutmix_minmax=None,
                                 mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode='batch', smoothing=0.1, nb_classes=K, model_ema_decay=0.9999)
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
    ema = amd_loop.model_ema(model, args)
    ema_ref = copy.deepcopy(ema.ema, {id(engine.arena_of(ema.ema)): None})
    x0 = torch.randn(B, 3, 224, 224, device=DEV)
    y = torch.randint(0, K, (B,), device=DEV)
    x = x0.clone()

    def fused():
        x.copy_(x0)
        xs, ts = mixup_fn(x, y)
        opt.zero_grad()
        loss = crit(model({'rgb': xs})['cls'], ts)
        scaler(loss, opt, clip_grad=None, parameters=model.parameters())
        ema.update(model)

    def eager():
        x.copy_(x0)
        lam, cut = mixup_fn._params_per_batch()
        box = None
        if lam != 1. and cut:
            box, lam = mixup_fn._box_and_lam(224, 224, lam)
        xs = eager_mix_batch(x, lam, box) if lam != 1. else x
        ts = eager_mix_target(y, K, lam, 0.1)
        opt.zero_grad()
        loss = eager_soft_ce(model({'rgb': xs})['cls'].float(), ts)
        scaler(loss, opt, clip_grad=None, parameters=model.parameters())
        eager_ema_update(ema_ref, model, 0.9999)

    engine.set_direct_grads(True)
    try:
        with engine.precision('bf16'):
            np.random.seed(0)
            out = _pair(_alternate({'eager': eager, 'fused': fused}, a.iters, a.warmup))
    finally:
        engine.set_direct_grads(False)
    out['geometry'] = dict(B=B, K=K, model='multivit_base', precision='bf16')
    res['finetune_step'] = out
    print('step', json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--only', choices=['mix', 'loss', 'ema', 'step', 'all'], default='all')
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cls_recipe_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(), 'iters': a.iters, 'warmup': a.warmup, 'hbm_stream_tb_per_s': HBM_STREAM_TBS}
    if a.only in ('mix', 'all'):
        bench_mix(a, res)
    if a.only in ('loss', 'all'):
        bench_loss(a, res)
    if a.only in ('ema', 'step', 'all'):
        model = _vit_b()
        if a.only in ('ema', 'all'):
            bench_ema(a, res, model)
        if a.only in ('step', 'all'):
            bench_step(a, res, model)
    if not a.no_write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
