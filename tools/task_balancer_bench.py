"""The uncertainty task balancer: what it costs, measured two ways in one process (profiles/task_balancer_bench.json).

(1) forward + backward as the loop calls it -- ``weighted = balancer(task_losses); sum(weighted.values()).backward()`` on T = 4
    device scalars -- with the engine's module (functions.TaskBalanceFn: 2 launches of its own) against an eager torch module of
    the same formula (w = (exp(-s) L + s) (L != 0): stack, ne, neg, exp, mul, add, mul, unbind and their autograd) on the same
    device scalars.  Engine and yardstick alternate; a round is --calls calls between two host clocks with a device synchronise at
    its end, --rounds rounds after --warmup; medians of the rounds.  Both are HOST-bound (a few microseconds of device work): the
    figure is launch and autograd bookkeeping, not kernel time.  The ``sum()`` of the loop and its backward are in both.
(2) the cfg3 B = 256 bf16 step with ``--task_balancer uncertainty`` (amd_loop.task_balancer / create_optimizer's two groups /
    the tail entry point) against ``none`` (the one-group step), the bench configuration otherwise (direct gradients, adapter and
    weight-gradient streams), eager launches, device events around --steps steps; the two alternate and the order within a pair
    flips from one alternation to the next (none, uncertainty, then uncertainty, none, ...), so neither always runs first.

    python tools/task_balancer_bench.py [--out FILE] [--skip-step]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimae_amd as M  # noqa: E402
import bench  # noqa: E402
from dropin import amd_loop  # noqa: E402

DEV = 'cuda'


class EagerUncertainty(torch.nn.Module):
    """the yardstick: the same weighting written with torch operators"""

    def __init__(self, tasks):
        super().__init__()
        self.log_vars = torch.nn.Parameter(torch.zeros(len(tasks)))

    def forward(self, task_losses):
        stacked = torch.stack(list(task_losses.values()))
        keep = stacked != 0.0
        stacked = torch.exp(-self.log_vars) * stacked + self.log_vars
        stacked = stacked * keep
        return dict(zip(task_losses, stacked))


def module_bench(args):
    tasks = ['rgb', 'depth', 'semseg', 'norm_rgb']
    mods = {'fused': M.UncertaintyWeightingStrategy(tasks=tasks).to(DEV), 'eager': EagerUncertainty(tasks).to(DEV)}
    vals = torch.tensor([0.9, 0.4, 2.7, 0.8], device=DEV)
    losses = {k: vals[i].clone().requires_grad_() for i, k in enumerate(tasks)}

    def call(mod):
        weighted = mod(losses)
        sum(weighted.values()).backward()

    def one_round(mod):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(mod)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.calls * 1e6

    for mod in mods.values():
        for _ in range(args.warmup):
            one_round(mod)
    rounds = {k: [] for k in mods}
    for _ in range(args.rounds):
        for k, mod in mods.items():
            rounds[k].append(one_round(mod))
    # both computed the same thing
    gf, ge = mods['fused'].log_vars.grad, mods['eager'].log_vars.grad
    assert torch.allclose(gf, ge, rtol=1e-4), (gf, ge)          # (sums of some thousand identical contributions)
    # kernel launches of one call, counted by the profiler
    launches = {}
    for k, mod in mods.items():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
            call(mod)
            torch.cuda.synchronize()
        launches[k] = sum(1 for e in prof.events() if getattr(e, 'device_type', None) == torch.autograd.DeviceType.CUDA)
    med = {k: statistics.median(v) for k, v in rounds.items()}
    return dict(what='balancer forward + sum + backward per call, host clock with a synchronise per round (host-bound)', T=len(tasks),
                calls_per_round=args.calls, rounds=args.rounds, us_per_call_median=med, us_per_call_rounds=rounds,
                device_kernels_per_call=launches, eager_over_fused=med['eager'] / med['fused'])


def step_bench(args):
    B, n_vis = args.batch, 98
    res, runs = {}, {}
    for kind in ('none', 'uncertainty'):
        torch.manual_seed(0)
        model, doms = bench.build_model('cfg3')
        model.to(DEV)
        a = types.SimpleNamespace(opt='adamw', lr=1e-4, weight_decay=0.05, opt_eps=None, opt_betas=(0.9, 0.95), task_balancer=kind,
                                  balancer_lr_scale=1.0, out_domains=list(model.output_adapters))
        bal = amd_loop.task_balancer(a).to(DEV)
        model, reducer = amd_loop.wrap_model(model, a, balancer=bal)
        opt = amd_loop.create_optimizer(a, model, reducer, balancer=bal)
        scaler = amd_loop.LossScaler()
        x = bench.synthetic_batch(doms, B, torch.device(DEV), seed=0)
        tgt = dict(x, norm_rgb=x['rgb'])
        fns = bench.loss_fns()

        def step(model=model, opt=opt, bal=bal, scaler=scaler, x=x, tgt=tgt, fns=fns, a=a):
            for g in opt.param_groups:
                g['lr'] = a.lr * g['lr_scale']
            preds, masks = model(x, num_encoded_tokens=n_vis, alphas=1.0, sample_tasks_uniformly=False, fp32_output_adapters=['semseg'])
            mk = dict(masks, norm_rgb=masks['rgb'])
            losses = {k: fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds}
            loss = sum(bal(losses).values())
            opt.zero_grad()
            scaler(loss, opt, clip_grad=None, skip_grad=None, parameters=model.parameters())
        runs[kind] = (step, opt)
        res[kind] = []
    try:
        with M.engine.precision('bf16'):
            for step, _ in runs.values():
                for _ in range(args.step_warmup):
                    step()
            torch.cuda.synchronize()
            for alt in range(args.alternations):
                order = list(runs.items())
                for kind, (step, opt) in (order if alt % 2 == 0 else order[::-1]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        step()
                    e1.record()
                    torch.cuda.synchronize()
                    res[kind].append(e0.elapsed_time(e1) / args.steps)
    finally:
        M.engine.set_direct_grads(False); M.engine.set_adapter_streams(False); M.engine.set_wgrad_stream(False)
    counters = {k: opt.counters() for k, (_, opt) in runs.items()}
    med = {k: statistics.median(v) for k, v in res.items()}
    return dict(what=f'cfg3 B = {B} bf16 step, eager launches, device events around {args.steps} steps, alternating in one process, '
                     'the order within a pair flipped every alternation',
                ms_per_step_median=med, ms_per_step=res, uncertainty_minus_none_ms=med['uncertainty'] - med['none'], counters=counters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--step-warmup', type=int, default=4)
    ap.add_argument('--alternations', type=int, default=4)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, module=module_bench(args))
    if not args.skip_step:
        out['step'] = step_bench(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
