"""Curves of the REFERENCE with ``--task_balancer uncertainty`` on the mini geometry of make_golden.py (rgb + depth + semseg,
32 x 32, patch 8, 12 of 48 tokens, encoder 128 / 2 / 2, decoders 64 / 1 / 2; the four task losses of its output adapters), B = 4,
12 steps, mask draws seeded 1000 + step:

  * model, balancer (utils/task_balancing.py) and optimiser are the reference's own: ``create_optimizer(args, {'model': ..,
    'balancer': ..})`` (utils/optim_factory.py:138-174) with lr 1e-3, weight decay 0.05, betas (0.9, 0.95) and
    ``balancer_lr_scale`` 10, so ``log_vars`` moves visibly; the loop's ``g['lr'] = lr * g['lr_scale']``
    (run_pretraining_multimae.py:474-480) is applied with a constant schedule;
  * the loss-scaler sequence is utils/native_scaler.py:20-40 with ``parameters=model.parameters()`` as the loop passes it
    (:536-537) and a disabled GradScaler (CPU): backward, ``clip_grad_norm_`` over the MODEL's parameters when ``clip_grad`` is
    set, otherwise the 2-norm of their gradients, then ``optimizer.step()`` -- ``log_vars``' gradient is neither clipped nor in
    the norm;
  * run A: no clip.  run B: ``clip_grad`` = half the smallest norm of run A (clipping asserted active at every step).  run C: run
    A with model, balancer and inputs in float64 -- |A - C| is the reference's own f32 rounding of the trajectory.  run D: run A
    under ``torch.autocast('cpu', bfloat16)`` with ``fp32_output_adapters=['semseg']`` -- the reference's OWN bf16 deviation per
    step, which calibrates the engine's bf16-mode tolerance as in make_golden_curve_cfg3.py.

Per step: the task losses, the weighted losses, ``log_vars`` after the step and the returned norm; at the end the optimiser's
state for ``log_vars``.  ``log_vars`` and its state are recorded BY TASK, in the order of ``tasks``: the balancer pairs
``log_vars[i]`` with the i-th loss it is handed, and the reference's forward moves the ``fp32_output_adapters`` predictions to the
end of ``preds`` (multimae/multimae.py:357-377), so in run D the losses arrive as rgb, depth, norm_rgb, semseg and the parameter's
slots 2 and 3 hold the other task than in runs A-C (``loss_order`` records the order each run handed them over).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_balancer.py
"""
import contextlib
import importlib
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

STEPS, B, LR, WD, SCALE = 12, 4, 1e-3, 0.05, 10.0
DOMS, P, S, NVIS = ['rgb', 'depth', 'semseg'], 8, 32, 12


def run(ref, orc, clip, f64, bf16=False):
    rm, ria, roa, rc, tb, of = ref
    torch.manual_seed(0)
    model = mg.build_ref(rm, ria, roa, DOMS, P, S, enc=(128, 2, 2), dec_dim=64, dec_depth=1, dec_heads=2, class_emb=16)
    x = mg.make_inputs(DOMS, B, S)
    tasks = list(model.output_adapters)
    balancer = tb.UncertaintyWeightingStrategy(tasks=tasks)
    if f64:
        model.double(), balancer.double()
        x = {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
    args = types.SimpleNamespace(opt='adamw', lr=LR, weight_decay=WD, opt_eps=None, opt_betas=(0.9, 0.95), balancer_lr_scale=SCALE)
    opt = of.create_optimizer(args, {'model': model, 'balancer': balancer})
    fns = {'rgb': rc.MaskedMSELoss(P, 1), 'depth': rc.MaskedL1Loss(P, 1), 'semseg': rc.MaskedCrossEntropyLoss(P, 4),
           'norm_rgb': rc.MaskedMSELoss(P, 1, norm_pix=True)}
    tgt = dict(x, norm_rgb=x['rgb'])
    rec = dict(task_losses=[], weighted_losses=[], log_vars=[], norm=[])
    for step in range(1, STEPS + 1):
        for g in opt.param_groups:
            g['lr'] = LR * g['lr_scale']
        torch.manual_seed(1000 + step)
        dist, tn, an = orc.draw_mask_randoms(B, [(S // P) ** 2] * len(DOMS), 1.0)
        spt = orc.samples_per_task_from_dirichlet(dist, NVIS)
        mask_all, ik, ir = orc.masks_from_noise(spt, tn, an, NVIS)
        n = (S // P) ** 2
        tm = {d: mask_all[:, i * n:(i + 1) * n].contiguous() for i, d in enumerate(DOMS)}
        model.generate_random_masks = lambda *a, **k: (tm, ik, ir)
        with (torch.autocast('cpu', dtype=torch.bfloat16) if bf16 else contextlib.nullcontext()):
            preds, masks = model(x, num_encoded_tokens=NVIS, alphas=1.0, fp32_output_adapters=['semseg'] if bf16 else [])
            mk = dict(masks, norm_rgb=masks['rgb'])
            losses = {k: fns[k](preds[k] if f64 else preds[k].float(), tgt[k], mask=mk[k]) for k in preds}
            weighted = balancer(losses)
            loss = sum(weighted.values())
        opt.zero_grad()
        loss.backward()
        if clip is not None:
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            assert float(norm) > clip, (step, float(norm), clip)          # clipping is active
        else:
            norm = torch.norm(torch.stack([torch.norm(p.grad.detach(), 2.0) for p in model.parameters() if p.grad is not None]), 2.0)
        opt.step()
        rec['task_losses'].append({k: float(v) for k, v in losses.items()})
        rec['weighted_losses'].append({k: float(v) for k, v in weighted.items()})
        order = list(losses)                                              # log_vars[i] belongs to the i-th loss handed over
        assert rec.setdefault('loss_order', order) == order and sorted(order) == sorted(tasks)
        rec['log_vars'].append([float(balancer.log_vars[order.index(t)]) for t in tasks])
        rec['norm'].append(float(norm))
    st = opt.state[balancer.log_vars]
    rec['log_vars_state'] = dict(step=int(float(st['step'])), exp_avg=[float(st['exp_avg'][order.index(t)]) for t in tasks],
                                 exp_avg_sq=[float(st['exp_avg_sq'][order.index(t)]) for t in tasks])
    rec['param_groups'] = [{k: v for k, v in g.items() if k != 'params'} | {'n_params': len(g['params'])} for g in opt.param_groups]
    return rec, tasks


def main():
    torch.set_num_threads(8)
    rm, ria, roa, rc = mg.import_reference()
    tb = importlib.import_module('utils.task_balancing')
    of = importlib.import_module('utils.optim_factory')
    orc = mg.load_oracle()
    ref = (rm, ria, roa, rc, tb, of)
    a, tasks = run(ref, orc, None, False)
    clip = 0.5 * min(a['norm'])
    b, _ = run(ref, orc, clip, False)
    c, _ = run(ref, orc, None, True)
    d, _ = run(ref, orc, None, False, bf16=True)
    tot = lambda r: [sum(s.values()) for s in r['weighted_losses']]
    print('max |run D - run A| of the weighted total:', max(abs(p - q) for p, q in zip(tot(a), tot(d))))
    dev = [max(abs(p - q) for p, q in zip(u, v)) for u, v in zip(a['log_vars'], c['log_vars'])]
    print('log_vars after the last step (run A):', a['log_vars'][-1])
    print('max |run A - run C| of log_vars per step:', dev)
    json.dump({'recipe': f'mini rgb+depth+semseg 32x32 patch 8, {NVIS} of 48 tokens, tasks {tasks}, B={B}, AdamW lr {LR} (.9,.95) wd {WD}, '
                         f'balancer_lr_scale {SCALE}, mask seed 1000+step, {STEPS} steps',
               'tasks': tasks, 'lr': LR, 'weight_decay': WD, 'balancer_lr_scale': SCALE, 'steps': STEPS, 'clip_grad_run_b': clip,
               'run_a': a, 'run_b': b, 'run_c_f64': c, 'run_d_bf16_autocast': d, 'torch_version': torch.__version__},
              open(os.path.join(HERE, 'balancer_curve.json'), 'w'), indent=1)


if __name__ == '__main__':
    main()
