"""CPU, world 2 over gloo (the harness of tests/test_dist_cpu.py): the uncertainty balancer's ``log_vars`` under data parallelism.
The reference wraps the balancer in DistributedDataParallel as well (run_pretraining_multimae.py:385-387): every rank starts from
rank 0's ``log_vars`` and steps it with the rank MEAN of its gradient.  Here ``amd_loop.wrap_model(..., balancer=...)`` puts it into
the arena, so the parameter broadcast, the reducer's last bucket and the optimiser's 1 / world gradient scale cover it.  The C ABI is
the type-checking stub (kernels do not run on CPU): the test reads the gradient arena after the exchange and the arguments of the
fused step, applies that step's AdamW update to ``log_vars`` with torch.optim.AdamW, and compares the ranks.

What this shows and what it does not: both ranks START the step with rank 0's ``log_vars``, the gradient arena holds the rank SUM
after the exchange, and the fused call is handed the 1 / world scale and the model-only norm prefix on both ranks -- the same inputs.
The fused kernel itself does not run here, so "both ranks END the engine's own step with identical ``log_vars``" is an inference from
identical inputs to a deterministic kernel (tests/test_task_balancer_gpu.py checks that kernel and its bit-reproducibility on one
GPU); ``end_same`` below compares a torch.optim.AdamW emulation of the step, not the step."""
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

TASKS = ['rgb', 'depth', 'semseg', 'norm_rgb']


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _losses(rank):
    """Rank-dependent task losses (one exactly zero on rank 1: its weighted loss and both gradients are masked there only)."""
    vals = [[1.5, 0.25, 3.0, 0.75], [0.5, 2.0, 0.0, 1.25]][rank]
    return {k: torch.tensor(v) for k, v in zip(TASKS, vals)}


def _worker(rank, world, port, q):
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        root = os.path.dirname(here)
        sys.path[:0] = [here, os.path.join(root, 'oracle'), root]
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        import dryrun_harness
        dryrun_harness.install()
        import multimae_amd as M
        from multimae_amd import _lib
        from dropin import amd_loop
        from helpers import build_mini_engine
        calls = []
        fake = _lib._lib

        class Recorder:
            def __getattr__(self, name):
                fn = getattr(fake, name)

                def rec(*args):
                    if name.startswith('mmae_opt_step'):
                        d = args[0]._obj
                        calls.append((name, float(d.grad_prescale), int(args[1]), int(d.n)))
                    return fn(*args)
                return rec
        _lib._lib = Recorder()
        torch.manual_seed(100 + rank)                 # the script seeds every rank differently (run_pretraining_multimae.py:300-302)
        model = build_mini_engine()
        args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=None, opt_betas=(0.9, 0.95),
                                     task_balancer='uncertainty', balancer_lr_scale=10.0, out_domains=list(TASKS))
        bal = amd_loop.task_balancer(args)
        with torch.no_grad():
            bal.log_vars.copy_(torch.tensor([0.1, -0.2, 0.3, 0.05]) * (rank + 1))          # differs per rank before the wrap
        model, reducer = amd_loop.wrap_model(model, args, bucket_mb=0.25, balancer=bal)
        opt = amd_loop.create_optimizer(args, model, reducer, balancer=bal)
        assert reducer is not None and opt.grad_prescale == 0.5 and reducer.buckets[-1][2][-1] == 'balancer.log_vars'
        lv0 = bal.log_vars.detach().clone()
        start = [torch.empty_like(lv0) for _ in range(world)]
        dist.all_gather(start, lv0)
        for g in opt.param_groups:
            g['lr'] = args.lr * g['lr_scale']
        opt.zero_grad()
        arena = opt.arena
        arena.grad[:opt.n_norm].fill_(float(rank + 1))                                    # stand-in model gradients
        losses = _losses(rank)
        weighted = bal(losses)
        scaler = amd_loop.LossScaler()
        scaler(sum(weighted.values()), opt, clip_grad=None, skip_grad=None, parameters=model.parameters())
        off = arena.offsets['balancer.log_vars']
        g_sum = arena.grad[off:off + 4].clone()                                           # after the exchange: the rank SUM
        mine = 1.0 - torch.exp(-lv0) * torch.stack(list(losses.values()))
        mine = mine * (torch.stack(list(losses.values())) != 0)
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        name, prescale, n_norm, n = calls[-1]
        # the step the library call describes, applied to log_vars: AdamW with the averaged gradient, lr * lr_scale, decay
        p = torch.nn.Parameter(lv0.clone())
        ref = torch.optim.AdamW([p], lr=opt.param_groups[1]['lr'], betas=(0.9, 0.95), weight_decay=opt.param_groups[1]['weight_decay'])
        p.grad = g_sum * prescale
        ref.step()
        end = [torch.empty_like(lv0) for _ in range(world)]
        dist.all_gather(end, p.detach())
        q.put((rank, dict(start_same=bool(torch.equal(start[0], start[1])), start_is_rank0=bool(torch.equal(lv0, torch.tensor([0.1, -0.2, 0.3, 0.05]))),
                          grad_is_sum=bool(torch.allclose(g_sum, both[0] + both[1], rtol=1e-6, atol=1e-7)),
                          grad_mean=bool(torch.allclose(g_sum * prescale, (both[0] + both[1]) / 2, rtol=1e-6, atol=1e-7)),
                          ranks_differ=bool(not torch.equal(both[0], both[1])), masked=float(both[1][2]),
                          end_same=bool(torch.equal(end[0], end[1])), moved=bool(not torch.equal(end[0], lv0)),
                          call=(name, prescale, n_norm == off, n == arena.n_trainable),
                          model_grad=bool(torch.equal(arena.grad[:opt.n_norm], torch.full((opt.n_norm,), 3.0))))))
        dist.destroy_process_group()
    except Exception:          # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def test_log_vars_is_broadcast_and_stepped_with_the_rank_mean_world2_gloo():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    for rank, r in res:
        assert isinstance(r, dict), f'rank {rank}: {r}'
        assert r['start_same'] and r['start_is_rank0'], (rank, r)                 # DDP-constructor semantics for the balancer too
        assert r['ranks_differ'] and r['masked'] == 0.0, (rank, r)
        assert r['grad_is_sum'] and r['grad_mean'] and r['model_grad'], (rank, r)   # summed in the last bucket, averaged by the step's scale
        assert r['call'] == ('mmae_opt_step_groups_tail', 0.5, True, True), (rank, r)
        assert r['end_same'] and r['moved'], (rank, r)                            # both ranks end the step with identical log_vars
