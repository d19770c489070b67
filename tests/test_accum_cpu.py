"""CPU, world_size 2, gloo: gradient accumulation (``--update_freq 2``) under data parallelism.

Two micro-backwards of the real model (host control flow on the stubbed C ABI, direct gradients on), the first through
``LossScaler(update_grad=False)``, must leave on every rank exactly the all-reduced sum of both micro-gradients, and no collective may
be launched during the first (held) backward.  The stubbed kernels write nothing, so the micro-gradients are stand-ins filled / added
into the gradient arena before each backward: small integers, so that every sum is exact.

Before ``GradAllReducer.hold()`` existed this failed for a behavioural reason, not only at import: ``update_grad=False`` merely skipped
the optimiser, the first backward's readiness reports launched every bucket but the tail, the second micro-gradient was added onto
already-reduced sums and never exchanged -- the result was ``sum_ranks(g1) + g2_local`` instead of ``sum_ranks(g1 + g2)``.
"""
import os
import socket
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [here, os.path.join(os.path.dirname(here), 'oracle'), os.path.dirname(here)]
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        import dryrun_harness
        dryrun_harness.install()
        import multimae_amd as M
        from dropin import amd_loop
        from helpers import MINI, build_mini_engine, load_mini
        torch.manual_seed(100)
        model = build_mini_engine()
        model, red = amd_loop.wrap_model(model, bucket_mb=0.25)
        assert red is not None and M.engine.direct_grads()
        args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
        opt = amd_loop.create_optimizer(args, model)
        scaler = amd_loop.LossScaler()
        arena = model.build_arena()
        order = []
        launch = red._launch
        red._launch = lambda i: (order.append(i) if not red._launched[i] else None, launch(i))[1]
        g = load_mini()
        P = MINI['P']
        fns = {'rgb': M.MaskedMSELoss(P, 1), 'depth': M.MaskedL1Loss(P, 1), 'semseg': M.MaskedCrossEntropyLoss(P, 4),
               'norm_rgb': M.MaskedMSELoss(P, 1, norm_pix=True)}

        def micro_loss():
            with M.engine.precision('bf16'):
                preds, masks = model(g['x'], num_encoded_tokens=MINI['nvis'], alphas=1.0, fp32_output_adapters=['semseg'])
                mk = dict(masks, norm_rgb=masks['rgb'])
                tgt = dict(g['x'], norm_rgb=g['x']['rgb'])
                return sum(fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds) / 2

        opt.zero_grad()
        arena.grad.fill_(float(rank + 1))                          # micro-gradient 1 (stand-in)
        ret = scaler(micro_loss(), opt, update_grad=False)
        held_launches, held_handles = list(order), len(red._handles)
        arena.grad.add_(10.0 * (rank + 1))                         # micro-gradient 2, accumulated onto the local partial sum
        scaler(micro_loss(), opt, clip_grad=None, update_grad=True)
        total = float(sum(r + 1 for r in range(world)) * 11)
        exact = bool(torch.equal(arena.grad, torch.full_like(arena.grad, total)))
        q.put((rank, ret is None, held_launches, held_handles, list(order), len(red.buckets), exact,
               sorted(set(arena.grad.tolist()))[:4]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:          # noqa: BLE001
        import traceback
        q.put((rank, 'error', traceback.format_exc()))


def test_accumulated_micro_gradients_are_reduced_once_world2_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    for r in res:
        assert r[1] != 'error', r[2]
        rank, ret_none, held_launches, held_handles, order, nb, exact, values = r
        assert ret_none, 'LossScaler(update_grad=False) returns None'
        assert held_launches == [] and held_handles == 0, f'rank {rank}: collectives launched during the held backward: {held_launches}'
        assert nb >= 4 and len(order) == nb and order == sorted(order), (order, nb)     # the last micro-step launches every bucket, in order
        assert exact, f'rank {rank}: gradient values {values}, expected {33.0} everywhere'
    assert res[0][4] == res[1][4], 'ranks must issue their collectives in the same order'


def test_hold_is_reentrant_and_released_on_error():
    from multimae_amd.dist import GradAllReducer
    grad = torch.zeros(256)
    red = GradAllReducer(grad, [('a', 0, 128), ('b', 128, 128)], bucket_mb=128 * 4 / 2 ** 20)
    try:
        with red.hold():
            with red.hold():
                red.mark_ready(['a'])
            red.mark_ready(['a', 'b'])
            assert red._remaining == [1, 1] and not any(red._launched)
            raise KeyError('boom')
    except KeyError:
        pass
    assert red._held == 0
    red.mark_ready(['a'])
    assert red._launched == [True, False] and red._remaining == [0, 1]
