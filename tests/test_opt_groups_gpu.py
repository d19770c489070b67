"""GPU: the grouped AdamW step (mmae_opt_step_groups, FusedAdamW(groups=...)) against torch.optim.AdamW over the same groups,
bit-identity with mmae_opt_step for one group, the device-side skips, a fine-tuning loop of a small MultiViT with a linear head,
hipGraph replay with per-group values changed between replays, and the group counts of ViT-L / the 256-group limit."""
import math
import types

import pytest
import torch
from torch import nn

import multimae_amd as M
from multimae_amd import ops
from multimae_amd.optim import FusedAdamW
from dropin import amd_loop

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIZES = [37, 130, 1000, 65, 7, 300, 2049, 90, 513, 11]          # none a multiple of 64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _plist(seed=0):
    g = torch.Generator().manual_seed(seed)
    return nn.ParameterList([nn.Parameter(torch.randn(n, generator=g)) for n in SIZES]).to(DEV)


def _groups(params):
    """5 groups with their own lr / weight_decay, members out of registration order."""
    ps = list(params)
    members = [[ps[6], ps[0]], [ps[1], ps[9], ps[4]], [ps[2]], [ps[3], ps[7]], [ps[8], ps[5]]]
    return [dict(params=m, lr=1e-2 * (k + 1), weight_decay=(0.0, 0.05, 0.1, 0.2, 0.01)[k], lr_scale=1.0) for k, m in enumerate(members)]


def _grads(step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(n, generator=g) * scale for n in SIZES]


def test_grouped_step_matches_torch_adamw():
    """10 tensors, 5 groups, 4 steps with clip_grad: rel. error <= 1e-6 per tensor; the alignment padding stays 0."""
    fused_p, ref_p = _plist(), _plist()
    opt = FusedAdamW(fused_p, betas=(0.9, 0.999), eps=1e-8, clip_grad=1.0, groups=_groups(fused_p))
    ref = torch.optim.AdamW(_groups(ref_p), betas=(0.9, 0.999), eps=1e-8, foreach=False)
    for step in range(4):
        for k, (g, r) in enumerate(zip(opt.param_groups, ref.param_groups)):
            g['lr'] = r['lr'] = 1e-2 * (k + 1) * (0.5 + 0.25 * step)
        for p, q, gr in zip(fused_p, ref_p, _grads(step, scale=0.3)):
            p.grad.copy_(gr)
            q.grad = gr.to(DEV)
        opt.step()
        torch.nn.utils.clip_grad_norm_(list(ref_p), 1.0)
        ref.step()
    torch.cuda.synchronize()
    assert opt.step_count == 4
    for i, (p, q) in enumerate(zip(fused_p, ref_p)):
        assert rel(p, q) <= 1e-6, (i, rel(p, q))
    a = opt.arena
    for n in a.names:
        o, s = a.offsets[n], a.sizes[n]
        pad = slice(o + s, (o + s + 63) // 64 * 64)
        assert not a.param[pad].any() and not opt.m[pad].any() and not opt.v[pad].any(), n


def _arena_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(DEV)
    p[n - 40:] = 0                                       # a padded tail
    return dict(p=p, m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV), state=torch.zeros(8, device=DEV),
                istate=torch.zeros(8, device=DEV, dtype=torch.int32), ws=torch.empty(1024, device=DEV),
                shadow=torch.zeros(n, device=DEV, dtype=torch.bfloat16))


def _run(s, grads, grouped, losses=None, skip_grad=None, clip_grad=1.0, hyper_dev=False):
    n = s['p'].numel()
    gm = torch.zeros((n + 63) // 64, dtype=torch.int16, device=DEV)
    table = torch.tensor([[3e-3, 0.05]], device=DEV)
    for t, gr in enumerate(grads):
        loss = None if losses is None else torch.tensor([losses[t]], device=DEV)
        kw = dict(beta1=0.9, beta2=0.95, eps=1e-8, clip_grad=clip_grad, skip_grad=skip_grad, loss_dev=loss, shadow=s['shadow'])
        if grouped:
            ops.opt_step_groups(s['p'], gr, s['m'], s['v'], s['state'], s['istate'], s['ws'], group_map=gm, n_groups=1,
                                hyper=None if hyper_dev else [3e-3, 0.05], hyper_dev=table if hyper_dev else None, **kw)
        else:
            ops.opt_step(s['p'], gr, s['m'], s['v'], s['state'], s['istate'], s['ws'], lr=3e-3, weight_decay=0.05, **kw)
    torch.cuda.synchronize()


def test_one_group_is_bit_identical_to_opt_step():
    n = 64 * 4099
    g = torch.Generator().manual_seed(5)
    grads = [(torch.randn(n, generator=g) * 0.01).to(DEV) for _ in range(3)]
    for gr in grads:
        gr[n - 40:] = 0
    single = _arena_state(n, 1)
    _run(single, grads, False)
    for hyper_dev in (False, True):
        grouped = _arena_state(n, 1)
        _run(grouped, grads, True, hyper_dev=hyper_dev)
        for k in ('p', 'm', 'v', 'state', 'istate', 'shadow'):
            assert torch.equal(grouped[k], single[k]), (hyper_dev, k)
    assert int(single['istate'][1]) == 3 and float(single['state'][2]) < 1.0      # clipping acted


def test_skips_move_no_group():
    """A NaN gradient, a non-finite loss and skip_grad: nothing moves, t stays, the counters equal the single-group ones."""
    n = 64 * 300
    g = torch.Generator().manual_seed(9)
    grads = [(torch.randn(n, generator=g) * 0.01).to(DEV) for _ in range(4)]
    grads[1][77] = float('nan')
    losses = [1.0, 1.0, float('inf'), 1.0]
    res = {}
    for grouped in (False, True):
        s = _arena_state(n, 2)
        _run(s, grads[:1], grouped, losses=losses[:1])
        p1 = s['p'].clone()
        _run(s, grads[1:3], grouped, losses=losses[1:3])         # NaN gradient, then a non-finite loss
        assert torch.equal(s['p'], p1) and int(s['istate'][1]) == 1
        _run(s, grads[3:], grouped, losses=losses[3:], skip_grad=1e-9, clip_grad=None)
        assert torch.equal(s['p'], p1) and int(s['istate'][1]) == 1
        res[grouped] = s
    assert torch.equal(res[True]['istate'], res[False]['istate'])
    assert res[True]['istate'].tolist()[:6] == [1, 1, 1, 3, 0, 1]


def _layer_id(name, n):
    if name == 'global_tokens' or name.startswith('input_adapters'):
        return 0
    if name.startswith('encoder'):
        return int(name.split('.')[1]) + 1
    return n - 1


def _finetune_setup(seed=3):
    torch.manual_seed(seed)
    ins = {'rgb': M.PatchedInputAdapter(3, 1, 8, image_size=32)}
    outs = {'cls': M.LinearOutputAdapter(num_classes=16, use_mean_pooling=True)}       # bf16 GEMMs: multiples of 8
    model = M.MultiViT(ins, outs, num_global_tokens=1, dim_tokens=128, depth=2, num_heads=2).to(DEV)
    model.build_arena()
    L = model.get_num_layers()
    values = [0.75 ** (L + 1 - i) for i in range(L + 2)]
    args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=(0.9, 0.999))
    opt = amd_loop.create_optimizer_groups(args, model, skip_list=model.no_weight_decay(),
                                           get_num_layer=lambda nm: _layer_id(nm, L + 2), get_layer_scale=lambda k: values[k])
    return model, opt


def _schedule(groups, it, n):
    for g in groups:
        g['lr'] = 1e-3 * 0.5 * (1 + math.cos(math.pi * it / n)) * g['lr_scale']
        if g['weight_decay'] > 0:
            g['weight_decay'] = 0.05 + 0.01 * it


def test_finetuning_loop_matches_torch_adamw_over_the_same_groups():
    """5 steps of the fine-tuning loop (per-group cosine lr x lr_scale, a weight-decay schedule, clip 5.0) in fp32 with direct
    gradients, against torch.optim.AdamW over the same groups fed the same gradients: rel. error <= 1e-5 per tensor.  Then two
    bf16 steps: the shadow is the cast of the parameters after each."""
    model, opt = _finetune_setup()
    assert len(opt.param_groups) == 8
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = dict(model.named_parameters())
    ref_p = {n: params[n].detach().clone().requires_grad_(True) for n in names}
    ref = torch.optim.AdamW([dict(params=[ref_p[n] for n in nms], weight_decay=g['weight_decay'], lr_scale=g['lr_scale'])
                             for g, nms in zip(opt.param_groups, opt.group_names)], lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                            foreach=False)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(4, 3, 32, 32, generator=gen).to(DEV)
    y = torch.randint(0, 16, (4,), generator=gen).to(DEV)
    M.engine.set_direct_grads(True)
    try:
        with M.engine.precision('fp32'):
            for it in range(5):
                _schedule(opt.param_groups, it, 5)
                _schedule(ref.param_groups, it, 5)
                opt.zero_grad()
                loss = nn.functional.cross_entropy(model(x)['cls'], y)
                loss.backward()
                for n in names:
                    ref_p[n].grad = params[n].grad.detach().clone()
                torch.nn.utils.clip_grad_norm_(list(ref_p.values()), 5.0)
                ref.step()
                opt.clip_grad = 5.0
                opt.step(loss)
            torch.cuda.synchronize()
        assert opt.step_count == 5
        for n in names:
            assert rel(params[n], ref_p[n]) <= 1e-5, (n, rel(params[n], ref_p[n]))
        a, nt = opt.arena, opt.arena.n_trainable
        with M.engine.precision('bf16'):
            for it in range(2):
                opt.zero_grad()
                loss = nn.functional.cross_entropy(model(x)['cls'].float(), y)
                loss.backward()
                opt.step(loss)
                torch.cuda.synchronize()
                assert a.shadow is not None and torch.equal(a.shadow[:nt], a.param[:nt].to(a.shadow.dtype)), it
        assert opt.step_count == 7
    finally:
        M.engine.set_direct_grads(False)


def test_graph_replay_takes_per_group_lr_changes():
    """The step captured in a hipGraph (graph.StepGraph): a per-group lr changed between replays takes effect, bit-equal to the
    same steps run eagerly."""
    from multimae_amd.graph import StepGraph
    eager_p, graph_p = _plist(), _plist()
    eager = FusedAdamW(eager_p, betas=(0.9, 0.999), clip_grad=1.0, groups=_groups(eager_p))
    graphed = FusedAdamW(graph_p, betas=(0.9, 0.999), clip_grad=1.0, groups=_groups(graph_p))
    run = StepGraph(lambda: graphed.step())
    for step in range(4):
        for opt, params in ((eager, eager_p), (graphed, graph_p)):
            for k, g in enumerate(opt.param_groups):
                g['lr'] = 1e-2 * (k + 1) * (1.0 + step) * (0.0 if (k == 2 and step == 2) else 1.0)
            for p, gr in zip(params, _grads(step)):
                p.grad.copy_(gr)
        eager.step()
        if step == 0:
            graphed.step()                               # one eager step first, as bench.py does
        else:
            p2 = graph_p[2].detach().clone()
            run()
            torch.cuda.synchronize()
            if step == 2:                                # group 2 had lr 0 (and decays nothing): it did not move
                assert torch.equal(graph_p[2], p2)
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(graph_p, eager_p)):
            assert torch.equal(p, q), (step, i)
    assert run.replays == 3 and graphed.step_count == 4


def test_group_counts_vit_large_and_256():
    """multivit_large's 52 groups and a synthetic 256-group case run; each group gets its own lr / weight_decay (first AdamW step
    from zero moments: p (1 - lr wd) - lr g / (|g| + eps))."""
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=224)}
    large = M.multivit_large(input_adapters=ins, output_adapters={'cls': M.LinearOutputAdapter(num_classes=1000)},
                             num_global_tokens=1).to(DEV)
    L = large.get_num_layers()
    values = [0.75 ** (L + 1 - i) for i in range(L + 2)]
    args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05)
    cases = []
    opt = amd_loop.create_optimizer_groups(args, large, skip_list=large.no_weight_decay(),
                                           get_num_layer=lambda nm: _layer_id(nm, L + 2), get_layer_scale=lambda k: values[k])
    assert len(opt.param_groups) == 52
    cases.append(opt)
    many = nn.ParameterList([nn.Parameter(torch.randn(3 + k % 70)) for k in range(300)]).to(DEV)
    ps = list(many)
    cases.append(FusedAdamW(many, groups=[dict(params=ps[k::256]) for k in range(256)]))
    for opt in cases:
        for k, g in enumerate(opt.param_groups):
            g['lr'] = 1e-3 * g['lr_scale'] * (1 + k % 7)
            g['weight_decay'] = 0.01 * (k % 5)
        before = opt.arena.param.clone()
        opt.arena.grad.normal_()
        opt.step()
        torch.cuda.synchronize()
        a = opt.arena
        for g, names in zip(opt.param_groups, opt.group_names):
            for nm in (names[0], names[-1]):
                o, s = a.offsets[nm], a.sizes[nm]
                p0, gr = before[o:o + s], a.grad[o:o + s]
                exp = p0 * (1 - g['lr'] * g['weight_decay']) - g['lr'] * gr / (gr.abs() + 1e-8)
                assert rel(a.param[o:o + s], exp) < 1e-6, nm
        assert opt.step_count == 1
