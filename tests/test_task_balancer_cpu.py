"""CPU: the uncertainty task balancer on the fused pre-training path -- the module against the reference's contract
(utils/task_balancing.py:21-44), ``log_vars`` at the end of the arena's trainable prefix, the two param groups of
utils/optim_factory.py:138-150 with the balancer's outside the gradient norm, the two-group checkpoint interchange, the new
library symbols, and the patched pre-training script's dry run with ``--task_balancer uncertainty``."""
import ctypes
import os
import subprocess
import sys
import types

import pytest
import torch
from torch import nn

import multimae_amd as M
from multimae_amd import _lib, checkpoint as ck, engine
from multimae_amd.optim import FusedAdamW
from dropin import amd_loop
from helpers import build_mini_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ['rgb', 'depth', 'semseg', 'norm_rgb']


def _args(**kw):
    a = dict(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=None, opt_betas=(0.9, 0.95), task_balancer='uncertainty',
             balancer_lr_scale=10.0, out_domains=list(TASKS))
    a.update(kw)
    return types.SimpleNamespace(**a)


# ------------------------------------------------------------------------------------------ the module
def test_module_parity_with_the_reference_contract():
    b = M.UncertaintyWeightingStrategy(tasks=TASKS)
    assert b.tasks == TASKS and isinstance(b.log_vars, nn.Parameter) and b.log_vars.shape == (4,) and b.log_vars.requires_grad
    assert torch.equal(b.log_vars.detach(), torch.zeros(4)) and b.log_vars.dtype == torch.float32
    assert list(b.state_dict()) == ['log_vars'] and [n for n, _ in b.named_parameters()] == ['log_vars']
    # a reference-format 'loss_balancer' checkpoint entry (an OrderedDict with the one key) loads strictly
    ref_entry = {'log_vars': torch.tensor([0.25, -0.5, 1.0, 0.0])}
    assert b.load_state_dict(ref_entry, strict=True).missing_keys == []
    assert torch.equal(b.log_vars.detach(), ref_entry['log_vars'])
    with pytest.raises(RuntimeError):
        b.load_state_dict({'log_vars': torch.zeros(4), 'other': torch.zeros(1)}, strict=True)
    n = M.NoWeightingStrategy()
    losses = {'rgb': torch.tensor(1.0)}
    assert n(losses) is losses and list(n.state_dict()) == [] and list(n.parameters()) == []
    M.NoWeightingStrategy(tasks=TASKS)                   # the reference's constructor swallows keyword arguments
    with pytest.raises(ValueError):
        M.UncertaintyWeightingStrategy(tasks=[str(i) for i in range(17)])
    assert isinstance(amd_loop.task_balancer(_args()), M.UncertaintyWeightingStrategy)
    assert amd_loop.task_balancer(_args()).tasks == TASKS
    assert isinstance(amd_loop.task_balancer(_args(task_balancer='none')), M.NoWeightingStrategy)
    with pytest.raises(ValueError):
        amd_loop.task_balancer(_args(task_balancer='gradnorm'))


@pytest.mark.parametrize('T', [1, 3])
def test_cpu_forward_backward_equal_the_formula(T):
    """w_i = (exp(-s_i) L_i + s_i) (L_i != 0) and its gradients in f64, an exact-zero loss included."""
    g = torch.Generator().manual_seed(T)
    s = (torch.rand(T, generator=g, dtype=torch.float64) * 6 - 3)
    L = torch.rand(T, generator=g, dtype=torch.float64) * 4 - 1
    if T > 1:
        L[1] = 0.0
    u = torch.rand(T, generator=g, dtype=torch.float64) + 0.5
    keys = [f't{i}' for i in range(T)]
    b = M.UncertaintyWeightingStrategy(tasks=keys).double()
    with torch.no_grad():
        b.log_vars.copy_(s)
    losses = {k: L[i].clone().requires_grad_() for i, k in enumerate(keys)}
    out = b(losses)
    assert list(out) == keys and all(out[k].shape == () for k in keys)
    sum(u[i] * out[k] for i, k in enumerate(keys)).backward()
    m = (L != 0).double()
    e = torch.exp(-s)
    assert torch.allclose(torch.stack([out[k].detach() for k in keys]), (e * L + s) * m, rtol=1e-14, atol=0)
    assert torch.allclose(torch.stack([losses[k].grad for k in keys]), u * e * m, rtol=1e-14, atol=0)
    assert torch.allclose(b.log_vars.grad, u * (1 - e * L) * m, rtol=1e-14, atol=1e-300)
    if T > 1:
        assert float(out['t1'].detach()) == 0.0 and float(b.log_vars.grad[1]) == 0.0 and float(losses['t1'].grad) == 0.0
    with pytest.raises(ValueError, match=f'{T + 1} task losses.*{T} log_vars'):
        b(dict(losses, extra=torch.tensor(1.0, dtype=torch.float64)))


# ------------------------------------------------------------------------------------------ the arena
def test_log_vars_is_the_last_trainable_tensor_of_the_arena():
    torch.manual_seed(0)
    model = build_mini_engine()
    next(p for n, p in model.named_parameters() if n.endswith('pos_emb')).requires_grad_(False)      # a frozen tensor behind the prefix
    bal = M.UncertaintyWeightingStrategy(tasks=TASKS)
    with torch.no_grad():
        bal.log_vars.copy_(torch.tensor([0.1, 0.2, 0.3, 0.4]))
    sd_model = {k: v.clone() for k, v in model.state_dict().items()}
    plain = model.build_arena()
    assert plain.extra_names == [] and 'balancer.log_vars' not in plain.offsets
    model, reducer = amd_loop.wrap_model(model, _args(), balancer=bal)
    try:
        a = engine.arena_of(model)
        assert a is not plain and reducer is None and a.intact()
        names = [n for n, _ in model.named_parameters()]
        assert a.param_order == names + ['balancer.log_vars'] and a.extra_names == ['balancer.log_vars']
        trainable = [n for n in a.names if a.trainable[n]]
        assert trainable[-1] == 'balancer.log_vars' and a.names.index('balancer.log_vars') == len(trainable) - 1
        off = a.offsets['balancer.log_vars']
        assert off % engine.ALIGN == 0 and off + engine.ALIGN == a.n_trainable          # a 64-element chunk of its own, the prefix's last
        assert all(a.offsets[n] + a.sizes[n] <= off for n in trainable[:-1])
        assert bal.log_vars.data_ptr() == a.param.data_ptr() + 4 * off and bal.log_vars.grad.data_ptr() == a.grad.data_ptr() + 4 * off
        assert a.tail_names()[-1] == 'balancer.log_vars' and a.tail_names()[0] != 'balancer.log_vars'     # the last bucket's, not one of its own
        # neither state dict changed
        assert list(bal.state_dict()) == ['log_vars'] and torch.equal(bal.state_dict()['log_vars'], torch.tensor([0.1, 0.2, 0.3, 0.4]))
        after = model.state_dict()
        assert list(after) == list(sd_model) and all(torch.equal(after[k], v) for k, v in sd_model.items())
        assert model.build_arena(extra={'balancer': bal}) is a and model.build_arena() is a                # idempotent
        from multimae_amd import dist as mdist
        buckets = mdist.GradAllReducer.for_arena(a, bucket_mb=1e-3).buckets
        assert buckets[-1][2][-1] == 'balancer.log_vars' and len(buckets[-1][2]) > 1 and buckets[-1][1] == a.n_trainable
        with pytest.raises(ValueError):
            engine.ParamArena(nn.Linear(2, 2), extra=[('balancer.log_vars', nn.Parameter(torch.zeros(2), requires_grad=False))])
    finally:
        M.engine.set_direct_grads(False)


# ------------------------------------------------------------------------------------------ the optimiser's groups
def test_create_optimizer_builds_the_two_groups_of_the_reference_factory():
    """Fails on a tree without the feature: the construction raised "trainable balancer weights outside the arena"."""
    torch.manual_seed(0)
    model = build_mini_engine()
    bal = amd_loop.task_balancer(_args())
    args = _args()
    try:
        model, reducer = amd_loop.wrap_model(model, args, balancer=bal)
        opt = amd_loop.create_optimizer(args, model, reducer, balancer=bal)
        assert isinstance(opt, FusedAdamW) and len(opt.param_groups) == 2
        g0, g1 = opt.param_groups
        assert [id(p) for p in g0['params']] == [id(p) for _, p in model.named_parameters() if p.requires_grad]
        assert len(g1['params']) == 1 and g1['params'][0] is bal.log_vars
        assert (g0['lr_scale'], g1['lr_scale']) == (1.0, 10.0)
        assert g0['weight_decay'] == g1['weight_decay'] == 0.05                       # log_vars decays too
        assert g0['lr'] == g1['lr'] == 1e-3 and tuple(g0['betas']) == (0.9, 0.95)     # the loop multiplies by lr_scale per iteration
        assert opt.group_names[1] == ['balancer.log_vars']
        assert opt.n_norm == opt.arena.offsets['balancer.log_vars'] == opt.arena.n_trainable - 64
        assert opt._group_map[-1] == 1 and (opt._group_map[:-1] == 0).all()
        # uncertainty without the balancer, or with one that is not in the arena: ValueError
        with pytest.raises(ValueError, match='balancer'):
            amd_loop.create_optimizer(args, model, reducer)
        with pytest.raises(ValueError, match='balancer'):
            amd_loop.create_optimizer(args, model, reducer, balancer=M.NoWeightingStrategy())
        with pytest.raises(ValueError, match='wrap_model'):
            amd_loop.create_optimizer(args, model, reducer, balancer=M.UncertaintyWeightingStrategy(tasks=TASKS))
        with pytest.raises(ValueError):
            amd_loop.create_optimizer(_args(task_balancer='gradnorm'), model, reducer, balancer=bal)
        # --task_balancer none: today's one group, whatever balancer is passed
        none = amd_loop.create_optimizer(_args(task_balancer='none'), build_mini_engine(), None, balancer=M.NoWeightingStrategy())
        assert len(none.param_groups) == 1 and none.group_names is None and none.n_norm is None
    finally:
        M.engine.set_direct_grads(False)


def test_norm_exempt_tensors_must_end_the_trainable_prefix():
    model = nn.Sequential(nn.Linear(6, 5), nn.Linear(5, 3))
    bal = M.UncertaintyWeightingStrategy(tasks=['a', 'b'])
    engine.ParamArena(model, extra=[('balancer.log_vars', bal.log_vars)])
    groups = [dict(params=list(model.parameters())), dict(params=[bal.log_vars], lr_scale=10.)]
    opt = FusedAdamW(model, groups=groups, norm_exempt=[bal.log_vars])
    assert opt.n_norm == opt.arena.offsets['balancer.log_vars']
    with pytest.raises(ValueError, match='last trainable'):
        FusedAdamW(model, groups=groups, norm_exempt=[model[0].weight])
    with pytest.raises(ValueError, match='last trainable'):
        FusedAdamW(model, groups=groups, norm_exempt=[model[1].bias])        # log_vars lies behind it
    with pytest.raises(ValueError, match='not a trainable tensor'):
        FusedAdamW(model, groups=groups, norm_exempt=[nn.Parameter(torch.zeros(2))])
    with pytest.raises(ValueError, match='groups'):
        FusedAdamW(model, norm_exempt=[bal.log_vars])
    from multimae_amd import ops
    z = torch.zeros(128)
    with pytest.raises(ValueError, match='n_norm'):
        ops.opt_step_groups(z, z, z, z, torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(1024),
                            group_map=torch.zeros(2, dtype=torch.int16), n_groups=1, hyper=[1e-3, 0.], beta1=0.9, beta2=0.95, eps=1e-8,
                            clip_grad=None, skip_grad=None, n_norm=96)


@pytest.fixture()
def stubbed():
    from multimae_amd import ops
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    calls = []
    fake = _lib._lib

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(fake, name)

            def rec(*args):
                if name.startswith('mmae_opt_step'):
                    d = args[0]._obj                      # (the host table lives for the call only: read it here)
                    hy = list((ctypes.c_float * (2 * d.n_groups)).from_address(d.hyper)) if getattr(d, 'hyper', None) else None
                    calls.append((name, d, args[1:], hy))
                return fn(*args)
            return rec
    _lib._lib = Recorder()
    yield calls
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


def test_step_with_a_norm_exempt_group_calls_the_tail_entry_point(stubbed):
    model = nn.Sequential(nn.Linear(6, 5), nn.Linear(5, 3))
    bal = M.UncertaintyWeightingStrategy(tasks=['a', 'b'])
    engine.ParamArena(model, extra=[('balancer.log_vars', bal.log_vars)])
    opt = FusedAdamW(model, lr=1e-3, groups=[dict(params=list(model.parameters())), dict(params=[bal.log_vars], lr_scale=10.)],
                     norm_exempt=[bal.log_vars])
    opt.param_groups[1]['lr'] = 1e-2
    opt.step()
    (name, d, rest, hy), = stubbed
    assert name == 'mmae_opt_step_groups_tail' and rest[0] == opt.n_norm == opt.arena.n_trainable - 64
    assert d.n == opt.arena.n_trainable and d.n_groups == 2
    assert hy == [float(torch.tensor(x, dtype=torch.float32)) for x in (1e-3, 0.05, 1e-2, 0.05)]
    assert opt.grad_norm.data_ptr() == opt._state.data_ptr() + 4          # the model-only norm, state[1]
    # without the exemption the same groups take the existing entry point
    stubbed.clear()
    model2 = nn.Sequential(nn.Linear(6, 5), nn.Linear(5, 3))
    FusedAdamW(model2, groups=[dict(params=list(model2.parameters()))]).step()
    assert stubbed[0][0] == 'mmae_opt_step_groups'


# ------------------------------------------------------------------------------------------ checkpoints
def test_two_group_optimizer_state_round_trips_through_torch_adamw(tmp_path):
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(6, 5), nn.LayerNorm(5), nn.Linear(5, 3))
    bal = M.UncertaintyWeightingStrategy(tasks=['a', 'b', 'c'])
    arena = engine.ParamArena(model, extra=[('balancer.log_vars', bal.log_vars)])
    names = [[n for n, _ in model.named_parameters()], ['balancer.log_vars']]
    mk = lambda step: types.SimpleNamespace(
        arena=arena, m=torch.randn(arena.n_trainable), v=torch.rand(arena.n_trainable), step_count=step, group_names=names,
        param_groups=[dict(lr=1e-3, weight_decay=0.05, lr_scale=1.0, betas=(0.9, 0.95), eps=1e-8),
                      dict(lr=1e-2, weight_decay=0.05, lr_scale=10.0, betas=(0.9, 0.95), eps=1e-8)])
    opt = mk(7)
    sd = ck.optimizer_state_to_torch(opt)
    n_model = len(names[0])
    assert [g['params'] for g in sd['param_groups']] == [list(range(n_model)), [n_model]]
    assert [g['lr_scale'] for g in sd['param_groups']] == [1.0, 10.0]
    # the layout of the reference's optimiser: torch.optim.AdamW over {'model', 'balancer'} groups loads it
    ref = torch.optim.AdamW([dict(params=list(model.parameters()), lr_scale=1.), dict(params=list(bal.parameters()), lr_scale=10.)],
                            lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    ref.load_state_dict(sd)
    o = arena.offsets['balancer.log_vars']
    assert torch.equal(ref.state[bal.log_vars]['exp_avg'], opt.m[o:o + 3]) and torch.equal(ref.state[bal.log_vars]['exp_avg_sq'], opt.v[o:o + 3])
    assert float(ref.state[bal.log_vars]['step']) == 7.0 and ref.param_groups[1]['lr'] == 1e-2
    back = mk(0)
    back.m.zero_(); back.v.zero_()
    back.param_groups[1].update(lr=0.0, lr_scale=0.0)
    ck.optimizer_state_from_torch(back, ref.state_dict())                 # a reference checkpoint with the balancer: both groups load
    assert back.step_count == 7 and back.param_groups[1]['lr'] == 1e-2 and back.param_groups[1]['lr_scale'] == 10.0
    for nm in names[0] + names[1]:
        oo, s = arena.offsets[nm], arena.sizes[nm]
        assert torch.equal(back.m[oo:oo + s], opt.m[oo:oo + s]) and torch.equal(back.v[oo:oo + s], opt.v[oo:oo + s]), nm
    # an optimiser without a balancer group keeps ignoring the reference's second group
    model1 = nn.Sequential(nn.Linear(6, 5), nn.LayerNorm(5), nn.Linear(5, 3))
    arena1 = engine.ParamArena(model1)
    single = types.SimpleNamespace(arena=arena1, m=torch.zeros(arena1.n_trainable), v=torch.zeros(arena1.n_trainable), step_count=0,
                                   param_groups=[dict(lr=0., weight_decay=0., lr_scale=1.0, betas=(0.9, 0.95), eps=1e-8)])
    ck.optimizer_state_from_torch(single, ref.state_dict())
    assert single.step_count == 7 and single.param_groups[0]['lr'] == 1e-3
    # files: 'loss_balancer' is written and restored
    with torch.no_grad():
        bal.log_vars.copy_(torch.tensor([0.5, -0.25, 0.125]))
    path = ck.save_checkpoint(str(tmp_path), 3, model, opt, loss_balancer=bal)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert list(saved['loss_balancer']) == ['log_vars'] and len(saved['optimizer']['param_groups']) == 2
    bal2 = M.UncertaintyWeightingStrategy(tasks=['a', 'b', 'c'])
    model2 = nn.Sequential(nn.Linear(6, 5), nn.LayerNorm(5), nn.Linear(5, 3))
    assert ck.load_checkpoint(path, model2, loss_balancer=bal2, resize_pos_emb=False) == 0
    assert torch.equal(bal2.log_vars.detach(), torch.tensor([0.5, -0.25, 0.125]))
    assert ck.load_checkpoint(path, model2, resize_pos_emb=False) == 0      # without a balancer: as before


# ------------------------------------------------------------------------------------------ the library
def test_library_exports_the_new_entry_points_at_abi_7():
    decl = _lib.declared_symbols()
    for name in ('mmae_task_balance_fwd', 'mmae_task_balance_bwd', 'mmae_opt_step_groups_tail'):
        assert name in decl, name
    assert _lib._PROTOS['mmae_opt_step_groups_tail'][1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert len(_lib._PROTOS['mmae_task_balance_fwd'][1]) == 7 and len(_lib._PROTOS['mmae_task_balance_bwd'][1]) == 8
    assert os.path.exists(_lib.LIB_PATH), 'libmmae_hip.so is not built (build() makes it): a missing library is a broken tree, not missing hardware'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mmae_task_balance_fwd', 'mmae_task_balance_bwd', 'mmae_opt_step_groups_tail'):
        assert hasattr(lib, name), name
    assert lib.mmae_abi_version() == 7
    assert lib.mmae_struct_size(8) == ctypes.sizeof(_lib.OptGroupsDesc) and lib.mmae_struct_size(4) == ctypes.sizeof(_lib.OptDesc)


# ------------------------------------------------------------------------------------------ the patched script
def test_patched_pretraining_script_dry_run_with_the_uncertainty_balancer():
    """The reference's run_pretraining_multimae.py with dropin/run_pretraining_multimae.patch applied, run end to end on the
    type-checking stub of the C ABI (tools/run_reference_script_dryrun.py) with --task_balancer uncertainty: two epochs of
    train_one_epoch through amd_loop.task_balancer / wrap_model / create_optimizer / LossScaler."""
    tool = os.path.join(ROOT, 'tools', 'run_reference_script_dryrun.py')
    ref = next(l.split("'")[1] for l in open(tool) if l.startswith('REF = '))
    if not os.path.exists(os.path.join(ref, 'run_pretraining_multimae.py')):
        pytest.skip('the reference checkout is not on this machine')
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT', 'SLURM_PROCID'):      # a single-process run, whatever an
        env.pop(k, None)                                                                             # earlier test left in the environment
    r = subprocess.run([sys.executable, tool, '--patched', '--task_balancer', 'uncertainty'], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert '[dryrun] the script ran to completion' in r.stdout
    assert 'rgb_loss' in r.stdout and 'grad_norm' in r.stdout
