"""CPU: the fine-tuning optimiser's param groups (dropin.amd_loop.create_optimizer_groups) against the reference factory's own
groups (tests/golden/param_groups.json, generator committed), the grouped state-dict interchange with torch.optim.AdamW, and
FusedAdamW(groups=...)'s host logic against a type-checking stub of the C ABI (mmae_opt_step_groups)."""
import ctypes
import functools
import json
import os
import types

import pytest
import torch
from torch import nn

import multimae_amd as M
from multimae_amd import checkpoint as ck
from multimae_amd import engine
from multimae_amd.optim import FusedAdamW
from dropin import amd_loop

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'param_groups.json')
with open(GOLD) as _f:
    CASES = json.load(_f)


class Synth(nn.Module):
    """The synthetic module of make_golden_param_groups.py (same names and shapes)."""

    def __init__(self):
        super().__init__()
        self.global_tokens = nn.Parameter(torch.zeros(1, 1, 8))
        self.encoder = nn.Sequential(*[nn.Sequential(nn.LayerNorm(8), nn.Linear(8, 8)) for _ in range(3)])
        self.decoder = nn.ModuleDict(dict(proj=nn.Linear(8, 8), norm=nn.LayerNorm(8), head=nn.Linear(8, 4)))
        self.extra = nn.Linear(8, 8)
        self.frozen = nn.Parameter(torch.zeros(8, 8), requires_grad=False)

    def get_num_layers(self):
        return 3

    def no_weight_decay(self):
        return {'global_tokens'}

    def decoder_weight_decay(self):
        return {'extra.weight'}


@functools.lru_cache(maxsize=1)
def _model(name, doms):
    if name == 'synthetic':
        return Synth()
    ins = {d: M.PatchedInputAdapter(num_channels=3 if d == 'rgb' else 1, stride_level=1, patch_size_full=16, image_size=224)
           for d in doms}
    outs = {'cls': M.LinearOutputAdapter(num_classes=1000, use_mean_pooling=True, init_scale=1.0)}
    return getattr(M, name)(input_adapters=ins, output_adapters=outs, num_global_tokens=1)


def _layer_id(name, n):
    """Layer ids of a ViT for layer-wise lr decay: tokens and input adapters 0, encoder block i -> i + 1, everything else n - 1."""
    if name in ('cls_token', 'mask_token', 'pos_embed', 'global_tokens') or name.startswith(('patch_embed', 'input_adapters')):
        return 0
    if name.startswith(('blocks', 'encoder')):
        return int(name.split('.')[1]) + 1
    return n - 1


def _args(case):
    c = CASES[case]
    args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=c['weight_decay'], opt_eps=1e-8, opt_betas=None)
    if c['decoder_decay'] is not None:
        args.decoder_decay = c['decoder_decay']
    if c['no_lr_scale_list'] is not None:
        args.no_lr_scale_list = c['no_lr_scale_list']
    return args


def _assigner(case, model):
    ld, L = CASES[case]['layer_decay'], model.get_num_layers()
    if ld >= 1.0:
        return None, None
    values = list(ld ** (L + 1 - i) for i in range(L + 2))
    return (lambda name: _layer_id(name, len(values))), (lambda lid: values[lid])


def _expected(case):
    """The reference's groups.  Its weight_decay == 0 fallback hands every tensor to torch.optim.AdamW, frozen ones included (they
    get no gradient, so no update); FusedAdamW takes the trainable ones.  A group without lr_scale is scale 1 to the loop."""
    c = CASES[case]
    frozen = set(c['frozen'])
    return [(([n for n in g['names'] if n not in frozen]), g['weight_decay'], 1.0 if g['lr_scale'] is None else g['lr_scale'])
            for g in c['groups']]


@pytest.mark.parametrize('case', sorted(CASES))
def test_groups_match_the_reference_factory(case):
    c = CASES[case]
    model = _model(c['model'], tuple(c['domains']))
    get_num_layer, get_layer_scale = _assigner(case, model)
    groups = amd_loop.finetune_param_groups(_args(case), model, skip_list=model.no_weight_decay(), get_num_layer=get_num_layer,
                                            get_layer_scale=get_layer_scale)
    name_of = {id(p): n for n, p in model.named_parameters()}
    got = [([name_of[id(p)] for p in g['params']], g['weight_decay'], g['lr_scale']) for g in groups]
    assert got == _expected(case)
    if case == 'base_ld065':
        assert len(groups) == 28 and sum(p.numel() for g in groups for p in g['params']) == 86_416_360
    if case == 'large_ld075':
        assert len(groups) == 52


def test_create_optimizer_groups_builds_the_fused_optimiser():
    """End to end on the synthetic case: the fused optimiser holds the reference's groups, the chunk map follows the arena."""
    model = Synth()
    get_num_layer, get_layer_scale = _assigner('synthetic_decoder_decay', model)
    opt = amd_loop.create_optimizer_groups(_args('synthetic_decoder_decay'), model, skip_list=model.no_weight_decay(),
                                           get_num_layer=get_num_layer, get_layer_scale=get_layer_scale)
    assert isinstance(opt, FusedAdamW)
    exp = _expected('synthetic_decoder_decay')
    assert opt.group_names == [e[0] for e in exp]
    assert [(g['weight_decay'], g['lr_scale'], g['lr']) for g in opt.param_groups] == [(e[1], e[2], 1e-3) for e in exp]
    a, gm = opt.arena, opt._group_map
    assert gm.dtype == torch.int16 and gm.numel() == a.n_trainable // engine.ALIGN
    for k, names in enumerate(opt.group_names):
        for n in names:
            o, s = a.offsets[n], a.sizes[n]
            assert (gm[o // 64:(o + s + 63) // 64] == k).all(), n
    with pytest.raises(ValueError):                      # the fused step is AdamW only
        amd_loop.create_optimizer_groups(types.SimpleNamespace(opt='sgd', lr=1e-3, weight_decay=0.05), Synth())


# ------------------------------------------------------------------------------------------ checkpoints
def _toy():
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(6, 5), nn.LayerNorm(5), nn.Linear(5, 3), nn.Linear(3, 70))
    model[1].bias.requires_grad_(False)                  # frozen: in no group
    return model


def _toy_groups(model):
    """Three groups whose order is not named_parameters() order."""
    return [dict(params=[model[3].weight, model[0].weight], weight_decay=0.05, lr_scale=0.25),
            dict(params=[model[2].bias, model[1].weight, model[0].bias, model[3].bias], weight_decay=0.0, lr_scale=0.5),
            dict(params=[model[2].weight], weight_decay=0.05, lr_scale=1.0, lr=3e-4)]


def _fake_grouped(model, step=3):
    """A grouped FusedAdamW-shaped object on CPU tensors (tests/test_checkpoint_cpu.py's stand-in, with groups)."""
    arena = engine.arena_of(model) or engine.ParamArena(model)
    name_of = {id(p): n for n, p in model.named_parameters()}
    groups = _toy_groups(model)
    pg = [dict(lr=g.get('lr', 1e-3) * 2 ** k, weight_decay=g['weight_decay'], lr_scale=g['lr_scale'], betas=(0.9, 0.999), eps=1e-8)
          for k, g in enumerate(groups)]
    return types.SimpleNamespace(arena=arena, m=torch.randn(arena.n_trainable), v=torch.rand(arena.n_trainable), step_count=step,
                                 param_groups=pg, group_names=[[name_of[id(p)] for p in g['params']] for g in groups])


def test_grouped_state_interchanges_with_torch_adamw():
    model = _toy()
    opt = _fake_grouped(model)
    sd = ck.optimizer_state_to_torch(opt)
    assert [g['params'] for g in sd['param_groups']] == [[0, 1], [2, 3, 4, 5], [6]]
    assert [g['lr_scale'] for g in sd['param_groups']] == [0.25, 0.5, 1.0]
    ref = torch.optim.AdamW(_toy_groups(model), lr=1e-3, betas=(0.9, 0.999))
    ref.load_state_dict(sd)                              # torch validates the group sizes / shapes here
    a = opt.arena
    for g, names in zip(ref.param_groups, opt.group_names):
        for p, n in zip(g['params'], names):
            o, s = a.offsets[n], a.sizes[n]
            assert torch.equal(ref.state[p]['exp_avg'].reshape(-1), opt.m[o:o + s]), n
            assert torch.equal(ref.state[p]['exp_avg_sq'].reshape(-1), opt.v[o:o + s]), n
    assert [g['lr'] for g in ref.param_groups] == [g['lr'] for g in opt.param_groups]
    back = _fake_grouped(model, step=0)
    back.m.zero_(); back.v.zero_()
    for g in back.param_groups:
        g['lr'], g['lr_scale'] = 0.0, 0.0
    ck.optimizer_state_from_torch(back, ref.state_dict())
    assert back.step_count == 3
    for names in opt.group_names:
        for n in names:
            o, s = a.offsets[n], a.sizes[n]
            assert torch.equal(back.m[o:o + s], opt.m[o:o + s]) and torch.equal(back.v[o:o + s], opt.v[o:o + s]), n
    assert [(g['lr'], g['lr_scale'], g['weight_decay']) for g in back.param_groups] == \
        [(g['lr'], g['lr_scale'], g['weight_decay']) for g in opt.param_groups]
    # another layout is refused: two groups, or the same number of groups with other sizes
    other = ref.state_dict()
    with pytest.raises(ValueError):
        ck.optimizer_state_from_torch(back, dict(other, param_groups=other['param_groups'][:2]))
    moved = [dict(g) for g in other['param_groups']]
    moved[0]['params'], moved[1]['params'] = [0], [1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        ck.optimizer_state_from_torch(back, dict(other, param_groups=moved))


def test_single_group_export_is_unchanged():
    """The one-group export keeps its exact layout (keys, order, values), as the pre-training checkpoints have it."""
    model = _toy()
    arena = engine.ParamArena(model)
    opt = types.SimpleNamespace(arena=arena, m=torch.randn(arena.n_trainable), v=torch.rand(arena.n_trainable), step_count=5,
                                param_groups=[dict(lr=1e-3, weight_decay=0.05, lr_scale=1.0, betas=(0.9, 0.95), eps=1e-8)])
    sd = ck.optimizer_state_to_torch(opt)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    exp_state = {}
    for i, n in enumerate(names):
        o, s, shape = arena.offsets[n], arena.sizes[n], arena._params[n].shape
        exp_state[i] = {'step': torch.tensor(5.0), 'exp_avg': opt.m[o:o + s].view(shape).clone(),
                        'exp_avg_sq': opt.v[o:o + s].view(shape).clone()}
    exp = {'state': exp_state, 'param_groups': [{'lr': 1e-3, 'betas': (0.9, 0.95), 'eps': 1e-8, 'weight_decay': 0.05, 'amsgrad': False,
                                                 'lr_scale': 1.0, 'params': list(range(len(names)))}]}
    assert list(sd) == list(exp) and list(sd['param_groups'][0]) == list(exp['param_groups'][0])
    assert sd['param_groups'] == exp['param_groups']
    for i in exp_state:
        assert list(sd['state'][i]) == ['step', 'exp_avg', 'exp_avg_sq']
        assert all(torch.equal(sd['state'][i][k], exp_state[i][k]) for k in exp_state[i])
    # the extra (balancer) group of a reference pre-training checkpoint is still ignored on load
    sd2 = dict(sd, param_groups=sd['param_groups'] + [dict(sd['param_groups'][0], params=[], lr_scale=0.5)])
    back = types.SimpleNamespace(arena=arena, m=torch.zeros(arena.n_trainable), v=torch.zeros(arena.n_trainable), step_count=0,
                                 param_groups=[dict(opt.param_groups[0])])
    ck.optimizer_state_from_torch(back, sd2)
    assert back.step_count == 5 and all(torch.equal(back.m[o:o + s], opt.m[o:o + s]) for _, o, s, _ in ck._trainable(back))


# ------------------------------------------------------------------------------------------ host logic (stubbed C ABI)
@pytest.fixture()
def stubbed(monkeypatch):
    from multimae_amd import _lib, ops
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
                    d = args[0]._obj
                    hy = None
                    if name == 'mmae_opt_step_groups' and d.hyper:
                        hy = list((ctypes.c_float * (2 * d.n_groups)).from_address(d.hyper))
                    calls.append((name, d, hy))
                return fn(*args)
            return rec
    _lib._lib = Recorder()
    yield calls
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


def test_grouped_step_calls_the_grouped_entry_point(stubbed):
    model = _toy()
    opt = FusedAdamW(model, lr=1e-3, betas=(0.9, 0.999), clip_grad=1.0, groups=_toy_groups(model))
    for k, g in enumerate(opt.param_groups):
        g['lr'] = 1e-3 * g['lr_scale'] * (k + 1)
    opt.param_groups[1]['weight_decay'] = 0.0
    opt.step()
    (name, d, hy), = stubbed
    assert name == 'mmae_opt_step_groups'
    assert d.n_groups == 3 and d.group_map == opt._group_map.data_ptr() and not d.hyper_dev
    assert d.n == opt.arena.n_trainable and d.p == opt.arena.param.data_ptr() and d.g == opt.arena.grad.data_ptr()
    assert d.clip_grad == 1.0 and abs(d.beta2 - 0.999) < 1e-7 and d.grad_prescale == 1.0
    exp = [x for g in opt.param_groups for x in (g['lr'], g['weight_decay'])]
    assert hy == [float(torch.tensor(x, dtype=torch.float32)) for x in exp]
    # the state dict carries the layout; another layout is refused
    sd = opt.state_dict()
    assert sd['group_names'] == opt.group_names
    opt.load_state_dict(sd)
    single = FusedAdamW(_toy())
    with pytest.raises(ValueError):
        single.load_state_dict(sd)
    with pytest.raises(ValueError):
        opt.load_state_dict(single.state_dict())
    with pytest.raises(RuntimeError):
        opt.add_param_group(dict(params=[nn.Parameter(torch.zeros(3))]))


def test_grouped_step_under_capture_reads_a_device_table(stubbed):
    model = _toy()
    opt = FusedAdamW(model, groups=_toy_groups(model))
    cap = engine.HostInputs()
    engine._capture = cap
    try:
        opt.step()
    finally:
        engine._capture = None
    (name, d, hy), = stubbed
    assert name == 'mmae_opt_step_groups' and not d.hyper and d.hyper_dev
    table, thunk, _ = cap.items[0]
    assert d.hyper_dev == table.data_ptr() and table.shape == (3, 2)
    opt.param_groups[2]['lr'] = 0.125
    assert thunk()[2, 0] == 0.125                        # refreshed from the groups as they stand before each replay


def test_single_group_still_calls_opt_step(stubbed):
    opt = FusedAdamW(_toy(), lr=2e-3, weight_decay=0.05)
    opt.step()
    (name, d, _), = stubbed
    assert name == 'mmae_opt_step' and abs(d.lr - 2e-3) < 1e-9 and abs(d.weight_decay - 0.05) < 1e-9
    assert 'group_names' not in opt.state_dict() and opt.group_names is None
    opt.add_param_group(dict(params=[nn.Parameter(torch.zeros(3))]))      # unchanged: torch's own behaviour


def test_groups_are_validated():
    model = _toy()
    other = nn.Linear(2, 2)
    g = _toy_groups(model)
    with pytest.raises(ValueError, match='not a parameter'):
        FusedAdamW(model, groups=g[:2] + [dict(params=[model[2].weight, other.weight])])
    with pytest.raises(ValueError, match='frozen'):
        FusedAdamW(model, groups=g + [dict(params=[model[1].bias])])
    with pytest.raises(ValueError, match='more than one group'):
        FusedAdamW(model, groups=g + [dict(params=[model[0].weight])])
    with pytest.raises(ValueError, match='in no group'):
        FusedAdamW(model, groups=g[:2])
    with pytest.raises(ValueError, match='betas and eps'):
        FusedAdamW(model, groups=g[:2] + [dict(g[2], betas=(0.8, 0.95))])
    with pytest.raises(ValueError, match='betas and eps'):
        FusedAdamW(model, groups=g[:2] + [dict(g[2], eps=1e-6)])
    with pytest.raises(ValueError, match='at most'):
        big = nn.ParameterList([nn.Parameter(torch.zeros(1)) for _ in range(257)])
        FusedAdamW(big, groups=[dict(params=[p]) for p in big])
    with pytest.raises(ValueError):
        FusedAdamW(model, groups=[])
    many = nn.ParameterList([nn.Parameter(torch.zeros(1)) for _ in range(256)])
    opt = FusedAdamW(many, groups=[dict(params=[p]) for p in many])
    assert len(opt.param_groups) == 256 and opt._group_map.tolist() == list(range(256))
