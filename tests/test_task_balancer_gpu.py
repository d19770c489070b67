"""GPU: the uncertainty task balancer on the fused pre-training path.

  kernels     mmae_task_balance_fwd / _bwd element by element against f64 (T in {1, 3, 16}; a zero, a negative and a 1e4 loss;
              log_vars in [-3, 3]), guarded outputs, untouched inputs, exact zeros where the mask applies, bit-equal reruns
  optimiser   mmae_opt_step_groups_tail: the norm, the clip and the skip see g[0, n_norm) only, the tail takes the unclipped scale
              (helpers.adamw_ref / opt_decision_ref with the respective scale), n_norm == n is mmae_opt_step_groups bit for bit
  end to end  12 steps of the mini model with the balancer, the two param groups and the LossScaler of dropin/amd_loop.py against
              the REFERENCE's own runs (tests/golden/balancer_curve.json, make_golden_balancer.py): fp32 and bf16 mode, direct
              and autograd-returned gradients, and a StepGraph replay against the eager steps

Error bounds of the kernels (u = 2^-24, gamma_k = k u / (1 - k u), helpers.gamma; expf is accurate to 1 ulp = 2 u relative):
  weighted  e L + s            expf (2), product (1), sum (1):                         gamma_4 (e |L| + |s|)
  saved e                      expf alone:                                             gamma_2 e
  d_losses  u e                expf (2), product (1):                                  gamma_3 |u| e
  d_log_vars u (1 - e L)       e L carries expf and its product (3), the difference (1) and the product with u (1) round
                               values <= 1 + e |L|:                                    gamma_5 |u| (1 + e |L|)
              accumulating     + the rounding of the sum:                              u (|d0 + ds| + bound)
each plus helpers.TINY32 for a product that leaves the normal range.  The mask multiplies, so a masked entry is exactly (+-)0."""
import json
import math
import os
import types

import pytest
import torch

import multimae_amd as M
import multimae_oracle as orc
from multimae_amd import ops
from multimae_amd.optim import FusedAdamW
from dropin import amd_loop
from helpers import (GOLD, MINI, TINY32, Guarded, adamw_ref, assert_within, bf16_bits_ref, build_mini_engine, gamma, make_inputs,
                     opt_decision_ref, rel_err, same_bits, sumsq_ref, ulp)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------- kernels
def _case(T, which=0):
    g = torch.Generator().manual_seed(10 * T + which)
    s = torch.rand(T, generator=g) * 6 - 3
    L = torch.rand(T, generator=g) * 4 + 0.05
    special = [0.0, -2.5, 1e4]
    if T == 1:
        L[0] = special[which]
    else:
        for k, v in enumerate(special):
            L[(k * 5 + 1) % T] = v
        s[0], s[T - 1] = -3.0, 3.0
    u = torch.rand(T, generator=g) * 2 - 0.5
    d0 = torch.randn(T, generator=g)
    return s.to(DEV), L.to(DEV), u.to(DEV), d0.to(DEV)


def _vec(n, fill=None):
    return Guarded(1, n, n, torch.float32, DEV, fill=fill)


@pytest.mark.parametrize('T, which', [(1, 0), (1, 1), (1, 2), (3, 0), (16, 0)])
@pytest.mark.parametrize('packed', [False, True])
def test_balance_kernels_element_by_element(T, which, packed):
    s, L, u, d0 = _case(T, which)
    s0, L0, u0 = s.clone(), L.clone(), u.clone()
    loss_in = L if packed else [L[i] for i in range(T)]
    up_in = u if packed else [u[i] if i != T - 1 or T == 1 else None for i in range(T)]      # one gradient that never arrived
    if not packed and T > 1:
        u[T - 1] = 0.0
        u0 = u.clone()
    sd, Ld, ud = s.double(), L.double(), u.double()
    e = torch.exp(-sd)
    m = (Ld != 0).double()
    runs = []
    for rep in range(2):
        W, S, DL = _vec(T), _vec(2 * T), _vec(T)
        ops.task_balance_fwd(loss_in, s, W.view[0], S.view[0])
        ops.task_balance_bwd(up_in, S.view[0], DL.view[0], (DS := _vec(T)).view[0], False)
        ACC = _vec(T, fill=d0)
        ops.task_balance_bwd(up_in, S.view[0], (DL2 := _vec(T)).view[0], ACC.view[0], True)
        torch.cuda.synchronize()
        for G, nm in ((W, 'weighted'), (S, 'saved'), (DL, 'd_losses'), (DS, 'd_log_vars'), (ACC, 'd_log_vars (accumulate)'), (DL2, 'd_losses 2')):
            G.intact(f'T = {T}: {nm}')
        runs.append([G.view[0].clone() for G in (W, S, DL, DS, ACC)])
    w, sv, dl, ds, acc = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert same_bits(a, b)                                                   # no atomics, no order left to chance
    assert same_bits(s, s0) and same_bits(L, L0) and same_bits(u, u0)            # inputs untouched
    assert_within(w, (e * Ld + sd) * m, gamma(4) * (e * Ld.abs() + sd.abs()) * m + TINY32, f'T = {T}: weighted')
    assert_within(sv[:T], e, gamma(2) * e, f'T = {T}: saved exp(-s)')
    assert same_bits(sv[T:], L)
    assert_within(dl, ud * e * m, gamma(3) * ud.abs() * e * m + TINY32, f'T = {T}: d_losses')
    ds_ref = ud * (1 - e * Ld) * m
    b_ds = gamma(5) * ud.abs() * (1 + e * Ld.abs()) * m + TINY32
    assert_within(ds, ds_ref, b_ds, f'T = {T}: d_log_vars')
    assert_within(acc, d0.double() + ds_ref, b_ds + U32 * ((d0.double() + ds_ref).abs() + b_ds), f'T = {T}: d_log_vars accumulated')
    masked = (L == 0).nonzero().flatten().tolist()
    assert (masked != []) == (T > 1 or which == 0)
    for i in masked:                                                             # exactly zero, whatever log_vars is
        assert float(w[i]) == 0.0 and float(dl[i]) == 0.0 and float(ds[i]) == 0.0 and float(acc[i]) == float(d0[i]), i


def test_balance_kernels_nan_loss_is_not_masked_and_sizes_are_checked():
    s = torch.tensor([0.5, -0.5], device=DEV)
    L = torch.tensor([float('nan'), 2.0], device=DEV)
    w, sv, dl, ds = (torch.zeros(k, device=DEV) for k in (2, 4, 2, 2))
    ops.task_balance_fwd(L, s, w, sv)
    ops.task_balance_bwd(torch.ones(2, device=DEV), sv, dl, ds, False)
    torch.cuda.synchronize()
    assert math.isnan(float(w[0])) and math.isnan(float(ds[0])) and float(dl[0]) == float(sv[0])       # NaN != 0: "non-zero", as in torch
    assert math.isfinite(float(w[1]))
    bal = M.UncertaintyWeightingStrategy(tasks=['a', 'b']).to(DEV)
    with pytest.raises(ValueError, match='3 task losses.*2 log_vars'):
        bal({k: torch.tensor(1.0, device=DEV) for k in 'abc'})
    with pytest.raises(ValueError):
        M.UncertaintyWeightingStrategy(tasks=list(range(17)))
    lib = M._lib.load()
    z = torch.zeros(40, device=DEV)
    assert lib.mmae_task_balance_fwd(None, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 17, None) != 0
    assert lib.mmae_task_balance_bwd(None, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 0, None) != 0


@pytest.mark.parametrize('direct', [False, True])
def test_module_forward_backward_on_the_device(direct):
    """The module through autograd against the f64 formula; direct mode: d log_vars lands in the arena view -- stored on the
    first write after zero_grad(), accumulated on the second backward."""
    T = 3
    s, L, u, _ = _case(T)
    bal = M.UncertaintyWeightingStrategy(tasks=['a', 'b', 'c']).to(DEV)
    host = torch.nn.Linear(4, 4).to(DEV)
    arena = M.engine.ParamArena(host, extra=[('balancer.log_vars', bal.log_vars)])
    with torch.no_grad():
        bal.log_vars.copy_(s)
    M.engine.set_direct_grads(direct)
    try:
        arena.zero_grad()
        arena.grad.fill_(7.0) if not direct else None              # (autograd mode accumulates onto what is there)
        grads = []
        for rep in range(2):
            losses = {k: L[i].clone().requires_grad_() for i, k in enumerate('abc')}
            out = bal(losses)
            assert list(out) == ['a', 'b', 'c'] and all(v.shape == () for v in out.values())
            sum(u[i] * out[k] for i, k in enumerate('abc')).backward()
            grads.append(bal.log_vars.grad.detach().clone())
        torch.cuda.synchronize()
    finally:
        M.engine.set_direct_grads(False)
    sd, Ld, ud = s.double(), L.double(), u.double()
    e, m = torch.exp(-sd), (Ld != 0).double()
    ds_ref = ud * (1 - e * Ld) * m
    b = gamma(5) * ud.abs() * (1 + e * Ld.abs()) + TINY32           # (the node's upstream is 1 * u_i, exact)
    base = 0.0 if direct else 7.0
    assert bal.log_vars.grad.data_ptr() == arena.grad.data_ptr() + 4 * arena.offsets['balancer.log_vars']
    assert_within(grads[0], base + ds_ref, b + U32 * (base + ds_ref).abs(), 'first backward')
    assert_within(grads[1], base + 2 * ds_ref, 2 * b + 2 * U32 * (base + 2 * ds_ref).abs(), 'second backward accumulates')
    assert_within(torch.stack([losses[k].grad for k in 'abc']), ud * e * m, gamma(3) * ud.abs() * e + TINY32, 'd loss')
    assert_within(torch.stack([out[k].detach() for k in 'abc']), (e * Ld + sd) * m, gamma(4) * (e * Ld.abs() + sd.abs()) + TINY32, 'weighted')


# ---------------------------------------------------------------------------------------------- optimiser tail
B1, B2, EPS = 0.9, 0.95, 1e-8
HYPER = [1e-3, 0.05, 1e-2, 0.05]                 # group 0: the prefix; group 1: the tail (lr x 10, the same decay)


class _Arena:
    def __init__(self, n_norm, seed, tail_scale=1.0):
        n = self.n = n_norm + 64
        self.n_norm = n_norm
        g = torch.Generator().manual_seed(seed)
        p = torch.randn(n, generator=g)
        gr = torch.randn(n, generator=g) * 0.1
        p[n_norm + 3:] = 0
        gr[n_norm + 3:] = 0                      # the tail: one 64-element chunk with 3 live elements
        gr[n_norm:n_norm + 3] *= tail_scale
        m0, v0 = torch.rand(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-3
        m0[n_norm + 3:] = 0
        v0[n_norm + 3:] = 0                      # the alignment padding of an arena: parameter, gradient and moments are 0 and stay 0
        self.P, self.M, self.V = _vec(n, fill=p), _vec(n, fill=m0), _vec(n, fill=v0)
        self.S = Guarded(1, n, n, torch.bfloat16, DEV, fill=torch.zeros(n, dtype=torch.bfloat16))
        self.g = gr.to(DEV)
        self.state, self.istate = _vec(8, fill=torch.zeros(8)), Guarded(1, 8, 8, torch.int32, DEV, fill=torch.zeros(8, dtype=torch.int32))
        self.ws = torch.empty(1024, device=DEV)
        self.gmap = torch.zeros(n // 64, dtype=torch.int16, device=DEV)
        self.gmap[n_norm // 64:] = 1
        self.table = torch.tensor(HYPER, device=DEV).view(2, 2)

    p = property(lambda s: s.P.view[0])
    m = property(lambda s: s.M.view[0])
    v = property(lambda s: s.V.view[0])

    def step(self, *, by_value, clip=None, skip_at=None, prescale=1.0, n_norm='own', loss=None):
        ops.opt_step_groups(self.p, self.g, self.m, self.v, self.state.view[0], self.istate.view[0], self.ws, group_map=self.gmap, n_groups=2,
                            hyper=HYPER if by_value else None, hyper_dev=None if by_value else self.table, beta1=B1, beta2=B2, eps=EPS,
                            clip_grad=clip, skip_grad=skip_at, grad_prescale=prescale, shadow=self.S.view[0], loss_dev=loss,
                            n_norm=self.n_norm if n_norm == 'own' else n_norm)
        torch.cuda.synchronize()
        for G, nm in ((self.P, 'p'), (self.M, 'm'), (self.V, 'v'), (self.S, 'shadow'), (self.state, 'state'), (self.istate, 'istate')):
            G.intact(nm)
        return self.state.view[0].cpu().tolist(), self.istate.view[0].cpu().tolist()

    def snapshot(self):
        return self.p.clone(), self.m.clone(), self.v.clone(), self.S.view[0].clone()


@pytest.mark.parametrize('n_norm', [64, 1088])
@pytest.mark.parametrize('by_value', [True, False])
def test_tail_is_outside_the_norm_the_clip_and_the_skip(n_norm, by_value):
    """n = n_norm + 64: with n_norm = 1088 the second workgroup's 1024-element stride straddles the boundary.  Clip active, clip
    inactive and a skip_grad skip, with grad_prescale 0.5 so that the tail's scale is not 1."""
    A = _Arena(n_norm, seed=n_norm)
    ss, b_ss = sumsq_ref(A.g[:n_norm])
    norm = 0.5 * math.sqrt(ss)
    lr_el = torch.tensor([HYPER[0]] * n_norm + [HYPER[2]] * 64, dtype=torch.float64)
    wd_el = torch.tensor([HYPER[1]] * n_norm + [HYPER[3]] * 64, dtype=torch.float64)
    cases = [('clip active', dict(clip=0.5 * norm), False), ('clip inactive', dict(clip=2.0 * norm), False),
             ('skip_grad skips both parts', dict(skip_at=0.5 * norm), True), ('no clip', dict(), False)]
    for what, cfg, skips in cases:
        s_before, i_before = A.state.view[0].cpu().tolist(), A.istate.view[0].cpu().tolist()
        snap = A.snapshot()
        s, i = A.step(by_value=by_value, prescale=0.5, **cfg)
        ref = opt_decision_ref(ss, b_ss, istate=i_before, lr=HYPER[0], wd=HYPER[1], b1=B1, b2=B2, clip=cfg.get('clip'),
                               skip_at=cfg.get('skip_at'), prescale=0.5)
        assert ref['skip'] == skips and i[:6] == ref['istate'] and i[6:] == [0, 0], (what, i, ref['istate'])
        assert abs(s[0] - ss) <= b_ss, (what, s[0], ss)                          # the sum of squares of the PREFIX
        for k in (1, 2):
            want, bound = ref['state'][k]
            assert abs(s[k] - want) <= bound, (what, k, s[k], want, bound)
        assert s[3] == ref['state'][3] and s[4] == ref['state'][4], (what, s)
        for k in (5, 6):                                                         # formed in double on the device: within one f32 ulp
            assert abs(s[k] - ref['state'][k]) <= float(ulp(torch.float32, torch.tensor(ref['state'][k]))), (what, k, s[k])
        assert s[7] == 0.5, (what, s[7])                                         # the tail's scale: grad_prescale, never the clip's
        if what == 'clip active':
            assert s[2] < 0.3
        if skips:
            for cur, old in zip(A.snapshot(), snap):
                assert same_bits(cur, old), what
            continue
        gs = torch.tensor([s[2]] * n_norm + [s[7]] * 64, dtype=torch.float64)
        (pr, bp), (mr, bm), (vr, bv) = adamw_ref(snap[0], A.g, snap[1], snap[2], lr=lr_el, wd=wd_el, b1=B1, b2=B2, eps=EPS, bc1=s[5],
                                                 bc2_sqrt=s[6], gs=gs)
        assert_within(A.m, mr, bm, f"{what}: m'")
        assert_within(A.v, vr, bv, f"{what}: v'")
        assert_within(A.p, pr, bp, f"{what}: p'")
        assert same_bits(A.S.view[0].view(torch.int16), bf16_bits_ref(A.p)), what      # the shadow: RNE of the kernel's own p'
        # the tail moved by its own, larger learning rate and was not clipped: its first moment took the unclipped gradient
        live = slice(n_norm, n_norm + 3)
        assert_within(A.m[live], B1 * snap[1][live].double() + (1 - B1) * 0.5 * A.g[live].double(), 1e-6 * A.g[live].abs().double() + 1e-9, what)
        assert not A.p[n_norm + 3:].any() and not A.g[n_norm + 3:].any()


@pytest.mark.parametrize('n_norm', [64, 1088])
def test_a_huge_or_non_finite_tail_gradient_does_not_reach_the_norm(n_norm):
    small, huge, nan = _Arena(n_norm, seed=3), _Arena(n_norm, seed=3, tail_scale=1e30), _Arena(n_norm, seed=3)
    nan.g[n_norm + 1] = float('nan')
    res = [A.step(by_value=True, clip=1e-3) for A in (small, huge, nan)]
    (s0, i0), (s1, i1), (s2, i2) = res
    assert s0[0] == s1[0] == s2[0] and s0[1] == s1[1] == s2[1] and s0[2] == s1[2] == s2[2]        # state[1], the logged norm: unchanged
    assert i0 == i1 == i2 == [0, 1, 0, 0, 0, 0, 0, 0]                                              # istate[5] included: nothing counted
    for A in (huge, nan):
        assert same_bits(A.p[:n_norm], small.p[:n_norm]) and same_bits(A.m[:n_norm], small.m[:n_norm])
    assert math.isnan(float(nan.p[n_norm + 1])) and math.isfinite(float(nan.p[n_norm])) and math.isfinite(float(huge.p[n_norm]))
    # a non-finite LOSS still skips, tail included
    snap = small.snapshot()
    s, i = small.step(by_value=True, loss=torch.tensor([float('inf')], device=DEV))
    assert i[:4] == [1, 1, 1, 1] and all(same_bits(a, b) for a, b in zip(small.snapshot(), snap))


@pytest.mark.parametrize('by_value', [True, False])
def test_n_norm_equal_to_n_is_bit_identical_to_opt_step_groups(by_value):
    n_norm = 1088
    a, b = _Arena(n_norm, seed=5), _Arena(n_norm, seed=5)
    for t in range(3):
        kw = dict(by_value=by_value, clip=0.05, prescale=0.5)
        sa, ia = a.step(n_norm=a.n, **kw)
        sb, ib = b.step(n_norm=None, **kw)
        assert ia == ib and sa[:7] == sb[:7] and sa[7] == 0.5 and sb[7] == 0.0, (t, sa, sb)      # the existing entry point writes no slot 7
        for x, y in zip(a.snapshot(), b.snapshot()):
            assert same_bits(x, y), t
    assert sa[2] < 0.5                                                                             # the clip acted
    for bad in (0, 96, a.n + 64):
        with pytest.raises((ValueError, M._lib.KernelError)):
            a.step(by_value=True, n_norm=bad)


def test_norm_exempt_tensor_that_is_not_last_is_refused():
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3)).to(DEV)
    bal = M.UncertaintyWeightingStrategy(tasks=['a', 'b']).to(DEV)
    M.engine.ParamArena(model, extra=[('balancer.log_vars', bal.log_vars)])
    groups = [dict(params=list(model.parameters())), dict(params=[bal.log_vars], lr_scale=10.)]
    with pytest.raises(ValueError, match='last trainable'):
        FusedAdamW(model, groups=groups, norm_exempt=[model[1].bias])
    opt = FusedAdamW(model, groups=groups, norm_exempt=[bal.log_vars], lr=1e-2, weight_decay=0.0)
    opt.zero_grad()
    model[0].weight.grad.fill_(3.0)
    bal.log_vars.grad.copy_(torch.tensor([1e10, -1e10]))
    norm = opt.step()
    torch.cuda.synchronize()
    assert abs(float(norm) - 3.0 * math.sqrt(30)) < 1e-4 and opt.grad_norm is norm                 # the model-only norm
    assert torch.allclose(bal.log_vars.detach().cpu(), torch.tensor([-1e-2, 1e-2]), rtol=1e-5)      # stepped, unclipped: lr * sign


# ---------------------------------------------------------------------------------------------- end to end
with open(os.path.join(GOLD, 'balancer_curve.json')) as _f:
    CURVE = json.load(_f)
TASKS = CURVE['tasks']


def _args():
    return types.SimpleNamespace(opt='adamw', lr=CURVE['lr'], weight_decay=CURVE['weight_decay'], opt_eps=None, opt_betas=(0.9, 0.95),
                                 task_balancer='uncertainty', balancer_lr_scale=CURVE['balancer_lr_scale'], out_domains=list(TASKS))


def _loss_fns():
    P = MINI['P']
    return {'rgb': M.MaskedMSELoss(P, 1), 'depth': M.MaskedL1Loss(P, 1), 'semseg': M.MaskedCrossEntropyLoss(P, 4),
            'norm_rgb': M.MaskedMSELoss(P, 1, norm_pix=True)}


def _masks(step, B=4):
    n = (MINI['S'] // MINI['P']) ** 2
    torch.manual_seed(1000 + step)
    dist, tn, an = orc.draw_mask_randoms(B, [n] * 3, 1.0)
    spt = orc.samples_per_task_from_dirichlet(dist, MINI['nvis'])
    mask_all, ik, ir = orc.masks_from_noise(spt, tn, an, MINI['nvis'])
    return {d: mask_all[:, i * n:(i + 1) * n].contiguous().to(DEV) for i, d in enumerate(MINI['doms'])}, ik.to(DEV), ir.to(DEV)


def _setup():
    """The generator's recipe: seed 0 -> model, inputs; the balancer, the arena with log_vars, the two groups, the loss scaler."""
    args = _args()
    torch.manual_seed(0)
    model = build_mini_engine()
    x = make_inputs(MINI['doms'], 4, MINI['S'])
    model.to(DEV)
    bal = amd_loop.task_balancer(args).to(DEV)
    assert bal.tasks == TASKS == list(model.output_adapters)
    model.build_arena(extra={'balancer': bal})
    opt = amd_loop.create_optimizer(args, model, None, balancer=bal)
    xd = {k: v.to(DEV) for k, v in x.items()}
    return args, model, bal, opt, xd


def _run(mode, direct, clip, steps=12):
    args, model, bal, opt, xd = _setup()
    tgt = dict(xd, norm_rgb=xd['rgb'])
    fns, scaler = _loss_fns(), amd_loop.LossScaler()
    rec = dict(task=[], weighted=[], log_vars=[], norm=[])
    M.engine.set_direct_grads(direct)
    try:
        with M.engine.precision(mode):
            for step in range(1, steps + 1):
                for g in opt.param_groups:
                    g['lr'] = args.lr * g['lr_scale']                 # run_pretraining_multimae.py:474-480, a constant schedule
                tm, ik, ir = _masks(step)
                model.generate_random_masks = lambda *a, **k: (tm, ik, ir)
                preds, masks = model(xd, num_encoded_tokens=MINI['nvis'], alphas=1.0, fp32_output_adapters=['semseg'] if mode != 'fp32' else [])
                mk = dict(masks, norm_rgb=masks['rgb'])
                losses = {k: fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds}
                weighted = bal(losses)
                loss = sum(weighted.values())
                opt.zero_grad()
                norm = scaler(loss, opt, clip_grad=clip, skip_grad=None, parameters=model.parameters())
                rec['task'].append({k: float(v) for k, v in losses.items()})
                rec['weighted'].append({k: float(v) for k, v in weighted.items()})
                rec['log_vars'].append(bal.log_vars.detach().cpu().tolist())
                rec['norm'].append(float(norm))
    finally:
        M.engine.set_direct_grads(False)
    assert opt.counters(detail=True) == dict(steps=steps, nonfinite_loss=0, skipped=0, amp_overflow=0, nonfinite_grad=0)
    o = opt.arena.offsets['balancer.log_vars']
    rec['m'], rec['v'] = opt.m[o:o + 4].cpu().tolist(), opt.v[o:o + 4].cpu().tolist()
    return rec


_CACHE = {}


def _engine(mode, direct, clipped):
    """One engine run per configuration, shared by the tests that compare it."""
    key = (mode, direct, clipped)
    if key not in _CACHE:
        _CACHE[key] = _run(mode, direct, CURVE['clip_grad_run_b'] if clipped else None)
    return _CACHE[key]


def _log_var_bound(t):
    """Step t (from 1): max(8 x the reference's own f32 rounding |run A - run C|, 1e-4 of the distance the balancer's lr could have
    covered) -- the first with a margin for the engine's other summation order, the second in the spirit of the 1e-4 loss bound."""
    a, c = CURVE['run_a']['log_vars'][t - 1], CURVE['run_c_f64']['log_vars'][t - 1]
    own = max(abs(p - q) for p, q in zip(a, c))
    return max(8.0 * own, 1e-4 * CURVE['lr'] * CURVE['balancer_lr_scale'] * t)


def _write_parity(update):
    """profiles/task_balancer_parity.json: the measured deviations beside the bound (merged over the tests of one session)."""
    path = os.path.join(ROOT, 'profiles', 'task_balancer_parity.json')
    doc = {}
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {}
    doc.setdefault('recipe', CURVE['recipe'])
    doc.setdefault('bound', 'log_vars after step t: |engine - reference f32| <= max(8 |run A - run C| at t, 1e-4 sum of the balancer lr up to t)')
    doc.update(update)
    try:
        with open(path, 'w') as f:
            json.dump(doc, f, indent=1)
    except OSError:
        pass


@pytest.mark.parametrize('run', ['run_a', 'run_b'])
def test_fp32_mode_follows_the_reference_with_the_balancer(run):
    """12 steps in fp32 parity mode against the reference's run A (no clip) and run B (clip active at every step): every task's
    loss and weighted loss within 1e-4 per step, the returned (model-only) norm within 1e-4 relative, log_vars within
    _log_var_bound, the optimiser's final moments of log_vars within 1e-4 relative."""
    gold = CURVE[run]
    rec = _engine('fp32', True, run == 'run_b')
    worst = dict(task=0.0, weighted=0.0, norm=0.0)
    dev_lv, bounds = [], []
    for t in range(CURVE['steps']):
        for k in TASKS:
            worst['task'] = max(worst['task'], abs(rec['task'][t][k] - gold['task_losses'][t][k]))
            worst['weighted'] = max(worst['weighted'], abs(rec['weighted'][t][k] - gold['weighted_losses'][t][k]))
        worst['norm'] = max(worst['norm'], abs(rec['norm'][t] - gold['norm'][t]) / gold['norm'][t])
        dev_lv.append(max(abs(p - q) for p, q in zip(rec['log_vars'][t], gold['log_vars'][t])))
        bounds.append(_log_var_bound(t + 1))
    own = [max(abs(p - q) for p, q in zip(a, c)) for a, c in zip(CURVE['run_a']['log_vars'], CURVE['run_c_f64']['log_vars'])]
    print(f'{run}: worst {worst}; log_vars |engine - reference| {dev_lv}; bound {bounds}; reference |f32 - f64| {own}')
    _write_parity({f'fp32_mode_{run}': dict(log_vars_engine_minus_reference_f32=dev_lv, reference_f32_minus_f64=own, bound=bounds,
                                            worst_task_loss_dev=worst['task'], worst_weighted_loss_dev=worst['weighted'],
                                            worst_norm_rel_dev=worst['norm'])})
    assert worst['task'] < 1e-4 and worst['weighted'] < 1e-4, worst
    assert worst['norm'] < 1e-4, worst
    if run == 'run_b':
        assert all(n > CURVE['clip_grad_run_b'] for n in rec['norm'])             # the clip was active at every step here too
    for t, (d, b) in enumerate(zip(dev_lv, bounds)):
        assert d <= b, (run, t + 1, d, b, [x / y for x, y in zip(dev_lv, bounds)])
    st = gold['log_vars_state']
    assert st['step'] == CURVE['steps']
    for got, want in ((rec['m'], st['exp_avg']), (rec['v'], st['exp_avg_sq'])):
        assert all(abs(p - q) <= 1e-4 * abs(q) + 1e-9 for p, q in zip(got, want)), (got, want)
    # log_vars really moved, and was never clipped: run A and run B end at different model weights but log_vars' steps are Adam's
    assert min(abs(v) for v in rec['log_vars'][-1]) > 0.02


def test_bf16_mode_follows_the_reference_with_the_balancer():
    """bf16 speed mode, the rule and the factor of test_loss_curve_bf16_mode_cfg3_headline_geometry: per step within
    max(5e-3, 2 x the reference's OWN bf16-autocast deviation at that step or a neighbour) of the reference's fp32 run, and within 2 x
    its mean deviation on average -- for the total of the task losses and for the total of the weighted losses.

    log_vars: the issue's bound (_log_var_bound) is the reference's F32 rounding and cannot hold for bf16 products -- the
    reference's own bf16-autocast run leaves its fp32 run by up to 1.9e-4 where that bound is 1.2e-5.  In bf16 mode it is therefore
    REPLACED by the same calibrated rule as the losses: per step within 2 x the reference's own bf16 deviation of log_vars at that
    step or a neighbour (or within the fp32 bound where that is larger: step 1, where Adam's first update is lr x sign).  The
    deviation is taken TASK BY TASK: the fixture records log_vars in the order of ``tasks`` for every run, although run D's
    parameter held semseg and norm_rgb in swapped slots (the reference moves fp32_output_adapters predictions to the end of
    ``preds``, make_golden_balancer.py)."""
    a, d = CURVE['run_a'], CURVE['run_d_bf16_autocast']
    assert d['loss_order'] != a['loss_order'] and sorted(d['loss_order']) == sorted(TASKS)      # the swap the fixture undoes
    rec = _engine('bf16', True, False)
    for key, gk in (('task', 'task_losses'), ('weighted', 'weighted_losses')):
        tot = lambda rows: [sum(r.values()) for r in rows]
        ref32, ref16, eng = tot(a[gk]), tot(d[gk]), tot(rec[key])
        ref_dev = [abs(p - q) for p, q in zip(ref16, ref32)]
        dev = [abs(p - q) for p, q in zip(eng, ref32)]
        print(f'bf16 {key}: engine dev {dev}; reference own dev {ref_dev}')
        for i, x in enumerate(dev):
            r = max(ref_dev[max(i - 1, 0):i + 2])
            assert x < max(5e-3, 2.0 * r), (key, i, x, r)
        assert sum(dev) / len(dev) < 2.0 * sum(ref_dev) / len(ref_dev), (key, sum(dev) / len(dev), sum(ref_dev) / len(ref_dev))
    lv_ref_dev = [max(abs(p - q) for p, q in zip(u, v)) for u, v in zip(d['log_vars'], a['log_vars'])]
    lv_dev = [max(abs(p - q) for p, q in zip(u, v)) for u, v in zip(rec['log_vars'], a['log_vars'])]
    print(f'bf16 log_vars: engine dev {lv_dev}; reference own dev {lv_ref_dev}')
    _write_parity({'bf16_mode_run_a': dict(
        rule='bf16 mode replaces the f32 bound on log_vars: per step |engine - reference f32| <= max(f32 bound, 2 x the '
             "reference's own |bf16 autocast - f32| at that step or a neighbour), every deviation taken task by task",
        log_vars_engine_minus_reference_f32=lv_dev, reference_bf16_autocast_minus_f32=lv_ref_dev,
        allowed=[max(_log_var_bound(i + 1), 2.0 * max(lv_ref_dev[max(i - 1, 0):i + 2])) for i in range(len(lv_dev))])})
    for i, x in enumerate(lv_dev):
        assert x <= max(_log_var_bound(i + 1), 2.0 * max(lv_ref_dev[max(i - 1, 0):i + 2])), (i, x, lv_ref_dev[i])


def test_direct_and_autograd_returned_gradients_agree():
    """engine.direct_grads() off: d log_vars is handed to autograd, AccumulateGrad adds it into the same arena view.  Same curve."""
    d, r = _engine('fp32', True, False), _run('fp32', False, None, steps=4)
    for t in range(4):
        for k in TASKS:
            assert abs(d['weighted'][t][k] - r['weighted'][t][k]) < 1e-5, (t, k)
        assert max(abs(p - q) for p, q in zip(d['log_vars'][t], r['log_vars'][t])) <= _log_var_bound(t + 1), t
        assert abs(d['norm'][t] - r['norm'][t]) <= 1e-5 * d['norm'][t], t


def _graph_steps(use_graph, n=4):
    from multimae_amd.graph import StepGraph
    args, model, bal, opt, xd = _setup()
    tgt = dict(xd, norm_rgb=xd['rgb'])
    fns, scaler = _loss_fns(), amd_loop.LossScaler()
    tm, ik, ir = _masks(1)
    model.generate_random_masks = lambda *a, **k: (tm, ik, ir)
    out = {}

    def step():
        preds, masks = model(xd, num_encoded_tokens=MINI['nvis'], alphas=1.0, fp32_output_adapters=['semseg'])
        mk = dict(masks, norm_rgb=masks['rgb'])
        weighted = bal({k: fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds})
        loss = sum(weighted.values())
        opt.zero_grad()
        out['norm'] = scaler(loss, opt, clip_grad=0.5, skip_grad=None, parameters=model.parameters())
        out['loss'] = loss
        return loss

    M.engine.set_direct_grads(True); M.engine.set_adapter_streams(True); M.engine.set_wgrad_stream(True)
    losses, lvs = [], []
    try:
        with M.engine.precision('bf16'):
            run = None
            for it in range(n):
                for k, g in enumerate(opt.param_groups):
                    g['lr'] = args.lr * g['lr_scale'] * (1.0 + 0.5 * it)          # the schedule moves between replays: read from the device table
                if it == 0 or not use_graph:
                    step()                                                        # one eager step first, as bench.py does
                else:
                    run = run or StepGraph(step)
                    run()
                torch.cuda.synchronize()
                losses.append(float(out['loss'])); lvs.append(bal.log_vars.detach().cpu().tolist())
    finally:
        M.engine.set_direct_grads(False); M.engine.set_adapter_streams(False); M.engine.set_wgrad_stream(False)
    assert opt.step_count == n and (run is None or run.replays == n - 1)
    return losses, lvs, opt.arena.param[:opt.arena.n_trainable].clone()


def test_step_graph_replay_with_the_balancer_matches_eager_steps():
    """One eager step, then three replays of the captured step (balancer forward / backward, the tail entry point with the groups'
    device table) against four eager steps, under the equality tests/test_model_gpu.py holds for a captured step: loss curve within
    2e-3 relative, parameters (log_vars among them) within 2e-3 in relative norm; log_vars itself within 2e-3 of its travel."""
    le, ve, pe = _graph_steps(False)
    lg, vg, pg = _graph_steps(True)
    assert max(abs(a - b) / abs(a) for a, b in zip(le, lg)) < 2e-3, (le, lg)
    assert rel_err(pg, pe) < 2e-3
    travel = max(abs(v) for v in ve[-1])
    assert travel > 0.03 and max(abs(p - q) for p, q in zip(ve[-1], vg[-1])) < 2e-3 * travel, (ve[-1], vg[-1])
