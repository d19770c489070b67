"""The kernels every parameter and every input pixel passes through, element by element: the optimiser (losses.hip: mmae_sumsq,
mmae_adamw, mmae_adamw_dev, mmae_opt_step, mmae_opt_step_groups), the streaming casts, splits and sums (rowops.hip,
gemm_f32x3.hip: mmae_cast_*, mmae_transpose_cast, mmae_axpy_f32, mmae_add_n_f32, mmae_x3_split, mmae_x3_prepare_weights) and the
truncated depth standardisation (depth.hip: mmae_depth_standardize, mmae_ingest_depth).

The optimiser and the depth kernel are compared with fp64 references under bounds derived from the kernels' rounding points
(helpers.adamw_ref, sumsq_ref, opt_decision_ref, depth_std_ref); casts, transposes, axpy, add_n and the bf16 split bit for bit with
restatements in torch on the CPU.  Sizes cover one element, the vector / scalar-tail switch, the 64-element chunk borders and the
second trip of every grid-stride loop.  Everything a kernel writes lives in a Guarded buffer; nothing is left out of a comparison."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import (Guarded, adamw_ref, add_n_ref, assert_within, bf16_bits_ref, bf16_to_f32_ref, bias_corrections,
                     depth_std_ref, f16_to_f32_ref, f32_to_f16_ref, f32r, fma_f32_ref, opt_decision_ref, sumsq_ref, ulp, x3_split_ref)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16, F16, U16, I32 = 0, 1, 5, 6, 7
EINVAL = -1
B1, B2, EPS = 0.9, 0.95, 1e-8
# adamw_kernel's grid is capped at 8192 workgroups x 1024 elements, sumsq_stage1's at 1024 x 1024, the stream_grid kernels' at
# 4096 x 256 x 4, x3_split's at 16384 x 256 units of 8: one size past the cap of each, with a ragged tail
N_ADAMW_2 = 2 * 8388608 + 1027               # third trip of adamw's loop, second and beyond of sumsq's
N_SUMSQ_2, N_SUMSQ_3 = 1048577, 2 * 1048576 + 1027
N_STREAM_2 = 4194304 + 1027
SIZES = [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1027, 262147]


def _lib():
    from multimae_amd import _lib as L
    return L.load()


def _L():
    from multimae_amd import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ps):
    return ctypes.cast((ctypes.c_void_p * len(ps))(*ps), ctypes.c_void_p)


def _i32s(vals):
    return ctypes.cast((ctypes.c_int32 * len(vals))(*vals), ctypes.c_void_p)


_INT = {4: torch.int32, 2: torch.int16}


def _bits_equal(out, ref, what):
    """bit-for-bit equality of two f32 / 16-bit tensors of one shape (NaN payloads and the sign of zero included)"""
    it = _INT[out.element_size()]
    o = out.detach().contiguous().view(it)
    r = ref.detach().to(o.device).contiguous()
    r = r.view(it) if r.dtype != it else r
    assert o.shape == r.shape, (what, o.shape, r.shape)
    bad = o != r
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{what}: {n} of {o.numel()} elements differ in their bits; first at flat {i}: '
                             f'{int(o.reshape(-1)[i]) & (2 ** (8 * out.element_size()) - 1):#x} vs '
                             f'{int(r.reshape(-1)[i]) & (2 ** (8 * out.element_size()) - 1):#x}')


def _equal_nan_as_nan(out, ref, what):
    """bit-for-bit wherever the reference is a number; where it is a NaN the output must be a NaN (mmae.h: 'a NaN stays a NaN';
    the payload of an fp16 NaN is the conversion instruction's)"""
    o, r = out.detach().cpu(), ref.detach().cpu()
    nan = torch.isnan(r)
    assert bool((torch.isnan(o) == nan).all()), f'{what}: NaNs appear or vanish'
    assert o.dtype == r.dtype, (what, o.dtype, r.dtype)
    z = torch.zeros((), dtype=o.dtype)
    _bits_equal(torch.where(nan, z, o), torch.where(nan, z, r), what)


def _untouched(G, what):
    """nothing written: the view of a Guarded still holds the sentinel, as its guard zones do"""
    G.intact(what)
    assert bool((G.view.contiguous().view(_INT[G.esz]) == {4: -5898331, 2: -91}[G.esz]).all()), f'{what}: the output was written'


def _vec(n, dtype=torch.float32, fill=None):
    return Guarded(1, n, n, dtype, DEV, fill=fill)


# =================================================================================================================================
# Optimiser
# =================================================================================================================================
def _operands(n, mix, seed):
    g_ = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda: torch.randn(n, device=DEV, generator=g_)
    p, g, m, v = r(), r(), r() * 0.1, torch.rand(n, device=DEV, generator=g_) * 0.01
    if mix == 'cancel':                                  # m' = b1 m + (1 - b1) g cancels to ~1e-6 of its terms
        m = -(1 - f32r(B1)) / f32r(B1) * g * (1 + 1e-6 * r())
    elif mix == 'zero':                                  # g = 0, v = 0: the denominator is eps
        g, v = torch.zeros_like(g), torch.zeros_like(v)
    elif mix == 'tiny':                                  # |g| ~ 1e-20: gj^2 leaves the normal range
        g, m, v = g * 1e-20, m * 1e-20, v * 1e-40
    elif mix == 'huge':                                  # |g| ~ 1e15
        g = g * 1e15
    return p, g, m, v


class Arena:
    """p, m, v and the shadow in Guarded buffers, the gradient beside them with a copy of its bits"""

    def __init__(self, n, mix='random', shadow=None, seed=1):
        p, g, m, v = _operands(n, mix, seed)
        self.n = n
        self.P, self.M, self.V = _vec(n, fill=p), _vec(n, fill=m), _vec(n, fill=v)
        self.g = g.contiguous()
        self.g0 = self.g.clone()
        self.shadow_dtype = shadow
        self.S = _vec(n, shadow) if shadow is not None else None

    p = property(lambda s: s.P.view[0])
    m = property(lambda s: s.M.view[0])
    v = property(lambda s: s.V.view[0])

    def ptrs(self):
        return self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr()

    def sh(self):
        if self.S is None:
            return None, F32
        return self.S.view.data_ptr(), {torch.float32: F32, torch.bfloat16: BF16}[self.shadow_dtype]

    def snapshot(self):
        return self.p.clone(), self.m.clone(), self.v.clone(), (self.S.view[0].clone() if self.S is not None else None)

    def check_frame(self, what):
        for G, nm in ((self.P, 'p'), (self.M, 'm'), (self.V, 'v'), (self.S, 'shadow')):
            if G is not None:
                G.intact(f'{what}: {nm}')
        _bits_equal(self.g, self.g0, f'{what}: the gradient')

    def check_unchanged(self, snap, what):
        for cur, old, nm in ((self.p, snap[0], 'p'), (self.m, snap[1], 'm'), (self.v, snap[2], 'v')):
            _bits_equal(cur, old, f'{what}: {nm} of a skipped step')
        if self.S is not None:
            _bits_equal(self.S.view[0], snap[3], f'{what}: shadow of a skipped step')
        self.check_frame(what)

    def check_step(self, snap, what, *, lr, wd, bc1, bc2_sqrt, gs=1.0, g=None):
        """every element of p, m, v against adamw_ref on the values before the step; the shadow from the kernel's own p'"""
        (pr, bp), (mr, bm), (vr, bv) = adamw_ref(snap[0], self.g if g is None else g, snap[1], snap[2], lr=lr, wd=wd, b1=B1, b2=B2,
                                                 eps=EPS, bc1=bc1, bc2_sqrt=bc2_sqrt, gs=gs)
        assert_within(self.m, mr, bm, f"{what}: m'")
        assert_within(self.v, vr, bv, f"{what}: v'")
        assert_within(self.p, pr, bp, f"{what}: p'")
        if self.S is not None and self.shadow_dtype == torch.float32:
            _bits_equal(self.S.view[0], self.p, f'{what}: f32 shadow')
        elif self.S is not None:                         # round to nearest even of the kernel's OWN p', NaN quieted
            _bits_equal(self.S.view[0], bf16_bits_ref(self.p), f'{what}: bf16 shadow')
        self.check_frame(what)


class OptState:
    def __init__(self):
        self.state = _vec(8, fill=torch.zeros(8))
        self.istate = _vec(8, torch.int32, fill=torch.zeros(8, dtype=torch.int32))
        self.ws = _vec(1024)

    def read(self):
        return self.state.view[0].cpu().tolist(), self.istate.view[0].cpu().tolist()

    def intact(self, what):
        self.state.intact(f'{what}: state')
        self.istate.intact(f'{what}: istate')
        self.ws.intact(f'{what}: ws')


def _group_setup(n, n_groups, lr, wd):
    """a map whose borders fall on consecutive 64-element chunks (the chunk of the scalar tail included), one entry beyond
    n_groups (read as n_groups - 1, mmae.h), a distinct (lr, wd) per group; returns the map, the host table, lr / wd per element"""
    nc = (n + 63) // 64
    gm = torch.arange(nc) % n_groups
    if nc > 2:
        gm[nc // 2] = 65535 if n_groups < 65536 else 0
    eff = gm.clamp_max(n_groups - 1)
    k = torch.arange(n_groups, dtype=torch.float64)
    lrs = (lr * (1 + k / 4)).to(torch.float32)
    wds = (wd * (k + 1) / 2).to(torch.float32)
    hyper = torch.stack([lrs, wds], 1).reshape(-1)
    idx = eff.repeat_interleave(64)[:n]
    gmap = torch.where(gm >= 32768, gm - 65536, gm).to(torch.int16).to(DEV)
    return gmap, hyper, lrs[idx].to(DEV), wds[idx].to(DEV)


ENTRIES = ['mmae_adamw', 'mmae_adamw_dev', 'mmae_opt_step', 'mmae_opt_step_groups:hyper', 'mmae_opt_step_groups:hyper_dev']


def _opt_desc(A, st, **kw):
    d = _L().OptDesc()
    d.p, d.g, d.m, d.v = A.ptrs()
    d.n = A.n
    d.shadow, d.shadow_dtype = A.sh()
    d.beta1, d.beta2, d.eps, d.grad_prescale = B1, B2, EPS, 1.0
    d.state, d.istate, d.ws = st.state.view.data_ptr(), st.istate.view.data_ptr(), st.ws.view.data_ptr()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _groups_desc(A, st, gmap, n_groups, hyper=None, hyper_dev=None, **kw):
    d = _L().OptGroupsDesc()
    d.p, d.g, d.m, d.v = A.ptrs()
    d.n = A.n
    d.shadow, d.shadow_dtype = A.sh()
    d.beta1, d.beta2, d.eps, d.grad_prescale = B1, B2, EPS, 1.0
    d.state, d.istate, d.ws = st.state.view.data_ptr(), st.istate.view.data_ptr(), st.ws.view.data_ptr()
    d.group_map, d.n_groups = gmap.data_ptr(), n_groups
    keep = None
    if hyper_dev is not None:
        d.hyper_dev = hyper_dev.data_ptr()
    else:
        keep = (ctypes.c_float * len(hyper))(*hyper)
        d.hyper = ctypes.addressof(keep)
    for k, v in kw.items():
        setattr(d, k, v)
    return d, keep


def _run_steps(entry, A, lr, wd, what, steps=3):
    """`steps` consecutive updates through one entry point; before each the arrays are copied, so every step is checked as ONE step
    from the kernel's own previous outputs"""
    lib = _lib()
    st = OptState()
    gmap = None
    if entry.startswith('mmae_opt_step_groups'):
        gmap, hyper, lr_el, wd_el = _group_setup(A.n, 3, lr, wd)
        hyper_dev = hyper.to(DEV)
    for t in range(1, steps + 1):
        snap = A.snapshot()
        bc1, bc2 = bias_corrections(B1, B2, t)
        w = f'{what}, step {t}'
        if entry == 'mmae_adamw':
            sp, sd = A.sh()
            rc = lib.mmae_adamw(*A.ptrs(), A.n, lr, B1, B2, EPS, wd, t, None, None, sp, sd, _st())
            eff = dict(lr=lr, wd=wd, bc1=bc1, bc2_sqrt=bc2)
        elif entry == 'mmae_adamw_dev':
            hy = torch.tensor([lr, wd, bc1, bc2], dtype=torch.float32, device=DEV)
            sp, sd = A.sh()
            rc = lib.mmae_adamw_dev(*A.ptrs(), A.n, hy.data_ptr(), B1, B2, EPS, None, None, sp, sd, _st())
            eff = dict(lr=lr, wd=wd, bc1=bc1, bc2_sqrt=bc2)
        else:
            if entry == 'mmae_opt_step':
                d = _opt_desc(A, st, lr=lr, weight_decay=wd)
                rc = lib.mmae_opt_step(ctypes.byref(d), _st())
                eff = dict(lr=lr, wd=wd)
            else:
                by_value = entry.endswith(':hyper')
                d, keep = _groups_desc(A, st, gmap, 3, hyper=hyper.tolist() if by_value else None, hyper_dev=None if by_value else hyper_dev)
                rc = lib.mmae_opt_step_groups(ctypes.byref(d), _st())
                eff = dict(lr=lr_el, wd=wd_el)
            s, i = st.read()
            assert i[:6] == [0, t, 0, 0, 0, 0], (w, i)
            _check_bc(s, t, w)
            assert s[2] == 1.0, (w, s)
            eff.update(bc1=s[5], bc2_sqrt=s[6], gs=s[2])
            st.intact(w)
        assert rc == 0, (w, rc, lib.mmae_last_error())
        A.check_step(snap, w, **eff)
        A.g.copy_(torch.roll(A.g0, 17 * t))            # another gradient for the next step
        A.g0 = A.g.clone()


def _check_bc(s, t, what):
    """state[5..6] against (float)(1 - b1^t), (float)sqrt(1 - b2^t): opt_finalize_kernel forms them in double with the device's pow
    and sqrt (a few fp64 ulps), so after the rounding to f32 they equal the host's values or, when the double falls within those few
    ulps of an f32 rounding border, sit one f32 ulp away"""
    bc1, bc2 = bias_corrections(B1, B2, max(t, 1))
    for got, want, nm in ((s[5], bc1, '1 - b1^t'), (s[6], bc2, 'sqrt(1 - b2^t)')):
        assert abs(got - want) <= float(ulp(torch.float32, torch.tensor(want))), (what, nm, got, want)


@pytest.mark.parametrize('entry', ENTRIES)
def test_adamw_every_element_at_the_tail_and_chunk_sizes(entry):
    for k, n in enumerate(SIZES):
        shadow = [None, torch.float32, torch.bfloat16][k % 3]
        _run_steps(entry, Arena(n, 'random', shadow, seed=n), 1e-3, 0.05, f'{entry}, n = {n}, shadow {shadow}')


@pytest.mark.parametrize('entry', ENTRIES)
def test_adamw_every_element_past_the_second_grid_stride_trip(entry):
    _run_steps(entry, Arena(N_ADAMW_2, 'random', torch.bfloat16, seed=3), 1e-3, 0.05, f'{entry}, n = {N_ADAMW_2}')


@pytest.mark.parametrize('mix', ['random', 'cancel', 'zero', 'tiny', 'huge', 'wd = 0', 'lr = 0'])
@pytest.mark.parametrize('entry', ENTRIES)
def test_adamw_operand_mixes(entry, mix):
    lr, wd = (0.0 if mix == 'lr = 0' else 1e-3), (0.0 if mix == 'wd = 0' else 0.05)
    for n, shadow in ((1027, torch.bfloat16), (262147, torch.float32)):
        A = Arena(n, mix if '=' not in mix else 'random', shadow, seed=5)
        p0 = A.p.clone()
        _run_steps(entry, A, lr, wd, f'{entry}, {mix}, n = {n}')
        if mix == 'lr = 0':                              # decay = 1 - 0 wd = 1 and the step is 0: p keeps its bits
            _bits_equal(A.p, p0, f'{entry}: p after three steps with lr = 0')


@pytest.mark.parametrize('entry', ['mmae_adamw', 'mmae_adamw_dev'])
def test_adamw_grad_scale_dev_and_skip_flag(entry):
    lib = _lib()
    lr, wd, t = 1e-3, 0.05, 2
    bc1, bc2 = bias_corrections(B1, B2, t)
    hy = torch.tensor([lr, wd, bc1, bc2], dtype=torch.float32, device=DEV)

    def call(A, gs, skip):
        sp, sd = A.sh()
        if entry == 'mmae_adamw':
            return lib.mmae_adamw(*A.ptrs(), A.n, lr, B1, B2, EPS, wd, t, gs.data_ptr(), skip.data_ptr() if skip is not None else None, sp, sd, _st())
        return lib.mmae_adamw_dev(*A.ptrs(), A.n, hy.data_ptr(), B1, B2, EPS, gs.data_ptr(), skip.data_ptr() if skip is not None else None, sp, sd, _st())

    for n in (5, 1027, 262147):
        for shadow in (torch.bfloat16, torch.float32):
            for gsv in (0.37, 65536.0):
                A = Arena(n, 'random', shadow, seed=7)
                gs = torch.tensor([gsv], device=DEV)
                snap = A.snapshot()
                w = f'{entry}, n = {n}, grad_scale_dev = {gsv}'
                assert call(A, gs, torch.zeros(1, dtype=torch.int32, device=DEV)) == 0          # a zero flag: the step runs
                A.check_step(snap, w, lr=lr, wd=wd, bc1=bc1, bc2_sqrt=bc2, gs=gsv)
            for flag in (1, -7):                         # nonzero: all four arrays and the shadow keep their bits
                A = Arena(n, 'random', shadow, seed=8)
                snap = A.snapshot()
                assert call(A, torch.tensor([0.5], device=DEV), torch.tensor([flag], dtype=torch.int32, device=DEV)) == 0
                A.check_unchanged(snap, f'{entry}, n = {n}, skip_flag = {flag}')
                _untouched(A.S, f'{entry}, n = {n}, skip_flag = {flag}: shadow')


def _decision_step(entry, A, st, cfg, w, n_groups=2):
    """one mmae_opt_step / mmae_opt_step_groups call under `cfg`, state and istate against opt_decision_ref, then every element
    with the scale, learning rate, weight decay and bias corrections the kernel reported"""
    lib = _lib()
    s_before, i_before = st.read()
    snap = A.snapshot()
    dev = lambda x, dt=torch.float32: None if x is None else torch.tensor([x] if not isinstance(x, (list, tuple)) else list(x), dtype=dt, device=DEV)
    loss, finf, gsc, lrwd = dev(cfg.get('loss')), dev(cfg.get('found_inf')), dev(cfg.get('grad_scale')), dev(cfg.get('lrwd'))
    fields = dict(clip_grad=cfg.get('clip', 0.0), skip_grad=cfg.get('skip_at', 0.0), grad_prescale=cfg.get('prescale', 1.0),
                  loss_dev=loss.data_ptr() if loss is not None else None, found_inf_dev=finf.data_ptr() if finf is not None else None,
                  grad_scale_dev=gsc.data_ptr() if gsc is not None else None)
    lr, wd = cfg.get('lr', 1e-3), cfg.get('wd', 0.05)
    if entry == 'mmae_opt_step':
        d = _opt_desc(A, st, lr=lr, weight_decay=wd, lrwd_dev=lrwd.data_ptr() if lrwd is not None else None, **fields)
        rc = lib.mmae_opt_step(ctypes.byref(d), _st())
        lr_el, wd_el = (cfg['lrwd'] if lrwd is not None else (lr, wd))
        lr0, wd0 = lr_el, wd_el
    else:
        gmap, hyper, lr_el, wd_el = _group_setup(A.n, n_groups, lr, wd)
        hd = hyper.to(DEV)
        by_value = entry.endswith(':hyper')
        d, keep = _groups_desc(A, st, gmap, n_groups, hyper=hyper.tolist() if by_value else None, hyper_dev=None if by_value else hd, **fields)
        rc = lib.mmae_opt_step_groups(ctypes.byref(d), _st())
        lr0, wd0 = float(hyper[0]), float(hyper[1])     # state[3..4] record group 0's
    assert rc == 0, (w, rc, lib.mmae_last_error())
    ss, b_ss = sumsq_ref(A.g)
    ref = opt_decision_ref(ss, b_ss, istate=i_before, lr=lr0, wd=wd0, b1=B1, b2=B2, clip=cfg.get('clip'), skip_at=cfg.get('skip_at'),
                           prescale=cfg.get('prescale', 1.0), loss=cfg.get('loss'), found_inf=cfg.get('found_inf'),
                           grad_scale=cfg.get('grad_scale'))
    s, i = st.read()
    assert i[:6] == ref['istate'] and i[6:] == [0, 0], (w, i, ref['istate'])
    assert ref['skip'] == cfg['skips'], (w, 'the case does not exercise the branch it names')
    for k in (1, 2):
        want, bound = ref['state'][k]
        if math.isfinite(want):
            assert abs(s[k] - want) <= bound, (w, f'state[{k}]', s[k], want, bound)
        else:
            assert not math.isfinite(s[k]) and (math.isnan(s[k]) == math.isnan(want)), (w, f'state[{k}]', s[k], want)
    if math.isfinite(ss):
        assert abs(s[0] - ss) <= b_ss, (w, 'state[0]', s[0], ss, b_ss)
    assert s[3] == ref['state'][3] and s[4] == ref['state'][4] and s[7] == 0.0, (w, s, ref['state'])
    _check_bc(s, ref['istate'][1], w)
    st.intact(w)
    if ref['skip']:
        A.check_unchanged(snap, w)
    else:
        A.check_step(snap, w, lr=lr_el, wd=wd_el, bc1=s[5], bc2_sqrt=s[6], gs=s[2])
    return s, i


@pytest.mark.parametrize('entry', ENTRIES[2:])
def test_opt_step_decisions_counters_and_elements(entry):
    n = 262147
    A = Arena(n, 'random', torch.bfloat16, seed=9)
    st = OptState()

    g_clean = A.g.clone()
    norm = math.sqrt(sumsq_ref(g_clean)[0])
    run = lambda cfg, w: _decision_step(entry, A, st, cfg, f'{entry}: {w}')

    def set_g(g):
        A.g.copy_(g)
        A.g0 = A.g.clone()

    s, i = run(dict(skips=False), 'no clip, no skip')
    assert i[1] == 1 and s[2] == 1.0
    s, i = run(dict(clip=0.5 * norm, skips=False), 'clip only')
    assert s[2] < 1.0                                                                          # the clip engaged
    s, i = run(dict(clip=2.0 * norm, skips=False), 'clip above the norm: scale 1')
    assert s[2] == 1.0 and i[1] == 3
    s, i = run(dict(skip_at=0.5 * norm, skips=True), 'skip only')
    assert i[:4] == [1, 3, 0, 1]                                                               # t stays put across a skipped step
    s, i = run(dict(skip_at=2.0 * norm, skips=False), 'skip_grad above the norm')
    assert i[1] == 4
    s, i = run(dict(clip=0.5 * norm, skip_at=0.5 * norm, skips=False), 'clip and skip: clip first, no skip')
    assert i[:4] == [0, 5, 0, 1] and s[2] < 1.0
    s, i = run(dict(prescale=0.25, clip=0.2 * norm, skips=False), 'grad_prescale 0.25 with clip')
    assert s[1] < 0.5 * norm
    # GradScaler's scale still on the gradients: the same step as with the unscaled gradient, its norm and scale within their bounds
    set_g(g_clean * 65536.0)
    s, i = run(dict(grad_scale=65536.0, prescale=0.5, clip=0.4 * norm, skips=False), 'grad_scale_dev 65536 on pre-multiplied gradients')
    ss, b_ss = sumsq_ref(g_clean)
    un = opt_decision_ref(ss, b_ss, istate=[0] * 6, lr=1e-3, wd=0.05, b1=B1, b2=B2, clip=0.4 * norm, skip_at=0.0, prescale=0.5)
    assert abs(s[1] - un['state'][1][0]) <= un['state'][1][1] and abs(s[2] * 65536.0 - un['state'][2][0]) <= un['state'][2][1]
    set_g(g_clean)
    t = i[1]
    s, i = run(dict(found_inf=1.0, skips=True), 'found_inf_dev > 0')
    assert i[:6] == [1, t, 0, 2, 1, 0]
    s, i = run(dict(found_inf=0.0, loss=1.5, skips=False), 'found_inf_dev = 0 and a finite loss')
    s, i = run(dict(loss=float('inf'), skips=True), 'a non-finite loss')
    s, i = run(dict(loss=float('nan'), clip=0.5 * norm, skips=True), 'a NaN loss')
    assert i[:6] == [1, t + 1, 2, 4, 1, 0]
    bad = g_clean.clone()
    bad[n - 2] = float('nan')                                                                    # in the scalar tail of the last workgroup
    set_g(bad)
    s, i = run(dict(clip=0.5 * norm, skips=True), 'a NaN gradient')
    bad[n - 2] = 1.0
    bad[70000] = float('-inf')
    set_g(bad)
    s, i = run(dict(skips=True), 'an inf gradient')
    assert i[:6] == [1, t + 1, 2, 6, 1, 2]
    set_g(g_clean)
    if entry == 'mmae_opt_step':
        s, i = run(dict(lrwd=(3e-3, 0.0), skips=False), 'lrwd_dev overrides the host lr / wd')
        assert s[3] == f32r(3e-3) and s[4] == 0.0
    else:
        s, i = run(dict(lr=3e-3, wd=0.01, skips=False), 'another table of group values')
    assert i[:6] == [0, t + 2, 2, 6, 1, 2]


@pytest.mark.parametrize('n_groups,kind', [(1, 'hyper'), (2, 'hyper'), (256, 'hyper'), (257, 'hyper_dev'), (1, 'hyper_dev'), (2, 'hyper_dev')])
def test_opt_step_groups_every_element_gets_its_own_group(n_groups, kind):
    lib = _lib()
    for n in (64 * 9 + 37, 64 * 300 + 1):              # ten chunks, the last one holds the scalar tail; 301 chunks reach every group
        A = Arena(n, 'random', torch.bfloat16, seed=10)
        st = OptState()
        gmap, hyper, lr_el, wd_el = _group_setup(n, n_groups, 1e-3, 0.02)
        hd = hyper.to(DEV)
        for t in (1, 2, 3):
            snap = A.snapshot()
            d, keep = _groups_desc(A, st, gmap, n_groups, hyper=hyper.tolist() if kind == 'hyper' else None, hyper_dev=hd if kind != 'hyper' else None)
            assert lib.mmae_opt_step_groups(ctypes.byref(d), _st()) == 0, lib.mmae_last_error()
            s, i = st.read()
            assert i[:2] == [0, t] and s[3] == float(hyper[0]) and s[4] == float(hyper[1])
            A.check_step(snap, f'mmae_opt_step_groups, {n_groups} groups by {kind}, n = {n}, step {t}', lr=lr_el, wd=wd_el, bc1=s[5],
                         bc2_sqrt=s[6], gs=s[2])
        if n_groups == 1:                                # one group: mmae_opt_step's results bit for bit (mmae.h)
            B = Arena(n, 'random', torch.bfloat16, seed=10)
            sb = OptState()
            for t in (1, 2, 3):
                d = _opt_desc(B, sb, lr=float(hyper[0]), weight_decay=float(hyper[1]))
                assert lib.mmae_opt_step(ctypes.byref(d), _st()) == 0
            for x, y, nm in ((A.p, B.p, 'p'), (A.m, B.m, 'm'), (A.v, B.v, 'v'), (A.S.view[0], B.S.view[0], 'shadow')):
                _bits_equal(x, y, f'one group against mmae_opt_step, n = {n}: {nm}')


def test_opt_step_groups_refuses_257_groups_by_value_and_writes_nothing():
    lib = _lib()
    n = 64 * 300 + 1
    A = Arena(n, 'random', torch.bfloat16, seed=10)
    st = OptState()
    gmap, hyper, _, _ = _group_setup(n, 257, 1e-3, 0.02)
    snap = A.snapshot()
    s0, i0 = st.read()
    d, keep = _groups_desc(A, st, gmap, 257, hyper=hyper.tolist())
    assert lib.mmae_opt_step_groups(ctypes.byref(d), _st()) < 0
    for ng in (0, -1, 65537):
        d, keep = _groups_desc(A, st, gmap, ng, hyper_dev=hyper.to(DEV))
        assert lib.mmae_opt_step_groups(ctypes.byref(d), _st()) < 0
    torch.cuda.synchronize()
    assert st.read() == (s0, i0)
    _untouched(st.ws, 'refused call: ws')
    A.check_unchanged(snap, 'refused call')
    _untouched(A.S, 'refused call: shadow')


def test_shadow_dtype_and_alignment_without_a_kernel_flavour_are_refused():
    """A shadow is f32 or bf16; any other code (fp16 included) took the f32 kernel.  The shadow given here has 4 bytes per element
    inside a Guarded buffer whatever its code says, and the call must return MMAE_EINVAL with nothing launched: p, m, v, the
    shadow, state, istate and ws keep their bits."""
    lib = _lib()
    n = 1027
    A = Arena(n, 'random', torch.float32, seed=11)
    st = OptState()
    gmap, hyper, _, _ = _group_setup(n, 2, 1e-3, 0.02)
    hy = torch.tensor([1e-3, 0.05, 0.1, 0.2], dtype=torch.float32, device=DEV)
    snap = A.snapshot()
    s0, i0 = st.read()
    base = A.S.view.data_ptr()

    def all_four(sp, code, why):
        assert lib.mmae_adamw(*A.ptrs(), n, 1e-3, B1, B2, EPS, 0.05, 1, None, None, sp, code, _st()) == EINVAL, f'mmae_adamw: {why}'
        assert lib.mmae_adamw_dev(*A.ptrs(), n, hy.data_ptr(), B1, B2, EPS, None, None, sp, code, _st()) == EINVAL, f'mmae_adamw_dev: {why}'
        d = _opt_desc(A, st, lr=1e-3, weight_decay=0.05, shadow=sp, shadow_dtype=code)
        assert lib.mmae_opt_step(ctypes.byref(d), _st()) == EINVAL, f'mmae_opt_step: {why}'
        d, keep = _groups_desc(A, st, gmap, 2, hyper=hyper.tolist(), shadow=sp, shadow_dtype=code)
        assert lib.mmae_opt_step_groups(ctypes.byref(d), _st()) == EINVAL, f'mmae_opt_step_groups (hyper): {why}'
        d, keep = _groups_desc(A, st, gmap, 2, hyper_dev=hyper.to(DEV), shadow=sp, shadow_dtype=code)
        assert lib.mmae_opt_step_groups(ctypes.byref(d), _st()) == EINVAL, f'mmae_opt_step_groups (hyper_dev): {why}'

    for code in (F16, 2, 3, 4, U16, I32, -1, 99):
        all_four(base, code, f'shadow_dtype {code}')
    all_four(base + 4, F32, 'f32 shadow 4 bytes off a 16-byte border')       # st4 on f32 needs 16 bytes
    all_four(base + 8, F32, 'f32 shadow 8 bytes off a 16-byte border')
    all_four(base + 2, BF16, 'bf16 shadow 2 bytes off an 8-byte border')     # st4 on bf16 needs 8 bytes
    all_four(base + 4, BF16, 'bf16 shadow 4 bytes off an 8-byte border')
    torch.cuda.synchronize()
    assert st.read() == (s0, i0)
    _untouched(st.ws, 'refused shadow: ws')
    A.check_unchanged(snap, 'refused shadow')
    _untouched(A.S, 'refused shadow')
    # a null shadow ignores the code, as before
    assert lib.mmae_adamw(*A.ptrs(), n, 1e-3, B1, B2, EPS, 0.05, 1, None, None, None, F16, _st()) == 0


@pytest.mark.parametrize('n', SIZES + [N_SUMSQ_2, N_SUMSQ_3, N_ADAMW_2])
def test_sumsq_against_fp64_and_ws_written_only_below_nb(n):
    lib = _lib()
    g_ = torch.Generator(device=DEV).manual_seed(n)
    cases = [('random', torch.randn(n, device=DEV, generator=g_))]
    tiny = torch.full((n,), 1e-3, device=DEV)
    tiny[n // 2] = 3.0                                   # one large element among tiny ones
    cases.append(('one large element among tiny ones', tiny))
    for name, x in cases:
        x0 = x.clone()
        out, ws = _vec(1, fill=torch.zeros(1)), _vec(1024)
        assert lib.mmae_sumsq(x.data_ptr(), n, out.view.data_ptr(), ws.view.data_ptr(), _st()) == 0
        s, b = sumsq_ref(x)
        got = float(out.view[0, 0])
        assert abs(got - s) <= b, (name, n, got, s, b)
        nb = min((n + 1023) // 1024, 1024)
        wsv = ws.view[0]
        assert bool(torch.isfinite(wsv[:nb]).all()) and abs(float(wsv[:nb].double().sum()) - s) <= b, (name, n, 'partials')
        assert bool((wsv[nb:].view(torch.int32) == -5898331).all()), f'n = {n}: ws written at or beyond nb = {nb}'
        out.intact('sumsq out')
        ws.intact('sumsq ws')
        _bits_equal(x, x0, 'sumsq input')


# =================================================================================================================================
# Streaming casts, transposes, axpy, add_n, the bf16 split
# =================================================================================================================================
def _from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


# +-0, subnormals, +-inf, NaNs (quiet, signalling, negative with payload), values that round up to inf in bf16 (>= 0x7f7f8000), the
# largest finite f32, round-to-nearest-even ties both ways in bf16 (0x3f808000 down to even, 0x3f818000 up to even), one past a tie;
# fp16: the largest finite value, just below the border to inf, the border (a tie: to even = inf), beyond it, values that land in
# the fp16 subnormals (2^-24 spacing), the tie at half the smallest subnormal (to even = 0) and just above it
SPECIALS = torch.cat([_from_bits([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000, 0x7f800000, 0xff800000, 0x7fc00000,
                                  0x7fa00001, 0xffc12345, 0x7f7f8000, 0xff7f8000, 0x7f7fffff, 0x7f7f7fff, 0x3f808000, 0x3f818000,
                                  0x3f808001, 0xbf808000, 0xbf818000]),
                      torch.tensor([65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e5, -1e5, 2.0 ** -14, 2.0 ** -15, 3.3e-6, 2.0 ** -24,
                                    2.0 ** -25, 2.0 ** -25 * 1.0001, -(2.0 ** -25), 6e-8, 1e-7, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24])])
STREAM_SIZES = [0, 1, 3, 4, 5, 1023, 1025, N_STREAM_2]


def _stream_input(n, seed, scale=1.0):
    """f32 values over many magnitudes with SPECIALS at the head (vector path) and at the tail (scalar path)"""
    g_ = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g_) * torch.exp2(torch.randint(-20, 20, (n,), generator=g_).float()) * scale
    k = len(SPECIALS)
    if n >= 2 * k:
        x[:k], x[-k:] = SPECIALS, SPECIALS.flip(0)
    elif n:
        x[:] = SPECIALS[(seed % 7):][:n] if n <= k - 7 else torch.cat([SPECIALS, SPECIALS])[:n]
    return x


def _src(x):
    """a source on the device; for n = 0 four elements, so that the pointer is not null"""
    return x.to(DEV) if x.numel() else torch.zeros(4, dtype=x.dtype, device=DEV)


def _all_16bit_patterns(n, seed):
    """every 16-bit pattern (all NaNs, infs, subnormals of bf16 / fp16) when n allows, random ones otherwise"""
    g_ = torch.Generator().manual_seed(seed)
    b = torch.randint(-32768, 32768, (n,), generator=g_, dtype=torch.int64)
    if n >= 65536:
        b[:65536] = torch.arange(-32768, 32768)
    return b.to(torch.int16)


@pytest.mark.parametrize('n', STREAM_SIZES)
def test_cast_f32_bf16_both_ways_bit_exact(n):
    lib = _lib()
    x = _stream_input(n, 20 + n % 5)
    xd = _src(x)
    out = _vec(max(n, 1), torch.bfloat16)
    assert lib.mmae_cast_f32_to_bf16(xd.data_ptr(), out.view.data_ptr(), n, _st()) == 0
    if n:
        _bits_equal(out.view[0], bf16_bits_ref(x), f'mmae_cast_f32_to_bf16, n = {n}')
        out.intact(f'mmae_cast_f32_to_bf16, n = {n}')
    else:
        _untouched(out, 'mmae_cast_f32_to_bf16, n = 0')
    _bits_equal(xd[:n], x, 'cast source')
    b = _all_16bit_patterns(n, 21)
    bd = _src(b)
    out = _vec(max(n, 1), torch.float32)
    assert lib.mmae_cast_bf16_to_f32(bd.data_ptr(), out.view.data_ptr(), n, _st()) == 0
    if n:
        _bits_equal(out.view[0], bf16_to_f32_ref(b), f'mmae_cast_bf16_to_f32, n = {n}')
        out.intact(f'mmae_cast_bf16_to_f32, n = {n}')
    else:
        _untouched(out, 'mmae_cast_bf16_to_f32, n = 0')


# scale_amax: None (no scalar), 2^k {1, 1.5, 1.999} with k at both ends of the range the formula is applied in ([-119, 126]) and in
# the middle, both sides of both cut-offs, and the values that switch the scale off
AMAX = [None] + [2.0 ** k * f for k in (-119, -118, -21, 0, 7, 125, 126) for f in (1.0, 1.5, 1.999)] + \
       [2.0 ** -119 * (1 - 2.0 ** -24), 2.0 ** -120, 2.0 ** -126, 2.0 ** 127, 2.0 ** 127 * 1.5, 0.0, 1e-45, 2.0 ** -127, float('inf'), float('nan')]


def _cast_f16_case(n, amax, seed):
    lib = _lib()
    am = None if amax is None else torch.tensor([amax], dtype=torch.float32, device=DEV)
    amp = None if am is None else am.data_ptr()
    m = f32r(amax) if amax is not None and math.isfinite(amax) and 0 < amax else 1.0
    m = min(max(m, 2.0 ** -100), 2.0 ** 100)
    x = _stream_input(n, seed)
    if n > 2 * len(SPECIALS):                            # gradient-like values around the scalar: they land all over fp16's range
        k = len(SPECIALS)
        g_ = torch.Generator().manual_seed(seed + 1)
        x[k:n - k] = torch.randn(n - 2 * k, generator=g_) * m * torch.exp2(torch.randint(-26, 14, (n - 2 * k,), generator=g_).float())
    xd = _src(x)
    out = _vec(max(n, 1), torch.float16)
    assert lib.mmae_cast_f32_to_f16(xd.data_ptr(), out.view.data_ptr(), n, amp, _st()) == 0
    w = f'mmae_cast_f32_to_f16, n = {n}, scale_amax = {amax}'
    if n:
        _equal_nan_as_nan(out.view[0], f32_to_f16_ref(x, amax), w)
        out.intact(w)
    else:
        _untouched(out, w)
    h = _all_16bit_patterns(n, seed + 2).view(torch.float16)
    hd = _src(h)
    out = _vec(max(n, 1), torch.float32)
    assert lib.mmae_cast_f16_to_f32(hd.data_ptr(), out.view.data_ptr(), n, amp, _st()) == 0
    w = f'mmae_cast_f16_to_f32, n = {n}, scale_amax = {amax}'
    if n:
        _equal_nan_as_nan(out.view[0], f16_to_f32_ref(h, amax), w)
        out.intact(w)
    else:
        _untouched(out, w)
    if am is not None:
        _bits_equal(am, torch.tensor([amax], dtype=torch.float32), 'the scale_amax scalar')


@pytest.mark.parametrize('n', STREAM_SIZES)
def test_cast_f16_both_ways_bit_exact_with_and_without_scale(n):
    for amax in (None, 0.9e-6, 2.0 ** -119, 2.0 ** 126 * 1.999):
        _cast_f16_case(n, amax, 30 + n % 7)


def test_cast_f16_scale_over_its_whole_exponent_range():
    for j, amax in enumerate(AMAX):
        for n in (5, 70003):                             # 70003 holds every fp16 pattern and a 3-element tail
            _cast_f16_case(n, amax, 40 + j)


def test_cast_f16_overflow_becomes_inf_not_a_clamp():
    lib = _lib()
    x = torch.tensor([65504.0, 65519.996, 65520.0, -65520.0, 1e5, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001], device=DEV)
    out = _vec(8, torch.float16)
    assert lib.mmae_cast_f32_to_f16(x.data_ptr(), out.view.data_ptr(), 8, None, _st()) == 0
    assert out.view[0].cpu().tolist() == [65504.0, 65504.0, float('inf'), float('-inf'), float('inf'), 2.0 ** -24, 0.0, 2.0 ** -24]


TC_SHAPES = [(1, 1), (1, 257), (257, 1), (63, 65), (64, 64), (65, 63), (64, 130), (130, 257), (257, 130), (65, 1), (63, 64)]


@pytest.mark.parametrize('dst', ['f32', 'bf16'])
def test_transpose_cast_bit_exact(dst):
    lib = _lib()
    for rows, cols in TC_SHAPES:
        x = _stream_input(rows * cols, rows + cols).reshape(rows, cols)
        xd = x.to(DEV)
        dt = torch.float32 if dst == 'f32' else torch.bfloat16
        out = Guarded(cols, rows, rows, dt, DEV)
        assert lib.mmae_transpose_cast(xd.data_ptr(), out.view.data_ptr(), F32 if dst == 'f32' else BF16, rows, cols, _st()) == 0
        ref = x.t().contiguous()
        w = f'mmae_transpose_cast to {dst}, {rows} x {cols}'
        _bits_equal(out.view, ref if dst == 'f32' else bf16_bits_ref(ref), w)
        out.intact(w)
        _bits_equal(xd, x, 'transpose source')


def test_transpose_cast_refuses_a_destination_type_without_a_kernel():
    lib = _lib()
    rows, cols = 65, 63
    xd = torch.randn(rows, cols, device=DEV)
    out = Guarded(cols, rows, rows, torch.float32, DEV)          # 4 bytes per element whatever the code says
    for code in (F16, 2, 3, 4, U16, I32, -1):
        assert lib.mmae_transpose_cast(xd.data_ptr(), out.view.data_ptr(), code, rows, cols, _st()) == EINVAL, code
    for r, c in ((0, 4), (4, 0), (-1, 4)):
        assert lib.mmae_transpose_cast(xd.data_ptr(), out.view.data_ptr(), F32, r, c, _st()) == EINVAL
    torch.cuda.synchronize()
    _untouched(out, 'refused mmae_transpose_cast')


@pytest.mark.parametrize('n', STREAM_SIZES)
def test_axpy_is_one_fma_per_element(n):
    """axpy_kernel's `y += a * x` compiles to v_pk_fma_f32 on the vector path and v_fmac_f32 on the scalar tail (hipcc
    --offload-arch=gfx950 -S, default -ffp-contract=fast): one rounding, so the reference is the correctly rounded fmaf."""
    lib = _lib()
    g_ = torch.Generator().manual_seed(50 + n % 3)
    for a in (0.3, 1.0, -2.5e-3):
        x = torch.randn(n, generator=g_) * torch.exp2(torch.randint(-8, 8, (n,), generator=g_).float())
        y = torch.randn(n, generator=g_)
        if n > 8:
            y[:4], y[-3:] = -a * x[:4], -a * x[-3:]          # cancellation: what mul + add and the FMA disagree on most
        xd = _src(x)
        Y = _vec(max(n, 1), fill=y if n else None)
        assert lib.mmae_axpy_f32(Y.view.data_ptr(), xd.data_ptr(), a, n, _st()) == 0
        w = f'mmae_axpy_f32, n = {n}, a = {a}'
        if n:
            _bits_equal(Y.view[0], fma_f32_ref(a, x, y), w)
            Y.intact(w)
        else:
            _untouched(Y, w)
        _bits_equal(xd[:n], x, 'axpy x')


@pytest.mark.parametrize('n_in', [1, 2, 3, 4, 5, 6, 7, 8])
def test_add_n_is_the_left_to_right_chain(n_in):
    lib = _lib()
    g_ = torch.Generator().manual_seed(60 + n_in)
    for n in [0, 4, 1024, 4100] + ([N_STREAM_2 + 1] if n_in in (2, 8) else []):
        xs = [torch.randn(n, generator=g_) * 10.0 ** (k % 4) for k in range(n_in)]
        ref = add_n_ref(xs)
        xd = [_src(x) for x in xs]
        out = _vec(max(n, 4))
        assert lib.mmae_add_n_f32(out.view.data_ptr(), _ptrs([x.data_ptr() for x in xd]), n_in, n, _st()) == 0
        w = f'mmae_add_n_f32, {n_in} inputs, n = {n}'
        if n:
            _bits_equal(out.view[0, :n], ref, w)
            out.intact(w)
        else:
            _untouched(out, w)
        for x, d in zip(xs, xd):
            _bits_equal(d[:n], x, 'add_n input')
        if n:                                            # out aliasing in[0]
            al = _vec(n, fill=xs[0])
            assert lib.mmae_add_n_f32(al.view.data_ptr(), _ptrs([al.view.data_ptr()] + [x.data_ptr() for x in xd[1:]]), n_in, n, _st()) == 0
            _bits_equal(al.view[0], ref, w + ', out = in[0]')
            al.intact(w + ', out = in[0]')
    out = _vec(8)
    x = torch.randn(8, device=DEV)
    for bad_n_in, bad_n in ((0, 8), (9, 8), (2, 6), (2, -4)):
        assert lib.mmae_add_n_f32(out.view.data_ptr(), _ptrs([x.data_ptr()] * 9), bad_n_in, bad_n, _st()) == EINVAL
    _untouched(out, 'refused mmae_add_n_f32')


def _x3_input(rows, cols, seed):
    g_ = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g_) * torch.exp2(torch.randint(-90, 90, (rows, cols), generator=g_).float())
    e = _from_bits([0x00000000, 0x80000000, 0x3f808000, 0x3f818000, 0x3f80ffff, 0x7f7f7fff, 0x00800000, 0x80800001])
    x.view(-1)[:8], x.view(-1)[-8:] = e, e.flip(0)
    return x


def _x3_expect(x, lo_seg):
    hi, lo = x3_split_ref(x)
    return [lo if s == lo_seg else hi for s in range(3)]


@pytest.mark.parametrize('rows,cols', [(1, 8), (5, 24), (33, 64), (1000, 72), (4099, 8200)])
def test_x3_split_both_layouts_bit_exact(rows, cols):
    """(4099, 8200): 4 201 475 units of 8 elements, past the 16384 x 256 grid of x3_split_kernel"""
    lib = _lib()
    big = rows * cols > 10 ** 6
    x = _x3_input(rows, cols, rows)
    for lo_seg in ((1,) if big else (0, 1, 2)):
        segs = _x3_expect(x, lo_seg)
        for ldx, pad in ((cols, 0),) if big else ((cols, 0), (cols + 12, 16)):
            xb = torch.full((rows, ldx), float('nan'))   # NaN in the ld padding: never read
            xb[:, :cols] = x
            xd = xb.to(DEV)
            w = f'mmae_x3_split {rows} x {cols}, lo_seg {lo_seg}, ldx {ldx}'
            # segments side by side in a row: out [rows][out_ld], seg_stride = cols; out_ld > 3 cols leaves the pad untouched
            out = Guarded(rows, 3 * cols, 3 * cols + pad, torch.bfloat16, DEV)
            assert lib.mmae_x3_split(xd.data_ptr(), ldx, rows, cols, out.view.data_ptr(), 3 * cols + pad, cols, lo_seg, _st()) == 0, lib.mmae_last_error()
            _bits_equal(out.view, torch.cat(segs, 1), w + ', segments along the row')
            out.intact(w)
            # segments stacked along the rows: out [3 rows][cols], seg_stride = rows cols
            out = Guarded(3 * rows, cols, cols, torch.bfloat16, DEV)
            assert lib.mmae_x3_split(xd.data_ptr(), ldx, rows, cols, out.view.data_ptr(), cols, rows * cols, lo_seg, _st()) == 0
            _bits_equal(out.view, torch.cat(segs, 0), w + ', segments stacked')
            out.intact(w)
            _bits_equal(xd, xb, 'x3_split source')
    out = Guarded(rows, 3 * cols, 3 * cols, torch.bfloat16, DEV)
    xd = x.to(DEV)
    for args in ((cols, rows, cols, 3 * cols, cols, 3), (cols, rows, cols, 3 * cols, cols, -1), (cols, rows, cols - 4, 3 * cols, cols, 1),
                 (cols, 0, cols, 3 * cols, cols, 1), (cols + 2, rows, cols, 3 * cols, cols, 1), (cols, rows, cols, 3 * cols + 4, cols, 1)):
        ldx, r, c, old, ss, ls = args
        assert lib.mmae_x3_split(xd.data_ptr(), ldx, r, c, out.view.data_ptr(), old, ss, ls, _st()) == EINVAL, args
    _untouched(out, 'refused mmae_x3_split')


def test_x3_prepare_weights_writes_both_layouts():
    lib = _lib()
    shapes = [(40, 24), (7, 64), (130, 8)]               # [n_out][k_in]
    ws = [_x3_input(no, ki, 70 + no) for no, ki in shapes]
    wd = [w.to(DEV) for w in ws]
    fwd = [Guarded(no, 3 * ki, 3 * ki, torch.bfloat16, DEV) for no, ki in shapes]
    dx = [Guarded(3 * no, ki, ki, torch.bfloat16, DEV) for no, ki in shapes]
    dst = []
    for a, b in zip(fwd, dx):
        dst += [a.view.data_ptr(), b.view.data_ptr()]
    assert lib.mmae_x3_prepare_weights(len(ws), _ptrs([w.data_ptr() for w in wd]), _i32s([s[0] for s in shapes]),
                                       _i32s([s[1] for s in shapes]), _ptrs(dst), _st()) == 0
    for w, a, b, s in zip(ws, fwd, dx, shapes):
        hi, lo = x3_split_ref(w)
        _bits_equal(a.view, torch.cat([hi, lo, hi], 1), f'mmae_x3_prepare_weights {s}: [hi | lo | hi]')
        _bits_equal(b.view, torch.cat([hi, lo, hi], 0), f'mmae_x3_prepare_weights {s}: [hi ; lo ; hi]')
        a.intact(f'x3_prepare_weights {s}')
        b.intact(f'x3_prepare_weights {s}')
    assert lib.mmae_x3_prepare_weights(0, None, None, None, None, _st()) == 0


# =================================================================================================================================
# Truncated depth standardisation
# =================================================================================================================================
DEPTH_N = [2, 3, 7, 1000, 1023, 1024, 1025, 50176]
DEPTH_EPS = 1e-6


def _cuts(n):
    c = [(0, n), (0, 2), (n - 2, n), (int(0.1 * n), int(0.9 * n)), (n // 2 - 1, n // 2 + 1)]
    return sorted({(lo, hi) for lo, hi in c if 0 <= lo and hi <= n and hi - lo >= 2})


def _runs(n, counts, g_):
    """a map of len(counts) distinct values, value j in counts[j] copies, shuffled (integers; the caller scales them)"""
    v = torch.cat([torch.full((max(c, 0),), j) for j, c in enumerate(counts)])[:n]
    v = torch.cat([v, torch.full((n - len(v),), len(counts) - 1)])
    return v[torch.randperm(n, generator=g_)]


def _depth_int_maps(n, lo, hi, seed):
    """integer-valued maps [B][n] whose ties sit where the cuts (lo, hi) fall:
      0 first copies: rank lo is the FIRST copy of a run and rank hi - 1 the LAST copy of one
      1 last / first: rank lo is the LAST copy of a run, rank hi - 1 the FIRST of the next one
      2 both cuts inside one run (k1 == k2: the slice is constant)
      3 constant    4 two-valued    5 seven values, long runs    6 all distinct"""
    g_ = torch.Generator().manual_seed(seed)
    w = hi - lo
    a = max(1, w // 3)
    maps = [_runs(n, [lo, a, w - 2 * a, a, n - hi], g_),
            _runs(n, [lo + 1, max(w - 2, 0), n - hi + 1], g_),
            _runs(n, [lo // 2, n - lo // 2 - (n - hi) // 2, (n - hi) // 2], g_),
            torch.full((n,), 3),
            (torch.arange(n) % 2) * 5,
            torch.randint(0, 7, (n,), generator=g_),
            torch.randperm(n, generator=g_)]
    return torch.stack(maps)


def _depth_f32_maps(n, lo, hi, seed):
    im = _depth_int_maps(n, lo, hi, seed).float()
    g_ = torch.Generator().manual_seed(seed + 1)
    neg = -(im * 0.37 + 0.6)                             # all-negative: the sign branch of key_of / val_of
    mixed = (im - im.median(dim=1, keepdim=True).values) * 0.37
    # a run of zeros of both signs around the median, so that a cut in the middle falls inside it
    z = torch.randn(n, generator=g_).sort().values
    z[n // 4: n - n // 4] = 0.0
    z[n // 4: n // 2] *= -1.0                            # -0.0 for the lower half of the run, +0.0 for the upper
    z = z[torch.randperm(n, generator=g_)]
    rnd = torch.randn(2, n, generator=g_) * torch.tensor([[3.0], [1e-3]]) + torch.tensor([[10.0], [-1.0]])
    return torch.cat([im * 0.37 - 0.6, neg, mixed, z[None], rnd])


def _check_depth(y, x, lo, hi, what):
    ref, bound = depth_std_ref(x, lo, hi, DEPTH_EPS)
    assert_within(y, ref, bound, what, names=('b', 'i'))


@pytest.mark.parametrize('n', DEPTH_N)
def test_depth_standardize_every_element_against_fp64(n):
    lib = _lib()
    for lo, hi in _cuts(n):
        x = _depth_f32_maps(n, lo, hi, n + lo).to(DEV)
        B = x.shape[0]
        x0 = x.clone()
        y = Guarded(B, n, n, torch.float32, DEV)
        w = f'mmae_depth_standardize, n = {n}, cuts [{lo}, {hi})'
        assert lib.mmae_depth_standardize(x.data_ptr(), y.view.data_ptr(), B, n, lo, hi, DEPTH_EPS, _st()) == 0
        _check_depth(y.view, x, lo, hi, w)
        y.intact(w)
        _bits_equal(x, x0, 'depth input')
        z = Guarded(B, n, n, torch.float32, DEV, fill=x)                   # y aliasing x: bit-equal to out of place
        assert lib.mmae_depth_standardize(z.view.data_ptr(), z.view.data_ptr(), B, n, lo, hi, DEPTH_EPS, _st()) == 0
        _bits_equal(z.view, y.view, w + ', in place')
        z.intact(w + ', in place')


@pytest.mark.parametrize('n', DEPTH_N)
def test_ingest_depth_standardize_u16_and_i32_against_fp64(n):
    lib = _lib()
    for lo, hi in _cuts(n):
        im = _depth_int_maps(n, lo, hi, 3 * n + hi)
        g_ = torch.Generator().manual_seed(n + hi)
        u16 = torch.cat([im * 9001 % 65536, torch.randint(0, 65536, (2, n), generator=g_), torch.full((1, n), 65535)])
        big = torch.randint(-2 ** 31, 2 ** 31, (2, n), generator=g_)       # |v| > 2^24: distinct integers round to one float
        big[1] = big[1] // 128 * 128 + torch.randint(0, 3, (n,), generator=g_)   # neighbours that share their float
        i32 = torch.cat([im * 40001 - 123457, -(im * 9001) - 1, big, (2 ** 24 + im), torch.randint(0, 65536, (1, n), generator=g_)])
        for code, vals in ((U16, u16), (I32, i32)):
            if code == U16:
                xd = torch.from_numpy(vals.numpy().astype(np.uint16).view(np.int16)).to(DEV)
            else:
                xd = vals.to(torch.int32).to(DEV)
            xf = (vals.to(torch.int32).to(torch.float32) * 2.0 ** -16).to(DEV)       # float(v) 2^-16, the value the kernel standardises
            B = vals.shape[0]
            y = Guarded(B, n, n, torch.float32, DEV)
            w = f'mmae_ingest_depth {"u16" if code == U16 else "i32"}, n = {n}, cuts [{lo}, {hi})'
            assert lib.mmae_ingest_depth(xd.data_ptr(), code, y.view.data_ptr(), B, n, 1, lo, hi, DEPTH_EPS, _st()) == 0
            _check_depth(y.view, xf, lo, hi, w)
            y.intact(w)
            y2 = Guarded(B, n, n, torch.float32, DEV)                      # mmae.h: bit-identical to converting first
            assert lib.mmae_depth_standardize(xf.data_ptr(), y2.view.data_ptr(), B, n, lo, hi, DEPTH_EPS, _st()) == 0
            _bits_equal(y.view, y2.view, w + ' against the f32 loader')
            conv = Guarded(B, n, n, torch.float32, DEV)                    # standardize = 0: the conversion alone
            assert lib.mmae_ingest_depth(xd.data_ptr(), code, conv.view.data_ptr(), B, n, 0, 0, 0, 0.0, _st()) == 0
            _bits_equal(conv.view, xf, w + ', conversion alone')
            conv.intact(w)


def test_depth_cut_arguments_out_of_range_are_refused():
    lib = _lib()
    n, B = 1000, 2
    x = torch.randn(B, n, device=DEV)
    xi = torch.randint(0, 65536, (B, n), dtype=torch.int32, device=DEV)
    xu = xi.to(torch.int16)
    y = Guarded(B, n, n, torch.float32, DEV)
    for lo, hi in ((10, 11), (10, 10), (500, 400), (0, n + 1), (-1, n), (-3, -1), (n - 1, n)):
        assert lib.mmae_depth_standardize(x.data_ptr(), y.view.data_ptr(), B, n, lo, hi, DEPTH_EPS, _st()) == EINVAL, (lo, hi)
        assert lib.mmae_ingest_depth(xi.data_ptr(), I32, y.view.data_ptr(), B, n, 1, lo, hi, DEPTH_EPS, _st()) == EINVAL, (lo, hi)
        assert lib.mmae_ingest_depth(xu.data_ptr(), U16, y.view.data_ptr(), B, n, 1, lo, hi, DEPTH_EPS, _st()) == EINVAL, (lo, hi)
    assert lib.mmae_depth_standardize(x.data_ptr(), y.view.data_ptr(), B, 1, 0, 1, DEPTH_EPS, _st()) == EINVAL
    assert lib.mmae_ingest_depth(xi.data_ptr(), F32, y.view.data_ptr(), B, n, 1, 0, n, DEPTH_EPS, _st()) == EINVAL
    torch.cuda.synchronize()
    _untouched(y, 'refused depth calls')
