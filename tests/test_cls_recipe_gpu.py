"""GPU: the classification fine-tuning recipe's kernels (csrc/clsrecipe.hip) and their host side (multimae_amd.Mixup,
SoftTargetCrossEntropy, LabelSmoothingCrossEntropy, ModelEma; dropin.amd_loop.mixup / cls_criterion / model_ema / LossScaler).

mixup_pairs, mix_target and ema_update are checked BIT FOR BIT (torch.equal) against the reference's own outputs in
tests/golden/cls_recipe.npz and against torch restatements of the reference's lines run on the same device; outputs live in Guarded
buffers.  The soft-target loss is checked element by element against fp64 torch (log_softmax expression + autograd).

Bounds of the loss (u = 2^-24, gamma_n as helpers.gamma; the file is compiled without FMA contraction, so every operation rounds
once).  A workgroup of 256 threads takes one row; n_t = ceil(K / 256) classes per thread.  bf16 logits are read exactly: the fp64
reference starts from the rounded values.
  lse    the exponential is exp2(d log2 e): d and the product round once each (2 u |d|), v_exp_f32 is good to 1 ulp (2 u).  A term
         exp(x_k - M) reaches the row's sum through its own exponential (2 u, argument 2 u range), at most n_t + 1 rescale products
         (product u, exponential 2 u each; their arguments add up to <= range: 2 u range) and n_t thread additions + 6 shuffle
         additions + 2 wave additions:
             r_s = gamma_(n_t + 8) + 2 u + 3 u (n_t + 1) + 4 u range;   |dlse| <= 1.01 r_s + 2 u |lse - max| + u |lse| = b_lse
         (logf taken as 2 u relative, the form of helpers.ce_loss_ref and tests/test_seg_loss_gpu.py).
  t_k    dense: given, exact.  Label form: off = s / K, conf = 1 - s, off + conf -- one rounding each, s the f32 the kernel
         receives: |dt_k| <= 3 u t_k = e_t.
  row    sum_k t_k (lse - x_k): the difference moves by b_lse and rounds (u |lse - x_k|), the product rounds (u); the sum over K
         terms in the same tree as above: sum_k |t_k| b_lse + (gamma_(n_t + 8) + 2 u + e_t / t_k) sum_k |t_k| |lse - x_k|
  loss   the rows are summed and divided by B in double, rounded to f32 once: mean(b_row) + 2 u |loss|
  dx     p = exp2((x - lse) log2 e): |dp| <= p (expm1(b_lse + 2 u |x - lse|) + 2 u).  tsum (dense form) is an fp32 sum of K
         targets: |dtsum| <= gamma_(n_t + 8) sum |t| (label form: exactly 1).  p tsum rounds (u), minus t_k rounds (u), scale = up / B
         is one division (u) and is applied with one product (u):
             |ddx| <= |scale| (tsum dp + p dtsum + u p tsum + e_t + u |p tsum - t_k|) + 2 u |dx| + ulp_out(dx)
         ulp_out the spacing of the logits' dtype at dx (f32: the last product's rounding; bf16: the store's).
Against the golden (the reference's f32 CPU run): kernel and reference are two f32 evaluations of the same fp64 value, so they agree
within the kernel's bound plus the same expression for the reference's own roundings: 2 b.
"""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multimae_amd as M
from multimae_amd import engine, ops
from dropin import amd_loop
from helpers import Guarded, assert_within, f32r, gamma, rel_err, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_cls_recipe import LOSS_GEOMS, STEP_K, VIT, perturbed  # noqa: E402

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'cls_recipe.npz'))
CASES = json.loads(GOLD['mix/cases'].item())
for _kw in CASES.values():
    if _kw.get('cutmix_minmax') is not None:
        _kw['cutmix_minmax'] = tuple(_kw['cutmix_minmax'])
U = 2.0 ** -24


def _t(key):
    return torch.from_numpy(GOLD[key])


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _guarded_batch(x0: torch.Tensor):
    B = x0.shape[0]
    g = Guarded(B, x0[0].numel(), x0[0].numel(), torch.float32, DEV, fill=x0.reshape(B, -1))
    return g, g.view.view(x0.shape)


# ------------------------------------------------------------------------------------------------ mixup_pairs / mix_target --
@pytest.mark.parametrize('case', list(CASES))
def test_mixup_matches_the_reference_bit_for_bit(case):
    """four consecutive calls of Mixup.__call__ under the fixture's seed: mixed batch and soft target equal the reference's bits"""
    kw = CASES[case]
    mix = M.Mixup(**kw)
    x0, labels = _t('mix/x'), _t('mix/labels').to(DEV)
    np.random.seed(1000 + list(CASES).index(case))
    for c in range(4):
        g, x = _guarded_batch(x0)
        xm, tgt = mix(x, labels)
        torch.cuda.synchronize()
        assert xm is x
        g.intact(f'{case} call {c}')
        assert torch.equal(_bits(xm), _bits(_t(f'mix/{case}/out{c}'))), (case, c)
        assert torch.equal(_bits(tgt), _bits(_t(f'mix/{case}/tgt{c}'))), (case, c)
    assert np.random.rand() == float(GOLD[f'mix/{case}/rand'][0])


def _restate(mode: str, x: torch.Tensor, rows: np.ndarray) -> torch.Tensor:
    """The three reference methods (utils/mixup.py:166-214) restated in torch on the parameters of one draw: the same eager
    expressions -- x.flip(0).mul_ / mul_ / add_ for the batch, the per-sample loops over a clone for 'elem' and 'pair'."""
    B = x.shape[0]
    w = rows[:, :4].copy().view(np.float32)
    box = rows[:, 4:]
    if mode == 'batch':
        yl, yh, xl, xh = (int(v) for v in box[0])
        if yl == ops.MIX_KEEP:
            return x
        if yl == ops.MIX_BLEND:
            x_flipped = x.flip(0).mul_(float(w[0, 1]))
            x.mul_(float(w[0, 0])).add_(x_flipped)
        else:
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        return x
    x_orig = x.clone()
    for i in range(B if mode == 'elem' else B // 2):
        j = B - i - 1
        yl, yh, xl, xh = (int(v) for v in box[i])
        if yl == ops.MIX_KEEP:
            continue
        if yl == ops.MIX_BLEND:
            x[i] = x[i] * float(w[i, 0]) + x_orig[j] * float(w[i, 1])
            if mode == 'pair':
                x[j] = x[j] * float(w[i, 0]) + x_orig[i] * float(w[i, 1])
        else:
            x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
            if mode == 'pair':
                x[j][:, yl:yh, xl:xh] = x_orig[i][:, yl:yh, xl:xh]
    return x


@pytest.mark.parametrize('mode', ['batch', 'pair', 'elem'])
@pytest.mark.parametrize('shape', [(2, 1, 1, 1), (4, 3, 7, 5), (8, 3, 224, 224)])
def test_mixup_pairs_against_the_torch_restatement(shape, mode):
    """random f32 data; (4, 3, 7, 5): the element-wise path with rows that start at any alignment; (8, 3, 224, 224): 16-byte accesses.
    Mixup only, CutMix only, both, and min / max boxes, three draws each."""
    g0 = torch.Generator().manual_seed(sum(shape))
    x0 = torch.randn(shape, generator=g0)
    variants = [dict(mixup_alpha=0.8, cutmix_alpha=0.), dict(mixup_alpha=0., cutmix_alpha=1.0), dict(mixup_alpha=0.8, cutmix_alpha=1.0),
                dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.6)]
    if min(shape[2:]) >= 5:
        variants.append(dict(mixup_alpha=0., cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8)))
    np.random.seed(5)
    kinds = set()
    for kw in variants:
        mix = M.Mixup(mode=mode, num_classes=5, **kw)
        for _ in range(3):
            rows = mix.draw(shape)
            kinds |= {min(int(v), 0) for v in rows[:, 4]}
            g, x = _guarded_batch(x0)
            ops.mixup_pairs(x, torch.from_numpy(rows).to(DEV))
            ref = _restate(mode, x0.to(DEV).clone(), rows)
            torch.cuda.synchronize()
            g.intact(f'{shape} {mode}')
            assert torch.equal(_bits(x), _bits(ref)), (shape, mode, kw)
    assert kinds >= {ops.MIX_BLEND, 0}


@pytest.mark.parametrize('shape', [(4, 3, 7, 5), (4, 2, 8, 12)])
def test_sample_with_lam_one_is_not_written(shape):
    """a sample the reference skips (lam == 1) keeps its bits although its partner holds NaN / inf -- a * 1 + b * 0 would not"""
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(2))
    x0[3, :, 1, 2] = float('nan')
    x0[3, :, 2, 3] = float('inf')
    x0[0, 0, 0, 0] = -0.0
    rows = np.zeros((4, 8), dtype=np.int32)
    w = np.array([[1., 0., 1., 0.], [0.25, 0.75, 0.25, 0.75], [0.5, 0.5, 0.5, 0.5], [0.3, 0.7, 0.3, 0.7]], dtype=np.float32)
    rows[:, :4] = w.view(np.int32)
    rows[:, 4] = [ops.MIX_KEEP, ops.MIX_KEEP, ops.MIX_BLEND, ops.MIX_BLEND]
    g, x = _guarded_batch(x0)
    ops.mixup_pairs(x, torch.from_numpy(rows).to(DEV))
    torch.cuda.synchronize()
    g.intact('lam == 1')
    assert torch.equal(_bits(x[:2]), _bits(x0[:2]))
    x0d = x0.to(DEV)
    exp2 = x0d[2] * 0.5 + x0d[1] * 0.5
    exp3 = x0d[3] * float(w[3, 0]) + x0d[0] * float(w[3, 1])
    assert torch.equal(_bits(x[2]), _bits(exp2)) and torch.equal(_bits(x[3]), _bits(exp3))
    assert bool(torch.isnan(x[3, :, 1, 2]).all())


def test_mixup_rejects_what_the_kernel_cannot_take():
    mix = M.Mixup(num_classes=5)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    x = torch.zeros(4, 3, 8, 8, device=DEV)
    for bad in (x.cpu(), x.double(), x.bfloat16(), x[:, :, ::2], x[0]):
        with pytest.raises(ValueError):
            mix(bad, y)
    with pytest.raises(ValueError):
        mix(x[:3], y[:3])
    with pytest.raises(ValueError):
        mix(x, torch.tensor([0, 1, 2, 5]))                         # host labels are range-checked before any launch


# ----------------------------------------------------------------------------------------------------------- soft-target CE --
def _soft_reference(xr: torch.Tensor, K: int, dense, labels, smoothing: float, up: float, out_dtype):
    """fp64 reference on the logits as the kernel reads them (xr [B, K] fp64) with the module docstring's bounds"""
    B = xr.shape[0]
    n_t = (K + 255) // 256
    x = xr.clone().requires_grad_(True)
    if dense is not None:
        t = dense.double()
        e_t = torch.zeros_like(t)
    else:
        s = f32r(smoothing)
        t = torch.full((B, K), s / K, dtype=torch.float64, device=xr.device)
        t[torch.arange(B, device=xr.device), labels] += 1.0 - s
        e_t = 3 * U * t
    loss = torch.sum(-t * F.log_softmax(x, dim=-1), dim=-1).mean()
    (d,) = torch.autograd.grad(loss * up, x)
    lse = torch.logsumexp(xr, 1)
    mx, rng = xr.amax(1), xr.amax(1) - xr.amin(1)
    r_s = gamma(n_t + 8) + 2 * U + 3 * U * (n_t + 1) + 4 * U * rng
    b_lse = 1.01 * r_s + 2 * U * (lse - mx).abs() + U * lse.abs()
    diff = (lse[:, None] - xr).abs()
    b_row = t.abs().sum(1) * b_lse + ((gamma(n_t + 8) + 2 * U) * t.abs() * diff + e_t * diff).sum(1)
    b_loss = float(b_row.mean()) + 2 * U * abs(float(loss))
    p = torch.exp(xr - lse[:, None])
    dp = p * (torch.expm1(b_lse[:, None] + 2 * U * diff) + 2 * U)
    if dense is not None:
        tsum, b_ts = t.sum(1, keepdim=True), gamma(n_t + 8) * t.abs().sum(1, keepdim=True)
    else:
        tsum, b_ts = torch.ones(B, 1, dtype=torch.float64, device=xr.device), torch.zeros(B, 1, dtype=torch.float64, device=xr.device)
    scale = abs(up) / B
    b_d = scale * (tsum.abs() * dp + p * b_ts + U * p * tsum.abs() + e_t + U * (p * tsum - t).abs()) + 2 * U * d.abs()
    b_d = b_d + ulp(out_dtype, d.abs() + b_d)
    return dict(lse=lse, b_lse=b_lse, loss=float(loss), b_loss=b_loss, d=d.detach(), b_d=b_d, tsum=tsum)


def _soft_run(xpad: torch.Tensor, ld: int, B: int, K: int, dense, labels, smoothing: float, up: float):
    lse_g = Guarded(1, B, B, torch.float32, DEV)
    lse, tsum, out = ops.soft_ce_fwd(xpad, ld, B, K, dense, labels, smoothing, lse=lse_g.view.view(B))
    d_g = Guarded(B, ld, ld, xpad.dtype, DEV)
    ops.soft_ce_bwd(xpad, ld, B, K, dense, labels, smoothing, lse, tsum, torch.tensor([up], device=DEV), d_g.view)
    torch.cuda.synchronize()
    lse_g.intact('soft_ce_fwd lse')
    d_g.intact('soft_ce_bwd dx')
    return lse, tsum, out, d_g


def _soft_target(B, K, g):
    """what Mixup returns: two smoothed one-hot rows blended per sample"""
    a, b = torch.randint(0, K, (B,), generator=g), torch.randint(0, K, (B,), generator=g)
    lam = torch.rand(B, 1, generator=g)
    off = 0.1 / K
    y1 = torch.full((B, K), off).scatter_(1, a[:, None], 0.9 + off)
    y2 = torch.full((B, K), off).scatter_(1, b[:, None], 0.9 + off)
    return y1 * lam + y2 * (1. - lam)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('B', [1, 6, 128])
@pytest.mark.parametrize('K', [1, 3, 7, 1000, 1001, 21841])
def test_soft_ce_forward_and_backward_per_element(K, B, dtype):
    """both target forms; the padding columns K .. ld - 1 hold NaN on input and come back as exact zeros in dx"""
    g = torch.Generator().manual_seed(K * 131 + B)
    ld = K + 3
    xpad = torch.full((B, ld), float('nan'))
    xpad[:, :K] = torch.randn(B, K, generator=g) * 3
    xpad = xpad.to(DEV).to(dtype)
    xr = xpad[:, :K].double()
    labels = torch.randint(0, K, (B,), generator=g).to(DEV)
    dense = _soft_target(B, K, g).to(DEV)
    for form, (dn, lb, s, up) in {'dense': (dense, None, 0.0, 1.0), 'dense_up': (dense * 1.7, None, 0.0, 0.5),
                                  'labels': (None, labels, 0.1, 1.0), 'labels_s0': (None, labels, 0.0, 2.0)}.items():
        ref = _soft_reference(xr, K, dn, lb, s, up, dtype)
        lse, tsum, out, d_g = _soft_run(xpad, ld, B, K, dn, lb, s, up)
        what = f'{form} K={K} B={B}'
        assert_within(lse, ref['lse'], ref['b_lse'], what + ' lse', names=('b',))
        err = abs(float(out[0]) - ref['loss'])
        print(f'{what}: loss {float(out[0])!r} ref {ref["loss"]!r} err {err:.3e} bound {ref["b_loss"]:.3e}')
        assert err <= ref['b_loss'], (what, float(out[0]), ref['loss'], ref['b_loss'])
        assert_within(d_g.view[:, :K], ref['d'], ref['b_d'], what + ' dx', names=('b', 'k'))
        assert bool((d_g.view[:, K:] == 0).all()), what + ': padding columns of dx'
        if lb is not None:
            assert bool((tsum == 1).all())


@pytest.mark.parametrize('geom', LOSS_GEOMS, ids=lambda g: f'{g[0]}x{g[1]}')
def test_criteria_against_the_reference_golden(geom):
    """SoftTargetCrossEntropy and LabelSmoothingCrossEntropy modules (autograd included) against the reference's f32 results"""
    B, K = geom
    pre = f'loss/{B}x{K}/'
    x = _t(pre + 'x').to(DEV).requires_grad_(True)
    target, labels = _t(pre + 'target').to(DEV), _t(pre + 'labels').to(DEV)
    for tag, crit, t, ref in (('soft', M.SoftTargetCrossEntropy(), target, _soft_reference(x.detach().double(), K, target, None, 0.0, 1.0, torch.float32)),
                              ('ls', M.LabelSmoothingCrossEntropy(0.1), labels, _soft_reference(x.detach().double(), K, None, labels, 0.1, 1.0, torch.float32))):
        x.grad = None
        loss = crit(x, t)
        loss.backward()
        torch.cuda.synchronize()
        gl = float(GOLD[pre + tag + '_loss'][0])
        print(f'{tag} {B}x{K}: loss {float(loss)!r} golden {gl!r} bound {2 * ref["b_loss"]:.3e}')
        assert abs(float(loss) - gl) <= 2 * ref['b_loss'], (tag, float(loss), gl)
        assert_within(x.grad, _t(pre + tag + '_dx'), 2 * ref['b_d'], f'{tag} {B}x{K} dx against the golden', names=('b', 'k'))


def test_criteria_take_bf16_logits_and_return_bf16_gradients():
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(6, 1000, generator=g) * 2).to(DEV).bfloat16().requires_grad_(True)
    t = _soft_target(6, 1000, g).to(DEV)
    ref = _soft_reference(x.detach().double(), 1000, t, None, 0.0, 1.0, torch.bfloat16)
    loss = M.SoftTargetCrossEntropy()(x, t)
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == torch.bfloat16
    assert abs(float(loss) - ref['loss']) <= ref['b_loss']
    assert_within(x.grad, ref['d'], ref['b_d'], 'bf16 dx', names=('b', 'k'))


# ---------------------------------------------------------------------------------------------------------------------- EMA --
def _tiny_vit(dom='rgb', num_classes=7):
    ins = {dom: M.PatchedInputAdapter(3 if dom == 'rgb' else 1, 1, VIT['P'], image_size=VIT['S'])}
    outs = {'cls': M.LinearOutputAdapter(num_classes=num_classes, use_mean_pooling=True)}
    return M.MultiViT(ins, outs, num_global_tokens=1, dim_tokens=VIT['D'], depth=VIT['depth'], num_heads=VIT['heads'])


@pytest.mark.parametrize('decay', [0.9, 0.9999])
def test_ema_matches_the_reference_bit_for_bit(decay):
    sd0 = {k[len('ema/sd/'):]: _t(k) for k in GOLD.files if k.startswith('ema/sd/')}
    model = _tiny_vit('depth')
    model.load_state_dict(sd0)
    model = model.to(DEV)
    model.build_arena()
    ema = M.ModelEma(model, decay=decay, shadow=True)
    assert not ema.ema.training and ema.decay == decay
    a = engine.arena_of(ema.ema)
    for step in range(3):
        model.load_state_dict({k: perturbed(v, step) for k, v in sd0.items()})
        ema.update(model)
        torch.cuda.synchronize()
        got = ema.ema.state_dict()
        assert list(got) == list(sd0)
        for k, v in got.items():
            assert torch.equal(_bits(v), _bits(_t(f'ema/{decay}/{step}/{k}'))), (decay, step, k)
        assert torch.equal(a.shadow, a.param.bfloat16()), 'the shadow written by the same launch'
        assert a._shadow_token
    used = torch.zeros(a.numel, dtype=torch.bool, device=DEV)
    for n in a.names:
        used[a.offsets[n]:a.offsets[n] + a.sizes[n]] = True
    assert bool((a.param[~used] == 0).all()), 'the alignment padding stays zero'
    x = torch.randn(4, 1, VIT['S'], VIT['S'], generator=torch.Generator().manual_seed(3)).to(DEV)
    for mode in ('fp32', 'bf16'):
        with engine.precision(mode), torch.no_grad():
            y = ema.ema({'depth': x})['cls']
        assert y.shape == (4, 7) and bool(torch.isfinite(y.float()).all())
    with engine.precision('fp32'), torch.no_grad():
        model.load_state_dict(ema.ema.state_dict())
        assert torch.equal(model({'depth': x})['cls'], ema.ema({'depth': x})['cls'])


def test_ema_update_unaligned_tail_and_no_shadow():
    """ops.ema_update on arrays whose length is no multiple of 4 and whose base is not 16-byte aligned (the element-wise path)"""
    g = torch.Generator().manual_seed(4)
    for n, off in ((1027, 1), (4096, 0), (5, 3)):
        e0, p0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
        eg = Guarded(1, n + off, n + off, torch.float32, DEV, fill=torch.cat([torch.zeros(off), e0])[None])
        sg = Guarded(1, n + off, n + off, torch.bfloat16, DEV, fill=torch.zeros(1, n + off))
        e = eg.view.view(-1)[off:]
        p = torch.cat([torch.zeros(off), p0]).to(DEV)[off:]
        ops.ema_update(e, p, 0.999, sg.view.view(-1)[off:])
        torch.cuda.synchronize()
        eg.intact('ema'), sg.intact('shadow')
        ref = e0.to(DEV) * 0.999 + (1. - 0.999) * p0.to(DEV)
        assert torch.equal(_bits(e), _bits(ref)), (n, off)
        assert torch.equal(sg.view.view(-1)[off:], ref.bfloat16())


# --------------------------------------------------------------------------------------------------------------------- step --
def _layer_id(name, n):
    if name == 'global_tokens' or name.startswith('input_adapters'):
        return 0
    if name.startswith('encoder'):
        return int(name.split('.')[1]) + 1
    return n - 1


def _cls_args():
    return types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, momentum=0.9, mixup=0.8, cutmix=1.0,
                                 cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode='batch', smoothing=0.1, nb_classes=STEP_K)


def _golden_step(mode: str):
    """the fixture's update_freq = 2 step through amd_loop.mixup / cls_criterion / create_optimizer_groups / LossScaler"""
    pre = 'step/sd/'
    model = _tiny_vit('rgb', STEP_K)
    model.load_state_dict({k[len(pre):]: _t(k) for k in GOLD.files if k.startswith(pre)})
    model = model.to(DEV).train()
    model.build_arena()
    args = _cls_args()
    mixup_fn = amd_loop.mixup(args)
    criterion = amd_loop.cls_criterion(args, mixup_fn)
    assert isinstance(mixup_fn, M.Mixup) and isinstance(criterion, M.SoftTargetCrossEntropy)
    L = model.get_num_layers()
    values = [0.75 ** (L + 1 - i) for i in range(L + 2)]
    opt = amd_loop.create_optimizer_groups(args, model, skip_list=model.no_weight_decay(), get_num_layer=lambda nm: _layer_id(nm, L + 2),
                                           get_layer_scale=lambda k: values[k])
    for grp in opt.param_groups:
        grp['lr'] = args.lr * grp.get('lr_scale', 1.0)
    scaler = amd_loop.LossScaler()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    losses = []
    engine.set_direct_grads(True)
    try:
        with engine.precision(mode):
            np.random.seed(77)
            opt.zero_grad()
            for m in range(2):
                x, y = _t(f'step/x{m}').to(DEV), _t(f'step/y{m}').to(DEV)
                xs, ts = mixup_fn(x, y)
                loss = criterion(model({'rgb': xs})['cls'], ts)
                losses.append(loss.detach())
                ret = scaler(loss / 2, opt, clip_grad=None, parameters=model.parameters(), update_grad=(m == 1))
                assert (ret is None) == (m == 0)
            torch.cuda.synchronize()
    finally:
        engine.set_direct_grads(False)
    return model, opt, before, [float(l) for l in losses]


def test_update_freq_2_step_matches_the_reference_in_fp32():
    """loss within 1e-5 relative, accumulated gradients rel <= 1e-4, parameter update within 5 % + 1e-7 per tensor: the tolerances of
    tests/test_convnext_head_gpu.py's golden step"""
    model, opt, before, losses = _golden_step('fp32')
    for m in range(2):
        gl = float(GOLD[f'step/loss{m}'][0])
        print(f'micro-step {m}: loss {losses[m]!r} golden {gl!r}')
        assert abs(losses[m] - gl) <= 1e-5 * abs(gl), (m, losses[m], gl)
    for n, p in model.named_parameters():
        if f'step/grad/{n}' in GOLD.files:
            r = rel_err(p.grad, _t(f'step/grad/{n}'))
            assert r <= 1e-4, (n, r)
    assert opt.step_count == 1
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        d_e = (p.detach() - before[n]).double().cpu()
        d_g = _t(f'step/param/{n}').double() - before[n].double().cpu()
        assert float((d_e - d_g).norm()) <= 0.05 * float(d_g.norm()) + 1e-7, n


def test_update_freq_2_step_runs_in_bf16():
    model, opt, before, losses = _golden_step('bf16')
    assert all(math.isfinite(l) for l in losses) and opt.step_count == 1
    moved = 0
    for n, p in model.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        moved += int(p.requires_grad and not torch.equal(p, before[n]))
    assert moved > 0


# -------------------------------------------------------------------------------------------------------------------- graph --
def test_mixup_and_criterion_inside_a_step_graph():
    """Mixup + SoftTargetCrossEntropy (forward and gradient) captured in graph.StepGraph: the per-sample block is a host input that
    is redrawn before every replay, so two replays under one seed give the two mixed batches of two eager calls, bit for bit."""
    from multimae_amd.graph import StepGraph
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(6, 3, 16, 20, generator=g).to(DEV)
    labels = torch.randint(0, 7, (6,), generator=g).to(DEV)
    logits = (torch.randn(6, 7, generator=g) * 2).to(DEV).requires_grad_(True)
    mix, crit = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode='elem', num_classes=7), M.SoftTargetCrossEntropy()
    work = x0.clone()

    def step():
        work.copy_(x0)
        xm, t = mix(work, labels)
        loss = crit(logits, t)
        (d,) = torch.autograd.grad(loss, logits)
        return xm, t, loss, d

    np.random.seed(21)
    eager = []
    for _ in range(3):
        eager.append([v.detach().clone() for v in step()])
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0])
    run = StepGraph(step)
    np.random.seed(21)
    for k in range(3):
        out = run()
        torch.cuda.synchronize()
        for a, b in zip(out, eager[k]):
            assert torch.equal(_bits(a), _bits(b)), k
    assert run.replays == 3 and run.n_host_inputs == 1
