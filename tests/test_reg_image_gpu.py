"""GPU: the masked L1 / MSE / berHu losses and the NYU depth metrics on a prediction that is the image itself -- the DPT head's
contiguous f32 NCHW output -- (csrc/regloss.hip: mmae_reg_img_fwd / mmae_reg_img_bwd / mmae_depth_metrics_img) and their host side
(criterion.masked_*_loss through functions.RegImageLossFn, metrics.depth_metrics / DepthMetric).  Kernels element by element against
fp64 torch with bounds derived from the unit roundoff, every kernel output in a Guarded buffer; against the reference's recorded
losses and metric values (tests/golden/reg_loss.npz); the DPT head + loss step fused against eager in one process; a whole step under
torch's synchronisation check.

Bounds: those of tests/test_reg_loss_gpu.py's module docstring with the interpolated value replaced by the prediction itself, so
e_z = 0, e_w = 0 and a window of one term (u = 2^-24, gamma_n as helpers.gamma, N the number of elements, n_v the valid ones).
  d      pred - t, one rounding: bit-equal to torch's f32 where(valid, pred - t, 0); against fp64 e_d = u |d|; a masked element is 0.
  count  exact (integers below 2^24).   max|d|: bit-equal to the f32 max of |diff|; against fp64 b_max = max e_d.
  c      max(0.2f max|d|, 1e-5f): the constant and the product round once each: b_c = 0.2 b_max + 2 u c.
  L1     sum |d| in any order: (sum e_d + gamma_(N + 16) sum |d|) / n_v, the division and its rounding: + 2 u |loss|.
  MSE    a term d^2 moves by 2 |d| e_d + e_d^2 and rounds once (u d^2); then as L1.
  berHu  f(d, c) = |d| below c, (d^2 + c^2) / (2 c) from c on, is C^1 in (d, c); along the segment from the exact to the computed
         (d, c) a term moves by at most G_d e_d + G_c b_c with G_d = max(1, (|d| + e_d) / (c - b_c)),
         G_c = max(0, ((|d| + e_d)^2 / (c - b_c)^2 - 1) / 2); the outer branch rounds at most four times: gamma_4 f.  Then as L1.
  dpred  element e = scale g(d), scale = up / count.  g moves by
           L1     2 where a valid element has |d| <= e_d (here only d = 0), else 0
           MSE    2 e_d
           berHu  the L1 term, and where the element can lie in the outer branch (|d| + e_d >= c - b_c):
                  e_d / (c - b_c) + (|d| + e_d) b_c / (c - b_c)^2 + u |d| / (c - b_c)
         scale (dg + (u + gamma_1) |g|); the scale is formed with two roundings and applied with one: + 4 u |dpred| + ulp(dpred).
  metrics  p = z std + mean, t' = t std + mean (std, mean as the f32 the kernel receives; a product and a sum each):
         e_p = 2 u |p|, e_t = 2 u |t'|;  a clamped value max(v, 1e-6) moves by the same, or by u 1e-6 when v + e < 1e-6;
         diff = |p - t'|: e_f = e_p + e_t + u diff.  Terms: diff^2: 2 diff e_f + e_f^2 + u diff^2;  a quotient a / b:
         (e_a + (a / b) e_b) / (b - e_b) + u a / b;  logf within 1 ulp, so log pc - log tc moves by
         e_pc / (pc - e_pc) + e_tc / (tc - e_tc) + 2 u (|log pc| + |log tc|) + u |lg| = e_l, its square by 2 |lg| e_l + e_l^2 + u lg^2.
         Sums in any order: sum of the terms' bounds + gamma_(N + 16) sum |term|, the mean 2 u; a root: |sqrt a - sqrt b| <= |a - b| / sqrt b.
         A delta count can differ by the elements whose ratio lies within its own bound of the threshold: n_amb / n_v + 2 u.
         Against the fixture (the reference's f32 evaluation on the CPU, with the same roundings) the bound is taken twice; the delta
         counts themselves must be equal.
  acc    three additions of the same f32 [7] into zeros: within 4 ulp of three times the output.

Shapes (B, K, H, W): fewer elements than a wave; an odd plane of 221 elements (no 16-byte alignment between planes: the scalar
path); 16 channels; the 16-byte path over several workgroups; another odd plane over 38 workgroups; and a contiguous view that
starts one element into a larger buffer (a misaligned base pointer: the scalar path on a plane that is a multiple of four)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import engine, metrics, ops
from dropin import amd_loop
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dpt_fixture as DF  # noqa: E402
from dpt_fixture import CASES, UNUSED  # noqa: E402

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'reg_loss.npz'))
U = 2.0 ** -24
KINDS = ('l1', 'mse', 'berhu')
KEYS = metrics.DEPTH_METRIC_KEYS
# (B, K, H, W, elements the prediction's base pointer is shifted off its 16-byte boundary)
SHAPES = [(2, 1, 5, 7, 0), (2, 3, 13, 17, 0), (1, 16, 9, 33, 0), (2, 1, 48, 80, 0), (3, 3, 37, 29, 0), (2, 1, 5, 8, 1)]
IDS = ['x'.join(str(v) for v in s[:4]) + ('_shifted' if s[4] else '') for s in SHAPES]
MEAN32, STD32 = float(np.float32(metrics.NYU_MEAN)), float(np.float32(metrics.NYU_STD))


# ------------------------------------------------------------------------------------------------------ helpers --
def _image(B, K, H, W, shift, seed, scale=2.0):
    """a contiguous f32 [B, K, H, W] prediction on the device; with shift, a view that starts `shift` elements into a larger buffer"""
    g = torch.Generator().manual_seed(seed)
    n = B * K * H * W
    buf = torch.zeros(n + shift, device=DEV)
    y = buf[shift:].view(B, K, H, W)
    y.copy_(torch.randn(B, K, H, W, generator=g) * scale)
    assert y.is_contiguous() and (y.data_ptr() % 16 != 0) == bool(shift)
    return y


def _masks(B, K, H, W, seed):
    """the mask patterns of tests/test_reg_loss_gpu.py: name -> torch.bool [B, Cm, H, W] or None; with K > 1 both Cm = 1 and Cm = K"""
    g = torch.Generator().manual_seed(seed)
    out = {'none': None}
    for Cm in sorted({1, K}):
        block = torch.ones(B, Cm, H, W, dtype=torch.bool)
        block[:, :, H // 4:H // 2 + 1, 1:W // 2] = False
        image = torch.ones(B, Cm, H, W, dtype=torch.bool)
        image[B - 1] = False
        single = torch.zeros(B, Cm, H, W, dtype=torch.bool)
        single[B - 1, Cm - 1, H // 2, W - 2] = True
        out.update({f'all{Cm}': torch.ones(B, Cm, H, W, dtype=torch.bool), f'block{Cm}': block, f'image{Cm}': image,
                    f'random{Cm}': torch.rand(B, Cm, H, W, generator=g) < 0.6, f'empty{Cm}': torch.zeros(B, Cm, H, W, dtype=torch.bool),
                    f'single{Cm}': single})
    return out


def _berhu(d, c):
    a = d.abs()
    return torch.where(a < c, a, (d * d + c * c) / 2 / c)


def _reference(kind, pred, target, mask, up=1.0):
    """fp64 restatement on the image, with the module docstring's bounds; pred, target on the device, mask anywhere or None"""
    p, t = pred.detach().double(), target.to(DEV).double()
    valid = torch.ones_like(t, dtype=torch.bool) if mask is None else mask.to(DEV).expand(p.shape)
    n_v, N = int(valid.sum()), t.numel()
    d = torch.where(valid, p - t, torch.zeros_like(t))
    e_d = U * d.abs()
    a = d.abs()
    mx, b_max = float(a.max()), float(e_d.max())
    c = max(0.2 * mx, 1e-5)
    b_c = 0.2 * b_max + 2 * U * c
    cl = c - b_c
    out = dict(d=d, e_d=e_d, n_v=n_v, max=mx, b_max=b_max, c=c, b_c=b_c)
    amb = valid & (a <= e_d)
    if kind == 'l1':
        f, e_f, g = a, e_d, torch.sign(d)
        dg = 2.0 * amb
    elif kind == 'mse':
        f, e_f, g = d * d, 2 * a * e_d + e_d ** 2 + U * d ** 2, 2 * d
        dg = 2 * e_d
    else:
        f = _berhu(d, c)
        G_d = ((a + e_d) / cl).clamp_min(1.0)
        G_c = ((((a + e_d) / cl) ** 2 - 1) / 2).clamp_min(0.0)
        e_f = torch.where(valid, G_d * e_d + G_c * b_c + gamma(4) * f, torch.zeros_like(d))
        g = torch.where(a < c, torch.sign(d), d / c)
        outer = (a + e_d) >= cl
        dg = 2.0 * amb + torch.where(outer, e_d / cl + (a + e_d) * b_c / cl ** 2 + U * a / cl, torch.zeros_like(d))
    if n_v == 0:
        out.update(loss=0.0, b_loss=0.0, dx=torch.zeros_like(d), b_dx=torch.zeros_like(d))
        return out
    loss = float(f.sum()) / n_v
    b_loss = (float(e_f.sum()) + gamma(N + 16) * float(f.abs().sum())) / n_v + 2 * U * abs(loss)
    scale = abs(up) / n_v
    dx = (up / n_v) * g
    b_dx = scale * (dg + (U + gamma(1)) * g.abs())
    out.update(loss=loss, b_loss=b_loss, dx=dx, b_dx=b_dx + 4 * U * dx.abs() + ulp(torch.float32, dx))
    return out


def _run(kind, pred, target, mask, up=1.0, partial=None):
    """forward + backward through ops.* with every output in a Guarded buffer -> (diff, out [4], dpred), same shapes as pred"""
    B, K, H, W = pred.shape
    tg = target.to(DEV).contiguous()
    mk = None if mask is None else mask.to(DEV).contiguous()
    diff_g = Guarded(B * K, H * W, H * W, torch.float32, DEV)
    out_g = Guarded(1, 4, 4, torch.float32, DEV)
    diff, out = ops.reg_img_fwd(pred, tg, mk, kind, diff=diff_g.view.view(B, K, H, W), out=out_g.view.view(4), partial=partial)
    d_g = Guarded(B * K, H * W, H * W, torch.float32, DEV)
    dpred = ops.reg_img_bwd(diff, out, torch.tensor([up], device=DEV), kind, dpred=d_g.view.view(B, K, H, W))
    torch.cuda.synchronize()
    diff_g.intact('reg_img_fwd diff')
    out_g.intact('reg_img_fwd out')
    d_g.intact('reg_img_bwd dpred')
    return diff, out, dpred


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ kernels --
@pytest.mark.parametrize('B,K,H,W,shift', SHAPES, ids=IDS)
def test_loss_and_gradient_against_fp64(B, K, H, W, shift):
    """diff (bit for bit), count, max |d| (bit for bit), c, the loss and dpred per element for every kind and mask pattern, the guard
    zones intact (_run); with nothing valid the loss is 0 and the gradient all zero (the reference: NaN)"""
    pred = _image(B, K, H, W, shift, seed=20 + K)
    target = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(30 + K))
    for name, mask in _masks(B, K, H, W, seed=40).items():
        valid = torch.ones(B, K, H, W, dtype=torch.bool, device=DEV) if mask is None else mask.to(DEV).expand(B, K, H, W)
        diff32 = torch.where(valid, pred - target.to(DEV), torch.zeros((), device=DEV))
        for kind in KINDS:
            ref = _reference(kind, pred, target, mask, up=1.7)
            diff, out, d = _run(kind, pred, target, mask, up=1.7)
            what = f'{kind} {name} {(B, K, H, W)} shift {shift}'
            loss, cnt, mx, c = (float(v) for v in out)
            print(what, 'loss', loss, 'ref', ref['loss'], 'bound', ref['b_loss'], 'c', c, 'ref', ref['c'], 'bound', ref['b_c'],
                  'max |dpred - ref|', float((d.double() - ref['dx']).abs().max()))
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all()), what
            assert torch.equal(_bits(diff), _bits(diff32)), (what, int((diff != diff32).sum()))
            assert not diff[~valid].any() and not d[~valid].any(), what           # exactly 0 where the mask is false
            assert cnt == ref['n_v'], what
            assert torch.equal(_bits(out[2:3]), _bits(diff32.abs().max().reshape(1))), what
            assert abs(mx - ref['max']) <= ref['b_max'] + float(ulp(torch.float32, ref['max'])), what
            assert abs(c - ref['c']) <= ref['b_c'] + float(ulp(torch.float32, ref['c'])), what
            if name.startswith('empty') or ref['n_v'] == 0:
                assert loss == 0.0 and not d.any() and c == float(np.float32(1e-5)), what
                continue
            assert abs(loss - ref['loss']) <= ref['b_loss'] + float(ulp(torch.float32, ref['loss'])), what
            assert_within(d, ref['dx'], ref['b_dx'], 'dpred ' + what, names=('b', 'k', 'y', 'x'))


def test_several_workgroups_write_their_partials():
    """the number of partial rows the forward writes is the number of its workgroups: more than two on both paths"""
    for (B, K, H, W, shift), want in ((SHAPES[3], 8), (SHAPES[4], 38)):
        pred = _image(B, K, H, W, shift, seed=5)
        target = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(6))
        part_g = Guarded(1, 4 * ops.REG_PARTIALS, 4 * ops.REG_PARTIALS, torch.float32, DEV)
        partial = part_g.view.view(-1)
        partial.fill_(float('nan'))
        _, out, _ = _run('l1', pred, target, None, partial=partial)
        part_g.intact('reg_img_fwd partial')
        rows = int((~partial.view(-1, 4).isnan().any(dim=1)).sum())
        assert rows == want and rows > 2 and float(out[1]) == B * K * H * W, (rows, want)


def test_nan_and_inf_under_a_false_mask_reach_nothing():
    for B, K, H, W, shift in (SHAPES[1], SHAPES[3]):
        pred = _image(B, K, H, W, shift, seed=7)
        target = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(8)).to(DEV)
        for Cm in sorted({1, K}):
            mask = (torch.rand(B, Cm, H, W, generator=torch.Generator().manual_seed(9)) < 0.6).to(DEV)
            valid = mask.expand(B, K, H, W)
            bad_p, bad_t = pred.clone(), target.clone()
            bad_p[~valid] = float('inf')
            bad_p[~valid & (torch.arange(pred.numel(), device=DEV).view(pred.shape) % 2 == 0)] = float('-inf')
            bad_t[~valid] = float('nan')
            for kind in KINDS:
                clean = _run(kind, pred, target, mask, up=0.9)
                dirty = _run(kind, bad_p, bad_t, mask, up=0.9)
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(clean, dirty)), (kind, Cm)
                diff, out, d = dirty
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all()) and not d[~valid].any() and not diff[~valid].any()
            if K == 1:
                m_clean = ops.depth_metrics_img(pred, target, mask, metrics.NYU_MEAN, metrics.NYU_STD).clone()
                m_dirty = ops.depth_metrics_img(bad_p, bad_t, mask, metrics.NYU_MEAN, metrics.NYU_STD)
                assert torch.equal(_bits(m_clean), _bits(m_dirty)) and bool(torch.isfinite(m_dirty).all())


def test_prediction_equal_to_the_target():
    """pred == target: every kind gives loss 0 and an all-zero gradient (sign(0) = 0), berHu's c is its floor 1e-5"""
    B, K, H, W, shift = SHAPES[1]
    pred = _image(B, K, H, W, shift, seed=50)
    for kind in KINDS:
        diff, out, d = _run(kind, pred, pred.clone(), None)
        assert not diff.any() and not d.any() and float(out[0]) == 0.0 and float(out[1]) == B * K * H * W and float(out[2]) == 0.0
        assert float(out[3]) == float(np.float32(1e-5))


@pytest.mark.parametrize('B,K,H,W,shift', [SHAPES[3], SHAPES[4]], ids=[IDS[3], IDS[4]])
def test_two_runs_are_bit_equal(B, K, H, W, shift):
    pred = _image(B, K, H, W, shift, seed=60, scale=3.0)
    target = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(61))
    mask = _masks(B, K, H, W, seed=62)['random1']
    for kind in KINDS:
        runs = [_run(kind, pred, target, mask, up=0.3) for _ in range(2)]
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs)), kind
    p1, t1, m = pred[:, :1].contiguous(), target[:, :1].contiguous().to(DEV), mask.to(DEV).contiguous()
    outs = [ops.depth_metrics_img(p1, t1, m, 0.5, 2.0).clone() for _ in range(2)]
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


# ------------------------------------------------------------------------------------------------------ metrics --
def _metrics_ref(z, target, valid):
    """fp64 values [7] and their bounds [7] (module docstring) from the prediction z, the target and the valid mask"""
    z, target = z.double(), target.double()
    p, t = z * STD32 + MEAN32, target * STD32 + MEAN32
    e_p, e_t = 2 * U * p.abs(), 2 * U * t.abs()
    clampb = lambda v, e: torch.where(v + e < 1e-6, torch.full_like(v, U * 1e-6), e)
    pc, tc, e_pc, e_tc = p.clamp_min(1e-6), t.clamp_min(1e-6), clampb(p, e_p), clampb(t, e_t)
    df = (p - t).abs()
    e_f = e_p + e_t + U * df
    quot = lambda a, e_a, b, e_b: (e_a + (a / b) * e_b) / (b - e_b) + U * a / b
    sq, e_sq = df * df, 2 * df * e_f + e_f ** 2 + U * df * df
    lg = pc.log() - tc.log()
    e_l = e_pc / (pc - e_pc) + e_tc / (tc - e_tc) + 2 * U * (pc.log().abs() + tc.log().abs()) + U * lg.abs()
    terms = [(sq, e_sq), (df / tc, quot(df, e_f, tc, e_tc)), (sq / tc, quot(sq, e_sq, tc, e_tc)), (lg * lg, 2 * lg.abs() * e_l + e_l ** 2 + U * lg * lg)]
    n_v, N = int(valid.sum()), valid.numel()
    vals, bounds = [], []
    for v, e in terms:
        s, b = float((v * valid).sum()) / n_v, (float((e * valid).sum()) + gamma(N + 16) * float((v * valid).sum())) / n_v
        vals.append(s)
        bounds.append(b + 2 * U * s)
    for i in (0, 3):                                                          # rmse, log10: the root
        s, b = vals[i], bounds[i]
        vals[i], bounds[i] = math.sqrt(s), b / math.sqrt(s) + 2 * U * math.sqrt(s)
    r = torch.maximum(p / tc, t / pc)
    e_r = torch.maximum(quot(p.abs(), e_p, tc, e_tc), quot(t.abs(), e_t, pc, e_pc))
    for th in (1.25, 1.25 ** 2, 1.25 ** 3):
        vals.append(float(((r < th) & valid).sum()) / n_v)
        bounds.append(float((((r - th).abs() <= e_r) & valid).sum()) / n_v + 2 * U)
    return vals, bounds


def _metric_inputs(B, H, W, seed, clamp):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(B, 1, H, W, generator=g) * 3.6 - 1.8
    if clamp:
        target.view(-1)[::9] = -2.9                                            # target std + mean < 0: clamped to 1e-6
    mask = torch.rand(B, 1, H, W, generator=g) < 0.6
    return target, mask


@pytest.mark.parametrize('B,K,H,W,shift', SHAPES, ids=IDS)
def test_depth_metrics_against_fp64_and_acc_accumulates(B, K, H, W, shift):
    """the shapes' (B, H, W) with one channel: the seven values within the docstring's bounds, NaN for an empty mask, and acc after
    three calls within 4 ulp of three times the output with acc[7] == 3"""
    pred = _image(B, 1, H, W, shift, seed=70, scale=0.9)
    for clamp in (False, True):
        target, mask = _metric_inputs(B, H, W, 71, clamp)
        tg = target.to(DEV)
        for mk in (None, mask):
            valid = torch.ones(B, 1, H, W, dtype=torch.bool, device=DEV) if mk is None else mk.to(DEV)
            vals, bounds = _metrics_ref(pred, tg, valid)
            out_g, acc_g = Guarded(1, 7, 8, torch.float32, DEV), Guarded(1, 8, 8, torch.float32, DEV)
            part_g = Guarded(1, 8 * ops.REG_PARTIALS, 8 * ops.REG_PARTIALS, torch.float32, DEV)
            acc = acc_g.view.view(8)
            acc.zero_()
            args = (pred, tg, None if mk is None else mk.to(DEV).contiguous(), metrics.NYU_MEAN, metrics.NYU_STD)
            out = ops.depth_metrics_img(*args, acc=acc, out=out_g.view.view(7), partial=part_g.view.view(-1))
            first = acc.clone()
            ops.depth_metrics_img(*args, acc=acc)
            ops.depth_metrics_img(*args, acc=acc)
            torch.cuda.synchronize()
            out_g.intact('depth_metrics_img out')
            acc_g.intact('depth_metrics_img acc')
            part_g.intact('depth_metrics_img partial')
            for k, got, v, b in zip(KEYS, out.tolist(), vals, bounds):
                print((B, H, W), shift, 'clamp' if clamp else '', 'mask' if mk is not None else '', k, got, v, b)
                assert abs(got - v) <= b + float(ulp(torch.float32, v)), (k, got, v, b)
            assert torch.equal(first[:7], out) and float(first[7]) == 1.0
            three = 3.0 * out.double()
            assert bool(((acc[:7].double() - three).abs() <= 4 * ulp(torch.float32, three)).all()) and float(acc[7]) == 3.0
    empty = torch.zeros(B, 1, H, W, dtype=torch.bool, device=DEV)
    acc = torch.zeros(8, device=DEV)
    out = ops.depth_metrics_img(pred, tg, empty, metrics.NYU_MEAN, metrics.NYU_STD, acc=acc)
    assert bool(out.isnan().all()) and bool(acc[:7].isnan().all()) and float(acc[7]) == 1.0


# ------------------------------------------------------------------------------- the reference's recorded values --
@pytest.mark.parametrize('K,c', [(1, 1), (3, 1), (3, 3)])
def test_losses_against_the_references_values(K, c):
    """the fixture's full-resolution image with its targets and masks: each loss within twice its bound of the loss the reference's
    own masked_*_loss recorded; an empty mask gives 0 here where the reference recorded NaN (the documented deviation)"""
    pre = f'loss/K{K}/'
    pred, target = torch.from_numpy(GOLD[pre + 'pred']).to(DEV), torch.from_numpy(GOLD[pre + 'target']).to(DEV)
    names = sorted({k.split('/')[4] for k in GOLD.files if k.startswith(f'{pre}l1/c{c}/')})
    assert set(names) >= {'all', 'block', 'image', 'random', 'empty'}
    for kind in KINDS:
        for name in names:
            mask = None if name == 'none' else torch.from_numpy(GOLD[f'{pre}mask/c{c}/{name}'])
            gold = float(GOLD[f'{pre}{kind}/c{c}/{name}/loss'][0])
            _, out, _ = _run(kind, pred, target, mask)
            got = float(out[0])
            if name == 'empty':
                assert np.isnan(gold) and got == 0.0
                continue
            ref = _reference(kind, pred, target, mask)
            b = ref['b_loss'] + float(ulp(torch.float32, ref['loss']))
            print(kind, K, c, name, got, 'golden', gold, 'fp64', ref['loss'], 'bound', b)
            assert abs(got - ref['loss']) <= b and abs(got - gold) <= 2 * b, (kind, name, got, gold, b)


@pytest.mark.parametrize('case', ['none', 'block', 'image', 'random', 'clamp'])
def test_depth_metrics_against_the_references_values(case):
    pre = f'metric/{case}/'
    pred, target = torch.from_numpy(GOLD[pre + 'pred']).to(DEV), torch.from_numpy(GOLD[pre + 'target']).to(DEV)
    mask = torch.from_numpy(GOLD[pre + 'mask']).to(DEV) if pre + 'mask' in GOLD.files else None
    out = ops.depth_metrics_img(pred, target, mask, metrics.NYU_MEAN, metrics.NYU_STD)
    valid = torch.ones_like(pred, dtype=torch.bool) if mask is None else mask
    n_v = int(valid.sum())
    vals, bounds = _metrics_ref(pred, target, valid)
    for i, (k, got, gold, v, b) in enumerate(zip(KEYS, out.tolist(), GOLD[pre + 'values'].tolist(), vals, bounds)):
        print(case, k, got, 'golden', gold, 'fp64', v, 'bound', b)
        assert abs(got - v) <= b + float(ulp(torch.float32, v)), (k, got, v, b)
        assert abs(got - gold) <= 2 * (b + float(ulp(torch.float32, v))), (k, got, gold, b)
        if i >= 4:                                                             # the delta counts themselves are equal
            assert round(got * n_v) == round(gold * n_v), (k, got, gold, n_v)


# ---------------------------------------------------------------------------------------------- DPT head + loss --
def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


_HEADS = {}


def _head(case):
    """(head on the device, tokens, info, target, mask) of a fixture case, built once"""
    if case not in _HEADS:
        K, tasks, D, (NH, NW) = CASES[case]
        g = torch.Generator().manual_seed(11)
        shape = (DF.B, K, 16 * NH, 16 * NW)
        _HEADS[case] = (DF.seeded_head(case).to(DEV), [t.to(DEV) for t in DF.tokens(case)], DF.case_info(case),
                        (torch.randn(shape, generator=g) * 0.5).to(DEV), (torch.rand(DF.B, 1, *shape[2:], generator=g) < 0.7).to(DEV))
    return _HEADS[case]


def _step(case, kind, fused):
    head, toks, info, target, mask = _head(case)
    head.zero_grad(set_to_none=True)
    toks = [t.clone().requires_grad_(True) for t in toks]
    y = head(toks, info)
    assert type(y) is torch.Tensor and y._mmae_img.matches(y) and y.float() is y
    fn = {'l1': amd_loop.taskonomy_criterion(['depth'])['depth'], 'mse': M.masked_mse_loss, 'berhu': amd_loop.depth_criterion('berhu')['depth']}[kind]
    loss = fn(y.float() if fused else y * 1, target, mask)                   # y * 1, a derived tensor: the eager path
    assert (type(loss.grad_fn).__name__ == 'RegImageLossFnBackward') == fused
    loss.backward()
    engine.join_wgrad_streams()
    torch.cuda.synchronize()
    grads = {f'tok{i}': t.grad.clone() for i, t in enumerate(toks)}
    grads.update({n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None})
    assert set(n for n, _ in head.named_parameters()) - set(grads) == set(UNUSED)
    return loss.detach(), y.detach(), grads


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', list(CASES))
def test_fused_path_against_the_eager_path_in_one_process(case, kind):
    """One training step of the DPT head both ways in fp32 mode, r1 (K = 1) and r3 (K = 3).  The two paths share the head's forward,
    so they hold bit-identical images; each loss is within the module docstring's bound of the fp64 value on that image (the eager
    sum is an f32 sum of the same terms in another order), so they agree within twice that bound.  Every token and parameter gradient
    agrees within the 1e-4 relative norm test_reg_loss_gpu holds the ConvNeXt head's two paths to."""
    with engine.precision('fp32'):
        loss_e, y_e, g_e = _step(case, kind, fused=False)
        loss_f, y, g_f = _step(case, kind, fused=True)
    assert torch.equal(_bits(y), _bits(y_e))
    _, _, _, target, mask = _head(case)
    r = _reference(kind, y, target, mask)
    b = r['b_loss'] + float(ulp(torch.float32, r['loss']))
    print(case, kind, 'loss eager', float(loss_e), 'fused', float(loss_f), 'fp64 on the image', r['loss'], 'bound', b)
    assert abs(float(loss_f) - r['loss']) <= b and abs(float(loss_f) - float(loss_e)) <= 2 * b
    assert set(g_f) == set(g_e)
    for n in g_f:
        print(f'  {n}: fused against eager {_rel(g_f[n], g_e[n]):.3e}')
        assert _rel(g_f[n], g_e[n]) <= 1e-4, n


def test_bf16_step_gives_finite_results():
    with engine.precision('bf16'):
        loss, y, grads = _step('r1', 'berhu', fused=True)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert float(loss) > 0 and any(bool(g.any()) for g in grads.values())


def test_head_loss_and_metrics_never_synchronise():
    """DPT head + berHu + metrics + backward run with torch's synchronisation check set to 'error': nothing in the loss or the metrics
    reads a device value back.  Three batches through the same static tensors give three different, finite results, and DepthMetric
    has accumulated all three inside the kernel."""
    head, toks0, info, t0, m0 = _head('r1')
    params = [p for n, p in head.named_parameters() if n not in UNUSED]
    xs = [t.clone().requires_grad_(True) for t in toks0]
    ts, ms = t0.clone(), m0.clone()
    dm = M.DepthMetric(device=DEV)

    def step():
        y = head(xs, info)
        loss = M.masked_berhu_loss(y.float(), ts, ms)
        assert type(loss.grad_fn).__name__ == 'RegImageLossFnBackward'
        vals = torch.stack(list(M.depth_metrics(y, ts, ms).values()))
        dm.update(y, ts, ms)
        grads = torch.autograd.grad(loss, xs + params)
        return [loss.detach(), vals] + [g.detach() for g in grads]

    g = torch.Generator().manual_seed(9)
    batches = [(toks0, t0, m0)] + [([torch.randn(t.shape, generator=g).to(DEV) for t in toks0], (torch.randn(t0.shape, generator=g) * 0.5).to(DEV),
                                    (torch.rand(m0.shape, generator=g) < 0.7).to(DEV)) for _ in range(2)]
    outs = []
    with engine.precision('fp32'):
        for xb, tb, mb in batches:
            with torch.no_grad():
                for x, v in zip(xs, xb):
                    x.copy_(v)
                ts.copy_(tb), ms.copy_(mb)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode('error')
            try:
                out = step()
            finally:
                torch.cuda.set_sync_debug_mode('default')
            outs.append([v.clone() for v in out])
    engine.join_wgrad_streams()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for o in outs for v in o)
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[1][0], outs[2][0]) and not torch.equal(outs[0][0], outs[2][0])
    assert float(dm.acc[7]) == 3.0
    total = sum(o[1].double() for o in outs)
    assert bool(((dm.acc[:7].double() - total).abs() <= 4 * ulp(torch.float32, total)).all())
