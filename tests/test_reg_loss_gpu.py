"""GPU: the fused resize + masked L1 / MSE / berHu losses and the NYU depth metrics of csrc/regloss.hip, and their host side
(criterion.masked_*_loss, metrics.depth_metrics / DepthMetric).  Kernels element by element against fp64 torch (F.interpolate + the
formulas + autograd) with bounds derived from the unit roundoff, outputs in Guarded buffers, the map's padding columns poisoned with
NaN; the interpolation bit for bit against the image mmae_resize_fwd writes; the head + loss step against the reference's recorded
step; the fused path against the eager path in one process; a whole step under torch's synchronisation check.

Bounds (u = 2^-24, gamma_n as helpers.gamma, N the number of elements, n_v the number of valid ones).
  z      interpolated value.  Bilinear: test_resize_fwd's bound e_z = (8 u (max(h, w) + 2) + 8 u) max|x| + ulp(z); nearest: 0 (a copy).
  d      z - t, one rounding: e_d = e_z + u |d| on a valid element; a masked element is exactly 0.
  count  exact (integers below 2^24).   max|d|: max is 1-Lipschitz: b_max = max e_d.
  c      max(0.2f max|d|, 1e-5f): the constant and the product round once each: b_c = 0.2 b_max + 2 u c.
  L1     sum |d| in any order: (sum e_d + gamma_(N + 16) sum |d|) / n_v, the division and its rounding: + 2 u |loss|.
  MSE    a term d^2 moves by 2 |d| e_d + e_d^2 and rounds once (u d^2); then as L1.
  berHu  f(d, c) = |d| below c, (d^2 + c^2) / (2 c) from c on, is C^1 in (d, c): df/dd = sign(d) or d / c, df/dc = 0 or
         (c^2 - d^2) / (2 c^2).  By the mean value theorem along the segment from the exact to the computed (d, c), a term moves by at
         most G_d e_d + G_c b_c with the suprema over the segment G_d = max(1, (|d| + e_d) / (c - b_c)),
         G_c = max(0, ((|d| + e_d)^2 / (c - b_c)^2 - 1) / 2) -- an element that changes branch is covered, the derivatives being
         continuous across |d| = c.  Evaluating the outer branch rounds at most four times on non-negative terms: gamma_4 f.  Then as L1.
  dx     element (iy, ix, k) = scale sum_window weight g(d), scale = up / count, at most n = (2 ceil(H / h) + 3)(2 ceil(W / w) + 3)
         terms (test_resize_bwd_gather's count), a weight within e_w = 8 u (max(h, w) + 2) (0 for nearest).  g moves by
           L1     2 where |d| <= e_d (the sign may come out as any of -1, 0, 1), else 0
           MSE    2 e_d
           berHu  the L1 term, and where the element can lie in the outer branch (|d| + e_d >= c - b_c), where g is Lipschitz in d with
                  1 / (c - b_c) and in c with (|d| + e_d) / (c - b_c)^2:  e_d / (c - b_c) + (|d| + e_d) b_c / (c - b_c)^2 + u |d| / (c - b_c)
         With W(v) the interpolation's exact backward applied to v:  scale (W(dg) + (u + gamma_n) W(|g|) + n e_w max|g|); scale is formed
         with two roundings and applied with one: + 4 u |dx| + ulp(dx).
  metrics  p = z std + mean, t' = t std + mean (std, mean as the f32 the kernel receives; a product and a sum each):
         e_p = std e_z + 2 u |p|, e_t = 2 u |t'|;  a clamped value max(v, 1e-6) moves by the same, or by u 1e-6 when v + e < 1e-6 (the
         constant on both sides);  diff = |p - t'|: e_f = e_p + e_t + u diff.  Terms: diff^2: 2 diff e_f + e_f^2 + u diff^2;  a quotient
         a / b: (e_a + (a / b) e_b) / (b - e_b) + u a / b;  logf within 1 ulp (2 u relative), so log pc - log tc moves by
         e_pc / (pc - e_pc) + e_tc / (tc - e_tc) + 2 u (|log pc| + |log tc|) + u |lg| = e_l, its square by 2 |lg| e_l + e_l^2 + u lg^2.
         Sums in any order: sum of the terms' bounds + gamma_(N + 16) sum |term|, the mean 2 u; a root: |sqrt a - sqrt b| <= |a - b| / sqrt b.
         A delta count can differ by the elements whose ratio lies within its own bound of the threshold: n_amb / n_v + 2 u.
         Against the fixture (the reference's f32 evaluation on the CPU, with the same roundings) the bound is taken twice."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multimae_amd as M
from multimae_amd import metrics, ops, output_adapters as OA
from dropin import amd_loop
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_convnext import input_info  # noqa: E402
from make_golden_reg_loss import HEAD  # noqa: E402

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'reg_loss.npz'))
U = 2.0 ** -24
KINDS = ('l1', 'mse', 'berhu')
KEYS = metrics.DEPTH_METRIC_KEYS
# (h, w) -> (H, W): upsampling by 2, by a non-integer factor, the identity, and W > 64 with several workgroups
SHAPES = [((5, 7), (10, 14)), ((5, 7), (13, 17)), ((5, 7), (5, 7)), ((24, 40), (48, 80))]
B = 2


# ------------------------------------------------------------------------------------------------------ helpers --
def _map(h, w, K, seed, scale=1.0):
    """low-resolution map [B h w, ld] as the head holds it; the padding columns K .. ld - 1 are NaN (never to be read)"""
    ld = ops.round_up(K, 8)
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B * h * w, ld), float('nan'))
    x[:, :K] = torch.randn(B * h * w, K, generator=g) * scale
    return x.to(DEV), ld


def _kw(mode):
    return {'align_corners': False} if mode == 'bilinear' else {}


def _masks(K, H, W, seed):
    """the mask patterns of the issue: name -> torch.bool [B, Cm, H, W] or None; with K = 3 both Cm = 1 and Cm = 3"""
    g = torch.Generator().manual_seed(seed)
    out = {'none': None}
    for Cm in sorted({1, K}):
        block = torch.ones(B, Cm, H, W, dtype=torch.bool)
        block[:, :, H // 4:H // 2 + 1, 1:W // 2] = False
        image = torch.ones(B, Cm, H, W, dtype=torch.bool)
        image[B - 1] = False
        single = torch.zeros(B, Cm, H, W, dtype=torch.bool)
        single[1, Cm - 1, H // 2, W - 2] = True
        out.update({f'all{Cm}': torch.ones(B, Cm, H, W, dtype=torch.bool), f'block{Cm}': block, f'image{Cm}': image,
                    f'random{Cm}': torch.rand(B, Cm, H, W, generator=g) < 0.6, f'empty{Cm}': torch.zeros(B, Cm, H, W, dtype=torch.bool),
                    f'single{Cm}': single})
    return out


def _interp64(x, h, w, K, H, W, mode):
    """the fp64 interpolation of the map's real columns -> (leaf xd [B, K, h, w], z [B, K, H, W], e_z)"""
    xd = x[:, :K].double().view(B, h, w, K).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    z = F.interpolate(xd, size=(H, W), mode=mode, **_kw(mode))
    if mode == 'bilinear':
        e_z = (8 * U * (max(h, w) + 2) + 8 * U) * float(x[:, :K].abs().max()) + ulp(torch.float32, z.detach().abs())
    else:
        e_z = torch.zeros_like(z.detach())
    return xd, z, e_z


def _berhu(d, c):
    a = d.abs()
    return torch.where(a < c, a, (d * d + c * c) / 2 / c)


def _reference(kind, x, h, w, K, H, W, mode, target, mask, up=1.0):
    """fp64 restatement on the same low-resolution map, with the module docstring's bounds"""
    xd, z, e_z = _interp64(x, h, w, K, H, W, mode)
    t = target.double().to(DEV)
    valid = torch.ones_like(t, dtype=torch.bool) if mask is None else mask.to(DEV).expand(B, K, H, W)
    n_v, N = int(valid.sum()), t.numel()
    d = torch.where(valid, z - t, torch.zeros_like(t))
    dd = d.detach()
    e_d = torch.where(valid, e_z + U * dd.abs(), torch.zeros_like(dd))
    mx = float(dd.abs().max())
    b_max = float(e_d.max())
    c = max(0.2 * mx, 1e-5)
    b_c = 0.2 * b_max + 2 * U * c
    cl = c - b_c
    out = dict(d=dd, e_d=e_d, n_v=n_v, max=mx, b_max=b_max, c=c, b_c=b_c)
    a = dd.abs()
    amb = valid & (a <= e_d)
    if kind == 'l1':
        f, e_f, g = d.abs(), e_d, torch.sign(dd)
        dg = 2.0 * amb
    elif kind == 'mse':
        f, e_f, g = d * d, 2 * a * e_d + e_d ** 2 + U * dd ** 2, 2 * dd
        dg = 2 * e_d
    else:
        f = _berhu(d, c)
        G_d = ((a + e_d) / cl).clamp_min(1.0)
        G_c = ((((a + e_d) / cl) ** 2 - 1) / 2).clamp_min(0.0)
        e_f = torch.where(valid, G_d * e_d + G_c * b_c + gamma(4) * f.detach(), torch.zeros_like(dd))
        g = torch.where(a < c, torch.sign(dd), dd / c)
        outer = (a + e_d) >= cl
        dg = 2.0 * amb + torch.where(outer, e_d / cl + (a + e_d) * b_c / cl ** 2 + U * a / cl, torch.zeros_like(dd))
    rows = lambda v: v.permute(0, 2, 3, 1).reshape(B * h * w, K)
    if n_v == 0:
        out.update(loss=0.0, b_loss=0.0, dx=torch.zeros(B * h * w, K, dtype=torch.float64, device=DEV), b_dx=torch.zeros((), device=DEV))
        return out
    loss = f.sum() / n_v
    (dx,) = torch.autograd.grad(loss * up, xd, retain_graph=True)
    fs = f.detach()
    b_loss = (float(e_f.sum()) + gamma(N + 16) * float(fs.abs().sum())) / n_v + 2 * U * abs(float(loss.detach()))
    Wof = lambda v: torch.autograd.grad(z, xd, v, retain_graph=True)[0]
    n = (2 * math.ceil(H / h) + 3) * (2 * math.ceil(W / w) + 3)
    e_w = 8 * U * (max(h, w) + 2) if mode == 'bilinear' else 0.0
    scale = abs(up) / n_v
    dx = rows(dx)
    b_dx = scale * (rows(Wof(dg)) + (U + gamma(n)) * rows(Wof(g.abs())) + n * e_w * float(g.abs().max()))
    out.update(loss=float(loss.detach()), b_loss=b_loss, dx=dx, b_dx=b_dx + 4 * U * dx.abs() + ulp(torch.float32, dx))
    return out


def _run(kind, x, ld, h, w, K, H, W, mode, target, mask, up=1.0):
    """forward + backward through ops.* into Guarded buffers -> (diff [B, K, H, W], out [4], d_logits [B h w, ld])"""
    tg = target.to(DEV).contiguous()
    mk = None if mask is None else mask.to(DEV).contiguous()
    diff_g = Guarded(B * K, H * W, H * W, torch.float32, DEV)
    diff, out = ops.reg_loss_fwd(x, ld, tg, mk, kind, B, h, w, K, H, W, mode, diff=diff_g.view.view(B, K, H, W))
    d_g = Guarded(B * h * w, ld, ld, torch.float32, DEV)
    ops.reg_loss_bwd(diff, out, torch.tensor([up], device=DEV), kind, B, h, w, K, H, W, mode, d_g.view, ld)
    torch.cuda.synchronize()
    diff_g.intact('reg_loss_fwd diff')
    d_g.intact('reg_loss_bwd d_logits')
    return diff, out, d_g.view


# ------------------------------------------------------------------------------------------------------ kernels --
@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('lo,hi', SHAPES)
def test_difference_against_zero_is_the_image_resize_fwd_writes(lo, hi, K, mode):
    (h, w), (H, W) = lo, hi
    x, ld = _map(h, w, K, seed=10 + K, scale=2.0)
    img = ops.resize_fwd(x, ld, torch.empty(B, K, H, W, device=DEV), B, h, w, K, H, W, mode)
    for kind in KINDS:
        diff, out, _ = _run(kind, x, ld, h, w, K, H, W, mode, torch.zeros(B, K, H, W), None)
        assert torch.equal(diff.view(torch.int32), img.view(torch.int32)), (kind, int((diff != img).sum()))
        assert float(out[1]) == B * K * H * W and float(out[2]) == float(img.abs().max())


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('lo,hi', SHAPES)
def test_loss_and_gradient_against_fp64(lo, hi, K, mode):
    """diff, count, max |d|, c, the loss and d_logits per element for every kind and mask pattern; the padding columns are zero, the
    guard zones intact (_run); with nothing valid the loss is 0 and the gradient all zero (the reference: NaN)"""
    (h, w), (H, W) = lo, hi
    x, ld = _map(h, w, K, seed=20 + K, scale=2.0)
    target = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(30 + K))
    for name, mask in _masks(K, H, W, seed=40).items():
        for kind in KINDS:
            ref = _reference(kind, x, h, w, K, H, W, mode, target, mask, up=1.7)
            diff, out, d = _run(kind, x, ld, h, w, K, H, W, mode, target, mask, up=1.7)
            what = f'{kind} {name} {mode} K={K} {lo}->{hi}'
            loss, cnt, mx, c = (float(v) for v in out)
            print(what, 'loss', loss, 'ref', ref['loss'], 'bound', ref['b_loss'], 'c', c, 'ref', ref['c'], 'bound', ref['b_c'],
                  'max |dx - ref|', float((d[:, :K].double() - ref['dx']).abs().max()), 'min bound', float(torch.as_tensor(ref['b_dx']).min()))
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all()), what
            assert_within(diff, ref['d'], ref['e_d'] + ulp(torch.float32, ref['d']), 'diff ' + what, names=('b', 'k', 'y', 'x'))
            if mask is not None:
                assert not diff[~mask.to(DEV).expand(B, K, H, W)].any(), what        # exactly 0 where the mask is false
            assert cnt == ref['n_v'], what
            assert abs(mx - ref['max']) <= ref['b_max'] + float(ulp(torch.float32, ref['max'])), what
            assert abs(c - ref['c']) <= ref['b_c'] + float(ulp(torch.float32, ref['c'])), what
            assert not d[:, K:].any(), what                                   # 0, not NaN: the next GEMM's operand padding
            if name.startswith('empty'):
                assert loss == 0.0 and not d.any() and c == float(np.float32(1e-5)), what
                continue
            assert abs(loss - ref['loss']) <= ref['b_loss'] + float(ulp(torch.float32, ref['loss'])), what
            assert_within(d[:, :K], ref['dx'], ref['b_dx'], 'd_logits ' + what)
            if name.startswith('image'):                                      # the fully masked image receives no gradient at all
                assert not d.view(B, h * w, ld)[B - 1].any()


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('K', [1, 3])
def test_prediction_equal_to_the_target(K, mode):
    """pred == target: every kind gives loss 0 and an all-zero gradient (sign(0) = 0), berHu's c is its floor 1e-5"""
    (h, w), (H, W) = SHAPES[1]
    x, ld = _map(h, w, K, seed=50)
    target = ops.resize_fwd(x, ld, torch.empty(B, K, H, W, device=DEV), B, h, w, K, H, W, mode)
    for kind in KINDS:
        diff, out, d = _run(kind, x, ld, h, w, K, H, W, mode, target, None)
        assert not diff.any() and not d.any() and float(out[0]) == 0.0 and float(out[1]) == B * K * H * W and float(out[2]) == 0.0
        assert float(out[3]) == float(np.float32(1e-5))


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
def test_two_runs_are_bit_equal(mode):
    (h, w), (H, W), K = (24, 40), (48, 80), 3
    x, ld = _map(h, w, K, seed=60, scale=3.0)
    target = torch.randn(B, K, H, W, generator=torch.Generator().manual_seed(61))
    mask = _masks(K, H, W, seed=62)['random1']
    bits = lambda t: t.contiguous().view(torch.int32)
    for kind in KINDS:
        runs = [_run(kind, x, ld, h, w, K, H, W, mode, target, mask, up=0.3) for _ in range(2)]
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*runs)), kind
    m = mask.to(DEV).contiguous()
    t1 = target[:, :1].contiguous().to(DEV)
    outs = [ops.depth_metrics(x, ld, t1, m, 0.5, 2.0, B, h, w, H, W, mode).clone() for _ in range(2)]
    assert torch.equal(bits(outs[0]), bits(outs[1]))


# ------------------------------------------------------------------------------------------------------ metrics --
MEAN32, STD32 = float(np.float32(metrics.NYU_MEAN)), float(np.float32(metrics.NYU_STD))


def _metrics_ref(z, e_z, target, valid):
    """fp64 values [7] and their bounds [7] (module docstring) from the fp64 prediction z, its bound e_z, target and valid mask"""
    p, t = z * STD32 + MEAN32, target.double() * STD32 + MEAN32
    e_p, e_t = STD32 * e_z + 2 * U * p.abs(), 2 * U * t.abs()
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


def _metric_inputs(H, W, seed, clamp):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(B, 1, H, W, generator=g) * 3.6 - 1.8
    if clamp:
        target.view(-1)[::9] = -2.9                                            # target std + mean < 0: clamped to 1e-6
    mask = torch.rand(B, 1, H, W, generator=g) < 0.6
    return target, mask


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('lo,hi', SHAPES)
def test_depth_metrics_against_fp64_and_acc_accumulates(lo, hi, mode):
    (h, w), (H, W) = lo, hi
    x, ld = _map(h, w, 1, seed=70, scale=0.9)
    for clamp in (False, True):
        target, mask = _metric_inputs(H, W, 71, clamp)
        for mk in (None, mask):
            _, z, e_z = _interp64(x, h, w, 1, H, W, mode)
            valid = torch.ones(B, 1, H, W, dtype=torch.bool, device=DEV) if mk is None else mk.to(DEV)
            vals, bounds = _metrics_ref(z.detach(), e_z, target.to(DEV), valid)
            out_g, acc_g = Guarded(1, 7, 8, torch.float32, DEV), Guarded(1, 8, 8, torch.float32, DEV)
            acc = acc_g.view.view(8)
            acc.zero_()
            args = (x, ld, target.to(DEV), None if mk is None else mk.to(DEV).contiguous(), metrics.NYU_MEAN, metrics.NYU_STD, B, h, w, H, W, mode)
            out = ops.depth_metrics(*args, acc=acc, out=out_g.view.view(7))
            first = acc.clone()
            ops.depth_metrics(*args, acc=acc)
            torch.cuda.synchronize()
            out_g.intact('depth_metrics out')
            acc_g.intact('depth_metrics acc')
            for k, got, v, b in zip(KEYS, out.tolist(), vals, bounds):
                print(lo, hi, mode, 'clamp' if clamp else '', 'mask' if mk is not None else '', k, got, v, b)
                assert abs(got - v) <= b + float(ulp(torch.float32, v)), (k, got, v, b)
            assert torch.equal(first[:7], out) and float(first[7]) == 1.0
            assert torch.equal(acc[:7], out + out) and float(acc[7]) == 2.0     # x + x is exact


@pytest.mark.parametrize('case', ['none', 'block', 'image', 'random', 'clamp'])
def test_depth_metrics_against_the_references_values(case):
    """the fixture's prediction as a map of the image's own size: the bilinear resize of equal sizes has the weights (1, 0) and copies"""
    pre = f'metric/{case}/'
    pred, target = torch.from_numpy(GOLD[pre + 'pred']).to(DEV), torch.from_numpy(GOLD[pre + 'target']).to(DEV)
    mask = torch.from_numpy(GOLD[pre + 'mask']).to(DEV) if pre + 'mask' in GOLD.files else None
    _, _, H, W = pred.shape
    x = torch.full((B * H * W, 8), float('nan'), device=DEV)
    x[:, 0] = pred.permute(0, 2, 3, 1).reshape(-1)
    out = ops.depth_metrics(x, 8, target, mask, metrics.NYU_MEAN, metrics.NYU_STD, B, H, W, H, W, 'bilinear')
    valid = torch.ones_like(pred, dtype=torch.bool) if mask is None else mask
    vals, bounds = _metrics_ref(pred.double(), torch.zeros_like(pred, dtype=torch.float64), target, valid)
    for k, got, gold, v, b in zip(KEYS, out.tolist(), GOLD[pre + 'values'].tolist(), vals, bounds):
        print(case, k, got, 'golden', gold, 'fp64', v, 'bound', b)
        assert abs(got - v) <= b + float(ulp(torch.float32, v)), (k, got, v, b)
        assert abs(got - gold) <= 2 * (b + float(ulp(torch.float32, v))), (k, got, gold, b)


# ------------------------------------------------------------------------------------------------ head + loss --
def _gold_head(mode='bilinear'):
    tasks, _, p, C, K, depth, (NH, NW), D, Bh = HEAD
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                              interpolate_mode=mode)
    head.init(dim_tokens_enc=D)
    head.load_state_dict({k[len('head/sd/'):]: torch.from_numpy(GOLD[k]) for k in GOLD.files if k.startswith('head/sd/')})
    t = lambda n: torch.from_numpy(GOLD['head/' + n]).to(DEV)
    return head.to(DEV), input_info(tasks, NH * NW, 16 * NH, 16 * NW), t('x'), t('target'), t('mask')


def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize('mode,tol_y,tol_g', [('fp32', 1e-5, 1e-4), ('bf16', 0.05, 0.05)])
def test_head_with_one_channel_and_berhu_matches_the_reference_step(mode, tol_y, tol_g):
    """the reference's ConvNeXtAdapter(num_classes=1) + masked_berhu_loss step (tests/golden/reg_loss.npz head/*): prediction, loss,
    token gradient and every parameter's gradient within test_convnext_head_gpu's bounds for its golden heads -- fp32 mode: 1e-5
    (prediction, loss) and 1e-4 (gradients) in relative norm; bf16 mode: that file's bf16 budget, 0.05 -- and the image is never
    written on the way"""
    head, info, x, target, mask = _gold_head()
    xg = x.clone().requires_grad_(True)
    with M.engine.precision(mode):
        y = head(xg, info)
        loss = amd_loop.depth_criterion('berhu')['depth'](y.float(), target, mask)
        assert type(loss.grad_fn).__name__ == 'RegLossFnBackward'
        loss.backward()
        torch.cuda.synchronize()
        assert not y.materialized
        gl = float(GOLD['head/loss'][0])
        print(mode, 'loss', float(loss), 'golden', gl, 'y', _rel(y.detach().clone(), GOLD['head/y']), 'dx', _rel(xg.grad, GOLD['head/dx']))
        for n, p in head.named_parameters():
            print('  ', n, _rel(p.grad, GOLD[f'head/grad/{n}']))
        assert abs(float(loss) - gl) <= tol_y * abs(gl)
        assert _rel(y.detach().clone(), GOLD['head/y']) <= tol_y
        assert _rel(xg.grad, GOLD['head/dx']) <= tol_g
        for n, p in head.named_parameters():
            assert _rel(p.grad, GOLD[f'head/grad/{n}']) <= tol_g, n


def _step(head, x, info, target, mask, kind, fused):
    head.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    M.engine.set_lazy_predictions(fused)
    try:
        y = head(xg, info)
        loss = amd_loop.depth_criterion(kind)['depth'](y if fused else y * 1, target, mask)       # a modified prediction: the eager path
        loss.backward()
    finally:
        M.engine.set_lazy_predictions(True)
    assert (type(loss.grad_fn).__name__ == 'RegLossFnBackward') == fused and y.materialized == (not fused)
    torch.cuda.synchronize()
    return loss.detach(), y, {'x': xg.grad.clone(), **{n: p.grad.clone() for n, p in head.named_parameters()}}


@pytest.mark.parametrize('kind', KINDS)
def test_fused_path_against_the_eager_path_in_one_process(kind):
    """One training step of the head both ways in fp32 mode.  The two paths share the head's forward, so they hold bit-identical
    low-resolution maps; each loss is within the module docstring's bound of the fp64 value on that map (the eager sum is an f32 sum
    of the same terms in another order), so they agree within twice that bound.  The gradients differ in how d_logits is formed
    (eager: torch's autograd on the image, then mmae_resize_bwd; fused: one gather): both reach every parameter through the same
    linear backward, and are held to the 1e-4 relative norm of the fp32 head tests against each other."""
    head, info, x, target, mask = _gold_head()
    with M.engine.precision('fp32'):
        loss_e, _, g_e = _step(head, x, info, target, mask, kind, fused=False)
        loss_f, y, g_f = _step(head, x, info, target, mask, kind, fused=True)
    hd = y._mmae_seg
    r = _reference(kind, hd.logits, hd.h, hd.w, hd.K, hd.H, hd.W, hd.mode, target, mask)
    b = r['b_loss'] + float(ulp(torch.float32, r['loss']))
    print(kind, 'loss eager', float(loss_e), 'fused', float(loss_f), 'fp64 on the map', r['loss'], 'bound', b)
    assert abs(float(loss_f) - r['loss']) <= b and abs(float(loss_f) - float(loss_e)) <= 2 * b
    for n in g_f:
        print(f'  {n}: fused against eager {_rel(g_f[n], g_e[n]):.3e}')
        assert _rel(g_f[n], g_e[n]) <= 1e-4, n


def test_head_loss_and_metrics_never_synchronise():
    """head + berHu + metrics + backward run with torch's synchronisation check set to 'error': nothing in the loss or the metrics
    reads a device value back (the reference's berHu takes a Python max() of a device scalar and indexes with boolean masks).  Three
    batches through the same static tensors give three different, finite results.

    A substitute: tests/test_cls_recipe_gpu.py shows the same property by capturing its step in graph.StepGraph, where any
    synchronisation fails the capture.  Capture of a head + regression-loss step is unsupported (criterion._refuse_under_capture: the
    one capture of this step ended in a fault of the runtime at the end of the capture, cause unknown), so the replay test of that
    file has no counterpart here and torch's own check stands in for it."""
    head, info, x0, t0, m0 = _gold_head()
    params = list(head.parameters())
    xs, ts, ms = x0.clone().requires_grad_(True), t0.clone(), m0.clone()

    def step():
        y = head(xs, info)
        loss = M.masked_berhu_loss(y.float(), ts, ms)
        vals = torch.stack(list(M.depth_metrics(y, ts, ms).values()))
        grads = torch.autograd.grad(loss, [xs] + params)
        return [loss.detach(), vals] + [g.detach() for g in grads]

    g = torch.Generator().manual_seed(9)
    batches = [(x0, t0, m0)] + [(torch.randn(x0.shape, generator=g).to(DEV), torch.randn(t0.shape, generator=g).to(DEV),
                                 (torch.rand(m0.shape, generator=g) < 0.7).to(DEV)) for _ in range(2)]
    outs = []
    with M.engine.precision('fp32'):
        for xb, tb, mb in batches:
            with torch.no_grad():
                xs.copy_(xb), ts.copy_(tb), ms.copy_(mb)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode('error')
            try:
                out = step()
            finally:
                torch.cuda.set_sync_debug_mode('default')
            outs.append([v.clone() for v in out])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for o in outs for v in o)
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[1][0], outs[2][0])


def test_a_head_prediction_is_refused_inside_a_graph_capture():
    """the head runs uncaptured; inside a (one-node) torch.cuda.graph capture the loss and the metrics raise for its prediction before
    they launch anything, and work again once the capture is over"""
    head, info, x, target, mask = _gold_head()
    with M.engine.precision('fp32'):
        y = head(x.clone().requires_grad_(True), info)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        seen = []
        with torch.cuda.graph(g):
            t2 = target + 1
            for fn in (lambda: M.masked_berhu_loss(y.float(), target, mask), lambda: M.depth_metrics(y, target, mask)):
                try:
                    fn()
                except RuntimeError as e:
                    seen.append(str(e))
        torch.cuda.synchronize()
        assert len(seen) == 2 and all('unsupported and untested' in m for m in seen), seen
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(t2, target + 1) and not y.materialized
        loss = M.masked_berhu_loss(y.float(), target, mask)
        assert type(loss.grad_fn).__name__ == 'RegLossFnBackward' and bool(torch.isfinite(loss))


def test_resize_fwd_keeps_the_bits_it_wrote_before_its_roundings_were_spelled_out():
    """tests/golden/resize_bits.npz: maps and the images mmae_resize_fwd wrote for them when its four-tap line was left to the
    compiler's contraction; with common.h's resize_tap4 the images are the same, bit for bit (W = 17, 14, 23: every ox mod 4, the
    scalar tail included)"""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'resize_bits.npz'))
    for key in [k for k in z.files if k.startswith('x_')]:
        h, w, H, W = (int(v) for v in key.split('_')[1:])
        x, gold = torch.from_numpy(z[key]).to(DEV), torch.from_numpy(z['img_' + key[2:]]).to(DEV)
        Bk, K = gold.shape[:2]
        img = ops.resize_fwd(x, 8, torch.empty(Bk, K, H, W, device=DEV), Bk, h, w, K, H, W, 'bilinear')
        assert torch.equal(img.view(torch.int32), gold.view(torch.int32)), (key, int((img != gold).sum()))
