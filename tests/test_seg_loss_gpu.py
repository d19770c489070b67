"""GPU: the fused resize + cross-entropy loss, the fused argmax and the device histograms of csrc/segloss.hip, and their host side
(criterion.SegCrossEntropyLoss, metrics.seg_argmax / SegMetric).  Kernels element by element against fp64 torch (F.interpolate +
F.cross_entropy and their autograd) with bounds derived from the unit roundoff, outputs in Guarded buffers, the logits' padding
columns poisoned with NaN; the interpolation bit for bit against the image mmae_resize_fwd writes; the head + loss step against the
reference's golden fine-tuning step; the fused path against the eager path in the same process.

Bounds (u = 2^-24, gamma_n as helpers.gamma).  n_l = ceil(K / 64) classes per lane.
  z      interpolated logit.  Bilinear: test_resize_fwd's bound e_z = (8 u (max(h, w) + 2) + 8 u) max|x| + ulp(z); nearest: 0 (a copy).
  lse    every z_k moves by <= e_z, so the exact log-sum-exp moves by <= e_z.  The kernel's exponential is exp2(d log2 e): the
         difference d and the product round once each (2 u |d|), v_exp_f32 is good to 1 ulp (2 u).  A term exp(z_k - M) reaches the
         wave's sum through its own exponential (2 u, argument: 2 u range), at most n_l + 1 rescale products (product u, exponential
         2 u each; their arguments add up to <= range: 2 u range) and n_l lane additions + 6 shuffle additions:
             r_s = gamma_(n_l + 6) + 2 u + 3 u (n_l + 1) + 4 u range;   |dlse| <= e_z + 1.01 r_s + 2 u |lse - max| + u |lse|
         (logf taken as 2 u relative, the sum as helpers.ce_loss_ref does).
  loss   per valid pixel lse - z_t: b_lse + e_z + u |nll|; the sum over N valid pixels in any order: gamma_N sum |nll|; the mean: one
         division and one rounding: 2 u |loss|.
  dx     element (iy, ix, k) sums at most n = (2 ceil(H / h) + 3)(2 ceil(W / w) + 3) terms weight (p - y) (test_resize_bwd_gather's
         count), a weight within e_w = 8 u (max(h, w) + 2) (0 for nearest), |p - y| <= 1, p = exp2((z - lse) log2 e) (the
         difference and the product round once each: 2 u |z - lse|; v_exp_f32 is good to 1 ulp: 2 u) within
         dp = expm1(b_lse + e_z + 2 u |z - lse|) + 2 u, the difference p - y one rounding: with S_w the element's exact weight sum over valid
         pixels:  scale (S_w (dp + u + gamma_n) + n e_w), scale = up / count formed with <= 3 roundings and applied with one:
         + 4 u |dx| + ulp(dx)."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import multimae_amd as M
from multimae_amd import ops, output_adapters as OA
from dropin import amd_loop
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_convnext import HEADS, input_info  # noqa: E402

GOLD_HEAD = os.path.join(ROOT, 'tests', 'golden', 'convnext_head.npz')
GOLD_SEG = os.path.join(ROOT, 'tests', 'golden', 'seg_metrics.npz')
U = 2.0 ** -24
IGN = 255


# ------------------------------------------------------------------------------------------------------ helpers --
def _logits(B, h, w, K, seed, scale=1.0):
    """low-resolution logits [B h w, ld] as the head holds them; the padding columns K .. ld - 1 are NaN (never to be read)"""
    ld = ops.round_up(K, 8)
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B * h * w, ld), float('nan'))
    x[:, :K] = torch.randn(B * h * w, K, generator=g) * scale
    return x.to(DEV), ld


def _size(h, w, r):
    return int(round(h * r)), int(round(w * r))


def _targets(B, H, W, K, seed):
    """the target patterns of the issue: name -> int64 [B, H, W]"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, K, (B, H, W), generator=g)
    block = base.clone()
    block[:, H // 4:H // 2 + 1, 1:W // 2] = IGN
    image = base.clone()
    image[B - 1] = IGN
    oor = base.clone()
    oor.view(-1)[0::7] = -1
    oor.view(-1)[1::7] = K
    oor.view(-1)[2::7] = 254 if K <= 254 else K + 7
    oor.view(-1)[3::7] = IGN
    return {'none': base, 'block': block, 'image': image, 'batch': torch.full((B, H, W), IGN), 'out_of_range': oor}


def _kw(mode):
    return {'align_corners': False} if mode == 'bilinear' else {}


def _reference(x, ld, B, h, w, K, H, W, mode, target, up=1.0):
    """fp64 restatement on the same low-resolution logits, with the module docstring's bounds"""
    xd = x[:, :K].double().view(B, h, w, K).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    z = F.interpolate(xd, size=(H, W), mode=mode, **_kw(mode))
    tg = target.to(DEV)
    valid = (tg >= 0) & (tg < K) & (tg != IGN)
    tc = torch.where(valid, tg, torch.full_like(tg, IGN))
    n_valid = int(valid.sum())
    zd = z.detach()
    lse = torch.logsumexp(zd, 1)
    mx, rng = zd.amax(1), zd.amax(1) - zd.amin(1)
    xmax = float(x[:, :K].abs().max())
    e_z = (8 * U * (max(h, w) + 2) + 8 * U) * xmax + ulp(torch.float32, zd.abs().amax(1)) if mode == 'bilinear' else torch.zeros_like(lse)
    n_l = (K + 63) // 64
    r_s = gamma(n_l + 6) + 2 * U + 3 * U * (n_l + 1) + 4 * U * (rng + 2 * e_z)
    b_lse = e_z + 1.01 * r_s + 2 * U * (lse - mx).abs() + U * lse.abs()
    out = dict(z=zd, lse=lse, b_lse=b_lse, valid=valid, n_valid=n_valid)
    n = (2 * math.ceil(H / h) + 3) * (2 * math.ceil(W / w) + 3)
    if n_valid == 0:
        out.update(loss=0.0, b_loss=0.0, d=torch.zeros(B * h * w, K, dtype=torch.float64, device=DEV), b_d=torch.zeros((), device=DEV))
        return out
    loss = F.cross_entropy(z, tc, ignore_index=IGN)
    (d,) = torch.autograd.grad(loss * up, xd, retain_graph=True)
    nll = (lse - torch.gather(zd, 1, torch.where(valid, tg, torch.zeros_like(tg))[:, None]).squeeze(1)) * valid
    e_n = ((b_lse + e_z + U * nll.abs()) * valid).sum() + gamma(n_valid + 16) * nll.abs().sum()
    out.update(loss=float(loss), b_loss=float(e_n) / n_valid + 2 * U * abs(float(loss)))
    # S_w: each element's exact weight sum over the valid pixels (the interpolation's backward applied to the valid mask)
    (S_w,) = torch.autograd.grad(z, xd, valid[:, None].expand_as(z).double())
    dp = torch.expm1((b_lse + e_z).amax() + 2 * U * (zd - lse[:, None]).abs().amax()) + 2 * U
    e_w = 8 * U * (max(h, w) + 2) if mode == 'bilinear' else 0.0
    scale = abs(up) / n_valid
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * h * w, K)
    d = to_rows(d)
    b_d = scale * (to_rows(S_w) * (dp + U + gamma(n)) + n * e_w)
    out.update(d=d, b_d=b_d + 4 * U * d.abs() + ulp(torch.float32, d))
    return out


def _run(x, ld, B, h, w, K, H, W, mode, target, up=1.0):
    """forward + backward through ops.* into Guarded buffers -> (lse [B, H, W], out [2], d_logits Guarded)"""
    tg = target.to(DEV).contiguous()
    lse_g = Guarded(B, H * W, H * W, torch.float32, DEV)
    lse, out = ops.seg_ce_fwd(x, ld, tg, IGN, B, h, w, K, H, W, mode, lse=lse_g.view.view(B, H, W))
    d_g = Guarded(B * h * w, ld, ld, torch.float32, DEV)
    ops.seg_ce_bwd(x, ld, tg, IGN, B, h, w, K, H, W, mode, lse, out, torch.tensor([up], device=DEV), d_g.view)
    torch.cuda.synchronize()
    lse_g.intact('seg_ce_fwd lse')
    d_g.intact('seg_ce_bwd d_logits')
    return lse, out, d_g


# upsampling by 4, 8 and 16 / 3 (preds_per_patch = 9: h = 3 NH against H = 16 NH), non-square images, B from 1 to 4
GEOMS = [(1, 8, 8, 4), (2, 4, 6, 8), (3, 3, 6, 16 / 3), (4, 5, 9, 4)]
KS = [3, 4, 150, 151]


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('B,h,w,r', GEOMS)
def test_forward_against_fp64(B, h, w, r, K, mode):
    """test 1: the lse map per element and the scalar loss against F.interpolate + F.cross_entropy in fp64"""
    H, W = _size(h, w, r)
    x, ld = _logits(B, h, w, K, seed=20 + K, scale=2.0)
    for name, tg in _targets(B, H, W, K, seed=30).items():
        ref = _reference(x, ld, B, h, w, K, H, W, mode, tg)
        lse, out, _ = _run(x, ld, B, h, w, K, H, W, mode, tg)
        what = f'{name} {mode} K={K}'
        print(what, 'max |lse - ref|', float((lse.double() - ref['lse']).abs().max()), 'min bound', float(ref['b_lse'].min()),
              'loss', float(out[0]), 'ref', ref['loss'], 'bound', ref['b_loss'])
        assert_within(lse, ref['lse'], ref['b_lse'], 'lse ' + what, names=('b', 'y', 'x'))
        assert float(out[1]) == ref['n_valid'], what
        if name == 'batch':
            assert float(out[0]) == 0.0 and out.dtype == torch.float32        # torch: NaN
        else:
            assert abs(float(out[0]) - ref['loss']) <= ref['b_loss'] + float(ulp(torch.float32, ref['loss'])), what


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('B,h,w,r', GEOMS)
def test_backward_against_fp64_autograd(B, h, w, r, K, mode):
    """test 2: d_logits per element against fp64 autograd; padding columns exactly zero, guard zones intact (_run)"""
    H, W = _size(h, w, r)
    x, ld = _logits(B, h, w, K, seed=40 + K, scale=2.0)
    for name, tg in _targets(B, H, W, K, seed=50).items():
        ref = _reference(x, ld, B, h, w, K, H, W, mode, tg, up=1.7)
        _, _, d_g = _run(x, ld, B, h, w, K, H, W, mode, tg, up=1.7)
        what = f'{name} {mode} K={K}'
        d = d_g.view
        print(what, 'max |d - ref|', float((d[:, :K].double() - ref['d']).abs().max()), 'max |ref|', float(ref['d'].abs().max()),
              'min bound', float(torch.as_tensor(ref['b_d']).min()))
        assert not d[:, K:].any(), what                                   # 0, not NaN: the next GEMM's operand padding
        if name == 'batch':
            assert not d.any(), what
        else:
            assert_within(d[:, :K], ref['d'], ref['b_d'], 'd_logits ' + what)
        if name == 'image':                                               # the fully ignored image receives no gradient at all
            assert not d.view(B, h * w, ld)[B - 1].any()


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
def test_two_runs_are_bit_equal(mode):
    """test 4"""
    B, h, w, K, (H, W) = 3, 12, 18, 150, (64, 96)
    x, ld = _logits(B, h, w, K, seed=60, scale=3.0)
    tg = _targets(B, H, W, K, seed=61)['block']
    runs = [_run(x, ld, B, h, w, K, H, W, mode, tg, up=0.3) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2].view, runs[1][2].view)


def _first_argmax(img, n_cls):
    """argmax over the first n_cls channels, the lowest index on ties (torch.argmax does not promise which)"""
    v = img[:, :n_cls]
    idx = torch.arange(n_cls, device=img.device).view(1, -1, 1, 1).expand_as(v)
    return torch.where(v == v.amax(1, keepdim=True), idx, torch.full_like(idx, n_cls)).amin(1)


def _argmax(x, ld, B, h, w, K, n_cls, H, W, mode):
    g = Guarded(B, 2 * H * W, 2 * H * W, torch.int32, DEV)               # an int64 [B, H, W] output inside int32 guard zones
    pred = g.full.view(torch.int64).view(B, H, W)
    ops.seg_argmax(x, ld, pred, B, h, w, K, n_cls, H, W, mode)
    torch.cuda.synchronize()
    g.intact('seg_argmax')
    return pred


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('h,w,K', [(32, 32, 150), (12, 18, 4), (16, 24, 3)])
def test_argmax_is_the_argmax_of_the_image_resize_fwd_writes(h, w, K, mode):
    """test 5: exact agreement with the first-index argmax of the image the existing ops.resize_fwd writes (N(0, 1) logits, and the
    same logits with constructed ties), and agreement with the fp64 interpolation wherever its top-two gap exceeds twice the resize
    bound -- at most 1 % of the pixels may be excluded that way"""
    B, (H, W) = 2, (4 * h, 4 * w)
    x, ld = _logits(B, h, w, K, seed=70)
    ties = x.clone()
    v = ties.view(B, h, w, ld)
    v[:, : h // 2, :, 1] = v[:, : h // 2, :, 0] = 4.0 + v[:, : h // 2, :, 0]      # classes 0 and 1 equal and largest: 0 wins
    v[:, h // 2:, : w // 2, :K] = 0.25                                          # all classes equal: 0 wins
    v[:, :, w - 2:, K - 1] = v[:, :, w - 2:, K - 2] = 6.0                           # the last two equal and largest: K - 2 wins
    for name, lg in (('normal', x), ('ties', ties)):
        img = ops.resize_fwd(lg, ld, torch.empty(B, K, H, W, device=DEV), B, h, w, K, H, W, mode)
        for n_cls in (K, K - 1):
            pred = _argmax(lg, ld, B, h, w, K, n_cls, H, W, mode)
            ref = _first_argmax(img, n_cls)
            assert torch.equal(pred, ref), (name, n_cls, int((pred != ref).sum()))
    z = F.interpolate(x[:, :K].double().view(B, h, w, K).permute(0, 3, 1, 2), size=(H, W), mode=mode, **_kw(mode))
    top = z.topk(2, dim=1).values
    e_z = (8 * U * (max(h, w) + 2) + 8 * U) * float(x[:, :K].abs().max()) + ulp(torch.float32, top[:, 0]) if mode == 'bilinear' else 0.0
    sure = (top[:, 0] - top[:, 1]) > 2 * e_z
    excluded = 1.0 - float(sure.double().mean())
    print(f'argmax {mode} ({h}, {w}, {K}): excluded share {excluded:.5f}')
    assert excluded <= 0.01
    pred = _argmax(x, ld, B, h, w, K, K, H, W, mode)
    assert torch.equal(pred[sure], z.argmax(1)[sure])


# ------------------------------------------------------------------------------------------------ head + loss --
def _layer_id(name, n):
    if name == 'global_tokens' or name.startswith('input_adapters'):
        return 0
    if name.startswith('encoder'):
        return int(name.split('.')[1]) + 1
    return n - 1


def test_head_and_fused_loss_fp32_step_matches_reference_golden():
    """test 6: the reference's fine-tuning step (tests/golden/convnext_head.npz step/*) with the fused criterion: loss within 1e-5
    relative, each parameter's step within 0.05 of the reference step's norm (the bounds of
    test_multivit_with_head_fp32_forward_backward_and_one_step_match_golden); the image is never written on the way, and reading it
    afterwards gives the eager path's image bit for bit"""
    gold = np.load(GOLD_HEAD)
    from test_convnext_head_cpu import build_vit
    model = build_vit()
    pre = 'vit/sd/'
    model.load_state_dict({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)})
    model = model.to(DEV)
    model.build_arena()
    xs, target = torch.from_numpy(gold['step/x']).to(DEV), torch.from_numpy(gold['step/target']).to(DEV)
    with M.engine.precision('fp32'):
        M.engine.set_lazy_predictions(False)
        try:
            with torch.no_grad():
                eager = model({'rgb': xs})['semseg'].detach().clone()
        finally:
            M.engine.set_lazy_predictions(True)
        L = model.get_num_layers()
        values = [0.75 ** (L + 1 - i) for i in range(L + 2)]
        args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, momentum=0.9)
        opt = amd_loop.create_optimizer_groups(args, model, skip_list=model.no_weight_decay(),
                                               get_num_layer=lambda nm: _layer_id(nm, L + 2), get_layer_scale=lambda k: values[k])
        for grp in opt.param_groups:
            grp['lr'] = args.lr * grp.get('lr_scale', 1.0)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        opt.zero_grad()
        logits = model({'rgb': xs})['semseg']
        loss = amd_loop.seg_criterion(255)(logits, target)
        assert type(loss.grad_fn).__name__ == 'SegCEFnBackward'
        print('loss', loss.item(), 'golden', float(gold['step/loss'][0]))
        assert abs(loss.item() - float(gold['step/loss'][0])) <= 1e-5 * abs(float(gold['step/loss'][0]))
        loss.backward()
        assert logits.materialized is False
        opt.step()
        torch.cuda.synchronize()
        assert logits.materialized is False
        assert torch.equal(logits.detach().clone(), eager) and logits.materialized        # read after backward() and step()
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        d_e = (p.detach() - before[n]).double().cpu()
        d_g = torch.from_numpy(gold[f'step/param/{n}']).double() - before[n].double().cpu()
        assert float((d_e - d_g).norm()) <= 0.05 * float(d_g.norm()) + 1e-7, n


def _head_from_gold(gold, name):
    tasks, mode, p, C, K, depth, (NH, NW), D, B = HEADS[name]
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                              interpolate_mode=mode)
    head.init(dim_tokens_enc=D)
    pre = f'{name}/sd/'
    head.load_state_dict({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)})
    return head.to(DEV), input_info(tasks, NH * NW, 16 * NH, 16 * NW)


def _restate_fp64_loss(head, P, x, info, target):
    """ConvNeXtAdapter.forward + CrossEntropyLoss(ignore_index=255) written out in fp64 from the parameters P (not the reference's code)"""
    H, W = info['image_size']
    NH, NW = H // 16, W // 16
    s, C = int(round(head.preds_per_patch ** 0.5)), head.class_dim
    toks = torch.cat([x[:, info['tasks'][t]['start_idx']:info['tasks'][t]['end_idx']] for t in head.main_tasks], -1)
    z = toks @ P['proj_dec.weight'].t() + P['proj_dec.bias']
    z = z.view(x.shape[0], NH, NW, s, s, C).permute(0, 5, 1, 3, 2, 4).reshape(x.shape[0], C, NH * s, NW * s)
    for i in range(len(head.blocks)):
        q = f'blocks.{i}.'
        t = F.conv2d(z, P[q + 'dwconv.weight'], P[q + 'dwconv.bias'], padding=3, groups=C).permute(0, 2, 3, 1)
        t = F.layer_norm(t, (C,), P[q + 'norm.weight'], P[q + 'norm.bias'], 1e-6)
        t = t @ P[q + 'pwconv1.weight'].t() + P[q + 'pwconv1.bias']
        t = 0.5 * t * (1 + torch.erf(t / math.sqrt(2)))
        t = t @ P[q + 'pwconv2.weight'].t() + P[q + 'pwconv2.bias']
        z = z + t.permute(0, 3, 1, 2)
    z = F.conv2d(z, P['final_layer.weight'], P['final_layer.bias'])
    z = F.interpolate(z, size=(H, W), mode=head.interpolate_mode, **_kw(head.interpolate_mode))
    return F.cross_entropy(z, target, ignore_index=IGN)


def _step(head, x, info, target, fused):
    head.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    M.engine.set_lazy_predictions(fused)
    try:
        y = head(xg, info)
        loss = (M.SegCrossEntropyLoss if fused else nn.CrossEntropyLoss)(ignore_index=IGN)(y, target)
        loss.backward()
    finally:
        M.engine.set_lazy_predictions(True)
    assert (type(loss.grad_fn).__name__ == 'SegCEFnBackward') == fused and y.materialized == (not fused)
    torch.cuda.synchronize()
    return loss.detach(), y, {'x': xg.grad.clone(), **{n: p.grad.clone() for n, p in head.named_parameters()}}


@pytest.mark.parametrize('mode,tol', [('fp32', 1e-4), ('bf16', 0.05)])
@pytest.mark.parametrize('name', ['head', 'rgbd_nearest', 'p9'])
def test_fused_path_against_the_eager_path_in_one_process(name, mode, tol):
    """test 7: the parent path (set_lazy_predictions(False) + nn.CrossEntropyLoss) and the fused path on the same head and batch.

    The two paths share the head's forward, so they hold bit-identical low-resolution logits; they differ in how d_logits is formed
    (eager: torch's log-softmax / NLL backward on the image, then mmae_resize_bwd; fused: one gather with the softmax recomputed).
    The loss: each is within test 1's bound of the fp64 value on those logits, so they agree within twice that bound.  The gradients:
    the head's backward is one linear map of d_logits, but its operator norm is not something this test can state, so -- as
    test_head_bf16_within_bf16_bounds_of_fp64 does -- both paths are measured against the fp64 restatement of head + loss, each
    parameter's gradient (and the token gradient) in relative norm: 1e-4 in fp32 mode (the bound test_head_fp32_matches_reference_golden
    holds this head's gradients to), 0.05 in bf16 mode (that test's budget: 2 + 2 depth chained products with two bf16 operand
    roundings each and four bf16-stored activations per block at u = 2^-9).  The fused path has to meet the bound; the eager path's
    figure is printed beside it."""
    gold = np.load(GOLD_HEAD)
    head, info = _head_from_gold(gold, name)
    K, B = HEADS[name][4], HEADS[name][8]
    H, W = info['image_size']
    x = torch.from_numpy(gold[f'{name}/x']).to(DEV)
    target = _targets(B, H, W, K, seed=80)['block'].to(DEV)
    P = {k: v.detach().double().requires_grad_(True) for k, v in head.state_dict().items()}
    xd = x.double().requires_grad_(True)
    ref_loss = _restate_fp64_loss(head, P, xd, info, target)
    ref_loss.backward()
    ref = {'x': xd.grad, **{n: P[n].grad for n, _ in head.named_parameters()}}
    with M.engine.precision(mode):
        loss_e, _, g_e = _step(head, x, info, target, fused=False)
        loss_f, y, g_f = _step(head, x, info, target, fused=True)
    hd = y._mmae_seg
    r = _reference(hd.logits, hd.ld, *hd.geom(), target)
    print(name, mode, 'loss eager', float(loss_e), 'fused', float(loss_f), 'fp64 on the logits', r['loss'], 'bound', r['b_loss'],
          'fp64 restatement', float(ref_loss))
    assert abs(float(loss_f) - r['loss']) <= r['b_loss'] + float(ulp(torch.float32, r['loss']))
    assert abs(float(loss_f) - float(loss_e)) <= 2 * (r['b_loss'] + float(ulp(torch.float32, r['loss'])))
    rel = lambda a, b: float((a.double() - b).norm() / (b.norm() + 1e-30))
    for n in ref:
        e, f = rel(g_e[n], ref[n]), rel(g_f[n], ref[n])
        print(f'  {n}: eager {e:.3e} fused {f:.3e} fused-eager {rel(g_f[n], g_e[n].double()):.3e}')
        assert f <= tol, (n, f, e)


def test_fallbacks_return_torchs_value_and_two_fused_losses_add():
    """test 8"""
    gold = np.load(GOLD_HEAD)
    head, info = _head_from_gold(gold, 'head')
    K, B = HEADS['head'][4], HEADS['head'][8]
    H, W = info['image_size']
    x = torch.from_numpy(gold['head/x']).to(DEV)
    t1, t2 = (_targets(B, H, W, K, seed=s)['block'].to(DEV) for s in (90, 91))
    wts = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    with M.engine.precision('fp32'):
        M.engine.set_lazy_predictions(False)
        try:
            with torch.no_grad():
                img = head(x, info).detach().clone()
        finally:
            M.engine.set_lazy_predictions(True)
        cases = [(dict(ignore_index=IGN), lambda y: y * 1), (dict(ignore_index=IGN, weight=wts), lambda y: y),
                 (dict(ignore_index=IGN, label_smoothing=0.1), lambda y: y), (dict(ignore_index=IGN, reduction='sum'), lambda y: y)]
        for kw, prep in cases:
            y = head(x.clone().requires_grad_(True), info)
            assert not y.materialized
            loss = M.SegCrossEntropyLoss(**kw)(prep(y), t1)
            assert type(loss.grad_fn).__name__ != 'SegCEFnBackward' and y.materialized, kw
            assert torch.equal(y.detach().clone(), img)
            assert torch.allclose(loss.detach(), nn.CrossEntropyLoss(**kw)(img, t1), rtol=1e-6, atol=0), kw
            loss.backward()
        crit = M.SegCrossEntropyLoss(ignore_index=IGN)
        grads = []
        for which in ((t1,), (t2,), (t1, t2)):
            head.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_(True)
            y = head(xg, info)
            sum(crit(y, t) for t in which).backward()
            assert not y.materialized
            grads.append([xg.grad.clone()] + [p.grad.clone() for p in head.parameters()])
        # the head's backward is linear in d_logits; f32 roundings along its chains: the 1e-4 relative norm of the fp32 head tests
        for a, b, ab in zip(*grads):
            assert float((ab.double() - (a.double() + b.double())).norm()) <= 1e-4 * float((a.double() + b.double()).norm()) + 1e-12


# ---------------------------------------------------------------------------------------------------- metrics --
def _hist_ref(pred, label, K):
    keep = label != IGN
    p, l = pred[keep], label[keep]
    pin, lin = (p >= 0) & (p < K), (l >= 0) & (l < K)
    cp, cl = torch.bincount(p[pin], minlength=K), torch.bincount(l[lin], minlength=K)
    ci = torch.bincount(p[pin & (p == l)], minlength=K)
    return torch.stack([ci, cp + cl - ci, cp, cl])


@pytest.mark.parametrize('case', ['ade', 'small', 'absent'])
def test_seg_metric_equals_the_reference_histograms(case):
    """test 9: the histograms of the reference's intersect_and_union (the fixture) exactly; two updates accumulate; compute() is the
    numpy arithmetic of eval_metrics, NaN for an absent class included"""
    z = np.load(GOLD_SEG)
    parts = [(torch.from_numpy(z[f'{case}/{i}/pred'].astype(np.int64)).to(DEV), torch.from_numpy(z[f'{case}/{i}/label'].astype(np.int64)).to(DEV),
              z[f'{case}/{i}/hist']) for i in range(2)]
    K = parts[0][2].shape[1]
    m = M.SegMetric(K, IGN)
    g = Guarded(4, 2 * K, 2 * K, torch.int32, DEV)
    g.full.zero_()
    m.hist = g.full.view(torch.int64)
    m.update(parts[0][0], parts[0][1])
    assert np.array_equal(m.hist.cpu().numpy(), parts[0][2])
    m.update(parts[1][0].to(torch.int32), parts[1][1].to(torch.uint8))          # other integer dtypes are converted
    total = parts[0][2] + parts[1][2]
    torch.cuda.synchronize()
    g.intact('seg_hist')
    assert np.array_equal(m.hist.cpu().numpy(), total)
    all_acc, acc, iou = m.compute()
    with np.errstate(divide='ignore', invalid='ignore'):
        assert all_acc == total[0].sum() / total[3].sum()
        assert np.array_equal(acc, total[0] / total[3], equal_nan=True) and np.array_equal(iou, total[0] / total[1], equal_nan=True)
    if case == 'absent':
        assert np.isnan(iou[-1]) and np.isnan(acc[-1])


def test_seg_hist_drops_values_outside_the_classes():
    """a prediction or label outside [0, K) is dropped -- a value equal to K is NOT counted into class K - 1 (np.histogram would)"""
    K = 7
    g = torch.Generator().manual_seed(5)
    pred = torch.randint(-2, K + 3, (3, 33, 17), generator=g).to(DEV)
    label = torch.randint(-1, K + 2, (3, 33, 17), generator=g).to(DEV)
    label[0, :4] = IGN
    m = M.SegMetric(K, IGN)
    m.update(pred, label)
    assert torch.equal(m.hist, _hist_ref(pred, label, K))


def test_seg_metric_takes_the_heads_prediction():
    gold = np.load(GOLD_HEAD)
    head, info = _head_from_gold(gold, 'p9')
    K, B = HEADS['p9'][4], HEADS['p9'][8]
    H, W = info['image_size']
    x = torch.from_numpy(gold['p9/x']).to(DEV)
    tg = _targets(B, H, W, K, seed=95)['block'].to(DEV)
    with torch.no_grad(), M.engine.precision('fp32'):
        y = head(x, info)
        m = amd_loop.seg_metric(K, IGN)
        m.update(y, tg)
        a = M.seg_argmax(y, K - 1)
        assert not y.materialized and a.dtype == torch.int64
        img = y.detach().clone()
    assert torch.equal(a, _first_argmax(img, K - 1))
    assert torch.equal(m.hist, _hist_ref(_first_argmax(img, K), tg, K))
    assert torch.equal(M.seg_argmax(img, K - 1), img[:, :K - 1].argmax(1))        # a plain tensor: torch's own argmax


# ------------------------------------------------------------------------------------------------- ADE20K size --
def test_ade20k_geometry_against_fp64_on_a_sample():
    """test 10: B = 4, 512 x 512, K = 150 on 128 x 128 logits: forward, backward, argmax and histograms are finite and agree with the
    fp64 restatement on a random sample of pixels"""
    B, h, w, K, H, W = 4, 128, 128, 150, 512, 512
    x, ld = _logits(B, h, w, K, seed=100, scale=3.0)
    g = torch.Generator().manual_seed(101)
    tg = torch.randint(0, K, (B, H, W), generator=g)
    tg[torch.rand(B, H, W, generator=g) < 0.1] = IGN
    tg[1, 100:300, 50:400] = IGN
    ref = _reference(x, ld, B, h, w, K, H, W, 'bilinear', tg, up=1.0)
    lse, out, d_g = _run(x, ld, B, h, w, K, H, W, 'bilinear', tg)
    d = d_g.view
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(d).all()) and not d[:, K:].any()
    print('ADE20K loss', float(out[0]), 'ref', ref['loss'], 'bound', ref['b_loss'], 'count', float(out[1]))
    assert float(out[1]) == ref['n_valid']
    assert abs(float(out[0]) - ref['loss']) <= ref['b_loss'] + float(ulp(torch.float32, ref['loss']))
    pix = torch.randint(0, B * H * W, (20000,), generator=g).to(DEV)
    assert_within(lse.view(-1)[pix], ref['lse'].view(-1)[pix], ref['b_lse'].view(-1)[pix], 'ADE20K lse sample')
    rows = torch.randint(0, B * h * w, (4000,), generator=g).to(DEV)
    assert_within(d[rows, :K], ref['d'][rows], ref['b_d'][rows], 'ADE20K d_logits sample')
    pred = _argmax(x, ld, B, h, w, K, K, H, W, 'bilinear')
    top = ref['z'].topk(2, dim=1).values
    e_z = (8 * U * (max(h, w) + 2) + 8 * U) * float(x[:, :K].abs().max()) + ulp(torch.float32, top[:, 0])
    sure = ((top[:, 0] - top[:, 1]) > 2 * e_z).view(-1)[pix]
    assert float(sure.double().mean()) >= 0.99
    assert torch.equal(pred.view(-1)[pix][sure], ref['z'].argmax(1).view(-1)[pix][sure])
    m = M.SegMetric(K, IGN)
    m.update(pred, tg.to(DEV))
    assert torch.equal(m.hist, _hist_ref(pred, tg.to(DEV), K)) and int(m.hist[3].sum()) == ref['n_valid']
    assert all(np.isfinite(v).all() for v in m.compute())
