"""GPU: the ConvNeXt semantic-segmentation head (csrc/convnext.hip + ConvNeXtAdapter).  Each new kernel element by element against
fp64 torch (F.conv2d(groups=C), F.interpolate and their autograd) on odd geometries, outputs in Guarded buffers; the pixel shuffle
bit-exact; bit-equal gradients from two backward passes; the fp32 mode against the reference's golden outputs, gradients and one
fine-tuning step (tests/golden/convnext_head.npz); the bf16 mode against an fp64 restatement; the ADE20K geometry end to end."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multimae_amd as M
from multimae_amd import ops, output_adapters as OA
from dropin import amd_loop
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_convnext import HEADS, VIT, input_info, weight_like  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden', 'convnext_head.npz')
U = 2.0 ** -24                                                    # fp32 unit roundoff
GEOMS = [(1, 1, 1, 4), (3, 3, 7, 12), (1, 13, 37, 40), (3, 37, 13, 4), (1, 7, 1, 384), (3, 1, 13, 12), (1, 37, 37, 3), (1, 13, 7, 384)]


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def _guarded(shape):
    rows = shape[0]
    cols = int(np.prod(shape[1:]))
    return Guarded(rows, cols, cols, torch.float32, DEV)


# ----------------------------------------------------------------------------------------------------- kernels --
@pytest.mark.parametrize('B,NH,NW,s,C', [(1, 1, 1, 1, 4), (3, 2, 3, 4, 12), (2, 3, 1, 3, 40), (1, 2, 2, 2, 384), (2, 3, 2, 3, 5)])
def test_pixel_shuffle_bit_exact(B, NH, NW, s, C):
    """map[b, nh s + ph, nw s + pw, c] = proj[b, nh NW + nw, (ph s + pw) C + c] (the reference's two rearranges), and back"""
    proj = _rand(B, NH * NW, s * s * C, seed=1)
    ref = proj.view(B, NH, NW, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(B * NH * s * NW * s, C)
    out = _guarded((B * NH * s * NW * s, C))
    ops.convnext_shuffle(proj, out.view, B, NH, NW, s, C)
    back = _guarded((B * NH * NW, s * s * C))
    ops.convnext_shuffle(ref.contiguous(), back.view, B, NH, NW, s, C, inverse=True)
    torch.cuda.synchronize()
    out.intact('shuffle_fwd')
    back.intact('shuffle_bwd')
    assert torch.equal(out.view, ref)
    assert torch.equal(back.view, proj.view(B * NH * NW, -1))


def _nchw(x, B, h, w, C):
    return x.view(B, h, w, C).permute(0, 3, 1, 2).double()


@pytest.mark.parametrize('B,h,w,C', GEOMS)
def test_dwconv7_fwd(B, h, w, C):
    x, wt, b = _rand(B * h * w, C, seed=2), _rand(C, 1, 7, 7, seed=3) * 0.2, _rand(C, seed=4)
    y = _guarded((B * h * w, C))
    ops.dwconv7_fwd(x, wt, b, y.view, B, h, w, C)
    torch.cuda.synchronize()
    y.intact('dwconv7_fwd')
    xd = _nchw(x, B, h, w, C)
    ref = F.conv2d(xd, wt.double(), b.double(), padding=3, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    T = F.conv2d(xd.abs(), wt.double().abs(), padding=3, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    # 49 products summed in fp32 from 0, then the bias added: any-order summation of 50 terms, gamma_50 (|x| * |w| + |b|),
    # plus the final rounding to fp32
    bound = gamma(50) * (T + b.double().abs()) + ulp(torch.float32, ref)
    assert_within(y.view, ref, bound, 'dwconv7_fwd')


@pytest.mark.parametrize('B,h,w,C', GEOMS)
def test_dwconv7_dgrad_adds_residual_gradient(B, h, w, C):
    dy, wt, dxin = _rand(B * h * w, C, seed=5), _rand(C, 1, 7, 7, seed=6) * 0.2, _rand(B * h * w, C, seed=7)
    out = _guarded((B * h * w, C))
    ops.dwconv7_dgrad(dy, wt, dxin, out.view, B, h, w, C)
    torch.cuda.synchronize()
    out.intact('dwconv7_dgrad')
    xd = torch.zeros(B, C, h, w, dtype=torch.float64, device=DEV, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(xd, wt.double(), padding=3, groups=C), xd, _nchw(dy, B, h, w, C))
    ref = g.permute(0, 2, 3, 1).reshape(-1, C) + dxin.double()
    (ga,) = torch.autograd.grad(F.conv2d(xd, wt.double().abs(), padding=3, groups=C), xd, _nchw(dy, B, h, w, C).abs())
    T = ga.permute(0, 2, 3, 1).reshape(-1, C)
    # 49 fp32 FMAs from 0 and one add of dx_in: gamma_50 (|dy| * |w| + |dx_in|) plus the final rounding
    bound = gamma(50) * (T + dxin.double().abs()) + ulp(torch.float32, ref)
    assert_within(out.view, ref, bound, 'dwconv7_dgrad')


@pytest.mark.parametrize('B,h,w,C', GEOMS)
def test_dwconv7_wgrad_fixed_order_partials(B, h, w, C):
    x, dy = _rand(B * h * w, C, seed=8), _rand(B * h * w, C, seed=9)
    part = ops.dwconv7_wgrad(x, dy, B, h, w, C)
    out = Guarded(1, C * 49, C * 49, torch.float32, DEV)
    ops.reduce_partials(part, out.view.view(-1), False)
    again = ops.reduce_partials(ops.dwconv7_wgrad(x, dy, B, h, w, C), torch.empty(C * 49, device=DEV), False)
    torch.cuda.synchronize()
    out.intact('dwconv7_wgrad')
    assert torch.equal(out.view.view(-1), again)                   # deterministic
    wd = torch.zeros(C, 1, 7, 7, dtype=torch.float64, device=DEV, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv2d(_nchw(x, B, h, w, C), wd, padding=3, groups=C), wd, _nchw(dy, B, h, w, C))
    (T,) = torch.autograd.grad(F.conv2d(_nchw(x, B, h, w, C).abs(), wd, padding=3, groups=C), wd, _nchw(dy, B, h, w, C).abs())
    # a sum of at most B h w products (FMA chains per workgroup, 4 row groups, then the rows of partials): any order of
    # n = B h w + 4 + nblk terms, gamma_n * sum |dy| |x|, plus the final rounding
    n = B * h * w + 4 + part.shape[0]
    bound = gamma(n) * T.reshape(1, -1) + ulp(torch.float32, ref.reshape(1, -1))
    assert_within(out.view, ref.reshape(1, -1), bound, 'dwconv7_wgrad')


RESIZES = [(1, 3, 4, 5, 4), (3, 1, 3, 4, 8), (1, 3, 3, 7, 16 / 3), (2, 7, 13, 3, 4), (1, 13, 37, 12, 8), (1, 37, 13, 2, 4), (1, 13, 7, 5, 37 / 13)]


def _resize_case(B, h, w, K, r, seed):
    H, W = int(round(h * r)), int(round(w * r))
    return H, W, _rand(B * h * w, K, seed=seed)


# nearest: the fp32 and fp64 source indices floor(dst * in / out) agree where in / out is a binary fraction (ratios 4, 8, 16/3)
RESIZE_FWD = [(c, m) for c in RESIZES for m in ('bilinear', 'nearest') if m == 'bilinear' or abs(c[4] * 3 - round(c[4] * 3)) < 1e-9]


@pytest.mark.parametrize('case,mode', RESIZE_FWD)
def test_resize_fwd(case, mode):
    B, h, w, K, r = case
    H, W, x = _resize_case(B, h, w, K, r, 10)
    out = _guarded((B, K * H * W))
    ops.resize_fwd(x, K, out.view, B, h, w, K, H, W, mode)
    torch.cuda.synchronize()
    out.intact('resize_fwd')
    ref = F.interpolate(_nchw(x, B, h, w, K), size=(H, W), mode=mode, **({'align_corners': False} if mode == 'bilinear' else {}))
    if mode == 'nearest':
        assert torch.equal(out.view.view(B, K, H, W).double(), ref)           # a copy
        return
    # the source coordinate scale (dst + 0.5) - 0.5 is computed in fp32 (scale rounded, one multiply, one subtract): its error and
    # the lambdas' is <= 4 u (max(h, w) + 2); a lambda error e moves the value by <= 2 e max|x|; the four products and three sums
    # add <= 8 u max|x|
    bound = (4 * U * (max(h, w) + 2) * 2 + 8 * U) * x.abs().max().double() + ulp(torch.float32, ref)
    assert_within(out.view.view(B, K, H, W), ref, bound, 'resize_fwd')


@pytest.mark.parametrize('mode', ['bilinear', 'nearest'])
@pytest.mark.parametrize('B,h,w,K,r', RESIZES)
def test_resize_bwd_gather(B, h, w, K, r, mode):
    H, W, _ = _resize_case(B, h, w, K, r, 11)
    g = _rand(B, K, H, W, seed=12)
    ld = (K + 7) // 8 * 8
    out = Guarded(B * h * w, ld, ld, torch.float32, DEV)
    ops.resize_bwd(g, out.view, ld, B, h, w, K, H, W, mode)
    again = ops.resize_bwd(g, torch.empty(B * h * w, ld, device=DEV), ld, B, h, w, K, H, W, mode)
    torch.cuda.synchronize()
    out.intact('resize_bwd')
    assert torch.equal(out.view, again)                            # fixed order
    assert not out.view[:, K:].any()                              # the operand padding is zero
    xd = torch.zeros(B, K, h, w, dtype=torch.float64, device=DEV, requires_grad=True)
    kw = {'align_corners': False} if mode == 'bilinear' else {}
    (ref,) = torch.autograd.grad(F.interpolate(xd, size=(H, W), mode=mode, **kw), xd, g.double())
    ref = ref.permute(0, 2, 3, 1).reshape(-1, K)
    # an element sums at most n = (2 H / h + 3)(2 W / w + 3) weighted terms, each |weight| <= 1 with an fp32 error <= 8 u (max(h, w) + 2)
    # (source index, as in the forward): (gamma_n + 8 u (max(h, w) + 2)) n max|g|, plus the final rounding
    n = (2 * math.ceil(H / h) + 3) * (2 * math.ceil(W / w) + 3)
    bound = (gamma(n) + 8 * U * (max(h, w) + 2)) * n * g.abs().max().double() + ulp(torch.float32, ref)
    if mode == 'nearest':
        bound = gamma(n) * n * g.abs().max().double() + ulp(torch.float32, ref)
    assert_within(out.view[:, :K], ref, bound, 'resize_bwd')


# ------------------------------------------------------------------------------------------------------- the head --
def _head_from_gold(gold, name):
    tasks, mode, p, C, K, depth, (NH, NW), D, B = HEADS[name]
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                              interpolate_mode=mode)
    head.init(dim_tokens_enc=D)
    pre = f'{name}/sd/'
    head.load_state_dict({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)})
    return head.to(DEV), input_info(tasks, NH * NW, 16 * NH, 16 * NW)


def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize('name', list(HEADS))
def test_head_fp32_matches_reference_golden(name):
    gold = np.load(GOLD)
    head, info = _head_from_gold(gold, name)
    x = torch.from_numpy(gold[f'{name}/x']).to(DEV).requires_grad_(True)
    with M.engine.precision('fp32'):
        y = head(x, info)
        (y * weight_like(y.cpu()).to(DEV)).sum().backward()
    assert y.shape == gold[f'{name}/y'].shape and y.is_contiguous()
    assert _rel(y, gold[f'{name}/y']) <= 1e-5, _rel(y, gold[f'{name}/y'])
    assert _rel(x.grad, gold[f'{name}/dx']) <= 1e-4
    N = info['tasks'][head.main_tasks[0]]['num_tokens']
    assert not x.grad[:, N * len(head.main_tasks):].any()           # the global token's row gets no gradient
    for n, p in head.named_parameters():
        assert _rel(p.grad, gold[f'{name}/grad/{n}']) <= 1e-4, (n, _rel(p.grad, gold[f'{name}/grad/{n}']))


def test_head_two_backward_passes_bit_equal():
    head = OA.ConvNeXtAdapter(num_classes=150, embed_dim=16 * 64, preds_per_patch=16, depth=2).to(DEV)
    head.init(64)
    head.to(DEV)
    info = input_info(('rgb',), 20, 64, 80)
    x = _rand(2, 21, 64, seed=13).requires_grad_(True)
    res = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        x.grad = None
        y = head(x, info)
        (y * weight_like(y.cpu()).to(DEV)).sum().backward()
        res.append([x.grad.clone()] + [p.grad.clone() for p in head.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _restate_fp64(head, x, info):
    """ConvNeXtAdapter.forward written out in fp64 from its parameters (not the reference's code)"""
    H, W = info['image_size']
    NH, NW = H // 16, W // 16
    s, C = int(round(head.preds_per_patch ** 0.5)), head.class_dim
    P = {k: v.double() for k, v in head.state_dict().items()}
    toks = torch.cat([x[:, info['tasks'][t]['start_idx']:info['tasks'][t]['end_idx']] for t in head.main_tasks], -1).double()
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
    return F.interpolate(z, size=(H, W), mode=head.interpolate_mode, **({'align_corners': False} if head.interpolate_mode == 'bilinear' else {}))


@pytest.mark.parametrize('name', ['head', 'rgbd_nearest', 'p9'])
def test_head_bf16_within_bf16_bounds_of_fp64(name):
    gold = np.load(GOLD)
    head, info = _head_from_gold(gold, name)
    x = torch.from_numpy(gold[f'{name}/x']).to(DEV)
    with torch.no_grad():
        y = head(x, info)
        ref = _restate_fp64(head, x, info)
    # bf16 operands (u = 2^-9 each side) in every GEMM: 2 + 2 depth products in a chain, the LayerNorm in front of each block
    # renormalises, so per block the relative error is <= 2 u_bf16 (operand roundings) + 4 u_bf16 (the bf16-stored LN output,
    # GELU output and its derivative); with the 2^-9 unit and depth <= 2: <= 0.05 of the output's scale (max |ref| per sample)
    scale = ref.abs().amax(dim=(1, 2, 3), keepdim=True)
    assert_within(y, ref, 0.05 * scale.expand_as(ref), f'{name} bf16')


def _layer_id(name, n):
    if name == 'global_tokens' or name.startswith('input_adapters'):
        return 0
    if name.startswith('encoder'):
        return int(name.split('.')[1]) + 1
    return n - 1


def test_multivit_with_head_fp32_forward_backward_and_one_step_match_golden():
    gold = np.load(GOLD)
    from test_convnext_head_cpu import build_vit
    model = build_vit()
    pre = 'vit/sd/'
    model.load_state_dict({k[len(pre):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(pre)})
    model = model.to(DEV)
    model.build_arena()
    with M.engine.precision('fp32'):
        x = torch.from_numpy(gold['vit/x']).to(DEV).requires_grad_(True)
        y = model({'rgb': x})['semseg']
        (y * weight_like(y.cpu()).to(DEV)).sum().backward()
        assert _rel(y, gold['vit/y']) <= 1e-5
        assert _rel(x.grad, gold['vit/dx']) <= 1e-4
        for n, p in model.named_parameters():
            if f'vit/grad/{n}' in gold.files:
                assert _rel(p.grad, gold[f'vit/grad/{n}']) <= 1e-4, n
        # one fine-tuning step: CrossEntropyLoss(ignore_index=255) + the grouped fused AdamW (run_finetuning_semseg.py:450-468)
        L = model.get_num_layers()
        values = [0.75 ** (L + 1 - i) for i in range(L + 2)]
        args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, momentum=0.9)
        opt = amd_loop.create_optimizer_groups(args, model, skip_list=model.no_weight_decay(),
                                               get_num_layer=lambda nm: _layer_id(nm, L + 2), get_layer_scale=lambda k: values[k])
        for grp in opt.param_groups:
            grp['lr'] = args.lr * grp.get('lr_scale', 1.0)
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        opt.zero_grad()
        logits = model({'rgb': torch.from_numpy(gold['step/x']).to(DEV)})['semseg']
        loss = F.cross_entropy(logits, torch.from_numpy(gold['step/target']).to(DEV), ignore_index=255)
        assert abs(loss.item() - float(gold['step/loss'][0])) <= 1e-5 * abs(float(gold['step/loss'][0]))
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        d_e = (p.detach() - before[n]).double().cpu()
        d_g = torch.from_numpy(gold[f'step/param/{n}']).double() - before[n].double().cpu()
        # the first AdamW update is ~ lr sign(g): an element whose gradient is at the fp32 noise level may flip
        assert float((d_e - d_g).norm()) <= 0.05 * float(d_g.norm()) + 1e-7, n


def test_ade20k_geometry_forward_backward_finite():
    """B = 2, 512 x 512, D = 768, embed_dim 6144, preds_per_patch 16 (C = 384 on a 128 x 128 map), depth 4, 150 classes, bf16"""
    torch.manual_seed(0)
    head = OA.ConvNeXtAdapter(num_classes=150, embed_dim=6144, preds_per_patch=16, depth=4)
    head.init(768)
    head = head.to(DEV)
    info = input_info(('rgb',), 32 * 32, 512, 512)
    x = (_rand(2, 1025, 768, seed=14) * 0.5).requires_grad_(True)
    y = head(x, info)
    assert y.shape == (2, 150, 512, 512)
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all()) and x.grad[:, :1024].abs().sum() > 0
    assert all(bool(torch.isfinite(p.grad).all()) for p in head.parameters())
