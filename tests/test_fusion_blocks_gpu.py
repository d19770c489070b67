"""GPU: dense 3 x 3 convolutions, the align-corners x2 upsample and the RefineNet fusion blocks of the DPT head (csrc/conv3x3.hip,
multimae_amd/output_adapter_utils.py).  The gathers bit for bit in guarded buffers; the convolution (forward, data and weight
gradient) element by element against an f64 F.conv2d of the operands as the kernels see them, at the smallest maps that can still
go wrong, with the batch in chunks; the upsample against torch's CPU f32; the blocks against the reference's recorded f64 values
(tests/golden/fusion_blocks.npz), the engine's deviation measured against the reference's own f32 / autocast-bf16 deviation.

Measured on an MI355X (engine deviation / reference deviation, the largest ratio over the 54 tensors of both fixture cases):
fp32 mode 2.14 of the 4 allowed (grad out_conv.weight, c16, two inputs), bf16 mode 1.47 of the 2 allowed (grad resConfUnit2.conv1.bias,
c8, two inputs) -- profiles/fusion_block_bench.json holds all 108."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from multimae_amd import engine, functions as Fn, ops, output_adapter_utils as OU
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from make_golden_fusion import CASES  # noqa: E402
import fusion_oracle as FO  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden', 'fusion_blocks.npz')
U32 = 2.0 ** -24
BIG = 1 << 40                                                    # a cap no test shape reaches: one chunk

# (h, w, stride): 1 x 1 -- only the centre tap is real; odd sizes; non-square; stride 2 on odd and on even sizes (ho rounds differently)
MAPS = [(1, 1, 1), (5, 7, 1), (9, 6, 1), (5, 7, 2), (6, 6, 2)]
CHANNELS = [('bf16', 8, 8), ('bf16', 8, 40), ('bf16', 24, 8), ('bf16', 24, 40), ('fp32', 3, 5)]
SWITCHES = [(r, b, s) for r in (False, True) for b in (False, True) for s in (False, True)]        # ReLU, bias, residual


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _act(mode):
    return torch.bfloat16 if mode == 'bf16' else torch.float32


def _seen(t, mode):
    """an operand as the GEMM multiplies it: rounded to bf16 in bf16 mode, as it is in fp32 mode; f64 on the CPU"""
    return (t.bfloat16() if mode == 'bf16' else t).double().cpu()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _windows(x_nchw, stride, ho, wo):
    """[B, ho, wo, 9, C]: the 3 x 3 window of every output pixel in (ky, kx) order, zeros outside the map (copies only)"""
    xp = F.pad(x_nchw, (1, 1, 1, 1))
    taps = [xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]
    return torch.stack([_nhwc(t) for t in taps], dim=3)


# ------------------------------------------------------------------------------------------------------ the gathers --
@pytest.mark.parametrize('h,w,stride', MAPS)
@pytest.mark.parametrize('mode,C', [('bf16', 8), ('bf16', 24), ('fp32', 3), ('fp32', 8)])
@pytest.mark.parametrize('relu', [False, True])
def test_im2col_bit_exact(h, w, stride, mode, C, relu):
    """rows of 9 C columns in (ky, kx, c) order, zeros at padded taps, the ReLU on the fly, the source untouched, nothing written
    outside the rows"""
    B = 2
    ho, wo = ops.conv_out_size(h, stride), ops.conv_out_size(w, stride)
    x = _rand(B, h, w, C, seed=1)
    keep = x.clone()
    col = Guarded(B * ho * wo, 9 * C, 9 * C, _act(mode), DEV)
    ops.conv3x3_im2col(x, col.view, B, h, w, C, stride, relu)
    torch.cuda.synchronize()
    col.intact('im2col')
    assert torch.equal(x, keep)
    ref = _windows(_nchw(F.relu(x) if relu else x), stride, ho, wo).reshape(B * ho * wo, 9 * C).to(_act(mode))
    assert torch.equal(col.view.contiguous().view(torch.int16 if mode == 'bf16' else torch.int32),
                       ref.contiguous().view(torch.int16 if mode == 'bf16' else torch.int32))


@pytest.mark.parametrize('h,w,stride', MAPS)
@pytest.mark.parametrize('C', [3, 8])
@pytest.mark.parametrize('mask,addend', [(False, False), (True, True)])
def test_col2im_gather(h, w, stride, C, mask, addend):
    """every input pixel sums its (at most nine) taps in a fixed order: within gamma(9 + 1) of the f64 sum, bit-equal from run to run"""
    B = 2
    ho, wo = ops.conv_out_size(h, stride), ops.conv_out_size(w, stride)
    dcol = _rand(B * ho * wo, 9 * C, seed=2)
    x = _rand(B, h, w, C, seed=3)
    add = _rand(B, h, w, C, seed=4)
    out = Guarded(B * h * w, C, C, torch.float32, DEV)
    args = (x if mask else None, add if addend else None)
    ops.conv3x3_col2im(dcol, *args, out.view, B, h, w, C, stride)
    again = ops.conv3x3_col2im(dcol, *args, torch.empty(B * h * w, C, device=DEV), B, h, w, C, stride)
    torch.cuda.synchronize()
    out.intact('col2im')
    assert torch.equal(out.view, again)
    # the transpose of the window gather, by autograd in f64
    xd = torch.zeros(B, C, h, w, dtype=torch.float64, device=DEV, requires_grad=True)
    win = _windows(xd, stride, ho, wo).reshape(B * ho * wo, 9 * C)
    (ref,) = torch.autograd.grad(win, xd, dcol.double())
    (mag,) = torch.autograd.grad(win, xd, dcol.double().abs())
    ref, mag = _nhwc(ref), _nhwc(mag)
    if mask:
        ref, mag = ref * (x > 0), mag * (x > 0)
    if addend:
        ref, mag = ref + add.double(), mag + add.double().abs()
    bound = gamma(10) * mag
    assert_within(out.view.view(B, h, w, C), ref, bound + ulp(torch.float32, ref.abs() + bound), 'col2im', names=('b', 'y', 'x', 'c'))


@pytest.mark.parametrize('Cout,Cin', [(8, 8), (5, 3), (40, 24)])
def test_weight_layouts_bit_exact(Cout, Cin):
    w = _rand(Cout, Cin, 3, 3, seed=5)
    ref = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)
    assert torch.equal(ops.conv3x3_weight_pack(w, torch.float32), ref)
    assert torch.equal(ops.conv3x3_weight_pack(w, torch.bfloat16).view(torch.int16), ref.bfloat16().contiguous().view(torch.int16))
    g = _rand(Cout, 9 * Cin, seed=6)
    back = g.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
    dst = Guarded(Cout, Cin * 9, Cin * 9, torch.float32, DEV)
    ops.conv3x3_weight_unpack(g, dst.view.view(Cout, Cin, 3, 3), False)
    acc = w.clone()
    ops.conv3x3_weight_unpack(g, acc, True)
    torch.cuda.synchronize()
    dst.intact('weight_unpack')
    assert torch.equal(dst.view.view(Cout, Cin, 3, 3), back) and torch.equal(acc, w + back)


@pytest.mark.parametrize('h,w,stride', [(5, 7, 1), (6, 6, 2)])
def test_gathers_on_pointers_off_the_16_byte_grid(h, w, stride):
    """C % 4 == 0 with a pointer that is not 16-byte aligned takes the element-wise kernels and gives the same bits; the bf16 gather,
    which has only the 16-byte form, refuses such a pointer"""
    from multimae_amd import _lib
    B, C = 2, 8
    ho, wo = ops.conv_out_size(h, stride), ops.conv_out_size(w, stride)
    x = _rand(B, h, w, C, seed=1)
    x_off = torch.empty(x.numel() + 1, device=DEV)[1:].view(B, h, w, C).copy_(x)
    assert x_off.data_ptr() % 16 == 4
    ref = torch.empty(B * ho * wo, 9 * C, device=DEV)
    ops.conv3x3_im2col(x, ref, B, h, w, C, stride, True)
    for src, shift in ((x, 1), (x_off, 0), (x_off, 3)):
        col = Guarded(B * ho * wo, 9 * C, 9 * C, torch.float32, DEV, shift=shift)
        ops.conv3x3_im2col(src, col.view, B, h, w, C, stride, True)
        torch.cuda.synchronize()
        col.intact('im2col, unaligned')
        assert torch.equal(col.view, ref)
    col16 = Guarded(B * ho * wo, 9 * C, 9 * C, torch.bfloat16, DEV, shift=1)
    with pytest.raises(_lib.KernelError, match='16-byte'):
        ops.conv3x3_im2col(x, col16.view, B, h, w, C, stride, False)
    with pytest.raises(_lib.KernelError, match='16-byte'):
        ops.conv3x3_im2col(x_off, torch.empty(B * ho * wo, 9 * C, device=DEV, dtype=torch.bfloat16), B, h, w, C, stride, False)
    torch.cuda.synchronize()
    col16.intact('refused im2col')
    dcol, add = _rand(B * ho * wo, 9 * C, seed=2), _rand(B, h, w, C, seed=4)
    want = ops.conv3x3_col2im(dcol, x, add, torch.empty(B, h, w, C, device=DEV), B, h, w, C, stride)
    for mask, shift in ((x, 1), (x_off, 0), (x_off, 2)):
        out = Guarded(B * h * w, C, C, torch.float32, DEV, shift=shift)
        ops.conv3x3_col2im(dcol, mask, add, out.view, B, h, w, C, stride)
        torch.cuda.synchronize()
        out.intact('col2im, unaligned')
        assert torch.equal(out.view.view(B, h, w, C), want)
    up, g = ops.upsample2x_fwd(x, B, h, w, C), _rand(B, 2 * h, 2 * w, C, seed=8)
    down = ops.upsample2x_bwd(g, B, h, w, C)
    y = Guarded(B * 4 * h * w, C, C, torch.float32, DEV, shift=1)
    _lib.check(_lib.load().mmae_upsample2x_fwd(x_off.data_ptr(), y.view.data_ptr(), B, h, w, C, ops._stream()), 'upsample2x_fwd')
    dx = Guarded(B * h * w, C, C, torch.float32, DEV, shift=1)
    _lib.check(_lib.load().mmae_upsample2x_bwd(g.data_ptr(), dx.view.data_ptr(), B, h, w, C, ops._stream()), 'upsample2x_bwd')
    torch.cuda.synchronize()
    y.intact('upsample2x_fwd, unaligned')
    dx.intact('upsample2x_bwd, unaligned')
    # the 4-wide and the element-wise forms contract the same expressions per lane; compared within the forward's own bound
    assert_within(y.view.view(B, 2 * h, 2 * w, C), up, 8 * U32 * float(x.abs().max()), 'upsample2x_fwd, unaligned')
    n = _window(h) * _window(w)
    assert_within(dx.view.view(B, h, w, C), down, gamma(n) * n * float(g.abs().max()) + ulp(torch.float32, down), 'upsample2x_bwd, unaligned')


# --------------------------------------------------------------------------------------------------- the convolution --
def _conv_case(mode, B, h, w, stride, Cin, Cout, relu, bias, resid, cap, seed):
    """forward, data gradient and weight gradient of one convolution against f64 on the operands as the GEMM sees them:
      forward  gamma(9 Cin + 2) (|x| conv |w| + |b| + |resid|) + ulp     9 Cin products summed in fp32 in any order, bias, residual
      dx       gamma(9 Cout + 2) (|dy| conv^T |w| (masked) + |addend|) + ulp      nine taps of Cout products each, the addend
      dw       gamma(B ho wo) (|x|^T |dy|) + ulp                         one term per output pixel of the batch, chunks included"""
    act = _act(mode)
    ho, wo = ops.conv_out_size(h, stride), ops.conv_out_size(w, stride)
    x = _rand(B, h, w, Cin, seed=seed)
    wt = _rand(Cout, Cin, 3, 3, seed=seed + 1, scale=0.2)
    b = _rand(Cout, seed=seed + 2) if bias else None
    r = _rand(B, ho, wo, Cout, seed=seed + 3) if resid else None
    dy = _rand(B, ho, wo, Cout, seed=seed + 4)
    add = _rand(B, h, w, Cin, seed=seed + 5) if resid else None
    keep = x.clone()
    wp = ops.conv3x3_weight_pack(wt, act)
    y = Fn.conv3x3_fwd(x, wp, b, stride, relu, r, cap)
    dx, dwp = Fn.conv3x3_bwd(dy, x, wp, stride, relu, add, cap, True, True)
    dw = ops.conv3x3_weight_unpack(dwp, torch.empty_like(wt), False)
    torch.cuda.synchronize()
    assert torch.equal(x, keep), 'the source map was modified'
    xs = _seen(F.relu(x) if relu else x, mode)
    ws, dys = _seen(wt, mode), _seen(dy, mode)
    xn, dyn = _nchw(xs), _nchw(dys)
    what = f'{mode} B{B} {h}x{w}/{stride} {Cin}->{Cout} relu={relu} bias={bias} resid={resid}'
    # forward
    bd = None if b is None else b.double().cpu()
    ref = _nhwc(F.conv2d(xn, ws, bd, stride=stride, padding=1))
    mag = _nhwc(F.conv2d(xn.abs(), ws.abs(), None if bd is None else bd.abs(), stride=stride, padding=1))
    if resid:
        ref, mag = ref + r.double().cpu(), mag + r.double().abs().cpu()
    bound = gamma(9 * Cin + 2) * mag
    assert_within(y, ref, bound + ulp(torch.float32, ref.abs() + bound), 'forward ' + what, names=('b', 'y', 'x', 'c'))
    # data gradient
    size = (B, Cin, h, w)
    ref = _nhwc(torch.nn.grad.conv2d_input(size, ws, dyn, stride=stride, padding=1))
    mag = _nhwc(torch.nn.grad.conv2d_input(size, ws.abs(), dyn.abs(), stride=stride, padding=1))
    if relu:
        ref, mag = ref * (x > 0).cpu(), mag * (x > 0).cpu()
    if resid:
        ref, mag = ref + add.double().cpu(), mag + add.double().abs().cpu()
    bound = gamma(9 * Cout + 2) * mag
    assert_within(dx, ref, bound + ulp(torch.float32, ref.abs() + bound), 'data gradient ' + what, names=('b', 'y', 'x', 'c'))
    # weight gradient
    ref = torch.nn.grad.conv2d_weight(xn, tuple(wt.shape), dyn, stride=stride, padding=1)
    mag = torch.nn.grad.conv2d_weight(xn.abs(), tuple(wt.shape), dyn.abs(), stride=stride, padding=1)
    bound = gamma(B * ho * wo) * mag
    assert_within(dw, ref, bound + ulp(torch.float32, ref.abs() + bound), 'weight gradient ' + what, names=('o', 'c', 'ky', 'kx'))


@pytest.mark.parametrize('h,w,stride', MAPS)
@pytest.mark.parametrize('mode,Cin,Cout', CHANNELS)
def test_conv3x3_elementwise(h, w, stride, mode, Cin, Cout):
    """B = 2, every combination of ReLU, bias and residual"""
    for i, (relu, bias, resid) in enumerate(SWITCHES):
        _conv_case(mode, 2, h, w, stride, Cin, Cout, relu, bias, resid, BIG, 20 + 7 * i)


@pytest.mark.parametrize('mode,Cin,Cout', [('bf16', 8, 8), ('fp32', 3, 5)])
@pytest.mark.parametrize('stride', [1, 2])
def test_conv3x3_chunked(mode, Cin, Cout, stride):
    """B = 5 with a cap that holds two samples of gathered rows: three chunks, the last one short, in the forward (rows in the
    activation type) and in the backward (its f32 dY x W rows decide)"""
    h, w = 5, 7
    R1, K9 = ops.conv_out_size(h, stride) * ops.conv_out_size(w, stride), 9 * Cin
    esz = 2 if mode == 'bf16' else 4
    caps = (2 * R1 * K9 * esz, 2 * R1 * K9 * 4 + 3)               # two samples of forward rows; two samples (and a bit) of backward rows
    assert Fn._col_rows(5, R1, K9, esz, caps[0]) == 2 and Fn._col_rows(5, R1, K9, 4, caps[1]) == 2
    for cap in caps:
        _conv_case(mode, 5, h, w, stride, Cin, Cout, True, True, True, cap, 90)


def test_conv3x3_module_refuses_a_wrong_channel_count():
    """more channels than the weight was built for would overrun the gathered rows: refused like nn.Conv2d refuses it"""
    conv = OU.Conv3x3(8, 8).to(DEV)
    for mode in ('fp32', 'bf16'):
        with engine.precision(mode), pytest.raises(ValueError, match='shape'):
            conv(torch.zeros(2, 16, 4, 4, device=DEV))
    torch.cuda.synchronize()


def test_conv3x3_module_refuses_odd_channels_in_bf16():
    conv = OU.Conv3x3(12, 8).to(DEV)
    with engine.precision('bf16'), pytest.raises(ValueError, match='multiples of 8'):
        conv(torch.zeros(1, 12, 4, 4, device=DEV))
    with engine.precision('fp32'):
        assert conv(torch.zeros(1, 12, 4, 4, device=DEV)).shape == (1, 8, 4, 4)


# -------------------------------------------------------------------------------------------------------- upsample --
def _window(n_in):
    """largest number of outputs of the x2 align-corners map that read one input index (PyTorch's index formula in f32)"""
    n_out = 2 * n_in
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    cnt = np.zeros(n_in, dtype=np.int64)
    for o in range(n_out):
        i0 = min(int(np.float32(scale * np.float32(o))), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        cnt[i0] += 1
        if i1 != i0:
            cnt[i1] += 1
    return int(cnt.max())


@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (7, 7)])
@pytest.mark.parametrize('C', [3, 8])
def test_upsample2x_against_torch(h, w, C):
    B = 2
    x = _rand(B, h, w, C, seed=7)
    g = _rand(B, 2 * h, 2 * w, C, seed=8)
    y = Guarded(B * 4 * h * w, C, C, torch.float32, DEV)
    from multimae_amd import _lib
    _lib.check(_lib.load().mmae_upsample2x_fwd(x.data_ptr(), y.view.data_ptr(), B, h, w, C, ops._stream()), 'upsample2x_fwd')
    dx = Guarded(B * h * w, C, C, torch.float32, DEV)
    _lib.check(_lib.load().mmae_upsample2x_bwd(g.data_ptr(), dx.view.data_ptr(), B, h, w, C, ops._stream()), 'upsample2x_bwd')
    again = ops.upsample2x_bwd(g, B, h, w, C)
    torch.cuda.synchronize()
    y.intact('upsample2x_fwd')
    dx.intact('upsample2x_bwd')
    assert torch.equal(dx.view.view(B, h, w, C), again)                  # fixed order
    xc = _nchw(x).cpu().contiguous().requires_grad_(True)
    ref = F.interpolate(xc, scale_factor=2, mode='bilinear', align_corners=True)
    (dref,) = torch.autograd.grad(ref, xc, _nchw(g).cpu().contiguous())
    # a convex combination of four values with at most seven roundings
    assert_within(y.view.view(B, 2 * h, 2 * w, C), _nhwc(ref.detach()), 8 * U32 * float(x.abs().max()), 'upsample2x_fwd', names=('b', 'y', 'x', 'c'))
    n = _window(h) * _window(w)
    dref = _nhwc(dref)
    assert_within(dx.view.view(B, h, w, C), dref, gamma(n) * n * float(g.abs().max()) + ulp(torch.float32, dref), 'upsample2x_bwd',
                  names=('b', 'y', 'x', 'c'))
    if h == 1 and w == 1:                                                # a one-pixel input is replicated
        assert torch.equal(y.view.view(B, 4, C), x.view(B, 1, C).expand(B, 4, C))


# ---------------------------------------------------------------------------------------------------------- blocks --
_GOLD = {}


def gold():
    if 'z' not in _GOLD:
        _GOLD['z'] = np.load(GOLD)
    return _GOLD['z']


def _gold_sd(prefix):
    z = gold()
    return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def _engine_run(name, which, mode, direct=False, channels_last=False):
    """the engine's forward + backward of one fixture block on the GPU: (y, [dx], {name: grad}) as CPU f64"""
    z = gold()
    f = CASES[name][0]
    kind = 'rcu' if which == 'rcu' else 'ffb'
    m = OU.ResidualConvUnit_custom(f, nn.ReLU(False), False) if kind == 'rcu' else OU.make_fusion_block(f, False)
    m.load_state_dict(_gold_sd(f'{name}/{kind}/sd/'))
    m.to(DEV)
    if direct:
        arena = engine.ParamArena(m)
        arena.zero_grad()
    xs = [torch.from_numpy(z[f'{name}/x0'])] + ([torch.from_numpy(z[f'{name}/x1'])] if which == 'ffb2' else [])
    xs = [x.to(DEV) for x in xs]
    if channels_last:
        xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
    xs = [x.requires_grad_(True) for x in xs]
    engine.set_direct_grads(direct)
    try:
        with engine.precision(mode):
            y = m(*xs)
            (y * FO.weight_like(y)).sum().backward()
    finally:
        engine.set_direct_grads(False)
    engine.join_wgrad_streams()
    torch.cuda.synchronize()
    assert y.shape[1] == f and y.is_contiguous(memory_format=torch.channels_last)
    grads = {n: p.grad.detach().cpu().double().clone() for n, p in m.named_parameters() if p.grad is not None and (which != 'ffb1' or 'resConfUnit1' not in n)}
    return y.detach().cpu().double(), [x.grad.detach().cpu().double() for x in xs], grads


def _tensors(name, which, prec):
    """the fixture's tensors of one block in one precision as f64: {'y', 'dx0', ['dx1',] 'grad/<param>'}"""
    z = gold()
    pre = f'{name}/{which}/{prec}/'
    return {k[len(pre):]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith(pre)}


def _deviation_ratios(name, which, mode):
    """per tensor: (engine deviation from f64) / (reference deviation from f64), both as max-abs over the f64 tensor's max-abs"""
    y, dxs, grads = _engine_run(name, which, mode)
    mine = {'y': y, **{f'dx{i}': d for i, d in enumerate(dxs)}, **{'grad/' + n: g for n, g in grads.items()}}
    f64, ref = _tensors(name, which, 'f64'), _tensors(name, which, 'f32' if mode == 'fp32' else 'bf16')
    assert sorted(mine) == sorted(f64) == sorted(ref)
    out = {}
    for k, t64 in f64.items():
        scale = float(t64.abs().max())
        out[k] = (float((mine[k] - t64).abs().max()) / scale, float((ref[k] - t64).abs().max()) / scale)
    return out


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('which', ['rcu', 'ffb1', 'ffb2'])
@pytest.mark.parametrize('mode,allowed', [('fp32', 4.0), ('bf16', 2.0)])
def test_blocks_against_the_reference(name, which, mode, allowed):
    """fp32 mode: the engine's deviation from the f64 values is at most four times the reference's own f32 deviation (another summation
    order -- GEMM tiles against a direct convolution -- over the same number of operations).  bf16 mode: at most twice the deviation of
    the reference under torch.autocast(bfloat16) (the engine rounds the gathered activations once, autocast inputs and outputs)."""
    ratios = _deviation_ratios(name, which, mode)
    for k, (mine, ref) in ratios.items():
        print(f'FUSION_RATIO {json.dumps(dict(case=name, block=which, mode=mode, tensor=k, engine=mine, reference=ref, ratio=mine / ref if ref > 0 else None))}')
    bad = {k: v for k, v in ratios.items() if not v[0] <= allowed * v[1]}
    assert not bad, f'{name}/{which} {mode}: engine deviation above {allowed} x the reference deviation: {bad}'


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_both_gradient_modes_give_the_same_gradients(mode):
    """gradients returned to autograd and gradients accumulated into a zeroed gradient arena (engine.set_direct_grads) are the same
    numbers; an input that is already channels-last gives the same results as a contiguous one"""
    y0, dx0, g0 = _engine_run('c16', 'ffb2', mode, direct=False)
    y1, dx1, g1 = _engine_run('c16', 'ffb2', mode, direct=True, channels_last=True)
    assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(dx0, dx1))
    assert sorted(g0) == sorted(g1) and len(g0) == 10
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_two_passes_are_bit_equal(mode):
    a = _engine_run('c16', 'ffb2', mode)
    b = _engine_run('c16', 'ffb2', mode)
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_restatement_at_a_shape_the_fixture_does_not_hold():
    """the fusion block on a 7 x 5 map with 24 channels, B = 3, one sample per chunk, fp32 mode, against the tests' restatement: the same
    criterion as the fixture cases -- per tensor, the engine's deviation from the f64 restatement is at most four times the deviation
    of the f32 restatement (which is the reference bit for bit, tests/test_fusion_blocks_cpu.py)"""
    torch.manual_seed(5)
    m = OU.make_fusion_block(24, False).to(DEV)
    x0, x1 = _rand(3, 24, 7, 5, seed=11).requires_grad_(True), _rand(3, 24, 7, 5, seed=12).requires_grad_(True)
    old = OU.set_col_workspace_bytes(7 * 5 * 9 * 24 * 4)
    try:
        with engine.precision('fp32'):
            y = m(x0, x1)
            (y * FO.weight_like(y)).sum().backward()
    finally:
        OU.set_col_workspace_bytes(old)
    torch.cuda.synchronize()
    ry, rdx, rg = FO.run(FO.fusion, [x0, x1], m.state_dict(), torch.float64)
    sy, sdx, sg = FO.run(FO.fusion, [x0, x1], m.state_dict(), torch.float32)
    pairs = [('y', y, ry, sy), ('dx0', x0.grad, rdx[0], sdx[0]), ('dx1', x1.grad, rdx[1], sdx[1])]
    pairs += [(n, p.grad, rg[n], sg[n]) for n, p in m.named_parameters()]
    for k, mine, ref, f32 in pairs:
        dev, allowed = float((mine.detach().cpu().double() - ref).abs().max()), 4.0 * float((f32.double() - ref).abs().max())
        assert dev <= allowed, (k, dev, allowed)
