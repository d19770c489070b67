"""GPU: the implicit-GEMM 3 x 3 convolution (csrc/conv3x3_igemm.hip) -- forward and data gradient element by element against f64 on the
operands as the kernel sees them (bf16-rounded, ReLU applied: the reference of tests/test_fusion_blocks_gpu.py::_conv_case, with its
bounds), no halo across samples, the transposed weight bit for bit, run-to-run bits, and the dispatch behind
engine.set_conv3x3_impl('implicit') through functions.conv3x3_fwd / conv3x3_bwd, a residual unit and the DPT head."""
import contextlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from multimae_amd import _lib, engine, functions as Fn, ops, output_adapter_utils as OU
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dpt_fixture as DF  # noqa: E402

BF = torch.bfloat16
BIG = 1 << 40                                                    # a cap no test shape reaches: one chunk
TH, TW = ops.CONV3X3_IGEMM_TILE                                  # the kernel's own tile of output pixels
# the small maps, exactly one tile, a tile plus one in each direction, several tiles in both directions with a ragged edge
MAPS = [(1, 1), (2, 3), (7, 5), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW + 6)]
CHANNELS = [(32, 32), (96, 64), (64, 96)]                        # several K stages, several output-channel tiles; no power of two


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _seen(t):
    """an operand as the MFMA multiplies it: rounded to bf16; f64 on the CPU"""
    return t.bfloat16().double().cpu()


def _inside(t: torch.Tensor):
    """(Guarded, view): t as a 16-byte aligned view inside a larger allocation whose every other element is a NaN"""
    rows, cols = t.numel() // t.shape[-1], t.shape[-1]
    g = Guarded(rows, cols, cols, torch.float32, DEV, fill=t.reshape(rows, cols).to(DEV))
    v = g.view.view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return g, v


def _out(B, h, w, C):
    g = Guarded(B * h * w, C, C, torch.float32, DEV)                 # the view itself starts as NaNs: an unwritten element shows
    return g, g.view.view(B, h, w, C)


def fwd_ref(x, wt, b, r, relu):
    """(reference, bound) of the forward in f64: gamma(9 Cin + 2) (|a(x)| conv |w| + |bias| + |resid|) + ulp"""
    Cin = x.shape[-1]
    xn, ws = _nchw(_seen(F.relu(x) if relu else x)), _seen(wt)
    bd = None if b is None else b.double().cpu()
    ref = _nhwc(F.conv2d(xn, ws, bd, padding=1))
    mag = _nhwc(F.conv2d(xn.abs(), ws.abs(), None if bd is None else bd.abs(), padding=1))
    if r is not None:
        ref, mag = ref + r.double().cpu(), mag + r.double().abs().cpu()
    bound = gamma(9 * Cin + 2) * mag
    return ref, bound + ulp(torch.float32, ref.abs() + bound)


def dgrad_ref(dy, wt, xmask, add, Cin):
    """(reference, bound) of the data gradient in f64: gamma(9 Cout + 2) (|dy| conv^T |w|, masked, + |addend|) + ulp"""
    B, h, w, Cout = dy.shape
    dyn, ws = _nchw(_seen(dy)), _seen(wt)
    size = (B, Cin, h, w)
    ref = _nhwc(torch.nn.grad.conv2d_input(size, ws, dyn, padding=1))
    mag = _nhwc(torch.nn.grad.conv2d_input(size, ws.abs(), dyn.abs(), padding=1))
    if xmask is not None:
        ref, mag = ref * (xmask > 0).cpu(), mag * (xmask > 0).cpu()
    if add is not None:
        ref, mag = ref + add.double().cpu(), mag + add.double().abs().cpu()
    bound = gamma(9 * Cout + 2) * mag
    return ref, bound + ulp(torch.float32, ref.abs() + bound)


@contextlib.contextmanager
def impl(which):
    old = engine.conv3x3_impl()
    engine.set_conv3x3_impl(which)
    try:
        yield
    finally:
        engine.set_conv3x3_impl(old)


# ------------------------------------------------------------------------------------------ 1. element by element --
@pytest.mark.parametrize('Cin,Cout', CHANNELS)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('h,w', MAPS)
def test_forward_elementwise(h, w, B, Cin, Cout):
    """every combination of ReLU, bias and residual; the input inside a NaN-filled allocation, the output guarded"""
    x, wt = _rand(B, h, w, Cin, seed=1), _rand(Cout, Cin, 3, 3, seed=2, scale=0.2)
    b, r = _rand(Cout, seed=3), _rand(B, h, w, Cout, seed=4)
    gx, xv = _inside(x)
    wp = ops.conv3x3_weight_pack(wt.to(DEV), BF)
    bd, rd = b.to(DEV), r.to(DEV)
    for relu in (False, True):
        for bias in (False, True):
            for resid in (False, True):
                gy, y = _out(B, h, w, Cout)
                ops.conv3x3_igemm_fwd(xv, wp, bd if bias else None, rd if resid else None, y, B, h, w, Cin, Cout, relu)
                torch.cuda.synchronize()
                what = f'forward B{B} {h}x{w} {Cin}->{Cout} relu={relu} bias={bias} resid={resid}'
                gy.intact(what)
                gx.intact(what + ': the input allocation')
                assert torch.equal(xv.cpu(), x), what + ': the source map was modified'
                ref, bound = fwd_ref(x, wt, b if bias else None, r if resid else None, relu)
                assert_within(y, ref, bound, what, names=('b', 'y', 'x', 'c'))


@pytest.mark.parametrize('Cin,Cout', CHANNELS)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('h,w', MAPS)
def test_dgrad_elementwise(h, w, B, Cin, Cout):
    """every combination of ReLU mask and addend; dy inside a NaN-filled allocation, dx guarded"""
    dy, wt = _rand(B, h, w, Cout, seed=5), _rand(Cout, Cin, 3, 3, seed=6, scale=0.2)
    xm, add = _rand(B, h, w, Cin, seed=7), _rand(B, h, w, Cin, seed=8)
    gd, dyv = _inside(dy)
    wpt = ops.conv3x3_weight_pack_t(ops.conv3x3_weight_pack(wt.to(DEV), BF))
    xmd, addd = xm.to(DEV), add.to(DEV)
    for mask in (False, True):
        for addend in (False, True):
            gx, dx = _out(B, h, w, Cin)
            ops.conv3x3_igemm_dgrad(dyv, wpt, xmd if mask else None, addd if addend else None, dx, B, h, w, Cout, Cin)
            torch.cuda.synchronize()
            what = f'data gradient B{B} {h}x{w} {Cout}->{Cin} mask={mask} addend={addend}'
            gx.intact(what)
            gd.intact(what + ': the gradient allocation')
            assert torch.equal(dyv.cpu(), dy), what + ': dy was modified'
            ref, bound = dgrad_ref(dy, wt, xm if mask else None, add if addend else None, Cin)
            assert_within(dx, ref, bound, what, names=('b', 'y', 'x', 'c'))


# ------------------------------------------------------------------------------------------ 2. no halo across samples --
@pytest.mark.parametrize('h,w', [(2, 3), (TH + 1, TW + 1)])
def test_no_halo_across_samples(h, w):
    """sample b holds the constant b + 1, the weight is all ones: every output is (b + 1) C (taps inside the map), exactly"""
    B, C = 3, 32
    x = (torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1).expand(B, h, w, C)).contiguous().to(DEV)
    wp = ops.conv3x3_weight_pack(torch.ones(C, C, 3, 3, device=DEV), BF)
    ny = torch.tensor([min(i + 1, h - 1) - max(i - 1, 0) + 1 for i in range(h)], dtype=torch.float32)
    nx = torch.tensor([min(i + 1, w - 1) - max(i - 1, 0) + 1 for i in range(w)], dtype=torch.float32)
    want = (torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1) * C * (ny.view(1, h, 1, 1) * nx.view(1, 1, w, 1))).expand(B, h, w, C)
    y = ops.conv3x3_igemm_fwd(x, wp, None, None, torch.empty(B, h, w, C, device=DEV), B, h, w, C, C, False)
    dx = ops.conv3x3_igemm_dgrad(x, ops.conv3x3_weight_pack_t(wp), None, None, torch.empty(B, h, w, C, device=DEV), B, h, w, C, C)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want)
    assert torch.equal(dx.cpu(), want)


# ------------------------------------------------------------------------------------------ 3. the transposed weight --
def test_weight_pack_t_bit_exact():
    """wpt[c][(8 - t) Cout + o] = wp[o][t Cin + c] on a weight whose every element is another bit pattern"""
    Cout, Cin = 32, 96
    bits = torch.arange(Cout * 9 * Cin, dtype=torch.int32).to(torch.int16).view(Cout, 9 * Cin)
    wp = bits.view(BF).to(DEV)
    want = bits.view(Cout, 9, Cin).flip(1).permute(2, 1, 0).reshape(Cin, 9 * Cout)
    g = Guarded(Cin, 9 * Cout, 9 * Cout, BF, DEV)
    _lib.check(_lib.load().mmae_conv3x3_weight_pack_t(wp.data_ptr(), g.view.data_ptr(), Cout, Cin, ops._stream()), 'conv3x3_weight_pack_t')
    wpt = ops.conv3x3_weight_pack_t(wp)
    torch.cuda.synchronize()
    g.intact('conv3x3_weight_pack_t')
    assert wpt.shape == (Cin, 9 * Cout) and wpt.dtype == BF
    assert torch.equal(wpt.view(torch.int16).cpu(), want) and torch.equal(g.view.view(torch.int16).cpu(), want)
    assert torch.equal(wp.view(torch.int16).cpu(), bits)


def test_fragment_maps_with_integer_data():
    """exact small integers and an asymmetric weight (one non-zero tap, a value that depends on (o, c) asymmetrically): a swapped
    row / column or k order in the fragments gives another integer"""
    B, h, w, Cin, Cout = 1, TH + 1, TW + 1, 64, 96
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-3, 4, (B, h, w, Cin), generator=g).float()
    wt = torch.zeros(Cout, Cin, 3, 3)
    o, c = torch.arange(Cout).view(-1, 1), torch.arange(Cin).view(1, -1)
    wt[:, :, 0, 2] = ((3 * o + c) % 5 - 2).float()
    wt[:, :, 2, 1] = ((o + 2 * c) % 3 - 1).float()
    want = _nhwc(F.conv2d(_nchw(x).double(), wt.double(), padding=1))
    assert float(want.abs().max()) < 2 ** 20
    wp = ops.conv3x3_weight_pack(wt.to(DEV), BF)
    y = ops.conv3x3_igemm_fwd(x.to(DEV), wp, None, None, torch.empty(B, h, w, Cout, device=DEV), B, h, w, Cin, Cout, False)
    dy = torch.randint(-3, 4, (B, h, w, Cout), generator=g).float()
    dx = ops.conv3x3_igemm_dgrad(dy.to(DEV), ops.conv3x3_weight_pack_t(wp), None, None, torch.empty(B, h, w, Cin, device=DEV), B, h, w, Cout, Cin)
    want_dx = _nhwc(torch.nn.grad.conv2d_input((B, Cin, h, w), wt.double(), _nchw(dy).double(), padding=1))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), want)
    assert torch.equal(dx.cpu().double(), want_dx)


# ------------------------------------------------------------------------------------------ 4. two runs --
def test_two_runs_are_bit_equal():
    B, (h, w), (Cin, Cout) = 3, MAPS[-1], CHANNELS[1]
    x, dy = _rand(B, h, w, Cin, seed=1).to(DEV), _rand(B, h, w, Cout, seed=2).to(DEV)
    wp = ops.conv3x3_weight_pack(_rand(Cout, Cin, 3, 3, seed=3, scale=0.2).to(DEV), BF)
    wpt = ops.conv3x3_weight_pack_t(wp)
    b, r = _rand(Cout, seed=4).to(DEV), _rand(B, h, w, Cout, seed=5).to(DEV)
    runs = []
    for _ in range(2):
        y = ops.conv3x3_igemm_fwd(x, wp, b, r, torch.empty(B, h, w, Cout, device=DEV), B, h, w, Cin, Cout, True)
        dx = ops.conv3x3_igemm_dgrad(dy, wpt, x, x, torch.empty(B, h, w, Cin, device=DEV), B, h, w, Cout, Cin)
        runs.append((y, dx))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_entry_points_refuse_what_is_not_eligible():
    """the library itself refuses (and launches nothing for) channel counts off the grid of 32 and misaligned pointers"""
    lib = _lib.load()
    B, h, w = 1, 3, 3
    x, wp = torch.zeros(B * h * w * 32 + 4, device=DEV), torch.zeros(9 * 32 * 32, device=DEV, dtype=BF)
    gy = Guarded(B * h * w, 32, 32, torch.float32, DEV)
    y = gy.view.data_ptr()
    s = ops._stream()
    assert lib.mmae_conv3x3_igemm_fwd(x.data_ptr(), wp.data_ptr(), None, None, y, B, h, w, 24, 32, 0, s) != 0
    assert lib.mmae_conv3x3_igemm_fwd(x.data_ptr(), wp.data_ptr(), None, None, y, B, h, w, 32, 40, 0, s) != 0
    assert lib.mmae_conv3x3_igemm_fwd(x.data_ptr() + 4, wp.data_ptr(), None, None, y, B, h, w, 32, 32, 0, s) != 0
    assert lib.mmae_conv3x3_igemm_fwd(x.data_ptr(), wp.data_ptr(), None, x.data_ptr() + 4, y, B, h, w, 32, 32, 0, s) != 0
    assert lib.mmae_conv3x3_igemm_dgrad(x.data_ptr(), wp.data_ptr(), None, None, y, B, h, w, 32, 8, s) != 0
    assert lib.mmae_conv3x3_igemm_dgrad(x.data_ptr(), wp.data_ptr(), None, x.data_ptr() + 4, y, B, h, w, 32, 32, s) != 0
    assert b'16-byte' in lib.mmae_last_error()
    torch.cuda.synchronize()
    from helpers import assert_untouched
    assert_untouched(gy, 'a refused conv3x3_igemm call')


# ------------------------------------------------------------------------------------------ 5. dispatch --
class _Count:
    """counts the calls of some ops functions while it is active"""

    def __init__(self, *names):
        self.names, self.n, self.old = names, {k: 0 for k in names}, {}

    def __enter__(self):
        for k in self.names:
            self.old[k] = getattr(ops, k)

            def wrapped(*a, _k=k, **kw):
                self.n[_k] += 1
                return self.old[_k](*a, **kw)
            setattr(ops, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k in self.names:
            setattr(ops, k, self.old[k])


_CALLS = ('conv3x3_igemm_fwd', 'conv3x3_igemm_dgrad', 'conv3x3_weight_pack_t', 'conv3x3_im2col', 'conv3x3_col2im', 'linear_dw', 'linear_dx')


def test_dispatch_eligible_against_f64():
    B, h, w, Cin, Cout = 2, TH + 1, TW + 1, 64, 96
    x, wt = _rand(B, h, w, Cin, seed=21), _rand(Cout, Cin, 3, 3, seed=22, scale=0.2)
    b, r, dy, add = _rand(Cout, seed=23), _rand(B, h, w, Cout, seed=24), _rand(B, h, w, Cout, seed=25), _rand(B, h, w, Cin, seed=26)
    xd, dyd = x.to(DEV), dy.to(DEV)
    wp = ops.conv3x3_weight_pack(wt.to(DEV), BF)
    with impl('implicit'), _Count(*_CALLS) as cnt:
        y = Fn.conv3x3_fwd(xd, wp, b.to(DEV), 1, True, r.to(DEV), BIG)
        dx, dwp = Fn.conv3x3_bwd(dyd, xd, wp, 1, True, add.to(DEV), BIG, True, True)
        dx_only, none = Fn.conv3x3_bwd(dyd, xd, wp, 1, True, add.to(DEV), BIG, True, False)
    with impl('gather'):
        _, dwp_g = Fn.conv3x3_bwd(dyd, xd, wp, 1, True, add.to(DEV), BIG, True, True)
    torch.cuda.synchronize()
    assert cnt.n == {'conv3x3_igemm_fwd': 1, 'conv3x3_igemm_dgrad': 2, 'conv3x3_weight_pack_t': 2, 'conv3x3_im2col': 1, 'conv3x3_col2im': 0,
                     'linear_dw': 1, 'linear_dx': 0}
    assert none is None and torch.equal(dx, dx_only)
    assert torch.equal(xd.cpu(), x)
    assert_within(y, *fwd_ref(x, wt, b, r, True), 'conv3x3_fwd under implicit', names=('b', 'y', 'x', 'c'))
    assert_within(dx, *dgrad_ref(dy, wt, x, add, Cin), 'conv3x3_bwd under implicit', names=('b', 'y', 'x', 'c'))
    assert torch.equal(dwp, dwp_g), 'the weight gradient is the same launches on the same data'


def _both(run):
    """run() under 'gather' and under 'implicit': the two outcomes -- a tuple of tensors, or the error the call raised"""
    out = []
    for which in ('gather', 'implicit'):
        with impl(which), _Count('conv3x3_igemm_fwd', 'conv3x3_igemm_dgrad', 'conv3x3_weight_pack_t') as cnt:
            try:
                res = run()
            except (_lib.KernelError, ValueError) as e:
                res = (type(e), str(e))
        torch.cuda.synchronize()
        assert sum(cnt.n.values()) == 0, f'{which}: an ineligible convolution reached the implicit-GEMM entry points'
        out.append(res)
    return out


@pytest.mark.parametrize('case', ['8->8', 'stride 2', 'fp32', 'offset'])
def test_dispatch_ineligible_takes_the_gather_path(case):
    """8 -> 8 channels, stride 2, the fp32 mode and an input view 4 bytes off the 16-byte grid: under 'implicit' the outcome is the
    gather path's, bit for bit (for the misaligned view in bf16 mode that outcome is the bf16 gather's own refusal, in fp32 mode the
    element-wise gather's result: both are compared)"""
    B, h, w = 2, 5, 7
    C = 8 if case == '8->8' else 32
    stride = 2 if case == 'stride 2' else 1
    acts = [torch.float32] if case == 'fp32' else ([BF, torch.float32] if case == 'offset' else [BF])
    ho, wo = ops.conv_out_size(h, stride), ops.conv_out_size(w, stride)
    x = _rand(B, h, w, C, seed=31).to(DEV)
    if case == 'offset':
        x = torch.empty(x.numel() + 1, device=DEV)[1:].view(B, h, w, C).copy_(x)
        assert x.data_ptr() % 16 == 4
    wt = _rand(C, C, 3, 3, seed=32, scale=0.2).to(DEV)
    b, r = _rand(C, seed=33).to(DEV), _rand(B, ho, wo, C, seed=34).to(DEV)
    dy, add = _rand(B, ho, wo, C, seed=35).to(DEV), _rand(B, h, w, C, seed=36).to(DEV)
    for act in acts:
        wp = ops.conv3x3_weight_pack(wt, act)

        def run():
            y = Fn.conv3x3_fwd(x, wp, b, stride, True, r, BIG)
            dx, dwp = Fn.conv3x3_bwd(dy, x, wp, stride, True, add, BIG, True, True)
            return y, dx, dwp
        ga, im = _both(run)
        if isinstance(ga[0], type):
            assert case == 'offset' and act == BF and ga == im and '16-byte' in ga[1]
        else:
            assert all(torch.equal(p, q) for p, q in zip(ga, im)), (case, act)


# ------------------------------------------------------------------------------------------ 6. a chain --
def _rcu_run(which, direct, x, sd):
    m = OU.ResidualConvUnit_custom(32, nn.ReLU(False), False)
    m.load_state_dict(sd)
    m.to(DEV)
    if direct:
        engine.ParamArena(m).zero_grad()
    xd = x.to(DEV).requires_grad_(True)
    engine.set_direct_grads(direct)
    try:
        with impl(which), engine.precision('bf16'), _Count('conv3x3_igemm_fwd', 'conv3x3_igemm_dgrad') as cnt:
            y = m(xd)
            (y * torch.linspace(-1.0, 1.0, y.numel(), device=DEV).view(y.shape)).sum().backward()
    finally:
        engine.set_direct_grads(False)
    engine.join_wgrad_streams()
    torch.cuda.synchronize()
    assert cnt.n == ({'conv3x3_igemm_fwd': 2, 'conv3x3_igemm_dgrad': 2} if which == 'implicit' else {'conv3x3_igemm_fwd': 0, 'conv3x3_igemm_dgrad': 0})
    return y.detach().cpu(), xd.grad.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


def test_residual_unit_chain():
    """ResidualConvUnit_custom(32), 6 x 10, B = 2: y = conv2(relu(conv1(relu(x)))) + x under both settings.  Both first convolutions
    are within b1 of the exact t; the bf16 rounding of relu(t) can therefore differ by 2 b1 plus one bf16 spacing (2^-8 |t|); the
    second convolution is within b2 of the exact result on its own operands: |y_i - y_g| <= |w2| conv (2 b1 + 2^-8 |t|) + 2 b2."""
    B, C, h, w = 2, 32, 6, 10
    torch.manual_seed(5)
    ref = OU.ResidualConvUnit_custom(C, nn.ReLU(False), False)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    x = _rand(B, C, h, w, seed=41)
    yg, dxg, gg = _rcu_run('gather', False, x, sd)
    yi, dxi, gi = _rcu_run('implicit', False, x, sd)
    xh = _nhwc(x).contiguous()
    t, b1 = fwd_ref(xh, sd['conv1.weight'], sd['conv1.bias'], None, True)
    _, b2 = fwd_ref(t.float(), sd['conv2.weight'], sd['conv2.bias'], xh, True)
    w2 = _seen(sd['conv2.weight']).abs()
    bound = _nhwc(F.conv2d(_nchw(2 * b1 + 2.0 ** -8 * t.abs()), w2, padding=1)) + 2 * b2
    assert_within(_nhwc(yi), _nhwc(yg), bound, 'residual unit, implicit against gather', names=('b', 'y', 'x', 'c'))
    assert torch.isfinite(dxi).all() and dxi.shape == dxg.shape
    # both gradient modes under 'implicit'
    yd, dxd, gd = _rcu_run('implicit', True, x, sd)
    assert torch.equal(yi, yd) and torch.equal(dxi, dxd)
    assert sorted(gi) == sorted(gd) and len(gi) == 4
    for k in gi:
        assert torch.equal(gi[k], gd[k]), k


# ------------------------------------------------------------------------------------------ 7. the DPT head --
def _head_run(which):
    K, tasks, D, (NH, NW) = DF.CASES['r1']
    head = DF.seeded_head('r1').to(DEV)
    toks = [t.to(DEV).requires_grad_(True) for t in DF.tokens('r1')]
    with impl(which), engine.precision('bf16'), _Count('conv3x3_igemm_fwd', 'conv3x3_igemm_dgrad') as cnt:
        y = head(toks, DF.case_info('r1'))
        (y * DF.weight_like(y.detach().cpu()).to(DEV)).sum().backward()
    engine.join_wgrad_streams()
    torch.cuda.synchronize()
    assert sum(cnt.n.values()) == 0                                  # 8 .. 32 channels: not one convolution is eligible
    return y.detach().cpu(), [t.grad.detach().cpu() for t in toks]


def test_dpt_head_falls_back_silently():
    """the fixture head's channel counts are ineligible: all ten nodes run the gather path under 'implicit', bit for bit"""
    (ya, da), (yb, db) = _head_run('gather'), _head_run('implicit')
    assert torch.equal(ya, yb) and len(da) == len(db) == 4
    for a, b in zip(da, db):
        assert torch.equal(a, b)
