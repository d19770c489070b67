"""GPU: the DPT head (csrc/dpt.hip, functions.DPTReassembleFn / DPTHeadFn, output_adapters.DPTOutputAdapter).  The regression tail
kernel forward and backward element by element against f64 in guarded buffers; the transposed convolutions' weight layouts bit for
bit and the layer end to end (rows -> GEMM -> pixel shuffle) against an f64 F.conv_transpose2d of the operands as the GEMM sees
them; the whole head and a tiny MultiViT with it against the reference's recorded f64 values (tests/golden/dpt_head_<case>.npz),
the engine's deviation measured against the reference's own f32 / autocast-bf16 deviation.

The tail's backward works in tiles of 128 pixels, one workgroup per tile up to 2048 workgroups: the 3 x 37 x 29 map has 3219 pixels =
26 workgroups with a ragged last one; 1 x 520 x 520 = 270400 pixels is the smallest square map at which workgroups walk more than one
tile (2113 tiles)."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import multimae_amd as M
from multimae_amd import engine, functions as Fn, ops, output_adapter_utils as OU, output_adapters as OA
from multimae_amd.optim import FusedAdamW
from helpers import Guarded, assert_within, gamma, ulp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dpt_fixture as DF  # noqa: E402
from dpt_fixture import B, CASES, GEOM, UNUSED, VIT  # noqa: E402

F32 = torch.float32
TAIL_MAPS = [(1, 1, 1), (2, 5, 7), (3, 37, 29)]
TAIL_KC = [(K, C) for K in (1, 3, 16) for C in (32, 8)]
ALLOWED = {'fp32': 4.0, 'bf16': 5.0}        # engine deviation / reference deviation, see test_head_against_the_reference
TAIL_CASES = [(K, C, m) for K, C in TAIL_KC for m in TAIL_MAPS] + [(3, 32, (1, 520, 520))]


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _act(mode):
    return torch.bfloat16 if mode == 'bf16' else F32


def _seen(t, mode):
    """an operand as the GEMM multiplies it: rounded to bf16 in bf16 mode, as it is in fp32 mode; f64"""
    return (t.bfloat16() if mode == 'bf16' else t).double()


# ------------------------------------------------------------------------------------------------------------ the tail --
@pytest.mark.parametrize('K,C,geom', TAIL_CASES)
def test_tail_forward(K, C, geom):
    """out[b, k, p] = bias[k] + sum_c w[k, c] max(x[b, p, c], 0): C products and C additions in f32, so within gamma(C + 1) of the sum
    of magnitudes plus the rounding of the result; NCHW output in a guarded buffer, x untouched"""
    Bn, H, W = geom
    x, w, b = _rand(Bn, H, W, C, seed=1), _rand(K, C, seed=2), _rand(K, seed=3)
    keep = x.clone()
    out = Guarded(Bn * K, H * W, H * W, F32, DEV)
    ops.dpt_tail_fwd(x, w, b, out=out.view)
    torch.cuda.synchronize()
    out.intact('dpt_tail_fwd')
    assert torch.equal(x, keep)
    r = F.relu(x).double().view(-1, C)
    ref = (r @ w.double().t() + b.double()).view(Bn, H * W, K).permute(0, 2, 1)
    mag = (r @ w.double().abs().t() + b.double().abs()).view(Bn, H * W, K).permute(0, 2, 1)
    assert_within(out.view.view(Bn, K, H * W), ref, gamma(C + 1) * mag + ulp(F32, ref), 'dpt_tail_fwd', names=('b', 'k', 'p'))
    assert torch.equal(ops.dpt_tail_fwd(x, w, b).view(Bn * K, H * W), out.view)


@pytest.mark.parametrize('K,C,geom', TAIL_CASES)
def test_tail_backward(K, C, geom):
    """dx = (x > 0) * sum_k g w within gamma(K) of the magnitudes and exactly 0 where x <= 0; dW = sum g max(x, 0) and db = sum g over
    the n pixels within gamma(n) of theirs, whatever the order; two runs bit-equal; dx in a guarded buffer"""
    Bn, H, W = geom
    n = Bn * H * W
    x, w, g = _rand(Bn, H, W, C, seed=4), _rand(K, C, seed=5), _rand(Bn, K, H, W, seed=6)
    keep = x.clone()
    dx = Guarded(n, C, C, F32, DEV)
    _, part = ops.dpt_tail_bwd(g, x, w, dx=dx.view)
    red = ops.reduce_partials(part, torch.empty(K * C + K, device=DEV), False)
    dx2, part2 = ops.dpt_tail_bwd(g, x, w)
    red2 = ops.reduce_partials(part2, torch.empty(K * C + K, device=DEV), False)
    torch.cuda.synchronize()
    dx.intact('dpt_tail_bwd')
    assert torch.equal(x, keep)
    assert torch.equal(dx.view, dx2.view(n, C)) and torch.equal(part, part2) and torch.equal(red, red2)
    assert part.shape[0] == min((n + 127) // 128, 2048)
    gr = g.double().view(Bn, K, H * W).permute(0, 2, 1).reshape(n, K)
    pos = (x > 0).view(n, C)
    ref = (gr @ w.double()) * pos
    assert_within(dx.view, ref, gamma(K) * (gr.abs() @ w.double().abs()), 'dpt_tail_bwd dx', names=('pixel', 'c'))
    assert bool((dx.view[~pos] == 0).all())
    r = F.relu(x).double().view(n, C)
    assert_within(red[:K * C].view(K, C), gr.t() @ r, gamma(n) * (gr.abs().t() @ r), 'dpt_tail_bwd dW', names=('k', 'c'))
    assert_within(red[K * C:], gr.sum(0), gamma(n) * gr.abs().sum(0), 'dpt_tail_bwd db', names=('k',))


# --------------------------------------------------------------------------------------- transposed-convolution weights --
@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('mode,Cin,Cout', [('bf16', 8, 8), ('bf16', 8, 24), ('bf16', 24, 8), ('fp32', 3, 5)])
def test_deconv_weight_layouts(s, mode, Cin, Cout):
    """pack: wp[(i s + j) Cout + co][ci] = w[ci][co][i][j] and the bias tiled s s times, bit for bit; unpack: the way back bit for bit for
    the weight, the s s bias terms summed within gamma(s s), with and without accumulation"""
    act = _act(mode)
    bits = torch.int16 if mode == 'bf16' else torch.int32
    w, b = _rand(Cin, Cout, s, s, seed=7), _rand(Cout, seed=8)
    wp, bp = ops.deconv_weight_pack(w, b, s, act)
    ref = w.permute(2, 3, 1, 0).reshape(s * s * Cout, Cin).to(act).contiguous()
    assert torch.equal(wp.view(bits), ref.view(bits)) and torch.equal(bp, b.repeat(s * s))
    dwp, dbp = _rand(s * s * Cout, Cin, seed=9), _rand(s * s * Cout, seed=10)
    back = dwp.view(s, s, Cout, Cin).permute(3, 2, 0, 1).contiguous()
    dw, db = Guarded(Cin, Cout * s * s, Cout * s * s, F32, DEV), Guarded(1, Cout, Cout, F32, DEV)
    ops.deconv_weight_unpack(dwp, dbp, dw.view.view(Cin, Cout, s, s), db.view.view(Cout), s, False)
    aw, ab = w.clone(), b.clone()
    ops.deconv_weight_unpack(dwp, dbp, aw, ab, s, True)
    only_b = torch.empty(Cout, device=DEV)
    ops.deconv_weight_unpack(None, dbp, None, only_b, s, False, Cin=Cin)
    torch.cuda.synchronize()
    dw.intact('deconv_weight_unpack dw')
    db.intact('deconv_weight_unpack db')
    assert torch.equal(dw.view.view(Cin, Cout, s, s), back) and torch.equal(aw, w + back)
    t = dbp.double().view(s * s, Cout)
    bound = gamma(s * s) * t.abs().sum(0)
    assert_within(db.view.view(Cout), t.sum(0), bound, 'deconv db', names=('co',))
    assert torch.equal(only_b, db.view.view(Cout))
    assert_within(ab, b.double() + t.sum(0), gamma(s * s + 1) * (t.abs().sum(0) + b.double().abs()), 'deconv db accumulated', names=('co',))


@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('nh,nw', [(1, 1), (2, 3), (3, 2)])
@pytest.mark.parametrize('mode,Cin,Cout', [('bf16', 8, 24), ('bf16', 24, 8), ('fp32', 3, 5)])
def test_transposed_convolution_end_to_end(s, nh, nw, mode, Cin, Cout):
    """rows -> GEMM against the packed weight (bias in the epilogue) -> pixel shuffle == nn.ConvTranspose2d(kernel_size=s, stride=s):
    Cin products and the bias per element, against f64 of the operands as the GEMM sees them"""
    act = _act(mode)
    x, w, b = _rand(B, nh, nw, Cin, seed=11), _rand(Cin, Cout, s, s, seed=12), _rand(Cout, seed=13)
    with engine.precision(mode):
        rows = ops.cast(x.view(B * nh * nw, Cin), act)
        wp, bp = ops.deconv_weight_pack(w, b, s, act)
        proj = ops.linear_fwd(rows, wp, bp, torch.empty(B * nh * nw, s * s * Cout, device=DEV))
        out = Guarded(B * nh * s * nw * s, Cout, Cout, F32, DEV)
        ops.convnext_shuffle(proj, out.view, B, nh, nw, s, Cout)
    torch.cuda.synchronize()
    out.intact('deconv map')
    xs, ws = _seen(x, mode).permute(0, 3, 1, 2), _seen(w, mode)
    ref = F.conv_transpose2d(xs, ws, b.double(), stride=s).permute(0, 2, 3, 1)
    mag = F.conv_transpose2d(xs.abs(), ws.abs(), b.double().abs(), stride=s).permute(0, 2, 3, 1)
    assert_within(out.view.view(B, nh * s, nw * s, Cout), ref, gamma(Cin + 1) * mag + ulp(F32, ref), 'transposed convolution',
                  names=('b', 'y', 'x', 'co'))


# ------------------------------------------------------------------------------------------------------- the whole head --
def _engine_run(case, mode, direct=False, cap=None, spy=None):
    """the engine's forward + backward of one fixture case on the GPU: {'y', 'dx0'.., 'grad/<param>'} as CPU f64.  spy: a list that
    receives, per call of functions.conv3x3_bwd in call order, (dy, x, stride, relu, dx, packed weight gradient)."""
    K, tasks, D, (NH, NW) = CASES[case]
    head = OA.DPTOutputAdapter(num_classes=K, main_tasks=tasks, dim_tokens_enc=D, **GEOM)
    head.load_state_dict(DF.gold_sd(case), strict=True)
    head.to(DEV)
    if direct:
        engine.ParamArena(head).zero_grad()
    toks = [t.to(DEV).requires_grad_(True) for t in DF.tokens(case)]
    old = OU.set_col_workspace_bytes(cap) if cap else None
    engine.set_direct_grads(direct)
    conv_bwd = Fn.conv3x3_bwd

    def spied(dy, x, wp, stride, relu, addend, cap_, need_dx, need_dw):
        dx, dwp = conv_bwd(dy, x, wp, stride, relu, addend, cap_, need_dx, need_dw)
        spy.append((dy, x, stride, relu, dx, dwp))
        return dx, dwp
    if spy is not None:
        Fn.conv3x3_bwd = spied
    try:
        with engine.precision(mode):
            y = head(toks, DF.case_info(case))
            (y * DF.weight_like(y.detach().cpu()).to(DEV)).sum().backward()
    finally:
        Fn.conv3x3_bwd = conv_bwd
        engine.set_direct_grads(False)
        if cap:
            OU.set_col_workspace_bytes(old)
    engine.join_wgrad_streams()
    torch.cuda.synchronize()
    assert y.shape == (B, K, 16 * NH, 16 * NW) and y.is_contiguous() and type(y) is torch.Tensor
    out = {'y': y.detach().cpu().double()}
    out.update({f'dx{i}': t.grad.detach().cpu().double() for i, t in enumerate(toks)})
    out.update({f'grad/{n}': p.grad.detach().cpu().double().clone() for n, p in head.named_parameters() if p.grad is not None})
    return out


_RUNS = {}


def _run_once(case, mode):
    if (case, mode) not in _RUNS:
        _RUNS[case, mode] = _engine_run(case, mode)
    return _RUNS[case, mode]


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('mode,allowed', [('fp32', ALLOWED['fp32']), ('bf16', ALLOWED['bf16'])])
def test_head_against_the_reference(case, mode, allowed):
    """Per tensor (the output, four token gradients, 60 parameter gradients): the engine's deviation from the reference's f64 values,
    max-abs over the f64 tensor's max-abs, is at most `allowed` times the reference's own deviation in that precision.  The four
    parameters of refinenet4.resConfUnit1 take no part (their gradient is None in the reference), and the global-token row of every
    token gradient is exactly zero.

    fp32 mode: 4, the fusion blocks' figure (another summation order over the same operations).  Measured on an MI355X: 2.33 at most
    (r3, y; r1: 1.76, y).

    bf16 mode: 5.  The fusion blocks' figure of 2 does not hold for the whole head: measured 2.73 at most (r1,
    grad act_1_postprocess.1.bias: 0.342 against the reference's 0.125 under torch.autocast(bfloat16); nine tensors of r1 lie between
    2 and 2.73, all of r3 within 1.77).  The cause is where the roundings sit, not an error: the reference's own head on the CPU with
    the engine's rounding points -- convolution operands rounded to bf16, f32 accumulation, f32 maps and residual adds between the
    convolutions, the output gradient rounded once before each convolution's backward (make_golden_dpt.py --emulate) -- deviates
    from f64 by the same amounts tensor by tensor (0.352 for that bias; 0.1946 against the engine's 0.1946 for
    grad refinenet4.out_conv.bias), whereas autocast rounds every convolution's output to bf16.  On maps of 2 x 4 tokens a few ReLU
    sign flips decide these tensors' deviation under either placement.  5 = 2.73 x 1.5 rounded up to one significant digit;
    profiles/dpt_head_bench.json holds every ratio.  At these map sizes the bf16 check constrains little and the fp32 one is the one that
    bites; a fixture case on a larger token grid would give the bf16 check weight and is left as follow-up work."""
    mine, f64 = _run_once(case, mode), DF.tensors(case, 'f64')
    dev = DF.tensors(case, 'dev/f32' if mode == 'fp32' else 'dev/bf16')
    assert sorted(f64) == sorted(dev) and len(f64) == 65
    for n in UNUSED:
        assert f'grad/{n}' not in f64 and (f'grad/{n}' not in mine or not bool(mine[f'grad/{n}'].any())), n
    assert sorted(k for k in mine if k[5:] not in UNUSED) == sorted(f64)
    bad = {}
    for k, t64 in f64.items():
        e = float((mine[k] - t64.double()).abs().max()) / float(t64.abs().max())
        print(f'DPT_RATIO {json.dumps(dict(case=case, mode=mode, tensor=k, engine=e, reference=dev[k], ratio=e / dev[k] if dev[k] > 0 else None))}')
        if not e <= allowed * dev[k]:
            bad[k] = (e, dev[k])
    for i in range(4):
        assert not bool(mine[f'dx{i}'][:, -1].any()), i
    assert not bad, f'{case} {mode}: engine deviation above {allowed} x the reference deviation: {bad}'


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_both_gradient_modes_give_the_same_gradients(mode):
    """gradients returned to autograd and gradients accumulated into a zeroed arena (engine.set_direct_grads): identical bits"""
    a, b = _run_once('r1', mode), _engine_run('r1', mode, direct=True)
    assert torch.equal(a['y'], b['y']) and all(torch.equal(a[f'dx{i}'], b[f'dx{i}']) for i in range(4))
    names = [k for k in b if k.startswith('grad/')]
    assert len(names) == 64 and sorted(k for k in names if k[5:] not in UNUSED) == sorted(k for k in a if k.startswith('grad/'))
    for k in names:
        if k[5:] in UNUSED:
            assert not bool(b[k].any()), k                                # in the arena with a zero gradient
        else:
            assert torch.equal(a[k], b[k]), k


def test_chunked_batch_is_bit_identical():
    """A cap on the gathered rows small enough that every convolution runs sample by sample: the output, the token gradients and
    every parameter gradient that is one sum over the whole batch (biases, 1 x 1 and transposed convolutions, the tail) keep their
    bits, and so does every data gradient inside.  The weight gradient of a 3 x 3 convolution is accumulated chunk by chunk
    (functions.conv3x3_bwd): both runs add up the same n = B ho wo exact products of bf16 operands in f32, in another order, so each
    is within gamma(n) sum|terms| of the exact sum and the two are compared directly, per element of the packed gradient of each of
    the 21 calls, within 2 gamma(n) sum|terms| -- the magnitudes recomputed from the call's own operands as the GEMM sees them.  (A
    chunk left out or added twice misses that by orders of magnitude.)"""
    whole, chunked = [], []
    a, b = _engine_run('r3', 'bf16', spy=whole), _engine_run('r3', 'bf16', cap=64, spy=chunked)
    assert sorted(a) == sorted(b)
    head = DF.seeded_head('r3')
    conv3 = {f'grad/{n}' for n, p in head.named_parameters() if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3)}
    assert len(conv3) == 23 and len(conv3 & set(a)) == 21            # two belong to the unused refinenet4.resConfUnit1
    for k in a:
        if k not in conv3:
            assert torch.equal(a[k], b[k]), k
    assert len(whole) == len(chunked) == 21
    differ = 0
    for i, ((dy, x, stride, relu, dx, dwp), (dy2, x2, stride2, relu2, dx2, dwp2)) in enumerate(zip(whole, chunked)):
        assert (stride, relu) == (stride2, relu2) and torch.equal(dy, dy2) and torch.equal(x, x2), i
        assert (dx is None and dx2 is None) or torch.equal(dx, dx2), i
        Bn, h, w, Cin = x.shape
        Cout = dy.shape[-1]
        n = Bn * ops.conv_out_size(h, stride) * ops.conv_out_size(w, stride)
        col = ops.conv3x3_im2col(x, torch.empty(n, 9 * Cin, device=DEV, dtype=torch.bfloat16), Bn, h, w, Cin, stride, relu)
        mag = ops.cast(dy.reshape(n, Cout), torch.bfloat16).double().abs().t() @ col.double().abs()
        assert dwp.shape == dwp2.shape == mag.shape
        assert_within(dwp2, dwp, 2 * gamma(n) * mag, f'chunked weight gradient of convolution call {i}', names=('co', 'tap_c'))
        differ += int(not torch.equal(dwp, dwp2))
    print(f'DPT_CHUNK {differ} of 21 packed weight gradients differ in some bit between the chunked and the unchunked run')


# --------------------------------------------------------------------------------------------------------- model level --
def _build_vit():
    """the engine twin of make_golden_dpt.vit_case's model"""
    torch.manual_seed(7)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=(VIT['H'], VIT['W']))}
    outs = {'depth': OA.DPTOutputAdapter(num_classes=1, main_tasks=('rgb',), **GEOM)}
    return M.MultiViT(input_adapters=ins, output_adapters=outs, num_global_tokens=1, dim_tokens=VIT['D'], depth=VIT['depth'],
                      num_heads=VIT['heads'])


def test_multivit_with_the_head_and_one_optimiser_step():
    """A tiny MultiViT with the r1 head, return_all_layers=True, masked_l1_loss, fp32 mode: the prediction and the gradient of the patch
    projection -- which receives gradient through all four hooks -- within the fp32 ratio of the fixture; then one FusedAdamW step
    changes every used head parameter and leaves everything finite."""
    model = _build_vit()
    sd = DF.gold_sd('vit')
    assert list(model.state_dict()) == list(sd)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.build_arena()
    z = DF.gold('vit')
    x, target, mask = (torch.from_numpy(z[f'vit/{k}']).to(DEV) for k in ('x', 'target', 'mask'))
    f64, dev = DF.tensors('vit', 'f64'), DF.tensors('vit', 'dev/f32')
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.05)
    opt.zero_grad()
    with engine.precision('fp32'):
        y = model({'rgb': x}, return_all_layers=True)['depth']
        assert type(y) is torch.Tensor and getattr(y, '_mmae_seg', None) is None
        loss = M.masked_l1_loss(y, target, mask)
        loss.backward()
        engine.join_wgrad_streams()
        torch.cuda.synchronize()
        mine = {'y': y.detach(), 'grad/input_adapters.rgb.proj.weight': model.input_adapters['rgb'].proj.weight.grad.detach().clone()}
        assert sorted(mine) == sorted(f64)
        bad = {}
        for k, t64 in f64.items():
            e = float((mine[k].cpu().double() - t64.double()).abs().max()) / float(t64.abs().max())
            print(f'DPT_RATIO {json.dumps(dict(case="vit", mode="fp32", tensor=k, engine=e, reference=dev[k], ratio=e / dev[k]))}')
            if not e <= ALLOWED['fp32'] * dev[k]:
                bad[k] = (e, dev[k])
        head = model.output_adapters['depth']
        before = {n: p.detach().clone() for n, p in head.named_parameters()}
        opt.step()
        torch.cuda.synchronize()
    for n, p in head.named_parameters():
        assert bool(torch.isfinite(p).all()), n
        if n not in UNUSED:
            assert not torch.equal(p.detach(), before[n]), n
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert not bad, f'vit fp32: engine deviation above 4 x the reference deviation: {bad}'
