"""GPU: ConvNeXtHeadFn (functions.py) stage by stage.  One forward + backward of the head per case and precision mode runs under
tests/stage_recorder.py; then EVERY recorded launch is checked per element against fp64 of its operands AS RECORDED (so an error can
neither hide behind the stage before nor be blamed on it), and the data-flow graph of tests/test_convnext_stages_cpu.py is walked
again on the real buffers with bits=True.  Every stage prints its largest error / bound ratio and where it sits on a line
`CONVNEXT_STAGE ...` (collected in profiles/convnext_stage_margins.json); a ratio above 1 fails.

Bounds -- all from tests/helpers.py and tests/test_convnext_head_gpu.py, none tuned (u = 2^-24, gamma_n = n u / (1 - n u)).  Both
precision modes multiply exactly into fp32 (bf16 operands on the bf16 MFMA; 'fp32' is the exact-f32 GEMM): u_op = 0, k_mult = 1.
  gather, scatter, shuffle, casts   bit for bit (bf16_bits_ref for the rounding); what a launch must not write keeps its bits
  GEMM stages          linear_ref / linear_dx_ref(mul=) / linear_dw_ref(g0=): gamma_K |x| |w|^T, 2u per epilogue addition, the final
                       rounding into the output's type; an accumulate destination's recorded `before` is g0
  GELU pair            value GELU_D1 e + GELU_ABS + GELU_REL |lin|, stored derivative GELU_D2 e + DGELU_ABS (e: the pre-activation's
                       bound), + the rounding into the activation type -- check_block_fwd of test_composite_gpu.py
  LayerNorm            layernorm_ref: mean, rstd, y; backward dx and the three column sums of the partial rows (summed in fp64 here,
                       bounds with extra = the partial rows of the launch; colsum(dx): the rows' dx bounds summed + gamma_(R + extra)
                       sum |dx|); the reduction into the gradients: colsum_ref over the partial rows (+ 1 term when accumulating)
  dwconv7 fwd, dgrad   gamma_50 (|x| * |w| + |b or dx_in|) + ulp;   wgrad + reduce: gamma_(B h w + 4 + nblk) sum |dy| |x| + ulp
  resize fwd, bwd      test_resize_fwd / test_resize_bwd_gather's bounds; nearest forward is a copy
  axpy_                y + x is one f32 addition: bit for bit
Which comparisons of the gradient-routing test are bounds and which are bits is said in its docstring."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multimae_amd as M
from multimae_amd import _lib, ops
from helpers import (DGELU_ABS, GELU_ABS, GELU_D1, GELU_D2, GELU_REL, Guarded, assert_untouched, assert_within, bf16_bits_ref, colsum_ref,
                     gamma, gelu_ref, layernorm_ref, linear_dw_ref, linear_dx_ref, linear_ref, same_bits, ulp)
from stage_recorder import HEAD_OPS, record
from test_convnext_stages_cpu import CASES, build_case, check_graph, run_head

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
EPS = 1e-6                                               # ConvNeXtBlock's LayerNorm
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _nchw(x, B, h, w, C):
    return x.reshape(B, h, w, C).permute(0, 3, 1, 2).double()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------- one stage, one check --
def stage_items(c, st):
    """The checks of one recorded call.  Exact properties are asserted here; yields (label, got, reference, bound, index names) of
    every bounded output.  st: state carried between calls (the dwconv7_wgrad call a reduce_partials belongs to)."""
    a, n = c.a, c.name
    if n == 'convnext_rows_gather':
        enc, out, start, N, col = a['enc'], a['out'], a['start'], a['N'], a['col_off']
        B, n_tok, D = enc.shape
        src = enc.before[:, start:start + N].reshape(B * N, D)
        got = out.after[:, col:col + D]
        want = src if out.dtype == torch.float32 else bf16_bits_ref(src).view(torch.bfloat16)
        assert _eq(got, want), f'{c}: the gathered rows are not the (rounded) token rows bit for bit'
        keep = torch.ones(out.shape[1], dtype=torch.bool, device=got.device)
        keep[col:col + D] = False
        assert _eq(out.after[:, keep], out.before[:, keep]), f'{c}: columns outside [col_off, col_off + D) were written'
        assert _eq(enc.after, enc.before), f'{c}: the source changed'
    elif n == 'convnext_rows_scatter':
        src, d_enc, start, N, col = a['src'], a['d_enc'], a['start'], a['N'], a['col_off']
        B, n_tok, D = d_enc.shape
        got = d_enc.after[:, start:start + N].reshape(B * N, D)
        assert _eq(got, src.before[:, col:col + D].float()), f'{c}: the scattered rows are not the source columns bit for bit'
        keep = torch.ones(n_tok, dtype=torch.bool, device=got.device)
        keep[start:start + N] = False
        assert _eq(d_enc.after[:, keep], d_enc.before[:, keep]), f'{c}: rows outside [start, start + N) were written'
    elif n == 'convnext_shuffle':
        B, NH, NW, s, C = a['B'], a['NH'], a['NW'], a['s'], a['C']
        proj, mp = (a['dst'].after, a['src'].before) if a['inverse'] else (a['src'].before, a['dst'].after)
        assert _eq(proj.view(B, NH, NW, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C), mp), f'{c}: not the pixel shuffle bit for bit'
    elif n == 'cast':
        x, y = a['x'], c.ret
        if x.dtype == a['dtype']:
            assert y.ptr == x.ptr, f'{c}: a cast to the same type must return its argument'
        elif a['dtype'] == torch.bfloat16:
            assert _eq(y.after.view(torch.int16), bf16_bits_ref(x.before)), f'{c}: not round-to-nearest-even bit for bit'
        else:
            assert _eq(y.after, x.before.float()), f'{c}: not the exact widening'
    elif n == 'linear_fwd':
        x, w, bias, out, resid, aux = a['x'].before, a['w'].before, a['bias'].before, a['out'], a['resid'], a['aux']
        if a['epi'] == ops.EPI_GELU_G:
            act = out.dtype
            _, _, (lin, e) = linear_ref(x, w, bias)
            ge, dge = gelu_ref(lin)
            bg = GELU_D1 * e + GELU_ABS + GELU_REL * lin.abs()
            yield 'gelu', out.after, ge, bg + ulp(act, ge.abs() + bg), ('row', 'col')
            bh = GELU_D2 * e + DGELU_ABS
            yield 'dgelu', aux.after, dge, bh + ulp(act, dge.abs() + bh), ('row', 'col')
        else:
            assert a['epi'] == ops.EPI_NONE and aux is None
            ref, bd, _ = linear_ref(x, w, bias, resid=None if resid is None else resid.before, out_dtype=out.dtype)
            yield 'y', out.after, ref, bd, ('row', 'col')
    elif n == 'gemm':                                    # the final_layer product into rows of stride round_up(K, 8)
        N_, K_ = a['N'], a['K']
        C_ = a['C']
        ref, bd, _ = linear_ref(a['A'].before, a['B'].before.reshape(N_, K_), a['bias'].before)
        assert _eq(C_.after[:, N_:], C_.before[:, N_:]), f'{c}: the pad columns N .. ldc - 1 were written'
        yield 'logits', C_.after[:, :N_], ref, bd, ('row', 'col')
    elif n == 'linear_dx':
        dy, w, out = a['dy'].before, a['w'].before, a['out']
        mul = None
        if a['epi'] == ops.EPI_MUL:
            mul = a['aux'].before
        else:
            assert a['epi'] == ops.EPI_NONE
        ref, bd, _ = linear_dx_ref(dy, w.reshape(dy.shape[1], -1), out.dtype, mul=mul)
        yield 'dx', out.after, ref, bd, ('row', 'col')
    elif n == 'linear_dw':
        dy, x, dw, db = a['dy'].before, a['x'].before, a['dw'], a['db']
        N_, K_ = dy.shape[1], x.shape[1]
        g0 = None
        if a['accumulate']:
            assert db is None or a['db_accumulate']
            g0 = (dw.before.reshape(N_, K_), torch.zeros(N_, device=dy.device) if db is None else db.before.reshape(-1))
        else:
            assert not a['db_accumulate']
        (rw, bw), (rb, bb) = linear_dw_ref(dy, x, g0=g0)
        yield 'dw', dw.after.reshape(N_, K_), rw, bw, ('row', 'col')
        if db is not None:
            yield 'db', db.after.reshape(-1), rb, bb, ('col',)
    elif n == 'layernorm_fwd':
        ln = layernorm_ref(a['x'].before, a['gamma'].before, a['beta'].before, a['eps'])
        y, mean, rstd = c.ret
        yield 'mean', mean.after, ln.mean, ln.b_mean, ('row',)
        yield 'rstd', rstd.after, ln.rstd, ln.b_rstd, ('row',)
        yield 'y', y.after, ln.y, ln.b_y(y.dtype), ('row', 'col')
    elif n == 'layernorm_bwd_part':
        gam = a['gamma'].before
        ln = layernorm_ref(a['x'].before, gam, torch.zeros_like(gam), EPS)
        dx, _, part = c.ret
        nblk, D = part.shape[0], gam.numel()
        o = ln.bwd(a['dy'].before, None, extra=nblk)
        yield 'dx', dx.after, o['dx'][0], o['dx'][1], ('row', 'col')
        sums = part.after.double().sum(0)
        yield 'part_dgamma', sums[:D], o['dgamma'][0], o['dgamma'][1], ('col',)
        yield 'part_dbeta', sums[D:2 * D], o['dbeta'][0], o['dbeta'][1], ('col',)
        ref, b32 = o['dx']
        yield 'part_colsum_dx', sums[2 * D:], ref.sum(0), b32.sum(0) + gamma(ln.R + nblk) * ref.abs().sum(0), ('col',)
    elif n in ('colsum_scatter', 'colsum'):
        part = a['dy'].before
        dsts = a['dsts'] if n == 'colsum_scatter' else [a['out']]
        seg_w = a['seg_w'] if n == 'colsum_scatter' else part.shape[1]
        for i, d in enumerate(dsts):
            if d is None:
                continue
            ref, bd = colsum_ref(part[:, i * seg_w:(i + 1) * seg_w], g0=d.before.reshape(-1) if a['accumulate'] else None)
            yield f'seg{i}', d.after.reshape(-1), ref, bd, ('col',)
    elif n == 'dwconv7_fwd':
        B, h, w, C = a['B'], a['h'], a['w'], a['C']
        wt, b = a['w7'].before.double(), a['bias'].before.double()
        xd = _nchw(a['x'].before, B, h, w, C)
        ref = _rows(F.conv2d(xd, wt, b, padding=3, groups=C))
        T = _rows(F.conv2d(xd.abs(), wt.abs(), padding=3, groups=C))
        yield 'y', a['out'].after, ref, gamma(50) * (T + b.abs()) + ulp(torch.float32, ref), ('row', 'col')
    elif n == 'dwconv7_dgrad':
        B, h, w, C = a['B'], a['h'], a['w'], a['C']
        wt, dxin = a['w7'].before.double(), a['dx_in'].before.double()
        dy = _nchw(a['dy'].before, B, h, w, C)
        xd = torch.zeros(B, C, h, w, dtype=torch.float64, device=dy.device, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(xd, wt, padding=3, groups=C), xd, dy)
        (ga,) = torch.autograd.grad(F.conv2d(xd, wt.abs(), padding=3, groups=C), xd, dy.abs())
        ref = _rows(g) + dxin
        yield 'dx', a['out'].after, ref, gamma(50) * (_rows(ga) + dxin.abs()) + ulp(torch.float32, ref), ('row', 'col')
    elif n == 'dwconv7_wgrad':
        st['wgrad'] = c                                  # checked together with its reduction
    elif n == 'reduce_partials':
        part, out = a['part'], a['out']
        assert not a['accumulate']
        nblk = part.shape[0]
        ref, bd = colsum_ref(part.before.reshape(nblk, -1))
        yield 'reduce', out.after.reshape(-1), ref, bd, ('col',)
        wg = st.pop('wgrad')
        assert wg.ret.ptr == part.ptr and _eq(wg.ret.after, part.before)
        B, h, w, C = wg.a['B'], wg.a['h'], wg.a['w'], wg.a['C']
        x, dy = _nchw(wg.a['x'].before, B, h, w, C), _nchw(wg.a['dy'].before, B, h, w, C)
        wd = torch.zeros(C, 1, 7, 7, dtype=torch.float64, device=x.device, requires_grad=True)
        (ref,) = torch.autograd.grad(F.conv2d(x, wd, padding=3, groups=C), wd, dy)
        (T,) = torch.autograd.grad(F.conv2d(x.abs(), wd, padding=3, groups=C), wd, dy.abs())
        yield 'wgrad', out.after.reshape(-1), ref.reshape(-1), gamma(B * h * w + 4 + nblk) * T.reshape(-1) + ulp(torch.float32, ref.reshape(-1)), ('col',)
    elif n == 'axpy_':
        assert a['a'] == 1.0 and _eq(a['y'].after, a['y'].before + a['x'].before.reshape(a['y'].shape)), f'{c}: not y + x bit for bit'
    elif n == 'resize_fwd':
        B, h, w, K, H, W, mode = a['B'], a['h'], a['w'], a['K'], a['H'], a['W'], a['mode']
        x = a['x'].before[:, :K]
        ref = F.interpolate(_nchw(x, B, h, w, K), size=(H, W), mode=mode, **({'align_corners': False} if mode == 'bilinear' else {}))
        if mode == 'nearest':
            assert bool(torch.equal(a['out'].after.double(), ref)), f'{c}: nearest is a copy'
        else:
            bound = (4 * U * (max(h, w) + 2) * 2 + 8 * U) * x.abs().max().double() + ulp(torch.float32, ref)
            yield 'image', a['out'].after, ref, bound, ('b', 'k', 'y', 'x')
    elif n == 'resize_bwd':
        B, h, w, K, H, W, mode = a['B'], a['h'], a['w'], a['K'], a['H'], a['W'], a['mode']
        g, dx = a['g'].before, a['dx'].after
        assert not dx[:, K:].any(), f'{c}: the pad columns K .. ldx - 1 are not zero'
        xd = torch.zeros(B, K, h, w, dtype=torch.float64, device=g.device, requires_grad=True)
        kw = {'align_corners': False} if mode == 'bilinear' else {}
        (ref,) = torch.autograd.grad(F.interpolate(xd, size=(H, W), mode=mode, **kw), xd, g.double())
        ref = _rows(ref)
        nt = (2 * math.ceil(H / h) + 3) * (2 * math.ceil(W / w) + 3)
        bound = (gamma(nt) + (8 * U * (max(h, w) + 2) if mode == 'bilinear' else 0.0)) * nt * g.abs().max().double() + ulp(torch.float32, ref)
        yield 'd_logits', dx[:, :K], ref, bound, ('row', 'col')
    elif n == 'seg_ce_bwd':                              # per element in test_seg_loss_gpu.py; here only what the head relies on
        assert not a['dx'].after[:, a['K']:].any(), f'{c}: the pad columns K .. ldx - 1 are not zero'
    elif n == 'seg_ce_fwd':
        pass
    else:
        raise AssertionError(f'{c}: a recorded launch without a stage check')


def held(tag, c, item):
    """prints the stage's largest error / bound ratio with its place, then holds every element to the bound"""
    label, got, ref, bound, names = item
    o = got.detach().double()
    r = ref.detach().double().to(o.device)
    bd = torch.as_tensor(bound).double().to(o.device).expand_as(r)
    err = (o - r).abs()
    ratio = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bd), nan=float('inf'), posinf=float('inf'))
    flat = int(torch.argmax(ratio))
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(r.shape)))
    print(f'CONVNEXT_STAGE {tag} stage={c.index:02d}.{c.name}.{label} ratio={float(ratio.reshape(-1)[flat]):.4g} at={idx}')
    assert_within(got, ref, bound, f'{tag} #{c.index} {c.name} {label}', names)


def check_stages(tag, calls):
    st = {}
    for c in calls:
        items = list(stage_items(c, st))
        if not items and c.name != 'dwconv7_wgrad':
            print(f'CONVNEXT_STAGE {tag} stage={c.index:02d}.{c.name} ratio=0 exact')
        for it in items:
            held(tag, c, it)
    assert not st, 'a dwconv7_wgrad without its reduction'


# ----------------------------------------------------------------------------------------------------- recorded runs --
_RUNS = {}


def recorded(name, mode, loss=False, image=None):
    """one recorded forward + backward per (case, mode, gradient source), shared by the tests that only read it"""
    key = (name, mode, loss, image)
    if key not in _RUNS:
        head, info, x = build_case(name, DEV)
        target = None
        if loss:
            K, (H, W) = head.num_classes, info['image_size']
            target = torch.randint(0, K, (x.shape[0], H, W), generator=torch.Generator().manual_seed(9)).to(DEV)
            target[:, :3, :5] = 255
        _RUNS[key] = run_head(head, info, x, mode, target=target, image=image)
    return _RUNS[key]


def _final(run):
    """what must hold at the end of any recorded run: the encoder gradient is the last scatter's buffer, rows of other tasks and of the
    global token exactly zero; the cast logits gradient's pad columns exactly zero"""
    head, info, x = run.head, run.info, run.x
    sc = run.rec.named('convnext_rows_scatter')
    assert _eq(x.grad, sc[-1].a['d_enc'].after)
    mine = torch.zeros(x.shape[1], dtype=torch.bool, device=x.device)
    for t in head.main_tasks:
        mine[info['tasks'][t]['start_idx']:info['tasks'][t]['end_idx']] = True
    assert not x.grad[:, ~mine].any() and x.grad[:, mine].abs().sum() > 0
    K = head.num_classes
    dy = run.rec.named('linear_dx')[0].a['dy']                      # the final_layer dX runs first
    if dy.rows_before is not None:
        assert dy.rows_before.shape[1] == ops.round_up(K, 8) and not dy.rows_before[:, K:].any()


RUN_CASES = [(n, m) for n in CASES for m in ('bf16', 'fp32') if (n, m) != ('fp32_only', 'bf16')]


@pytest.mark.parametrize('name,mode', RUN_CASES)
def test_every_stage_against_fp64_of_its_recorded_operands(name, mode):
    run = recorded(name, mode)
    check_graph(run, bits=True)
    check_stages(f'case={name} mode={mode} grad=image', run.rec.calls)
    _final(run)


def test_fp32_only_geometry_is_refused_in_bf16():
    head, info, x = build_case('fp32_only', DEV)
    with M.engine.precision('bf16'), pytest.raises(ValueError, match='multiples of 8'):
        head(x, info)


@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
def test_two_tasks_gradient_through_the_fused_loss_handle(mode):
    """d_logits arrives through SegHandle from SegCrossEntropyLoss: no resize_bwd, the cast reads seg_ce_bwd's buffer"""
    run = recorded('two_tasks', mode, loss=True)
    assert not run.rec.named('resize_bwd') and len(run.rec.named('seg_ce_bwd')) == 1
    check_graph(run, bits=True)
    check_stages(f'case=two_tasks mode={mode} grad=loss', run.rec.calls)
    _final(run)


@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
def test_two_tasks_loss_and_image_gradients_add_in_place(mode):
    """a loss on the logits and a consumer of the image at once: the cast reads seg_ce_bwd's buffer, which then holds the f32 sum of
    the two gradients bit for bit (one addition per element)"""
    run = recorded('two_tasks', mode, loss=True, image=True)
    assert len(run.rec.named('resize_bwd')) == 1 and len(run.rec.named('seg_ce_bwd')) == 1
    check_graph(run, bits=True)
    check_stages(f'case=two_tasks mode={mode} grad=loss+image', run.rec.calls)
    _final(run)


# ----------------------------------------------------------------------------------------- final_layer with K < Kp --
@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
def test_final_layer_gradients_stay_inside_K_rows(mode):
    """The recorded final_layer dW + db launch of two_tasks (K = 13, rows of stride 16) again on test-owned Guarded destinations with
    the recorded operands: nothing is written past row K of dW or element K of db, and both hold to linear_dw_ref's bounds."""
    run = recorded('two_tasks', mode)
    c = run.rec.named('linear_dw')[0]
    K, Kp = run.head.num_classes, ops.round_up(run.head.num_classes, 8)
    dy = c.a['dy'].rows_before.clone()
    assert dy.shape[1] == Kp and K < Kp and not dy[:, K:].any()
    x = c.a['x'].before.clone()
    C = x.shape[1]
    gw, gb = Guarded(K, C, C, torch.float32, DEV), Guarded(1, K, K, torch.float32, DEV)
    ops.linear_dw(dy[:, :K], x, gw.view, False, db=gb.view.view(-1), db_accumulate=False)
    torch.cuda.synchronize()
    gw.intact('final_layer dW')
    gb.intact('final_layer db')
    (rw, bw), (rb, bb) = linear_dw_ref(dy[:, :K], x)
    assert_within(gw.view, rw, bw, 'final_layer dW on guarded rows', ('row', 'col'))
    assert_within(gb.view.view(-1), rb, bb, 'final_layer db on guarded elements', ('col',))


# ------------------------------------------------------------------------------------------------- gradient routing --
def _pattern(n):
    return (0.05 * torch.sin(0.11 * torch.arange(n, dtype=torch.float64))).float().to(DEV)


def _routed(mode, direct, wgrad_stream, rec_names=()):
    """two forward + backward passes of the same inputs in one routing mode -> (runs, [d_enc, gradients in _params() order] per pass);
    direct: the gradient arena holds _pattern() before each backward"""
    head, info, x = build_case('two_tasks', DEV, arena=direct)
    arena = M.engine.arena_of(head) if direct else None
    out, runs = [], []
    for _ in range(2):
        x.grad = None
        if direct:
            arena.zero_grad()
            arena.grad.copy_(_pattern(arena.grad.numel()))
        else:
            head.zero_grad(set_to_none=True)
        runs.append(run_head(head, info, x, mode, direct=direct, wgrad_stream=wgrad_stream, names=rec_names))
        rec_names = ()
        out.append([x.grad.clone()] + [p.grad.clone() for p in head._params()])
    return runs, out, head


@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
def test_gradient_routing_autograd_direct_and_side_stream(mode):
    """two_tasks in the three routing modes, two passes each.
    Bits: the two passes of every mode; the side-stream run against the single-stream direct run (every gradient and d_enc);
          dwconv.weight in direct mode against pattern + the autograd-mode gradient -- one f32 addition of the same two numbers (axpy_).
    Bounds: every other parameter in direct mode -- its launch adds the pattern inside the reduction, in another order than a separate
          addition would -- through the recorded direct pass: each destination's `before` is the pattern, and the stage check holds
          `after` to linear_dw_ref(g0 = pattern) / colsum_ref(g0 = pattern).  The first side-stream pass is recorded and checked the
          same way."""
    _, auto, _ = _routed(mode, False, False)
    runs, direct, head = _routed(mode, True, False, rec_names=HEAD_OPS)
    old = M.engine.wgrad_stream()
    try:
        side_runs, side, _ = _routed(mode, True, True, rec_names=HEAD_OPS)
    finally:
        M.engine.set_wgrad_stream(old)
    for what, (a, b) in (('autograd', auto), ('direct', direct), ('side stream', side)):
        for i, (u, v) in enumerate(zip(a, b)):
            assert same_bits(u, v), f'{what}: pass 1 and pass 2 differ in tensor {i}'
    for i, (u, v) in enumerate(zip(direct[0], side[0])):
        assert same_bits(u, v), f'side stream against single stream: tensor {i} differs'
    arena = M.engine.arena_of(head)
    pat = _pattern(arena.grad.numel())
    ps = head._params()
    for i in range(len(head.blocks)):
        p = ps[8 * i]
        off = (p.grad.data_ptr() - arena.grad.data_ptr()) // 4
        assert same_bits(direct[0][1 + 8 * i], pat[off:off + p.numel()].view(p.shape) + auto[0][1 + 8 * i]), f'dwconv.weight of block {i}'
    # the recorded direct pass: the graph (arena views, accumulate flags) and every stage with g0 = what the destination held
    rec = runs[0]
    check_graph(rec, bits=True)
    for c in rec.rec.calls:
        if c.name == 'linear_dw':
            off = (c.a['dw'].ptr - arena.grad.data_ptr()) // 4
            assert _eq(c.a['dw'].before.reshape(-1), pat[off:off + c.a['dw'].before.numel()]), f'{c}: the destination did not hold the pattern'
    check_stages(f'case=two_tasks mode={mode} grad=image routing=direct', rec.rec.calls)
    # ... and the recorded side-stream pass: the clones taken on the side stream are ordered behind the launches they watch
    check_graph(side_runs[0], bits=True)
    check_stages(f'case=two_tasks mode={mode} grad=image routing=side_stream', side_runs[0].rec.calls)


# -------------------------------------------------------------------------------------- sensitivity of the stage checks --
def _one(calls, name, pred=lambda c: True):
    return [c for c in calls if c.name == name and pred(c)][0]


@pytest.mark.parametrize('which', ['bf16 GELU-pair GEMM', 'LayerNorm backward', 'dwconv7 forward'])
def test_stage_checks_notice_four_bounds_on_one_element(which):
    """on the recorded data of two_tasks / bf16, no kernel re-run: four times the local bound added to ONE element of a stage's
    recorded output must fail that stage's check and name the element"""
    run = recorded('two_tasks', 'bf16')
    calls = run.rec.calls
    if which == 'bf16 GELU-pair GEMM':
        c, label, el = _one(calls, 'linear_fwd', lambda c: c.a['epi'] == ops.EPI_GELU_G), 'gelu', (37, 53)
    elif which == 'LayerNorm backward':
        c, label, el = _one(calls, 'layernorm_bwd_part'), 'dx', (70, 11)
    else:
        c, label, el = _one(calls, 'dwconv7_fwd'), 'y', (5, 23)
    item = [it for it in stage_items(c, {}) if it[0] == label][0]
    bound = torch.as_tensor(item[3]).double().expand_as(item[2])
    c2 = copy.copy(c)
    c2.a = dict(c.a)
    if which == 'LayerNorm backward':
        c2.ret = list(c.ret)
        t2 = c2.ret[0] = copy.copy(c.ret[0])
    else:
        t2 = c2.a['out'] = copy.copy(c.a['out'])
    t2.after = t2.after.clone()
    t2.after[el] = (t2.after[el].double() + 4 * bound[el]).to(t2.after.dtype)
    for it in stage_items(c, {}):                                        # the untouched recording passes
        assert_within(*it[1:4], 'untouched', it[4])
    with pytest.raises(AssertionError, match=rf'row={el[0]}, col={el[1]}\)'):
        for it in stage_items(c2, {}):
            assert_within(it[1], it[2], it[3], it[0], it[4])


# ---------------------------------------------------------------------------------------- pad columns of the logits --
@pytest.mark.parametrize('mode', ['bf16', 'fp32'])
def test_consumers_never_read_the_logits_pad_columns(mode):
    """logits is torch.empty([R, Kp]) with K = 13 columns written: NaN in columns K .. Kp - 1 of handle.logits must leave the fused
    loss, its backward (d_logits[:, :K], with d_logits[:, K:] exactly 0), seg_argmax and the lazy image fill with the bits they have
    with zeros there (tests/test_seg_loss_gpu.py feeds NaN pads to the loss kernels and the argmax against fp64, not to the lazy fill
    and not through the head's own handle)"""
    head, info, x = build_case('two_tasks', DEV)
    K, (H, W) = head.num_classes, info['image_size']
    target = torch.randint(0, K, (x.shape[0], H, W), generator=torch.Generator().manual_seed(9)).to(DEV)
    target[:, :3, :5] = 255
    res = []
    for poison in (0.0, float('nan')):
        x.grad = None
        head.zero_grad(set_to_none=True)
        with M.engine.precision(mode), record(('seg_ce_bwd',)) as rec:
            y = head(x, info)
            hd = y._mmae_seg
            assert hd.ld == ops.round_up(K, 8) > K and y.materialized is False
            hd.logits[:, K:] = poison
            loss = M.SegCrossEntropyLoss(ignore_index=255)(y, target)
            loss.backward()
            pred = M.seg_argmax(y, K)
            assert y.materialized is False
            img = y + 0.0                                                # the first read fills the image
        d = rec.named('seg_ce_bwd')[0].a['dx'].after
        assert not d[:, K:].any(), 'd_logits[:, K:] is not exactly zero'
        res.append([loss.detach().clone(), d[:, :K].clone(), pred, img.detach().clone(), x.grad.clone()])
    for i, (u, v) in enumerate(zip(*res)):
        assert same_bits(u, v), ('loss', 'd_logits', 'argmax', 'image', 'd_enc')[i]
    assert bool(torch.isfinite(res[1][0])) and bool(torch.isfinite(res[1][3]).all())


# ------------------------------------------------------------------- the two kernels no other test calls directly --
ROWS = [(2, 7, 5, 3), (3, 50, 96, 24)]                  # (B, n_tok, D, N): one workgroup with odd sizes; 27 workgroups


def _tokens(B, n_tok, D, seed):
    return torch.randn(B, n_tok, D, generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,n_tok,D,N', ROWS)
def test_rows_gather_direct(B, n_tok, D, N, dtype):
    """two tasks with col_off (start = 0 and start + N = n_tok) into rows of stride ld_out > col_off + D, f32 and bf16, in a Guarded
    buffer: the slice bit for bit, the other task's columns, the ld padding and the guard zones untouched, the source unchanged"""
    enc = _tokens(B, n_tok, D, 21)
    keep = enc.clone()
    fill = torch.randn(B * N, 2 * D, generator=torch.Generator().manual_seed(22)).to(DEV).to(dtype)
    g = Guarded(B * N, 2 * D, 2 * D + 3, dtype, DEV, fill=fill)
    want = lambda st: enc[:, st:st + N].reshape(B * N, D) if dtype == torch.float32 else \
        bf16_bits_ref(enc[:, st:st + N].reshape(B * N, D)).view(torch.bfloat16)
    ops.convnext_rows_gather(enc, g.view, 0, N, 0)
    torch.cuda.synchronize()
    g.intact('rows_gather task 0')
    assert _eq(g.view[:, :D], want(0)) and _eq(g.view[:, D:], fill[:, D:])
    ops.convnext_rows_gather(enc, g.view, n_tok - N, N, D)
    torch.cuda.synchronize()
    g.intact('rows_gather task 1')
    assert _eq(g.view[:, :D], want(0)) and _eq(g.view[:, D:], want(n_tok - N))
    assert _eq(enc, keep)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,n_tok,D,N', ROWS)
def test_rows_scatter_direct(B, n_tok, D, N, dtype):
    """the destination holds a pattern: rows [start, start + N) receive the source columns (bf16 widened exactly), every other row
    keeps its bits -- 'rows of other tasks untouched' is the kernel's contract"""
    src = torch.randn(B * N, 2 * D + 3, generator=torch.Generator().manual_seed(23)).to(DEV).to(dtype)
    keep = src.clone()
    fill = -torch.arange(B * n_tok * D, dtype=torch.float32, device=DEV).view(B, n_tok * D) * 0.5      # -0.0 first
    for start, col in ((0, 0), (n_tok - N, D), (1, 3)):
        g = Guarded(B, n_tok * D, n_tok * D, torch.float32, DEV, fill=fill)
        ops.convnext_rows_scatter(src, g.view.view(B, n_tok, D), start, N, col)
        torch.cuda.synchronize()
        g.intact('rows_scatter')
        got, was = g.view.view(B, n_tok, D), fill.view(B, n_tok, D)
        assert _eq(got[:, start:start + N].reshape(B * N, D), src[:, col:col + D].float())
        other = torch.ones(n_tok, dtype=torch.bool, device=DEV)
        other[start:start + N] = False
        assert _eq(got[:, other], was[:, other])
    assert _eq(src, keep)


def test_rows_gather_and_scatter_refuse_bad_arguments():
    """start + N > n_tok, a row stride below col_off + D and a dtype code that is neither f32 nor bf16: MMAE_EINVAL, nothing written"""
    B, n_tok, D, N = 2, 7, 8, 3
    enc = _tokens(B, n_tok, D, 24)
    lib = _lib.load()
    EINVAL, F16 = -1, 5
    s = torch.cuda.current_stream().cuda_stream
    out = Guarded(B * N, D, D, torch.float32, DEV)
    with pytest.raises(_lib.KernelError, match=r'rc=-1'):
        ops.convnext_rows_gather(enc, out.view, n_tok - N + 1, N, 0)
    with pytest.raises(_lib.KernelError, match=r'rc=-1'):
        ops.convnext_rows_gather(enc, out.view, 0, N, 1)                       # ld = D < col_off + D
    assert lib.mmae_convnext_rows_gather(enc.data_ptr(), out.view.data_ptr(), F16, B, n_tok, D, 0, N, D, 0, s) == EINVAL
    assert lib.mmae_convnext_rows_gather(enc.data_ptr(), out.view.data_ptr(), 7, B, n_tok, D, 0, N, D, 0, s) == EINVAL
    torch.cuda.synchronize()
    assert_untouched(out, 'rows_gather refused')
    src = torch.randn(B * N, D, device=DEV)
    keep = src.clone()
    dst = Guarded(B, n_tok * D, n_tok * D, torch.float32, DEV)
    d_enc = dst.view.view(B, n_tok, D)
    with pytest.raises(_lib.KernelError, match=r'rc=-1'):
        ops.convnext_rows_scatter(src, d_enc, n_tok - N + 1, N, 0)
    with pytest.raises(_lib.KernelError, match=r'rc=-1'):
        ops.convnext_rows_scatter(src, d_enc, 0, N, 1)
    assert lib.mmae_convnext_rows_scatter(src.data_ptr(), F16, d_enc.data_ptr(), B, n_tok, D, 0, N, D, 0, s) == EINVAL
    assert lib.mmae_convnext_rows_scatter(src.data_ptr(), 7, d_enc.data_ptr(), B, n_tok, D, 0, N, D, 0, s) == EINVAL
    torch.cuda.synchronize()
    assert_untouched(dst, 'rows_scatter refused')
    assert _eq(src, keep)
