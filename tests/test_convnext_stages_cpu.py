"""CPU: the wiring of ConvNeXtHeadFn (functions.py) checked by storage identity on the C ABI stub (tests/dryrun_harness.py: numbers are
garbage, pointers are real).  One forward + backward of the head runs under tests/stage_recorder.py; check_graph() then walks the
recorded calls along the head's data-flow graph as written out below -- not derived from the code: every operand of every launch
must be the buffer the graph names (the producer's output, the parameter itself, cfg.wc's copy of exactly that weight, the arena
view p.grad of exactly that parameter).  Mis-wired copies of a recording must fail it; frozen parameters and an input without a
gradient must drop exactly the launches they make unnecessary.  tests/test_convnext_stages_gpu.py repeats the walk on real buffers
with bits=True: the producer's output after its call and the consumer's input before its call then also have to agree bit for bit."""
import os
import sys

import pytest
import torch

import multimae_amd as M
from multimae_amd import ops, output_adapters as OA
from stage_recorder import HEAD_OPS, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_convnext import perturb, weight_like  # noqa: E402

# name -> (all tasks in token order, main tasks, interpolate mode, preds_per_patch, C, num_classes, depth, (NH, NW), D, B); patch 16, one
# global token last
CASES = {
    'two_tasks': (('rgb', 'depth'), ('rgb', 'depth'), 'bilinear', 4, 24, 13, 2, (2, 3), 32, 3),
    'gap': (('rgb', 'depth'), ('depth',), 'nearest', 9, 40, 3, 1, (3, 2), 24, 2),
    'tiny': (('rgb',), ('rgb',), 'bilinear', 4, 8, 8, 1, (1, 1), 8, 1),
    'fp32_only': (('rgb',), ('rgb',), 'bilinear', 4, 12, 5, 1, (2, 2), 20, 2),
}


def build_case(name, device='cpu', arena=False):
    """(head, input_info, encoder tokens [B, n_tok, D] requiring grad) of a case: seeded, every parameter perturbed"""
    all_tasks, tasks, mode, p, C, K, depth, (NH, NW), D, B = CASES[name]
    seed = list(CASES).index(name)
    torch.manual_seed(300 + seed)
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                              interpolate_mode=mode)
    head.init(dim_tokens_enc=D)
    perturb(head, 400 + seed)
    head = head.to(device)
    N = NH * NW
    info = {'tasks': {}, 'image_size': (16 * NH, 16 * NW), 'num_task_tokens': N * len(all_tasks), 'num_global_tokens': 1}
    for i, t in enumerate(all_tasks):
        info['tasks'][t] = {'num_tokens': N, 'has_2d_posemb': True, 'start_idx': i * N, 'end_idx': (i + 1) * N}
    g = torch.Generator().manual_seed(500 + seed)
    x = torch.randn(B, N * len(all_tasks) + 1, D, generator=g).to(device).requires_grad_(True)
    if arena:
        M.engine.ParamArena(head)
    return head, info, x


class Run:
    """one recorded forward + backward: rec (the Recording), cfg (the call's _Cfg), head, info, x, y, mode, direct, loss / image
    (whether a gradient came through SegCrossEntropyLoss / through the image), hooked {index in _params(): (data_ptr, shape) of the
    tensor autograd delivered}"""


def run_head(head, info, x, mode, direct=False, wgrad_stream=False, target=None, image=None, names=HEAD_OPS):
    """the gradient comes through the image (weight_like), with `target` through SegCrossEntropyLoss instead, with image=True also both"""
    run = Run()
    run.head, run.info, run.x, run.mode, run.direct, run.loss, run.cfg = head, info, x, mode, direct, target is not None, None
    run.image = target is None if image is None else bool(image)
    assert run.loss or run.image
    run.hooked = {}

    def hook(i):
        def got(g):
            if g is not None:                       # direct mode hands autograd None
                run.hooked[i] = (g.data_ptr(), tuple(g.shape))
        return got
    hooks = [p.register_hook(hook(i)) for i, p in enumerate(head._params()) if p.requires_grad]
    spied = OA._cfg

    def spy(*a, **k):
        run.cfg = spied(*a, **k)
        return run.cfg
    OA._cfg = spy
    old = (M.engine.lazy_predictions(), M.engine.direct_grads(), M.engine.wgrad_stream())
    M.engine.set_lazy_predictions(False)
    M.engine.set_direct_grads(direct)
    M.engine.set_wgrad_stream(wgrad_stream)
    try:
        with M.engine.precision(mode), record(names) as rec:
            run.rec = rec
            y = head(x, info)
            total = 0.0
            if run.loss:
                total = total + M.SegCrossEntropyLoss(ignore_index=255)(y, target)
            if run.image:
                total = total + (y * weight_like(torch.empty(y.shape)).to(y.device)).sum()
            total.backward()
        run.y = y
    finally:
        OA._cfg = spied
        M.engine.set_lazy_predictions(old[0])
        M.engine.set_direct_grads(old[1])
        M.engine.set_wgrad_stream(old[2])
        for h in hooks:
            h.remove()
    return run


# ------------------------------------------------------------------------------------------------- the data-flow graph --
class _Walk:
    def __init__(self, calls):
        self.calls, self.i = calls, 0

    def next(self, name):
        assert self.i < len(self.calls), f'the recording ends where the graph expects {name}'
        c = self.calls[self.i]
        assert c.name == name, f'call {self.i}: the graph expects {name}, recorded {c.name}'
        self.i += 1
        return c


def _bits_equal(a, b):
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.numel() == b.numel() and bool(torch.equal(a.contiguous().view(it).reshape(-1), b.contiguous().view(it).reshape(-1)))


def check_graph(run, calls=None, bits=False):
    """Walks `calls` (default: the run's recording) along the graph of the head.  Raises AssertionError naming the first operand that
    is not the buffer the graph says.  bits=True (real buffers): a producer's output after its call and the consumer's input before
    its call must also hold the same bits -- equal pointers alone can be the allocator handing a freed block out again."""
    head, cfg, info, x = run.head, run.cfg, run.info, run.x
    ps = head._params()
    act, direct = cfg.act, run.direct
    B, n_tok, D = x.shape
    N, NH, NW, s, C, K, H, W, depth = cfg.N, cfg.NH, cfg.NW, cfg.s, cfg.C, cfg.K, cfg.H, cfg.W, cfg.depth
    h, w, T = NH * s, NW * s, len(head.main_tasks)
    R, Kp = B * h * w, (K + 7) // 8 * 8
    fw, fb, pw, pb = ps[8 * depth:8 * depth + 4]
    pptr = {p.data_ptr() for p in ps}
    calls = run.rec.calls if calls is None else calls
    wk = _Walk([c for c in calls if not (c.name == 'cast' and c.a['x'].ptr in pptr)])     # WeightCache's own casts of the weights

    def edge(prod, cons, what):
        assert cons is not None and prod is not None and cons.same_buffer(prod), f'{what}: reads {cons}, the graph says {prod}'
        if bits:
            cb = cons.rows_before if cons.rows_before is not None and cons.rows_before.numel() == prod.after.numel() else cons.before
            assert _bits_equal(prod.after, cb), f'{what}: the bits read are not the bits the producer left in {prod}'

    def param(rec, p, what):
        assert rec is not None and rec.ptr == p.data_ptr() and rec.dtype == torch.float32, f'{what}: {rec} is not the parameter itself'

    def weight(rec, p, what, shape=None):
        wt = cfg.wc(p)
        assert rec.ptr == wt.data_ptr() and rec.dtype == act, f'{what}: {rec} is not what cfg.wc returns for this parameter'
        assert shape is None or rec.shape == shape, (what, rec.shape)
        if bits:
            assert _bits_equal(rec.before.reshape(-1), wt.detach().reshape(-1)), f'{what}: not the bits of cfg.wc(parameter)'

    def grad_dst(rec, acc, idx, what):
        """a parameter-gradient destination: the arena view p.grad, accumulated into (direct) / a fresh tensor, stored, that autograd got"""
        p = ps[idx]
        if not p.requires_grad:
            assert rec is None, f'{what}: a frozen parameter got a destination'
            return
        assert rec is not None, f'{what}: no destination'
        if direct:
            assert rec.ptr == p.grad.data_ptr() and rec.dtype == torch.float32, f'{what}: {rec} is not the arena view p.grad'
            assert acc is True or acc == 1, f'{what}: direct mode must accumulate'
        else:
            assert not acc, f'{what}: autograd mode must store'
            assert run.hooked.get(idx, (None,))[0] == rec.ptr, f'{what}: autograd did not receive {rec} for parameter {idx} of _params()'

    def geom(c, what, **kw):
        for k, v in kw.items():
            assert c.a[k] == v, f'{what}: {k} = {c.a[k]!r}, the graph says {v!r}'

    # ---- forward: gather once per main task, start from input_info, col_off = t D
    x_tok = None
    for t, task in enumerate(head.main_tasks):
        c = wk.next('convnext_rows_gather')
        assert c.a['enc'].ptr == x.data_ptr() and c.a['enc'].shape == (B, n_tok, D), 'gather: not the encoder tokens'
        geom(c, f'gather {task}', start=int(info['tasks'][task]['start_idx']), N=N, col_off=t * D)
        if x_tok is not None:
            edge(x_tok, c.a['out'], f'gather {task}: destination')
        x_tok = c.a['out']
        assert x_tok.shape == (B * N, T * D) and x_tok.dtype == act
    c = wk.next('linear_fwd')
    edge(x_tok, c.a['x'], 'proj_dec: x')
    weight(c.a['w'], pw, 'proj_dec: w')
    param(c.a['bias'], pb, 'proj_dec: bias')
    assert c.a['resid'] is None and c.a['aux'] is None and c.a['epi'] == ops.EPI_NONE
    assert c.a['out'].shape == (B * N, s * s * C) and c.a['out'].dtype == torch.float32
    proj = c.a['out']
    c = wk.next('convnext_shuffle')
    edge(proj, c.a['src'], 'shuffle: src')
    geom(c, 'shuffle', B=B, NH=NH, NW=NW, s=s, C=C, inverse=False)
    xmap = c.a['dst']
    blocks = []
    for i in range(depth):
        dww, dwb, gam, bet, w1, b1, w2, b2 = ps[8 * i:8 * i + 8]
        q = f'block {i} '
        c = wk.next('dwconv7_fwd')
        edge(xmap, c.a['x'], q + 'dwconv7_fwd: x (the previous block output / the shuffle output)')
        param(c.a['w7'], dww, q + 'dwconv7_fwd: weight')
        param(c.a['bias'], dwb, q + 'dwconv7_fwd: bias')
        geom(c, q + 'dwconv7_fwd', B=B, h=h, w=w, C=C)
        t_ = c.a['out']
        c = wk.next('layernorm_fwd')
        edge(t_, c.a['x'], q + 'layernorm_fwd: x')
        param(c.a['gamma'], gam, q + 'layernorm_fwd: gamma')
        param(c.a['beta'], bet, q + 'layernorm_fwd: beta')
        geom(c, q + 'layernorm_fwd', eps=cfg.eps, out_dtype=act)
        n, mean, rstd = c.ret
        c = wk.next('linear_fwd')
        edge(n, c.a['x'], q + 'pwconv1: x')
        weight(c.a['w'], w1, q + 'pwconv1: w')
        param(c.a['bias'], b1, q + 'pwconv1: bias')
        assert c.a['epi'] == ops.EPI_GELU_G and c.a['aux'] is not None and c.a['resid'] is None, q + 'pwconv1: the GELU pair epilogue'
        assert c.a['aux'].shape == (R, 4 * C) and c.a['aux'].dtype == act and c.a['out'].dtype == act
        h1, gp = c.a['out'], c.a['aux']
        c = wk.next('linear_fwd')
        edge(h1, c.a['x'], q + 'pwconv2: x')
        weight(c.a['w'], w2, q + 'pwconv2: w')
        param(c.a['bias'], b2, q + 'pwconv2: bias')
        edge(xmap, c.a['resid'], q + "pwconv2: resid (this block's input map)")
        assert c.a['epi'] == ops.EPI_NONE and c.a['aux'] is None and c.a['out'].dtype == torch.float32
        blocks.append(dict(x=xmap, t=t_, n=n, mean=mean, rstd=rstd, h1=h1, gp=gp))
        xmap = c.a['out']
    c = wk.next('cast')
    edge(xmap, c.a['x'], 'final_layer: cast input')
    geom(c, 'final_layer cast', dtype=act)
    xa = c.ret
    c = wk.next('gemm')
    edge(xa, c.a['A'], 'final_layer: A')
    weight(c.a['B'], fw, 'final_layer: B', shape=(K, C))
    param(c.a['bias'], fb, 'final_layer: bias')
    geom(c, 'final_layer', M=R, N=K, K=C, lda=C, ldb=C, ldc=ops.round_up(K, 8), a_trans=False, b_trans=False, accumulate=False)
    logits = c.a['C']
    assert logits.shape == (R, Kp) and logits.dtype == torch.float32
    c = wk.next('resize_fwd')
    edge(logits, c.a['x'], 'resize_fwd: x')
    geom(c, 'resize_fwd', ldx=Kp, B=B, h=h, w=w, K=K, H=H, W=W, mode=cfg.mode)
    assert c.a['out'].shape == (B, K, H, W)

    # ---- backward
    d_log = d_img = None
    if run.loss:
        c = wk.next('seg_ce_fwd')
        edge(logits, c.a['x'], 'seg_ce_fwd: x')
        c = wk.next('seg_ce_bwd')
        edge(logits, c.a['x'], 'seg_ce_bwd: x')
        geom(c, 'seg_ce_bwd', ldx=Kp, B=B, h=h, w=w, K=K, H=H, W=W, mode=cfg.mode)
        d_log = c.a['dx']
        assert d_log.shape == (R, Kp) and d_log.dtype == torch.float32
    if run.image:
        c = wk.next('resize_bwd')
        geom(c, 'resize_bwd', ldx=Kp, B=B, h=h, w=w, K=K, H=H, W=W, mode=cfg.mode)
        assert c.a['g'].shape == (B, K, H, W)
        d_img = c.a['dx']
        assert d_img.shape == (R, Kp) and d_img.dtype == torch.float32
    c = wk.next('cast')
    if d_log is not None and d_img is not None:          # two gradients of one prediction: added in place onto the loss's buffer
        assert c.a['x'].same_buffer(d_log) and not c.a['x'].same_buffer(d_img), f'logits gradient: the cast reads {c.a["x"]}, not {d_log}'
        if bits:
            assert _bits_equal(c.a['x'].before, d_log.after + d_img.after), 'logits gradient: not the f32 sum of the two gradients'
    else:
        edge(d_log if d_log is not None else d_img, c.a['x'], 'logits gradient: cast input')
    geom(c, 'logits gradient cast', dtype=act)
    d_log_a = c.ret

    def strided_dlog(rec, what):
        """the cast gradient read as [R, K] with row stride round_up(K, 8)"""
        edge(d_log_a, rec, what)
        assert rec.shape == (R, K) and rec.stride == (ops.round_up(K, 8), 1), f'{what}: {rec} is not [R, K] with row stride round_up(K, 8)'

    c = wk.next('linear_dx')
    strided_dlog(c.a['dy'], 'final_layer dX: dy')
    weight(c.a['w'], fw, 'final_layer dX: w', shape=(K, C))
    assert c.a['aux'] is None and c.a['epi'] == ops.EPI_NONE and c.a['out'].shape == (R, C) and c.a['out'].dtype == torch.float32
    dx = c.a['out']
    c = wk.next('linear_dw')
    strided_dlog(c.a['dy'], 'final_layer dW: dy')
    edge(xa, c.a['x'], 'final_layer dW: x')
    grad_dst(c.a['dw'], c.a['accumulate'], 8 * depth, 'final_layer.weight gradient')
    grad_dst(c.a['db'], c.a['db_accumulate'], 8 * depth + 1, 'final_layer.bias gradient')
    for i in reversed(range(depth)):
        dww, dwb, gam, bet, w1, b1, w2, b2 = ps[8 * i:8 * i + 8]
        b, q = blocks[i], f'block {i} backward '
        dy = dx
        c = wk.next('cast')
        edge(dy, c.a['x'], q + 'cast of dy')
        dy_a = c.ret
        c = wk.next('linear_dx')
        edge(dy_a, c.a['dy'], q + 'pwconv2 dX: dy')
        weight(c.a['w'], w2, q + 'pwconv2 dX: w')
        assert c.a['epi'] == ops.EPI_MUL, q + 'pwconv2 dX: the EPI_MUL epilogue'
        edge(b['gp'], c.a['aux'], q + "pwconv2 dX: aux (the GELU' this block's forward GEMM wrote)")
        assert c.a['out'].dtype == act
        d_pre = c.a['out']
        c = wk.next('linear_dx')
        edge(d_pre, c.a['dy'], q + 'pwconv1 dX: dy')
        weight(c.a['w'], w1, q + 'pwconv1 dX: w')
        assert c.a['epi'] == ops.EPI_NONE and c.a['aux'] is None and c.a['out'].dtype == torch.float32
        d_n = c.a['out']
        c = wk.next('linear_dw')
        edge(dy_a, c.a['dy'], q + 'pwconv2 dW: dy')
        edge(b['h1'], c.a['x'], q + "pwconv2 dW: x (this block's h1)")
        grad_dst(c.a['dw'], c.a['accumulate'], 8 * i + 6, q + 'pwconv2.weight gradient')
        grad_dst(c.a['db'], c.a['db_accumulate'], 8 * i + 7, q + 'pwconv2.bias gradient')
        c = wk.next('linear_dw')
        edge(d_pre, c.a['dy'], q + 'pwconv1 dW: dy')
        edge(b['n'], c.a['x'], q + "pwconv1 dW: x (this block's LayerNorm output)")
        grad_dst(c.a['dw'], c.a['accumulate'], 8 * i + 4, q + 'pwconv1.weight gradient')
        grad_dst(c.a['db'], c.a['db_accumulate'], 8 * i + 5, q + 'pwconv1.bias gradient')
        c = wk.next('layernorm_bwd_part')
        edge(d_n, c.a['dy'], q + 'layernorm_bwd_part: dy')
        edge(b['t'], c.a['x'], q + "layernorm_bwd_part: x (this block's dwconv output)")
        param(c.a['gamma'], gam, q + 'layernorm_bwd_part: gamma')
        edge(b['mean'], c.a['mean'], q + 'layernorm_bwd_part: mean')
        edge(b['rstd'], c.a['rstd'], q + 'layernorm_bwd_part: rstd')
        assert c.a['dx_in'] is None and c.a['act_dtype'] is None
        dt, _, part = c.ret
        c = wk.next('colsum_scatter')
        edge(part, c.a['dy'], q + 'colsum_scatter: the partial sums')
        geom(c, q + 'colsum_scatter', seg_w=C)
        assert len(c.a['dsts']) == 3, q + 'colsum_scatter: three segments'
        for d, idx, what in zip(c.a['dsts'], (8 * i + 2, 8 * i + 3, 8 * i + 1), ('norm.weight', 'norm.bias', 'dwconv.bias')):
            grad_dst(d, c.a['accumulate'], idx, q + f'colsum_scatter: {what} gradient')
        if dww.requires_grad:
            c = wk.next('dwconv7_wgrad')
            edge(b['x'], c.a['x'], q + "dwconv7_wgrad: x (this block's input map)")
            edge(dt, c.a['dy'], q + "dwconv7_wgrad: dy (layernorm_bwd_part's dx)")
            geom(c, q + 'dwconv7_wgrad', B=B, h=h, w=w, C=C)
            part7 = c.ret
            c = wk.next('reduce_partials')
            edge(part7, c.a['part'], q + 'reduce_partials: part')
            geom(c, q + 'reduce_partials', accumulate=False)
            gdw = c.a['out']
            if direct:
                c = wk.next('axpy_')
                assert c.a['y'].ptr == dww.grad.data_ptr(), q + 'axpy_: y is not the arena view of dwconv.weight'
                edge(gdw, c.a['x'], q + 'axpy_: x')
                geom(c, q + 'axpy_', a=1.0)
            else:
                assert run.hooked.get(8 * i, (None,))[0] == gdw.ptr, q + 'dwconv.weight: autograd did not receive the reduced gradient'
        c = wk.next('dwconv7_dgrad')
        edge(dt, c.a['dy'], q + "dwconv7_dgrad: dy (layernorm_bwd_part's dx)")
        param(c.a['w7'], dww, q + 'dwconv7_dgrad: weight')
        edge(dy, c.a['dx_in'], q + "dwconv7_dgrad: dx_in (the block's incoming dy, the residual addend)")
        geom(c, q + 'dwconv7_dgrad', B=B, h=h, w=w, C=C)
        dx = c.a['out']
    c = wk.next('convnext_shuffle')
    edge(dx, c.a['src'], 'inverse shuffle: src')
    geom(c, 'inverse shuffle', B=B, NH=NH, NW=NW, s=s, C=C, inverse=True)
    d_proj = c.a['dst']
    c = wk.next('cast')
    edge(d_proj, c.a['x'], 'proj_dec backward: cast input')
    dp_a = c.ret
    if x.requires_grad:
        c = wk.next('linear_dx')
        edge(dp_a, c.a['dy'], 'proj_dec dX: dy')
        weight(c.a['w'], pw, 'proj_dec dX: w')
        assert c.a['epi'] == ops.EPI_NONE and c.a['aux'] is None
        d_tok = c.a['out']
        assert d_tok.shape == (B * N, T * D) and d_tok.dtype == torch.float32
        d_enc = None
        for t, task in enumerate(head.main_tasks):
            c = wk.next('convnext_rows_scatter')
            edge(d_tok, c.a['src'], f'scatter {task}: src')
            geom(c, f'scatter {task}', start=int(info['tasks'][task]['start_idx']), N=N, col_off=t * D)
            if d_enc is None:
                assert c.a['d_enc'].shape == (B, n_tok, D) and c.a['d_enc'].dtype == torch.float32
                assert not c.a['d_enc'].before.any(), 'scatter: the destination is not zero-filled'
            else:
                edge(d_enc, c.a['d_enc'], f'scatter {task}: destination')
            d_enc = c.a['d_enc']
    c = wk.next('linear_dw')
    edge(dp_a, c.a['dy'], 'proj_dec dW: dy')
    edge(x_tok, c.a['x'], 'proj_dec dW: x')
    grad_dst(c.a['dw'], c.a['accumulate'], 8 * depth + 2, 'proj_dec.weight gradient')
    grad_dst(c.a['db'], c.a['db_accumulate'], 8 * depth + 3, 'proj_dec.bias gradient')
    assert wk.i == len(wk.calls), f'{len(wk.calls) - wk.i} recorded call(s) after the end of the graph, first {wk.calls[wk.i]}'
    if direct:
        assert not run.hooked, f'direct mode handed autograd gradients for parameters {sorted(run.hooked)}'
    else:
        want ={i for i, p in enumerate(ps) if p.requires_grad}
        assert set(run.hooked) == want, f'autograd delivered gradients for {sorted(run.hooked)}, the trainable parameters are {sorted(want)}'


# -------------------------------------------------------------------------------------------------------------- tests --
@pytest.fixture()
def stubbed():
    from multimae_amd import _lib
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


def test_recorder_restores_and_records_only_outermost_calls(stubbed):
    """the wrapped functions are put back even when the block raises; a gemm inside linear_fwd is not a stage of its own"""
    before = {n: getattr(ops, n) for n in HEAD_OPS}
    with pytest.raises(RuntimeError, match='boom'):
        with record() as rec:
            assert ops.gemm is not before['gemm']
            x, w = torch.zeros(4, 8), torch.zeros(16, 8)
            base = torch.zeros(4, 24)
            out = base[:, :16]                                  # a strided destination: cloned through its strides, full rows kept
            ops.linear_fwd(x, w, None, out)
            ops.gemm(x, w, base, 4, 16, 8, lda=8, ldb=8, ldc=24)
            raise RuntimeError('boom')
    assert all(getattr(ops, n) is before[n] for n in HEAD_OPS)
    assert [c.name for c in rec.calls] == ['linear_fwd', 'gemm']
    o = rec.calls[0].a['out']
    assert o.ptr == base.data_ptr() and o.shape == (4, 16) and o.stride == (24, 1) and o.dtype == torch.float32
    assert o.before.shape == (4, 16) and o.rows_before.shape == (4, 24) and o.after.shape == (4, 16) and o.rows_after.shape == (4, 24)
    assert rec.calls[0].a['bias'] is None and rec.calls[0].a['epi'] == ops.EPI_NONE and rec.calls[1].a['ldc'] == 24
    assert rec.calls[0].ret.ptr == o.ptr and rec.calls[1].ret is False


@pytest.mark.parametrize('direct', [False, True])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', ['two_tasks', 'gap'])
def test_head_wiring_follows_the_graph(stubbed, name, mode, direct):
    """forward and backward, autograd mode (fresh destinations, stored, handed to autograd in _params() order) and direct mode on a
    ParamArena (the arena views, accumulated into)"""
    head, info, x = build_case(name, arena=direct)
    run = run_head(head, info, x, mode, direct=direct)
    check_graph(run)
    assert x.grad is not None and x.grad.shape == x.shape


@pytest.mark.parametrize('image', [False, True])
def test_head_wiring_with_the_gradient_through_the_loss_handle(stubbed, image):
    """d_logits from SegCrossEntropyLoss through the SegHandle: alone (no resize_bwd) and added in place to the image's gradient"""
    head, info, x = build_case('two_tasks')
    H, W = info['image_size']
    run = run_head(head, info, x, 'bf16', target=torch.zeros(x.shape[0], H, W, dtype=torch.int64), image=image)
    assert len(run.rec.named('resize_bwd')) == int(image) and len(run.rec.named('seg_ce_bwd')) == 1
    check_graph(run)


def test_mis_wired_recordings_fail_the_graph_check(stubbed):
    """no re-run: in copies of one recording, two blocks' GELU' aux entries swapped, and two colsum_scatter destinations swapped"""
    head, info, x = build_case('two_tasks')
    run = run_head(head, info, x, 'bf16')
    check_graph(run)
    calls = run.rec.calls
    mul = [i for i, c in enumerate(calls) if c.name == 'linear_dx' and c.a['epi'] == ops.EPI_MUL]
    assert len(mul) == 2
    swapped = list(calls)
    swapped[mul[0]] = calls[mul[0]].replace(aux=calls[mul[1]].a['aux'])
    swapped[mul[1]] = calls[mul[1]].replace(aux=calls[mul[0]].a['aux'])
    with pytest.raises(AssertionError, match='aux'):
        check_graph(run, swapped)
    cs = [i for i, c in enumerate(calls) if c.name == 'colsum_scatter']
    d = calls[cs[0]].a['dsts']
    swapped = list(calls)
    swapped[cs[0]] = calls[cs[0]].replace(dsts=[d[1], d[0], d[2]])
    with pytest.raises(AssertionError, match='colsum_scatter: norm.weight gradient'):
        check_graph(run, swapped)
    # ... and across blocks: block 1's destinations handed to block 0's reduction
    swapped = list(calls)
    swapped[cs[0]] = calls[cs[0]].replace(dsts=calls[cs[1]].a['dsts'])
    swapped[cs[1]] = calls[cs[1]].replace(dsts=calls[cs[0]].a['dsts'])
    with pytest.raises(AssertionError, match='colsum_scatter'):
        check_graph(run, swapped)


@pytest.mark.parametrize('direct', [False, True])
def test_frozen_and_partial_cases_drop_exactly_their_launches(stubbed, direct):
    head, info, x = build_case('two_tasks', arena=direct)
    full = [c.name for c in run_head(head, info, x, 'bf16', direct=direct).rec.calls]
    # frozen depthwise weights: no dwconv7_wgrad (nor its reduction), everything else as before
    head, info, x = build_case('two_tasks')
    for b in head.blocks:
        b.dwconv.weight.requires_grad_(False)
    if direct:
        M.engine.ParamArena(head)
    run = run_head(head, info, x, 'bf16', direct=direct)
    check_graph(run)
    names = [c.name for c in run.rec.calls]
    assert 'dwconv7_wgrad' not in names and 'reduce_partials' not in names and 'axpy_' not in names
    assert names == [n for n in full if n not in ('dwconv7_wgrad', 'reduce_partials', 'axpy_')]
    # the input does not require a gradient: no scatter, no proj_dec dX
    head, info, x = build_case('two_tasks', arena=direct)
    x = x.detach()
    run = run_head(head, info, x, 'bf16', direct=direct)
    check_graph(run)
    names = [c.name for c in run.rec.calls]
    assert 'convnext_rows_scatter' not in names
    assert names.count('linear_dx') == full.count('linear_dx') - 1 and len(names) == len(full) - 1 - len(head.main_tasks)
    # frozen final_layer.bias: the fused dW + db launch becomes the dW-only launch
    head, info, x = build_case('two_tasks')
    head.final_layer.bias.requires_grad_(False)
    if direct:
        M.engine.ParamArena(head)
    run = run_head(head, info, x, 'bf16', direct=direct)
    check_graph(run)
    assert [c.name for c in run.rec.calls] == full
    dws = run.rec.named('linear_dw')
    assert dws[0].a['db'] is None and dws[0].a['dw'] is not None and all(c.a['db'] is not None for c in dws[1:])
    assert head.final_layer.bias.grad is None
