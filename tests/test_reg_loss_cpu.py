"""CPU: host side of the fused regression losses and the device depth metrics (criterion.masked_l1_loss / masked_mse_loss /
masked_berhu_loss, functions.RegLossFn, metrics.depth_metrics / DepthMetric, dropin/amd_loop.py) against the C ABI stub of
dryrun_harness: which path a call takes, the shape of every buffer handed to a kernel, the laziness of the prediction, the eager
restatement against the reference's recorded values (tests/golden/reg_loss.npz), DepthMetric's arithmetic and its sync() at world
size 2 on gloo.  Numbers from the stub are garbage by design; the kernels are checked in tests/test_reg_loss_gpu.py.

Bound of the eager restatement against the fixture (u = 2^-24).  Both evaluate the same f32 element-wise expressions with torch on
the CPU; what may differ is the order of the sums (masked_select + sum there, where + sum here) and, for berHu, c^2 (1e-10 rounded
from double there when c is the floor, c c in f32 here: one rounding of a term).  Every summed term is non-negative, so any two f32
summation orders of N terms agree within 2 gamma_N of the sum; the division adds one rounding on each side, a root halves the relative
error.  With N <= B K H W = 1326:  |value - golden| <= (2 gamma_(N + 8) + 4 u) |golden|."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import multimae_amd as M
from multimae_amd import _lib, criterion, functions, metrics, ops, output_adapters as OA
from multimae_amd.lazy import LazyPrediction
from helpers import gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'reg_loss.npz')
U = 2.0 ** -24
LOSSES = {'l1': M.masked_l1_loss, 'mse': M.masked_mse_loss, 'berhu': M.masked_berhu_loss}
KEYS = ('rmse', 'rel', 'srel', 'log10', 'delta_1', 'delta_2', 'delta_3')


@pytest.fixture()
def stubbed():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


class Recorder:
    """wraps the stub library: records the arguments of the regression, metric and resize kernels"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not name.startswith(('mmae_reg_', 'mmae_depth_metrics', 'mmae_resize_')):
            return fn

        def rec(*args):
            self.calls.append((name, args))
            return fn(*args)
        return rec

    def names(self):
        return [n for n, _ in self.calls]


def _head(K=1, mode='bilinear', p=64, C=8):
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=C * p, preds_per_patch=p, main_tasks=('rgb',), depth=1, interpolate_mode=mode)
    head.init(16)
    info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': 6}}, 'image_size': (32, 48)}
    return head, info


def _data(K=1, Cm=1, B=2, H=32, W=48):
    g = torch.Generator().manual_seed(3)
    return torch.randn(B, K, H, W, generator=g), torch.rand(B, Cm, H, W, generator=g) < 0.7


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind', list(LOSSES))
def test_fused_path_is_selected_and_never_writes_the_image(stubbed, mode, kind):
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head()
    x = torch.randn(2, 7, 16, requires_grad=True)
    target, mask = _data()
    with M.engine.precision(mode):
        y = head(x, info)
        assert isinstance(y, LazyPrediction) and not y.materialized and y.shape == (2, 1, 32, 48)
        h = y._mmae_seg
        assert isinstance(h, functions.SegHandle) and h.geom() == (2, 16, 24, 1, 32, 48, 'bilinear') and h.ld == 8
        assert y.float() is y                                                 # preds[task].float() keeps the side channel
        loss = LOSSES[kind](y.float(), target, mask)
        assert type(loss.grad_fn).__name__ == 'RegLossFnBackward' and loss.shape == () and loss.dtype == torch.float32
        loss.backward()
    assert rec.names() == ['mmae_reg_loss_fwd', 'mmae_reg_loss_bwd']          # no resize in either direction
    fwd, bwd = rec.calls[0][1], rec.calls[1][1]
    assert fwd[0] == h.logits.data_ptr() and fwd[1] == 8 and fwd[4:13] == (1, ops.REG_KINDS[kind], 2, 16, 24, 1, 32, 48, 0)
    assert bwd[3:11] == (ops.REG_KINDS[kind], 2, 16, 24, 1, 32, 48, 0) and bwd[12] == 8
    assert not y.materialized and h.d_logits is None                          # consumed by the head's backward
    assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in head.parameters())
    _ = y + 0                                                                 # reading it afterwards writes it, from the same map
    assert y.materialized and rec.names()[-1] == 'mmae_resize_fwd' and rec.calls[-1][1][0] == h.logits.data_ptr()


@pytest.mark.parametrize('K,Cm', [(1, 1), (3, 1), (3, 3), (3, None)])
def test_loss_buffers_have_the_kernels_shapes(stubbed, monkeypatch, K, Cm):
    seen = {}
    real_fwd, real_bwd = ops.reg_loss_fwd, ops.reg_loss_bwd

    def fwd(x, ldx, target, mask, kind, *geom, **kw):
        diff, out = real_fwd(x, ldx, target, mask, kind, *geom, **kw)
        seen['fwd'] = (x.shape, ldx, target.dtype, target.is_contiguous(), None if mask is None else (mask.dtype, tuple(mask.shape)),
                       diff.shape, diff.dtype, out.shape)
        return diff, out

    def bwd(diff, out, up, kind, B, h, w, K_, H, W, mode, dx, ldx):
        seen['bwd'] = (diff.shape, out.shape, up.shape, up.dtype, dx.shape, dx.dtype, ldx)
        return real_bwd(diff, out, up, kind, B, h, w, K_, H, W, mode, dx, ldx)
    monkeypatch.setattr(ops, 'reg_loss_fwd', fwd)
    monkeypatch.setattr(ops, 'reg_loss_bwd', bwd)
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head(K=K, mode='nearest', p=9)
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    target, mask = _data(K, Cm or 1)
    target = target.transpose(2, 3).contiguous().transpose(2, 3)                # not contiguous: made so by the loss
    M.masked_berhu_loss(y, target, mask if Cm else None).backward()
    assert seen['fwd'] == ((2 * 6 * 9, 8), 8, torch.float32, True, (torch.bool, (2, Cm, 32, 48)) if Cm else None, (2, K, 32, 48),
                           torch.float32, (4,))
    assert seen['bwd'] == ((2, K, 32, 48), (4,), (1,), torch.float32, (2 * 6 * 9, 8), torch.float32, 8)
    args = rec.calls[0][1]
    assert (args[3] is None) == (Cm is None) and args[4] == (Cm or 1) and args[12] == 1
    hdr = open(_lib.HEADER).read()
    assert int(re.search(r'#define\s+MMAE_REG_PARTIALS\s+(\d+)', hdr).group(1)) == ops.REG_PARTIALS
    assert int(re.search(r'#define\s+MMAE_REG_MAX_K\s+(\d+)', hdr).group(1)) == ops.REG_MAX_K == 16
    assert _lib.load().mmae_abi_version() == 7


def _zero_image_value(kind, target, mask):
    """the three formulas on a zero prediction, written out (the stub writes nothing, the test zeroes the image)"""
    valid = torch.ones_like(target, dtype=torch.bool) if mask is None else mask.expand_as(target)
    d = torch.where(valid, -target, torch.zeros(()))
    if kind == 'l1':
        e = d.abs()
    elif kind == 'mse':
        e = d * d
    else:
        c = max(float(d.abs().max()) * 0.2, 1e-5)
        c = torch.tensor(c, dtype=torch.float32)
        e = torch.where(d.abs() < c, d.abs(), (d * d + c * c) / 2. / c)
    return e.sum() / valid.sum()


FALLBACKS = {
    'modified': dict(prep=lambda y, t, m: (y * 1, t, m)),
    'more_than_16_channels': dict(K=17, C=24),
    'double_target': dict(prep=lambda y, t, m: (y, t.double(), m)),
    'integer_mask': dict(prep=lambda y, t, m: (y, t, m.to(torch.uint8))),
    'target_of_another_shape': dict(prep=lambda y, t, m: (y, t[:, :, :1], None)),
}


@pytest.mark.parametrize('kind', list(LOSSES))
@pytest.mark.parametrize('case', list(FALLBACKS))
def test_everything_else_is_the_eager_restatement_on_the_image(stubbed, case, kind):
    rec = _lib._lib = Recorder(_lib._lib)
    spec = FALLBACKS[case]
    K = spec.get('K', 3)
    head, info = _head(K=K, p=16, C=spec.get('C', 8))
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    with torch.no_grad():
        y._mmae_plain.data.zero_()                                             # the stub writes nothing: give torch finite numbers
    target, mask = _data(K, 1)
    inp, tgt, msk = spec.get('prep', lambda y, t, m: (y, t, m))(y, target, mask)
    loss = LOSSES[kind](inp, tgt, msk)
    assert type(loss.grad_fn).__name__ != 'RegLossFnBackward' and y.materialized
    ref = _zero_image_value(kind, tgt.float() if case != 'target_of_another_shape' else tgt.expand(2, K, 32, 48),
                            None if msk is None else msk.bool())
    assert torch.allclose(loss.detach().float(), ref, rtol=1e-5, atol=0), (float(loss), float(ref))
    loss.backward()
    assert 'mmae_reg_loss_fwd' not in rec.names() and rec.names().count('mmae_resize_fwd') == 1 and 'mmae_resize_bwd' in rec.names()


def test_a_cpu_tensor_and_eager_mode_take_the_eager_path(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    target, mask = _data()
    plain = torch.randn(2, 1, 32, 48, requires_grad=True)
    for kind, fn in LOSSES.items():
        loss = fn(plain, target, mask)
        assert type(loss.grad_fn).__name__ != 'RegLossFnBackward'
    assert rec.names() == [] and criterion._seg_handle(plain) is None
    head, info = _head()
    M.engine.set_lazy_predictions(False)
    try:
        y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    finally:
        M.engine.set_lazy_predictions(True)
    assert y.materialized and rec.names() == ['mmae_resize_fwd']              # written by the forward, as before


@pytest.mark.parametrize('K,c', [(1, 1), (3, 1), (3, 3)])
def test_eager_restatement_reproduces_the_references_losses(K, c):
    z = np.load(GOLD)
    pre = f'loss/K{K}/'
    pred, target = torch.from_numpy(z[pre + 'pred']), torch.from_numpy(z[pre + 'target'])
    N = pred.numel()
    names = sorted({k.split('/')[4] for k in z.files if k.startswith(f'{pre}l1/c{c}/')})
    assert set(names) >= {'all', 'block', 'image', 'random', 'empty'}
    for kind, fn in LOSSES.items():
        for name in names:
            mask = None if name == 'none' else torch.from_numpy(z[f'{pre}mask/c{c}/{name}'])
            gold = float(z[f'{pre}{kind}/c{c}/{name}/loss'][0])
            got = float(fn(pred, target, mask))
            if name == 'empty':
                assert np.isnan(gold) and np.isnan(got)                       # 0 / 0 stays NaN on the eager path
                continue
            bound = (2 * gamma(N + 8) + 4 * U) * abs(gold)
            print(kind, K, c, name, got, gold, bound)
            assert abs(got - gold) <= bound, (kind, name, got, gold, bound)


def test_eager_restatement_reproduces_the_references_metrics():
    z = np.load(GOLD)
    assert tuple(z['metric/mean_std']) == (metrics.NYU_MEAN, metrics.NYU_STD)
    for case in ('none', 'block', 'image', 'random', 'clamp'):
        pre = f'metric/{case}/'
        pred, target = torch.from_numpy(z[pre + 'pred']), torch.from_numpy(z[pre + 'target'])
        mask = torch.from_numpy(z[pre + 'mask']) if pre + 'mask' in z.files else None
        got = M.depth_metrics(pred, target, mask)
        assert tuple(got) == KEYS and all(v.shape == () and v.dtype == torch.float32 for v in got.values())
        gold = z[pre + 'values']
        for k, g in zip(KEYS, gold):
            bound = (2 * gamma(pred.numel() + 8) + 4 * U) * abs(float(g))
            print(case, k, float(got[k]), float(g), bound)
            assert abs(float(got[k]) - float(g)) <= bound, (case, k)
    got = M.depth_metrics(pred, target, torch.zeros_like(pred, dtype=torch.bool))      # nothing valid: 0 / 0, as the reference
    assert all(np.isnan(float(v)) for v in got.values())


def test_two_losses_on_one_prediction_add_their_gradients(stubbed, monkeypatch):
    head, info = _head(K=3, p=16)
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    h, fills = y._mmae_seg, iter([1.0, 2.0])
    monkeypatch.setattr(ops, 'reg_loss_bwd', lambda *a: a[-2].fill_(next(fills)))
    seen = {}
    real = ops.cast

    def cast(t, dt, *a, **k):
        if t.shape == h.logits.shape and 'd' not in seen:
            seen['d'] = t.clone()
        return real(t, dt, *a, **k)
    monkeypatch.setattr(ops, 'cast', cast)
    target, mask = _data(3, 1)
    (M.masked_l1_loss(y, target, mask) + M.masked_berhu_loss(y.clone(), target)).backward()    # clone() keeps the side channel
    assert torch.equal(seen['d'], torch.full_like(h.logits, 3.0)) and not y.materialized


def test_target_modified_in_place_is_refused(stubbed):
    head, info = _head()
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    target, mask = _data()
    loss = M.masked_mse_loss(y, target, mask)
    target.add_(1)
    with pytest.raises(RuntimeError, match='modified in place'):
        loss.backward()


def test_depth_metrics_paths(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head()
    target, mask = _data()
    with torch.no_grad():
        y = head(torch.randn(2, 7, 16), info)
        got = M.depth_metrics(y, target, mask)
    assert tuple(got) == KEYS and not y.materialized and rec.names() == ['mmae_depth_metrics']
    a = rec.calls[0][1]
    assert a[0] == y._mmae_seg.logits.data_ptr() and a[1] == 8 and a[6:12] == (2, 16, 24, 32, 48, 0) and a[14] is None
    assert a[4] == metrics.NYU_MEAN and a[5] == metrics.NYU_STD
    m = M.DepthMetric()
    m.update(y, target, mask, loss=torch.tensor(2.0))
    m.update(y, target, None, loss=torch.tensor(4.0))
    assert rec.names() == ['mmae_depth_metrics'] * 3 and rec.calls[1][1][14] == m.acc.data_ptr() and rec.calls[2][1][3] is None
    assert m.acc.shape == (8,) and m.acc.dtype == torch.float32 and not y.materialized
    with pytest.raises(ValueError):
        m.update(y, target, mask, other=torch.tensor(1.0))
    with torch.no_grad():
        y3 = _head(K=3, p=16)[0](torch.randn(2, 7, 16), info)                   # K = 3: not the depth kernel's case
        y3._mmae_plain.data.zero_()
        M.depth_metrics(y3, _data(3)[0], None)
    assert y3.materialized and rec.names()[-1] == 'mmae_resize_fwd'
    m.sync()                                                                  # torch.distributed not initialised: nothing to do


def test_depth_metric_averages_per_update():
    """MetricLogger's global_avg: the mean over the updates of the per-batch values, not a sum pooled over the pixels"""
    z = np.load(GOLD)
    m = M.DepthMetric()
    cases = ('none', 'image', 'random')                                        # different valid counts: a pooled sum would differ
    for i, case in enumerate(cases):
        pre = f'metric/{case}/'
        mask = torch.from_numpy(z[pre + 'mask']) if pre + 'mask' in z.files else None
        m.update(torch.from_numpy(z[pre + 'pred']), torch.from_numpy(z[pre + 'target']), mask, loss=torch.tensor(float(i + 1)))
    got = m.compute()
    assert list(got) == list(KEYS) + ['loss'] and got['loss'] == 2.0
    mean = np.mean([z[f'metric/{c}/values'].astype(np.float64) for c in cases], axis=0)
    for k, g in zip(KEYS, mean):
        assert abs(got[k] - g) <= (2 * gamma(890) + 8 * U) * abs(g), k        # the per-case bound + the f32 running total
    m.reset()
    assert not m.acc.any()


def test_amd_loop_helpers_return_the_engine_functions():
    from dropin import amd_loop
    assert amd_loop.depth_criterion('l1') == {'depth': criterion.masked_l1_loss}
    assert amd_loop.depth_criterion('berhu') == {'depth': criterion.masked_berhu_loss}
    assert amd_loop.depth_criterion('mse') == {'depth': criterion.masked_mse_loss}
    with pytest.raises(ValueError):
        amd_loop.depth_criterion('huber')
    assert amd_loop.taskonomy_criterion(['rgb', 'normal']) == {'rgb': criterion.masked_l1_loss, 'normal': criterion.masked_l1_loss}
    assert type(amd_loop.depth_metric()) is metrics.DepthMetric
    assert M.masked_berhu_loss is criterion.masked_berhu_loss and M.DepthMetric is metrics.DepthMetric
    assert M.masked_l1_loss is criterion.masked_l1_loss and M.masked_mse_loss is criterion.masked_mse_loss


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _sync_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        m = M.DepthMetric()
        m.names = list(KEYS) + ['loss']
        m.acc = torch.arange(8, dtype=torch.float32) * (rank + 1)              # what this rank's updates would have left
        m.acc[7] = 2 + rank                                                   # 2 and 3 updates
        m.extra = torch.tensor([10.0 * (rank + 1)])
        m.sync()
        ok = torch.equal(m.acc, torch.tensor([0., 3., 6., 9., 12., 15., 18., 5.])) and torch.equal(m.extra, torch.tensor([30.0]))
        got = m.compute()
        ok = ok and got == {**{k: 3.0 * i / 5.0 for i, k in enumerate(KEYS)}, 'loss': 6.0}
        q.put((rank, bool(ok), repr(got)))
        dist.destroy_process_group()
    except Exception as e:                                                    # surface failures instead of a queue timeout
        q.put((rank, False, repr(e)))


def test_depth_metric_sync_world2_gloo():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(timeout=60)
    for rank, ok, why in res:
        assert ok, f'rank {rank}: {why}'


def test_a_head_prediction_is_refused_while_a_graph_is_captured(stubbed, monkeypatch):
    """capture of a head + regression-loss step is unsupported: the losses and the metrics raise for the head's prediction (fused or
    not) under graph.StepGraph's capture and under a plain torch.cuda.graph capture, before anything is launched; a tensor without
    the head's side channel is none of their business"""
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head()
    target, mask = _data()
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    plain = torch.randn(2, 1, 32, 48)
    for arm in ('step_graph', 'torch_graph'):
        with monkeypatch.context() as mp_:
            if arm == 'step_graph':
                mp_.setattr(M.engine, '_capture', object())
            else:
                mp_.setattr(torch.cuda, 'is_available', lambda: True)
                mp_.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
            for fn in LOSSES.values():
                with pytest.raises(RuntimeError, match='unsupported and untested'):
                    fn(y.float(), target, mask)
                assert fn(plain, target, mask).shape == ()
            with pytest.raises(RuntimeError, match='unsupported and untested'):
                M.depth_metrics(y, target, mask)
            with pytest.raises(RuntimeError, match='unsupported and untested'):
                M.DepthMetric().update(y.clone(), target, mask)
    assert rec.names() == [] and not y.materialized
    assert type(M.masked_l1_loss(y, target, mask).grad_fn).__name__ == 'RegLossFnBackward'        # and nothing sticks afterwards
