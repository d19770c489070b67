"""CPU: host side of the fused segmentation loss and the device mIoU (criterion.SegCrossEntropyLoss, functions.SegHandle / SegCEFn,
metrics.py, dropin/amd_loop.py) against the C ABI stub of dryrun_harness: which path a call takes, the shape of every buffer handed
to a kernel, the laziness of the prediction, the compute() arithmetic, the fixture's own consistency and SegMetric.sync() at world
size 2 on gloo.  Numbers from the stub are garbage by design; the kernels are checked in tests/test_seg_loss_gpu.py."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

import multimae_amd as M
from multimae_amd import _lib, criterion, functions, metrics, ops, output_adapters as OA
from multimae_amd.lazy import LazyPrediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'seg_metrics.npz')


@pytest.fixture()
def stubbed():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


class Recorder:
    """wraps the stub library: records the arguments of the seg kernels"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if not name.startswith(('mmae_seg_', 'mmae_resize_')):
            return fn

        def rec(*args):
            self.calls.append((name, args))
            return fn(*args)
        return rec

    def names(self):
        return [n for n, _ in self.calls]


def _head(K=5, mode='bilinear', p=16):
    head = OA.ConvNeXtAdapter(num_classes=K, embed_dim=16 * p, preds_per_patch=p, main_tasks=('rgb',), depth=1, interpolate_mode=mode)
    head.init(16)
    info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': 6}}, 'image_size': (32, 48)}
    return head, info


def _target(B=2, H=32, W=48, K=5):
    t = torch.randint(0, K, (B, H, W))
    t[:, :3] = 255
    return t


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
def test_fused_path_is_selected_and_never_writes_the_image(stubbed, mode):
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head()
    x = torch.randn(2, 7, 16, requires_grad=True)
    with M.engine.precision(mode):
        y = head(x, info)
        assert isinstance(y, LazyPrediction) and not y.materialized and y.shape == (2, 5, 32, 48)
        h = y._mmae_seg
        assert isinstance(h, functions.SegHandle) and h.geom() == (2, 8, 12, 5, 32, 48, 'bilinear') and h.ld == 8
        assert h.logits.shape == (2 * 8 * 12, 8) and h.logits.dtype == torch.float32 and h.token is not None
        loss = M.SegCrossEntropyLoss(ignore_index=255)(y, _target())
        assert type(loss.grad_fn).__name__ == 'SegCEFnBackward' and loss.shape == () and loss.dtype == torch.float32
        loss.backward()
    assert rec.names() == ['mmae_seg_ce_fwd', 'mmae_seg_ce_bwd']          # no resize in either direction
    fwd, bwd = rec.calls[0][1], rec.calls[1][1]
    assert fwd[1] == 8 and fwd[3] == 255 and fwd[4:11] == (2, 8, 12, 5, 32, 48, 0)
    assert bwd[4:11] == (2, 8, 12, 5, 32, 48, 0)
    assert not y.materialized and h.d_logits is None                      # consumed by the head's backward
    assert x.grad.shape == x.shape and all(p.grad is not None and p.grad.shape == p.shape for p in head.parameters())
    _ = y + 0                                                             # reading it afterwards writes it, from the same logits
    assert y.materialized and rec.names()[-1] == 'mmae_resize_fwd' and rec.calls[-1][1][0] == h.logits.data_ptr()


def test_loss_buffers_have_the_kernels_shapes(stubbed, monkeypatch):
    seen = {}
    real_fwd, real_bwd = ops.seg_ce_fwd, ops.seg_ce_bwd

    def fwd(x, ldx, target, ignore, *geom, **kw):
        lse, out = real_fwd(x, ldx, target, ignore, *geom, **kw)
        seen['fwd'] = (x.shape, ldx, target.dtype, target.is_contiguous(), lse.shape, out.shape)
        return lse, out

    def bwd(x, ldx, target, ignore, B, h, w, K, H, W, mode, lse, out, up, dx):
        seen['bwd'] = (up.shape, up.dtype, dx.shape, dx.dtype)
        return real_bwd(x, ldx, target, ignore, B, h, w, K, H, W, mode, lse, out, up, dx)
    monkeypatch.setattr(ops, 'seg_ce_fwd', fwd)
    monkeypatch.setattr(ops, 'seg_ce_bwd', bwd)
    head, info = _head(K=150, mode='nearest', p=9)
    y = head(torch.randn(1, 7, 16, requires_grad=True), info)
    M.SegCrossEntropyLoss()(y, _target(1, 32, 48, 150).to(torch.int32)).backward()      # any integer dtype: converted with .long()
    assert seen['fwd'] == ((6 * 9, 152), 152, torch.int64, True, (1, 32, 48), (2,))
    assert seen['bwd'] == ((1,), torch.float32, (6 * 9, 152), torch.float32)
    hdr = open(_lib.HEADER).read()
    assert int(re.search(r'#define\s+MMAE_SEG_PARTIALS\s+(\d+)', hdr).group(1)) == ops.SEG_PARTIALS
    assert int(re.search(r'#define\s+MMAE_SEG_HIST_MAX_K\s+(\d+)', hdr).group(1)) == ops.SEG_HIST_MAX_K


FALLBACKS = {
    'modified': (dict(ignore_index=255), lambda y, t: (y * 1, t)),
    'weights': (dict(ignore_index=255, weight=torch.ones(5)), lambda y, t: (y, t)),
    'smoothing': (dict(ignore_index=255, label_smoothing=0.1), lambda y, t: (y, t)),
    'sum': (dict(ignore_index=255, reduction='sum'), lambda y, t: (y, t)),
    'probabilities': (dict(), lambda y, t: (y, torch.rand(2, 5, 32, 48).softmax(1))),        # torch takes no ignore_index with these
}


@pytest.mark.parametrize('case', list(FALLBACKS))
def test_everything_else_is_torchs_loss_on_the_image(stubbed, case):
    rec = _lib._lib = Recorder(_lib._lib)
    kw, prep = FALLBACKS[case]
    head, info = _head()
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    with torch.no_grad():
        y._mmae_plain.data.zero_()                                             # the stub writes nothing: give torch finite numbers
    inp, tgt = prep(y, _target())
    loss = M.SegCrossEntropyLoss(**kw)(inp, tgt)
    assert type(loss.grad_fn).__name__ != 'SegCEFnBackward' and y.materialized
    assert torch.equal(loss.detach(), nn.CrossEntropyLoss(**kw)(torch.zeros(2, 5, 32, 48), tgt))
    loss.backward()
    assert 'mmae_seg_ce_fwd' not in rec.names() and rec.names().count('mmae_resize_fwd') == 1 and 'mmae_resize_bwd' in rec.names()


def test_eager_mode_and_wrong_target_size(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head()
    M.engine.set_lazy_predictions(False)
    try:
        y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    finally:
        M.engine.set_lazy_predictions(True)
    assert rec.names() == ['mmae_resize_fwd'] and y.materialized          # written by the forward, as before
    assert type(nn.CrossEntropyLoss(ignore_index=255)(y, _target()).grad_fn).__name__ != 'SegCEFnBackward'
    y2 = head(torch.randn(2, 7, 16, requires_grad=True), info)
    with pytest.raises((RuntimeError, ValueError)):                       # torch's own complaint about a (B, 16, 48) target
        M.SegCrossEntropyLoss()(y2, _target(2, 16, 48))
    assert y2.materialized
    assert criterion._seg_handle(torch.zeros(2, 5, 32, 48)) is None


def test_two_losses_on_one_prediction_add_their_gradients(stubbed, monkeypatch):
    head, info = _head()
    y = head(torch.randn(2, 7, 16, requires_grad=True), info)
    h, fills = y._mmae_seg, iter([1.0, 2.0])
    monkeypatch.setattr(ops, 'seg_ce_bwd', lambda *a: a[-1].fill_(next(fills)))
    crit = M.SegCrossEntropyLoss()
    seen = {}
    real = ops.cast

    def cast(t, dt, *a, **k):
        if t.shape == h.logits.shape and 'd' not in seen:
            seen['d'] = t.clone()
        return real(t, dt, *a, **k)
    monkeypatch.setattr(ops, 'cast', cast)
    (crit(y, _target()) + crit(y.clone(), _target())).backward()          # clone() keeps the side channel (DDP's output sink)
    assert torch.equal(seen['d'], torch.full_like(h.logits, 3.0)) and not y.materialized


def test_seg_argmax_paths(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    head, info = _head()
    with torch.no_grad():
        y = head(torch.randn(2, 7, 16), info)
        a = M.seg_argmax(y, 4)
    assert a.shape == (2, 32, 48) and a.dtype == torch.int64 and not y.materialized
    assert rec.names() == ['mmae_seg_argmax'] and rec.calls[0][1][2:10] == (2, 8, 12, 5, 4, 32, 48, 0)
    plain = torch.randn(2, 5, 6, 7)
    assert torch.equal(M.seg_argmax(plain, 3), plain[:, :3].argmax(1)) and rec.names() == ['mmae_seg_argmax']
    with torch.no_grad():
        y._mmae_plain.data.zero_()
    assert torch.equal(M.seg_argmax(y * 1, 4), torch.zeros(2, 32, 48, dtype=torch.int64)) and y.materialized


def test_seg_metric_host_logic(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    m = M.SegMetric(5, 255)
    t = _target()
    m.update(torch.randint(0, 5, (2, 32, 48), dtype=torch.int32), t)      # a class map
    head, info = _head()
    with torch.no_grad():
        m.update(head(torch.randn(2, 7, 16), info), t)                    # a prediction: fused argmax first
    assert rec.names() == ['mmae_seg_hist', 'mmae_seg_argmax', 'mmae_seg_hist']
    assert m.hist.shape == (4, 5) and m.hist.dtype == torch.int64
    assert rec.calls[0][1][2:5] == (2 * 32 * 48, 5, 255) and rec.calls[0][1][5] == m.hist.data_ptr()
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 16, 48, dtype=torch.int64), t)
    with pytest.raises(ValueError):
        M.SegMetric(ops.SEG_HIST_MAX_K + 1)
    m.sync()                                                              # torch.distributed not initialised: nothing to do


def test_amd_loop_helpers_return_the_engine_classes():
    from dropin import amd_loop
    c = amd_loop.seg_criterion(254)
    assert type(c) is criterion.SegCrossEntropyLoss and isinstance(c, nn.CrossEntropyLoss) and c.ignore_index == 254
    m = amd_loop.seg_metric(150, 255)
    assert type(m) is metrics.SegMetric and (m.num_classes, m.ignore_index) == (150, 255)
    assert M.SegCrossEntropyLoss is criterion.SegCrossEntropyLoss and M.SegMetric is metrics.SegMetric


def test_compute_is_eval_metrics_arithmetic():
    hist = np.array([[3, 0, 5, 0], [6, 2, 5, 0], [4, 2, 5, 0], [5, 0, 5, 0]])
    m = M.SegMetric(4)
    m.hist = torch.from_numpy(hist)
    all_acc, acc, iou = m.compute()
    assert all_acc == 8 / 10
    assert np.array_equal(acc[[0, 2]], [3 / 5, 1.0]) and np.isnan(acc[1]) and np.isnan(acc[3])     # 0 / 0: absent from the labels
    assert np.array_equal(iou[:3], [0.5, 0.0, 1.0]) and np.isnan(iou[3])                        # absent from both


def test_fixture_is_consistent_with_a_numpy_restatement():
    z = np.load(GOLD)
    cases = sorted({k.split('/')[0] for k in z.files})
    assert cases == ['absent', 'ade', 'small']
    for c in cases:
        for part in '01':
            pred, label, hist = (z[f'{c}/{part}/{n}'].astype(np.int64) for n in ('pred', 'label', 'hist'))
            K = hist.shape[1]
            assert set(np.unique(label)) <= set(range(K)) | {255} and pred.max() < K
            keep = label != 255
            p, l = pred[keep], label[keep]
            cp, cl, ci = np.bincount(p, minlength=K), np.bincount(l, minlength=K), np.bincount(p[p == l], minlength=K)
            assert np.array_equal(hist, np.stack([ci, cp + cl - ci, cp, cl]))
    h = z['absent/0/hist'] + z['absent/1/hist']
    assert h[3, -1] == 0 and h[2, -1] == 0 and np.isnan(metrics.ratios(h)[2][-1])


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _sync_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        z = np.load(GOLD)
        m = M.SegMetric(150, 255)
        m.hist = torch.from_numpy(z[f'ade/{rank}/hist'].copy())           # what this rank's update() calls would have left
        m.sync()
        total = z['ade/0/hist'] + z['ade/1/hist']
        ok = np.array_equal(m.hist.numpy(), total)
        ref = metrics.ratios(total)
        ok = ok and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(m.compute(), ref))
        q.put((rank, bool(ok), ''))
        dist.destroy_process_group()
    except Exception as e:                                                # surface failures instead of a queue timeout
        q.put((rank, False, repr(e)))


def test_seg_metric_sync_world2_gloo():
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
