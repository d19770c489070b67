"""GPU: the classification evaluation kernels (csrc/clseval.hip: mmae_cls_eval) and their host side (multimae_amd.cls_accuracy,
ClsMetric, ops.cls_eval).

Per element against fp64 on the logits as the kernel reads them (bf16 logits are read exactly), with the bounds of
tests/cls_eval_ref.py -- the soft-target loss's bound (tests/test_cls_recipe_gpu.py's module docstring) with a one-hot target:
    lse within b_lse, nll within b_lse + u |lse - z_t|, loss within mean(b_row) + 2 u |loss|
    rank EQUAL to the rank rule restated with comparisons (also the bf16 check: ties are common there and topk no yardstick)
    the percentages bit-equal to fl(fl(c 100) / B), the f64 accumulator equal to MetricLogger's updates on the f32 outputs
The logits sit in rows of ld = round_up(K, 8) elements with NaN in the padding columns, the outputs in Guarded buffers.
Against the golden (the reference's f32 CPU run, no tie at a target): percentages bit-equal, loss within 2 b.
"""
import os
import sys

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import metrics, ops
from helpers import Guarded, assert_within, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from cls_eval_ref import cls_eval_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'cls_eval.npz'))
GEOMS = ((6, 3), (6, 7), (128, 1000), (6, 1001))
ML_SIZES = (6, 128, 5)
KS = (1, 5, 2, 300)


def _case(B, K):
    pre = f'case/{B}x{K}/'
    return torch.from_numpy(GOLD[pre + 'x']), torch.from_numpy(GOLD[pre + 'target'])


def _ml_batch(i, B):
    if f'ml/x{i}' in GOLD.files:
        return torch.from_numpy(GOLD[f'ml/x{i}']), torch.from_numpy(GOLD[f'ml/target{i}'])
    return _case(B, 1000)


def _logits(B, K, dtype, seed, invalid=True):
    """2 randn with a uniform [0, 8) bonus at the target (hits and misses both occur); from B = 6 on, one ignore_index and one
    target one past the last class"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, (B,), generator=g)
    x = torch.randn(B, K, generator=g) * 2
    x[torch.arange(B), t] += torch.rand(B, generator=g) * 8
    if invalid and B >= 6:
        t[1], t[4] = -100, K
    return x.to(dtype), t


def _padded(x):
    B, K = x.shape
    ld = ops.round_up(K, 8)
    xp = torch.full((B, ld), float('nan'), dtype=x.dtype, device=DEV)
    xp[:, :K] = x.to(DEV)
    return xp, ld


def _run(xp, ld, B, K, t, ks, with_acc=True):
    """ops.cls_eval into guarded outputs; returns (lse, nll, rank, out, acc) on the CPU after the guard zones were checked"""
    n = len(ks)
    gl, gn = Guarded(1, B, B, torch.float32, DEV), Guarded(1, B, B, torch.float32, DEV)
    gr, go = Guarded(1, B, B, torch.int32, DEV), Guarded(1, 1 + n, 1 + n, torch.float32, DEV)
    ga = Guarded(1, 3 + n, 3 + n, torch.float64, DEV, fill=torch.zeros(1, 3 + n, dtype=torch.float64)) if with_acc else None
    ops.cls_eval(xp, ld, B, K, t.to(DEV), ks, acc=None if ga is None else ga.view.view(3 + n), lse=gl.view.view(B), nll=gn.view.view(B),
                 rank=gr.view.view(B), out=go.view.view(1 + n))
    torch.cuda.synchronize()
    for g, name in ((gl, 'lse'), (gn, 'nll'), (gr, 'rank'), (go, 'out'), (ga, 'acc')):
        if g is not None:
            g.intact(f'{name} B={B} K={K}')
    return tuple(None if g is None else g.view.reshape(-1).cpu() for g in (gl, gn, gr, go, ga))


def _check(what, xr, t, ks, lse, nll, rank, out, acc=None):
    B = xr.shape[0]
    ref = cls_eval_ref(xr, t, ks)
    assert_within(lse, ref['lse'], ref['b_lse'], what + ' lse', names=('b',))
    assert_within(nll, ref['nll'], ref['b_nll'], what + ' nll', names=('b',))
    assert torch.equal(rank.long(), ref['rank']), (what, rank.tolist(), ref['rank'].tolist())
    err = abs(float(out[0]) - ref['loss'])
    print(f'{what}: loss {float(out[0])!r} ref {ref["loss"]!r} err {err:.3e} bound {ref["b_loss"]:.3e} counts {ref["counts"]}')
    assert err <= ref['b_loss'], (what, float(out[0]), ref['loss'], ref['b_loss'])
    assert np.array_equal(out[1:].numpy().view(np.int32), ref['acc'].view(np.int32)), (what, out[1:].tolist(), ref['acc'].tolist())
    if acc is not None:
        want = [float(out[0]), 1.0, float(B)] + [float(v) * B for v in out[1:]]
        assert acc.tolist() == want, (what, acc.tolist(), want)
    return ref


# ------------------------------------------------------------------------------------------------------------- per element --
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('K', [1, 3, 5, 6, 255, 256, 257, 1000, 1001])
def test_rows_and_batch_values_element_by_element(K, dtype):
    for B in (1, 6, 128):
        x, t = _logits(B, K, dtype, 1000 * K + B)
        xp, ld = _padded(x)
        lse, nll, rank, out, acc = _run(xp, ld, B, K, t, KS)
        ref = _check(f'{dtype} K={K} B={B}', x.double(), t, KS, lse, nll, rank, out, acc)
        if B >= 6:
            assert ref['n_valid'] == B - 2 and int(rank[1]) == K and int(rank[4]) == K and float(nll[1]) == 0.0 and float(nll[4]) == 0.0
    if dtype == torch.bfloat16 and K >= 255:
        x, t = _logits(128, K, dtype, 1000 * K + 128, invalid=False)
        ties = int((x == x.gather(1, t[:, None])).sum()) - 128
        assert ties > 0, 'the bf16 case is meant to hold logits equal to a target\'s'


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_many_classes(dtype):
    """K = 21841 (ImageNet-21k): 86 classes per thread"""
    B, K = 6, 21841
    x, t = _logits(B, K, dtype, 5)
    xp, ld = _padded(x)
    assert ld == 21848
    _check(f'{dtype} K={K}', x.double(), t, (1, 5), *_run(xp, ld, B, K, t, (1, 5)))


# ------------------------------------------------------------------------------------------------------- against the golden --
@pytest.mark.parametrize('B,K', GEOMS)
def test_golden_accuracies_bit_equal_and_loss_within_2b(B, K):
    x, t = _case(B, K)
    xd, td = x.to(DEV), t.to(DEV)
    acc = M.cls_accuracy(xd, td, topk=(1, 5))
    assert all(a.is_cuda and a.shape == () and a.dtype == torch.float32 for a in acc)
    got = torch.stack(acc).cpu().numpy()
    assert np.array_equal(got.view(np.int32), GOLD[f'case/{B}x{K}/acc'].view(np.int32)), (got, GOLD[f'case/{B}x{K}/acc'])
    out = ops.cls_eval(xd, K, B, K, td, (1, 5))[3].cpu()
    ref = cls_eval_ref(x.double(), t, (1, 5))
    gold = float(GOLD[f'case/{B}x{K}/loss'][0])
    print(f'{B}x{K}: loss {float(out[0])!r} golden {gold!r} err {abs(float(out[0]) - gold):.3e} bound 2 x {ref["b_loss"]:.3e}')
    assert abs(float(out[0]) - gold) <= 2 * ref['b_loss']


def test_accumulation_matches_metric_loggers_global_avg(monkeypatch):
    calls = []
    real = ops.cls_eval
    monkeypatch.setattr(ops, 'cls_eval', lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1])
    m = M.ClsMetric(topk=(1, 5), device=DEV)
    bound = 0.0
    for i, B in enumerate(ML_SIZES):
        x, t = _ml_batch(i, B)
        xd, td = x.to(DEV), t.to(DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')                      # update() reads nothing back
        try:
            m.update(xd, td)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        bound += 2 * cls_eval_ref(x.double(), t, (1, 5))['b_loss']
    assert calls == list(ML_SIZES)                                   # every update took the fused path
    m.sync()
    got = m.compute()
    g_loss, g_a1, g_a5 = (float(v) for v in GOLD['ml/global_avg'])
    print(f'global_avg {got} golden loss {g_loss!r} bound {bound / 3:.3e}')
    assert got['acc1'] == g_a1 and got['acc5'] == g_a5
    assert abs(got['loss'] - g_loss) <= bound / len(ML_SIZES)
    assert m.acc.tolist()[1:3] == [3.0, float(sum(ML_SIZES))]
    m.reset()
    assert m.acc.tolist() == [0.0] * 5
    x, t = _case(6, 7)
    m.update(x.to(DEV), t.to(DEV))
    one = m.compute()
    assert one['acc1'] == float(GOLD['case/6x7/acc'][0]) and one['acc5'] == float(GOLD['case/6x7/acc'][1])


def test_two_runs_are_bit_equal():
    B, K = 128, 1001
    x, t = _logits(B, K, torch.float32, 11)
    xp, ld = _padded(x)
    a, b = _run(xp, ld, B, K, t, KS), _run(xp, ld, B, K, t, KS)
    for u, v, name in zip(a, b, ('lse', 'nll', 'rank', 'out', 'acc')):
        assert same_bits(u, v), name


# ------------------------------------------------------------------------------------------------------------ the rank rule --
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_tie_row_on_the_device(dtype):
    """the target's logit again at two lower and two higher indices: rank 2, wrong at k = 2, right at k = 3; and every other target
    of the same row, across the 256-column stride of the threads (K = 600, the copies 300 columns apart)"""
    K = 600
    x = torch.full((6, K), -1.0)
    cols = [10, 150, 300, 450, 599]
    x[:, cols] = 2.5
    x[:, 7] = 1.0
    t = torch.tensor([300, 10, 150, 450, 599, 7])
    xp, ld = _padded(x.to(dtype))
    lse, nll, rank, out, _ = _run(xp, ld, 6, K, t, (2, 3, 5, 6), with_acc=False)
    assert rank.tolist() == [2, 0, 1, 3, 4, 5]
    assert out[1:].tolist() == [float(np.float32(np.float32(c * 100.0) / np.float32(6))) for c in (2, 3, 5, 6)]
    _check(f'tie {dtype}', x.double(), t, (2, 3, 5, 6), lse, nll, rank, out)
    acc = M.cls_accuracy(xp[:1, :K], t[:1].to(DEV), topk=(1, 2, 3))
    assert [float(a) for a in acc] == [0.0, 0.0, 100.0]


def test_out_of_range_ignore_index_and_all_invalid_batches():
    B, K = 5, 7
    x, _ = _logits(B, K, torch.float32, 3, invalid=False)
    best = x.argmax(1)
    t = best.clone()
    t[1], t[3] = 7, -100
    xp, ld = _padded(x)
    lse, nll, rank, out, acc = _run(xp, ld, B, K, t, (1, 5))
    ref = _check('out of range', x.double(), t, (1, 5), lse, nll, rank, out, acc)
    assert ref['n_valid'] == 3 and rank.tolist() == [0, 7, 0, 7, 0] and out[1:].tolist() == [60.0, 60.0]
    assert nll[1] == 0 and nll[3] == 0
    # nothing valid: loss 0 (torch gives NaN), accuracies 0, and the batch still counts
    for bad in (torch.full((B,), -100), torch.full((B,), K), torch.tensor([-1, 7, 2 ** 40, -2 ** 40, 100])):
        lse2, nll2, rank2, out2, acc2 = _run(xp, ld, B, K, bad, (1, 5))
        assert out2.tolist() == [0.0, 0.0, 0.0] and nll2.tolist() == [0.0] * B and rank2.tolist() == [K] * B
        assert acc2.tolist() == [0.0, 1.0, float(B), 0.0, 0.0]
        assert same_bits(lse2, lse)                                  # the log-sum-exp does not depend on the target
    m = M.ClsMetric(topk=(1,))
    m.update(xp[:, :K], torch.full((B,), -100, device=DEV))
    assert m.acc.is_cuda and m.compute() == {'loss': 0.0, 'acc1': 0.0} and m.acc.tolist() == [0.0, 1.0, 5.0, 0.0]


# --------------------------------------------------------------------------------------------------------- which path runs --
def _counted(monkeypatch):
    calls = []
    real = ops.cls_eval
    monkeypatch.setattr(ops, 'cls_eval', lambda *a, **k: (calls.append((a[1], a[2], a[3])), real(*a, **k))[1])
    return calls


def test_strided_view_takes_the_fused_path(monkeypatch):
    calls = _counted(monkeypatch)
    B, K = 6, 1001
    x, t = _logits(B, K, torch.bfloat16, 21)
    xp, ld = _padded(x)                                              # ld = 1008, NaN behind every row
    td = t.to(DEV)
    a = torch.stack(M.cls_accuracy(xp[:, :K], td, topk=(1, 5))).cpu()
    b = torch.stack(M.cls_accuracy(xp[:, :K].contiguous(), td, topk=(1, 5))).cpu()
    assert calls == [(1008, B, K), (K, B, K)]
    assert same_bits(a, b)
    ref = cls_eval_ref(x.double(), t, (1, 5))
    assert np.array_equal(a.numpy().view(np.int32), ref['acc'].view(np.int32))


def test_fp16_logits_take_the_restatement_and_agree_with_the_fused_f32_result(monkeypatch):
    calls = _counted(monkeypatch)
    B, K = 128, 1000
    x, t = _logits(B, K, torch.float16, 31)
    xd, td = x.to(DEV), t.to(DEV)
    m16, m32 = M.ClsMetric(device=DEV), M.ClsMetric(device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                          # the restatement reads nothing back either
    try:
        m16.update(xd, td)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert calls == []
    m32.update(xd.float(), td)                                       # the same values, exactly
    assert calls == [(K, B, K)]
    a16, a32 = m16.acc.cpu(), m32.acc.cpu()
    ref = cls_eval_ref(x.double(), t, (1, 5))
    assert a16[1:].tolist() == a32[1:].tolist()                      # counts and percentages: exact on both paths
    assert abs(float(a16[0]) - ref['loss']) <= ref['b_loss'] and abs(float(a32[0]) - ref['loss']) <= ref['b_loss']
    assert abs(float(a16[0]) - float(a32[0])) <= 2 * ref['b_loss']
    out = metrics._cls_eval_eager(xd, td, (1, 5)).cpu()
    assert np.array_equal(out[1:].numpy().view(np.int32), ref['acc'].view(np.int32))
