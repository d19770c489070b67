"""CPU: the classification evaluation's host side (multimae_amd.metrics.cls_accuracy / ClsMetric, ops.cls_eval,
dropin.amd_loop.cls_metric) and the C ABI entry mmae_cls_eval.

* the eager restatement (metrics._cls_eval_eager, what every CPU tensor takes) against the golden fixture
  (tests/golden/make_golden_cls_eval.py: the reference's ``accuracy``, ``nn.CrossEntropyLoss`` and ``MetricLogger`` on the CPU): the
  percentages bit for bit, the loss within 2 b (tests/cls_eval_ref.py), ``ClsMetric``'s three ``global_avg`` values;
* the tie rule, K < 5, targets outside [0, K), more than four thresholds;
* which path a call takes, against the C ABI stub of dryrun_harness with a call recorder (numbers from the stub are garbage by design;
  the kernels are checked in tests/test_cls_eval_gpu.py);
* the entry point of the built library: declared, exported, refusing bad arguments before anything touches a device.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, metrics, ops
from dropin import amd_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from cls_eval_ref import cls_eval_ref, pct, rank_ref  # noqa: E402

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'cls_eval.npz'))
GEOMS = ((6, 3), (6, 7), (128, 1000), (6, 1001))
ML_SIZES = (6, 128, 5)


def _case(B, K):
    pre = f'case/{B}x{K}/'
    return torch.from_numpy(GOLD[pre + 'x']), torch.from_numpy(GOLD[pre + 'target'])


def _ml_batch(i, B):
    if f'ml/x{i}' in GOLD.files:
        return torch.from_numpy(GOLD[f'ml/x{i}']), torch.from_numpy(GOLD[f'ml/target{i}'])
    return _case(B, 1000)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------- against the golden --
def test_fixture_has_no_tie_at_a_target_and_covers_hits_and_misses():
    seen = set()
    for B, K in GEOMS:
        x, t = _case(B, K)
        assert x.shape == (B, K) and x.dtype == torch.float32 and t.dtype == torch.int64
        assert int((x == x.gather(1, t[:, None])).sum()) == B
        seen |= {float(v) for v in GOLD[f'case/{B}x{K}/acc']}
    assert any(0 < v < 100 for v in seen)
    a1, a5 = GOLD['case/128x1000/acc']
    assert 0 < a1 < a5 < 100


@pytest.mark.parametrize('B,K', GEOMS)
def test_eager_restatement_reproduces_the_reference(B, K):
    x, t = _case(B, K)
    acc = M.cls_accuracy(x, t, topk=(1, 5))
    assert len(acc) == 2 and all(a.shape == () and a.dtype == torch.float32 for a in acc)
    got = np.array([float(a) for a in acc], dtype=np.float32)
    assert np.array_equal(_bits(got), _bits(GOLD[f'case/{B}x{K}/acc'])), (got, GOLD[f'case/{B}x{K}/acc'])
    out = metrics._cls_eval_eager(x, t, (1, 5))
    assert out.shape == (3,) and out.dtype == torch.float32
    ref = cls_eval_ref(x.double(), t, (1, 5))
    gold = float(GOLD[f'case/{B}x{K}/loss'][0])
    print(f'{B}x{K}: loss {float(out[0])!r} golden {gold!r} fp64 {ref["loss"]!r} bound 2 x {ref["b_loss"]:.3e}')
    assert abs(float(out[0]) - gold) <= 2 * ref['b_loss']
    assert abs(float(out[0]) - ref['loss']) <= ref['b_loss'] and abs(gold - ref['loss']) <= ref['b_loss']
    assert np.array_equal(_bits(out[1:].numpy()), _bits(ref['acc']))


def test_cls_metric_reproduces_metric_loggers_global_avg():
    m = M.ClsMetric()
    assert m.topk == (1, 5) and m.acc is None
    bound = 0.0
    for i, B in enumerate(ML_SIZES):
        x, t = _ml_batch(i, B)
        assert x.shape == (B, 1000)
        m.update(x, t)
        bound += 2 * cls_eval_ref(x.double(), t, (1, 5))['b_loss']
    assert m.acc.dtype == torch.float64 and m.acc.shape == (5,) and float(m.acc[1]) == 3 and float(m.acc[2]) == sum(ML_SIZES)
    m.sync()                                                          # no process group: a no-op
    got = m.compute()
    assert list(got) == ['loss', 'acc1', 'acc5'] and all(type(v) is float for v in got.values())
    g_loss, g_a1, g_a5 = (float(v) for v in GOLD['ml/global_avg'])
    assert got['acc1'] == g_a1 and got['acc5'] == g_a5                # the same f64 operations in the same order
    print(f'global_avg loss {got["loss"]!r} golden {g_loss!r} bound {bound / 3:.3e}')
    assert abs(got['loss'] - g_loss) <= bound / len(ML_SIZES)
    m.reset()
    assert float(m.acc.abs().sum()) == 0
    x, t = _case(6, 7)
    m.update(x, t)
    one = m.compute()
    assert one['acc1'] == float(GOLD['case/6x7/acc'][0]) and one['acc5'] == float(GOLD['case/6x7/acc'][1])


# ------------------------------------------------------------------------------------------------------------ the rank rule --
def _tie_row():
    """K = 9, target 4: its logit again at indices 1, 2 (rank before it) and 6, 8 (after it); everything else smaller"""
    x = torch.tensor([[-1.0, 2.5, 2.5, 0.0, 2.5, -3.0, 2.5, 1.0, 2.5]])
    return x, torch.tensor([4])


def test_tie_row_ranks_by_index():
    x, t = _tie_row()
    valid, zt, rank = metrics._cls_rank_eager(x, t)
    assert bool(valid[0]) and float(zt[0]) == 2.5 and int(rank[0]) == 2
    assert int(rank_ref(x, t)[1][0]) == 2
    got = [float(a) for a in M.cls_accuracy(x, t, topk=(1, 2, 3, 9))]
    assert got == [0.0, 0.0, 100.0, 100.0]
    for tgt, want in ((1, 0), (2, 1), (6, 3), (8, 4), (7, 5), (5, 8)):
        assert int(metrics._cls_rank_eager(x, torch.tensor([tgt]))[2][0]) == want, tgt


def test_k_below_five_makes_acc5_100_for_valid_targets():
    g = torch.Generator().manual_seed(0)
    for K in (1, 3, 4):
        x = torch.randn(7, K, generator=g)
        t = torch.randint(0, K, (7,), generator=g)
        a1, a5 = M.cls_accuracy(x, t, topk=(1, 5))
        assert float(a5) == 100.0
        assert float(a1) == float(pct(int((x.argmax(1) == t).sum()), 7))


def test_out_of_range_and_ignore_index_targets():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 7, generator=g)
    best = x.argmax(1)
    t = best.clone()
    t[1], t[3] = 7, -100                                             # one past the last class, and F.cross_entropy's ignore_index
    out = metrics._cls_eval_eager(x, t, (1, 5))
    ref = cls_eval_ref(x.double(), t, (1, 5))
    assert ref['n_valid'] == 3 and ref['counts'] == [3, 3]
    assert [float(v) for v in out[1:]] == [60.0, 60.0]               # B = 5 stays the denominator
    assert abs(float(out[0]) - ref['loss']) <= ref['b_loss']
    want = torch.nn.functional.cross_entropy(x, torch.where((t >= 0) & (t < 7), t, torch.full_like(t, -100)))
    assert abs(float(out[0]) - float(want)) <= 2 * ref['b_loss']     # torch's mean over the targets that are not ignored
    valid, _, rank = metrics._cls_rank_eager(x, t)
    assert valid.tolist() == [True, False, True, False, True] and rank.tolist() == [0, 7, 0, 7, 0]
    # nothing valid: loss 0 (torch: NaN), accuracies 0, and the batch still counts
    m = M.ClsMetric(topk=(1,))
    m.update(x, torch.full((5,), -100))
    assert m.acc.tolist() == [0.0, 1.0, 5.0, 0.0]
    assert m.compute() == {'loss': 0.0, 'acc1': 0.0}


def test_argument_errors():
    x = torch.zeros(4, 7)
    t = torch.zeros(4, dtype=torch.int64)
    for bad in ((), (0,), (1, -5)):
        with pytest.raises(ValueError, match='threshold'):
            M.cls_accuracy(x, t, topk=bad)
        with pytest.raises(ValueError, match='threshold'):
            M.ClsMetric(topk=bad)
    for bx, bt in ((x[0], t), (x, t[:3]), (x, torch.zeros(4, 7)), (x, t.float())):
        with pytest.raises(ValueError):
            M.cls_accuracy(bx, bt)


def test_other_dtypes_and_int32_targets_take_the_restatement():
    x, t = _case(6, 7)
    want = [float(v) for v in GOLD['case/6x7/acc']]
    for xx, tt in ((x.double(), t), (x, t.int()), (x.t().contiguous().t(), t)):
        assert [float(a) for a in M.cls_accuracy(xx, tt, topk=(1, 5))] == want
    xh = x.half()
    ref = cls_eval_ref(xh.double(), t, (1, 5))
    out = metrics._cls_eval_eager(xh, t, (1, 5))
    assert np.array_equal(_bits(out[1:].numpy()), _bits(ref['acc'])) and abs(float(out[0]) - ref['loss']) <= ref['b_loss']


def test_amd_loop_cls_metric_constructs():
    m = amd_loop.cls_metric()
    assert isinstance(m, M.ClsMetric) and m.topk == (1, 5) and m.acc is None
    m = amd_loop.cls_metric(topk=(1, 3), device='cpu')
    assert m.topk == (1, 3) and m.acc.shape == (5,) and m.acc.dtype == torch.float64 and m.acc.device.type == 'cpu'


# ---- against the C ABI stub ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed():
    import dryrun_harness
    from multimae_amd import functions
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()
    functions.ops._require_gpu = ops._require_gpu


class Recorder:
    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def rec(*args):
            self.calls.append((name, args))
            return fn(*args)
        return rec

    def names(self):
        return [n for n, _ in self.calls]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_fused_path_is_one_call_with_the_expected_arguments(stubbed, dtype):
    rec = _lib._lib = Recorder(_lib._lib)
    x = torch.randn(6, 7).to(dtype).requires_grad_(True)
    t = torch.tensor([0, 1, 2, 3, 4, 6])
    acc = M.cls_accuracy(x, t, topk=(1, 5))
    assert len(acc) == 2 and all(a.shape == () and a.dtype == torch.float32 and not a.requires_grad for a in acc)
    assert rec.names() == ['mmae_cls_eval']
    a = rec.calls[0][1]
    code = _lib.F32 if dtype == torch.float32 else _lib.BF16
    assert a[0] == x.data_ptr() and a[1] == code and a[2] == 7 and a[3] == t.data_ptr()
    assert a[4:11] == (6, 7, 2, 1, 5, 0, 0) and a[15] is None and a[16] == 0
    assert acc[0].data_ptr() == a[14] + 4 and acc[1].data_ptr() == a[14] + 8          # views of out, nothing copied or read back
    # a view with a larger row stride: still fused, ldx = stride(0); one row: ldx = K
    wide = torch.randn(6, 16).to(dtype)
    M.cls_accuracy(wide[:, :7], t, topk=(3,))
    M.cls_accuracy(wide[:1, :7], t[:1])
    assert rec.names() == ['mmae_cls_eval'] * 3
    b, c = rec.calls[1][1], rec.calls[2][1]
    assert b[0] == wide.data_ptr() and b[2] == 16 and b[4:11] == (6, 7, 1, 3, 0, 0, 0)
    assert c[2] == 7 and c[4:11] == (1, 7, 1, 1, 0, 0, 0)
    # ClsMetric hands its f64 accumulator to the same launch
    m = M.ClsMetric(topk=(1, 2, 3, 4))
    m.update(x, t)
    m.update(x, t)
    assert rec.names() == ['mmae_cls_eval'] * 5
    for _, d in rec.calls[3:]:
        assert d[6:11] == (4, 1, 2, 3, 4) and d[15] == m.acc.data_ptr()
    assert m.acc.shape == (7,) and m.acc.dtype == torch.float64


def test_everything_else_is_the_restatement(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    x, t = _case(6, 7)
    want = [float(v) for v in GOLD['case/6x7/acc']]
    got = M.cls_accuracy(x, t, topk=(1, 5, 2, 3, 4))                  # five thresholds
    assert [float(got[0]), float(got[1])] == want and len(got) == 5
    for xx, tt in ((x.half(), t), (x.double(), t), (x, t.int()), (x.t().contiguous().t(), t), (x[:, ::2], t),
                   (x[:1].expand(6, 7), t)):
        M.cls_accuracy(xx, tt, topk=(1, 5))
        M.ClsMetric().update(xx, tt)
    m = M.ClsMetric(topk=(1, 2, 3, 4, 5))
    m.update(x, t)
    assert m.compute()['acc1'] == want[0] and m.compute()['acc5'] == want[1]
    assert rec.names() == []


def test_launcher_validates_its_arguments(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    x, t = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    lse, nll, rank, out = ops.cls_eval(x, 8, 4, 7, t, (1, 5))
    assert lse.shape == (4,) and nll.shape == (4,) and rank.shape == (4,) and rank.dtype == torch.int32 and out.shape == (3,)
    for fn in (lambda: ops.cls_eval(x, 8, 4, 7, t, ()),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1, 2, 3, 4, 5)),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1, 0)),
               lambda: ops.cls_eval(x, 8, 4, 7, t.int(), (1,)),
               lambda: ops.cls_eval(x, 8, 4, 7, t[:3], (1,)),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1,), acc=torch.zeros(4)),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1,), acc=torch.zeros(5, dtype=torch.float64)),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1,), rank=torch.zeros(4, dtype=torch.int64)),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1,), out=torch.zeros(3)),
               lambda: ops.cls_eval(x, 8, 4, 7, t, (1,), lse=torch.zeros(5))):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(TypeError):
        ops.cls_eval(x.double(), 8, 4, 7, t, (1,))
    assert rec.names() == ['mmae_cls_eval']


# ---------------------------------------------------------------------------------------------------------- the C ABI --
def test_entry_point_is_declared_exported_and_refuses_bad_arguments():
    """the symbol with its argument list, the version unchanged, and every refusal with the entry's name in mmae_last_error() -- on a
    machine without a GPU, so before anything touches a device; the output buffers keep their bytes"""
    I, L, V = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    want = [V, I, L, V, I, I, I, I, I, I, I, V, V, V, V, V, V]
    assert 'mmae_cls_eval' in _lib.declared_symbols() and _lib._PROTOS['mmae_cls_eval'] == (I, want)
    lib = _lib.load()
    assert lib.mmae_abi_version() == 7
    assert lib.mmae_cls_eval.argtypes == want and ops.CLS_TOPK_MAX == 4
    EINVAL, ESUPPORT = -1, -3
    buf = (ctypes.c_float * 4096)()
    outs = (ctypes.c_int32 * 64)(*([0x5a5a5a5a] * 64))
    p, o = ctypes.addressof(buf), ctypes.addressof(outs)
    # x dtype ldx target B K n_k k0 k1 k2 k3 lse nll rank out acc stream
    good = [p, 0, 8, p, 4, 7, 2, 1, 5, 0, 0, o, o + 64, o + 128, o + 192, None, None]

    def refused(code, **kw):
        args = list(good)
        for i, v in kw.items():
            args[int(i[1:])] = v
        assert lib.mmae_cls_eval(*args) == code, kw
        assert b'cls_eval' in lib.mmae_last_error(), (kw, lib.mmae_last_error())
        assert all(v == 0x5a5a5a5a for v in outs), kw

    for v in (0, -1):
        refused(EINVAL, _4=v)                                            # B
        refused(EINVAL, _5=v)                                            # K
    refused(EINVAL, _2=6)                                                # ldx < K
    for v in (0, 5, -1):
        refused(EINVAL, _6=v)                                            # n_k
    refused(EINVAL, _7=0)
    refused(EINVAL, _8=-3)
    refused(EINVAL, _6=4, _9=3, _10=0)                                        # the fourth threshold counts once n_k = 4
    for v in (2, 3, 5, -1):
        refused(ESUPPORT, _1=v)                                          # F32X3, F32F16, F16, junk
    for i in (0, 3, 11, 12, 13, 14):
        refused(EINVAL, **{f'_{i}': None})
