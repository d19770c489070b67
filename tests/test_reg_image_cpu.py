"""CPU: host side of the fused regression losses and depth metrics on the DPT head's prediction (criterion._image_fused_ok,
functions.ImageMark / RegImageLossFn, metrics._depth_values, ops.reg_img_fwd / reg_img_bwd / depth_metrics_img) against the C ABI stub
of dryrun_harness with a call recorder: which path a call takes and in which order the kernels are called; and the three new entry
points of the built library: declared, exported, refusing bad arguments before anything touches a device.  Numbers from the stub are
garbage by design; the kernels are checked in tests/test_reg_image_gpu.py."""
import ctypes
import os
import sys

import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, engine, functions, metrics, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dpt_fixture as DF  # noqa: E402
from dpt_fixture import B, CASES, UNUSED  # noqa: E402

LOSSES = {'l1': M.masked_l1_loss, 'mse': M.masked_mse_loss, 'berhu': M.masked_berhu_loss}
NEW = ('mmae_reg_img_fwd', 'mmae_reg_img_bwd', 'mmae_depth_metrics_img')


@pytest.fixture()
def stubbed():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()
    functions.ops._require_gpu = ops._require_gpu


class Recorder:
    """wraps the stub library: the name of every call in order, and the arguments of the regression and metric kernels"""

    def __init__(self, inner):
        self.inner, self.order, self.calls = inner, [], []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def rec(*args):
            self.order.append(name)
            if name.startswith(('mmae_reg_', 'mmae_depth_metrics')):
                self.calls.append((name, args))
            return fn(*args)
        return rec

    def names(self):
        return [n for n, _ in self.calls]


def _predict(case, grad=True):
    """(head, tokens, the head's prediction) of a fixture case on the stub"""
    head = DF.seeded_head(case)
    toks = [t.clone().requires_grad_(grad) for t in DF.tokens(case)]
    return head, toks, head(toks, DF.case_info(case))


def _data(y, Cm=1, seed=3):
    g = torch.Generator().manual_seed(seed)
    Bs, K, H, W = y.shape
    return torch.randn(Bs, K, H, W, generator=g), torch.rand(Bs, Cm, H, W, generator=g) < 0.7


# ---------------------------------------------------------------------------------------------------------- the C ABI --
def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    """the three symbols with the issue's argument lists, the version unchanged, and MMAE_EINVAL with the entry point's own name in
    mmae_last_error() for every invalid-argument case -- on a machine without a GPU, so before anything touches a device"""
    lib = _lib.load()
    assert lib.mmae_abi_version() == 7
    I, L, F, V = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {'mmae_reg_img_fwd': [V, V, V, I, I, I, I, I, I, V, V, V, V], 'mmae_reg_img_bwd': [V, V, V, I, L, V, V],
            'mmae_depth_metrics_img': [V, V, V, F, F, I, I, I, V, V, V, V]}
    for name, args in want.items():
        assert name in _lib.declared_symbols() and _lib._PROTOS[name] == (I, args), name
        assert getattr(lib, name).argtypes == args
    EINVAL = -1                                                           # MMAE_EINVAL
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)

    def refused(fn, tag, *args):
        assert fn(*args) == EINVAL, (tag, args)
        assert tag in lib.mmae_last_error(), (tag, lib.mmae_last_error())

    fwd = [p, p, p, 3, 2, 2, 3, 4, 4, p, p, p, None]                      # pred target mask Cm kind B K H W diff partial out stream
    for i in (5, 6, 7, 8):                                                # a non-positive dimension
        for v in (0, -1):
            refused(lib.mmae_reg_img_fwd, b'reg_img_fwd', *(fwd[:i] + [v] + fwd[i + 1:]))
    for kind in (-1, 3):
        refused(lib.mmae_reg_img_fwd, b'reg_img_fwd', *(fwd[:4] + [kind] + fwd[5:]))
    for cm in (2, 0, 4):                                                  # neither 1 nor K = 3, with a mask
        refused(lib.mmae_reg_img_fwd, b'reg_img_fwd', *(fwd[:3] + [cm] + fwd[4:]))
    for i in (0, 1, 9, 10, 11):                                           # a NULL required pointer
        refused(lib.mmae_reg_img_fwd, b'reg_img_fwd', *(fwd[:i] + [None] + fwd[i + 1:]))

    bwd = [p, p, p, 0, 16, p, None]                                       # diff out up kind n dpred stream
    for n in (0, -4):
        refused(lib.mmae_reg_img_bwd, b'reg_img_bwd', *(bwd[:4] + [n] + bwd[5:]))
    for kind in (-1, 3):
        refused(lib.mmae_reg_img_bwd, b'reg_img_bwd', *(bwd[:3] + [kind] + bwd[4:]))
    for i in (0, 1, 2, 5):
        refused(lib.mmae_reg_img_bwd, b'reg_img_bwd', *(bwd[:i] + [None] + bwd[i + 1:]))

    met = [p, p, p, 0.5, 2.0, 2, 4, 4, p, p, None, None]                  # pred target mask mean std B H W partial out acc stream
    for i in (5, 6, 7):
        for v in (0, -1):
            refused(lib.mmae_depth_metrics_img, b'depth_metrics_img', *(met[:i] + [v] + met[i + 1:]))
    for i in (0, 1, 8, 9):
        refused(lib.mmae_depth_metrics_img, b'depth_metrics_img', *(met[:i] + [None] + met[i + 1:]))


def test_launchers_validate_their_arguments(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    y, t, m = torch.zeros(2, 3, 4, 6), torch.zeros(2, 3, 4, 6), torch.ones(2, 1, 4, 6, dtype=torch.bool)
    diff, out = ops.reg_img_fwd(y, t, m, 'berhu')
    assert diff.shape == y.shape and diff.dtype == torch.float32 and out.shape == (4,)
    assert ops.reg_img_bwd(diff, out, torch.ones(1), 'berhu').shape == y.shape
    assert ops.depth_metrics_img(y[:, :1].contiguous(), t[:, :1].contiguous(), m, 0.5, 2.0, acc=torch.zeros(8)).shape == (7,)
    assert rec.names() == list(NEW)
    fwd = rec.calls[0][1]
    assert fwd[:9] == (y.data_ptr(), t.data_ptr(), m.data_ptr(), 1, 2, 2, 3, 4, 6) and fwd[9] == diff.data_ptr()
    assert rec.calls[1][1][3:5] == (2, 2 * 3 * 4 * 6)
    for fn in (lambda: ops.reg_img_fwd(y, t, m, 'huber'),
               lambda: ops.reg_img_fwd(y.double(), t, m, 'l1'),
               lambda: ops.reg_img_fwd(y.transpose(2, 3), t.transpose(2, 3), None, 'l1'),
               lambda: ops.reg_img_fwd(y[0], t[0], None, 'l1'),
               lambda: ops.reg_img_fwd(y, t.double(), m, 'l1'),
               lambda: ops.reg_img_fwd(y, t[:, :1], m, 'l1'),
               lambda: ops.reg_img_fwd(y, t, m.float(), 'l1'),
               lambda: ops.reg_img_fwd(y, t, torch.ones(2, 2, 4, 6, dtype=torch.bool), 'l1'),
               lambda: ops.reg_img_fwd(y, t, m, 'l1', diff=torch.zeros(2, 3, 4, 5)),
               lambda: ops.reg_img_fwd(y, t, m, 'l1', partial=torch.zeros(8)),
               lambda: ops.reg_img_bwd(diff, out, torch.ones(1), 'huber'),
               lambda: ops.reg_img_bwd(diff, out[:3], torch.ones(1), 'l1'),
               lambda: ops.reg_img_bwd(diff, out, torch.ones(2), 'l1'),
               lambda: ops.reg_img_bwd(diff, out, torch.ones(1), 'l1', dpred=torch.zeros(3)),
               lambda: ops.depth_metrics_img(y, t, None, 0.5, 2.0),                          # K = 3
               lambda: ops.depth_metrics_img(y[:, :1].contiguous(), t[:, :1].contiguous(), None, 0.5, 2.0, acc=torch.zeros(7))):
        with pytest.raises(ValueError):
            fn()
    assert rec.names() == list(NEW)                                       # nothing more was called


# ------------------------------------------------------------------------------------------------------ fused routing --
@pytest.mark.parametrize('direct', [False, True])
@pytest.mark.parametrize('kind', list(LOSSES))
@pytest.mark.parametrize('case', list(CASES))
def test_the_heads_own_prediction_takes_the_fused_kernels(stubbed, case, kind, direct):
    """y and y.float() (the same object) both record mmae_reg_img_fwd on the head's image; backward() records mmae_reg_img_bwd before
    any of the head's backward kernels, and every token and parameter gets its gradient, in both gradient modes"""
    rec = _lib._lib = Recorder(_lib._lib)
    K, tasks, D, (NH, NW) = CASES[case]
    H, W = 16 * NH, 16 * NW
    head = DF.seeded_head(case)
    if direct:
        engine.ParamArena(head)
    toks = [t.clone().requires_grad_(True) for t in DF.tokens(case)]
    engine.set_direct_grads(direct)
    try:
        with engine.precision('fp32'):
            y = head(toks, DF.case_info(case))
            assert type(y) is torch.Tensor and getattr(y, '_mmae_seg', None) is None
            mark = y._mmae_img
            assert isinstance(mark, functions.ImageMark) and mark.shape == (B, K, H, W) and mark.matches(y) and y.float() is y
            n_fwd = len(rec.order)
            t, m1 = _data(y, 1)
            _, mk = _data(y, K, seed=4)
            la, lb = LOSSES[kind](y, t, m1), LOSSES[kind](y.float(), t, mk)
            for l in (la, lb):
                assert type(l.grad_fn).__name__ == 'RegImageLossFnBackward' and l.shape == () and l.dtype == torch.float32
            assert rec.order[n_fwd:] == ['mmae_reg_img_fwd'] * 2
            for (name, a), mask in zip(rec.calls, (m1, mk)):
                assert a[:2] == (y.data_ptr(), t.data_ptr()) and a[2] == mask.data_ptr()
                assert a[3:9] == (mask.shape[1], ops.REG_KINDS[kind], B, K, H, W)
            (la + lb).backward()
    finally:
        engine.set_direct_grads(False)
    back = rec.order[n_fwd + 2:]
    assert back[:2] == ['mmae_reg_img_bwd'] * 2 and 'mmae_reg_img_bwd' not in back[2:] and 'mmae_dpt_tail_bwd' in back[2:]
    for name, a in rec.calls[2:]:
        assert name == 'mmae_reg_img_bwd' and a[3:5] == (ops.REG_KINDS[kind], B * K * H * W)
    for tk in toks:
        assert tk.grad is not None and tk.grad.shape == tk.shape
    for n, p in head.named_parameters():
        if n in UNUSED and not direct:
            assert p.grad is None, n
        else:
            assert p.grad is not None and p.grad.shape == p.shape, n


def test_no_mask_is_a_null_pointer_and_the_target_is_made_contiguous(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    _, _, y = _predict('r3')
    t, _ = _data(y)
    t = t.transpose(2, 3).contiguous().transpose(2, 3)
    loss = M.masked_berhu_loss(y, t)
    assert type(loss.grad_fn).__name__ == 'RegImageLossFnBackward'
    a = rec.calls[0][1]
    assert a[2] is None and a[3] == 1 and a[1] != t.data_ptr()


def test_target_modified_in_place_is_refused(stubbed):
    _, _, y = _predict('r1')
    t, m = _data(y)
    loss = M.masked_mse_loss(y, t, m)
    t.add_(1)
    with pytest.raises(RuntimeError, match='modified in place'):
        loss.backward()


# ------------------------------------------------------------------------------------------------------ eager routing --
def _no_grad_touch(y, t, m):
    with torch.no_grad():
        y.add_(0)
    return y, t, m


EAGER = {
    'times_one': lambda y, t, m: (y * 1, t, m),
    'clone': lambda y, t, m: (y.clone(), t, m),
    'modified_in_place': _no_grad_touch,
    'double_target': lambda y, t, m: (y, t.double(), m),
    'target_of_another_shape': lambda y, t, m: (y, t[:, :, :1], None),
    'float_mask': lambda y, t, m: (y, t, m.float()),
    'two_channel_mask': lambda y, t, m: (y, t, m.expand(-1, 2, -1, -1).contiguous()),
    'plain_tensor': lambda y, t, m: (torch.randn(y.shape, requires_grad=True), t, m),
}


@pytest.mark.parametrize('kind', list(LOSSES))
@pytest.mark.parametrize('case', list(EAGER))
def test_everything_else_is_the_eager_restatement(stubbed, case, kind):
    rec = _lib._lib = Recorder(_lib._lib)
    _, _, y = _predict('r3')
    t, m = _data(y)
    inp, tgt, msk = EAGER[case](y, t, m)
    if case == 'two_channel_mask':
        # a mask of 2 channels against K = 3 fits neither path: the fused one declines it, and the eager restatement fails on it in
        # torch's broadcast exactly as before this path existed (repeat_interleave makes 6 channels of it) -- no grad_fn to look at
        with pytest.raises(RuntimeError, match='must match the size'):
            LOSSES[kind](inp, tgt, msk)
    else:
        loss = LOSSES[kind](inp, tgt, msk)
        assert type(loss.grad_fn).__name__ != 'RegImageLossFnBackward' and loss.grad_fn is not None
    assert not set(NEW) & set(rec.order)


@pytest.mark.parametrize('kind', list(LOSSES))
def test_patch_domain_loss_off_is_the_eager_path(stubbed, kind):
    rec = _lib._lib = Recorder(_lib._lib)
    _, _, y_on = _predict('r3')
    engine.set_patch_domain_loss(False)
    try:
        _, _, y_off = _predict('r3')
        assert getattr(y_off, '_mmae_img', None) is None                  # switched off when the head ran: no mark at all
        for y in (y_off, y_on):                                           # ... or only when the loss runs
            t, m = _data(y)
            loss = LOSSES[kind](y, t, m)
            assert type(loss.grad_fn).__name__ != 'RegImageLossFnBackward' and loss.grad_fn is not None
            with torch.no_grad():
                M.depth_metrics(y[:, :1], t[:, :1], m)
    finally:
        engine.set_patch_domain_loss(True)
    assert not set(NEW) & set(rec.order)
    t, m = _data(y_on)
    assert type(LOSSES[kind](y_on, t, m).grad_fn).__name__ == 'RegImageLossFnBackward'         # and nothing sticks afterwards


def test_inside_a_capture_the_prediction_takes_the_eager_path_without_raising(stubbed, monkeypatch):
    """both fake-capture arms of test_reg_loss_cpu's refusal test: the DPT head's prediction carries no ConvNeXt side channel, so
    nothing raises, and nothing fused is launched into the capture"""
    rec = _lib._lib = Recorder(_lib._lib)
    _, _, y = _predict('r1')
    t, m = _data(y)
    for arm in ('step_graph', 'torch_graph'):
        with monkeypatch.context() as mp_:
            if arm == 'step_graph':
                mp_.setattr(M.engine, '_capture', object())
            else:
                mp_.setattr(torch.cuda, 'is_available', lambda: True)
                mp_.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
            for fn in LOSSES.values():
                loss = fn(y.float(), t, m)
                assert type(loss.grad_fn).__name__ != 'RegImageLossFnBackward' and loss.grad_fn is not None
            assert len(M.depth_metrics(y, t, m)) == 7
            M.DepthMetric().update(y, t, m)
    assert not set(NEW) & set(rec.order)
    assert type(M.masked_l1_loss(y, t, m).grad_fn).__name__ == 'RegImageLossFnBackward'


# ---------------------------------------------------------------------------------------------------- metrics routing --
def test_depth_metrics_paths(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    K, tasks, D, (NH, NW) = CASES['r1']
    with torch.no_grad():
        _, _, y = _predict('r1', grad=False)
        t, m = _data(y)
        got = M.depth_metrics(y, t, m)
    assert tuple(got) == metrics.DEPTH_METRIC_KEYS and rec.names() == ['mmae_depth_metrics_img']
    a = rec.calls[0][1]
    assert a[:3] == (y.data_ptr(), t.data_ptr(), m.data_ptr()) and a[3:8] == (metrics.NYU_MEAN, metrics.NYU_STD, B, 16 * NH, 16 * NW)
    assert a[10] is None
    dm = M.DepthMetric()
    dm.update(y, t, m, loss=torch.tensor(2.0))
    dm.update(y.float(), t, None, loss=torch.tensor(4.0))
    assert rec.names() == ['mmae_depth_metrics_img'] * 3
    assert rec.calls[1][1][10] == dm.acc.data_ptr() and rec.calls[2][1][10] == dm.acc.data_ptr() and rec.calls[2][1][2] is None
    assert dm.acc.shape == (8,) and dm.acc.dtype == torch.float32
    n = len(rec.order)
    for pred in (y * 1, y.clone()):                                       # derived tensors: the eager restatement
        M.depth_metrics(pred, t, m)
    with torch.no_grad():
        _, _, y3 = _predict('r3', grad=False)                             # K = 3: not the depth kernel's case
        t3, m3 = _data(y3)
        M.depth_metrics(y3, t3, m3)
        M.DepthMetric().update(y3, t3, m3)
    assert not set(NEW) & set(rec.order[n:])


def test_amd_loop_criteria_keep_the_mark(stubbed):
    """dropin/amd_loop.py needs no change: its criteria are the engine's functions and preds[task].float() is the marked tensor"""
    from dropin import amd_loop
    rec = _lib._lib = Recorder(_lib._lib)
    _, _, y = _predict('r1')
    t, m = _data(y)
    preds = {'depth': y}
    assert preds['depth'].float() is y and preds['depth'].float()._mmae_img.matches(y)
    loss = amd_loop.depth_criterion('berhu')['depth'](preds['depth'].float(), t, m)
    assert type(loss.grad_fn).__name__ == 'RegImageLossFnBackward'
    _, _, y3 = _predict('r3')
    t3, m3 = _data(y3)
    loss = amd_loop.taskonomy_criterion(['normal'])['normal'](y3.float(), t3, m3)
    assert type(loss.grad_fn).__name__ == 'RegImageLossFnBackward'
    amd_loop.depth_metric().update(y, t, m)
    assert rec.names() == ['mmae_reg_img_fwd', 'mmae_reg_img_fwd', 'mmae_depth_metrics_img']
