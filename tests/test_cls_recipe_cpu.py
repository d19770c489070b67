"""CPU: host side of the classification fine-tuning recipe (multimae_amd/mixup.py, criterion.py, ema.py, dropin/amd_loop.py).

* ``Mixup.draw`` against the golden fixture (tests/golden/make_golden_cls_recipe.py, the reference's own ``Mixup`` on the CPU): for
  every mode x variant and four consecutive calls under one ``np.random.seed``, the per-sample block -- applied to the stored input by
  the numpy restatement of the kernels' contract below, every product and sum rounding to float32 on its own -- reproduces the
  reference's mixed batch and soft target BIT FOR BIT, and ``np.random`` is left at the recorded position.
* constructor / ``amd_loop.mixup`` / ``cls_criterion`` / ``model_ema`` argument handling, the ValueError / NotImplementedError cases.
* control flow of ``Mixup.__call__``, both criteria (forward and backward) and ``ModelEma.update`` against the C ABI stub of
  dryrun_harness, which checks every call's argument count and types against include/mmae.h.  Numbers from the stub are garbage by
  design; the kernels are checked in tests/test_cls_recipe_gpu.py.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, engine, ops
from dropin import amd_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'cls_recipe.npz'))
CASES = json.loads(GOLD['mix/cases'].item())
for _kw in CASES.values():
    if _kw.get('cutmix_minmax') is not None:
        _kw['cutmix_minmax'] = tuple(_kw['cutmix_minmax'])


def apply_rows(x0: np.ndarray, labels: np.ndarray, rows: np.ndarray, K: int, smoothing: float):
    """mmae_mixup_pairs + mmae_mix_target as include/mmae.h states them, in numpy float32 (one rounding per operation)"""
    B = x0.shape[0]
    w = rows[:, :4].copy().view(np.float32)
    box = rows[:, 4:]
    out = x0.copy()
    for i in range(B):
        j = B - 1 - i
        yl, yh, xl, xh = (int(v) for v in box[i])
        if yl == ops.MIX_KEEP:
            continue
        if yl == ops.MIX_BLEND:
            out[i] = x0[i] * w[i, 0] + x0[j] * w[i, 1]
        else:
            out[i, :, yl:yh, xl:xh] = x0[j, :, yl:yh, xl:xh]
    off = smoothing / K
    on = 1. - smoothing + off
    y = np.full((B, K), np.float32(off), dtype=np.float32)
    y[np.arange(B), labels] = np.float32(on)
    tgt = y * w[:, 2:3] + y[::-1] * w[:, 3:4]
    assert out.dtype == np.float32 and tgt.dtype == np.float32
    return out, tgt


@pytest.mark.parametrize('case', list(CASES))
def test_host_draw_reproduces_the_reference(case):
    kw = CASES[case]
    x0, labels = GOLD['mix/x'], GOLD['mix/labels']
    mix = M.Mixup(**kw)
    np.random.seed(1000 + list(CASES).index(case))
    kinds = set()
    for c in range(4):
        rows = mix.draw(x0.shape)
        assert rows.shape == (x0.shape[0], ops.MIX_ROW_WORDS) and rows.dtype == np.int32
        out, tgt = apply_rows(x0, labels, rows, kw['num_classes'], kw['label_smoothing'])
        assert np.array_equal(out.view(np.int32), GOLD[f'mix/{case}/out{c}'].view(np.int32)), (case, c)
        assert np.array_equal(tgt.view(np.int32), GOLD[f'mix/{case}/tgt{c}'].view(np.int32)), (case, c)
        kinds |= {min(int(v), 0) for v in rows[:, 4]}
    assert np.random.rand() == float(GOLD[f'mix/{case}/rand'][0]), 'np.random is not where the reference leaves it'
    if case.endswith('_mixup'):
        assert ops.MIX_BLEND in kinds
    if case.endswith(('_cutmix', '_minmax')):
        assert 0 in kinds                                          # a box


def test_fixture_covers_every_kind_of_row():
    """over all cases the reference drew blends, boxes and untouched samples (prob 0.5), with smoothing 0.1 and 0"""
    assert len(CASES) == 15 and {kw['label_smoothing'] for kw in CASES.values()} == {0.1, 0.0}
    x0 = GOLD['mix/x']
    untouched = sum(np.array_equal(GOLD[f'mix/{c}/out{k}'], x0) for c in CASES for k in range(4))
    assert 0 < untouched < 4 * len(CASES)


def test_disabled_and_lam_one_draw_as_the_reference_and_keep_x():
    mix = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode='batch')
    mix.mixup_enabled = False
    np.random.seed(3)
    rows = mix.draw((4, 3, 8, 8))
    np.random.seed(3)
    first = np.random.rand()
    np.random.seed(3)
    mix.draw((4, 3, 8, 8))
    assert np.random.rand() == first, 'a disabled batch-mode Mixup draws nothing'
    assert (rows[:, 4] == ops.MIX_KEEP).all()
    w = rows[:, :4].copy().view(np.float32)
    assert (w[:, 2] == 1).all() and (w[:, 3] == 0).all()
    mix = M.Mixup(mixup_alpha=0.8, cutmix_alpha=0., mode='elem', prob=0.0)       # draws, but every lam stays 1
    np.random.seed(4)
    rows = mix.draw((4, 3, 8, 8))
    assert (rows[:, 4] == ops.MIX_KEEP).all()
    after = np.random.rand()
    np.random.seed(4)
    np.random.beta(0.8, 0.8, size=4), np.random.rand(4)
    assert np.random.rand() == after


def test_constructor_and_argument_errors():
    m = M.Mixup(cutmix_minmax=(0.2, 0.8))
    assert m.cutmix_alpha == 1.0 and m.mixup_enabled and m.mode == 'batch' and m.num_classes == 1000 and m.label_smoothing == 0.1
    with pytest.raises(ValueError):
        M.Mixup(cutmix_minmax=(0.2,))
    with pytest.raises(ValueError, match='even'):
        M.Mixup().draw((3, 3, 8, 8))
    with pytest.raises(AssertionError):
        M.Mixup(mixup_alpha=0., cutmix_alpha=0.).draw((2, 3, 8, 8))
    x = torch.zeros(4, 3, 8, 8)
    y = torch.zeros(4, dtype=torch.int64)
    for bad in (x, x.double(), x[:, :, ::2], x[0]):                # on the CPU, float64, not contiguous, 3-D
        with pytest.raises(ValueError, match='float32'):
            M.Mixup(num_classes=5)(bad, y)


def _args(**kw):
    base = dict(mixup=0.8, cutmix=1.0, cutmix_minmax=None, mixup_prob=1.0, mixup_switch_prob=0.5, mixup_mode='batch', smoothing=0.1,
                nb_classes=1000, model_ema_decay=0.9999, model_ema_force_cpu=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_amd_loop_mixup_and_three_way_criterion():
    fn = amd_loop.mixup(_args())
    assert isinstance(fn, M.Mixup)
    assert (fn.mixup_alpha, fn.cutmix_alpha, fn.mix_prob, fn.switch_prob, fn.mode, fn.label_smoothing, fn.num_classes) == \
        (0.8, 1.0, 1.0, 0.5, 'batch', 0.1, 1000)
    assert amd_loop.mixup(_args(mixup=0., cutmix=0.)) is None
    assert isinstance(amd_loop.mixup(_args(mixup=0., cutmix=0., cutmix_minmax=(0.2, 0.8))), M.Mixup)
    assert isinstance(amd_loop.cls_criterion(_args(), fn), M.SoftTargetCrossEntropy)
    ls = amd_loop.cls_criterion(_args(smoothing=0.2), None)
    assert isinstance(ls, M.LabelSmoothingCrossEntropy) and ls.smoothing == 0.2 and ls.confidence == 0.8
    assert type(amd_loop.cls_criterion(_args(smoothing=0.), None)) is torch.nn.CrossEntropyLoss


def test_criterion_target_errors():
    x = torch.zeros(4, 7)
    with pytest.raises(ValueError, match='float32 tensor of the logits'):
        M.SoftTargetCrossEntropy()(x, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='float32 tensor of the logits'):
        M.SoftTargetCrossEntropy()(x, torch.zeros(4, 6))
    with pytest.raises(ValueError, match='int64 tensor of 4 class indices'):
        M.LabelSmoothingCrossEntropy()(x, torch.zeros(4, 7))
    with pytest.raises(ValueError, match='int64 tensor of 4 class indices'):
        M.LabelSmoothingCrossEntropy()(x, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match='logits'):
        M.SoftTargetCrossEntropy()(x.double(), torch.zeros(4, 7))
    with pytest.raises(ValueError):
        M.LabelSmoothingCrossEntropy(smoothing=1.0)


# ---- against the C ABI stub ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


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


def test_new_entry_points_are_declared():
    for n in ('mmae_mixup_pairs', 'mmae_mix_target', 'mmae_soft_ce_fwd', 'mmae_soft_ce_bwd', 'mmae_ema_update'):
        assert n in _lib.declared_symbols()
    assert len(_lib._PROTOS['mmae_soft_ce_fwd'][1]) == 13 and len(_lib._PROTOS['mmae_ema_update'][1]) == 7


def test_mixup_call_is_two_launches_and_one_block(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    mix = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, num_classes=7, mode='elem')
    x = torch.randn(6, 3, 16, 20)
    y = torch.tensor([0, 1, 2, 3, 4, 6])
    np.random.seed(0)
    xm, t = mix(x, y)
    assert xm is x and t.shape == (6, 7) and t.dtype == torch.float32
    assert rec.names() == ['mmae_mixup_pairs', 'mmae_mix_target']
    (_, a), (_, b) = rec.calls
    assert a[0] == x.data_ptr() and a[2:6] == (6, 3, 16, 20) and a[1] == b[1]          # the same parameter block
    assert b[3:5] == (6, 7) and b[5] == pytest.approx(0.9 + 0.1 / 7) and b[6] == pytest.approx(0.1 / 7)
    with pytest.raises(ValueError, match=r'outside \[0, 7\)'):
        mix(x, torch.tensor([0, 1, 2, 3, 4, 7]))
    with pytest.raises(ValueError, match='even'):
        mix(torch.randn(3, 3, 8, 8), y[:3])
    with pytest.raises(ValueError, match='class indices'):
        mix(x, torch.zeros(6, 7))


def test_mixup_block_is_redrawn_for_every_replay_of_a_captured_step(stubbed):
    """while a step is captured the block is a static device tensor that HostInputs.refresh() redraws: two refreshes, two draws"""
    mix = M.Mixup(mixup_alpha=0.8, num_classes=7)
    x = torch.randn(4, 3, 8, 8)
    hi = engine.HostInputs()
    engine._capture = hi
    try:
        np.random.seed(1)
        mix(x, torch.tensor([0, 1, 2, 3]))
    finally:
        engine._capture = None
    assert len(hi.items) == 1
    dev = hi.items[0][0]
    hi.refresh()
    first = dev.clone()
    hi.refresh()
    assert dev.shape == (4, ops.MIX_ROW_WORDS) and not torch.equal(first, dev)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_criteria_forward_backward_control_flow(stubbed, dtype):
    rec = _lib._lib = Recorder(_lib._lib)
    x = torch.randn(6, 7).to(dtype).requires_grad_(True)
    t = torch.softmax(torch.randn(6, 7), -1)
    loss = M.SoftTargetCrossEntropy()(x, t)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    assert x.grad.shape == x.shape and x.grad.dtype == dtype
    labels = torch.tensor([0, 1, 2, 3, 4, 6])
    M.LabelSmoothingCrossEntropy(0.1)(x, labels).backward()
    assert rec.names() == ['mmae_soft_ce_fwd', 'mmae_soft_ce_bwd'] * 2
    f0, b0, f1, b1 = (a for _, a in rec.calls)
    code = _lib.F32 if dtype == torch.float32 else _lib.BF16
    assert f0[1] == code and f0[2] == 7 and f0[3] == t.data_ptr() and f0[4] is None and f0[5] == 0.0 and f0[6:8] == (6, 7)
    assert f1[3] is None and f1[4] == labels.data_ptr() and f1[5] == pytest.approx(0.1)
    assert b0[8] == f0[8] and b0[9] == f0[9]                        # backward reads the lse / tsum the forward wrote
    # a target modified between forward and backward is an error, not a silently wrong gradient
    loss = M.SoftTargetCrossEntropy()(x, t)
    t.mul_(2)
    with pytest.raises(RuntimeError, match='modified in place'):
        loss.backward()


def _tiny_vit():
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(3, 1, 8, image_size=16)}
    outs = {'cls': M.LinearOutputAdapter(num_classes=7, use_mean_pooling=True)}
    return M.MultiViT(ins, outs, num_global_tokens=1, dim_tokens=16, depth=1, num_heads=2)


def test_model_ema_is_one_launch_over_two_equal_arenas(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    model = _tiny_vit()
    ema = amd_loop.model_ema(model, _args(model_ema_decay=0.99))
    assert isinstance(ema, M.ModelEma) and ema.decay == 0.99 and not ema.ema.training
    a, e = model.build_arena(), engine.arena_of(ema.ema)
    assert e is not None and e is not a and e.param.data_ptr() != a.param.data_ptr()
    assert e.names == a.names and e.offsets == a.offsets and e.numel == a.numel and torch.equal(e.param, a.param)
    assert list(ema.ema.state_dict()) == list(model.state_dict())
    assert all(not p.requires_grad and p.grad is None for p in ema.ema.parameters()) and e.grad.numel() == 0
    assert all(p.requires_grad for n, p in model.named_parameters() if 'pos_emb' not in n), 'the model keeps its flags'
    rec.calls.clear()
    ema.update(model)
    assert rec.names() == ['mmae_ema_update']
    args = rec.calls[0][1]
    assert args[0] == e.param.data_ptr() and args[1] == a.param.data_ptr() and args[2] is None and args[3] == a.numel
    assert args[4] == 0.99 and args[5] == 1. - 0.99
    sh = M.ModelEma(model, decay=0.5, shadow=True)
    rec.calls.clear()
    sh.update(model)
    se = engine.arena_of(sh.ema)
    assert rec.calls[0][1][2] == se.shadow.data_ptr() and se._shadow_token
    # a model whose arena no longer matches: raise, never fall back
    other = _tiny_vit()
    other.output_adapters['cls'].head.weight.requires_grad_(False)
    other.build_arena()
    with pytest.raises(RuntimeError, match='laid out'):
        ema.update(other)
    with pytest.raises(NotImplementedError):
        M.ModelEma(model, device='cpu')
    with pytest.raises(NotImplementedError):
        M.ModelEma(model, resume='checkpoint.pth')
    with pytest.raises(NotImplementedError):
        amd_loop.model_ema(model, _args(model_ema_force_cpu=True))
