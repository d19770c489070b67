"""CPU: host side of random erasing (multimae_amd/random_erasing.py, data_ops.py, staging.ClsStager, dropin/amd_loop.py).

* ``RandomErasing.draw`` against the golden fixture (tests/golden/make_golden_random_erasing.py, the reference's own
  ``RandomErasing(device='cpu')`` in batch mode): the table, applied to the stored input by the numpy restatement of the kernels'
  contract (tests/erase_ref.py), reproduces the reference's output BIT FOR BIT, and both Python's ``random`` and torch's CPU
  generator are left where the reference leaves them.
* the restatement's Philox4x32-10 against known-answer vectors.
* constructor / call ValueErrors, ``amd_loop.random_erasing``, the forms ``ClsStager`` refuses.
* control flow against the C ABI stub of dryrun_harness, which checks every call's argument count and types against
  include/mmae.h.  The kernels are checked in tests/test_random_erasing_gpu.py.
"""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, data_ops, engine, ops, staging
from dropin import amd_loop

import erase_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'random_erasing.npz'))
CASES = json.loads(GOLD['cases'].item())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the restatement --
@pytest.mark.parametrize('counter, key, want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(v) for v in erase_ref.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_restatement_noise_is_a_function_of_header_and_index():
    t = erase_ref.make_table(1, [[(0, 0, 4, 6)]], seed=(5 << 32) | 7, calls=(1 << 32) | 2, mode='pixel')
    assert list(t[0, :5]) == [7, 5, 2, 1, 2] and not t[0, 5:].any()
    z, r = erase_ref.noise(t, (1, 2, 4, 6))
    z2, _ = erase_ref.noise(t, (2, 2, 4, 6))
    assert np.array_equal(z.ravel(), z2.ravel()[:48])              # element e does not depend on the batch around it
    assert np.all(np.abs(z) <= r) and np.all(r > 0)
    # elements 4k, 4k + 1 share (u1, u2): cosine and sine of one angle
    assert np.allclose(z.ravel()[0::4] ** 2 + z.ravel()[1::4] ** 2, r.ravel()[0::4] ** 2, rtol=1e-12)
    out, mask = erase_ref.apply(np.ones((1, 2, 4, 6), np.float32), t)
    assert mask.all() and np.array_equal(out, z.astype(np.float32))


def test_restatement_highest_rectangle_wins():
    t = erase_ref.make_table(2, [[(0, 0, 3, 3, (1., 2.)), (1, 1, 3, 2, (3., 4.)), (0, 0, 0, 4, (9., 9.))], []], mode='rand')
    x = np.full((2, 2, 4, 4), 7, np.float32)
    out, mask = erase_ref.apply(x, t)
    assert mask.sum() == 2 * (9 + 6 - 4) and not mask[1].any()
    assert out[0, 0, 0, 0] == 1. and out[0, 1, 0, 0] == 2. and out[0, 0, 1, 1] == 3. and out[0, 1, 3, 2] == 4. and out[0, 0, 3, 3] == 7.


# ------------------------------------------------------------------------------------------------------------------- the draws --
@pytest.mark.parametrize('case', list(CASES))
def test_host_draw_reproduces_the_reference(case):
    c = CASES[case]
    x, want = erase_ref.golden_case(GOLD, case)
    era = M.RandomErasing(**c['kwargs'])
    random.seed(c['seed'])
    torch.manual_seed(c['seed'])
    table = era.draw(x.shape)
    assert table.shape == (x.shape[0] + 1, erase_ref.ROW) and table.dtype == np.int32
    nxt_random, nxt_torch = random.random(), torch.rand(1)
    out, mask = erase_ref.apply(x, table)
    assert torch.equal(torch.from_numpy(_bits(out)), torch.from_numpy(_bits(want))), case
    assert mask.any() and mask[want != x].all() and np.array_equal(out[~mask], x[~mask])
    assert nxt_random == float(GOLD[f'{case}/random'][0]), 'random is not where the reference leaves it'
    assert float(nxt_torch) == float(GOLD[f'{case}/torch_rand'][0]), "torch's generator is not where the reference leaves it"
    assert era.noise_calls == 1 and era.noise_seed == torch.initial_seed()
    assert list(table[0, :5]) == [c['seed'], 0, 0, 0, erase_ref.MODES[c['kwargs']['mode']]]


@pytest.mark.parametrize('case', list(CASES))
def test_pixel_mode_draws_the_same_rectangles_and_no_torch_numbers(case):
    c = CASES[case]
    shape = tuple(c['shape'])
    random.seed(c['seed'])
    ref_table = M.RandomErasing(**c['kwargs']).draw(shape)
    after_ref = random.random()
    random.seed(c['seed'])
    torch.manual_seed(c['seed'])
    before = torch.get_rng_state()
    table = M.RandomErasing(**dict(c['kwargs'], mode='pixel')).draw(shape)
    assert random.random() == after_ref
    assert torch.equal(torch.get_rng_state(), before), "'pixel' mode must not advance torch's generator"
    rect = [slice(4 + 8 * r, 8 + 8 * r) for r in range(8)]
    assert np.array_equal(table[1:, 0], ref_table[1:, 0])
    for s in rect:
        assert np.array_equal(table[1:, s], ref_table[1:, s])
    assert table[0, 4] == 2 and after_ref == float(GOLD[f'{case}/random'][0])


def test_image_is_one_erase_without_the_split_skip():
    era = M.RandomErasing(probability=1, mode='const', num_splits=3)
    random.seed(11)
    t_img = era.draw((3, 9, 11))
    random.seed(11)
    t_one = M.RandomErasing(probability=1, mode='const').draw((1, 3, 9, 11))
    assert t_img.shape == (2, 68) and t_img[1, 0] == 1 and np.array_equal(t_img, t_one)


def test_noise_key_is_plain_state():
    era = M.RandomErasing(probability=1, mode='pixel')
    era.noise_seed, era.noise_calls = (3 << 32) | 9, (1 << 32) | 4
    t = era.draw((2, 3, 8, 8))
    assert list(t[0, :5]) == [9, 3, 4, 1, 2] and era.noise_calls == (1 << 32) | 5
    assert list(era.draw((2, 3, 8, 8))[0, :5]) == [9, 3, 5, 1, 2]


# -------------------------------------------------------------------------------------------------------------- argument errors --
def test_constructor_refuses_what_the_table_cannot_hold():
    with pytest.raises(ValueError, match='max_count'):
        M.RandomErasing(max_count=9)
    with pytest.raises(ValueError, match='mode'):
        M.RandomErasing(mode='noise')
    assert M.RandomErasing(max_count=8).max_count == 8 and M.RandomErasing(min_count=2).max_count == 2
    d = M.RandomErasing()
    assert (d.probability, d.min_area, d.max_area, d.min_count, d.max_count, d.num_splits, d.mode) == (0.5, 0.02, 1 / 3, 1, 1, 0, 'const')
    assert d.log_aspect_ratio == (np.log(0.3), np.log(1 / 0.3))


@pytest.fixture
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


def test_call_refuses_other_dtypes_layouts_and_too_many_channels(stubbed):
    era = M.RandomErasing(probability=1)
    for bad in (torch.zeros(2, 3, 8, 8, dtype=torch.float16), torch.zeros(2, 3, 8, 8, dtype=torch.float64),
                torch.zeros(2, 3, 8, 8).permute(0, 1, 3, 2)[..., :4], torch.zeros(8, 8), torch.zeros(1, 2, 3, 8, 8),
                torch.zeros(0, 3, 8, 8), np.zeros((2, 3, 8, 8), np.float32)):
        with pytest.raises(ValueError):
            era(bad)
    with pytest.raises(ValueError, match='4 colours'):
        M.RandomErasing(probability=1, mode='rand')(torch.zeros(2, 5, 8, 8))
    assert era.noise_calls == 0                                       # nothing was drawn for a refused call
    M.RandomErasing(probability=1, mode='pixel')(torch.zeros(2, 5, 8, 8))
    old = ops._device_ok
    ops._device_ok = lambda t: False                                  # a tensor that is not on the GPU
    try:
        with pytest.raises(ValueError, match='GPU'):
            era(torch.zeros(2, 3, 8, 8))
    finally:
        ops._device_ok = old


def test_wrappers_check_their_arguments(stubbed):
    x = torch.zeros(2, 3, 4, 4)
    tab = torch.zeros(3, 68, dtype=torch.int32)
    lut = data_ops.rgb_table(staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD)
    u8 = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    for bad in (torch.zeros(2, 68, dtype=torch.int32), torch.zeros(3, 68, dtype=torch.int64), torch.zeros(3, 136, dtype=torch.int32)[:, ::2],
                None):
        with pytest.raises(ValueError, match='table'):
            data_ops.random_erase_(x, bad)
    with pytest.raises(ValueError, match='table'):
        data_ops.ingest_rgb_u8_chw(u8, lut, torch.zeros(2, 68, dtype=torch.int32))
    for bad in (x.double(), x[0], x[:, :, :, ::2]):
        with pytest.raises(ValueError, match='random_erase_'):
            data_ops.random_erase_(bad, tab)
    for bad in (x, u8.permute(0, 2, 3, 1), u8[:, :2], u8[:0]):
        with pytest.raises(ValueError, match='ingest_rgb_u8_chw'):
            data_ops.ingest_rgb_u8_chw(bad, lut)
    with pytest.raises(ValueError, match='lut'):
        data_ops.ingest_rgb_u8_chw(u8, lut[:2])
    with pytest.raises(ValueError, match='out must be'):
        data_ops.ingest_rgb_u8_chw(u8, lut, out=torch.zeros(2, 3, 4, 5))


def test_stub_sees_both_entry_points_with_the_headers_arguments(stubbed):
    for n in ('mmae_random_erase', 'mmae_ingest_rgb_u8_chw_erase'):
        assert n in _lib.declared_symbols()
    assert len(_lib._PROTOS['mmae_random_erase'][1]) == 7 and len(_lib._PROTOS['mmae_ingest_rgb_u8_chw_erase'][1]) == 8
    assert (_lib.ERASE_MAX_RECTS, _lib.ERASE_ROW) == (8, 68)
    header = open(_lib.HEADER).read()
    assert '#define MMAE_ERASE_MAX_RECTS 8' in header and '#define MMAE_ERASE_ROW 68' in header and '#define MMAE_ABI_VERSION 7' in header
    rec = _lib._lib = Recorder(_lib._lib)
    x = torch.zeros(2, 3, 4, 4)
    assert M.RandomErasing(probability=1, mode='pixel')(x) is x
    img = torch.zeros(3, 4, 4)
    assert M.RandomErasing(probability=1)(img) is img
    lut = data_ops.rgb_table(staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD)
    u8 = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    y = data_ops.ingest_rgb_u8_chw(u8, lut)
    y2 = data_ops.ingest_rgb_u8_chw(u8, lut, torch.zeros(3, 68, dtype=torch.int32), out=y)
    assert y2 is y and y.shape == (2, 3, 4, 4) and y.dtype == torch.float32
    names = [n for n, _ in rec.calls]
    assert names == ['mmae_random_erase', 'mmae_random_erase', 'mmae_ingest_rgb_u8_chw_erase', 'mmae_ingest_rgb_u8_chw_erase']
    assert rec.calls[0][1][2:6] == (2, 3, 4, 4) and rec.calls[1][1][2:6] == (1, 3, 4, 4)
    assert rec.calls[2][1][2] is None and isinstance(rec.calls[3][1][2], int) and rec.calls[2][1][4:7] == (2, 4, 4)


def test_table_is_redrawn_for_every_replay_of_a_captured_step(stubbed):
    """while a step is captured the table is a static device tensor that HostInputs.refresh() redraws: the capture draws once (the
    first replay's table), the second refresh draws again -- two tables, two values of the call counter"""
    era = M.RandomErasing(probability=1, mode='pixel')
    x = torch.zeros(4, 3, 8, 8)
    hi = engine.HostInputs()
    engine._capture = hi
    try:
        random.seed(1)
        era(x)
    finally:
        engine._capture = None
    assert len(hi.items) == 1 and era.noise_calls == 1
    dev = hi.items[0][0]
    hi.refresh()
    first = dev.clone()
    assert era.noise_calls == 1 and first[0, 2] == 0
    hi.refresh()
    assert era.noise_calls == 2 and dev[0, 2] == 1
    assert dev.shape == (5, 68) and dev.dtype == torch.int32 and not torch.equal(first[1:], dev[1:])
    hi.refresh()
    assert era.noise_calls == 3


# ------------------------------------------------------------------------------------------------------------------------ wiring --
def _args(**kw):
    return types.SimpleNamespace(**dict(dict(reprob=0.25, remode='pixel', recount=1), **kw))


def test_amd_loop_random_erasing():
    assert amd_loop.random_erasing(_args(reprob=0.)) is None
    assert amd_loop.random_erasing(_args(reprob=0)) is None
    era = amd_loop.random_erasing(_args())
    assert isinstance(era, M.RandomErasing) and (era.probability, era.mode, era.min_count, era.max_count, era.num_splits) == (0.25, 'pixel', 1, 1, 0)
    era = amd_loop.random_erasing(_args(remode='rand', recount=3))
    assert (era.mode, era.min_count, era.max_count) == ('rand', 1, 3)
    with pytest.raises(ValueError):
        amd_loop.random_erasing(_args(recount=9))


def test_cls_stager_refuses_wrong_forms():
    assert staging.cls_form(torch.empty(2, 3, 8, 8, dtype=torch.uint8)) == 'compact'
    assert staging.cls_form(torch.empty(2, 3, 8, 8)) == 'reference'
    bad = [torch.empty(2, 8, 8, 3, dtype=torch.uint8),           # HWC
           torch.empty(2, 1, 8, 8, dtype=torch.uint8),
           torch.empty(2, 3, 8, 8, dtype=torch.float16),
           torch.empty(2, 3, 8, 8, dtype=torch.int32),
           torch.empty(3, 8, 8, dtype=torch.uint8),
           torch.empty(0, 3, 8, 8, dtype=torch.uint8)]
    for t in bad:
        with pytest.raises(ValueError) as e:
            staging.cls_form(t)
        assert str(tuple(t.shape)) in str(e.value) and str(t.dtype) in str(e.value)
        with pytest.raises(ValueError):
            staging.ClsStager._pair((t, torch.zeros(t.shape[0], dtype=torch.int64)))
    ok = torch.empty(2, 3, 8, 8, dtype=torch.uint8)
    for item in (ok, (ok,), (ok, [0, 1]), (ok, torch.zeros(3, dtype=torch.int64)), (ok, torch.tensor(1)), {'rgb': ok}):
        with pytest.raises(ValueError):
            staging.ClsStager._pair(item)
    assert staging.ClsStager._pair([ok, torch.zeros(2, dtype=torch.int64)])[0] is ok
    with pytest.raises(ValueError, match='ClsStager'):
        staging.ClsStagedLoader([], object())
    assert issubclass(staging.ClsStager, staging.BatchStager) and issubclass(staging.ClsStagedLoader, staging.StagedLoader)
    assert M.ClsStager is staging.ClsStager and M.ClsStagedLoader is staging.ClsStagedLoader
