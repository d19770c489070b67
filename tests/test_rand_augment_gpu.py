"""GPU: ``mmae_rand_augment_u8`` (csrc/randaug.hip) against the numpy restatement (tests/randaug_ref.py) and the reference's own
outputs (tests/golden/rand_augment.npz), byte for byte -- every comparison is ``torch.equal``.

1. Every op alone: the golden's op cases (each of the increasing ops and the non-increasing variants, magnitudes 0 / 5 / 10, both signs,
   both interpolations) on the 24 x 40 noise image, the 8 x 8 noise image (Equalize's step is 0) and the one-colour image, one batch
   per image with a case per sample.
2. Layers: a stats op (AutoContrast, Equalize, Contrast) after a geometric op in two- and four-layer rows -- its statistics are those of
   the previous layer's output --, B = 5 with a different op per sample and one sample without layers, the golden's policy cases.
3. Shapes: a policy draw at 33 x 65 (odd width, H W no multiple of the 4-byte access) and at the recipe's 224 x 224.
4. Rows that are wrong on purpose (op codes and layer counts out of range) leave the sample copied; guard bytes around y stay intact,
   with y on and off a 4-byte boundary.  These are valid launches whose bounds are checked, nothing faults.
5. ``ClsStager`` end to end: uint8 batch + policy + random erasing equals restatement, decode, ``mmae_random_erase`` with the same
   tables; the policy's table is drawn first.  Two runs of one call are byte-identical.
"""
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import data_ops, staging

import randaug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'rand_augment.npz'))
META = json.loads(GOLD['meta'].item())
FILL = tuple(META['fill'])


def _run(x, table, layers=4, out=None):
    """numpy batch + numpy table -> numpy output of the kernel"""
    y = data_ops.rand_augment_u8(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(table)).to(DEV),
                                 out=out, layers=layers)
    torch.cuda.synchronize()
    return y


def _same(y, want):
    return torch.equal(y.cpu(), torch.from_numpy(np.ascontiguousarray(want)))


def _noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- 1. every op alone --
@pytest.mark.parametrize('image', ['r24x40', 'r8x8', 'c8x8'])
def test_every_golden_op_case(image):
    cases = [c for c in META['ops'] if c['image'] == image]
    img = GOLD['img/' + image]
    H, W = img.shape[1:]
    rows = []
    for c in cases:
        w = R.fn_layer(c['fn'], c['args'], c['interp'], H, W)
        rows.append(R.make_row([] if w is None else [w], FILL))
    table = np.stack(rows)
    x = np.broadcast_to(img, (len(cases),) + img.shape).copy()
    y = _run(x, table, layers=1)
    assert _same(y, R.apply_table(x, table))
    got = y.cpu().numpy()
    for b, c in enumerate(cases):                                                     # and the reference's own bytes
        if image == 'r24x40':
            assert hashlib.sha256(got[b].tobytes()).digest() == GOLD['op_digest'][c['slot']].tobytes(), c
        else:
            assert np.array_equal(got[b], GOLD['op_small'][c['slot']]), c
    assert {c['fn'] for c in cases} >= {'equalize', 'auto_contrast', 'contrast', 'sharpness', 'rotate', 'shear_x', 'translate_y_rel'}


# ------------------------------------------------------------------------------------------------------------------------ 2. layers --
def _geo(H, W, interp=R.BICUBIC):
    return [R.layer(R.AFFINE, interp=interp, coef=R.rotate_matrix(-21.5, W, H)), R.layer(R.AFFINE, interp=interp, coef=(1, 0.27, 0, 0, 1, 0)),
            R.layer(R.AFFINE, interp=R.BILINEAR, coef=(1, 0, 0, 0, 1, -0.3 * H))]


def test_stats_ops_take_their_statistics_from_the_previous_layer():
    H, W = 24, 40
    x = (60 + _noise((6, 3, H, W), 1) // 3).astype(np.uint8)                         # a narrow range: the fill colour widens it
    g = _geo(H, W)
    rows = [R.make_row([g[0], R.layer(R.AUTOCONTRAST)], FILL),
            R.make_row([g[1], R.layer(R.EQUALIZE)], FILL),
            R.make_row([g[2], R.layer(R.CONTRAST, fbits=R.f32_bits(1.63))], (255, 0, 7)),
            R.make_row([g[0], R.layer(R.EQUALIZE), g[1], R.layer(R.AUTOCONTRAST)], FILL),
            R.make_row([R.layer(R.SOLARIZE, iarg=100), R.layer(R.CONTRAST, fbits=R.f32_bits(0.4)), g[2], R.layer(R.EQUALIZE)], (0, 0, 0)),
            R.make_row([R.layer(R.SHARPNESS, fbits=R.f32_bits(1.9)), R.layer(R.COLOR, fbits=R.f32_bits(0.1)), R.layer(R.AUTOCONTRAST),
                        R.layer(R.BRIGHTNESS, fbits=R.f32_bits(1.3))], FILL)]
    table = np.stack(rows)
    want = R.apply_table(x, table)
    for b in range(3):                      # statistics of the ORIGINAL image would give other bytes: the test can tell the two apart
        assert not np.array_equal(_stale(x[b], table[b]), want[b])
    assert _same(_run(x, table), want)
    assert _same(_run(x, table, layers=2), R.apply_table(x, np.stack([R.make_row([r[4:20], r[20:36]], r[1:4]) for r in rows])))


def _stale(img, row):
    """layer 0 then layer 1 of ``row``, layer 1 with the statistics of ``img`` instead of those of layer 0's output: what a kernel that
    read the wrong buffer would write"""
    fill = row[1:4]
    g = R.apply_layer(img, *R.layer_fields(row, 0), fill)
    op, _, _, fbits, _ = R.layer_fields(row, 1)
    if op == R.CONTRAST:
        grey = R.grey(img)
        return R.blend(np.full_like(g, int(int(grey.astype(np.int64).sum()) / grey.size + 0.5)), g, fbits)
    make = R.autocontrast_lut if op == R.AUTOCONTRAST else R.equalize_lut
    return R._lut(g, [make(h) for h in R.histograms(img)])


def test_a_different_op_per_sample_and_one_without_layers():
    H, W = 24, 40
    x = _noise((5, 3, H, W), 2)
    rows = [R.make_row([R.layer(R.POSTERIZE, iarg=3)], FILL), R.make_row([], FILL),
            R.make_row([R.layer(R.AFFINE, interp=R.BICUBIC, coef=R.rotate_matrix(30.0, W, H))], FILL),
            R.make_row([R.layer(R.EQUALIZE), R.layer(R.INVERT)], FILL),
            R.make_row([R.layer(R.SOLARIZE_ADD, iarg=110), R.layer(R.SHARPNESS, fbits=R.f32_bits(0.1))], FILL)]
    table = np.stack(rows)
    y = _run(x, table)
    assert _same(y, R.apply_table(x, table))
    assert _same(y[1], x[1]) and not _same(y[0], x[0])
    again = _run(x, table)
    assert torch.equal(y, again)                                                      # two runs, the same bytes


@pytest.mark.parametrize('i', range(len(META['policies'])))
def test_golden_policy_cases(i):
    pc = META['policies'][i]
    x = np.stack([GOLD['img/' + k] for k in pc['images']])
    ra = M.RandAugment(pc['config'], dict(pc['hparams']))
    random.seed(pc['seed'])
    np.random.seed(pc['seed'])
    table = ra.draw(x.shape)
    assert _same(_run(x, table, layers=ra.num_layers), GOLD['policy_out'][i])


# ------------------------------------------------------------------------------------------------------------------------ 3. shapes --
@pytest.mark.parametrize('B, H, W, config', [(6, 33, 65, 'rand-m9-n4-mstd0.5-inc1'), (4, 224, 224, 'rand-m9-mstd0.5-inc1')])
def test_policy_draw_at_other_shapes(B, H, W, config):
    x = _noise((B, 3, H, W), 3)
    x[1] = (80 + x[1] // 4).astype(np.uint8)
    ra = M.RandAugment(config, dict(img_mean=FILL, interpolation='bicubic' if W == 224 else 'random'))
    random.seed(21)
    np.random.seed(21)
    table = ra.draw(x.shape)
    assert table[:, 0].max() >= 2 and len({int(v) for v in table[:, 4]}) >= 3
    want = R.apply_table(x, table)
    assert not np.array_equal(want, x)
    assert _same(_run(x, table, layers=ra.num_layers), want)


# ------------------------------------------------------------------------------------------------------------------ 4. wrong rows --
@pytest.mark.parametrize('shift', [0, 3], ids=['aligned', 'unaligned'])
def test_rows_out_of_range_copy_and_nothing_outside_y_is_written(shift):
    B, H, W = 7, 12, 20
    x = _noise((B, 3, H, W), 4)
    inv = R.layer(R.INVERT)
    big = R.layer(R.AFFINE, interp=R.BICUBIC, coef=(1e300, -1e300, 1e308, 7.0, 1e-300, -3.5))
    rows = [R.make_row([R.layer(12), R.layer(-1)], FILL), R.make_row([R.layer(2 ** 31 - 1), R.layer(-2 ** 31)], FILL),
            R.make_row([inv], FILL, n=-5), R.make_row([inv] * 4, FILL, n=2 ** 31 - 1), R.make_row([R.layer(R.AFFINE, interp=9, coef=(1, 0, 0, 0, 1, 0))], FILL),
            R.make_row([big, R.layer(R.POSTERIZE, iarg=-4), R.layer(R.SOLARIZE, iarg=-2 ** 31)], (300, -1, 256)),
            R.make_row([inv, inv, inv], FILL)]
    table = np.stack(rows)
    want = R.apply_table(x, table)
    for b in (0, 1, 2, 3, 4):
        assert np.array_equal(want[b], x[b])                                          # no-ops, n <= 0, n clamped to 4 (an even count of inversions)
    n, guard = x.size, 256
    flat = torch.full((guard + n + guard + shift,), 0xA5, dtype=torch.uint8, device=DEV)[shift:]
    y = flat[guard:guard + n].view(B, 3, H, W)
    assert y.data_ptr() % 4 == shift % 4
    out = _run(x, table, out=y)
    assert out.data_ptr() == y.data_ptr() and _same(y, want)
    assert bool((flat[:guard] == 0xA5).all()) and bool((flat[guard + n:] == 0xA5).all())
    for bad_layers in (0, 5):
        with pytest.raises(ValueError, match='layers'):
            _run(x, table, layers=bad_layers)


# ------------------------------------------------------------------------------------------------------------------- 5. the stager --
def test_cls_stager_augments_then_decodes_and_erases():
    B, H, W = 6, 24, 40
    batches = [(torch.from_numpy(_noise((B, 3, H, W), 10 + k)), torch.arange(B) + 10 * k) for k in range(3)]
    order = []

    class Policy(M.RandAugment):
        def draw(self, shape, chosen=None):
            order.append('policy')
            return super().draw(shape, chosen)

    class Erasing(M.RandomErasing):
        def draw(self, shape):
            order.append('erase')
            return super().draw(shape)

    def make():
        return (Policy('rand-m9-mstd0.5-inc1', dict(img_mean=FILL, interpolation='bicubic')),
                Erasing(probability=1, mode='rand', max_count=2))

    # what the stager must deliver: the policy's table first, then the erase table, per batch, in the order the batches are staged
    ra, era = make()
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    lut = data_ops.rgb_table(staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD).to(DEV)
    want, plain = [], []
    for img, _ in batches:
        t_ra, t_er = ra.draw(img.shape), era.draw(img.shape)
        aug = torch.from_numpy(R.apply_table(img.numpy(), t_ra)).to(DEV)
        x = data_ops.ingest_rgb_u8_chw(aug, lut)
        plain.append(data_ops.ingest_rgb_u8_chw(img.to(DEV), lut))
        want.append(data_ops.random_erase_(x, torch.from_numpy(t_er).to(DEV)))
    torch.cuda.synchronize()
    assert any(not torch.equal(w, p) for w, p in zip(want, plain))
    del order[:]
    ra, era = make()
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    got = [(x.clone(), t.clone()) for x, t in M.ClsStagedLoader(batches, M.ClsStager(DEV, random_erasing=era, rand_augment=ra))]
    torch.cuda.synchronize()
    assert order == ['policy', 'erase'] * 3 and len(got) == 3
    for (x, t), w, (_, host_t) in zip(got, want, batches):
        assert x.dtype == torch.float32 and torch.equal(x.view(torch.int32), w.view(torch.int32)) and torch.equal(t.cpu(), host_t)
    # without a policy the stager is what it was
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    state = np.random.get_state()[1].copy()
    first = next(iter(M.ClsStagedLoader(batches[:1], M.ClsStager(DEV))))
    torch.cuda.synchronize()
    assert torch.equal(first[0], plain[0]) and np.array_equal(np.random.get_state()[1], state)
    # a float32 batch cannot be augmented
    with pytest.raises(ValueError, match='cannot be augmented'):
        M.ClsStager(DEV, rand_augment=ra).stage((torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.int64)))
