"""CPU: host side of RandAugment (multimae_amd/rand_augment.py, data_ops.rand_augment_u8, staging.ClsStager, dropin/amd_loop.py) and
the restatement the GPU tests take as their oracle (tests/randaug_ref.py).

* the restatement reproduces every output of the golden's op cases (tests/golden/rand_augment.npz, from the reference's own functions
  on PIL images) byte for byte, and -- where PIL is importable -- a fresh seeded sweep of PIL itself;
* ``RandAugment.draw`` under the golden's seeds picks the reference's ops, computes its arguments, leaves both generators where the
  reference leaves them, and its table fed to the restatement gives the reference's output bytes;
* config parsing, what raises ``ValueError`` / ``NotImplementedError``, ``ClsStager``'s argument checks, ``amd_loop.rand_augment``;
* the library exports the entry points, the ABI version is still 7, and a dry run shows ``ClsStager(rand_augment=None)`` issuing the
  calls it issued before the policy existed.
"""
import ctypes
import hashlib
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, data_ops, ops, rand_augment as RA, staging
from dropin import amd_loop

import randaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'rand_augment.npz'))
META = json.loads(GOLD['meta'].item())
FILL = tuple(META['fill'])


def _case_output(case):
    x = GOLD['img/' + case['image']]
    w = R.fn_layer(case['fn'], case['args'], case['interp'], x.shape[1], x.shape[2])
    return R.apply_row(x, R.make_row([] if w is None else [w], FILL))


# ---------------------------------------------------------------------------------------------------------------- the restatement --
def test_golden_covers_every_op_and_what_the_generator_promises():
    names = {c['name'] for c in META['ops']}
    assert names == set(RA.RAND_INCREASING_TRANSFORMS) | set(RA.RAND_TRANSFORMS)
    assert {c['image'] for c in META['ops']} == {'r24x40', 'r8x8', 'c8x8'}
    assert {c['magnitude'] for c in META['ops'] if c['name'] == 'Rotate'} == {0.0, 5.0, 10.0}
    assert {(c['negate'], c['interp']) for c in META['ops'] if c['name'] == 'ShearX'} == {(False, 2), (False, 3), (True, 2), (True, 3)}
    assert GOLD['img/r24x40'].shape == (3, 24, 40) and os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'rand_augment.npz')) < 100 * 1024


def test_restatement_reproduces_every_golden_op_case():
    bad = []
    for case in META['ops']:
        y = _case_output(case)
        if case['image'] == 'r24x40':
            ok = hashlib.sha256(y.tobytes()).digest() == GOLD['op_digest'][case['slot']].tobytes()
        else:
            ok = np.array_equal(y, GOLD['op_small'][case['slot']])
        if not ok:
            bad.append((case['id'], case['name'], case['image'], case['magnitude'], case['negate'], case['interp']))
    assert not bad, bad


def test_restatement_edge_cases_named_by_the_golden():
    x8, c8 = GOLD['img/r8x8'], GOLD['img/c8x8']
    assert all(np.array_equal(R.equalize_lut(h), np.arange(256)) for h in R.histograms(x8))        # step == 0
    assert np.array_equal(R.autocontrast(c8), c8) and np.array_equal(R.equalize(c8), c8)           # hi <= lo, a single bin
    x = GOLD['img/r24x40']
    y = R.enhance(x, R.BRIGHTNESS, R.f32_bits(1.9))
    assert ((y == 255) & (x < 200)).any()                                                           # a factor above 1 clips
    y = R.affine(x, R.rotate_matrix(30.0, 40, 24), R.BICUBIC, FILL)
    assert np.all(y == np.array(FILL, dtype=np.uint8)[:, None, None], axis=0).any()                # fill pixels are left
    assert np.array_equal(R.apply_row(x, R.make_row([R.layer(99), R.layer(-1), R.layer(R.AFFINE, interp=7)])), x)
    assert np.array_equal(R.apply_row(x, R.make_row([R.layer(R.INVERT)], n=0)), x)
    assert np.array_equal(R.apply_row(x, R.make_row([R.layer(R.INVERT)] * 4, n=9)), x)             # clamped to 4: inverted 4 times


def test_restatement_against_pil_itself():
    """a fresh seeded sweep, in full bytes: every op family at sizes the golden does not hold"""
    Image = pytest.importorskip('PIL.Image')
    from PIL import ImageEnhance, ImageOps
    rng = np.random.RandomState(7)

    def pil(a):
        return Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)))

    def arr(im):
        return np.asarray(im).transpose(2, 0, 1)

    bad = {}

    def chk(name, got, want):
        n = int((got != want).sum())
        if n:
            bad[name] = bad.get(name, 0) + n

    for it in range(12):
        H, W = [(24, 40), (8, 8), (33, 65), (5, 3)][it % 4]
        a = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
        if it % 5 == 1:
            a = (a // 64 * 64).astype(np.uint8)
        if it % 5 == 2:
            a = rng.randint(100, 110, (3, H, W)).astype(np.uint8)
        im = pil(a)
        chk('autocontrast', R.autocontrast(a), arr(ImageOps.autocontrast(im)))
        chk('equalize', R.equalize(a), arr(ImageOps.equalize(im)))
        chk('invert', R.invert(a), arr(ImageOps.invert(im)))
        for bits in range(1, 8):
            chk('posterize', R.posterize(a, bits), arr(ImageOps.posterize(im, bits)))
        for t in (0, 1, 77, 128, 255, 256):
            chk('solarize', R.solarize(a, t), arr(ImageOps.solarize(im, t)))
        for f in (0.0, 0.1, 0.37, 1.0, 1.3, 1.9):
            for op, cls in ((R.BRIGHTNESS, ImageEnhance.Brightness), (R.COLOR, ImageEnhance.Color), (R.CONTRAST, ImageEnhance.Contrast),
                            (R.SHARPNESS, ImageEnhance.Sharpness)):
                chk(cls.__name__, R.enhance(a, op, R.f32_bits(f)), arr(cls(im).enhance(f)))
        for interp in (R.BICUBIC, R.BILINEAR):
            for f in (0.13, -0.3):
                for m in ((1, f, 0, 0, 1, 0), (1, 0, 0, f, 1, 0), (1, 0, f * W, 0, 1, 0), (1, 0, 0, 0, 1, f * H)):
                    chk(f'affine/{interp}', R.affine(a, m, interp, FILL),
                        arr(im.transform(im.size, Image.AFFINE, m, resample=interp, fillcolor=FILL)))
            for deg in (3.0, -27.3, 30.0):
                chk(f'rotate/{interp}', R.affine(a, R.rotate_matrix(deg, W, H), interp, FILL), arr(im.rotate(deg, resample=interp, fillcolor=FILL)))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ the policy --
@pytest.mark.parametrize('i', range(len(META['policies'])))
def test_draw_reproduces_the_reference_policy(i):
    pc = META['policies'][i]
    x = np.stack([GOLD['img/' + k] for k in pc['images']])
    ra = M.RandAugment(pc['config'], dict(pc['hparams']))
    random.seed(pc['seed'])
    np.random.seed(pc['seed'])
    chosen = []
    table = ra.draw(x.shape, chosen)
    assert (random.random(), float(np.random.rand())) == (pc['random'], pc['np_rand'])             # both generators end where the reference's do
    assert table.shape == (8, 68) and table.dtype == np.int32
    assert chosen == [[a[0] for a in app] for app in pc['applied']]
    H, W = x.shape[2:]
    for b, app in enumerate(pc['applied']):                                                          # the arguments, layer by layer
        want = [R.fn_layer(fn, args, interp, H, W) for _, fn, args, interp in app if fn is not None]
        want = [w for w in want if w is not None]
        assert np.array_equal(table[b], R.make_row(want, FILL)), (b, app)
    assert np.array_equal(R.apply_table(x, table), GOLD['policy_out'][i])


def test_draw_resolves_no_ops_on_the_host():
    ra = M.RandAugment('rand-m0-n4', dict(img_mean=FILL, interpolation='bicubic'))
    random.seed(3)
    np.random.seed(3)
    t = ra.draw((16, 3, 8, 8))
    n = t[:, 0]
    assert n.min() == 0 and n.max() <= 4 and 0 < n.sum() < 64                                        # prob skipped some, kept some
    for b in range(16):
        assert not t[b, 4 + 16 * int(n[b]):].any() and all(t[b, 4 + 16 * l] != R.NOOP for l in range(int(n[b])))
    ra.prob = 1.0
    row = np.zeros(68, dtype=np.int32)
    ra._draw_op(row, 'Rotate', 8, 8)                                                                  # magnitude 0: a rotation by 0 degrees
    assert row[0] == 0
    ra._draw_op(row, 'ShearX', 8, 8)                                                                  # a shear by 0 stays: PIL resamples
    assert row[0] == 1 and row[4] == R.AFFINE and row[5] == R.BICUBIC
    ra20 = M.RandAugment('rand-m20-mmax20')
    ra20.prob = 1.0
    row = np.zeros(68, dtype=np.int32)
    ra20._draw_op(row, 'Posterize', 8, 8)                                                             # int(2 * 4) = 8 bits: PIL returns the image
    assert row[0] == 0
    ra20._draw_op(row, 'PosterizeIncreasing', 8, 8)                                                   # 4 - 8 bits: everything is masked
    assert row[0] == 1 and list(row[4:7]) == [R.POSTERIZE, 0, 0]


def test_config_parsing_and_errors():
    ra = M.RandAugment('rand-m9-mstd0.5-inc1', dict(translate_const=100, img_mean=FILL))
    assert (ra.magnitude, ra.num_layers, ra.magnitude_std, ra.magnitude_max, ra.choice_weights) == (9, 2, 0.5, None, None)
    assert ra.names == RA.RAND_INCREASING_TRANSFORMS and ra.interpolation == (2, 3) and ra.fill == FILL and ra.translate_pct == 0.45
    ra = M.RandAugment('rand-m7-n3-w0-mstd101-mmax15', dict(interpolation=3, translate_pct=0.3))
    assert (ra.magnitude, ra.num_layers, ra.magnitude_std, ra.magnitude_max) == (7, 3, float('inf'), 15)
    assert ra.names == RA.RAND_TRANSFORMS and ra.interpolation == 3 and ra.translate_pct == 0.3 and ra.fill == (128, 128, 128)
    assert abs(ra.choice_weights.sum() - 1) < 1e-12 and ra.choice_weights[RA.RAND_TRANSFORMS.index('Rotate')] == pytest.approx(0.3)
    assert M.RandAugment('rand-inc0').names == RA.RAND_INCREASING_TRANSFORMS                       # the reference tests the string
    assert M.RandAugment('rand').magnitude == 10 and M.RandAugment('rand', dict(interpolation='random')).interpolation == (2, 3)
    assert M.RandAugment('rand-n4').num_layers == 4
    hp = dict(img_mean=FILL)
    M.RandAugment('rand-mstd0.5', hp)
    assert hp == dict(img_mean=FILL)                                                                # the caller's dict is not written
    with pytest.raises(ValueError, match='n = 5'):
        M.RandAugment('rand-n5')
    with pytest.raises(ValueError, match='unknown config section'):
        M.RandAugment('rand-q3')
    with pytest.raises(ValueError, match='w1'):
        M.RandAugment('rand-w1')
    with pytest.raises(ValueError, match='img_mean'):
        M.RandAugment('rand', dict(img_mean=(1, 2, 300)))
    for cfg in ('augmix-m5-w4-d2', 'original', 'v0', 'originalr'):
        with pytest.raises(NotImplementedError):
            M.RandAugment(cfg, {})
    for interp in ('lanczos', 'hamming', 1, 5, 0, (2, 1)):
        with pytest.raises(NotImplementedError, match='interpolation'):
            M.RandAugment('rand', dict(interpolation=interp))
    with pytest.raises(NotImplementedError, match='transpose'):
        RA.rotate_matrix(90.0, 8, 8)
    for shape in ((3, 8, 8), (2, 1, 8, 8), (0, 3, 8, 8), (2, 3, 0, 8)):
        with pytest.raises(ValueError, match='shape'):
            M.RandAugment('rand').draw(shape)
    row = np.zeros(68, dtype=np.int32)
    for _ in range(4):
        RA.pack_layer(row, RA.INVERT)
    with pytest.raises(ValueError, match='4 layers'):
        RA.pack_layer(row, RA.INVERT)


def _args(**kw):
    d = dict(aa='rand-m9-mstd0.5-inc1', input_size=224, train_interpolation='bicubic', imagenet_default_mean_and_std=True, reprob=0.25,
             remode='pixel', recount=1, device='cuda')
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_amd_loop_rand_augment():
    ra = amd_loop.rand_augment(_args())
    assert isinstance(ra, M.RandAugment) and ra.fill == (124, 116, 104) and ra.interpolation == 3 and ra.translate_const == 100
    assert (ra.magnitude, ra.magnitude_std, ra.num_layers) == (9, 0.5, 2) and ra.names == RA.RAND_INCREASING_TRANSFORMS
    assert amd_loop.rand_augment(_args(train_interpolation='random')).interpolation == (2, 3)
    assert amd_loop.rand_augment(_args(train_interpolation='bilinear')).interpolation == 2
    assert amd_loop.rand_augment(_args(train_interpolation='nearest')).interpolation == 2          # _pil_interp's default
    assert amd_loop.rand_augment(_args(imagenet_default_mean_and_std=False)).fill == (128, 128, 128)
    assert amd_loop.rand_augment(_args(input_size=(160, 192))).translate_const == 72
    assert amd_loop.rand_augment(_args(aa=None)) is None and amd_loop.rand_augment(_args(aa='none')) is None
    with pytest.raises(NotImplementedError):
        amd_loop.rand_augment(_args(train_interpolation='lanczos'))
    with pytest.raises(NotImplementedError):
        amd_loop.rand_augment(_args(aa='augmix-m5'))


# ------------------------------------------------------------------------------------------------------------- library and plumbing --
def test_library_exports_the_entry_points_and_abi_stays_7():
    for n in ('mmae_rand_augment_u8', 'mmae_rand_augment_scratch_bytes'):
        assert n in _lib.declared_symbols()
    assert len(_lib._PROTOS['mmae_rand_augment_u8'][1]) == 10 and _lib._PROTOS['mmae_rand_augment_scratch_bytes'][0] is ctypes.c_int64
    assert (_lib.RA_MAX_LAYERS, _lib.RA_ROW) == (4, 68) == (R.MAX_LAYERS, R.ROW) == (RA.MAX_LAYERS, RA.ROW_WORDS)
    header = open(_lib.HEADER).read()
    assert '#define MMAE_RA_MAX_LAYERS 4' in header and '#define MMAE_RA_ROW 68' in header and '#define MMAE_ABI_VERSION 7' in header
    assert os.path.exists(_lib.LIB_PATH), 'libmmae_hip.so is not built'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.mmae_abi_version() == 7
    fn = lib.mmae_rand_augment_scratch_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int] * 4
    img = (5 * 3 * 33 * 65 + 15) // 16 * 16
    assert [fn(5, 33, 65, n) for n in (1, 2, 3, 4)] == [5 * 1024, 5 * 1024 + img, 5 * 1024 + 2 * img, 5 * 1024 + 2 * img]
    assert fn(5, 33, 65, 0) == -1 and fn(5, 33, 65, 5) == -1 and fn(0, 33, 65, 2) == -1
    aug = lib.mmae_rand_augment_u8                    # refused before any launch: no GPU is touched
    aug.restype = ctypes.c_int
    aug.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert aug(None, p, p, p, 4096, 1, 2, 2, 1, None) != 0
    assert aug(p, p, p + 64, p + 1024, 64, 1, 2, 2, 1, None) != 0             # scratch too small
    assert aug(p, p + 512, p + 4, p + 1024, 2048, 1, 2, 2, 1, None) != 0      # x and y overlap
    assert aug(p, p + 512, p + 64, p + 1024, 2048, 1, 2, 2, 5, None) != 0     # layers out of range


@pytest.fixture
def recorded():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    rec = _lib._lib = dryrun_harness.RecordingLib()
    yield rec
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


def test_rand_augment_u8_validates_its_arguments(recorded):
    x = torch.zeros(2, 3, 4, 6, dtype=torch.uint8)
    t = torch.zeros(2, 68, dtype=torch.int32)
    y = data_ops.rand_augment_u8(x, t, layers=2)
    assert y.shape == x.shape and y.dtype == torch.uint8 and y.data_ptr() != x.data_ptr()
    out = torch.empty_like(x)
    assert data_ops.rand_augment_u8(x, t, out=out) is out
    assert [n for n, _ in recorded.calls] == ['mmae_rand_augment_scratch_bytes', 'mmae_rand_augment_u8'] * 2
    assert recorded.calls[1][1][4:9] == [16, 2, 4, 6, 2] and recorded.calls[3][1][8] == 4
    for bad in (x.float(), x[:, :2], x[0], x.permute(0, 1, 3, 2), torch.zeros(0, 3, 4, 6, dtype=torch.uint8), np.zeros((2, 3, 4, 6), np.uint8)):
        with pytest.raises((ValueError, AttributeError)):
            data_ops.rand_augment_u8(bad, t)
    for bad in (t.long(), torch.zeros(3, 68, dtype=torch.int32), torch.zeros(2, 67, dtype=torch.int32), t.numpy(),
                torch.zeros(2, 136, dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match='table'):
            data_ops.rand_augment_u8(x, bad)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match='layers'):
            data_ops.rand_augment_u8(x, t, layers=bad)
    with pytest.raises(ValueError, match='out must not be x'):
        data_ops.rand_augment_u8(x, t, out=x)
    with pytest.raises(ValueError, match='out must be'):
        data_ops.rand_augment_u8(x, t, out=torch.zeros(2, 3, 4, 6))


def _bare_stager(**kw):
    """a ClsStager without its copy stream: ``_stage_one`` alone runs on the host under the stubbed library"""
    s = object.__new__(staging.ClsStager)
    s.device = torch.device('cpu')
    s.table = data_ops.rgb_table(staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD)
    s.random_erasing, s.erase_float32, s.rand_augment = None, True, None
    s.__dict__.update(kw)
    s._upload = lambda table, hold: (hold.append(table), torch.from_numpy(table))[1]
    return s


def test_stager_without_a_policy_issues_the_calls_it_issued_before(recorded):
    h = torch.zeros(2, 3, 4, 6, dtype=torch.uint8)
    hold = []
    out = _bare_stager()._stage_one('images', h, 'compact', None, hold)
    assert out.shape == (2, 3, 4, 6) and out.dtype == torch.float32 and hold == []
    assert recorded.calls == [('mmae_ingest_rgb_u8_chw_erase', ['ptr', 'ptr', 'NULL', 'ptr', 2, 4, 6, 'NULL'])]
    del recorded.calls[:]
    _bare_stager(random_erasing=M.RandomErasing(probability=1))._stage_one('images', h, 'compact', None, hold)
    assert recorded.calls == [('mmae_ingest_rgb_u8_chw_erase', ['ptr', 'ptr', 'ptr', 'ptr', 2, 4, 6, 'NULL'])] and len(hold) == 1
    del recorded.calls[:]
    _bare_stager(random_erasing=M.RandomErasing(probability=1))._stage_one('images', h.float(), 'reference', None, hold)
    assert [n for n, _ in recorded.calls] == ['mmae_random_erase']


def test_stager_with_a_policy_augments_between_copy_and_ingest_and_draws_its_table_first(recorded):
    order = []

    class Policy(M.RandAugment):
        def draw(self, shape, chosen=None):
            order.append('policy')
            return super().draw(shape, chosen)

    class Erasing(M.RandomErasing):
        def draw(self, shape):
            order.append('erase')
            return super().draw(shape)

    h = torch.zeros(2, 3, 4, 6, dtype=torch.uint8)
    hold = []
    s = _bare_stager(rand_augment=Policy('rand-m9-n3-mstd0.5-inc1', dict(img_mean=FILL)), random_erasing=Erasing(probability=1))
    s._stage_one('images', h, 'compact', None, hold)
    assert order == ['policy', 'erase'] and len(hold) == 2 and hold[0].shape == (2, 68) and hold[1].shape == (3, 68)
    assert [n for n, _ in recorded.calls] == ['mmae_rand_augment_scratch_bytes', 'mmae_rand_augment_u8', 'mmae_ingest_rgb_u8_chw_erase']
    assert recorded.calls[1][1][5:9] == [2, 4, 6, 3]                                                 # B, H, W, the policy's n
    del recorded.calls[:]
    s._stage_one('target', torch.zeros(2, dtype=torch.int64), 'reference', None, hold)               # labels: a copy, no launch
    assert recorded.calls == []


def test_stager_argument_validation():
    with pytest.raises(ValueError, match='rand_augment must be'):
        staging.ClsStager('cuda', rand_augment='rand-m9')
    with pytest.raises(ValueError, match='rand_augment must be'):
        staging.ClsStager('cuda', rand_augment=M.RandomErasing())
    s = _bare_stager(rand_augment=M.RandAugment('rand'))
    f32 = (torch.zeros(2, 3, 4, 6), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='cannot be augmented'):
        s._accept(f32)
    u8 = (torch.zeros(2, 3, 4, 6, dtype=torch.uint8), f32[1])
    assert s._accept(u8)[0] is u8[0] and _bare_stager()._accept(f32)[0] is f32[0]
    assert M.RandAugment is RA.RandAugment
    import inspect
    assert inspect.signature(staging.ClsStager.__init__).parameters['rand_augment'].default is None
    assert inspect.signature(amd_loop.cls_staged_loader).parameters['rand_augment'].default is None
