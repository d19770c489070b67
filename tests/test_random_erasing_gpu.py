"""GPU: the random-erasing kernels (csrc/erase.hip) and their callers.

1. golden: ``RandomErasing.__call__`` on the inputs of tests/golden/random_erasing.npz (the reference's own class on the CPU) gives
   the reference's output, ``torch.equal``; in 'pixel' mode the same rectangles are erased and nothing else is touched.
2. hand-written tables against the numpy restatement tests/erase_ref.py, for the in-place and the fused kernel: no rectangle, 8
   overlapping ones, empty ones, the four corners, the whole image, odd H W.  'const' / 'rand' bit for bit; 'pixel' bit-equal outside
   the rectangles and within 16 * 2^-24 * max(1, r) of the float64 restatement inside (r = sqrt(-2 ln u1)): u1, u2 are exact, logf is
   within 2 ulp (about 1 ulp on r after the root), sqrtf adds 0.5, cospif / sinpif are within 2 ulp absolute, the product adds 0.5 --
   about 5 units, 16 leaves a threefold margin.
3. moments of the noise over one whole-image rectangle, 5-sigma bounds.
4. fused decode + erase == table lookup then in-place erase, bit for bit in all modes; ``table=None`` == ``ingest_rgb_u8`` of the HWC
   permutation.
5. ``ClsStagedLoader`` / ``ClsStager`` deliver what decoding and erasing each batch directly gives, labels intact, ``into=`` honoured.
6. ``RandomErasing`` + ``Mixup`` + ``SoftTargetCrossEntropy`` inside ``graph.StepGraph``: every replay erases a freshly drawn table.
"""
import json
import os
import random

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import data_ops, staging
from helpers import Guarded

import erase_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'random_erasing.npz'))
CASES = json.loads(GOLD['cases'].item())
MODES = ('const', 'rand', 'pixel')
U = 2.0 ** -24
SEED, CALLS = (0x1234 << 32) | 0x9abcdef0, (1 << 32) | 5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _guarded(shape, fill=None, shift=0):
    B, n = shape[0], int(np.prod(shape[1:]))
    g = Guarded(B, n, n, torch.float32, DEV, fill=None if fill is None else fill.reshape(B, -1), shift=shift)
    return g, g.view.view(shape)


def _lut():
    return data_ops.rgb_table(staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD)


# -------------------------------------------------------------------------------------------------------------------- 1. golden --
@pytest.mark.parametrize('case', list(CASES))
def test_call_matches_the_reference_bit_for_bit(case):
    c = CASES[case]
    x, want = (torch.from_numpy(a) for a in erase_ref.golden_case(GOLD, case))
    g, xd = _guarded(x.shape, fill=x.to(DEV))
    era = M.RandomErasing(**c['kwargs'])
    random.seed(c['seed'])
    torch.manual_seed(c['seed'])
    assert era(xd) is xd
    torch.cuda.synchronize()
    g.intact(case)
    assert torch.equal(xd.cpu(), want) and torch.equal(_bits(xd), _bits(want))
    assert random.random() == float(GOLD[f'{case}/random'][0])


def test_pixel_mode_erases_the_reference_rectangles_and_nothing_else():
    c = CASES['const_p1']
    x, gold = (torch.from_numpy(a) for a in erase_ref.golden_case(GOLD, 'const_p1'))
    g, xd = _guarded(x.shape, fill=x.to(DEV))
    random.seed(c['seed'])
    M.RandomErasing(**dict(c['kwargs'], mode='pixel'))(xd)
    torch.cuda.synchronize()
    g.intact('pixel')
    out = xd.cpu()
    kept = gold == x                                    # the inputs are normal, none is 0: the golden erased exactly the others
    assert (x != 0).all() and (~kept).any()
    assert torch.equal(_bits(out)[kept], _bits(x)[kept])
    assert (out[~kept] != x[~kept]).all() and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------- 2. hand-written tables --
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 7), (1, 3, 13, 17), (3, 4, 9, 3), (2, 3, 8, 16), (1, 2, 5, 48)]


def _layouts(H, W, C, rng):
    """four sets of rectangles: none; 8 overlapping; the corners + empty ones; the whole image (under / over smaller ones)"""
    def col():
        return tuple(rng.standard_normal(4).astype(np.float32)[:max(C, 1)][:4])
    hh, ww = max(1, (H + 1) // 2), max(1, (W + 1) // 2)
    over8 = [(min(r, H - hh), min((3 * r) % 5, W - ww), hh, ww, col()) for r in range(8)]
    h3, w3 = max(1, H // 3), max(1, W // 3)
    corners = [(0, 0, h3, w3, col()), (0, W - w3, h3, w3, col()), (H - h3, 0, h3, w3, col()), (H - h3, W - w3, h3, w3, col()),
               (0, 0, 0, W, col()), (0, 0, H, 0, col()), (H, W, 0, 0, col())]
    whole = [(0, 0, h3, w3, col()), (0, 0, H, W, col()), (H - h3, W - w3, h3, w3, col())]
    return [[], over8, corners, whole]


def _hand_tables(shape, mode):
    B, C, H, W = shape
    rng = np.random.default_rng(sum(shape))
    lay = _layouts(H, W, C, rng)
    return [erase_ref.make_table(B, [lay[(b + k) % 4] for b in range(B)], seed=SEED, calls=CALLS + k, mode=mode) for k in range(4)]


def _check_against_restatement(out, x, table, mode, what):
    """out, x: CPU f32 tensors"""
    want, mask = erase_ref.apply(x.numpy(), table)
    mask_t = torch.from_numpy(mask.copy())
    assert torch.equal(_bits(out)[~mask_t], _bits(x)[~mask_t]), f'{what}: an element outside the rectangles changed'
    if mode != 'pixel':
        assert torch.equal(_bits(out), _bits(torch.from_numpy(want))), what
        return
    z, r = erase_ref.noise(table, x.shape)
    err = np.abs(out.numpy().astype(np.float64) - z)[mask]
    bound = (16 * U * np.maximum(1.0, r))[mask]
    if err.size:
        i = int(np.argmax(err / bound))
        assert (err <= bound).all(), f'{what}: |z - z_ref| = {err[i]:.3e} > {bound[i]:.3e} at erased element {i} of {err.size}'


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', SHAPES)
def test_inplace_kernel_against_the_restatement(shape, mode):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    erased_any = whole = False
    for k, table in enumerate(_hand_tables(shape, mode)):
        g, xd = _guarded(shape, fill=x.to(DEV))
        data_ops.random_erase_(xd, torch.from_numpy(table).to(DEV))
        torch.cuda.synchronize()
        g.intact(f'{shape} {mode} table {k}')
        _check_against_restatement(xd.cpu(), x, table, mode, f'{shape} {mode} table {k}')
        hit = erase_ref.hit_map(table, shape)
        erased_any |= bool((hit >= 0).any())
        whole |= any(bool((hit[b] >= 0).all()) for b in range(shape[0]))
    assert erased_any and whole


# the fused kernel's own paths, beside the shapes above: several workgroups per sample and more than one quad per thread (a workgroup
# covers 4096 elements, a thread's quads lie 1024 elements apart) at (2, 3, 64, 72); quads that straddle a row on the vector path
# (H W % 4 == 0, W % 4 != 0) within one workgroup at (2, 3, 10, 6) and (1, 3, 4, 6) and across workgroups at (2, 3, 50, 54)
FUSED_SHAPES = [s for s in SHAPES if s[1] == 3] + [(2, 3, 64, 72), (2, 3, 50, 54), (2, 3, 10, 6), (1, 3, 4, 6)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', FUSED_SHAPES)
def test_fused_kernel_against_the_restatement(shape, mode):
    u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(sum(shape)))
    lut = _lut()
    x = torch.stack([lut[c][u8[:, c].long()] for c in range(3)], dim=1)
    for k, table in enumerate(_hand_tables(shape, mode)):
        for shift in (0, 1):                                  # shift 1: the output leaves its 16-byte boundary (scalar path)
            g, yd = _guarded(shape, shift=shift)
            got = data_ops.ingest_rgb_u8_chw(u8.to(DEV), lut.to(DEV), torch.from_numpy(table).to(DEV), out=yd)
            torch.cuda.synchronize()
            assert got is yd
            g.intact(f'{shape} {mode} table {k} shift {shift}')
            _check_against_restatement(yd.cpu(), x, table, mode, f'fused {shape} {mode} table {k} shift {shift}')


def test_a_table_that_leaves_the_image_is_intersected_with_it():
    """the host guarantees rectangles inside the image; the kernels intersect what they are given with the image (include/mmae.h) and
    never write outside the tensor"""
    shape = (2, 3, 6, 10)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    table = erase_ref.make_table(2, [[(0, 0, 1, 1)] * 6, [(0, 0, 6, 10)]], mode='const')
    for r, rect in enumerate([(4, 7, 100, 100),                   # leaves the image at the bottom and the right: rows 4-5, columns 7-9
                              (-3, -2, 5, 6),                       # ... at the top and the left: rows 0-1, columns 0-3
                              (2, 2, -4, 3),                        # a negative height: nothing
                              (-10, 0, 5, 10),                      # wholly above the image: nothing
                              (2 ** 31 - 1, 0, 2 ** 31 - 1, 10),    # top + h beyond 32 bits: nothing
                              (3, 5, 0, 2 ** 31 - 1)]):             # empty
        table[1, 4 + 8 * r:8 + 8 * r] = rect
    table[2, 4:8] = (-3, -2, 1 << 30, 1 << 30)                     # covers the image from outside
    table[2, 0] = 100                                               # more rectangles than a row holds
    g, xd = _guarded(shape, fill=x.to(DEV))
    data_ops.random_erase_(xd, torch.from_numpy(table).to(DEV))
    gy, yd = _guarded(shape)
    u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    data_ops.ingest_rgb_u8_chw(u8.to(DEV), _lut().to(DEV), torch.from_numpy(table).to(DEV), out=yd)
    torch.cuda.synchronize()
    g.intact('in place')
    gy.intact('fused')
    want = x.clone()
    want[0, :, 4:, 7:] = 0
    want[0, :, :2, :4] = 0
    want[1] = 0
    assert torch.equal(xd.cpu(), want)
    assert torch.equal(yd.cpu() == 0, want == 0)


def test_entry_points_refuse_bad_arguments():
    from multimae_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2, 3, 4, 4, device=DEV)
    u8 = torch.zeros(2, 3, 4, 4, dtype=torch.uint8, device=DEV)
    lut = _lut().to(DEV)
    tab = torch.zeros(3, 68, dtype=torch.int32, device=DEV)
    for dims in ((0, 3, 4, 4), (2, 0, 4, 4), (2, 3, -1, 4), (2, 3, 4, 0)):
        assert lib.mmae_random_erase(x.data_ptr(), tab.data_ptr(), *dims, None) == -1
    assert lib.mmae_random_erase(None, tab.data_ptr(), 2, 3, 4, 4, None) == -1
    assert lib.mmae_random_erase(x.data_ptr(), None, 2, 3, 4, 4, None) == -1
    for dims in ((0, 4, 4), (2, 0, 4), (2, 4, -2)):
        assert lib.mmae_ingest_rgb_u8_chw_erase(u8.data_ptr(), lut.data_ptr(), tab.data_ptr(), x.data_ptr(), *dims, None) == -1
    for ptrs in ((None, lut.data_ptr(), None, x.data_ptr()), (u8.data_ptr(), None, None, x.data_ptr()), (u8.data_ptr(), lut.data_ptr(), None, None)):
        assert lib.mmae_ingest_rgb_u8_chw_erase(*ptrs, 2, 4, 4, None) == -1
    assert b'null pointer' in lib.mmae_last_error()
    torch.cuda.synchronize()
    assert not x.any()


# ------------------------------------------------------------------------------------------------------------------- 3. moments --
def test_noise_moments_and_call_counter():
    shape = (1, 3, 256, 256)
    n = 3 * 256 * 256
    tables = [erase_ref.make_table(1, [[(0, 0, 256, 256)]], seed=2024, calls=k, mode='pixel') for k in (0, 1)]

    def moments(z):
        z = z.astype(np.float64)
        mean, var = z.mean(), z.var()
        a, b = z[..., :-1] - mean, z[..., 1:] - mean
        return mean, var, (a * b).mean() / var

    def check(z, what):
        mean, var, corr = moments(z)
        assert abs(mean) <= 5 / np.sqrt(n), (what, mean)
        assert abs(var - 1) <= 5 * np.sqrt(2 / n), (what, var)
        assert abs(corr) <= 5 / np.sqrt(n), (what, corr)

    ref = [erase_ref.noise(t, shape)[0] for t in tables]
    check(ref[0], 'restatement')                       # the seed passes on the CPU: a failure below is the kernel's
    out = []
    for t in tables:
        xd = torch.zeros(shape, device=DEV)
        data_ops.random_erase_(xd, torch.from_numpy(t).to(DEV))
        out.append(xd.cpu().numpy())
    check(out[0], 'kernel')
    assert np.abs(out[0] - ref[0]).max() <= 16 * U * 6
    assert not np.array_equal(out[0], out[1]) and (out[0] != out[1]).mean() > 0.99
    assert np.abs(out[1] - ref[1]).max() <= 16 * U * 6


# ------------------------------------------------------------------------------------------------------ 4. fused equals composed --
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('shape', [(2, 3, 13, 17), (1, 3, 8, 16), (3, 3, 5, 3), (2, 3, 64, 72), (2, 3, 50, 54), (2, 3, 10, 6), (1, 3, 4, 6)])
def test_fused_equals_decode_then_erase(shape, mode):
    u8 = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(sum(shape) + 1)).to(DEV)
    lut = _lut().to(DEV)
    looked_up = torch.stack([lut[c][u8[:, c].long()] for c in range(3)], dim=1).contiguous()
    erased = 0
    for k, table in enumerate(_hand_tables(shape, mode)):
        t = torch.from_numpy(table).to(DEV)
        g, yd = _guarded(shape)
        data_ops.ingest_rgb_u8_chw(u8, lut, t, out=yd)
        composed = data_ops.random_erase_(looked_up.clone(), t)
        torch.cuda.synchronize()
        g.intact(f'{shape} {mode} table {k}')
        assert torch.equal(_bits(yd), _bits(composed)), (shape, mode, k)
        erased += int((_bits(composed) != _bits(looked_up)).sum())
    assert erased > 0
    g, yd = _guarded(shape)
    data_ops.ingest_rgb_u8_chw(u8, lut, None, out=yd)
    hwc = data_ops.ingest_rgb_u8(u8.permute(0, 2, 3, 1).contiguous(), lut)
    torch.cuda.synchronize()
    g.intact('decode only')
    assert torch.equal(_bits(yd), _bits(hwc)) and torch.equal(_bits(yd), _bits(looked_up))


# ------------------------------------------------------------------------------------------------------------------- 5. staging --
def _host_batches(form, pinned):
    g = torch.Generator().manual_seed(31)
    out = []
    for k in range(3):
        if form == 'compact':
            img = torch.randint(0, 256, (4, 3, 13, 17), dtype=torch.uint8, generator=g)
        else:
            img = torch.randn(4, 3, 13, 17, generator=g)
        tgt = torch.randint(0, 1000, (4,), generator=g)
        out.append((img.pin_memory(), tgt.pin_memory()) if pinned else (img, tgt))
    return out


def _era(mode='pixel'):
    era = M.RandomErasing(probability=0.75, mode=mode, max_count=2)
    era.noise_seed = 77
    return era


def _direct(batches, era):
    """each batch decoded and erased directly, in order"""
    lut = _lut().to(DEV)
    out = []
    for img, tgt in batches:
        d = img.to(DEV)
        x = torch.stack([lut[c][d[:, c].long()] for c in range(3)], dim=1).contiguous() if img.dtype == torch.uint8 else d.clone()
        out.append((era(x), tgt.to(DEV)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('pinned', [False, True], ids=['pageable', 'pinned'])
@pytest.mark.parametrize('form', ['compact', 'reference'])
def test_cls_staged_loader_equals_direct_decode_and_erase(form, pinned):
    batches = _host_batches(form, pinned)
    plain = _direct(batches, M.RandomErasing(probability=0))
    random.seed(5)
    want = _direct(batches, _era())
    assert any(not torch.equal(w[0], p[0]) for w, p in zip(want, plain)), 'the seed erases nothing'
    random.seed(5)
    loader = M.ClsStagedLoader(batches, M.ClsStager(DEV, random_erasing=_era()))
    assert len(loader) == 3
    got = []
    for x, tgt in loader:
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tgt.is_cuda
        got.append((x.clone(), tgt.clone()))
    torch.cuda.synchronize()
    assert len(got) == 3
    for (x, tgt), (wx, wt), (_, host_t) in zip(got, want, batches):
        assert torch.equal(_bits(x), _bits(wx))
        assert tgt.dtype == host_t.dtype and torch.equal(tgt, wt) and torch.equal(tgt.cpu(), host_t)
    # without a RandomErasing (the evaluation loader) the batch is decoded only
    decoded = list(M.ClsStagedLoader(batches[:1], M.ClsStager(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(_bits(decoded[0][0]), _bits(plain[0][0]))
    # erase_float32=False (a host transform that erases already): float32 batches are copied only and nothing is drawn for them,
    # uint8 batches are erased as before
    era = _era()
    random.seed(5)
    state = random.getstate()
    once = list(M.ClsStagedLoader(batches, M.ClsStager(DEV, random_erasing=era, erase_float32=False)))
    torch.cuda.synchronize()
    if form == 'reference':
        assert era.noise_calls == 0 and random.getstate() == state
        assert all(torch.equal(_bits(o[0]), _bits(p[0])) for o, p in zip(once, plain))
    else:
        assert era.noise_calls == 3 and all(torch.equal(_bits(o[0]), _bits(w[0])) for o, w in zip(once, want))


def test_cls_stager_into_writes_the_given_tensors(monkeypatch):
    batches = _host_batches('compact', False)
    stager = M.ClsStager(DEV, random_erasing=_era('const'))
    gx, xs = _guarded((4, 3, 13, 17))
    ts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    random.seed(9)
    want = _direct(batches, _era('const'))
    random.seed(9)
    for (img, tgt), (wx, wt) in zip(batches, want):
        done = torch.cuda.Event()
        done.record()
        x, t = stager.get(stager.stage((img, tgt), into=(xs, ts), after=done))
        assert x.data_ptr() == xs.data_ptr() and t.data_ptr() == ts.data_ptr()
        torch.cuda.synchronize()
        gx.intact('into')
        assert torch.equal(_bits(xs), _bits(wx)) and torch.equal(ts, wt)
    with pytest.raises(ValueError, match='into'):
        stager.stage(batches[0], into=(xs[:2], ts[:2]))
    with pytest.raises(ValueError, match='into'):
        stager.stage(batches[0], into={'images': xs})
    with pytest.raises(ValueError, match='already on'):
        stager.stage((batches[0][0].to(DEV), batches[0][1]))
    with pytest.raises(ValueError, match=r'\(4, 13, 17, 3\).*uint8'):
        stager.stage((batches[0][0].permute(0, 2, 3, 1), batches[0][1]))
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='capture'):
        stager.stage(batches[0])


# ------------------------------------------------------------------------------------------------------------------- 6. capture --
def test_erasing_mixup_and_criterion_inside_a_step_graph():
    """RandomErasing + Mixup + SoftTargetCrossEntropy captured in graph.StepGraph: the erase table and the mixup block are host inputs
    redrawn before every replay, so three runs under one seed give the batches of three eager calls, bit for bit"""
    from multimae_amd.graph import StepGraph
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(6, 3, 16, 20, generator=g).to(DEV)
    labels = torch.randint(0, 7, (6,), generator=g).to(DEV)
    logits = (torch.randn(6, 7, generator=g) * 2).to(DEV).requires_grad_(True)
    mix, crit = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode='elem', num_classes=7), M.SoftTargetCrossEntropy()
    work = x0.clone()

    def make_step(era):
        def step():
            work.copy_(x0)
            era(work)
            xm, t = mix(work, labels)
            loss = crit(logits, t)
            (d,) = torch.autograd.grad(loss, logits)
            return xm, t, loss, d
        return step

    def seed():
        random.seed(21)
        np.random.seed(21)

    era = M.RandomErasing(probability=0.75, mode='pixel', max_count=2)
    era.noise_seed = 99
    step = make_step(era)
    seed()
    eager = []
    for _ in range(3):
        eager.append([v.detach().clone() for v in step()])
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0]) and era.noise_calls == 3
    era = M.RandomErasing(probability=0.75, mode='pixel', max_count=2)
    era.noise_seed = 99
    run = StepGraph(make_step(era))
    seed()
    for k in range(3):
        out = run()
        torch.cuda.synchronize()
        for a, b in zip(out, eager[k]):
            assert torch.equal(_bits(a), _bits(b)), k
    assert run.replays == 3 and run.n_host_inputs == 2 and era.noise_calls == 3
