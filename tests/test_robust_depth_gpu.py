"""GPU: the mask-aware robust depth standardisation and the masking of invalid inputs (csrc/depth.hip: mmae_depth_standardize_masked,
mmae_mask_invalid) and their host side (data_ops.robust_depth_standardize, robust_depth_standardize_, mask_invalid_,
dropin/amd_loop.prepare_dense_inputs).

Every element against fp64: the reference of a sample is helpers.depth_std_ref on that sample's compacted valid values with the cuts
(int)((float)n_valid * frac) -- one f32 product each, truncated -- and its returned bound is the tolerance (the arithmetic of the
kernel's last line is the same as mmae_depth_standardize's).  A mask-false element must be +0 in its bits, a mask-true element of a
sample whose slice has fewer than two values a NaN; a NaN matches only a NaN.  Outputs live in Guarded buffers.  Against the fixture
(the reference's own f32 lines on the CPU): 2e-6 max|y| + 1e-6 over the finite elements of a case, the bound
test_truncated_depth_standardize_vs_reference_golden uses, NaN pattern identical.  mmae_mask_invalid: bit for bit."""
import os

import numpy as np
import pytest
import torch

import multimae_amd as M
from dropin import amd_loop
from helpers import Guarded, assert_within, depth_std_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EINVAL = -1
EPS = 1e-6
LO, HI = 0.1, 0.9
SIZES = [2, 3, 7, 1000, 1023, 1024, 1025, 4099]        # below, at and just past the 1024-thread stride; 4099: four strides, n % 4 != 0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'robust_depth.npz')
SENT = -5898331                                        # Guarded's sentinel as int32
NAN, INF = float('nan'), float('inf')
GARBAGE = ([NAN, INF, -INF, 1e30, -1e30, 1e-40, -1e-42, -0.0], [-3.0e38, -NAN, 7.0, 1e-45, INF, NAN, -INF, 2.5e-39])


def _lib():
    from multimae_amd import _lib as L
    return L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _bits_equal(out, ref, what):
    o, r = _bits(out).cpu(), _bits(ref).cpu()
    assert o.shape == r.shape, (what, o.shape, r.shape)
    bad = o != r
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {o.numel()} elements differ in their bits; first at flat {i}: '
                             f'{int(o.reshape(-1)[i]) & 0xffffffff:#x} vs {int(r.reshape(-1)[i]) & 0xffffffff:#x}')


def _untouched(G, what):
    G.intact(what)
    assert bool((_bits(G.view) == SENT).all()), f'{what}: the output was written'


def cuts(nv, lo=LO, hi=HI):
    """(int)((float)n_valid * frac): one f32 product each, truncated"""
    return int(np.float32(nv) * np.float32(lo)), int(np.float32(nv) * np.float32(hi))


def _runs(nv, bounds, g):
    """a shuffled map of nv integers whose sorted form steps up by one at every rank in `bounds` (clipped to the map)"""
    j = torch.arange(nv)
    v = sum((j >= min(max(b, 0), nv)).long() for b in bounds)
    return (v + torch.zeros(nv, dtype=torch.long))[torch.randperm(nv, generator=g)]


def _families(nv, g):
    """f32 [F][nv]: values for the valid positions of a sample, with ties where the cuts of nv fall
      0 rank lo is the FIRST copy of a run and rank hi - 1 the LAST copy of one      1 the last copy / the first copy
      2 both cuts inside one run (the slice is constant)      3 constant      4 family 0, all negative      5 family 1 around zero
      6 a run of zeros of both signs across the cuts      7 continuous, far from zero      8 continuous, small spread"""
    lo, hi = cuts(nv)
    a = max(1, (hi - lo) // 3)
    f0 = _runs(nv, [lo, lo + a, hi - a, hi], g).float()
    f1 = _runs(nv, [lo + 1, hi - 1], g).float()
    f2 = _runs(nv, [lo // 2, nv - (nv - hi) // 2], g).float()
    z = torch.randn(nv, generator=g).sort().values
    z[nv // 12: nv - nv // 12] = 0.0
    z[nv // 12: nv // 2] *= -1.0                          # -0.0 for the lower half of the run, +0.0 for the upper
    z = z[torch.randperm(nv, generator=g)]
    return torch.stack([f0 * 0.37 - 0.6, f1 * 0.37 + 0.25, f2 * 1.5 + 2.0, torch.full((nv,), 3.0), -(f0 * 0.37 + 0.6), (f1 - 1.0) * 0.37, z,
                        torch.randn(nv, generator=g) * 3.0 + 10.0, torch.randn(nv, generator=g) * 1e-3 - 1.0])


def _masks(n, g):
    """bool [K][n]: all valid, none, exactly 1, 2 and 3 (as far as n allows), only the last partial stride, all but one, about half"""
    def some(k):
        m = torch.zeros(n, dtype=torch.bool)
        m[torch.randperm(n, generator=g)[:k]] = True
        return m
    last = torch.zeros(n, dtype=torch.bool)
    last[(n - 1) // 1024 * 1024:] = True
    return torch.stack([torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.bool), some(1), some(2), some(3), last, some(n - 1),
                        torch.rand(n, generator=g) < 0.5])


def _fill_garbage(x, mask, which):
    """what sits under the invalid positions: NaN, +-inf, 1e30, denormals, -0"""
    junk = torch.tensor(GARBAGE[which], dtype=torch.float32)
    idx = torch.nonzero(~mask.reshape(-1)).reshape(-1)
    x.reshape(-1)[idx] = junk[(idx * 7 + which) % len(junk)]
    return x


def _batch(n, seed, which=0):
    """x f32 [B][n], mask bool [B][n]: every mask of _masks with every family of _families in its valid positions"""
    g = torch.Generator().manual_seed(seed)
    xs, ms = [], []
    for m in _masks(n, g):
        fam = _families(int(m.sum()), g)
        x = torch.zeros(fam.shape[0], n)
        x[:, m] = fam
        xs.append(x)
        ms.append(m.expand(fam.shape[0], n))
    x, mask = torch.cat(xs), torch.cat(ms).contiguous()
    return _fill_garbage(x, mask, which), mask


_REFS = {}


def _check(y, x, mask, what, key=None):
    """every element of y [B][n] (on the device) against the fp64 reference of x, mask (on the CPU)"""
    y = y.detach().cpu()
    if key is None or key not in _REFS:
        part = mask & ~torch.isnan(x)
        ref = torch.zeros(x.shape, dtype=torch.float64)
        bound = torch.zeros(x.shape, dtype=torch.float64)
        for b in range(x.shape[0]):
            lo, hi = cuts(int(part[b].sum()))
            if hi - lo < 2:
                ref[b][mask[b]] = NAN
            else:
                r, bd = depth_std_ref(x[b][part[b]][None], lo, hi, EPS)
                ref[b][part[b]], bound[b][part[b]] = r[0], bd[0]
                ref[b][mask[b] & ~part[b]] = NAN                        # a valid NaN stays a NaN
        if key is not None:
            _REFS[key] = (ref, bound)
    ref, bound = _REFS[key] if key is not None else (ref, bound)
    nan = torch.isnan(ref)
    got_nan = torch.isnan(y)
    assert torch.equal(got_nan, nan), (f'{what}: {int((got_nan & ~nan).sum())} NaN(s) where a number is due, {int((nan & ~got_nan).sum())} '
                                       f'number(s) where a NaN is due; first at {torch.nonzero(got_nan != nan)[0].tolist()}')
    zero = torch.zeros(())
    assert_within(torch.where(nan, zero, y), torch.where(nan, zero.double(), ref), bound, what, names=('b', 'i'))
    off = _bits(y)[~mask]
    assert bool((off == 0).all()), f'{what}: {int((off != 0).sum())} mask-false element(s) are not +0.0'


def _run(lib, x, mask, y_ptr, n, lo=LO, hi=HI, eps=EPS):
    return lib.mmae_depth_standardize_masked(x.data_ptr(), None if mask is None else mask.data_ptr(), y_ptr, x.shape[0], n, lo, hi, eps, _st())


@pytest.mark.parametrize('n', SIZES)
def test_masked_standardize_every_element_against_fp64(n):
    lib = _lib()
    xc, mc = _batch(n, 100 + n)
    x, mask = xc.to(DEV), mc.to(DEV)
    x0, m0 = x.clone(), mask.clone()
    B = x.shape[0]
    w = f'mmae_depth_standardize_masked, n = {n}'
    y = Guarded(B, n, n, torch.float32, DEV)
    assert _run(lib, x, mask, y.view.data_ptr(), n) == 0
    _check(y.view, xc, mc, w, key=n)
    y.intact(w)
    _bits_equal(x, x0, w + ': the input')
    assert torch.equal(mask, m0)
    z = Guarded(B, n, n, torch.float32, DEV, fill=x)                   # y aliasing x: bit-equal to out of place
    assert _run(lib, z.view, mask, z.view.data_ptr(), n) == 0
    _bits_equal(z.view, y.view, w + ', in place')
    z.intact(w + ', in place')


@pytest.mark.parametrize('n', SIZES)
def test_garbage_under_the_mask_does_not_reach_the_output(n):
    lib = _lib()
    xa, mc = _batch(n, 100 + n, which=0)
    xb, _ = _batch(n, 100 + n, which=1)
    assert torch.equal(xa[mc], xb[mc]) and (n < 7 or not torch.equal(_bits(xa), _bits(xb)))
    outs = []
    for xc in (xa, xb):
        y = Guarded(xc.shape[0], n, n, torch.float32, DEV)
        assert _run(lib, xc.to(DEV), mc.to(DEV), y.view.data_ptr(), n) == 0
        y.intact(f'garbage {n}')
        outs.append(y.view.clone())
    _bits_equal(outs[0], outs[1], f'n = {n}: two kinds of garbage under the mask')
    _check(outs[1], xb, mc, f'n = {n}, second kind of garbage', key=n)


@pytest.mark.parametrize('n', SIZES)
def test_a_valid_nan_is_left_out_of_the_statistics_and_stays_nan(n):
    lib = _lib()
    xc, mc = _batch(n, 300 + n)
    g = torch.Generator().manual_seed(n)
    hit = mc & (torch.rand(mc.shape, generator=g) < (0.5 if n < 8 else 0.02))
    xc[hit] = NAN
    assert bool(hit.any())
    y = Guarded(xc.shape[0], n, n, torch.float32, DEV)
    assert _run(lib, xc.to(DEV), mc.to(DEV), y.view.data_ptr(), n) == 0
    _check(y.view, xc, mc, f'n = {n}, NaN at valid positions')
    y.intact(f'valid NaN {n}')


@pytest.mark.parametrize('n', [n for n in SIZES if cuts(n)[1] - cuts(n)[0] >= 2])
def test_all_valid_is_bit_equal_to_the_unmasked_kernel(n):
    lib = _lib()
    g = torch.Generator().manual_seed(500 + n)
    x = _families(n, g).to(DEV)
    B = x.shape[0]
    lo, hi = cuts(n)
    ref = Guarded(B, n, n, torch.float32, DEV)
    assert lib.mmae_depth_standardize(x.data_ptr(), ref.view.data_ptr(), B, n, lo, hi, EPS, _st()) == 0
    ones = torch.ones(B, n, dtype=torch.bool, device=DEV)
    for name, mask in (('mask = NULL', None), ('a mask of ones', ones)):
        y = Guarded(B, n, n, torch.float32, DEV)
        assert _run(lib, x, mask, y.view.data_ptr(), n) == 0
        _bits_equal(y.view, ref.view, f'n = {n}, {name} against mmae_depth_standardize [{lo}, {hi})')
        y.intact(name)
    assert not bool(torch.isnan(ref.view).any())


def test_n_2_has_no_slice_of_two():
    assert [n for n in SIZES if cuts(n)[1] - cuts(n)[0] < 2] == [2]


def _gold():
    z = np.load(GOLD)
    return z, sorted(f[2:] for f in z.files if f.startswith('x/'))


def _assert_gold(out, y, k):
    out = out.detach().cpu()
    assert torch.equal(torch.isnan(out), torch.isnan(y)), f'{k}: NaN pattern'
    fin = torch.isfinite(y)
    scale = float(y[fin].abs().max()) if bool(fin.any()) else 0.0
    err = float((out - y)[fin].abs().max()) if bool(fin.any()) else 0.0
    print(k, 'max |engine - fixture|', err, 'bound', 2e-6 * scale + 1e-6)
    assert err <= 2e-6 * scale + 1e-6, (k, err, scale)
    assert bool(torch.isfinite(out[fin]).all())


def test_both_forms_against_the_references_fixture():
    z, cases = _gold()
    for k in cases:
        x, m, y = (torch.from_numpy(z[f'{p}/{k}']) for p in 'xmy')
        xd, md = x.to(DEV), m.to(DEV)
        out = M.robust_depth_standardize(xd, md)
        _assert_gold(out, y, k)
        _bits_equal(xd, x, f'{k}: the input of the out-of-place form')
        buf = torch.empty_like(xd)
        assert M.robust_depth_standardize(xd, md, out=buf) is buf
        inp = xd.clone()
        assert M.robust_depth_standardize_(inp, md) is inp
        _bits_equal(buf, out, f'{k}: out=')
        _bits_equal(inp, out, f'{k}: in place')
    ein, eout, m = (torch.from_numpy(z[k]) for k in ('extra/in', 'extra/out', 'm/multi32'))
    got = ein.to(DEV)
    assert M.mask_invalid_(got, m.to(DEV)) is got
    assert torch.equal(got.cpu(), eout) and bool(torch.isfinite(eout[~m.expand_as(eout)]).all())
    _bits_equal(got, eout, 'mask_invalid_ against the fixture')


def test_prepare_dense_inputs_against_the_references_fixture():
    z, _ = _gold()
    x, m, y, ein, eout, dm = (torch.from_numpy(z[k]).to(DEV) for k in ('x/multi32', 'm/multi32', 'y/multi32', 'extra/in', 'extra/out',
                                                                      'extra/depth_masked_only'))
    rgb = torch.randn(2, 3, 32, 32, device=DEV)
    for std in (True, False):
        tasks = {'rgb': rgb.clone(), 'depth': x.clone(), 'normal': ein.clone(), 'mask_valid': m.clone()}
        inp = {k: v for k, v in tasks.items() if k != 'mask_valid'}
        out = amd_loop.prepare_dense_inputs(inp, tasks, std)
        assert out is inp and torch.equal(out['rgb'], rgb) and out['rgb'] is tasks['rgb'] and torch.equal(tasks['mask_valid'], m)
        assert out['normal'] is tasks['normal'] and torch.equal(out['normal'], eout)        # in place, as the reference
        if std:
            _assert_gold(out['depth'], y.cpu(), 'prepare_dense_inputs')
            assert out['depth'] is not tasks['depth']
            _bits_equal(tasks['depth'], x, 'the loss target stays raw')
        else:
            assert out['depth'] is tasks['depth'] and torch.equal(out['depth'], dm)
    only = {'rgb': rgb}
    assert amd_loop.prepare_dense_inputs(only, {'rgb': rgb, 'depth': x, 'mask_valid': m}, True) is only and only['rgb'] is rgb


@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('n', [1, 3, 1023, 1024, 4099])
def test_mask_invalid_bit_for_bit(C, n):
    lib = _lib()
    B = 3
    g = torch.Generator().manual_seed(17 * n + C)
    x = torch.randn(B, C, n, generator=g)
    special = torch.tensor([NAN, -NAN, INF, -INF, -0.0, 0.0, 1e-42, -1e30])
    at = torch.rand(B, C, n, generator=g) < 0.3                        # NaN, inf and -0.0 on both sides of the mask
    x[at] = special[torch.randint(0, 8, (int(at.sum()),), generator=g)]
    mask = torch.rand(B, n, generator=g) < 0.6
    mask[1] = (torch.arange(n) // 4) % 3 != 0                          # whole quads valid, whole quads invalid
    if n > 100:
        assert bool(torch.isnan(x[mask[:, None].expand_as(x)]).any()) and bool(torch.isnan(x[~mask[:, None].expand_as(x)]).any())
    want = torch.where(mask[:, None], x, torch.zeros(()))
    for shift in (0, 1):                                               # 1: off the 16-byte boundary (the scalar form also at n % 4 == 0)
        buf = Guarded(B * C, n, n, torch.float32, DEV, fill=x.view(B * C, n), shift=shift)
        md = mask.to(DEV)
        assert lib.mmae_mask_invalid(buf.view.data_ptr(), md.data_ptr(), B, C, n, _st()) == 0
        _bits_equal(buf.view, want.view(B * C, n), f'mmae_mask_invalid C = {C}, n = {n}, shift {shift}')
        buf.intact(f'mmae_mask_invalid C = {C}, n = {n}, shift {shift}')
        assert torch.equal(md.cpu(), mask)
    bytes_ = (mask.to(torch.uint8) * 255).to(DEV)                      # any non-zero byte is valid
    buf = Guarded(B * C, n, n, torch.float32, DEV, fill=x.view(B * C, n))
    assert lib.mmae_mask_invalid(buf.view.data_ptr(), bytes_.data_ptr(), B, C, n, _st()) == 0
    _bits_equal(buf.view, want.view(B * C, n), 'a mask of 0 / 255 bytes')


def test_bad_arguments_are_refused_and_nothing_is_written():
    lib = _lib()
    n, B = 1000, 2
    x = torch.randn(B, n, device=DEV)
    mask = torch.rand(B, n, device=DEV) < 0.5
    y = Guarded(B, n, n, torch.float32, DEV)
    yp, xp, mp = y.view.data_ptr(), x.data_ptr(), mask.data_ptr()
    f = lib.mmae_depth_standardize_masked
    assert f(None, mp, yp, B, n, LO, HI, EPS, _st()) == EINVAL
    assert f(xp, mp, None, B, n, LO, HI, EPS, _st()) == EINVAL
    for b in (0, -1):
        assert f(xp, mp, yp, b, n, LO, HI, EPS, _st()) == EINVAL
    for bad_n in (0, -5, 2 ** 24 + 1):                                 # refused through its arguments alone: nothing that large exists
        assert f(xp, mp, yp, B, bad_n, LO, HI, EPS, _st()) == EINVAL, bad_n
    for lo, hi in ((-0.1, 0.9), (0.5, 0.4), (0.1, 1.5), (-1.0, -0.5), (1.1, 1.2), (NAN, 0.9), (0.1, NAN), (NAN, NAN), (-INF, INF)):
        assert f(xp, mp, yp, B, n, lo, hi, EPS, _st()) == EINVAL, (lo, hi)
    assert f(xp, mp, yp, B, n, LO, HI, NAN, _st()) == EINVAL
    m = lib.mmae_mask_invalid
    assert m(None, mp, B, 1, n, _st()) == EINVAL and m(yp, None, B, 1, n, _st()) == EINVAL
    for b, c, nn in ((0, 1, n), (B, 0, n), (B, 1, 0), (-1, 1, n)):
        assert m(yp, mp, b, c, nn, _st()) == EINVAL
    torch.cuda.synchronize()
    _untouched(y, 'refused calls')
    for lo, hi in ((0.0, 1.0), (0.0, 0.0), (1.0, 1.0), (0.3, 0.3)):    # the closed ends are arguments like any other
        assert f(xp, mp, yp, B, n, lo, hi, EPS, _st()) == 0, (lo, hi)
    torch.cuda.synchronize()
    y.intact('accepted calls')
    assert bool(torch.isnan(y.view[mask]).all()) and not bool(y.view[~mask].any())          # lo == hi: the empty slice


def test_no_host_synchronisation():
    z, _ = _gold()
    x, m, ein = (torch.from_numpy(z[k]).to(DEV) for k in ('x/multi32', 'm/multi32', 'extra/in'))
    rgb = torch.randn(2, 3, 32, 32, device=DEV)
    buf, inp, e1 = torch.empty_like(x), x.clone(), ein.clone()
    tasks = {'rgb': rgb, 'depth': x.clone(), 'normal': ein.clone(), 'mask_valid': m}
    ind = {k: v for k, v in tasks.items() if k != 'mask_valid'}
    tasks2 = {'rgb': rgb, 'depth': x.clone(), 'mask_valid': m}
    ind2 = {'rgb': rgb, 'depth': tasks2['depth']}
    _lib()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a = M.robust_depth_standardize(x, m)
        M.robust_depth_standardize(x, None, out=buf)
        M.robust_depth_standardize_(inp, m)
        M.mask_invalid_(e1, m)
        amd_loop.prepare_dense_inputs(ind, tasks, True)
        amd_loop.prepare_dense_inputs(ind2, tasks2, False)
        amd_loop.prepare_dense_inputs({'rgb': rgb}, tasks, True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    _bits_equal(a, inp, 'the calls ran')
    _bits_equal(ind['depth'], a, 'prepare_dense_inputs ran')
