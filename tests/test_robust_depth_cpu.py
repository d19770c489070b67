"""CPU: host side of the mask-aware robust depth standardisation and the masking of invalid inputs (data_ops.robust_depth_standardize,
robust_depth_standardize_, mask_invalid_, dropin/amd_loop.prepare_dense_inputs) against the C ABI stub of dryrun_harness: which entry
point each function calls, with which B, C, n, fractions and pointers; every refusal; the exported symbols; and the fixture
(tests/golden/robust_depth.npz, the reference's own lines) against an fp64 restatement written here.  Numbers from the stub are
garbage by design; the kernels are checked in tests/test_robust_depth_gpu.py.

Bound of the restatement against the fixture: 2e-6 max|y| + 1e-6 over the finite elements of a case, the bound
test_truncated_depth_standardize_vs_reference_golden uses (the reference sums in f32); the generator asserted half of it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, data_ops, ops
from dropin import amd_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'robust_depth.npz')
STD, MSK = 'mmae_depth_standardize_masked', 'mmae_mask_invalid'


@pytest.fixture()
def stubbed():
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()


class Recorder:
    """wraps the stub library: records the arguments of every call but the bookkeeping ones"""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name in ('mmae_last_error', 'mmae_abi_version', 'mmae_struct_size'):
            return fn

        def rec(*args):
            self.calls.append((name, args))
            return fn(*args)
        return rec

    def names(self):
        return [n for n, _ in self.calls]


def _f32(x):
    return float(np.float32(x))


def _batch(B=3, H=6, W=10, C=3):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(B, 1, H, W, generator=g) + 0.5, torch.rand(B, 1, H, W, generator=g) < 0.7,
            torch.randn(B, C, H, W, generator=g), torch.randn(B, 3, H, W, generator=g))


def test_robust_depth_standardize_calls_the_masked_kernel_out_of_place(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask, _, _ = _batch()
    d0 = depth.clone()
    y = M.robust_depth_standardize(depth, mask)
    assert rec.names() == [STD]
    a = rec.calls[0][1]
    assert a[0] == depth.data_ptr() and a[1] == mask.data_ptr() and a[2] == y.data_ptr() and a[2] != a[0]
    assert a[3:5] == (3, 60) and (_f32(a[5]), _f32(a[6]), _f32(a[7])) == (_f32(0.1), _f32(0.9), _f32(1e-6)) and a[8] == 0
    assert y is not depth and y.shape == depth.shape and y.dtype == torch.float32 and torch.equal(depth, d0)
    out = torch.empty_like(depth)
    assert M.robust_depth_standardize(depth, None, lo=0.25, hi=0.75, eps=1e-3, out=out) is out
    a = rec.calls[1][1]
    assert a[0] == depth.data_ptr() and a[1] is None and a[2] == out.data_ptr() and a[3:8] == (3, 60, 0.25, 0.75, 1e-3)
    assert M.robust_depth_standardize(depth, mask, out=depth) is depth                  # out= may be the input: the aliasing pointer
    assert rec.calls[2][1][0] == rec.calls[2][1][2] == depth.data_ptr()
    assert rec.names() == [STD] * 3


def test_the_in_place_form_passes_the_aliasing_pointer(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask, _, _ = _batch(B=2, H=5, W=7)
    assert M.robust_depth_standardize_(depth, mask) is depth
    a = rec.calls[0][1]
    assert rec.names() == [STD] and a[0] == a[2] == depth.data_ptr() and a[1] == mask.data_ptr() and a[3:5] == (2, 35)
    assert M.robust_depth_standardize_(depth) is depth and rec.calls[1][1][1] is None


@pytest.mark.parametrize('C', [1, 3])
def test_mask_invalid_calls_its_kernel_with_b_c_n(stubbed, C):
    rec = _lib._lib = Recorder(_lib._lib)
    _, mask, x, _ = _batch(C=C)
    assert M.mask_invalid_(x, mask) is x
    assert rec.names() == [MSK] and rec.calls[0][1] == (x.data_ptr(), mask.data_ptr(), 3, C, 60, 0)


def test_prepare_dense_inputs_rgb_only_makes_no_call(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask, _, rgb = _batch()
    tasks = {'rgb': rgb, 'depth': depth, 'mask_valid': mask}
    for std in (True, False):
        inp = {'rgb': rgb}
        assert amd_loop.prepare_dense_inputs(inp, tasks, std) is inp and inp == {'rgb': rgb}
    assert rec.calls == []


def test_prepare_dense_inputs_without_standardisation_masks_the_depth_in_place(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask, _, rgb = _batch()
    tasks = {'rgb': rgb, 'depth': depth, 'mask_valid': mask}
    inp = {'rgb': rgb, 'depth': depth}
    out = amd_loop.prepare_dense_inputs(inp, tasks, False)
    assert out is inp and out['depth'] is depth is tasks['depth']                       # in place, aliasing the target as the reference does
    assert rec.names() == [MSK] and rec.calls[0][1] == (depth.data_ptr(), mask.data_ptr(), 3, 1, 60, 0)


def test_prepare_dense_inputs_standardises_the_depth_and_masks_the_others(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask, normal, rgb = _batch()
    edges = torch.randn(3, 1, 6, 10)
    tasks = {'rgb': rgb, 'depth': depth, 'normal': normal, 'edges': edges, 'mask_valid': mask}
    inp = {k: v for k, v in tasks.items() if k != 'mask_valid'}
    d0 = depth.clone()
    out = amd_loop.prepare_dense_inputs(inp, tasks, True)
    assert out is inp and list(out) == ['rgb', 'depth', 'normal', 'edges'] and out['rgb'] is rgb
    assert rec.names() == [STD, MSK, MSK]
    s = rec.calls[0][1]
    assert s[0] == depth.data_ptr() and s[1] == mask.data_ptr() and s[2] == out['depth'].data_ptr() and s[3:5] == (3, 60)
    assert (_f32(s[5]), _f32(s[6]), _f32(s[7])) == (_f32(0.1), _f32(0.9), _f32(1e-6))
    assert out['depth'] is not depth and tasks['depth'] is depth and s[2] != depth.data_ptr() and torch.equal(depth, d0)
    assert rec.calls[1][1] == (normal.data_ptr(), mask.data_ptr(), 3, 3, 60, 0) and out['normal'] is normal
    assert rec.calls[2][1] == (edges.data_ptr(), mask.data_ptr(), 3, 1, 60, 0) and out['edges'] is edges


def _bad_inputs():
    depth, mask, x, _ = _batch()
    return {
        'double': (depth.double(), mask),
        'half': (depth.half(), mask),
        'not_contiguous': (depth.transpose(2, 3), mask.transpose(2, 3)),
        'three_dims': (depth[:, 0], mask[:, 0]),
        'not_a_tensor': (depth.numpy(), mask),
        'mask_uint8': (depth, mask.to(torch.uint8)),
        'mask_float': (depth, mask.float()),
        'mask_other_shape': (depth, mask[:, :, :5]),
        'mask_other_batch': (depth, mask[:2]),
        'mask_three_dims': (depth, mask[:, 0]),
        'mask_not_contiguous': (depth, torch.zeros(3, 1, 10, 6, dtype=torch.bool).transpose(2, 3)),
        'mask_other_device': (depth, torch.zeros(3, 1, 6, 10, dtype=torch.bool, device='meta')),
        'mask_not_a_tensor': (depth, mask.numpy()),
    }


@pytest.mark.parametrize('case', list(_bad_inputs()))
def test_anything_else_raises_value_error(stubbed, case):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask = _bad_inputs()[case]
    with pytest.raises(ValueError, match='robust_depth_standardize:'):
        M.robust_depth_standardize(depth, mask)
    with pytest.raises(ValueError, match='robust_depth_standardize_:'):
        M.robust_depth_standardize_(depth, mask)
    with pytest.raises(ValueError, match='mask_invalid_:'):
        M.mask_invalid_(depth, mask)
    if isinstance(depth, torch.Tensor) and depth.dim() == 4 and isinstance(mask, torch.Tensor):
        with pytest.raises(ValueError):
            amd_loop.prepare_dense_inputs({'depth': depth}, {'depth': depth, 'mask_valid': mask}, True)
        with pytest.raises(ValueError):
            amd_loop.prepare_dense_inputs({'depth': depth}, {'depth': depth, 'mask_valid': mask}, False)
    assert rec.calls == []


def test_more_refusals(stubbed):
    rec = _lib._lib = Recorder(_lib._lib)
    depth, mask, x, _ = _batch()
    with pytest.raises(ValueError, match='one channel'):
        M.robust_depth_standardize(x, mask)                                          # three channels are no depth map
    with pytest.raises(ValueError, match='one channel'):
        M.robust_depth_standardize_(x, None)
    with pytest.raises(ValueError, match='mask_valid'):
        M.mask_invalid_(x, mask.expand(3, 3, 6, 10).contiguous())                    # the mask has one channel
    with pytest.raises(ValueError, match='mask_valid'):
        M.mask_invalid_(x, None)
    for bad in (torch.empty(3, 1, 6, 9), torch.empty(3, 1, 6, 10, dtype=torch.float64), torch.empty(3, 1, 10, 6).transpose(2, 3),
                torch.empty(3, 1, 6, 10, device='meta')):
        with pytest.raises(ValueError, match='out must be'):
            M.robust_depth_standardize(depth, mask, out=bad)
    with pytest.raises(ValueError, match='empty'):
        M.robust_depth_standardize(torch.empty(0, 1, 6, 10), None)
    assert rec.calls == []


def test_a_cpu_tensor_is_refused_without_the_stub():
    depth, mask, x, _ = _batch()
    with pytest.raises(ValueError, match='on the GPU'):
        M.robust_depth_standardize(depth, mask)
    with pytest.raises(ValueError, match='on the GPU'):
        M.robust_depth_standardize_(depth, mask)
    with pytest.raises(ValueError, match='on the GPU'):
        M.mask_invalid_(x, mask)


def test_the_three_functions_are_exported():
    assert M.robust_depth_standardize is data_ops.robust_depth_standardize
    assert M.robust_depth_standardize_ is data_ops.robust_depth_standardize_
    assert M.mask_invalid_ is data_ops.mask_invalid_


def test_the_library_exports_both_symbols_and_keeps_its_abi_version():
    lib = _lib.load()
    assert lib.mmae_abi_version() == 7
    V, F, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    assert _lib._PROTOS[STD] == (I, [V, V, V, I, I, F, F, F, V]) and _lib._PROTOS[MSK] == (I, [V, V, I, I, I, V])
    for name in (STD, MSK):
        assert name in _lib.declared_symbols() and getattr(lib, name).argtypes == _lib._PROTOS[name][1]


def restate64(x, mask, lo_frac=0.1, hi_frac=0.9, eps=1e-6):
    """the step in fp64: per sample the valid, non-NaN values sorted, the cuts as one f32 product each, truncated, mean and unbiased
    variance of the slice, (x - mean) / sqrt(var + eps) where the mask is set and 0 elsewhere; a slice of fewer than two: NaN there"""
    y = torch.zeros(x.shape, dtype=torch.float64)
    for b in range(x.shape[0]):
        v, m = x[b].double(), mask[b]
        part = v[m & ~torch.isnan(v)].sort().values
        nv = torch.tensor(part.numel(), dtype=torch.float32)
        lo, hi = int(nv * torch.tensor(lo_frac, dtype=torch.float32)), int(nv * torch.tensor(hi_frac, dtype=torch.float32))
        if hi - lo < 2:
            y[b][m] = float('nan')
        else:
            s = part[lo:hi]
            y[b][m] = (v[m] - s.mean()) / torch.sqrt(s.var(unbiased=True) + eps)
    return y


def test_the_fixture_loads_and_the_fp64_restatement_reproduces_it():
    assert os.path.getsize(GOLD) < 300 * 1000
    z = np.load(GOLD)
    cases = sorted(f[2:] for f in z.files if f.startswith('x/'))
    assert set(cases) == {f'{k}{s}' for k in ('cont', 'quant', 'skew', 'few') for s in (32, 64)} | {'multi32'}
    for k in cases:
        x, m, y = (torch.from_numpy(z[f'{p}/{k}']) for p in 'xmy')
        S = int(k[-2:])
        assert x.shape == m.shape == y.shape == (x.shape[0], 1, S, S) and m.dtype == torch.bool and y.dtype == torch.float32
        ref = restate64(x, m)
        assert torch.equal(torch.isnan(y), torch.isnan(ref)), k
        assert not bool(torch.isinf(y).any()) and bool((y[~m] == 0).all()), k
        fin = torch.isfinite(y)
        scale = float(y[fin].abs().max()) if bool(fin.any()) else 0.0
        err = float((y.double() - ref)[fin].abs().max()) if bool(fin.any()) else 0.0
        print(k, 'max |fixture - fp64|', err, 'bound', 2e-6 * scale + 1e-6)
        assert err <= 2e-6 * scale + 1e-6, (k, err, scale)
    # what the cases are there for
    valid = {k: torch.from_numpy(z['m/' + k]).flatten(1).sum(1).tolist() for k in cases}
    for S in (32, 64):
        assert valid[f'few{S}'] == [0, 1, 2, 3] and bool(torch.from_numpy(z[f'm/few{S}'])[3].flatten()[-3:].all())
        y = torch.from_numpy(z[f'y/few{S}'])
        mk = torch.from_numpy(z[f'm/few{S}'])
        assert not bool(y[0].any()) and bool(torch.isnan(y[1:3][mk[1:3]]).all()) and bool(torch.isfinite(y[3]).all())
        assert valid[f'cont{S}'][-1] == S * S                                          # 100 % valid
    assert valid['cont32'][0] < 0.08 * 1024                                            # ~5 % valid
    q = torch.from_numpy(z['x/quant32'])[-1].flatten().sort().values                   # ties at both cuts of the all-valid sample
    assert q[int(0.1 * 1024) - 1] == q[int(0.1 * 1024)] and q[int(0.9 * 1024) - 1] == q[int(0.9 * 1024)]
    ein, eout, m = torch.from_numpy(z['extra/in']), torch.from_numpy(z['extra/out']), torch.from_numpy(z['m/multi32'])
    assert ein.shape == eout.shape == (2, 3, 32, 32)
    special = torch.zeros_like(ein, dtype=torch.bool)
    special[0, 1, 0, :4] = True                                                        # -0, inf, -inf, +0, whatever the mask says there
    assert bool(torch.isnan(ein[~m.expand_as(ein) & ~special]).all()) and bool((~m.expand_as(ein)).any())
    assert ein[0, 1, 0, :4].view(torch.int32).tolist() == [-2 ** 31, 0x7f800000, 0xff800000 - 2 ** 32, 0]
    want = torch.where(m, ein, torch.zeros(()))
    assert torch.equal(eout.view(torch.int32), want.view(torch.int32))                  # kept bits, +0 under the mask
    dm = torch.from_numpy(z['extra/depth_masked_only'])
    assert torch.equal(dm, torch.where(m, torch.from_numpy(z['x/multi32']), torch.zeros(())))
