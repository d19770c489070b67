"""Golden fixture for the mask-aware robust depth standardisation and the masking of invalid input values of the dense fine-tuning
loops, made BY THE REFERENCE'S OWN LINES.

The reference has no function for the step: it is inline in ``train_one_epoch`` and ``evaluate`` of run_finetuning_depth.py and of
run_finetuning_taskonomy.py, from the comment ``# Robust depth standardization`` to the fill ``input_dict[task][~...] = 0.0``.  This
script reads that block from the read-only checkout at generation time, asserts that all four copies are the same text after
dedent, executes it unmodified on CPU tensors and records inputs, masks and outputs (nothing of the text is copied into the repo).
It then asserts that an fp64 restatement of its own agrees with the reference's f32 output within HALF the bound
tests/test_robust_depth_gpu.py uses against the fixture (2e-6 max|y| + 1e-6 over the finite elements of a case), NaN pattern
identical, and prints how far inside each case stayed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_robust_depth.py          (build container only)

Cases, at 32 x 32 and 64 x 64: continuous depth (rand * 9 + 0.5), quantised depth (randint(0, 24) / 8: ties at both cuts), skewed
depth (rand ** 2 * 80), valid fractions per sample from 5 % to 100 %; samples with 0, 1 and 2 valid pixels (NaN at the valid
positions) and one with exactly 3 at the end of the map (the smallest finite one); and a run with a second, 3-channel input whose
invalid positions hold NaN, for the masking lines.
"""
import os
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
SCRIPTS = ('run_finetuning_depth.py', 'run_finetuning_taskonomy.py')
OUT = os.path.join(HERE, 'robust_depth.npz')
FRACTIONS = {32: (0.05, 0.25, 0.5, 0.8, 0.95, 1.0), 64: (0.4, 1.0)}


def reference_blocks(path):
    lines = open(path).read().splitlines()
    firsts = [i for i, l in enumerate(lines) if l.strip() == '# Robust depth standardization']
    blocks = []
    for first in firsts:
        last = next(i for i in range(first, len(lines)) if lines[i].strip().startswith('input_dict[task][~') and lines[i].rstrip().endswith('= 0.0'))
        blocks.append(textwrap.dedent('\n'.join(lines[first:last + 1])))
    return blocks


def reference_code():
    blocks = [b for s in SCRIPTS for b in reference_blocks(os.path.join(REF, s))]
    assert len(blocks) == 4, len(blocks)                       # train + eval of both scripts
    assert all(b == blocks[0] for b in blocks), 'the four copies of the block differ'
    b = blocks[0]
    assert 'torch.sort' in b and '.var()' in b and 'repeat_interleave' in b and '.float()' not in b, b
    return b


def run_reference(code, inputs, mask, standardize=True):
    """executes the block on clones; returns the resulting input_dict and the tasks_dict it ran with"""
    from einops import rearrange
    tasks_dict = {k: v.clone() for k, v in inputs.items()}
    tasks_dict['mask_valid'] = mask.clone()
    input_dict = {k: v for k, v in tasks_dict.items() if k != 'mask_valid'}
    ns = dict(torch=torch, np=np, rearrange=rearrange, standardize_depth=standardize, tasks_dict=tasks_dict, input_dict=input_dict)
    exec(compile(code, os.path.join(REF, SCRIPTS[0]), 'exec'), ns)
    return ns['input_dict'], tasks_dict


def restate64(x, mask, lo_frac=0.1, hi_frac=0.9, eps=1e-6):
    """the step in fp64 with numpy: x f32 (B, 1, H, W), mask bool of the same shape"""
    x, mask = np.asarray(x), np.asarray(mask)
    y = np.zeros(x.shape, np.float64)
    for b in range(x.shape[0]):
        v, m = x[b].reshape(-1).astype(np.float64), mask[b].reshape(-1)
        part = np.sort(v[m & ~np.isnan(v)])
        nv = np.float32(len(part))
        lo, hi = int(nv * np.float32(lo_frac)), int(nv * np.float32(hi_frac))      # one f32 product each, truncated
        out = np.zeros_like(v)
        if hi - lo < 2:
            out[m] = np.nan
        else:
            s = part[lo:hi]
            out[m] = (v[m] - s.mean()) / np.sqrt(s.var(ddof=1) + eps)
        y[b] = out.reshape(x[b].shape)
    return y


def bound(y):
    """the test's bound against the fixture, from the finite elements of the case"""
    f = np.isfinite(y)
    return 2e-6 * float(np.abs(y[f]).max() if f.any() else 0.0) + 1e-6


def _mask(gen, B, S, fractions):
    m = torch.zeros(B, 1, S, S, dtype=torch.bool)
    for b, f in enumerate(fractions):
        m[b] = torch.rand(1, S, S, generator=gen) < f if f < 1.0 else True
    return m


def _few(S):
    """masks of 0, 1, 2 valid pixels, and of exactly 3 at the end of the map"""
    m = torch.zeros(4, 1, S, S, dtype=torch.bool)
    m[1].view(-1)[S + 3] = True
    m[2].view(-1)[[5, S * S // 2]] = True
    m[3].view(-1)[-3:] = True
    return m


def main():
    code = reference_code()
    gen = torch.Generator().manual_seed(23)
    families = {
        'cont': lambda B, S: torch.rand(B, 1, S, S, generator=gen) * 9.0 + 0.5,
        'quant': lambda B, S: torch.randint(0, 24, (B, 1, S, S), generator=gen).float() / 8.0,
        'skew': lambda B, S: (torch.rand(B, 1, S, S, generator=gen) ** 2) * 80.0,
    }
    out = {}
    for S, fr in FRACTIONS.items():
        for name, make in families.items():
            k = f'{name}{S}'
            x, m = make(len(fr), S), _mask(gen, len(fr), S, fr)
            res, _ = run_reference(code, {'rgb': torch.zeros(len(fr), 3, 2, 2), 'depth': x}, m)
            out['x/' + k], out['m/' + k], out['y/' + k] = x.numpy(), m.numpy(), res['depth'].numpy()
        k = f'few{S}'
        x, m = families['quant' if S == 64 else 'cont'](4, S), _few(S)
        res, _ = run_reference(code, {'depth': x}, m)
        out['x/' + k], out['m/' + k], out['y/' + k] = x.numpy(), m.numpy(), res['depth'].numpy()
    # the masking lines: a 3-channel extra input beside the depth, NaN under the invalid positions; once with the depth standardised
    # and once with standardize_depth off (the depth is then masked like any other input)
    B, S = 2, 32
    m = _mask(gen, B, S, (0.7, 0.3))
    x = families['cont'](B, S)
    extra = torch.randn(B, 3, S, S, generator=gen)
    extra[~m.expand(B, 3, S, S)] = float('nan')
    extra[0, 1, 0, :4] = torch.tensor([-0.0, float('inf'), float('-inf'), 0.0])        # whatever the mask says there
    rgb = torch.randn(B, 3, S, S, generator=gen)
    res, _ = run_reference(code, {'rgb': rgb, 'depth': x, 'normal': extra}, m)
    assert torch.equal(res['rgb'], rgb)
    off, _ = run_reference(code, {'rgb': rgb, 'depth': x, 'normal': extra}, m, standardize=False)
    out.update({'x/multi32': x.numpy(), 'm/multi32': m.numpy(), 'y/multi32': res['depth'].numpy(), 'extra/in': extra.numpy(),
                'extra/out': res['normal'].numpy(), 'extra/depth_masked_only': off['depth'].numpy()})
    assert np.array_equal(off['normal'].numpy(), res['normal'].numpy(), equal_nan=True)

    for k in sorted(f[2:] for f in out if f.startswith('x/')):
        y, r = out['y/' + k], restate64(out['x/' + k], out['m/' + k])
        assert np.array_equal(np.isnan(y), np.isnan(r)), k
        assert not np.isinf(y).any(), k
        f = np.isfinite(y)
        err, bd = float(np.abs(y[f] - r[f]).max()) if f.any() else 0.0, bound(y)
        print(f'{k}: max |reference - fp64| = {err:.3e}, bound {bd:.3e}, {bd / max(err, 1e-300):.1f}x inside', flush=True)
        assert err <= 0.5 * bd, (k, err, bd)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes:', {k: tuple(v.shape) for k, v in out.items() if k.startswith(('x/', 'extra/'))})
    assert os.path.getsize(OUT) < 300 * 1000


if __name__ == '__main__':
    main()
