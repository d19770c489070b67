"""Golden fixture for random erasing from the reference's own ``RandomErasing(device='cpu')`` (utils/random_erasing.py) in batch
mode on seeded f32 batches.  The file is loaded by path, so that ``utils/__init__.py``'s other imports are not needed.

``random_erasing.npz``:
  cases              JSON: case name -> {shape, seed, kwargs}
  <case>/x           the input batch: standard normal rounded to fp16's 11 bits and stored as fp16 (an erased pixel is distinguishable
                     from an untouched one; the reference ran on its float32 value)
  <case>/erased      the elements of the reference's output that differ from the input, after ``random.seed(seed);
                     torch.manual_seed(seed)``: a bit mask over the flattened batch (np.packbits)
  <case>/values      the float32 values of those elements, in order.  Input + mask + values are the output bit for bit
                     (``tests/erase_ref.golden_case`` puts it together; this generator checks that it does)
  <case>/random      the next ``random.random()`` after the call: the position of Python's generator
  <case>/torch_rand  the next ``torch.rand(1)`` after the call: the position of torch's CPU generator

What the reference does on the cases: ``const_p05`` erases 2 of 8 samples, ``thin`` rejects 15 of 21 attempts, ``splits`` leaves
samples 0-1 untouched, ``rand_cnt3`` draws 14 rectangles (3, 3, 3, 1, 3, 1 per sample; the count goes through ``randint``).

The generator counts what the reference did on each case (attempts drawn, rectangles placed per sample) and fails when an edit to the
cases loses one of: a case with both an untouched and an erased sample; a rejected attempt; a sample with 3 rectangles; a split skip
that leaves the first ``B // num_splits`` samples alone.

Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_random_erasing.py
"""
import importlib.util
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

OUT = os.path.join(HERE, 'random_erasing.npz')
CASES = {
    'const_p1': dict(shape=(4, 3, 13, 17), seed=1, kwargs=dict(probability=1, mode='const')),
    'const_p05': dict(shape=(8, 3, 12, 20), seed=2, kwargs=dict(probability=0.5, mode='const')),
    'rand_cnt3': dict(shape=(6, 3, 16, 16), seed=3, kwargs=dict(probability=1, mode='rand', max_count=3)),
    'thin': dict(shape=(6, 3, 5, 48), seed=4, kwargs=dict(probability=1, mode='const')),
    'splits': dict(shape=(6, 3, 9, 11), seed=5, kwargs=dict(probability=1, mode='rand', num_splits=3)),
    'c1': dict(shape=(3, 1, 7, 9), seed=6, kwargs=dict(probability=1, mode='rand', min_count=2, max_count=2)),
}


def load_reference():
    spec = importlib.util.spec_from_file_location('ref_random_erasing', os.path.join(REF, 'utils', 'random_erasing.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class CountingRandom:
    """Python's ``random`` module with the ``uniform`` calls counted (two per attempt)"""

    def __init__(self):
        self.uniform_calls = 0

    def __getattr__(self, name):
        return getattr(random, name)

    def uniform(self, a, b):
        self.uniform_calls += 1
        return random.uniform(a, b)


def main():
    ref = load_reference()
    counter = ref.random = CountingRandom()
    placed = []                                   # rectangles placed, one entry per _get_pixels call
    get_pixels = ref._get_pixels

    def counting_get_pixels(*a, **kw):
        placed.append(1)
        return get_pixels(*a, **kw)

    ref._get_pixels = counting_get_pixels

    class Counting(ref.RandomErasing):
        def _erase(self, *a):
            before = len(placed)
            super()._erase(*a)
            self.per_sample.append(len(placed) - before)

    out = {'cases': np.array(json.dumps(CASES))}
    kept = {}
    seen = dict(mixed=False, rejected=False, three=False, split=False)
    for name, case in CASES.items():
        shape, seed, kw = case['shape'], case['seed'], case['kwargs']
        x = torch.randn(shape, generator=torch.Generator().manual_seed(100 + seed)).half().float()   # 11 significant bits: a smaller file
        era = Counting(device='cpu', **kw)
        era.per_sample = []
        counter.uniform_calls, n0 = 0, len(placed)
        random.seed(seed)
        torch.manual_seed(seed)
        y = era(x.clone())
        nxt_random, nxt_torch = random.random(), torch.rand(1)
        erased = [bool((y[b] != x[b]).any()) for b in range(shape[0])]
        assert any(erased), f'{name}: the reference erased nothing'
        attempts, rects = counter.uniform_calls // 2, len(placed) - n0
        skipped = shape[0] // kw['num_splits'] if kw.get('num_splits', 0) > 1 else 0
        assert len(era.per_sample) == shape[0] - skipped
        print(f'{name}: erased samples {sum(erased)} of {shape[0]}, attempts {attempts}, rectangles {rects}, per sample {era.per_sample}')
        seen['mixed'] |= any(erased) and not all(erased) and not skipped
        seen['rejected'] |= attempts > rects
        seen['three'] |= 3 in era.per_sample
        if skipped:
            seen['split'] |= not any(erased[:skipped]) and all(erased[skipped:])
        xn, yn = x.numpy(), y.numpy()
        kept[name] = (xn, yn)
        changed = yn.view(np.int32) != xn.view(np.int32)
        out[f'{name}/x'] = xn.astype(np.float16)
        out[f'{name}/erased'] = np.packbits(changed)
        out[f'{name}/values'] = yn[changed]
        out[f'{name}/random'] = np.array([nxt_random], dtype=np.float64)
        out[f'{name}/torch_rand'] = nxt_torch.numpy()
    assert all(seen.values()), f'the cases no longer cover {[k for k, v in seen.items() if not v]}'
    np.savez_compressed(OUT, **out)
    sys.path.insert(0, os.path.dirname(HERE))
    import erase_ref
    gold = np.load(OUT)
    for name in CASES:                            # the stored form gives back the reference's input and output bit for bit
        gx, gy = erase_ref.golden_case(gold, name)
        assert np.array_equal(gx.view(np.int32), kept[name][0].view(np.int32)) and np.array_equal(gy.view(np.int32), kept[name][1].view(np.int32))
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
