"""Golden fixture for multimae_amd.metrics.SegMetric: seeded prediction and label maps and the four histograms the reference's
``intersect_and_union`` (utils/semseg_metrics.py:6-61) returns for them, called directly (``mean_iou`` goes through ``np.float``,
which current numpy no longer has).  Labels are in [0, K) or 255 (ignored); predictions in [0, K).  Two batches per case so that
the tests can check that ``update`` accumulates; class K - 1 of case 'absent' occurs in neither map (its ratios are NaN).
Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_seg_metrics.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

# case -> (K, B, H, W, classes that actually occur, share of ignored labels, share of pixels where the prediction copies the label)
CASES = {'ade': (150, 2, 24, 40, 150, 0.1, 0.6), 'small': (4, 3, 9, 7, 4, 0.3, 0.5), 'absent': (5, 2, 8, 8, 4, 0.0, 0.7)}
IGNORE = 255


def maps(seed, K, B, H, W, used, p_ignore, p_hit):
    rng = np.random.RandomState(seed)
    label = rng.randint(0, used, size=(B, H, W)).astype(np.int64)
    pred = np.where(rng.rand(B, H, W) < p_hit, label, rng.randint(0, used, size=(B, H, W))).astype(np.int64)
    label[rng.rand(B, H, W) < p_ignore] = IGNORE
    return pred, label


def main():
    spec = importlib.util.spec_from_file_location('ref_semseg_metrics', os.path.join(REF, 'utils', 'semseg_metrics.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for i, (name, (K, B, H, W, used, p_ignore, p_hit)) in enumerate(CASES.items()):
        for part in range(2):
            pred, label = maps(1000 + 10 * i + part, K, B, H, W, used, p_ignore, p_hit)
            hist = ref.intersect_and_union(pred.copy(), label.copy(), K, IGNORE, label_map=None)
            out[f'{name}/{part}/pred'], out[f'{name}/{part}/label'] = pred.astype(np.uint8), label.astype(np.uint8)
            out[f'{name}/{part}/hist'] = np.stack([np.asarray(h, dtype=np.int64) for h in hist])
    path = os.path.join(HERE, 'seg_metrics.npz')
    np.savez_compressed(path, **out)
    print('wrote seg_metrics.npz with', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
