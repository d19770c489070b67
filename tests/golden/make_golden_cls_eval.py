"""Golden fixture for the classification evaluation from the reference's own code on the CPU: ``accuracy`` (utils/metrics.py:31-38),
``torch.nn.CrossEntropyLoss`` as ``evaluate()`` of run_finetuning_cls.py builds it (:582), and ``MetricLogger`` / ``SmoothedValue``
(utils/logger.py) updated the way ``evaluate()`` updates them (:604-607).  ``utils`` is stood in for by an empty package with the
reference's path, so that ``utils/__init__.py``'s other imports are not needed while ``utils/logger.py``'s relative import works.

Groups of ``cls_eval.npz``:
  case/<B>x<K>/x, target     seeded f32 logits and int64 targets, (B, K) in GEOMS.  The logits are 2 randn with a uniform [0, 8) bonus on
                             the target's class, so that top-1, top-5 and misses all occur
  case/<B>x<K>/acc           f32 [2]: accuracy(x, target, topk=(1, 5)) -- for K = 3 the reference clamps top-5 to K
  case/<B>x<K>/loss          f32 [1]: nn.CrossEntropyLoss()(x, target)
  ml/x<i>, ml/target<i>      the three batches of the accumulation check, K = 1000, batch sizes ML_SIZES (the middle one is the
                             128 x 1000 case itself and is not stored twice)
  ml/global_avg              f64 [3]: MetricLogger's global_avg of loss, acc1, acc5 after the three updates and
                             synchronize_between_processes() (a no-op without an initialised process group)

No row holds a second logit equal to its target's (asserted below): ``topk`` leaves the order among equal logits unspecified, the
engine fixes it (the lower index first), and without such a tie the two cannot differ -- every case can be compared bit for bit.

Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cls_eval.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

GEOMS = ((6, 3), (6, 7), (128, 1000), (6, 1001))
ML_K = 1000
ML_SIZES = (6, 128, 5)


def batch(B: int, K: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, K, (B,), generator=g)
    x = torch.randn(B, K, generator=g) * 2
    x[torch.arange(B), target] += torch.rand(B, generator=g) * 8
    zt = x.gather(1, target[:, None])
    assert int((x == zt).sum()) == B, 'a logit ties with its target\'s: choose another seed'
    return x, target


def import_utils():
    pkg = types.ModuleType('utils')
    pkg.__path__ = [os.path.join(REF, 'utils')]
    sys.modules['utils'] = pkg
    import utils.logger as lg
    import utils.metrics as mt
    return lg, mt


def main():
    lg, mt = import_utils()
    crit = torch.nn.CrossEntropyLoss()
    out = {}
    for B, K in GEOMS:
        x, target = batch(B, K, 100 * B + K)
        acc1, acc5 = mt.accuracy(x, target, topk=(1, 5))
        assert acc1.dtype == torch.float32 and acc5.dtype == torch.float32
        pre = f'case/{B}x{K}/'
        out[pre + 'x'], out[pre + 'target'] = x.numpy(), target.numpy()
        out[pre + 'acc'] = np.array([acc1.item(), acc5.item()], dtype=np.float32)
        out[pre + 'loss'] = np.array([crit(x, target).item()], dtype=np.float32)
    logger = lg.MetricLogger(delimiter='  ')
    for i, B in enumerate(ML_SIZES):
        if (B, ML_K) in GEOMS:
            x, target = torch.from_numpy(out[f'case/{B}x{ML_K}/x']), torch.from_numpy(out[f'case/{B}x{ML_K}/target'])
        else:
            x, target = batch(B, ML_K, 7000 + i)
            out[f'ml/x{i}'], out[f'ml/target{i}'] = x.numpy(), target.numpy()
        loss = crit(x, target)                                   # run_finetuning_cls.py:600-607
        acc1, acc5 = mt.accuracy(x, target, topk=(1, 5))
        logger.update(loss=loss.item())
        logger.meters['acc1'].update(acc1.item(), n=B)
        logger.meters['acc5'].update(acc5.item(), n=B)
    logger.synchronize_between_processes()
    out['ml/global_avg'] = np.array([logger.meters[k].global_avg for k in ('loss', 'acc1', 'acc5')], dtype=np.float64)
    path = os.path.join(HERE, 'cls_eval.npz')
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print('wrote cls_eval.npz with', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    for k in sorted(out):
        if k.endswith(('acc', 'loss', 'global_avg')):
            print(' ', k, out[k])


if __name__ == '__main__':
    main()
