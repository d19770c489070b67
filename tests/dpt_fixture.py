"""What the DPT head's CPU and GPU tests share: the fixture files of tests/golden/make_golden_dpt.py (one per case), the state_dict
with its repeated names restored, and the engine twin of a case's seeded head."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
from make_golden_dpt import B, CASES, GEOM, UNUSED, VIT, alias_of, case_seed, input_info, perturb, weight_like  # noqa: E402,F401

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = np.load(os.path.join(ROOT, 'tests', 'golden', f'dpt_head_{case}.npz'))
    return _GOLD[case]


def gold_sd(case):
    """the reference's state_dict of a case, every key in the reference's order (a repeated name reads the tensor it repeats)"""
    z = gold(case)
    sd = {}
    for k in z[f'{case}/keys'].tolist():
        sd[k] = torch.from_numpy(z[f'{case}/sd/{alias_of(k) or k}'])
    return sd


def tensors(case, kind='f64'):
    """{'y', 'dx0'.., 'grad/<param>'}: the f64 tensors, or (kind 'dev/f32' | 'dev/bf16') the reference's own deviation per tensor"""
    z = gold(case)
    pre = f'{case}/{kind}/'
    return {k[len(pre):]: (torch.from_numpy(z[k]) if kind == 'f64' else float(z[k].reshape(-1)[0])) for k in z.files if k.startswith(pre)}


def tokens(case):
    z = gold(case)
    return [torch.from_numpy(z[f'{case}/tok{i}']) for i in range(4)]


def case_info(case):
    K, tasks, D, (NH, NW) = CASES[case]
    return input_info(tasks, NH * NW, 16 * NH, 16 * NW)


def seeded_head(case):
    """the engine's head built as the fixture builds the reference's: same seed, init(), the same bias perturbation"""
    from multimae_amd.output_adapters import DPTOutputAdapter
    K, tasks, D, _ = CASES[case]
    torch.manual_seed(case_seed(case))
    head = DPTOutputAdapter(num_classes=K, main_tasks=tasks, **GEOM)
    head.init(dim_tokens_enc=D)
    perturb(head, case_seed(case) + 1)
    return head
