"""Golden fixture for the RefineNet pieces of the DPT head (output_adapter_utils.py:60-257) from the reference's own classes on the
CPU: the seeded parameters of make_scratch, and per case those of one ResidualConvUnit_custom and one FeatureFusionBlock_custom
(make_fusion_block) with inputs, outputs and all gradients -- the fusion block with one and with two inputs -- evaluated three times:
in f32, in f64 (the same parameters and inputs widened) and under torch.autocast(bfloat16) on the CPU.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fusion.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

# case -> (features, B, h, w): the fusion block's output is (B, features, 2h, 2w)
CASES = {'c8': (8, 2, 3, 4), 'c16': (16, 2, 3, 5)}
SCRATCH = dict(in_shape=[8, 16, 8, 16], out_shape=16, seed=300)
PRECISIONS = ('f32', 'f64', 'bf16')


def weight_like(y):
    """the fixed output weighting of the backward checks, sin(0.37 i) (recomputed by the tests instead of stored)"""
    return torch.sin(0.37 * torch.arange(y.numel(), dtype=torch.float64)).to(y.dtype).view(y.shape)


def case_seed(name):
    return 310 + 10 * list(CASES).index(name)


def case_inputs(name):
    f, B, h, w = CASES[name]
    g = torch.Generator().manual_seed(case_seed(name) + 5)
    return torch.randn(B, f, h, w, generator=g), torch.randn(B, f, h, w, generator=g)


def evaluate(module, xs, prec):
    """forward + backward of module(*xs) in one precision: (y, [dx], {name: grad}) as f32 (f64 for 'f64') numpy arrays"""
    m = copy.deepcopy(module)
    if prec == 'f64':
        m = m.double()
    m.zero_grad(set_to_none=True)
    xs = [(x.double() if prec == 'f64' else x.clone()).requires_grad_(True) for x in xs]
    if prec == 'bf16':
        with torch.autocast('cpu', dtype=torch.bfloat16):
            y = m(*xs)
    else:
        y = m(*xs)
    y = y.float() if prec == 'bf16' else y
    (y * weight_like(y)).sum().backward()
    grads = {n: p.grad.numpy() for n, p in m.named_parameters() if p.grad is not None}
    return y.detach().numpy(), [x.grad.numpy() for x in xs], grads


def record(out, key, module, xs):
    for prec in PRECISIONS:
        y, dxs, grads = evaluate(module, xs, prec)
        out[f'{key}/{prec}/y'] = y
        for i, d in enumerate(dxs):
            out[f'{key}/{prec}/dx{i}'] = d
        for n, g in grads.items():
            out[f'{key}/{prec}/grad/{n}'] = g


def main():
    import_reference()
    import multimae.output_adapter_utils as rou
    out = {}
    torch.manual_seed(SCRATCH['seed'])
    scratch = rou.make_scratch(SCRATCH['in_shape'], SCRATCH['out_shape'], groups=1, expand=False)
    for k, v in scratch.state_dict().items():
        out[f'scratch/sd/{k}'] = v.detach().clone().numpy()
    for name, (f, B, h, w) in CASES.items():
        x0, x1 = case_inputs(name)
        out[f'{name}/x0'], out[f'{name}/x1'] = x0.numpy(), x1.numpy()
        torch.manual_seed(case_seed(name))
        rcu = rou.ResidualConvUnit_custom(f, torch.nn.ReLU(False), False)
        torch.manual_seed(case_seed(name) + 1)
        ffb = rou.make_fusion_block(f, False)
        for k, v in rcu.state_dict().items():
            out[f'{name}/rcu/sd/{k}'] = v.detach().clone().numpy()
        for k, v in ffb.state_dict().items():
            out[f'{name}/ffb/sd/{k}'] = v.detach().clone().numpy()
        record(out, f'{name}/rcu', rcu, [x0])
        record(out, f'{name}/ffb1', ffb, [x0])
        record(out, f'{name}/ffb2', ffb, [x0, x1])
    path = os.path.join(HERE, 'fusion_blocks.npz')
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print('wrote fusion_blocks.npz with', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
