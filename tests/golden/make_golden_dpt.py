"""Golden fixture for DPTOutputAdapter (output_adapters.py:576-759, head_type='regression') from the reference's own class on the
CPU.  Two cases of the head alone -- seeded state_dict (biases perturbed so none is zero), the four hooked token tensors (one
trailing global-token row each), and from the f64 evaluation the output, the four token gradients and every parameter gradient
under the output weighting sin(0.37 i) -- plus, per tensor, the reference's own deviation from f64 when it evaluates in f32 and
under torch.autocast('cpu', bfloat16): max-abs difference over the f64 tensor's max-abs.  And one tiny MultiViT with the r1 head:
one forward + backward of masked_l1_loss (run_finetuning_depth.py:59-66): the prediction and the gradient of the patch projection,
recorded the same way.  One file per case, tests/golden/dpt_head_<case>.npz.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dpt.py [--emulate]

--emulate writes nothing: it evaluates the reference head of both cases once more on the CPU with the engine's rounding points in
place of autocast's -- convolution operands rounded to bf16, f32 accumulation, f32 maps and residual adds between the
convolutions, the output gradient rounded to bf16 once before each convolution's backward -- and prints, per tensor, that
evaluation's deviation from f64 beside the recorded autocast deviation (the reasoning behind the bf16 allowance of
tests/test_dpt_head_gpu.py).
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

GEOM = dict(hooks=[0, 1, 2, 3], layer_dims=[8, 16, 24, 32], feature_dim=16, patch_size=16, stride_level=1)
B = 2
# case -> (num_classes, main tasks, dim_tokens_enc, (N_H, N_W))
CASES = {'r1': (1, ('rgb',), 16, (2, 4)), 'r3': (3, ('rgb', 'depth'), 8, (4, 2))}
VIT = dict(D=16, depth=4, heads=2, H=32, W=64)
UNUSED = tuple(f'scratch.refinenet4.resConfUnit1.conv{c}.{p}' for c in (1, 2) for p in ('weight', 'bias'))


def weight_like(y):
    """the fixed output weighting of the backward checks, sin(0.37 i) (recomputed by the tests instead of stored)"""
    return torch.sin(0.37 * torch.arange(y.numel(), dtype=torch.float64)).to(y.dtype).view(y.shape)


def perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias'):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)


def input_info(tasks, N, H, W, G=1):
    info = {'tasks': {}, 'image_size': (H, W), 'num_task_tokens': N * len(tasks), 'num_global_tokens': G}
    for i, t in enumerate(tasks):
        info['tasks'][t] = {'num_tokens': N, 'has_2d_posemb': True, 'start_idx': i * N, 'end_idx': (i + 1) * N}
    return info


def case_seed(name):
    return 500 + 10 * list(CASES).index(name)


def build_head(roa, name):
    K, tasks, D, _ = CASES[name]
    torch.manual_seed(case_seed(name))
    head = roa.DPTOutputAdapter(num_classes=K, main_tasks=tasks, **GEOM)
    head.init(dim_tokens_enc=D)
    return head


def evaluate(run, module, xs, prec):
    """forward + backward of run(module, xs) in one precision: (y, [dx], {name: grad})"""
    m = copy.deepcopy(module)
    if prec == 'f64':
        m = m.double()
    m.zero_grad(set_to_none=True)
    xs = [(x.double() if prec == 'f64' else x.clone()).requires_grad_(True) for x in xs]
    if prec == 'bf16':
        with torch.autocast('cpu', dtype=torch.bfloat16):
            y, loss = run(m, xs)
    else:
        y, loss = run(m, xs)
    loss.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    return y.detach(), [x.grad for x in xs], grads


def record(out, key, run, module, xs, keep=None):
    """the f64 tensors in full (all, or those named in `keep`); per tensor the f32 and bf16 evaluations' deviation from them"""
    y, dxs, grads = evaluate(run, module, xs, 'f64')
    ref = {'y': y, **{f'dx{i}': d for i, d in enumerate(dxs)}, **{f'grad/{n}': g for n, g in grads.items()}}
    ref = {k: v for k, v in ref.items() if keep is None or k in keep}
    for k, v in ref.items():
        out[f'{key}/f64/{k}'] = v.numpy()
    for prec in ('f32', 'bf16'):
        y, dxs, grads = evaluate(run, module, xs, prec)
        got = {'y': y, **{f'dx{i}': d for i, d in enumerate(dxs)}, **{f'grad/{n}': g for n, g in grads.items()}}
        assert set(ref) <= set(got), sorted(set(ref) - set(got))
        for k, v in ref.items():
            dev = float((got[k].double() - v).abs().max() / v.abs().max())
            out[f'{key}/dev/{prec}/{k}'] = np.array(dev, dtype=np.float64)
    return ref


def head_cases(roa, out):
    for name, (K, tasks, D, (NH, NW)) in CASES.items():
        head = build_head(roa, name)
        perturb(head, case_seed(name) + 1)                           # (the tests repeat the seeded construction and this)
        for k, v in head.state_dict().items():
            out[f'{name}/sd/{k}'] = v.detach().clone().numpy()
        N = NH * NW
        g = torch.Generator().manual_seed(case_seed(name) + 2)
        toks = [torch.randn(B, N * len(tasks) + 1, D, generator=g) for _ in range(4)]
        for i, t in enumerate(toks):
            out[f'{name}/tok{i}'] = t.numpy()
        info = input_info(tasks, N, 16 * NH, 16 * NW)

        def run(m, xs):
            y = m(xs, info).float() if xs[0].dtype != torch.float64 else m(xs, info)
            return y, (y * weight_like(y)).sum()
        ref = record(out, name, run, head, toks)
        assert all(f'grad/{n}' not in ref for n in UNUSED)           # refinenet4 has one input: resConfUnit1 never runs
        assert all(float(ref[f'dx{i}'][:, -1].abs().max()) == 0.0 for i in range(4))     # the global-token row


def vit_case(rm, ria, roa, out):
    torch.manual_seed(7)
    ins = {'rgb': ria.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=(VIT['H'], VIT['W']))}
    outs = {'depth': roa.DPTOutputAdapter(num_classes=1, main_tasks=('rgb',), **GEOM)}
    model = rm.MultiViT(input_adapters=ins, output_adapters=outs, num_global_tokens=1, dim_tokens=VIT['D'], depth=VIT['depth'],
                        num_heads=VIT['heads'])
    perturb(model.output_adapters['depth'], 77)
    for k, v in model.state_dict().items():
        out[f'vit/sd/{k}'] = v.detach().clone().numpy()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 3, VIT['H'], VIT['W'], generator=g)
    target = torch.randn(B, 1, VIT['H'], VIT['W'], generator=g)
    mask = torch.rand(B, 1, VIT['H'], VIT['W'], generator=g) > 0.2
    out['vit/x'], out['vit/target'], out['vit/mask'] = x.numpy(), target.numpy(), mask.numpy()

    def run(m, xs):
        y = m({'rgb': xs[0]}, return_all_layers=True)['depth']
        y = y.float() if xs[0].dtype != torch.float64 else y
        d = (y - target.to(y.dtype)).abs()                           # masked_l1_loss (run_finetuning_depth.py:59-66)
        d = torch.where(mask, d, torch.zeros((), dtype=d.dtype))
        return y, d.sum() / mask.sum()
    # the prediction, and the one weight that receives gradient through all four hooks
    record(out, 'vit', run, model, [x], keep=('y', 'grad/input_adapters.rgb.proj.weight'))


def alias_of(key):
    """the state_dict lists act_N_postprocess and scratch.layerN_rn a second time under act_postprocess.{N-1} and
    scratch.layer_rn.{N-1}: the name such a key repeats, or None"""
    for pre, fmt in (('act_postprocess.', 'act_{}_postprocess.'), ('scratch.layer_rn.', 'scratch.layer{}_rn.')):
        if pre in key:
            head, rest = key.split(pre)
            i, tail = rest.split('.', 1)
            return head + fmt.format(int(i) + 1) + tail
    return None


def emulate(roa):
    import torch.nn.functional as F

    class RoundOperand(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.bfloat16().float()

        @staticmethod
        def backward(ctx, g):
            return g

    class RoundGradient(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            return g.bfloat16().float()

    plain = {'conv2d': F.conv2d, 'conv_transpose2d': F.conv_transpose2d}

    def wrap(fn):
        def conv(x, w, b=None, *a, **k):
            y = RoundGradient.apply(fn(RoundOperand.apply(x), RoundOperand.apply(w), None, *a, **k))
            return y if b is None else y + b.view(1, -1, 1, 1)                # the bias and its gradient stay f32
        return conv
    for name, (K, tasks, D, (NH, NW)) in CASES.items():
        z = np.load(os.path.join(HERE, f'dpt_head_{name}.npz'))
        head = build_head(roa, name)
        perturb(head, case_seed(name) + 1)
        toks = [torch.from_numpy(z[f'{name}/tok{i}']).requires_grad_(True) for i in range(4)]
        for k, fn in plain.items():
            setattr(F, k, wrap(fn))
        try:
            y = head(toks, input_info(tasks, NH * NW, 16 * NH, 16 * NW))
            (y * weight_like(y)).sum().backward()
        finally:
            for k, fn in plain.items():
                setattr(F, k, fn)
        mine = {'y': y.detach(), **{f'dx{i}': t.grad for i, t in enumerate(toks)},
                **{f'grad/{n}': p.grad for n, p in head.named_parameters() if p.grad is not None}}
        rows = []
        for k, v in mine.items():
            t64 = torch.from_numpy(z[f'{name}/f64/{k}'])
            e, ref = float((v.double() - t64).abs().max() / t64.abs().max()), float(z[f'{name}/dev/bf16/{k}'].reshape(-1)[0])
            rows.append((e / ref, k, e, ref))
        for ratio, k, e, ref in sorted(rows, reverse=True):
            print(f'{name} {k}: engine rounding points {e:.4f}, autocast {ref:.4f}, ratio {ratio:.2f}')


def main():
    rm, ria, roa, _ = import_reference()
    if '--emulate' in sys.argv[1:]:
        return emulate(roa)
    out = {}
    head_cases(roa, out)
    vit_case(rm, ria, roa, out)
    # one file per case (each within the size limit of a committed file): <case>/sd/<key> is stored once per tensor, <case>/keys
    # lists the state_dict's keys in order, repeated names included
    for case in (*CASES, 'vit'):
        part = {k: v for k, v in out.items() if k.startswith(case + '/')}
        keys = [k[len(case) + 4:] for k in part if k.startswith(case + '/sd/')]
        for k in keys:
            a = alias_of(k)
            if a is not None:
                assert np.array_equal(part[f'{case}/sd/{k}'], part[f'{case}/sd/{a}'])
                del part[f'{case}/sd/{k}']
        part[f'{case}/keys'] = np.array(keys)
        path = os.path.join(HERE, f'dpt_head_{case}.npz')
        np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in part.items()})
        print(f'wrote dpt_head_{case}.npz with', len(part), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
