"""Golden fixture for ConvNeXtAdapter (output_adapters.py:481-573) from the reference's own classes on the CPU: seeded state dicts,
inputs, outputs, input and parameter gradients of the head alone (rgb / bilinear / depth 2 on a 4 x 5 patch grid; rgb-depth with
nearest; preds_per_patch 4 and 9), of a tiny MultiViT with the head, and one fine-tuning step of that model with
nn.CrossEntropyLoss(ignore_index=255) and the optimiser run_finetuning_semseg.py:450-468 builds (create_optimizer with a
LayerDecayValueAssigner).  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_convnext.py
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402

# case -> (main tasks, interpolate mode, preds_per_patch, C, num_classes, depth, (NH, NW), D, B); patch size 16, global token last
HEADS = {
    'head': (('rgb',), 'bilinear', 16, 16, 3, 2, (4, 5), 32, 1),
    'rgbd_nearest': (('rgb', 'depth'), 'nearest', 16, 16, 3, 1, (2, 3), 24, 2),
    'p4': (('rgb',), 'bilinear', 4, 24, 3, 1, (2, 3), 32, 1),
    'p9': (('rgb',), 'bilinear', 9, 16, 4, 1, (2, 3), 32, 1),
}
VIT = dict(D=16, depth=2, heads=2, K=4, E=256, p=16, head_depth=2, B=2, H=32, W=48)


def weight_like(y):
    """the fixed output weighting of the backward checks, sin(0.37 i) (recomputed by the tests instead of stored)"""
    return torch.sin(0.37 * torch.arange(y.numel(), dtype=torch.float64)).float().view(y.shape)


def perturb(m, seed):
    """non-zero biases / LayerNorm affine so that every parameter gradient path is exercised"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or 'norm' in n:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)


def input_info(tasks, N, H, W, G=1):
    info = {'tasks': {}, 'image_size': (H, W), 'num_task_tokens': N * len(tasks), 'num_global_tokens': G}
    for i, t in enumerate(tasks):
        info['tasks'][t] = {'num_tokens': N, 'has_2d_posemb': True, 'start_idx': i * N, 'end_idx': (i + 1) * N}
    return info


def head_cases(roa, out):
    for seed, (name, (tasks, mode, p, C, K, depth, (NH, NW), D, B)) in enumerate(HEADS.items()):
        torch.manual_seed(100 + seed)
        head = roa.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                                   interpolate_mode=mode)
        head.init(dim_tokens_enc=D)
        perturb(head, 200 + seed)
        N = NH * NW
        x = torch.randn(B, N * len(tasks) + 1, D, requires_grad=True)
        y = head(x, input_info(tasks, N, 16 * NH, 16 * NW))
        (y * weight_like(y)).sum().backward()
        for k, v in head.state_dict().items():
            out[f'{name}/sd/{k}'] = v.detach().clone().numpy()
        out[f'{name}/x'], out[f'{name}/y'], out[f'{name}/dx'] = x.detach().numpy(), y.detach().numpy(), x.grad.numpy()
        for n, prm in head.named_parameters():
            out[f'{name}/grad/{n}'] = prm.grad.numpy()


def build_vit(rm, ria, roa):
    torch.manual_seed(7)
    ins = {'rgb': ria.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=(VIT['H'], VIT['W']))}
    outs = {'semseg': roa.ConvNeXtAdapter(num_classes=VIT['K'], embed_dim=VIT['E'], preds_per_patch=VIT['p'], main_tasks=('rgb',),
                                          patch_size=16, depth=VIT['head_depth'])}
    return rm.MultiViT(input_adapters=ins, output_adapters=outs, num_global_tokens=1, dim_tokens=VIT['D'], depth=VIT['depth'],
                       num_heads=VIT['heads'])


def vit_cases(rm, ria, roa, out):
    sys.path.insert(0, REF)
    import utils.optim_factory as of
    sys.path.pop(0)
    model = build_vit(rm, ria, roa)
    for k, v in model.state_dict().items():
        out[f'vit/sd/{k}'] = v.detach().clone().numpy()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(VIT['B'], 3, VIT['H'], VIT['W'], generator=g, requires_grad=True)
    y = model({'rgb': x})['semseg']
    (y * weight_like(y)).sum().backward()
    out['vit/x'], out['vit/y'], out['vit/dx'] = x.detach().numpy(), y.detach().numpy(), x.grad.numpy()
    for n, prm in model.named_parameters():
        if prm.grad is not None:                             # the fixed sin-cos position embedding has none
            out[f'vit/grad/{n}'] = prm.grad.numpy()
    # one fine-tuning step (run_finetuning_semseg.py:450-468 builds the optimiser; the loop sets lr = schedule * lr_scale)
    model.zero_grad(set_to_none=True)
    L = model.get_num_layers()
    assigner = of.LayerDecayValueAssigner(list(0.75 ** (L + 1 - i) for i in range(L + 2)))
    args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, momentum=0.9)
    opt = of.create_optimizer(args, model, skip_list=model.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                              get_layer_scale=assigner.get_scale)
    for grp in opt.param_groups:
        grp['lr'] = args.lr * grp.get('lr_scale', 1.0)
    tgt = torch.randint(0, VIT['K'], (VIT['B'], VIT['H'], VIT['W']), generator=g).to(torch.int64)
    tgt[:, :5, :7] = 255                                       # ignored pixels
    xs = torch.randn(VIT['B'], 3, VIT['H'], VIT['W'], generator=g)
    loss = nn.CrossEntropyLoss(ignore_index=255)(model({'rgb': xs})['semseg'], tgt)
    loss.backward()
    opt.step()
    out['step/x'], out['step/target'], out['step/loss'] = xs.numpy(), tgt.numpy(), np.array([loss.item()], dtype=np.float32)
    for n, prm in model.named_parameters():
        out[f'step/param/{n}'] = prm.detach().clone().numpy()


def main():
    rm, ria, roa, _ = import_reference()
    out = {}
    head_cases(roa, out)
    vit_cases(rm, ria, roa, out)
    path = os.path.join(HERE, 'convnext_head.npz')
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print('wrote convnext_head.npz with', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
