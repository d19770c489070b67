"""Golden fixture for the dense regression losses and the NYU depth metrics (run_finetuning_depth.py:49-117) from the reference's own
functions on the CPU.  The four functions are taken out of the script with ``ast`` and only those FunctionDef nodes are executed, so
the script's imports (datasets, wandb, ...) are not needed; NYU_MEAN / NYU_STD come from utils/data_constants.py by file path.  Nothing
of the reference's text is stored: only seeded inputs and what its functions returned.

  loss/K{1,3}/...        a low-resolution map x [B, K, 5, 7], pred = F.interpolate(x, (13, 17), 'bilinear'), target, the masks, and per
                         kind (l1, mse, berhu) and mask pattern the loss and its gradient with respect to x
  metric/{case}/...      pred, target, mask and the seven metrics; case 'clamp' drives some targets below the 1e-6 clamp
  head/...               one step of the reference ConvNeXtAdapter(num_classes=1) at a tiny geometry with berHu and a block mask:
                         state dict, tokens, target, mask, prediction, loss, token gradient and every parameter's gradient

Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_reg_loss.py
"""
import ast
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402
from make_golden_convnext import input_info, perturb  # noqa: E402

KINDS = ('l1', 'mse', 'berhu')
B, LOW, SIZE = 2, (5, 7), (13, 17)
# the head step: (main tasks, mode, preds_per_patch, C, num_classes, depth, (NH, NW), D, B)
HEAD = (('rgb',), 'bilinear', 4, 8, 1, 1, (2, 3), 32, 2)


def reference_functions():
    """{name: function} of masked_{mse, l1, berhu}_loss and masked_nyu_metrics, compiled from their FunctionDef nodes alone"""
    spec = importlib.util.spec_from_file_location('ref_data_constants', os.path.join(REF, 'utils', 'data_constants.py'))
    dc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dc)
    path = os.path.join(REF, 'run_finetuning_depth.py')
    want = ('masked_mse_loss', 'masked_l1_loss', 'masked_berhu_loss', 'masked_nyu_metrics')
    nodes = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(n.name for n in nodes) == sorted(want)
    ns = {'torch': torch, 'NYU_MEAN': dc.NYU_MEAN, 'NYU_STD': dc.NYU_STD}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return {n: ns[n] for n in want}, dc.NYU_MEAN, dc.NYU_STD


def masks(K, Cm, H, W, g):
    """name -> torch.bool [B, Cm, H, W] or None.  Every non-empty pattern keeps at least 30 % of the elements."""
    rnd = torch.rand(B, Cm, H, W, generator=g) < 0.7
    block = torch.ones(B, Cm, H, W, dtype=torch.bool)
    block[:, :, H // 4:H // 2 + 1, 1:W // 2] = False
    image = torch.ones(B, Cm, H, W, dtype=torch.bool)
    image[B - 1] = False
    out = {'none': None, 'all': torch.ones(B, Cm, H, W, dtype=torch.bool), 'block': block, 'image': image, 'random': rnd,
           'empty': torch.zeros(B, Cm, H, W, dtype=torch.bool)}
    for n, m in out.items():
        assert m is None or n == 'empty' or float(m.float().mean()) >= 0.3, n
    return out


def loss_cases(fns, out):
    for K, cms in ((1, (1,)), (3, (1, 3))):
        g = torch.Generator().manual_seed(300 + K)
        x = torch.randn(B, K, *LOW, generator=g)
        target = torch.randn(B, K, *SIZE, generator=g)
        pre = f'loss/K{K}/'
        out[pre + 'x'], out[pre + 'target'] = x.numpy(), target.numpy()
        out[pre + 'pred'] = F.interpolate(x, size=SIZE, mode='bilinear', align_corners=False).numpy()
        for Cm in cms:
            for name, m in masks(K, Cm, *SIZE, g).items():
                if m is not None:
                    out[f'{pre}mask/c{Cm}/{name}'] = m.numpy()
                elif Cm != cms[0]:
                    continue
                for kind in KINDS:
                    xg = x.clone().requires_grad_(True)
                    pred = F.interpolate(xg, size=SIZE, mode='bilinear', align_corners=False)
                    loss = fns[f'masked_{kind}_loss'](pred, target.clone(), None if m is None else m.clone())
                    key = f'{pre}{kind}/c{Cm}/{name}/'
                    out[key + 'loss'] = np.array([loss.item()], dtype=np.float32)
                    if name != 'empty':
                        loss.backward()
                        out[key + 'dx'] = xg.grad.numpy()
                    else:
                        assert not np.isfinite(loss.item())             # 0 / 0


def metric_cases(fns, mean, std, out):
    H, W = SIZE
    g = torch.Generator().manual_seed(400)
    block = torch.ones(B, 1, H, W, dtype=torch.bool)
    block[:, :, 2:7, 3:11] = False
    image = torch.ones(B, 1, H, W, dtype=torch.bool)
    image[0] = False
    rnd = torch.rand(B, 1, H, W, generator=g) < 0.6
    for case, m in (('none', None), ('block', block), ('image', image), ('random', rnd), ('clamp', rnd)):
        pred = torch.rand(B, 1, H, W, generator=g) * 4 - 2
        target = (pred + torch.randn(B, 1, H, W, generator=g) * 0.8).clamp(-2, 2)
        if case == 'clamp':
            target.view(-1)[::9] = -2.9                        # target std + mean < 0: clamped to 1e-6 in the ratios and the log
            assert int(((target * std + mean) < 1e-6).sum()) > 10
        else:
            assert float((pred * std + mean).min()) > 0 and float((target * std + mean).min()) > 0
            assert float(pred.abs().max()) <= 2 and float(target.abs().max()) <= 2
        assert m is None or float(m.float().mean()) >= 0.3

        def near(th):
            p, t = pred.double() * std + mean, target.double() * std + mean
            r = torch.maximum(p / t.clamp_min(1e-6), t / p.clamp_min(1e-6))
            return (r - th).abs() / th < 2e-4
        for _ in range(20):                                     # move the few targets whose ratio sits on a threshold off it
            bad = near(1.25) | near(1.25 ** 2) | near(1.25 ** 3)
            if not bool(bad.any()):
                break
            target[bad] -= 0.01 * target[bad].sign()
        for th in (1.25, 1.25 ** 2, 1.25 ** 3):                 # a rounding difference cannot move a delta count
            assert not bool(near(th).any()), (case, th)
        res = fns['masked_nyu_metrics'](pred.clone(), target.clone(), None if m is None else m.clone())
        pre = f'metric/{case}/'
        out[pre + 'pred'], out[pre + 'target'] = pred.numpy(), target.numpy()
        if m is not None:
            out[pre + 'mask'] = m.numpy()
        out[pre + 'values'] = np.array([res[k].item() for k in ('rmse', 'rel', 'srel', 'log10', 'delta_1', 'delta_2', 'delta_3')],
                                       dtype=np.float32)
        assert np.isfinite(out[pre + 'values']).all()
    out['metric/mean_std'] = np.array([mean, std], dtype=np.float64)


def head_case(fns, roa, out):
    tasks, mode, p, C, K, depth, (NH, NW), D, Bh = HEAD
    torch.manual_seed(500)
    head = roa.ConvNeXtAdapter(num_classes=K, embed_dim=p * C, preds_per_patch=p, main_tasks=tasks, patch_size=16, depth=depth,
                               interpolate_mode=mode)
    head.init(dim_tokens_enc=D)
    perturb(head, 501)
    H, W = 16 * NH, 16 * NW
    g = torch.Generator().manual_seed(502)
    x = torch.randn(Bh, NH * NW + 1, D, generator=g, requires_grad=True)
    target = torch.randn(Bh, K, H, W, generator=g)
    mask = torch.ones(Bh, 1, H, W, dtype=torch.bool)
    mask[:, :, H // 4:H // 2 + 1, 1:W // 2] = False
    y = head(x, input_info(tasks, NH * NW, H, W))
    loss = fns['masked_berhu_loss'](y, target.clone(), mask.clone())
    loss.backward()
    for k, v in head.state_dict().items():
        out[f'head/sd/{k}'] = v.detach().clone().numpy()
    out['head/x'], out['head/target'], out['head/mask'] = x.detach().numpy(), target.numpy(), mask.numpy()
    out['head/y'], out['head/loss'], out['head/dx'] = y.detach().numpy(), np.array([loss.item()], dtype=np.float32), x.grad.numpy()
    for n, prm in head.named_parameters():
        out[f'head/grad/{n}'] = prm.grad.numpy()


def main():
    fns, mean, std = reference_functions()
    _, _, roa, _ = import_reference()
    out = {}
    loss_cases(fns, out)
    metric_cases(fns, mean, std, out)
    head_case(fns, roa, out)
    path = os.path.join(HERE, 'reg_loss.npz')
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print('wrote reg_loss.npz with', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
