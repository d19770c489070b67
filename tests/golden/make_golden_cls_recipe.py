"""Golden fixture for the classification fine-tuning recipe from the reference's own classes on the CPU: ``Mixup`` (utils/mixup.py),
``SoftTargetCrossEntropy`` / ``LabelSmoothingCrossEntropy`` (utils/cross_entropy.py), ``ModelEma`` (utils/model_ema.py) and one
``update_freq = 2`` step of run_finetuning_cls.py's loop.  The three utility files are loaded by file path, so that
``utils/__init__.py``'s other imports are not needed.

The reference's ``Mixup._params_per_elem`` uses ``np.bool``, which numpy >= 1.24 no longer has: this generator aliases
``np.bool = bool`` IN ITS OWN PROCESS (the alias it stood for) before it calls the class.

Groups of ``cls_recipe.npz``:
  mix/cases                  JSON: case name -> Mixup constructor arguments, in the order of the seeds (np.random.seed(1000 + index))
  mix/x, mix/labels          the input batch (6, 3, 16, 20) -- multiples of 1/4, which keeps the file small and still rounds in both
                             products and in the sum -- and the labels; every call mixes a fresh copy
  mix/<case>/out<c>, tgt<c>  the mixed batch and the soft target of call c = 0..3 (consecutive calls under the one seed)
  mix/<case>/rand            one np.random.rand() drawn after the four calls: the generator's position
  loss/<B>x<K>/...           logits x, dense target, labels, and for both criteria the loss and the gradient with respect to x
  ema/...                    a seeded tiny MultiViT (depth input) + LinearOutputAdapter: its state dict, and the reference ModelEma's state dict after
                             each of three update() calls towards the parameter sets ``perturbed(sd, k)`` (recomputed by the tests),
                             for decay 0.9 and 0.9999
  step/...                   update_freq = 2: two micro-batches through Mixup (batch mode, np.random.seed(77)) and
                             SoftTargetCrossEntropy, loss / 2 each, the layer-decay AdamW of run_finetuning_cls.py:386-389, one step.
                             The head's weights are multiplied by 1e-3 after construction (what the script's --init_scale 0.001
                             asks for; MultiViT's own initialisation walk overwrites the adapter's scaling).  That keeps the step
                             comparable: the key bias of attention has an exactly zero gradient, what a run computes for it is
                             rounding noise of about 2^-24 times the other gradients, and AdamW's first update g / (|g| + 1e-8)
                             turns noise near 1e-8 into a step of the size of the others.  With the small head the
                             encoder's gradients are ~1e-4 and that noise ~1e-11: three orders below eps.  STEP_K = 8 classes instead
                             of 7: the engine's bf16 products need leading dimensions that are multiples of 8, and the same
                             step must also run in bf16 mode.

Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cls_recipe.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402

K = 7
MIX_SHAPE = (6, 3, 16, 20)
VARIANTS = {
    'mixup': dict(mixup_alpha=0.8, cutmix_alpha=0.),
    'cutmix': dict(mixup_alpha=0., cutmix_alpha=1.0),
    'both': dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5),
    'minmax': dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8)),
    'prob': dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5),
}
LOSS_GEOMS = ((6, 7), (4, 1000), (3, 1001))
VIT = dict(D=16, depth=1, heads=2, P=8, S=16, B=4)
STEP_K = 8


def mix_cases():
    """case name -> constructor arguments; label smoothing alternates between 0.1 and 0 over the 15 cases"""
    cases = {}
    for mode in ('batch', 'pair', 'elem'):
        for name, kw in VARIANTS.items():
            cases[f'{mode}_{name}'] = dict(kw, mode=mode, num_classes=K, label_smoothing=0.1 if len(cases) % 2 == 0 else 0.0)
    return cases


def perturbed(t: torch.Tensor, k: int) -> torch.Tensor:
    """parameter set k of the EMA check: t + a multiple of 2^-16 in [-0.01, 0.01) from integer arithmetic (exact on every platform)"""
    i = torch.arange(t.numel(), dtype=torch.int64)
    r = ((i * 2654435761 + (k + 1) * 40503) % 65536).to(torch.float32) / 65536.0 - 0.5
    return t + (r * 0.02).view(t.shape)


def load_by_path(name):
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(REF, 'utils', name + '.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build_vit(rm, ria, roa, seed=5, dom='rgb', num_classes=K, init_scale=1.0):
    """the tiny classification model: one input domain ('rgb': 3 channels, 'depth': 1), a global token, a linear head"""
    torch.manual_seed(seed)
    ins = {dom: ria.PatchedInputAdapter(num_channels=3 if dom == 'rgb' else 1, stride_level=1, patch_size_full=VIT['P'],
                                        image_size=VIT['S'])}
    outs = {'cls': roa.LinearOutputAdapter(num_classes=num_classes, use_mean_pooling=True, init_scale=init_scale)}
    return rm.MultiViT(input_adapters=ins, output_adapters=outs, num_global_tokens=1, dim_tokens=VIT['D'], depth=VIT['depth'],
                       num_heads=VIT['heads'])


def mix_group(mx, out):
    g = torch.Generator().manual_seed(1)
    x0 = torch.randint(-4, 5, MIX_SHAPE, generator=g).float() / 4
    labels = torch.randint(0, K, (MIX_SHAPE[0],), generator=g)
    out['mix/x'], out['mix/labels'] = x0.numpy(), labels.numpy()
    cases = mix_cases()
    out['mix/cases'] = np.array(json.dumps(cases))
    for idx, (name, kw) in enumerate(cases.items()):
        fn = mx.Mixup(**kw)
        np.random.seed(1000 + idx)
        for c in range(4):
            xm, tg = fn(x0.clone(), labels)
            out[f'mix/{name}/out{c}'], out[f'mix/{name}/tgt{c}'] = xm.numpy(), tg.numpy()
        out[f'mix/{name}/rand'] = np.array([np.random.rand()])


def loss_group(mx, ce, out):
    for B, Kc in LOSS_GEOMS:
        g = torch.Generator().manual_seed(10 * B + Kc)
        labels = torch.randint(0, Kc, (B,), generator=g)
        target = mx.mixup_target(labels if B % 2 == 0 else torch.cat([labels, labels[:1]]), Kc, lam=0.3, smoothing=0.1, device='cpu')[:B]
        pre = f'loss/{B}x{Kc}/'
        out[pre + 'target'], out[pre + 'labels'] = target.numpy(), labels.numpy()
        x = (torch.randn(B, Kc, generator=g) * 2).requires_grad_(True)
        out[pre + 'x'] = x.detach().numpy()
        for tag, crit, t in (('soft', ce.SoftTargetCrossEntropy(), target), ('ls', ce.LabelSmoothingCrossEntropy(smoothing=0.1), labels)):
            x.grad = None
            loss = crit(x, t)
            loss.backward()
            out[pre + tag + '_loss'], out[pre + tag + '_dx'] = np.array([loss.item()], dtype=np.float32), x.grad.clone().numpy()


def ema_group(rm, ria, roa, me, out):
    model = build_vit(rm, ria, roa, dom='depth')                 # one input channel: a third of the patch projection
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, v in sd0.items():
        out[f'ema/sd/{k}'] = v.numpy()
    for decay in (0.9, 0.9999):
        model.load_state_dict(sd0)
        ema = me.ModelEma(model, decay=decay)
        for step in range(3):
            model.load_state_dict({k: perturbed(v, step) for k, v in sd0.items()})
            ema.update(model)
            for k, v in ema.ema.state_dict().items():
                out[f'ema/{decay}/{step}/{k}'] = v.detach().clone().numpy()


def step_group(rm, ria, roa, mx, ce, out):
    sys.path.insert(0, REF)
    import utils.optim_factory as of
    sys.path.pop(0)
    model = build_vit(rm, ria, roa, seed=6, num_classes=STEP_K, init_scale=0.001)
    with torch.no_grad():
        model.output_adapters['cls'].head.weight.mul_(1e-3)           # see the module docstring
    for k, v in model.state_dict().items():
        out[f'step/sd/{k}'] = v.detach().clone().numpy()
    L = model.get_num_layers()
    assigner = of.LayerDecayValueAssigner(list(0.75 ** (L + 1 - i) for i in range(L + 2)))
    args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None, momentum=0.9)
    opt = of.create_optimizer(args, model, skip_list=model.no_weight_decay(), get_num_layer=assigner.get_layer_id,
                              get_layer_scale=assigner.get_scale)
    for grp in opt.param_groups:
        grp['lr'] = args.lr * grp.get('lr_scale', 1.0)
    mix = mx.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                   label_smoothing=0.1, num_classes=STEP_K)
    crit = ce.SoftTargetCrossEntropy()
    g = torch.Generator().manual_seed(12)
    np.random.seed(77)
    opt.zero_grad()
    for m in range(2):
        x = torch.randn(VIT['B'], 3, VIT['S'], VIT['S'], generator=g)
        y = torch.randint(0, STEP_K, (VIT['B'],), generator=g)
        out[f'step/x{m}'], out[f'step/y{m}'] = x.numpy().copy(), y.numpy()
        xs, ts = mix(x.clone(), y)
        loss = crit(model({'rgb': xs})['cls'], ts)
        (loss / 2).backward()
        out[f'step/loss{m}'] = np.array([loss.item()], dtype=np.float32)
    for n, p in model.named_parameters():
        if p.grad is not None:
            out[f'step/grad/{n}'] = p.grad.clone().numpy()
    opt.step()
    for n, p in model.named_parameters():
        out[f'step/param/{n}'] = p.detach().clone().numpy()


def main():
    if not hasattr(np, 'bool'):
        np.bool = bool                                           # see the module docstring
    rm, ria, roa, _ = import_reference()
    mx, ce, me = load_by_path('mixup'), load_by_path('cross_entropy'), load_by_path('model_ema')
    out = {}
    mix_group(mx, out)
    loss_group(mx, ce, out)
    ema_group(rm, ria, roa, me, out)
    step_group(rm, ria, roa, mx, ce, out)
    path = os.path.join(HERE, 'cls_recipe.npz')
    np.savez_compressed(path, **{k: np.ascontiguousarray(v) for k, v in out.items()})
    print('wrote cls_recipe.npz with', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
