"""Golden fixture for the fine-tuning param groups (dropin.amd_loop.create_optimizer_groups) from the reference's own factory:
utils/optim_factory.py's ``create_optimizer`` (module branch, ``get_parameter_groups``) with its ``LayerDecayValueAssigner``,
called the way run_finetuning_cls.py:369-390 calls it.  For every case the group list is recorded in order: the tensor names,
``weight_decay`` and ``lr_scale`` (null where the reference group has none).  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_param_groups.py
"""
import json
import os
import sys
import types

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, import_reference  # noqa: E402

# case -> (model, input domains, layer_decay, weight_decay, decoder_decay, no_lr_scale_list); 'synthetic' is SYNTH below
CASES = {
    'base_ld065': ('multivit_base', ('rgb',), 0.65, 0.05, None, None),
    'base_ld075_no_lr_scale': ('multivit_base', ('rgb',), 0.75, 0.05, None,
                               'global_tokens-input_adapters.rgb.proj.weight-output_adapters.cls.head.weight'),
    'rgb_depth_decoder_decay': ('multivit_base', ('rgb', 'depth'), 0.75, 0.05, 0.1, None),
    'base_ld1': ('multivit_base', ('rgb',), 1.0, 0.05, None, None),
    'base_wd0': ('multivit_base', ('rgb',), 0.65, 0.0, None, None),
    'large_ld075': ('multivit_large', ('rgb',), 0.75, 0.05, None, None),
    'synthetic_decoder_decay': ('synthetic', (), 0.65, 0.05, 0.1, 'decoder.head.weight'),
}


class Synth(nn.Module):
    """A module with ``decoder.*`` tensors, a ``decoder_weight_decay()`` list and a frozen tensor (tests/test_opt_groups_cpu.py
    builds the same names)."""

    def __init__(self):
        super().__init__()
        self.global_tokens = nn.Parameter(torch.zeros(1, 1, 8))
        self.encoder = nn.Sequential(*[nn.Sequential(nn.LayerNorm(8), nn.Linear(8, 8)) for _ in range(3)])
        self.decoder = nn.ModuleDict(dict(proj=nn.Linear(8, 8), norm=nn.LayerNorm(8), head=nn.Linear(8, 4)))
        self.extra = nn.Linear(8, 8)
        self.frozen = nn.Parameter(torch.zeros(8, 8), requires_grad=False)

    def get_num_layers(self):
        return 3

    def no_weight_decay(self):
        return {'global_tokens'}

    def decoder_weight_decay(self):
        return {'extra.weight'}


def build(rm, ria, roa, model, doms):
    if model == 'synthetic':
        return Synth()
    ins = {d: ria.PatchedInputAdapter(num_channels=3 if d == 'rgb' else 1, stride_level=1, patch_size_full=16, image_size=224)
           for d in doms}
    outs = {'cls': roa.LinearOutputAdapter(num_classes=1000, use_mean_pooling=True, init_scale=1.0)}
    return getattr(rm, model)(input_adapters=ins, output_adapters=outs, num_global_tokens=1)


def main():
    rm, ria, roa, _ = import_reference()
    sys.path.insert(0, REF)
    import utils.optim_factory as of
    sys.path.pop(0)
    out = {}
    for case, (model_name, doms, ld, wd, dec, nls) in CASES.items():
        torch.manual_seed(0)
        model = build(rm, ria, roa, model_name, doms)
        L = model.get_num_layers()
        assigner = of.LayerDecayValueAssigner(list(ld ** (L + 1 - i) for i in range(L + 2))) if ld < 1.0 else None
        args = types.SimpleNamespace(opt='adamw', lr=1e-3, weight_decay=wd, opt_eps=1e-8, opt_betas=None, momentum=0.9)
        if dec is not None:
            args.decoder_decay = dec
        if nls is not None:
            args.no_lr_scale_list = nls
        opt = of.create_optimizer(args, model, skip_list=model.no_weight_decay(),
                                  get_num_layer=assigner.get_layer_id if assigner is not None else None,
                                  get_layer_scale=assigner.get_scale if assigner is not None else None)
        name_of = {id(p): n for n, p in model.named_parameters()}
        out[case] = dict(model=model_name, domains=list(doms), layer_decay=ld, weight_decay=wd, decoder_decay=dec,
                         no_lr_scale_list=nls,
                         frozen=[n for n, p in model.named_parameters() if not p.requires_grad],
                         groups=[dict(names=[name_of[id(p)] for p in g['params']], weight_decay=g['weight_decay'],
                                      lr_scale=g.get('lr_scale')) for g in opt.param_groups])
        print(case, len(opt.param_groups), 'groups')
    with open(os.path.join(HERE, 'param_groups.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
