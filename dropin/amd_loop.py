"""The three services of run_pretraining_multimae.py that keep the reference's loop host-bound on the MI355X engine, replaced by
the engine's own -- so that the UNMODIFIED ``train_one_epoch`` (run_pretraining_multimae.py:472-560) runs at the native step time.

Why: through the plain drop-in seam (``dropin/multimae``) the reference loop is functionally right but 25 % slower than the native
loop (profiles/r04_dropin_host_profile.txt: 38 ms of host work per 29 ms GPU step): 351 ``AccumulateGrad`` nodes + DDP's reducer
hooks (13.4 ms), the 345 ``torch.norm`` calls of ``get_grad_norm_`` (9.9 ms), DDP's pre-forward (5.8 ms), ``GradScaler.unscale_``
(1.8 ms).  All four are per-PARAMETER services; the engine's gradient arena makes each of them one pass / one call:

  reference (file:line)                                         here
  ------------------------------------------------------------  ---------------------------------------------------------------
  DistributedDataParallel(model, find_unused_parameters=True)    wrap_model(model, args): model.build_arena() (flat, gradient-
      run_pretraining_multimae.py:380-382                        readiness-ordered arenas), direct gradients, dist.GradAllReducer
                                                                 + dist.attach: buckets all-reduced over RCCL while backward runs
  create_optimizer(args, {'model': .., 'balancer': ..})          create_optimizer(args, model): optim.FusedAdamW -- the ONE group
      :389-390, utils/optim_factory.py:138-174                   the dict branch builds (weight decay on every trainable tensor);
                                                                 with ``--task_balancer uncertainty`` its two groups, the balancer's
                                                                 (lr_scale = balancer_lr_scale) outside the gradient norm and the clip
  UncertaintyWeightingStrategy(tasks=..) / NoWeightingStrategy   task_balancer(args): the engine's strategies -- the weighting and its
      :316-319, utils/task_balancing.py                          backward as one launch each, ``log_vars`` inside the parameter arena
  NativeScaler()  (GradScaler + unscale_ + get_grad_norm_)       LossScaler(): same call signature and return value (the gradient
      :391, utils/native_scaler.py:14-62                         2-norm); backward, reducer.finish(), ONE fused library call for
                                                                 norm + clip / skip + non-finite guard + AdamW.  bf16 needs no
                                                                 loss scale: state_dict() reports scale 1.0
  create_optimizer(args, model_without_ddp, skip_list=..,       create_optimizer_groups(args, model, ...): FusedAdamW(groups=..)
      get_num_layer=.., get_layer_scale=..)  (fine-tuning,       over the same param groups (no decay for biases / 1-D / skip list,
      run_finetuning_cls.py:386-389, utils/optim_factory.py:21)  layer-wise lr decay), still one fused library call per step
  Mixup(...), the criterion choice, ModelEma(...)                mixup(args), cls_criterion(args, mixup_fn), model_ema(model, args):
      run_finetuning_cls.py:299-306, :403-409, :344-352          the batch mixed in place in one launch, the soft-target loss as one
                                                                 autograd node, the EMA as one launch over two parameter arenas
  loss_scaler(..., update_grad=False)  (--update_freq > 1)       LossScaler: the backward of an accumulation micro-step runs inside
      run_finetuning_cls.py:528-531                              reducer.hold() -- gradients are exchanged once per update

The patch that wires them in is ``dropin/run_pretraining_multimae.patch`` (four call sites).  Everything else in the script --
argument parsing, cosine tables, the per-iteration ``param_group['lr']`` assignment (:474-480), ``train_one_epoch`` itself,
logging, ``utils.save_model`` -- stays the reference's.  ``tests/test_dropin_loop_gpu.py`` runs the loop body with these services at
the bench geometry against the native loop.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

import multimae_amd as M
from multimae_amd import dist as mdist
from multimae_amd.optim import FusedAdamW


def task_balancer(args) -> torch.nn.Module:
    """Replaces the balancer construction (run_pretraining_multimae.py:316-319): ``multimae_amd.UncertaintyWeightingStrategy`` over
    ``args.out_domains`` for ``--task_balancer uncertainty``, ``NoWeightingStrategy`` for ``none``."""
    kind = getattr(args, 'task_balancer', 'none')
    if kind == 'uncertainty':
        return M.UncertaintyWeightingStrategy(tasks=args.out_domains)
    if kind == 'none':
        return M.NoWeightingStrategy()
    raise ValueError(f'amd_loop.task_balancer: --task_balancer {kind!r} is not one of none, uncertainty')


def _trainable_balancer(balancer) -> bool:
    return balancer is not None and any(p.requires_grad for p in balancer.parameters())


def wrap_model(model: torch.nn.Module, args=None, bucket_mb: float = 64.0, balancer=None):
    """Replaces the DistributedDataParallel wraps (run_pretraining_multimae.py:380-387).  Returns ``(model, reducer)``: the model is
    NOT wrapped (``model_without_ddp is model``; checkpoints keep the reference's keys), the reducer is None outside
    torch.distributed.  Rank 0's parameters are broadcast as DDP's constructor does (the script seeds every rank differently, :300-302).
    ``balancer``: the loss balancer (already on the model's device); its trainable ``log_vars`` joins the END of the arena's trainable
    prefix, so the broadcast, the reducer's last bucket (its gradient is averaged over the ranks as under the script's second DDP
    wrap, :385-387) and the fused step cover it.  Neither ``state_dict()`` changes."""
    arena = model.build_arena(extra={'balancer': balancer}) if _trainable_balancer(balancer) else model.build_arena()
    M.engine.set_direct_grads(True)              # backward writes straight into the gradient arena: no AccumulateGrad per parameter
    on_gpu = arena.param.is_cuda                 # (a CPU dry run of the host logic has no streams)
    M.engine.set_adapter_streams(on_gpu)
    M.engine.set_wgrad_stream(on_gpu)
    reducer = None
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        mdist.broadcast_parameters(arena)
        reducer = mdist.GradAllReducer.for_arena(arena, bucket_mb=bucket_mb)
        reducer.gemm_cu_reserve = 16
    model._amd_reducer = reducer
    return model, reducer


def create_optimizer(args, model: torch.nn.Module, reducer=None, balancer=None) -> FusedAdamW:
    """Replaces utils.optim_factory.create_optimizer(args, {'model': model, 'balancer': balancer}) for the pre-training recipe
    (``--opt adamw``).  ``--task_balancer none``: the balancer group is empty (utils/optim_factory.py:138-155) -- the ONE group of
    every trainable tensor, whatever ``balancer`` is.  ``--task_balancer uncertainty``: the two groups of :139-150 -- the model's
    tensors with ``lr_scale`` 1, the balancer's with ``args.balancer_lr_scale``, both with ``args.weight_decay`` (``log_vars``
    decays too) -- the balancer's outside the gradient norm, the clip and the skip decision, as the loop's
    ``parameters=model.parameters()`` has it (run_pretraining_multimae.py:536-537); ``balancer`` must be the one
    ``wrap_model(..., balancer=...)`` put into the arena, otherwise ValueError."""
    _check_adamw_args(args)
    if getattr(args, 'task_balancer', 'none') == 'none':
        return _fused(args, model, reducer, args.weight_decay)
    if not _trainable_balancer(balancer):
        raise ValueError('amd_loop.create_optimizer: --task_balancer uncertainty needs the balancer whose log_vars the optimiser '
                         'steps: create_optimizer(args, model, reducer, balancer=loss_balancer)')
    arena = M.engine.arena_of(model)
    bal = [p for p in balancer.parameters() if p.requires_grad]
    if arena is None or not all(any(arena._params.get(n) is p for n in arena.extra_names) for p in bal):
        raise ValueError('amd_loop.create_optimizer: the balancer\'s parameters are not in the model\'s arena; call '
                         'wrap_model(model, args, balancer=loss_balancer) first')
    groups = [dict(params=[p for _, p in model.named_parameters() if p.requires_grad], lr_scale=1.),
              dict(params=bal, lr_scale=args.balancer_lr_scale)]
    return _fused(args, model, reducer, args.weight_decay, groups=groups, norm_exempt=bal)


def _check_adamw_args(args) -> None:
    if getattr(args, 'opt', 'adamw').lower().split('_')[-1] != 'adamw':
        raise ValueError('amd_loop.create_optimizer: the fused step is AdamW (--opt adamw); use the reference factory for other optimisers')
    if getattr(args, 'task_balancer', 'none') not in ('none', 'uncertainty'):
        raise ValueError(f'amd_loop.create_optimizer: --task_balancer {args.task_balancer!r} is not one of none, uncertainty')


def _fused(args, model, reducer, weight_decay, groups=None, norm_exempt=None) -> FusedAdamW:
    kw = dict(lr=args.lr, weight_decay=weight_decay)
    if getattr(args, 'opt_eps', None) is not None:
        kw['eps'] = args.opt_eps
    if getattr(args, 'opt_betas', None) is not None:
        kw['betas'] = tuple(args.opt_betas)
    if norm_exempt is not None:
        kw['norm_exempt'] = norm_exempt
    opt = FusedAdamW(model, groups=groups, **kw) if groups is not None else FusedAdamW(model, **kw)
    reducer = reducer if reducer is not None else getattr(model, '_amd_reducer', None)
    if reducer is not None:
        mdist.attach(model, reducer, opt)
    opt._amd_reducer = reducer
    return opt


def _group_rule(model: torch.nn.Module, weight_decay: float, skip_list, get_num_layer, get_layer_scale, decoder_decay, decoder_list,
                no_lr_scale_list) -> list:
    """One group per (layer id, decay class, lr-scale exemption), in the order the trainable tensors first open them.
      decay class   none: a 1-D tensor, a ``.bias`` or a name in ``skip_list``; else ``decoder_decay`` for a ``decoder.*`` name or
                    one in ``decoder_list`` when ``decoder_decay`` is given; else ``weight_decay``
      layer id      ``get_num_layer(name)`` (None without it); with it, a name in ``no_lr_scale_list`` gets a group of its own
      lr_scale      ``get_layer_scale(layer id)`` when given and the group is not exempt, else 1"""
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.ndim == 1 or name.endswith('.bias') or name in skip_list:
            cls, wd = 'no_decay', 0.
        elif decoder_decay is not None and (name.startswith('decoder.') or name in decoder_list):
            cls, wd = 'decoder_decay', decoder_decay
        else:
            cls, wd = 'decay', weight_decay
        layer = get_num_layer(name) if get_num_layer is not None else None
        exempt = get_num_layer is not None and name in no_lr_scale_list
        key = (layer, cls, exempt)
        if key not in groups:
            scale = get_layer_scale(layer) if get_layer_scale is not None and not exempt else 1.
            groups[key] = dict(weight_decay=wd, params=[], lr_scale=scale)
        groups[key]['params'].append(p)
    return list(groups.values())


def finetune_param_groups(args, model: torch.nn.Module, skip_list=None, get_num_layer=None, get_layer_scale=None,
                          filter_bias_and_bn: bool = True) -> list:
    """The param groups utils.optim_factory.create_optimizer(args, model, ...) gives a fine-tuning script (the rule of
    utils/optim_factory.py:51-101 and its caller :105-133): no weight decay for 1-D tensors, biases and the skip list (default
    ``model.no_weight_decay()``), ``args.decoder_decay`` on ``decoder.*`` and ``model.decoder_weight_decay()``, layer-wise lr
    scales, and the '-'-separated ``args.no_lr_scale_list`` exempt from them.  ``args.weight_decay == 0`` or
    ``filter_bias_and_bn=False``: one group of every trainable tensor with ``args.weight_decay``."""
    if not (args.weight_decay and filter_bias_and_bn):
        return [dict(params=[p for p in model.parameters() if p.requires_grad], weight_decay=args.weight_decay, lr_scale=1.)]
    if skip_list is None:
        skip_list = model.no_weight_decay() if hasattr(model, 'no_weight_decay') else ()
    decoder_list = model.decoder_weight_decay() if hasattr(model, 'decoder_weight_decay') else ()
    nls = getattr(args, 'no_lr_scale_list', None)
    return _group_rule(model, args.weight_decay, skip_list, get_num_layer, get_layer_scale, getattr(args, 'decoder_decay', None),
                       decoder_list, nls.split('-') if nls is not None else ())


def create_optimizer_groups(args, model: torch.nn.Module, skip_list=None, get_num_layer=None, get_layer_scale=None, reducer=None,
                            filter_bias_and_bn: bool = True) -> FusedAdamW:
    """Replaces utils.optim_factory.create_optimizer(args, model, skip_list=..., get_num_layer=..., get_layer_scale=...), the
    module branch every fine-tuning script builds its optimiser with (run_finetuning_cls.py:386-389; the same in _semseg, _depth
    and _taskonomy): FusedAdamW(groups=finetune_param_groups(...)), one fused library call per step.  The loop's
    ``g['lr'] = lr_schedule[it] * g['lr_scale']`` and ``g['weight_decay'] = wd_schedule[it]`` (where > 0) act on its groups
    unchanged (run_finetuning_cls.py:504-508)."""
    _check_adamw_args(args)
    groups = finetune_param_groups(args, model, skip_list, get_num_layer, get_layer_scale, filter_bias_and_bn)
    return _fused(args, model, reducer, 0., groups=groups)


class LossScaler:
    """``utils.NativeScalerWithGradNormCount`` for the engine: same ``__call__`` signature and return value.

    utils/native_scaler.py:20-40 is ``scale(loss).backward(); unscale_; norm = clip_grad_norm_ | get_grad_norm_ (skip if >= skip_grad);
    step; update`` -- clip and skip exclusive, clip first.  Here: ``loss.backward()`` (bf16 exponent range: no loss scale), the
    gradient exchange's ``finish()``, then ``FusedAdamW.step(loss)``: norm, the same clip / skip rule, the non-finite guards and
    AdamW in one library call with every decision on the device.  The returned norm is a device scalar (``metric_logger.update``
    reads it when it prints)."""
    state_dict_key = 'amp_scaler'

    def __init__(self, enabled: bool = True):
        self.enabled = enabled

    def __call__(self, loss, optimizer: FusedAdamW, clip_grad: Optional[float] = None, skip_grad: Optional[float] = None,
                 parameters=None, create_graph: bool = False, update_grad: bool = True):
        reducer = getattr(optimizer, '_amd_reducer', None)
        if not update_grad:
            # an accumulation micro-step (``--update_freq > 1``): the gradients stay local partial sums -- the reducer neither counts
            # readiness nor launches a bucket; FusedAdamW.zero_grad() / engine.claim_first_write make the next backward accumulate
            with (reducer.hold() if reducer is not None else contextlib.nullcontext()):
                loss.backward(create_graph=create_graph)
            return None
        loss.backward(create_graph=create_graph)
        if reducer is not None:
            reducer.finish()
        optimizer.clip_grad, optimizer.skip_grad = clip_grad, skip_grad
        return optimizer.step(loss)

    def state_dict(self):
        return {'scale': 1.0, 'growth_factor': 2.0, 'backoff_factor': 0.5, 'growth_interval': 2000, '_growth_tracker': 0}

    def load_state_dict(self, state_dict):
        pass


def staged_loader(data_loader, args, device=None):
    """Wraps the pre-training DataLoader (run_pretraining_multimae.py:472) in ``multimae_amd.StagedLoader``: it yields
    ``(x_on_device, target)`` with every batch copied on the stager's stream one step ahead, compact arrays
    (``dropin.amd_data.CompactAugmentation``) decoded on the device, and the depth standardised there when
    ``args.standardize_depth`` -- then pass ``standardize_depth=False`` to ``train_one_epoch``.  The loop's
    ``tensor.to(device, non_blocking=True)`` (:482-485) becomes a no-op."""
    from multimae_amd import staging
    default = getattr(args, 'imagenet_default_mean_and_std', True)
    mean = staging.IMAGENET_DEFAULT_MEAN if default else staging.IMAGENET_INCEPTION_MEAN
    std = staging.IMAGENET_DEFAULT_STD if default else staging.IMAGENET_INCEPTION_STD
    device = torch.device(device if device is not None else getattr(args, 'device', 'cuda'))
    stager = staging.BatchStager(device, mean, std,
                                 standardize_depth=(0.1, 0.9, 1e-6) if getattr(args, 'standardize_depth', False) else None)
    return staging.StagedLoader(data_loader, stager)


def seg_criterion(ignore_index: int = 255):
    """Replaces ``torch.nn.CrossEntropyLoss(ignore_index=utils.SEG_IGNORE_INDEX)`` (run_finetuning_semseg.py:483): the loss and its
    gradient from the ConvNeXt head's low-resolution logits, the full-resolution image neither written nor read."""
    from multimae_amd.criterion import SegCrossEntropyLoss
    return SegCrossEntropyLoss(ignore_index=ignore_index)


def seg_metric(num_classes: int, ignore_index: int = 255, device=None):
    """Replaces the host-side lists + ``compute_metrics_distributed`` of ``evaluate()`` (run_finetuning_semseg.py): call
    ``metric.update(seg_pred, seg_gt)`` per batch, then ``metric.sync()`` and ``all_acc, acc, iou = metric.compute()``."""
    from multimae_amd.metrics import SegMetric
    return SegMetric(num_classes, ignore_index, device)


def depth_criterion(loss_name: str = 'berhu'):
    """Replaces the ``tasks_loss_fn`` choice of run_finetuning_depth.py (``--loss l1 | berhu``; ``mse`` is offered as well):
    ``{'depth': fn}`` with the engine's masked loss, evaluated on the ConvNeXt head's low-resolution map without a host
    synchronisation (``--output_adapter convnext``)."""
    from multimae_amd import criterion
    fns = {'l1': criterion.masked_l1_loss, 'berhu': criterion.masked_berhu_loss, 'mse': criterion.masked_mse_loss}
    if loss_name not in fns:
        raise ValueError(f'depth_criterion: loss {loss_name!r} is not one of {sorted(fns)}')
    return {'depth': fns[loss_name]}


def taskonomy_criterion(tasks):
    """Replaces ``tasks_loss_fn = {task: masked_l1_loss for task in args.out_domains}`` of run_finetuning_taskonomy.py."""
    from multimae_amd.criterion import masked_l1_loss
    return {task: masked_l1_loss for task in tasks}


def depth_metric(device=None):
    """Replaces ``masked_nyu_metrics`` + ``metric_logger.update(**metrics)`` in the training loop and ``evaluate()`` of
    run_finetuning_depth.py: call ``metric.update(preds['depth'], target, mask_valid, loss=loss)`` per batch, then ``metric.sync()``
    and ``metric.compute()`` -- the only read-back -- for MetricLogger's ``global_avg`` of every value."""
    from multimae_amd.metrics import DepthMetric
    return DepthMetric(device)


def cls_metric(topk=(1, 5), device=None):
    """Replaces ``criterion`` + ``accuracy`` + the three ``.item()`` read-backs of ``evaluate()`` (run_finetuning_cls.py:582-613): call
    ``metric.update(output, target)`` per batch, then ``metric.sync()`` and ``metric.compute()`` -- the only read-back -- for
    MetricLogger's ``global_avg`` of ``loss``, ``acc1`` and ``acc5``.  The training loop's ``class_acc`` line (:541) is
    ``multimae_amd.cls_accuracy(output, targets)[0] / 100`` without its read-back."""
    from multimae_amd.metrics import ClsMetric
    return ClsMetric(topk, device)


def prepare_dense_inputs(input_dict: dict, tasks_dict: dict, standardize_depth: bool) -> dict:
    """Replaces the two blocks between the ``input_dict`` comprehension and the forward pass of run_finetuning_depth.py (:671-695
    in ``train_one_epoch``, :808-832 in ``evaluate``) and of run_finetuning_taskonomy.py (:645-668, :766-789), without a sort, a
    Python loop over device scalars or a boolean temporary -- no host synchronisation:

      - ``standardize_depth`` and ``'depth' in input_dict``: ``input_dict['depth']`` is REBOUND to
        ``robust_depth_standardize(input_dict['depth'], tasks_dict['mask_valid'])``, a new tensor that is already 0 where the mask
        is not set.  ``tasks_dict['depth']``, the loss target, was the same object and stays raw, as in the reference (:687).
      - every other non-rgb input is masked IN PLACE with ``mask_invalid_``, as in the reference (:691-695) -- and, as there, an
        input that was not standardised is the very tensor ``tasks_dict[task]`` holds, so the target of that task is masked with it.
      - an rgb-only ``input_dict`` (every shipped cfgs/finetune/{depth,taskonomy} config) makes no library call and no launch.

    Returns ``input_dict``."""
    from multimae_amd import data_ops
    done = None
    if standardize_depth and 'depth' in input_dict:
        input_dict['depth'] = data_ops.robust_depth_standardize(input_dict['depth'], tasks_dict['mask_valid'])
        done = 'depth'
    for task in input_dict:
        if task in ('rgb', done):
            continue
        data_ops.mask_invalid_(input_dict[task], tasks_dict['mask_valid'])
    return input_dict


def mixup(args):
    """Replaces the ``Mixup(...)`` construction of run_finetuning_cls.py:299-306: the engine's ``multimae_amd.Mixup`` from the same
    arguments, or None when ``--mixup``, ``--cutmix`` and ``--cutmix_minmax`` are all off."""
    active = args.mixup > 0 or args.cutmix > 0. or args.cutmix_minmax is not None
    if not active:
        return None
    return M.Mixup(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax, prob=args.mixup_prob,
                   switch_prob=args.mixup_switch_prob, mode=args.mixup_mode, label_smoothing=args.smoothing,
                   num_classes=args.nb_classes)


def random_erasing(args):
    """Replaces the ``RandomErasing(re_prob, mode=re_mode, max_count=re_count, num_splits=re_num_splits, device='cpu')`` that
    ``create_transform`` appends to the training transform (utils/transforms_factory.py:127-129) from ``--reprob / --remode /
    --recount``: the engine's ``multimae_amd.RandomErasing``, applied to the batch on the device, or None when ``--reprob`` is 0."""
    reprob = getattr(args, 'reprob', 0.)
    if not reprob or reprob <= 0.:
        return None
    return M.RandomErasing(probability=reprob, mode=getattr(args, 'remode', 'pixel'), max_count=getattr(args, 'recount', 1),
                           num_splits=0, device='cuda')


def rand_augment(args):
    """Replaces the ``rand_augment_transform(auto_augment, aa_params)`` that ``transforms_imagenet_train`` builds from ``--aa``,
    ``--input_size`` and ``--train_interpolation`` (utils/transforms_factory.py:86-99): the engine's ``multimae_amd.RandAugment``
    with the same ``aa_params``, applied to the uint8 batch on the device (hand it to ``cls_staged_loader``), or None when ``--aa``
    is off.  AutoAugment / AugMix configs raise ``NotImplementedError``: they stay on the host."""
    from multimae_amd import staging
    aa = getattr(args, 'aa', None)
    if not aa or str(aa).lower() == 'none':
        return None
    img_size = getattr(args, 'input_size', 224)
    img_size_min = min(img_size) if isinstance(img_size, (tuple, list)) else img_size
    default = getattr(args, 'imagenet_default_mean_and_std', True)
    mean = staging.IMAGENET_DEFAULT_MEAN if default else staging.IMAGENET_INCEPTION_MEAN
    aa_params = dict(translate_const=int(img_size_min * 0.45), img_mean=tuple([min(255, round(255 * x)) for x in mean]))
    interpolation = getattr(args, 'train_interpolation', 'bicubic')
    if interpolation and interpolation != 'random':
        # _pil_interp (utils/transforms.py): every name but bicubic / lanczos / hamming means bilinear
        aa_params['interpolation'] = interpolation if interpolation in ('bicubic', 'lanczos', 'hamming') else 'bilinear'
    return M.RandAugment(aa, aa_params)


def cls_staged_loader(data_loader, args, device=None, train=True, erase_float32=True, rand_augment=None):
    """Wraps a classification DataLoader in ``multimae_amd.ClsStagedLoader``: it yields ``(samples, targets)`` on the device, every
    batch copied on the stager's stream one step ahead.  With a transform that ends in the reference's prefetch form (``ToNumpy()``:
    uint8 (3, H, W)) the batch is copied as bytes and normalised -- and, for the training loader, erased per
    ``--reprob / --remode / --recount`` -- there in one launch.  float32 batches are copied as they are and, for the training loader,
    erased in place: that is right only when the host transform does NOT erase (``create_transform(..., re_prob=0.)``).  The
    UNCHANGED ``build_transform`` passes ``re_prob=args.reprob`` and so already ends in ``RandomErasing(device='cpu')``
    (utils/datasets.py:177, utils/transforms_factory.py:127-129): with it pass ``erase_float32=False``, which only moves the copy
    off the compute stream, or every sample is erased twice.  The loop's ``.to(device, non_blocking=True)``
    (run_finetuning_cls.py:510-511, :593-594) becomes a no-op.
    ``rand_augment``: the policy of ``rand_augment(args)``; the training loader's uint8 batches are then augmented on the device
    before they are normalised, and the host transform must be built with ``auto_augment=None, color_jitter=None``."""
    from multimae_amd import staging
    default = getattr(args, 'imagenet_default_mean_and_std', True)
    mean = staging.IMAGENET_DEFAULT_MEAN if default else staging.IMAGENET_INCEPTION_MEAN
    std = staging.IMAGENET_DEFAULT_STD if default else staging.IMAGENET_INCEPTION_STD
    device = torch.device(device if device is not None else getattr(args, 'device', 'cuda'))
    stager = staging.ClsStager(device, mean, std, random_erasing=random_erasing(args) if train else None, erase_float32=erase_float32,
                               rand_augment=rand_augment if train else None)
    return staging.ClsStagedLoader(data_loader, stager)


def cls_criterion(args, mixup_fn=None):
    """Replaces the criterion choice of run_finetuning_cls.py:403-409: soft targets under mixup (the smoothing is in the target),
    label smoothing without it, plain cross-entropy (``torch.nn.CrossEntropyLoss``, as the script) when both are off."""
    if mixup_fn is not None:
        return M.SoftTargetCrossEntropy()
    if args.smoothing > 0.:
        return M.LabelSmoothingCrossEntropy(smoothing=args.smoothing)
    return torch.nn.CrossEntropyLoss()


def model_ema(model: torch.nn.Module, args=None, decay: Optional[float] = None):
    """Replaces ``ModelEma(model, decay=args.model_ema_decay, device=..., resume='')`` (run_finetuning_cls.py:344-352): the engine's
    ``multimae_amd.ModelEma``, one launch per update.  ``--model_ema_force_cpu`` is not supported (NotImplementedError)."""
    if decay is None:
        decay = getattr(args, 'model_ema_decay', 0.9999)
    return M.ModelEma(model, decay=decay, device='cpu' if getattr(args, 'model_ema_force_cpu', False) else '', resume='')
