"""Task-loss balancers of the pre-training loop (utils/task_balancing.py): same class names, constructors, attributes and
state dicts as the reference, so ``--task_balancer`` and the ``'loss_balancer'`` entry of a checkpoint (utils/checkpoint.py:89-90)
carry over.  ``UncertaintyWeightingStrategy.forward`` is one autograd node over the T scalar task losses and ``log_vars``
(functions.TaskBalanceFn, csrc/balance.hip: one launch forward, one backward) instead of torch's eight-kernel chain and its
backward; on CPU tensors it is the reference's torch formula (the dry-run harness and the drop-in CPU run)."""
from __future__ import annotations

import torch
from torch import nn

from . import functions, ops


class NoWeightingStrategy(nn.Module):
    """``--task_balancer none``: the task losses as they are (utils/task_balancing.py:11-19)."""

    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, task_losses):
        return task_losses


class UncertaintyWeightingStrategy(nn.Module):
    """``--task_balancer uncertainty`` (utils/task_balancing.py:21-44): ``w_i = (exp(-s_i) * L_i + s_i) * (L_i != 0)`` with the
    trainable ``log_vars`` s (zeros at init), returned under the keys of ``task_losses``.

    Which task ``log_vars[i]`` belongs to: as in the reference, the i-th loss of ``task_losses`` in the dict's own order -- nothing
    is matched by name.  The engine's model returns ``preds`` (hence the losses) in ``output_adapters`` order whatever
    ``fp32_output_adapters`` is, so here slot i is always the i-th output adapter.  The reference's forward moves the
    ``fp32_output_adapters`` predictions to the END of ``preds`` (multimae/multimae.py:357-377): a reference run with an fp32 adapter
    that is not already the last output (e.g. ``--extra_norm_pix_loss`` adds ``norm_rgb`` behind an fp32 ``semseg``) trained its slots
    in that moved order, and its ``'loss_balancer'`` checkpoint entry, though it loads strictly, must be permuted to the adapters' order
    first.  The shipped rgb-depth-semseg recipe with fp32 ``semseg`` is unaffected: semseg is the last output either way."""

    def __init__(self, tasks):
        super().__init__()
        if len(tasks) > ops.BALANCE_MAX_TASKS:
            raise ValueError(f'UncertaintyWeightingStrategy: {len(tasks)} tasks, at most {ops.BALANCE_MAX_TASKS} are supported')
        self.tasks = tasks
        self.log_vars = nn.Parameter(torch.zeros(len(tasks)))

    def forward(self, task_losses):
        losses = list(task_losses.values())
        if len(losses) != self.log_vars.numel():
            raise ValueError(f'UncertaintyWeightingStrategy: {len(losses)} task losses ({list(task_losses)}) for '
                             f'{self.log_vars.numel()} log_vars (tasks {list(self.tasks)})')
        if not self.log_vars.is_cuda:
            stacked = torch.stack(losses)
            mask = stacked != 0.0
            weighted = (torch.exp(-self.log_vars) * stacked + self.log_vars) * mask
        else:
            weighted = functions.TaskBalanceFn.apply(
                self.log_vars, *[l if l.dtype == torch.float32 and l.dim() == 0 else l.float().reshape(()) for l in losses])
        out = task_losses.copy()
        out.update(zip(out, weighted))
        return out
