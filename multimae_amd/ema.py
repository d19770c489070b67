"""Exponential moving average of the model's weights (mirror of the reference's ``utils/model_ema.py`` ``ModelEma``) on the engine's
flat parameter arena.

Reference: ModelEma utils/model_ema.py:18-83 walks two ``state_dict()``s and issues ``ema_v * decay + (1 - decay) * model_v`` plus a
``copy_`` per tensor -- four eager kernels for each of ViT-B's ~150 tensors, every step.  The engine keeps every parameter of a model
in ONE flat fp32 array (``engine.ParamArena.param``), so here the EMA model gets an arena of the same layout and ``update()`` is one
``mmae_ema_update`` launch over the two arrays (csrc/clsrecipe.hip), bit-identical to the reference per element: the factors are
``f32(decay)`` and ``f32(1. - decay)`` (the difference in double), each product and the sum rounded on its own.  The alignment
padding between tensors is zero in both arenas and stays zero.

Like the reference, the average covers ``state_dict()``: for the engine's models that is the parameters (there are no buffers).
Not provided: ``device='cpu'`` (the average lives beside the model) and ``resume=`` (load ``state_dict_ema`` into ``.ema`` with
``load_state_dict``) -- both raise NotImplementedError.
"""
from __future__ import annotations

import copy

import torch

from . import engine, ops


class ModelEma:
    """``utils.ModelEma(model, decay)``: ``.ema`` is a copy of the model in ``eval()`` without gradients, ``update(model)`` moves it
    towards the model's current weights, ``.ema.state_dict()`` is what the fine-tuning script stores as ``state_dict_ema``.
    ``shadow=True`` also writes the EMA arena's bf16 shadow in the update's launch, so that a bf16 forward of ``.ema`` needs no cast."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, device='', resume='', shadow: bool = False):
        if device:
            raise NotImplementedError('ModelEma: device= is not supported -- the average is kept on the model\'s device, in an arena '
                                      'laid out like the model\'s')
        if resume:
            raise NotImplementedError('ModelEma: resume= is not supported -- load the checkpoint\'s state_dict_ema into .ema with '
                                      'load_state_dict()')
        src = model.build_arena()
        # the copy takes the parameters' values and requires_grad flags; the engine state hanging off the model (its arena, a gradient
        # reducer and the callback bound to it) stays with the model
        memo = {id(src): None}
        for attr in ('_amd_reducer', '_grad_ready_cb'):
            if getattr(model, attr, None) is not None:
                memo[id(getattr(model, attr))] = None
        self.ema = copy.deepcopy(model, memo)
        self.ema.eval()
        self.decay = decay
        self.shadow = bool(shadow)
        self._arena = self.ema.build_arena()              # laid out while the flags are still the model's: same order, same offsets
        for p in self.ema.parameters():
            p.requires_grad_(False)
            p.grad = None
        self._arena.grad = self._arena.grad.new_empty(0)  # no gradients
        self._check_layout(src)

    def _check_layout(self, src) -> None:
        a = self._arena
        if src is None or src.numel != a.numel or src.names != a.names or src.offsets != a.offsets:
            raise RuntimeError('ModelEma: the model\'s parameter arena is no longer laid out like the EMA copy\'s (a parameter was added, '
                               'frozen or re-materialised after ModelEma was built); build a new ModelEma')

    @torch.no_grad()
    def update(self, model: torch.nn.Module) -> None:
        src = engine.arena_of(getattr(model, 'module', model))
        self._check_layout(src)
        a = self._arena
        sh = None
        if self.shadow:
            if a.shadow is None:
                a.shadow = torch.empty(a.numel, device=a.device, dtype=torch.bfloat16)
            sh = a.shadow
        ops.ema_update(a.param, src.param, self.decay, sh)
        a._shadow_token = False                           # the parameters moved: a shadow cast earlier is stale ...
        if sh is not None:
            a.mark_shadow_fresh()                         # ... unless this launch wrote it
