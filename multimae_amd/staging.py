"""Batch staging: host batches copied on a dedicated stream and decoded on the device, one batch ahead of the step.

The reference loop moves each batch with ``tensor.to(device, non_blocking=True)`` on the compute stream
(run_pretraining_multimae.py:482-485), so the H2D copy of the 212 MB fp32 / int64 cfg3 batch (B = 256) runs in series with the
step.  ``BatchStager`` queues the copy on a stream of its own and, for the compact form the decoder produced before ``to_tensor``
(uint8 HWC rgb, uint16 / int32 depth, uint8 semseg: 65 MB), the conversions after it (csrc/ingest.hip), then records a ready
event; ``StagedLoader`` stages batch k + 1 before it hands out batch k, so that copy runs under step k.

Forms accepted per task (anything else raises ``ValueError``):

  task                  compact form (decoded on the device)       reference form (copied as it is)
  rgb                   uint8 (B, H, W, 3)                         float32 (B, 3, H, W)
  depth                 uint16 / int32 (B, H, W) or (B, 1, H, W)   float32 (B, 1, H, W)
  semseg, semseg_coco   uint8 (B, h, w)                            int64 (B, h, w)

Depth comes out as (B, 1, H, W) f32, standardised on the copy stream when ``standardize_depth=(lo, hi, eps)`` (in the decode
launch for the compact form); the training loop must then not standardise it again.

``ClsStager`` / ``ClsStagedLoader`` (end of the file) do the same for the ``(images, target)`` batches of classification
fine-tuning: uint8 (B, 3, H, W) images normalised and randomly erased by one launch on the copy stream (csrc/erase.hip), after
RandAugment on the bytes when a policy is given (csrc/randaug.hip).
"""
from __future__ import annotations

import collections
from typing import Dict, Optional

import torch

from . import data_ops

IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMAGENET_INCEPTION_MEAN, IMAGENET_INCEPTION_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)

_COMPACT = {'rgb': 'uint8 (B, H, W, 3)', 'depth': 'uint16 / int32 (B, H, W) or (B, 1, H, W)', 'semseg': 'uint8 (B, h, w)'}
_REFERENCE = {'rgb': 'float32 (B, 3, H, W)', 'depth': 'float32 (B, 1, H, W)', 'semseg': 'int64 (B, h, w)'}


def _kind(task: str) -> Optional[str]:
    return 'semseg' if task in ('semseg', 'semseg_coco') else task if task in ('rgb', 'depth') else None


def batch_form(task: str, t) -> str:
    """'compact' or 'reference' for one task's batch tensor; ``ValueError`` naming the task, shape and dtype otherwise."""
    k, s, d = _kind(task), tuple(t.shape), t.dtype
    compact = reference = False
    if k == 'rgb':
        compact = d == torch.uint8 and len(s) == 4 and s[3] == 3
        reference = d == torch.float32 and len(s) == 4 and s[1] == 3
    elif k == 'depth':
        compact = d in (torch.uint16, torch.int32) and (len(s) == 3 or (len(s) == 4 and s[1] == 1))
        reference = d == torch.float32 and len(s) == 4 and s[1] == 1
    elif k == 'semseg':
        compact = d == torch.uint8 and len(s) == 3
        reference = d == torch.int64 and len(s) == 3
    if k is not None and (compact or reference) and s[0] > 0 and all(v > 0 for v in s):
        return 'compact' if compact else 'reference'
    if k is None:
        raise ValueError(f'BatchStager: task {task!r} (shape {s}, dtype {d}) is not one of rgb, depth, semseg, semseg_coco')
    raise ValueError(f'BatchStager: task {task!r}: shape {s}, dtype {d} is neither the compact form ({_COMPACT[k]}) '
                     f'nor the reference form ({_REFERENCE[k]}), or is empty')


def batch_forms(batch: Dict[str, torch.Tensor]) -> Dict[str, str]:
    """``batch_form`` of every task, plus one batch size across the tasks."""
    if not isinstance(batch, dict) or not batch:
        raise ValueError(f'BatchStager: a batch is a non-empty dict task -> tensor, got {type(batch).__name__}')
    forms = {task: batch_form(task, t) for task, t in batch.items()}
    sizes = {task: int(t.shape[0]) for task, t in batch.items()}
    if len(set(sizes.values())) != 1:
        raise ValueError(f'BatchStager: the tasks disagree on the batch size: {sizes}')
    return forms


def _out_spec(task: str, t, form: str):
    """(shape, dtype) of the staged tensor"""
    if form == 'reference':
        return tuple(t.shape), t.dtype
    k = _kind(task)
    if k == 'rgb':
        B, H, W, _ = t.shape
        return (B, 3, H, W), torch.float32
    if k == 'depth':
        return (t.shape[0], 1, t.shape[-2], t.shape[-1]), torch.float32
    return tuple(t.shape), torch.int64


def _nbytes(shape, dtype) -> int:
    n = 1
    for v in shape:
        n *= int(v)
    return n * torch.empty((), dtype=dtype).element_size()


def bytes_per_batch(batch, standardize_depth: bool = False) -> Dict[str, int]:
    """Bytes one batch costs: ``h2d`` copied over PCIe, ``device`` in the staged tensors, ``hbm`` the decode / standardisation
    kernels read and write once (the selection passes of the standardisation re-read the map from L2, not counted).  ``batch``
    may hold meta tensors: only shapes and dtypes are read."""
    forms = batch_forms(batch)
    h2d = dev = hbm = 0
    for task, t in batch.items():
        inp = _nbytes(t.shape, t.dtype)
        out = _nbytes(*_out_spec(task, t, forms[task]))
        h2d += inp
        dev += out
        if forms[task] == 'compact':
            hbm += inp + out
        elif standardize_depth and _kind(task) == 'depth':
            hbm += 2 * out
    return {'h2d': h2d, 'device': dev, 'hbm': hbm}


class StagedBatch:
    """A batch queued on the stager's copy stream: ``tensors`` become valid for a stream once it has waited on ``event``
    (``BatchStager.get`` does both)."""
    __slots__ = ('tensors', 'event', 'owned')

    def __init__(self, tensors, event, owned):
        self.tensors, self.event, self.owned = tensors, event, owned


class BatchStager:
    """Copies host batches to ``device`` on one dedicated stream and decodes compact forms there (module docstring).

    Host side: pinned tensors (DataLoader ``pin_memory=True``) are copied from directly; pageable ones are first copied into one
    of two pinned slots the stager owns, and a slot is rewritten only after the event of its previous H2D has completed.  Every
    host tensor is referenced until its copy's event has completed.  Outputs come from torch's caching allocator (allocated on
    the copy stream, ``record_stream``-ed to the consumer by ``get``), so callers may keep them."""

    def __init__(self, device=None, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, standardize_depth=None):
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError(f'BatchStager: device {self.device} is not a GPU (the decode runs on HIP kernels only)')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if standardize_depth is not None:
            lo, hi, eps = standardize_depth
            standardize_depth = (float(lo), float(hi), float(eps))
        self.standardize_depth = standardize_depth
        self.stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self.stream):
            self.table = data_ops.rgb_table(mean, std).to(self.device)
        self.stream.synchronize()
        self._slots = [{}, {}]                     # task -> pinned uint8 buffer
        self._slot_event = [None, None]
        self._next_slot = 0
        self._held = collections.deque()           # (event, host tensors) until the event has completed

    def bytes_per_batch(self, batch) -> Dict[str, int]:
        return bytes_per_batch(batch, self.standardize_depth is not None)

    def _release(self):
        while self._held and self._held[0][0].query():
            self._held.popleft()

    def _pinned(self, slot: int, task: str, t: torch.Tensor) -> torch.Tensor:
        n = t.numel() * t.element_size()
        buf = self._slots[slot].get(task)
        if buf is None or buf.numel() < n:
            buf = self._slots[slot][task] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        dst = buf[:n].view(t.dtype).view(t.shape)
        dst.copy_(t)
        return dst

    def stage(self, batch: Dict[str, torch.Tensor], into: Optional[Dict[str, torch.Tensor]] = None,
              after: Optional[torch.cuda.Event] = None) -> StagedBatch:
        """Queue one batch.  ``into``: caller-owned static tensors (e.g. the inputs a ``graph.StepGraph`` replays on) to write
        instead of new ones; the copy stream first waits on ``after``, an event the caller recorded after its last use of them."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('BatchStager.stage: not allowed inside a graph capture (stage between replays, with into=)')
        forms = batch_forms(batch)
        specs = {task: _out_spec(task, t, forms[task]) for task, t in batch.items()}
        return self._queue('BatchStager', batch, forms, specs, into, after)

    def _queue(self, who: str, batch, forms, specs, into, after) -> StagedBatch:
        """The part of ``stage`` that does not depend on what a batch holds: ``specs`` is task -> (shape, dtype) of the staged
        tensor."""
        for task, t in batch.items():
            if t.is_cuda:
                raise ValueError(f'{who}: task {task!r} is already on {t.device}; the stager copies host batches')
        if into is not None:
            for task, t in batch.items():
                shape, dtype = specs[task]
                o = into.get(task)
                if o is None or tuple(o.shape) != shape or o.dtype != dtype or o.device != self.device or not o.is_contiguous():
                    raise ValueError(f'{who}: into[{task!r}] must be a contiguous {dtype} tensor of shape {shape} on {self.device}')
        self._release()
        host = {task: t.contiguous() for task, t in batch.items()}
        pageable = [task for task, t in host.items() if not t.is_pinned()]
        slot = None
        if pageable:
            slot, self._next_slot = self._next_slot, self._next_slot ^ 1
            if self._slot_event[slot] is not None:
                self._slot_event[slot].synchronize()          # the slot's previous H2D has completed
            for task in pageable:
                host[task] = self._pinned(slot, task, host[task])
        out, hold = {}, []                         # hold: further host tensors a subclass's _stage_one copies from
        with torch.cuda.stream(self.stream):
            if after is not None:
                self.stream.wait_event(after)
            for task, h in host.items():
                o = None if into is None else into[task]
                out[task] = self._stage_one(task, h, forms[task], o, hold)
            event = torch.cuda.Event()
            event.record(self.stream)
        if slot is not None:
            self._slot_event[slot] = event
        self._held.append((event, list(batch.values()) + list(host.values()) + hold))
        return StagedBatch(out, event, into is None)

    def _stage_one(self, task, h, form, o, hold):
        """Copy (and decode) one task's pinned host tensor ``h`` on the copy stream, into ``o`` when given.  A host tensor made here and
        copied from without blocking is appended to ``hold``: it is kept until the batch's event has completed."""
        kind = _kind(task)
        if form == 'reference':
            d = torch.empty(h.shape, dtype=h.dtype, device=self.device) if o is None else o
            d.copy_(h, non_blocking=True)
            if kind == 'depth' and self.standardize_depth is not None:
                data_ops.depth_standardize_(d, *self.standardize_depth)
            return d
        src = h.view(torch.int16) if h.dtype == torch.uint16 else h     # the copy moves bytes; uint16 has few kernels of its own in torch
        d = torch.empty(src.shape, dtype=src.dtype, device=self.device)
        d.copy_(src, non_blocking=True)
        if kind == 'rgb':
            return data_ops.ingest_rgb_u8(d, self.table, out=o)
        if kind == 'depth':
            d = d.view(h.dtype)
            return data_ops.ingest_depth(d, standardize=self.standardize_depth, out=o)
        return data_ops.ingest_semseg_u8(d, out=o)

    def get(self, staged: StagedBatch) -> Dict[str, torch.Tensor]:
        """The staged tensors, made safe to use on the current stream: it waits on the ready event, and each tensor the stager
        allocated is ``record_stream``-ed to it."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(staged.event)
        if staged.owned:
            for t in staged.tensors.values():
                t.record_stream(cur)
        return dict(staged.tensors)

    def __call__(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """stage + get: the copy still runs on the copy stream, but nothing overlaps it (StagedLoader prefetches)."""
        return self.get(self.stage(batch))


class StagedLoader:
    """Iterates ``iterable`` with prefetch depth 1: batch k + 1 is staged before batch k is handed out, so its copy runs under
    step k (also with a ``torch.cuda.synchronize()`` at the end of every step).  Items are a batch dict or a tuple / list whose
    first element is one (a DataLoader's ``(x, target)``); the rest passes through."""

    def __init__(self, iterable, stager: BatchStager):
        self.iterable, self.stager = iterable, stager

    def __len__(self):
        return len(self.iterable)

    def _stage(self, item):
        if isinstance(item, dict):
            return self.stager.stage(item), None
        if isinstance(item, (tuple, list)) and item and isinstance(item[0], dict):
            return self.stager.stage(item[0]), (type(item), item[1:])
        raise ValueError(f'StagedLoader: an item is a batch dict or a tuple (batch dict, ...), got {type(item).__name__}')

    def _get(self, staged):
        sb, rest = staged
        x = self.stager.get(sb)
        if rest is None:
            return x
        cls, tail = rest
        return (x, *tail) if cls is tuple else cls([x, *tail])

    def __iter__(self):
        it = iter(self.iterable)
        try:
            cur = self._stage(next(it))
        except StopIteration:
            return
        for item in it:
            nxt = self._stage(item)
            yield self._get(cur)
            cur = nxt
        yield self._get(cur)


# ------------------------------------------------------------------------------------------ classification fine-tuning --
# run_finetuning_cls.py moves (samples, targets) with ``.to(device, non_blocking=True)`` on the compute stream, the samples already
# normalised and erased on the host (ToTensor -> Normalize -> RandomErasing, utils/transforms_factory.py:117-129): 77 MB per batch
# of 128 at 224 x 224.  With the reference's own prefetch form (``create_transform(use_prefetcher=True)`` ends in ``ToNumpy()``:
# uint8 (3, H, W)) 19 MB cross PCIe, and one launch on the copy stream normalises and erases (csrc/erase.hip).

def cls_form(images) -> str:
    """'compact' (uint8 (B, 3, H, W), the prefetch form) or 'reference' (float32 (B, 3, H, W)); ``ValueError`` otherwise."""
    if torch.is_tensor(images):
        s, d = tuple(images.shape), images.dtype
        if len(s) == 4 and s[1] == 3 and all(v > 0 for v in s) and d in (torch.uint8, torch.float32):
            return 'compact' if d == torch.uint8 else 'reference'
        got = f'shape {s}, dtype {d}'
    else:
        got = type(images).__name__
    raise ValueError(f'ClsStager: images: {got} is neither the prefetch form (uint8 (B, 3, H, W)) nor the reference form '
                     f'(float32 (B, 3, H, W)), or is empty')


class ClsStager(BatchStager):
    """``BatchStager`` for the classification loop's ``(images, target)`` batches: same pinned slots, copy stream, held host
    tensors, ready event and ``into=`` / ``after=`` contract.

      images   uint8 (B, 3, H, W)    copied as bytes, then normalised and erased by one ``mmae_ingest_rgb_u8_chw_erase`` launch
               float32 (B, 3, H, W)  copied as it is, then erased in place when ``random_erasing`` is given and ``erase_float32``
      target   any tensor of B rows (labels), copied alongside

    ``random_erasing``: a ``multimae_amd.RandomErasing`` whose ``draw()`` is called once per staged batch, at stage time (so in the
    order the batches are staged); None (the evaluation loader) decodes only.
    ``erase_float32``: a float32 batch comes from a host transform that has already normalised it.  If that transform also ends in
    the reference's ``RandomErasing(device='cpu')`` -- ``create_transform`` appends it whenever ``re_prob > 0``
    (utils/transforms_factory.py:127-129) -- erasing here would erase every sample a second time: pass ``erase_float32=False`` then,
    and float32 batches are only copied (no table is drawn for them).  uint8 batches are erased either way.
    ``rand_augment``: a ``multimae_amd.RandAugment``; a uint8 batch is then augmented on the copy stream between the byte copy and the
    normalise-and-erase launch (``mmae_rand_augment_u8``), where the reference's transform has RandAugment.  Its table is drawn at
    stage time, before the erase table: the reference's order within a batch.  The host transform must then not augment
    (``auto_augment=None, color_jitter=None``).  A float32 batch is already normalised and cannot be augmented: ``ValueError``."""

    def __init__(self, device=None, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, random_erasing=None, erase_float32=True,
                 rand_augment=None):
        if rand_augment is not None and not (callable(getattr(rand_augment, 'draw', None)) and hasattr(rand_augment, 'num_layers')):
            raise ValueError(f'ClsStager: rand_augment must be a multimae_amd.RandAugment, got {type(rand_augment).__name__}')
        super().__init__(device, mean, std)
        self.random_erasing = random_erasing
        self.erase_float32 = bool(erase_float32)
        self.rand_augment = rand_augment

    def bytes_per_batch(self, batch) -> Dict[str, int]:
        images, target = self._pair(batch)
        inp, out = _nbytes(images.shape, images.dtype), _nbytes(images.shape, torch.float32)
        tgt = _nbytes(target.shape, target.dtype)
        compact = cls_form(images) == 'compact'
        return {'h2d': inp + tgt, 'device': out + tgt, 'hbm': inp + out if compact else 0}

    @staticmethod
    def _pair(item):
        if not (isinstance(item, (tuple, list)) and len(item) == 2):
            raise ValueError(f'ClsStager: a batch is an (images, target) pair, got {type(item).__name__}')
        images, target = item
        cls_form(images)
        if not torch.is_tensor(target) or target.dim() < 1 or target.shape[0] != images.shape[0]:
            got = f'shape {tuple(target.shape)}, dtype {target.dtype}' if torch.is_tensor(target) else type(target).__name__
            raise ValueError(f'ClsStager: target: {got} is not a tensor of {images.shape[0]} rows')
        return images, target

    def _accept(self, item):
        """``_pair`` plus what this stager's settings rule out"""
        images, target = self._pair(item)
        if self.rand_augment is not None and cls_form(images) != 'compact':
            raise ValueError('ClsStager: rand_augment is set and the images are float32: a normalised batch cannot be augmented '
                             '(hand over the uint8 prefetch form)')
        return images, target

    def stage(self, item, into=None, after: Optional[torch.cuda.Event] = None) -> StagedBatch:
        """Queue one ``(images, target)`` batch.  ``into``: a caller-owned ``(x, target)`` pair of static device tensors to write
        instead of new ones; the copy stream first waits on ``after`` (``BatchStager.stage``)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('ClsStager.stage: not allowed inside a graph capture (stage between replays, with into=)')
        images, target = self._accept(item)
        batch = {'images': images, 'target': target}
        forms = {'images': cls_form(images), 'target': 'reference'}
        specs = {'images': (tuple(images.shape), torch.float32), 'target': (tuple(target.shape), target.dtype)}
        if into is not None:
            if not (isinstance(into, (tuple, list)) and len(into) == 2):
                raise ValueError('ClsStager: into is an (x, target) pair of device tensors')
            into = {'images': into[0], 'target': into[1]}
        return self._queue('ClsStager', batch, forms, specs, into, after)

    def _table(self, shape, hold):
        """this batch's erase table on the device (drawn now, once the batch has been accepted), or None.  The host copy is pinned
        anew for every batch -- 35 KB at B = 128, served from torch's pinned-memory cache after the first -- and held until the
        batch's event has completed."""
        if self.random_erasing is None:
            return None
        return self._upload(self.random_erasing.draw(tuple(shape)), hold)

    def _upload(self, table, hold):
        """a table drawn on the host -> the device, from a pinned copy held until the batch's event has completed"""
        host = torch.from_numpy(table).pin_memory()
        hold.append(host)
        return host.to(self.device, non_blocking=True)

    def _stage_one(self, task, h, form, o, hold):
        if task == 'target' or form == 'reference':
            d = torch.empty(h.shape, dtype=h.dtype, device=self.device) if o is None else o
            d.copy_(h, non_blocking=True)
            if task == 'images' and self.random_erasing is not None and self.erase_float32:
                data_ops.random_erase_(d, self._table(h.shape, hold))
            return d
        d = torch.empty(h.shape, dtype=h.dtype, device=self.device)
        d.copy_(h, non_blocking=True)
        if self.rand_augment is not None and self.rand_augment.num_layers > 0:   # its table first, then the erase table
            d = data_ops.rand_augment_u8(d, self._upload(self.rand_augment.draw(tuple(h.shape)), hold),
                                         layers=self.rand_augment.num_layers)
        return data_ops.ingest_rgb_u8_chw(d, self.table, self._table(h.shape, hold), out=o)

    def get(self, staged: StagedBatch):
        """``(x, target)`` on the device, safe to use on the current stream (``BatchStager.get``)."""
        t = super().get(staged)
        return t['images'], t['target']


class ClsStagedLoader(StagedLoader):
    """``StagedLoader`` over a classification DataLoader's ``(images, target)`` batches: yields ``(x_on_device, target_on_device)``,
    batch k + 1 staged (copied, normalised, erased) under step k."""

    def __init__(self, iterable, stager: ClsStager):
        if not isinstance(stager, ClsStager):
            raise ValueError(f'ClsStagedLoader: the stager must be a ClsStager, got {type(stager).__name__}')
        super().__init__(iterable, stager)

    def _stage(self, item):
        return self.stager.stage(item)

    def _get(self, staged):
        return self.stager.get(staged)
