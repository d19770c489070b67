"""Records the kernel launches of a Python-composed autograd node stage by stage.

`record(names)` replaces the named functions of multimae_amd.ops for the duration of a `with` block (functions.py and GradSink call
everything as ops.<name>, so the module attributes are all there is to replace) and always puts them back.  Every OUTERMOST call is
stored as a Call:
  name    the ops function
  a       its arguments by parameter name (inspect.signature, defaults applied): a tensor becomes a TensorRec, a list or tuple that
          holds tensors (colsum_scatter's destinations) a list of TensorRec / None, anything else is kept as it is
  ret     the return value, recorded the same way
A TensorRec holds data_ptr / shape / stride / dtype, `before` and `after` -- clones of the tensor as the kernel sees it (a strided
view such as d_log[:, :K] is cloned through its strides) taken before and after the call, so `before` of an accumulate destination
is what it held -- and, for a 2-D view whose row stride exceeds its width, `rows_before` / `rows_after`: the full underlying rows
[rows, stride(0)] (the pad columns of the logits and their gradient).  `live` keeps the tensor itself: while the recording exists no
recorded buffer returns to the allocator, so within one recording equal data_ptr means the same buffer.

Nested calls: ops.linear_fwd / linear_dx / linear_dw find gemm and colsum in the same module namespace, so a wrapped gemm also fires
inside a wrapped linear_*.  A depth counter (one counter, not per thread: autograd runs the backward on its own thread, one call at a
time) lets only depth 0 record.

Stream order: every clone is enqueued on the stream that is current inside the call.  GradSink launches a weight gradient on the side
stream under `with torch.cuda.stream(side)` after side.wait_stream(main), so the wrapper runs with the side stream current: the
`before` clones are behind everything main had enqueued, the `after` clones behind the launch itself.  Leaving the block joins the
side streams (engine.join_wgrad_streams) and synchronises the device before anybody reads a clone from another stream."""
import contextlib
import copy
import inspect

import torch

from multimae_amd import engine, ops

# every ops function ConvNeXtHeadFn, GradSink and the fused segmentation loss launch
HEAD_OPS = ('convnext_rows_gather', 'convnext_rows_scatter', 'convnext_shuffle', 'linear_fwd', 'linear_dx', 'linear_dw', 'gemm', 'colsum',
            'colsum_scatter', 'reduce_partials', 'axpy_', 'cast', 'layernorm_fwd', 'layernorm_bwd_part', 'dwconv7_fwd', 'dwconv7_dgrad',
            'dwconv7_wgrad', 'resize_fwd', 'resize_bwd', 'seg_ce_fwd', 'seg_ce_bwd')


def _full_rows(t):
    """the underlying rows [rows, stride(0)], from the view's first element on, of a 2-D view narrower than its row stride (for a view
    that starts at column 0, such as d_log[:, :K], the whole padded rows); None where the storage ends before the last one does"""
    if t.dim() != 2 or t.shape[0] == 0 or t.stride(1) != 1 or t.stride(0) <= t.shape[1]:
        return None
    rows, ld = t.shape[0], t.stride(0)
    if (t.storage_offset() + rows * ld) * t.element_size() > t.untyped_storage().nbytes():
        return None
    return t.as_strided((rows, ld), (ld, 1))


class TensorRec:
    __slots__ = ('ptr', 'shape', 'stride', 'dtype', 'before', 'after', 'rows_before', 'rows_after', 'live')

    def __init__(self, t):
        t = t.detach()
        self.live = t
        self.ptr, self.shape, self.stride, self.dtype = t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype
        self.before = self.after = self.rows_before = self.rows_after = None

    def snap(self, when: str):
        rows = _full_rows(self.live)
        setattr(self, when, self.live.clone())
        setattr(self, 'rows_' + when, None if rows is None else rows.clone())

    def same_buffer(self, other) -> bool:
        return other is not None and self.ptr == other.ptr and self.dtype == other.dtype

    def __repr__(self):
        return f'<{str(self.dtype)[6:]} {list(self.shape)} stride {list(self.stride)} @{self.ptr:#x}>'


def _is_tensor_list(v):
    return isinstance(v, (list, tuple)) and len(v) > 0 and any(torch.is_tensor(e) for e in v) and all(e is None or torch.is_tensor(e) for e in v)


def _rec(v):
    if torch.is_tensor(v):
        return TensorRec(v)
    if _is_tensor_list(v):
        return [None if e is None else TensorRec(e) for e in v]
    return v


def _tensors(v):
    if isinstance(v, TensorRec):
        yield v
    elif isinstance(v, list):
        for e in v:
            if isinstance(e, TensorRec):
                yield e


class Call:
    def __init__(self, index, name, a):
        self.index, self.name, self.a, self.ret = index, name, a, None

    def tensors(self):
        for v in self.a.values():
            yield from _tensors(v)

    def replace(self, **a):
        """a shallow copy with some arguments replaced (for mis-wiring a copy of a recording)"""
        c = copy.copy(self)
        c.a = dict(self.a, **a)
        return c

    def __repr__(self):
        return f'#{self.index} {self.name}'


class Recording:
    def __init__(self):
        self.calls = []
        self._depth = 0

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapper(*args, **kwargs):
            if self._depth > 0:
                return fn(*args, **kwargs)
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            call = Call(len(self.calls), name, {k: _rec(v) for k, v in bound.arguments.items()})
            for t in call.tensors():
                t.snap('before')
            self.calls.append(call)
            self._depth += 1
            try:
                out = fn(*args, **kwargs)
            finally:
                self._depth -= 1
            for t in call.tensors():
                t.snap('after')
            call.ret = _rec(list(out) if isinstance(out, tuple) else out)
            for t in _tensors(call.ret):
                t.snap('after')
            return out
        wrapper.__wrapped__ = fn
        return wrapper

    def named(self, name):
        return [c for c in self.calls if c.name == name]


@contextlib.contextmanager
def record(names=HEAD_OPS, module=ops):
    rec = Recording()
    saved = {n: getattr(module, n) for n in names}
    try:
        for n, fn in saved.items():
            setattr(module, n, rec._wrap(n, fn))
        yield rec
    finally:
        for n, fn in saved.items():
            setattr(module, n, fn)
        engine.join_wgrad_streams()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
