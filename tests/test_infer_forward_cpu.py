"""CPU: which route EncoderStackFn.forward takes -- ops.stack_fwd_infer (nothing to differentiate, switch on, no stochastic depth, no
dropout sites, no MX products, stack composites available) or exactly what it ran before -- the engine switch, and one no-grad MultiViT
forward through the type-checking stub of the C ABI (dryrun_harness serves new prototypes of include/mmae.h as they are declared)."""
import ctypes

import pytest
import torch

import multimae_amd as M
from multimae_amd import engine, ops
from multimae_amd.functions import EncoderStackFn, _Cfg

L, B, N, D, HEADS = 3, 2, 5, 64, 2


@pytest.fixture()
def stubbed():
    from multimae_amd import _lib
    import dryrun_harness
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    prev = engine.inference_forward()
    dryrun_harness.install()
    yield
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    ops._WS.clear()
    ops.set_composite_blocks(True)
    ops.set_stack_composites(True)
    engine.set_inference_forward(prev)


def _params(d=D, requires_grad=True):
    shapes = [(d,), (d,), (3 * d, d), (3 * d,), (d, d), (d,), (d,), (d,), (4 * d, d), (4 * d,), (d, 4 * d), (d,)]
    return [torch.zeros(s, requires_grad=requires_grad) for _ in range(L) for s in shapes]


def _cfg(all_layers=False, heads=HEADS, **kw):
    return _Cfg(act=torch.bfloat16, wc=lambda w: w.detach().to(torch.bfloat16), heads=heads, eps=1e-6, all_layers=all_layers,
                on_layer_done=None, **kw)


@pytest.fixture()
def recorders(stubbed, monkeypatch):
    calls = []

    def fake_fwd(x, params, wc, heads, eps, act, B_, N_, dp=None, mx=False):
        calls.append(('fwd', dict(dp=dp, mx=mx)))
        return [torch.zeros_like(x) for _ in range(len(params) // 12)], object()

    def fake_infer(x, params, wc, heads, eps, act, B_, N_, keep='last'):
        calls.append(('infer', dict(keep=keep)))
        n = len(params) // 12 if keep == 'all_layers' else 1
        return [torch.zeros_like(x) for _ in range(n)]

    monkeypatch.setattr(ops, 'stack_fwd', fake_fwd)
    monkeypatch.setattr(ops, 'stack_fwd_infer', fake_infer)
    return calls


def _names(calls):
    return [c[0] for c in calls]


@pytest.mark.parametrize('all_layers', [False, True])
def test_no_grad_takes_the_inference_forward(recorders, all_layers):
    x = torch.randn(B, N, D)
    with torch.no_grad():
        y = EncoderStackFn.apply(_cfg(all_layers), x, *_params())
    assert recorders == [('infer', dict(keep='all_layers' if all_layers else 'last'))]
    ys = list(y) if all_layers else [y]
    assert len(ys) == (L if all_layers else 1) and all(t.shape == (B, N, D) and not t.requires_grad for t in ys)


def test_frozen_everything_counts_as_nothing_to_differentiate(recorders):
    """gradients enabled but no input wants one (a frozen encoder fed constant tokens): the same route"""
    EncoderStackFn.apply(_cfg(), torch.randn(B, N, D), *_params(requires_grad=False))
    assert _names(recorders) == ['infer']


@pytest.mark.parametrize('switch', [True, False])
def test_with_gradients_the_training_forward_whatever_the_switch_says(recorders, switch):
    engine.set_inference_forward(switch)
    y = EncoderStackFn.apply(_cfg(), torch.randn(B, N, D), *_params())
    assert _names(recorders) == ['fwd'] and y.requires_grad
    recorders.clear()
    EncoderStackFn.apply(_cfg(), torch.randn(B, N, D, requires_grad=True), *_params(requires_grad=False))    # only the input wants one
    assert _names(recorders) == ['fwd']


def test_switch_off_restores_the_training_forward_under_no_grad(recorders):
    assert engine.inference_forward() is True              # default on
    engine.set_inference_forward(False)
    assert engine.inference_forward() is False
    with torch.no_grad():
        EncoderStackFn.apply(_cfg(), torch.randn(B, N, D), *_params())
    assert _names(recorders) == ['fwd']
    engine.set_inference_forward(True)
    recorders.clear()
    with torch.no_grad():
        EncoderStackFn.apply(_cfg(), torch.randn(B, N, D), *_params())
    assert _names(recorders) == ['infer']


def test_drop_path_scales_keep_the_training_forward(recorders):
    some = torch.ones(B)
    with torch.no_grad():
        EncoderStackFn.apply(_cfg(dp=[None] * (2 * L - 1) + [some]), torch.randn(B, N, D), *_params())
        assert _names(recorders) == ['fwd'] and recorders[0][1]['dp'][-1] is some
        recorders.clear()
        EncoderStackFn.apply(_cfg(dp=[None] * (2 * L)), torch.randn(B, N, D), *_params())      # eval() mode: every scale None
        assert _names(recorders) == ['infer']


def test_mx_products_keep_the_training_forward_only_where_they_would_run(recorders):
    with torch.no_grad():
        EncoderStackFn.apply(_cfg(mx=True, heads=8), torch.randn(B, N, 256), *_params(256))             # D, Hd multiples of 256: MX products selected
        assert recorders == [('fwd', dict(dp=None, mx=True))]
        recorders.clear()
        EncoderStackFn.apply(_cfg(mx=True), torch.randn(B, N, D), *_params())                  # D = 64: stack_fwd would run bf16 products anyway
        assert _names(recorders) == ['infer']
        recorders.clear()
        EncoderStackFn.apply(_cfg(mx=True, heads=8), torch.randn(1, 300, 256), *_params(256))           # beyond 256 tokens: bf16 products
        assert _names(recorders) == ['infer']


def test_without_the_stack_composite_nothing_changes(recorders):
    """dropout sites, a switched-off composite or an unsupported head width run the per-kernel route as before: neither stack call"""
    with torch.no_grad():
        EncoderStackFn.apply(_cfg(drops=[(0.0, 0.0)] * L), torch.randn(B, N, D), *_params())
        assert recorders == []
        ops.set_stack_composites(False)
        EncoderStackFn.apply(_cfg(), torch.randn(B, N, D), *_params())
        assert recorders == []
        ops.set_stack_composites(True)
        EncoderStackFn.apply(_cfg(heads=4), torch.randn(B, N, D), *_params())                  # head_dim 16
        assert recorders == []


def test_no_grad_multivit_reaches_the_library_call_once(stubbed):
    """MultiViT under torch.no_grad() through the stub: one mmae_stack_fwd_infer with the header's argument types (the stub checks
    count and types of every call), no mmae_stack_fwd, outputs that own their memory; with gradients: mmae_stack_fwd"""
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=8, image_size=32)}
    model = M.MultiViT(input_adapters=ins, output_adapters=None, num_global_tokens=1, dim_tokens=64, depth=3, num_heads=2).eval()
    x = torch.randn(2, 3, 32, 32)
    calls = []
    lib = M._lib.load()

    class Spy:                                            # in front of the stub (the fixture puts the real handle back)
        def __getattr__(self, name):
            fn = getattr(lib, name)

            def wrapped(*a):
                calls.append((name, a))
                return fn(*a)
            return wrapped
    M._lib._lib = Spy()
    try:
        with M.engine.precision('bf16'):
            with torch.no_grad():
                y = model(x)
                ys = model(x, return_all_layers=True)
            n_infer = [c for c in calls if c[0] == 'mmae_stack_fwd_infer']
            assert len(n_infer) == 2 and not [c for c in calls if c[0] == 'mmae_stack_fwd'], [c[0] for c in calls]
            assert [c[0] for c in calls].count('mmae_stack_infer_bytes') == 2
            for (_, (d, outs, st)), kept in zip(n_infer, ([2], [0, 1, 2])):
                assert type(d).__name__ == 'CArgObject' and isinstance(d._obj, M._lib.StackDesc) and d._obj.L == 3 and (d._obj.B, d._obj.N, d._obj.D) == (2, 17, 64)
                assert isinstance(outs, ctypes.c_void_p) and isinstance(st, int)
                table = ctypes.cast(outs, ctypes.POINTER(ctypes.c_void_p * 3)).contents
                assert [l for l in range(3) if table[l]] == kept
            assert y.shape == (2, 17, 64) and len(ys) == 3
            for t in [y] + list(ys):
                assert t.untyped_storage().nbytes() == t.numel() * t.element_size()
            calls.clear()
            model(x)
            assert [c[0] for c in calls].count('mmae_stack_fwd') == 1 and not [c for c in calls if c[0] == 'mmae_stack_fwd_infer']
    finally:
        M._lib._lib = lib
