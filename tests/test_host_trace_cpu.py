"""CPU: the host layer's library-call trace, pinned.  Every configuration below runs on the type-checking stub of the C ABI with
dryrun_harness.RecordingLib in front of it; what the library would have seen -- which entry points, in which order, with which scalar
arguments, descriptor fields, NULL / non-NULL pointers and aliased pointer fields (never the addresses) -- must equal
tests/golden/host_trace.json call for call.  The fixture holds a table of names and, per configuration, one (name index, digest of
the canonical arguments) pair per call; tests/golden/make_golden_host_trace.py writes it.  A refactor of functions.py / ops.py that
changes nothing the library can observe leaves this test green; on a mismatch it prints the first differing call."""
import contextlib
import gc
import json
import os
from functools import partial

import pytest
import torch
from torch import nn

import dryrun_harness
from helpers import MINI, build_engine_model, build_mini_engine, load_mini, make_inputs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'host_trace.json')


@contextlib.contextmanager
def recording_stub():
    """the stub of the C ABI with a fresh RecordingLib in front of it; every switch a configuration moves is put back afterwards"""
    from multimae_amd import _lib, engine, ops
    old = (_lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0])
    prev = (engine.fp32_adapter_gemm(), ops._X3_PRESPLIT)
    dryrun_harness.install()
    r = _lib._lib = dryrun_harness.RecordingLib()
    yield r
    _lib._lib, ops._require_gpu, ops._stream, ops._device_ok, ops._WS_ELEMS[0] = old
    engine.set_fp32_adapter_gemm(prev[0])
    ops._X3_PRESPLIT = prev[1]
    engine.set_direct_grads(False)
    ops._WS.clear()
    ops.set_composite_blocks(True)
    ops.set_stack_composites(True)


@pytest.fixture()
def rec():
    with recording_stub() as r:
        yield r


def _mini_step(model, mode, direct, x, fp32_adapters=('semseg',)):
    """the step of tests/test_dryrun_cpu.py; afterwards every prediction is read once (the lazily written images)"""
    import multimae_amd as M
    from multimae_amd import lazy
    P = MINI['P']
    fns = {'rgb': M.MaskedMSELoss(P, 1), 'depth': M.MaskedL1Loss(P, 1), 'semseg': M.MaskedCrossEntropyLoss(P, 4),
           'norm_rgb': M.MaskedMSELoss(P, 1, norm_pix=True)}
    M.engine.set_direct_grads(direct)
    with M.engine.precision(mode):
        preds, masks = model(x, num_encoded_tokens=MINI['nvis'], alphas=1.0, fp32_output_adapters=list(fp32_adapters))
        tgt = dict(x, norm_rgb=x['rgb'])
        mk = dict(masks, norm_rgb=masks['rgb'])
        losses = {k: fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds}
        sum(losses.values()).backward()
        for k in preds:
            lazy.materialize(preds[k])


def _mini(direct, ready_cb=False, bwd_chunk=None):
    torch.manual_seed(0)
    g = load_mini()
    model = build_mini_engine()
    model.load_state_dict(g['sd'])
    if direct:
        model.build_arena()
    if ready_cb:
        model._grad_ready_cb = lambda name: None
    if bwd_chunk is not None:
        model._bwd_chunk_layers = bwd_chunk
    return model, g['x']


def _composites(setting):
    from multimae_amd import ops
    ops.set_composite_blocks(setting != 'none')
    ops.set_stack_composites(setting == 'stack')


def run_matrix(mode, direct, composite):
    _composites(composite)
    model, x = _mini(direct)
    _mini_step(model, mode, direct, x)


def run_fp32_adapter(gemm, adapter='semseg', presplit=False):
    from multimae_amd import engine, ops
    engine.set_fp32_adapter_gemm(gemm)
    ops._X3_PRESPLIT = presplit
    model, x = _mini(True)
    for _ in range(2):                                    # twice: the second forward finds the weight shadows of the first
        _mini_step(model, 'bf16', True, x, fp32_adapters=(adapter,))


def run_chunked(bwd_chunk):
    model, x = _mini(True, ready_cb=True, bwd_chunk=bwd_chunk)
    _mini_step(model, 'bf16', True, x)


def _adapter_options_model(depth, **opts):
    """the models of test_dryrun_cpu.py's drop-path and dropout tests: `opts` per output adapter key, or for all"""
    import multimae_amd as M
    doms, P, S = MINI['doms'], MINI['P'], MINI['S']
    torch.manual_seed(0)
    ins = {d: (M.SemSegInputAdapter(num_classes=133, dim_class_emb=16, interpolate_class_emb=False, stride_level=4, patch_size_full=P, image_size=S)
               if d == 'semseg' else M.PatchedInputAdapter(num_channels=3 if d == 'rgb' else 1, stride_level=1, patch_size_full=P, image_size=S))
           for d in doms}
    enc_opts = opts.pop('encoder', {})
    xattn = opts.pop('use_xattn', lambda key: True)
    outs = {}
    for key, task in [(d, d) for d in doms] + [('norm_rgb', 'rgb')]:
        ch = {'rgb': 3, 'depth': 1, 'semseg': 133}[task]
        outs[key] = M.SpatialOutputAdapter(num_channels=ch, stride_level=4 if task == 'semseg' else 1, patch_size_full=P, dim_tokens=64, depth=depth,
                                           num_heads=2, use_task_queries=True, task=task, context_tasks=list(doms), use_xattn=xattn(key),
                                           image_size=S, **opts)
    return M.MultiMAE(ins, outs, num_global_tokens=1, dim_tokens=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                      norm_layer=partial(nn.LayerNorm, eps=1e-6), **enc_opts).train()


def run_drop_path(mode):
    model = _adapter_options_model(3, drop_path_rate=0.3)
    _mini_step(model, mode, False, load_mini()['x'])


def run_dropout(mode):
    model = _adapter_options_model(2, drop_rate=0.1, attn_drop_rate=0.2, use_xattn=lambda key: key != 'depth',
                                   encoder=dict(drop_rate=0.1, attn_drop_rate=0.2))
    _mini_step(model, mode, False, load_mini()['x'])


def run_mxfp8():
    import multimae_amd as M
    from multimae_amd import ops
    torch.manual_seed(0)
    doms = ['rgb', 'semseg']
    model = build_engine_model(doms, 8, 32, enc=(256, 2, 4), posemb_size=32)
    x = make_inputs(doms, 2, 32)
    M.engine.set_direct_grads(True)
    model.build_arena()
    ops._X3_PRESPLIT = True
    with M.engine.precision('mxfp8'):
        preds, masks = model(x, num_encoded_tokens=9, alphas=1.0, fp32_output_adapters=['semseg'])
        sum(p.float().sum() for p in preds.values()).backward()


def _multivit():
    import multimae_amd as M
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=8, image_size=32)}
    model = M.MultiViT(input_adapters=ins, output_adapters=None, num_global_tokens=1, dim_tokens=64, depth=3, num_heads=2)
    return model, torch.randn(2, 3, 32, 32)


def run_infer(all_layers):
    import multimae_amd as M
    model, x = _multivit()
    model.eval()
    with M.engine.precision('bf16'), torch.no_grad():
        model(x, return_all_layers=all_layers)


def run_all_layers_bwd(composite):
    import multimae_amd as M
    _composites(composite)
    model, x = _multivit()
    with M.engine.precision('bf16'):
        ys = model(x, return_all_layers=True)
        (ys[0].sum() + ys[2].sum()).backward()


def run_convnext():
    import multimae_amd as M
    from multimae_amd import lazy, output_adapters as OA
    torch.manual_seed(0)
    head = OA.ConvNeXtAdapter(num_classes=5, embed_dim=256, preds_per_patch=16, main_tasks=('rgb',), depth=1, interpolate_mode='bilinear')
    head.init(16)
    info = {'tasks': {'rgb': {'start_idx': 0, 'end_idx': 6}}, 'image_size': (32, 48)}
    target = torch.randint(0, 5, (2, 32, 48))
    with M.engine.precision('bf16'):
        y = head(torch.randn(2, 7, 16, requires_grad=True), info)
        M.SegCrossEntropyLoss(ignore_index=255)(y, target).backward()
        lazy.materialize(y)


CONFIGS = {}
for _mode, _settings in (('bf16', ('stack', 'block', 'none')), ('fp32', ('stack',))):    # (fp32 records the same under all three settings)
    for _direct in (False, True):
        for _c in _settings:
            CONFIGS[f'step-{_mode}-{"direct" if _direct else "autograd"}-{_c}'] = partial(run_matrix, _mode, _direct, _c)
for _gemm in ('exact', 'x3', 'f16', 'h16'):
    CONFIGS[f'fp32-semseg-{_gemm}'] = partial(run_fp32_adapter, _gemm)
CONFIGS['fp32-semseg-x3-presplit'] = partial(run_fp32_adapter, 'x3', presplit=True)
CONFIGS['fp32-rgb-h16'] = partial(run_fp32_adapter, 'h16', adapter='rgb')       # 192-column patch rows: on the fp16-storage grid
for _chunk in (1, 3):
    CONFIGS[f'chunked-bwd-{_chunk}'] = partial(run_chunked, _chunk)
for _mode in ('bf16', 'fp32'):
    CONFIGS[f'drop-path-{_mode}'] = partial(run_drop_path, _mode)
    CONFIGS[f'dropout-{_mode}'] = partial(run_dropout, _mode)
CONFIGS['mxfp8-x3-presplit'] = run_mxfp8
for _all in (False, True):
    CONFIGS[f'infer-{"all-layers" if _all else "last"}'] = partial(run_infer, _all)
for _c in ('stack', 'none'):
    CONFIGS[f'all-layers-bwd-{_c}'] = partial(run_all_layers_bwd, _c)
CONFIGS['convnext-seg-ce'] = run_convnext


def record(name, lib):
    """run configuration `name` on the recording stub `lib`; returns its calls [(symbol, canonical arguments)]"""
    lib.calls.clear()
    CONFIGS[name]()
    gc.collect()
    return list(lib.calls)


def encode(traces):
    """{configuration: calls} -> the fixture's content"""
    names = sorted({n for calls in traces.values() for n, _ in calls})
    idx = {n: i for i, n in enumerate(names)}
    return {'names': names, 'configs': {k: [[idx[n], dryrun_harness.digest(a)] for n, a in calls] for k, calls in traces.items()}}


def test_fixture_covers_every_configuration():
    with open(GOLD) as f:
        gold = json.load(f)
    assert sorted(gold['configs']) == sorted(CONFIGS)
    seen = {gold['names'][i] for calls in gold['configs'].values() for i, _ in calls}
    # what the dry run did not reach before it went through the composite adapter calls
    for sym in ('mmae_adapter_fwd', 'mmae_adapter_bwd', 'mmae_stack_fwd', 'mmae_stack_bwd', 'mmae_stack_fwd_infer', 'mmae_block_fwd', 'mmae_block_bwd',
                'mmae_masked_pixel_loss_pat_bwd', 'mmae_masked_ce_pat_bwd', 'mmae_unpatchify', 'mmae_resize_fwd', 'mmae_x3_prepare_weights',
                'mmae_mx_prepare_weights', 'mmae_cast_f32_to_f16'):
        assert sym in seen, sym


@pytest.mark.parametrize('name', list(CONFIGS))
def test_library_sees_the_pinned_calls(rec, name):
    with open(GOLD) as f:
        gold = json.load(f)
    want = [(gold['names'][i], d) for i, d in gold['configs'][name]]
    calls = record(name, rec)
    got = [(n, dryrun_harness.digest(a)) for n, a in calls]
    for i, (w, g) in enumerate(zip(want, got)):
        if w != g:
            print(f'{name}: first differing call is #{i}: recorded {w[0]} ({w[1]}), now {g[0]} ({g[1]}) with arguments\n'
                  + json.dumps(calls[i][1], indent=1, sort_keys=True))
            print('calls around it now:', [n for n, _ in got[max(0, i - 5):i + 5]], 'recorded:', [n for n, _ in want[max(0, i - 5):i + 5]])
            break
    assert got[:len(want)] == want[:len(got)], f'{name}: call #{i} differs (see the captured output)'
    assert len(got) == len(want), f'{name}: {len(got)} calls, {len(want)} recorded; the first {min(len(got), len(want))} agree'


# ------------------------------------------------------------------------------------------------------------------------------
# Lifetimes: what the trace cannot see.  The host arrays a saved descriptor points to must stay alive with the state the forward
# returns -- the backward hands the same descriptor to the library again.
# ------------------------------------------------------------------------------------------------------------------------------
def _host_arrays(obj, found, seen):
    """addresses of every ctypes array reachable from obj through tuples, lists and the attributes of plain objects"""
    import ctypes
    if id(obj) in seen or obj is None or isinstance(obj, (torch.Tensor, ctypes.Structure, int, float, str, torch.dtype)):
        return found
    seen.add(id(obj))
    if isinstance(obj, ctypes.Array):
        found.add(ctypes.addressof(obj))
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _host_arrays(o, found, seen)
    else:
        for n in list(getattr(obj, '__slots__', ())) + list(getattr(obj, '__dict__', {})):
            _host_arrays(getattr(obj, n, None), found, seen)
    return found


def _assert_host_fields_alive(state, fields, expect_set):
    from multimae_amd import ops
    ops._PTRS.tabs.clear()                                # the caches must not be what keeps the tables alive
    ops._SHADOWS.tabs.clear()
    gc.collect()
    alive = _host_arrays(state, set(), set())
    held = {f: getattr(state.desc, f) for f in fields if getattr(state.desc, f)}
    assert set(held) >= set(expect_set), (sorted(held), expect_set)
    for f, addr in held.items():
        assert addr in alive, f'{type(state.desc).__name__}.{f} points to a host array the returned state does not hold'


def test_stack_state_holds_the_host_arrays_of_its_descriptor(rec):
    from multimae_amd import ops
    L, B, N, D = 2, 2, 5, 256
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (4 * D, D), (4 * D,), (D, 4 * D), (D,)]
    params = [torch.zeros(s) for _ in range(L) for s in shapes]
    dp = [None, torch.ones(B), None, None]
    outs, state = ops.stack_fwd(torch.zeros(B * N, D), params, lambda w: w.detach().to(torch.bfloat16), 4, 1e-6, torch.bfloat16, B, N, dp, mx=True)
    del params, dp, outs
    _assert_host_fields_alive(state, ('w', 'p', 'dp', 'mx_w'), ('w', 'p', 'dp', 'mx_w'))


def test_adapter_state_holds_the_host_arrays_of_its_descriptor(rec, monkeypatch):
    from multimae_amd import engine, ops
    states = []
    real = ops.adapter_fwd
    monkeypatch.setattr(ops, 'adapter_fwd', lambda *a, **k: (lambda out: (states.append(out[1]), out)[1])(real(*a, **k)))
    engine.set_fp32_adapter_gemm('x3')
    ops._X3_PRESPLIT = True
    model, x = _mini(False)
    import multimae_amd as M
    with M.engine.precision('bf16'):
        preds, masks = model(x, num_encoded_tokens=MINI['nvis'], alphas=1.0, fp32_output_adapters=['semseg'])
    del model, x, preds, masks
    assert len(states) == 4
    fields = ('task_offsets_host', 'w', 'p', 'task_emb', 'x3_w')
    assert sum(bool(s.desc.x3_w) for s in states) == 1                 # the fp32 adapter's pre-split weights
    for s in states:
        _assert_host_fields_alive(s, fields, fields[:4])
