"""GPU: batch staging (multimae_amd/staging.py, csrc/ingest.hip).  The device decode of every compact form is bit-identical to
the host conversion of the reference transform (utils/datasets.py:93-107), the fused depth standardisation to converting first
and calling truncated_depth_standardize, batches arrive in order and intact through the prefetching loader under a busy
consumer stream, and a few cfg3 training steps fed through the stager equal those fed the reference way bit for bit."""
import numpy as np
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, data_ops, staging

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORMS = [(staging.IMAGENET_DEFAULT_MEAN, staging.IMAGENET_DEFAULT_STD), (staging.IMAGENET_INCEPTION_MEAN, staging.IMAGENET_INCEPTION_STD)]


def _rgb_ref(u8: torch.Tensor, mean, std) -> torch.Tensor:
    return u8.permute(0, 3, 1, 2).float().div(255).sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1))


def _depth_ref(d: torch.Tensor) -> torch.Tensor:
    """torch.Tensor(np.array(img) / 2**16), batched"""
    return torch.Tensor(d.numpy().astype(np.float64) / 2 ** 16).unsqueeze(1)


def _sort_standardize(d: torch.Tensor) -> torch.Tensor:
    """run_pretraining_multimae.py:487-492"""
    t = torch.sort(d.flatten(1), dim=1)[0]
    t = t[:, int(0.1 * t.shape[1]): int(0.9 * t.shape[1])]
    return (d - t.mean(dim=1)[:, None, None, None]) / torch.sqrt(t.var(dim=1)[:, None, None, None] + 1e-6)


@pytest.mark.parametrize('mean, std', NORMS)
def test_rgb_decode_is_bit_exact(mean, std):
    table = data_ops.rgb_table(mean, std).to(DEV)
    g = torch.Generator().manual_seed(1)
    every = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()     # all 256 values x 3 channels
    every[..., 1] = every[..., 1].flip(1)
    cases = [every, torch.randint(0, 256, (8, 224, 224, 3), dtype=torch.uint8, generator=g),
             torch.randint(0, 256, (8, 223, 221, 3), dtype=torch.uint8, generator=g),                          # H*W odd: the scalar tail
             torch.randint(0, 256, (3, 5, 3, 3), dtype=torch.uint8, generator=g)]
    for u8 in cases:
        out = data_ops.ingest_rgb_u8(u8.to(DEV), table).cpu()
        assert torch.equal(out, _rgb_ref(u8, mean, std)), tuple(u8.shape)


@pytest.mark.parametrize('dtype', [torch.uint16, torch.int32])
def test_depth_decode_and_fused_standardisation_are_bit_exact(dtype):
    g = torch.Generator().manual_seed(2)
    if dtype == torch.uint16:
        d = torch.randint(0, 65536, (6, 224, 224), generator=g, dtype=torch.int32)
        d[1] = (d[1] // 4096) * 4096                                 # long runs of equal values: the cuts fall inside them
        d[2] = 777                                                   # constant map (variance 0)
        host = d.to(torch.uint16)
    else:
        d = torch.randint(-9000, 80000, (6, 224, 224), generator=g, dtype=torch.int32)     # a bicubic resize in 'I' mode overshoots
        d[1] = (d[1] // 4096) * 4096
        d[2] = -5
        d[3, :7] = 2 ** 24 + 3                                       # beyond fp32's exact integers: the key is the converted value's
        host = d
    conv = _depth_ref(d.to(torch.int64) if dtype == torch.uint16 else d)
    assert torch.equal(data_ops.ingest_depth(host.to(DEV)).cpu(), conv)
    assert torch.equal(data_ops.ingest_depth(host[:1, :7, :5].contiguous().to(DEV)).cpu(), conv[:1, :, :7, :5])      # odd count
    fused = data_ops.ingest_depth(host.to(DEV), standardize=(0.1, 0.9, 1e-6)).cpu()
    two_step = M.truncated_depth_standardize(conv.to(DEV)).cpu()
    assert torch.equal(fused, two_step), float((fused - two_step).abs().max())
    ref = _sort_standardize(conv)
    scale = float(ref.abs().max())
    assert float((fused - ref).abs().max()) <= 2e-6 * scale + 1e-6                # tests/test_kernels_gpu.py's depth tolerance


def test_semseg_decode_and_argument_checks():
    g = torch.Generator().manual_seed(3)
    for shape in [(8, 56, 56), (3, 7, 5)]:
        s = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)      # ids past the model's classes pass through
        assert torch.equal(data_ops.ingest_semseg_u8(s.to(DEV)).cpu(), s.to(torch.long))
    lib, x, y = _lib.load(), torch.zeros(64, dtype=torch.uint8, device=DEV), torch.zeros(64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mmae_ingest_rgb_u8(x.data_ptr(), y.data_ptr(), y.data_ptr(), 0, 4, 4, st) == -1
    assert lib.mmae_ingest_semseg_u8(x.data_ptr(), y.data_ptr(), 0, 4, st) == -1
    assert lib.mmae_ingest_depth(x.data_ptr(), _lib.U16, y.data_ptr(), 0, 4, 0, 0, 0, 0.0, st) == -1
    assert lib.mmae_ingest_depth(x.data_ptr(), 0, y.data_ptr(), 1, 4, 0, 0, 0, 0.0, st) == -1                      # f32 is not an ingest dtype
    assert lib.mmae_ingest_depth(x.data_ptr(), _lib.U16, y.data_ptr(), 1, 4, 1, 3, 4, 0.0, st) == -1               # hi - lo < 2
    torch.cuda.synchronize()


def _host_batch(seed, B, S=224, compact=True, pinned=False, classes=133):
    g = torch.Generator().manual_seed(seed)
    x = {'rgb': torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g),
         'depth': torch.randint(0, 65536, (B, S, S), dtype=torch.int32, generator=g).to(torch.uint16),
         'semseg': torch.randint(0, classes, (B, S // 4, S // 4), dtype=torch.uint8, generator=g)}
    if not compact:
        x = _reference_form(x, *NORMS[0])
    return {k: v.pin_memory() for k, v in x.items()} if pinned else x


def _reference_form(x, mean, std):
    return {'rgb': _rgb_ref(x['rgb'], mean, std), 'depth': _depth_ref(x['depth'].to(torch.int64)), 'semseg': x['semseg'].to(torch.long)}


@pytest.mark.parametrize('pinned', [False, True])
def test_staged_loader_delivers_each_batch_intact_under_a_busy_consumer(pinned):
    stager = M.BatchStager(DEV)
    batches = [_host_batch(100 + k, 16, pinned=pinned) for k in range(6)]
    expect = [_reference_form(b, *NORMS[0]) for b in batches]
    a = torch.randn(4096, 4096, device=DEV)
    got = []
    for x, tag in M.StagedLoader([(b, i) for i, b in enumerate(batches)], stager):
        for _ in range(5):                                           # ~5 ms of unrelated GEMMs queued before the batch is read
            a = torch.mm(a, a).mul_(1.0 / 64)
        got.append((tag, {t: v.clone() for t, v in x.items()}, x))   # read on the consumer stream; the staged tensors stay referenced
    torch.cuda.synchronize()
    assert [t for t, _, _ in got] == list(range(6))
    for k, (_, copy, held) in enumerate(got):
        for t in expect[k]:
            assert torch.equal(copy[t].cpu(), expect[k][t]), (k, t)
            assert torch.equal(held[t].cpu(), expect[k][t]), (k, t)
    # reference form: copied as it is; depth standardised on the copy stream when asked
    stager = M.BatchStager(DEV, standardize_depth=(0.1, 0.9, 1e-6))
    ref = _host_batch(7, 4, compact=False, pinned=pinned)
    out = stager(ref)
    assert torch.equal(out['rgb'].cpu(), ref['rgb']) and torch.equal(out['semseg'].cpu(), ref['semseg'])
    assert torch.equal(out['depth'].cpu(), M.truncated_depth_standardize(ref['depth'].to(DEV)).cpu())
    with pytest.raises(ValueError):
        stager({'rgb': torch.zeros(2, 224, 224, 3, dtype=torch.float64)})


def test_into_mode_writes_the_static_tensors():
    stager = M.BatchStager(DEV, standardize_depth=(0.1, 0.9, 1e-6))
    into = {'rgb': torch.empty(4, 3, 224, 224, device=DEV), 'depth': torch.empty(4, 1, 224, 224, device=DEV),
            'semseg': torch.empty(4, 56, 56, dtype=torch.long, device=DEV)}
    ptrs = {k: v.data_ptr() for k, v in into.items()}
    for seed in (11, 12):
        host = _host_batch(seed, 4)
        done = torch.cuda.Event()
        into['rgb'].mul_(2.0)                                        # the caller's last use of the static tensors ...
        done.record()                                                # ... and the event the copy stream waits on
        out = stager.get(stager.stage(host, into=into, after=done))
        assert {k: v.data_ptr() for k, v in out.items()} == ptrs
        ref = _reference_form(host, *NORMS[0])
        assert torch.equal(into['rgb'].cpu(), ref['rgb']) and torch.equal(into['semseg'].cpu(), ref['semseg'])
        assert torch.equal(into['depth'].cpu(), M.truncated_depth_standardize(ref['depth'].to(DEV)).cpu())
    with pytest.raises(ValueError):
        stager.stage(_host_batch(13, 2), into=into)                 # batch size differs from the static tensors


def _train_steps(feed, steps=3, B=8):
    """3 cfg3 steps (tests/test_curves_gpu.py's protocol); ``feed`` yields the (device) batch of each step"""
    import bench
    from multimae_amd.optim import FusedAdamW
    torch.manual_seed(0)
    model, doms = bench.build_model('cfg3')
    model.to(DEV)
    model.build_arena()
    M.engine.set_direct_grads(True)
    opt = FusedAdamW(model, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
    fns = bench.loss_fns()
    losses, norms = [], []
    try:
        with M.engine.precision('bf16'):
            for it, x in zip(range(steps), feed):
                torch.manual_seed(1000 + it)
                torch.cuda.manual_seed(1000 + it)
                opt.zero_grad()
                preds, masks = model(x, num_encoded_tokens=98, alphas=1.0, sample_tasks_uniformly=False, fp32_output_adapters=['semseg'])
                mk = dict(masks, norm_rgb=masks['rgb'])
                tgt = dict(x, norm_rgb=x['rgb'])
                loss = sum(fns[k](preds[k].float(), tgt[k], mask=mk[k]) for k in preds)
                loss.backward()
                norms.append(opt.step(loss).detach().clone())
                losses.append(loss.detach())
                torch.cuda.synchronize()                             # as the reference loop does after every step
    finally:
        M.engine.set_direct_grads(False)
    out = [float(v) for v in losses], [float(v) for v in norms]
    del opt, model
    torch.cuda.empty_cache()
    return out


def test_training_through_the_stager_equals_the_reference_feed():
    host = [_host_batch(200 + k, 8) for k in range(3)]

    def reference_feed():                                            # run_pretraining_multimae.py:482-492 with the engine's standardisation
        for b in host:
            x = {t: v.to(DEV, non_blocking=True) for t, v in _reference_form(b, *NORMS[0]).items()}
            x['depth'] = M.truncated_depth_standardize(x['depth'])
            yield x

    stager = M.BatchStager(DEV, standardize_depth=(0.1, 0.9, 1e-6))
    staged = (x for x, _ in M.StagedLoader([(b, 0) for b in host], stager))
    a = _train_steps(staged)
    b = _train_steps(reference_feed())
    assert a[0] == b[0], (a[0], b[0])
    assert a[1] == b[1], (a[1], b[1])


def test_dropin_staged_loader_feeds_the_reference_loop_unchanged():
    """amd_loop.staged_loader: (x_on_device, target) pairs with the args' mean / std and depth standardisation; the loop's own
    ``tensor.to(device, non_blocking=True)`` (run_pretraining_multimae.py:482-485) is then a no-op"""
    import types
    from dropin import amd_loop
    args = types.SimpleNamespace(device='cuda', imagenet_default_mean_and_std=False, standardize_depth=True)
    host = [_host_batch(300 + k, 2) for k in range(3)]
    seen = 0
    for step, (x, target) in enumerate(amd_loop.staged_loader([(h, k) for k, h in enumerate(host)], args)):
        tasks_dict = {task: tensor.to(args.device, non_blocking=True) for task, tensor in x.items()}
        assert target == step and all(tasks_dict[t] is x[t] for t in x)
        ref = _reference_form(host[step], *NORMS[1])
        assert torch.equal(x['rgb'].cpu(), ref['rgb']) and torch.equal(x['semseg'].cpu(), ref['semseg'])
        assert torch.equal(x['depth'].cpu(), M.truncated_depth_standardize(ref['depth'].to(DEV)).cpu())
        seen += 1
    assert seen == 3
