"""The input preparation of the dense fine-tuning loops (run_finetuning_depth.py:671-695) at two geometries, two variants alternating in
one process, each round timed with device events on the stream after a warm-up:

  eager  a restatement of the script's lines with torch: clone, NaN under the mask, a sort of every map, the cuts read from device
         scalars in a Python loop with a mean and a var per sample, the division, the boolean-mask fills (through a repeat_interleave'd
         mask for every non-rgb input)
  fused  dropin/amd_loop.prepare_dense_inputs: mmae_depth_standardize_masked and mmae_mask_invalid (csrc/depth.hip), one launch each

  depth      B = 64, 1 x 256 x 256, about 80 % valid, --standardize_depth: the depth recipe with a depth input
  taskonomy  B = 64, a 3-channel 256 x 256 extra input (surface normals) masked in place, no depth input

A round is `--inner` calls between two events; medians and the min-max spread of the per-call time of each variant, the kernel launches
of one call (torch.profiler) and the host synchronisations of two consecutive calls (torch's synchronisation check in 'warn' mode) go
to profiles/robust_depth_bench.json.  Two conditions are checked, not measured: the fused path shows 0 host synchronisations, and each
of the two kernels is 1 launch per call (exit status 1 otherwise, after the file is written).  The fused result is compared with the
eager one before anything is timed.  Refuses to run without a GPU.

    python tools/robust_depth_bench.py [--iters 20] [--warmup 5] [--inner 10] [--out profiles/robust_depth_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimae_amd as M  # noqa: E402,F401
from dropin import amd_loop  # noqa: E402

B, H, W, C_EXTRA, VALID = 64, 256, 256, 3, 0.8


def eager_prepare(input_dict, tasks_dict, standardize_depth):
    """what the script's loop does between building input_dict and the forward pass, with the same torch operations"""
    mask = tasks_dict['mask_valid']
    if standardize_depth and 'depth' in input_dict:
        depth = input_dict['depth']
        work = depth.clone()
        work[~mask] = float('nan')
        ordered = torch.sort(work.flatten(1), dim=1)[0]                       # NaN sorts last: the valid values come first
        n_valid = (~torch.isnan(ordered)).sum(dim=1)
        first, last = (n_valid * 0.1).long(), (n_valid * 0.9).long()
        means = torch.stack([ordered[b, i:j].mean() for b, (i, j) in enumerate(zip(first, last))])      # two read-backs per sample
        variances = torch.stack([ordered[b, i:j].var() for b, (i, j) in enumerate(zip(first, last))])
        depth = (depth - means[:, None, None, None]) / torch.sqrt(variances[:, None, None, None] + 1e-6)
        depth[~mask] = 0.0
        input_dict['depth'] = depth
    for task in input_dict:
        if task == 'rgb':
            continue
        x = input_dict[task]
        x[~mask.repeat_interleave(repeats=x.shape[1], dim=1)] = 0.0
    return input_dict


def _alternate(variants, iters, warmup, inner):
    """variants: name -> thunk.  Runs them in turn, `warmup` untimed rounds first; returns name -> list of ms per call."""
    times = {n: [] for n in variants}
    for it in range(warmup + iters):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[n].append(e0.elapsed_time(e1) / inner)
    return times


def _stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts), 'spread_ms': max(ts) - min(ts), 'n': len(ts)}


def _counts(fn, with_names):
    """kernel launches (torch.profiler's device kernel events; by name with `with_names`) of one call and host synchronisations
    (torch's synchronisation check in 'warn' mode) of two consecutive calls; a count that could not be taken is None"""
    syncs = []
    for _ in range(2):                                         # two rounds, both recorded: a count in the first only is a first-call effect
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                fn()
            finally:
                torch.cuda.set_sync_debug_mode('default')
        syncs.append(sum('synchroniz' in str(x.message) for x in ws))
    torch.cuda.synchronize()
    launches, names = None, None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]
        launches = len(ev) or None
        if with_names:
            names = {}
            for e in ev:
                names[e.name] = names.get(e.name, 0) + 1
    except Exception as e:                                     # the profiler is optional: the timings do not depend on it
        print('launch count not taken:', repr(e), flush=True)
    out = {'launches': launches, 'host_syncs': syncs}
    if with_names:
        out['kernels'] = names
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--batch', type=int, default=B)
    ap.add_argument('--no-write', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'robust_depth_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('robust_depth_bench: needs a GPU (the engine has no CPU path)')
    if a.iters < 5:
        sys.exit('robust_depth_bench: at least 5 timed rounds')
    dev, nb = 'cuda', a.batch
    torch.manual_seed(0)
    rgb = torch.randn(nb, 3, H, W, device=dev)
    depth = torch.rand(nb, 1, H, W, device=dev) ** 2 * 10.0 + 0.3
    mask = torch.rand(nb, 1, H, W, device=dev) < VALID
    normal = torch.randn(nb, C_EXTRA, H, W, device=dev)
    res = {'device': torch.cuda.get_device_name(), 'geometry': dict(B=nb, H=H, W=W, extra_channels=C_EXTRA, valid_fraction=VALID),
           'iters': a.iters, 'warmup': a.warmup, 'calls_per_round': a.inner}

    def depth_case(fn):
        tasks = {'rgb': rgb, 'depth': depth, 'mask_valid': mask}                 # the depth itself is never written: rebound
        return lambda: fn({'rgb': rgb, 'depth': depth}, tasks, True)

    def extra_case(fn):
        tasks = {'rgb': rgb, 'normal': normal, 'mask_valid': mask}               # in place; masking a masked input costs the same
        return lambda: fn({'rgb': rgb, 'normal': normal}, tasks, False)

    cases = {'depth_standardize_B64_1x256x256': depth_case, 'taskonomy_mask_B64_3x256x256': extra_case}
    # the two variants compute the same thing (the bound of tests/test_robust_depth_gpu.py against the reference's f32 lines)
    e, f = depth_case(eager_prepare)()['depth'], depth_case(amd_loop.prepare_dense_inputs)()['depth']
    err, scale = float((e - f).abs().max()), float(e.abs().max())
    res['fused_against_eager'] = {'max_abs_diff': err, 'max_abs_value': scale, 'bound': 2e-6 * scale + 1e-6}
    print('fused against eager', json.dumps(res['fused_against_eager']), flush=True)
    for key, case in cases.items():
        variants = {'eager': case(eager_prepare), 'fused': case(amd_loop.prepare_dense_inputs)}
        t = _alternate(variants, a.iters, a.warmup, a.inner)
        res[key] = {n: _stats(v) for n, v in t.items()}
        res[key]['eager_over_fused_medians'] = res[key]['eager']['median_ms'] / res[key]['fused']['median_ms']
        print(key, json.dumps(res[key]), flush=True)

    def write():
        if not a.no_write:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(res, fh, indent=1)
                fh.write('\n')
    write()                                                    # the timings are kept even if the profiler below gives up
    for key, case in cases.items():
        res[key]['per_call'] = {'eager': _counts(case(eager_prepare), False), 'fused': _counts(case(amd_loop.prepare_dense_inputs), True)}
        print(key, json.dumps(res[key]['per_call']), flush=True)
    write()
    bad = []
    if not err <= 2e-6 * scale + 1e-6:
        bad.append(f'the fused depth differs from the eager one by {err} (bound {2e-6 * scale + 1e-6})')
    for key in cases:
        c = res[key]['per_call']['fused']
        if c['host_syncs'] != [0, 0]:
            bad.append(f'{key}: the fused path synchronised the host {c["host_syncs"]}')
        if c['launches'] != 1:
            bad.append(f'{key}: the fused path is {c["launches"]} launches per call, not 1 ({c["kernels"]})')
    if bad:
        sys.exit('robust_depth_bench: ' + '; '.join(bad))


if __name__ == '__main__':
    main()
