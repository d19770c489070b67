"""A/B of the encoder stack's forward under torch.no_grad(): the inference forward (engine.set_inference_forward(True), the default:
ops.stack_fwd_infer -> mmae_stack_fwd_infer) against the same call with the switch off (ops.stack_fwd -> mmae_stack_fwd, the training
forward, which is what every no-grad call ran before the switch existed).

    python tools/infer_forward_bench.py [--rounds 20] [--iters 5] [--out profiles/infer_forward_bench.json] [--bench-evidence FILE]

Method (measuring guide: compare two versions in the same call, alternating them): a ViT-B encoder (12 blocks, width 768, 12 heads) of a
MultiViT with its parameter arena, bf16 mode; per shape both sides are warmed up, then `rounds` rounds of (switch on: `iters` forwards,
switch off: `iters` forwards), each window timed with device events behind a synchronise; the figure per side is the median over the
rounds, the spread its (p90 - p10) / median.  The outputs of the two sides are compared with torch.equal at every shape.  Peak memory:
torch.cuda.max_memory_allocated of ONE forward per side above what was allocated before it, next to the figure derived from
mmae_stack_infer_bytes / mmae_stack_act_bytes.

--bench-evidence: a JSON file with bench.py result lines of the parent commit and of this one from one alternating run
({"parent": [...], "this": [...]}); embedded as given (bench.py runs with gradients, so it never takes the new route)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import multimae_amd as M  # noqa: E402
from multimae_amd import _lib, ops  # noqa: E402
from multimae_amd.multimae_utils import run_blocks  # noqa: E402

SHAPES = [dict(name='cls evaluation', B=192, N=197), dict(name='semseg evaluation at 512 x 512', B=4, N=1025), dict(name='B = 256, N = 99', B=256, N=99)]
D, HEADS, DEPTH, HD = 768, 12, 12, 3072


def derived_bytes(B, N):
    d = _lib.StackDesc()
    d.L, d.B, d.N, d.D, d.heads, d.Hd = DEPTH, B, N, D, HEADS, HD
    d.act_dtype = _lib.BF16
    lib = _lib.load()
    infer, act = int(lib.mmae_stack_infer_bytes(ctypes.byref(d))), int(lib.mmae_stack_act_bytes(ctypes.byref(d)))
    return dict(infer_scratch=infer, infer_output=B * N * D * 4, infer_total=infer + B * N * D * 4, training_slab=act)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    return peak


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, int(round(q * (len(v) - 1)))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'infer_forward_bench.json'))
    ap.add_argument('--bench-evidence', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'infer_forward_bench needs a GPU'
    assert args.rounds >= 20, 'medians of at least 20 rounds'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=224)}
    model = M.MultiViT(input_adapters=ins, output_adapters=None, num_global_tokens=1, dim_tokens=D, depth=DEPTH, num_heads=HEADS).to(dev).eval()
    model.build_arena()
    res = dict(what='no-grad forward of the ViT-B encoder stack, bf16: inference forward (switch on) vs training forward (switch off)',
               switch_off_is_the_parent_route='checked by reading the code: with engine.set_inference_forward(False) EncoderStackFn.forward skips the '
               'new branch and calls ops.stack_fwd with the arguments it was called with before (functions.py); ops.stack_fwd changed only in '
               'that its pointer tables are built by a helper shared with stack_fwd_infer; mmae_stack_fwd and the kernels it launches are untouched',
               method=dict(rounds=args.rounds, iters_per_window=args.iters, warmup=args.warmup, timing='device events around each window, synchronise before and after',
                           order='alternating: on, off, on, off, ...', statistic='median over rounds; spread = (p90 - p10) / median'),
               device=torch.cuda.get_device_name(0), shapes=[])
    with M.engine.precision('bf16'), torch.no_grad():
        for s in SHAPES:
            B, N = s['B'], s['N']
            x = torch.randn(B, N, D, device=dev)

            def fwd():
                return run_blocks(model.encoder, x, root=model)
            ys = {}
            for on in (True, False):
                M.engine.set_inference_forward(on)
                for _ in range(args.warmup):
                    ys[on] = fwd()
            torch.cuda.synchronize()
            equal = bool(torch.equal(ys[True], ys[False]))
            owns = ys[True].untyped_storage().nbytes() == ys[True].numel() * 4
            del ys
            t = {True: [], False: []}
            for _ in range(args.rounds):
                for on in (True, False):
                    M.engine.set_inference_forward(on)
                    t[on].append(window(fwd, args.iters))
            peaks = {}
            for on in (True, False):
                M.engine.set_inference_forward(on)
                peaks[on] = peak_of(fwd)
            M.engine.set_inference_forward(True)
            side = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=pct(v, 0.1), p90_ms=pct(v, 0.9),
                                  spread=(pct(v, 0.9) - pct(v, 0.1)) / statistics.median(v))
            on_s, off_s = side(t[True]), side(t[False])
            der = derived_bytes(B, N)
            row = dict(name=s['name'], B=B, N=N, rows=B * N, outputs_bit_equal=equal, output_owns_its_memory=owns,
                       inference_forward=on_s, training_forward=off_s, time_ratio_on_over_off=on_s['median_ms'] / off_s['median_ms'],
                       slower_beyond_spread=on_s['median_ms'] > off_s['median_ms'] * (1.0 + max(on_s['spread'], off_s['spread'])),
                       peak_bytes_above_baseline=dict(inference_forward=peaks[True], training_forward=peaks[False]),
                       derived_bytes=der,
                       peak_ratio_measured=peaks[False] / max(1, peaks[True]), peak_ratio_derived=der['training_slab'] / der['infer_total'])
            res['shapes'].append(row)
            print(json.dumps(row))
            del x
            torch.cuda.empty_cache()
    if args.bench_evidence:
        with open(args.bench_evidence) as f:
            res['bench_py'] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
