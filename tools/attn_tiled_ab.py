"""A/B of the tiled bf16 attention kernels (sequences beyond 256 tokens) against the batched-GEMM + softmax path, in one process.

  python tools/attn_tiled_ab.py [--out profiles/attn_tiled_ab] [--window 0.5] [--repeats 3] [--quick]

Method: per shape the two paths alternate (tiled, GEMM, tiled, GEMM, ...), `--repeats` pairs; every (shape, path, direction) is warmed
before its first window; a window is at least `--window` seconds of back-to-back calls between two HIP events.  ops.set_fused_attention(
False) selects the GEMM path: S materialised as f32 [B][H][Nq][Nk], a row-softmax pass, P saved in bf16 for the backward.
Reported per shape: both times (median and min..max of the repeats), the algorithmic FLOPs (4 B H Nq Nk hd forward, 10 ... backward, no
recompute counted), TF/s and the share of the 2.5 PF/s bf16 MFMA peak, and -- as arithmetic from the shapes, not a measurement -- the
bytes the GEMM path moves for S and P.
Encoder leg: a 12-block ViT-B at B = 16, N = 1025, forward + backward: per-kernel blocks + GEMM attention (fused attention off) against
the stack composite + tiled attention.
Fails without a GPU.  Writes <out>.json and <out>.txt."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16 = 2.5e15


def window(fn, seconds):
    """time of one call of fn, from a window of >= `seconds` of back-to-back calls between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    n = max(3, int(math.ceil(seconds / max(e0.elapsed_time(e1) * 1e-3, 1e-6))))
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def attention_case(B, H, N, hd):
    from multimae_amd import ops
    from multimae_amd.ops import AttnView
    D = H * hd
    g = torch.Generator(device='cuda').manual_seed(N + hd)
    qkv = torch.randn(B * N, 3 * D, device='cuda', generator=g).to(torch.bfloat16)
    do = torch.randn(B * N, D, device='cuda', generator=g).to(torch.bfloat16)
    o, dqkv = torch.empty_like(do), torch.empty_like(qkv)
    v = lambda t, c: AttnView(t, c, t.shape[1], N)
    sc = hd ** -0.5

    def fwd():
        return ops.attention_fwd(v(qkv, 0), v(qkv, D), v(qkv, 2 * D), v(o, 0), B, H, hd, sc)

    def fwd_bwd():
        st = fwd()
        ops.attention_bwd(v(qkv, 0), v(qkv, D), v(qkv, 2 * D), st, v(o, 0), v(do, 0), v(dqkv, 0), v(dqkv, D), v(dqkv, 2 * D), B, H, hd, sc)

    return fwd, fwd_bwd


def ab(fn, args, want_tags=None):
    """alternate the two paths; returns {'tiled': [t...], 'gemm': [t...]}"""
    from multimae_amd import ops
    out = {'tiled': [], 'gemm': []}
    try:
        for path in ('tiled', 'gemm'):                    # warm both
            ops.set_fused_attention(path == 'tiled')
            fn(); fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for path in ('tiled', 'gemm'):
                ops.set_fused_attention(path == 'tiled')
                out[path].append(window(fn, args.window))
    finally:
        ops.set_fused_attention(True)
    return out


def summary(ts):
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts), all=ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attn_tiled_ab'))
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='two shapes and a 2-block encoder: a rehearsal, not a measurement')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('attn_tiled_ab: no GPU found -- this tool measures, it has no CPU mode')
    import multimae_amd as M
    from multimae_amd import ops
    from multimae_amd.multimae_utils import Block, run_blocks
    shapes = [(name, H, 64, N) for name, H in (('ViT-B', 12), ('ViT-L', 16)) for N in (257, 577, 1025, 2049, 3201)] + [('hd32', 8, 32, 1025)]
    if args.quick:
        shapes = [('ViT-B', 12, 64, 257), ('hd32', 8, 32, 1025)]
    rows = []
    for name, H, hd, N in shapes:
        B = max(1, round(16384 / N))
        fwd, fwd_bwd = attention_case(B, H, N, hd)
        st = fwd()
        assert st[0] == 'fused', st[0]
        flops_f = 4.0 * B * H * N * N * hd
        for direction, fn, flops in (('fwd', fwd, flops_f), ('fwd+bwd', fwd_bwd, 3.5 * flops_f)):
            t = ab(fn, args)
            st_, sg = summary(t['tiled']), summary(t['gemm'])
            Np = (N + 7) // 8 * 8
            s_bytes, p_bytes = B * H * N * Np * 4, B * H * N * Np * 2
            # arithmetic, from the shapes: forward writes S, reads S, writes P, reads P; backward adds dP (f32) write + read, P read x2, dS (bf16) write + read x2
            moved = (2 * s_bytes + 2 * p_bytes) if direction == 'fwd' else (2 * s_bytes + 2 * p_bytes) + (2 * s_bytes + 2 * p_bytes + 3 * p_bytes)
            row = dict(shape=name, B=B, H=H, N=N, hd=hd, direction=direction, flops=flops, tiled=st_, gemm=sg,
                       tiled_tflops=flops / st_['median'] / 1e12, gemm_tflops=flops / sg['median'] / 1e12,
                       tiled_share_of_peak=flops / st_['median'] / PEAK_BF16, speedup=sg['median'] / st_['median'],
                       wins_beyond_spread=st_['max'] < sg['min'], gemm_S_P_bytes_arithmetic=moved)
            rows.append(row)
            print(f"{name:6s} B {B:3d} H {H:2d} N {N:5d} hd {hd} {direction:8s} tiled {st_['median'] * 1e3:8.3f} ms [{st_['min'] * 1e3:.3f}..{st_['max'] * 1e3:.3f}] "
                  f"gemm {sg['median'] * 1e3:8.3f} ms [{sg['min'] * 1e3:.3f}..{sg['max'] * 1e3:.3f}]  x{row['speedup']:.2f}  "
                  f"{row['tiled_tflops']:.1f} TF/s = {100 * row['tiled_share_of_peak']:.1f} % of peak", flush=True)
        del fwd, fwd_bwd
        torch.cuda.empty_cache()
    # ---- encoder leg
    L, D, heads, B, N = (2 if args.quick else 12), 768, 12, (2 if args.quick else 16), 1025
    torch.manual_seed(0)
    blocks = torch.nn.ModuleList([Block(D, heads, qkv_bias=True) for _ in range(L)]).cuda()
    x = torch.randn(B, N, D, device='cuda')
    dy = torch.randn(B, N, D, device='cuda')
    calls = []
    real = ops.stack_fwd
    ops.stack_fwd = lambda *a, **k: (calls.append(ops._FUSED_ATTN[0]), real(*a, **k))[1]

    def step():
        xi = x.clone().requires_grad_(True)
        with M.engine.precision('bf16'):
            y = run_blocks(blocks, xi)
            y.backward(dy)
        M.engine.join_wgrad_streams()
        for p in blocks.parameters():
            p.grad = None

    try:
        t = ab(step, args)
    finally:
        ops.stack_fwd = real
    assert calls and all(calls), 'the new route did not go through the stack composite, or the parent route did'
    se, sg = summary(t['tiled']), summary(t['gemm'])
    enc = dict(L=L, D=D, heads=heads, B=B, N=N, new_route='stack composite + tiled attention', parent_route='per-kernel blocks + GEMM attention',
               new=se, parent=sg, speedup=sg['median'] / se['median'], wins_beyond_spread=se['max'] < sg['min'])
    print(f"encoder L {L} B {B} N {N}: new {se['median'] * 1e3:.2f} ms [{se['min'] * 1e3:.2f}..{se['max'] * 1e3:.2f}]  parent {sg['median'] * 1e3:.2f} ms "
          f"[{sg['min'] * 1e3:.2f}..{sg['max'] * 1e3:.2f}]  x{enc['speedup']:.2f}", flush=True)
    res = dict(device=torch.cuda.get_device_name(0), window_s=args.window, repeats=args.repeats, quick=args.quick, peak_bf16_flops=PEAK_BF16,
               attention=rows, encoder=enc)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out + '.json', 'w') as f:
        json.dump(res, f, indent=1)
    with open(args.out + '.txt', 'w') as f:
        f.write(f"# tools/attn_tiled_ab.py on {res['device']}: tiled bf16 attention vs the batched-GEMM path, windows >= {args.window} s, {args.repeats} alternating repeats\n")
        f.write('# times in ms: median [min..max]; FLOPs algorithmic (4 B H N^2 hd forward, 10 backward); S/P bytes of the GEMM path are arithmetic from shapes\n')
        for r in rows:
            f.write(f"{r['shape']:6s} B={r['B']:<3d} H={r['H']:<2d} N={r['N']:<5d} hd={r['hd']} {r['direction']:8s} tiled {r['tiled']['median'] * 1e3:8.3f} "
                    f"[{r['tiled']['min'] * 1e3:.3f}..{r['tiled']['max'] * 1e3:.3f}]  gemm {r['gemm']['median'] * 1e3:8.3f} [{r['gemm']['min'] * 1e3:.3f}..{r['gemm']['max'] * 1e3:.3f}]  "
                    f"x{r['speedup']:.2f}  tiled {r['tiled_tflops']:.1f} TF/s ({100 * r['tiled_share_of_peak']:.1f} % of 2.5 PF/s)  gemm {r['gemm_tflops']:.1f} TF/s  "
                    f"gemm S+P traffic {r['gemm_S_P_bytes_arithmetic'] / 1e9:.2f} GB\n")
        f.write(f"encoder L={L} D={D} B={B} N={N} fwd+bwd: new {se['median'] * 1e3:.2f} [{se['min'] * 1e3:.2f}..{se['max'] * 1e3:.2f}]  "
                f"parent {sg['median'] * 1e3:.2f} [{sg['min'] * 1e3:.2f}..{sg['max'] * 1e3:.2f}]  x{enc['speedup']:.2f}\n")
    print('wrote', args.out + '.json')


if __name__ == '__main__':
    main()
