"""Bit fixture for every kernel that reads or differentiates the heads' LOW-RESOLUTION map (csrc/resize_map.h and its users in
convnext.hip, segloss.hip, regloss.hip) and for the fixed-order sums of clsrecipe.hip's soft-target cross-entropy:
tests/golden/lowres_bits.npz holds seeded inputs (generated on the CPU) and what the library built from the commit BEFORE the index
map, the gather walk and the reductions were written once returned for them on an MI355X.  tests/test_lowres_bits_gpu.py runs
run() below on the stored inputs and compares every output bit for bit, so the file is recorded once and not regenerated from
later code (MMAE_LIB selects the library, multimae_amd/_lib.py; pack() below is the layout of the outputs):

    MMAE_LIB=<the earlier build> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lowres_bits.py

Cases.  Geometries (h, w) -> (H, W) at B = 2, each in both modes: (5, 7) -> (13, 17) a non-integer upscale with every ox mod 4,
(5, 7) -> (10, 14) x2, (6, 5) -> (4, 3) a downscale (nearest leaves inputs unread), (1, 1) -> (3, 2) one pixel (i1 == i0), (4, 4) ->
(4, 4) the identity.  A full cross product of the variants below does not fit a small file (a 300 x 300 soft-CE case alone is
1 MB), so each variant is recorded where it can change the result:
  resize_fwd / resize_bwd   K = 3, ld = 8: every geometry and mode
  reg_loss_fwd / _bwd       all three kinds at every geometry and mode with (K = 3, K-channel mask) and (K = 1, 1-channel mask); the
                            other mask forms -- (K = 3, 1 channel), (K = 3, none), (K = 1, none) -- at (6, 5) -> (4, 3), the mask being
                            applied per output pixel whatever the geometry.  dx is pre-filled with NaN.  The stored difference does not
                            depend on the kind: it is recorded once and run() asserts that the three kinds agree
  depth_metrics             out[7] and acc[8] (pre-filled with 0.25) wherever K = 1 runs
  seg_ce_fwd / _bwd, seg_argmax (n_cls = K and K - 1)
                            K = 3 (ld = 8) at every geometry and mode; K = 70 (ld = 72: two 64-class chunks) at (5, 7) -> (13, 17) and
                            (1, 1) -> (3, 2), the class loop being the same at every geometry.  Targets hold ignore_index (255) and the
                            out-of-range classes 99 and -3
  soft_ce_fwd / _bwd        (B, K) = (3, 5) with dense / label targets and f32 / bf16 logits; (3, 300) -- a thread takes two classes --
                            dense f32 and label bf16; (300, 5) -- the finish kernel's strided pre-sum takes two rows -- dense bf16 and
                            label f32; ld = K + 3
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, 'lowres_bits.npz')

B, LD = 2, 8
GEOMS = (((5, 7), (13, 17)), ((5, 7), (10, 14)), ((6, 5), (4, 3)), ((1, 1), (3, 2)), ((4, 4), (4, 4)))
MODES = ('bilinear', 'nearest')
KINDS = ('l1', 'mse', 'berhu')
K70, LD70, GEOMS70 = 70, 72, (GEOMS[0], GEOMS[3])
ALL_MASKS = GEOMS[2]                                           # the geometry that also runs the remaining mask forms
IGNORE = 255
MEAN, STD = 2.5, 1.3
# (B, K, dense target?, bf16 logits?)
SOFT = ((3, 5, True, False), (3, 5, True, True), (3, 5, False, False), (3, 5, False, True), (3, 300, True, False), (3, 300, False, True),
        (300, 5, True, True), (300, 5, False, False))
SMOOTHING = 0.1
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def geom_tag(geom):
    (h, w), (H, W) = geom
    return f'{h}_{w}_{H}_{W}'


def labels(K, H, W, g):
    lab = torch.randint(0, K, (B, H, W), generator=g)
    r = torch.rand((B, H, W), generator=g)
    lab[r < 0.15] = IGNORE
    lab[(r >= 0.15) & (r < 0.22)] = 99
    lab[(r >= 0.22) & (r < 0.28)] = -3
    return lab


def make_inputs():
    """{name: numpy array}: everything run() reads, from one seeded CPU generator"""
    g = torch.Generator().manual_seed(20260)
    inp = {'up': torch.tensor([0.7])}
    for (h, w), (H, W) in GEOMS:
        inp.setdefault(f'x3_{h}_{w}', torch.randn((B, h, w, LD), generator=g))
        tag = geom_tag(((h, w), (H, W)))
        inp[f't_{tag}'] = torch.randn((B, 3, H, W), generator=g)           # the regression target, and resize_bwd's upstream gradient
        inp[f'mk_{tag}'] = torch.rand((B, 3, H, W), generator=g) > 0.3
        inp[f'lab3_{tag}'] = labels(3, H, W, g)
    for (h, w), (H, W) in GEOMS70:
        inp[f'x70_{h}_{w}'] = 2.0 * torch.randn((B, h, w, LD70), generator=g)
        inp[f'lab70_{geom_tag(((h, w), (H, W)))}'] = labels(K70, H, W, g)
    for Bs, K in sorted({(c[0], c[1]) for c in SOFT}):
        inp[f'sx_{Bs}_{K}'] = 3.0 * torch.randn((Bs, K + 3), generator=g)
        lab = torch.randint(0, K, (Bs,), generator=g)
        inp[f'sl_{Bs}_{K}'] = lab
        # a mixup target: two smoothed one-hot rows blended per sample
        one = torch.full((Bs, K), SMOOTHING / K).scatter_(1, lab[:, None], 1.0 - SMOOTHING + SMOOTHING / K)
        lam = torch.rand((Bs, 1), generator=g)
        inp[f'st_{Bs}_{K}'] = one * lam + one.flip(0) * (1.0 - lam)
    return {k: v.numpy() for k, v in inp.items()}


def reg_variants(geom):
    """(K, mask channels: 'K', '1' or None) run at a geometry"""
    v = [(3, 'K'), (1, '1')]
    return v + [(3, '1'), (3, None), (1, None)] if geom == ALL_MASKS else v


def run(inp, dev='cuda'):
    """{name: tensor}: every output of the cases above for the inputs `inp` ({name: numpy array})"""
    from multimae_amd import ops
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}
    up, out = t['up'], {}

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float('nan'), device=dev, dtype=dtype)

    def same_bits(a, b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))

    for geom in GEOMS:
        (h, w), (H, W) = geom
        tag, x = geom_tag(geom), t[f'x3_{h}_{w}']
        for mode in MODES:
            gm = f'{tag}_{mode}'
            out[f'resize_fwd_{gm}'] = ops.resize_fwd(x, LD, torch.empty((B, 3, H, W), device=dev), B, h, w, 3, H, W, mode)
            out[f'resize_bwd_{gm}'] = ops.resize_bwd(t[f't_{tag}'], nan(B, h, w, LD), LD, B, h, w, 3, H, W, mode)
            for K, mc in reg_variants(geom):
                v = f'{gm}_K{K}_m{mc}'
                tgt = t[f't_{tag}'][:, :K].contiguous()
                mask = None if mc is None else t[f'mk_{tag}'][:, :(K if mc == 'K' else 1)].contiguous()
                for kind in KINDS:
                    diff, o = ops.reg_loss_fwd(x, LD, tgt, mask, kind, B, h, w, K, H, W, mode)
                    assert same_bits(out.setdefault(f'reg_diff_{v}', diff), diff), (v, kind)
                    out[f'reg_out_{v}_{kind}'] = o
                    out[f'reg_dx_{v}_{kind}'] = ops.reg_loss_bwd(diff, o, up, kind, B, h, w, K, H, W, mode, nan(B, h, w, LD), LD)
                if K == 1:
                    acc = torch.full((8,), 0.25, device=dev)
                    out[f'depth_out_{v}'] = ops.depth_metrics(x, LD, tgt.abs() + 0.1, mask, MEAN, STD, B, h, w, H, W, mode, acc=acc)
                    out[f'depth_acc_{v}'] = acc
            for K, ld, xk in ((3, LD, x),) + (((K70, LD70, t.get(f'x70_{h}_{w}')),) if geom in GEOMS70 else ()):
                v, lab = f'{gm}_K{K}', t[f'lab{K}_{tag}']
                lse, o = ops.seg_ce_fwd(xk, ld, lab, IGNORE, B, h, w, K, H, W, mode)
                out[f'seg_lse_{v}'], out[f'seg_out_{v}'] = lse, o
                out[f'seg_dx_{v}'] = ops.seg_ce_bwd(xk, ld, lab, IGNORE, B, h, w, K, H, W, mode, lse, o, up, nan(B, h, w, ld))
                for n_cls in (K, K - 1):
                    pred = torch.full((B, H, W), -1, device=dev, dtype=torch.int64)
                    out[f'seg_argmax_{v}_n{n_cls}'] = ops.seg_argmax(xk, ld, pred, B, h, w, K, n_cls, H, W, mode)
    for Bs, K, dense, bf16 in SOFT:
        v = f'{Bs}_{K}_{"dense" if dense else "label"}_{"bf16" if bf16 else "f32"}'
        x = t[f'sx_{Bs}_{K}'].bfloat16() if bf16 else t[f'sx_{Bs}_{K}']
        target, lab, sm = (t[f'st_{Bs}_{K}'], None, 0.0) if dense else (None, t[f'sl_{Bs}_{K}'], SMOOTHING)
        lse, tsum, o = ops.soft_ce_fwd(x, K + 3, Bs, K, target, lab, sm)
        out[f'soft_lse_{v}'], out[f'soft_tsum_{v}'], out[f'soft_out_{v}'] = lse, tsum, o
        out[f'soft_dx_{v}'] = ops.soft_ce_bwd(x, K + 3, Bs, K, target, lab, sm, lse, tsum, up, nan(Bs, K + 3, dtype=x.dtype))
    torch.cuda.synchronize()
    return out


def bits(v):
    """a result as the integer tensor of its bits, on the CPU"""
    v = v.contiguous()
    return (v.view(INT_VIEW[v.dtype]) if v.dtype in INT_VIEW else v).cpu()


def pack(res):
    """(index, {integer type: flat tensor}): the results' bits concatenated in name order, index = [[name, integer type, shape]] --
    one archive member per type instead of one per result (some 300 members' headers were a fifth of the file)"""
    index, flat = [], {}
    for k in sorted(res):
        b = bits(res[k])
        d = str(b.dtype).split('.')[1]
        index.append([k, d, list(b.shape)])
        flat.setdefault(d, []).append(b.reshape(-1))
    return index, {d: torch.cat(v) for d, v in flat.items()}


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    inp = make_inputs()
    res = run(inp)
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    index, flat = pack(res)
    np.savez_compressed(path, out_index=np.array(json.dumps(index)), **{'in_' + k: v for k, v in inp.items()},
                        **{'out_' + d: v.numpy() for d, v in flat.items()})
    print(f'wrote {path}: {len(inp)} inputs, {len(res)} outputs, {os.path.getsize(path)} bytes')
