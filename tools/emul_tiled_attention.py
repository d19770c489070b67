"""CPU emulation (fp32 torch) of tiled attention with online softmax, checked against tests/helpers.attention_bounds.
Run from the repository root (no GPU needed):  python tools/emul_tiled_attention.py [--delta-from-o]
It emulates the algorithm of attention.hip's tiled kernels: key tiles of 64 / 128 / 256 with the online rescale, P and dS rounded to bf16 before their
products, delta from fp32 P . dP, query tiles of 128 for dK / dV.  Worst error / bound: o 0.53, lse 0.03, dq 0.32, dk 0.38, dv 0.43, no violations.
--delta-from-o: the flash shortcut delta = rowsum(dO . O_bf16) instead of the sweep over fp32 P . dP (it breaks the dq / dk bounds)."""
import os, sys, math, torch
ALT = '--delta-from-o' in sys.argv
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ('', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, d))
from helpers import attention_bounds
torch.manual_seed(0)
bf = lambda t: t.to(torch.bfloat16).float()
LOG2E = 1.4426950408889634


def tiled(q, k, v, do, scale, KT, QT):
    Z, Nq, hd = q.shape
    Nk = k.shape[1]
    c = torch.tensor(scale * LOG2E, dtype=torch.float32)
    m = torch.full((Z, Nq), -float('inf')); l = torch.zeros(Z, Nq); O = torch.zeros(Z, Nq, hd)
    for j in range(0, Nk, KT):
        s = (q @ k[:, j:j + KT].transpose(-1, -2)) * c
        mn = torch.maximum(m, s.amax(-1))
        a = torch.exp2(m - mn)
        p = torch.exp2(s - mn[..., None])
        l = l * a + p.sum(-1)
        O = O * a[..., None] + bf(p) @ v[:, j:j + KT]
        m = mn
    o = bf(O / l[..., None])
    lse = m * 0.69314718056 + torch.log(l)
    # backward: P recomputed from lse; delta sweep in fp32 from own P, dP
    P = torch.exp2((q @ k.transpose(-1, -2)) * c - (lse * LOG2E)[..., None])
    dP = do @ v.transpose(-1, -2)
    delta = torch.zeros(Z, Nq)
    for j in range(0, Nk, KT):
        delta = delta + (P[..., j:j + KT] * dP[..., j:j + KT]).sum(-1)
    if ALT:
        delta = (do * o).sum(-1)
    dS = bf(P * (dP - delta[..., None]))
    dq = torch.zeros(Z, Nq, hd)
    for j in range(0, Nk, KT):
        dq = dq + dS[..., j:j + KT] @ k[:, j:j + KT]
    dq = bf(dq * scale)
    dk = torch.zeros(Z, Nk, hd); dv = torch.zeros(Z, Nk, hd)
    for i in range(0, Nq, QT):
        dk = dk + dS[:, i:i + QT].transpose(-1, -2) @ q[:, i:i + QT]
        dv = dv + bf(P[:, i:i + QT]).transpose(-1, -2) @ do[:, i:i + QT]
    return dict(o=o, lse=lse, dq=dq, dk=bf(dk * scale), dv=bf(dv))


for (Z, Nq, Nk, hd, qs) in [(2, 257, 257, 64, 1), (2, 1025, 1025, 64, 2), (1, 3201, 3201, 64, 2), (2, 300, 1025, 32, 2), (1, 1025, 1025, 64, 4)]:
    q, k = bf(torch.randn(Z, Nq, hd) * qs), bf(torch.randn(Z, Nk, hd) * qs)
    v, do = bf(torch.randn(Z, Nk, hd)), bf(torch.randn(Z, Nq, hd))
    sc = hd ** -0.5
    r = attention_bounds(q, k, v, do, sc, u_in=0.0, u_p=2.0 ** -8, out_dtype=torch.bfloat16)
    for KT in (64, 128, 256):
        got = tiled(q, k, v, do, sc, KT, 128)
        line = []
        for n in ('o', 'lse', 'dq', 'dk', 'dv'):
            ref, bd = r[n]
            err = (got[n].double() - ref).abs()
            line.append(f'{n} max err/bound {float((err / bd).max()):.3f} viol {int((err > bd).sum())}')
        print((Z, Nq, Nk, hd, qs), 'KT', KT, ' | '.join(line), flush=True)
