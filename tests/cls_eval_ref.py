"""fp64 reference, error bounds and the rank rule of the classification evaluation (csrc/clseval.hip), shared by
tests/test_cls_eval_cpu.py and tests/test_cls_eval_gpu.py.

Bounds: the row kernel computes the log-sum-exp with soft_ce_fwd's per-thread recurrence, wave xor tree and wave-order merge, so the
derivation in tests/test_cls_recipe_gpu.py's module docstring holds with a one-hot target (t_k exact: e_t = 0); FMA contraction, which
this file's build allows, only removes roundings.  u = 2^-24, n_t = ceil(K / 256):
    r_s   = gamma_(n_t + 8) + 2 u + 3 u (n_t + 1) + 4 u range
    b_lse = 1.01 r_s + 2 u |lse - max| + u |lse|
    nll   = lse - z_t, one subtraction:            b_nll = b_lse + u |lse - z_t|
    row   (the docstring's row bound, sum_k |t_k| = 1):  b_row = b_lse + (gamma_(n_t + 8) + 2 u) |lse - z_t|
    loss  the valid rows summed and divided by their number in double, rounded to f32 once:  mean(b_row) + 2 u |loss|
Two f32 evaluations of the same fp64 value (the kernel or the eager restatement against the reference's f32 run in the golden file)
agree within the sum of their bounds: 2 b.

The rank rule (mmae.h): rank = #{k: z_k > z_t} + #{k < t: z_k == z_t}, K for a target outside [0, K); a row is correct at k iff
rank < min(k, K).  Restated here with comparisons on the exact values -- integers, so the check is equality.  The percentages are the
f32 operations of utils/metrics.py:38, fl(fl(c 100) / B), restated in numpy float32.
"""
import numpy as np
import torch

from helpers import gamma

U = 2.0 ** -24


def rank_ref(xr: torch.Tensor, target: torch.Tensor):
    """(valid bool [B], rank int64 [B]) on the logits as read (any float dtype; compared exactly)"""
    B, K = xr.shape
    t = target.to(xr.device).long()
    valid = (t >= 0) & (t < K)
    rank = torch.full((B,), K, dtype=torch.int64, device=xr.device)
    for b in range(B):
        if bool(valid[b]):
            tb = int(t[b])
            zt = xr[b, tb]
            rank[b] = int((xr[b] > zt).sum()) + int((xr[b, :tb] == zt).sum())
    return valid, rank


def pct(c: int, B: int) -> np.float32:
    return np.float32(np.float32(np.float32(c) * np.float32(100.0)) / np.float32(B))


def cls_eval_ref(xr: torch.Tensor, target: torch.Tensor, ks):
    """xr fp64 [B, K]: the logits as the kernel reads them.  Returns lse / nll with bounds (nll 0 with bound 0 on an invalid row),
    rank, valid, loss with bound (0, 0 without a valid row), the counts and the expected f32 percentages."""
    xr = xr.double()
    B, K = xr.shape
    n_t = (K + 255) // 256
    valid, rank = rank_ref(xr, target)
    tc = target.to(xr.device).long().clamp(0, K - 1)
    zt = xr.gather(1, tc[:, None]).squeeze(1)
    lse = torch.logsumexp(xr, 1)
    mx, rng = xr.amax(1), xr.amax(1) - xr.amin(1)
    r_s = gamma(n_t + 8) + 2 * U + 3 * U * (n_t + 1) + 4 * U * rng
    b_lse = 1.01 * r_s + 2 * U * (lse - mx).abs() + U * lse.abs()
    zero = torch.zeros_like(lse)
    nll = torch.where(valid, lse - zt, zero)
    b_nll = torch.where(valid, b_lse + U * (lse - zt).abs(), zero)
    b_row = torch.where(valid, b_lse + (gamma(n_t + 8) + 2 * U) * (lse - zt).abs(), zero)
    nv = int(valid.sum())
    loss = float(nll.sum()) / nv if nv else 0.0
    b_loss = float(b_row.sum()) / nv + 2 * U * abs(loss) if nv else 0.0
    counts = [int((rank < min(int(k), K)).sum()) for k in ks]
    return dict(lse=lse, b_lse=b_lse, nll=nll, b_nll=b_nll, rank=rank, valid=valid, loss=loss, b_loss=b_loss, counts=counts,
                acc=np.array([pct(c, B) for c in counts], dtype=np.float32), n_valid=nv)
