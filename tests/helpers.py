"""Shared test helpers: golden loading, model builders for the engine and the oracle config."""
import json
import math
import os

import numpy as np
import torch

import multimae_oracle as orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_mini():
    z = np.load(os.path.join(GOLD, 'mini_fwd_bwd.npz'))
    g = lambda pre: {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    out = dict(sd=g('sd/'), grad=g('grad/'), x=g('x/'), pred=g('pred/'), loss={k: float(v) for k, v in g('loss/').items()},
               noise=g('noise/'), mask=g('mask/'))
    for k in ('dirichlet', 'noise_all', 'ids_keep', 'ids_restore', 'enc_in', 'enc_out'):
        out[k] = torch.from_numpy(z[k])
    return out


def load_masks_base():
    z = np.load(os.path.join(GOLD, 'masks_base.npz'))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def load_scalars():
    with open(os.path.join(GOLD, 'scalars.json')) as f:
        return json.load(f)


MINI = dict(doms=['rgb', 'depth', 'semseg'], P=8, S=32, B=3, nvis=12, dim=128, depth=2, heads=2, dec_dim=64, dec_depth=1,
            dec_heads=2, class_emb=16)


def mini_oracle_cfg():
    m = MINI
    return orc.standard_config(m['doms'], patch_size=m['P'], image_size=m['S'], dim_tokens=m['dim'], depth=m['depth'],
                               num_heads=m['heads'], dec_dim=m['dec_dim'], dec_depth=m['dec_depth'], dec_heads=m['dec_heads'],
                               dim_class_emb=m['class_emb'])


def build_engine_model(doms, P, S, *, enc=None, dec_dim=256, dec_depth=2, dec_heads=8, class_emb=64, posemb_size=None,
                       factory='pretrain_multimae_base', learnable_pos=False):
    """Engine model built with the same call sequence as tests/golden/make_golden.py::build_ref."""
    import multimae_amd as M
    from functools import partial
    from torch import nn
    Sg = posemb_size or S
    ins = {}
    for d in doms:
        if d == 'semseg':
            ins[d] = M.SemSegInputAdapter(num_classes=133, dim_class_emb=class_emb, interpolate_class_emb=False, stride_level=4,
                                          patch_size_full=P, image_size=Sg, learnable_pos_emb=learnable_pos)
        else:
            ins[d] = M.PatchedInputAdapter(num_channels=3 if d == 'rgb' else 1, stride_level=1, patch_size_full=P, image_size=Sg,
                                           learnable_pos_emb=learnable_pos)
    outs = {}
    for key, task in [(d, d) for d in doms] + ([('norm_rgb', 'rgb')] if 'rgb' in doms else []):
        ch = {'rgb': 3, 'depth': 1, 'semseg': 133}[task]
        outs[key] = M.SpatialOutputAdapter(num_channels=ch, stride_level=4 if task == 'semseg' else 1, patch_size_full=P,
                                           dim_tokens=dec_dim, depth=dec_depth, num_heads=dec_heads, use_task_queries=True,
                                           task=task, context_tasks=list(doms), use_xattn=True, image_size=Sg)
    if enc is None:
        return M.create_model(factory, input_adapters=ins, output_adapters=outs, num_global_tokens=1, drop_path_rate=0.0).train()
    return M.MultiMAE(ins, outs, num_global_tokens=1, dim_tokens=enc[0], depth=enc[1], num_heads=enc[2], mlp_ratio=4,
                      qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)).train()


def build_mini_engine(learnable_pos=False):
    m = MINI
    return build_engine_model(m['doms'], m['P'], m['S'], enc=(m['dim'], m['depth'], m['heads']), dec_dim=m['dec_dim'],
                              dec_depth=m['dec_depth'], dec_heads=m['dec_heads'], class_emb=m['class_emb'], learnable_pos=learnable_pos)


def make_inputs(doms, B, S):
    x = {}
    if 'rgb' in doms:
        x['rgb'] = torch.randn(B, 3, S, S)
    if 'depth' in doms:
        x['depth'] = torch.randn(B, 1, S, S)
    if 'semseg' in doms:
        x['semseg'] = torch.randint(0, 133, (B, S // 4, S // 4))
    return x


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ----------------------------------------------------------------------------------------------
# Element-wise checks.  rel_err is one number over the whole output: an error confined to a tile tail, one row or one element
# drowns in a norm over a million elements (tests/test_check_helpers_cpu.py records cases it passes).  The helpers below bound
# every element on its own, in fp64, and guard the memory around an output.

# significand bits (hidden bit included) and the smallest normal exponent of each storage format
_FMT = {torch.bfloat16: (8, -126), torch.float16: (11, -14), torch.float32: (24, -126)}


def unit_roundoff(dtype) -> float:
    """u = 2^-p: round-to-nearest into `dtype` moves a value by at most u times its magnitude (normal range)."""
    return 2.0 ** -_FMT[dtype][0]


def gamma(n, u: float = 2.0 ** -24) -> float:
    """gamma_n = n u / (1 - n u): bound on the relative error of any order of summation of n terms (Higham, Accuracy and Stability
    of Numerical Algorithms, Lemma 3.1) -- with u = 2^-24 the fp32 accumulation every kernel here does."""
    return n * u / (1.0 - n * u)


def ulp(dtype, x):
    """Spacing of `dtype` numbers at |x| (fp64 tensor of x's shape): 2^(e - p + 1) with e = floor(log2 |x|), clamped to the
    subnormal spacing below the normal range.  A rounding to nearest moves a value by at most half of it."""
    p, emin = _FMT[dtype]
    x = torch.as_tensor(x).double().abs()
    e = torch.floor(torch.log2(x.clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.exp2(e - (p - 1))


def prod_bound(absA, absB, K: int, out_dtype=None, ref=None, u_op: float = 0.0, extra=None):
    """Element-wise error bound of C = A . B^T [M, K] x [N, K] computed with fp32 accumulation and stored as `out_dtype`:
        gamma_K (|A| |B|^T)          any summation order of K exact products in fp32 (split-K slabs and their sum included)
      + u_op (|A| |B|^T)             operands rounded inside the product (split-bf16 / fp16 operands; 0 when they are exact)
      + extra                        caller's epilogue terms (already an absolute bound)
      + ulp(out_dtype, |ref| + all)  the final rounding (half an ulp at the computed value <= one ulp at the reference's)
    absA [M, K], absB [N, K] non-negative; computed in fp64 on their device."""
    t = absA.double() @ absB.double().t()
    b = (gamma(K) + u_op) * t
    if extra is not None:
        b = b + extra
    if out_dtype is not None and ref is not None:
        b = b + ulp(out_dtype, ref.double().abs() + b)
    return b


def _fmt_index(idx, names):
    if names is None:
        return str(tuple(idx))
    return '(' + ', '.join(f'{n}={i}' for n, i in zip(names, idx)) + ')'


def assert_within(out, ref, bound, what: str, names=None):
    """|out - ref| <= bound element by element, in fp64 (a NaN / inf in out is a violation).  On failure: how many elements
    violate the bound, the worst one (largest |out - ref| / bound) by index -- (row, col), or (b, h, q, d) with names=('b', 'h',
    'q', 'd') -- with its value, reference and bound."""
    o = out.detach().double()
    r = ref.detach().double().to(o.device)
    bd = torch.as_tensor(bound).double().to(o.device).expand_as(r)
    err = (o - r).abs()
    bad = ~(err <= bd)
    n = int(bad.sum())
    if n == 0:
        return
    ratio = torch.where(torch.isfinite(err), err / bd.clamp_min(1e-300), torch.full_like(err, float('inf')))
    ratio = torch.where(bad, ratio, torch.zeros_like(ratio))
    flat = int(torch.argmax(torch.nan_to_num(ratio, nan=float('inf'))))
    idx = np.unravel_index(flat, tuple(r.shape))
    raise AssertionError(f'{what}: {n} of {r.numel()} elements outside the bound; worst at {_fmt_index(idx, names)}: '
                         f'value {float(o.reshape(-1)[flat])!r}, reference {float(r.reshape(-1)[flat])!r}, bound {float(bd.reshape(-1)[flat]):.3e}')


# ----------------------------------------------------------------------------------------------
# Guarded outputs and poisoned operands
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# the sentinel: bytes a5 ff repeated -- a NaN as bf16 / fp16 (0xffa5) and as f32 (0xffa5ffa5); as an int64 output (8-byte elements: the
# mask sampler's ids) a large negative number no index or mask value can equal
_SENT = {2: -91, 4: -5898331, 8: 0xffa5ffa5ffa5ffa5 - 2 ** 64}      # int16 0xffa5, int32 0xffa5ffa5, int64 0xffa5ffa5ffa5ffa5


class Guarded:
    """One flat allocation that holds the logical [rows][cols] view with leading dimension ld >= cols, `guard` elements of
    guard zone before it and after it.  Every element outside the view holds a fixed sentinel bit pattern (a NaN in every
    float format here); intact() asserts that all of them still do, bit for bit.  Pass `flat` with element offset `off` (or
    `full` / `view`, which start at the view) to the code under test.  `shift` elements are left unused in front of it all: the
    allocator's alignment (and guard % 8 == 0) puts the view on a 16-byte boundary, a shift takes it off again."""

    def __init__(self, rows: int, cols: int, ld: int, dtype, device, guard: int = 64, fill=None, shift: int = 0):
        assert ld >= cols and guard % 8 == 0 and ld > 0
        self.rows, self.cols, self.ld, self.dtype, self.off = rows, cols, ld, dtype, guard
        self.esz = torch.empty((), dtype=dtype).element_size()
        n = guard + rows * ld + guard
        self.flat = torch.empty((n + shift,), dtype=dtype, device=device)[shift:]
        self._bits().fill_(_SENT[self.esz])
        self.full = self.flat[guard:guard + rows * ld].view(rows, ld)
        self.view = self.full[:, :cols]
        if fill is not None:
            self.view.copy_(fill)
        m = torch.ones((n,), dtype=torch.bool, device=device)
        m[guard:guard + rows * ld].view(rows, ld)[:, :cols] = False
        self._outside = m

    def _bits(self):
        return self.flat.view(_INT_OF[self.esz])

    def intact(self, what: str = 'guarded buffer'):
        bits = self._bits()
        bad = self._outside & (bits != _SENT[self.esz])
        n = int(bad.sum())
        if n:
            i = int(torch.nonzero(bad)[0])
            if i < self.off:
                where = f'guard zone before the view, element {i - self.off}'
            elif i >= self.off + self.rows * self.ld:
                where = f'guard zone after the view, element {i - self.off - self.rows * self.ld}'
            else:
                where = f'(row {(i - self.off) // self.ld}, col {(i - self.off) % self.ld}) of the ld padding'
            raise AssertionError(f'{what}: {n} element(s) outside the [{self.rows}][{self.cols}] view (ld {self.ld}) were written; '
                                 f'first at {where}')


def byte_slab(nbytes: int, device, guard: int = 64):
    """A guarded slab of exactly nbytes bytes (a multiple of 4) for the library's byte-carved slabs: f32 elements, so that the guard
    zones (64 elements = 256 bytes) keep the 256-byte alignment the carving assumes and start at the first byte past the slab."""
    assert nbytes % 4 == 0 and nbytes > 0
    return Guarded(1, nbytes // 4, nbytes // 4, torch.float32, device, guard=guard)


def assert_untouched(g: 'Guarded', what: str):
    """every element of a Guarded buffer allocated without `fill` -- the view included -- still holds the sentinel"""
    n = int((g._bits() != _SENT[g.esz]).sum())
    assert n == 0, f'{what}: {n} element(s) were written although the call was refused'


def same_bits(a, b) -> bool:
    """bit-for-bit equality of two tensors of one dtype and shape (NaN payloads and the sign of zero included)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    it = _INT_OF[a.element_size()]
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def poisoned(X, ld: int, dtype, device, *, finite_to: int = 0, junk: float = 0.0, col0: int = 8, nan_rows: int = 8):
    """X [rows][cols] placed at column `col0` of a flat buffer with row stride ld (returns (flat, offset of X[0][0], ld)).  Columns
    cols .. finite_to hold `junk` (finite, the bytes a kernel may read past a ragged contraction edge: mmae.h's bf16 rule rounds
    reads up to the next multiple of 8 along k), every other element of the buffer -- the rest of the ld padding, the col0 columns
    in front of each row, nan_rows rows after the last one and ld elements before the first -- is NaN."""
    rows, cols = X.shape
    assert col0 + max(cols, finite_to) <= ld
    flat = torch.full(((rows + nan_rows + 1) * ld,), float('nan'), dtype=dtype, device=device)
    off = ld + col0
    v = flat[ld:ld + rows * ld].view(rows, ld)
    v[:, col0:col0 + cols] = X.to(device=device, dtype=dtype)
    if finite_to > cols:
        v[:, col0 + cols:col0 + finite_to] = junk
    return flat, off


def attention_bounds(q, k, v, do, scale: float, *, u_in: float, u_p: float, out_dtype, grad_dtype=None, eta_p: float = 0.0,
                     eta_ds: float = 0.0):
    """fp64 references and element-wise error bounds of one attention forward (o, lse) and backward (dq, dk, dv) on the operands
    exactly as the kernel sees them: q, do [Z, Nq, hd], k, v [Z, Nk, hd] (Z = batch x heads).
      u_in  relative error of ONE product of two operands inside the kernel's matrix products (0 for bf16 / fp16 operands, which
            multiply exactly into fp32; the caller states it for split or rounded f32 operands)
      u_p   unit roundoff of the type P -- and in the backward dS -- is rounded to before its product (attention.hip: 'P and dS right
            before their MFMA'; the GEMM path stores P / dS in the activation type)
      eta_p, eta_ds  the absolute floor of that rounding for P (<= 1) and dS: fp16 flushes below its smallest subnormal, so a rounding
            moves x by u |x| + 2^-25 (x in the units the kernel rounds in); 0 for bf16 / f32, whose range reaches e^-88
    Derivation (fp32 accumulation everywhere, gamma_n as in gamma()):
      scores  |ds_ij| <= e_i = (u_in + gamma_hd + 4 * 2^-24) * scale * max_j |q_i| . |k_j|   (products + sum + scale / log2 e multiplies)
      P       every score of row i moves by <= e_i, so softmax entries move by a factor within exp(+-2 e_i); the normaliser's fp32 sum adds
              gamma_Nk, v_exp_f32 2^-22:  rho_i = exp(2 e_i) - 1 + gamma_Nk + 2^-22
      o       |do_| <= (rho_i + u_p + u_in + gamma_Nk) (P |V|) + eta_p sum_j |V_j| + ulp(out_dtype)
      lse     |dlse| <= e_i + gamma_Nk + 8 ulp_f32(|lse| + 1)   (max * ln 2 and __logf in fp32)
      bwd P   recomputed from the stored lse and read rounded by the GEMM path's softmax backward:
              rb_i = exp(2 e_i + dlse_i) - 1 + u_p + 2^-22
      dP      |ddP_ij| <= (u_in + gamma_hd) |dO_i| . |V_j| = EdP_ij;   delta_i = sum_j P_ij dP_ij:
              |ddelta_i| <= sum_j P_ij (rb_i |dP_ij| + EdP_ij) + gamma_Nk sum_j P_ij |dP_ij|
      dS      |ddS_ij| <= (rb_i P_ij + eta_p) |dP_ij - delta_i| + P_ij (EdP_ij + |ddelta_i|), then rounded: + u_p (|dS_ij| + that) + eta_ds
      dq      scale (EdS |K| + (u_in + gamma_Nk) (|dS| + EdS) |K|) + ulp(grad_dtype);  dk the same with dS^T, Q
      dv      ((rb_i + u_p + u_in + gamma_Nq) P + eta_p)^T |dO| + ulp(grad_dtype)"""
    grad_dtype = grad_dtype or out_dtype
    q, k, v, do = (t.double() for t in (q, k, v, do))
    Nq, hd = q.shape[-2:]
    Nk = k.shape[-2]
    u32 = 2.0 ** -24
    s = scale * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    qk = q.abs() @ k.abs().transpose(-1, -2)
    e = (u_in + gamma(hd) + 4 * u32) * scale * qk.amax(-1)                   # [Z, Nq]
    rho = torch.expm1(2 * e) + gamma(Nk) + 2.0 ** -22
    o = P @ v
    pv = P @ v.abs()
    b_o = (rho + u_p + u_in + gamma(Nk))[..., None] * pv + eta_p * v.abs().sum(-2, keepdim=True)
    b_o = b_o + ulp(out_dtype, o.abs() + b_o)
    b_lse = e + gamma(Nk) + 8 * ulp(torch.float32, lse.abs() + 1)
    dP = do @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1)
    dS = P * (dP - delta[..., None])
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-1, -2) @ q)
    dv = P.transpose(-1, -2) @ do
    rb = (torch.expm1(2 * e + b_lse) + u_p + 2.0 ** -22)[..., None]
    EdP = (u_in + gamma(hd)) * (do.abs() @ v.abs().transpose(-1, -2))
    Ed = (P * (rb * dP.abs() + EdP)).sum(-1) + gamma(Nk) * (P * dP.abs()).sum(-1)
    EdS = (rb * P + eta_p) * (dP - delta[..., None]).abs() + P * (EdP + Ed[..., None])
    EdS = EdS + u_p * (dS.abs() + EdS) + eta_ds
    aS = dS.abs() + EdS
    b_dq = scale * (EdS @ k.abs() + (u_in + gamma(Nk)) * (aS @ k.abs()))
    b_dk = scale * (EdS.transpose(-1, -2) @ q.abs() + (u_in + gamma(Nq)) * (aS.transpose(-1, -2) @ q.abs()))
    b_dv = ((rb + u_p + u_in + gamma(Nq)) * P + eta_p).transpose(-1, -2) @ do.abs()
    b_dq = b_dq + ulp(grad_dtype, dq.abs() + b_dq)
    b_dk = b_dk + ulp(grad_dtype, dk.abs() + b_dk)
    b_dv = b_dv + ulp(grad_dtype, dv.abs() + b_dv)
    return dict(o=(o, b_o), lse=(lse, b_lse), dq=(dq, b_dq), dk=(dk, b_dk), dv=(dv, b_dv), P=P)


# ----------------------------------------------------------------------------------------------
# Masked losses (losses.hip): fp64 references with element-wise bounds, shared by the image- and patch-domain tests and the helper
# self-tests.  The kernels' rounding points, u = 2^-24, device expf / logf taken as <= 1 ulp (<= 2u relative):
#   counts     exact (integers below 2^24)
#   norm_pix   mu = fp32 sum / nval:              |dmu| <= (gamma_nval + u) mean|t| = e_mu
#              var = fp32 sum of (t - mu^)^2 / (nval - 1): |dvar| <= (gamma_nval + 4u)(var + k e_mu^2) + k e_mu^2 + u 1e-6,
#              k = nval / (nval - 1) (the shift by mu^ - mu adds k dmu^2; the fp32 constant 1e-6f is 1e-6 within u)
#              rs = 1 / sqrtf(var + 1e-6):       |drs| / rs <= 0.51 |dvar| / (var + 1e-6) + 3u = r_rs   (first order, 2 % slack)
#   residual   d = p - (t - mu^) rs^:            |dd| <= e_mu rs (1 + r_rs) + |t - mu| rs (r_rs + 2u) + u (|d| + that)  (u |d| alone
#              without norm_pix)
#   error      MSE: |d^2 - d^^2| <= 2 |d| dd + dd^2 + u d^2;  L1: dd
#   sums       fp32 over the n masked elements of a sample, the split partials and the /C:  + (gamma_(n + 16) + u) sum|e|
#   loss       sum_b s_b / c_b (fp32), / nvalid:  sum_b ds_b / c_b + (gamma_(B + 8) + 2u) sum_b s_b / c_b, / nvalid
#   weight     w_b = up / (nvalid c_b C) in fp32 (two products and a division): |dw| <= 4u |w|
#   gradient   MSE: g = w 2 d:  |dg| <= 2 |w| dd + 6u |g|;  L1: g = w sign(d^) -- exact unless |d| <= dd, then any of {-w, 0, +w}
#   CE lse     online max + rescaled fp32 sum of C exps, each exp's argument rounded (u |v - mx| <= u range, the rescales' arguments
#              add up to at most the range), every rescale one more expf and product (3u; n_r rescales: the records of the running maximum
#              in the image domain, the lane's groups of eight plus two per slot combination on patch rows):
#              |ds| / s <= gamma_(C + 8) + 2u + 3u n_r + 4u range = r_s;  lse = mx + logf(s): |dlse| <= 1.01 r_s + 2u |log s| + u |lse|
#   CE nll     ls - l_t (+ eps (ls - sx / C), sx an fp32 sum of C logits):  per pixel
#              (1 - eps)(dlse + u nll) + eps (dlse + (gamma_C sum|l| + u |sx|) / C + u |ls - sx / C|) + 3u |contrib|
#   CE grad    p^ = expf(l - lse^): |dp| <= p (exp(dlse + u |l - lse|) - 1 + 2u);  g = w (p - y):  |dg| <= |w| (dp + u |p - y| + u) + 5u |g|
U32 = 2.0 ** -24


def _img_rows(x, P):
    """[B, C, H, W] -> [B, nh*nw, C*P*P] patch rows (column order c, i, j), the adapters' out_proj layout."""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // P) * (W // P), C * P * P)


def _rows_img(r, C, H, W, P):
    B = r.shape[0]
    return r.reshape(B, H // P, W // P, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def _finish(s, bs, cnt, B, up):
    """per-sample (sum, its bound), counts -> loss, its bound, nvalid, the fp64 weights up / (nvalid c_b)."""
    valid = cnt > 0
    nvalid = int(valid.sum())
    q = torch.where(valid, s / cnt.clamp_min(1), torch.zeros_like(s))
    dq = torch.where(valid, bs / cnt.clamp_min(1), torch.zeros_like(s))
    loss = float(q.sum()) / nvalid if nvalid else 0.0
    bl = (float(dq.sum()) + (gamma(B + 8) + 2 * U32) * float(q.abs().sum())) / nvalid if nvalid else 0.0
    w = torch.where(valid, up / (max(nvalid, 1) * cnt.clamp_min(1)), torch.zeros_like(s))
    return loss, bl, nvalid, w


def pixel_loss_ref(kind: int, norm_pix: bool, pred, target, mask, P: int, up: float = 1.0):
    """fp64 reference and bounds of mmae_masked_pixel_loss_* (kind 0 MSE, 1 L1) on pred / target [B, C, H, W] (any device), mask [B, nh*nw].
    Returns a dict: mean / rstd [B, np] with bounds (norm_pix), sum [B] with bound, cnt [B] (exact), loss / nvalid, and the gradient
    g [B, C, H, W] with bound bg; for L1 `amb` marks the elements whose sign the kernel may round either way."""
    p, t = pred.double(), target.double()
    B, C, H, W = t.shape
    nval = C * P * P
    m = mask.to(p.device).bool()
    tr = _img_rows(t, P)
    out = {}
    if norm_pix:
        mu = tr.mean(-1)
        var = tr.var(-1)
        rs = 1.0 / torch.sqrt(var + 1e-6)
        e_mu = (gamma(nval) + U32) * tr.abs().mean(-1)
        k = nval / (nval - 1)
        dvar = (gamma(nval) + 4 * U32) * (var + k * e_mu ** 2) + k * e_mu ** 2 + U32 * 1e-6
        r_rs = 0.51 * dvar / (var + 1e-6) + 3 * U32
        out.update(mean=(mu, e_mu), rstd=(rs, r_rs * rs))
        tn = (tr - mu[..., None]) * rs[..., None]
        et = e_mu[..., None] * rs[..., None] * (1 + r_rs[..., None]) + (tr - mu[..., None]).abs() * rs[..., None] * (r_rs[..., None] + 2 * U32)
        tn, et = _rows_img(tn, C, H, W, P), _rows_img(et, C, H, W, P)
    else:
        tn, et = t, torch.zeros_like(t)
    d = p - tn
    dd = et + U32 * (d.abs() + et)
    if kind == 0:
        e, de = d * d, 2 * d.abs() * dd + dd * dd + U32 * d * d
    else:
        e, de = d.abs(), dd
    mi = m.reshape(B, H // P, W // P).repeat_interleave(P, 1).repeat_interleave(P, 2)[:, None].expand(B, C, H, W)
    e, de = e * mi, de * mi
    n = mi.flatten(1).sum(1).double()
    s = e.flatten(1).sum(1) / C
    bs = (de.flatten(1).sum(1) + (gamma(int(n.max()) + 16) + U32) * e.flatten(1).sum(1)) / C
    cnt = m.sum(1).double() * P * P
    loss, bl, nvalid, w = _finish(s, bs, cnt, B, up)
    wc = (w / C)[:, None, None, None]
    if kind == 0:
        g = wc * 2 * d * mi
        bg = (2 * wc.abs() * dd + 6 * U32 * g.abs()) * mi
        amb = torch.zeros_like(mi)
    else:
        g = wc * torch.sign(d) * mi
        bg = 6 * U32 * g.abs()
        amb = mi & (d.abs() <= dd)
    out.update(sum=(s, bs), cnt=cnt, loss=(loss, bl), nvalid=nvalid, g=g, bg=bg, amb=amb, w=wc * mi)
    return out


def ce_loss_ref(logits, target, mask, P: int, eps: float, up: float = 1.0, n_rescale=None):
    """fp64 reference and bounds of mmae_masked_ce_* on logits [B, C, H, W], target [B, H, W] (outside [0, C): ignored, as
    F.cross_entropy's ignore_index; the pixel still counts), mask [B, nh*nw].  Returns lse [B, H, W] with bound, sum [B] with bound,
    cnt [B] (exact), loss / nvalid, the gradient g [B, C, H, W] with bound bg, and w (the weight per sample)."""
    l = logits.double()
    B, C, H, W = l.shape
    tg = target.to(l.device)
    ok = (tg >= 0) & (tg < C)
    mi = mask.to(l.device).bool().reshape(B, H // P, W // P).repeat_interleave(P, 1).repeat_interleave(P, 2)
    mx = l.amax(1)
    rng = mx - l.amin(1)
    lse = torch.logsumexp(l, 1)
    if n_rescale is None:                             # image domain: a rescale needs a new running maximum -- at most the records of the row
        cm = torch.cummax(l, 1).values
        n_rescale = (l[:, 1:] > cm[:, :-1]).sum(1).double() + 1
    r_s = gamma(C + 8) + 2 * U32 + 3 * U32 * n_rescale + 4 * U32 * rng
    b_lse = 1.01 * r_s + 2 * U32 * (lse - mx).abs() + U32 * lse.abs()
    lt = torch.gather(l, 1, torch.where(ok, tg, torch.zeros_like(tg))[:, None]).squeeze(1)
    nll = lse - lt
    mean_l = l.mean(1)
    sm = lse - mean_l
    contrib = (1 - eps) * nll + eps * sm
    e_c = ((1 - eps) * (b_lse + U32 * nll.abs()) + eps * (b_lse + (gamma(C) * l.abs().sum(1) + U32 * l.sum(1).abs()) / C
                                                        + U32 * sm.abs()) + 3 * U32 * contrib.abs())
    use = mi & ok
    contrib, e_c = contrib * use, e_c * use
    n = mi.flatten(1).sum(1)
    s = contrib.flatten(1).sum(1)
    bs = e_c.flatten(1).sum(1) + (gamma(int(n.max()) + 16) + U32) * contrib.abs().flatten(1).sum(1)
    cnt = mask.to(l.device).sum(1).double() * P * P
    loss, bl, nvalid, w = _finish(s, bs, cnt, B, up)
    pr = torch.exp(l - lse[:, None])
    y = torch.zeros_like(l)
    y.scatter_(1, torch.where(ok, tg, torch.zeros_like(tg))[:, None], 1.0)
    y = (1 - eps) * y + eps / C
    wc = w[:, None, None, None]
    g = wc * (pr - y) * use[:, None]
    dp = pr * (torch.expm1(b_lse[:, None] + U32 * (l - lse[:, None]).abs()) + 2 * U32)
    bg = (wc.abs() * (dp + U32 * (pr - y).abs() + U32) + 5 * U32 * g.abs()) * use[:, None]
    return dict(lse=(lse, b_lse), sum=(s, bs), cnt=cnt, loss=(loss, bl), nvalid=nvalid, g=g, bg=bg, w=w, mi=mi)


# ----------------------------------------------------------------------------------------------
# Optimiser (losses.hip: sumsq_stage1/2, opt_finalize_kernel, adamw_kernel, adamw_groups_kernel), streaming casts (rowops.hip,
# gemm_f32x3.hip: x3_split) and the truncated depth standardisation (depth.hip).  The library is built without fast-math:
# sqrtf and `/` are the correctly rounded forms (one rounding each, u = 2^-24), products and sums may contract to FMAs
# (fewer roundings, never more).  Every product can also leave the normal range: hardware may flush the result or keep it
# subnormal, either way it moves by at most one f32 minimum normal, TINY32, which the bounds add per product as an absolute floor.
TINY32 = 2.0 ** -126


def f32r(x) -> float:
    """a Python float rounded to f32 (what a `float` argument of the C ABI carries)"""
    return float(np.float32(x))


def bias_corrections(b1: float, b2: float, t: int):
    """(float)(1 - b1^t), (float)sqrt(1 - b2^t) formed in double from the f32 betas, as mmae_adamw / opt_finalize_kernel do"""
    b1, b2 = f32r(b1), f32r(b2)
    return f32r(1.0 - b1 ** t), f32r(math.sqrt(1.0 - b2 ** t))


def _h(x, dev):
    """a hyper-parameter as the kernel receives it -- rounded to f32 -- widened to fp64 (a scalar, or one value per element)"""
    return torch.as_tensor(x, dtype=torch.float64).to(torch.float32).to(device=dev, dtype=torch.float64)


def adamw_ref(p, g, m, v, *, lr, wd, b1, b2, eps, bc1, bc2_sqrt, gs=1.0):
    """One AdamW step of adamw_kernel / adamw_groups_kernel in fp64 on the f32 operands and the f32-rounded hyper-parameters the
    kernel receives (lr, wd: scalars or one value per element).  Returns (p', bound), (m', bound), (v', bound).  Rounding points of
        gj = g gs;  m' = b1 m + (1 - b1) gj;  v' = b2 v + (1 - b2) gj gj;  den = sqrtf(v') / bc2_sqrt + eps;
        p' = p (1 - lr wd) - (lr / bc1) (m' / den)
    counted along each term (the two paths of each kernel contract differently, each to fewer roundings than counted here):
      m'   b1 m: product, sum = 2;  (1 - b1) gj: 1 - b1, gj, product, sum = 4.  The terms can cancel, so each is bounded on its
           own magnitude: gamma_2 |b1 m| + gamma_4 |(1 - b1) g gs|, + 3 TINY32 (three products)
      v'   b2 v: 2;  (1 - b2) gj gj: 1 - b2, gj twice, two products, sum = 6; all terms non-negative: gamma_2 b2 v + gamma_6 (..),
           + 4 TINY32 (gj^2 leaves the normal range below |gj| ~ 1e-19)
      den  sqrt moves by |dv| / (sqrt v' + sqrt v^) <= min(dv / sqrt v', sqrt dv), + u sqrt v' (sqrtf); / bc2_sqrt and + eps round
           values <= den: gamma_2 den
      step (lr / bc1) m' / den: lr / bc1, the division by den and the product round once each (gamma_3 |step|); m' and den enter
           to first order as (lr / bc1) dm / den and |step| dden / den, their cross term through the factor 1 / (1 - dden / den)
      p'   lr wd and 1 - lr wd round once each: |ddecay| <= u (|lr wd| + |1 - lr wd|); p decay rounds once; the difference once:
           |p| ddecay + u |p decay| + dstep + u |p'| (the last two roundings taken at the perturbed values)"""
    dev = p.device
    P, G, M, V = (t.detach().double() for t in (p, g, m, v))
    lr, wd, b1, b2, eps, bc1, bc2, gs = (_h(x, dev) for x in (lr, wd, b1, b2, eps, bc1, bc2_sqrt, gs))
    gj = G * gs
    t1, t2 = b1 * M, (1 - b1) * gj
    m2 = t1 + t2
    b_m = gamma(2) * t1.abs() + gamma(4) * t2.abs() + 3 * TINY32
    w1, w2 = b2 * V, (1 - b2) * gj * gj
    v2 = w1 + w2
    b_v = gamma(2) * w1.abs() + gamma(6) * w2 + 4 * TINY32
    sv = v2.clamp_min(0).sqrt()
    b_s = torch.minimum(b_v / sv.clamp_min(1e-300), b_v.sqrt()) + U32 * sv
    den = sv / bc2 + eps
    b_den = (b_s / bc2) * (1 + gamma(2)) + gamma(2) * den
    c = lr / bc1
    step = c * m2 / den
    r_den = b_den / den
    b_step = (c.abs() / den * b_m + step.abs() * r_den) / (1 - r_den)
    b_step = b_step + gamma(3) * (step.abs() + b_step) + 2 * TINY32
    lw = lr * wd
    dec = 1 - lw
    b_dec = U32 * (lw.abs() + dec.abs()) * (1 + U32)
    pd = P * dec
    b_pd = P.abs() * b_dec
    b_pd = b_pd + U32 * (pd.abs() + b_pd) + TINY32
    p2 = pd - step
    b_p = b_pd + b_step
    b_p = b_p + U32 * (p2.abs() + b_p)
    return (p2, b_p), (m2, b_m), (v2, b_v)


def sumsq_chain(n: int) -> int:
    """Longest chain of fp32 roundings a term of mmae_sumsq's sum passes.  sumsq_stage1 runs nb = min(ceil(n / 1024), 1024)
    workgroups of 256 lanes, a lane takes 4 elements per trip and T = ceil(n / (1024 nb)) trips: a term of its first trip is
    squared (1), summed in its pair (1) and with the other pair (1), added to the lane's sum (1), then moved once by each of the
    T - 1 later additions; the lane whose last trip is the scalar tail adds up to 3 terms one by one instead of one quad (+2):
    T + 5.  block_sum2: 6 wave shuffles + 2 additions of the four wave sums = 8.  sumsq_stage2: a lane adds at most
    ceil(1024 / 256) = 4 partials, then the same block reduction: 4 + 8.  L = T + 25."""
    nb = min((n + 1023) // 1024, 1024)
    T = (n + 1024 * nb - 1) // (1024 * nb)
    return T + 25


def sumsq_ref(x):
    """sum x^2 in fp64 and its bound gamma_L sum x^2 (every term non-negative, so the relative bound of the longest chain holds
    for the sum), + n TINY32 for squares that leave the normal range.  A non-finite x gives a non-finite sum and bound."""
    X = x.detach().double().reshape(-1)
    s = float((X * X).sum())
    return s, gamma(sumsq_chain(X.numel())) * s + X.numel() * TINY32


def opt_decision_ref(ss: float, b_ss: float, *, istate, lr, wd, b1, b2, clip, skip_at, prescale, lrwd=None, loss=None,
                     found_inf=None, grad_scale=None):
    """The decisions of opt_finalize_kernel (mmae.h, mmae_opt_step) restated: ss, b_ss the gradient's sum of squares and its bound
    (sumsq_ref), istate the six counters before the step, every other argument as in mmae_opt_desc (None / 0: not given).
    Returns the expected state[1..6] -- norm and scale as (value, bound), lr, wd and the two bias corrections as f32 values -- the
    expected istate[0..5] and `skip`.
      pre    = grad_prescale / grad_scale                       one division
      norm   = sqrtf(ss) pre: sqrt halves ss's relative error, sqrtf and the product round once each, pre carries one:
               relative b_ss / (2 ss) + gamma_3
      scale  = pre min(1, clip / (norm + 1e-6f)): norm's error, then 1e-6f, the sum, the division and the product (gamma_4), + pre's;
               min(1, .) is 1-Lipschitz, so the bound holds on either side of the switch.  Without clip: pre alone (u)
    A test keeps skip_at away from norm by more than norm's bound; the integers are exact."""
    clip, skip_at = float(clip or 0.0), float(skip_at or 0.0)
    pre = f32r(prescale)
    if grad_scale is not None:
        pre = pre / f32r(grad_scale)
    norm = math.sqrt(ss) * pre if ss >= 0 else float('nan')
    fin = math.isfinite(norm)
    r_norm = (b_ss / (2 * ss) if fin and ss > 0 else 0.0) + gamma(3)
    loss_bad = loss is not None and not math.isfinite(loss)
    amp_bad = found_inf is not None and found_inf > 0
    skip = (not fin) or (clip <= 0 and skip_at > 0 and norm >= skip_at) or loss_bad or amp_bad
    scale, r_scale = pre, U32
    if clip > 0:
        cc = f32r(clip) / (norm + 1e-6) if not math.isnan(norm) else float('nan')
        scale *= cc if cc < 1 else 1.0                 # a NaN norm leaves pre, an infinite one gives 0 -- as the kernel's comparison does
        r_scale = r_norm + gamma(4) + U32
    t = int(istate[1]) + (0 if skip else 1)
    ist = [1 if skip else 0, t, int(istate[2]) + loss_bad, int(istate[3]) + skip, int(istate[4]) + amp_bad, int(istate[5]) + (not fin)]
    bc1, bc2 = bias_corrections(b1, b2, max(t, 1))
    lr_, wd_ = (lrwd[0], lrwd[1]) if lrwd is not None else (lr, wd)
    b_norm = r_norm * norm if fin else float('nan')
    return dict(state={1: (norm, b_norm), 2: (scale, r_scale * abs(scale) if math.isfinite(scale) else float('nan')),
                       3: f32r(lr_), 4: f32r(wd_), 5: bc1, 6: bc2}, istate=[int(x) for x in ist], skip=bool(skip))


def depth_std_ref(x, lo: int, hi: int, eps: float):
    """Truncated standardisation of x [B, n] in fp64: stable sort, slice [lo, hi), mean, unbiased variance, (x - mean) /
    sqrt(var + eps) (eps as the f32 the kernel receives), with the bound of depth_standardize_kernel's last line
        y = (x - (float)mean) * (1.0f / sqrtf((float)var + eps))
      absolute  rs u |mean|: the mean rounded to f32 shifts every element by as much -- what is left where x ~ mean
      relative  rs: (float)var and + eps round once each, the root halves them (u), sqrtf and the reciprocal round once each: 3u;
                the difference and the product once each: gamma_5 |y|, taken at the shifted value
    The kernel's sums are fp64 over at most n terms (relative n 2^-53 on the mean of the magnitudes, and on var by the two-pass
    form), folded in as n 2^-52 on both parts."""
    X = x.detach().double()
    n = X.shape[-1]
    s = torch.sort(X, dim=-1, stable=True).values[..., lo:hi]
    mean = s.mean(-1, keepdim=True)
    var = s.var(-1, unbiased=True, keepdim=True)
    e = float(_h(eps, 'cpu'))
    rs = 1.0 / torch.sqrt(var + e)
    y = (X - mean) * rs
    d64 = n * 2.0 ** -52
    a = rs * (U32 * mean.abs() + d64 * s.abs().mean(-1, keepdim=True))
    return y, a * (1 + gamma(5)) + (gamma(5) + d64) * y.abs()


# ---- bit-exact restatements (torch on the CPU; integer arithmetic wherever the header fixes the bits) --------------------------
def _i16(r):
    """integers 0 .. 65535 (int64) -> the int16 tensor with those bits"""
    return torch.where(r >= 32768, r - 65536, r).to(torch.int16)


def bf16_bits_ref(x):
    """common.h's f32_to_bf16_bits on an f32 tensor: round to nearest even on the integer image (a value at or above 0x7f7f8000
    carries into the exponent: inf), a NaN keeps its top 16 bits with the quiet bit set.  Returns int16 bit patterns."""
    u = x.detach().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff       # integer arithmetic: the same on any device
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    return _i16(torch.where(nan, ((u >> 16) | 0x40) & 0xffff, r))


def bf16_to_f32_ref(bits):
    """bf16_bits_to_f32: the 16 bits (int16 or bfloat16 tensor) become the top half of an f32, NaN payloads included"""
    return (bits.detach().contiguous().view(torch.int16).to(torch.int32) << 16).view(torch.float32)


def h16_scale_ref(amax):
    """(S, 1 / S) of mmae.h's MMAE_F16 gradient scale, S = 2^(4 - floor(log2 m)), from the formula; S = 1 without the scalar, for
    m = 0, a subnormal, inf, NaN, and outside 2^-119 <= m < 2^127 (the range common.h's h16_grad_scale applies the formula in)."""
    if amax is None:
        return 1.0, 1.0
    m = abs(f32r(amax))
    if not (math.isfinite(m) and 2.0 ** -119 <= m < 2.0 ** 127):
        return 1.0, 1.0
    k = 4 - (math.frexp(m)[1] - 1)                     # frexp: m = f 2^e with 0.5 <= f < 1, so floor(log2 m) = e - 1
    return 2.0 ** k, 2.0 ** -k


def f32_to_f16_ref(x, amax=None):
    """cast_f16_kernel<true>: the f32 product x S (S a power of two: exact unless it leaves f32's range), then IEEE round to
    nearest even into fp16 -- beyond 65520 to inf, never clamped"""
    return (x.detach().cpu().float() * h16_scale_ref(amax)[0]).to(torch.float16)


def f16_to_f32_ref(h, amax=None):
    """cast_f16_kernel<false>: the exact fp16 -> f32 conversion times 1 / S, rounded to f32"""
    return h.detach().cpu().to(torch.float32) * h16_scale_ref(amax)[1]


def fma_f32_ref(a, x, y):
    """fmaf(a, x, y) element-wise on f32 tensors, correctly rounded: a x is exact in fp64 (48 bits); the fp64 sum with y is made
    round-to-odd -- when TwoSum leaves a remainder and the sum's last bit is even, step one fp64 towards the remainder -- and
    rounding that to f32 cannot double-round (53 >= 2 * 24 + 2 bits)."""
    ax = torch.as_tensor(a, dtype=torch.float32).double() * x.detach().cpu().double()
    yd = y.detach().cpu().double()
    s = ax + yd
    bb = s - ax
    e = (ax - (s - bb)) + (yd - bb)                    # TwoSum: ax + y = s + e exactly
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(e > 0, torch.full_like(s, float('inf')), torch.full_like(s, float('-inf')))
    s = torch.where((e != 0) & even & torch.isfinite(s), torch.nextafter(s, toward), s)
    return s.to(torch.float32)


def add_n_ref(xs):
    """add_n_kernel: the left-to-right chain ((in0 + in1) + in2) + ... in f32"""
    s = xs[0].detach().cpu().float().clone()
    for t in xs[1:]:
        s = s + t.detach().cpu().float()
    return s


def x3_split_ref(x):
    """split8 on finite f32 values: hi = bf16(x), lo = bf16(x - hi) (the difference is exact in f32).  Returns int16 bits (hi, lo)."""
    x = x.detach().cpu().float()
    hi = bf16_bits_ref(x)
    return hi, bf16_bits_ref(x - bf16_to_f32_ref(hi))


# ----------------------------------------------------------------------------------------------
# The input side (tokens.hip: patch_rows, semseg_emb_bwd[_det], mask_sample; embed.hip: patch_embed_fwd), from mmae.h's formulae.  A
# task is a dict: data (f32 [B][C][H][W], kind 0; int64 class ids [B][H][W], kind 1), emb (f32 [n_cls][C], kind 1), kind, C, H, W, ph,
# pw, k_off, n_cls.  Token idx of task t (offs[t] <= idx < offs[t + 1]) is patch p = idx - offs[t] at (p // (W / pw), p % (W / pw)).
def _task_patches(s):
    """every patch of one task flattened in (c, i, j) order: f32 [B][(H / ph) (W / pw)][C ph pw], copies only (NaN payloads survive);
    class ids outside [0, n_cls) embed as zeros"""
    d = s['data']
    C, H, W, ph, pw = s['C'], s['H'], s['W'], s['ph'], s['pw']
    if s['kind'] == 1:
        ok = (d >= 0) & (d < s['n_cls'])
        e = s['emb'].float()[torch.where(ok, d, torch.zeros_like(d))]                     # [B][H][W][C]
        d = torch.where(ok[..., None], e, torch.zeros_like(e)).permute(0, 3, 1, 2)
    B = d.shape[0]
    return d.reshape(B, C, H // ph, ph, W // pw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // ph) * (W // pw), C * ph * pw)


def token_owner(idx, offs):
    """task of every token index: the last t with offs[t] <= idx (an empty task owns nothing)"""
    return torch.bucketize(idx, torch.as_tensor(list(offs[1:-1]), dtype=idx.dtype, device=idx.device), right=True)


def patch_rows_ref(srcs, offs, sel, Ktot: int):
    """mmae_patch_rows in f32 [B * n_sel][Ktot]: row (b, r) holds the flattened patch of token sel[b][r] at its task's k_off, zeros in
    every other column -- gaps between segments and a tail past the last one included.  The bf16 form is bf16_bits_ref of it."""
    B, n_sel = sel.shape
    out = torch.zeros(B * n_sel, Ktot, dtype=torch.float32)
    flat = sel.reshape(-1)
    own = token_owner(flat, offs)
    bidx = torch.arange(B).repeat_interleave(n_sel)
    for t, s in enumerate(srcs):
        m = own == t
        K = s['C'] * s['ph'] * s['pw']
        assert s['k_off'] >= 0 and s['k_off'] + K <= Ktot
        out[m, s['k_off']:s['k_off'] + K] = _task_patches(s)[bidx[m], flat[m] - offs[t]]
    return out


def patch_embed_ref(srcs, ws, bs, poss, offs, sel, glob, D: int):
    """mmae_patch_embed_fwd in fp64 on the operands as the kernel multiplies them -- the patch and the weight rounded to bf16, bias and
    position row in f32: tok[b][r] = W_t . x^ + b_t + pos_t[p], tok[b][n_sel + g] = glob[g] (a copy: bound 0).  Bound of a token
    element: K_t exact products summed in fp32 in any order, then the two fp32 additions of the epilogue,
        gamma(K_t + 2) (|W_t| . |x^| + |b_t| + |pos_t[p]|) + ulp_f32(|ref| + that)
    Returns (tok fp64 [B][n_sel + G][D], bound, x^ as f32 [B * n_sel][sum K_t as laid out by k_off] -- None of it read from the GPU)."""
    B, n_sel = sel.shape
    G = 0 if glob is None else glob.shape[0]
    Kend = max(s['k_off'] + s['C'] * s['ph'] * s['pw'] for s in srcs)
    xh = bf16_to_f32_ref(bf16_bits_ref(patch_rows_ref(srcs, offs, sel, Kend)))
    ref = torch.zeros(B, n_sel + G, D, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    flat = sel.reshape(-1)
    own = token_owner(flat, offs)
    r2, b2 = torch.zeros(B * n_sel, D, dtype=torch.float64), torch.zeros(B * n_sel, D, dtype=torch.float64)
    for t, s in enumerate(srcs):
        m = own == t
        if not bool(m.any()):
            continue
        K = s['C'] * s['ph'] * s['pw']
        X = xh[m, s['k_off']:s['k_off'] + K].double()
        Wt = bf16_to_f32_ref(bf16_bits_ref(ws[t].float().reshape(D, K))).double()
        add = bs[t].double()[None, :] + poss[t].double()[flat[m] - offs[t]]
        absadd = bs[t].double().abs()[None, :] + poss[t].double().abs()[flat[m] - offs[t]]
        rt = X @ Wt.t() + add
        r2[m] = rt
        b2[m] = prod_bound(X.abs(), Wt.abs(), K + 2, torch.float32, rt, extra=gamma(K + 2) * absadd)
    ref[:, :n_sel] = r2.view(B, n_sel, D)
    bound[:, :n_sel] = b2.view(B, n_sel, D)
    if G:
        ref[:, n_sel:] = glob.double()
    return ref, bound, xh


def semseg_emb_grad_ref(d_rows, cls, sel, *, E, ph, pw, k_off, tok_off, n_patches, n_cls):
    """Gradient of the class-embedding table (mmae_semseg_emb_bwd[_det]) in fp64: d_emb[c][e] = sum over the selected tokens of
    [tok_off, tok_off + n_patches) and their pixels (i, j) with class c of d_rows[row][k_off + e ph pw + i pw + j]; ids outside
    [0, n_cls) contribute nothing.  d_rows [B * n_sel][ld] (any float type), cls int64 [B][H][W], sel [B][n_sel].
    Returns (grad [n_cls][E], n [n_cls][1] the number of terms of each entry, S [n_cls][E] = sum |term|)."""
    B, H, W = cls.shape
    n_sel = sel.shape[1]
    nh, nw = H // ph, W // pw
    assert nh * nw == n_patches
    p = sel.reshape(-1).cpu() - tok_off
    rows = torch.nonzero((p >= 0) & (p < n_patches)).reshape(-1)
    b = rows // n_sel
    ids = cls.cpu().reshape(B, nh, ph, nw, pw).permute(0, 1, 3, 2, 4).reshape(B, nh * nw, ph * pw)[b, p[rows]]          # [R][ph pw]
    terms = d_rows.detach().cpu()[rows, k_off:k_off + E * ph * pw].double().reshape(-1, E, ph * pw).permute(0, 2, 1)    # [R][ph pw][E]
    ids, terms = ids.reshape(-1), terms.reshape(-1, E)
    ok = (ids >= 0) & (ids < n_cls)
    grad = torch.zeros(n_cls, E, dtype=torch.float64)
    S = torch.zeros_like(grad)
    grad.index_add_(0, ids[ok], terms[ok])
    S.index_add_(0, ids[ok], terms[ok].abs())
    n = torch.bincount(ids[ok], minlength=n_cls).double()[:, None]
    return grad, n, S


def semseg_emb_grad_bound(grad, n, S):
    """any summation tree of the n fp32 terms of an entry is within gamma(n) S (so neither the sub-tables nor the grid matter), one more
    addition for `accumulate`: gamma(n + 1) S, + the final ulp as prod_bound adds it.  An entry without terms: exactly 0."""
    nn = n + 1
    b = nn * U32 / (1.0 - nn * U32) * S
    return torch.where(n > 0, b + ulp(torch.float32, grad.abs() + b), torch.zeros_like(b))


def mask_sample_ref(spt, task_noise, all_noise, offs, n_keep: int):
    """mmae_mask_sample restated with stable argsorts (mmae.h; multimae.py:191-216): per task, order = the stable argsort of its noise;
    SORTED POSITION j is pre-selected iff order[j] < k_t (the reference's quirk: the position, not the token of that rank); the keys
    (0 pre-selected / 1 not) + all_noise, one f32 addition, are sorted stably again: ids_restore[b][j] = rank of token j, the first
    n_keep ranks are visible (mask 0) and ids_keep lists them by rank.  spt int64 [B][T], task_noise / all_noise f32 [B][Ntot].
    Returns int64 (mask_all, ids_keep, ids_restore)."""
    B, Ntot = all_noise.shape
    key = torch.empty(B, Ntot, dtype=torch.float32)
    for t in range(len(offs) - 1):
        lo, hi = offs[t], offs[t + 1]
        order = torch.argsort(task_noise[:, lo:hi].float(), dim=1, stable=True)
        key[:, lo:hi] = (order >= spt[:, t:t + 1]).float()
    key = key + all_noise.float()
    shuffle = torch.argsort(key, dim=1, stable=True)
    restore = torch.empty_like(shuffle)
    restore.scatter_(1, shuffle, torch.arange(Ntot).expand(B, Ntot).contiguous())
    return (restore >= n_keep).long(), shuffle[:, :n_keep].contiguous(), restore


# ----------------------------------------------------------------------------------------------
# Stage references of a pre-LN transformer block (composite.hip: mmae_block_fwd / mmae_block_bwd), each in fp64 on the operands its
# stage reads, with the element-wise bounds of the per-kernel checks: layernorm_ref restates the bound of
# test_kernels_gpu._layernorm_per_element, linear_ref / linear_dx_ref / linear_dw_ref are prod_bound with the epilogue terms of
# test_kernels_gpu._epilogues_per_element, the GELU pair carries that file's measured constants of the bf16 epilogues' polynomial.
U_X3 = 2.0 ** -14                      # relative error of one split-bf16 product (MMAE_F32X3: hi hi + hi lo + lo hi, lo lo dropped)
GELU_ABS, GELU_REL, DGELU_ABS = 1.3e-4, 2.6e-5, 5.5e-4      # DESIGN.md section 6 item 12 (tools/gelu_poly_fit.py)
GELU_D1, GELU_D2 = 1.13, 0.8           # max |gelu'|, max |gelu''|: how a pre-activation error propagates


def gelu_ref(z):
    """(gelu(z), gelu'(z)) in fp64, the erf form"""
    z = z.double()
    Phi = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return z * Phi, Phi + z * phi


class layernorm_ref:
    """LayerNorm over the last dimension of x [R, D] (f32 values) in fp64 with the kernels' bounds (u = 2^-24, fp32 arithmetic):
      mean    |dm| <= gamma_D mean|x| + ulp
      rstd    relative rho <= gamma_(2D+4) mean(x^2) / var / 2 + 2^-21     (one- or two-pass variance, halved by the root; rsq within 1 ulp)
      xhat    |dxh| <= |xh| (rho + 2u) + rstd |dm|
      y       |dy_| <= |w| |dxh| + 4u (|xh w| + |b|) + ulp(out)
    bwd(dy, dx_in): dx = dx_in + rstd (g - mean g - xh mean(g xh)), g = dy w, with
      |ddx| <= rho |dx - dx_in| + rstd (gamma_D mean|g| + |dxh| mean|g xh| + |xh| mean(|g| |dxh|) + gamma_D |xh| mean|g xh|)
               + 6u (|dx_in| + rstd (|g| + mean|g| + |xh| mean|g xh|)) + ulp_f32
    and the parameter gradients dgamma = sum_r dy xh, dbeta = sum_r dy over R rows in `extra` more partial sums:
      the rows' bounds summed + gamma_(R + extra) sum of magnitudes."""

    def __init__(self, x, w, b, eps: float):
        u = U32
        self.x, self.w, self.b = x.double(), w.double(), b.double()
        self.R, self.D = self.x.shape
        D = self.D
        self.mean = self.x.mean(1)
        xc = self.x - self.mean[:, None]
        self.var = (xc * xc).mean(1)
        self.rstd = 1.0 / torch.sqrt(self.var + float(_h(eps, 'cpu')))
        self.xh = xc * self.rstd[:, None]
        self.b_mean = gamma(D) * self.x.abs().mean(1) + ulp(torch.float32, self.mean)
        self.rho = gamma(2 * D + 4) * (self.x * self.x).mean(1) / (self.var + float(_h(eps, 'cpu'))) / 2 + 2.0 ** -21
        self.b_rstd = self.rho * self.rstd + ulp(torch.float32, self.rstd)
        self.e_xh = self.xh.abs() * (self.rho[:, None] + 2 * u) + self.rstd[:, None] * self.b_mean[:, None]
        self.y = self.xh * self.w + self.b
        self._b_y = self.w.abs() * self.e_xh + 4 * u * ((self.xh * self.w).abs() + self.b.abs())

    def b_y(self, out_dtype):
        return self._b_y + ulp(out_dtype, self.y.abs() + self._b_y)

    def bwd(self, dy, dx_in=None, act_dtype=None, extra: int = 0):
        """returns dict: dx (ref, bound f32[, bound in act_dtype]), dgamma (ref, bound), dbeta (ref, bound)"""
        u, D, R = U32, self.D, self.R
        dy = dy.double()
        dx_in = torch.zeros_like(dy) if dx_in is None else dx_in.double()
        rs, xh, e_xh = self.rstd[:, None], self.xh, self.e_xh
        g = dy * self.w
        mg = g.abs().mean(1, keepdim=True)
        gx = (g * xh).mean(1, keepdim=True)
        agx = (g * xh).abs().mean(1, keepdim=True)
        ref = dx_in + rs * (g - g.mean(1, keepdim=True) - xh * gx)
        bd = (self.rho[:, None] * (ref - dx_in).abs()
              + rs * (gamma(D) * mg + e_xh * agx + xh.abs() * (g.abs() * e_xh).mean(1, keepdim=True) + gamma(D) * xh.abs() * agx)
              + 6 * u * (dx_in.abs() + rs * (g.abs() + mg + xh.abs() * agx)))
        b32 = bd + ulp(torch.float32, ref.abs() + bd)
        out = dict(dx=(ref, b32), dx_act=None)
        if act_dtype is not None:
            out['dx_act'] = (ref, b32 + ulp(act_dtype, ref.abs() + b32))
        dg = (dy * xh).sum(0)
        out['dgamma'] = (dg, (dy.abs() * e_xh).sum(0) + gamma(R + 1 + extra) * (dy * xh).abs().sum(0))
        out['dbeta'] = (dy.sum(0), gamma(R + extra) * dy.abs().sum(0) + 0 * dg)
        return out


def linear_ref(x, w, bias=None, resid=None, out_dtype=torch.float32, u_op: float = 0.0, k_mult: int = 1):
    """y = x w^T (+ bias) (+ resid) in fp64 on the operands as stored ([M, K], [N, K]) and its bound: prod_bound's product term over
    k_mult K accumulated terms (3 K when a split-bf16 product runs as one bf16 product over [hi | lo | hi]), one fp32 rounding per
    epilogue addition (2u |y| for the bias, 2u more for the residual), the final rounding into out_dtype.
    Returns (y, bound, pre) -- pre = (x w^T + bias, its bound before the final rounding), what an activation epilogue starts from."""
    x, w = x.double(), w.double()
    K = x.shape[1]
    lin = x @ w.t()
    if bias is not None:
        lin = lin + bias.double()
    e = prod_bound(x.abs(), w.abs(), k_mult * K, u_op=u_op) + 2 * U32 * lin.abs()
    y = lin
    b = e
    if resid is not None:
        y = lin + resid.double()
        b = e + 2 * U32 * y.abs()
    return y, b + ulp(out_dtype, y.abs() + b), (lin, e)


def linear_dx_ref(dy, w, out_dtype, u_op: float = 0.0, k_mult: int = 1, mul=None, dgelu_of=None):
    """dx = dy w (dy [M, N], w [N, K]) in fp64, optionally times `mul` (MMAE_EPI_MUL: a stored derivative) or times gelu'(dgelu_of)
    (MMAE_EPI_DGELU: re-evaluated from the stored pre-activation), with the bounds of test_kernels_gpu._epilogues_per_element.
    Returns (ref, bound incl. the rounding into out_dtype, bound before that rounding -- what the epilogue's column sums add up)."""
    dy, w = dy.double(), w.double()
    N = dy.shape[1]
    g = dy @ w
    Eg = prod_bound(dy.abs(), w.t().abs(), k_mult * N, u_op=u_op)
    if mul is not None:
        r = g * mul.double()
        b = Eg * mul.double().abs() + 2 * U32 * r.abs()
    elif dgelu_of is not None:
        r = g * gelu_ref(dgelu_of)[1]
        b = GELU_D1 * Eg + g.abs() * DGELU_ABS + 2 * U32 * r.abs()
    else:
        r, b = g, Eg
    return r, b + ulp(out_dtype, r.abs() + b), b


def linear_dw_ref(dy, x, u_op: float = 0.0, g0=None):
    """dw = dy^T x ([M, N], [M, K] -> [N, K]) and db = colsum(dy) in fp64 over the M rows, f32 destinations; g0 = (dw0, db0): added
    onto these (grad_acc: one more term in gamma).  Returns (dw, bound), (db, bound)."""
    dy, x = dy.double(), x.double()
    M = dy.shape[0]
    t = 0 if g0 is None else 1
    dw = dy.t() @ x
    db = dy.sum(0)
    aw, ab = dy.t().abs() @ x.abs(), dy.abs().sum(0)
    if g0 is not None:
        dw, db = dw + g0[0].double(), db + g0[1].double()
        aw, ab = aw + g0[0].double().abs(), ab + g0[1].double().abs()
    bw = (gamma(M + t) + u_op) * aw
    bb = gamma(M + t) * ab
    return (dw, bw + ulp(torch.float32, dw.abs() + bw)), (db, bb + ulp(torch.float32, db.abs() + bb))


def colsum_ref(x, terms: int = 0, g0=None):
    """fp64 column sums of x [M, n] as stored and the bound of ANY fp32 summation tree over its M (+ terms more partial sums, + 1 when
    added onto g0) terms: gamma times the column sums of the magnitudes."""
    x = x.double()
    s, a = x.sum(0), x.abs().sum(0)
    n = x.shape[0] + terms
    if g0 is not None:
        s, a, n = s + g0.double(), a + g0.double().abs(), n + 1
    return s, gamma(n) * a


def heads_of(t, B, N, H, hd, col0: int = 0):
    """[B * N][ld] rows, head h at columns col0 + h * hd -> [B * H][N][hd]"""
    return t[:, col0:col0 + H * hd].reshape(B, N, H, hd).permute(0, 2, 1, 3).reshape(B * H, N, hd)


def rows_of(t, B, N, H, hd):
    """inverse of heads_of: [B * H][N][hd] -> [B * N][H * hd]"""
    return t.reshape(B, H, N, hd).permute(0, 2, 1, 3).reshape(B * N, H * hd)


def block_ref(x0, P, heads: int, eps: float, B: int, N: int, dy=None, dp1=None, dp2=None):
    """One pre-LN block composed from the stage references above (layernorm_ref, linear_ref, attention_bounds, gelu_ref), every stage
    fed with the previous stage's fp64 result: x1 = x0 + dp1 attn(norm1(x0)), x2 = x1 + dp2 mlp(norm2(x1)); with dy = d(x2) also the
    backward.  P: the 12 parameters in the order n1_w n1_b qkv_w qkv_b proj_w proj_b n2_w n2_b fc1_w fc1_b fc2_w fc2_b; dp1 / dp2:
    per-sample scales [B] or None.  Returns a dict of every stage's reference (bounds dropped: this is what
    tests/test_check_helpers_cpu.py holds against torch autograd of a plainly written block)."""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = (t.double() for t in P)
    R, D = x0.shape
    hd = D // heads
    sc = hd ** -0.5
    row = lambda s: torch.ones(R, 1, dtype=torch.float64, device=x0.device) if s is None else s.double().repeat_interleave(N)[:, None]
    s1, s2 = row(dp1), row(dp2)
    o = {}
    l1 = layernorm_ref(x0, n1w, n1b, eps)
    o['ln1'] = l1.y
    o['qkv'] = linear_ref(o['ln1'], qkvw, qkvb)[0]
    hv = lambda c: heads_of(o['qkv'], B, N, heads, hd, c)
    s = sc * (hv(0) @ hv(D).transpose(-1, -2))
    o['lse'] = torch.logsumexp(s, -1)
    o['ao'] = rows_of(torch.exp(s - o['lse'][..., None]) @ hv(2 * D), B, N, heads, hd)
    o['x1'] = x0.double() + s1 * linear_ref(o['ao'], projw, projb)[0]
    l2 = layernorm_ref(o['x1'], n2w, n2b, eps)
    o['ln2'] = l2.y
    o['pre'] = linear_ref(o['ln2'], fc1w, fc1b)[0]
    o['hact'], o['dgelu'] = gelu_ref(o['pre'])
    o['x2'] = o['x1'] + s2 * linear_ref(o['hact'], fc2w, fc2b)[0]
    if dy is None:
        return o
    dy = dy.double()
    dm = dy * s2
    (o['g_fc2_w'], _), (o['g_fc2_b'], _) = linear_dw_ref(dm, o['hact'])
    o['d_hpre'] = linear_dx_ref(dm, fc2w, torch.float32, mul=o['dgelu'])[0]
    (o['g_fc1_w'], _), (o['g_fc1_b'], _) = linear_dw_ref(o['d_hpre'], o['ln2'])
    o['d_ln2'] = linear_dx_ref(o['d_hpre'], fc1w, torch.float32)[0]
    b2 = l2.bwd(o['d_ln2'], dy)
    o['dx1'], o['g_n2_w'], o['g_n2_b'] = b2['dx'][0], b2['dgamma'][0], b2['dbeta'][0]
    da = o['dx1'] * s1
    (o['g_proj_w'], _), (o['g_proj_b'], _) = linear_dw_ref(da, o['ao'])
    o['d_ao'] = linear_dx_ref(da, projw, torch.float32)[0]
    ab = attention_bounds(hv(0), hv(D), hv(2 * D), heads_of(o['d_ao'], B, N, heads, hd), sc, u_in=0.0, u_p=0.0, out_dtype=torch.float32)
    o['d_qkv'] = torch.cat([rows_of(ab[k][0], B, N, heads, hd) for k in ('dq', 'dk', 'dv')], 1)
    (o['g_qkv_w'], _), (o['g_qkv_b'], _) = linear_dw_ref(o['d_qkv'], o['ln1'])
    o['d_ln1'] = linear_dx_ref(o['d_qkv'], qkvw, torch.float32)[0]
    b1 = l1.bwd(o['d_ln1'], o['dx1'])
    o['dx0'], o['g_n1_w'], o['g_n1_b'] = b1['dx'][0], b1['dgamma'][0], b1['dbeta'][0]
    o['g_cs'] = colsum_ref(o['dx0'])[0]
    return o


# ----------------------------------------------------------------------------------------------
# The whole SpatialOutputAdapter in fp64, restated from mmae.h's description of mmae_adapter_desc and mmae_decoder_build (not from the
# oracle): the yardstick the per-kernel path's error is MEASURED against, and the composite's held to (tests/test_composite_gpu.py).
def plain_block(x, P, heads: int, eps: float, B: int, N: int):
    """a pre-LN block written out plainly in torch (any float dtype, differentiable): x [B * N, D], P the 12 parameters"""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = P
    D = x.shape[1]
    hd = D // heads
    F = torch.nn.functional
    qkv = F.linear(F.layer_norm(x, (D,), n1w, n1b, eps), qkvw, qkvb).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = ((qkv[0] @ qkv[1].transpose(-1, -2)) * hd ** -0.5).softmax(-1) @ qkv[2]
    x1 = x + F.linear(a.transpose(1, 2).reshape(B * N, D), projw, projb)
    h = F.linear(F.layer_norm(x1, (D,), n2w, n2b, eps), fc1w, fc1b)
    return x1 + F.linear(h * 0.5 * (1 + torch.erf(h / math.sqrt(2))), fc2w, fc2b)


def decoder_rows_ref(ctx, ids_keep, ids_restore, mask_token, temb, pos, offs, q_task: int, G: int, n_q: int):
    """mmae_decoder_build's formulae: ctx [B, n_keep + G, D] -> (queries [B, n_q, D], context [B, n_keep + G, D]).
      q[b][j] = (ids_restore[b][off(q_task) + j] < n_keep ? ctx[b][that rank] : mask_token) + task_emb[q_task] + pos[j]
      q_task = -1: q[b][j] = mask_token + pos[j]
      c[b][r] = ctx[b][r] + task_emb[task(ids_keep[b][r])] + pos[ids_keep[b][r] - off(task)] for r < n_keep; global rows copied
    temb: list of [D] tensors or None (= zeros)."""
    B, NC, D = ctx.shape
    n_keep = NC - G
    te = torch.stack([torch.zeros(D, dtype=ctx.dtype, device=ctx.device) if t is None else t for t in temb])
    if q_task < 0:
        q = (mask_token + pos)[None].expand(B, n_q, D)
    else:
        rank = ids_restore[:, offs[q_task]:offs[q_task] + n_q]
        vis = rank < n_keep
        got = torch.gather(ctx, 1, rank.clamp_max(NC - 1)[..., None].expand(B, n_q, D))
        q = torch.where(vis[..., None], got, mask_token.expand(B, n_q, D)) + te[q_task] + pos
    task = token_owner(ids_keep, offs)
    off_t = torch.as_tensor(list(offs), device=ids_keep.device)[task]
    c = ctx[:, :n_keep] + te[task] + pos[ids_keep - off_t]
    return q, torch.cat([c, ctx[:, n_keep:]], 1)


def adapter_ref(enc, ids_keep, ids_restore, params, *, T, q_task, G, D, heads, depth, pos, offs, C, nh, nw, ph, pw, eps, d_img=None):
    """SpatialOutputAdapter.forward in fp64 from its parameters (SpatialAdapterFn's order: mask_token, task_emb[0..T-1] (None = none),
    q.w q.b kv.w kv.b proj.w proj.b ctxn.w ctxn.b qn.w qn.b outn.w outn.b fc1.w fc1.b fc2.w fc2.b, 12 per block, out_proj.w out_proj.b,
    proj_context.w proj_context.b; weights as the products read them): proj_context, the query / context rows, cross-attention
    (queries over the context, no residual around it), x + mlp(out_norm(x)), the blocks, out_proj, patch rows -> image.  With d_img
    also the backward, by autograd of exactly this forward.  Returns (img, pat) or (img, pat, d_enc, [gradient per parameter or None])."""
    F = torch.nn.functional
    ps = [None if p is None else p.detach().double().clone().requires_grad_(d_img is not None) for p in params]
    enc = enc.detach().double().clone().requires_grad_(d_img is not None)
    mask, temb = ps[0], ps[1:1 + T]
    qw, qb, kvw, kvb, pw_, pb, cnw, cnb, qnw, qnb, onw, onb, f1w, f1b, f2w, f2b = ps[1 + T:17 + T]
    blocks = ps[17 + T:17 + T + 12 * depth]
    ow, ob, pcw, pcb = ps[17 + T + 12 * depth:]
    B, NC, _ = enc.shape
    n_q, hd = nh * nw, D // heads
    ctx = F.linear(enc, pcw, pcb)
    q_rows, c_rows = decoder_rows_ref(ctx, ids_keep, ids_restore, mask.reshape(D), [None if t is None else t.reshape(D) for t in temb],
                                      pos.double(), offs, q_task, G, n_q)
    qn, cn = F.layer_norm(q_rows, (D,), qnw, qnb, eps), F.layer_norm(c_rows, (D,), cnw, cnb, eps)
    q = F.linear(qn, qw, qb).reshape(B, n_q, heads, hd).transpose(1, 2)
    kv = F.linear(cn, kvw, kvb).reshape(B, NC, 2, heads, hd).permute(2, 0, 3, 1, 4)
    xo = (((q @ kv[0].transpose(-1, -2)) * hd ** -0.5).softmax(-1) @ kv[1]).transpose(1, 2).reshape(B * n_q, D)
    x = F.linear(xo, pw_, pb)
    h = F.linear(F.layer_norm(x, (D,), onw, onb, eps), f1w, f1b)
    x = x + F.linear(h * 0.5 * (1 + torch.erf(h / math.sqrt(2))), f2w, f2b)
    for l in range(depth):
        x = plain_block(x, blocks[12 * l:12 * l + 12], heads, eps, B, n_q)
    pat = F.linear(x, ow, ob)
    img = _rows_img_rect(pat.reshape(B, n_q, C * ph * pw), C, nh, nw, ph, pw)
    if d_img is None:
        return img.detach(), pat.detach()
    img.backward(d_img.double())
    return img.detach(), pat.detach(), enc.grad, [None if p is None else p.grad for p in ps]


def _rows_img_rect(r, C, nh, nw, ph, pw):
    """[B, nh * nw, C * ph * pw] patch rows (column order c, i, j) -> [B, C, nh * ph, nw * pw]"""
    B = r.shape[0]
    return r.reshape(B, nh, nw, C, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B, C, nh * ph, nw * pw)
