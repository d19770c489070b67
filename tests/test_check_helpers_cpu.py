"""The element-wise check helpers of tests/helpers.py against known answers, on the CPU.

The exact result rounded to the output type -- what a correct kernel can at best produce -- must pass; each corruption below must
be flagged.  The corruptions are the ones the kernel tests' single rel-L2 number (helpers.rel_err at the tolerances those tests
used) lets through; that is asserted too, so the reason for the element-wise checks stays visible here."""
import math

import pytest
import torch

from helpers import (Guarded, assert_within, attention_bounds, ce_loss_ref, gamma, pixel_loss_ref, poisoned, prod_bound, rel_err,
                     ulp)


def _gemm():
    g = torch.Generator().manual_seed(1)
    M, N, K = 2504, 520, 256                    # test_round3_gemm_structures_vs_fp32_reference's first shape
    A = torch.randn(M, K, generator=g).bfloat16().double()
    B = torch.randn(N, K, generator=g).bfloat16().double()
    ref = A @ B.t()
    out = ref.to(torch.bfloat16).double()       # the exact product, rounded once to the bf16 output
    return A, B, ref, out, prod_bound(A.abs(), B.abs(), K, torch.bfloat16, ref)


def test_ulp_and_gamma():
    assert float(ulp(torch.bfloat16, torch.tensor(1.0))) == 2.0 ** -7
    assert float(ulp(torch.bfloat16, torch.tensor(1.5))) == 2.0 ** -7
    assert float(ulp(torch.bfloat16, torch.tensor(-3.0))) == 2.0 ** -6
    assert float(ulp(torch.float16, torch.tensor(1.0))) == 2.0 ** -10
    assert float(ulp(torch.float32, torch.tensor(1.0))) == 2.0 ** -23
    assert float(ulp(torch.float32, torch.tensor(0.0))) == 2.0 ** -149          # subnormal spacing
    assert float(ulp(torch.float16, torch.tensor(0.0))) == 2.0 ** -24
    x = (torch.randn(10000) * 100).double()           # f32 values: one rounding to each narrower format
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert bool(((x.to(dt).double() - x).abs() <= 0.5 * ulp(dt, x)).all())
    assert gamma(256) == pytest.approx(256 * 2.0 ** -24, rel=1e-4)


def test_gemm_bound_passes_the_rounded_exact_result():
    A, B, ref, out, bound = _gemm()
    assert_within(out, ref, bound, 'exact product rounded to bf16')


@pytest.mark.parametrize('corruption', ['corner block zeroed', 'one sign flipped', 'last 8 rows 1 % large'])
def test_gemm_corruptions_are_flagged_though_rel_l2_passes(corruption):
    A, B, ref, out, bound = _gemm()
    bad = out.clone()
    if corruption == 'corner block zeroed':
        bad[-4:, -4:] = 0.0                      # the ragged corner tile (rel-L2 3.7e-3)
    elif corruption == 'one sign flipped':
        bad[-1, -1] = -bad[-1, -1]                # (a typical magnitude: 13.8, 1.2 x the rms)
    else:
        bad[-8:] *= 1.01                          # (rel-L2 1.8e-3)
    assert rel_err(bad, ref) < 4e-3              # the rel-L2 test tolerance for 16-bit outputs lets it through
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, ref, bound, corruption)


def _attention():
    g = torch.Generator().manual_seed(2)
    B, H, N, hd = 2, 16, 197, 64                 # test_attention_fwd_bwd's (2, 16, 197, 197, 64)
    q, k, v, do = (torch.randn(B * H, N, hd, generator=g).bfloat16().double() for _ in range(4))
    return q, k, v, do, hd ** -0.5


def test_attention_bounds_pass_the_rounded_exact_result():
    q, k, v, do, sc = _attention()
    r = attention_bounds(q, k, v, do, sc, u_in=0.0, u_p=2.0 ** -8, out_dtype=torch.bfloat16)
    for name in ('o', 'dq', 'dk', 'dv'):
        ref, bd = r[name]
        assert_within(ref.to(torch.bfloat16), ref, bd, name)
    lse, bl = r['lse']
    assert_within(lse.float(), lse, bl, 'lse')


def test_attention_dq_tail_rows_off_by_20_percent_is_flagged():
    q, k, v, do, sc = _attention()
    r = attention_bounds(q, k, v, do, sc, u_in=0.0, u_p=2.0 ** -8, out_dtype=torch.bfloat16)
    ref, bd = r['dq']
    bad = ref.to(torch.bfloat16).double()
    bad[5, 192:] *= 1.2                          # the 5 rows past 6 x 32 of one head
    assert rel_err(bad, ref) < 2e-2
    with pytest.raises(AssertionError, match=r'worst at \(z=5, q=19[2-6]'):
        assert_within(bad, ref, bd, 'dq', names=('z', 'q', 'd'))


def test_attention_forward_dropped_last_key_is_flagged():
    q, k, v, do, sc = _attention()
    r = attention_bounds(q, k, v, do, sc, u_in=0.0, u_p=2.0 ** -8, out_dtype=torch.bfloat16)
    ref, bd = r['o']
    bad = ref.clone()
    z = 3
    s = sc * (q[z] @ k[z, :-1].t())
    bad[z] = s.softmax(-1) @ v[z, :-1]           # the last key of one (b, h) left out of the softmax
    bad = bad.to(torch.bfloat16).double()
    # rel-L2 barely registers it: ~1e-2, the forward tolerance of the bf16 paths (it lands within 20 % of it either side)
    assert 0.8e-2 < rel_err(bad, ref) < 1.2e-2
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, ref, bd, 'o')


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
def test_guarded_buffer_flags_a_write_into_one_guard_column(dtype):
    gb = Guarded(13, 20, 24, dtype, 'cpu')
    gb.view.copy_(torch.randn(13, 20))           # writes inside the view leave it intact
    gb.intact()
    assert torch.isnan(gb.flat[:gb.off]).all() and torch.isnan(gb.full[:, 20:]).all()
    gb.full[7, 21] = 0.0                         # one element of the ld padding
    with pytest.raises(AssertionError, match=r'row 7, col 21'):
        gb.intact()
    gb2 = Guarded(4, 8, 8, dtype, 'cpu')
    gb2.flat[gb2.off + 4 * 8] = 1.0              # the first element past the view
    with pytest.raises(AssertionError, match='guard zone after'):
        gb2.intact()


def test_poisoned_operand_layout():
    X = torch.randn(5, 11)
    flat, off = poisoned(X, 32, torch.bfloat16, 'cpu', finite_to=16, junk=3.0)
    v = flat[off - 8:off - 8 + 5 * 32].view(5, 32)
    assert torch.equal(v[:, 8:19], X.bfloat16())
    assert bool((v[:, 19:24] == 3.0).all())
    assert torch.isnan(v[:, :8]).all() and torch.isnan(v[:, 24:]).all() and torch.isnan(flat[:off - 8]).all()
    assert torch.isnan(flat[off - 8 + 5 * 32:]).all()


def test_assert_within_reports_index_value_reference_and_bound():
    ref = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    out = ref.clone()
    out[1, 2, 3, 4] = 0.5
    out[0, 0, 0, 0] = float('nan')
    with pytest.raises(AssertionError) as e:
        assert_within(out, ref, 0.1, 'x', names=('b', 'h', 'q', 'd'))
    msg = str(e.value)
    assert '2 of 120 elements' in msg and '(b=0, h=0, q=0, d=0)' in msg and 'nan' in msg
    out[0, 0, 0, 0] = 0.0
    with pytest.raises(AssertionError, match=r'\(b=1, h=2, q=3, d=4\): value 0.5, reference 0.0, bound 1.000e-01'):
        assert_within(out, ref, 0.1, 'x', names=('b', 'h', 'q', 'd'))
    assert math.isfinite(float(prod_bound(torch.ones(1, 1), torch.ones(1, 1), 1).sum()))


# ---- masked-loss references (pixel_loss_ref, ce_loss_ref) ----------------------------------------------------------------------
def _pix_case(kind, norm_pix):
    g = torch.Generator().manual_seed(3 + kind)
    B, C, H, W, P = 4, 3, 64, 64, 8                 # 196 608 gradient elements
    pred = torch.randn(B, C, H, W, generator=g)
    target = torch.randn(B, C, H, W, generator=g)
    target[:, :, :P, :P] = 0.1                       # a constant patch: var = 0
    mask = (torch.rand(B, 64, generator=g) < 0.6).long()
    mask[1] = 0
    mask[0, 0] = 1
    return pixel_loss_ref(kind, norm_pix, pred, target, mask, P, up=0.75), P


def _ce_case(eps):
    g = torch.Generator().manual_seed(5)
    B, C, H, W, P = 2, 20, 32, 48, 4                 # 61 440 gradient elements
    logits = torch.randn(B, C, H, W, generator=g) * 3
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[:, ::5, ::3] = 255                        # ignored
    mask = (torch.rand(B, (H // P) * (W // P), generator=g) < 0.6).long()
    return ce_loss_ref(logits, target, mask, P, eps, up=1.25), P


@pytest.mark.parametrize('kind,norm_pix', [(0, False), (0, True), (1, False), (1, True)])
def test_pixel_loss_bounds_pass_the_rounded_exact_result(kind, norm_pix):
    ref, _ = _pix_case(kind, norm_pix)
    for dt in (torch.float32, torch.bfloat16):
        out = ref['g'].to(dt).double()
        extra = ulp(dt, ref['g'].abs() + ref['bg']) / 2 if dt != torch.float32 else 0
        assert_within(out, ref['g'], ref['bg'] + extra + (ref['g'].abs() * 2.0 ** -24 if dt == torch.float32 else 0), f'gradient as {dt}')
    assert_within(ref['sum'][0].float(), ref['sum'][0], ref['sum'][1], 'per-sample sum as f32')
    if norm_pix:
        for k in ('mean', 'rstd'):
            assert_within(ref[k][0].float(), ref[k][0], ref[k][1], f'{k} as f32')


def test_ce_bounds_pass_the_rounded_exact_result():
    for eps in (0.0, 0.1, 1.0):
        ref, _ = _ce_case(eps)
        assert_within(ref['g'].float(), ref['g'], ref['bg'], f'eps {eps} d_logits as f32')
        assert_within(ref['lse'][0].float(), ref['lse'][0], ref['lse'][1], f'eps {eps} lse as f32')
        assert_within(ref['sum'][0].float(), ref['sum'][0], ref['sum'][1], f'eps {eps} per-sample sum as f32')


def _corrupt(x, how, P):
    x = x.clone()
    if how == 'element':
        i = int(torch.nonzero(x.reshape(-1))[len(torch.nonzero(x.reshape(-1))) // 2])
        x.view(-1)[i] *= 1 + 2e-3
    elif how == 'patch':                              # one patch of one sample, every channel: a weight off by 5e-5
        b = int(torch.nonzero(x.flatten(1).abs().sum(1))[0])
        nz = torch.nonzero(x[b, 0])[-1]
        y0, x0 = int(nz[0]) // P * P, int(nz[1]) // P * P
        x[b, :, y0:y0 + P, x0:x0 + P] *= 1 + 5e-5
    else:                                             # the tail: last 8 non-zero elements off by 3e-4
        idx = torch.nonzero(x.reshape(-1)).reshape(-1)[-8:]
        x.view(-1)[idx] *= 1 + 3e-4
    return x


@pytest.mark.parametrize('how', ['element', 'patch', 'tail'])
def test_masked_loss_gradient_corruptions_are_flagged_though_rel_l2_passes(how):
    ref, P = _pix_case(0, True)
    bad = _corrupt(ref['g'], how, P).float()
    assert rel_err(bad, ref['g']) < 1e-5               # test_masked_pixel_losses' tolerance on the gradient
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, ref['g'], ref['bg'] + ref['g'].abs() * 2.0 ** -24, f'MSE norm_pix gradient, {how} corrupted')
    cref, P = _ce_case(0.1)
    bad = _corrupt(cref['g'], how, P).float()
    assert rel_err(bad, cref['g']) < 4e-3              # test_masked_cross_entropy_label_smoothing's tolerance
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, cref['g'], cref['bg'], f'CE gradient, {how} corrupted')


def test_ce_lse_of_one_pixel_off_and_an_ignored_target_read_are_flagged():
    ref, P = _ce_case(0.1)
    lse = ref['lse'][0].float().clone()
    lse[1, 7, 9] += 1e-4
    assert rel_err(lse, ref['lse'][0]) < 1e-5
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(lse, ref['lse'][0], ref['lse'][1], 'lse')
    # a kernel that read the logits at an ignored pixel's clamped target (class 0) instead of skipping it
    g = ref['g'].clone()
    y, x = (int(v) for v in torch.nonzero(ref['mi'][0, ::5, ::3])[0])
    y, x = 5 * y, 3 * x                               # an ignored pixel (target[:, ::5, ::3] = 255) inside a masked patch
    assert bool((g[0, :, y, x] == 0).all())
    g[0, 0, y, x] -= ref['w'][0] * 0.9
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(g.float(), ref['g'], ref['bg'], 'CE gradient at an ignored pixel')


# ---- optimiser, cast and depth references (adamw_ref, sumsq_ref, opt_decision_ref, depth_std_ref, the bit-exact restatements) ----
from helpers import (TINY32, adamw_ref, add_n_ref, bf16_bits_ref, bf16_to_f32_ref, bias_corrections, depth_std_ref, f16_to_f32_ref,  # noqa: E402
                     f32_to_f16_ref, f32r, fma_f32_ref, h16_scale_ref, opt_decision_ref, sumsq_chain, sumsq_ref, x3_split_ref)

_HY = dict(lr=1e-3, wd=0.05, b1=0.9, b2=0.95, eps=1e-8)


def _adamw_f32(p, g, m, v, *, lr, wd, b1, b2, eps, bc1, bc2_sqrt, gs=1.0):
    """adamw_kernel's expressions in plain f32 on the CPU, one rounding per operation (no FMA contraction)"""
    t = lambda x: torch.as_tensor(x, dtype=torch.float64).to(torch.float32)
    lr, wd, b1, b2, eps, bc1, bc2, gs = (t(x) for x in (lr, wd, b1, b2, eps, bc1, bc2_sqrt, gs))
    gj = g * gs
    m2 = b1 * m + (1 - b1) * gj
    v2 = b2 * v + (1 - b2) * gj * gj
    p2 = p * (1 - lr * wd) - (lr / bc1) * (m2 / (v2.sqrt() / bc2 + eps))
    return p2, m2, v2


def _opt_operands(mix, n=100003, seed=11):
    g_ = torch.Generator().manual_seed(seed)
    p, g, m = torch.randn(n, generator=g_), torch.randn(n, generator=g_), torch.randn(n, generator=g_) * 0.1
    v = torch.rand(n, generator=g_) * 0.01
    if mix == 'cancel':                                  # m' = b1 m + (1 - b1) g cancels to ~1e-6 of its terms
        m = -(1 - f32r(0.9)) / f32r(0.9) * g * (1 + 1e-6 * torch.randn(n, generator=g_))
    elif mix == 'zero':                                  # the denominator is eps
        g, v = torch.zeros(n), torch.zeros(n)
    elif mix == 'tiny':                                  # gj^2 below the normal range
        g, m, v = g * 1e-20, m * 1e-20, v * 1e-40
    elif mix == 'huge':
        g = g * 1e15
    return p, g, m, v


@pytest.mark.parametrize('t', [1, 3, 1000])
@pytest.mark.parametrize('mix', ['random', 'cancel', 'zero', 'tiny', 'huge'])
def test_adamw_ref_passes_a_plain_f32_restatement(mix, t):
    p, g, m, v = _opt_operands(mix)
    bc1, bc2 = bias_corrections(0.9, 0.95, t)
    for gs in (1.0, 0.37):
        kw = dict(_HY, bc1=bc1, bc2_sqrt=bc2, gs=gs)
        for name, o, (r, b) in zip('pmv', _adamw_f32(p, g, m, v, **kw), adamw_ref(p, g, m, v, **kw)):
            assert_within(o, r, b, f"{name}' ({mix}, t = {t}, gs = {gs})")


def _old_opt_criterion(p_bad, v_bad, p_ref, v_ref):
    """test_adamw_and_sumsq's: rel-L2 < 1e-6 on p and v (m was not compared)"""
    return rel_err(p_bad, p_ref) < 1e-6 and rel_err(v_bad, v_ref) < 1e-6


# (corruption, does the old rel-L2 criterion pass it?)
@pytest.mark.parametrize('corruption,old_passes', [('tail element not updated', False), ('chunk with the neighbour group\'s weight decay', False),
                                                   ('bias corrections of t + 1', False), ('m not written', True)])
def test_optimiser_corruptions_are_flagged(corruption, old_passes):
    p, g, m, v = _opt_operands('random')
    t = 3
    bc1, bc2 = bias_corrections(0.9, 0.95, t)
    kw = dict(_HY, bc1=bc1, bc2_sqrt=bc2)
    (pr, bp), (mr, bm), (vr, bv) = adamw_ref(p, g, m, v, **kw)
    pb, mb, vb = (x.clone() for x in _adamw_f32(p, g, m, v, **kw))
    if corruption == 'tail element not updated':         # the last element of the scalar tail (n % 4 = 3)
        pb[-1], mb[-1], vb[-1] = p[-1], m[-1], v[-1]
    elif corruption.startswith('chunk'):                 # one 64-element chunk decayed with wd = 0 (the no-decay group next to it)
        c = slice(64 * 700, 64 * 701)
        pb[c] = _adamw_f32(p[c], g[c], m[c], v[c], **dict(kw, wd=0.0))[0]
    elif corruption.startswith('bias'):
        b1n, b2n = bias_corrections(0.9, 0.95, t + 1)
        pb = _adamw_f32(p, g, m, v, **dict(kw, bc1=b1n, bc2_sqrt=b2n))[0]
    else:
        mb = m.clone()
    assert _old_opt_criterion(pb, vb, pr, vr) == old_passes
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(pb, pr, bp, 'p')
        assert_within(mb, mr, bm, 'm')
        assert_within(vb, vr, bv, 'v')


def test_truncated_shadow_is_flagged_by_the_bit_comparison():
    p = _opt_operands('random')[0]
    good = bf16_bits_ref(p)
    assert torch.equal(good, p.bfloat16().view(torch.int16))          # finite values: torch's own rounding
    trunc = (p.view(torch.int32) >> 16).to(torch.int16)
    n_bad = int((trunc != good).sum())
    assert 0.4 * p.numel() < n_bad < 0.6 * p.numel()                  # half of all values round up
    # the old check, torch.equal with p.bfloat16(), catches this one too; rel-L2 at the bf16 tolerance 4e-3 would not
    assert rel_err(bf16_to_f32_ref(trunc), p) < 4e-3


def test_sumsq_ref_and_chain():
    assert sumsq_chain(1) == 26 and sumsq_chain(1048576) == 26 and sumsq_chain(1048577) == 27 and sumsq_chain(3 * 1048576) == 28
    g_ = torch.Generator().manual_seed(12)
    for n in (1, 5, 100003, 2 * 1048576 + 1027):
        x = torch.randn(n, generator=g_)
        s, b = sumsq_ref(x)
        assert abs(float((x * x).sum()) - s) <= b                      # f32 products, torch's cascaded f32 sum
        assert abs(float((x * x).sum()) * (1 + 3e-6) - s) > b          # a sum 3e-6 off is outside gamma_26 = 1.6e-6
    x = torch.full((4096,), 1e-3)
    x[1234] = 3.0                                                      # one large element among tiny ones
    s, b = sumsq_ref(x)
    assert abs(9.0 - s) > b and abs(float((x * x).sum()) - s) <= b     # dropping the tiny ones is flagged


def test_opt_decision_ref_rules():
    kw = dict(lr=1e-3, wd=0.05, b1=0.9, b2=0.95)
    z = [0] * 6
    r = opt_decision_ref(4.0, 0.0, istate=z, clip=1.0, skip_at=1.5, prescale=1.0, **kw)          # clip before skip_grad: exclusive
    assert r['istate'] == [0, 1, 0, 0, 0, 0] and not r['skip'] and r['state'][1][0] == 2.0
    assert r['state'][2][0] == pytest.approx(1.0 / (2.0 + 1e-6)) and r['state'][5] == f32r(1 - f32r(0.9))
    r = opt_decision_ref(4.0, 0.0, istate=[0, 7, 1, 2, 3, 4], clip=0.0, skip_at=1.5, prescale=1.0, **kw)
    assert r['istate'] == [1, 7, 1, 3, 3, 4] and r['state'][2][0] == 1.0                          # t stays put
    assert (r['state'][5], r['state'][6]) == bias_corrections(0.9, 0.95, 7)
    r = opt_decision_ref(4.0 * 65536 ** 2, 0.0, istate=z, clip=0.0, skip_at=0.0, prescale=0.5, grad_scale=65536.0, **kw)
    assert r['state'][1][0] == 1.0 and r['state'][2][0] == 0.5 / 65536 and r['istate'][:2] == [0, 1]
    r = opt_decision_ref(4.0, 0.0, istate=z, clip=0.0, skip_at=0.0, prescale=1.0, found_inf=1.0, loss=float('inf'), **kw)
    assert r['istate'] == [1, 0, 1, 1, 1, 0]
    r = opt_decision_ref(float('nan'), float('nan'), istate=z, clip=1.0, skip_at=0.0, prescale=1.0, lrwd=(0.5, 0.25), **kw)
    assert r['istate'] == [1, 0, 0, 1, 0, 1] and r['state'][2][0] == 1.0 and (r['state'][3], r['state'][4]) == (0.5, 0.25)
    r = opt_decision_ref(float('inf'), float('nan'), istate=z, clip=1.0, skip_at=0.0, prescale=1.0, **kw)
    assert r['istate'] == [1, 0, 0, 1, 0, 1] and r['state'][2][0] == 0.0


# ---- depth --------------------------------------------------------------------------------------------------------------------
def _depth_f32(x, lo, hi, eps):
    """the kernel's arithmetic on the CPU: fp64 statistics of the sorted slice, the last line in f32"""
    s = torch.sort(x.double(), dim=-1).values[..., lo:hi]
    mu = s.mean(-1, keepdim=True).float()
    var = s.var(-1, unbiased=True, keepdim=True).float()
    return (x - mu) * (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32)))


def _depth_maps(n=1000, seed=13):
    g_ = torch.Generator().manual_seed(seed)
    ties = torch.randint(0, 7, (n,), generator=g_).float() * 0.25 - 0.5          # seven values, long runs: every cut is inside one
    return torch.stack([torch.randn(n, generator=g_) * 3 + 10, -torch.rand(n, generator=g_) * 5 - 1, ties,
                        torch.full((n,), 2.5), (torch.arange(n) % 2).float() * 4 - 1])


@pytest.mark.parametrize('lohi', [(0, 1000), (0, 2), (998, 1000), (100, 900), (499, 501)])
def test_depth_std_ref_passes_a_plain_f32_restatement(lohi):
    x = _depth_maps()
    y, b = depth_std_ref(x, *lohi, 1e-6)
    assert_within(_depth_f32(x, *lohi, 1e-6), y, b, f'depth standardisation, cuts {lohi}', names=('b', 'i'))


def _old_depth_criterion(bad, ref):
    """test_depth_standardize's: max |difference| < 2e-6 max |reference| + 1e-6"""
    return float((bad.double() - ref).abs().max()) < 2e-6 * float(ref.abs().max()) + 1e-6


@pytest.mark.parametrize('corruption,old_passes', [('cut value counted once', False), ('biased variance', False), ('lo + 1', False)])
def test_depth_corruptions_are_flagged(corruption, old_passes):
    x = _depth_maps()[2:3]                                # the map with long runs of ties
    lo, hi = 100, 900
    y, b = depth_std_ref(x, lo, hi, 1e-6)
    s = torch.sort(x.double(), dim=-1).values
    if corruption == 'cut value counted once':            # values strictly between the cuts, each cut value once
        k1, k2 = s[0, lo], s[0, hi - 1]
        sl = torch.cat([s[0][(s[0] > k1) & (s[0] < k2)], k1[None], k2[None]])[None]
    elif corruption == 'biased variance':
        sl = s[:, lo:hi]
    else:
        sl = s[:, lo + 1:hi]
    mu, var = sl.mean(-1, keepdim=True), sl.var(-1, unbiased=corruption != 'biased variance', keepdim=True)
    bad = ((x.double() - mu) / torch.sqrt(var + 1e-6)).float()
    assert _old_depth_criterion(bad, y) == old_passes
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, y, b, corruption)


# ---- bit-exact restatements ----------------------------------------------------------------------------------------------------
def _f(bits):
    """f32 values from their bit patterns"""
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def test_bf16_restatement_known_answers():
    x = _f([0x3f800000, 0x3f808000, 0x3f818000, 0x3f808001, 0x7f7f8000, 0x7f7f7fff, 0xff7f8000, 0x7f800000, 0x7fa00001, 0xffc12345,
            0x00000000, 0x80000000, 0x00008000, 0x00018000, 0x00000001])
    want = [0x3f80, 0x3f80, 0x3f82, 0x3f81, 0x7f80, 0x7f7f, 0xff80, 0x7f80, 0x7fe0, 0xffc1, 0x0000, 0x8000, 0x0000, 0x0002, 0x0000]
    got = [int(b) & 0xffff for b in bf16_bits_ref(x)]
    assert got == want                                   # ties to even both ways, the carry into inf, quieted NaN, subnormals
    back = bf16_to_f32_ref(bf16_bits_ref(x))
    assert [int(b) & 0xffffffff for b in back.view(torch.int32)] == [w << 16 for w in want]
    g_ = torch.Generator().manual_seed(14)
    r = torch.randn(100003, generator=g_) * 1e3
    assert torch.equal(bf16_bits_ref(r), r.bfloat16().view(torch.int16))
    hi, lo = x3_split_ref(r)
    rec = bf16_to_f32_ref(hi).double() + bf16_to_f32_ref(lo).double()
    assert bool(((rec - r.double()).abs() <= r.double().abs() * 2.0 ** -16).all())       # hi + lo keeps 16 bits of x


def test_h16_scale_restatement():
    assert h16_scale_ref(None) == (1.0, 1.0)
    for m in (0.0, 1e-45, 2.0 ** -127, float('inf'), float('nan'), 2.0 ** -120, 2.0 ** -119 * (1 - 2.0 ** -24), 2.0 ** 127, 3e38):
        assert h16_scale_ref(m) == (1.0, 1.0), m
    for k in (-119, -60, 0, 5, 126):
        for f in (1.0, 1.5, 1.999):
            assert h16_scale_ref(2.0 ** k * f) == (2.0 ** (4 - k), 2.0 ** (k - 4))
    assert h16_scale_ref(0.9e-6)[0] == 2.0 ** 25                      # test_h16_gpu's value: 2^-21 <= 0.9e-6 < 2^-20
    x = torch.tensor([65504.0, 65519.996, 65520.0, -65520.0, 1e5, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 6e-8, float('nan')])
    h = f32_to_f16_ref(x)
    assert h[:9].tolist() == [65504.0, 65504.0, float('inf'), float('-inf'), float('inf'), 2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -24]
    assert bool(torch.isnan(h[9]))
    assert f16_to_f32_ref(f32_to_f16_ref(torch.tensor([3e-5]), 2e-5), 2e-5).item() == pytest.approx(3e-5, rel=2.0 ** -11)


def test_fma_and_add_n_restatements():
    g_ = torch.Generator().manual_seed(15)
    x, y = torch.randn(200003, generator=g_), torch.randn(200003, generator=g_)
    a = 0.3
    f = fma_f32_ref(a, x, y)
    exact = torch.tensor(a, dtype=torch.float32).double() * x.double() + y.double()
    assert bool(((f.double() - exact).abs() <= 0.5 * ulp(torch.float32, exact) * (1 + 1e-9)).all())   # correctly rounded
    two = y + torch.tensor(a, dtype=torch.float32) * x
    assert 0 < int((two != f).sum()) < 0.2 * x.numel()                # mul + add differs from the FMA in some elements
    # a tie the fp64 sum alone would double-round: a x = 2^-30 exactly behind a half-ulp of y = 1
    assert float(fma_f32_ref(2.0 ** -15, torch.tensor([2.0 ** -15 + 2.0 ** -38]), torch.tensor([1.0 + 2.0 ** -24 - 2.0 ** -30]))) >= 1.0
    xs = [torch.randn(4096, generator=g_) * 10 ** k for k in range(4)]
    assert torch.equal(add_n_ref(xs), ((xs[0] + xs[1]) + xs[2]) + xs[3])


def test_ops_refuses_a_shadow_dtype_the_optimiser_kernels_do_not_write():
    from multimae_amd import ops
    assert ops._shadow_args(None) == (None, 0)
    for dt, code in ((torch.float32, 0), (torch.bfloat16, 1)):
        t = torch.zeros(8, dtype=dt)
        assert ops._shadow_args(t) == (t.data_ptr(), code)
    for dt in (torch.float16, torch.float64, torch.int16):
        with pytest.raises(TypeError, match='float32 or bfloat16'):
            ops._shadow_args(torch.zeros(8, dtype=dt))


# ---- the input side: patch rows, fused patch embedding, class-embedding gradient, mask sampler ---------------------------------
from helpers import (mask_sample_ref, patch_embed_ref, patch_rows_ref, semseg_emb_grad_bound, semseg_emb_grad_ref,  # noqa: E402
                     token_owner)


def _input_case(B=128, seed=21):
    """two tasks, neither image nor patch square, both with K = 96: class ids 8 x 12 in 2 x 4 patches (E = 12, 7 classes, ids drawn from
    [-1, 7]) at k_off 104, an image 3 x 16 x 24 in 4 x 8 patches at k_off 0; columns 96 .. 104 are a gap, 200 .. 208 a tail.  Every
    token of both tasks is selected, in a random order per sample."""
    g_ = torch.Generator().manual_seed(seed)
    srcs = [dict(data=torch.randint(-1, 8, (B, 8, 12), generator=g_), emb=torch.randn(7, 12, generator=g_), kind=1, C=12, H=8, W=12,
                 ph=2, pw=4, k_off=104, n_cls=7),
            dict(data=torch.randn(B, 3, 16, 24, generator=g_), emb=None, kind=0, C=3, H=16, W=24, ph=4, pw=8, k_off=0, n_cls=0)]
    offs = [0, 12, 24]
    sel = torch.stack([torch.randperm(24, generator=g_) for _ in range(B)])
    return srcs, offs, sel, 208, g_


def _rows_by_index(srcs, offs, sel, Ktot, swap_patch=False, swap_grid=False):
    """patch_rows_kernel's index arithmetic, column by column: (c, i, j) of column k, pixel (py ph + i, px pw + j) of patch p =
    (py, px).  swap_patch decodes (i, j) with ph in pw's place, swap_grid decodes (py, px) with H / ph in W / pw's place (both kept
    inside the image by a modulo, so the wrong kernel reads a wrong pixel, not past the end)."""
    B, n_sel = sel.shape
    out = torch.zeros(B * n_sel, Ktot)
    flat = sel.reshape(-1)
    own = token_owner(flat, offs)
    b = torch.arange(B).repeat_interleave(n_sel)
    for t, s in enumerate(srcs):
        m = own == t
        C, H, W, ph, pw = s['C'], s['H'], s['W'], s['ph'], s['pw']
        p = flat[m] - offs[t]
        nw = H // ph if swap_grid else W // pw
        py, px = (p // nw)[:, None], (p % nw)[:, None]
        kk = torch.arange(C * ph * pw)[None, :]
        c, ij = kk // (ph * pw), kk % (ph * pw)
        q = ph if swap_patch else pw
        y, x = (py * ph + ij // q) % H, (px * pw + ij % q) % W
        bb = b[m][:, None]
        if s['kind'] == 0:
            v = s['data'][bb, c, y, x]
        else:
            ids = s['data'][bb, y, x]
            ok = (ids >= 0) & (ids < s['n_cls'])
            v = torch.where(ok, s['emb'][ids.clamp(0, s['n_cls'] - 1), c], torch.zeros(()))
        out[m, s['k_off']:s['k_off'] + C * ph * pw] = v
    return out


def test_patch_rows_ref_equals_the_index_arithmetic_and_flags_the_swaps():
    srcs, offs, sel, Ktot, _ = _input_case(B=3)
    ref = patch_rows_ref(srcs, offs, sel, Ktot)
    assert torch.equal(ref, _rows_by_index(srcs, offs, sel, Ktot))
    assert bool((ref[:, 96:104] == 0).all()) and bool((ref[:, 200:] == 0).all())            # the gap and the tail
    own = token_owner(sel.reshape(-1), offs)
    assert bool((ref[own == 0, :96] == 0).all()) and bool((ref[own == 1, 104:] == 0).all())    # the other task's segment
    assert not torch.equal(ref, _rows_by_index(srcs, offs, sel, Ktot, swap_patch=True))
    assert not torch.equal(ref, _rows_by_index(srcs, offs, sel, Ktot, swap_grid=True))
    bad = ref.clone()
    bad[5, 64:96] = 0                                        # the last 32 of a segment's 96 columns
    assert not torch.equal(ref, bad)
    srcs[1]['data'][1, 2, 5, 9] = float('nan')               # a copy: NaNs and their payloads come through
    r2 = patch_rows_ref(srcs, offs, sel, Ktot)
    assert int(torch.isnan(r2).sum()) == 1 and torch.equal(r2.view(torch.int32), _rows_by_index(srcs, offs, sel, Ktot).view(torch.int32))


def _embed_operands(srcs, g_, D=32):
    ws = [(torch.randn(D, 96, generator=g_) * 96 ** -0.5).bfloat16() for _ in srcs]
    bs = [torch.randn(D, generator=g_) for _ in srcs]
    poss = [torch.randn(12, D, generator=g_) for _ in srcs]
    return ws, bs, poss, torch.randn(2, D, generator=g_)


def _embed_f32(rows, srcs, ws, bs, poss, offs, sel, glob):
    """the kernel's arithmetic in plain f32 on given patch rows: bf16 operands, f32 products and sums, (acc + bias) + pos"""
    B, n_sel = sel.shape
    D = glob.shape[1]
    flat = sel.reshape(-1)
    own = token_owner(flat, offs)
    xh = rows.bfloat16().float()
    tok = torch.zeros(B * n_sel, D)
    for t, s in enumerate(srcs):
        m = own == t
        tok[m] = (xh[m, s['k_off']:s['k_off'] + 96] @ ws[t].float().t() + bs[t]) + poss[t][flat[m] - offs[t]]
    return torch.cat([tok.view(B, n_sel, D), glob.expand(B, -1, -1)], 1)


def test_patch_embed_ref_passes_a_plain_f32_restatement():
    srcs, offs, sel, Ktot, g_ = _input_case()
    ws, bs, poss, glob = _embed_operands(srcs, g_)
    ref, bound, xh = patch_embed_ref(srcs, ws, bs, poss, offs, sel, glob, 32)
    assert torch.equal(xh, patch_rows_ref(srcs, offs, sel, 200).bfloat16().float())
    out = _embed_f32(_rows_by_index(srcs, offs, sel, Ktot), srcs, ws, bs, poss, offs, sel, glob)
    assert_within(out, ref, bound, 'f32 patch embedding', names=('b', 'r', 'd'))
    assert torch.equal(ref[:, 24:], glob.double().expand(128, -1, -1)) and float(bound[:, 24:].abs().max()) == 0.0
    assert float(bound[:, :24].min()) > 0.0


@pytest.mark.parametrize('corruption,old_passes', [('ph and pw swapped', False), ('H/ph and W/pw swapped', False),
                                                   ('last K chunk of one row dropped', True)])
def test_patch_embed_corruptions_are_flagged(corruption, old_passes):
    """the old criterion: rel_err < 1e-2 over all token rows (test_patch_embed_assemble_vs_oracle's bf16 tolerance)"""
    srcs, offs, sel, Ktot, g_ = _input_case()
    ws, bs, poss, glob = _embed_operands(srcs, g_)
    ref, bound, _ = patch_embed_ref(srcs, ws, bs, poss, offs, sel, glob, 32)
    rows = _rows_by_index(srcs, offs, sel, Ktot, swap_patch=corruption == 'ph and pw swapped', swap_grid=corruption == 'H/ph and W/pw swapped')
    if corruption == 'last K chunk of one row dropped':
        r = 24 * 77 + 23
        k0 = srcs[int(token_owner(sel.reshape(-1)[r:r + 1], offs))]['k_off']
        rows[r, k0 + 64:k0 + 96] = 0                         # 32 of the 96 columns
    bad = _embed_f32(rows, srcs, ws, bs, poss, offs, sel, glob)
    assert (rel_err(bad, ref) < 1e-2) == old_passes
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, ref, bound, corruption, names=('b', 'r', 'd'))


def _emb_grad_f32(d_rows, srcs, offs, sel, swap_patch=False, swap_grid=False, drop_row=None):
    """the class-embedding gradient as a chain of f32 additions, pixel by pixel, with patch_rows_kernel's index arithmetic"""
    s = srcs[0]
    E, H, W, ph, pw = s['C'], s['H'], s['W'], s['ph'], s['pw']
    B, n_sel = sel.shape
    flat = sel.reshape(-1)
    rows = torch.nonzero(token_owner(flat, offs) == 0).reshape(-1)
    p = flat[rows] - offs[0]
    nw = H // ph if swap_grid else W // pw
    q = ph if swap_patch else pw
    ij = torch.arange(ph * pw)[None, :]
    y, x = ((p // nw)[:, None] * ph + ij // q) % H, ((p % nw)[:, None] * pw + ij % q) % W
    ids = s['data'][(rows // n_sel)[:, None], y, x].reshape(-1)
    d = d_rows.clone()
    if drop_row is not None:
        d[rows[drop_row], s['k_off'] + 64:s['k_off'] + 96] = 0
    terms = d[rows, s['k_off']:s['k_off'] + E * ph * pw].reshape(-1, E, ph * pw).permute(0, 2, 1).reshape(-1, E)
    ok = (ids >= 0) & (ids < s['n_cls'])
    tab = torch.zeros(s['n_cls'], E)
    for c in range(s['n_cls']):
        tc = terms[ok & (ids == c)]
        for i in range(tc.shape[0]):
            tab[c] += tc[i]
    return tab


def _emb_grad_case():
    srcs, offs, sel, Ktot, g_ = _input_case(B=4)
    srcs[0]['data'][srcs[0]['data'] == 3] = 4                 # class 3 is never hit
    d_rows = torch.randn(4 * 24, 216, generator=g_)           # ld 216 > Ktot
    s = srcs[0]
    kw = dict(E=s['C'], ph=s['ph'], pw=s['pw'], k_off=s['k_off'], tok_off=0, n_patches=12, n_cls=7)
    return srcs, offs, sel, d_rows, kw


def test_semseg_emb_grad_ref_passes_a_plain_f32_restatement():
    srcs, offs, sel, d_rows, kw = _emb_grad_case()
    grad, n, S = semseg_emb_grad_ref(d_rows, srcs[0]['data'], sel, **kw)
    bound = semseg_emb_grad_bound(grad, n, S)
    assert float(n.sum()) == float(((srcs[0]['data'] >= 0) & (srcs[0]['data'] < 7)).sum())      # every token is selected: every valid pixel is a term
    assert float(n[3]) == 0 and float(grad[3].abs().max()) == 0.0 and float(bound[3].max()) == 0.0
    assert_within(_emb_grad_f32(d_rows, srcs, offs, sel), grad, bound, 'f32 class-embedding gradient', names=('class', 'e'))


@pytest.mark.parametrize('corruption', ['ph and pw swapped', 'H/ph and W/pw swapped', 'last K chunk of one row dropped'])
def test_semseg_emb_grad_corruptions_are_flagged(corruption):
    srcs, offs, sel, d_rows, kw = _emb_grad_case()
    grad, n, S = semseg_emb_grad_ref(d_rows, srcs[0]['data'], sel, **kw)
    bad = _emb_grad_f32(d_rows, srcs, offs, sel, swap_patch=corruption == 'ph and pw swapped', swap_grid=corruption == 'H/ph and W/pw swapped',
                        drop_row=5 if corruption == 'last K chunk of one row dropped' else None)
    with pytest.raises(AssertionError, match='outside the bound'):
        assert_within(bad, grad, semseg_emb_grad_bound(grad, n, S), corruption, names=('class', 'e'))


def test_mask_sample_ref_known_answer_and_the_oracle():
    import multimae_oracle as orc
    # the quirk: order = argsort(noise) = [1, 2, 0, 3]; POSITIONS 0 and 2 hold order < 2, so tokens 0 and 2 are pre-selected (not 1 and 2)
    m, k, r = mask_sample_ref(torch.tensor([[2]]), torch.tensor([[0.3, 0.1, 0.2, 0.4]]), torch.tensor([[0.5, 0.6, 0.7, 0.8]]), [0, 4], 2)
    assert m.tolist() == [[0, 1, 0, 1]] and k.tolist() == [[0, 2]] and r.tolist() == [[0, 2, 1, 3]]
    g_ = torch.Generator().manual_seed(22)
    for offs in ([0, 49, 113, 309], [0, 16, 16, 40], [0, 7]):
        T, N, B = len(offs) - 1, offs[-1], 9
        tn, an = torch.rand(B, N, generator=g_), torch.rand(B, N, generator=g_)
        tn[1, 1:5] = tn[1, 0]                                 # ties in both arrays
        an[2, 3:6] = an[2, 0]
        spt = torch.stack([torch.tensor([int(torch.randint(0, offs[t + 1] - offs[t] + 1, (1,), generator=g_)) for t in range(T)]) for _ in range(B)])
        for n_keep in (0, 1, N // 3, N):
            mine = mask_sample_ref(spt, tn, an, offs, n_keep)
            theirs = orc.masks_from_noise(spt, [tn[:, offs[t]:offs[t + 1]] for t in range(T)], an, n_keep)
            assert all(torch.equal(a, b) for a, b in zip(mine, theirs)), (offs, n_keep)
            assert mine[0].dtype == mine[1].dtype == mine[2].dtype == torch.int64
            assert torch.equal(torch.sort(mine[2], 1).values, torch.arange(N).expand(B, -1)) and bool((mine[0] == 0).sum(1).eq(n_keep).all())


def test_guarded_int64_buffer_flags_a_write_into_one_guard_element():
    gb = Guarded(5, 7, 9, torch.int64, 'cpu')
    gb.view.copy_(torch.arange(35).view(5, 7))
    gb.intact()
    assert int(gb.flat[0]) == 0xffa5ffa5ffa5ffa5 - 2 ** 64
    gb.full[2, 8] = 0
    with pytest.raises(AssertionError, match=r'row 2, col 8'):
        gb.intact()
    gb2 = Guarded(5, 7, 7, torch.int64, 'cpu')
    gb2.flat[gb2.off - 1] = 3
    with pytest.raises(AssertionError, match='guard zone before'):
        gb2.intact()


# ----------------------------------------------------------------------------------------------
# The stage references of a transformer block (tests/test_composite_gpu.py composes them against mmae_block_fwd / mmae_block_bwd)
def _plain_block(x, P, heads, eps, B, N, dp1=None, dp2=None):
    """a pre-LN block written out plainly in torch (fp64 autograd is the reference of block_ref)"""
    n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b = P
    D = x.shape[1]
    hd = D // heads
    F = torch.nn.functional
    row = lambda s: 1.0 if s is None else s.double().repeat_interleave(N)[:, None]
    qkv = F.linear(F.layer_norm(x, (D,), n1w, n1b, eps), qkvw, qkvb).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = ((qkv[0] @ qkv[1].transpose(-1, -2)) * hd ** -0.5).softmax(-1) @ qkv[2]
    x1 = x + row(dp1) * F.linear(a.transpose(1, 2).reshape(B * N, D), projw, projb)
    h = F.linear(F.layer_norm(x1, (D,), n2w, n2b, eps), fc1w, fc1b)
    return x1 + row(dp2) * F.linear(h * 0.5 * (1 + torch.erf(h / math.sqrt(2))), fc2w, fc2b), x1


def _block_params(D, Hd, g):
    shapes = [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (Hd, D), (Hd,), (D, Hd), (D,)]
    return [(torch.randn(s, generator=g) * (0.1 if len(s) == 2 else 0.2) + (1.0 if i in (0, 6) else 0.0)).double() for i, s in enumerate(shapes)]


@pytest.mark.parametrize('dp', [False, True])
def test_block_stage_references_compose_to_autograd_of_a_plain_block(dp):
    from helpers import block_ref
    g = torch.Generator().manual_seed(5)
    B, N, D, heads, Hd = 2, 7, 16, 2, 24
    P = [p.requires_grad_(True) for p in _block_params(D, Hd, g)]
    x = (torch.randn(B * N, D, generator=g) + 0.3).double().requires_grad_(True)
    dy = torch.randn(B * N, D, generator=g).double()
    dp1 = torch.tensor([0.0, 1.25]) if dp else None
    dp2 = torch.tensor([2.0, 0.0]) if dp else None
    y, x1 = _plain_block(x, P, heads, 1e-6, B, N, dp1, dp2)
    y.backward(dy)
    o = block_ref(x.detach(), [p.detach() for p in P], heads, 1e-6, B, N, dy=dy, dp1=dp1, dp2=dp2)
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12, msg=lambda m: f'{what}: {m}')
    close(o['x1'], x1.detach(), 'x1')
    close(o['x2'], y.detach(), 'x2')
    close(o['dx0'], x.grad, 'dx0')
    names = ['g_n1_w', 'g_n1_b', 'g_qkv_w', 'g_qkv_b', 'g_proj_w', 'g_proj_b', 'g_n2_w', 'g_n2_b', 'g_fc1_w', 'g_fc1_b', 'g_fc2_w', 'g_fc2_b']
    for n, p in zip(names, P):
        close(o[n], p.grad, n)
    close(o['g_cs'], x.grad.sum(0), 'g_cs')
    if dp:                                             # a dropped sample: its rows pass through, its branch gets no gradient
        assert torch.equal(o['x1'][:N], x.detach()[:N]) and torch.equal(o['x2'][N:], o['x1'][N:])
        assert not o['d_hpre'][N:].any() and not o['d_ao'][:N].any()


def test_layernorm_ref_bounds_hold_for_an_fp32_evaluation_and_flag_a_stale_statistic():
    from helpers import layernorm_ref
    g = torch.Generator().manual_seed(6)
    R, D = 100, 128
    x = torch.randn(R, D, generator=g) * 2 + 0.5
    w, b, dy, dxin = torch.randn(D, generator=g), torch.randn(D, generator=g), torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    ln = layernorm_ref(x, w, b, 1e-6)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-6)          # an fp32 evaluation: inside the bounds
    y.backward(dy)
    assert_within(y, ln.y, ln.b_y(torch.float32), 'y f32')
    assert_within(y.bfloat16(), ln.y, ln.b_y(torch.bfloat16), 'y bf16')
    r = ln.bwd(dy, dxin, torch.bfloat16)
    assert_within(xr.grad + dxin, *r['dx'], 'dx')
    assert_within((xr.grad + dxin).bfloat16(), *r['dx_act'], 'dx bf16')
    assert_within(wr.grad, *r['dgamma'], 'dgamma')
    assert_within(br.grad, *r['dbeta'], 'dbeta')
    stale = y.detach().clone()
    stale[17] = (x[17] - x[16].mean()) * float(ln.rstd[17]) * w + b      # row 17 normalised with row 16's mean
    with pytest.raises(AssertionError, match='row=17|\\(17,'):
        assert_within(stale, ln.y, ln.b_y(torch.float32), 'y', names=('row', 'col'))


def test_linear_and_colsum_references_pass_the_rounded_exact_result_and_flag_one_wrong_bias_entry():
    from helpers import colsum_ref, gelu_ref, linear_dw_ref, linear_dx_ref, linear_ref
    g = torch.Generator().manual_seed(7)
    M, N, K = 100, 48, 128
    x, w = torch.randn(M, K, generator=g).bfloat16(), (torch.randn(N, K, generator=g) * 0.1).bfloat16()
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    y, by, (lin, e) = linear_ref(x, w, bias, resid)
    assert_within(y.float(), y, by, 'linear f32')
    y16, by16, _ = linear_ref(x, w, bias, out_dtype=torch.bfloat16)
    assert_within(y16.bfloat16(), y16, by16, 'linear bf16')
    bad = y.float().clone()
    bad[:, 5] += 4 * float(by[:, 5].max())
    with pytest.raises(AssertionError):
        assert_within(bad, y, by, 'linear, one bias entry off')
    dy = torch.randn(M, N, generator=g).bfloat16()
    pre = torch.randn(M, K, generator=g).bfloat16()
    r, b, _ = linear_dx_ref(dy, w, torch.bfloat16, dgelu_of=pre)
    assert_within(r.bfloat16(), r, b, 'dgelu')
    r2, b2, _ = linear_dx_ref(dy, w, torch.bfloat16, mul=gelu_ref(pre)[1])
    assert torch.equal(r, r2)
    (dw, bw), (db, bb) = linear_dw_ref(dy, x)
    assert_within(dw.float(), dw, bw, 'dw')
    assert_within(db.float(), db, bb, 'db')
    g0 = (torch.randn(N, K, generator=g), torch.randn(N, generator=g))
    (dwa, bwa), (dba, bba) = linear_dw_ref(dy, x, g0=g0)
    assert torch.equal(dwa, dw + g0[0].double()) and bool((bwa >= bw).all()) and bool((bba >= bb).all())
    s, bs = colsum_ref(dy)
    assert_within(dy.float().sum(0), s, bs, 'column sums in fp32')
    wrong = s.float().clone()
    wrong[3] = float(dy.float()[:-1, 3].sum())          # one row missing from one column
    with pytest.raises(AssertionError):
        assert_within(wrong, s, bs, 'column sums, one row short')


def _tiny_adapter(depth, q_task, seed=3):
    g = torch.Generator().manual_seed(seed)
    B, T, nh, nw, n_keep, G, Denc, D, heads, Hd, C, ph, pw = 2, 3, 2, 3, 5, 1, 8, 8, 2, 12, 2, 2, 2
    n_q, KP = nh * nw, C * ph * pw
    rn = lambda *s: torch.randn(*s, generator=g).double() * 0.4
    lin = lambda n, k: [rn(n, k), rn(n)]
    ln = lambda: [1 + rn(D), rn(D)]
    params = [rn(D), rn(D), None, rn(D)] + lin(D, D) + lin(2 * D, D) + lin(D, D) + ln() + ln() + ln() + lin(Hd, D) + lin(D, Hd)
    for _ in range(depth):
        params += ln() + lin(3 * D, D) + lin(D, D) + ln() + lin(Hd, D) + lin(D, Hd)
    params += lin(KP, D) + lin(D, Denc)
    perm = torch.stack([torch.randperm(T * n_q, generator=g) for _ in range(B)])
    kw = dict(T=T, q_task=q_task, G=G, D=D, heads=heads, depth=depth, pos=rn(n_q, D), offs=[0, n_q, 2 * n_q, 3 * n_q], C=C, nh=nh, nw=nw, ph=ph,
              pw=pw, eps=1e-6)
    return rn(B, n_keep + G, Denc), perm[:, :n_keep].contiguous(), torch.argsort(perm, 1), params, kw


@pytest.mark.parametrize('q_task', [-1, 1])
def test_decoder_rows_ref_against_the_formulae_written_as_loops(q_task):
    from helpers import decoder_rows_ref
    g = torch.Generator().manual_seed(4)
    B, T, n_q, n_keep, G, D = 2, 3, 6, 5, 1, 4
    offs = [0, 6, 12, 18]
    ctx, mask, pos = torch.randn(B, n_keep + G, D, generator=g).double(), torch.randn(D, generator=g).double(), torch.randn(n_q, D, generator=g).double()
    temb = [torch.randn(D, generator=g).double(), None, torch.randn(D, generator=g).double()]
    perm = torch.stack([torch.randperm(T * n_q, generator=g) for _ in range(B)])
    keep, restore = perm[:, :n_keep].contiguous(), torch.argsort(perm, 1)
    q, c = decoder_rows_ref(ctx, keep, restore, mask, temb, pos, offs, q_task, G, n_q)
    te = lambda t: 0 if temb[t] is None else temb[t]
    for b in range(B):
        for j in range(n_q):
            if q_task < 0:
                want = mask + pos[j]
            else:
                r = int(restore[b, offs[q_task] + j])
                want = (ctx[b, r] if r < n_keep else mask) + te(q_task) + pos[j]
            assert torch.equal(q[b, j], want)
        for r in range(n_keep):
            t = int(keep[b, r]) // n_q
            assert torch.equal(c[b, r], ctx[b, r] + te(t) + pos[int(keep[b, r]) - offs[t]])
        assert torch.equal(c[b, n_keep:], ctx[b, n_keep:])
    if q_task >= 0:                                   # every kept token of the query task is looked up at its own rank
        assert any(int(restore[b, offs[q_task] + j]) < n_keep for b in range(B) for j in range(n_q))


def test_adapter_ref_blocks_are_block_ref_and_its_gradients_match_finite_differences():
    from helpers import adapter_ref, block_ref, plain_block
    g = torch.Generator().manual_seed(8)
    P = _block_params(16, 24, g)
    x = torch.randn(14, 16, generator=g).double()
    torch.testing.assert_close(plain_block(x, P, 2, 1e-6, 2, 7), block_ref(x, P, 2, 1e-6, 2, 7)['x2'], rtol=1e-10, atol=1e-12)
    enc, keep, restore, params, kw = _tiny_adapter(depth=1, q_task=1)
    d_img = torch.randn(2, 2, 4, 6, generator=g).double()
    img, pat, d_enc, grads = adapter_ref(enc, keep, restore, params, d_img=d_img, **kw)
    assert grads[2] is None and img.shape == (2, 2, 4, 6)
    loss = lambda e, ps: float((adapter_ref(e, keep, restore, ps, **kw)[0] * d_img).sum())
    h = 1e-6

    def fd(bump):                                      # central difference of <img, d_img> along one coordinate
        return (loss(*bump(+h)) - loss(*bump(-h))) / (2 * h)
    for idx in [(0, 0, 0), (1, 3, 5), (1, 5, 7)]:      # a kept token of each sample, the global token
        def bump(s, idx=idx):
            e = enc.clone()
            e[idx] += s
            return e, params
        assert fd(bump) == pytest.approx(float(d_enc[idx]), rel=1e-5, abs=1e-8)
    for i in (0, 1, 4, 9, 17, 20, len(params) - 4, len(params) - 1):      # mask token, a task embedding, q.w, ctxn.b, fc1.w, block n1.b, out_proj.w, pc.b
        flat = 1 if params[i].numel() > 1 else 0
        def bump(s, i=i, flat=flat):
            ps = [None if p is None else p.clone() for p in params]
            ps[i].view(-1)[flat] += s
            return enc, ps
        assert fd(bump) == pytest.approx(float(grads[i].reshape(-1)[flat]), rel=1e-5, abs=1e-8), i
