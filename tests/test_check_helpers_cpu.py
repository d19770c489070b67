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
