"""GPU: the tiled bf16 attention kernels (attention.hip: attn_fwd_tiled_kernel, attn_bwd_tiled_dq_kernel, attn_bwd_tiled_dkdv_kernel)
for sequences beyond 256 tokens, through ops.attention_fwd / attention_bwd, the raw C ABI, the block / stack composites and a MultiViT
fine-tuning step.  Element-wise checks use helpers.attention_bounds AS IT IS with the rounding points of the 'fused' entry of
test_kernels_gpu._ATTN_ROUNDING, restated here: u_in = 0 (bf16 operands multiply exactly into fp32), u_p = 2^-8 (P and dS are rounded
to bf16 right before their MFMA).  The online rescale of the forward needs no extra allowance (checked on an fp32 emulation of the
algorithm before the kernels were written: worst error / bound 0.53 for o, 0.32 dq, 0.38 dk, 0.43 dv, 0.03 lse)."""
import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, ops
from multimae_amd.ops import AttnView
from helpers import Guarded, assert_within, attention_bounds, rel_err
from test_kernels_gpu import _ATTN_ROUNDING, _attention_packed, _heads, bf

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U_IN, U_P = 0.0, 2.0 ** -8
assert _ATTN_ROUNDING['fused'] == (U_IN, U_P)


def _bounds(B, H, Nq, Nk, hd, q, k, v, do):
    f = lambda t, n: _heads(t.to(DEV), B, n, H, hd)
    return attention_bounds(f(q, Nq), f(k, Nk), f(v, Nk), f(do, Nq), hd ** -0.5, u_in=U_IN, u_p=U_P, out_dtype=torch.bfloat16)


def _within(r, outs, lse, what, B, H, Nq):
    for name, got in outs.items():
        ref, bd = r[name]
        assert_within(got, ref, bd, f'{what}: {name}', names=('bh', 'row', 'd'))
    if lse is not None:
        ref, bd = r['lse']
        assert_within(lse.reshape(B * H, Nq), ref, bd, f'{what}: lse', names=('bh', 'q'))


def _operands(B, H, Nq, Nk, hd, amp, seed):
    D = H * hd
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randn(B * n, D, generator=g) * amp for n in (Nq, Nk))
    v, do = torch.randn(B * Nk, D, generator=g), torch.randn(B * Nq, D, generator=g)
    return tuple(bf(t).float() for t in (q, k, v, do))


# (B, H, Nq, Nk, hd, scale of q and k)
GEOMS = [(1, 2, 257, 257, 64, 2), (1, 1, 256, 257, 32, 2), (1, 1, 257, 33, 64, 2), (2, 2, 300, 1025, 32, 2), (1, 2, 383, 385, 64, 2),
         (1, 1, 513, 511, 32, 2), (1, 12, 1025, 1025, 64, 2), (1, 2, 3201, 3201, 64, 2), (1, 1, 1025, 1, 64, 2), (1, 2, 1025, 1025, 64, 4)]


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_tiled_packed_guarded_per_element(geom):
    """Random bf16 operands with peaky scores (q and k x2, one case x4): q inside a packed qkv with NaN columns beside it, k | v inside a
    packed kv, outputs in Guarded buffers; o, lse, dq, dk, dv per element within attention_bounds; the state tag is 'fused'."""
    B, H, Nq, Nk, hd, amp = geom
    q, k, v, do = _operands(B, H, Nq, Nk, hd, amp, Nq * 7 + Nk + amp)
    outs, lse = _attention_packed('fused', B, H, Nq, Nk, hd, q, k, v, do)
    assert lse is not None, 'state tag is not "fused": the sequence went down the batched-GEMM path'
    assert lse.shape == (B, H, Nq) and lse.dtype == torch.float32
    _within(_bounds(B, H, Nq, Nk, hd, q, k, v, do), outs, lse, f'tiled {geom}', B, H, Nq)


@pytest.mark.parametrize('geom', [(1, 2, 300, 530, 64), (1, 1, 257, 1025, 32), (2, 2, 515, 259, 64)], ids=lambda g: 'x'.join(map(str, g)))
def test_tiled_one_hot_probe_across_key_tiles(geom):
    """The construction of test_kernels_gpu.test_attention_one_hot_probe (margin 30) with the chosen keys 0, 127, 128, 129, 255, 256, 257
    and Nk - 1: the running maximum arrives in the first, a middle and the last 128-key tile, and on both sides of every tile edge.
    o is bit-equal to the chosen key's v row, dv lands on exactly the chosen rows, lse, dq, dk within their bounds."""
    B, H, Nq, Nk, hd = geom
    D, sc = H * hd, hd ** -0.5
    g = torch.Generator().manual_seed(Nq * 1000 + Nk)
    chosen = sorted({c for c in (0, 127, 128, 129, 255, 256, 257, Nk - 1) if c < Nk})
    assert len(chosen) <= 8
    a = 8.0
    b = 30.0 / (a * sc)
    k = torch.zeros(B * Nk, H, hd)
    k[..., 8:] = bf(torch.randn(B * Nk, H, hd - 8, generator=g) * 0.5).float()
    kr = k.view(B, Nk, H, hd)
    for i, c in enumerate(chosen):
        kr[:, c, :, i] = a                                            # key c alone has a component on dimension i
    pick = torch.tensor(chosen)[torch.arange(Nq) % len(chosen)]      # query row r selects key pick[r]
    q = torch.zeros(B, Nq, H, hd)
    q[:, torch.arange(Nq), :, (torch.arange(Nq) % len(chosen))] = bf(torch.tensor(b)).float()
    v = torch.randn(B * Nk, D, generator=g).sign() * (1 + torch.rand(B * Nk, D, generator=g))
    v = bf(v).float()                                                 # |v| in [1, 2]
    do = torch.zeros(B, Nq, H, hd)
    do[:, :, :, 0] = bf(torch.randn(B, Nq, H, generator=g)).float()
    q, k, do = q.reshape(B * Nq, D), k.reshape(B * Nk, D), do.reshape(B * Nq, D)
    outs, lse = _attention_packed('fused', B, H, Nq, Nk, hd, q, k, v, do)
    assert lse is not None, 'state tag is not "fused"'
    what = f'tiled one-hot {geom}'
    want = _heads(v.to(DEV), B, Nk, H, hd)[:, pick.to(DEV)]         # [B * H][Nq][hd]: the chosen key's v row
    assert_within(outs['o'], want, 0.0, what + ': o', names=('bh', 'q', 'd'))
    # dv on exactly the chosen rows (the others get e^-30 of a dO row: inside the bound's ulp), dq, dk, lse per element
    _within(_bounds(B, H, Nq, Nk, hd, q, k, v, do), {'dv': outs['dv'], 'dq': outs['dq'], 'dk': outs['dk']}, lse, what, B, H, Nq)
    unchosen = torch.ones(Nk, dtype=torch.bool)
    unchosen[torch.tensor(chosen)] = False
    assert float(outs['dv'][:, unchosen.to(DEV)].abs().max()) <= 1e-10, 'dv reached a key no query selected'


@pytest.mark.parametrize('hd', [32, 64])
def test_tiled_raw_abi_batch_gap_rows(hd):
    """mmae_attn_fwd_tiled / mmae_attn_bwd_tiled called directly with batch strides larger than N x row stride: NaN rows between the
    batches of q, k, v, o and dO.  Tail rows of the last tiles must be zero-filled, not read; the outputs' gap rows stay untouched."""
    lib = _lib.load()
    B, H, Nq, Nk, gap = 2, 2, 300, 530, 5
    D, ld = H * hd, H * hd + 8
    g = torch.Generator().manual_seed(hd)

    def gapped(N, vals):
        t = torch.full((B, N + gap, ld), float('nan'))
        t[:, :N, :D] = vals.view(B, N, D)
        return t.reshape(B * (N + gap), ld).to(DEV, torch.bfloat16)

    q, k, v, do = (bf(torch.randn(B * n, D, generator=g) * s).float() for n, s in ((Nq, 2), (Nk, 2), (Nk, 1), (Nq, 1)))
    qd, kd, vd, dod = gapped(Nq, q), gapped(Nk, k), gapped(Nk, v), gapped(Nq, do)
    sbq, sbk = (Nq + gap) * ld, (Nk + gap) * ld
    O, dQ = Guarded(B * (Nq + gap), D, ld, torch.bfloat16, DEV), Guarded(B * (Nq + gap), D, ld, torch.bfloat16, DEV)
    dK, dV = Guarded(B * (Nk + gap), D, ld, torch.bfloat16, DEV), Guarded(B * (Nk + gap), D, ld, torch.bfloat16, DEV)
    lse = torch.full((B, H, Nq), float('nan'), device=DEV)
    delta = Guarded(1, B * H * Nq, B * H * Nq, torch.float32, DEV)
    sc = hd ** -0.5
    _lib.check(lib.mmae_attn_fwd_tiled(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), O.full.data_ptr(), lse.data_ptr(), B, H, Nq, Nk, hd,
                                       sbq, ld, sbk, ld, sbk, ld, sbq, ld, sc, ops._stream()), 'attn_fwd_tiled')
    _lib.check(lib.mmae_attn_bwd_tiled(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), O.full.data_ptr(), dod.data_ptr(), lse.data_ptr(),
                                       delta.full.data_ptr(), dQ.full.data_ptr(), dK.full.data_ptr(), dV.full.data_ptr(), B, H, Nq, Nk, hd,
                                       sbq, ld, sbk, ld, sbk, ld, sbq, ld, sbq, ld, sbk, ld, sbk, ld, sc, ops._stream()), 'attn_bwd_tiled')
    torch.cuda.synchronize()
    delta.intact('delta')
    rows = lambda G, N: G.view.view(B, N + gap, D)
    for G, N, name in ((O, Nq, 'o'), (dQ, Nq, 'dq'), (dK, Nk, 'dk'), (dV, Nk, 'dv')):
        G.intact(name)
        assert bool((rows(G, N)[:, N:].contiguous().view(torch.int16) == -91).all()), f'{name}: a gap row between batches was written'
    dense = lambda G, N: rows(G, N)[:, :N].reshape(B * N, D)
    outs = {name: _heads(dense(G, N), B, N, H, hd) for G, N, name in ((O, Nq, 'o'), (dQ, Nq, 'dq'), (dK, Nk, 'dk'), (dV, Nk, 'dv'))}
    r = _bounds(B, H, Nq, Nk, hd, q, k, v, do)
    _within(r, outs, lse, f'tiled raw ABI gap rows hd {hd}', B, H, Nq)
    # delta = sum_j P_ij dP_ij of the fp64 reference, to the dS bound's own delta term (loosely: 1e-2 of the row's |P| . |dP|)
    P = r['P']
    dP = _heads(do.to(DEV), B, Nq, H, hd).double() @ _heads(v.to(DEV), B, Nk, H, hd).double().transpose(-1, -2)
    assert_within(delta.view.view(B * H, Nq), (P * dP).sum(-1), 1e-2 * (P * dP.abs()).sum(-1) + 1e-6, 'delta', names=('bh', 'q'))


def test_tiled_rejects_what_it_cannot_index():
    lib = _lib.load()
    t = torch.zeros(4096, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    call = lambda hd, sr: lib.mmae_attn_fwd_tiled(p, p, p, p, lse.data_ptr(), 1, 1, 1, 1, hd, 0, sr, 0, sr, 0, sr, 0, sr, 1.0, ops._stream())
    assert call(48, 64) != 0
    assert call(64, 68) != 0                                           # not a multiple of 8
    assert call(64, (1 << 22) + 8) != 0 and b'32-bit' in lib.mmae_last_error()
    assert call(64, 64) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('geom', [(2, 2, 300, 1025, 32), (1, 2, 383, 385, 64)], ids=lambda g: 'x'.join(map(str, g)))
def test_tiled_bit_reproducible(geom):
    B, H, Nq, Nk, hd = geom
    q, k, v, do = _operands(B, H, Nq, Nk, hd, 2, 11)
    a, lse_a = _attention_packed('fused', B, H, Nq, Nk, hd, q, k, v, do)
    b, lse_b = _attention_packed('fused', B, H, Nq, Nk, hd, q, k, v, do)
    assert lse_a is not None and torch.equal(lse_a, lse_b)
    for name in ('o', 'dq', 'dk', 'dv'):
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize('n,ld', [(257, 264), (1025, 1032), (300, 300)])
def test_softmax_long_rows(n, ld):
    """mmae_softmax_fwd / _bwd on rows longer than 256 (the materialised-score path at these sequence lengths): the per-element bounds of
    test_kernels_gpu.test_softmax_colsum_cast_transpose, guarded outputs, zeros in the ld padding."""
    from helpers import gamma, ulp
    torch.manual_seed(n)
    rows, u = 37, 2.0 ** -24
    S = torch.randn(rows, ld) * 3
    Pg = Guarded(rows, ld, ld, torch.float32, DEV, fill=torch.full((rows, ld), 7.0))
    P = Pg.view
    ops.softmax_fwd(S.to(DEV), P, rows, n, 0.125)
    s64 = S[:, :n].double().to(DEV) * 0.125
    p64 = torch.softmax(s64, -1)
    bP = p64 * (4 * u * s64.abs().amax(1, keepdim=True) + gamma(n) + 2.0 ** -21)
    assert_within(P[:, :n], p64, bP + ulp(torch.float32, p64), 'softmax P', names=('row', 'col'))
    assert n == ld or float(P[:, n:].abs().max()) == 0.0
    Pg.intact('softmax P')
    dP = torch.randn(rows, ld)
    dSg = Guarded(rows, ld, ld, torch.float32, DEV, fill=torch.full((rows, ld), 7.0))
    dS = dSg.view
    ops.softmax_bwd(P, dP.to(DEV), dS, rows, n, 0.125)
    Pk, dPd = P[:, :n].double(), dP[:, :n].double().to(DEV)
    delta = (Pk * dPd).sum(1, keepdim=True)
    dS64 = 0.125 * Pk * (dPd - delta)
    bS = 0.125 * Pk * (3 * u * ((dPd - delta).abs() + delta.abs()) + gamma(n) * (Pk * dPd.abs()).sum(1, keepdim=True))
    assert_within(dS[:, :n], dS64, bS + ulp(torch.float32, dS64.abs() + bS), 'softmax dS', names=('row', 'col'))
    assert n == ld or float(dS[:, n:].abs().max()) == 0.0
    dSg.intact('softmax dS')


def test_tiled_agrees_with_the_gemm_path():
    """(2, 12, 1025, 1025, 64): the tiled kernels and the batched-GEMM path (set_fused_attention(False), what ran before) are both inside the
    per-element bounds."""
    B, H, Nq, Nk, hd = 2, 12, 1025, 1025, 64
    q, k, v, do = _operands(B, H, Nq, Nk, hd, 2, 5)
    t, lse = _attention_packed('fused', B, H, Nq, Nk, hd, q, k, v, do)
    g, none = _attention_packed('gemm', B, H, Nq, Nk, hd, q, k, v, do)
    assert lse is not None and none is None
    between = {n: rel_err(t[n], g[n]) for n in t}
    print('tiled vs gemm rel_err:', between)
    r = _bounds(B, H, Nq, Nk, hd, q, k, v, do)
    try:
        _within(r, t, lse, 'tiled', B, H, Nq)
        _within(r, g, None, 'gemm', B, H, Nq)
    except AssertionError as e:
        raise AssertionError(f'{e}\nrel_err tiled vs gemm: {between}') from None


def test_dispatch_at_256_is_bit_equal_to_the_resident_kernel():
    """At N = 256 ops.attention_fwd / attention_bwd give bit for bit what mmae_attn_fwd / mmae_attn_bwd give when called directly."""
    lib = _lib.load()
    B, H, N, hd = 2, 2, 256, 64
    D, sc = H * hd, hd ** -0.5
    q, k, v, do = (t.to(DEV, torch.bfloat16) for t in _operands(B, H, N, N, hd, 2, 3))
    vw = lambda t: AttnView(t, 0, D, N)
    o1, dq1, dk1, dv1 = (torch.zeros(B * N, D, device=DEV, dtype=torch.bfloat16) for _ in range(4))
    st = ops.attention_fwd(vw(q), vw(k), vw(v), vw(o1), B, H, hd, sc)
    assert st[0] == 'fused'
    ops.attention_bwd(vw(q), vw(k), vw(v), st, vw(o1), vw(do), vw(dq1), vw(dk1), vw(dv1), B, H, hd, sc)
    o2, dq2, dk2, dv2 = (torch.zeros(B * N, D, device=DEV, dtype=torch.bfloat16) for _ in range(4))
    lse2 = torch.zeros(B, H, N, device=DEV)
    s = [N * D, D]
    _lib.check(lib.mmae_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o2.data_ptr(), lse2.data_ptr(), B, H, N, N, hd, *(s * 4), sc, ops._stream()), 'attn_fwd')
    _lib.check(lib.mmae_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o2.data_ptr(), do.data_ptr(), lse2.data_ptr(), dq2.data_ptr(), dk2.data_ptr(),
                                 dv2.data_ptr(), B, H, N, N, hd, *(s * 7), sc, ops._stream()), 'attn_bwd')
    torch.cuda.synchronize()
    for a, b, name in ((o1, o2, 'o'), (st[1], lse2, 'lse'), (dq1, dq2, 'dq'), (dk1, dk2, 'dk'), (dv1, dv2, 'dv')):
        assert torch.equal(a, b), name


def test_nothing_of_size_nq_nk_is_allocated():
    """(2, 12, 2049, 2049, 64), every output allocated by the caller first: forward + backward raise the peak by less than 8 MB (lse + delta
    are 0.4 MB together, the rest is allocator granularity).  The GEMM path needs 404 MB for S alone here -- asserted too, so the cap
    discriminates."""
    B, H, N, hd = 2, 12, 2049, 64
    D, sc = H * hd, hd ** -0.5
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * N, 3 * D, generator=g).to(DEV, torch.bfloat16)
    do = torch.randn(B * N, D, generator=g).to(DEV, torch.bfloat16)
    o = torch.empty(B * N, D, device=DEV, dtype=torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    vw = lambda t, c: AttnView(t, c, t.shape[1], N)

    def rise():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        st = ops.attention_fwd(vw(qkv, 0), vw(qkv, D), vw(qkv, 2 * D), vw(o, 0), B, H, hd, sc)
        ops.attention_bwd(vw(qkv, 0), vw(qkv, D), vw(qkv, 2 * D), st, vw(o, 0), vw(do, 0), vw(dqkv, 0), vw(dqkv, D), vw(dqkv, 2 * D), B, H, hd, sc)
        torch.cuda.synchronize()
        tag = st[0]
        del st
        return tag, torch.cuda.max_memory_allocated() - base

    tag, tiled = rise()
    assert tag == 'fused'
    ops.set_fused_attention(False)
    try:
        tag_g, gemm = rise()
    finally:
        ops.set_fused_attention(True)
    print(f'peak rise: tiled {tiled / 2 ** 20:.2f} MiB, gemm {gemm / 2 ** 20:.1f} MiB')
    assert tag_g == 'gemm' and gemm >= B * H * N * N * 4, gemm
    assert tiled < 8e6, tiled
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(dqkv.float()).all())


def _stack_run(blocks, x, dy, mode, fused):
    from multimae_amd.multimae_utils import run_blocks
    for p in blocks.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(True)
    ops.set_fused_attention(fused)
    try:
        with M.engine.precision(mode):
            y = run_blocks(blocks, xi)
            (y * dy).sum().backward()
        M.engine.join_wgrad_streams()
        torch.cuda.synchronize()
    finally:
        ops.set_fused_attention(True)
    grads = {n: p.grad.detach().clone().float() for n, p in blocks.named_parameters()}
    grads['x'] = xi.grad.detach().clone()
    return y.detach().float(), grads


@pytest.mark.parametrize('N,heads', [(1025, 2), (257, 4)])
def test_stack_composite_beyond_256_tokens(N, heads, monkeypatch):
    """A 2-layer encoder, D = 128, B = 2: the stack composite with the tiled kernels against the same blocks in fp32 mode, with the thresholds of
    the bf16-versus-fp32-mode comparison of tests/test_parity_geometry_gpu.py::test_bench_batch_vs_oracle_and_bf16_vs_fp32_mode (lines 293 and
    310-311: outputs 1.5e-2, per-tensor gradients 3.0e-2, all gradients together 1.2e-2).  Those were calibrated at N = 99 and 12 layers, so the
    batched-GEMM path (set_fused_attention(False): what ran at this length before) is held to the same thresholds against the same fp32 run."""
    from multimae_amd.multimae_utils import Block
    torch.manual_seed(N)
    blocks = torch.nn.ModuleList([Block(128, heads, qkv_bias=True) for _ in range(2)]).to(DEV)
    x = torch.randn(2, N, 128, device=DEV)
    dy = torch.randn(2, N, 128, device=DEV)
    calls = []
    real_fwd, real_bwd = ops.stack_fwd, ops.stack_bwd
    monkeypatch.setattr(ops, 'stack_fwd', lambda *a, **k: (calls.append('fwd'), real_fwd(*a, **k))[1])
    monkeypatch.setattr(ops, 'stack_bwd', lambda *a, **k: (calls.append('bwd'), real_bwd(*a, **k))[1])
    y32, g32 = _stack_run(blocks, x, dy, 'fp32', True)
    calls.clear()
    yt, gt = _stack_run(blocks, x, dy, 'bf16', True)
    assert calls == ['fwd', 'bwd'], f'the encoder did not go through the stack composite: {calls}'
    calls.clear()
    yg, gg = _stack_run(blocks, x, dy, 'bf16', False)
    assert calls == [], calls
    cat = lambda g: torch.cat([g[n].reshape(-1) for n in sorted(g)])
    rows = [(n, rel_err(gt[n], g32[n]), rel_err(gg[n], g32[n])) for n in sorted(g32)]
    e_out, e_all = (rel_err(yt, y32), rel_err(yg, y32)), (rel_err(cat(gt), cat(g32)), rel_err(cat(gg), cat(g32)))
    print(f'N {N}: output tiled {e_out[0]:.3e} gemm {e_out[1]:.3e}; all gradients tiled {e_all[0]:.3e} gemm {e_all[1]:.3e}')
    for n, a, b in rows:
        print(f'  {n:28s} tiled {a:.3e}  gemm {b:.3e}')
    for which in (0, 1):
        name = ('tiled', 'gemm')[which]
        assert e_out[which] < 1.5e-2, (name, e_out)
        assert e_all[which] < 1.2e-2, (name, e_all)
        assert max(r[1 + which] for r in rows) < 3.0e-2, (name, sorted(rows, key=lambda r: -r[1 + which])[:4])


def test_multivit_512_finetuning_step_goes_through_the_stack(monkeypatch):
    """MultiViT at 512 x 512 rgb (1024 patches + 1 global token = 1025 tokens, small width) with a ConvNeXtAdapter on top: forward, backward and
    one FusedAdamW step; finite loss and gradients; the encoder went through ops.stack_fwd once."""
    import torch.nn.functional as F
    from multimae_amd import output_adapters as OA
    from multimae_amd.optim import FusedAdamW
    torch.manual_seed(3)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=16, image_size=(512, 512))}
    outs = {'semseg': OA.ConvNeXtAdapter(num_classes=5, embed_dim=256, preds_per_patch=16, main_tasks=('rgb',), patch_size=16, depth=1)}
    model = M.MultiViT(input_adapters=ins, output_adapters=outs, num_global_tokens=1, dim_tokens=128, depth=2, num_heads=2).to(DEV)
    model.build_arena()
    opt = FusedAdamW(model, lr=1e-4)
    calls = []
    real = ops.stack_fwd

    def counted(x, *a, **k):
        calls.append(tuple(x.shape))
        return real(x, *a, **k)

    monkeypatch.setattr(ops, 'stack_fwd', counted)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    x = torch.randn(1, 3, 512, 512, device=DEV)
    target = torch.randint(0, 5, (1, 512, 512), device=DEV)
    with M.engine.precision('bf16'):
        opt.zero_grad()
        logits = model({'rgb': x})['semseg']
        assert logits.shape == (1, 5, 512, 512)
        loss = F.cross_entropy(logits.float(), target)
        loss.backward()
        M.engine.join_wgrad_streams()
        torch.cuda.synchronize()
        assert calls == [(1025, 128)], calls
        assert bool(torch.isfinite(loss))
        for n, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        opt.step()
        torch.cuda.synchronize()
    moved = [n for n, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(n.startswith('encoder.') for n in moved) and any(n.startswith('output_adapters.') for n in moved), moved[:8]
