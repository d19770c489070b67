"""Token routing (tokens.hip, rowops.hip's rowscale / token-mean) and masked losses (losses.hip), element by element.

Fixed, short fp32 sequences (a copy, a sum of two or three terms in a known order) are compared bit for bit with torch doing the
same operations in the same order on the GPU; every reduction against fp64 under a bound derived from the kernel's rounding points.
Outputs go into Guarded buffers or NaN-filled ones, so a missed or an extra write shows."""
import ctypes
import math

import pytest
import torch

import multimae_oracle as orc
from helpers import Guarded, U32, assert_within, ce_loss_ref, gamma, pixel_loss_ref, ulp, _img_rows

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16, F16 = 0, 1, 5


def _lib():
    from multimae_amd import _lib as L
    return L.load()


def _check(rc, what):
    from multimae_amd import _lib as L
    L.check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _i32(vals):
    return ctypes.cast((ctypes.c_int32 * len(vals))(*vals), ctypes.c_void_p)


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), ctypes.c_void_p)


def _bits_equal(out, ref, what):
    """bit-for-bit equality of two f32 / 16-bit tensors of one shape (NaN sentinels included)."""
    it = {4: torch.int32, 2: torch.int16}[out.element_size()]
    o, r = out.contiguous().view(it), ref.to(out.dtype).contiguous().view(it)
    bad = o != r
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{what}: {n} of {o.numel()} elements differ in their bits; first at flat {i}: '
                             f'{float(out.reshape(-1)[i])!r} vs {float(ref.reshape(-1)[i])!r}')


def _untouched(G, what):
    """nothing written: the view of a Guarded still holds the sentinel, as its guard zones do."""
    G.intact(what)
    assert bool((G.view.contiguous().view({4: torch.int32, 2: torch.int16}[G.esz]) == {4: -5898331, 2: -91}[G.esz]).all()), \
        f'{what}: the output was written'


# ==============================================================================================
# token routing
OFFS = {1: [0, 49], 2: [0, 49, 113], 3: [0, 49, 113, 309]}


def _sel(B, offs, extra, g):
    """[B, n_sel] token ids: the first and the last token of every task plus `extra` other distinct ones, in a random order."""
    Ntot = offs[-1]
    ends = [i for t in range(len(offs) - 1) for i in (offs[t], offs[t + 1] - 1)]
    rows = []
    for _ in range(B):
        rest = [i for i in torch.randperm(Ntot, generator=g).tolist() if i not in ends][:extra]
        r = torch.tensor(ends + rest)
        rows.append(r[torch.randperm(len(r), generator=g)])
    return torch.stack(rows).long()


def _owner(idx, offs):
    return torch.bucketize(idx, torch.tensor(offs[1:], device=idx.device), right=True)


@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('G', [0, 1, 2])
@pytest.mark.parametrize('D', [4, 36, 260, 768, 1024])
def test_tokens_assemble_exact(T, G, D):
    """tok[b][r] = (proj + bias_t) + pos_t[idx - off_t], tok[b][n_sel + g] = global[g]: bit for bit, guard zones intact."""
    lib = _lib()
    offs = OFFS[T]
    g = torch.Generator().manual_seed(1000 * T + 10 * G + D)
    for B in (1, 3, 257):
        sel = _sel(B, offs, 3, g)
        n_sel = sel.shape[1]
        proj = torch.randn(B * n_sel, D, generator=g).to(DEV)
        bias = [torch.randn(D, generator=g).to(DEV) for _ in range(T)]
        pos = [torch.randn(offs[t + 1] - offs[t], D, generator=g).to(DEV) for t in range(T)]
        glob = torch.randn(max(G, 1), D, generator=g).to(DEV)
        seld = sel.to(DEV)
        out = Guarded(B * (n_sel + G), D, D, torch.float32, DEV)
        _check(lib.mmae_tokens_assemble(out.view.data_ptr(), proj.data_ptr(), _ptrs(bias), _ptrs(pos), _i32(offs), T, seld.data_ptr(),
                                        glob.data_ptr() if G else None, B, n_sel, G, D, _st()), 'tokens_assemble')
        torch.cuda.synchronize()
        t = _owner(seld.reshape(-1), offs)
        brow = torch.stack(bias)[t]
        prow = torch.cat(pos)[seld.reshape(-1)]                   # the stacked tables: row idx of task t is pos_t[idx - off_t]
        ref = torch.empty(B, n_sel + G, D, device=DEV)
        ref[:, :n_sel] = ((proj + brow) + prow).view(B, n_sel, D)
        ref[:, n_sel:] = glob[:G]
        _bits_equal(out.view, ref.view(-1, D), f'tokens_assemble T {T} G {G} D {D} B {B}')
        out.intact(f'tokens_assemble T {T} G {G} D {D} B {B}')


def test_tokens_assemble_refusals():
    """D = 1028 (> 1024), D = 6 (not a multiple of 4), T = 0 and T = 9 (> 8 tasks) are refused, and nothing is written."""
    lib = _lib()
    g = torch.Generator().manual_seed(5)
    for D, T in ((1028, 2), (6, 2), (8, 0), (8, 9)):
        offs = [0] + [16 * (t + 1) for t in range(T)] if T else [0, 16]
        Tt = max(T, 1)
        B, n_sel = 2, 4
        sel = torch.randint(0, offs[-1], (B, n_sel), generator=g).to(DEV)
        proj = torch.randn(B * n_sel, D, generator=g).to(DEV)
        bias = [torch.randn(D, generator=g).to(DEV) for _ in range(max(Tt, 1))]
        pos = [torch.randn(16, D, generator=g).to(DEV) for _ in range(max(Tt, 1))]
        out = Guarded(B * n_sel, D, D, torch.float32, DEV)
        rc = lib.mmae_tokens_assemble(out.view.data_ptr(), proj.data_ptr(), _ptrs(bias), _ptrs(pos), _i32(offs), T, sel.data_ptr(), None,
                                      B, n_sel, 0, D, _st())
        torch.cuda.synchronize()
        assert rc != 0, f'tokens_assemble accepted D {D} T {T}'
        _untouched(out, f'tokens_assemble D {D} T {T}')


@pytest.mark.parametrize('B', [1, 3, 300])
@pytest.mark.parametrize('TG', [(1, 0), (2, 1), (3, 2), (6, 2)])
@pytest.mark.parametrize('D', [4, 260, 1024])
@pytest.mark.parametrize('act', [torch.float32, torch.bfloat16])
def test_tokens_assemble_bwd(B, TG, D, act):
    """d_proj: the kept tokens' rows, exact in f32 and round-to-nearest-even in bf16.  Every partial row [nblk][T+G][D] is written
    (blocks that own no row included: B = 1 has 4 blocks for 2 rows); the partials' sum is the fp64 column sum within
    gamma(rows per block) sum|terms| (one fp32 accumulation per block, the partials summed in fp64 here)."""
    lib = _lib()
    T, G = TG
    offs = [0, 49, 113, 309, 330, 351, 372][:T + 1]
    g = torch.Generator().manual_seed(B * 7 + T * 3 + D)
    sel = _sel(B, offs, 0 if B == 1 else 3, g)
    n_sel = sel.shape[1]
    if B == 1 and T == 1:
        assert n_sel == 2
    seld = sel.to(DEV)
    d_tok = torch.randn(B, n_sel + G, D, generator=g).to(DEV)
    nblk = lib.mmae_tokens_assemble_bwd_nblk(B)
    assert nblk == min(4 * B, 1024)
    dproj = Guarded(B * n_sel, D, D, act, DEV)
    part = Guarded(nblk * (T + G), D, D, torch.float32, DEV)
    _check(lib.mmae_tokens_assemble_bwd(d_tok.data_ptr(), dproj.view.data_ptr(), BF16 if act == torch.bfloat16 else F32, _i32(offs), T,
                                        seld.data_ptr(), part.view.data_ptr(), B, n_sel, G, D, _st()), 'tokens_assemble_bwd')
    torch.cuda.synchronize()
    what = f'tokens_assemble_bwd B {B} T {T} G {G} D {D} {act}'
    dproj.intact(what + ' d_proj')
    part.intact(what + ' part')
    _bits_equal(dproj.view, d_tok[:, :n_sel].reshape(-1, D).to(act), what + ' d_proj')
    p = part.view.view(nblk, T + G, D)
    assert bool(torch.isfinite(p).all()), f'{what}: a partial row was not written'
    rows = d_tok.double()
    t = _owner(seld.reshape(-1), offs)
    ref = torch.zeros(T + G, D, dtype=torch.float64, device=DEV)
    ab = torch.zeros_like(ref)
    ref[:T].index_add_(0, t, rows[:, :n_sel].reshape(-1, D))
    ab[:T].index_add_(0, t, rows[:, :n_sel].reshape(-1, D).abs())
    ref[T:] = rows[:, n_sel:].sum(0)
    ab[T:] = rows[:, n_sel:].abs().sum(0)
    per_blk = -(-B * (n_sel + G) // nblk)
    assert_within(p.double().sum(0), ref, gamma(per_blk) * ab + gamma(nblk, 2.0 ** -53) * ab, what + ' column sums', names=('slot', 'col'))


def test_tokens_assemble_bwd_slot_limit():
    """T + G = 8 slots are accepted, 9 refused with nothing written."""
    lib = _lib()
    g = torch.Generator().manual_seed(9)
    B, D = 2, 8
    for T, G, ok in ((3, 5, True), (3, 6, False)):
        offs = [0, 10, 20, 30]
        sel = _sel(B, offs, 2, g)
        n_sel = sel.shape[1]
        seld = sel.to(DEV)
        d_tok = torch.randn(B, n_sel + G, D, generator=g).to(DEV)
        nblk = lib.mmae_tokens_assemble_bwd_nblk(B)
        dproj = Guarded(B * n_sel, D, D, torch.float32, DEV)
        part = Guarded(nblk * (T + G), D, D, torch.float32, DEV)
        rc = lib.mmae_tokens_assemble_bwd(d_tok.data_ptr(), dproj.view.data_ptr(), F32, _i32(offs), T, seld.data_ptr(), part.view.data_ptr(),
                                          B, n_sel, G, D, _st())
        torch.cuda.synchronize()
        if ok:
            _check(rc, 'tokens_assemble_bwd T + G = 8')
            _bits_equal(dproj.view, d_tok[:, :n_sel].reshape(-1, D), 'T + G = 8 d_proj')
            ref = d_tok[:, n_sel:].double().sum(0)
            assert_within(part.view.view(nblk, T + G, D)[:, T:].double().sum(0), ref, gamma(B) * d_tok[:, n_sel:].double().abs().sum(0), 'T + G = 8 globals')
        else:
            assert rc != 0, 'tokens_assemble_bwd accepted T + G = 9'
            _untouched(dproj, 'T + G = 9 d_proj')
            _untouched(part, 'T + G = 9 part')


# ---- decoder query / context build
def _ids(vis_sets, Ntot, g):
    """ids_keep [B, n_keep] and ids_restore [B, Ntot] for given visible sets (each of n_keep distinct ids, kept in a random order)."""
    keep, restore = [], []
    for vis in vis_sets:
        v = torch.tensor(vis)[torch.randperm(len(vis), generator=g)]
        rest = torch.tensor([i for i in range(Ntot) if i not in set(vis)], dtype=torch.long)
        shuf = torch.cat([v, rest[torch.randperm(len(rest), generator=g)]])
        keep.append(shuf[:len(vis)])
        restore.append(torch.argsort(shuf))
    return torch.stack(keep).long(), torch.stack(restore).long()


def _masks(B, offs, n_keep, g, adversarial):
    T, Ntot = len(offs) - 1, offs[-1]
    if not adversarial:
        spt = torch.full((B, T), n_keep // T, dtype=torch.long)
        spt[:, 0] += n_keep - spt.sum(1)
        _, keep, restore = orc.masks_from_noise(spt, [torch.rand(B, offs[t + 1] - offs[t], generator=g) for t in range(T)],
                                                torch.rand(B, Ntot, generator=g), n_keep)
        return keep.long(), restore.long()
    # sample 0: no visible token of task 0 (nor of q_task = 1 when T > 2 leaves enough room); sample 1: every visible token from task 0;
    # sample 2: the first and last token of every task among the visible ones
    sets = [list(range(offs[-1] - n_keep, offs[-1])), list(range(n_keep))]
    ends = [i for t in range(T) for i in (offs[t], offs[t + 1] - 1)][:n_keep]
    sets.append(ends + [i for i in range(Ntot) if i not in ends][:n_keep - len(ends)])
    return _ids(sets[:B], Ntot, g)


def _build_ref(ctx, keep, restore, mask_token, task_emb, pos, offs, q_task, B, n_keep, G, D, n_q):
    NC = n_keep + G
    c3 = ctx.view(B, NC, D)
    z = torch.zeros(D, device=DEV)
    if q_task < 0:
        q = mask_token + (z + pos[:n_q])
        q = q.expand(B, n_q, D)
    else:
        rank = restore[:, offs[q_task]:offs[q_task] + n_q]
        vis = rank < n_keep
        base = torch.where(vis[..., None], torch.gather(c3, 1, rank.clamp(max=n_keep - 1)[..., None].expand(B, n_q, D)), mask_token)
        q = base + (task_emb[q_task] + pos[:n_q])
    t = _owner(keep, offs)
    local = keep - torch.tensor(offs, device=DEV)[t]
    cx = c3.clone()
    cx[:, :n_keep] = c3[:, :n_keep] + (task_emb[t] + pos[local])
    return q.reshape(B * n_q, D), cx.reshape(B * NC, D)


@pytest.mark.parametrize('D', [4, 64, 256, 260, 512, 516, 1024])
@pytest.mark.parametrize('G', [0, 1, 2])
def test_decoder_build_exact(D, G):
    """queries = base + (task_emb + pos[j]) (base: the kept token's context row if it is visible, else the mask token; q_task = -1:
    mask_token + (0 + pos[j])), context = ctx + (task_emb_t + pos[idx - off_t]), global rows copied: bit for bit, every q_task,
    noise masks and adversarial ones (no visible token of the query task, all visible tokens from one task, n_keep = 1)."""
    lib = _lib()
    offs = [0, 49, 113, 309]
    T, Ntot = 3, 309
    g = torch.Generator().manual_seed(D * 3 + G)
    for n_keep, adversarial, B in ((37, False, 4), (41, True, 3), (1, False, 3)):
        keep, restore = _masks(B, offs, n_keep, g, adversarial)
        keep, restore = keep.to(DEV), restore.to(DEV)
        NC = n_keep + G
        ctx = torch.randn(B * NC, D, generator=g).to(DEV)
        task_emb = torch.randn(T, D, generator=g).to(DEV)
        mask_token = torch.randn(D, generator=g).to(DEV)
        pos = torch.randn(196, D, generator=g).to(DEV)
        for q_task in (-1, 0, 1, 2):
            n_q = 29 if q_task < 0 else offs[q_task + 1] - offs[q_task]
            Q = Guarded(B * n_q, D, D, torch.float32, DEV)
            Cx = Guarded(B * NC, D, D, torch.float32, DEV)
            _check(lib.mmae_decoder_build(ctx.data_ptr(), keep.data_ptr(), restore.data_ptr(), mask_token.data_ptr(), task_emb.data_ptr(),
                                          pos.data_ptr(), _i32(offs), T, q_task, B, n_keep, G, D, n_q, Q.view.data_ptr(), Cx.view.data_ptr(),
                                          _st()), 'decoder_build')
            torch.cuda.synchronize()
            what = f'decoder_build D {D} G {G} n_keep {n_keep} q_task {q_task}'
            qr, cr = _build_ref(ctx, keep, restore, mask_token, task_emb, pos, offs, q_task, B, n_keep, G, D, n_q)
            Q.intact(what + ' queries')
            Cx.intact(what + ' context')
            _bits_equal(Q.view, qr, what + ' queries')
            _bits_equal(Cx.view, cr, what + ' context')


def _build_bwd(lib, dq, dc, keep, restore, offs, q_task, B, n_keep, G, D, n_q):
    T = len(offs) - 1
    nblk = lib.mmae_decoder_build_bwd_nblk(B)
    d_ctx = Guarded(B * (n_keep + G), D, D, torch.float32, DEV)
    part = Guarded(nblk * (T + 1), D, D, torch.float32, DEV)
    _check(lib.mmae_decoder_build_bwd(dq.data_ptr(), dc.data_ptr(), keep.data_ptr(), restore.data_ptr(), _i32(offs), T, q_task, B, n_keep, G, D,
                                      n_q, d_ctx.view.data_ptr(), part.view.data_ptr(), _st()), 'decoder_build_bwd')
    torch.cuda.synchronize()
    return d_ctx, part, nblk


@pytest.mark.parametrize('B', [1, 3, 512, 513, 1025])
@pytest.mark.parametrize('D', [4, 64, 260, 1024])
def test_decoder_build_bwd(B, D):
    """d_ctx = d_context (+ d_queries[its query] for a visible token of the query task, in that order): bit for bit, every row written.
    Partials fully written; their sum within gamma(rows a workgroup reads) sum|terms| of the fp64 task-embedding and mask-token sums
    (q_task = -1: row T is the sum of all query rows).  B = 512 / 513 switches the split 4 -> 1, B = 1025 runs the capped grid's b loop."""
    lib = _lib()
    offs = [0, 16, 36]
    T, Ntot, G = 2, 36, 1
    n_keep = 11
    g = torch.Generator().manual_seed(B + D)
    keep, restore = _masks(B, offs, n_keep, g, False)
    if B >= 3:
        k2, r2 = _masks(3, offs, n_keep, g, True)
        keep[:3], restore[:3] = k2, r2
    keep, restore = keep.to(DEV), restore.to(DEV)
    NC = n_keep + G
    nblk_x = min(B, 1024)
    for q_task in (-1, 0, 1):
        n_q = 13 if q_task < 0 else offs[q_task + 1] - offs[q_task]
        dq = torch.randn(B * n_q, D, generator=g).to(DEV)
        dc = torch.randn(B * NC, D, generator=g).to(DEV)
        d_ctx, part, nblk = _build_bwd(lib, dq, dc, keep, restore, offs, q_task, B, n_keep, G, D, n_q)
        what = f'decoder_build_bwd B {B} D {D} q_task {q_task}'
        d_ctx.intact(what + ' d_ctx')
        part.intact(what + ' part')
        t = _owner(keep, offs)
        ref = dc.clone().view(B, NC, D)
        if q_task >= 0:
            hit = t == q_task
            local = (keep - offs[q_task]).clamp(0, n_q - 1)
            qrow = torch.gather(dq.view(B, n_q, D), 1, local[..., None].expand(B, n_keep, D))
            ref[:, :n_keep] = torch.where(hit[..., None], dc.view(B, NC, D)[:, :n_keep] + qrow, dc.view(B, NC, D)[:, :n_keep])
        _bits_equal(d_ctx.view, ref.view(-1, D), what + ' d_ctx')
        p = part.view.view(nblk, T + 1, D)
        assert bool(torch.isfinite(p).all()), f'{what}: a partial row was not written'
        dcd, dqd = dc.double().view(B, NC, D)[:, :n_keep], dq.double().view(B, n_q, D)
        sums = torch.zeros(T + 1, D, dtype=torch.float64, device=DEV)
        ab = torch.zeros_like(sums)
        sums[:T].index_add_(0, t.reshape(-1), dcd.reshape(-1, D))
        ab[:T].index_add_(0, t.reshape(-1), dcd.reshape(-1, D).abs())
        if q_task >= 0:
            sums[q_task] += dqd.sum((0, 1))
            ab[q_task] += dqd.abs().sum((0, 1))
            masked = restore[:, offs[q_task]:offs[q_task] + n_q] >= n_keep
        else:
            masked = torch.ones(B, n_q, dtype=torch.bool, device=DEV)
        sums[T] = (dqd * masked[..., None]).sum((0, 1))
        ab[T] = (dqd.abs() * masked[..., None]).sum((0, 1))
        n = -(-B // nblk_x) * (NC + n_q)
        assert_within(p.double().sum(0), sums, gamma(n) * ab + gamma(nblk, 2.0 ** -53) * ab, what + ' sums', names=('slot', 'col'))


@pytest.mark.parametrize('q_task', [-1, 0, 1])
def test_decoder_build_adjoint(q_task):
    """<build(x), y> == <x, build_bwd(y)> in fp64 for x = (ctx, task_emb, mask_token) with pos = 0 (the build is then linear in x).
    Small integers everywhere, so every fp32 sum is exact and the identity holds exactly, independent of how either side is written."""
    lib = _lib()
    offs = [0, 16, 36]
    T, G, n_keep, D = 2, 2, 9, 260
    g = torch.Generator().manual_seed(77 + q_task)
    B = 5
    keep, restore = _masks(B, offs, n_keep, g, False)
    k2, r2 = _masks(3, offs, n_keep, g, True)
    keep[:3], restore[:3] = k2, r2
    keep, restore = keep.to(DEV), restore.to(DEV)
    n_q = 7 if q_task < 0 else offs[q_task + 1] - offs[q_task]
    NC = n_keep + G
    ri = lambda *s: torch.randint(-8, 9, s, generator=g).float().to(DEV)
    ctx, te, mt = ri(B * NC, D), ri(T, D), ri(D)
    pos = torch.zeros(20, D, device=DEV)
    Q = torch.empty(B * n_q, D, device=DEV)
    Cx = torch.empty(B * NC, D, device=DEV)
    _check(lib.mmae_decoder_build(ctx.data_ptr(), keep.data_ptr(), restore.data_ptr(), mt.data_ptr(), te.data_ptr(), pos.data_ptr(), _i32(offs),
                                  T, q_task, B, n_keep, G, D, n_q, Q.data_ptr(), Cx.data_ptr(), _st()), 'decoder_build')
    yq, yc = ri(B * n_q, D), ri(B * NC, D)
    d_ctx, part, nblk = _build_bwd(lib, yq, yc, keep, restore, offs, q_task, B, n_keep, G, D, n_q)
    s = part.view.view(nblk, T + 1, D).double().sum(0)
    lhs = float((Q.double() * yq.double()).sum() + (Cx.double() * yc.double()).sum())
    rhs = float((ctx.double() * d_ctx.view.double()).sum() + (te.double() * s[:T]).sum() + (mt.double() * s[T]).sum())
    assert lhs == rhs, f'adjoint identity q_task {q_task}: <build(x), y> = {lhs} but <x, build_bwd(y)> = {rhs}'


# ---- positional-embedding gradient, rows -> image, class-embedding image
def test_pos_emb_bwd():
    """d_pos[sel[b][j]] += d_tok[b][j] (global-token rows skipped; positions repeat across the batch): fp64 sum within
    gamma(count) sum|terms| (float atomics: order-dependent, not bit-stable); positions nobody selected stay exactly zero."""
    lib = _lib()
    g = torch.Generator().manual_seed(3)
    for B, n_sel, G, D, n_pos in ((1, 5, 0, 4, 9), (7, 40, 2, 260, 60), (300, 24, 1, 768, 50)):
        sel = torch.randint(0, n_pos - 3, (B, n_sel), generator=g).to(DEV)      # the last 3 positions are never selected
        d_tok = torch.randn(B, n_sel + G, D, generator=g).to(DEV)
        d_tok[:, n_sel:] = float('nan')                                         # global rows: any read of them shows
        d_pos = Guarded(n_pos, D, D, torch.float32, DEV, fill=torch.zeros(n_pos, D))
        _check(lib.mmae_pos_emb_bwd(d_tok.data_ptr(), sel.data_ptr(), d_pos.view.data_ptr(), B, n_sel, G, D, n_pos, _st()), 'pos_emb_bwd')
        torch.cuda.synchronize()
        what = f'pos_emb_bwd B {B} n_sel {n_sel} G {G} D {D}'
        d_pos.intact(what)
        rows = d_tok[:, :n_sel].double().reshape(-1, D)
        ref = torch.zeros(n_pos, D, dtype=torch.float64, device=DEV).index_add_(0, sel.reshape(-1), rows)
        ab = torch.zeros_like(ref).index_add_(0, sel.reshape(-1), rows.abs())
        cnt = torch.bincount(sel.reshape(-1), minlength=n_pos).double()[:, None]
        bound = torch.where(cnt > 0, cnt * U32 / (1 - cnt * U32), torch.zeros_like(cnt)) * ab
        assert_within(d_pos.view, ref, bound, what, names=('pos', 'col'))
        assert bool((d_pos.view[n_pos - 3:] == 0).all()), f'{what}: an unselected position got a gradient'


def test_rows_to_image_exact():
    """d_img[b][c][pi*ph + di][pj*pw + dj] = d_rows[row][k_off + k]: an exact scatter.  Unselected patches stay zero, tokens of other tasks
    (sel outside [tok_off, tok_off + n_patches)) are ignored, k_off > 0 and ldr > K, guard zones intact."""
    lib = _lib()
    g = torch.Generator().manual_seed(4)
    for B, C, H, W, ph, pw, tok_off, k_off in ((2, 3, 16, 24, 4, 4, 10, 5), (3, 1, 14, 10, 2, 2, 0, 0), (1, 3, 12, 18, 3, 6, 35, 17)):
        nh, nw = H // ph, W // pw
        n_patches, K = nh * nw, C * ph * pw
        ldr = k_off + K + 7
        n_sel = n_patches // 2 + 3
        outside = [tok_off + n_patches, tok_off + n_patches + 5] + ([tok_off - 1] if tok_off else [tok_off + n_patches + 1])
        sel = torch.stack([torch.tensor((tok_off + torch.randperm(n_patches, generator=g)[:n_sel - 3]).tolist() + outside)[torch.randperm(n_sel, generator=g)]
                           for _ in range(B)]).long()                 # three tokens of other tasks per sample
        d_rows = torch.randn(B * n_sel, ldr, generator=g).to(DEV)
        d_img = Guarded(B * C * H, W, W, torch.float32, DEV, fill=torch.zeros(B * C * H, W))
        seld = sel.to(DEV)
        _check(lib.mmae_rows_to_image(d_rows.data_ptr(), ldr, k_off, seld.data_ptr(), d_img.view.data_ptr(), B, n_sel, tok_off, n_patches,
                                      C, H, W, ph, pw, _st()), 'rows_to_image')
        torch.cuda.synchronize()
        what = f'rows_to_image C {C} {H}x{W} patch {ph}x{pw} tok_off {tok_off}'
        d_img.intact(what)
        ref = torch.zeros(B, n_patches, K, device=DEV)
        p = seld - tok_off
        inside = (p >= 0) & (p < n_patches)
        assert bool(inside.any()) and not bool(inside.all())
        for b in range(B):
            rb = d_rows.view(B, n_sel, ldr)[b, :, k_off:k_off + K]
            ref[b, p[b][inside[b]]] = rb[inside[b]]
        img = ref.view(B, nh, nw, C, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B * C * H, W)
        _bits_equal(d_img.view, img, what)


@pytest.mark.parametrize('geo', [(2, 56, 56, 4, 4), (3, 24, 36, 3, 4), (1, 20, 30, 5, 6)])
def test_semseg_avg_emb(geo):
    """forward: the mean of the centre taps' class embeddings (classes outside [0, n_cls) embed as zero) within gamma(4) sum|terms|;
    backward: 0.25 d_img into every tap's class within gamma(count) sum|terms| (float atomics); classes >= n_cls (255 from u8 labels)
    and pad_idx get no gradient."""
    lib = _lib()
    B, H, W, ph, pw = geo
    n_cls, E, pad = 133, 24, 7
    g = torch.Generator().manual_seed(H * W)
    x = torch.randint(0, 256, (B, H, W), generator=g)
    x[0, :, :W // 2] = pad
    x = x.to(DEV)
    emb = torch.randn(n_cls, E, generator=g).to(DEV)
    nh, nw = H // ph, W // pw
    out = Guarded(B * E * nh, nw, nw, torch.float32, DEV)
    _check(lib.mmae_semseg_avg_emb_fwd(x.data_ptr(), emb.data_ptr(), out.view.data_ptr(), B, H, W, E, ph, pw, n_cls, _st()), 'semseg_avg_emb_fwd')
    taps = lambda n, p: (torch.arange(n) * p + p // 2 - (0 if p & 1 else 1), torch.arange(n) * p + p // 2)
    r0, r1 = taps(nh, ph)
    c0, c1 = taps(nw, pw)
    tcls = [x[:, rr.to(DEV)][:, :, cc.to(DEV)] for rr in (r0, r1) for cc in (c0, c1)]       # 4 x [B, nh, nw]
    e64 = emb.double()
    ref = torch.zeros(B, E, nh, nw, dtype=torch.float64, device=DEV)
    ab = torch.zeros_like(ref)
    for c in tcls:
        ok = (c >= 0) & (c < n_cls)
        v = 0.25 * e64[c.clamp(0, n_cls - 1)].permute(0, 3, 1, 2) * ok[:, None]
        ref += v
        ab += v.abs()
    torch.cuda.synchronize()
    out.intact('semseg_avg_emb_fwd')
    assert_within(out.view.view(B, E, nh, nw), ref, gamma(4) * ab, f'semseg_avg_emb_fwd {geo}', names=('b', 'e', 'i', 'j'))
    d_img = torch.randn(B, E, nh, nw, generator=g).to(DEV)
    d_emb = Guarded(n_cls, E, E, torch.float32, DEV, fill=torch.zeros(n_cls, E))
    _check(lib.mmae_semseg_avg_emb_bwd(d_img.data_ptr(), x.data_ptr(), d_emb.view.data_ptr(), B, H, W, E, ph, pw, n_cls, pad, _st()),
           'semseg_avg_emb_bwd')
    dref = torch.zeros(n_cls, E, dtype=torch.float64, device=DEV)
    dab = torch.zeros_like(dref)
    cnt = torch.zeros(n_cls, dtype=torch.float64, device=DEV)
    gq = 0.25 * d_img.double().permute(0, 2, 3, 1).reshape(-1, E)
    for c in tcls:
        c = c.reshape(-1)
        ok = (c >= 0) & (c < n_cls) & (c != pad)
        dref.index_add_(0, c[ok], gq[ok])
        dab.index_add_(0, c[ok], gq[ok].abs())
        cnt.index_add_(0, c[ok], torch.ones_like(c[ok], dtype=torch.float64))
    torch.cuda.synchronize()
    d_emb.intact('semseg_avg_emb_bwd')
    b = torch.where(cnt > 0, cnt * U32 / (1 - cnt * U32), torch.zeros_like(cnt))[:, None] * dab
    assert_within(d_emb.view, dref, b, f'semseg_avg_emb_bwd {geo}', names=('cls', 'e'))
    assert bool((d_emb.view[pad] == 0).all()), 'pad_idx got a gradient'


# ---- stochastic-depth row scales and token mean
@pytest.mark.parametrize('aliased', [False, True])
def test_rowscale_add(aliased):
    """out = resid + s[r / N] y: at most one rounding of the product and one of the sum (or one fused), u (|s y| + |out|) per element;
    out may alias resid."""
    lib = _lib()
    g = torch.Generator().manual_seed(11)
    for B, N, D in ((1, 1, 4), (5, 7, 260), (3, 197, 768)):
        R = B * N
        resid = torch.randn(R, D, generator=g).to(DEV)
        y = torch.randn(R, D, generator=g).to(DEV)
        s = torch.tensor([0.0, 1.0, 1.0 / 0.9, 1.3, 2.5][:B]).to(DEV)
        r64 = resid.double()
        ref = r64 + s.double().repeat_interleave(N)[:, None] * y.double()
        prod = (s.double().repeat_interleave(N)[:, None] * y.double()).abs()
        if aliased:
            out = Guarded(R, D, D, torch.float32, DEV, fill=resid)
            rp = out.view.data_ptr()
        else:
            out = Guarded(R, D, D, torch.float32, DEV)
            rp = resid.data_ptr()
        _check(lib.mmae_rowscale_add(rp, y.data_ptr(), s.data_ptr(), out.view.data_ptr(), R, N, D, _st()), 'rowscale_add')
        torch.cuda.synchronize()
        what = f'rowscale_add B {B} N {N} D {D} aliased {aliased}'
        out.intact(what)
        assert_within(out.view, ref, U32 * (prod + ref.abs()) * (1 + 4 * U32), what)
        assert bool((out.view[:N] == resid[:N]).all()), f'{what}: s = 0 must leave resid as it is'


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_rowscale_cast(dtype):
    """out = cast(s[r / N] x): one f32 rounding of the product plus the storage rounding, per element.  A dtype code the kernel has no
    flavour for (2) is refused and nothing is written."""
    lib = _lib()
    code = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}[dtype]
    g = torch.Generator().manual_seed(12)
    for B, N, D in ((1, 1, 4), (5, 7, 260), (3, 197, 768)):
        R = B * N
        x = torch.randn(R, D, generator=g).to(DEV)
        s = torch.tensor([0.0, 1.0, 1.0 / 0.9, 1.3, 2.5][:B]).to(DEV)
        ref = s.double().repeat_interleave(N)[:, None] * x.double()
        out = Guarded(R, D, D, dtype, DEV)
        _check(lib.mmae_rowscale_cast(x.data_ptr(), s.data_ptr(), out.view.data_ptr(), code, R, N, D, _st()), 'rowscale_cast')
        torch.cuda.synchronize()
        what = f'rowscale_cast {dtype} B {B} N {N} D {D}'
        out.intact(what)
        b = U32 * ref.abs()
        b = b + (ulp(dtype, ref.abs() + b) / 2 if dtype != torch.float32 else 0)
        assert_within(out.view, ref, b, what)
    out = Guarded(4, 8, 8, torch.float32, DEV)
    x = torch.randn(4, 8, generator=g).to(DEV)
    s = torch.ones(4, device=DEV)
    rc = lib.mmae_rowscale_cast(x.data_ptr(), s.data_ptr(), out.view.data_ptr(), 2, 4, 1, 8, _st())
    torch.cuda.synchronize()
    assert rc != 0, 'rowscale_cast accepted dtype code 2'
    _untouched(out, 'rowscale_cast dtype code 2')


@pytest.mark.parametrize('N', [1, 7, 196])
def test_token_mean(N):
    """y = (fp32 sum of the N rows) / N within gamma(N) sum|x| / N + one ulp; dx = dy / N within one ulp (the division's rounding),
    every row of dx written."""
    lib = _lib()
    g = torch.Generator().manual_seed(N)
    for B, D in ((1, 4), (3, 768), (2, 1028)):
        x = torch.randn(B, N, D, generator=g).to(DEV)
        y = Guarded(B, D, D, torch.float32, DEV)
        _check(lib.mmae_token_mean_fwd(x.data_ptr(), y.view.data_ptr(), B, N, D, _st()), 'token_mean_fwd')
        dy = torch.randn(B, D, generator=g).to(DEV)
        dx = Guarded(B * N, D, D, torch.float32, DEV)
        _check(lib.mmae_token_mean_bwd(dy.data_ptr(), dx.view.data_ptr(), B, N, D, _st()), 'token_mean_bwd')
        torch.cuda.synchronize()
        what = f'token_mean N {N} B {B} D {D}'
        y.intact(what + ' fwd')
        dx.intact(what + ' bwd')
        ref = x.double().mean(1)
        b = gamma(N) * x.double().abs().sum(1) / N
        assert_within(y.view, ref, b + ulp(torch.float32, ref.abs() + b), what + ' fwd')
        dref = (dy.double() / N)[:, None].expand(B, N, D).reshape(B * N, D)
        assert_within(dx.view, dref, ulp(torch.float32, dref), what + ' bwd')


# ==============================================================================================
# masked losses
LSPLIT = 8


class _Bufs:
    def __init__(self, B):
        self.partial = torch.full((B, LSPLIT), float('nan'), device=DEV)
        self.per_sample = torch.full((B, 2), float('nan'), device=DEV)
        self.loss = torch.full((2,), float('nan'), device=DEV)


def _mask(B, np_, g, all_zero=False):
    m = (torch.rand(B, np_, generator=g) < 0.6).long()
    if all_zero:
        m.zero_()
    elif B > 1:
        m[1] = 0                                       # a sample with nothing masked
        m[0, 0] = 1
    return m.to(DEV)


def _check_fwd(ref, bufs, what, B):
    assert_within(bufs.per_sample[:, 0], ref['sum'][0], ref['sum'][1], what + ' per-sample sum', names=('b',))
    assert torch.equal(bufs.per_sample[:, 1].double(), ref['cnt']), f'{what}: per-sample count'
    assert float(bufs.loss[1]) == ref['nvalid'], f'{what}: number of samples with a masked token'
    assert_within(bufs.loss[:1], torch.tensor([ref['loss'][0]]), torch.tensor([ref['loss'][1]]), what + ' loss')


def _check_grad(out, g, bg, what, names=('b', 'c', 'y', 'x'), amb=None, w=None, store=torch.float32):
    """out against the fp64 gradient g under bg plus the storage rounding of `store`.  L1 (amb, w given): an element whose fp64
    residual is within its bound may hold any of {-w, 0, +w} (w within its own 6u and the storage rounding); every other one is bounded."""
    o = out.double()
    half = (lambda x: ulp(store, x) / 2) if store != torch.float32 else (lambda x: torch.zeros_like(x))
    if amb is not None:
        wa = w.abs()
        okv = (o == 0) | ((o.abs() - wa).abs() <= 6 * U32 * wa + half(wa))
        assert bool(okv[amb].all()), f'{what}: an element whose residual is within its bound is not one of -w, 0, +w'
        g = torch.where(amb, o, g)
        bg = torch.where(amb, torch.zeros_like(bg), bg)
    assert_within(o, g, bg + half(g.abs() + bg), what, names=names)


# (C, H, W, P, B): rgb 224 / 16, depth, P = 2 / 6 / 8 on non-square grids, 7 x 7 patches, B = 300
PIX_GEOS = [(3, 224, 224, 16, 2), (1, 224, 224, 16, 1), (3, 32, 48, 2, 5), (3, 36, 30, 6, 5), (3, 32, 48, 8, 5), (3, 56, 56, 8, 5),
            (1, 16, 16, 4, 300)]


def _pix_inputs(C, H, W, P, B, g, const_patches=True):
    pred = torch.randn(B, C, H, W, generator=g)
    target = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
    if const_patches:                                 # constant target patches: norm_pix var = 0, rs = 1 / sqrt(1e-6)
        target[:, :, :P, :P] = 0.1
        target[:, :, -P:, -P:] = -3.0
    return pred.to(DEV), target.to(DEV)


@pytest.mark.parametrize('geo', PIX_GEOS, ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('kind', [0, 1], ids=['mse', 'l1'])
@pytest.mark.parametrize('norm_pix', [False, True], ids=['raw', 'normpix'])
def test_pixel_loss_image_domain(geo, kind, norm_pix):
    """mmae_masked_pixel_loss_fwd / _bwd: per-sample sum and count, norm-pix stats, loss and every element of d_pred against fp64."""
    C, H, W, P, B = geo
    lib = _lib()
    g = torch.Generator().manual_seed(C * H * W + P + kind)
    pred, target = _pix_inputs(C, H, W, P, B, g)
    np_ = (H // P) * (W // P)
    for all_zero in (False, True):
        mask = _mask(B, np_, g, all_zero)
        bufs = _Bufs(B)
        stats = torch.full((B, np_, 2), float('nan'), device=DEV)
        _check(lib.mmae_masked_pixel_loss_fwd(pred.data_ptr(), target.data_ptr(), mask.data_ptr(), kind, int(norm_pix), B, C, H, W, P,
                                              stats.data_ptr() if norm_pix else None, bufs.partial.data_ptr(), bufs.per_sample.data_ptr(),
                                              bufs.loss.data_ptr(), _st()), 'pixel_loss_fwd')
        up = torch.tensor([0.75], device=DEV)
        d_pred = torch.full((B, C, H, W), float('nan'), device=DEV)
        _check(lib.mmae_masked_pixel_loss_bwd(pred.data_ptr(), target.data_ptr(), mask.data_ptr(), kind, int(norm_pix), B, C, H, W, P,
                                              stats.data_ptr() if norm_pix else None, bufs.per_sample.data_ptr(), bufs.loss.data_ptr(),
                                              up.data_ptr(), d_pred.data_ptr(), _st()), 'pixel_loss_bwd')
        torch.cuda.synchronize()
        what = f'pixel loss kind {kind} norm_pix {norm_pix} {geo} all_zero {all_zero}'
        ref = pixel_loss_ref(kind, norm_pix, pred, target, mask, P, up=0.75)
        _check_fwd(ref, bufs, what, B)
        if all_zero:
            assert float(bufs.loss[0]) == 0.0 and bool((d_pred == 0).all()), f'{what}: loss and gradient must be 0'
            continue
        if norm_pix:
            mk = mask.bool()
            assert_within(stats[..., 0][mk], ref['mean'][0][mk], ref['mean'][1][mk], what + ' mean')
            assert_within(stats[..., 1][mk], ref['rstd'][0][mk], ref['rstd'][1][mk], what + ' rstd')
        _check_grad(d_pred, ref['g'], ref['bg'], what + ' d_pred', amb=ref['amb'] if kind == 1 else None, w=ref['w'])


@pytest.mark.parametrize('geo', PIX_GEOS, ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('kind', [0, 1], ids=['mse', 'l1'])
@pytest.mark.parametrize('norm_pix', [False, True], ids=['raw', 'normpix'])
@pytest.mark.parametrize('act', [torch.float32, torch.bfloat16])
def test_pixel_loss_patch_domain(geo, kind, norm_pix, act):
    """mmae_masked_pixel_loss_pat_fwd / _bwd on patch rows: the same fp64 checks, d_pat in a Guarded buffer with ld_pat > C*P*P (pad
    columns zero, nothing outside written), bf16 rows within one more storage rounding, and amax = the largest |element| written."""
    C, H, W, P, B = geo
    lib = _lib()
    g = torch.Generator().manual_seed(C * H * W + P + kind + 1)
    pred, target = _pix_inputs(C, H, W, P, B, g)
    np_, nval = (H // P) * (W // P), C * P * P
    pat = _img_rows(pred, P).reshape(B * np_, nval).float().contiguous()
    ld = nval + (6 if P == 2 else 8)
    for all_zero in (False, True):
        mask = _mask(B, np_, g, all_zero)
        bufs = _Bufs(B)
        stats = torch.full((B, np_, 2), float('nan'), device=DEV)
        _check(lib.mmae_masked_pixel_loss_pat_fwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), kind, int(norm_pix), B, C, H, W, P,
                                                  stats.data_ptr() if norm_pix else None, bufs.partial.data_ptr(), bufs.per_sample.data_ptr(),
                                                  bufs.loss.data_ptr(), _st()), 'pixel_loss_pat_fwd')
        up = torch.tensor([0.75], device=DEV)
        dp = Guarded(B * np_, ld, ld, act, DEV)
        amax = torch.zeros(1, device=DEV)
        _check(lib.mmae_masked_pixel_loss_pat_bwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), kind, int(norm_pix), B, C, H, W, P,
                                                  stats.data_ptr() if norm_pix else None, bufs.per_sample.data_ptr(), bufs.loss.data_ptr(),
                                                  up.data_ptr(), dp.view.data_ptr(), BF16 if act == torch.bfloat16 else F32, ld, amax.data_ptr(),
                                                  _st()), 'pixel_loss_pat_bwd')
        torch.cuda.synchronize()
        what = f'pixel loss (patch rows) kind {kind} norm_pix {norm_pix} {geo} {act} all_zero {all_zero}'
        dp.intact(what + ' d_pat')
        assert bool((dp.view[:, nval:] == 0).all()), f'{what}: pad columns of d_pat are not zero'
        ref = pixel_loss_ref(kind, norm_pix, pred, target, mask, P, up=0.75)
        _check_fwd(ref, bufs, what, B)
        if all_zero:
            assert float(bufs.loss[0]) == 0.0 and bool((dp.view == 0).all()) and float(amax) == 0.0, f'{what}: loss and gradient must be 0'
            continue
        if norm_pix:
            mk = mask.bool()
            assert_within(stats[..., 0][mk], ref['mean'][0][mk], ref['mean'][1][mk], what + ' mean')
            assert_within(stats[..., 1][mk], ref['rstd'][0][mk], ref['rstd'][1][mk], what + ' rstd')
        rows = lambda t: _img_rows(t, P).reshape(B * np_, nval)
        o = dp.view[:, :nval]
        _check_grad(o, rows(ref['g']), rows(ref['bg']), what + ' d_pat', names=('row', 'col'), amb=rows(ref['amb']) if kind == 1 else None,
                    w=rows(ref['w']), store=act)
        o = o.double()
        m_written = float(o.abs().max())
        if act == torch.float32:
            assert float(amax) == m_written, f'{what}: amax {float(amax)!r} != largest |element| written {m_written!r}'
        else:
            assert abs(float(amax) - m_written) <= float(ulp(act, torch.tensor(float(amax)))), f'{what}: amax {float(amax)!r} vs {m_written!r}'


# (C, H, W, P, B, logit spread): semseg 56 x 56 / P = 4 / C = 133, P = 2 / 8 on a non-square grid, P = 6 (image domain only),
# 7 x 7 patches, B = 300
CE_GEOS = [(133, 56, 56, 4, 2, 60.0), (20, 32, 48, 2, 5, 3.0), (20, 32, 48, 8, 5, 60.0), (7, 36, 30, 6, 5, 3.0), (133, 28, 28, 4, 5, 3.0),
           (5, 8, 8, 4, 300, 3.0)]


def _ce_inputs(C, H, W, P, B, spread, g, ignore=False):
    logits = (torch.rand(B, C, H, W, generator=g) * 2 - 1) * spread if spread > 10 else torch.randn(B, C, H, W, generator=g) * spread
    target = torch.randint(0, C, (B, H, W), generator=g)
    if ignore:
        target[:, ::3, ::2] = -100
        target[:, 1::3, 1::2] = 255
        target[0, :P, :P] = -100                       # a whole masked patch ignored
    return logits.to(DEV), target.to(DEV)


def _pat_rescales(C, P):
    """rescales of one pixel's running sum in ce_pat_fwd_kernel: one per group of eight values of a lane (64 lanes, 512 values a round)
    and two per combination of the 64 / (P*P) class slots of a pixel."""
    return -(-C * P * P // 512) + 2 * int(math.log2(64 // (P * P))) + 1


def _ce_oracle_loss(logits, target, mask, P, eps):
    """the reference's definition with F.cross_entropy's ignore_index = -100 (targets outside [0, C) mapped to it): fp64."""
    C = logits.shape[1]
    t = torch.where((target >= 0) & (target < C), target, torch.full_like(target, -100))
    nll = torch.nn.functional.cross_entropy(logits.double(), t, ignore_index=-100, reduction='none', label_smoothing=eps)
    return float(orc._masked_reduce(nll, mask, P))


@pytest.mark.parametrize('geo', CE_GEOS, ids=lambda g: 'x'.join(map(str, g[:5])))
@pytest.mark.parametrize('eps', [0.0, 0.1, 1.0])
@pytest.mark.parametrize('domain', ['image', 'f32', 'bf16', 'f16'])
def test_masked_ce(geo, eps, domain):
    """mmae_masked_ce_* (image domain) and mmae_masked_ce_pat_* (patch rows in f32 / bf16 / fp16): lse, per-sample sum and count,
    loss and every gradient element against fp64.  fp16 rows: amax holds m = max_b |up / (nvalid c_b)| and the rows hold the gradient
    times S(m) within fp16 rounding; f32 / bf16 rows: amax = the largest |element| written.  P = 6 is refused by the patch-domain CE."""
    C, H, W, P, B, spread = geo
    lib = _lib()
    g = torch.Generator().manual_seed(C + H * W + P + int(eps * 10))
    logits, target = _ce_inputs(C, H, W, P, B, spread, g)
    np_, npix, nval = (H // P) * (W // P), P * P, C * P * P
    mask = _mask(B, np_, g)
    bufs = _Bufs(B)
    up = torch.tensor([1.25], device=DEV)
    what = f'CE {domain} {geo} eps {eps}'
    ref = ce_loss_ref(logits, target, mask, P, eps, up=1.25, n_rescale=None if domain == 'image' else _pat_rescales(C, P))
    if domain == 'image':
        lse = torch.full((B, H, W), float('nan'), device=DEV)
        _check(lib.mmae_masked_ce_fwd(logits.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(),
                                      bufs.partial.data_ptr(), bufs.per_sample.data_ptr(), bufs.loss.data_ptr(), _st()), 'ce_fwd')
        d = torch.full_like(logits, float('nan'))
        _check(lib.mmae_masked_ce_bwd(logits.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(),
                                      bufs.per_sample.data_ptr(), bufs.loss.data_ptr(), up.data_ptr(), d.data_ptr(), _st()), 'ce_bwd')
        torch.cuda.synchronize()
        mi = ref['mi']
        assert_within(lse[mi], ref['lse'][0][mi], ref['lse'][1][mi], what + ' lse')
        _check_fwd(ref, bufs, what, B)
        assert_within(d, ref['g'], ref['bg'], what + ' d_logits')
        return
    pat = _img_rows(logits, P).reshape(B * np_, nval).contiguous()
    dt = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}[domain]
    code = {'f32': F32, 'bf16': BF16, 'f16': F16}[domain]
    lse = torch.full((B * np_, npix), float('nan'), device=DEV)
    rc = lib.mmae_masked_ce_pat_fwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(), bufs.partial.data_ptr(),
                                    bufs.per_sample.data_ptr(), bufs.loss.data_ptr(), _st())
    ld = nval + 8
    dp = Guarded(B * np_, ld, ld, dt, DEV)
    amax = torch.zeros(1, device=DEV)
    if npix > 64 or npix & (npix - 1):
        assert rc == -3, f'{what}: ce_pat_fwd must refuse P = {P} with MMAE_ESUPPORT, got {rc}'
        rc = lib.mmae_masked_ce_pat_bwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(), bufs.per_sample.data_ptr(),
                                        bufs.loss.data_ptr(), up.data_ptr(), dp.view.data_ptr(), code, ld, amax.data_ptr(), _st())
        torch.cuda.synchronize()
        assert rc == -3, f'{what}: ce_pat_bwd must refuse P = {P} with MMAE_ESUPPORT, got {rc}'
        _untouched(dp, what + ' d_pat')
        return
    _check(rc, 'ce_pat_fwd')
    _check(lib.mmae_masked_ce_pat_bwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(), bufs.per_sample.data_ptr(),
                                      bufs.loss.data_ptr(), up.data_ptr(), dp.view.data_ptr(), code, ld, amax.data_ptr(), _st()), 'ce_pat_bwd')
    torch.cuda.synchronize()
    dp.intact(what + ' d_pat')
    assert bool((dp.view[:, nval:] == 0).all()), f'{what}: pad columns of d_pat are not zero'
    mk = mask.bool().reshape(-1)
    lref = ref['lse'][0].reshape(B, H // P, P, W // P, P).permute(0, 1, 3, 2, 4).reshape(B * np_, npix)
    lb = ref['lse'][1].reshape(B, H // P, P, W // P, P).permute(0, 1, 3, 2, 4).reshape(B * np_, npix)
    assert_within(lse[mk], lref[mk], lb[mk], what + ' lse_pat')
    _check_fwd(ref, bufs, what, B)
    gr = _img_rows(ref['g'], P).reshape(B * np_, nval)
    br = _img_rows(ref['bg'], P).reshape(B * np_, nval)
    o = dp.view[:, :nval].double()
    if domain == 'f16':
        m_ref = float((1.25 / (ref['nvalid'] * ref['cnt'][ref['cnt'] > 0])).abs().max())
        m = float(amax)
        assert abs(m - m_ref) <= 3 * U32 * m_ref, f'{what}: amax {m!r} is not m = {m_ref!r}'
        S = 2.0 ** (4 - math.floor(math.log2(m)))
        gr, br = gr * S, br * S
        assert_within(o, gr, br + ulp(torch.float16, gr.abs() + br) / 2, what + ' d_pat (fp16, x S)', names=('row', 'col'))
        return
    extra = ulp(dt, gr.abs() + br) / 2 if dt != torch.float32 else 0
    assert_within(o, gr, br + extra, what + ' d_pat', names=('row', 'col'))
    mw = float(o.abs().max())
    if dt == torch.float32:
        assert float(amax) == mw, f'{what}: amax {float(amax)!r} != largest |element| written {mw!r}'
    else:
        assert abs(float(amax) - mw) <= float(ulp(dt, torch.tensor(float(amax)))), f'{what}: amax {float(amax)!r} vs {mw!r}'


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('domain', ['image', 'f32', 'f16'])
def test_masked_ce_ignored_targets(eps, domain):
    """Targets -100 and 255 (outside [0, C), C = 133) are ignored as F.cross_entropy(ignore_index=-100) ignores them: no loss, no gradient
    (the label-smoothing term included), the pixel still counts.  The loss matches the reference's definition with that mapping."""
    lib = _lib()
    C, H, W, P, B = 133, 28, 28, 4, 3
    g = torch.Generator().manual_seed(31 + int(eps * 10))
    logits, target = _ce_inputs(C, H, W, P, B, 3.0, g, ignore=True)
    np_, npix, nval = (H // P) * (W // P), P * P, C * P * P
    mask = _mask(B, np_, g)
    bufs = _Bufs(B)
    up = torch.tensor([1.0], device=DEV)
    ref = ce_loss_ref(logits, target, mask, P, eps, up=1.0, n_rescale=None if domain == 'image' else _pat_rescales(C, P))
    oracle = _ce_oracle_loss(logits, target, mask, P, eps)
    assert abs(oracle - ref['loss'][0]) <= 1e-12 * abs(oracle), f'the fp64 reference {ref["loss"][0]} disagrees with F.cross_entropy {oracle}'
    what = f'CE ignored targets {domain} eps {eps}'
    ign = ((target < 0) | (target >= C))
    if domain == 'image':
        lse = torch.full((B, H, W), float('nan'), device=DEV)
        _check(lib.mmae_masked_ce_fwd(logits.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(),
                                      bufs.partial.data_ptr(), bufs.per_sample.data_ptr(), bufs.loss.data_ptr(), _st()), 'ce_fwd')
        d = torch.full_like(logits, float('nan'))
        _check(lib.mmae_masked_ce_bwd(logits.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(),
                                      bufs.per_sample.data_ptr(), bufs.loss.data_ptr(), up.data_ptr(), d.data_ptr(), _st()), 'ce_bwd')
        torch.cuda.synchronize()
        _check_fwd(ref, bufs, what, B)
        assert bool((d.permute(0, 2, 3, 1)[ign] == 0).all()), f'{what}: an ignored pixel got a gradient'
        assert_within(d, ref['g'], ref['bg'], what + ' d_logits')
        return
    pat = _img_rows(logits, P).reshape(B * np_, nval).contiguous()
    dt, code = (torch.float32, F32) if domain == 'f32' else (torch.float16, F16)
    lse = torch.full((B * np_, npix), float('nan'), device=DEV)
    _check(lib.mmae_masked_ce_pat_fwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(), bufs.partial.data_ptr(),
                                      bufs.per_sample.data_ptr(), bufs.loss.data_ptr(), _st()), 'ce_pat_fwd')
    ld = nval + 8
    dp = Guarded(B * np_, ld, ld, dt, DEV)
    amax = torch.zeros(1, device=DEV)
    _check(lib.mmae_masked_ce_pat_bwd(pat.data_ptr(), target.data_ptr(), mask.data_ptr(), B, C, H, W, P, eps, lse.data_ptr(), bufs.per_sample.data_ptr(),
                                      bufs.loss.data_ptr(), up.data_ptr(), dp.view.data_ptr(), code, ld, amax.data_ptr(), _st()), 'ce_pat_bwd')
    torch.cuda.synchronize()
    dp.intact(what + ' d_pat')
    _check_fwd(ref, bufs, what, B)
    gr = _img_rows(ref['g'], P).reshape(B * np_, nval)
    br = _img_rows(ref['bg'], P).reshape(B * np_, nval)
    ig = _img_rows(ign[:, None].expand(B, C, H, W).contiguous(), P).reshape(B * np_, nval)
    o = dp.view[:, :nval].double()
    assert bool((o[ig] == 0).all()), f'{what}: an ignored pixel got a gradient'
    if dt == torch.float16:
        S = 2.0 ** (4 - math.floor(math.log2(float(amax))))
        gr, br = gr * S, br * S + ulp(torch.float16, gr.abs() * S + br * S) / 2
    assert_within(o, gr, br, what + ' d_pat', names=('row', 'col'))
