"""The input side of the model, element by element: gather-first patch rows, class-embedding gradient, patch <-> image layout and the
mask sampler (tokens.hip), the fused patch embedding and its geometry check (embed.hip).

Raw ABI calls; every output lives in a Guarded buffer whose guard zones and ld padding are checked after every launch.  Copies and
integer outputs are compared bit for bit with the restatements of tests/helpers.py, sums against fp64 under the bounds derived there;
no element is excluded.  Shapes are the smallest that reach the branch a case names: non-square images and patches throughout."""
import ctypes

import pytest
import torch

import multimae_oracle as orc
from helpers import (Guarded, assert_within, bf16_bits_ref, mask_sample_ref, patch_embed_ref, patch_rows_ref, semseg_emb_grad_bound,
                     semseg_emb_grad_ref)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16, F16 = 0, 1, 5
ESUPPORT = -3
_INT = {8: torch.int64, 4: torch.int32, 2: torch.int16}
_SENT = {8: 0xffa5ffa5ffa5ffa5 - 2 ** 64, 4: -5898331, 2: -91}


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


def _code(dtype):
    return BF16 if dtype == torch.bfloat16 else F32


def _bits_equal(out, ref, what):
    """bit-for-bit equality of two tensors of one shape and element size (NaN payloads and sentinels included)."""
    it = _INT[out.element_size()]
    o, r = out.contiguous().view(it), ref.to(out.device).contiguous().view(it)
    assert o.shape == r.shape, f'{what}: shapes {tuple(o.shape)} vs {tuple(r.shape)}'
    bad = o != r
    n = int(bad.sum())
    if n:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{what}: {n} of {o.numel()} elements differ in their bits; first at flat {i}: '
                             f'{int(o.reshape(-1)[i]):#x} vs {int(r.reshape(-1)[i]):#x}')


def _untouched(G, what):
    """nothing written: the view of a Guarded still holds the sentinel, as its guard zones do."""
    G.intact(what)
    assert bool((G.view.contiguous().view(_INT[G.esz]) == _SENT[G.esz]).all()), f'{what}: the output was written'


def _last_error():
    msg = _lib().mmae_last_error()
    return msg.decode() if msg else ''


def _src_array(srcs, dev_data):
    """mmae_patch_src array of task dicts (helpers.py) with the device copies of data / emb in dev_data[t]"""
    from multimae_amd._lib import PatchSrc
    arr = (PatchSrc * len(srcs))()
    for i, s in enumerate(srcs):
        d, e = dev_data[i]
        arr[i].data, arr[i].emb = d.data_ptr(), (None if e is None else e.data_ptr())
        arr[i].kind, arr[i].C, arr[i].H, arr[i].W = s['kind'], s['C'], s['H'], s['W']
        arr[i].ph, arr[i].pw, arr[i].k_off, arr[i].n_cls = s['ph'], s['pw'], s['k_off'], s['n_cls']
    return arr


def _to_dev(srcs):
    return [(s['data'].to(DEV), None if s['emb'] is None else s['emb'].to(DEV)) for s in srcs]


def _make_tasks(tasks, B, gen, k_offs=None):
    """tasks: (kind, C, H, W, ph, pw, n_cls) each; images are normal, class ids drawn from [-1, n_cls] (both ends embed as zeros).
    k_off: the segments back to back in task order unless given.  Returns (task dicts, token offsets, end of the last segment)."""
    srcs, offs, k = [], [0], 0
    for i, (kind, C, H, W, ph, pw, n_cls) in enumerate(tasks):
        if kind == 0:
            data, emb = torch.randn(B, C, H, W, generator=gen), None
        else:
            data, emb = torch.randint(-1, n_cls + 1, (B, H, W), generator=gen), torch.randn(n_cls, C, generator=gen)
        K = C * ph * pw
        srcs.append(dict(data=data, emb=emb, kind=kind, C=C, H=H, W=W, ph=ph, pw=pw, k_off=k if k_offs is None else k_offs[i], n_cls=n_cls))
        offs.append(offs[-1] + (H // ph) * (W // pw))
        k += K
    return srcs, offs, max(s['k_off'] + s['C'] * s['ph'] * s['pw'] for s in srcs)


def _sel_with_ends(B, offs, extra, gen):
    """[B, n_sel]: the first and the last token of every task plus `extra` other distinct ones, in a random order per sample"""
    ends = sorted({i for t in range(len(offs) - 1) if offs[t + 1] > offs[t] for i in (offs[t], offs[t + 1] - 1)})
    rows = []
    for _ in range(B):
        rest = [i for i in torch.randperm(offs[-1], generator=gen).tolist() if i not in ends][:extra]
        r = torch.tensor(ends + rest)
        rows.append(r[torch.randperm(len(r), generator=gen)])
    return torch.stack(rows).long()


# ==============================================================================================
# mmae_patch_rows
ROW_TASKS = [(0, 3, 16, 24, 4, 8, 0), (0, 2, 12, 6, 3, 2, 0), (1, 8, 8, 12, 2, 4, 7)]          # K = 96, 12, 64; 12 tokens each
ROW_LAYOUTS = {'Ktot 188': ([72, 168, 0], 188),       # class ids first, a gap of 8 columns, image 0, image 1, a tail of 8
               'Ktot 304': ([200, 100, 0], 304)}      # gaps 64 .. 100 and 112 .. 200, tail 296 .. 304: more than one 256-column trip


def _f32_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize('layout', list(ROW_LAYOUTS))
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_patch_rows_exact(layout, B, dtype):
    """rows[b * n_sel + r] = the flattened (c, i, j) patch of token sel[b][r] in its task's segment, zeros in every other column:
    a copy in f32, round-to-nearest-even in bf16 (inf, NaN, a subnormal, both ties and the carry into inf among the pixels)."""
    lib = _lib()
    k_offs, Ktot = ROW_LAYOUTS[layout]
    gen = torch.Generator().manual_seed(31 + B)
    srcs, offs, kend = _make_tasks(ROW_TASKS, B, gen, k_offs)
    assert kend + 8 == Ktot
    # the first patch of image 0 (token 0, always selected): +-inf, a NaN with a payload, the smallest subnormal, ties to even both ways, 0x7f7f8000
    srcs[0]['data'][0, 0, 0, :8] = _f32_bits([0x7f800000, 0xff800000, 0x7fa00001, 0x00000001, 0x3f808000, 0x3f818000, 0x7f7f8000, 0x80000001])
    sel = _sel_with_ends(B, offs, 5, gen)
    n_sel = sel.shape[1]
    dev = _to_dev(srcs)
    arr = _src_array(srcs, dev)
    seld = sel.to(DEV)
    out = Guarded(B * n_sel, Ktot, Ktot, dtype, DEV)
    _check(lib.mmae_patch_rows(ctypes.cast(arr, ctypes.c_void_p), _i32(offs), 3, seld.data_ptr(), out.view.data_ptr(), _code(dtype), B, n_sel, Ktot,
                               _st()), 'patch_rows')
    torch.cuda.synchronize()
    what = f'patch_rows {layout} B {B} {dtype}'
    out.intact(what)
    ref = patch_rows_ref(srcs, offs, sel, Ktot)
    assert int(torch.isnan(ref).sum()) == 1 and int(torch.isinf(ref).sum()) == 2
    _bits_equal(out.view, ref if dtype == torch.float32 else bf16_bits_ref(ref), what)
    seg = torch.zeros(Ktot, dtype=torch.bool)
    for s in srcs:
        seg[s['k_off']:s['k_off'] + s['C'] * s['ph'] * s['pw']] = True
    assert int((~seg).sum()) >= 16 and bool((out.view[:, (~seg).to(DEV)].view(_INT[out.esz]) == 0).all()), f'{what}: gap / tail columns'


@pytest.mark.parametrize('code', [F16, 7])
def test_patch_rows_refuses_unknown_dtype_codes(code):
    """any rows_dtype but MMAE_F32 / MMAE_BF16 is refused with MMAE_ESUPPORT and nothing is written (the buffer is sized for 4-byte
    elements: whatever a build does with the code stays inside it)."""
    lib = _lib()
    gen = torch.Generator().manual_seed(32)
    k_offs, Ktot = ROW_LAYOUTS['Ktot 188']
    srcs, offs, _ = _make_tasks(ROW_TASKS, 2, gen, k_offs)
    sel = _sel_with_ends(2, offs, 2, gen)
    dev = _to_dev(srcs)
    arr = _src_array(srcs, dev)
    seld = sel.to(DEV)
    out = Guarded(2 * sel.shape[1], Ktot, Ktot, torch.float32, DEV)
    rc = lib.mmae_patch_rows(ctypes.cast(arr, ctypes.c_void_p), _i32(offs), 3, seld.data_ptr(), out.view.data_ptr(), code, 2, sel.shape[1], Ktot, _st())
    torch.cuda.synchronize()
    assert rc == ESUPPORT, f'patch_rows returned {rc} for dtype code {code}'
    assert 'patch_rows' in _last_error()
    _untouched(out, f'patch_rows dtype code {code}')


# ==============================================================================================
# mmae_patch_embed_fwd / mmae_patch_embed_supported
def _embed_operands(srcs, offs, D, G, gen):
    ws, bs, poss = [], [], []
    for t, s in enumerate(srcs):
        K = s['C'] * s['ph'] * s['pw']
        ws.append((torch.randn(D, K, generator=gen) * K ** -0.5).bfloat16())
        bs.append(torch.randn(D, generator=gen))
        poss.append(torch.randn(max(offs[t + 1] - offs[t], 1), D, generator=gen))
    return ws, bs, poss, (torch.randn(G, D, generator=gen) if G else None)


def _embed_call(lib, arr, wd, bd, pd, offs, T, seld, globd, tok, rows, B, n_sel, G, D, Ktot, tok_ptr=None):
    return lib.mmae_patch_embed_fwd(ctypes.cast(arr, ctypes.c_void_p), _ptrs(wd), _ptrs(bd), _ptrs(pd), _i32(offs), T, seld.data_ptr(),
                                    None if globd is None else globd.data_ptr(), tok.view.data_ptr() if tok_ptr is None else tok_ptr,
                                    None if rows is None else rows.view.data_ptr(), B, n_sel, G, D, Ktot, _st())


def _run_embed(tasks, D, B, G, sel_fn, seed, what):
    """one geometry through mmae_patch_embed_fwd with side rows, again without them, and through patch_rows -> GEMM per task ->
    tokens_assemble: token rows within patch_embed_ref's bound (all three), bit-equal between the two fused runs, global rows and
    side rows bit-exact."""
    from multimae_amd import ops
    lib = _lib()
    gen = torch.Generator().manual_seed(seed)
    srcs, offs, Ktot = _make_tasks(tasks, B, gen)
    T = len(srcs)
    sel = sel_fn(offs, gen)
    assert sel.shape[0] == B
    n_sel = sel.shape[1]
    ws, bs, poss, glob = _embed_operands(srcs, offs, D, G, gen)
    ref, bound, _ = patch_embed_ref(srcs, ws, bs, poss, offs, sel, glob, D)
    rows_bits = bf16_bits_ref(patch_rows_ref(srcs, offs, sel, Ktot))
    dev = _to_dev(srcs)
    arr = _src_array(srcs, dev)
    assert lib.mmae_patch_embed_supported(ctypes.cast(arr, ctypes.c_void_p), T, n_sel, D) == 1, f'{what}: not supported'
    wd, bd, pd = [w.to(DEV).contiguous() for w in ws], [b.to(DEV) for b in bs], [p.to(DEV) for p in poss]
    seld, globd = sel.to(DEV), None if glob is None else glob.to(DEV)
    tok = Guarded(B * (n_sel + G), D, D, torch.float32, DEV)
    rows = Guarded(B * n_sel, Ktot, Ktot, torch.bfloat16, DEV)
    _check(_embed_call(lib, arr, wd, bd, pd, offs, T, seld, globd, tok, rows, B, n_sel, G, D, Ktot), what)
    torch.cuda.synchronize()
    tok.intact(what + ' tok')
    rows.intact(what + ' side rows')
    _bits_equal(rows.view, rows_bits, what + ' side rows')
    t3 = tok.view.view(B, n_sel + G, D)
    assert_within(t3, ref, bound, what, names=('b', 'r', 'd'))
    if G:
        _bits_equal(t3[:, n_sel:], glob.expand(B, G, D), what + ' global tokens')
    tok2 = Guarded(B * (n_sel + G), D, D, torch.float32, DEV)
    _check(_embed_call(lib, arr, wd, bd, pd, offs, T, seld, globd, tok2, None, B, n_sel, G, D, Ktot), what + ' without side rows')
    torch.cuda.synchronize()
    tok2.intact(what + ' tok without side rows')
    _bits_equal(tok2.view, tok.view, what + ': with vs without side rows')
    # the three passes on the same operands
    rows3 = Guarded(B * n_sel, Ktot, Ktot, torch.bfloat16, DEV)
    _check(lib.mmae_patch_rows(ctypes.cast(arr, ctypes.c_void_p), _i32(offs), T, seld.data_ptr(), rows3.view.data_ptr(), BF16, B, n_sel, Ktot, _st()),
           what + ' patch_rows')
    torch.cuda.synchronize()
    rows3.intact(what + ' patch_rows')
    _bits_equal(rows3.view, rows_bits, what + ' patch_rows')
    r3 = rows3.view.contiguous()
    proj = torch.empty((B * n_sel, D), device=DEV, dtype=torch.float32)
    for i, (s, w) in enumerate(zip(srcs, wd)):
        ops.gemm(r3, w, proj, B * n_sel, D, w.shape[1], lda=Ktot, ldb=w.shape[1], ldc=D, a_off=s['k_off'], accumulate=(i > 0))
    tokb = ops.tokens_assemble(proj, bd, pd, offs, seld, globd, B, n_sel, G, D)
    assert_within(tokb, ref, bound, what + ' three passes', names=('b', 'r', 'd'))


def _rand_sel(n_sel):
    def fn(offs, gen, B):
        return torch.stack([torch.randperm(offs[-1], generator=gen)[:n_sel] for _ in range(B)])
    return fn


@pytest.mark.parametrize('n_sel,G', [(10, 2), (1, 0)])
def test_patch_embed_non_square(n_sel, G):
    """4 x 8 patches of a 16 x 32 image (the 8-pixel vector gather) and 4 x 4 patches of a 24 x 12 one (element by element), D = 192"""
    tasks = [(0, 4, 16, 32, 4, 8, 0), (0, 4, 24, 12, 4, 4, 0)]
    _run_embed(tasks, 192, 3, G, lambda offs, gen: _rand_sel(n_sel)(offs, gen, 3), 41, f'patch_embed non-square n_sel {n_sel} G {G}')


@pytest.mark.parametrize('D', [1024, 800])
def test_patch_embed_wide_flavour_partial_chunks(D):
    """D > 768: the <4, 64> flavour with K = 96, 160 (a partial last 128-element chunk: 3 and 1 of 4 staging units) and K = 32 (one unit,
    the vector gather)"""
    tasks = [(0, 6, 8, 12, 4, 4, 0), (0, 10, 8, 12, 4, 4, 0), (0, 1, 8, 16, 4, 8, 0)]
    _run_embed(tasks, D, 2, 0, lambda offs, gen: _sel_with_ends(2, offs, 3, gen), 42, f'patch_embed D {D} partial chunks')


@pytest.mark.parametrize('D', [32, 768])
def test_patch_embed_narrow_and_full_width(D):
    """D = 32: seven of the eight waves own no column block; D = 768: every wave owns three"""
    tasks = [(0, 4, 16, 32, 4, 8, 0), (1, 16, 8, 12, 2, 2, 7)]
    _run_embed(tasks, D, 2, 2, lambda offs, gen: _sel_with_ends(2, offs, 4, gen), 43, f'patch_embed D {D}')


@pytest.mark.parametrize('D', [768, 256])
def test_patch_embed_two_class_id_tasks(D):
    """two class-id tasks share the LDS table: (7 classes, E = 16) in 8 x 8 patches (ph pw = 64, the id cache's limit) and (152, 64) in
    3 x 3 patches (K = 576: the 8-element gather crosses channel boundaries) -- 152 x 64 bf16 is the largest table D <= 768 takes.
    Sample 1 selects nothing from the second task, so its table is never loaded there."""
    tasks = [(1, 16, 16, 24, 8, 8, 7), (1, 64, 6, 9, 3, 3, 152), (0, 4, 8, 8, 4, 4, 0)]

    def sel_fn(offs, gen):
        rows = [torch.randperm(offs[-1], generator=gen)[:9] for _ in range(3)]
        first, third = torch.arange(offs[0], offs[1]), torch.arange(offs[2], offs[3])
        rows[1] = torch.cat([first, third[:3]])[torch.randperm(9, generator=gen)]
        return torch.stack(rows)
    _run_embed(tasks, D, 3, 0, sel_fn, 44, f'patch_embed two class-id tasks D {D}')


def test_patch_embed_group_sizes():
    """per sample and task 0, 1, 32, 33, 64 and 65 kept tokens: no group, one row, exactly one / two 32-row blocks, one row into the
    second block / the second 64-row group"""
    tasks = [(0, 4, 32, 48, 4, 4, 0), (0, 2, 40, 64, 4, 8, 0)]            # 96 and 80 tokens, K = 64 both

    def sel_fn(offs, gen):
        rows = []
        for n0, n1 in ((0, 65), (1, 64), (32, 33)):
            r = torch.cat([torch.randperm(offs[1], generator=gen)[:n0], offs[1] + torch.randperm(offs[2] - offs[1], generator=gen)[:n1]])
            rows.append(r[torch.randperm(65, generator=gen)])
        return torch.stack(rows)
    _run_embed(tasks, 64, 3, 0, sel_fn, 45, 'patch_embed group sizes')


def test_patch_embed_1024_tokens():
    """n_sel = 1024, the limit: every token of a 128 x 128 image in 4 x 4 patches, B = 1"""
    _run_embed([(0, 4, 128, 128, 4, 4, 0)], 64, 1, 2, lambda offs, gen: torch.randperm(1024, generator=gen)[None], 46, 'patch_embed n_sel 1024')


REFUSALS = {
    # name: (tasks, D, n_sel, what changes, supported() can tell)
    'n_sel 1025': ([(0, 4, 132, 128, 4, 4, 0)], 64, 1025, None, True),
    'D 1056': ([(0, 4, 16, 32, 4, 8, 0)], 1056, 4, None, True),
    'D 48': ([(0, 4, 16, 32, 4, 8, 0)], 48, 4, None, True),
    'K 96 at D 768': ([(0, 6, 8, 12, 4, 4, 0)], 768, 4, None, True),
    'K 48 at D 1024': ([(0, 3, 8, 12, 4, 4, 0)], 1024, 4, None, True),
    'k_off 4': ([(0, 4, 16, 32, 4, 8, 0), (0, 4, 24, 12, 4, 4, 0)], 192, 4, 'k_off', True),
    'class ids, ph pw 65': ([(1, 64, 10, 26, 5, 13, 7)], 64, 4, None, True),
    'n_cls 32768': ([(1, 2, 8, 16, 4, 8, 7)], 64, 4, 'n_cls', True),
    '153 x 64 table at D 768': ([(1, 64, 8, 8, 2, 2, 153)], 768, 4, None, True),
    'patch count': ([(0, 4, 16, 32, 4, 8, 0)], 64, 4, 'offs', False),
    'unaligned tok': ([(0, 4, 16, 32, 4, 8, 0)], 64, 4, 'tok', False),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_patch_embed_refusals(name):
    """geometries outside the fused kernel: mmae_patch_embed_supported says 0 and mmae_patch_embed_fwd returns an error before it
    launches; tok and the side rows keep their sentinels.  (A patch count that does not match the task's tokens and an unaligned tok
    are arguments mmae_patch_embed_supported does not receive: there only the call itself refuses.)"""
    lib = _lib()
    tasks, D, n_sel, change, geometric = REFUSALS[name]
    gen = torch.Generator().manual_seed(47)
    B, G = 2, 0
    srcs, offs, Ktot = _make_tasks(tasks, B, gen)
    T = len(srcs)
    if change == 'k_off':
        srcs[1]['k_off'] += 4
        Ktot += 8
    if change == 'n_cls':
        srcs[0]['n_cls'] = 32768                          # (the table itself keeps its 7 rows: nothing is launched that could read it)
    sel = torch.stack([torch.randperm(offs[-1], generator=gen)[:n_sel] for _ in range(B)])
    if change == 'offs':
        offs = [0, offs[1] + 1]
    ws, bs, poss, _ = _embed_operands(srcs, offs, D, G, gen)
    dev = _to_dev(srcs)
    arr = _src_array(srcs, dev)
    sup = lib.mmae_patch_embed_supported(ctypes.cast(arr, ctypes.c_void_p), T, n_sel, D)
    assert sup == (0 if geometric else 1), f'{name}: mmae_patch_embed_supported returned {sup}'
    wd, bd, pd = [w.to(DEV).contiguous() for w in ws], [b.to(DEV) for b in bs], [p.to(DEV) for p in poss]
    seld = sel.to(DEV)
    tok = Guarded(B * (n_sel + G), D, D, torch.float32, DEV, shift=1 if change == 'tok' else 0)
    rows = Guarded(B * n_sel, Ktot, Ktot, torch.bfloat16, DEV)
    assert (tok.view.data_ptr() % 16 != 0) == (change == 'tok')
    rc = _embed_call(lib, arr, wd, bd, pd, offs, T, seld, None, tok, rows, B, n_sel, G, D, Ktot)
    torch.cuda.synchronize()
    assert rc != 0, f'{name}: mmae_patch_embed_fwd accepted it'
    _untouched(tok, name + ' tok')
    _untouched(rows, name + ' side rows')


# ==============================================================================================
# mmae_semseg_emb_bwd_det / mmae_semseg_emb_bwd
EMB_CASES = {
    # name: (B, n_sel, E, ph, pw, nh, nw, n_cls)
    'rows 600: rows_per 3': (2, 300, 64, 2, 2, 100, 64, 20),
    'rows 1300: rows_per 6 > nsub 4': (2, 650, 64, 2, 2, 100, 64, 20),
    'patch 2x3': (2, 300, 16, 2, 3, 25, 16, 9),
    'patch 4x2': (2, 300, 16, 4, 2, 25, 16, 9),
    'patch 2x8: pp 16, pw 8': (2, 300, 8, 2, 8, 25, 16, 9),
    'patch 4x4: unrolled': (2, 300, 8, 4, 4, 25, 16, 9),
    'E 48: nsub 5': (2, 300, 48, 2, 2, 100, 64, 9),
    'E 200: nsub 1': (2, 300, 200, 2, 2, 100, 64, 9),
    'E 256: nsub 1': (2, 300, 256, 2, 2, 100, 64, 9),
    'E 3: nsub 85': (2, 300, 3, 2, 2, 100, 64, 9),
    'n_cls 300: nsub cut to 2': (2, 300, 64, 2, 2, 100, 64, 300),
    'n_cls 301: nsub 1': (2, 300, 64, 2, 2, 100, 64, 301),
}
EMB_ATOMIC = ('rows 600: rows_per 3', 'E 48: nsub 5')


def _emb_case(name, dtype):
    """class ids from [-1, n_cls] with class 2 never drawn, tokens of the class-id task [5, 5 + nh nw) among tokens of other tasks on
    both sides (with repeats: the gradient is a sum over rows), the row gradients at k_off 8 of rows 8 columns wider than they need"""
    B, n_sel, E, ph, pw, nh, nw, n_cls = EMB_CASES[name]
    gen = torch.Generator().manual_seed(51 + len(name))
    H, W = nh * ph, nw * pw
    cls = torch.randint(-1, n_cls + 1, (B, H, W), generator=gen)
    cls[cls == 2] = 3
    tok_off, n_patches = 5, nh * nw
    sel = torch.randint(0, tok_off + n_patches + 5, (B, n_sel), generator=gen)
    k_off = 8
    ld = k_off + E * ph * pw + 8
    d_rows = torch.randn(B * n_sel, ld, generator=gen).to(dtype)
    kw = dict(E=E, ph=ph, pw=pw, k_off=k_off, tok_off=tok_off, n_patches=n_patches, n_cls=n_cls)
    return B, n_sel, H, W, cls, sel, d_rows, ld, kw


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('name', list(EMB_CASES))
def test_semseg_emb_gradient(name, dtype):
    """every table entry against the fp64 sum within gamma(n + 1) S + ulp (n terms, S the sum of their magnitudes): store mode twice
    with equal bits, a class never hit exactly 0; accumulate = prior + stored as one f32 addition, bit for bit; d_emb and the workspace
    (sized exactly to mmae_semseg_emb_bwd_ws_elems) guarded.  Two cases also through the float-atomic form under the same bound."""
    lib = _lib()
    B, n_sel, H, W, cls, sel, d_rows, ld, kw = _emb_case(name, dtype)
    E, n_cls = kw['E'], kw['n_cls']
    grad, n, S = semseg_emb_grad_ref(d_rows, cls, sel, **kw)
    bound = semseg_emb_grad_bound(grad, n, S)
    assert float(n[2]) == 0 and int((n[:, 0] > 0).sum()) >= 2
    clsd, seld, dr = cls.to(DEV), sel.to(DEV), d_rows.to(DEV)
    ws_elems = int(lib.mmae_semseg_emb_bwd_ws_elems(B, n_sel, E, n_cls))
    assert ws_elems > 0 and ws_elems % (n_cls * E) == 0
    what = f'semseg_emb_bwd_det {name} {dtype}'

    def run(d_emb, accumulate):
        ws = Guarded(1, ws_elems, ws_elems, torch.float32, DEV)
        _check(lib.mmae_semseg_emb_bwd_det(dr.data_ptr(), _code(dtype), ld, clsd.data_ptr(), seld.data_ptr(), d_emb.view.data_ptr(), B, H, W, E,
                                           kw['ph'], kw['pw'], n_sel, kw['k_off'], kw['tok_off'], kw['n_patches'], n_cls, ws.view.data_ptr(),
                                           ws_elems, accumulate, _st()), what)
        torch.cuda.synchronize()
        ws.intact(what + ' workspace')
        d_emb.intact(what + ' d_emb')
        assert bool(torch.isfinite(ws.view).all()), f'{what}: a workspace element was not written'
    outs = []
    for _ in range(2):
        d_emb = Guarded(n_cls, E, E, torch.float32, DEV)     # store mode: the sentinel NaNs of the view are overwritten
        run(d_emb, 0)
        outs.append(d_emb.view.clone())
    _bits_equal(outs[1], outs[0], what + ' second run')
    assert_within(outs[0], grad, bound, what, names=('class', 'e'))
    assert bool((outs[0][(n[:, 0] == 0).to(DEV)] == 0).all()), f'{what}: a class without terms is not 0'
    prior = torch.randn(n_cls, E, generator=torch.Generator().manual_seed(52)).to(DEV)
    acc = Guarded(n_cls, E, E, torch.float32, DEV, fill=prior)
    run(acc, 1)
    _bits_equal(acc.view, prior + outs[0], what + ' accumulate')
    _bits_equal(acc.view[2], prior[2], what + ' accumulate, class never hit')
    if name in EMB_ATOMIC:
        at = Guarded(n_cls, E, E, torch.float32, DEV, fill=torch.zeros(n_cls, E))
        _check(lib.mmae_semseg_emb_bwd(dr.data_ptr(), _code(dtype), ld, clsd.data_ptr(), seld.data_ptr(), at.view.data_ptr(), B, H, W, E, kw['ph'],
                                       kw['pw'], n_sel, kw['k_off'], kw['tok_off'], kw['n_patches'], n_cls, _st()), what + ' atomic form')
        torch.cuda.synchronize()
        at.intact(what + ' atomic form')
        assert_within(at.view, grad, bound, what + ' atomic form', names=('class', 'e'))


def test_semseg_emb_gradient_refuses_E_257():
    lib = _lib()
    B, n_sel, E, n_cls, H, W = 2, 8, 257, 5, 8, 12
    assert int(lib.mmae_semseg_emb_bwd_ws_elems(B, n_sel, E, n_cls)) == -1
    gen = torch.Generator().manual_seed(53)
    cls = torch.randint(0, n_cls, (B, H, W), generator=gen).to(DEV)
    sel = torch.randint(0, 24, (B, n_sel), generator=gen).to(DEV)
    dr = torch.randn(B * n_sel, E * 4, generator=gen).to(DEV)
    ws = Guarded(1, 256 * n_cls * E, 256 * n_cls * E, torch.float32, DEV)
    d_emb = Guarded(n_cls, E, E, torch.float32, DEV)
    rc = lib.mmae_semseg_emb_bwd_det(dr.data_ptr(), F32, E * 4, cls.data_ptr(), sel.data_ptr(), d_emb.view.data_ptr(), B, H, W, E, 2, 2, n_sel, 0, 0,
                                     24, n_cls, ws.view.data_ptr(), 256 * n_cls * E, 0, _st())
    torch.cuda.synchronize()
    assert rc == ESUPPORT
    _untouched(d_emb, 'semseg_emb_bwd_det E 257 d_emb')
    _untouched(ws, 'semseg_emb_bwd_det E 257 workspace')


@pytest.mark.parametrize('code', [F16, 7])
def test_semseg_emb_gradient_refuses_unknown_dtype_codes(code):
    """both forms: MMAE_ESUPPORT, d_emb untouched (the rows are a 4-byte buffer, so any kernel a build picks stays inside it)"""
    lib = _lib()
    B, n_sel, H, W, cls, sel, d_rows, ld, kw = _emb_case('patch 2x3', torch.float32)
    E, n_cls = kw['E'], kw['n_cls']
    clsd, seld, dr = cls.to(DEV), sel.to(DEV), d_rows.to(DEV)
    d_emb = Guarded(n_cls, E, E, torch.float32, DEV)
    rc = lib.mmae_semseg_emb_bwd(dr.data_ptr(), code, ld, clsd.data_ptr(), seld.data_ptr(), d_emb.view.data_ptr(), B, H, W, E, kw['ph'], kw['pw'],
                                 n_sel, kw['k_off'], kw['tok_off'], kw['n_patches'], n_cls, _st())
    torch.cuda.synchronize()
    assert rc == ESUPPORT, f'semseg_emb_bwd returned {rc} for dtype code {code}'
    assert 'semseg_emb_bwd' in _last_error()
    _untouched(d_emb, f'semseg_emb_bwd dtype code {code}')
    ws_elems = int(lib.mmae_semseg_emb_bwd_ws_elems(B, n_sel, E, n_cls))
    ws = Guarded(1, ws_elems, ws_elems, torch.float32, DEV)
    rc = lib.mmae_semseg_emb_bwd_det(dr.data_ptr(), code, ld, clsd.data_ptr(), seld.data_ptr(), d_emb.view.data_ptr(), B, H, W, E, kw['ph'], kw['pw'],
                                     n_sel, kw['k_off'], kw['tok_off'], kw['n_patches'], n_cls, ws.view.data_ptr(), ws_elems, 0, _st())
    torch.cuda.synchronize()
    assert rc == ESUPPORT
    _untouched(d_emb, f'semseg_emb_bwd_det dtype code {code} d_emb')
    _untouched(ws, f'semseg_emb_bwd_det dtype code {code} workspace')


def test_ops_semseg_emb_bwd_refuses_fp16_rows():
    from multimae_amd import ops
    d_emb = Guarded(5, 4, 4, torch.float32, DEV)
    with pytest.raises(ValueError, match='bf16 or f32'):
        ops.semseg_emb_bwd(torch.zeros(8, 16, device=DEV, dtype=torch.float16), torch.zeros(2, 4, 4, dtype=torch.long, device=DEV),
                           torch.zeros(2, 4, dtype=torch.long, device=DEV), d_emb.view, B=2, H=4, W=4, E=4, ph=2, pw=2, n_sel=4, k_off=0, tok_off=0,
                           n_patches=4, n_cls=5)
    torch.cuda.synchronize()
    _untouched(d_emb, 'ops.semseg_emb_bwd fp16 rows')


# ==============================================================================================
# mmae_patchify / mmae_unpatchify
PATCH_GEOMS = {
    # name: (B, C, nh, nw, ph, pw)
    'tile pw 4, C 17': (2, 17, 3, 5, 2, 4),
    'tile pw 8, C 17': (2, 17, 3, 2, 3, 8),
    'tile pw 12, C 17': (1, 17, 2, 3, 2, 12),
    'no tile fits: float4': (1, 1, 1, 520, 4, 4),
    'float4 pw 16': (2, 3, 3, 2, 2, 16),
    'float4 pw 20': (2, 3, 2, 3, 3, 20),
    'scalar pw 2': (2, 3, 3, 5, 4, 2),
    'scalar pw 3': (2, 3, 4, 3, 2, 3),
}


def _patch_ref(img, C, nh, nw, ph, pw):
    B = img.shape[0]
    return img.reshape(B, C, nh, ph, nw, pw).permute(0, 2, 4, 1, 3, 5).reshape(B * nh * nw, C * ph * pw)


def _salted(shape, gen):
    x = torch.randn(shape, generator=gen)
    x.reshape(-1)[:6] = _f32_bits([0x7f800000, 0x7fa00001, 0x00000001, 0x3f808000, 0x3f818000, 0x7f7f8000])
    return x


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', list(PATCH_GEOMS))
def test_patchify_exact(name, dtype):
    """'b c (nh ph) (nw pw) -> (b nh nw) (c ph pw)': a copy in f32, round-to-nearest-even in bf16, with ld = KP, a padded ld that keeps
    the vector paths, an ld that is no multiple of 4 (scalar kernel), and the image or the patch pointer one f32 off a 16-byte
    boundary (scalar kernel again); columns KP .. ld and the guard zones keep the sentinel."""
    lib = _lib()
    B, C, nh, nw, ph, pw = PATCH_GEOMS[name]
    KP, H, W = C * ph * pw, nh * ph, nw * pw
    gen = torch.Generator().manual_seed(61)
    img = _salted((B, C, H, W), gen)
    ref = _patch_ref(img, C, nh, nw, ph, pw)
    ref = ref if dtype == torch.float32 else bf16_bits_ref(ref)
    esz = 4 if dtype == torch.float32 else 2
    odd = KP + 1 if (KP + 1) % 4 else KP + 2
    base = torch.empty(img.numel() + 1, device=DEV)
    for ld in (KP, (KP + 7) // 8 * 8 + 8, odd):
        for off_img, off_pat in ((0, 0), (1, 0), (0, 1)):
            imgd = base[off_img:off_img + img.numel()].view(B, C, H, W)
            imgd.copy_(img)
            pat = Guarded(B * nh * nw, KP, ld, dtype, DEV, shift=off_pat * 4 // esz)
            assert imgd.data_ptr() % 16 == 4 * off_img and pat.view.data_ptr() % 16 == 4 * off_pat
            what = f'patchify {name} {dtype} ld {ld} image +{off_img} patches +{off_pat}'
            _check(lib.mmae_patchify(imgd.data_ptr(), pat.view.data_ptr(), _code(dtype), ld, B, C, nh, nw, ph, pw, _st()), what)
            torch.cuda.synchronize()
            pat.intact(what)
            _bits_equal(pat.view, ref, what)


@pytest.mark.parametrize('name', list(PATCH_GEOMS))
def test_unpatchify_exact(name):
    """'(b nh nw) (c ph pw) -> b c (nh ph) (nw pw)', f32 copies: aligned, and with either pointer one f32 off (scalar kernel)"""
    lib = _lib()
    B, C, nh, nw, ph, pw = PATCH_GEOMS[name]
    KP, H, W = C * ph * pw, nh * ph, nw * pw
    gen = torch.Generator().manual_seed(62)
    pat = _salted((B * nh * nw, KP), gen)
    ref = pat.reshape(B, nh, nw, C, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B * C * H, W)
    assert torch.equal(_patch_ref(ref.view(B, C, H, W), C, nh, nw, ph, pw).view(torch.int32), pat.view(torch.int32))
    base = torch.empty(pat.numel() + 1, device=DEV)
    for off_pat, off_img in ((0, 0), (1, 0), (0, 1)):
        patd = base[off_pat:off_pat + pat.numel()].view(B * nh * nw, KP)
        patd.copy_(pat)
        img = Guarded(B * C * H, W, W, torch.float32, DEV, shift=off_img)
        what = f'unpatchify {name} patches +{off_pat} image +{off_img}'
        _check(lib.mmae_unpatchify(patd.data_ptr(), img.view.data_ptr(), B, C, nh, nw, ph, pw, _st()), what)
        torch.cuda.synchronize()
        img.intact(what)
        _bits_equal(img.view, ref, what)


@pytest.mark.parametrize('code', [F16, 7])
def test_patchify_refuses_unknown_dtype_codes(code):
    lib = _lib()
    B, C, nh, nw, ph, pw = PATCH_GEOMS['tile pw 8, C 17']
    KP = C * ph * pw
    img = torch.randn(B, C, nh * ph, nw * pw, generator=torch.Generator().manual_seed(63)).to(DEV)
    pat = Guarded(B * nh * nw, KP, KP + 8, torch.float32, DEV)        # 4-byte elements: whatever a build does with the code stays inside
    rc = lib.mmae_patchify(img.data_ptr(), pat.view.data_ptr(), code, KP + 8, B, C, nh, nw, ph, pw, _st())
    torch.cuda.synchronize()
    assert rc == ESUPPORT, f'patchify returned {rc} for dtype code {code}'
    assert 'patchify' in _last_error()
    _untouched(pat, f'patchify dtype code {code}')


# ==============================================================================================
# mmae_mask_sample
def _mask_inputs(offs, B, gen):
    """noise with forced ties in both arrays; per-sample counts drawn from [0, n_t], row 0 all zeros, row 1 k_t = n_t"""
    T, N = len(offs) - 1, offs[-1]
    tn, an = torch.rand(B, N, generator=gen), torch.rand(B, N, generator=gen)
    for b in range(B):
        i = torch.randperm(N, generator=gen)[:min(N, 6)]
        tn[b, i] = float(tn[b, i[0]])
        j = torch.randperm(N, generator=gen)[:min(N, 6)]
        an[b, j] = float(an[b, j[0]])
    sizes = torch.tensor([offs[t + 1] - offs[t] for t in range(T)])
    spt = (torch.rand(B, T, generator=gen) * (sizes + 1)).long().clamp(max=sizes)
    spt[0] = 0
    if B > 1:
        spt[1] = sizes
    return spt, tn, an


def _mask_call(lib, spt, tn, an, offs, T, B, N, n_keep):
    outs = [Guarded(B, N, N, torch.int64, DEV), Guarded(B, n_keep, max(n_keep, 1), torch.int64, DEV), Guarded(B, N, N, torch.int64, DEV)]
    sd, td, ad = spt.to(DEV), tn.to(DEV), an.to(DEV)
    rc = lib.mmae_mask_sample(sd.data_ptr(), td.data_ptr(), ad.data_ptr(), _i32(offs), T, B, N, n_keep, outs[0].view.data_ptr(),
                              outs[1].flat[outs[1].off:].data_ptr(), outs[2].view.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, outs


MASK_OFFS = {'unequal': [0, 49, 113, 309], 'empty middle task': [0, 16, 16, 40], 'T 1': [0, 37], 'T 8, sizes 1..8': [0, 1, 3, 6, 10, 15, 21, 28, 36]}


@pytest.mark.parametrize('name', list(MASK_OFFS))
def test_mask_sample_exact(name):
    """mask_all, ids_keep, ids_restore bit for bit against the stable-argsort restatement and the oracle, n_keep 0, 1, a third and all
    of the tokens; int64 outputs guarded"""
    lib = _lib()
    offs = MASK_OFFS[name]
    T, N, B = len(offs) - 1, offs[-1], 5
    gen = torch.Generator().manual_seed(71 + T)
    spt, tn, an = _mask_inputs(offs, B, gen)
    for n_keep in (0, 1, N // 3, N):
        rc, outs = _mask_call(lib, spt, tn, an, offs, T, B, N, n_keep)
        what = f'mask_sample {name} n_keep {n_keep}'
        _check(rc, what)
        mine = mask_sample_ref(spt, tn, an, offs, n_keep)
        theirs = orc.masks_from_noise(spt, [tn[:, offs[t]:offs[t + 1]] for t in range(T)], an, n_keep)
        for o, a, b, nm in zip(outs, mine, theirs, ('mask_all', 'ids_keep', 'ids_restore')):
            o.intact(f'{what} {nm}')
            _bits_equal(o.view, a, f'{what} {nm} vs the restatement')
            _bits_equal(o.view, b, f'{what} {nm} vs the oracle')


def test_mask_sample_8192_tokens():
    """Ntot = 8192, the limit (64 KiB of LDS), B = 1"""
    lib = _lib()
    offs = [0, 1000, 5000, 8192]
    gen = torch.Generator().manual_seed(72)
    spt, tn, an = _mask_inputs(offs, 1, gen)
    spt[0] = torch.tensor([700, 0, 3192])
    rc, outs = _mask_call(lib, spt, tn, an, offs, 3, 1, 8192, 2048)
    _check(rc, 'mask_sample Ntot 8192')
    mine = mask_sample_ref(spt, tn, an, offs, 2048)
    theirs = orc.masks_from_noise(spt, [tn[:, offs[t]:offs[t + 1]] for t in range(3)], an, 2048)
    for o, a, b, nm in zip(outs, mine, theirs, ('mask_all', 'ids_keep', 'ids_restore')):
        o.intact(f'mask_sample Ntot 8192 {nm}')
        _bits_equal(o.view, a, f'mask_sample Ntot 8192 {nm} vs the restatement')
        _bits_equal(o.view, b, f'mask_sample Ntot 8192 {nm} vs the oracle')


def test_mask_sample_properties_at_batch_256():
    """B = 256 with unequal tasks: ids_restore a permutation, exactly n_keep visible, ids_keep = the visible tokens -- and the references"""
    lib = _lib()
    offs = MASK_OFFS['unequal']
    N, B, n_keep = 309, 256, 77
    spt, tn, an = _mask_inputs(offs, B, torch.Generator().manual_seed(73))
    rc, outs = _mask_call(lib, spt, tn, an, offs, 3, B, N, n_keep)
    _check(rc, 'mask_sample B 256')
    m, k, r = (o.view for o in outs)
    for o in outs:
        o.intact('mask_sample B 256')
    assert torch.equal(torch.sort(r, 1).values, torch.arange(N, device=DEV).expand(B, -1))
    assert bool((m == 0).sum(1).eq(n_keep).all()) and int(torch.gather(m, 1, k).sum()) == 0
    for o, a in zip(outs, mask_sample_ref(spt, tn, an, offs, n_keep)):
        _bits_equal(o.view, a, 'mask_sample B 256')


@pytest.mark.parametrize('name', ['Ntot 8193', 'T 9', 'offs[T] != Ntot'])
def test_mask_sample_refusals(name):
    lib = _lib()
    offs, T, N = {'Ntot 8193': ([0, 4000, 8193], 2, 8193), 'T 9': (list(range(0, 40, 4)), 9, 36), 'offs[T] != Ntot': ([0, 16, 39], 2, 40)}[name]
    gen = torch.Generator().manual_seed(74)
    spt, tn, an = torch.zeros(2, T, dtype=torch.long), torch.rand(2, N, generator=gen), torch.rand(2, N, generator=gen)
    rc, outs = _mask_call(lib, spt, tn, an, offs, T, 2, N, 8)
    assert rc != 0, f'mask_sample accepted {name}'
    for o in outs:
        _untouched(o, f'mask_sample {name}')
