"""GPU: the inference forward of the encoder stack (composite.hip: mmae_stack_fwd_infer; ops.stack_fwd_infer; EncoderStackFn's
no-grad route; engine.set_inference_forward).

The contract is bit equality: every value the inference forward stores comes from the same kernel, tile and instruction sequence as in
mmae_stack_fwd, with the backward's side outputs (GELU', LayerNorm statistics, attention lse) compiled out.  So nothing here has a
tolerance: the library call is compared with torch.equal against mmae_stack_fwd on the same operands, the model's no-grad forward
against its forward with gradients and against the no-grad forward with the switch off.  The scratch slab and every kept output are
guarded (helpers.Guarded) at exactly the sizes the library reports."""
import ctypes
import functools

import pytest
import torch

import multimae_amd as M
from multimae_amd import _lib, ops
from multimae_amd._lib import BF16, F32, F32X3, StackDesc
from helpers import Guarded, assert_untouched, byte_slab

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-6
EINVAL, ESUPPORT = -1, -3
WS = 1 << 17
L_STACK = 5                   # both rotating buffers of the scratch are written at least twice
MODES = {'bf16': (torch.bfloat16, BF16, 0), 'f32x3': (torch.float32, F32, F32X3)}
# (B, N, D, heads): 10 rows, far below a GEMM tile, head_dim 32 | head_dim 64, rows no multiple of a tile | the last length of the
# LDS-resident attention kernel | the tiled kernel (bf16 only)
SHAPES = [(2, 5, 64, 2), (2, 197, 128, 2), (1, 256, 64, 2)]
TILED = (1, 260, 64, 2)


def lib():
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr_arr(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def vp(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def last_error():
    m = lib().mmae_last_error()
    return m.decode() if m else ''


def block_shapes(D, Hd):
    return [(D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (Hd, D), (Hd,), (D, Hd), (D,)]


class Stack:
    """L blocks with Hd = 4 D driven through the C descriptors: mmae_stack_fwd into a slab of its own, mmae_stack_fwd_infer into a
    guarded scratch slab and guarded outputs."""

    def __init__(self, mode, geom, L=L_STACK, seed=0):
        self.mode, self.L, self.geom = mode, L, geom
        self.act, self.code, self.f32g = MODES[mode]
        B, N, D, heads = geom
        Hd = 4 * D
        self.Hd, self.R = Hd, B * N
        gen = torch.Generator().manual_seed(seed)
        self.P = [[(torch.randn(s, generator=gen) * (0.08 if len(s) == 2 else 0.1) + (1.0 if i in (0, 6) else 0.0)).to(DEV).contiguous()
                   for i, s in enumerate(block_shapes(D, Hd))] for _ in range(L)]
        self.W = [[p[i].to(self.act).contiguous() for i in (2, 4, 8, 10)] for p in self.P]
        self.x = (torch.randn(self.R, D, generator=gen) * 0.7 + 0.2).to(DEV)
        self.w_arr = ptr_arr([w.data_ptr() for ws in self.W for w in ws])
        self.p_arr = ptr_arr([p[i].data_ptr() for p in self.P for i in (0, 1, 3, 5, 6, 7, 9, 11)])
        self.ws_main = Guarded(1, WS, WS, torch.float32, DEV)
        self.infer_bytes = int(lib().mmae_stack_infer_bytes(ctypes.byref(self.desc())))

    def desc(self, L=None):
        B, N, D, heads = self.geom
        d = StackDesc()
        d.L, d.B, d.N, d.D, d.heads, d.Hd = (self.L if L is None else L), B, N, D, heads, self.Hd
        d.act_dtype, d.f32_gemm, d.eps = self.code, self.f32g, EPS
        d.w, d.p = vp(self.w_arr), vp(self.p_arr)
        d.x = self.x.data_ptr()
        d.ws_main, d.ws_main_elems = self.ws_main.full.data_ptr(), WS
        return d

    def train(self):
        """every layer's output from mmae_stack_fwd (copies)"""
        d = self.desc()
        nbytes = int(lib().mmae_stack_act_bytes(ctypes.byref(d)))
        slab = torch.empty((nbytes,), device=DEV, dtype=torch.uint8)
        d.act, d.act_bytes = slab.data_ptr(), nbytes
        rc = lib().mmae_stack_fwd(ctypes.byref(d), stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, last_error())
        outs = []
        for l in range(self.L):
            off = int(lib().mmae_stack_out_offset(ctypes.byref(d), l))
            outs.append(slab[off:off + self.R * self.geom[2] * 4].view(torch.float32).view(self.R, self.geom[2]).clone())
        return outs

    def infer(self, keep, *, expect=0, short=0, L=None, mutate=None):
        """mmae_stack_fwd_infer with destinations for the layers in `keep` only; returns {layer: Guarded}, the guarded scratch"""
        D = self.geom[2]
        outs = {l: Guarded(self.R, D, D, torch.float32, DEV) for l in keep}
        slab = byte_slab(self.infer_bytes, DEV)
        d = self.desc(L)
        d.act, d.act_bytes = slab.full.data_ptr(), self.infer_bytes - short
        if mutate is not None:
            mutate(d)
        o_arr = ptr_arr([outs[l].full.data_ptr() if l in outs else None for l in range(d.L)])
        rc = lib().mmae_stack_fwd_infer(ctypes.byref(d), vp(o_arr), stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, last_error())
        return outs, slab


@functools.lru_cache(maxsize=None)
def _case(mode, geom):
    """one stack and its training-forward reference per (mode, geometry), shared by the tests below and never modified"""
    s = Stack(mode, geom)
    return s, s.train()


LN_SIDE = (2, 40, 256, 8)     # D = 256, bf16: norm2 is the side output of the proj product (mmae_ln_fuse), here without its statistics
PINGPONG = (11, 197, 128, 2)  # 2 167 rows: at 2 048 rows the planner moves qkv / fc1 / fc2 (K >= 128) to the flavoured ping-pong GEMM, fc1 to its one-stream flavour
CASES = [(m, g) for g in SHAPES for m in MODES] + [('bf16', TILED), ('bf16', LN_SIDE), ('bf16', PINGPONG)]


@pytest.mark.parametrize('mode,geom', CASES, ids=[f'{m}-{"x".join(map(str, g))}' for m, g in CASES])
def test_every_layer_bit_equal_to_the_training_forward(mode, geom):
    s, ref = _case(mode, geom)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    x0 = s.x.clone()
    outs, slab = s.infer(range(s.L))
    for l in range(s.L):
        assert torch.equal(outs[l].view, ref[l]), f'{mode} {geom}: layer {l} differs from mmae_stack_fwd'
        outs[l].intact(f'output of layer {l}')
    slab.intact('scratch slab')
    s.ws_main.intact('ws_main')
    assert torch.equal(s.x, x0)


@pytest.mark.parametrize('mode,geom', [('bf16', SHAPES[1]), ('f32x3', SHAPES[0]), ('bf16', TILED)])
@pytest.mark.parametrize('keep', [(1, 4), (4,)])
def test_kept_subsets(mode, geom, keep):
    """destinations for some layers only: the kept ones are the full run's; the others went through the scratch and nowhere else --
    the guard bytes behind the scratch and the kept outputs, the stack input, the parameters and the workspace's guards are intact"""
    s, ref = _case(mode, geom)
    x0 = s.x.clone()
    p0 = [[t.clone() for t in p] for p in s.P]
    w0 = [[t.clone() for t in w] for w in s.W]
    outs, slab = s.infer(keep)
    assert sorted(outs) == sorted(keep)
    for l in keep:
        assert torch.equal(outs[l].view, ref[l]), f'layer {l}'
        outs[l].intact(f'output of layer {l}')
    slab.intact('scratch slab')
    s.ws_main.intact('ws_main')
    assert torch.equal(s.x, x0)
    assert all(torch.equal(a, b) for pa, pb in zip(s.P, p0) for a, b in zip(pa, pb))
    assert all(torch.equal(a, b) for wa, wb in zip(s.W, w0) for a, b in zip(wa, wb))


@pytest.mark.parametrize('mode', list(MODES))
def test_scratch_does_not_grow_with_depth(mode):
    """slab arithmetic, no GPU work"""
    act, code, f32g = MODES[mode]
    sizes = {}
    for L in (1, 12):
        d = StackDesc()
        d.L, d.B, d.N, d.D, d.heads, d.Hd = L, 4, 197, 768, 12, 3072
        d.act_dtype, d.f32_gemm = code, f32g
        sizes[L] = (int(lib().mmae_stack_infer_bytes(ctypes.byref(d))), int(lib().mmae_stack_act_bytes(ctypes.byref(d))))
    assert sizes[1][0] == sizes[12][0] > 0
    assert sizes[1][0] < sizes[1][1] < sizes[12][1]
    es = 2 if mode == 'bf16' else 4
    R, D, Hd = 4 * 197, 768, 3072
    # one block's ln1, qkv, ao, ln2, hact, x1 and two outputs (Hd <= 5 D: the scratch of a two-stream fc1 aliases ln1 | qkv | ao)
    assert sizes[1][0] == 256 * sum(-(-n // 256) for n in [R * D * es, R * 3 * D * es, R * D * es, R * D * es, R * Hd * es] + [R * D * 4] * 3)


def test_refusals_leave_everything_untouched():
    s, _ = _case('bf16', SHAPES[0])
    some = torch.zeros(8, device=DEV)
    dp_arr = ptr_arr([None] * (2 * s.L - 1) + [some.data_ptr()])

    def set_mx(d):
        d.mx_w = vp(s.w_arr)                              # any non-NULL table: refused before it is read

    def set_dp(d):
        d.dp = vp(dp_arr)

    for what, kw, code in [('mx_w', dict(keep=range(s.L), mutate=set_mx), ESUPPORT),
                           ('dp', dict(keep=range(s.L), mutate=set_dp), ESUPPORT),
                           ('last output missing', dict(keep=(0, 1, 2, 3)), EINVAL),
                           ('slab one byte short', dict(keep=range(s.L), short=1), EINVAL),
                           ('65 blocks', dict(keep=(s.L - 1,), L=65), EINVAL)]:
        if what == '65 blocks':                           # (the destination table must reach index 64)
            outs = {64: Guarded(s.R, s.geom[2], s.geom[2], torch.float32, DEV)}
            slab = byte_slab(s.infer_bytes, DEV)
            d = s.desc(65)
            d.act, d.act_bytes = slab.full.data_ptr(), s.infer_bytes
            o_arr = ptr_arr([None] * 64 + [outs[64].full.data_ptr()])
            rc = lib().mmae_stack_fwd_infer(ctypes.byref(d), vp(o_arr), stream())
            torch.cuda.synchronize()
            assert rc == code, (what, rc, last_error())
        else:
            outs, slab = s.infer(expect=code, **kw)
        assert last_error(), what
        for l, o in outs.items():
            assert_untouched(o, f'{what}: output of layer {l}')
        assert_untouched(slab, f'{what}: scratch slab')
    assert '64 blocks' in last_error()


# ------------------------------------------------------------------------------------------------------------ the model --
def _mini_vit(depth=3, drop_path_rate=0.0):
    """MultiViT at the mini geometry of helpers.MINI (8-pixel patches of 32 x 32 images, width 128, 2 heads): rgb + depth, no head"""
    torch.manual_seed(5)
    ins = {'rgb': M.PatchedInputAdapter(num_channels=3, stride_level=1, patch_size_full=8, image_size=32),
           'depth': M.PatchedInputAdapter(num_channels=1, stride_level=1, patch_size_full=8, image_size=32)}
    return M.MultiViT(input_adapters=ins, output_adapters=None, num_global_tokens=1, dim_tokens=128, depth=depth, num_heads=2,
                      drop_path_rate=drop_path_rate).to(DEV)


def _mini_x(B=3):
    g = torch.Generator().manual_seed(9)
    return {'rgb': torch.randn(B, 3, 32, 32, generator=g).to(DEV), 'depth': torch.randn(B, 1, 32, 32, generator=g).to(DEV)}


def _as_list(y):
    return list(y) if isinstance(y, (list, tuple)) else [y]


@pytest.fixture
def switch():
    prev = M.engine.inference_forward()
    yield M.engine.set_inference_forward
    M.engine.set_inference_forward(prev)


@pytest.mark.parametrize('prec', ['bf16', 'fp32'])
@pytest.mark.parametrize('all_layers', [False, True])
def test_model_no_grad_forward_bit_equal_and_owning(prec, all_layers, switch):
    model, x = _mini_vit().eval(), _mini_x()
    with M.engine.precision(prec):
        y_grad = _as_list(model(x, return_all_layers=all_layers))
        with torch.no_grad():
            y_inf = _as_list(model(x, return_all_layers=all_layers))
            switch(False)
            y_off = _as_list(model(x, return_all_layers=all_layers))
            switch(True)
    torch.cuda.synchronize()
    assert len(y_inf) == len(y_grad) == len(y_off) == (3 if all_layers else 1)
    for l, (a, b, c) in enumerate(zip(y_inf, y_grad, y_off)):
        assert a.shape == b.shape == (3, 33, 128) and not a.requires_grad and b.requires_grad
        assert torch.equal(a, b.detach()), f'layer {l}: no-grad forward differs from the forward with gradients'
        assert torch.equal(a, c), f'layer {l}: no-grad forward differs from the switch-off route'
        assert a.untyped_storage().nbytes() == a.numel() * a.element_size(), f'layer {l} is a view into {a.untyped_storage().nbytes()} bytes'


def _count(monkeypatch):
    calls = []
    real_inf, real_fwd = ops.stack_fwd_infer, ops.stack_fwd
    monkeypatch.setattr(ops, 'stack_fwd_infer', lambda *a, **k: (calls.append('infer'), real_inf(*a, **k))[1])
    monkeypatch.setattr(ops, 'stack_fwd', lambda *a, **k: (calls.append('fwd'), real_fwd(*a, **k))[1])
    return calls


def test_route_taken(monkeypatch, switch):
    model, x = _mini_vit().eval(), _mini_x()
    calls = _count(monkeypatch)
    grads = {}
    with M.engine.precision('bf16'):
        with torch.no_grad():
            model(x)
        assert calls == ['infer'], calls
        for on in (True, False):                          # with gradients the switch changes nothing: stack_fwd, and the same gradients
            switch(on)
            calls.clear()
            model.zero_grad(set_to_none=True)
            y = model(x)
            assert calls == ['fwd'], (on, calls)
            (y * torch.linspace(-1, 1, y.numel(), device=DEV).view_as(y)).sum().backward()
            torch.cuda.synchronize()
            grads[on] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        switch(False)
        calls.clear()
        with torch.no_grad():
            model(x)
        assert calls == ['fwd'], calls
    assert grads[True] and grads[True].keys() == grads[False].keys()
    for n in grads[True]:
        assert torch.equal(grads[True][n], grads[False][n]), n


def test_drop_path_in_training_mode_keeps_the_training_forward(monkeypatch):
    model, x = _mini_vit(drop_path_rate=0.3).train(), _mini_x()
    calls = _count(monkeypatch)
    with M.engine.precision('bf16'), torch.no_grad():
        model(x)
    assert calls == ['fwd'], calls
