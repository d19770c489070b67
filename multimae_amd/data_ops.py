"""Batch preparation steps the training loop performs right before the model call.

``truncated_depth_standardize`` replaces run_pretraining_multimae.py:487-492 -- a full ``torch.sort`` of the 50 176 values of
every depth map each step -- with one selection kernel (``mmae_depth_standardize``, csrc/depth.hip).  Drop-in for the loop:

    if standardize_depth and 'depth' in tasks_dict:
        tasks_dict['depth'] = truncated_depth_standardize(tasks_dict['depth'])

``robust_depth_standardize`` / ``mask_invalid_`` are the mask-aware form of the fine-tuning loops (run_finetuning_depth.py:671-695,
run_finetuning_taskonomy.py:645-668): ``mmae_depth_standardize_masked`` and ``mmae_mask_invalid`` of the same file, one launch each,
the cuts taken from the count of valid pixels on the device.  ``dropin/amd_loop.prepare_dense_inputs`` is the loop's call site.
"""
from __future__ import annotations

import torch

from . import _lib, ops


def truncated_depth_standardize(depth: torch.Tensor, lo: float = 0.1, hi: float = 0.9, eps: float = 1e-6) -> torch.Tensor:
    """(B, C, H, W) depth -> standardised with the mean / unbiased variance of each sample's values of rank
    [int(lo*n), int(hi*n)), n = C*H*W."""
    ops._require_gpu(depth, 'depth')
    B = depth.shape[0]
    x = depth.contiguous().float()
    n = x.numel() // B
    y = torch.empty_like(x)
    _lib.check(_lib.load().mmae_depth_standardize(x.data_ptr(), y.data_ptr(), B, n, int(lo * n), int(hi * n), eps, ops._stream()),
               'depth_standardize')
    return y.view(depth.shape)


# --------------------------------------------------------------------------- on-device ingest (csrc/ingest.hip) --
# The to-tensor conversions of utils/datasets.py:93-107 applied after the H2D copy of the compact arrays the decoder produced.
# multimae_amd.staging.BatchStager queues them on its copy stream; each is bit-identical to the host conversion it replaces.

def rgb_table(mean, std) -> torch.Tensor:
    """CPU f32 [3, 256]: the value of every uint8 in every channel, by torchvision's own ops -- ``to_tensor`` (``.float().div(255)``)
    then ``normalize`` (``.sub(mean).div(std)``, mean / std as f32 tensors)."""
    u = torch.arange(256, dtype=torch.uint8).float().div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1)
    return u.view(1, 256).sub(m).div(s).contiguous()


def ingest_rgb_u8(x: torch.Tensor, table: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """(B, H, W, 3) uint8 HWC -> (B, 3, H, W) f32: ``out[b, c, h, w] = table[c, x[b, h, w, c]]`` (``table`` from ``rgb_table``, on the device)."""
    ops._require_gpu(x, 'rgb')
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f'ingest_rgb_u8: expected (B, H, W, 3) uint8, got {tuple(x.shape)} {x.dtype}')
    if table.dtype != torch.float32 or table.shape != (3, 256) or not table.is_contiguous() or table.device != x.device:
        raise ValueError('ingest_rgb_u8: table must be a contiguous f32 (3, 256) tensor on the input\'s device')
    B, H, W, _ = x.shape
    x = x.contiguous()
    out = _out(out, (B, 3, H, W), torch.float32, x.device, 'ingest_rgb_u8')
    _lib.check(_lib.load().mmae_ingest_rgb_u8(x.data_ptr(), table.data_ptr(), out.data_ptr(), B, H, W, ops._stream()), 'ingest_rgb_u8')
    return out


def ingest_depth(x: torch.Tensor, standardize=None, out: torch.Tensor = None) -> torch.Tensor:
    """(B, H, W) or (B, 1, H, W) uint16 / int32 -> (B, 1, H, W) f32 ``float(v) * 2**-16`` (``torch.Tensor(np.array(img) / 2**16)``).
    ``standardize=(lo, hi, eps)`` also applies ``truncated_depth_standardize(.., lo, hi, eps)`` in the same launch, bit-identical to
    converting first."""
    ops._require_gpu(x, 'depth')
    codes = {torch.uint16: _lib.U16, torch.int32: _lib.I32}
    if x.dtype not in codes or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f'ingest_depth: expected (B, H, W) uint16 / int32, got {tuple(x.shape)} {x.dtype}')
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    n = H * W
    x = x.contiguous()
    out = _out(out, (B, 1, H, W), torch.float32, x.device, 'ingest_depth')
    lo, hi, eps = standardize if standardize is not None else (0.0, 0.0, 0.0)
    _lib.check(_lib.load().mmae_ingest_depth(x.data_ptr(), codes[x.dtype], out.data_ptr(), B, n, int(standardize is not None),
                                             int(lo * n), int(hi * n), eps, ops._stream()), 'ingest_depth')
    return out


def ingest_semseg_u8(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """(B, h, w) uint8 -> int64 (``pil_to_tensor(..).to(torch.long)``); every id passes through unchanged."""
    ops._require_gpu(x, 'semseg')
    if x.dtype != torch.uint8 or x.dim() != 3:
        raise ValueError(f'ingest_semseg_u8: expected (B, h, w) uint8, got {tuple(x.shape)} {x.dtype}')
    B = x.shape[0]
    x = x.contiguous()
    out = _out(out, tuple(x.shape), torch.int64, x.device, 'ingest_semseg_u8')
    _lib.check(_lib.load().mmae_ingest_semseg_u8(x.data_ptr(), out.data_ptr(), B, x.numel() // max(B, 1), ops._stream()), 'ingest_semseg_u8')
    return out


# ----------------------------------------------------------------------------------- random erasing (csrc/erase.hip) --
# The table is RandomErasing.draw()'s (multimae_amd/random_erasing.py; layout in include/mmae.h, "Random erasing").

ERASE_ROW_WORDS = _lib.ERASE_ROW


def _erase_table(table, B: int, device, what: str) -> None:
    if not torch.is_tensor(table) or table.dtype != torch.int32 or tuple(table.shape) != (B + 1, ERASE_ROW_WORDS) \
            or not table.is_contiguous() or table.device != device:
        got = f'{tuple(table.shape)} {table.dtype} on {table.device}' if torch.is_tensor(table) else type(table).__name__
        raise ValueError(f'{what}: table must be a contiguous int32 ({B + 1}, {ERASE_ROW_WORDS}) tensor on {device}, got {got}')


def random_erase_(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """Erases the rectangles of ``table`` in the contiguous f32 (B, C, H, W) batch ``x`` in place; only erased pixels are touched."""
    ops._require_gpu(x, 'x')
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f'random_erase_: expected a contiguous non-empty (B, C, H, W) float32 batch, got {tuple(x.shape)} {x.dtype}')
    B, C, H, W = x.shape
    _erase_table(table, B, x.device, 'random_erase_')
    _lib.check(_lib.load().mmae_random_erase(x.data_ptr(), table.data_ptr(), B, C, H, W, ops._stream()), 'random_erase')
    return x


def ingest_rgb_u8_chw(x: torch.Tensor, lut: torch.Tensor, table: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
    """(B, 3, H, W) uint8 CHW (``ToNumpy`` + the default collate) -> (B, 3, H, W) f32: ``out[b, c, h, w] = lut[c, x[b, c, h, w]]``
    (``lut`` from ``rgb_table``, on the device), except where a rectangle of ``table`` erases it -- bit-identical to
    ``random_erase_`` of the lookup.  ``table=None`` decodes only."""
    ops._require_gpu(x, 'rgb')
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError(f'ingest_rgb_u8_chw: expected a non-empty (B, 3, H, W) uint8 batch, got {tuple(x.shape)} {x.dtype}')
    if lut.dtype != torch.float32 or lut.shape != (3, 256) or not lut.is_contiguous() or lut.device != x.device:
        raise ValueError('ingest_rgb_u8_chw: lut must be a contiguous f32 (3, 256) tensor on the input\'s device')
    B, _, H, W = x.shape
    if table is not None:
        _erase_table(table, B, x.device, 'ingest_rgb_u8_chw')
    x = x.contiguous()
    out = _out(out, (B, 3, H, W), torch.float32, x.device, 'ingest_rgb_u8_chw')
    _lib.check(_lib.load().mmae_ingest_rgb_u8_chw_erase(x.data_ptr(), lut.data_ptr(), None if table is None else table.data_ptr(),
                                                        out.data_ptr(), B, H, W, ops._stream()), 'ingest_rgb_u8_chw_erase')
    return out


# -------------------------------------------------------------------------------------- RandAugment (csrc/randaug.hip) --
# The table is RandAugment.draw()'s (multimae_amd/rand_augment.py; layout in include/mmae.h, "RandAugment").

RA_ROW_WORDS, RA_MAX_LAYERS = _lib.RA_ROW, _lib.RA_MAX_LAYERS


def rand_augment_u8(x: torch.Tensor, table: torch.Tensor, out: torch.Tensor = None, layers: int = RA_MAX_LAYERS) -> torch.Tensor:
    """Applies the layers of ``table`` (int32 (B, 68) on the device) to the contiguous uint8 (B, 3, H, W) batch ``x``; returns a new
    tensor (or ``out``, which must not be ``x``: the geometric ops read neighbours).  ``layers``: the layer passes to run, the
    policy's ``n`` -- a sample's layers beyond it are dropped; the default runs every layer a row can hold."""
    ops._require_gpu(x, 'x')
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f'rand_augment_u8: expected a contiguous non-empty (B, 3, H, W) uint8 batch, got {tuple(x.shape)} {x.dtype}')
    B, _, H, W = x.shape
    if not torch.is_tensor(table) or table.dtype != torch.int32 or tuple(table.shape) != (B, RA_ROW_WORDS) \
            or not table.is_contiguous() or table.device != x.device:
        got = f'{tuple(table.shape)} {table.dtype} on {table.device}' if torch.is_tensor(table) else type(table).__name__
        raise ValueError(f'rand_augment_u8: table must be a contiguous int32 ({B}, {RA_ROW_WORDS}) tensor on {x.device}, got {got}')
    if isinstance(layers, bool) or not isinstance(layers, int) or not 1 <= layers <= RA_MAX_LAYERS:
        raise ValueError(f'rand_augment_u8: layers must be an int in [1, {RA_MAX_LAYERS}], got {layers!r}')
    out = _out(out, (B, 3, H, W), torch.uint8, x.device, 'rand_augment_u8')
    if out.data_ptr() == x.data_ptr():
        raise ValueError('rand_augment_u8: out must not be x')
    lib = _lib.load()
    nbytes = lib.mmae_rand_augment_scratch_bytes(B, H, W, layers)
    if nbytes < 0:
        raise ValueError(f'rand_augment_u8: no scratch size for shape {tuple(x.shape)}, layers {layers}')
    scratch = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mmae_rand_augment_u8(x.data_ptr(), table.data_ptr(), out.data_ptr(), scratch.data_ptr(), scratch.numel(), B, H, W,
                                        layers, ops._stream()), 'rand_augment_u8')
    return out


def depth_standardize_(x: torch.Tensor, lo: float = 0.1, hi: float = 0.9, eps: float = 1e-6) -> torch.Tensor:
    """``truncated_depth_standardize`` in place, on a contiguous f32 (B, ...) map (the kernel allows y to alias x)."""
    ops._require_gpu(x, 'depth')
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('depth_standardize_: expected a contiguous f32 tensor')
    B = x.shape[0]
    n = x.numel() // B
    _lib.check(_lib.load().mmae_depth_standardize(x.data_ptr(), x.data_ptr(), B, n, int(lo * n), int(hi * n), eps, ops._stream()),
               'depth_standardize')
    return x


def _dense_f32(x, what, name='input'):
    if not isinstance(x, torch.Tensor) or not ops._device_ok(x) or x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        got = f'{tuple(x.shape)} {x.dtype} on {x.device}' if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f'{what}: {name} must be a contiguous f32 (B, C, H, W) tensor on the GPU, got {got}')
    if x.numel() == 0:
        raise ValueError(f'{what}: {name} is empty, {tuple(x.shape)}')


def _valid_mask(mask, like, what):
    """a contiguous torch.bool (B, 1, H, W) mask on ``like``'s device"""
    shape = (like.shape[0], 1, like.shape[2], like.shape[3])
    if (not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or tuple(mask.shape) != shape or mask.device != like.device
            or not mask.is_contiguous()):
        got = f'{tuple(mask.shape)} {mask.dtype} on {mask.device}' if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f'{what}: mask_valid must be a contiguous torch.bool tensor of shape {shape} on {like.device}, got {got}')
    return mask


def _robust(depth, mask_valid, lo, hi, eps, out, what):
    _dense_f32(depth, what, 'depth')
    if depth.shape[1] != 1:
        raise ValueError(f'{what}: depth must have one channel, got {tuple(depth.shape)}')
    if mask_valid is not None:
        _valid_mask(mask_valid, depth, what)
    B, n = depth.shape[0], depth.shape[2] * depth.shape[3]
    _lib.check(_lib.load().mmae_depth_standardize_masked(depth.data_ptr(), None if mask_valid is None else mask_valid.data_ptr(),
                                                         out.data_ptr(), B, n, lo, hi, eps, ops._stream()), what)
    return out


def robust_depth_standardize(depth: torch.Tensor, mask_valid: torch.Tensor = None, lo: float = 0.1, hi: float = 0.9, eps: float = 1e-6,
                             out: torch.Tensor = None) -> torch.Tensor:
    """run_finetuning_depth.py:672-688 in one launch: ``depth`` f32 (B, 1, H, W), ``mask_valid`` bool of the same shape (None: all
    valid).  Per sample the mean and unbiased variance of the valid, non-NaN values of rank [int(n_valid * lo), int(n_valid * hi))
    -- the count and the cuts stay on the device -- then ``(depth - mean) / sqrt(var + eps)`` where the mask is set and 0 elsewhere;
    fewer than two values in the slice: NaN where the mask is set, as the reference.  Returns a new tensor (or ``out``); ``depth``
    is not written: the loop's ``tasks_dict['depth']``, the loss target, is the same object and stays raw."""
    what = 'robust_depth_standardize'
    _dense_f32(depth, what, 'depth')
    out = _out(out, tuple(depth.shape), torch.float32, depth.device, what)
    return _robust(depth, mask_valid, lo, hi, eps, out, what)


def robust_depth_standardize_(depth: torch.Tensor, mask_valid: torch.Tensor = None, lo: float = 0.1, hi: float = 0.9,
                              eps: float = 1e-6) -> torch.Tensor:
    """``robust_depth_standardize`` in place (the kernel allows y to alias x)."""
    return _robust(depth, mask_valid, lo, hi, eps, depth, 'robust_depth_standardize_')


def mask_invalid_(x: torch.Tensor, mask_valid: torch.Tensor) -> torch.Tensor:
    """run_finetuning_depth.py:694-695 for one task, in place and without the (B, C, H, W) boolean temporary: ``x`` f32 (B, C, H, W),
    ``mask_valid`` bool (B, 1, H, W); ``x[b, c, h, w] = 0`` where ``mask_valid[b, 0, h, w]`` is False, untouched elsewhere."""
    what = 'mask_invalid_'
    _dense_f32(x, what, 'x')
    _valid_mask(mask_valid, x, what)
    B, C, H, W = x.shape
    _lib.check(_lib.load().mmae_mask_invalid(x.data_ptr(), mask_valid.data_ptr(), B, C, H * W, ops._stream()), what)
    return x


def _out(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f'{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, '
                         f'got {tuple(out.shape)} {out.dtype} on {out.device}')
    return out
