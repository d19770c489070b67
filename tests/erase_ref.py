"""Numpy restatement of the random-erasing kernels' contract (include/mmae.h, "Random erasing"), written from the contract and not
from csrc/erase.hip: table -> erased mask (the highest rectangle wins), the erased value per mode, and the noise of 'pixel' mode --
the Philox4x32-10 block in integers, the Box-Muller transform in float64.  tests/test_random_erasing_cpu.py pins the Philox block
with known-answer vectors."""
import numpy as np

MAX_RECTS, ROW = 8, 68
MODES = {'const': 0, 'rand': 1, 'pixel': 2}
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> the 4 output words as uint64 arrays holding 32-bit values"""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def header(seed: int, calls: int, mode) -> np.ndarray:
    row = np.zeros(ROW, dtype=np.int32)
    seed, calls = int(seed) & (2 ** 64 - 1), int(calls) & (2 ** 64 - 1)
    row[:4] = np.array([seed & 0xffffffff, seed >> 32, calls & 0xffffffff, calls >> 32], dtype=np.uint32).view(np.int32)
    row[4] = MODES[mode] if isinstance(mode, str) else mode
    return row


def make_table(B: int, rects, seed: int = 0, calls: int = 0, mode='const') -> np.ndarray:
    """rects: per sample a list of (top, left, h, w[, colours of up to 4 channels]) -> int32 [B + 1, 68]"""
    t = np.zeros((B + 1, ROW), dtype=np.int32)
    t[0] = header(seed, calls, mode)
    assert len(rects) == B
    for b, rs in enumerate(rects):
        assert len(rs) <= MAX_RECTS
        t[1 + b, 0] = len(rs)
        for r, q in enumerate(rs):
            t[1 + b, 4 + 8 * r:8 + 8 * r] = q[:4]
            col = np.zeros(4, dtype=np.float32)
            if len(q) > 4:
                col[:len(q[4])] = q[4]
            t[1 + b, 8 + 8 * r:12 + 8 * r] = col.view(np.int32)
    return t


def hit_map(table: np.ndarray, shape) -> np.ndarray:
    """int [B, H, W]: the highest rectangle that covers each pixel, -1 where none does"""
    B, _, H, W = shape
    hit = np.full((B, H, W), -1, dtype=np.int64)
    for b in range(B):
        n = int(table[1 + b, 0])
        assert 0 <= n <= MAX_RECTS
        for r in range(n):
            top, left, h, w = (int(v) for v in table[1 + b, 4 + 8 * r:8 + 8 * r])
            assert 0 <= top and 0 <= left and 0 <= h and 0 <= w and top + h <= H and left + w <= W, 'a rectangle leaves the image'
            hit[b, top:top + h, left:left + w] = r
    return hit


def noise(table: np.ndarray, shape):
    """'pixel' mode: (z, r) float64 [B, C, H, W] -- the normal of every element and its Box-Muller radius sqrt(-2 ln u1)"""
    hdr = table[0].view(np.uint32)
    n = int(np.prod(shape))
    e = np.arange(n, dtype=np.uint64)
    blk = e >> np.uint64(2)
    o = philox4x32_10((blk & _MASK, blk >> np.uint64(32), int(hdr[2]), int(hdr[3])), (int(hdr[0]), int(hdr[1])))
    second = ((e & np.uint64(3)) >> np.uint64(1)).astype(bool)
    a = np.where(second, o[2], o[0])
    b = np.where(second, o[3], o[1])
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    odd = (e & np.uint64(1)).astype(bool)
    z = r * np.where(odd, np.sin(2.0 * np.pi * u2), np.cos(2.0 * np.pi * u2))
    return z.reshape(shape), r.reshape(shape)


def apply(x: np.ndarray, table: np.ndarray):
    """the erased batch (float32; 'pixel' values rounded from float64) and the bool mask [B, C, H, W] of erased elements"""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    hit = hit_map(table, x.shape)
    mask = np.broadcast_to((hit >= 0)[:, None], x.shape)
    mode = int(table[0, 4])
    out = x.copy()
    if mode == 0:
        out[mask] = 0.0
    elif mode == 1:
        for b in range(B):
            for r in range(int(table[1 + b, 0])):
                col = table[1 + b, 8 + 8 * r:12 + 8 * r].copy().view(np.float32)
                for c in range(C):
                    out[b, c][hit[b] == r] = col[min(c, 3)]
    elif mode == 2:
        z, _ = noise(table, x.shape)
        out[mask] = z[mask].astype(np.float32)
    else:
        raise ValueError(f'mode {mode}')
    return out, mask


def golden_case(gold, case: str):
    """(input, reference output) of one case of tests/golden/random_erasing.npz as float32 arrays: the file stores the input as fp16
    (its values have 11 bits) and the output as the elements that differ from it (tests/golden/make_golden_random_erasing.py)"""
    x = gold[f'{case}/x'].astype(np.float32)
    changed = np.unpackbits(gold[f'{case}/erased'])[:x.size].astype(bool).reshape(x.shape)
    out = x.copy()
    out[changed] = gold[f'{case}/values']
    return x, out
