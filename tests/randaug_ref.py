"""Numpy restatement of the RandAugment table (include/mmae.h, "RandAugment"): what ``mmae_rand_augment_u8`` must compute, byte for byte.

Every operation restates what PIL does to an RGB image (the recipes were checked against PIL with 0 differing bytes; the golden
``tests/golden/rand_augment.npz`` and, where PIL is importable, ``test_rand_augment_cpu.py`` re-check them):

  affine     ``Image.transform(AFFINE, (a..f), BILINEAR | BICUBIC, fillcolor)`` / ``Image.rotate``: f64 source coordinates of the pixel
             centre, the fill colour outside [0, W) x [0, H), taps clamped to the image, the a = -1 cubic in Horner form (or the
             two-tap lerp), the result truncated after clipping
  blend      ``ImageEnhance.*``: ``Image.blend(degenerate, image, factor)`` in f32
  point ops  ``ImageOps.autocontrast / equalize / posterize / solarize / invert`` and the reference's ``solarize_add``

Images are uint8 arrays (3, H, W); ``apply_table`` takes a batch (B, 3, H, W) and the int32 table.  The op codes and the layout are
written out here a second time on purpose: the oracle shares no code with ``multimae_amd/rand_augment.py``.
"""
import numpy as np

MAX_LAYERS, ROW, LAYER = 4, 68, 16
NOOP, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE = range(12)
BILINEAR, BICUBIC = 2, 3


# ----------------------------------------------------------------------------------------------------------------- point ops --
def _lut(img, lut):
    """lut uint8 (3, 256)"""
    return np.stack([lut[c][img[c]] for c in range(3)])


def autocontrast_lut(h):
    """one channel's histogram -> lut"""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], dtype=np.uint8)


def equalize_lut(h):
    nz = np.nonzero(h)[0]
    ident = np.arange(256, dtype=np.uint8)
    if len(nz) <= 1:
        return ident
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return ident
    n, lut = step // 2, []
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def histograms(img):
    return [np.bincount(img[c].ravel(), minlength=256) for c in range(3)]


def autocontrast(img):
    return _lut(img, [autocontrast_lut(h) for h in histograms(img)])


def equalize(img):
    return _lut(img, [equalize_lut(h) for h in histograms(img)])


def invert(img):
    return (255 - img).astype(np.uint8)


def posterize(img, bits):
    mask = 0 if bits <= 0 else (~(2 ** (8 - bits) - 1)) & 255
    return (img & np.uint8(mask)).astype(np.uint8)


def solarize(img, thresh):
    return np.where(img.astype(np.int32) < thresh, img, 255 - img).astype(np.uint8)


def solarize_add(img, add):
    v = img.astype(np.int32)
    return np.where(v < 128, np.minimum(255, v + add), v).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------- blend --
def blend(deg, img, factor_bits):
    """``Image.blend(deg, img, f)``: f a C float"""
    f = np.array([factor_bits], dtype=np.int32).view(np.float32)[0]
    d, s = deg.astype(np.int32), img.astype(np.int32)
    t = d.astype(np.float32) + f * (s - d).astype(np.float32)          # f32 product, f32 sum
    assert t.dtype == np.float32
    if not (f >= 0 and f <= 1):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)                          # truncation


def grey(img):
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13; the border is copied"""
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)).reshape(3, 3)
    out = img.copy()
    _, H, W = img.shape
    if H < 3 or W < 3:
        return out
    v = img.astype(np.float32)
    ss = np.full((3, H - 2, W - 2), 0.5, dtype=np.float32)
    for dy in (2, 1, 0):                                               # the row below first, as PIL sums
        rows = v[:, dy:dy + H - 2]
        ky = 2 - dy
        ss = ss + ((rows[:, :, 0:W - 2] * k[ky, 0] + rows[:, :, 1:W - 1] * k[ky, 1]) + rows[:, :, 2:W] * k[ky, 2])
    assert ss.dtype == np.float32
    out[:, 1:-1, 1:-1] = np.clip(ss, 0, 255).astype(np.int32).astype(np.uint8)
    return out


def enhance(img, op, factor_bits):
    if op == BRIGHTNESS:
        deg = np.zeros_like(img)
    elif op == COLOR:
        deg = np.broadcast_to(grey(img), img.shape)
    elif op == CONTRAST:
        g = grey(img)
        mean = int(int(g.astype(np.int64).sum()) / g.size + 0.5)
        deg = np.full_like(img, mean)
    else:
        deg = smooth(img)
    return blend(deg, img, factor_bits)


# -------------------------------------------------------------------------------------------------------------------- affine --
def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, coef, interp, fill):
    """coef: six f64; fill: three ints"""
    a, b, c, d, e, f = (np.float64(v) for v in coef)
    _, H, W = img.shape
    xs = np.arange(W, dtype=np.float64)[None, :] + 0.5
    ys = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = a * xs + b * ys + c
    yin = d * xs + e * ys + f
    inside = ~((xin < 0) | (xin >= W) | (yin < 0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = xin - x0, yin - y0
    x0 = np.where(inside, x0, 0).astype(np.int64)
    y0 = np.where(inside, y0, 0).astype(np.int64)
    v = img.astype(np.float64)
    out = np.empty_like(img)

    def tap(ch, yy, xx):
        return v[ch][np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]

    for ch in range(3):
        if interp == BICUBIC:
            rows = [_cubic(tap(ch, y0 + j, x0 - 1), tap(ch, y0 + j, x0), tap(ch, y0 + j, x0 + 1), tap(ch, y0 + j, x0 + 2), dx)
                    for j in (-1, 0, 1, 2)]
            r = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
            r = np.where(r <= 0, 0, np.where(r >= 255, 255, r))
        elif interp == BILINEAR:
            rows = []
            for j in (0, 1):
                p, q = tap(ch, y0 + j, x0), tap(ch, y0 + j, x0 + 1)
                rows.append(p + (q - p) * dx)
            r = rows[0] + (rows[1] - rows[0]) * dy
        else:
            raise ValueError(f'interpolation {interp}')
        out[ch] = np.where(inside, r.astype(np.int64), fill[ch]).astype(np.uint8)
    return out


# --------------------------------------------------------------------------------------------------------------------- table --
def layer_fields(row, l):
    w = row[4 + LAYER * l:4 + LAYER * (l + 1)]
    coef = np.ascontiguousarray(w[4:16]).view(np.float64)
    return int(w[0]), int(w[1]), int(w[2]), int(w[3]), coef


def apply_layer(img, op, interp, iarg, fbits, coef, fill):
    if op == AUTOCONTRAST:
        return autocontrast(img)
    if op == EQUALIZE:
        return equalize(img)
    if op == INVERT:
        return invert(img)
    if op == POSTERIZE:
        return posterize(img, iarg)
    if op == SOLARIZE:
        return solarize(img, iarg)
    if op == SOLARIZE_ADD:
        return solarize_add(img, iarg)
    if op in (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS):
        return enhance(img, op, fbits)
    if op == AFFINE and interp in (BILINEAR, BICUBIC):
        return affine(img, coef, interp, fill)
    return img.copy()                                                   # NOOP and everything out of range


def apply_row(img, row):
    """one sample: the layers in order, each on the previous layer's output; a layer count out of range is clamped"""
    n = min(max(int(row[0]), 0), MAX_LAYERS)
    fill = [int(v) & 255 for v in row[1:4]]
    for l in range(n):
        img = apply_layer(img, *layer_fields(row, l), fill)
    return img


def apply_table(x, table):
    return np.stack([apply_row(x[b], table[b]) for b in range(x.shape[0])])


# ---------------------------------------------------------------------------------------------- building tables by hand --
def rotate_matrix(degrees, W, H):
    """``Image.rotate(degrees)``'s coefficients for ``Image.transform(AFFINE)``; None where it returns a copy"""
    import math
    angle = degrees % 360.0
    if angle == 0:
        return None
    cx, cy = W / 2.0, H / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def f32_bits(f):
    return int(np.array([f], dtype=np.float32).view(np.int32)[0])


def layer(op, interp=0, iarg=0, fbits=0, coef=None):
    """one layer's 16 words"""
    w = np.zeros(LAYER, dtype=np.int32)
    w[0], w[1], w[2], w[3] = op, interp, iarg, fbits
    if coef is not None:
        w[4:16] = np.array([float(v) for v in coef], dtype=np.float64).view(np.int32)
    return w


def make_row(layers, fill=(0, 0, 0), n=None):
    """a table row from up to 4 ``layer()``s; ``n`` overrides the layer count (for rows that are deliberately wrong)"""
    row = np.zeros(ROW, dtype=np.int32)
    row[0] = len(layers) if n is None else n
    row[1:4] = fill
    for l, w in enumerate(layers):
        row[4 + LAYER * l:4 + LAYER * (l + 1)] = w
    return row


_ENHANCERS = {'color': COLOR, 'contrast': CONTRAST, 'brightness': BRIGHTNESS, 'sharpness': SHARPNESS}


def fn_layer(fn, args, interp, H, W):
    """the layer that restates the reference's image function ``fn(img, *args, resample=interp)`` (tests/golden/rand_augment.npz names
    them so) on an H x W image; None where the function returns the image unchanged"""
    if fn in ('auto_contrast', 'equalize', 'invert'):
        return layer({'auto_contrast': AUTOCONTRAST, 'equalize': EQUALIZE, 'invert': INVERT}[fn])
    if fn == 'posterize':
        return None if args[0] >= 8 else layer(POSTERIZE, iarg=max(int(args[0]), 0))
    if fn == 'solarize':
        return layer(SOLARIZE, iarg=int(args[0]))
    if fn == 'solarize_add':
        return layer(SOLARIZE_ADD, iarg=int(args[0]))
    if fn in _ENHANCERS:
        return layer(_ENHANCERS[fn], fbits=f32_bits(args[0]))
    a = args[0]
    coef = {'shear_x': (1, a, 0, 0, 1, 0), 'shear_y': (1, 0, 0, a, 1, 0), 'translate_x_rel': (1, 0, a * W, 0, 1, 0),
            'translate_y_rel': (1, 0, 0, 0, 1, a * H)}.get(fn)
    if fn == 'rotate':
        coef = rotate_matrix(a, W, H)
        if coef is None:
            return None
    return layer(AFFINE, interp=interp, coef=coef)
