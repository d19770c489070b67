// The one index map of the heads' resize and of everything that reads or differentiates the low-resolution map without writing the
// image: csrc/convnext.hip (resize_fwd / resize_bwd), csrc/segloss.hip, csrc/regloss.hip.  A loss sees "the pixel mmae_resize_fwd
// would store" because it takes its taps and weights from these functions and from no others.
#pragma once
#include "common.h"
#include <math.h>
#include <type_traits>

// PyTorch's upsample_bilinear2d / upsample_nearest2d index math (align_corners = False, no scale_factor): scale = (float)in / out;
// bilinear: src = max(scale * (dst + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1;
// nearest: i0 = min(floor(dst * scale), in - 1).  The source coordinate's product and sum are ONE FMA, written out so that no
// translation unit depends on the compiler's contraction for it.
struct Src { int i0, i1; float l0, l1; };
__device__ __forceinline__ Src src_bilinear(int dst, float scale, int in) {
    float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    s = s < 0.f ? 0.f : s;
    Src r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}
__device__ __forceinline__ int src_nearest(int dst, float scale, int in) {
    const int i = (int)floorf((float)dst * scale);
    return i < in - 1 ? i : in - 1;
}

// First output index whose source window reaches input index i (bilinear: i0 >= i - 1 or i1 >= i ... both begin at the first
// dst with i1(dst) >= i; nearest: i0(dst) >= i).  The estimate from the inverse map is corrected by walking with the exact forward
// formulas, so the window is the one the forward used.
template <int BILINEAR>
__device__ __forceinline__ int first_dst(int i, float scale, int in, int out) {
    int e = (int)(((float)i - (BILINEAR ? 1.0f : 0.0f)) / scale) - 2;
    e = e < 0 ? 0 : (e > out - 1 ? out - 1 : e);
    if (BILINEAR) {
        while (e > 0 && src_bilinear(e - 1, scale, in).i1 >= i) --e;
        while (e < out && src_bilinear(e, scale, in).i1 < i) ++e;
    } else {
        while (e > 0 && src_nearest(e - 1, scale, in) >= i) --e;
        while (e < out && src_nearest(e, scale, in) < i) ++e;
    }
    return e;
}

// The resize backward as a gather: the sum over the output pixels of one (b, k) plane gb [H][W] that read input pixel (iy, ix) of
// their weight times f(gb[oy][ox]): oy ascending, within a row ox ascending, the row sum then weighted -- a fixed order, no atomics.
// A pixel whose two taps land on the same element (border clamp, i1 == i0) contributes l0 + l1 as the autograd backward does.
template <int BILINEAR, class F>
__device__ __forceinline__ float resize_gather(const float* gb, int iy, int ix, int h, int w, int H, int W, float sy, float sx, F f) {
    const int oy0 = first_dst<BILINEAR>(iy, sy, h, H), ox0 = first_dst<BILINEAR>(ix, sx, w, W);
    float acc = 0.f;
    for (int oy = oy0; oy < H; ++oy) {
        float wy;
        if (BILINEAR) {
            const Src ry = src_bilinear(oy, sy, h);
            if (ry.i0 > iy) break;
            wy = (ry.i0 == iy ? ry.l0 : 0.f) + (ry.i1 == iy ? ry.l1 : 0.f);
        } else {
            if (src_nearest(oy, sy, h) > iy) break;
            wy = 1.f;
        }
        const float* gr = gb + (long long)oy * W;
        float rs = 0.f;
        for (int ox = ox0; ox < W; ++ox) {
            if (BILINEAR) {
                const Src rx = src_bilinear(ox, sx, w);
                if (rx.i0 > ix) break;
                const float wx = (rx.i0 == ix ? rx.l0 : 0.f) + (rx.i1 == ix ? rx.l1 : 0.f);
                rs = __builtin_fmaf(wx, f(gr[ox]), rs);
            } else {
                if (src_nearest(ox, sx, w) > ix) break;
                rs += f(gr[ox]);
            }
        }
        acc = BILINEAR ? __builtin_fmaf(wy, rs, acc) : acc + rs;
    }
    return acc;
}

// ---- host side of the three files: geometry check, scales, grid and the mode dispatch -------------------------------------------
inline bool resize_geom_ok(int B, int h, int w, int K, int H, int W, int64_t ldx, int mode) {
    return B > 0 && h > 0 && w > 0 && K > 0 && H > 0 && W > 0 && ldx >= K && (mode == 0 || mode == 1);
}
// the map's scales as PyTorch forms them
struct ResizeScale {
    float sy, sx;
    ResizeScale(int h, int w, int H, int W) : sy((float)h / (float)H), sx((float)w / (float)W) {}
};
// workgroups for `total` items at `per` items each, between 1 and cap
inline unsigned grid_for(long long total, long long cap = 65536, int per = 256) {
    const long long b = (total + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
// launch(std::integral_constant<int, BILINEAR>) for mode 0 (bilinear) or 1 (nearest)
template <class F>
void by_mode(int mode, F&& launch) {
    if (mode == 0) launch(std::integral_constant<int, 1>{});
    else launch(std::integral_constant<int, 0>{});
}
