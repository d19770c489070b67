// Dense 3x3 convolutions (padding 1, stride 1 or 2) and the align-corners x2 bilinear upsample of the DPT head's RefineNet fusion
// blocks (ResidualConvUnit_custom, FeatureFusionBlock_custom, make_scratch: output_adapter_utils.py:60-257).
//
// The feature map is the ConvNeXt head's: channels-last f32 [B][h][w][C], every pixel a row of C.  A convolution is a gather and a
// product of the engine's GEMM (mmae_gemm), so the MFMA work stays on the tuned kernels; this file holds the gathers:
//   - im2col: the 3x3 window of every output pixel as a row of 9 C columns in (ky, kx, c) order, zeros at padded taps, an optional
//     ReLU applied to the values read (the source map is left as it is), stored as bf16 or f32;
//   - col2im: the data gradient.  The GEMM dY x W gives one row of 9 C columns per output pixel; every INPUT pixel then sums its (at
//     most nine) contributions in (ky, kx) order -- a gather in a fixed order, no atomics -- and applies the ReLU mask of the forward
//     and an optional addend (the gradient of the residual branch) in the same pass;
//   - the weight in both layouts: (Cout, Cin, 3, 3) f32 as nn.Conv2d stores it -> [Cout][9 Cin] in (ky, kx, c) order in the GEMM's
//     operand type, and the way back for the weight gradient;
//   - F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) (output_adapter_utils.py:241-243) on the NHWC map, and its
//     backward as a gather in a fixed order.
// All of them are bandwidth-bound copies: 16-byte loads and stores wherever C and the pointers allow (eight channels per thread in
// the bf16 form, four in the f32 forms), consecutive threads on consecutive addresses of the side that is written.
#include "common.h"

namespace {

inline unsigned grid_for(long long total) {
    const long long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}
inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    return (f32x4){v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f, v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f};
}

// ------------------------------------------------------------------------------------------------------------ im2col --
// col[(b ho + oy) wo + ox][(ky 3 + kx) C + c] = act(x[b][oy s + ky - 1][ox s + kx - 1][c]), 0 outside the map.  One thread: V
// consecutive channels of one tap of one row; i enumerates (row, tap, channel group) with the channel group fastest, so a wave
// writes one contiguous span of col and reads contiguous spans of x.
//   T = uint16_t, V = 8: two 16-byte loads, one 16-byte store of eight bf16 (C % 8 == 0)
//   T = float,    V = 4: one 16-byte load, one 16-byte store (C % 4 == 0)
//   T = float,    V = 1: any C
//   I: the type the work-item index is taken apart in -- uint32_t when the launch has fewer than 2^32 items (every chunk under the
//   default cap), so the five divisions per item are 32-bit; long long otherwise.  Addresses are 64-bit either way.
template <typename T, int V, typename I>
__global__ void __launch_bounds__(256) im2col3_kernel(const float* __restrict__ x, T* __restrict__ col, int h, int w, int C, int ho, int wo,
                                                     int stride, int relu, long long total) {
    const I G = (I)(C / V), uwo = (I)wo, uho = (I)ho;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const I ii = (I)i;
        const int g = (int)(ii % G);
        const I t = ii / G;
        const int tap = (int)(t % 9);
        const I row = t / 9;
        const int ox = (int)(row % uwo);
        const I r2 = row / uwo;
        const int oy = (int)(r2 % uho);
        const long long b = (long long)(r2 / uho);
        const int iy = oy * stride + tap / 3 - 1, ix = ox * stride + tap % 3 - 1;
        const bool in = iy >= 0 && iy < h && ix >= 0 && ix < w;
        const float* src = in ? x + ((b * h + iy) * w + ix) * (long long)C + g * V : x;      // formed only for a pixel of the map
        T* dst = col + ((long long)row * 9 + tap) * (long long)C + g * V;
        if constexpr (V == 8) {
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f}, c = a;
            if (in) { a = ld4(src); c = ld4(src + 4); }
            if (relu) { a = relu4(a); c = relu4(c); }
            i32x4 o;
            o[0] = (int)pack_bf16x2(a[0], a[1]); o[1] = (int)pack_bf16x2(a[2], a[3]);
            o[2] = (int)pack_bf16x2(c[0], c[1]); o[3] = (int)pack_bf16x2(c[2], c[3]);
            *reinterpret_cast<i32x4*>(dst) = o;
        } else if constexpr (V == 4) {
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (in) a = ld4(src);
            if (relu) a = relu4(a);
            st4(dst, a);
        } else {
            float a = in ? *src : 0.f;
            if (relu) a = a > 0.f ? a : 0.f;
            *dst = a;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ col2im --
// dx[b][iy][ix][c] = mask(x[b][iy][ix][c]) * sum_{ky, kx} dcol[(b ho + oy) wo + ox][(ky 3 + kx) C + c] + addend[b][iy][ix][c]
// over the taps with oy s + ky - 1 == iy, ox s + kx - 1 == ix inside the output map; ky ascending, kx ascending within it, the sum
// starting from the first term.  mask = (x > 0) when xmask is given (the ReLU in front of the convolution), else 1.
template <int V, typename I>
__global__ void __launch_bounds__(256) col2im3_kernel(const float* __restrict__ dcol, const float* __restrict__ xmask, const float* __restrict__ addend,
                                                     float* __restrict__ dx, int h, int w, int C, int ho, int wo, int stride, long long total) {
    const I G = (I)(C / V), uw = (I)w, uh = (I)h;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const I ii = (I)i;
        const int g = (int)(ii % G);
        const long long p = (long long)(ii / G);               // input pixel (b, iy, ix)
        const I pp = ii / G;
        const int ix = (int)(pp % uw);
        const I p2 = pp / uw;
        const int iy = (int)(p2 % uh);
        const long long b = (long long)(p2 / uh);
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < 3; ++ky) {
            const int ny = iy + 1 - ky;
            if (ny < 0 || ny % stride) continue;
            const int oy = ny / stride;
            if (oy >= ho) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int nx = ix + 1 - kx;
                if (nx < 0 || nx % stride) continue;
                const int ox = nx / stride;
                if (ox >= wo) continue;
                const float* s = dcol + (((b * ho + oy) * wo + ox) * 9 + (ky * 3 + kx)) * (long long)C + g * V;
                if constexpr (V == 4) acc += ld4(s);
                else acc[0] += *s;
            }
        }
        const long long o = p * C + g * V;
        if constexpr (V == 4) {
            if (xmask) {
                const f32x4 m = ld4(xmask + o);
                acc = (f32x4){m[0] > 0.f ? acc[0] : 0.f, m[1] > 0.f ? acc[1] : 0.f, m[2] > 0.f ? acc[2] : 0.f, m[3] > 0.f ? acc[3] : 0.f};
            }
            if (addend) acc += ld4(addend + o);
            st4(dx + o, acc);
        } else {
            float v = acc[0];
            if (xmask) v = xmask[o] > 0.f ? v : 0.f;
            if (addend) v += addend[o];
            dx[o] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- weight layouts --
// wp[o][(ky 3 + kx) Cin + c] = w[o][c][ky][kx]; one element per thread, consecutive threads on consecutive elements of wp
template <typename T>
__global__ void __launch_bounds__(256) wpack3_kernel(const float* __restrict__ w, T* __restrict__ wp, int Cin, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % Cin);
        const long long t = i / Cin;
        const int tap = (int)(t % 9);
        const long long o = t / 9;
        ActT<T>::st(wp + i, w[(o * Cin + c) * 9 + tap]);
    }
}
// dw[o][c][ky][kx] (+)= dwp[o][(ky 3 + kx) Cin + c]; consecutive threads on consecutive elements of dw
__global__ void __launch_bounds__(256) wunpack3_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Cin, int accumulate, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int tap = (int)(i % 9);
        const long long t = i / 9;
        const int c = (int)(t % Cin);
        const long long o = t / Cin;
        const float v = dwp[(o * 9 + tap) * Cin + c];
        dw[i] = accumulate ? dw[i] + v : v;
    }
}

// ------------------------------------------------------------------------------------------- x2 upsample, align_corners --
// PyTorch's upsample_bilinear2d index math with align_corners = True: scale = (in - 1) / (out - 1) in f32 (0 when out == 1),
// src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.  A one-pixel input has scale 0: replicated.
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap tap_ac(int dst, float scale, int in) {
    const float s = scale * (float)dst;
    Tap r;
    r.i0 = (int)s;
    if (r.i0 > in - 1) r.i0 = in - 1;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}

// y[b][oy][ox][c] = l0y (l0x a + l1x b) + l1y (l0x c + l1x d)
template <int V>
__global__ void __launch_bounds__(256) up2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int h, int w, int C, int H, int W, float sy,
                                                     float sx, long long total) {
    const int G = C / V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int g = (int)(i % G);
        const long long p = i / G;
        const int ox = (int)(p % W);
        const long long p2 = p / W;
        const int oy = (int)(p2 % H);
        const long long b = p2 / H;
        const Tap ty = tap_ac(oy, sy, h), tx = tap_ac(ox, sx, w);
        const float* r0 = x + ((b * h + ty.i0) * w) * (long long)C + g * V;
        const float* r1 = x + ((b * h + ty.i1) * w) * (long long)C + g * V;
        const long long c0 = (long long)tx.i0 * C, c1 = (long long)tx.i1 * C;
        if constexpr (V == 4) {
            const f32x4 top = tx.l0 * ld4(r0 + c0) + tx.l1 * ld4(r0 + c1);
            const f32x4 bot = tx.l0 * ld4(r1 + c0) + tx.l1 * ld4(r1 + c1);
            st4(y + p * C + g * 4, ty.l0 * top + ty.l1 * bot);
        } else {
            const float top = tx.l0 * r0[c0] + tx.l1 * r0[c1];
            const float bot = tx.l0 * r1[c0] + tx.l1 * r1[c1];
            y[p * C + g] = ty.l0 * top + ty.l1 * bot;
        }
    }
}

// first output index whose window reaches input index i (its i1 >= i): an estimate from the inverse map, corrected by walking with
// the forward's own formula, so the window is the one the forward used
__device__ __forceinline__ int first_dst_ac(int i, float scale, int in, int out) {
    int e = scale > 0.f ? (int)(((float)i - 1.0f) / scale) - 2 : 0;
    e = e < 0 ? 0 : (e > out - 1 ? out - 1 : e);
    while (e > 0 && tap_ac(e - 1, scale, in).i1 >= i) --e;
    while (e < out && tap_ac(e, scale, in).i1 < i) ++e;
    return e;
}

// dx[b][iy][ix][c] = sum over the output pixels that read (iy, ix) of weight x g: oy ascending, within a row ox ascending, the row
// sum then weighted.  A pixel whose two taps land on the same element (i1 == i0 at the border) contributes l0 + l1.
template <int V>
__global__ void __launch_bounds__(256) up2_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, int h, int w, int C, int H, int W, float sy,
                                                     float sx, long long total) {
    const int G = C / V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cg = (int)(i % G);
        const long long p = i / G;
        const int ix = (int)(p % w);
        const long long p2 = p / w;
        const int iy = (int)(p2 % h);
        const long long b = p2 / h;
        const int oy0 = first_dst_ac(iy, sy, h, H), ox0 = first_dst_ac(ix, sx, w, W);
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int oy = oy0; oy < H; ++oy) {
            const Tap ty = tap_ac(oy, sy, h);
            if (ty.i0 > iy) break;
            const float wy = (ty.i0 == iy ? ty.l0 : 0.f) + (ty.i1 == iy ? ty.l1 : 0.f);
            const float* gr = g + ((b * H + oy) * W) * (long long)C + cg * V;
            f32x4 rs = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int ox = ox0; ox < W; ++ox) {
                const Tap tx = tap_ac(ox, sx, w);
                if (tx.i0 > ix) break;
                const float wx = (tx.i0 == ix ? tx.l0 : 0.f) + (tx.i1 == ix ? tx.l1 : 0.f);
                if constexpr (V == 4) rs += wx * ld4(gr + (long long)ox * C);
                else rs[0] += wx * gr[(long long)ox * C];
            }
            acc += wy * rs;
        }
        if constexpr (V == 4) st4(dx + p * C + cg * 4, acc);
        else dx[p * C + cg] = acc[0];
    }
}

constexpr long long WIDE = 1LL << 32;                            // launches with fewer work items take their index apart in 32 bits

inline bool conv_geom_ok(int n, int h, int w, int C, int stride) {
    return n > 0 && h > 0 && w > 0 && C > 0 && (stride == 1 || stride == 2) && (long long)n * h * w * 9 * C < (1LL << 40);
}

}  // namespace

extern "C" int mmae_conv3x3_im2col(const float* x, void* col, int col_dtype, int n, int h, int w, int C, int stride, int relu, void* stream) {
    MMAE_REQUIRE(x && col && conv_geom_ok(n, h, w, C, stride), "conv3x3_im2col: bad argument");
    MMAE_REQUIRE(col_dtype == MMAE_F32 || col_dtype == MMAE_BF16, "conv3x3_im2col: col_dtype must be f32 or bf16");
    const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    const long long rows = (long long)n * ho * wo;
    hipStream_t st = (hipStream_t)stream;
    if (col_dtype == MMAE_BF16) {
        MMAE_REQUIRE(C % 8 == 0 && al16(x) && al16(col), "conv3x3_im2col: the bf16 form needs C % 8 == 0 and 16-byte aligned pointers");
        const long long total = rows * 9 * (C / 8);
        if (total < WIDE) hipLaunchKernelGGL((im2col3_kernel<uint16_t, 8, uint32_t>), dim3(grid_for(total)), dim3(256), 0, st, x, (uint16_t*)col, h, w, C, ho, wo, stride, relu, total);
        else hipLaunchKernelGGL((im2col3_kernel<uint16_t, 8, long long>), dim3(grid_for(total)), dim3(256), 0, st, x, (uint16_t*)col, h, w, C, ho, wo, stride, relu, total);
    } else if (C % 4 == 0 && al16(x) && al16(col)) {
        const long long total = rows * 9 * (C / 4);
        if (total < WIDE) hipLaunchKernelGGL((im2col3_kernel<float, 4, uint32_t>), dim3(grid_for(total)), dim3(256), 0, st, x, (float*)col, h, w, C, ho, wo, stride, relu, total);
        else hipLaunchKernelGGL((im2col3_kernel<float, 4, long long>), dim3(grid_for(total)), dim3(256), 0, st, x, (float*)col, h, w, C, ho, wo, stride, relu, total);
    } else {
        const long long total = rows * 9 * C;
        if (total < WIDE) hipLaunchKernelGGL((im2col3_kernel<float, 1, uint32_t>), dim3(grid_for(total)), dim3(256), 0, st, x, (float*)col, h, w, C, ho, wo, stride, relu, total);
        else hipLaunchKernelGGL((im2col3_kernel<float, 1, long long>), dim3(grid_for(total)), dim3(256), 0, st, x, (float*)col, h, w, C, ho, wo, stride, relu, total);
    }
    return mmae_check_launch("conv3x3_im2col");
}

extern "C" int mmae_conv3x3_col2im(const float* dcol, const float* xmask, const float* addend, float* dx, int n, int h, int w, int C, int stride,
                                   void* stream) {
    MMAE_REQUIRE(dcol && dx && conv_geom_ok(n, h, w, C, stride), "conv3x3_col2im: bad argument");
    const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    const long long pix = (long long)n * h * w;
    hipStream_t st = (hipStream_t)stream;
    const bool v4 = C % 4 == 0 && al16(dcol) && al16(dx) && (!xmask || al16(xmask)) && (!addend || al16(addend));
    if (v4) {
        const long long total = pix * (C / 4);
        if (total < WIDE) hipLaunchKernelGGL((col2im3_kernel<4, uint32_t>), dim3(grid_for(total)), dim3(256), 0, st, dcol, xmask, addend, dx, h, w, C, ho, wo, stride, total);
        else hipLaunchKernelGGL((col2im3_kernel<4, long long>), dim3(grid_for(total)), dim3(256), 0, st, dcol, xmask, addend, dx, h, w, C, ho, wo, stride, total);
    } else {
        const long long total = pix * C;
        if (total < WIDE) hipLaunchKernelGGL((col2im3_kernel<1, uint32_t>), dim3(grid_for(total)), dim3(256), 0, st, dcol, xmask, addend, dx, h, w, C, ho, wo, stride, total);
        else hipLaunchKernelGGL((col2im3_kernel<1, long long>), dim3(grid_for(total)), dim3(256), 0, st, dcol, xmask, addend, dx, h, w, C, ho, wo, stride, total);
    }
    return mmae_check_launch("conv3x3_col2im");
}

extern "C" int mmae_conv3x3_weight_pack(const float* w, void* wp, int wp_dtype, int Cout, int Cin, void* stream) {
    MMAE_REQUIRE(w && wp && Cout > 0 && Cin > 0, "conv3x3_weight_pack: bad argument");
    MMAE_REQUIRE(wp_dtype == MMAE_F32 || wp_dtype == MMAE_BF16, "conv3x3_weight_pack: wp_dtype must be f32 or bf16");
    const long long total = (long long)Cout * 9 * Cin;
    if (wp_dtype == MMAE_BF16)
        hipLaunchKernelGGL(wpack3_kernel<uint16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, (uint16_t*)wp, Cin, total);
    else
        hipLaunchKernelGGL(wpack3_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, (float*)wp, Cin, total);
    return mmae_check_launch("conv3x3_weight_pack");
}

extern "C" int mmae_conv3x3_weight_unpack(const float* dwp, float* dw, int Cout, int Cin, int accumulate, void* stream) {
    MMAE_REQUIRE(dwp && dw && Cout > 0 && Cin > 0, "conv3x3_weight_unpack: bad argument");
    const long long total = (long long)Cout * 9 * Cin;
    hipLaunchKernelGGL(wunpack3_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, dwp, dw, Cin, accumulate, total);
    return mmae_check_launch("conv3x3_weight_unpack");
}

extern "C" int mmae_upsample2x_fwd(const float* x, float* y, int B, int h, int w, int C, void* stream) {
    MMAE_REQUIRE(x && y && B > 0 && h > 0 && w > 0 && C > 0 && (long long)B * h * w * 4 * C < (1LL << 40), "upsample2x_fwd: bad argument");
    const int H = 2 * h, W = 2 * w;
    const float sy = (float)(h - 1) / (float)(H - 1), sx = (float)(w - 1) / (float)(W - 1);
    const long long pix = (long long)B * H * W;
    if (C % 4 == 0 && al16(x) && al16(y))
        hipLaunchKernelGGL(up2_fwd_kernel<4>, dim3(grid_for(pix * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, y, h, w, C, H, W, sy, sx, pix * (C / 4));
    else
        hipLaunchKernelGGL(up2_fwd_kernel<1>, dim3(grid_for(pix * C)), dim3(256), 0, (hipStream_t)stream, x, y, h, w, C, H, W, sy, sx, pix * C);
    return mmae_check_launch("upsample2x_fwd");
}

extern "C" int mmae_upsample2x_bwd(const float* g, float* dx, int B, int h, int w, int C, void* stream) {
    MMAE_REQUIRE(g && dx && B > 0 && h > 0 && w > 0 && C > 0 && (long long)B * h * w * 4 * C < (1LL << 40), "upsample2x_bwd: bad argument");
    const int H = 2 * h, W = 2 * w;
    const float sy = (float)(h - 1) / (float)(H - 1), sx = (float)(w - 1) / (float)(W - 1);
    const long long pix = (long long)B * h * w;
    if (C % 4 == 0 && al16(g) && al16(dx))
        hipLaunchKernelGGL(up2_bwd_kernel<4>, dim3(grid_for(pix * (C / 4))), dim3(256), 0, (hipStream_t)stream, g, dx, h, w, C, H, W, sy, sx, pix * (C / 4));
    else
        hipLaunchKernelGGL(up2_bwd_kernel<1>, dim3(grid_for(pix * C)), dim3(256), 0, (hipStream_t)stream, g, dx, h, w, C, H, W, sy, sx, pix * C);
    return mmae_check_launch("upsample2x_bwd");
}
