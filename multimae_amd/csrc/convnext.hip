// ConvNeXt semantic-segmentation head (ConvNeXtAdapter, output_adapters.py:481-573; ConvNeXtBlock, output_adapter_utils.py:19-57).
//
// The feature map is kept channels-last, f32 [B][h][w][C]: every pixel is a row of C, so the block's LayerNorm and its two 1x1
// convolutions are the engine's row kernels and GEMMs (mmae_layernorm_*, mmae_gemm).  This file holds what is not a row op:
//   - the token-row gather in front of proj_dec (adapt_tokens, output_adapters.py:542-550) and its scatter for the backward;
//   - the pixel shuffle of the proj_dec output into the map (the two rearranges of output_adapters.py:558-563) and its inverse;
//   - the depthwise 7x7 convolution (ConvNeXtBlock.dwconv, output_adapter_utils.py:37,46): forward, data gradient with the
//     block's residual gradient added in the same pass, and the weight gradient as per-workgroup partials (no atomics; the
//     caller sums them in a fixed order with mmae_colsum_partials);
//   - the final F.interpolate (output_adapters.py:568) from the low-resolution NHWC logits to the full-resolution NCHW output,
//     bilinear or nearest with PyTorch's source-index formulas (align_corners=False, scale = in / out), and its backward as a
//     gather: every low-resolution element sums its own output window in a fixed order.  The index map and the gather walk are
//     resize_map.h's, shared with the losses that read the low-resolution map (segloss.hip, regloss.hip).
#include "resize_map.h"

namespace {

// ---------------------------------------------------------------------------------------------------- depthwise 7x7 --
// One workgroup: a TH x TW tile of output pixels x NG channel groups of V channels (V = 4: one 16-byte load per pixel and group,
// needs C % 4 == 0 and 16-byte aligned tensors; V = 1 for any C).  The input tile with its 3-pixel halo is staged in LDS,
// out-of-image pixels and channels >= C as zeros.  Each thread computes RW consecutive outputs of one row and one group,
// sliding the 7-tap window along the row in registers.
constexpr int DW_TH = 8, DW_TW = 16, DW_NG = 8, DW_RW = 4;
constexpr int DW_HH = DW_TH + 6, DW_HW = DW_TW + 6;
static_assert(DW_NG * DW_TH * (DW_TW / DW_RW) == 256, "dwconv: 256 threads");

template <int V> struct Vec;
template <> struct Vec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ T zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ T ld(const float* p, int nval) { (void)nval; return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ void st(float* p, T v) { *reinterpret_cast<f32x4*>(p) = v; }
};
template <> struct Vec<1> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ T ld(const float* p, int nval) { (void)nval; return *p; }
    static __device__ __forceinline__ void st(float* p, T v) { *p = v; }
};
template <int V> __device__ __forceinline__ float lane_of(typename Vec<V>::T v, int j);
template <> __device__ __forceinline__ float lane_of<4>(f32x4 v, int j) { return v[j]; }
template <> __device__ __forceinline__ float lane_of<1>(float v, int j) { (void)j; return v; }
template <int V> __device__ __forceinline__ void set_lane(typename Vec<V>::T& v, int j, float x);
template <> __device__ __forceinline__ void set_lane<4>(f32x4& v, int j, float x) { v[j] = x; }
template <> __device__ __forceinline__ void set_lane<1>(float& v, int j, float x) { (void)j; v = x; }

// y = dwconv(x) (+ bias[c]) (+ resid).  FLIP = 1 reads the taps mirrored: the transposed convolution of the data gradient,
// dx[y][x] = sum dy[y + 3 - ky][x + 3 - kx] w[ky][kx].  Per output: 49 FMAs in ky-major, kx-minor order from 0, then the
// bias, then the residual.
template <int V, int FLIP>
__global__ void __launch_bounds__(256) dwconv7_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                                                     const float* __restrict__ resid, float* __restrict__ y, int h, int w, int C, int tiles_w) {
    typedef typename Vec<V>::T T;
    __shared__ T xs[DW_HH * DW_HW][DW_NG];
    __shared__ T ws[49][DW_NG];
    const int tid = threadIdx.x;
    const int ty0 = (int)(blockIdx.x / tiles_w) * DW_TH, tx0 = (int)(blockIdx.x % tiles_w) * DW_TW;
    const int c0 = blockIdx.y * DW_NG * V;
    const long long img = (long long)blockIdx.z * h * w;
    for (int i = tid; i < 49 * DW_NG; i += 256) {
        const int k = i / DW_NG, g = i % DW_NG;
        T v = Vec<V>::zero();
        for (int j = 0; j < V; ++j) {
            const int c = c0 + g * V + j;
            if (c < C) set_lane<V>(v, j, wt[(long long)c * 49 + (FLIP ? 48 - k : k)]);
        }
        ws[k][g] = v;
    }
    for (int i = tid; i < DW_HH * DW_HW * DW_NG; i += 256) {
        const int g = i % DW_NG, p = i / DW_NG;
        const int iy = ty0 - 3 + p / DW_HW, ix = tx0 - 3 + p % DW_HW, c = c0 + g * V;
        T v = Vec<V>::zero();
        if (iy >= 0 && iy < h && ix >= 0 && ix < w && c < C) v = Vec<V>::ld(x + (img + (long long)iy * w + ix) * C + c, C - c);
        xs[p][g] = v;
    }
    __syncthreads();
    const int g = tid % DW_NG, r = tid / DW_NG;
    const int row = r / (DW_TW / DW_RW), ox0 = (r % (DW_TW / DW_RW)) * DW_RW;
    T acc[DW_RW];
#pragma unroll
    for (int q = 0; q < DW_RW; ++q) acc[q] = Vec<V>::zero();
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
        T xv[DW_RW + 6];
#pragma unroll
        for (int j = 0; j < DW_RW + 6; ++j) xv[j] = xs[(row + ky) * DW_HW + ox0 + j][g];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const T wv = ws[ky * 7 + kx][g];
#pragma unroll
            for (int q = 0; q < DW_RW; ++q) acc[q] = __builtin_elementwise_fma(xv[q + kx], wv, acc[q]);
        }
    }
    const int oy = ty0 + row, c = c0 + g * V;
    if (oy >= h || c >= C) return;
    T bv = Vec<V>::zero();
    if (bias) {
        for (int j = 0; j < V; ++j) set_lane<V>(bv, j, bias[c + j]);
    }
#pragma unroll
    for (int q = 0; q < DW_RW; ++q) {
        const int ox = tx0 + ox0 + q;
        if (ox >= w) break;
        const long long o = (img + (long long)oy * w + ox) * C + c;
        T v = acc[q];
        if (bias) v = v + bv;
        if (resid) v = v + Vec<V>::ld(resid + o, C - c);
        Vec<V>::st(y + o, v);
    }
}

// Weight-gradient partials: part[blk][c * 49 + ky * 7 + kx] = sum over the workgroup's pixels of dy[p][c] x[p + (ky - 3, kx - 3)][c],
// blk = one spatial strip (DW_TPER tiles of DW_TH rows down one column of DW_TW-wide tiles of one image).  Threads: NG groups x 7 ky x
// 4 row pairs (224 of 256 busy); each keeps 7 kx accumulators; the 4 row pairs are summed through LDS in a fixed order.
constexpr int DW_TPER = 4;
template <int V>
__global__ void __launch_bounds__(256) dwconv7_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                           int h, int w, int C, int tiles_w, int strips_h) {
    typedef typename Vec<V>::T T;
    constexpr int XS = DW_HH * DW_HW * DW_NG, DS = DW_TH * DW_TW * DW_NG, RED = 4 * 49 * DW_NG;
    constexpr int NS = (XS + DS) > RED ? (XS + DS) : RED;
    __shared__ T sm[NS];
    T* xs = sm;
    T* ds = sm + XS;
    const int tid = threadIdx.x;
    const int blk = blockIdx.x;
    const int b = blk / (strips_h * tiles_w), rem = blk % (strips_h * tiles_w);
    const int sy = rem / tiles_w, tx0 = (rem % tiles_w) * DW_TW;
    const int c0 = blockIdx.y * DW_NG * V;
    const long long img = (long long)b * h * w;
    const int g = tid % DW_NG, t2 = tid / DW_NG;            // t2 in [0, 32): ky = t2 % 7, row pair = t2 / 7 (< 4 busy)
    const int ky = t2 % 7, rp = t2 / 7;
    T acc[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = Vec<V>::zero();
    for (int t = 0; t < DW_TPER; ++t) {
        const int ty0 = (sy * DW_TPER + t) * DW_TH;
        if (ty0 >= h) break;
        for (int i = tid; i < DW_HH * DW_HW * DW_NG; i += 256) {
            const int gg = i % DW_NG, p = i / DW_NG;
            const int iy = ty0 - 3 + p / DW_HW, ix = tx0 - 3 + p % DW_HW, c = c0 + gg * V;
            T v = Vec<V>::zero();
            if (iy >= 0 && iy < h && ix >= 0 && ix < w && c < C) v = Vec<V>::ld(x + (img + (long long)iy * w + ix) * C + c, C - c);
            xs[i] = v;
        }
        for (int i = tid; i < DW_TH * DW_TW * DW_NG; i += 256) {
            const int gg = i % DW_NG, p = i / DW_NG;
            const int oy = ty0 + p / DW_TW, ox = tx0 + p % DW_TW, c = c0 + gg * V;
            T v = Vec<V>::zero();                            // pixels outside the image contribute nothing
            if (oy < h && ox < w && c < C) v = Vec<V>::ld(dy + (img + (long long)oy * w + ox) * C + c, C - c);
            ds[i] = v;
        }
        __syncthreads();
        if (rp < 4) {
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                const int py = rp * 2 + pr;
                T xv[DW_TW + 6];
#pragma unroll
                for (int j = 0; j < DW_TW + 6; ++j) xv[j] = xs[((py + ky) * DW_HW + j) * DW_NG + g];
#pragma unroll
                for (int px = 0; px < DW_TW; ++px) {
                    const T dv = ds[(py * DW_TW + px) * DW_NG + g];
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) acc[kx] = __builtin_elementwise_fma(dv, xv[px + kx], acc[kx]);
                }
            }
        }
        __syncthreads();
    }
    T* red = sm;                                             // [4][49][NG], after the last barrier above
    if (rp < 4) {
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) red[(rp * 49 + ky * 7 + kx) * DW_NG + g] = acc[kx];
    }
    __syncthreads();
    float* out = part + (long long)blk * C * 49;
    for (int i = tid; i < 49 * DW_NG; i += 256) {
        const int k = i / DW_NG, gg = i % DW_NG;
        T s = red[(0 * 49 + k) * DW_NG + gg];
        s = s + red[(1 * 49 + k) * DW_NG + gg];
        s = s + red[(2 * 49 + k) * DW_NG + gg];
        s = s + red[(3 * 49 + k) * DW_NG + gg];
        for (int j = 0; j < V; ++j) {
            const int c = c0 + gg * V + j;
            if (c < C) out[(long long)c * 49 + k] = lane_of<V>(s, j);
        }
    }
}

// ---------------------------------------------------------------------------------------------- rows / pixel shuffle --
// out[(b * N + n)][col_off + d] = enc[b][start + n][d]  (act dtype out, row stride ld_out)
template <typename TO>
__global__ void __launch_bounds__(256) rows_gather_kernel(const float* __restrict__ enc, TO* __restrict__ out, int n_tok, int D, int start, int N,
                                                         long long ld_out, int col_off, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int d = (int)(i % D);
        const long long r = i / D;
        const int n = (int)(r % N);
        const long long b = r / N;
        ActT<TO>::st(out + r * ld_out + col_off + d, enc[(b * n_tok + start + n) * D + d]);
    }
}
// d_enc[b][start + n][d] = src[(b * N + n)][col_off + d]  (f32 out; rows of other tasks untouched)
template <typename TI>
__global__ void __launch_bounds__(256) rows_scatter_kernel(const TI* __restrict__ src, float* __restrict__ d_enc, int n_tok, int D, int start,
                                                          int N, long long ld_src, int col_off, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int d = (int)(i % D);
        const long long r = i / D;
        const int n = (int)(r % N);
        const long long b = r / N;
        d_enc[(b * n_tok + start + n) * D + d] = ActT<TI>::ld(src + r * ld_src + col_off + d);
    }
}

// map[b][nh * s + ph][nw * s + pw][c] = proj[b][nh * NW + nw][(ph * s + pw) * C + c]: both are [B * NH * NW * s * s][C] row sets, and
// one map row (pixel) is one C-wide slice of a proj row.  INV = 1 moves the other way (the backward).  Pure copies: bit-exact.
template <int V, int INV>
__global__ void __launch_bounds__(256) shuffle_kernel(const float* __restrict__ src, float* __restrict__ dst, int NH, int NW, int s, int C,
                                                     long long total) {
    typedef typename Vec<V>::T T;
    const int CV = C / V;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cv = (int)(i % CV);
        long long p = i / CV;                                // map pixel index (b, y, x)
        const int w = NW * s;
        const int xx = (int)(p % w);
        long long t = p / w;
        const int yy = (int)(t % (NH * s));
        const long long b = t / (NH * s);
        const int nh = yy / s, ph = yy % s, nw = xx / s, pw = xx % s;
        const long long q = ((b * NH + nh) * NW + nw) * (long long)(s * s) + ph * s + pw;     // proj slice index
        const long long mo = p * C + cv * V, po = q * C + cv * V;
        if (INV) Vec<V>::st(dst + po, Vec<V>::ld(src + mo, V));
        else Vec<V>::st(dst + mo, Vec<V>::ld(src + po, V));
    }
}

// ------------------------------------------------------------------------------------------------------------ resize --
// out[b][k][oy][ox] from x[b][iy][ix][k] (row stride ldx); each thread 4 consecutive ox of one output row
template <int BILINEAR>
__global__ void __launch_bounds__(256) resize_fwd_kernel(const float* __restrict__ x, long long ldx, float* __restrict__ out, int h, int w, int K,
                                                        int H, int W, float sy, float sx, long long total, int vec_store) {
    const int Wq = (W + 3) / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int oq = (int)(i % Wq);
        long long t = i / Wq;
        const int oy = (int)(t % H);
        t /= H;
        const int k = (int)(t % K);
        const long long b = t / K;
        const float* xb = x + b * h * w * ldx + k;
        float v[4];
        if (BILINEAR) {
            const Src ry = src_bilinear(oy, sy, h);
            const float* r0 = xb + (long long)ry.i0 * w * ldx;
            const float* r1 = xb + (long long)ry.i1 * w * ldx;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ox = oq * 4 + q < W ? oq * 4 + q : W - 1;
                const Src rx = src_bilinear(ox, sx, w);
                // ry.l0 (rx.l0 a + rx.l1 b) + ry.l1 (rx.l0 c + rx.l1 d) with its roundings fixed (common.h): ox = 4 oq + q has q's parity
                v[q] = resize_tap4(ry.l0, ry.l1, rx.l0, rx.l1, r0[rx.i0 * ldx], r0[rx.i1 * ldx], r1[rx.i0 * ldx], r1[rx.i1 * ldx],
                                   (q & 1) != 0);
            }
        } else {
            const float* r0 = xb + (long long)src_nearest(oy, sy, h) * w * ldx;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ox = oq * 4 + q < W ? oq * 4 + q : W - 1;
                v[q] = r0[src_nearest(ox, sx, w) * ldx];
            }
        }
        float* o = out + ((b * K + k) * H + oy) * (long long)W + oq * 4;
        if (vec_store) {
            *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
        } else {
            for (int q = 0; q < 4 && oq * 4 + q < W; ++q) o[q] = v[q];
        }
    }
}

// dx[b][iy][ix][k] (row stride ldx; columns K .. ldx - 1 written as 0) = sum over the output pixels that read (iy, ix) of their
// weight times g[b][k][oy][ox], in resize_gather's fixed order
template <int BILINEAR>
__global__ void __launch_bounds__(256) resize_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, long long ldx, int h, int w, int K,
                                                        int H, int W, float sy, float sx, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ix = (int)(i % w);
        long long t = i / w;
        const int iy = (int)(t % h);
        t /= h;
        const int k = (int)(t % ldx);
        const long long b = t / ldx;
        float* o = dx + ((b * h + iy) * w + ix) * ldx + k;
        if (k >= K) { *o = 0.f; continue; }
        const float* gb = g + (b * K + k) * (long long)H * W;
        *o = resize_gather<BILINEAR>(gb, iy, ix, h, w, H, W, sy, sx, [](float g) { return g; });
    }
}

inline bool al16(const void* p) { return p == nullptr || ((uintptr_t)p % 16) == 0; }

}  // namespace

// adapt_tokens + the concatenation along features (output_adapters.py:542-550), one main task per call (col_off = its column block).
extern "C" int mmae_convnext_rows_gather(const float* enc, void* out, int out_dtype, int B, int n_tok, int D, int start, int N, int64_t ld_out,
                                         int col_off, void* stream) {
    MMAE_REQUIRE(enc && out && B > 0 && D > 0 && N > 0 && start >= 0 && start + N <= n_tok && col_off >= 0 && ld_out >= col_off + D,
                 "convnext_rows_gather: bad argument");
    MMAE_REQUIRE(out_dtype == MMAE_F32 || out_dtype == MMAE_BF16, "convnext_rows_gather: out_dtype must be f32 or bf16");
    const long long total = (long long)B * N * D;
    if (out_dtype == MMAE_BF16)
        hipLaunchKernelGGL(rows_gather_kernel<uint16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, enc, (uint16_t*)out, n_tok, D, start,
                           N, (long long)ld_out, col_off, total);
    else
        hipLaunchKernelGGL(rows_gather_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, enc, (float*)out, n_tok, D, start, N,
                           (long long)ld_out, col_off, total);
    return mmae_check_launch("convnext_rows_gather");
}

// its backward: the encoder_tokens gradient of one task's rows (torch.cat / slicing backward, output_adapters.py:542-550)
extern "C" int mmae_convnext_rows_scatter(const void* src, int src_dtype, float* d_enc, int B, int n_tok, int D, int start, int N, int64_t ld_src,
                                          int col_off, void* stream) {
    MMAE_REQUIRE(src && d_enc && B > 0 && D > 0 && N > 0 && start >= 0 && start + N <= n_tok && col_off >= 0 && ld_src >= col_off + D,
                 "convnext_rows_scatter: bad argument");
    MMAE_REQUIRE(src_dtype == MMAE_F32 || src_dtype == MMAE_BF16, "convnext_rows_scatter: src_dtype must be f32 or bf16");
    const long long total = (long long)B * N * D;
    if (src_dtype == MMAE_BF16)
        hipLaunchKernelGGL(rows_scatter_kernel<uint16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, d_enc, n_tok,
                           D, start, N, (long long)ld_src, col_off, total);
    else
        hipLaunchKernelGGL(rows_scatter_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)src, d_enc, n_tok, D,
                           start, N, (long long)ld_src, col_off, total);
    return mmae_check_launch("convnext_rows_scatter");
}

static int shuffle(const float* src, float* dst, int B, int NH, int NW, int s, int C, void* stream, int inv, const char* what) {
    MMAE_REQUIRE(src && dst && B > 0 && NH > 0 && NW > 0 && s > 0 && C > 0, what);
    const bool v4 = C % 4 == 0 && al16(src) && al16(dst);
    const long long total = (long long)B * NH * NW * s * s * (v4 ? C / 4 : C);
    const dim3 grid(grid_for(total)), block(256);
    if (v4) {
        if (inv) hipLaunchKernelGGL((shuffle_kernel<4, 1>), grid, block, 0, (hipStream_t)stream, src, dst, NH, NW, s, C, total);
        else hipLaunchKernelGGL((shuffle_kernel<4, 0>), grid, block, 0, (hipStream_t)stream, src, dst, NH, NW, s, C, total);
    } else {
        if (inv) hipLaunchKernelGGL((shuffle_kernel<1, 1>), grid, block, 0, (hipStream_t)stream, src, dst, NH, NW, s, C, total);
        else hipLaunchKernelGGL((shuffle_kernel<1, 0>), grid, block, 0, (hipStream_t)stream, src, dst, NH, NW, s, C, total);
    }
    return mmae_check_launch(what);
}
// proj_dec output [B][NH * NW][s * s * C] -> map f32 [B][NH * s][NW * s][C] (the two rearranges, output_adapters.py:558-563)
extern "C" int mmae_convnext_shuffle_fwd(const float* proj, float* map, int B, int NH, int NW, int s, int C, void* stream) {
    return shuffle(proj, map, B, NH, NW, s, C, stream, 0, "convnext_shuffle_fwd: bad argument");
}
// ... and back: d_map -> d_proj (their backward)
extern "C" int mmae_convnext_shuffle_bwd(const float* d_map, float* d_proj, int B, int NH, int NW, int s, int C, void* stream) {
    return shuffle(d_map, d_proj, B, NH, NW, s, C, stream, 1, "convnext_shuffle_bwd: bad argument");
}

static int dwconv(const float* x, const float* wt, const float* bias, const float* resid, float* y, int B, int h, int w, int C, void* stream, int flip,
                  const char* what) {
    MMAE_REQUIRE(x && wt && y && B > 0 && h > 0 && w > 0 && C > 0 && B <= 65535, what);
    const int tiles_w = (w + DW_TW - 1) / DW_TW, tiles_h = (h + DW_TH - 1) / DW_TH;
    MMAE_REQUIRE((long long)tiles_w * tiles_h < (1LL << 31), what);
    const bool v4 = C % 4 == 0 && al16(x) && al16(y) && al16(resid);
    const int V = v4 ? 4 : 1;
    const dim3 grid((unsigned)(tiles_w * tiles_h), (unsigned)((C + DW_NG * V - 1) / (DW_NG * V)), (unsigned)B), block(256);
    MMAE_REQUIRE(grid.y <= 65535, what);
    if (v4) {
        if (flip) hipLaunchKernelGGL((dwconv7_kernel<4, 1>), grid, block, 0, (hipStream_t)stream, x, wt, bias, resid, y, h, w, C, tiles_w);
        else hipLaunchKernelGGL((dwconv7_kernel<4, 0>), grid, block, 0, (hipStream_t)stream, x, wt, bias, resid, y, h, w, C, tiles_w);
    } else {
        if (flip) hipLaunchKernelGGL((dwconv7_kernel<1, 1>), grid, block, 0, (hipStream_t)stream, x, wt, bias, resid, y, h, w, C, tiles_w);
        else hipLaunchKernelGGL((dwconv7_kernel<1, 0>), grid, block, 0, (hipStream_t)stream, x, wt, bias, resid, y, h, w, C, tiles_w);
    }
    return mmae_check_launch(what);
}
// ConvNeXtBlock.dwconv (output_adapter_utils.py:37,46): y = depthwise 7x7 (padding 3) of x + bias; x, y f32 [B][h][w][C], w [C][7][7]
extern "C" int mmae_dwconv7_fwd(const float* x, const float* w7, const float* bias, float* y, int B, int h, int w, int C, void* stream) {
    return dwconv(x, w7, bias, nullptr, y, B, h, w, C, stream, 0, "dwconv7_fwd: bad argument");
}
// its data gradient with the block's residual gradient (output_adapter_utils.py:56, x = input + ...) added in the same pass:
// dx_out = dx_in + dwconv^T(dy).  dx_in may be NULL.
extern "C" int mmae_dwconv7_dgrad(const float* dy, const float* w7, const float* dx_in, float* dx_out, int B, int h, int w, int C, void* stream) {
    return dwconv(dy, w7, nullptr, dx_in, dx_out, B, h, w, C, stream, 1, "dwconv7_dgrad: bad argument");
}
// rows of the weight-gradient partials mmae_dwconv7_wgrad writes
extern "C" int mmae_dwconv7_wgrad_nblk(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0) return 0;
    const int tiles_w = (w + DW_TW - 1) / DW_TW, strips = ((h + DW_TH - 1) / DW_TH + DW_TPER - 1) / DW_TPER;
    return B * tiles_w * strips;
}
// its weight gradient: part[nblk][C * 49] (nblk = mmae_dwconv7_wgrad_nblk), row j = workgroup j's sums of dy . x_shifted in the
// layout of dwconv.weight (C, 1, 7, 7).  The caller sums the rows with mmae_colsum_partials (fixed order, no atomics).
extern "C" int mmae_dwconv7_wgrad(const float* x, const float* dy, float* part, int B, int h, int w, int C, void* stream) {
    MMAE_REQUIRE(x && dy && part && B > 0 && h > 0 && w > 0 && C > 0, "dwconv7_wgrad: bad argument");
    const int tiles_w = (w + DW_TW - 1) / DW_TW, strips = ((h + DW_TH - 1) / DW_TH + DW_TPER - 1) / DW_TPER;
    const bool v4 = C % 4 == 0 && al16(x) && al16(dy);
    const int V = v4 ? 4 : 1;
    const long long nblk = (long long)B * tiles_w * strips;
    MMAE_REQUIRE(nblk < (1LL << 31), "dwconv7_wgrad: map too large");
    const dim3 grid((unsigned)nblk, (unsigned)((C + DW_NG * V - 1) / (DW_NG * V))), block(256);
    MMAE_REQUIRE(grid.y <= 65535, "dwconv7_wgrad: C too large");
    if (v4) hipLaunchKernelGGL(dwconv7_wgrad_kernel<4>, grid, block, 0, (hipStream_t)stream, x, dy, part, h, w, C, tiles_w, strips);
    else hipLaunchKernelGGL(dwconv7_wgrad_kernel<1>, grid, block, 0, (hipStream_t)stream, x, dy, part, h, w, C, tiles_w, strips);
    return mmae_check_launch("dwconv7_wgrad");
}

// F.interpolate(x, size=(H, W), mode='bilinear' (mode 0) | 'nearest' (mode 1)) of output_adapters.py:568: x f32 [B][h][w][K] (row stride
// ldx >= K) -> out f32 NCHW [B][K][H][W]
extern "C" int mmae_resize_fwd(const float* x, int64_t ldx, float* out, int B, int h, int w, int K, int H, int W, int mode, void* stream) {
    MMAE_REQUIRE(x && out && resize_geom_ok(B, h, w, K, H, W, ldx, mode), "resize_fwd: bad argument");
    const ResizeScale sc(h, w, H, W);
    const long long total = (long long)B * K * H * ((W + 3) / 4);
    const int vec = (W % 4 == 0) && al16(out);
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(resize_fwd_kernel<decltype(bl)::value>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx, out,
                           h, w, K, H, W, sc.sy, sc.sx, total, vec);
    });
    return mmae_check_launch("resize_fwd");
}
// its backward as a gather: g f32 NCHW [B][K][H][W] -> dx f32 [B][h][w][ldx] (columns K .. ldx - 1 zeroed: a GEMM operand's padding)
extern "C" int mmae_resize_bwd(const float* g, float* dx, int64_t ldx, int B, int h, int w, int K, int H, int W, int mode, void* stream) {
    MMAE_REQUIRE(g && dx && resize_geom_ok(B, h, w, K, H, W, ldx, mode), "resize_bwd: bad argument");
    const ResizeScale sc(h, w, H, W);
    const long long total = (long long)B * h * w * ldx;
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(resize_bwd_kernel<decltype(bl)::value>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, g, dx, (long long)ldx,
                           h, w, K, H, W, sc.sy, sc.sx, total);
    });
    return mmae_check_launch("resize_bwd");
}
