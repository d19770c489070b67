// Dense regression losses and the NYU depth metrics on the ConvNeXt head's LOW-RESOLUTION map (functions.SegHandle,
// criterion.masked_l1_loss / masked_mse_loss / masked_berhu_loss, metrics.depth_metrics): the (B, K, H, W) image F.interpolate would
// write is never read.
//   reg_loss_fwd    masked L1 / MSE / berHu of the interpolated prediction against target f32 [B][K][H][W]: the masked difference is
//                   stored, per-workgroup partials (sum |d|, sum d^2, max |d|, valid count) are reduced in double by a finish kernel;
//                   berHu takes a second pass over the stored difference once c = max(0.2 max|d|, 1e-5) is known
//   reg_loss_bwd    the gradient with respect to the low-resolution map: the gather form of resize_bwd_kernel over g(d)
//   depth_metrics   the eight sums behind rmse, rel, srel, log10, delta_1..3 in one pass, the ratios in a finish kernel
// The interpolation takes its taps and weights from resize_map.h -- the functions resize_fwd_kernel calls -- and combines the four
// taps with common.h's resize_tap4 as that kernel does (every rounding written out), so the value the loss sees is the pixel
// mmae_resize_fwd would store (tests/test_reg_loss_gpu.py checks the bits); the backward is resize_map.h's gather walk over g(d).
//
// Work shape: K is 1 (depth) or 3 (normals, rgb), so pixels, not channels, lie on the lanes: one thread per output pixel, lanes along
// ox (coalesced target / mask / difference accesses; the low-resolution rows come from cache), a short loop over k <= MMAE_REG_MAX_K.
// In-wave reductions by wave64 shuffles, LDS only to join the four waves in wave order, no float atomics: run-to-run results are
// bit-equal.  Columns K .. ldx - 1 of the map are never read.
//
// The second part of the file (reg_img_fwd, reg_img_bwd, depth_metrics_img) evaluates the same losses and metrics on a prediction that
// is the image itself, the DPT head's, with the finish kernels of the first.
#include "resize_map.h"

namespace {

constexpr int WAVES = 4;                      // waves per workgroup (256 threads)
enum { KIND_L1 = 0, KIND_MSE = 1, KIND_BERHU = 2 };

// The source of one output pixel: element offsets of its (up to) four taps in the map, channel 0.
template <int BILINEAR>
struct Taps {
    Src ry, rx;
    long long o00, o01, o10, o11;
    bool odd;
    __device__ __forceinline__ Taps(long long b, int oy, int ox, int h, int w, long long ldx, float sy, float sx) {
        const long long base = b * h * w;
        odd = (ox & 1) != 0;
        if (BILINEAR) {
            ry = src_bilinear(oy, sy, h);
            rx = src_bilinear(ox, sx, w);
            o00 = (base + (long long)ry.i0 * w + rx.i0) * ldx;
            o01 = (base + (long long)ry.i0 * w + rx.i1) * ldx;
            o10 = (base + (long long)ry.i1 * w + rx.i0) * ldx;
            o11 = (base + (long long)ry.i1 * w + rx.i1) * ldx;
        } else {
            ry = rx = Src{0, 0, 0.f, 0.f};
            o00 = o01 = o10 = o11 = (base + (long long)src_nearest(oy, sy, h) * w + src_nearest(ox, sx, w)) * ldx;
        }
    }
    __device__ __forceinline__ float at(const float* __restrict__ x, int k) const {
        if (BILINEAR) return resize_tap4(ry.l0, ry.l1, rx.l0, rx.l1, x[o00 + k], x[o01 + k], x[o10 + k], x[o11 + k], odd);
        return x[o00 + k];
    }
};

// diff[b][k][oy][ox] = mask ? z - target : 0;  partial[4 i .. 4 i + 3] = workgroup i's sum |d|, sum d^2, max |d|, valid count
template <int BILINEAR>
__global__ void __launch_bounds__(256) reg_fwd_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ target,
                                                     const unsigned char* __restrict__ mask, int Cm, float* __restrict__ diff,
                                                     float* __restrict__ partial, int h, int w, int K, int H, int W, float sy, float sx,
                                                     long long total) {
    __shared__ float sh[4 * WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long plane = (long long)H * W;
    float sa = 0.f, sq = 0.f, mx = 0.f;
    int cnt = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % W);
        const long long t = i / W;
        const int oy = (int)(t % H);
        const long long b = t / H;
        const Taps<BILINEAR> tp(b, oy, ox, h, w, ldx, sy, sx);
        const long long pix = (long long)oy * W + ox;
        for (int k = 0; k < K; ++k) {
            const long long e = (b * K + k) * plane + pix;
            const bool m = mask == nullptr || mask[(b * Cm + (Cm == 1 ? 0 : k)) * plane + pix] != 0;
            const float d = m ? tp.at(x, k) - target[e] : 0.f;
            diff[e] = d;
            const float a = fabsf(d);
            sa += a;
            sq = __builtin_fmaf(d, d, sq);
            mx = fmaxf(mx, a);
            cnt += m ? 1 : 0;
        }
    }
    sa = wave_sum(sa);
    sq = wave_sum(sq);
    mx = wave_max(mx);
    const float cf = wave_sum((float)cnt);                      // integers far below 2^24: exact
    if (lane == 0) { sh[wave] = sa; sh[WAVES + wave] = sq; sh[2 * WAVES + wave] = mx; sh[3 * WAVES + wave] = cf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = partial + 4 * (long long)blockIdx.x;
        p[0] = join4_sum(sh);
        p[1] = join4_sum(sh + WAVES);
        p[2] = join4_max(sh + 2 * WAVES);
        p[3] = join4_sum(sh + 3 * WAVES);
    }
}

// out = [loss, count, max |d|, c]: L1 sum |d| / count, MSE sum d^2 / count (0 when nothing is valid), divided in double by the exact
// count; out[1] is the count rounded to f32 (exact up to 2^24), which berHu's finish and the backward's scale divide by.  berHu's loss is written by
// reg_berhu_finish_kernel.  c = max(0.2f max|d|, 1e-5f) in f32, as the reference forms it (run_finetuning_depth.py:78).
__global__ void __launch_bounds__(256) reg_finish_kernel(const float* __restrict__ partial, int nb, int kind, float* __restrict__ out) {
    __shared__ double s[256], q[256], c[256];
    __shared__ float m[256];
    double a = 0.0, b = 0.0, n = 0.0;
    float mm = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) {
        a += (double)partial[4 * i];
        b += (double)partial[4 * i + 1];
        mm = fmaxf(mm, partial[4 * i + 2]);
        n += (double)partial[4 * i + 3];
    }
    a = block_tree_sum(a, s);
    b = block_tree_sum(b, q);
    n = block_tree_sum(n, c);
    mm = block_tree_max(mm, m);
    if (threadIdx.x == 0) {
        const double sum = kind == KIND_MSE ? b : a;
        out[0] = n > 0.0 ? (float)(sum / n) : 0.f;
        out[1] = (float)n;
        out[2] = mm;
        out[3] = fmaxf(0.2f * mm, 1e-5f);
    }
}

// berHu, second pass: partial[i] = workgroup i's sum of |d| where |d| < c and of (d^2 + c^2) / 2 / c elsewhere.  A masked element holds
// d = 0 < c and adds 0.
__global__ void __launch_bounds__(256) reg_berhu_kernel(const float* __restrict__ diff, const float* __restrict__ out,
                                                       float* __restrict__ partial, long long n) {
    __shared__ float sh[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float c = out[3];
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = diff[i], a = fabsf(d);
        s += a < c ? a : (d * d + c * c) / 2.f / c;
    }
    s = wave_sum(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = join4_sum(sh);
}

__global__ void __launch_bounds__(256) reg_berhu_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ out) {
    __shared__ double s[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) a += (double)partial[i];
    a = block_tree_sum(a, s);
    if (threadIdx.x == 0) out[0] = out[1] > 0.f ? (float)(a / (double)out[1]) : 0.f;
}

// d(loss sum) / d(difference): L1 sign(d) with sign(0) = 0 (torch's abs gradient), MSE 2 d, berHu sign(d) inside |d| < c and d / c
// outside (c is a constant: the reference forms it under no_grad)
template <int KIND>
__device__ __forceinline__ float g_of(float d, float c) {
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    if (KIND == KIND_L1) return sg;
    if (KIND == KIND_MSE) return 2.f * d;
    return fabsf(d) < c ? sg : d / c;
}

// dx[b][iy][ix][k] = (up / count) sum over the output pixels whose window reaches (iy, ix) of weight g(diff): oy ascending, within a
// row ox ascending, the row sum then weighted -- resize_bwd_kernel's order.  One thread per (b, iy, ix, k < K), the only writer of its
// element; the thread of k = K - 1 also writes the zeros of columns K .. ldx - 1.  A masked element holds d = 0 and g(0) = 0.
template <int BILINEAR, int KIND>
__global__ void __launch_bounds__(256) reg_bwd_kernel(const float* __restrict__ diff, const float* __restrict__ out,
                                                     const float* __restrict__ up, float* __restrict__ dx, long long ldx, int h, int w,
                                                     int K, int H, int W, float sy, float sx, long long total) {
    const float count = out[1], c = out[3];
    const float scale = count > 0.f ? up[0] / count : 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int k = (int)(i % K);
        const long long p = i / K;                               // low-resolution pixel (b, iy, ix)
        const int ix = (int)(p % w);
        const long long q = p / w;
        const int iy = (int)(q % h);
        const long long b = q / h;
        const float* gb = diff + (b * K + k) * (long long)H * W;
        const float acc = resize_gather<BILINEAR>(gb, iy, ix, h, w, H, W, sy, sx, [c](float d) { return g_of<KIND>(d, c); });
        float* o = dx + p * ldx;
        o[k] = acc * scale;
        if (k == K - 1)
            for (int j = K; j < ldx; ++j) o[j] = 0.f;
    }
}

// The eight sums of masked_nyu_metrics (run_finetuning_depth.py:86-117) over the valid pixels, K = 1: with p = z std + mean and
// t = target std + mean (a product and a sum, each rounded, as torch evaluates them), tc = max(t, 1e-6), pc = max(p, 1e-6):
//   n, sum |p - t|^2, sum |p - t| / tc, sum |p - t|^2 / tc, sum (log pc - log tc)^2, and the counts of max(p / tc, t / pc) below 1.25,
//   1.25^2, 1.25^3.  partial[8 i .. 8 i + 7]: workgroup i's sums, its waves added in wave order.
template <int BILINEAR>
__global__ void __launch_bounds__(256) depth_metrics_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ target,
                                                           const unsigned char* __restrict__ mask, float mean, float std,
                                                           float* __restrict__ partial, int h, int w, int H, int W, float sy, float sx,
                                                           long long total) {
    __shared__ float sh[8 * WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (mask != nullptr && mask[i] == 0) continue;
        const int ox = (int)(i % W);
        const long long t = i / W;
        const int oy = (int)(t % H);
        const long long b = t / H;
        const Taps<BILINEAR> tp(b, oy, ox, h, w, ldx, sy, sx);
        const float z = tp.at(x, 0);
        {
#pragma clang fp contract(off)
            const float p = z * std + mean, tg = target[i] * std + mean;
            const float tc = fmaxf(tg, 1e-6f), pc = fmaxf(p, 1e-6f);
            const float d = fabsf(p - tg), d2 = d * d;
            const float lg = logf(pc) - logf(tc);
            const float r = fmaxf(p / tc, tg / pc);
            a[0] += 1.f;
            a[1] += d2;
            a[2] += d / tc;
            a[3] += d2 / tc;
            a[4] += lg * lg;
            a[5] += r < 1.25f ? 1.f : 0.f;
            a[6] += r < 1.5625f ? 1.f : 0.f;
            a[7] += r < 1.953125f ? 1.f : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = wave_sum(a[j]);
        if (lane == 0) sh[j * WAVES + wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) partial[8 * (long long)blockIdx.x + threadIdx.x] = join4_sum(sh + threadIdx.x * WAVES);
}

// out[7] = rmse, rel, srel, log10 (the natural log, as the reference's key), delta_1, delta_2, delta_3 from the partials summed in
// double; n = 0 gives NaN as the reference's 0 / 0 does.  acc, when given: acc[0..6] += out, acc[7] += 1 (one thread: no atomics).
__global__ void __launch_bounds__(256) depth_metrics_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ out,
                                                                  float* __restrict__ acc) {
    __shared__ double s[8][256];
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < nb; i += 256)
        for (int j = 0; j < 8; ++j) a[j] += (double)partial[8 * i + j];
    for (int j = 0; j < 8; ++j) a[j] = block_tree_sum(a[j], s[j]);
    if (threadIdx.x == 0) {
        const double n = a[0];
        out[0] = (float)sqrt(a[1] / n);
        out[1] = (float)(a[2] / n);
        out[2] = (float)(a[3] / n);
        out[3] = (float)sqrt(a[4] / n);
        out[4] = (float)(a[5] / n);
        out[5] = (float)(a[6] / n);
        out[6] = (float)(a[7] / n);
        if (acc != nullptr) {
            for (int j = 0; j < 7; ++j) acc[j] += out[j];
            acc[7] += 1.f;
        }
    }
}

// launch(std::integral_constant<int, KIND>) for the kind
template <class F>
void by_kind(int kind, F&& launch) {
    if (kind == KIND_L1) launch(std::integral_constant<int, KIND_L1>{});
    else if (kind == KIND_MSE) launch(std::integral_constant<int, KIND_MSE>{});
    else launch(std::integral_constant<int, KIND_BERHU>{});
}

}  // namespace

extern "C" int mmae_reg_loss_fwd(const float* x, int64_t ldx, const float* target, const void* mask, int mask_channels, int kind, int B, int h,
                                 int w, int K, int H, int W, int mode, float* diff, float* partial, float* out, void* stream) {
    MMAE_REQUIRE(x && target && diff && partial && out && resize_geom_ok(B, h, w, K, H, W, ldx, mode) && K <= MMAE_REG_MAX_K,
                 "reg_loss_fwd: bad argument (K <= 16)");
    MMAE_REQUIRE(kind >= KIND_L1 && kind <= KIND_BERHU, "reg_loss_fwd: kind is 0 (L1), 1 (MSE) or 2 (berHu)");
    MMAE_REQUIRE(mask == nullptr || mask_channels == 1 || mask_channels == K, "reg_loss_fwd: the mask has 1 or K channels");
    const ResizeScale sc(h, w, H, W);
    const long long total = (long long)B * H * W;
    const unsigned nb = grid_for(total, MMAE_REG_PARTIALS);
    hipStream_t st = (hipStream_t)stream;
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(reg_fwd_kernel<decltype(bl)::value>, dim3(nb), dim3(256), 0, st, x, (long long)ldx, target, (const unsigned char*)mask,
                           mask_channels, diff, partial, h, w, K, H, W, sc.sy, sc.sx, total);
    });
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb, kind, out);
    if (kind == KIND_BERHU) {
        const long long n = total * K;
        const unsigned nb2 = grid_for(n, MMAE_REG_PARTIALS);
        hipLaunchKernelGGL(reg_berhu_kernel, dim3(nb2), dim3(256), 0, st, (const float*)diff, (const float*)out, partial, n);
        hipLaunchKernelGGL(reg_berhu_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb2, out);
    }
    return mmae_check_launch("reg_loss_fwd");
}

extern "C" int mmae_reg_loss_bwd(const float* diff, const float* out, const float* up, int kind, int B, int h, int w, int K, int H, int W,
                                 int mode, float* dx, int64_t ldx, void* stream) {
    MMAE_REQUIRE(diff && out && up && dx && resize_geom_ok(B, h, w, K, H, W, ldx, mode) && K <= MMAE_REG_MAX_K,
                 "reg_loss_bwd: bad argument (K <= 16)");
    MMAE_REQUIRE(kind >= KIND_L1 && kind <= KIND_BERHU, "reg_loss_bwd: kind is 0 (L1), 1 (MSE) or 2 (berHu)");
    const ResizeScale sc(h, w, H, W);
    const long long total = (long long)B * h * w * K;
    by_mode(mode, [&](auto bl) {
        by_kind(kind, [&](auto kd) {
            hipLaunchKernelGGL((reg_bwd_kernel<decltype(bl)::value, decltype(kd)::value>), dim3(grid_for(total)), dim3(256), 0,
                               (hipStream_t)stream, diff, out, up, dx, (long long)ldx, h, w, K, H, W, sc.sy, sc.sx, total);
        });
    });
    return mmae_check_launch("reg_loss_bwd");
}

extern "C" int mmae_depth_metrics(const float* x, int64_t ldx, const float* target, const void* mask, float mean, float std, int B, int h, int w,
                                  int H, int W, int mode, float* partial, float* out, float* acc, void* stream) {
    MMAE_REQUIRE(x && target && partial && out && resize_geom_ok(B, h, w, 1, H, W, ldx, mode), "depth_metrics: bad argument");
    const ResizeScale sc(h, w, H, W);
    const long long total = (long long)B * H * W;
    const unsigned nb = grid_for(total, MMAE_REG_PARTIALS);
    hipStream_t st = (hipStream_t)stream;
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(depth_metrics_kernel<decltype(bl)::value>, dim3(nb), dim3(256), 0, st, x, (long long)ldx, target,
                           (const unsigned char*)mask, mean, std, partial, h, w, H, W, sc.sy, sc.sx, total);
    });
    hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb, out, acc);
    return mmae_check_launch("depth_metrics");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same losses and metrics on a prediction that IS the image: the DPT head's contiguous f32 NCHW [B][K][H][W] output (functions.
// ImageMark, functions.RegImageLossFn, metrics._depth_values).  No interpolation and no map: z = pred[e], element-wise streaming with
// the reductions, finish kernels and per-element expressions of the kernels above.
//   reg_img_fwd         diff[e] = mask ? pred[e] - target[e] : 0 and the four partials per workgroup; reg_finish_kernel; berHu's second
//                       pass over the stored difference and reg_berhu_finish_kernel
//   reg_img_bwd         dpred[e] = up / count * g(diff[e])
//   depth_metrics_img   the eight sums of depth_metrics_kernel over pred itself; depth_metrics_finish_kernel
// Work shape: HBM-bound, one thread per group of four consecutive elements with 16-byte accesses (the four mask bytes as one 32-bit
// word) when no group can straddle two planes (H W % 4 == 0) and every pointer is aligned for it, one thread per element otherwise;
// 64-bit element indices, grid-stride over at most MMAE_REG_PARTIALS workgroups.  Any K >= 1.
namespace {

inline bool img_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool img_al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// index of element e's mask byte: the mask's own element e when it has K channels (flat), else -- one channel broadcast over the K
// planes -- pixel e mod plane of image e / kp (kp = K plane elements per image).  small: every index fits 32 bits (cheaper divisions).
__device__ __forceinline__ long long img_mask_index(long long e, bool flat, long long plane, long long kp, bool small) {
    if (flat) return e;
    if (small) {
        const unsigned ue = (unsigned)e, b = ue / (unsigned)kp;
        return (long long)b * plane + (ue - b * (unsigned)kp) % (unsigned)plane;
    }
    const long long b = e / kp;
    return b * plane + (e - b * kp) % plane;
}

__device__ __forceinline__ void reg_img_term(float d, bool m, float& sa, float& sq, float& mx, int& cnt) {
    const float a = fabsf(d);
    sa += a;
    sq = __builtin_fmaf(d, d, sq);
    mx = fmaxf(mx, a);
    cnt += m ? 1 : 0;
}

// diff[e] = mask ? pred[e] - target[e] : 0 (a select: nothing under a false mask reaches the sums);  partial[4 i .. 4 i + 3] =
// workgroup i's sum |d|, sum d^2, max |d|, valid count.  groups = elements / VEC.
template <int VEC>
__global__ void __launch_bounds__(256) reg_img_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         const unsigned char* __restrict__ mask, int flat, long long plane, long long kp,
                                                         int small, float* __restrict__ diff, float* __restrict__ partial,
                                                         long long groups) {
    __shared__ float sh[4 * WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float sa = 0.f, sq = 0.f, mx = 0.f;
    int cnt = 0;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long e = g * VEC;
        if (VEC == 4) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(pred + e), tv = *reinterpret_cast<const f32x4*>(target + e);
            const unsigned mw = mask == nullptr ? 0x01010101u
                                                : *reinterpret_cast<const unsigned*>(mask + img_mask_index(e, flat != 0, plane, kp, small != 0));
            f32x4 dv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool m = ((mw >> (8 * j)) & 0xffu) != 0;
                const float d = m ? pv[j] - tv[j] : 0.f;
                dv[j] = d;
                reg_img_term(d, m, sa, sq, mx, cnt);
            }
            *reinterpret_cast<f32x4*>(diff + e) = dv;
        } else {
            const bool m = mask == nullptr || mask[img_mask_index(e, flat != 0, plane, kp, small != 0)] != 0;
            const float d = m ? pred[e] - target[e] : 0.f;
            diff[e] = d;
            reg_img_term(d, m, sa, sq, mx, cnt);
        }
    }
    sa = wave_sum(sa);
    sq = wave_sum(sq);
    mx = wave_max(mx);
    const float cf = wave_sum((float)cnt);                      // integers far below 2^24: exact
    if (lane == 0) { sh[wave] = sa; sh[WAVES + wave] = sq; sh[2 * WAVES + wave] = mx; sh[3 * WAVES + wave] = cf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = partial + 4 * (long long)blockIdx.x;
        p[0] = join4_sum(sh);
        p[1] = join4_sum(sh + WAVES);
        p[2] = join4_max(sh + 2 * WAVES);
        p[3] = join4_sum(sh + 3 * WAVES);
    }
}

// reg_berhu_kernel's sum with 16-byte reads of the stored difference
template <int VEC>
__global__ void __launch_bounds__(256) reg_img_berhu_kernel(const float* __restrict__ diff, const float* __restrict__ out,
                                                           float* __restrict__ partial, long long groups) {
    __shared__ float sh[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float c = out[3];
    float s = 0.f;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        float dv[VEC];
        if (VEC == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(diff + g * 4);
#pragma unroll
            for (int j = 0; j < VEC; ++j) dv[j] = v[j];
        } else {
            dv[0] = diff[g];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float d = dv[j], a = fabsf(d);
            s += a < c ? a : (d * d + c * c) / 2.f / c;
        }
    }
    s = wave_sum(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = join4_sum(sh);
}

// dpred[e] = (up / count) g(diff[e]); the scale formed as reg_bwd_kernel forms it (0 when nothing is valid).  A masked element holds
// d = 0 and g(0) = 0.
template <int VEC, int KIND>
__global__ void __launch_bounds__(256) reg_img_bwd_kernel(const float* __restrict__ diff, const float* __restrict__ out,
                                                         const float* __restrict__ up, float* __restrict__ dpred, long long groups) {
    const float count = out[1], c = out[3];
    const float scale = count > 0.f ? up[0] / count : 0.f;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        if (VEC == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(diff + g * 4);
            f32x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = g_of<KIND>(v[j], c) * scale;
            *reinterpret_cast<f32x4*>(dpred + g * 4) = r;
        } else {
            dpred[g] = g_of<KIND>(diff[g], c) * scale;
        }
    }
}

// one valid pixel's terms: depth_metrics_kernel's block with z = pred[e] (a product and a sum each rounded: no contraction)
__device__ __forceinline__ void depth_img_terms(float z, float t, float mean, float std, float (&a)[8]) {
#pragma clang fp contract(off)
    const float p = z * std + mean, tg = t * std + mean;
    const float tc = fmaxf(tg, 1e-6f), pc = fmaxf(p, 1e-6f);
    const float d = fabsf(p - tg), d2 = d * d;
    const float lg = logf(pc) - logf(tc);
    const float r = fmaxf(p / tc, tg / pc);
    a[0] += 1.f;
    a[1] += d2;
    a[2] += d / tc;
    a[3] += d2 / tc;
    a[4] += lg * lg;
    a[5] += r < 1.25f ? 1.f : 0.f;
    a[6] += r < 1.5625f ? 1.f : 0.f;
    a[7] += r < 1.953125f ? 1.f : 0.f;
}

// partial[8 i .. 8 i + 7]: workgroup i's eight sums over its valid pixels (K = 1: the mask is the image's shape); an invalid pixel
// is never evaluated
template <int VEC>
__global__ void __launch_bounds__(256) depth_metrics_img_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                               const unsigned char* __restrict__ mask, float mean, float std,
                                                               float* __restrict__ partial, long long groups) {
    __shared__ float sh[8 * WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long e = g * VEC;
        if (VEC == 4) {
            const unsigned mw = mask == nullptr ? 0x01010101u : *reinterpret_cast<const unsigned*>(mask + e);
            if (mw == 0) continue;
            const f32x4 pv = *reinterpret_cast<const f32x4*>(pred + e), tv = *reinterpret_cast<const f32x4*>(target + e);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((mw >> (8 * j)) & 0xffu) != 0) depth_img_terms(pv[j], tv[j], mean, std, a);
        } else {
            if (mask != nullptr && mask[e] == 0) continue;
            depth_img_terms(pred[e], target[e], mean, std, a);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = wave_sum(a[j]);
        if (lane == 0) sh[j * WAVES + wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) partial[8 * (long long)blockIdx.x + threadIdx.x] = join4_sum(sh + threadIdx.x * WAVES);
}

}  // namespace

extern "C" int mmae_reg_img_fwd(const float* pred, const float* target, const void* mask, int mask_channels, int kind, int B, int K, int H,
                                int W, float* diff, float* partial, float* out, void* stream) {
    MMAE_REQUIRE(pred && target && diff && partial && out, "reg_img_fwd: pred, target, diff, partial and out must not be NULL");
    MMAE_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "reg_img_fwd: B, K, H and W must be positive");
    MMAE_REQUIRE(kind >= KIND_L1 && kind <= KIND_BERHU, "reg_img_fwd: kind is 0 (L1), 1 (MSE) or 2 (berHu)");
    MMAE_REQUIRE(mask == nullptr || mask_channels == 1 || mask_channels == K, "reg_img_fwd: the mask has 1 or K channels");
    const long long plane = (long long)H * W, kp = plane * K, n = kp * B;
    const int flat = mask == nullptr || mask_channels == K, small = n <= 0xffffffffLL;
    const bool vec = plane % 4 == 0 && img_al16(pred) && img_al16(target) && img_al16(diff) && img_al4(mask);
    const long long groups = vec ? n / 4 : n;
    const unsigned nb = grid_for(groups, MMAE_REG_PARTIALS);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(reg_img_fwd_kernel<4>, dim3(nb), dim3(256), 0, st, pred, target, (const unsigned char*)mask, flat, plane, kp, small,
                           diff, partial, groups);
    else
        hipLaunchKernelGGL(reg_img_fwd_kernel<1>, dim3(nb), dim3(256), 0, st, pred, target, (const unsigned char*)mask, flat, plane, kp, small,
                           diff, partial, groups);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb, kind, out);
    if (kind == KIND_BERHU) {
        const bool vec2 = n % 4 == 0 && img_al16(diff);
        const long long groups2 = vec2 ? n / 4 : n;
        const unsigned nb2 = grid_for(groups2, MMAE_REG_PARTIALS);
        if (vec2) hipLaunchKernelGGL(reg_img_berhu_kernel<4>, dim3(nb2), dim3(256), 0, st, (const float*)diff, (const float*)out, partial, groups2);
        else hipLaunchKernelGGL(reg_img_berhu_kernel<1>, dim3(nb2), dim3(256), 0, st, (const float*)diff, (const float*)out, partial, groups2);
        hipLaunchKernelGGL(reg_berhu_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb2, out);
    }
    return mmae_check_launch("reg_img_fwd");
}

extern "C" int mmae_reg_img_bwd(const float* diff, const float* out, const float* up, int kind, int64_t n, float* dpred, void* stream) {
    MMAE_REQUIRE(diff && out && up && dpred, "reg_img_bwd: diff, out, up and dpred must not be NULL");
    MMAE_REQUIRE(n > 0, "reg_img_bwd: n must be positive");
    MMAE_REQUIRE(kind >= KIND_L1 && kind <= KIND_BERHU, "reg_img_bwd: kind is 0 (L1), 1 (MSE) or 2 (berHu)");
    const bool vec = n % 4 == 0 && img_al16(diff) && img_al16(dpred);
    const long long groups = vec ? n / 4 : n;
    by_kind(kind, [&](auto kd) {
        if (vec)
            hipLaunchKernelGGL((reg_img_bwd_kernel<4, decltype(kd)::value>), dim3(grid_for(groups)), dim3(256), 0, (hipStream_t)stream, diff, out,
                               up, dpred, groups);
        else
            hipLaunchKernelGGL((reg_img_bwd_kernel<1, decltype(kd)::value>), dim3(grid_for(groups)), dim3(256), 0, (hipStream_t)stream, diff, out,
                               up, dpred, groups);
    });
    return mmae_check_launch("reg_img_bwd");
}

extern "C" int mmae_depth_metrics_img(const float* pred, const float* target, const void* mask, float mean, float std, int B, int H, int W,
                                      float* partial, float* out, float* acc, void* stream) {
    MMAE_REQUIRE(pred && target && partial && out, "depth_metrics_img: pred, target, partial and out must not be NULL");
    MMAE_REQUIRE(B > 0 && H > 0 && W > 0, "depth_metrics_img: B, H and W must be positive");
    const long long n = (long long)B * H * W;
    const bool vec = n % 4 == 0 && img_al16(pred) && img_al16(target) && img_al4(mask);
    const long long groups = vec ? n / 4 : n;
    const unsigned nb = grid_for(groups, MMAE_REG_PARTIALS);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(depth_metrics_img_kernel<4>, dim3(nb), dim3(256), 0, st, pred, target, (const unsigned char*)mask, mean, std, partial,
                           groups);
    else
        hipLaunchKernelGGL(depth_metrics_img_kernel<1>, dim3(nb), dim3(256), 0, st, pred, target, (const unsigned char*)mask, mean, std, partial,
                           groups);
    hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb, out, acc);
    return mmae_check_launch("depth_metrics_img");
}
