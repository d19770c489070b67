// Dense regression losses and the NYU depth metrics on the ConvNeXt head's LOW-RESOLUTION map (functions.SegHandle,
// criterion.masked_l1_loss / masked_mse_loss / masked_berhu_loss, metrics.depth_metrics): the (B, K, H, W) image F.interpolate would
// write is never read.
//   reg_loss_fwd    masked L1 / MSE / berHu of the interpolated prediction against target f32 [B][K][H][W]: the masked difference is
//                   stored, per-workgroup partials (sum |d|, sum d^2, max |d|, valid count) are reduced in double by a finish kernel;
//                   berHu takes a second pass over the stored difference once c = max(0.2 max|d|, 1e-5) is known
//   reg_loss_bwd    the gradient with respect to the low-resolution map: the gather form of resize_bwd_kernel over g(d)
//   depth_metrics   the eight sums behind rmse, rel, srel, log10, delta_1..3 in one pass, the ratios in a finish kernel
// The interpolation uses the index math of csrc/convnext.hip (src_bilinear / src_nearest / first_dst) and combines the four taps with
// the function resize_fwd_kernel calls (common.h resize_tap4: every rounding written out), so the value the loss sees is the pixel
// mmae_resize_fwd would store (tests/test_reg_loss_gpu.py checks the bits).
//
// Work shape: K is 1 (depth) or 3 (normals, rgb), so pixels, not channels, lie on the lanes: one thread per output pixel, lanes along
// ox (coalesced target / mask / difference accesses; the low-resolution rows come from cache), a short loop over k <= MMAE_REG_MAX_K.
// In-wave reductions by wave64 shuffles, LDS only to join the four waves in wave order, no float atomics: run-to-run results are
// bit-equal.  Columns K .. ldx - 1 of the map are never read.
#include "common.h"
#include <math.h>

namespace {

// ---- index math of csrc/convnext.hip (its source coordinate's product and sum contract to one FMA: spelled out here) ------------
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

// the four waves' values joined in wave order by thread 0 (sh: WAVES floats per quantity)
__device__ __forceinline__ float join_sum(const float* sh) { return ((sh[0] + sh[1]) + sh[2]) + sh[3]; }

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
        p[0] = join_sum(sh);
        p[1] = join_sum(sh + WAVES);
        p[2] = fmaxf(fmaxf(sh[2 * WAVES], sh[2 * WAVES + 1]), fmaxf(sh[2 * WAVES + 2], sh[2 * WAVES + 3]));
        p[3] = join_sum(sh + 3 * WAVES);
    }
}

// a fixed tree over 256 doubles held in LDS; the result in s[0]
__device__ __forceinline__ void tree_sum(double* s) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
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
    s[threadIdx.x] = a;
    q[threadIdx.x] = b;
    c[threadIdx.x] = n;
    m[threadIdx.x] = mm;
    tree_sum(s);
    tree_sum(q);
    tree_sum(c);
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) m[threadIdx.x] = fmaxf(m[threadIdx.x], m[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double sum = kind == KIND_MSE ? q[0] : s[0];
        out[0] = c[0] > 0.0 ? (float)(sum / c[0]) : 0.f;
        out[1] = (float)c[0];
        out[2] = m[0];
        out[3] = fmaxf(0.2f * m[0], 1e-5f);
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
    if (threadIdx.x == 0) partial[blockIdx.x] = join_sum(sh);
}

__global__ void __launch_bounds__(256) reg_berhu_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ out) {
    __shared__ double s[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) a += (double)partial[i];
    s[threadIdx.x] = a;
    tree_sum(s);
    if (threadIdx.x == 0) out[0] = out[1] > 0.f ? (float)(s[0] / (double)out[1]) : 0.f;
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
                    rs = __builtin_fmaf(wx, g_of<KIND>(gr[ox], c), rs);
                } else {
                    if (src_nearest(ox, sx, w) > ix) break;
                    rs += g_of<KIND>(gr[ox], c);
                }
            }
            acc = BILINEAR ? __builtin_fmaf(wy, rs, acc) : acc + rs;
        }
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
    if (threadIdx.x < 8) partial[8 * (long long)blockIdx.x + threadIdx.x] = join_sum(sh + threadIdx.x * WAVES);
}

// out[7] = rmse, rel, srel, log10 (the natural log, as the reference's key), delta_1, delta_2, delta_3 from the partials summed in
// double; n = 0 gives NaN as the reference's 0 / 0 does.  acc, when given: acc[0..6] += out, acc[7] += 1 (one thread: no atomics).
__global__ void __launch_bounds__(256) depth_metrics_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ out,
                                                                  float* __restrict__ acc) {
    __shared__ double s[8][256];
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < nb; i += 256)
        for (int j = 0; j < 8; ++j) a[j] += (double)partial[8 * i + j];
    for (int j = 0; j < 8; ++j) s[j][threadIdx.x] = a[j];
    for (int j = 0; j < 8; ++j) tree_sum(s[j]);
    if (threadIdx.x == 0) {
        const double n = s[0][0];
        out[0] = (float)sqrt(s[1][0] / n);
        out[1] = (float)(s[2][0] / n);
        out[2] = (float)(s[3][0] / n);
        out[3] = (float)sqrt(s[4][0] / n);
        out[4] = (float)(s[5][0] / n);
        out[5] = (float)(s[6][0] / n);
        out[6] = (float)(s[7][0] / n);
        if (acc != nullptr) {
            for (int j = 0; j < 7; ++j) acc[j] += out[j];
            acc[7] += 1.f;
        }
    }
}

inline unsigned grid_for(long long total) {
    const long long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > MMAE_REG_PARTIALS ? MMAE_REG_PARTIALS : b));
}
inline bool geom_ok(int B, int h, int w, int K, int H, int W, int64_t ldx, int mode) {
    return B > 0 && h > 0 && w > 0 && K > 0 && K <= MMAE_REG_MAX_K && H > 0 && W > 0 && ldx >= K && (mode == 0 || mode == 1);
}

template <int BILINEAR>
void launch_bwd(int kind, unsigned nb, hipStream_t st, const float* diff, const float* out, const float* up, float* dx, long long ldx, int h,
                int w, int K, int H, int W, float sy, float sx, long long total) {
    if (kind == KIND_L1)
        hipLaunchKernelGGL((reg_bwd_kernel<BILINEAR, KIND_L1>), dim3(nb), dim3(256), 0, st, diff, out, up, dx, ldx, h, w, K, H, W, sy, sx, total);
    else if (kind == KIND_MSE)
        hipLaunchKernelGGL((reg_bwd_kernel<BILINEAR, KIND_MSE>), dim3(nb), dim3(256), 0, st, diff, out, up, dx, ldx, h, w, K, H, W, sy, sx, total);
    else
        hipLaunchKernelGGL((reg_bwd_kernel<BILINEAR, KIND_BERHU>), dim3(nb), dim3(256), 0, st, diff, out, up, dx, ldx, h, w, K, H, W, sy, sx,
                           total);
}

}  // namespace

extern "C" int mmae_reg_loss_fwd(const float* x, int64_t ldx, const float* target, const void* mask, int mask_channels, int kind, int B, int h,
                                 int w, int K, int H, int W, int mode, float* diff, float* partial, float* out, void* stream) {
    MMAE_REQUIRE(x && target && diff && partial && out && geom_ok(B, h, w, K, H, W, ldx, mode), "reg_loss_fwd: bad argument (K <= 16)");
    MMAE_REQUIRE(kind >= KIND_L1 && kind <= KIND_BERHU, "reg_loss_fwd: kind is 0 (L1), 1 (MSE) or 2 (berHu)");
    MMAE_REQUIRE(mask == nullptr || mask_channels == 1 || mask_channels == K, "reg_loss_fwd: the mask has 1 or K channels");
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const long long total = (long long)B * H * W;
    const unsigned nb = grid_for(total);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0)
        hipLaunchKernelGGL(reg_fwd_kernel<1>, dim3(nb), dim3(256), 0, st, x, (long long)ldx, target, (const unsigned char*)mask, mask_channels,
                           diff, partial, h, w, K, H, W, sy, sx, total);
    else
        hipLaunchKernelGGL(reg_fwd_kernel<0>, dim3(nb), dim3(256), 0, st, x, (long long)ldx, target, (const unsigned char*)mask, mask_channels,
                           diff, partial, h, w, K, H, W, sy, sx, total);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb, kind, out);
    if (kind == KIND_BERHU) {
        const long long n = total * K;
        const unsigned nb2 = grid_for(n);
        hipLaunchKernelGGL(reg_berhu_kernel, dim3(nb2), dim3(256), 0, st, (const float*)diff, (const float*)out, partial, n);
        hipLaunchKernelGGL(reg_berhu_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb2, out);
    }
    return mmae_check_launch("reg_loss_fwd");
}

extern "C" int mmae_reg_loss_bwd(const float* diff, const float* out, const float* up, int kind, int B, int h, int w, int K, int H, int W,
                                 int mode, float* dx, int64_t ldx, void* stream) {
    MMAE_REQUIRE(diff && out && up && dx && geom_ok(B, h, w, K, H, W, ldx, mode), "reg_loss_bwd: bad argument (K <= 16)");
    MMAE_REQUIRE(kind >= KIND_L1 && kind <= KIND_BERHU, "reg_loss_bwd: kind is 0 (L1), 1 (MSE) or 2 (berHu)");
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const long long total = (long long)B * h * w * K;
    const long long blocks = (total + 255) / 256;
    const unsigned nb = (unsigned)(blocks > 65536 ? 65536 : blocks);
    if (mode == 0)
        launch_bwd<1>(kind, nb, (hipStream_t)stream, diff, out, up, dx, (long long)ldx, h, w, K, H, W, sy, sx, total);
    else
        launch_bwd<0>(kind, nb, (hipStream_t)stream, diff, out, up, dx, (long long)ldx, h, w, K, H, W, sy, sx, total);
    return mmae_check_launch("reg_loss_bwd");
}

extern "C" int mmae_depth_metrics(const float* x, int64_t ldx, const float* target, const void* mask, float mean, float std, int B, int h, int w,
                                  int H, int W, int mode, float* partial, float* out, float* acc, void* stream) {
    MMAE_REQUIRE(x && target && partial && out && geom_ok(B, h, w, 1, H, W, ldx, mode), "depth_metrics: bad argument");
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    const long long total = (long long)B * H * W;
    const unsigned nb = grid_for(total);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0)
        hipLaunchKernelGGL(depth_metrics_kernel<1>, dim3(nb), dim3(256), 0, st, x, (long long)ldx, target, (const unsigned char*)mask, mean, std,
                           partial, h, w, H, W, sy, sx, total);
    else
        hipLaunchKernelGGL(depth_metrics_kernel<0>, dim3(nb), dim3(256), 0, st, x, (long long)ldx, target, (const unsigned char*)mask, mean, std,
                           partial, h, w, H, W, sy, sx, total);
    hipLaunchKernelGGL(depth_metrics_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)partial, (int)nb, out, acc);
    return mmae_check_launch("depth_metrics");
}
