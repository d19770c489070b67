// Semantic-segmentation loss and evaluation on the ConvNeXt head's LOW-RESOLUTION logits (functions.SegHandle, criterion.SegCrossEntropyLoss,
// metrics.py): the (B, K, H, W) image F.interpolate would write is never read.
//   seg_ce_fwd   nn.CrossEntropyLoss(ignore_index) of the interpolated logits: per-pixel log-sum-exp, fixed-order partial sums, sum / count
//   seg_ce_bwd   its gradient with respect to the low-resolution logits: the gather form of resize_bwd_kernel, softmax recomputed from lse
//   seg_argmax   argmax over the first n_cls interpolated logits (lowest index on ties)
//   seg_hist     the four histograms of the reference's intersect_and_union (utils/semseg_metrics.py:49-59), added into an int64 buffer.
//                np.histogram's closed last bin would count a value exactly equal to K into class K - 1; that quirk is NOT reproduced:
//                a prediction or label outside [0, K) is dropped.
// The interpolation takes its taps and weights from resize_map.h, the functions resize_fwd_kernel calls.  It combines the four taps
// with its own tap4 below, which is left to the compiler's contraction, NOT with common.h's resize_tap4 as that kernel does: an
// interpolated logit lies within test_resize_fwd's bound of the pixel mmae_resize_fwd would store, not on its bits.  What is
// guaranteed and tested (tests/test_seg_loss_gpu.py) is that seg_argmax agrees with the argmax of the written image.  Calling
// resize_tap4 here would move lse, loss and gradient by ulps: a change of behaviour, not done in passing.
// A target outside [0, K) that is not ignore_index counts as ignored (csrc/losses.hip; torch raises a device assert).
//
// Work shape: one wave per output pixel (forward, argmax) or per low-resolution pixel and 64-class chunk (backward), lanes over classes,
// so every logit row is read as coalesced 256-byte segments and a lane owns its accumulator.  No float atomics, no LDS accumulators:
// run-to-run results are bit-equal.  The low-resolution logits (39 MB at the ADE20K geometry) stay in the L2 / Infinity Cache.
#include "resize_map.h"

namespace {

// the four taps (a, b: row i0 at columns i0, i1; c, d: row i1) in resize_fwd_kernel's form, its roundings left to the compiler
__device__ __forceinline__ float tap4(const Src& ry, const Src& rx, float a, float b, float c, float d) {
    return ry.l0 * (rx.l0 * a + rx.l1 * b) + ry.l1 * (rx.l0 * c + rx.l1 * d);
}

constexpr int WAVES = 4;                      // waves per workgroup (256 threads)
constexpr int RUN = 8;                        // consecutive output pixels of one row per wave task (forward, argmax)

// The source of one output pixel: the two logit rows and the column taps.  Everything in it is wave-uniform.
template <int BILINEAR>
struct Taps {
    const float *r0, *r1;
    Src ry, rx;
    long long c0, c1;
    __device__ __forceinline__ void row(const float* xb, long long ldx, int oy, int h, int w, float sy) {
        if (BILINEAR) {
            ry = src_bilinear(oy, sy, h);
            r0 = xb + (long long)ry.i0 * w * ldx;
            r1 = xb + (long long)ry.i1 * w * ldx;
        } else {
            r0 = r1 = xb + (long long)src_nearest(oy, sy, h) * w * ldx;
        }
    }
    __device__ __forceinline__ void col(long long ldx, int ox, int w, float sx) {
        if (BILINEAR) {
            rx = src_bilinear(ox, sx, w);
            c0 = rx.i0 * ldx;
            c1 = rx.i1 * ldx;
        } else {
            c0 = c1 = src_nearest(ox, sx, w) * ldx;
        }
    }
    __device__ __forceinline__ float at(int k) const {
        if (BILINEAR) return tap4(ry, rx, r0[c0 + k], r0[c1 + k], r1[c0 + k], r1[c1 + k]);
        return r0[c0 + k];
    }
};

// task -> (b, oy, first ox) of a run of RUN output pixels
__device__ __forceinline__ void run_of(long long t, int H, int W, long long& b, int& oy, int& ox0) {
    const int Wr = (W + RUN - 1) / RUN;
    ox0 = (int)(t % Wr) * RUN;
    t /= Wr;
    oy = (int)(t % H);
    b = t / H;
}

// lse[b][oy][ox] = log sum_k exp z_k and the wave's share of sum (lse - z[target]) and of the valid-pixel count.  A lane keeps a
// running maximum and rescaled sum over its classes k = lane, lane + 64, ...; the 64 pairs are merged once per pixel.
// partial[2 i], partial[2 i + 1]: sum and count of workgroup i, its waves added in wave order.
template <int BILINEAR>
__global__ void __launch_bounds__(256) seg_ce_fwd_kernel(const float* __restrict__ x, long long ldx, const long long* __restrict__ target,
                                                        long long ignore, float* __restrict__ lse, float* __restrict__ partial, int h, int w,
                                                        int K, int H, int W, float sy, float sx, long long tasks) {
    __shared__ float sh[2 * WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float sum = 0.f, cnt = 0.f;
    for (long long t = (long long)blockIdx.x * WAVES + wave; t < tasks; t += (long long)gridDim.x * WAVES) {
        long long b;
        int oy, ox0;
        run_of(t, H, W, b, oy, ox0);
        Taps<BILINEAR> tp;
        tp.row(x + b * h * w * ldx, ldx, oy, h, w, sy);
        const long long po = (b * H + oy) * (long long)W;
        const int ox1 = ox0 + RUN < W ? ox0 + RUN : W;
        for (int ox = ox0; ox < ox1; ++ox) {
            tp.col(ldx, ox, w, sx);
            float m = -INFINITY, s = 0.f;
            for (int k = lane; k < K; k += 64) {
                const float z = tp.at(k);
                const float mn = fmaxf(m, z);
                s = s * __expf(m - mn) + __expf(z - mn);        // exp2(d log2 e): one v_exp_f32 each
                m = mn;
            }
            const float M = wave_max(m);
            const float S = wave_sum(s * __expf(m - M));          // a lane without a class: 0 * exp(-inf) = 0
            const float l = M + logf(S);
            if (lane == 0) lse[po + ox] = l;
            const long long tg = target[po + ox];
            if (tg >= 0 && tg < K && tg != ignore) {
                sum += l - tp.at((int)tg);
                cnt += 1.f;
            }
        }
    }
    if (lane == 0) { sh[wave] = sum; sh[WAVES + wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = join4_sum(sh);
        partial[2 * blockIdx.x + 1] = join4_sum(sh + WAVES);
    }
}

// out[0] = sum / count (0 when no pixel is valid), out[1] = count: the partials in a fixed tree, in double (counts are integers: exact)
__global__ void __launch_bounds__(256) seg_ce_finish_kernel(const float* __restrict__ partial, int nb, float* __restrict__ out) {
    __shared__ double s[256], c[256];
    double a = 0.0, n = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += (double)partial[2 * i]; n += (double)partial[2 * i + 1]; }
    a = block_tree_sum(a, s);
    n = block_tree_sum(n, c);
    if (threadIdx.x == 0) {
        out[0] = n > 0.0 ? (float)(a / n) : 0.f;
        out[1] = (float)n;
    }
}

// dx[b][iy][ix][k] = (up / count) sum over the valid output pixels whose window reaches (iy, ix) of weight (exp(z_k - lse) - [k == target]):
// oy ascending, within a row ox ascending, the row sum then weighted -- resize_bwd_kernel's order.  One wave per (low-resolution pixel,
// chunk of 64 columns); a lane holds the 3 x 3 neighbourhood of its class in registers (every window tap is one of the nine) and is the
// only writer of its element.  What is the same for all classes of an output pixel -- its column taps, target and lse -- is worked out
// once per row for up to 64 columns at a time, lane j taking column ox0 + j (coalesced target / lse loads), and read back with
// v_readlane in the loop over the columns.  p = exp2((z - lse) log2 e) (__expf: one v_exp_f32).  Columns K .. ldx - 1 are written as zeros.
__device__ __forceinline__ float lane_f(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

template <int BILINEAR>
__global__ void __launch_bounds__(256) seg_ce_bwd_kernel(const float* __restrict__ x, long long ldx, const long long* __restrict__ target,
                                                        long long ignore, const float* __restrict__ lse, const float* __restrict__ out,
                                                        const float* __restrict__ up, float* __restrict__ dx, int h, int w, int K, int H, int W,
                                                        float sy, float sx, int nch, long long tasks) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const float count = out[1];
    const float scale = count > 0.f ? up[0] / count : 0.f;
    for (long long t = (long long)blockIdx.x * WAVES + wave; t < tasks; t += (long long)gridDim.x * WAVES) {
        const int k = (int)(t % nch) * 64 + lane;
        const long long p = t / nch;                             // low-resolution pixel (b, iy, ix)
        const int ix = (int)(p % w);
        const long long q = p / w;
        const int iy = (int)(q % h);
        const long long b = q / h;
        const bool mine = k < K;                                 // every lane walks the window (the column data lives in lanes)
        const float* xb = x + b * h * w * ldx + (mine ? k : 0);
        float R[3][3];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int dxx = 0; dxx < 3; ++dxx) {
                if (!BILINEAR && (dy != 1 || dxx != 1)) { R[dy][dxx] = 0.f; continue; }
                int yy = iy + dy - 1, xx = ix + dxx - 1;
                yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
                xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
                R[dy][dxx] = xb[((long long)yy * w + xx) * ldx];
            }
        }
        const int oy0 = first_dst<BILINEAR>(iy, sy, h, H), ox0 = first_dst<BILINEAR>(ix, sx, w, W);
        const long long pb = b * H * (long long)W;
        float acc = 0.f;
        for (int oy = oy0; oy < H; ++oy) {
            Src ry = {0, 0, 0.f, 0.f};
            float wy = 1.f, T[3], Bt[3];
            if (BILINEAR) {
                ry = src_bilinear(oy, sy, h);
                if (ry.i0 > iy) break;
                wy = (ry.i0 == iy ? ry.l0 : 0.f) + (ry.i1 == iy ? ry.l1 : 0.f);
#pragma unroll
                for (int j = 0; j < 3; ++j) {                    // row i0 is iy - 1 or iy, row i1 is iy or iy + 1
                    T[j] = ry.i0 == iy ? R[1][j] : R[0][j];
                    Bt[j] = ry.i1 == iy ? R[1][j] : R[2][j];
                }
            } else {
                if (src_nearest(oy, sy, h) > iy) break;
            }
            const long long po = pb + (long long)oy * W;
            float rs = 0.f;
            for (int c0 = ox0; c0 < W; c0 += 64) {
                // lane j: column c0 + j.  `in`: the column exists and its window still reaches ix -- a prefix of the lanes.
                const int ox = c0 + lane;
                const int oxc = ox < W ? ox : W - 1;
                Src rx = {0, 0, 0.f, 0.f};
                float wx = 1.f;
                bool in;
                if (BILINEAR) {
                    rx = src_bilinear(oxc, sx, w);
                    in = ox < W && rx.i0 <= ix;
                    wx = (rx.i0 == ix ? rx.l0 : 0.f) + (rx.i1 == ix ? rx.l1 : 0.f);
                } else {
                    in = ox < W && src_nearest(oxc, sx, w) <= ix;
                }
                const long long tg = in ? target[po + ox] : -1;
                const float ls = in ? lse[po + ox] : 0.f;
                const bool ok = in && tg >= 0 && tg < K && tg != ignore;
                const int flags = (rx.i0 == ix ? 1 : 0) | (rx.i1 == ix ? 2 : 0) | (ok ? 4 : 0);
                const int tgi = ok ? (int)tg : -1;
                const unsigned long long m = __ballot(in);
                const int n = m == ~0ull ? 64 : __builtin_ctzll(~m);
                for (int j = 0; j < n; ++j) {
                    const int f = __builtin_amdgcn_readlane(flags, j);
                    if (!(f & 4)) continue;                      // not a valid pixel: no term
                    float z;
                    if (BILINEAR) {
                        Src cx = {0, 0, lane_f(rx.l0, j), lane_f(rx.l1, j)};
                        z = tap4(ry, cx, (f & 1) ? T[1] : T[0], (f & 2) ? T[1] : T[2], (f & 1) ? Bt[1] : Bt[0], (f & 2) ? Bt[1] : Bt[2]);
                    } else {
                        z = R[1][1];
                    }
                    const float g = __expf(z - lane_f(ls, j)) - (k == __builtin_amdgcn_readlane(tgi, j) ? 1.f : 0.f);
                    rs = BILINEAR ? __builtin_fmaf(lane_f(wx, j), g, rs) : rs + g;
                }
                if (n < 64) break;
            }
            acc = BILINEAR ? __builtin_fmaf(wy, rs, acc) : acc + rs;
        }
        if (k < ldx) dx[p * ldx + k] = mine ? acc * scale : 0.f;
    }
}

// pred[b][oy][ox] = argmax over k < n_cls of the interpolated logits; the lowest index wins a tie (within a lane: strict >; across lanes:
// the smaller index of equal values)
template <int BILINEAR>
__global__ void __launch_bounds__(256) seg_argmax_kernel(const float* __restrict__ x, long long ldx, long long* __restrict__ pred, int h, int w,
                                                        int n_cls, int H, int W, float sy, float sx, long long tasks) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (long long t = (long long)blockIdx.x * WAVES + wave; t < tasks; t += (long long)gridDim.x * WAVES) {
        long long b;
        int oy, ox0;
        run_of(t, H, W, b, oy, ox0);
        Taps<BILINEAR> tp;
        tp.row(x + b * h * w * ldx, ldx, oy, h, w, sy);
        const long long po = (b * H + oy) * (long long)W;
        const int ox1 = ox0 + RUN < W ? ox0 + RUN : W;
        for (int ox = ox0; ox < ox1; ++ox) {
            tp.col(ldx, ox, w, sx);
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int k = lane; k < n_cls; k += 64) {
                const float z = tp.at(k);
                if (z > bv || bi == 0x7fffffff) { bv = z; bi = k; }
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const float ov = __shfl_xor(bv, s, 64);
                const int oi = __shfl_xor(bi, s, 64);
                if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (lane == 0) pred[po + ox] = (long long)bi;
        }
    }
}

// hist[0..3][K] += (intersection, union, prediction, label) counts over the pixels with label != ignore: per-workgroup LDS counters
// (intersection, prediction, label; union = prediction + label - intersection), then 64-bit integer adds to global memory.  Counts are
// exact, so the order of the adds does not matter.
__global__ void __launch_bounds__(256) seg_hist_kernel(const long long* __restrict__ pred, const long long* __restrict__ label, long long n,
                                                      int K, long long ignore, unsigned long long* __restrict__ hist) {
    extern __shared__ int cnt[];                                // [3][K]
    for (int i = threadIdx.x; i < 3 * K; i += 256) cnt[i] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long l = label[i];
        if (l == ignore) continue;
        const long long p = pred[i];
        const bool pin = p >= 0 && p < K, lin = l >= 0 && l < K;
        if (pin) atomicAdd(&cnt[K + (int)p], 1);
        if (lin) atomicAdd(&cnt[2 * K + (int)l], 1);
        if (pin && p == l) atomicAdd(&cnt[(int)p], 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const int ci = cnt[k], cp = cnt[K + k], cl = cnt[2 * K + k];
        if (ci) atomicAdd(hist + k, (unsigned long long)ci);
        if (cp + cl - ci) atomicAdd(hist + K + k, (unsigned long long)(cp + cl - ci));
        if (cp) atomicAdd(hist + 2 * K + k, (unsigned long long)cp);
        if (cl) atomicAdd(hist + 3 * K + k, (unsigned long long)cl);
    }
}

}  // namespace

extern "C" int mmae_seg_ce_fwd(const float* x, int64_t ldx, const int64_t* target, int64_t ignore_index, int B, int h, int w, int K, int H, int W,
                               int mode, float* lse, float* partial, float* out, void* stream) {
    MMAE_REQUIRE(x && target && lse && partial && out && resize_geom_ok(B, h, w, K, H, W, ldx, mode), "seg_ce_fwd: bad argument");
    const ResizeScale sc(h, w, H, W);
    const long long tasks = (long long)B * H * ((W + RUN - 1) / RUN);
    const unsigned nb = grid_for(tasks, MMAE_SEG_PARTIALS, WAVES);
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(seg_ce_fwd_kernel<decltype(bl)::value>, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, (long long)ldx,
                           (const long long*)target, (long long)ignore_index, lse, partial, h, w, K, H, W, sc.sy, sc.sx, tasks);
    });
    hipLaunchKernelGGL(seg_ce_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, (int)nb, out);
    return mmae_check_launch("seg_ce_fwd");
}

extern "C" int mmae_seg_ce_bwd(const float* x, int64_t ldx, const int64_t* target, int64_t ignore_index, int B, int h, int w, int K, int H, int W,
                               int mode, const float* lse, const float* out, const float* up, float* dx, void* stream) {
    MMAE_REQUIRE(x && target && lse && out && up && dx && resize_geom_ok(B, h, w, K, H, W, ldx, mode), "seg_ce_bwd: bad argument");
    const ResizeScale sc(h, w, H, W);
    const int nch = (int)((ldx + 63) / 64);
    const long long tasks = (long long)B * h * w * nch;
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(seg_ce_bwd_kernel<decltype(bl)::value>, dim3(grid_for(tasks, 65536, WAVES)), dim3(256), 0, (hipStream_t)stream, x,
                           (long long)ldx, (const long long*)target, (long long)ignore_index, lse, out, up, dx, h, w, K, H, W, sc.sy, sc.sx, nch,
                           tasks);
    });
    return mmae_check_launch("seg_ce_bwd");
}

extern "C" int mmae_seg_argmax(const float* x, int64_t ldx, int B, int h, int w, int K, int n_cls, int H, int W, int mode, int64_t* pred,
                               void* stream) {
    MMAE_REQUIRE(x && pred && resize_geom_ok(B, h, w, K, H, W, ldx, mode) && n_cls > 0 && n_cls <= K, "seg_argmax: bad argument");
    const ResizeScale sc(h, w, H, W);
    const long long tasks = (long long)B * H * ((W + RUN - 1) / RUN);
    by_mode(mode, [&](auto bl) {
        hipLaunchKernelGGL(seg_argmax_kernel<decltype(bl)::value>, dim3(grid_for(tasks, 65536, WAVES)), dim3(256), 0, (hipStream_t)stream, x,
                           (long long)ldx, (long long*)pred, h, w, n_cls, H, W, sc.sy, sc.sx, tasks);
    });
    return mmae_check_launch("seg_argmax");
}

extern "C" int mmae_seg_hist(const int64_t* pred, const int64_t* label, int64_t n, int K, int64_t ignore_index, int64_t* hist, void* stream) {
    MMAE_REQUIRE(pred && label && hist && n > 0 && K > 0 && K <= MMAE_SEG_HIST_MAX_K, "seg_hist: bad argument (K <= 4096)");
    const long long blocks = (n + 256 * 16 - 1) / (256 * 16);                  // >= 16 pixels per thread: few global adds per class
    const unsigned nb = (unsigned)(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks));
    hipLaunchKernelGGL(seg_hist_kernel, dim3(nb), dim3(256), (size_t)3 * K * sizeof(int), (hipStream_t)stream, (const long long*)pred,
                       (const long long*)label, (long long)n, K, (long long)ignore_index, (unsigned long long*)hist);
    return mmae_check_launch("seg_hist");
}
