// The classification fine-tuning recipe of run_finetuning_cls.py (multimae_amd/mixup.py, criterion.py, ema.py):
//   mixup_pairs   Mixup._mix_batch / _mix_pair / _mix_elem (utils/mixup.py:166-214) on the batch in place: one work item holds the same
//                 pixels of samples i and B - 1 - i, reads both originals and writes both results -- the reference's x_orig / x.flip(0)
//                 semantics without a clone, the batch read once and written once
//   mix_target    mixup_target (utils/mixup.py:23-33): the two smoothed one-hot rows and their blend, never materialised separately
//   soft_ce_fwd   SoftTargetCrossEntropy / LabelSmoothingCrossEntropy (utils/cross_entropy.py:17-43): one workgroup per row, log-sum-exp
//                 and sum_k t_k (lse - x_k) in two passes over the row (the second one hits the L2), the row losses summed in a fixed tree
//   soft_ce_bwd   its gradient, softmax recomputed from the saved lse
//   ema_update    ModelEma.update (utils/model_ema.py:72-83) over two flat arenas, optionally with the EMA arena's bf16 shadow
// mixup_pairs, mix_target and ema_update are BIT-IDENTICAL to the reference's eager f32 expressions: every product and every sum rounds
// on its own.  The whole file is compiled without FMA contraction -- the Makefile's -ffp-contract=off for this file (it also covers the
// header intrinsics, which are plain operators once inlined) and the pragma below; the loss kernels lose nothing by it.
// No float atomics: every reduction has a fixed order, results are bit-equal from run to run.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int MIX_BLEND = MMAE_MIX_BLEND, MIX_KEEP = MMAE_MIX_KEEP;

// one sample's row of the parameter block (mmae.h): 8 x 4 bytes
struct MixRow { float w_self, w_other, t_self, t_other; int yl, yh, xl, xh; };

__device__ __forceinline__ float blend(float a, float b, float ws, float wo) { return __fadd_rn(__fmul_rn(a, ws), __fmul_rn(b, wo)); }

// out = mix(self, other) for one pixel at (y, x) of a sample with row r (r.yl != MIX_KEEP)
__device__ __forceinline__ float mix1(const MixRow& r, float self, float other, int y, int x) {
    if (r.yl == MIX_BLEND) return blend(self, other, r.w_self, r.w_other);
    return (y >= r.yl && y < r.yh && x >= r.xl && x < r.xh) ? other : self;
}
// does the pixel run [x, x + n) of image row y need a write for a sample with row r?
__device__ __forceinline__ bool touches(const MixRow& r, int y, int x, int n) {
    if (r.yl == MIX_KEEP) return false;
    if (r.yl == MIX_BLEND) return true;
    return y >= r.yl && y < r.yh && x + n > r.xl && x < r.xh;
}

// grid.y: the pair (i, B - 1 - i); grid.x strides over the C H W elements of a sample, VEC at a time.  VEC == 4 needs W % 4 == 0 (a
// group never straddles two image rows) and a 16-byte aligned base.
template <int VEC>
__global__ void __launch_bounds__(256) mixup_pairs_kernel(float* __restrict__ x, const MixRow* __restrict__ rows, int B, unsigned chw,
                                                         unsigned H, unsigned W) {
    const int i = blockIdx.y, j = B - 1 - i;
    const MixRow ri = rows[i], rj = rows[j];
    if (ri.yl == MIX_KEEP && rj.yl == MIX_KEEP) return;
    float* xi = x + (long long)i * chw;
    float* xj = x + (long long)j * chw;
    const unsigned groups = chw / VEC;                            // chw < 2^31 (checked by the host): 32-bit index math
    for (unsigned g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        const unsigned e = g * VEC;
        const unsigned r = e / W;
        const int px = (int)(e - r * W);
        const int py = (int)(r % H);
        const bool wi = touches(ri, py, px, VEC), wj = touches(rj, py, px, VEC);
        if (!wi && !wj) continue;
        if (VEC == 4) {
            const f32x4 a = ld4(xi + e), b = ld4(xj + e);
            if (wi) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = mix1(ri, a[k], b[k], py, px + k);
                st4(xi + e, o);
            }
            if (wj) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = mix1(rj, b[k], a[k], py, px + k);
                st4(xj + e, o);
            }
        } else {
            const float a = xi[e], b = xj[e];
            if (wi) xi[e] = mix1(ri, a, b, py, px);
            if (wj) xj[e] = mix1(rj, b, a, py, px);
        }
    }
}

// target[i][k] = fl(fl(y1 t_self) + fl(y2 t_other)), y1 / y2 the smoothed one-hot rows of labels[i] / labels[B - 1 - i]
__global__ void __launch_bounds__(256) mix_target_kernel(const long long* __restrict__ labels, const MixRow* __restrict__ rows,
                                                        float* __restrict__ target, int B, int K, float on, float off) {
    const unsigned n = (unsigned)B * (unsigned)K;               // B K < 2^31 (checked by the host)
    for (unsigned e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int i = (int)(e / (unsigned)K), k = (int)(e - (unsigned)i * (unsigned)K);
        const float y1 = labels[i] == k ? on : off, y2 = labels[B - 1 - i] == k ? on : off;
        target[e] = blend(y1, y2, rows[i].t_self, rows[i].t_other);
    }
}

// ---- soft-target cross-entropy ------------------------------------------------------------------------------------------------------
// (block_sum / block_max, the fixed-order sums and maxima over the workgroup: common.h)
// the target of element k of a row: the dense row, or smoothing / K + (1 - smoothing) [k == label]
struct Tgt {
    const float* dense;
    long long label;
    float off, conf;
    __device__ __forceinline__ float at(int k) const { return dense ? dense[k] : off + (k == label ? conf : 0.f); }
};
__device__ __forceinline__ Tgt row_target(const float* target, const long long* labels, float smoothing, int K, long long b) {
    Tgt t;
    t.dense = target ? target + b * K : nullptr;
    t.label = target ? -1 : labels[b];
    t.off = smoothing / (float)K;
    t.conf = 1.0f - smoothing;
    return t;
}

// One workgroup per row b: lse[b], tsum[b] = sum_k t_k (exactly 1 for the label form), rowloss[b] = sum_k t_k (lse - x_k).  A thread keeps a
// running maximum and rescaled sum over k = tid, tid + 256, ...; the 256 pairs are merged once.
template <typename T>
__global__ void __launch_bounds__(256) soft_ce_fwd_kernel(const T* __restrict__ x, long long ldx, const float* __restrict__ target,
                                                         const long long* __restrict__ labels, float smoothing, int K,
                                                         float* __restrict__ lse, float* __restrict__ tsum, float* __restrict__ rowloss) {
    __shared__ float sh[4];
    const long long b = blockIdx.x;
    const T* xr = x + b * ldx;
    float m = -INFINITY, s = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float z = ActT<T>::ld(xr + k);
        const float mn = fmaxf(m, z);
        s = s * __expf(m - mn) + __expf(z - mn);
        m = mn;
    }
    const float M = block_max(m, sh);
    const float S = block_sum(m == -INFINITY ? 0.f : s * __expf(m - M), sh);      // a thread without a class contributes nothing
    const float l = M + logf(S);
    const Tgt t = row_target(target, labels, smoothing, K, b);
    float acc = 0.f, ts = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float tk = t.at(k);
        acc += tk * (l - ActT<T>::ld(xr + k));
        ts += tk;
    }
    acc = block_sum(acc, sh);
    ts = block_sum(ts, sh);
    if (threadIdx.x == 0) {
        lse[b] = l;
        tsum[b] = target ? ts : 1.0f;
        rowloss[b] = acc;
    }
}

// out[0] = (sum_b rowloss[b]) / B: a fixed tree in double
__global__ void __launch_bounds__(256) soft_ce_finish_kernel(const float* __restrict__ rowloss, int B, float* __restrict__ out) {
    __shared__ double s[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) a += (double)rowloss[i];
    a = block_tree_sum(a, s);
    if (threadIdx.x == 0) out[0] = (float)(a / (double)B);
}

// dx[b][k] = (up / B) (exp(x_k - lse_b) tsum_b - t_k) for k < K, 0 for K <= k < ldx; one workgroup per row
template <typename T>
__global__ void __launch_bounds__(256) soft_ce_bwd_kernel(const T* __restrict__ x, long long ldx, const float* __restrict__ target,
                                                         const long long* __restrict__ labels, float smoothing, int B, int K,
                                                         const float* __restrict__ lse, const float* __restrict__ tsum,
                                                         const float* __restrict__ up, T* __restrict__ dx) {
    const long long b = blockIdx.x;
    const float scale = up[0] / (float)B, l = lse[b], ts = tsum[b];
    const Tgt t = row_target(target, labels, smoothing, K, b);
    const T* xr = x + b * ldx;
    T* dr = dx + b * ldx;
    for (int k = threadIdx.x; k < ldx; k += 256)
        ActT<T>::st(dr + k, k < K ? scale * (__expf(ActT<T>::ld(xr + k) - l) * ts - t.at(k)) : 0.f);
}

// ---- EMA ----------------------------------------------------------------------------------------------------------------------------
// ema[i] = fl(fl(ema[i] d) + fl(c p[i])); shadow (bf16 bits, may be null) = bf16(ema[i]).  VEC == 4: 16-byte accesses.
template <int VEC>
__global__ void __launch_bounds__(256) ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, uint16_t* __restrict__ shadow,
                                                        long long n, float d, float c) {
    const long long groups = n / VEC;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long e = g * VEC;
        if (VEC == 4) {
            const f32x4 a = ld4(ema + e), b = ld4(p + e);
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = __fadd_rn(__fmul_rn(a[k], d), __fmul_rn(c, b[k]));
            st4(ema + e, o);
            if (shadow) st4(shadow + e, o);
        } else {
            const float o = __fadd_rn(__fmul_rn(ema[e], d), __fmul_rn(c, p[e]));
            ema[e] = o;
            if (shadow) shadow[e] = f32_to_bf16_bits(o);
        }
    }
}

inline unsigned stream_grid(long long items) {                   // 256 threads each; at most 8 workgroups per CU, the rest by the stride
    const long long b = (items + 255) / 256, cap = (long long)mmae_cu_count() * 8;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mmae_mixup_pairs(float* x, const void* rows, int B, int C, int H, int W, void* stream) {
    const long long chw = (long long)C * H * W;
    MMAE_REQUIRE(x && rows && B > 0 && B % 2 == 0 && C > 0 && H > 0 && W > 0 && B / 2 <= 65535 && chw < (1ll << 31),
                 "mixup_pairs: bad argument (B even, <= 131070; C H W < 2^31)");
    if (W % 4 == 0 && aligned16(x))
        hipLaunchKernelGGL(mixup_pairs_kernel<4>, dim3(stream_grid(chw / 4), B / 2), dim3(256), 0, (hipStream_t)stream, x, (const MixRow*)rows, B,
                           (unsigned)chw, (unsigned)H, (unsigned)W);
    else
        hipLaunchKernelGGL(mixup_pairs_kernel<1>, dim3(stream_grid(chw), B / 2), dim3(256), 0, (hipStream_t)stream, x, (const MixRow*)rows, B,
                           (unsigned)chw, (unsigned)H, (unsigned)W);
    return mmae_check_launch("mixup_pairs");
}

extern "C" int mmae_mix_target(const int64_t* labels, const void* rows, float* target, int B, int K, float on_value, float off_value,
                               void* stream) {
    MMAE_REQUIRE(labels && rows && target && B > 0 && K > 0 && (long long)B * K < (1ll << 31), "mix_target: bad argument (B K < 2^31)");
    hipLaunchKernelGGL(mix_target_kernel, dim3(stream_grid((long long)B * K)), dim3(256), 0, (hipStream_t)stream, (const long long*)labels,
                       (const MixRow*)rows, target, B, K, on_value, off_value);
    return mmae_check_launch("mix_target");
}

extern "C" int mmae_soft_ce_fwd(const void* x, int x_dtype, int64_t ldx, const float* target, const int64_t* labels, float smoothing, int B, int K,
                                float* lse, float* tsum, float* rowloss, float* out, void* stream) {
    MMAE_REQUIRE(x && (target != nullptr) != (labels != nullptr) && lse && tsum && rowloss && out && B > 0 && K > 0 && ldx >= K &&
                     (x_dtype == MMAE_F32 || x_dtype == MMAE_BF16),
                 "soft_ce_fwd: bad argument (f32 or bf16 logits, exactly one of target / labels)");
    if (x_dtype == MMAE_F32)
        hipLaunchKernelGGL(soft_ce_fwd_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)x, (long long)ldx, target,
                           (const long long*)labels, smoothing, K, lse, tsum, rowloss);
    else
        hipLaunchKernelGGL(soft_ce_fwd_kernel<uint16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (long long)ldx, target,
                           (const long long*)labels, smoothing, K, lse, tsum, rowloss);
    hipLaunchKernelGGL(soft_ce_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)rowloss, B, out);
    return mmae_check_launch("soft_ce_fwd");
}

extern "C" int mmae_soft_ce_bwd(const void* x, int x_dtype, int64_t ldx, const float* target, const int64_t* labels, float smoothing, int B, int K,
                                const float* lse, const float* tsum, const float* up, void* dx, void* stream) {
    MMAE_REQUIRE(x && (target != nullptr) != (labels != nullptr) && lse && tsum && up && dx && B > 0 && K > 0 && ldx >= K &&
                     (x_dtype == MMAE_F32 || x_dtype == MMAE_BF16),
                 "soft_ce_bwd: bad argument (f32 or bf16 logits, exactly one of target / labels)");
    MMAE_REQUIRE(ldx < (1ll << 31), "soft_ce_bwd: ldx < 2^31");
    if (x_dtype == MMAE_F32)
        hipLaunchKernelGGL(soft_ce_bwd_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)x, (long long)ldx, target,
                           (const long long*)labels, smoothing, B, K, lse, tsum, up, (float*)dx);
    else
        hipLaunchKernelGGL(soft_ce_bwd_kernel<uint16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (long long)ldx, target,
                           (const long long*)labels, smoothing, B, K, lse, tsum, up, (uint16_t*)dx);
    return mmae_check_launch("soft_ce_bwd");
}

extern "C" int mmae_ema_update(float* ema, const float* p, void* shadow, int64_t n, float decay, float one_minus_decay, void* stream) {
    MMAE_REQUIRE(ema && p && n > 0, "ema_update: bad argument");
    if (n % 4 == 0 && aligned16(ema) && aligned16(p) && (((uintptr_t)shadow) & 7) == 0)
        hipLaunchKernelGGL(ema_update_kernel<4>, dim3(stream_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, ema, p, (uint16_t*)shadow,
                           (long long)n, decay, one_minus_decay);
    else
        hipLaunchKernelGGL(ema_update_kernel<1>, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, ema, p, (uint16_t*)shadow, (long long)n,
                           decay, one_minus_decay);
    return mmae_check_launch("ema_update");
}
