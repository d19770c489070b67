// Truncated depth standardisation (run_pretraining_multimae.py:487-492): per sample, mean and unbiased variance of the
// values whose rank lies in [lo, hi) -- the reference sorts all c*h*w = 50 176 values of every depth map per step and slices
// the sorted row -- then (x - mean) / sqrt(var + eps) over the whole map.
//
// No sort: only the two cut VALUES matter.  One workgroup per sample finds the keys of rank lo and hi-1 by a 4-pass 8-bit
// radix select over order-preserving integer keys (both ranks in the same passes, two 256-bin LDS histograms), then sums
// the values strictly between the cuts and adds the right number of copies of the cut values themselves (ties at a cut are
// counted by rank, exactly as the slice of a sorted row would).  The map (196 KB) stays in the workgroup's L2 across the
// passes; HBM sees one read and one write.  Sums are accumulated in fp64 (a few thousand adds per lane, off the critical path)
// so the result does not depend on the summation order the reference's mean()/var() happened to use.
#include "common.h"

namespace {

__device__ __forceinline__ unsigned key_of(float f) {          // monotone: a < b  <=>  key(a) < key(b)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float val_of(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ double block_sum_d(double v, double* red) {    // all threads get the total; red: 16 doubles
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}

// Element loaders: the kernel below is one thread-to-element mapping and one fp64 reduction order for every input form, so a
// map decoded on the device (csrc/ingest.hip) and standardised in the same launch is bit-identical to one converted first and
// standardised as fp32.  key(i) is an order-preserving integer key of val(i) in the low KEY_BITS bits; val_of(key) inverts it.
struct LoadF32 {                                                  // the fp32 map as it is
    static constexpr int KEY_BITS = 32;
    const float* p;
    __device__ __forceinline__ LoadF32 at(long long o) const { return {p + o}; }
    __device__ __forceinline__ float val(int i) const { return p[i]; }
    __device__ __forceinline__ unsigned key(int i) const { return key_of(p[i]); }
    __device__ __forceinline__ static float val_of_key(unsigned k) { return val_of(k); }
};
struct LoadU16 {                                                  // 16-bit PNG depth: v * 2^-16 is exact and strictly increasing in v,
    static constexpr int KEY_BITS = 16;                           // so the raw value is the key: 2 passes over 2-byte elements
    const uint16_t* p;
    __device__ __forceinline__ LoadU16 at(long long o) const { return {p + o}; }
    __device__ __forceinline__ float val(int i) const { return (float)p[i] * 0x1p-16f; }
    __device__ __forceinline__ unsigned key(int i) const { return p[i]; }
    __device__ __forceinline__ static float val_of_key(unsigned k) { return (float)k * 0x1p-16f; }
};
struct LoadI32 {                                                  // Pillow 'I' depth (a bicubic resize may leave 0..65535).  The key is the
    static constexpr int KEY_BITS = 32;                           // one of the CONVERTED value: beyond |v| = 2^24 distinct integers round to
    const int32_t* p;                                             // one float, and a key of the integer would then count them apart
    __device__ __forceinline__ LoadI32 at(long long o) const { return {p + o}; }
    __device__ __forceinline__ float val(int i) const { return (float)p[i] * 0x1p-16f; }
    __device__ __forceinline__ unsigned key(int i) const { return key_of(val(i)); }
    __device__ __forceinline__ static float val_of_key(unsigned k) { return val_of(k); }
};

__device__ __forceinline__ int block_sum_i(int v, int* red) {              // all threads get the total; red: 16 ints
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}

// Validity predicates.  AllValid is the pre-training form: every element takes part, the caller gives the cuts.  ByteMask is the
// fine-tuning form (run_finetuning_depth.py:671-688): an element takes part iff its mask byte is non-zero (m == nullptr: all are)
// and its value is not a NaN; the cuts are fractions of the count of those, taken on the device by one counting pass in front.
// What x holds under a zero mask byte never enters a sum or a product: the output there is a stored 0.
struct AllValid {
    static constexpr bool MASKED = false;
    __device__ __forceinline__ AllValid at(long long) const { return {}; }
    __device__ __forceinline__ bool keep(int) const { return true; }
    __device__ __forceinline__ bool part(int, float) const { return true; }
};
struct ByteMask {
    static constexpr bool MASKED = true;
    const uint8_t* m;
    __device__ __forceinline__ ByteMask at(long long o) const { return {m ? m + o : nullptr}; }
    __device__ __forceinline__ bool keep(int i) const { return !m || m[i] != 0; }
    __device__ __forceinline__ bool part(int i, float v) const { return keep(i) && v == v; }
};

// lo, hi: the cuts (AllValid) -- ignored by ByteMask, which takes them as (int)((float)n_valid * lo_frac) and the same of hi_frac, one
// f32 product each, truncated: the reference's (n_valid * 0.1).long().  A slice of fewer than two values (hi - lo < 2: var() of the reference is
// NaN, the mean of an empty slice too) gives NaN at every mask-true element; every thread still passes every barrier.
template <class L, class V>
__global__ void __launch_bounds__(1024) depth_standardize_kernel(L x, V valid, float* __restrict__ y, int n, int lo, int hi, float lo_frac,
                                                                 float hi_frac, float eps) {
    __shared__ int hist[2][256];
    __shared__ unsigned sel_prefix[2];
    __shared__ int sel_rank[2], sel_less[2], sel_eq[2];
    __shared__ double red[16];
    const L xs = x.at((long long)blockIdx.x * n);
    const V vs = valid.at((long long)blockIdx.x * n);
    float* ys = y + (long long)blockIdx.x * n;
    const int tid = threadIdx.x;
    if constexpr (V::MASKED) {
        __shared__ int redi[16];
        int c = 0;
        for (int i = tid; i < n; i += 1024) c += vs.part(i, xs.val(i)) ? 1 : 0;
        const int n_valid = block_sum_i(c, redi);                  // <= 2^24: exact as a float
        lo = (int)((float)n_valid * lo_frac);
        hi = (int)((float)n_valid * hi_frac);
    }
    if (tid < 2) { sel_prefix[tid] = 0u; sel_rank[tid] = tid == 0 ? lo : hi - 1; sel_less[tid] = 0; }
    for (int shift = L::KEY_BITS - 8; shift >= 0; shift -= 8) {
        for (int i = tid; i < 512; i += 1024) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned p0 = sel_prefix[0], p1 = sel_prefix[1];
        for (int i = tid; i < n; i += 1024) {
            if (V::MASKED && !vs.part(i, xs.val(i))) continue;
            const unsigned k = xs.key(i);
            const unsigned top = shift == L::KEY_BITS - 8 ? 0u : (k >> (shift + 8));
            const int bin = (k >> shift) & 255;
            if (top == p0) atomicAdd(&hist[0][bin], 1);
            if (top == p1) atomicAdd(&hist[1][bin], 1);
        }
        __syncthreads();
        if (tid < 2) {                                             // serial 256-bin scan: negligible next to the histogram pass
            int r = sel_rank[tid], b = 0, cum = 0;
            for (; b < 255; ++b) { if (cum + hist[tid][b] > r) break; cum += hist[tid][b]; }
            sel_rank[tid] = r - cum;
            sel_less[tid] += cum;
            sel_eq[tid] = hist[tid][b];
            sel_prefix[tid] = (sel_prefix[tid] << 8) | (unsigned)b;
        }
        __syncthreads();
    }
    const unsigned k1 = sel_prefix[0], k2 = sel_prefix[1];
    const float v1 = L::val_of_key(k1), v2 = L::val_of_key(k2);
    // copies of the cut values inside [lo, hi)
    const int cnt = hi - lo;
    const int n1 = (k1 == k2) ? cnt : (sel_less[0] + sel_eq[0] - lo);
    const int n2 = (k1 == k2) ? 0 : (hi - sel_less[1]);
    double s = 0.0;
    for (int i = tid; i < n; i += 1024) {
        if (V::MASKED && !vs.part(i, xs.val(i))) continue;
        const unsigned k = xs.key(i);
        if (k > k1 && k < k2) s += (double)xs.val(i);
    }
    s = block_sum_d(s, red) + (double)n1 * (double)v1 + (double)n2 * (double)v2;
    const double mean = s / (double)cnt;
    double q = 0.0;
    for (int i = tid; i < n; i += 1024) {
        if (V::MASKED && !vs.part(i, xs.val(i))) continue;
        const unsigned k = xs.key(i);
        if (k > k1 && k < k2) { const double d = (double)xs.val(i) - mean; q += d * d; }
    }
    q = block_sum_d(q, red) + (double)n1 * ((double)v1 - mean) * ((double)v1 - mean) + (double)n2 * ((double)v2 - mean) * ((double)v2 - mean);
    const float var = (float)(q / (double)(cnt - 1));            // unbiased, as Tensor.var
    const float mu = (float)mean, rs = 1.0f / sqrtf(var + eps);
    if constexpr (V::MASKED) {
        const bool degenerate = cnt < 2;                           // the selection above ran on whatever it found: nothing of it is used
        for (int i = tid; i < n; i += 1024) {
            float o = 0.0f;                                        // a mask-false element: +0, whatever x holds there
            if (vs.keep(i)) o = degenerate ? __uint_as_float(0x7fc00000u) : (xs.val(i) - mu) * rs;
            ys[i] = o;
        }
    } else {
        for (int i = tid; i < n; i += 1024) ys[i] = (xs.val(i) - mu) * rs;
    }
}

// x[b][c][i] = mask[b][i] ? x[b][c][i] : +0 (run_finetuning_depth.py:690-695 for one task).  Nothing is multiplied: a valid element is
// not touched, an invalid one is overwritten.  VEC: 16-byte quads (n % 4 == 0, x 16-byte and mask 4-byte aligned) -- a quad without an
// invalid element is neither read nor written, one without a valid element is written without being read.
template <bool VEC>
__global__ void __launch_bounds__(256) mask_invalid_kernel(float* __restrict__ x, const uint8_t* __restrict__ mask, long long total, int C, int n) {
    const long long stride = (long long)gridDim.x * 256;
    if constexpr (VEC) {
        const int nq = n >> 2;                                     // total counts quads
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += stride) {
            const long long row = q / nq;                          // b * C + c
            const int iq = (int)(q - row * nq);
            const uchar4 m = reinterpret_cast<const uchar4*>(mask + (row / C) * n)[iq];
            const bool a = m.x != 0, b = m.y != 0, c = m.z != 0, d = m.w != 0;
            if (a && b && c && d) continue;
            uint4* p = reinterpret_cast<uint4*>(x) + q;            // as integers: the bits of a kept element pass through untouched
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (a || b || c || d) {
                v = *p;
                v.x = a ? v.x : 0u; v.y = b ? v.y : 0u; v.z = c ? v.z : 0u; v.w = d ? v.w : 0u;
            }
            *p = v;
        }
    } else {
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
            const long long row = e / n;
            const int i = (int)(e - row * n);
            if (mask[(row / C) * n + i] == 0) x[e] = 0.0f;
        }
    }
}

}  // namespace

extern "C" int mmae_depth_standardize(const float* x, float* y, int B, int n, int lo, int hi, float eps, void* stream) {
    MMAE_REQUIRE(x && y && B > 0 && n > 1, "depth_standardize: bad argument");
    MMAE_REQUIRE(lo >= 0 && hi <= n && hi - lo >= 2, "depth_standardize: need 0 <= lo, lo + 2 <= hi <= n");
    hipLaunchKernelGGL((depth_standardize_kernel<LoadF32, AllValid>), dim3(B), dim3(1024), 0, (hipStream_t)stream, LoadF32{x}, AllValid{}, y, n,
                       lo, hi, 0.0f, 0.0f, eps);
    return mmae_check_launch("depth_standardize");
}

extern "C" int mmae_depth_standardize_masked(const float* x, const uint8_t* mask, float* y, int B, int n, float lo_frac, float hi_frac,
                                             float eps, void* stream) {
    MMAE_REQUIRE(x && y && B > 0, "depth_standardize_masked: bad argument");
    MMAE_REQUIRE(n >= 1 && n <= (1 << 24), "depth_standardize_masked: need 1 <= n <= 2^24 (the count must be exact as a float)");
    // written so that a NaN fails every comparison
    MMAE_REQUIRE(lo_frac >= 0.0f && lo_frac <= hi_frac && hi_frac <= 1.0f, "depth_standardize_masked: need 0 <= lo_frac <= hi_frac <= 1");
    MMAE_REQUIRE(eps == eps, "depth_standardize_masked: eps is NaN");
    hipLaunchKernelGGL((depth_standardize_kernel<LoadF32, ByteMask>), dim3(B), dim3(1024), 0, (hipStream_t)stream, LoadF32{x}, ByteMask{mask}, y,
                       n, 0, 0, lo_frac, hi_frac, eps);
    return mmae_check_launch("depth_standardize_masked");
}

extern "C" int mmae_mask_invalid(float* x, const uint8_t* mask, int B, int C, int n, void* stream) {
    MMAE_REQUIRE(x && mask && B > 0 && C > 0 && n > 0, "mask_invalid: bad argument");
    const long long total = (long long)B * C * n;
    const bool vec = n % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    const long long units = vec ? total / 4 : total;
    const long long blocks = (units + 255) / 256;
    const dim3 grid((unsigned)(blocks > 8192 ? 8192 : blocks));
    if (vec) hipLaunchKernelGGL(mask_invalid_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, mask, units, C, n);
    else hipLaunchKernelGGL(mask_invalid_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, mask, units, C, n);
    return mmae_check_launch("mask_invalid");
}

// mmae_ingest_depth's fused form (csrc/ingest.hip): the same kernel over the host-decoded integer map; arguments checked there
int mmae_depth_standardize_int(const void* x, int x_dtype, float* y, int B, int n, int lo, int hi, float eps, hipStream_t stream) {
    if (x_dtype == MMAE_U16)
        hipLaunchKernelGGL((depth_standardize_kernel<LoadU16, AllValid>), dim3(B), dim3(1024), 0, stream, LoadU16{(const uint16_t*)x}, AllValid{}, y,
                           n, lo, hi, 0.0f, 0.0f, eps);
    else
        hipLaunchKernelGGL((depth_standardize_kernel<LoadI32, AllValid>), dim3(B), dim3(1024), 0, stream, LoadI32{(const int32_t*)x}, AllValid{}, y,
                           n, lo, hi, 0.0f, 0.0f, eps);
    return mmae_check_launch("ingest_depth");
}
