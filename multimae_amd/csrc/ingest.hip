// On-device ingest of a host-decoded batch (include/mmae.h, "On-device ingest"; multimae_amd/staging.py): the to-tensor
// conversions of utils/datasets.py:93-107 run after the H2D copy instead of before it, so the compact arrays cross PCIe
// (uint8 HWC rgb, 16-bit depth, uint8 semseg: 65 MB per cfg3 batch of 256) and the fp32 / int64 tensors are written in HBM.
//
// Each thread handles 4 consecutive elements: one 12-byte (rgb), 8- or 16-byte (depth) or 4-byte (semseg) load, 16-byte stores.
// An rgb quad turns into one float4 per channel plane, so every plane is written coalesced.  When the element count (per image
// for rgb) is not a multiple of 4, or a pointer is not aligned for the vector forms, the same mapping runs with scalar accesses.
#include "common.h"

namespace {

constexpr int NT = 256;         // threads per workgroup
constexpr int RGB_QUADS = 4;    // rgb quads per thread: the LDS table is filled once per 4 KB of pixels

// rgb: y[b][c][p] = table[c][x[b][p][c]].  Grid (workgroups per image, B).  The 3 x 256 table sits in LDS (3 KB); the gather has
// no arithmetic, so the result is the caller's host-computed value bit for bit.
template <bool VEC>
__global__ void __launch_bounds__(NT) ingest_rgb_kernel(const uint8_t* __restrict__ x, const float* __restrict__ table, float* __restrict__ y,
                                                        int hw) {
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += NT) tab[i] = table[i];
    __syncthreads();
    const uint8_t* xb = x + (long long)blockIdx.y * hw * 3;
    float* yb = y + (long long)blockIdx.y * hw * 3;
    const int n_quads = (hw + 3) / 4;
    for (int r = 0; r < RGB_QUADS; ++r) {
        const int q = (blockIdx.x * RGB_QUADS + r) * NT + threadIdx.x;
        if (q >= n_quads) return;
        const int p = q * 4;
        if (VEC) {                                                // hw % 4 == 0: 12 bytes at a 4-byte boundary, 16-byte plane stores
            const uint32_t* src = reinterpret_cast<const uint32_t*>(xb + (long long)p * 3);
            const uint32_t w[3] = {src[0], src[1], src[2]};
#define MMAE_RGB_BYTE(j) ((w[(j) >> 2] >> (8 * ((j) & 3))) & 255u)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* t = tab + c * 256;
                *reinterpret_cast<float4*>(yb + (long long)c * hw + p) =
                    make_float4(t[MMAE_RGB_BYTE(c)], t[MMAE_RGB_BYTE(3 + c)], t[MMAE_RGB_BYTE(6 + c)], t[MMAE_RGB_BYTE(9 + c)]);
            }
#undef MMAE_RGB_BYTE
        } else {
            for (int k = 0; k < 4 && p + k < hw; ++k)
                for (int c = 0; c < 3; ++c) yb[(long long)c * hw + p + k] = tab[c * 256 + xb[(long long)(p + k) * 3 + c]];
        }
    }
}

// depth: float(v) * 2^-16 (exact scaling of a once-rounded conversion: what the float64 division then fp32 cast gives)
template <class T, class V, bool VEC>
__global__ void __launch_bounds__(NT) ingest_depth_kernel(const T* __restrict__ x, float* __restrict__ y, long long n) {
    const long long i = ((long long)blockIdx.x * NT + threadIdx.x) * 4;
    if (i >= n) return;
    if (VEC) {
        const V v = *reinterpret_cast<const V*>(x + i);
        *reinterpret_cast<float4*>(y + i) = make_float4((float)v.x * 0x1p-16f, (float)v.y * 0x1p-16f, (float)v.z * 0x1p-16f, (float)v.w * 0x1p-16f);
    } else {
        for (int k = 0; k < 4 && i + k < n; ++k) y[i + k] = (float)x[i + k] * 0x1p-16f;
    }
}

// semseg: class ids widened to int64, unchanged (ids beyond the model's classes included)
template <bool VEC>
__global__ void __launch_bounds__(NT) ingest_semseg_kernel(const uint8_t* __restrict__ x, int64_t* __restrict__ y, long long n) {
    const long long i = ((long long)blockIdx.x * NT + threadIdx.x) * 4;
    if (i >= n) return;
    if (VEC) {
        const uchar4 v = *reinterpret_cast<const uchar4*>(x + i);
        longlong2* d = reinterpret_cast<longlong2*>(y + i);
        d[0] = make_longlong2(v.x, v.y);
        d[1] = make_longlong2(v.z, v.w);
    } else {
        for (int k = 0; k < 4 && i + k < n; ++k) y[i + k] = x[i + k];
    }
}

inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }
inline unsigned flat_blocks(long long n) { return (unsigned)((n + 4LL * NT - 1) / (4LL * NT)); }

}  // namespace

extern "C" int mmae_ingest_rgb_u8(const uint8_t* x, const float* table, float* y, int B, int H, int W, void* stream) {
    MMAE_REQUIRE(x && table && y, "ingest_rgb_u8: null pointer");
    MMAE_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W * 3 <= 0x7fffffffLL, "ingest_rgb_u8: bad shape");
    const int hw = H * W;
    const unsigned gx = (unsigned)(((hw + 3) / 4 + RGB_QUADS * NT - 1) / (RGB_QUADS * NT));
    const bool vec = hw % 4 == 0 && aligned(x, 4) && aligned(y, 16);
    if (vec)
        hipLaunchKernelGGL(ingest_rgb_kernel<true>, dim3(gx, B), dim3(NT), 0, (hipStream_t)stream, x, table, y, hw);
    else
        hipLaunchKernelGGL(ingest_rgb_kernel<false>, dim3(gx, B), dim3(NT), 0, (hipStream_t)stream, x, table, y, hw);
    return mmae_check_launch("ingest_rgb_u8");
}

extern "C" int mmae_ingest_depth(const void* x, int x_dtype, float* y, int B, int n, int standardize, int lo, int hi, float eps, void* stream) {
    MMAE_REQUIRE(x && y, "ingest_depth: null pointer");
    MMAE_REQUIRE(x_dtype == MMAE_U16 || x_dtype == MMAE_I32, "ingest_depth: x_dtype must be MMAE_U16 or MMAE_I32");
    MMAE_REQUIRE(B > 0 && n > 0, "ingest_depth: bad shape");
    if (standardize) {
        MMAE_REQUIRE(n > 1 && lo >= 0 && hi <= n && hi - lo >= 2, "ingest_depth: need 0 <= lo, lo + 2 <= hi <= n");
        return mmae_depth_standardize_int(x, x_dtype, y, B, n, lo, hi, eps, (hipStream_t)stream);
    }
    const long long total = (long long)B * n;
    const unsigned g = flat_blocks(total);
    const hipStream_t s = (hipStream_t)stream;
    if (x_dtype == MMAE_U16) {
        const uint16_t* xs = (const uint16_t*)x;
        if (total % 4 == 0 && aligned(x, 8) && aligned(y, 16))
            hipLaunchKernelGGL((ingest_depth_kernel<uint16_t, ushort4, true>), dim3(g), dim3(NT), 0, s, xs, y, total);
        else
            hipLaunchKernelGGL((ingest_depth_kernel<uint16_t, ushort4, false>), dim3(g), dim3(NT), 0, s, xs, y, total);
    } else {
        const int32_t* xs = (const int32_t*)x;
        if (total % 4 == 0 && aligned(x, 16) && aligned(y, 16))
            hipLaunchKernelGGL((ingest_depth_kernel<int32_t, int4, true>), dim3(g), dim3(NT), 0, s, xs, y, total);
        else
            hipLaunchKernelGGL((ingest_depth_kernel<int32_t, int4, false>), dim3(g), dim3(NT), 0, s, xs, y, total);
    }
    return mmae_check_launch("ingest_depth");
}

extern "C" int mmae_ingest_semseg_u8(const uint8_t* x, int64_t* y, int B, int n, void* stream) {
    MMAE_REQUIRE(x && y, "ingest_semseg_u8: null pointer");
    MMAE_REQUIRE(B > 0 && n > 0, "ingest_semseg_u8: bad shape");
    const long long total = (long long)B * n;
    const unsigned g = flat_blocks(total);
    if (total % 4 == 0 && aligned(x, 4) && aligned(y, 16))
        hipLaunchKernelGGL(ingest_semseg_kernel<true>, dim3(g), dim3(NT), 0, (hipStream_t)stream, x, y, total);
    else
        hipLaunchKernelGGL(ingest_semseg_kernel<false>, dim3(g), dim3(NT), 0, (hipStream_t)stream, x, y, total);
    return mmae_check_launch("ingest_semseg_u8");
}
