// Implicit-GEMM 3x3 convolution (padding 1, stride 1) for the dense heads: forward and data gradient on the bf16 MFMA, the 3x3 window
// taken from an LDS halo image instead of a [pixels][9 C] buffer in HBM (csrc/conv3x3.hip's gather path writes and re-reads that
// buffer: im2col + mmae_gemm, and mmae_gemm + col2im for the data gradient).
//
// One kernel serves both directions.  Maps are the engine's channels-last f32 [B][h][w][C]; the weight is the bf16 operand
// wp[N][9 K] in (ky, kx, k) order that mmae_conv3x3_weight_pack writes (forward: N = Cout, K = Cin), or its transposed, tap-reversed
// form wpt[Cin][9 Cout] from mmae_conv3x3_weight_pack_t (data gradient: the same kernel run on dY, N = Cin, K = Cout).
//
// Work split.  A 256-thread workgroup owns TH x TW = 8 x 32 output pixels and TN = 64 output channels.  Wave v owns the two pixel
// rows 2v, 2v + 1 of the tile (two 32-pixel M tiles of v_mfma_f32_32x32x16_bf16: a tile is 32 pixels of ONE row) and all 64 channels
// (two N tiles): four 32x32 accumulators, 64 registers.  When only 32 of the 64 channels exist (Cout % 64 == 32) the second N tile is
// skipped by every wave alike.  The contraction runs over K in stages of KC = 32 channels; per stage the workgroup writes to LDS
//   sA: the (TH + 2) x (TW + 2) halo of the input tile, 32 channels per pixel, read as f32, ReLU applied if asked, rounded to bf16
//       (round to nearest even: the operand the gather path's GEMM sees), zeros outside the map -- 340 pixels x 64 B = 21,760 B;
//   sB: the weights of the stage, [tap][channel of the N tile][32 k] -- 9 x 64 x 64 B = 36,864 B;
// and every wave then issues 9 taps x 2 k-steps x 4 MFMAs from them.  The halo is staged once per K stage and used by all nine taps.
// Summation order is fixed (K stage, ky, kx, k-step ascending; the MFMA's own order inside): two runs are bit-equal; no atomics.
//
// Fragment maps (v_mfma_f32_32x32x16_bf16, lane l, r = l & 31, g = l >> 5): A[row r][k = 8 g + j], B[k = 8 g + j][col r], j = 0..7;
// C/D: col = r, row = (reg & 3) + 8 (reg >> 2) + 4 g.  A rows are pixels, B columns are output channels, so a lane reads 16 bytes
// (eight consecutive k) of one halo pixel / one weight row per fragment (ds_read_b128) and holds ONE channel of 16 pixels at the end:
// the 32 lanes of a half-wave store 128 contiguous bytes of a pixel's channels.
//
// LDS layout.  Both images are rows of 64 B (a pixel / a weight row: four 16-byte slots, slot s = k / 8).  The 32 lanes of a half-wave
// read 32 CONSECUTIVE rows (the pixels of one map row; 32 channels), i.e. a 64-byte stride: unswizzled, rows 4 apart share their
// banks and each of ds_read_b128's four 16-lane groups would be 4-way conflicted.  Slot s of row p is stored at slot
// s ^ ((p >> 2) & 3): every 16-lane group ({0-3, 12-15, 20-27} and so on) covers all residues of p mod 16, hence 16 distinct slots
// of the 256-byte bank row -- conflict-free for any base row, which the tap offset (kx) shifts by 0 .. 2.  The 16-byte stores of the
// staging loops write a row's four slots from four consecutive lanes (a permutation inside 64 contiguous bytes: no conflict either).
//
// Resource use (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   igemm3_kernel:  92 VGPRs + 64 AGPRs (the four accumulators), 72 SGPRs, no scratch, no spills, 58,624 B of static LDS per workgroup;
//                   occupancy 2 waves per SIMD -- set by the LDS (two workgroups of four waves per compute unit; the registers
//                   would allow three), so one workgroup stages its next K stage while the other issues MFMAs
//   wpack3t_kernel: 59 VGPRs, no scratch, no LDS, 8 waves per SIMD
// The LDS is static and below 64 KiB: no dynamic-LDS opt-in is involved.
#include "common.h"

namespace {

constexpr int TH = 8, TW = 32;                  // output pixels of a workgroup (ops.CONV3X3_IGEMM_TILE restates them for the tests)
constexpr int TN = 64;                          // output channels of a workgroup
constexpr int KC = 32;                          // contraction channels per LDS stage
constexpr int HH = TH + 2, HW = TW + 2;         // the halo
constexpr int A_BYTES = HH * HW * KC * 2;       // 21,760
constexpr int B_BYTES = 9 * TN * KC * 2;        // 36,864

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// byte offset of 16-byte slot q (0..3) of 64-byte row `row`
__device__ __forceinline__ int swz(int row, int q) { return row * 64 + ((q ^ ((row >> 2) & 3)) << 4); }

// y[b][oy][ox][n] = m * (sum_{ky, kx, k} a(x[b][oy + ky - 1][ox + kx - 1][k]) wp[n][(3 ky + kx) K + k] + bias[n]) + add[b][oy][ox][n]
//   a = bf16 rounding (after max(., 0) when relu), 0 outside the map; m = (mask[b][oy][ox][n] > 0), 1 without a mask.
// The forward passes (bias, no mask, resid); the data gradient (no bias, xmask, addend).
__global__ void __launch_bounds__(256) igemm3_kernel(const float* __restrict__ x, const uint16_t* __restrict__ wp, const float* __restrict__ bias,
                                                    const float* __restrict__ mask, const float* __restrict__ add, float* __restrict__ y, int h, int w,
                                                    int K, int N, int relu, int tiles_x, int tiles_y, int tiles_n) {
    __shared__ __attribute__((aligned(16))) char sA[A_BYTES];
    __shared__ __attribute__((aligned(16))) char sB[B_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, g = lane >> 5;
    int bid = blockIdx.x;                                            // N tile fastest: the workgroups that share a halo run together
    const int tn = bid % tiles_n; bid /= tiles_n;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const long long b = bid / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW, n0 = tn * TN;
    const bool two = n0 + 32 < N;                                    // the second 32-channel N tile exists (N % 32 == 0)
    const float* xb = x + b * h * w * (long long)K;

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

    for (int k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();                                             // the previous stage's fragments have been read
        // the halo: one item = eight channels of one halo pixel (two 16-byte loads, one 16-byte LDS store)
        for (int i = tid; i < HH * HW * 4; i += 256) {
            const int hp = i >> 2, q = i & 3;
            const int hy = hp / HW, hx = hp - hy * HW;
            const int iy = oy0 + hy - 1, ix = ox0 + hx - 1;
            i32x4 o = (i32x4){0, 0, 0, 0};
            if (iy >= 0 && iy < h && ix >= 0 && ix < w) {            // the address is formed only for a pixel of the map
                const float* s = xb + ((long long)iy * w + ix) * K + k0 + q * 8;
                f32x4 a = ld4(s), c = ld4(s + 4);
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = a[e] > 0.f ? a[e] : 0.f; c[e] = c[e] > 0.f ? c[e] : 0.f; }
                }
                o[0] = (int)pack_bf16x2(a[0], a[1]); o[1] = (int)pack_bf16x2(a[2], a[3]);
                o[2] = (int)pack_bf16x2(c[0], c[1]); o[3] = (int)pack_bf16x2(c[2], c[3]);
            }
            *reinterpret_cast<i32x4*>(sA + swz(hp, q)) = o;
        }
        // the weights: one item = eight k of one (tap, channel) row; channels beyond N are zero rows (never multiplied: see `two`)
        for (int i = tid; i < 9 * TN * 4; i += 256) {
            const int row = i >> 2, q = i & 3;                       // row = tap * TN + n
            const int n = row & (TN - 1), tap = row >> 6;
            i32x4 v = (i32x4){0, 0, 0, 0};
            if (n0 + n < N) v = *reinterpret_cast<const i32x4*>(wp + ((long long)(n0 + n) * 9 + tap) * K + k0 + q * 8);
            *reinterpret_cast<i32x4*>(sB + swz(row, q)) = v;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int q = kk * 2 + g;
                bf16x8 af[2], bf[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) af[mi] = *reinterpret_cast<const bf16x8*>(sA + swz((2 * wave + mi + ky) * HW + kx + r, q));
                bf[0] = *reinterpret_cast<const bf16x8*>(sB + swz(tap * TN + r, q));
                if (two) bf[1] = *reinterpret_cast<const bf16x8*>(sB + swz(tap * TN + 32 + r, q));
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    acc[mi][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mi], bf[0], acc[mi][0], 0, 0, 0);
                    if (two) acc[mi][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mi], bf[1], acc[mi][1], 0, 0, 0);
                }
            }
        }
    }

    // epilogue: lane (r, g) holds channel n0 + 32 ni + r of the pixels (reg & 3) + 8 (reg >> 2) + 4 g of row 2 wave + mi
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int oy = oy0 + 2 * wave + mi;
        if (oy >= h) continue;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if (ni == 1 && !two) continue;
            const int ch = n0 + 32 * ni + r;
            const float bv = bias ? bias[ch] : 0.f;
            const long long row0 = ((b * h + oy) * w) * (long long)N + ch;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ox = ox0 + (e & 3) + 8 * (e >> 2) + 4 * g;
                if (ox >= w) continue;
                const long long o = row0 + (long long)ox * N;
                float v = acc[mi][ni][e] + bv;
                if (mask) v = mask[o] > 0.f ? v : 0.f;
                if (add) v += add[o];
                y[o] = v;
            }
        }
    }
}

// wpt[c][(8 - t) Cout + o] = wp[o][t Cin + c]; one element per thread, consecutive threads on consecutive elements of wpt
__global__ void __launch_bounds__(256) wpack3t_kernel(const uint16_t* __restrict__ wp, uint16_t* __restrict__ wpt, int Cout, int Cin, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int o = (int)(i % Cout);
        const long long t2 = i / Cout;
        const int tt = (int)(t2 % 9);
        const long long c = t2 / 9;
        wpt[i] = wp[((long long)o * 9 + (8 - tt)) * Cin + c];
    }
}

// one launch over the whole batch; K = contraction channels, N = output channels
int launch_igemm(const char* what, const float* x, const void* wp, const float* bias, const float* mask, const float* add, float* y, int B, int h,
                 int w, int K, int N, int relu, void* stream) {
    const long long tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH, tiles_n = (N + TN - 1) / TN;
    const long long blocks = (long long)B * tiles_y * tiles_x * tiles_n;
    if (blocks >= (1LL << 31)) { mmae_set_error("conv3x3_igemm: the map needs more workgroups than a launch has"); return MMAE_EINVAL; }
    hipLaunchKernelGGL(igemm3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (const uint16_t*)wp, bias, mask, add, y, h, w, K, N,
                       relu, (int)tiles_x, (int)tiles_y, (int)tiles_n);
    return mmae_check_launch(what);
}

inline bool igemm_geom_ok(int B, int h, int w, int Ca, int Cb) {
    return B > 0 && h > 0 && w > 0 && Ca > 0 && Cb > 0 && Ca % 32 == 0 && Cb % 32 == 0 &&
           (long long)B * h * w * (Ca > Cb ? Ca : Cb) < (1LL << 40);
}

}  // namespace

extern "C" int mmae_conv3x3_igemm_fwd(const float* x, const void* wp, const float* bias, const float* resid, float* y, int B, int h, int w, int Cin,
                                      int Cout, int relu, void* stream) {
    MMAE_REQUIRE(x && wp && y && B > 0 && h > 0 && w > 0 && Cin > 0 && Cout > 0, "conv3x3_igemm_fwd: bad argument");
    MMAE_REQUIRE(igemm_geom_ok(B, h, w, Cin, Cout), "conv3x3_igemm_fwd: needs Cin % 32 == 0, Cout % 32 == 0 and fewer than 2^40 map elements");
    MMAE_REQUIRE(al16(x) && al16(wp) && al16(y) && al16(resid), "conv3x3_igemm_fwd: x, wp, y and resid must be 16-byte aligned");
    MMAE_REQUIRE(x != y, "conv3x3_igemm_fwd: y must not be x (neighbouring workgroups read the halo)");
    return launch_igemm("conv3x3_igemm_fwd", x, wp, bias, nullptr, resid, y, B, h, w, Cin, Cout, relu, stream);
}

extern "C" int mmae_conv3x3_igemm_dgrad(const float* dy, const void* wpt, const float* xmask, const float* addend, float* dx, int B, int h, int w,
                                        int Cout, int Cin, void* stream) {
    MMAE_REQUIRE(dy && wpt && dx && B > 0 && h > 0 && w > 0 && Cin > 0 && Cout > 0, "conv3x3_igemm_dgrad: bad argument");
    MMAE_REQUIRE(igemm_geom_ok(B, h, w, Cin, Cout), "conv3x3_igemm_dgrad: needs Cin % 32 == 0, Cout % 32 == 0 and fewer than 2^40 map elements");
    MMAE_REQUIRE(al16(dy) && al16(wpt) && al16(dx) && al16(addend) && al16(xmask),
                 "conv3x3_igemm_dgrad: dy, wpt, dx, xmask and addend must be 16-byte aligned");
    MMAE_REQUIRE(dy != dx, "conv3x3_igemm_dgrad: dx must not be dy (neighbouring workgroups read the halo)");
    return launch_igemm("conv3x3_igemm_dgrad", dy, wpt, nullptr, xmask, addend, dx, B, h, w, Cout, Cin, 0, stream);
}

extern "C" int mmae_conv3x3_weight_pack_t(const void* wp, void* wpt, int Cout, int Cin, void* stream) {
    MMAE_REQUIRE(wp && wpt && wp != wpt && Cout > 0 && Cin > 0, "conv3x3_weight_pack_t: bad argument");
    const long long total = (long long)Cout * 9 * Cin;
    const long long nb = (total + 255) / 256;
    hipLaunchKernelGGL(wpack3t_kernel, dim3((unsigned)(nb > 65536 ? 65536 : nb)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)wp, (uint16_t*)wpt,
                       Cout, Cin, total);
    return mmae_check_launch("conv3x3_weight_pack_t");
}
