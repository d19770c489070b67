// The DPT head's regression tail and the weight layouts of its transposed convolutions (DPTOutputAdapter, output_adapters.py:576-759).
//
//   - tail: the last two layers of the regression head, nn.ReLU(True) -> nn.Conv2d(32, num_channels, 1) (output_adapters.py:631-632),
//     in one pass over the f32 channels-last map x [B][H][W][C]: every pixel's row of C is read once (a tile of rows at a time through
//     LDS, so the loads are consecutive), K <= 16 accumulators stay in registers, and the result is stored straight into the f32
//     NCHW image [B][K][H][W] -- consecutive threads hold consecutive pixels, so every store of a wave is one contiguous span of
//     an output plane.  The plain route (cast + GEMM into an 8-padded row + transposing copy) writes a bf16 copy of the map and
//     reads it again.
//   - its backward in one pass as well: dx = (x > 0) * (g . W), and the weight and bias gradients as per-workgroup partial rows
//     [nblk][K C + K] -- no float atomics, every sum in a fixed order (pixels ascending within a tile, a workgroup's tiles ascending,
//     the rows then summed by mmae_colsum_partials).
//   - nn.ConvTranspose2d(C, C, kernel_size=s, stride=s) of act_1 / act_2_postprocess (output_adapters.py:667-672,681-686) has no
//     overlap, so it is a row GEMM [B nh nw, Cin] x [Cin, s s Cout] and the pixel shuffle of the ConvNeXt head
//     (mmae_convnext_shuffle_fwd) when the GEMM's columns are ordered (i, j, co): the (Cin, Cout, s, s) weight is packed into that
//     operand, the bias tiled s s times for the GEMM's bias epilogue, and the gradients taken back.
// All f32 arithmetic; x is never modified (the reference's in-place ReLU is not observable from outside).
#include "common.h"

namespace {

constexpr int TAIL_MAX_K = 16;                                   // == MMAE_REG_MAX_K: the regression losses' limit
constexpr int TAIL_TP = 128;                                     // pixels of one tile = threads of its workgroup
constexpr int TAIL_MAX_BLK = 2048;                               // rows of the backward's partials at most

inline unsigned grid_for(long long total, int per) {
    const long long b = (total + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}
inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

inline bool tail_geom_ok(int B, int H, int W, int C, int K) {
    return B > 0 && H > 0 && W > 0 && C % 4 == 0 && C >= 4 && C <= 64 && K >= 1 && K <= TAIL_MAX_K &&
           (long long)B * H * W * 64 < (1LL << 42);
}

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    return (f32x4){v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f, v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f};
}

// ---------------------------------------------------------------------------------------------------------- tail forward --
// out[b][k][p] = bias[k] + sum_c w[k][c] max(x[b][p][c], 0), c ascending, one FMA per term.  A workgroup of TAIL_TP threads walks tiles
// of TAIL_TP pixels.  A tile's rows are one contiguous span of x: the threads copy it into LDS with consecutive 16-byte loads (the
// ReLU applied on the way; rows padded by four floats against bank conflicts), then thread t holds pixel t, reads its row from LDS
// and keeps KT >= K accumulators (1, 4 or 16 at compile time) in registers; the weight reads are uniform over the wave.  Every
// store of a wave is one contiguous span of an output plane.  LDS (floats): xs [TAIL_TP][C + 4].
template <int KT>
__global__ void __launch_bounds__(TAIL_TP) tail_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, long long HW, int C, int K, long long P, long long tiles) {
    extern __shared__ float lds[];
    const int ldx = C + 4, G = C / 4, t = threadIdx.x;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * TAIL_TP;
        const int np = (int)(P - p0 < TAIL_TP ? P - p0 : TAIL_TP);          // pixels of this tile
        const float* src = x + p0 * C;
        for (int j = t; j < np * G; j += TAIL_TP) {
            const int p = j / G, c4 = j - p * G;
            st4(lds + p * ldx + c4 * 4, relu4(ld4(src + (long long)j * 4)));
        }
        __syncthreads();
        if (t < np) {
            float acc[KT];
#pragma unroll
            for (int k = 0; k < KT; ++k) acc[k] = k < K ? bias[k] : 0.f;
            const float* row = lds + t * ldx;
            for (int c = 0; c < C; c += 4) {
                const f32x4 v = ld4(row + c);
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    if (k < K) {
                        const f32x4 wk = ld4(w + k * C + c);
                        acc[k] = __builtin_fmaf(wk[0], v[0], acc[k]);
                        acc[k] = __builtin_fmaf(wk[1], v[1], acc[k]);
                        acc[k] = __builtin_fmaf(wk[2], v[2], acc[k]);
                        acc[k] = __builtin_fmaf(wk[3], v[3], acc[k]);
                    }
                }
            }
            const long long i = p0 + t, b = i / HW, p = i - b * HW;
            float* o = out + b * K * HW + p;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) o[(long long)k * HW] = acc[k];
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------- tail backward --
// One workgroup of TAIL_TP threads walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of TAIL_TP pixels.  Per tile:
//   1. the tile's rows of x go into LDS as in the forward -- max(x, 0), plus a column of ones, which makes the bias gradient one more
//      column -- and thread t, which holds pixel t, reads g[b][.][p] into registers and LDS (zeros for a pixel past the end);
//   2. entry e = k (C + 1) + c of the [K][C + 1] gradient block is summed over the tile's pixels in ascending order by the thread that
//      owns it (e = t, t + TAIL_TP, ...) and added to the workgroup's running sum in LDS, which only that thread touches;
//   3. thread t overwrites its row with dx = (x > 0) * sum_k g[k] w[k][.] (k ascending; max(x, 0) > 0 exactly where x > 0);
//   4. the rows leave for dx as one contiguous span, consecutive 16-byte stores.
// LDS (floats): xs [TAIL_TP][C + 4] | gs [TAIL_TP][K + 1] | run [K (C + 1)].
template <int KT>
__global__ void __launch_bounds__(TAIL_TP) tail_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ w,
                                                          float* __restrict__ dx, float* __restrict__ part, long long HW, int C, int K,
                                                          long long P, long long tiles) {
    extern __shared__ float lds[];
    const int ldx = C + 4, ldg = K + 1, C1 = C + 1, E = K * C1, G = C / 4;
    float* xs = lds;
    float* gs = xs + TAIL_TP * ldx;
    float* run = gs + TAIL_TP * ldg;
    const int t = threadIdx.x;
    for (int e = t; e < E; e += TAIL_TP) run[e] = 0.f;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = tile * TAIL_TP;
        const int np = (int)(P - p0 < TAIL_TP ? P - p0 : TAIL_TP);
        const bool in = t < np;
        float gk[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) gk[k] = 0.f;
        if (in) {
            const long long i = p0 + t, b = i / HW, p = i - b * HW;
            const float* gp = g + b * K * HW + p;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < K) gk[k] = gp[(long long)k * HW];
        }
#pragma unroll
        for (int k = 0; k < KT; ++k)
            if (k < K) gs[t * ldg + k] = gk[k];
        const float* src = x + p0 * C;
        for (int j = t; j < TAIL_TP * G; j += TAIL_TP) {
            const int p = j / G, c4 = j - p * G;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (p < np) v = relu4(ld4(src + (long long)j * 4));
            st4(xs + p * ldx + c4 * 4, v);
        }
        xs[t * ldx + C] = in ? 1.f : 0.f;
        __syncthreads();
        for (int e = t; e < E; e += TAIL_TP) {
            const int k = e / C1, c = e - k * C1;
            float s = 0.f;
#pragma unroll 8
            for (int p = 0; p < TAIL_TP; ++p) s = __builtin_fmaf(gs[p * ldg + k], xs[p * ldx + c], s);
            run[e] += s;
        }
        __syncthreads();
        if (in) {
            float* row = xs + t * ldx;
            for (int c = 0; c < C; c += 4) {
                const f32x4 v = ld4(row + c);
                f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    if (k < K) {
                        const f32x4 wk = ld4(w + k * C + c);
                        a[0] = __builtin_fmaf(gk[k], wk[0], a[0]);
                        a[1] = __builtin_fmaf(gk[k], wk[1], a[1]);
                        a[2] = __builtin_fmaf(gk[k], wk[2], a[2]);
                        a[3] = __builtin_fmaf(gk[k], wk[3], a[3]);
                    }
                }
                st4(row + c, (f32x4){v[0] > 0.f ? a[0] : 0.f, v[1] > 0.f ? a[1] : 0.f, v[2] > 0.f ? a[2] : 0.f, v[3] > 0.f ? a[3] : 0.f});
            }
        }
        __syncthreads();
        float* dst = dx + p0 * C;
        for (int j = t; j < np * G; j += TAIL_TP) {
            const int p = j / G, c4 = j - p * G;
            st4(dst + (long long)j * 4, ld4(xs + p * ldx + c4 * 4));
        }
        __syncthreads();
    }
    // row blockIdx.x of the partials: [K C] weight-gradient sums, then [K] bias-gradient sums
    float* row = part + (long long)blockIdx.x * (K * C + K);
    for (int e = t; e < E; e += TAIL_TP) {
        const int k = e / C1, c = e - k * C1;
        row[c < C ? k * C + c : K * C + k] = run[e];
    }
}

inline int tail_nblk(long long P) {
    const long long tiles = (P + TAIL_TP - 1) / TAIL_TP;
    return (int)(tiles < 1 ? 1 : (tiles > TAIL_MAX_BLK ? TAIL_MAX_BLK : tiles));
}

// ------------------------------------------------------------------------------------------ transposed-convolution weights --
// wp[(i s + j) Cout + co][ci] = w[ci][co][i][j]; one element per thread, consecutive threads on consecutive elements of wp
template <typename T>
__global__ void __launch_bounds__(256) deconv_wpack_kernel(const float* __restrict__ w, T* __restrict__ wp, int Cin, int Cout, int ss, long long total) {
    for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < total; n += (long long)gridDim.x * 256) {
        const int ci = (int)(n % Cin);
        const long long r = n / Cin;
        const int co = (int)(r % Cout);
        const int ij = (int)(r / Cout);
        ActT<T>::st(wp + n, w[((long long)ci * Cout + co) * ss + ij]);
    }
}
// bp[ij Cout + co] = bias[co]
__global__ void __launch_bounds__(256) deconv_bpack_kernel(const float* __restrict__ bias, float* __restrict__ bp, int Cout, int total) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < total) bp[n] = bias[n % Cout];
}
// dw[ci][co][i][j] (+)= dwp[((i s + j) Cout + co)][ci]; consecutive threads on consecutive elements of dw
__global__ void __launch_bounds__(256) deconv_wunpack_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int Cin, int Cout, int ss, int accumulate,
                                                            long long total) {
    for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < total; n += (long long)gridDim.x * 256) {
        const int ij = (int)(n % ss);
        const long long r = n / ss;
        const int co = (int)(r % Cout);
        const long long ci = r / Cout;
        const float v = dwp[((long long)ij * Cout + co) * Cin + ci];
        dw[n] = accumulate ? dw[n] + v : v;
    }
}
// db[co] (+)= sum_ij dbp[ij Cout + co], ij ascending from the first term
__global__ void __launch_bounds__(256) deconv_bunpack_kernel(const float* __restrict__ dbp, float* __restrict__ db, int Cout, int ss, int accumulate) {
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Cout) return;
    float s = dbp[co];
    for (int ij = 1; ij < ss; ++ij) s += dbp[ij * Cout + co];
    db[co] = accumulate ? db[co] + s : s;
}

inline bool deconv_geom_ok(int Cin, int Cout, int s) {
    return Cin > 0 && Cout > 0 && s >= 1 && s <= 8 && (long long)Cin * Cout * s * s < (1LL << 31);
}

}  // namespace

extern "C" int mmae_dpt_tail_fwd(const float* x, const float* w, const float* bias, float* out, int B, int H, int W, int C, int K, void* stream) {
    MMAE_REQUIRE(tail_geom_ok(B, H, W, C, K), "dpt_tail_fwd: needs B, H, W > 0, C % 4 == 0, 4 <= C <= 64, 1 <= K <= 16");
    MMAE_REQUIRE(x && w && bias && out && al16(x) && al16(w), "dpt_tail_fwd: null or misaligned pointer (x and w: 16 bytes)");
    const long long HW = (long long)H * W, P = (long long)B * HW;
    const long long tiles = (P + TAIL_TP - 1) / TAIL_TP;
    const dim3 grid(grid_for(tiles, 1)), block(TAIL_TP);
    const size_t lds = sizeof(float) * (size_t)TAIL_TP * (C + 4);                                                       // <= 34.8 KB
    hipStream_t st = (hipStream_t)stream;
    if (K == 1) return mmae_launch_lds<tail_fwd_kernel<1>>(grid, block, lds, st, "dpt_tail_fwd", x, w, bias, out, HW, C, K, P, tiles);
    if (K <= 4) return mmae_launch_lds<tail_fwd_kernel<4>>(grid, block, lds, st, "dpt_tail_fwd", x, w, bias, out, HW, C, K, P, tiles);
    return mmae_launch_lds<tail_fwd_kernel<16>>(grid, block, lds, st, "dpt_tail_fwd", x, w, bias, out, HW, C, K, P, tiles);
}

// rows of the partials mmae_dpt_tail_bwd writes (host only)
extern "C" int mmae_dpt_tail_bwd_nblk(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return tail_nblk((long long)B * H * W);
}

extern "C" int mmae_dpt_tail_bwd(const float* g, const float* x, const float* w, float* dx, float* part, int B, int H, int W, int C, int K,
                                 void* stream) {
    MMAE_REQUIRE(tail_geom_ok(B, H, W, C, K), "dpt_tail_bwd: needs B, H, W > 0, C % 4 == 0, 4 <= C <= 64, 1 <= K <= 16");
    MMAE_REQUIRE(g && x && w && dx && part && al16(x) && al16(w) && al16(dx), "dpt_tail_bwd: null or misaligned pointer (x, w and dx: 16 bytes)");
    const long long HW = (long long)H * W, P = (long long)B * HW;
    const long long tiles = (P + TAIL_TP - 1) / TAIL_TP;
    const dim3 grid((unsigned)tail_nblk(P)), block(TAIL_TP);
    const size_t lds = sizeof(float) * ((size_t)TAIL_TP * (C + 4) + (size_t)TAIL_TP * (K + 1) + (size_t)K * (C + 1));   // <= 47.7 KB
    hipStream_t st = (hipStream_t)stream;
    if (K == 1) return mmae_launch_lds<tail_bwd_kernel<1>>(grid, block, lds, st, "dpt_tail_bwd", g, x, w, dx, part, HW, C, K, P, tiles);
    if (K <= 4) return mmae_launch_lds<tail_bwd_kernel<4>>(grid, block, lds, st, "dpt_tail_bwd", g, x, w, dx, part, HW, C, K, P, tiles);
    return mmae_launch_lds<tail_bwd_kernel<16>>(grid, block, lds, st, "dpt_tail_bwd", g, x, w, dx, part, HW, C, K, P, tiles);
}

extern "C" int mmae_deconv_weight_pack(const float* w, const float* bias, void* wp, int wp_dtype, float* bp, int Cin, int Cout, int s, void* stream) {
    MMAE_REQUIRE(w && wp && deconv_geom_ok(Cin, Cout, s), "deconv_weight_pack: bad argument");
    MMAE_REQUIRE(wp_dtype == MMAE_F32 || wp_dtype == MMAE_BF16, "deconv_weight_pack: wp_dtype must be f32 or bf16");
    MMAE_REQUIRE((bias == nullptr) == (bp == nullptr), "deconv_weight_pack: bias and bp go together");
    const int ss = s * s;
    const long long total = (long long)ss * Cout * Cin;
    hipStream_t st = (hipStream_t)stream;
    if (wp_dtype == MMAE_BF16) hipLaunchKernelGGL(deconv_wpack_kernel<uint16_t>, dim3(grid_for(total, 256)), dim3(256), 0, st, w, (uint16_t*)wp, Cin, Cout, ss, total);
    else hipLaunchKernelGGL(deconv_wpack_kernel<float>, dim3(grid_for(total, 256)), dim3(256), 0, st, w, (float*)wp, Cin, Cout, ss, total);
    if (bias) hipLaunchKernelGGL(deconv_bpack_kernel, dim3((ss * Cout + 255) / 256), dim3(256), 0, st, bias, bp, Cout, ss * Cout);
    return mmae_check_launch("deconv_weight_pack");
}

extern "C" int mmae_deconv_weight_unpack(const float* dwp, const float* dbp, float* dw, float* db, int Cin, int Cout, int s, int accumulate, void* stream) {
    MMAE_REQUIRE(deconv_geom_ok(Cin, Cout, s) && (dwp == nullptr) == (dw == nullptr) && (dbp == nullptr) == (db == nullptr) && (dw || db),
                 "deconv_weight_unpack: bad argument");
    const int ss = s * s;
    const long long total = (long long)ss * Cout * Cin;
    hipStream_t st = (hipStream_t)stream;
    if (dw) hipLaunchKernelGGL(deconv_wunpack_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, dwp, dw, Cin, Cout, ss, accumulate, total);
    if (db) hipLaunchKernelGGL(deconv_bunpack_kernel, dim3((Cout + 255) / 256), dim3(256), 0, st, dbp, db, Cout, ss, accumulate);
    return mmae_check_launch("deconv_weight_unpack");
}
