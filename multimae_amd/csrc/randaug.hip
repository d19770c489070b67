// RandAugment on the device (include/mmae.h, "RandAugment"; multimae_amd/rand_augment.py, staging.ClsStager): the per-image step the
// classification training transform applies between crop / flip and the tensor conversion (utils/auto_augment.py:624-694,
// utils/transforms_factory.py:85-99), applied to the uint8 CHW batch after the H2D copy.  The host makes every random choice and
// evaluates the level functions; the table carries the results, and the kernels here restate what PIL computes byte for byte.
//
// Launches: the layers run one after the other over the whole batch, each as two launches on the caller's stream.
//   stats   one workgroup per sample; it returns at once unless the sample's op of this layer needs the whole image: AutoContrast
//           and Equalize (per-channel 256-bin histogram -> a 3 x 256 byte lookup table), Contrast (integer sum of the grey image ->
//           the mean).  It reads the PREVIOUS layer's output, so the statistics are those of the image the op is applied to.
//           Histograms are uint32 in LDS, one per wave (16 waves), merged with integer adds; the results go to the sample's 1 KB of workspace.
//   apply   src -> dst, four consecutive pixels of a plane per thread (one 4-byte store per channel when H W % 4 == 0 and the
//           pointers are 4-byte aligned, byte stores otherwise); a sample without an op in this layer is copied.  Every byte of dst is
//           written exactly once per launch, and y is the destination of the last layer only: earlier layers alternate between two
//           scratch images.
// Nothing is written outside y and the caller's scratch.  An op code or interpolation outside the valid range is a no-op (a copy), a
// layer count is clamped to [0, MMAE_RA_MAX_LAYERS]: neither is ever used as an index.
//
// Rounding: the affine path (f64) and the blends / the SMOOTH filter (f32) restate C expressions PIL's compiler does not contract.
// This file is compiled with FMA contraction off twice over: `#pragma clang fp contract(off)` below covers every function defined
// here, and the Makefile builds the translation unit with -ffp-contract=off (the header intrinsics __dmul_rn / __dadd_rn are plain
// operators and would be contracted with their neighbours, so they are NOT what this file relies on).  Products and sums are written as
// plain operators in the order of the C source they restate.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int NTS = 1024;               // stats kernel: threads per workgroup (16 waves, a histogram each)
constexpr int NWS = NTS / 64;
constexpr int MAXL = MMAE_RA_MAX_LAYERS;
constexpr int ROW = MMAE_RA_ROW;
constexpr int LAYER = 16;                 // int32 words per layer
constexpr int WS = 1024;                  // workspace bytes per sample: 768 lookup bytes, then the int32 contrast mean
static_assert(ROW == 4 + LAYER * MAXL, "table row layout");

enum Op { NOOP = 0, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE };

// the op of layer l of sample b: NOOP beyond the sample's layer count and for every code out of range
__device__ __forceinline__ int layer_op(const int32_t* __restrict__ table, int b, int l) {
    const int32_t* row = table + (long long)b * ROW;
    int n = row[0];
    n = n < 0 ? 0 : (n > MAXL ? MAXL : n);
    if (l < 0 || l >= n) return NOOP;
    const int32_t* w = row + 4 + LAYER * l;
    const int op = w[0];
    if (op < NOOP || op > AFFINE) return NOOP;
    if (op == AFFINE && w[1] != 2 && w[1] != 3) return NOOP;
    return op;
}

__device__ __forceinline__ int grey_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ----------------------------------------------------------------------------------------------------------------------- stats --
// 1024 threads: one workgroup reads a whole sample, so what bounds it is the number of loads in flight; four independent loads per
// thread and sweep
template <bool VEC>
__global__ void __launch_bounds__(NTS) stats_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ table,
                                                   uint8_t* __restrict__ ws, int hw, int layer) {
    __shared__ uint32_t hist[NWS][768];
    __shared__ unsigned long long gsum;
    __shared__ int lo_hi[3][2];
    const int b = blockIdx.x, t = threadIdx.x;
    const int op = layer_op(table, b, layer);
    if (op != AUTOCONTRAST && op != EQUALIZE && op != CONTRAST) return;            // uniform over the workgroup
    const uint8_t* sb = src + (long long)b * 3 * hw;
    uint8_t* wb = ws + (long long)b * WS;
    if (op == CONTRAST) {
        if (t == 0) gsum = 0;
        __syncthreads();
        unsigned long long acc = 0;
        if (VEC) {
            const uint32_t* r4 = reinterpret_cast<const uint32_t*>(sb);
            const uint32_t* g4 = reinterpret_cast<const uint32_t*>(sb + hw);
            const uint32_t* b4 = reinterpret_cast<const uint32_t*>(sb + 2 * (long long)hw);
            const int n = hw / 4;
            for (int i0 = t; i0 < n; i0 += 4 * NTS) {
                uint32_t r[4], g[4], bl[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * NTS;
                    r[u] = i < n ? r4[i] : 0u;
                    g[u] = i < n ? g4[i] : 0u;
                    bl[u] = i < n ? b4[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + u * NTS < n)
                        for (int k = 0; k < 32; k += 8) acc += (unsigned)grey_of((r[u] >> k) & 255, (g[u] >> k) & 255, (bl[u] >> k) & 255);
            }
        } else {
            for (int p = t; p < hw; p += NTS) acc += (unsigned)grey_of(sb[p], sb[hw + p], sb[2 * (long long)hw + p]);
        }
        atomicAdd(&gsum, acc);
        __syncthreads();
        if (t == 0)                                                                // int(mean + 0.5), the mean an f64 quotient
            *reinterpret_cast<int32_t*>(wb + 768) = (int)((double)gsum / (double)hw + 0.5);
        return;
    }
    for (int i = t; i < NWS * 768; i += NTS) (&hist[0][0])[i] = 0;
    __syncthreads();
    uint32_t* mine = hist[t >> 6];
    if (VEC) {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(sb);
        const int plane = hw / 4, n = 3 * plane;
        for (int i0 = t; i0 < n; i0 += 4 * NTS) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = i0 + u * NTS < n ? s4[i0 + u * NTS] : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * NTS;
                if (i < n) {
                    const int c = (i >= plane) + (i >= 2 * plane);
                    for (int k = 0; k < 32; k += 8) atomicAdd(&mine[c * 256 + ((v[u] >> k) & 255)], 1u);
                }
            }
        }
    } else {
        for (long long i = t; i < 3LL * hw; i += NTS) {
            const int c = (i >= hw) + (i >= 2LL * hw);
            atomicAdd(&mine[c * 256 + sb[i]], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < 768; i += NTS) {
        uint32_t sum = 0;
        for (int w = 0; w < NWS; ++w) sum += hist[w][i];
        hist[0][i] = sum;
    }
    __syncthreads();
    const uint32_t* h = hist[0];
    if (op == AUTOCONTRAST) {
        if (t < 3) {
            int lo = 0, hi = 255;
            while (lo < 255 && h[t * 256 + lo] == 0) ++lo;
            while (hi > 0 && h[t * 256 + hi] == 0) --hi;
            lo_hi[t][0] = lo;
            lo_hi[t][1] = hi;
        }
        __syncthreads();
        for (int i = t; i < 768; i += NTS) {
            const int c = i >> 8, v = i & 255, lo = lo_hi[c][0], hi = lo_hi[c][1];
            int o = v;
            if (hi > lo) {
                const double scale = 255.0 / (double)(hi - lo);
                const double offset = -(double)lo * scale;
                const double r = (double)v * scale + offset;
                o = r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r);
            }
            wb[i] = (uint8_t)o;
        }
    } else if (t < 3) {                                                            // EQUALIZE: one thread walks a channel's bins
        const uint32_t* hc = h + t * 256;
        uint8_t* lut = wb + t * 256;
        long long total = 0;
        int bins = 0, last = 0;
        for (int i = 0; i < 256; ++i)
            if (hc[i]) { total += hc[i]; ++bins; last = i; }
        const long long step = bins > 1 ? (total - hc[last]) / 255 : 0;
        long long n = step / 2;
        for (int i = 0; i < 256; ++i) {
            if (step == 0) {
                lut[i] = (uint8_t)i;
            } else {
                const long long q = n / step;
                lut[i] = (uint8_t)(q > 255 ? 255 : q);
                n += hc[i];
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------------- apply --
// Image.blend(degenerate d, image s, f): d + f (s - d) in f32, truncated; clipped first when f lies outside [0, 1]
__device__ __forceinline__ int blend(int d, int s, float f) {
    float t = (float)d + f * (float)(s - d);
    if (!(f >= 0.0f && f <= 1.0f)) t = !(t > 0.0f) ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (int)t & 255;
}

// PIL's cubic (a = -1) in Horner form
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct LayerArgs {
    int op, interp, iarg;
    float factor;
    double m[6];
    int fill[3];
    int mean;
};

__device__ __forceinline__ double f64_of(const int32_t* w) {
    const unsigned long long bits = (unsigned long long)(uint32_t)w[0] | ((unsigned long long)(uint32_t)w[1] << 32);
    return __longlong_as_double((long long)bits);
}

// ImageFilter.SMOOTH of channel plane s at (y, x): (1 1 1 / 1 5 1 / 1 1 1) / 13 in f32, the row below first, + 0.5, clipped, truncated;
// border pixels are copied
__device__ __forceinline__ int smooth_at(const uint8_t* __restrict__ s, int y, int x, int H, int W) {
    const uint8_t* r0 = s + (long long)y * W + x;
    if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return r0[0];
    constexpr float K1 = 1.0f / 13.0f, K5 = 5.0f / 13.0f;
    const uint8_t* rm = r0 - W;
    const uint8_t* rp = r0 + W;
    float ss = 0.5f;
    ss = ss + (((float)rp[-1] * K1 + (float)rp[0] * K1) + (float)rp[1] * K1);
    ss = ss + (((float)r0[-1] * K1 + (float)r0[0] * K5) + (float)r0[1] * K1);
    ss = ss + (((float)rm[-1] * K1 + (float)rm[0] * K1) + (float)rm[1] * K1);
    return !(ss > 0.0f) ? 0 : (ss >= 255.0f ? 255 : (int)ss);
}

// Image.transform(AFFINE) at output pixel (y, x) of the sample whose planes start at s
__device__ __forceinline__ void affine_at(const LayerArgs& L, const uint8_t* __restrict__ s, int y, int x, int H, int W, int hw, int* out) {
    const double xs = (double)x + 0.5, ys = (double)y + 0.5;
    double xin = L.m[0] * xs + L.m[1] * ys + L.m[2];
    double yin = L.m[3] * xs + L.m[4] * ys + L.m[5];
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
        out[0] = L.fill[0]; out[1] = L.fill[1]; out[2] = L.fill[2];
        return;
    }
    xin = xin - 0.5;
    yin = yin - 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    const int ix = (int)fx, iy = (int)fy;                                          // in [-1, W - 1], [-1, H - 1]
    if (L.interp == 3) {
        int cx[4], cy[4];
        for (int j = 0; j < 4; ++j) {
            cx[j] = clampi(ix - 1 + j, 0, W - 1);
            cy[j] = clampi(iy - 1 + j, 0, H - 1) * W;
        }
        for (int c = 0; c < 3; ++c) {
            const uint8_t* p = s + (long long)c * hw;
            double r[4];
            for (int j = 0; j < 4; ++j) {
                const uint8_t* q = p + cy[j];
                r[j] = cubic((double)q[cx[0]], (double)q[cx[1]], (double)q[cx[2]], (double)q[cx[3]], dx);
            }
            const double v = cubic(r[0], r[1], r[2], r[3], dy);
            out[c] = !(v > 0.0) ? 0 : (v >= 255.0 ? 255 : (int)v);
        }
    } else {
        const int x0 = clampi(ix, 0, W - 1), x1 = clampi(ix + 1, 0, W - 1);
        const int y0 = clampi(iy, 0, H - 1) * W, y1 = clampi(iy + 1, 0, H - 1) * W;
        for (int c = 0; c < 3; ++c) {
            const uint8_t* p = s + (long long)c * hw;
            const double a0 = (double)p[y0 + x0], b0 = (double)p[y0 + x1], a1 = (double)p[y1 + x0], b1 = (double)p[y1 + x1];
            const double v0 = a0 + (b0 - a0) * dx;
            const double v1 = a1 + (b1 - a1) * dx;
            const double v = v0 + (v1 - v0) * dy;
            out[c] = clampi((int)v, 0, 255);
        }
    }
}

template <bool VEC>
__global__ void __launch_bounds__(NT) apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                   const int32_t* __restrict__ table, const uint8_t* __restrict__ ws, int H, int W,
                                                   int layer, int gx) {
    __shared__ uint8_t lut[768];
    const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
    const int hw = H * W;
    LayerArgs L;
    L.op = layer_op(table, b, layer);                                              // uniform over the workgroup
    {
        const int32_t* row = table + (long long)b * ROW;
        const int32_t* w = row + 4 + LAYER * (L.op == NOOP ? 0 : layer);           // (a NOOP reads none of it)
        L.interp = w[1];
        L.iarg = w[2];
        L.factor = __int_as_float(w[3]);
        for (int k = 0; k < 6; ++k) L.m[k] = f64_of(w + 4 + 2 * k);
        for (int k = 0; k < 3; ++k) L.fill[k] = row[1 + k] & 255;
    }
    const uint8_t* wb = ws + (long long)b * WS;
    L.mean = L.op == CONTRAST ? (*reinterpret_cast<const int32_t*>(wb + 768) & 255) : 0;
    if (L.op == AUTOCONTRAST || L.op == EQUALIZE)
        for (int i = threadIdx.x; i < 768; i += NT) lut[i] = wb[i];
    __syncthreads();
    const uint8_t* sb = src + (long long)b * 3 * hw;
    uint8_t* db = dst + (long long)b * 3 * hw;
    const int q = bx * NT + threadIdx.x;
    const int p0 = q * 4;
    if (p0 >= hw) return;
    const int np = hw - p0 < 4 ? hw - p0 : 4;                                      // 4 when VEC
    uint32_t in[3], o[3] = {0u, 0u, 0u};
    if (VEC) {
        for (int c = 0; c < 3; ++c) in[c] = *reinterpret_cast<const uint32_t*>(sb + (long long)c * hw + p0);
    } else {
        for (int c = 0; c < 3; ++c) {
            in[c] = 0;
            for (int k = 0; k < np; ++k) in[c] |= (uint32_t)sb[(long long)c * hw + p0 + k] << (8 * k);
        }
    }
    int y = 0, x = 0;
    if (L.op == SHARPNESS || L.op == AFFINE) {
        y = p0 / W;
        x = p0 - y * W;
    }
    for (int k = 0; k < np; ++k) {
        int v[3] = {(int)((in[0] >> (8 * k)) & 255u), (int)((in[1] >> (8 * k)) & 255u), (int)((in[2] >> (8 * k)) & 255u)};
        int r[3] = {v[0], v[1], v[2]};
        switch (L.op) {
        case AUTOCONTRAST:
        case EQUALIZE:
            for (int c = 0; c < 3; ++c) r[c] = lut[c * 256 + v[c]];
            break;
        case INVERT:
            for (int c = 0; c < 3; ++c) r[c] = 255 - v[c];
            break;
        case POSTERIZE: {
            const int bits = clampi(L.iarg, 0, 8);
            const int mask = bits == 0 ? 0 : (~((1 << (8 - bits)) - 1)) & 255;
            for (int c = 0; c < 3; ++c) r[c] = v[c] & mask;
            break;
        }
        case SOLARIZE:
            for (int c = 0; c < 3; ++c) r[c] = v[c] < L.iarg ? v[c] : 255 - v[c];
            break;
        case SOLARIZE_ADD:
            for (int c = 0; c < 3; ++c) {
                const long long a = (long long)v[c] + L.iarg;
                r[c] = v[c] < 128 ? (int)(a > 255 ? 255 : (a < 0 ? 0 : a)) : v[c];
            }
            break;
        case COLOR: {
            const int g = grey_of(v[0], v[1], v[2]);
            for (int c = 0; c < 3; ++c) r[c] = blend(g, v[c], L.factor);
            break;
        }
        case CONTRAST:
            for (int c = 0; c < 3; ++c) r[c] = blend(L.mean, v[c], L.factor);
            break;
        case BRIGHTNESS:
            for (int c = 0; c < 3; ++c) r[c] = blend(0, v[c], L.factor);
            break;
        case SHARPNESS:
            for (int c = 0; c < 3; ++c) r[c] = blend(smooth_at(sb + (long long)c * hw, y, x, H, W), v[c], L.factor);
            break;
        case AFFINE:
            affine_at(L, sb, y, x, H, W, hw, r);
            break;
        default:
            break;
        }
        for (int c = 0; c < 3; ++c) o[c] |= (uint32_t)(r[c] & 255) << (8 * k);
        if (++x == W) { x = 0; ++y; }
    }
    if (VEC) {
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(db + (long long)c * hw + p0) = o[c];
    } else {
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < np; ++k) db[(long long)c * hw + p0 + k] = (uint8_t)(o[c] >> (8 * k));
    }
}

inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }
inline long long image_bytes(int B, int H, int W) { return ((long long)B * 3 * H * W + 15) / 16 * 16; }

}  // namespace

extern "C" int64_t mmae_rand_augment_scratch_bytes(int B, int H, int W, int layers) {
    if (B <= 0 || H <= 0 || W <= 0 || layers < 1 || layers > MAXL) return -1;
    const int images = layers >= 3 ? 2 : layers - 1;
    return (int64_t)B * WS + images * image_bytes(B, H, W);
}

extern "C" int mmae_rand_augment_u8(const uint8_t* x, const int32_t* table, uint8_t* y, void* scratch, int64_t scratch_bytes,
                                    int B, int H, int W, int layers, void* stream) {
    MMAE_REQUIRE(x && table && y && scratch, "rand_augment_u8: null pointer");
    MMAE_REQUIRE(B > 0 && H > 0 && W > 0, "rand_augment_u8: bad shape");
    MMAE_REQUIRE(layers >= 1 && layers <= MAXL, "rand_augment_u8: layers must lie in [1, MMAE_RA_MAX_LAYERS]");
    MMAE_REQUIRE((long long)H * W * 3 <= 0x7fffffffLL - 3, "rand_augment_u8: a sample holds more than 2^31 - 4 elements");
    MMAE_REQUIRE(scratch_bytes >= mmae_rand_augment_scratch_bytes(B, H, W, layers), "rand_augment_u8: the scratch buffer is too small");
    MMAE_REQUIRE(aligned(scratch, 16), "rand_augment_u8: the scratch buffer must be 16-byte aligned");
    const long long total = (long long)B * 3 * H * W;
    MMAE_REQUIRE(x + total <= y || y + total <= x, "rand_augment_u8: x and y overlap (the geometric ops read neighbours)");
    const int hw = H * W;
    const long long gx = ((hw + 3LL) / 4 + NT - 1) / NT;
    MMAE_REQUIRE((long long)B * gx <= 0x7fffffffLL, "rand_augment_u8: the batch is too large for one launch");
    uint8_t* ws = static_cast<uint8_t*>(scratch);
    uint8_t* tmp[2] = {ws + (long long)B * WS, ws + (long long)B * WS + image_bytes(B, H, W)};
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = x;
    for (int l = 0; l < layers; ++l) {
        uint8_t* dst = l == layers - 1 ? y : tmp[l & 1];
        const bool vec = hw % 4 == 0 && aligned(src, 4) && aligned(dst, 4);
        if (vec) {
            hipLaunchKernelGGL(stats_kernel<true>, dim3((unsigned)B), dim3(NTS), 0, st, src, table, ws, hw, l);
            hipLaunchKernelGGL(apply_kernel<true>, dim3((unsigned)(B * gx)), dim3(NT), 0, st, src, dst, table, (const uint8_t*)ws, H, W, l, (int)gx);
        } else {
            hipLaunchKernelGGL(stats_kernel<false>, dim3((unsigned)B), dim3(NTS), 0, st, src, table, ws, hw, l);
            hipLaunchKernelGGL(apply_kernel<false>, dim3((unsigned)(B * gx)), dim3(NT), 0, st, src, dst, table, (const uint8_t*)ws, H, W, l, (int)gx);
        }
        const int rc = mmae_check_launch("rand_augment_u8");
        if (rc) return rc;
        src = dst;
    }
    return 0;
}
