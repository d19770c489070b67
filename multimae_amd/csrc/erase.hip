// Random erasing on the device (include/mmae.h, "Random erasing"; multimae_amd/random_erasing.py, staging.ClsStager): the last step
// of the classification training transform, ToTensor -> Normalize -> RandomErasing (utils/transforms_factory.py:117-129,
// utils/random_erasing.py:74-103), applied after the H2D copy.  The host draws the rectangles in the reference's order and hands
// them over as one int32 table; mmae_ingest_rgb_u8_chw_erase turns the uint8 CHW batch of the prefetch form into the normalised,
// erased f32 batch in one pass, mmae_random_erase erases an f32 batch in place.
//
// Both kernels decide "is this element erased, and by what value" with the same routines (erase_hit, erase_value and, for 'pixel'
// mode, philox4x32_10 + box_muller_pair), so the fused result and decode-then-erase agree bit for bit in every mode.  The noise is a
// function of the table's header and the element's linear index alone: neither the launch shape nor the path (vector / scalar,
// fused / in place) enters it.
//
// Fused kernel: a workgroup belongs to one sample, stages that sample's table row (every rectangle intersected with the image: the
// entry point cannot see the table) and the 3 x 256 lookup table in LDS, and walks the sample's 3 H W elements by linear index, 4
// per lane: one 4-byte load, one 16-byte store.  H W % 4 != 0 (a plane's base is then unaligned) or unaligned pointers take the same walk with scalar
// accesses.  Only quads in the rows that hold a rectangle are tested against the rectangles; Philox and the Box-Muller transform run
// only in lanes that hold an erased element.
// In-place kernel: launched over the rows of the rectangles, one wave per row, so it touches erased pixels only; a pixel under
// several rectangles is written once, by the highest one.
#include "common.h"

namespace {

constexpr int NT = 256;        // threads per workgroup
constexpr int QUADS = 4;       // fused kernel: quads per thread, the LDS tables are filled once per 16 KB of output
constexpr int MAXR = MMAE_ERASE_MAX_RECTS;
constexpr int ROW = MMAE_ERASE_ROW;
constexpr int ROWS_GX = 32;    // in-place kernel: workgroups per sample at most (4 rows each per sweep)
static_assert(ROW == 4 + 8 * MAXR, "table row layout");

struct EraseRow {              // one sample's view of the table, in LDS
    uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
    int mode, n;
    int lo, hi;                // the rows that hold a rectangle, as offsets into a plane: [lo, hi) = [y_min W, y_max W); empty without one
    int rect[MAXR][8];         // top, left, h, w (intersected with the image), colour bits of channels 0-3
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// [a, a + len) intersected with [0, size): start and length of what is left (length 0 when nothing is); 64-bit sums, so that no
// a + len of the table overflows
__device__ __forceinline__ void clip_span(int a, int len, int size, int& start, int& n) {
    const long long lo = a > 0 ? a : 0;
    long long hi = (long long)a + (len > 0 ? len : 0);
    hi = hi < size ? hi : size;
    start = hi > lo ? (int)lo : 0;
    n = hi > lo ? (int)(hi - lo) : 0;
}

// threads 0..MAXR-1 take one rectangle each, thread MAXR the header; the caller synchronises
__device__ __forceinline__ void stage_row(EraseRow& s, const int32_t* __restrict__ table, int b, int H, int W) {
    const int t = threadIdx.x;
    if (table == nullptr) {
        if (t == 0) { s.n = 0; s.mode = 0; s.lo = 0; s.hi = 0; }
        return;
    }
    const int32_t* row = table + (long long)(1 + b) * ROW;
    if (t < MAXR) {
        const int32_t* q = row + 4 + 8 * t;
        clip_span(q[0], q[2], H, s.rect[t][0], s.rect[t][2]);
        clip_span(q[1], q[3], W, s.rect[t][1], s.rect[t][3]);
        for (int k = 4; k < 8; ++k) s.rect[t][k] = q[k];
    } else if (t == MAXR) {
        s.seed_lo = (uint32_t)table[0];
        s.seed_hi = (uint32_t)table[1];
        s.ctr_lo = (uint32_t)table[2];
        s.ctr_hi = (uint32_t)table[3];
        s.mode = table[4];
        const int n = clampi(row[0], 0, MAXR);
        s.n = n;
        int y0 = H, y1 = 0;
        for (int r = 0; r < n; ++r) {
            const int32_t* q = row + 4 + 8 * r;
            int top, left, h, w;
            clip_span(q[0], q[2], H, top, h);
            clip_span(q[1], q[3], W, left, w);
            if (h > 0 && w > 0) {
                y0 = top < y0 ? top : y0;
                y1 = top + h > y1 ? top + h : y1;
            }
        }
        s.lo = y0 < y1 ? y0 * W : 0;
        s.hi = y0 < y1 ? y1 * W : 0;
    }
}

// the highest rectangle that covers (y, x), or -1
__device__ __forceinline__ int erase_hit(const EraseRow& s, int y, int x) {
    for (int r = s.n - 1; r >= 0; --r) {
        const int* q = s.rect[r];
        if ((unsigned)(y - q[0]) < (unsigned)q[2] && (unsigned)(x - q[1]) < (unsigned)q[3]) return r;
    }
    return -1;
}

// standard Philox4x32-10
__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ uint4 noise_block(const EraseRow& s, long long e) {
    const unsigned long long blk = (unsigned long long)e >> 2;
    return philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), s.ctr_lo, s.ctr_hi, s.seed_lo, s.seed_hi);
}

// One Box-Muller pair: the normals of elements 4k + 2p (cosine branch) and 4k + 2p + 1 (sine branch) from outputs (a, b) = (o[2p],
// o[2p + 1]) of block k.  Every path takes its values from this one routine, so they agree bit for bit.
__device__ __forceinline__ float2 box_muller_pair(uint32_t a, uint32_t b) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(b >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    const float t = 2.0f * u2;
    return make_float2(r * cospif(t), r * sinpif(t));
}

// the value rectangle r gives element e (channel c): shared by both kernels
__device__ __forceinline__ float erase_value(const EraseRow& s, int r, int c, long long e) {
    if (s.mode == 1) return __int_as_float(s.rect[r][4 + (c < 3 ? c : 3)]);
    if (s.mode == 2) {
        const uint4 o = noise_block(s, e);
        const float2 z = (e & 2) ? box_muller_pair(o.z, o.w) : box_muller_pair(o.x, o.y);
        return (e & 1) ? z.y : z.x;
    }
    return 0.0f;
}

// y[b][c][p] = erased ? value : lut[c][x[b][c][p]].  Grid: B * gx workgroups, gx per sample.
template <bool VEC>
__global__ void __launch_bounds__(NT) ingest_chw_erase_kernel(const uint8_t* __restrict__ x, const float* __restrict__ lut,
                                                              const int32_t* __restrict__ table, float* __restrict__ y, int H, int W,
                                                              int gx) {
    __shared__ float tab[3 * 256];
    __shared__ EraseRow s;
    const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
    for (int i = threadIdx.x; i < 3 * 256; i += NT) tab[i] = lut[i];
    stage_row(s, table, b, H, W);
    __syncthreads();
    const int hw = H * W, n3 = 3 * hw;
    const long long e_b = (long long)b * n3;
    const uint8_t* xb = x + e_b;
    float* yb = y + e_b;
    const int n_quads = (n3 + 3) / 4;
    const int lo = s.lo, hi = s.hi;                                // outside these rows nothing is erased: no division, no rectangle test
    for (int j = 0; j < QUADS; ++j) {
        const int q = (bx * QUADS + j) * NT + threadIdx.x;
        if (q >= n_quads) return;
        const int p = q * 4;
        if (VEC) {                                                 // hw % 4 == 0: the quad lies in one plane, e_b + p is a multiple of 4
            const int c = (p >= hw) + (p >= 2 * hw);
            const uint32_t v = *reinterpret_cast<const uint32_t*>(xb + p);
            const float* t = tab + c * 256;
            float o0 = t[v & 255u], o1 = t[(v >> 8) & 255u], o2 = t[(v >> 16) & 255u], o3 = t[v >> 24];
            const int pp = p - c * hw;
            if (pp + 3 >= lo && pp < hi) {
                int yy = pp / W, xx = pp - yy * W;
                const int h0 = erase_hit(s, yy, xx);
                if (++xx == W) { xx = 0; ++yy; }
                const int h1 = erase_hit(s, yy, xx);
                if (++xx == W) { xx = 0; ++yy; }
                const int h2 = erase_hit(s, yy, xx);
                if (++xx == W) { xx = 0; ++yy; }
                const int h3 = erase_hit(s, yy, xx);
                if ((h0 & h1 & h2 & h3) >= 0) {                  // some element is erased
                    if (s.mode == 2) {                             // one block serves the quad, one transform each pair
                        const uint4 blk = noise_block(s, e_b + p);
                        if ((h0 & h1) >= 0) {
                            const float2 z = box_muller_pair(blk.x, blk.y);
                            if (h0 >= 0) o0 = z.x;
                            if (h1 >= 0) o1 = z.y;
                        }
                        if ((h2 & h3) >= 0) {
                            const float2 z = box_muller_pair(blk.z, blk.w);
                            if (h2 >= 0) o2 = z.x;
                            if (h3 >= 0) o3 = z.y;
                        }
                    } else {
                        if (h0 >= 0) o0 = erase_value(s, h0, c, e_b + p);
                        if (h1 >= 0) o1 = erase_value(s, h1, c, e_b + p + 1);
                        if (h2 >= 0) o2 = erase_value(s, h2, c, e_b + p + 2);
                        if (h3 >= 0) o3 = erase_value(s, h3, c, e_b + p + 3);
                    }
                }
            }
            *reinterpret_cast<float4*>(yb + p) = make_float4(o0, o1, o2, o3);
        } else {
            for (int k = 0; k < 4 && p + k < n3; ++k) {
                const int pk = p + k;
                const int c = (pk >= hw) + (pk >= 2 * hw);
                float o = tab[c * 256 + xb[pk]];
                const int pp = pk - c * hw;
                if (pp >= lo && pp < hi) {
                    const int yy = pp / W, xx = pp - yy * W;
                    const int h = erase_hit(s, yy, xx);
                    if (h >= 0) o = erase_value(s, h, c, e_b + pk);
                }
                yb[pk] = o;
            }
        }
    }
}

// In place over the rectangles' rows: workgroup (b, bx) sweeps the C * h rows of each of sample b's rectangles, a wave per row.
__global__ void __launch_bounds__(NT) erase_inplace_kernel(float* __restrict__ x, const int32_t* __restrict__ table, int C, int H, int W,
                                                           int gx) {
    __shared__ EraseRow s;
    const int b = blockIdx.x / gx, bx = blockIdx.x - b * gx;
    stage_row(s, table, b, H, W);
    __syncthreads();
    const int n = s.n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = 0; r < n; ++r) {
        const int top = s.rect[r][0], left = s.rect[r][1], h = s.rect[r][2], w = s.rect[r][3];
        const long long rows = (long long)C * h;
        for (long long i = bx * 4 + wave; i < rows; i += gx * 4) {
            const int c = (int)(i / h);
            const int yy = top + (int)(i - (long long)c * h);
            const long long base = (((long long)b * C + c) * H + yy) * W;
            for (int xx = left + lane; xx < left + w; xx += 64)
                if (r == n - 1 || erase_hit(s, yy, xx) == r)       // a higher rectangle writes the pixels it covers
                    x[base + xx] = erase_value(s, r, c, base + xx);
        }
    }
}

inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

}  // namespace

extern "C" int mmae_random_erase(float* x, const int32_t* table, int B, int C, int H, int W, void* stream) {
    MMAE_REQUIRE(x && table, "random_erase: null pointer");
    MMAE_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "random_erase: bad shape");
    MMAE_REQUIRE((long long)C * H * W <= 0x7fffffffLL, "random_erase: a sample holds more than 2^31 - 1 elements");
    long long gx = ((long long)C * H + 3) / 4;
    if (gx > ROWS_GX) gx = ROWS_GX;
    MMAE_REQUIRE((long long)B * gx <= 0x7fffffffLL, "random_erase: the batch is too large for one launch");
    hipLaunchKernelGGL(erase_inplace_kernel, dim3((unsigned)(B * gx)), dim3(NT), 0, (hipStream_t)stream, x, table, C, H, W, (int)gx);
    return mmae_check_launch("random_erase");
}

extern "C" int mmae_ingest_rgb_u8_chw_erase(const uint8_t* x, const float* lut, const int32_t* table, float* y, int B, int H, int W,
                                            void* stream) {
    MMAE_REQUIRE(x && lut && y, "ingest_rgb_u8_chw_erase: null pointer");
    MMAE_REQUIRE(B > 0 && H > 0 && W > 0, "ingest_rgb_u8_chw_erase: bad shape");
    MMAE_REQUIRE((long long)H * W * 3 <= 0x7fffffffLL - 3, "ingest_rgb_u8_chw_erase: a sample holds more than 2^31 - 4 elements");
    const int hw = H * W;
    const long long quads = (3LL * hw + 3) / 4;
    const long long gx = (quads + QUADS * NT - 1) / (QUADS * NT);
    MMAE_REQUIRE((long long)B * gx <= 0x7fffffffLL, "ingest_rgb_u8_chw_erase: the batch is too large for one launch");
    const dim3 grid((unsigned)(B * gx));
    if (hw % 4 == 0 && aligned(x, 4) && aligned(y, 16))
        hipLaunchKernelGGL(ingest_chw_erase_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, x, lut, table, y, H, W, (int)gx);
    else
        hipLaunchKernelGGL(ingest_chw_erase_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, x, lut, table, y, H, W, (int)gx);
    return mmae_check_launch("ingest_rgb_u8_chw_erase");
}
