// Token-level kernels of the MultiMAE path: mask sampler, gather-first patch rows, token
// assembly, decoder query/context builder, patch <-> image layout.  All HBM / latency bound;
// integer outputs (masks, ids) are exact.
#include "common.h"

namespace {

constexpr int MAX_TASKS = 8;

struct TaskTable { int off[MAX_TASKS + 1]; int T; };

__device__ __forceinline__ int task_of(const TaskTable& tt, int idx) {
    int t = 0;
#pragma unroll
    for (int i = 1; i < MAX_TASKS; ++i) if (i < tt.T && idx >= tt.off[i]) t = i;
    return t;
}

// ------------------------------------------------------------------------------------------
// Mask sampler (multimae.py:191-216).  One workgroup per sample; O(N^2) rank counting in LDS
// (N = 588: 0.35 M compares per sample) instead of 5 device-wide argsorts.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mask_sample_kernel(const long long* __restrict__ spt, const float* __restrict__ task_noise,
                                                          const float* __restrict__ all_noise, const TaskTable tt, int Ntot,
                                                          int n_keep, long long* __restrict__ mask_all,
                                                          long long* __restrict__ ids_keep, long long* __restrict__ ids_restore) {
    extern __shared__ float sm[];
    float* noise = sm;                     // [Ntot] per-task noise, later the global keys
    int* order = (int*)(sm + Ntot);        // [Ntot] argsort of the per-task noise (local index)
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < Ntot; j += 256) noise[j] = task_noise[(long long)b * Ntot + j];
    __syncthreads();
    // per-task stable rank -> order[off + rank] = local index
    for (int j = tid; j < Ntot; j += 256) {
        const int t = task_of(tt, j), lo = tt.off[t], hi = tt.off[t + 1];
        const float v = noise[j];
        int rank = 0;
        for (int i = lo; i < hi; ++i) { const float u = noise[i]; rank += (u < v) || (u == v && i < j); }
        order[lo + rank] = j - lo;
    }
    __syncthreads();
    // reference quirk: SORTED POSITION j is kept iff order[j] < k_t; key = mask + noise2 (fp32 add)
    for (int j = tid; j < Ntot; j += 256) {
        const int t = task_of(tt, j);
        const int pre = (order[j] < (int)spt[(long long)b * tt.T + t]) ? 0 : 1;
        noise[j] = (float)pre + all_noise[(long long)b * Ntot + j];
    }
    __syncthreads();
    for (int j = tid; j < Ntot; j += 256) {
        const float v = noise[j];
        int rank = 0;
        for (int i = 0; i < Ntot; ++i) { const float u = noise[i]; rank += (u < v) || (u == v && i < j); }
        ids_restore[(long long)b * Ntot + j] = rank;
        mask_all[(long long)b * Ntot + j] = rank < n_keep ? 0 : 1;
        if (rank < n_keep) ids_keep[(long long)b * n_keep + rank] = j;
    }
}

// ------------------------------------------------------------------------------------------
// Gather-first patch rows.  rows[b*n_sel + r] is the concatenation over tasks of the flattened
// patch (Conv2d weight column order c,i,j), non-zero only in the segment of the task that owns
// token sel[b][r].  One wave per (row, 256-column slab).
// ------------------------------------------------------------------------------------------
struct PatchSrc {
    const void* data;      // f32 [B][C][H][W]  or  int64 [B][H][W] (semseg)
    const float* emb;      // semseg: f32 [n_cls][C]
    int kind, C, H, W, ph, pw, k_off, k_len, n_cls;
};
struct PatchSrcs { PatchSrc s[MAX_TASKS]; };

template <typename RT>
__global__ void __launch_bounds__(256) patch_rows_kernel(const PatchSrcs src, const TaskTable tt, const long long* __restrict__ sel,
                                                         RT* __restrict__ rows, long long n_rows, int n_sel, int Ktot) {
    const long long row = blockIdx.x;
    const int b = (int)(row / n_sel);
    const int idx = (int)sel[row];
    const int t = task_of(tt, idx);
    const PatchSrc& s = src.s[t];
    const int p = idx - tt.off[t];
    const int nw = s.W / s.pw;
    const int py = p / nw, px = p % nw;
    RT* out = rows + row * Ktot;
    for (int k = threadIdx.x; k < Ktot; k += 256) {
        float v = 0.f;
        const int kk = k - s.k_off;
        if (kk >= 0 && kk < s.k_len) {
            const int c = kk / (s.ph * s.pw), ij = kk % (s.ph * s.pw), i = ij / s.pw, j = ij % s.pw;
            const int y = py * s.ph + i, x = px * s.pw + j;
            if (s.kind == 0) v = ((const float*)s.data)[(((long long)b * s.C + c) * s.H + y) * s.W + x];
            else {
                const long long cls = ((const long long*)s.data)[((long long)b * s.H + y) * s.W + x];
                v = (s.n_cls > 0 && (cls < 0 || cls >= s.n_cls)) ? 0.f : s.emb[cls * s.C + c];      // out-of-range ids (e.g. an ignore label) embed as zeros
            }
        }
        ActT<RT>::st(out + k, v);
    }
}

// d_emb[cls][e] += d_rows[row][k_off + e*ph*pw + i*pw + j] over all semseg-owned selected tokens.
// LDS-privatised table per workgroup, flushed with global atomics.
template <typename RT>
__global__ void __launch_bounds__(256) semseg_emb_bwd_kernel(const RT* __restrict__ d_rows, long long ld, const long long* __restrict__ cls,
                                                             const long long* __restrict__ sel, float* __restrict__ d_emb, long long n_rows,
                                                             int n_sel, int H, int W, int E, int ph, int pw, int k_off, int tok_off,
                                                             int n_patches, int n_cls) {
    extern __shared__ float tab[];   // [n_cls*E]
    for (int i = threadIdx.x; i < n_cls * E; i += 256) tab[i] = 0.f;
    __syncthreads();
    const int nw = W / pw, klen = E * ph * pw;
    for (long long row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int p = (int)sel[row] - tok_off;
        if (p < 0 || p >= n_patches) continue;
        const int b = (int)(row / n_sel), py = p / nw, px = p % nw;
        for (int k = threadIdx.x; k < klen; k += 256) {
            const int e = k / (ph * pw), ij = k % (ph * pw), i = ij / pw, j = ij % pw;
            const long long c = cls[((long long)b * H + py * ph + i) * W + px * pw + j];
            if (c >= 0 && c < n_cls) atomicAdd(&tab[c * E + e], ActT<RT>::ld(d_rows + row * ld + k_off + k));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_cls * E; i += 256) { const float v = tab[i]; if (v != 0.f) atomicAdd(&d_emb[i], v); }
}

// The same gradient WITHOUT atomics (round 6; VERDICT r5 item 8: the one non-reproducible reduction of a step): every table entry is summed in
// a fixed order.  A workgroup owns a contiguous range of rows; its threads are NSUB groups of E, thread (sub, e) walks the rows sub, sub + NSUB, ...
// of the range and the pixels of each patch IN ORDER and adds into column e of group sub's PRIVATE LDS table -- no two threads ever touch the same
// entry, so the adds are plain read-modify-writes in program order; the NSUB tables are summed in index order into the workgroup's partial table
// (part[blockIdx.x][n_cls * E]), and a second launch sums the partials over the workgroups in index order.  Bit-identical from run to run, and the
// LDS / L2 atomic traffic of the old form (87 us at cfg3) is gone.
template <typename RT>
__global__ void __launch_bounds__(256) semseg_emb_bwd_part_kernel(const RT* __restrict__ d_rows, long long ld, const long long* __restrict__ cls,
                                                                  const long long* __restrict__ sel, float* __restrict__ part, long long n_rows,
                                                                  int rows_per, int n_sel, int H, int W, int E, int ph, int pw, int k_off, int tok_off,
                                                                  int n_patches, int n_cls, int nsub) {
    extern __shared__ float tab[];   // [nsub][n_cls * E]
    const int n = n_cls * E;
    for (int i = threadIdx.x; i < nsub * n; i += 256) tab[i] = 0.f;
    __syncthreads();
    const int sub = threadIdx.x / E, e = threadIdx.x - sub * E;
    const int nw = W / pw, pp = ph * pw;
    const long long r0 = (long long)blockIdx.x * rows_per, r1 = (r0 + rows_per < n_rows) ? r0 + rows_per : n_rows;
    if (sub < nsub) {
        float* mine = tab + (long long)sub * n;
        for (long long row = r0 + sub; row < r1; row += nsub) {
            const int p = (int)sel[row] - tok_off;
            if (p < 0 || p >= n_patches) continue;
            const int b = (int)(row / n_sel), py = p / nw, px = p - py * nw;
            const RT* src = d_rows + row * ld + k_off + (long long)e * pp;
            const long long* cb = cls + ((long long)b * H + py * ph) * W + px * pw;
            if (pp == 16 && pw == 4) {
                // the 4 x 4 patches of the pre-training recipe: all 16 class ids and the thread's 16 values are requested before the first add
                // (one pixel at a time every add waited for two dependent global loads: 132 us at cfg3 instead of ~20)
                long long cc[16];
                float vv[16];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) cc[i * 4 + j] = cb[(long long)i * W + j];
#pragma unroll
                for (int k = 0; k < 16; ++k) vv[k] = ActT<RT>::ld(src + k);
#pragma unroll
                for (int k = 0; k < 16; ++k)                 // fixed order: pixel 0 .. 15
                    if (cc[k] >= 0 && cc[k] < n_cls) mine[cc[k] * E + e] += vv[k];
            } else {
                for (int i = 0; i < ph; ++i)
                    for (int j = 0; j < pw; ++j) {
                        const long long c = cb[(long long)i * W + j];
                        if (c >= 0 && c < n_cls) mine[c * E + e] += ActT<RT>::ld(src + i * pw + j);
                    }
            }
        }
    }
    __syncthreads();
    float* dst = part + (long long)blockIdx.x * n;
    for (int i = threadIdx.x; i < n; i += 256) {
        float v = tab[i];
        for (int s2 = 1; s2 < nsub; ++s2) v += tab[(long long)s2 * n + i];
        dst[i] = v;
    }
}
__global__ void __launch_bounds__(64) semseg_emb_bwd_sum_kernel(const float* __restrict__ part, float* __restrict__ d_emb, int n, int nparts, int accumulate) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    int g = 0;
    for (; g + 8 <= nparts; g += 8) {                       // eight loads in flight; the adds stay in index order
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = part[(long long)(g + k) * n + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) v += t[k];
    }
    for (; g < nparts; ++g) v += part[(long long)g * n + i];
    d_emb[i] = accumulate ? d_emb[i] + v : v;
}

// tok[b][r][:] = proj[b*n_sel+r][:] + bias_t[:] + pos_t[p][:]   (t = owner of sel[b][r]);
// tok[b][n_sel+g][:] = global[g][:]
struct TaskVecs { const float* bias[MAX_TASKS]; const float* pos[MAX_TASKS]; };

__global__ void __launch_bounds__(256) tokens_assemble_kernel(float* __restrict__ tok, const float* __restrict__ proj, const TaskVecs tv,
                                                              const TaskTable tt, const long long* __restrict__ sel,
                                                              const float* __restrict__ global_tok, int n_sel, int G, int D) {
    const long long rowg = blockIdx.x;               // over B*(n_sel+G)
    const int b = (int)(rowg / (n_sel + G)), r = (int)(rowg % (n_sel + G));
    float* o = tok + rowg * D;
    if (r >= n_sel) {
        const float* gsrc = global_tok + (long long)(r - n_sel) * D;
        for (int c = threadIdx.x * 4; c < D; c += 1024) st4(o + c, ld4(gsrc + c));
        return;
    }
    const int idx = (int)sel[(long long)b * n_sel + r];
    const int t = task_of(tt, idx);
    const float* pr = proj + ((long long)b * n_sel + r) * D;
    const float* bi = tv.bias[t];
    const float* po = tv.pos[t] + (long long)(idx - tt.off[t]) * D;
    for (int c = threadIdx.x * 4; c < D; c += 1024) {
        const f32x4 a = ld4(pr + c), b4 = ld4(bi + c), p4 = ld4(po + c);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = a[j] + b4[j] + p4[j];
        st4(o + c, v);
    }
}

// backward: d_proj (act dtype) = d_tok rows of the kept tokens; per-block partial column sums
// part[blk][t][D] for the T task biases and part[blk][T+g][D] for the global tokens.
template <typename PT>
__global__ void __launch_bounds__(256) tokens_assemble_bwd_kernel(const float* __restrict__ d_tok, PT* __restrict__ d_proj, const TaskTable tt,
                                                                  const long long* __restrict__ sel, float* __restrict__ part, int B,
                                                                  int n_sel, int G, int D) {
    // thread owns columns c = tid*4 + 1024*q (q < 1 for D <= 1024)
    const int c = threadIdx.x * 4;
    f32x4 acc[MAX_TASKS];
#pragma unroll
    for (int i = 0; i < MAX_TASKS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long long n_rows = (long long)B * (n_sel + G);
    // two rows per iteration (two independent 16-byte loads in flight per lane) over up to 1 024 workgroups: with one
    // dependent load per iteration and 99 rows per workgroup this pass ran at 0.4 TB/s
    auto one = [&](long long rowg, const f32x4& v) {
        const int b = (int)(rowg / (n_sel + G)), r = (int)(rowg % (n_sel + G));
        int slot;
        if (r < n_sel) {
            st4(d_proj + ((long long)b * n_sel + r) * D + c, v);
            slot = task_of(tt, (int)sel[(long long)b * n_sel + r]);
        } else slot = tt.T + (r - n_sel);
#pragma unroll
        for (int i = 0; i < MAX_TASKS; ++i) if (i == slot) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += v[j];
        }
    };
    if (c < D) {
        long long rowg = blockIdx.x;
        for (; rowg + gridDim.x < n_rows; rowg += 2LL * gridDim.x) {
            const f32x4 v0 = ld4(d_tok + rowg * D + c), v1 = ld4(d_tok + (rowg + gridDim.x) * D + c);
            one(rowg, v0);
            one(rowg + gridDim.x, v1);
        }
        if (rowg < n_rows) one(rowg, ld4(d_tok + rowg * D + c));
    }
    if (c < D) {
        const int ns = tt.T + G;
#pragma unroll
        for (int i = 0; i < MAX_TASKS; ++i) if (i < ns) st4(part + ((long long)blockIdx.x * ns + i) * D + c, acc[i]);
    }
}

// ------------------------------------------------------------------------------------------
// Decoder query / context builder (output_adapters.py:160-234, use_task_queries path)
// ------------------------------------------------------------------------------------------
// one task-embedding row per INPUT task, by pointer (NULL = that task has none: zeros) -- the rows live wherever the parameters do,
// no staging copy (round 3 issued one hipMemcpyAsync per task and adapter: 12 of a cfg3 step's 91 copyBuffer launches)
struct TePtrs { const float* p[MAX_TASKS]; };
// query_norm / context_norm of the adapter (output_adapters.py:120-122, applied at :259-260) folded into the build (round 5): at D <= 256 a
// wave owns a whole row -- one float4 per lane -- so the LayerNorm of the row it has just assembled is two wave reductions and one more
// store, instead of two further launches that re-read 76 MB.  The arithmetic is ln_fwd_kernel<1>'s, operation for operation.
// (struct BuildLn: common.h)

template <typename YT>
__device__ __forceinline__ void build_ln_row(const f32x4 v, bool has, int c, int D, float eps, const float* __restrict__ g, const float* __restrict__ b,
                                              YT* __restrict__ yrow, float* __restrict__ mean, float* __restrict__ rstd, long long row, int lane) {
    const float s = has ? (v[0] + v[1]) + (v[2] + v[3]) : 0.f;
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
    if (has) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = v[j] - mu; q += d * d; }
    }
    const float var = wave_sum(q) / (float)D;
    const float rs = 1.0f / sqrtf(var + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    if (has) {
        const f32x4 g4 = ld4(g + c), b4 = ld4(b + c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[j] - mu) * rs * g4[j] + b4[j];
        st4(yrow + c, o);
    }
}

template <typename YT, bool LN>
__global__ void __launch_bounds__(256) decoder_build_kernel(const float* __restrict__ ctx, const long long* __restrict__ ids_keep,
                                                            const long long* __restrict__ ids_restore, const float* __restrict__ mask_token,
                                                            const TePtrs tep, const float* __restrict__ pos, const TaskTable tt,
                                                            int q_task, int n_keep, int G, int D, int n_q, int Ntot,
                                                            float* __restrict__ queries, float* __restrict__ context, long long total_rows,
                                                            const BuildLn ln) {
    // a row per group of `lpr` lanes: four rows per workgroup at the decoders' D = 256 (one workgroup per 1 KB row with 192 idle lanes, as
    // built in round 1, ran at 2.4 TB/s: every row is two dependent round trips -- index, then data)
    const int lpr = D <= 256 ? 64 : (D <= 512 ? 128 : 256);
    const int rows_per_b = n_q + n_keep + G;
    const long long grow = (long long)blockIdx.x * (256 / lpr) + threadIdx.x / lpr;
    if (grow >= total_rows) return;                              // (the grid is rounded up to whole workgroups)
    const int b = (int)(grow / rows_per_b), rr = (int)(grow % rows_per_b);
    const int tl = threadIdx.x % lpr, cstep = lpr * 4;
    const int NC = n_keep + G;
    if (rr < n_q) {
        const int j = rr;
        // q_task < 0: pure mask-token queries (output_adapters.py:213-220: the task is not among the encoder inputs, or
        // use_task_queries=False): mask_token + pos[j]; the optional task embedding of the adapter's own task is folded into
        // the mask_token vector the caller passes (it is added to every query row, exactly like the mask token)
        const long long rank = q_task < 0 ? (long long)n_keep : ids_restore[(long long)b * Ntot + tt.off[q_task] + j];
        const float* base = (rank < n_keep) ? ctx + ((long long)b * NC + rank) * D : mask_token;
        const float* te = q_task < 0 ? nullptr : tep.p[q_task];
        const float* pe = pos + (long long)j * D;
        float* o = queries + ((long long)b * n_q + j) * D;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int c = tl * 4; c < D; c += cstep) {
            const f32x4 a = ld4(base + c), t4 = te ? ld4(te + c) : f32x4{0.f, 0.f, 0.f, 0.f}, p4 = ld4(pe + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = a[k] + (t4[k] + p4[k]);
            st4(o + c, v);
        }
        if (LN) {                                        // D <= 256: lpr = 64, the loop above ran at most once
            const long long row = (long long)b * n_q + j;
            build_ln_row<YT>(v, tl * 4 < D, tl * 4, D, ln.eps, ln.qg, ln.qb, (YT*)ln.qn + row * D, ln.qmean, ln.qrstd, row, tl);
        }
    } else {
        const int r = rr - n_q;
        const float* src = ctx + ((long long)b * NC + r) * D;
        float* o = context + ((long long)b * NC + r) * D;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r >= n_keep) {                               // global tokens: copied as they are
            for (int c = tl * 4; c < D; c += cstep) { v = ld4(src + c); st4(o + c, v); }
        } else {
            const int idx = (int)ids_keep[(long long)b * n_keep + r];
            const int t = task_of(tt, idx);
            const float* te = tep.p[t];
            const float* pe = pos + (long long)(idx - tt.off[t]) * D;
            for (int c = tl * 4; c < D; c += cstep) {
                const f32x4 a = ld4(src + c), t4 = te ? ld4(te + c) : f32x4{0.f, 0.f, 0.f, 0.f}, p4 = ld4(pe + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = a[k] + (t4[k] + p4[k]);
                st4(o + c, v);
            }
        }
        if (LN) {
            const long long row = (long long)b * NC + r;
            build_ln_row<YT>(v, tl * 4 < D, tl * 4, D, ln.eps, ln.cg, ln.cb, (YT*)ln.cn + row * D, ln.cmean, ln.crstd, row, tl);
        }
    }
}

// backward.  Workgroup per sample-chunk; thread owns 4 columns.  d_ctx rows are each written
// exactly once (kept row r: d_context[r] + d_queries[its query] if the query task owns it).
__global__ void __launch_bounds__(256) decoder_build_bwd_kernel(const float* __restrict__ d_queries, const float* __restrict__ d_context,
                                                                const long long* __restrict__ ids_keep, const long long* __restrict__ ids_restore,
                                                                const TaskTable tt, int q_task, int B, int n_keep, int G, int D, int n_q,
                                                                int Ntot, float* __restrict__ d_ctx, float* __restrict__ part) {
    // D / 4 lanes cover a row; the workgroup's 256 / (D / 4) lane groups ("phases") and the SPLIT workgroups of a sample take
    // the sample's NC + n_q rows round-robin (one 64-lane group walking all 295 rows of a sample was pure latency: 154 us
    // for 100 MB); phases are combined through LDS, workgroups through the caller's column-sum pass over part.
    __shared__ f32x4 red[4][MAX_TASKS + 1][64];
    const int cg = D >> 2;                                // lanes per row
    const int phases = (cg <= 64) ? 4 : 1;
    const int ph = threadIdx.x / cg, lane = threadIdx.x % cg;
    const int c = lane * 4;
    const int NC = n_keep + G;
    const int split = gridDim.y;
    f32x4 acc[MAX_TASKS + 1];
#pragma unroll
    for (int i = 0; i <= MAX_TASKS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ph < phases) {
        const int stride = phases * split, first = blockIdx.y * phases + ph;
        for (int b = blockIdx.x; b < B; b += gridDim.x) {
            for (int rr = first; rr < NC + n_q; rr += stride) {
                if (rr < NC) {                            // context row
                    const int r = rr;
                    f32x4 v = ld4(d_context + ((long long)b * NC + r) * D + c);
                    if (r < n_keep) {
                        const int idx = (int)ids_keep[(long long)b * n_keep + r];
                        const int t = task_of(tt, idx);
#pragma unroll
                        for (int i = 0; i < MAX_TASKS; ++i) if (i == t) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[i][k] += v[k];
                        }
                        if (t == q_task) {
                            const f32x4 q = ld4(d_queries + ((long long)b * n_q + (idx - tt.off[t])) * D + c);
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[k] += q[k];
                        }
                    }
                    st4(d_ctx + ((long long)b * NC + r) * D + c, v);
                } else {                                  // query row: task embedding of the query task + mask token of the masked ones
                    const int j = rr - NC;
                    const f32x4 q = ld4(d_queries + ((long long)b * n_q + j) * D + c);
                    const bool vis = q_task >= 0 && ids_restore[(long long)b * Ntot + tt.off[q_task] + j] < n_keep;     // q_task < 0: every query row is mask_token + pos
#pragma unroll
                    for (int i = 0; i < MAX_TASKS; ++i) if (i == q_task) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[i][k] += q[k];
                    }
                    if (!vis) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[MAX_TASKS][k] += q[k];
                    }
                }
            }
        }
    }
    const int ns = tt.T + 1;
    const long long prow = (long long)blockIdx.y * gridDim.x + blockIdx.x;          // this workgroup's row of part
    if (phases == 1) {
        if (ph == 0) {
#pragma unroll
            for (int i = 0; i < MAX_TASKS; ++i) if (i < tt.T) st4(part + (prow * ns + i) * D + c, acc[i]);
            st4(part + (prow * ns + tt.T) * D + c, acc[MAX_TASKS]);
        }
        return;
    }
    if (ph < phases) {
#pragma unroll
        for (int i = 0; i <= MAX_TASKS; ++i) red[ph][i][lane] = acc[i];
    }
    __syncthreads();
    if (ph == 0) {
#pragma unroll
        for (int i = 0; i <= MAX_TASKS; ++i) {
            if (i < tt.T || i == MAX_TASKS) {
                f32x4 t = red[0][i][lane];
                for (int p = 1; p < phases; ++p) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) t[k] += red[p][i][lane][k];
                }
                st4(part + (prow * ns + (i == MAX_TASKS ? tt.T : i)) * D + c, t);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// 'b (nh nw) (c ph pw) -> b c (nh ph) (nw pw)' and back.  Thread per image pixel-run of pw.
// ------------------------------------------------------------------------------------------
__global__ void unpatchify_kernel(const float* __restrict__ pat, float* __restrict__ img, int C, int nh, int nw, int ph, int pw,
                                  long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over B*C*H*W
    if (i >= total) return;
    const int W = nw * pw, H = nh * ph;
    const int x = (int)(i % W); long long r = i / W;
    const int y = (int)(r % H); r /= H;
    const int c = (int)(r % C); const long long b = r / C;
    const int py = y / ph, iy = y % ph, px = x / pw, ix = x % pw;
    img[i] = pat[((b * nh + py) * nw + px) * ((long long)C * ph * pw) + ((long long)c * ph + iy) * pw + ix];
}
template <typename PT>
__global__ void patchify_kernel(const float* __restrict__ img, PT* __restrict__ pat, long long ld, int C, int nh, int nw, int ph, int pw,
                                long long total) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over B*N*(C*ph*pw)
    if (o >= total) return;
    const int KP = C * ph * pw;
    const int k = (int)(o % KP); long long r = o / KP;
    const int px = (int)(r % nw); r /= nw;
    const int py = (int)(r % nh); const long long b = r / nh;
    const int c = k / (ph * pw), iy = (k / pw) % ph, ix = k % pw;
    const int W = nw * pw, H = nh * ph;
    ActT<PT>::st(pat + (o / KP) * ld + k, img[((b * C + c) * H + py * ph + iy) * W + px * pw + ix]);
}

// pw % 4 == 0 fast paths: one thread per 4 consecutive pixels of a patch row, walking the PATCH layout (so the patch side is
// one fully coalesced stream and the image side moves in whole pw-pixel runs: 64-byte segments for 16-pixel patches, 16-byte
// ones merged by L2 for the 4-pixel semseg patches).  The scalar kernels above (a div/mod chain per pixel) ran at 1.3-1.9 TB/s.
__global__ void __launch_bounds__(256) unpatchify4_kernel(const float* __restrict__ pat, float* __restrict__ img, int C, int nh, int nw,
                                                          int ph, int pw, long long total4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // float4 index in patch layout [b][py][px][c][iy][q]
    if (i >= total4) return;
    const int qn = pw >> 2;
    const int q = (int)(i % qn); long long r = i / qn;
    const int iy = (int)(r % ph); r /= ph;
    const int c = (int)(r % C); r /= C;
    const int px = (int)(r % nw); r /= nw;
    const int py = (int)(r % nh); const long long b = r / nh;
    const int W = nw * pw, H = nh * ph;
    st4(img + ((b * C + c) * H + py * ph + iy) * W + px * pw + q * 4, ld4(pat + i * 4));
}
template <typename PT>
__global__ void __launch_bounds__(256) patchify4_kernel(const float* __restrict__ img, PT* __restrict__ pat, long long ld, int C, int nh,
                                                        int nw, int ph, int pw, long long total4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int qn = pw >> 2;
    const int q = (int)(i % qn); long long r = i / qn;
    const int iy = (int)(r % ph); r /= ph;
    const int c = (int)(r % C); r /= C;
    const long long tok = r;                                                  // b * nh * nw + py * nw + px
    const int px = (int)(r % nw); r /= nw;
    const int py = (int)(r % nh); const long long b = r / nh;
    const int W = nw * pw, H = nh * ph;
    st4(pat + tok * ld + ((long long)c * ph + iy) * pw + q * 4, ld4(img + ((b * C + c) * H + py * ph + iy) * W + px * pw + q * 4));
}

// Narrow patches (pw = 4 or 8: the stride-4 semseg maps): a 16-byte patch-row chunk is a quarter / half of a 64-byte
// sector, and the walk of the kernels above touches the other chunks of that sector from workgroups far apart -- PMC: 2.4 GB
// fetched for a 427 MB logits gradient.  Here a workgroup moves one (sample, patch row, channel block) tile through LDS:
// whole image rows on one side, whole per-token channel blocks on the other; every global access is a full contiguous run.
template <typename PT, bool TO_PATCH>
__global__ void __launch_bounds__(256) patch_tile_kernel(const float* __restrict__ src, PT* __restrict__ dst, long long ld, int C, int nh,
                                                         int nw, int ph, int pw, int CB) {
    extern __shared__ __attribute__((aligned(16))) float tile[];              // [CB][ph][W]
    const int W = nw * pw, H = nh * ph, ncb = (C + CB - 1) / CB;
    const int cb = blockIdx.x % ncb; long long r = blockIdx.x / ncb;
    const int py = (int)(r % nh); const long long b = r / nh;
    const int c0 = cb * CB, cn = (C - c0 < CB) ? C - c0 : CB;
    const int rowW4 = W >> 2, pw4 = pw >> 2;
    const int n_img4 = cn * ph * rowW4;                                       // float4 chunks on the image side (= patch side)
    if (TO_PATCH) {
        for (int e = threadIdx.x; e < n_img4; e += 256) {                     // image rows -> LDS (contiguous W-float runs)
            const int x4 = e % rowW4, rr = e / rowW4, iy = rr % ph, cl = rr / ph;
            *reinterpret_cast<f32x4*>(tile + (cl * ph + iy) * W + x4 * 4) = ld4(src + ((b * C + c0 + cl) * H + py * ph + iy) * W + x4 * 4);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n_img4; e += 256) {                     // LDS -> per-token channel blocks (contiguous cn*ph*pw floats)
            const int q = e % pw4; int rr = e / pw4;
            const int iy = rr % ph; rr /= ph;
            const int cl = rr % cn, px = rr / cn;
            const f32x4 v = *reinterpret_cast<const f32x4*>(tile + (cl * ph + iy) * W + px * pw + q * 4);
            st4(dst + ((b * nh + py) * nw + px) * ld + ((long long)(c0 + cl) * ph + iy) * pw + q * 4, v);
        }
    } else {
        for (int e = threadIdx.x; e < n_img4; e += 256) {                     // patch rows -> LDS
            const int q = e % pw4; int rr = e / pw4;
            const int iy = rr % ph; rr /= ph;
            const int cl = rr % cn, px = rr / cn;
            *reinterpret_cast<f32x4*>(tile + (cl * ph + iy) * W + px * pw + q * 4) =
                ld4(src + ((b * nh + py) * nw + px) * ld + ((long long)(c0 + cl) * ph + iy) * pw + q * 4);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < n_img4; e += 256) {                     // LDS -> image rows
            const int x4 = e % rowW4, rr = e / rowW4, iy = rr % ph, cl = rr / ph;
            st4(dst + ((b * C + c0 + cl) * H + py * ph + iy) * W + x4 * 4, *reinterpret_cast<const f32x4*>(tile + (cl * ph + iy) * W + x4 * 4));
        }
    }
}
// channels per tile: <= 16, LDS tile <= 32 KB
inline int patch_tile_cb(int ph, int W) { int cb = 8192 / (ph * W); return cb < 1 ? 0 : (cb > 16 ? 16 : cb); }

// hardware probe: what does ds_read_b64_tr_b16 return for a given LDS image / lane addresses
// SemSegInputAdapter(interpolate_class_emb=True), input_adapters.py:192-198: nn.Upsample(scale 1 / patch, bilinear) of the
// class-embedding image = per token the mean of the centre taps (even patch: the 2 x 2 centre pixels, odd: the centre pixel;
// src = (dst + 0.5) * patch - 0.5).  out f32 [B][E][nh][nw]; class ids outside [0, n_cls) embed as zeros.
__device__ __forceinline__ void centre_taps(int i, int p, int& t0, int& t1) {
    if (p & 1) { t0 = t1 = i * p + p / 2; } else { t0 = i * p + p / 2 - 1; t1 = t0 + 1; }
}
__global__ void __launch_bounds__(256) semseg_avg_emb_fwd_kernel(const long long* __restrict__ x, const float* __restrict__ emb, float* __restrict__ out,
                                                                 int B, int H, int W, int E, int ph, int pw, int n_cls) {
    const int nh = H / ph, nw = W / pw;
    const long long total = (long long)B * E * nh * nw;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int j = (int)(idx % nw), i = (int)((idx / nw) % nh), e = (int)((idx / ((long long)nw * nh)) % E), b = (int)(idx / ((long long)nw * nh * E));
        int r0, r1, c0, c1;
        centre_taps(i, ph, r0, r1); centre_taps(j, pw, c0, c1);
        const long long* xb = x + (long long)b * H * W;
        float acc = 0.f;
        const int rr[2] = {r0, r1}, cc[2] = {c0, c1};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long cls = xb[(long long)rr[a] * W + cc[c]];
                if (cls >= 0 && cls < n_cls) acc += 0.25f * emb[cls * E + e];
            }
        out[idx] = acc;
    }
}
// its gradient: d_emb[class of every tap][e] += 0.25 * d_img[b][e][i][j] (float atomics); pad_idx (nn.Embedding's padding_idx) gets none
__global__ void __launch_bounds__(256) semseg_avg_emb_bwd_kernel(const float* __restrict__ d_img, const long long* __restrict__ x, float* __restrict__ d_emb,
                                                                 int B, int H, int W, int E, int ph, int pw, int n_cls, int pad_idx) {
    const int nh = H / ph, nw = W / pw;
    const long long total = (long long)B * E * nh * nw;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int j = (int)(idx % nw), i = (int)((idx / nw) % nh), e = (int)((idx / ((long long)nw * nh)) % E), b = (int)(idx / ((long long)nw * nh * E));
        int r0, r1, c0, c1;
        centre_taps(i, ph, r0, r1); centre_taps(j, pw, c0, c1);
        const long long* xb = x + (long long)b * H * W;
        const float gq = 0.25f * d_img[idx];
        const int rr[2] = {r0, r1}, cc[2] = {c0, c1};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long cls = xb[(long long)rr[a] * W + cc[c]];
                if (cls >= 0 && cls < n_cls && cls != pad_idx) atomicAdd(d_emb + cls * E + e, gq);
            }
    }
}
// Gradient of an image-like input of the patch embedding: the selected tokens' row gradients d_rows (f32 [B * n_sel][ldr], this
// task's K = C * ph * pw columns starting at k_off) back into d_img f32 [B][C][H][W] (zeroed by the caller; patches are disjoint).
__global__ void __launch_bounds__(256) rows_to_image_kernel(const float* __restrict__ d_rows, long long ldr, int k_off, const long long* __restrict__ sel,
                                                            float* __restrict__ d_img, int n_sel, long long tok_off, int n_patches, int C, int H, int W,
                                                            int ph, int pw) {
    const int row = blockIdx.x, b = row / n_sel;
    const long long p = sel[row] - tok_off;
    if (p < 0 || p >= n_patches) return;
    const int nw = W / pw, pi = (int)(p / nw), pj = (int)(p % nw), K = C * ph * pw;
    for (int k = threadIdx.x; k < K; k += 256) {
        const int c = k / (ph * pw), di = (k / pw) % ph, dj = k % pw;
        d_img[(((long long)b * C + c) * H + pi * ph + di) * W + pj * pw + dj] = d_rows[(long long)row * ldr + k_off + k];
    }
}

// Gradient of learnable positional embeddings (input_adapters.py:75-78 with learnable_pos_emb=True): token (b, j) carries the
// embedding of position sel[b][j] (task offsets included), so d_pos[sel[b][j]] += d_tok[b][j].  One wave per selected token,
// float atomics (order-dependent in the last bit, like semseg_emb_bwd).
__global__ void pos_emb_bwd_kernel(const float* __restrict__ d_tok, const long long* __restrict__ sel, float* __restrict__ d_pos,
                                   int n_sel, int G, int D, int n_pos) {
    const int row = blockIdx.x, b = row / n_sel, j = row - b * n_sel;
    const long long p = sel[row];
    if (p < 0 || p >= n_pos) return;
    const float* src = d_tok + ((long long)b * (n_sel + G) + j) * D;
    float* dst = d_pos + p * D;
    for (int c = threadIdx.x * 4; c < D; c += 256) {
        const f32x4 v = ld4(src + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(dst + c + k, v[k]);
    }
}

__global__ void probe_tr16_kernel(const uint16_t* __restrict__ image, const uint32_t* __restrict__ addr, uint16_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[1024];
    for (int i = threadIdx.x; i < 1024; i += 64) lds[i] = image[i];
    __syncthreads();
    const char* p = (const char*)lds + addr[threadIdx.x];
    s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[threadIdx.x * 4 + j] = (uint16_t)v[j];
}

int fill_tt(TaskTable& tt, const int32_t* off_host, int T) {
    if (T < 1 || T > MAX_TASKS) return -1;
    tt.T = T;
    for (int i = 0; i <= MAX_TASKS; ++i) tt.off[i] = off_host[i <= T ? i : T];
    return 0;
}

}  // namespace

extern "C" {

int mmae_mask_sample(const int64_t* samples_per_task, const float* task_noise, const float* all_noise,
                     const int32_t* task_offsets_host, int T, int B, int Ntot, int n_keep, int64_t* mask_all,
                     int64_t* ids_keep, int64_t* ids_restore, void* stream) {
    MMAE_REQUIRE(samples_per_task && task_noise && all_noise && task_offsets_host && mask_all && ids_keep && ids_restore,
                 "mask_sample: null pointer");
    TaskTable tt;
    MMAE_REQUIRE(fill_tt(tt, task_offsets_host, T) == 0, "mask_sample: 1 <= T <= 8");
    MMAE_REQUIRE(B > 0 && Ntot > 0 && Ntot <= 8192 && n_keep >= 0 && n_keep <= Ntot && tt.off[T] == Ntot, "mask_sample: bad sizes");
    hipLaunchKernelGGL(mask_sample_kernel, dim3(B), dim3(256), (size_t)Ntot * 8, (hipStream_t)stream,
                       (const long long*)samples_per_task, task_noise, all_noise, tt, Ntot, n_keep, (long long*)mask_all,
                       (long long*)ids_keep, (long long*)ids_restore);
    return mmae_check_launch("mask_sample");
}

int mmae_patch_rows(const mmae_patch_src* srcs, const int32_t* task_offsets_host, int T, const int64_t* sel, void* rows,
                    int rows_dtype, int B, int n_sel, int Ktot, void* stream) {
    MMAE_REQUIRE(srcs && task_offsets_host && sel && rows && B > 0 && n_sel > 0 && Ktot > 0, "patch_rows: bad argument");
    TaskTable tt;
    MMAE_REQUIRE(fill_tt(tt, task_offsets_host, T) == 0, "patch_rows: 1 <= T <= 8");
    if (rows_dtype != MMAE_BF16 && rows_dtype != MMAE_F32) { mmae_set_error("patch_rows: bf16 / f32 rows"); return MMAE_ESUPPORT; }
    PatchSrcs ps;
    for (int t = 0; t < MAX_TASKS; ++t) {
        const mmae_patch_src& s = srcs[t < T ? t : 0];
        MMAE_REQUIRE(s.data && s.ph > 0 && s.pw > 0 && s.H % s.ph == 0 && s.W % s.pw == 0, "patch_rows: bad source");
        MMAE_REQUIRE(s.kind == 0 || s.emb, "patch_rows: semseg source needs the class embedding");
        MMAE_REQUIRE((s.H / s.ph) * (s.W / s.pw) == tt.off[(t < T ? t : 0) + 1] - tt.off[t < T ? t : 0], "patch_rows: patch count != task tokens");
        ps.s[t] = PatchSrc{s.data, s.emb, s.kind, s.C, s.H, s.W, s.ph, s.pw, s.k_off, s.C * s.ph * s.pw, s.n_cls};
    }
    const long long n_rows = (long long)B * n_sel;
    hipStream_t st = (hipStream_t)stream;
    if (rows_dtype == MMAE_BF16) hipLaunchKernelGGL((patch_rows_kernel<uint16_t>), dim3((unsigned)n_rows), dim3(256), 0, st, ps, tt, (const long long*)sel, (uint16_t*)rows, n_rows, n_sel, Ktot);
    else hipLaunchKernelGGL((patch_rows_kernel<float>), dim3((unsigned)n_rows), dim3(256), 0, st, ps, tt, (const long long*)sel, (float*)rows, n_rows, n_sel, Ktot);
    return mmae_check_launch("patch_rows");
}

int mmae_semseg_emb_bwd(const void* d_rows, int rows_dtype, int64_t ld, const int64_t* cls, const int64_t* sel, float* d_emb,
                        int B, int H, int W, int E, int ph, int pw, int n_sel, int k_off, int tok_off, int n_patches, int n_cls,
                        void* stream) {
    MMAE_REQUIRE(d_rows && cls && sel && d_emb && B > 0 && n_cls > 0 && E > 0, "semseg_emb_bwd: bad argument");
    if (rows_dtype != MMAE_BF16 && rows_dtype != MMAE_F32) { mmae_set_error("semseg_emb_bwd: bf16 / f32 rows"); return MMAE_ESUPPORT; }
    const long long n_rows = (long long)B * n_sel;
    const int grid = (int)(n_rows < 512 ? n_rows : 512);
    const size_t lds = (size_t)n_cls * E * 4;
    hipStream_t st = (hipStream_t)stream;                  // (a table beyond the LDS is refused by the launch)
    if (rows_dtype == MMAE_BF16)
        return mmae_launch_lds<semseg_emb_bwd_kernel<uint16_t>>(dim3(grid), dim3(256), lds, st, "semseg_emb_bwd", (const uint16_t*)d_rows, (long long)ld, (const long long*)cls, (const long long*)sel, d_emb, n_rows, n_sel, H, W, E, ph, pw, k_off, tok_off, n_patches, n_cls);
    return mmae_launch_lds<semseg_emb_bwd_kernel<float>>(dim3(grid), dim3(256), lds, st, "semseg_emb_bwd", (const float*)d_rows, (long long)ld, (const long long*)cls, (const long long*)sel, d_emb, n_rows, n_sel, H, W, E, ph, pw, k_off, tok_off, n_patches, n_cls);
}

// deterministic form: ws f32 [mmae_semseg_emb_bwd_ws_elems()] scratch; accumulate = 0 stores the gradient (no zero-fill of d_emb needed), 1 adds
static int semseg_det_geometry(int B, int n_sel, int E, int n_cls, int* nsub_out, int* rows_per_out) {
    if (B <= 0 || n_sel <= 0 || E < 1 || E > 256 || n_cls < 1) return -1;      // (no rows: rows_per would be 0)
    int nsub = 256 / E;
    const long long tab = (long long)n_cls * E * 4;
    while (nsub > 1 && nsub * tab > 150 * 1024) --nsub;
    if (nsub * tab > (long long)MMAE_LDS_BYTES) return -1;
    const long long n_rows = (long long)B * n_sel;
    int grid = (int)(n_rows < 256 ? n_rows : 256);
    if (grid < 1) grid = 1;
    *nsub_out = nsub;
    *rows_per_out = (int)((n_rows + grid - 1) / grid);
    return (int)((n_rows + *rows_per_out - 1) / *rows_per_out);
}
int64_t mmae_semseg_emb_bwd_ws_elems(int B, int n_sel, int E, int n_cls) {
    int nsub, rows_per;
    const int grid = semseg_det_geometry(B, n_sel, E, n_cls, &nsub, &rows_per);
    return grid < 0 ? -1 : (int64_t)grid * n_cls * E;
}
int mmae_semseg_emb_bwd_det(const void* d_rows, int rows_dtype, int64_t ld, const int64_t* cls, const int64_t* sel, float* d_emb,
                            int B, int H, int W, int E, int ph, int pw, int n_sel, int k_off, int tok_off, int n_patches, int n_cls,
                            float* ws, int64_t ws_elems, int accumulate, void* stream) {
    MMAE_REQUIRE(d_rows && cls && sel && d_emb && ws && B > 0 && n_cls > 0 && E > 0, "semseg_emb_bwd_det: bad argument");
    int nsub, rows_per;
    const int grid = semseg_det_geometry(B, n_sel, E, n_cls, &nsub, &rows_per);
    if (grid < 0) { mmae_set_error("semseg_emb_bwd_det: embedding table exceeds LDS / E > 256 / no rows"); return MMAE_ESUPPORT; }
    MMAE_REQUIRE(ws_elems >= (int64_t)grid * n_cls * E, "semseg_emb_bwd_det: workspace too small (mmae_semseg_emb_bwd_ws_elems)");
    const long long n_rows = (long long)B * n_sel;
    const size_t lds = (size_t)nsub * n_cls * E * 4;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (rows_dtype == MMAE_BF16)
        rc = mmae_launch_lds<semseg_emb_bwd_part_kernel<uint16_t>>(dim3(grid), dim3(256), lds, st, "semseg_emb_bwd_part", (const uint16_t*)d_rows, (long long)ld, (const long long*)cls, (const long long*)sel, ws, n_rows, rows_per, n_sel, H, W, E, ph, pw, k_off, tok_off, n_patches, n_cls, nsub);
    else if (rows_dtype == MMAE_F32)
        rc = mmae_launch_lds<semseg_emb_bwd_part_kernel<float>>(dim3(grid), dim3(256), lds, st, "semseg_emb_bwd_part", (const float*)d_rows, (long long)ld, (const long long*)cls, (const long long*)sel, ws, n_rows, rows_per, n_sel, H, W, E, ph, pw, k_off, tok_off, n_patches, n_cls, nsub);
    else { mmae_set_error("semseg_emb_bwd_det: bf16 / f32 rows"); return MMAE_ESUPPORT; }
    if (rc) return rc;
    const int n = n_cls * E;
    hipLaunchKernelGGL(semseg_emb_bwd_sum_kernel, dim3((n + 63) / 64), dim3(64), 0, st, (const float*)ws, d_emb, n, grid, accumulate);
    return mmae_check_launch("semseg_emb_bwd_sum");
}

int mmae_tokens_assemble(float* tok, const float* proj, const float* const* bias, const float* const* pos,
                         const int32_t* task_offsets_host, int T, const int64_t* sel, const float* global_tok, int B, int n_sel,
                         int G, int D, void* stream) {
    MMAE_REQUIRE(tok && proj && bias && pos && sel && (G == 0 || global_tok), "tokens_assemble: null pointer");
    MMAE_REQUIRE(D % 4 == 0 && D <= 1024 && B > 0 && n_sel > 0 && G >= 0, "tokens_assemble: bad sizes");
    TaskTable tt;
    MMAE_REQUIRE(fill_tt(tt, task_offsets_host, T) == 0, "tokens_assemble: 1 <= T <= 8");
    TaskVecs tv;
    for (int t = 0; t < MAX_TASKS; ++t) { tv.bias[t] = bias[t < T ? t : 0]; tv.pos[t] = pos[t < T ? t : 0]; }
    hipLaunchKernelGGL(tokens_assemble_kernel, dim3((unsigned)((long long)B * (n_sel + G))), dim3(256), 0, (hipStream_t)stream, tok,
                       proj, tv, tt, (const long long*)sel, global_tok, n_sel, G, D);
    return mmae_check_launch("tokens_assemble");
}

int mmae_tokens_assemble_bwd_nblk(int B) { const long long n = 4LL * B; return (int)(n < 1024 ? n : 1024); }

int mmae_tokens_assemble_bwd(const float* d_tok, void* d_proj, int proj_dtype, const int32_t* task_offsets_host, int T,
                             const int64_t* sel, float* part, int B, int n_sel, int G, int D, void* stream) {
    MMAE_REQUIRE(d_tok && d_proj && sel && part, "tokens_assemble_bwd: null pointer");
    MMAE_REQUIRE(D % 4 == 0 && D <= 1024 && T + G <= MAX_TASKS, "tokens_assemble_bwd: bad sizes");
    TaskTable tt;
    MMAE_REQUIRE(fill_tt(tt, task_offsets_host, T) == 0, "tokens_assemble_bwd: 1 <= T <= 8");
    const int nblk = mmae_tokens_assemble_bwd_nblk(B);
    hipStream_t st = (hipStream_t)stream;
    if (proj_dtype == MMAE_BF16) hipLaunchKernelGGL((tokens_assemble_bwd_kernel<uint16_t>), dim3(nblk), dim3(256), 0, st, d_tok, (uint16_t*)d_proj, tt, (const long long*)sel, part, B, n_sel, G, D);
    else hipLaunchKernelGGL((tokens_assemble_bwd_kernel<float>), dim3(nblk), dim3(256), 0, st, d_tok, (float*)d_proj, tt, (const long long*)sel, part, B, n_sel, G, D);
    return mmae_check_launch("tokens_assemble_bwd");
}

}  // extern "C"
// the same with the task-embedding rows given one by one (device pointers, NULL = zeros); used by mmae_adapter_fwd
// ln (optional, D <= 256): also the adapter's query_norm / context_norm of the rows -- outputs in act dtype `ln_dtype` + row statistics
int mmae_decoder_build_rows_ln(const float* ctx, const int64_t* ids_keep, const int64_t* ids_restore, const float* mask_token,
                               const float* const* task_emb_rows, const float* pos, const int32_t* task_offsets_host, int T, int q_task, int B,
                               int n_keep, int G, int D, int n_q, float* queries, float* context, const BuildLn* ln, int ln_dtype, void* stream);
int mmae_decoder_build_rows(const float* ctx, const int64_t* ids_keep, const int64_t* ids_restore, const float* mask_token,
                            const float* const* task_emb_rows, const float* pos, const int32_t* task_offsets_host, int T, int q_task, int B,
                            int n_keep, int G, int D, int n_q, float* queries, float* context, void* stream) {
    return mmae_decoder_build_rows_ln(ctx, ids_keep, ids_restore, mask_token, task_emb_rows, pos, task_offsets_host, T, q_task, B, n_keep, G, D, n_q,
                                      queries, context, nullptr, MMAE_F32, stream);
}
int mmae_decoder_build_rows_ln(const float* ctx, const int64_t* ids_keep, const int64_t* ids_restore, const float* mask_token,
                               const float* const* task_emb_rows, const float* pos, const int32_t* task_offsets_host, int T, int q_task, int B,
                               int n_keep, int G, int D, int n_q, float* queries, float* context, const BuildLn* ln, int ln_dtype, void* stream) {
    MMAE_REQUIRE(ctx && ids_keep && ids_restore && mask_token && task_emb_rows && pos && queries && context, "decoder_build: null pointer");
    MMAE_REQUIRE(D % 4 == 0 && D <= 1024 && B > 0, "decoder_build: bad sizes");
    TaskTable tt;
    MMAE_REQUIRE(fill_tt(tt, task_offsets_host, T) == 0 && q_task >= -1 && q_task < T, "decoder_build: bad task table");
    MMAE_REQUIRE(n_q > 0 && (q_task < 0 || tt.off[q_task + 1] - tt.off[q_task] == n_q), "decoder_build: n_q != tokens of the query task");
    TePtrs tep = {};
    for (int t = 0; t < T; ++t) {
        MMAE_REQUIRE(((uintptr_t)task_emb_rows[t] % 16) == 0, "decoder_build: unaligned task embedding");
        tep.p[t] = task_emb_rows[t];
    }
    const int rpw = D <= 256 ? 4 : (D <= 512 ? 2 : 1);
    const long long total_rows = (long long)B * (n_q + n_keep + G);
    const dim3 grid((unsigned)((total_rows + rpw - 1) / rpw));
    hipStream_t st = (hipStream_t)stream;
    const BuildLn none = {};
#define DB_LAUNCH(YT, LN, L) hipLaunchKernelGGL((decoder_build_kernel<YT, LN>), grid, dim3(256), 0, st, ctx, (const long long*)ids_keep, \
                       (const long long*)ids_restore, mask_token, tep, pos, tt, q_task, n_keep, G, D, n_q, tt.off[T], queries, context, total_rows, L)
    if (ln) {
        MMAE_REQUIRE(D <= 256 && ln->qg && ln->qb && ln->cg && ln->cb && ln->qn && ln->cn && ln->qmean && ln->qrstd && ln->cmean && ln->crstd,
                     "decoder_build: the fused LayerNorm needs D <= 256 and every output");
        if (ln_dtype == MMAE_BF16) DB_LAUNCH(uint16_t, true, *ln);
        else if (ln_dtype == MMAE_F16) DB_LAUNCH(h16_t, true, *ln);
        else DB_LAUNCH(float, true, *ln);
    } else DB_LAUNCH(float, false, none);
#undef DB_LAUNCH
    return mmae_check_launch("decoder_build");
}
extern "C" {

int mmae_decoder_build(const float* ctx, const int64_t* ids_keep, const int64_t* ids_restore, const float* mask_token,
                       const float* task_emb, const float* pos, const int32_t* task_offsets_host, int T, int q_task, int B,
                       int n_keep, int G, int D, int n_q, float* queries, float* context, void* stream) {
    MMAE_REQUIRE(task_emb && T >= 1 && T <= MAX_TASKS, "decoder_build: null task embedding table / bad task count");
    const float* rows[MAX_TASKS];
    for (int t = 0; t < T; ++t) rows[t] = task_emb + (long long)t * D;
    return mmae_decoder_build_rows(ctx, ids_keep, ids_restore, mask_token, rows, pos, task_offsets_host, T, q_task, B, n_keep, G, D, n_q,
                                   queries, context, stream);
}

static int dbb_split(int B) { return B <= 512 ? 4 : 1; }
int mmae_decoder_build_bwd_nblk(int B) { return (B < 1024 ? B : 1024) * dbb_split(B); }

int mmae_decoder_build_bwd(const float* d_queries, const float* d_context, const int64_t* ids_keep, const int64_t* ids_restore,
                           const int32_t* task_offsets_host, int T, int q_task, int B, int n_keep, int G, int D, int n_q,
                           float* d_ctx, float* part, void* stream) {
    MMAE_REQUIRE(d_queries && d_context && ids_keep && ids_restore && d_ctx && part, "decoder_build_bwd: null pointer");
    MMAE_REQUIRE(D % 4 == 0 && D <= 1024 && B > 0, "decoder_build_bwd: bad sizes");
    TaskTable tt;
    MMAE_REQUIRE(fill_tt(tt, task_offsets_host, T) == 0 && q_task >= -1 && q_task < T, "decoder_build_bwd: bad task table");
    hipLaunchKernelGGL(decoder_build_bwd_kernel, dim3(B < 1024 ? B : 1024, dbb_split(B)), dim3(256), 0, (hipStream_t)stream, d_queries,
                       d_context, (const long long*)ids_keep, (const long long*)ids_restore, tt, q_task, B, n_keep, G, D, n_q,
                       tt.off[T], d_ctx, part);
    return mmae_check_launch("decoder_build_bwd");
}

int mmae_unpatchify(const float* patches, float* img, int B, int C, int nh, int nw, int ph, int pw, void* stream) {
    MMAE_REQUIRE(patches && img && B > 0 && C > 0, "unpatchify: bad argument");
    const long long total = (long long)B * C * nh * ph * nw * pw;
    const int cbu = (pw % 4 == 0 && pw < 16) ? patch_tile_cb(ph, nw * pw) : 0;
    if (cbu > 0 && ((uintptr_t)patches % 16 == 0) && ((uintptr_t)img % 16 == 0)) {
        const long long nblk = (long long)B * nh * ((C + cbu - 1) / cbu);
        hipLaunchKernelGGL((patch_tile_kernel<float, false>), dim3((unsigned)nblk), dim3(256), (size_t)cbu * ph * nw * pw * 4, (hipStream_t)stream,
                           patches, img, (long long)C * ph * pw, C, nh, nw, ph, pw, cbu);
        return mmae_check_launch("unpatchify");
    }
    if (pw % 4 == 0 && ((uintptr_t)patches % 16 == 0) && ((uintptr_t)img % 16 == 0))
        hipLaunchKernelGGL(unpatchify4_kernel, dim3((unsigned)cdiv64(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, patches, img, C,
                           nh, nw, ph, pw, total / 4);
    else
        hipLaunchKernelGGL(unpatchify_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, patches, img, C, nh, nw,
                           ph, pw, total);
    return mmae_check_launch("unpatchify");
}

int mmae_patchify(const float* img, void* patches, int patches_dtype, int64_t ld, int B, int C, int nh, int nw, int ph, int pw, void* stream) {
    MMAE_REQUIRE(patches && img && B > 0 && C > 0 && ld >= (int64_t)C * ph * pw, "patchify: bad argument");
    if (patches_dtype != MMAE_BF16 && patches_dtype != MMAE_F32) { mmae_set_error("patchify: bf16 / f32 patches"); return MMAE_ESUPPORT; }
    const long long total = (long long)B * C * nh * ph * nw * pw;
    hipStream_t st = (hipStream_t)stream;
    const int cbp = (pw % 4 == 0 && pw < 16 && ld % 4 == 0) ? patch_tile_cb(ph, nw * pw) : 0;
    if (cbp > 0 && ((uintptr_t)patches % 16 == 0) && ((uintptr_t)img % 16 == 0)) {
        const dim3 grid((unsigned)((long long)B * nh * ((C + cbp - 1) / cbp)));
        const size_t lds = (size_t)cbp * ph * nw * pw * 4;
        if (patches_dtype == MMAE_BF16) hipLaunchKernelGGL((patch_tile_kernel<uint16_t, true>), grid, dim3(256), lds, st, img, (uint16_t*)patches, (long long)ld, C, nh, nw, ph, pw, cbp);
        else hipLaunchKernelGGL((patch_tile_kernel<float, true>), grid, dim3(256), lds, st, img, (float*)patches, (long long)ld, C, nh, nw, ph, pw, cbp);
        return mmae_check_launch("patchify");
    }
    if (pw % 4 == 0 && ld % 4 == 0 && ((uintptr_t)patches % 16 == 0) && ((uintptr_t)img % 16 == 0)) {
        const dim3 grid((unsigned)cdiv64(total / 4, 256));
        if (patches_dtype == MMAE_BF16) hipLaunchKernelGGL((patchify4_kernel<uint16_t>), grid, dim3(256), 0, st, img, (uint16_t*)patches, (long long)ld, C, nh, nw, ph, pw, total / 4);
        else hipLaunchKernelGGL((patchify4_kernel<float>), grid, dim3(256), 0, st, img, (float*)patches, (long long)ld, C, nh, nw, ph, pw, total / 4);
        return mmae_check_launch("patchify");
    }
    if (patches_dtype == MMAE_BF16) hipLaunchKernelGGL((patchify_kernel<uint16_t>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, img, (uint16_t*)patches, (long long)ld, C, nh, nw, ph, pw, total);
    else hipLaunchKernelGGL((patchify_kernel<float>), dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, img, (float*)patches, (long long)ld, C, nh, nw, ph, pw, total);
    return mmae_check_launch("patchify");
}

int mmae_semseg_avg_emb_fwd(const int64_t* x, const float* class_emb, float* out, int B, int H, int W, int E, int ph, int pw, int n_cls, void* stream) {
    MMAE_REQUIRE(x && class_emb && out && B > 0 && H > 0 && W > 0 && E > 0 && ph > 0 && pw > 0 && H % ph == 0 && W % pw == 0 && n_cls > 0, "semseg_avg_emb_fwd: bad argument");
    const long long total = (long long)B * E * (H / ph) * (W / pw);
    hipLaunchKernelGGL(semseg_avg_emb_fwd_kernel, dim3((unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)x, class_emb, out, B, H, W, E, ph, pw, n_cls);
    return mmae_check_launch("semseg_avg_emb_fwd");
}
int mmae_semseg_avg_emb_bwd(const float* d_img, const int64_t* x, float* d_class_emb, int B, int H, int W, int E, int ph, int pw, int n_cls, int pad_idx,
                            void* stream) {
    MMAE_REQUIRE(d_img && x && d_class_emb && B > 0 && H > 0 && W > 0 && E > 0 && ph > 0 && pw > 0 && H % ph == 0 && W % pw == 0 && n_cls > 0, "semseg_avg_emb_bwd: bad argument");
    const long long total = (long long)B * E * (H / ph) * (W / pw);
    hipLaunchKernelGGL(semseg_avg_emb_bwd_kernel, dim3((unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192)), dim3(256), 0, (hipStream_t)stream,
                       d_img, (const long long*)x, d_class_emb, B, H, W, E, ph, pw, n_cls, pad_idx);
    return mmae_check_launch("semseg_avg_emb_bwd");
}
int mmae_rows_to_image(const float* d_rows, int64_t ldr, int k_off, const int64_t* sel, float* d_img, int B, int n_sel, int64_t tok_off, int n_patches,
                       int C, int H, int W, int ph, int pw, void* stream) {
    MMAE_REQUIRE(d_rows && sel && d_img && B > 0 && n_sel > 0 && n_patches > 0 && C > 0 && ph > 0 && pw > 0 && H % ph == 0 && W % pw == 0 &&
                 (H / ph) * (W / pw) == n_patches, "rows_to_image: bad argument");
    hipLaunchKernelGGL(rows_to_image_kernel, dim3((unsigned)(B * n_sel)), dim3(256), 0, (hipStream_t)stream, d_rows, (long long)ldr, k_off, (const long long*)sel,
                       d_img, n_sel, (long long)tok_off, n_patches, C, H, W, ph, pw);
    return mmae_check_launch("rows_to_image");
}

int mmae_pos_emb_bwd(const float* d_tok, const int64_t* sel, float* d_pos, int B, int n_sel, int G, int D, int n_pos, void* stream) {
    MMAE_REQUIRE(d_tok && sel && d_pos && B > 0 && n_sel > 0 && G >= 0 && D > 0 && D % 4 == 0 && n_pos > 0, "pos_emb_bwd: bad argument");
    hipLaunchKernelGGL(pos_emb_bwd_kernel, dim3((unsigned)(B * n_sel)), dim3(64), 0, (hipStream_t)stream, d_tok, (const long long*)sel, d_pos, n_sel, G, D, n_pos);
    return mmae_check_launch("pos_emb_bwd");
}

int mmae_probe_tr16(const uint16_t* lds_image_1024, const uint32_t* lane_byte_addr_64, uint16_t* out_64x4, void* stream) {
    MMAE_REQUIRE(lds_image_1024 && lane_byte_addr_64 && out_64x4, "probe_tr16: null pointer");
    hipLaunchKernelGGL(probe_tr16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lds_image_1024, lane_byte_addr_64, out_64x4);
    return mmae_check_launch("probe_tr16");
}

}  // extern "C"
