// Classification evaluation (evaluate() of run_finetuning_cls.py:580-613: nn.CrossEntropyLoss, utils/metrics.py accuracy with its
// topk sort, three .item() read-backs per batch) in two launches without a sort or a read-back:
//   cls_row      one workgroup per row: the log-sum-exp in soft_ce_fwd's work shape (csrc/clsrecipe.hip: the same per-thread
//                recurrence, wave xor tree and wave-order merge, so its error bound carries over), and in the same single pass the
//                RANK of the target's logit -- how many logits beat it.  Row b is correct at k iff rank[b] < min(k, K).
//                Tie rule: among equal logits the lower index ranks first (seg_argmax's rule).
//   cls_finish   one workgroup: mean loss over the valid rows, the accuracies as the f32 operations of utils/metrics.py:38, and
//                (optionally) MetricLogger's total / count pairs in an f64 accumulator.
// No float atomics: every sum has a fixed order, results are bit-equal from run to run.
#include "common.h"
#include <math.h>

namespace {

constexpr int TOPK_MAX = MMAE_CLS_TOPK_MAX;
struct Topk { int k[TOPK_MAX]; };

__device__ __forceinline__ int block_count(int v, int* sh) {     // integers: any order gives the same sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// lse[b], nll[b] = lse - z_t, rank[b] = #{k: z_k > z_t} + #{k < t: z_k == z_t}; a target outside [0, K): nll 0, rank K.
// Columns K .. ldx - 1 are never read.
template <typename T>
__global__ void __launch_bounds__(256) cls_row_kernel(const T* __restrict__ x, long long ldx, const long long* __restrict__ target, int K,
                                                     float* __restrict__ lse, float* __restrict__ nll, int* __restrict__ rank) {
    __shared__ float sh[4];
    __shared__ int shi[4];
    const long long b = blockIdx.x;
    const T* xr = x + b * ldx;
    const long long t = target[b];
    const bool valid = t >= 0 && t < K;
    const float zt = valid ? ActT<T>::ld(xr + t) : 0.f;
    float m = -INFINITY, s = 0.f;
    int gt = 0, eq = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float z = ActT<T>::ld(xr + k);
        const float mn = fmaxf(m, z);
        s = s * __expf(m - mn) + __expf(z - mn);
        m = mn;
        gt += z > zt;
        eq += (z == zt && k < t);
    }
    const float M = block_max(m, sh);
    const float S = block_sum(m == -INFINITY ? 0.f : s * __expf(m - M), sh);      // a thread without a class contributes nothing
    const float l = M + logf(S);
    const int r = block_count(gt + eq, shi);
    if (threadIdx.x == 0) {
        lse[b] = l;
        nll[b] = valid ? l - zt : 0.f;
        rank[b] = valid ? r : K;
    }
}

// out[0] = sum nll / n_valid (0 when nothing is valid), out[1 + j] = fl(fl((float)c_j 100) / (float)B), c_j = #{b: rank[b] < min(k_j, K)}.
// A valid row has rank < K, an invalid one rank == K.  Sums in double through a fixed tree (the counts are exact in it).
// acc, when given: acc[0] += loss, acc[1] += 1, acc[2] += B, acc[3 + j] += acc_j B (one thread: no atomics).
__global__ void __launch_bounds__(256) cls_finish_kernel(const float* __restrict__ nll, const int* __restrict__ rank, int B, int K, int n_k,
                                                        Topk topk, float* __restrict__ out, double* __restrict__ acc) {
    __shared__ double s[256];
    double a = 0.0, nv = 0.0, c[TOPK_MAX] = {0.0, 0.0, 0.0, 0.0};
    int lim[TOPK_MAX];
#pragma unroll
    for (int j = 0; j < TOPK_MAX; ++j) lim[j] = j < n_k ? (topk.k[j] < K ? topk.k[j] : K) : 0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const int r = rank[i];
        a += (double)nll[i];
        nv += r < K ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < TOPK_MAX; ++j) c[j] += r < lim[j] ? 1.0 : 0.0;
    }
    a = block_tree_sum(a, s);
    __syncthreads();
    nv = block_tree_sum(nv, s);
#pragma unroll
    for (int j = 0; j < TOPK_MAX; ++j) {
        __syncthreads();
        c[j] = block_tree_sum(c[j], s);
    }
    if (threadIdx.x == 0) {
        const float loss = nv > 0.0 ? (float)(a / nv) : 0.f;
        out[0] = loss;
        if (acc != nullptr) {
            acc[0] += (double)loss;
            acc[1] += 1.0;
            acc[2] += (double)B;
        }
#pragma unroll
        for (int j = 0; j < TOPK_MAX; ++j) {
            if (j >= n_k) break;
            const float pct = __fdiv_rn(__fmul_rn((float)c[j], 100.f), (float)B);
            out[1 + j] = pct;
            if (acc != nullptr) acc[3 + j] += (double)pct * (double)B;
        }
    }
}

}  // namespace

extern "C" int mmae_cls_eval(const void* x, int x_dtype, int64_t ldx, const int64_t* target, int B, int K, int n_k, int k0, int k1, int k2,
                             int k3, float* lse, float* nll, int32_t* rank, float* out, double* acc, void* stream) {
    MMAE_REQUIRE(x && target && lse && nll && rank && out, "cls_eval: a required pointer is NULL (x, target, lse, nll, rank, out)");
    MMAE_REQUIRE(B > 0 && K > 0 && ldx >= K, "cls_eval: bad shape (B > 0, K > 0, ldx >= K)");
    MMAE_REQUIRE(n_k >= 1 && n_k <= TOPK_MAX, "cls_eval: n_k outside [1, MMAE_CLS_TOPK_MAX]");
    const Topk topk = {{k0, k1, k2, k3}};
    for (int j = 0; j < n_k; ++j) MMAE_REQUIRE(topk.k[j] >= 1, "cls_eval: a threshold k_j < 1");
    if (x_dtype != MMAE_F32 && x_dtype != MMAE_BF16) {
        mmae_set_error("cls_eval: logits must be MMAE_F32 or MMAE_BF16");
        return MMAE_ESUPPORT;
    }
    if (x_dtype == MMAE_F32)
        hipLaunchKernelGGL(cls_row_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)x, (long long)ldx,
                           (const long long*)target, K, lse, nll, (int*)rank);
    else
        hipLaunchKernelGGL(cls_row_kernel<uint16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (long long)ldx,
                           (const long long*)target, K, lse, nll, (int*)rank);
    hipLaunchKernelGGL(cls_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)nll, (const int*)rank, B, K, n_k, topk, out,
                       acc);
    return mmae_check_launch("cls_eval");
}
