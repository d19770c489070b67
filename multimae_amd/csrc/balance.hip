// Uncertainty task balancer (utils/task_balancing.py:21-44): T <= 16 scalar task losses L_i and the parameter log_vars s,
//   w_i = (exp(-s_i) * L_i + s_i) * m_i,   m_i = (L_i != 0)   (a NaN loss is "non-zero", as torch's != says)
// as one launch per direction instead of torch's stack / ne / neg / exp / mul / add / mul / unbind chain and its backward:
//   task_balance_fwd   lane i < T: reads L_i through its own device pointer (the losses are T separate scalars of T loss nodes)
//                      or from a packed f32 [T]; writes w_i and saves exp(-s_i) and L_i for the backward -- expf once per task
//   task_balance_bwd   lane i < T, upstream u_i (a null pointer: no gradient arrived, 0):
//                      dL_i = u_i * exp(-s_i) * m_i,   ds_i (+)= u_i * (1 - exp(-s_i) * L_i) * m_i
// One wave, plain vector stores, no atomics, nothing returned to the host: both launches may sit inside a captured step.
// The mask MULTIPLIES, as the reference's `losses_tensor *= non_zero_losses_mask` does: a masked entry is (+-)0 for finite s.
#include "common.h"
#include <math.h>

namespace {

constexpr int TMAX = MMAE_BALANCE_MAX_TASKS;
struct ScalarPtrs { const float* p[TMAX]; };

__global__ void __launch_bounds__(64) task_balance_fwd_kernel(const ScalarPtrs lp, const float* __restrict__ packed,
                                                              const float* __restrict__ log_vars, float* __restrict__ weighted,
                                                              float* __restrict__ saved, int T) {
    const int i = threadIdx.x;
    if (i >= T) return;
    const float L = packed ? packed[i] : *lp.p[i];
    const float s = log_vars[i];
    const float e = expf(-s);
    const float m = (L != 0.f) ? 1.f : 0.f;
    weighted[i] = (e * L + s) * m;
    saved[i] = e;
    saved[T + i] = L;
}

__global__ void __launch_bounds__(64) task_balance_bwd_kernel(const ScalarPtrs up, const float* __restrict__ packed,
                                                              const float* __restrict__ saved, float* __restrict__ d_losses,
                                                              float* __restrict__ d_log_vars, int accumulate, int T) {
    const int i = threadIdx.x;
    if (i >= T) return;
    const float u = packed ? packed[i] : (up.p[i] ? *up.p[i] : 0.f);
    const float e = saved[i], L = saved[T + i];
    const float m = (L != 0.f) ? 1.f : 0.f;
    d_losses[i] = u * e * m;
    const float ds = u * (1.f - e * L) * m;
    d_log_vars[i] = accumulate ? d_log_vars[i] + ds : ds;
}

}  // namespace

extern "C" {

int mmae_task_balance_fwd(const float* const* loss_ptrs, const float* losses, const float* log_vars, float* weighted, float* saved,
                          int T, void* stream) {
    MMAE_REQUIRE(T >= 1 && T <= TMAX, "task_balance_fwd: T outside 1 .. MMAE_BALANCE_MAX_TASKS");
    MMAE_REQUIRE((loss_ptrs != nullptr) != (losses != nullptr), "task_balance_fwd: give exactly one of loss_ptrs / losses");
    MMAE_REQUIRE(log_vars && weighted && saved, "task_balance_fwd: null pointer");
    ScalarPtrs lp;
    for (int i = 0; i < TMAX; ++i) lp.p[i] = (loss_ptrs && i < T) ? loss_ptrs[i] : nullptr;
    if (loss_ptrs)
        for (int i = 0; i < T; ++i) MMAE_REQUIRE(lp.p[i], "task_balance_fwd: null loss pointer");
    hipLaunchKernelGGL(task_balance_fwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lp, losses, log_vars, weighted, saved, T);
    return mmae_check_launch("task_balance_fwd");
}

int mmae_task_balance_bwd(const float* const* upstream_ptrs, const float* upstream, const float* saved, float* d_losses,
                          float* d_log_vars, int accumulate, int T, void* stream) {
    MMAE_REQUIRE(T >= 1 && T <= TMAX, "task_balance_bwd: T outside 1 .. MMAE_BALANCE_MAX_TASKS");
    MMAE_REQUIRE((upstream_ptrs != nullptr) != (upstream != nullptr), "task_balance_bwd: give exactly one of upstream_ptrs / upstream");
    MMAE_REQUIRE(saved && d_losses && d_log_vars, "task_balance_bwd: null pointer");
    ScalarPtrs up;
    for (int i = 0; i < TMAX; ++i) up.p[i] = (upstream_ptrs && i < T) ? upstream_ptrs[i] : nullptr;
    hipLaunchKernelGGL(task_balance_bwd_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, up, upstream, saved, d_losses, d_log_vars,
                       accumulate, T);
    return mmae_check_launch("task_balance_bwd");
}

}  // extern "C"
