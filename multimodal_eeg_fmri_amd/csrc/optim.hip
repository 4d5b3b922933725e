// The optimizer step: sum of squared gradients, then fused AdamW with the global-norm clip, on one flat fp32 bucket.
// Callers: optim.FusedAdamW and bridge_trainer.py's captured step (mm_sumsq, then mm_adamw_clip).
#include "common.h"

namespace {
// ---------------------------------------------------------------------------
// fused AdamW (decoupled weight decay) + global-norm clip on a flat fp32 bucket.
// state[0] = step counter (float, incremented on device so the launch can live
// in a hipGraph), state[2] = learning rate (host-updatable), state[3] = last clip
// coefficient, state[4] = last gradient norm, state[8 .. 8+1024) = per-block partial
// sums of squared gradients.  The partials are summed in a FIXED order (no float
// atomics), so data-parallel ranks holding the same all-reduced gradient compute
// bit-identical clip coefficients and their parameters never drift apart.
// ---------------------------------------------------------------------------
constexpr int SUMSQ_SLOTS = 1024;

__global__ void sumsq_kernel(const float* __restrict__ g, float* __restrict__ state, size_t n) {
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += g[i] * g[i];
    s = wave_sum(s);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) state[8 + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (blockIdx.x == 0)
        for (int i = gridDim.x + threadIdx.x; i < SUMSQ_SLOTS; i += blockDim.x) state[8 + i] = 0.f;
}
}  // namespace

extern "C" {
int mm_sumsq(const float* g, float* state, int64_t n, hipStream_t st) {
    MM_REQUIRE(g && state && n > 0, "sumsq: null");
    hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for((size_t)n, 1024)), dim3(256), 0, st, g, state, (size_t)n);
    return mm_check_launch("sumsq");
}
}  // extern "C"

namespace {
// every 256-thread block gets the same total, added in the same order
__device__ inline float sumsq_total(const float* __restrict__ state) {
    __shared__ float tot[4];
    const int t = threadIdx.x;
    float s = (state[8 + t] + state[8 + 256 + t]) + (state[8 + 512 + t] + state[8 + 768 + t]);
    s = wave_sum(s);
    if ((t & 63) == 0) tot[t >> 6] = s;
    __syncthreads();
    return (tot[0] + tot[1]) + (tot[2] + tot[3]);
}

// (The bookkeeping below - step counter, last norm / clip coefficient, the dropout epoch word of the next step - stays a
// one-workgroup launch of its own.  Folding it into the update kernel's LAST-ARRIVING workgroup was tried: 2 048 arrivals on
// one counter serialise at the L2 and the update went from 10 to 30 us, profiles/r04_step_kernel_summary.txt history.)
__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ state, size_t n, float beta1,
                             float beta2, float eps, float wd, float max_norm, float grad_scale, int zero_grad) {
    const float step = state[0] + 1.f;
    const float lr = state[2];
    const float gn = sqrtf(sumsq_total(state)) * grad_scale;
    const float clip = (max_norm > 0.f) ? fminf(1.f, max_norm / (gn + 1e-6f)) : 1.f;
    const float gs = grad_scale * clip;
    const float bc1 = 1.f - powf(beta1, step), bc2 = 1.f - powf(beta2, step);
    const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gs;
        float pi = p[i] * (1.f - lr * wd);
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        pi -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (zero_grad) g[i] = 0.f;                 // the next step's zero_grad(), for free
    }
}

__global__ void adamw_finish_kernel(float* __restrict__ state, float max_norm, float grad_scale, uint32_t* epoch) {
    const float ss = sumsq_total(state);
    if (threadIdx.x != 0) return;
    if (epoch) epoch[0] += 1;                      // dropout epoch word of the NEXT step (hipGraph replays)
    const float gn = sqrtf(ss) * grad_scale;
    state[3] = (max_norm > 0.f) ? fminf(1.f, max_norm / (gn + 1e-6f)) : 1.f;
    state[4] = gn;
    state[0] += 1.f;
    state[1] = ss;
}
}  // namespace

extern "C" {
int mm_adamw_clip(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                  float eps, float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                  hipStream_t st) {
    MM_REQUIRE(p && g && m && v && state && n > 0, "adamw_clip: null");
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, p, g, m, v, state, (size_t)n, beta1,
                       beta2, eps, weight_decay, max_norm, grad_scale, zero_grad);
    hipLaunchKernelGGL(adamw_finish_kernel, dim3(1), dim3(256), 0, st, state, max_norm, grad_scale, seed_epoch);
    return mm_check_launch("adamw_clip");
}
}  // extern "C"
