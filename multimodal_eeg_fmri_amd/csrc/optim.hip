// The optimizer step: sum of squared gradients, then fused AdamW with the global-norm clip, on one flat fp32 bucket.
// Callers: optim.FusedAdamW and bridge_trainer.py's captured step (mm_sumsq, then mm_adamw_clip or, with an exponential
// moving average of the weights, mm_adamw_clip_ema).
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
// state[5] = the weight-average decay of the last step: written by mm_adamw_clip_ema only (mm_adamw_clip never writes
// state[5..8)).
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

// The weight average of mm_adamw_clip_ema: the decay the step uses, from the step count AFTER this step (t = state[0] + 1,
// an integer held in a float: the two sums are exact, the quotient is one rounding).  Computed on the device, so the
// launch can live in a hipGraph; the update kernel and the finish kernel call this one function and agree on its bits.
__device__ inline float ema_decay_at(float t, float ema_decay, int ema_warmup) {
    return ema_warmup ? fminf(ema_decay, (1.f + t) / (10.f + t)) : ema_decay;
}

// (The bookkeeping below - step counter, last norm / clip coefficient, the dropout epoch word of the next step - stays a
// one-workgroup launch of its own.  Folding it into the update kernel's LAST-ARRIVING workgroup was tried: 2 048 arrivals on
// one counter serialise at the L2 and the update went from 10 to 30 us, profiles/r04_step_kernel_summary.txt history.)
// EMA = false is mm_adamw_clip: `ema` is never read or written, and the compiled loop is the one it always was.
// EMA = true (mm_adamw_clip_ema): after element i's update, ema[i] += (1 - d) * (p_new[i] - ema[i]) with 1 - d formed in
// fp32, the difference rounded, then ONE fused multiply-add: where ema[i] == p_new[i] the difference is exactly 0 and
// ema[i] keeps its bits.  One more read stream and one more write stream over the bucket, no new launch.
template <bool EMA>
__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ state, size_t n, float beta1,
                             float beta2, float eps, float wd, float max_norm, float grad_scale, int zero_grad,
                             float* __restrict__ ema, float ema_decay, int ema_warmup) {
    const float step = state[0] + 1.f;
    const float lr = state[2];
    const float gn = sqrtf(sumsq_total(state)) * grad_scale;
    const float clip = (max_norm > 0.f) ? fminf(1.f, max_norm / (gn + 1e-6f)) : 1.f;
    const float gs = grad_scale * clip;
    const float bc1 = 1.f - powf(beta1, step), bc2 = 1.f - powf(beta2, step);
    const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
    const float one_minus_d = EMA ? 1.f - ema_decay_at(step, ema_decay, ema_warmup) : 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gs;
        float pi = p[i] * (1.f - lr * wd);
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        pi -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (zero_grad) g[i] = 0.f;                 // the next step's zero_grad(), for free
        if (EMA) {
            const float e = ema[i];
            ema[i] = __fmaf_rn(one_minus_d, __fsub_rn(pi, e), e);
        }
    }
}

template <bool EMA>
__global__ void adamw_finish_kernel(float* __restrict__ state, float max_norm, float grad_scale, uint32_t* epoch,
                                    float ema_decay, int ema_warmup) {
    const float ss = sumsq_total(state);
    if (threadIdx.x != 0) return;
    if (epoch) epoch[0] += 1;                      // dropout epoch word of the NEXT step (hipGraph replays)
    const float gn = sqrtf(ss) * grad_scale;
    state[3] = (max_norm > 0.f) ? fminf(1.f, max_norm / (gn + 1e-6f)) : 1.f;
    state[4] = gn;
    if (EMA) state[5] = ema_decay_at(state[0] + 1.f, ema_decay, ema_warmup);   // the decay the update kernel just used
    state[0] += 1.f;
    state[1] = ss;
}

template <bool EMA>
int adamw_launch(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2, float eps,
                 float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch, float* ema,
                 float ema_decay, int ema_warmup, hipStream_t st, const char* what) {
    hipLaunchKernelGGL(adamw_kernel<EMA>, dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, p, g, m, v, state, (size_t)n,
                       beta1, beta2, eps, weight_decay, max_norm, grad_scale, zero_grad, ema, ema_decay, ema_warmup);
    hipLaunchKernelGGL(adamw_finish_kernel<EMA>, dim3(1), dim3(256), 0, st, state, max_norm, grad_scale, seed_epoch,
                       ema_decay, ema_warmup);
    return mm_check_launch(what);
}
}  // namespace

extern "C" {
int mm_adamw_clip(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                  float eps, float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                  hipStream_t st) {
    MM_REQUIRE(p && g && m && v && state && n > 0, "adamw_clip: null");
    return adamw_launch<false>(p, g, m, v, state, n, beta1, beta2, eps, weight_decay, max_norm, grad_scale, zero_grad,
                               seed_epoch, nullptr, 0.f, 0, st, "adamw_clip");
}

int mm_adamw_clip_ema(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                      float eps, float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                      float* ema, float ema_decay, int ema_warmup, hipStream_t st) {
    MM_REQUIRE(p && g && m && v && state && n > 0, "adamw_clip_ema: null");
    MM_REQUIRE(ema, "adamw_clip_ema: ema is null (mm_adamw_clip is the update without a weight average)");
    MM_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "adamw_clip_ema: ema_decay %g outside [0, 1)", (double)ema_decay);
    return adamw_launch<true>(p, g, m, v, state, n, beta1, beta2, eps, weight_decay, max_norm, grad_scale, zero_grad,
                              seed_epoch, ema, ema_decay, ema_warmup, st, "adamw_clip_ema");
}
}  // extern "C"
