// The optimizer step: sum of squared gradients, then fused AdamW with the global-norm clip, on one flat fp32 bucket.
// Caller: optim.adamw_update, for optim.FusedAdamW and bridge_trainer.py's captured step (mm_sumsq, then one of the four
// entry points of ONE update kernel template: mm_adamw_clip; with an exponential moving average of the weights,
// mm_adamw_clip_ema; with parameter groups - per-segment learning-rate multipliers and weight decays - mm_adamw_clip_groups /
// mm_adamw_clip_groups_ema).
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

// The update, written ONCE and instantiated four ways (mm_adamw_clip, _ema, _groups, _groups_ema), so every entry point's
// bits are one body's.  The forms are WRITTEN OUT (__fmaf_rn / __fmul_rn: what the compiler contracts the plain expressions
// into), so that the bits do not depend on what the optimizer makes of a differently shaped loop:
//     clip    max_norm / fma(sqrt(sumsq), grad_scale, 1e-6)
//     decay   fma(-wd, lr, 1)                      step_size  lr / bc1
//     m       fma(1 - b1, g, b1 * m)               v          fma(g, (1 - b2) * g, b2 * v)
//     p       fma(decay, p, -(step_size * m / fma(rsqrt(bc2), sqrt(v), eps)))
// EMA = false: `ema` is never read or written.  EMA = true: after element i's update, ema[i] += (1 - d) * (p_new[i] - ema[i])
// with 1 - d formed in fp32, the difference rounded, then ONE fused multiply-add: where ema[i] == p_new[i] the difference is
// exactly 0 and ema[i] keeps its bits.  One more read stream and one more write stream over the bucket, no new launch.
// GROUPS = false: decay and step_size are two scalars, from state[2] and `wd`; the table arguments are never read, and the
// table's LDS arrays are not allocated.
// GROUPS = true (parameter groups): the bucket is cut into n_seg <= MM_OPT_MAX_SEGMENTS contiguous segments, segment
// s = [seg_end[s-1], seg_end[s]) with its own learning rate lr_s = fl32(state[2] * seg_lr_mult[s]) and weight decay seg_wd[s]
// (`wd` is not read).  The table is DEVICE memory read at launch, so a captured launch serves any later change of its
// values.  Every workgroup stages {end, decay, step_size} of all segments in LDS once (16 bytes a segment, 16 KB at the cap)
// and finds an element's segment by binary search over the ends: the first s with i < end[s], else the last one - the search
// runs over [0, n_seg) only, so no element and no table content can form an address outside the table.
// (The bookkeeping - step counter, last norm / clip coefficient, the dropout epoch word of the next step - stays a
// one-workgroup launch of its own, adamw_finish_kernel.  Folding it into the update kernel's LAST-ARRIVING workgroup was
// tried: 2 048 arrivals on one counter serialise at the L2 and the update went from 10 to 30 us,
// profiles/r04_step_kernel_summary.txt history.)
constexpr int OPT_MAX_SEGMENTS = 1024;            // MM_OPT_MAX_SEGMENTS

template <bool EMA, bool GROUPS>
__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, const float* __restrict__ state, size_t n, float beta1,
                             float beta2, float eps, float wd, float max_norm, float grad_scale, int zero_grad,
                             const long long* __restrict__ seg_end, const float* __restrict__ seg_lr_mult,
                             const float* __restrict__ seg_wd, int n_seg, float* __restrict__ ema, float ema_decay,
                             int ema_warmup) {
    constexpr int LDS_SEGMENTS = GROUPS ? OPT_MAX_SEGMENTS : 1;              // (GROUPS = false: unused, and so not allocated)
    __shared__ long long s_end[LDS_SEGMENTS];
    __shared__ float s_decay[LDS_SEGMENTS], s_step[LDS_SEGMENTS];
    const float step = state[0] + 1.f;
    const float lr = state[2];
    const float gn = __fmaf_rn(sqrtf(sumsq_total(state)), grad_scale, 1e-6f);
    const float clip = (max_norm > 0.f) ? fminf(1.f, max_norm / gn) : 1.f;
    const float gs = __fmul_rn(grad_scale, clip);
    const float bc1 = 1.f - powf(beta1, step), bc2 = 1.f - powf(beta2, step);
    const float inv_sqrt_bc2 = rsqrtf(bc2);
    const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
    const float one_minus_d = EMA ? 1.f - ema_decay_at(step, ema_decay, ema_warmup) : 0.f;
    float decay = 0.f, step_size = 0.f;            // GROUPS: looked up per element
    if (GROUPS) {
        for (int s = threadIdx.x; s < n_seg; s += blockDim.x) {
            const float lr_s = __fmul_rn(lr, seg_lr_mult[s]);
            s_end[s] = seg_end[s];
            s_decay[s] = __fmaf_rn(-seg_wd[s], lr_s, 1.f);
            s_step[s] = lr_s / bc1;
        }
        __syncthreads();
    } else {
        decay = __fmaf_rn(-wd, lr, 1.f);
        step_size = lr / bc1;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (GROUPS) {
            int lo = 0, hi = n_seg - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((long long)i < s_end[mid]) hi = mid; else lo = mid + 1;
            }
            decay = s_decay[lo]; step_size = s_step[lo];
        }
        const float gi = __fmul_rn(g[i], gs);
        const float mi = __fmaf_rn(omb1, gi, __fmul_rn(beta1, m[i]));
        const float vi = __fmaf_rn(gi, __fmul_rn(omb2, gi), __fmul_rn(beta2, v[i]));
        const float q = __fmul_rn(step_size, mi) / __fmaf_rn(inv_sqrt_bc2, sqrtf(vi), eps);
        const float pi = __fmaf_rn(decay, p[i], -q);
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

// The argument checks (nothing is launched when one fails; `who` names the entry point), then the update and the finish
// kernel.  The table's CONTENTS are device memory: the host that builds it validates them - optim.segment_table.
template <bool EMA, bool GROUPS>
int adamw_launch(const char* who, float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                 float eps, float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                 const int64_t* seg_end, const float* seg_lr_mult, const float* seg_wd, int n_seg, float* ema,
                 float ema_decay, int ema_warmup, hipStream_t st) {
    MM_REQUIRE(p && g && m && v && state && n > 0, "%s: null", who);
    if (GROUPS) {
        MM_REQUIRE(seg_end && seg_lr_mult && seg_wd, "%s: a segment table array is null", who);
        MM_REQUIRE(n_seg >= 1 && n_seg <= OPT_MAX_SEGMENTS, "%s: n_seg %d outside [1, %d]", who, n_seg, OPT_MAX_SEGMENTS);
    }
    if (EMA) {
        MM_REQUIRE(ema, "%s: ema is null (the entry point without _ema is the update without a weight average)", who);
        MM_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "%s: ema_decay %g outside [0, 1)", who, (double)ema_decay);
    }
    hipLaunchKernelGGL((adamw_kernel<EMA, GROUPS>), dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, p, g, m, v, state,
                       (size_t)n, beta1, beta2, eps, weight_decay, max_norm, grad_scale, zero_grad,
                       (const long long*)seg_end, seg_lr_mult, seg_wd, n_seg, ema, ema_decay, ema_warmup);
    hipLaunchKernelGGL(adamw_finish_kernel<EMA>, dim3(1), dim3(256), 0, st, state, max_norm, grad_scale, seed_epoch,
                       ema_decay, ema_warmup);
    return mm_check_launch(who);
}
}  // namespace

extern "C" {
int mm_adamw_clip(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                  float eps, float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                  hipStream_t st) {
    return adamw_launch<false, false>("adamw_clip", p, g, m, v, state, n, beta1, beta2, eps, weight_decay, max_norm,
                                      grad_scale, zero_grad, seed_epoch, nullptr, nullptr, nullptr, 0, nullptr, 0.f, 0, st);
}

int mm_adamw_clip_ema(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                      float eps, float weight_decay, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                      float* ema, float ema_decay, int ema_warmup, hipStream_t st) {
    return adamw_launch<true, false>("adamw_clip_ema", p, g, m, v, state, n, beta1, beta2, eps, weight_decay, max_norm,
                                     grad_scale, zero_grad, seed_epoch, nullptr, nullptr, nullptr, 0, ema, ema_decay,
                                     ema_warmup, st);
}

int mm_adamw_clip_groups(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                         float eps, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                         const int64_t* seg_end, const float* seg_lr_mult, const float* seg_wd, int n_seg,
                         hipStream_t st) {
    return adamw_launch<false, true>("adamw_clip_groups", p, g, m, v, state, n, beta1, beta2, eps, 0.f, max_norm,
                                     grad_scale, zero_grad, seed_epoch, seg_end, seg_lr_mult, seg_wd, n_seg, nullptr, 0.f,
                                     0, st);
}

int mm_adamw_clip_groups_ema(float* p, float* g, float* m, float* v, float* state, int64_t n, float beta1, float beta2,
                             float eps, float max_norm, float grad_scale, int zero_grad, uint32_t* seed_epoch,
                             const int64_t* seg_end, const float* seg_lr_mult, const float* seg_wd, int n_seg,
                             float* ema, float ema_decay, int ema_warmup, hipStream_t st) {
    return adamw_launch<true, true>("adamw_clip_groups_ema", p, g, m, v, state, n, beta1, beta2, eps, 0.f, max_norm,
                                    grad_scale, zero_grad, seed_epoch, seg_end, seg_lr_mult, seg_wd, n_seg, ema, ema_decay,
                                    ema_warmup, st);
}
}  // extern "C"
