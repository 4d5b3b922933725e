// On-device EEG augmentation (the reference's EEGTransforms, EEG_CODE/CrossModal_EEG_scr.ipynb): per sample, with
// probability p_noise, Gaussian noise of noise_factor * std(sample); with probability p_drop, n_drop channels zeroed.
// Fused into the launch that stages a training step's inputs (mm_stage_inputs): the augmented batch never exists as a
// separate pass over the packed operand.
//
// ---- the random stream: h(stream, idx), stream(seed, step, rank, purpose), thresh(p) and the uniform draw are
// aug_stream.h's (tests/test_augment_*.py carry an fp64 replica).  This file's purposes: 0 noise decision,
// 1 drop decision, 2 channel keys, 3 gauss a, 4 gauss b; mm_stage_inputs_taug's time draws use 19..25.
//
//   sample b:         noise on  iff  h(stream0, b) < thresh(p_noise),   drop on  iff  h(stream1, b) < thresh(p_drop)
//   channel c:        key_c = h(stream2, b * C + c); dropped iff drop is on and fewer than n_drop channels c' have
//                     (key_c', c') < (key_c, c) lexicographically (= the first n_drop of a random permutation)
//   elements (t, t+1), t even, of row (b, c) share the Box-Muller pair idx = (b * C + c) * ceil(T / 2) + t / 2:
//                     u1 = (h(stream3, idx) + 1) * 2^-32 in (0, 1],  u2 = h(stream4, idx) * 2^-32
//                     z0 = sqrt(-2 ln u1) cos(2 pi u2) -> t,  z1 = sqrt(-2 ln u1) sin(2 pi u2) -> t + 1
//   out = x + z * (noise_factor * std_b), std_b = the unbiased standard deviation of the ORIGINAL sample over its C * T
//   values; then the dropped channels are set to 0.0f.  A sample without noise (or with std_b = 0) passes unchanged.
//
// ---- the two launches -----------------------------------------------------------------------------------------------
// mm_eeg_augment_plan: workgroup (b, k) sums chunk k of sample b - sum and sum of squares as fp64 partials, every thread
//   and every reduction step in a fixed order (no atomics): bit-reproducible, and the fp64 sum of squares loses
//   (1 + mean^2 / var) * 2^-53 to a mean offset, nothing at fp32 level.  4096 values per workgroup (16 per thread,
//   16-byte loads where the sample rows allow them): B = 32 samples of 64 x 1024 are 512 workgroups, two per CU - one
//   workgroup per sample would stream its 256 KB through a single CU.  Workgroup (b, 0) also draws the sample's two
//   decisions and its channel mask.
// mm_stage_inputs_aug: stage_inputs_kernel (igemm1d_pack.hip) with the augmentation between the load and the LDS transpose
//   tile.  Every tile workgroup adds its sample's partials in chunk order (<= 64 pairs of doubles, the same bits in
//   every workgroup) for std_b; the workgroup of the sample's first tile stores the scale and std_b into the plan.  A
//   thread handles the two elements of a Box-Muller pair: one log, one sqrt, one sincos per two elements.
//
// plan (32-bit words; include/mmeeg_hip.h): per sample S = 4 + ceil(C / 32) words, rounded up to even -
//   [0] noise scale (fp32; 0 = off), [1] std_b (fp32), [2] noise on, [3] drop on, [4...] channel mask (bit c % 32 of
//   word c / 32) - then, from word B * S, the partials double[B][nchunk][2].
#include "aug_stream.h"
#include "common.h"
#include "mmeeg_hip.h"

namespace {

constexpr int AUG_HDR = 4;

struct AugShape { int stride, chunk, nchunk; int64_t words; };
// the layout of the plan for (B, C, T): ops.eeg_augment_plan_words computes the same
inline AugShape aug_shape(int B, int C, int T) {
    AugShape s;
    const int64_t ct = (int64_t)C * T;
    s.stride = (AUG_HDR + (C + 31) / 32 + 1) & ~1;
    const AugChunks k = aug_chunks(ct);
    s.chunk = k.chunk;
    s.nchunk = k.nchunk;
    s.words = (int64_t)B * s.stride + 4 * (int64_t)B * s.nchunk;
    return s;
}
struct PlanArgs {
    const float* x; uint32_t* plan;
    int B, C, T, stride, chunk, nchunk, n_drop, vec;
    uint64_t t_noise, t_drop;
    uint32_t s_noise, s_drop, s_keys;
};

__global__ void __launch_bounds__(256) eeg_augment_plan_kernel(PlanArgs a) {
    __shared__ double red[4][2];
    const int b = blockIdx.x / a.nchunk, k = blockIdx.x % a.nchunk;
    const int tid = threadIdx.x;
    const size_t ct = (size_t)a.C * a.T;
    const float* xs = a.x + (size_t)b * ct;
    const size_t lo = (size_t)k * a.chunk, hi = lo + a.chunk < ct ? lo + a.chunk : ct;
    double s = 0.0, q = 0.0;
    if (a.vec) {                                   // C * T a multiple of 4 and the batch 16-byte aligned
        const float4* p = reinterpret_cast<const float4*>(xs);
#pragma unroll 4
        for (size_t i = lo / 4 + tid; i < hi / 4; i += 256) {
            const float4 v = p[i];
            s += (double)v.x; q += (double)v.x * (double)v.x;
            s += (double)v.y; q += (double)v.y * (double)v.y;
            s += (double)v.z; q += (double)v.z * (double)v.z;
            s += (double)v.w; q += (double)v.w * (double)v.w;
        }
    } else {
#pragma unroll 4
        for (size_t i = lo + tid; i < hi; i += 256) {
            const double v = (double)xs[i];
            s += v; q += v * v;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = s; red[tid >> 6][1] = q; }
    __syncthreads();
    if (tid == 0) {
        double* part = reinterpret_cast<double*>(a.plan + (size_t)a.B * a.stride) + ((size_t)b * a.nchunk + k) * 2;
        part[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        part[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
    if (k != 0) return;
    // the sample's decisions and channel mask
    uint32_t* hdr = a.plan + (size_t)b * a.stride;
    const bool noise_on = (uint64_t)aug_hash(a.s_noise, (uint32_t)b) < a.t_noise;
    const bool drop_on = (uint64_t)aug_hash(a.s_drop, (uint32_t)b) < a.t_drop;
    if (tid == 0) { hdr[2] = noise_on; hdr[3] = drop_on; }
    const int nw = (a.C + 31) / 32;
    const uint32_t kbase = (uint32_t)b * (uint32_t)a.C;
    for (int cb = 0; cb < a.C; cb += 256) {        // (uniform trip count: the ballot below needs every lane)
        const int c = cb + tid;
        bool dropped = false;
        if (drop_on && c < a.C) {
            const uint32_t key = aug_hash(a.s_keys, kbase + c);
            int before = 0;
            for (int o = 0; o < a.C; ++o) {
                const uint32_t ko = aug_hash(a.s_keys, kbase + o);
                before += (ko < key || (ko == key && o < c)) ? 1 : 0;
            }
            dropped = before < a.n_drop;
        }
        const unsigned long long m = __ballot(dropped);
        if ((tid & 63) == 0) {
            const int w = (cb + tid) / 32;
            if (w < nw) hdr[AUG_HDR + w] = (uint32_t)m;
            if (w + 1 < nw) hdr[AUG_HDR + w + 1] = (uint32_t)(m >> 32);
        }
    }
}

// the time transforms of mm_stage_inputs_taug: thresholds and stream words of the seven per-sample draws
struct TimeAugArgs {
    uint64_t t_shift, t_scale, t_invert, t_mask;
    uint32_t s_shift, s_shift_amt, s_scale, s_scale_u, s_invert, s_mask, s_mask_start;
    int max_shift, mask_len;
    float scale_range;
    int32_t* time_plan;
};

struct StageAugArgs {
    const float* x; uint32_t* plan; bf16* y; float* out;
    int B, C, T, Cp, tcw, stride, nchunk, npack;
    float noise_factor;
    uint32_t s_ga, s_gb;
    float4* d1; const float4* s1; size_t n1;
    TimeAugArgs tm;                                                // (read by the <true> instance only)
};

enum { TF_SHIFT = 1, TF_SCALE = 2, TF_INVERT = 4, TF_MASK = 8 };

// the noise of the Box-Muller pair idx onto the two elements of a thread: ONE expression for both instances of the kernel
// below, so that they round alike
__device__ __forceinline__ void aug_add_noise(float& v0, float& v1, bool two, uint32_t s_ga, uint32_t s_gb, uint32_t idx, float scale) {
    const float u1 = ((float)aug_hash(s_ga, idx) + 1.0f) * 2.3283064365386963e-10f;   // 2^-32
    const float w2 = (float)aug_hash(s_gb, idx) * 4.6566128730773926e-10f;            // 2 u2
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(w2, &sn, &cs);
    v0 = v0 + (r * cs) * scale;
    if (two) v1 = v1 + (r * sn) * scale;
}

// Workgroups [0, npack) are 32 x 32 (channel x time) tiles, the rest copy the fMRI batch (as stage_inputs_kernel).
// TIME: the time transforms as well (mm_stage_inputs_taug) - every tile workgroup draws its sample's shift, gain and mask
// window itself (seven hashes), so they need no plan; the EEG plan may then be absent (no noise, no channel drop).
template <bool TIME>
__global__ void __launch_bounds__(256) stage_inputs_aug_kernel(StageAugArgs a) {
    __shared__ float tile[32][33];
    if ((int)blockIdx.x >= a.npack) {
        const size_t nb = gridDim.x - a.npack;
        for (size_t i = (size_t)(blockIdx.x - a.npack) * blockDim.x + threadIdx.x; i < a.n1; i += nb * blockDim.x) a.d1[i] = a.s1[i];
        return;
    }
    const int tt = (a.T + 31) / 32;
    const int b = blockIdx.x / (tt * a.tcw), rem = blockIdx.x % (tt * a.tcw);
    const int t0 = (rem % tt) * 32, c0 = (rem / tt) * 32;
    const bool planned = !TIME || a.plan != nullptr;
    uint32_t* hdr = planned ? a.plan + (size_t)b * a.stride : nullptr;
    float scale = 0.f;
    bool drop_on = false;
    if (planned) {
        // std_b from the chunk partials, in chunk order
        const double* part = reinterpret_cast<const double*>(a.plan + (size_t)a.B * a.stride) + (size_t)b * a.nchunk * 2;
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < a.nchunk; ++k) { s1 += part[2 * k]; s2 += part[2 * k + 1]; }
        const double n = (double)a.C * (double)a.T;
        double var = (s2 - s1 * (s1 / n)) / (n - 1.0);
        var = var < 0.0 ? 0.0 : var;                               // (a NaN stays a NaN)
        const float std_b = (float)sqrt(var);
        scale = hdr[2] ? a.noise_factor * std_b : 0.f;
        if (rem == 0 && threadIdx.x == 0) { hdr[0] = __float_as_uint(scale); hdr[1] = __float_as_uint(std_b); }
        drop_on = hdr[3] != 0;
    }
    const uint32_t half_t = (uint32_t)((a.T + 1) / 2);
    // the sample's time draws: shift sh (out[t] = x[t - sh]), gain, mask window [m0, m0 + mlen)
    int sh = 0, m0 = 0, mlen = 0;
    uint32_t flags = 0;
    float gain = 1.0f;
    if constexpr (TIME) {
        const TimeAugArgs& tm = a.tm;
        const uint32_t ub = (uint32_t)b;
        if ((uint64_t)aug_hash(tm.s_shift, ub) < tm.t_shift) {
            flags |= TF_SHIFT;
            sh = (int)aug_uniform(aug_hash(tm.s_shift_amt, ub), 2u * (uint32_t)tm.max_shift + 1u) - tm.max_shift;
        }
        if ((uint64_t)aug_hash(tm.s_scale, ub) < tm.t_scale) {
            flags |= TF_SCALE;
            gain = aug_scale_factor(tm.scale_range, aug_hash(tm.s_scale_u, ub));
        }
        if ((uint64_t)aug_hash(tm.s_invert, ub) < tm.t_invert) { flags |= TF_INVERT; gain = -gain; }
        if ((uint64_t)aug_hash(tm.s_mask, ub) < tm.t_mask) {
            flags |= TF_MASK;
            m0 = (int)aug_uniform(aug_hash(tm.s_mask_start, ub), (uint32_t)(a.T - tm.mask_len + 1));
            mlen = tm.mask_len;
        }
        if (tm.time_plan && rem == 0 && threadIdx.x < 8) {
            const int w = threadIdx.x;
            tm.time_plan[(size_t)b * 8 + w] = w == 0 ? (int)flags : w == 1 ? sh : w == 2 ? (int)__float_as_uint(gain) : w == 3 ? m0 : w == 4 ? mlen : 0;
        }
    }
    const bool gain_on = (flags & (TF_SCALE | TF_INVERT)) != 0;

    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;         // a thread: elements (t, t + 1) of one row, t even
    for (int i = ty; i < 32; i += 16) {
        const int c = c0 + i, t = t0 + 2 * tx;
        float v0 = 0.f, v1 = 0.f;
        if (c < a.C && t < a.T) {
            const uint32_t row = (uint32_t)b * (uint32_t)a.C + (uint32_t)c;
            const size_t o = (size_t)row * a.T + t;
            const bool two = t + 1 < a.T;
            // (TIME) does the element have a source x[t - sh] inside the row - if not it is +0, and takes no noise
            bool in0 = true, in1 = two;
            if constexpr (TIME) {
                const int ts = t - sh;
                in0 = ts >= 0 && ts < a.T;
                in1 = two && ts + 1 >= 0 && ts + 1 < a.T;
                const float* xr = a.x + (size_t)row * a.T;
                if (in0) v0 = xr[ts];
                if (in1) v1 = xr[ts + 1];
            } else {
                v0 = a.x[o];
                if (two) v1 = a.x[o + 1];
            }
            if (scale != 0.f) aug_add_noise(v0, v1, two, a.s_ga, a.s_gb, row * half_t + (uint32_t)(t >> 1), scale);
            if constexpr (TIME) {
                if (gain_on) { v0 = v0 * gain; v1 = v1 * gain; }
                if (!in0 || (t >= m0 && t < m0 + mlen)) v0 = 0.f;
                if (!in1 || (t + 1 >= m0 && t + 1 < m0 + mlen)) v1 = 0.f;
            }
            if (drop_on && ((hdr[AUG_HDR + (c >> 5)] >> (c & 31)) & 1u)) v0 = v1 = 0.f;
            if (a.out) {
                a.out[o] = v0;
                if (two) a.out[o + 1] = v1;
            }
        }
        tile[i][2 * tx] = v0;
        tile[i][2 * tx + 1] = v1;
    }
    if (!a.y) return;
    __syncthreads();
    const int px = threadIdx.x & 31, py = threadIdx.x >> 5;
    for (int i = py; i < 32; i += 8) {
        const int t = t0 + i, c = c0 + px;
        if (t < a.T && c < a.Cp) a.y[((size_t)b * a.T + t) * a.Cp + c] = (bf16)tile[px][i];
    }
}

int aug_check_shape(const char* who, int B, int C, int T) {
    MM_REQUIRE(B > 0 && C > 0 && T > 0, "%s: bad shape", who);
    MM_REQUIRE((int64_t)C * T >= 2, "%s: a sample needs C * T >= 2 values for its standard deviation", who);
    MM_REQUIRE((int64_t)B * C * ((T + 1) / 2) < (1ll << 32), "%s: B * C * ceil(T / 2) must be below 2^32 (the stream's index)", who);
    return MM_OK;
}

// the launch of both staging entry points; tm: the time transforms of mm_stage_inputs_taug (the plan may then be null)
int stage_aug_launch(const char* who, const TimeAugArgs* tm, const float* eeg, uint32_t* plan, int64_t plan_words, void* eeg_packed_bf16,
                     float* eeg_out_f32, int B, int C, int T, int Cp, float noise_factor, uint32_t s_gauss_a, uint32_t s_gauss_b,
                     float* fmri_dst, const float* fmri_src, int64_t fmri_n, hipStream_t st) {
    if (plan || !tm) {
        if (int rc = aug_check_shape(who, B, C, T)) return rc;
    } else {
        MM_REQUIRE(B > 0 && C > 0 && T > 0, "%s: bad shape", who);
        MM_REQUIRE((int64_t)B * C < (1ll << 32), "%s: B * C must be below 2^32 (the kernel's row index)", who);
    }
    MM_REQUIRE(eeg && (plan || tm) && ((uintptr_t)plan & 7) == 0 && (eeg_packed_bf16 || eeg_out_f32) && eeg_out_f32 != eeg,
               "%s: bad EEG args (a batch, a plan and at least one output, not in place)", who);
    MM_REQUIRE(Cp >= C && Cp % 16 == 0, "%s: bad EEG args (Cp)", who);
    MM_REQUIRE(noise_factor >= 0.f, "%s: noise_factor must not be negative", who);
    AugShape s = {0, 0, 0, 0};
    if (plan) {
        s = aug_shape(B, C, T);
        MM_REQUIRE(plan_words >= s.words, "%s: the plan needs %lld words", who, (long long)s.words);
    }
    const bool copy = fmri_dst || fmri_src || fmri_n;
    if (copy)
        MM_REQUIRE(fmri_dst && fmri_src && fmri_n > 0 && fmri_n % 4 == 0 && (((uintptr_t)fmri_dst | (uintptr_t)fmri_src) & 15) == 0,
                   "%s: fMRI copy needs 16-byte alignment and a multiple of 4 floats", who);
    StageAugArgs a = {};
    a.tcw = ceil_div(eeg_packed_bf16 ? Cp : C, 32);
    const int64_t npack = (int64_t)B * ceil_div(T, 32) * a.tcw;
    const long n4 = copy ? fmri_n / 4 : 0;
    const int ncopy = (int)((n4 + 1023) / 1024 < 1024 ? (n4 + 1023) / 1024 : 1024);
    MM_REQUIRE(npack + ncopy < (1ll << 31), "%s: too many workgroups", who);
    a.x = eeg; a.plan = plan; a.y = (bf16*)eeg_packed_bf16; a.out = eeg_out_f32;
    a.B = B; a.C = C; a.T = T; a.Cp = Cp; a.stride = s.stride; a.nchunk = s.nchunk; a.npack = (int)npack;
    a.noise_factor = noise_factor; a.s_ga = s_gauss_a; a.s_gb = s_gauss_b;
    a.d1 = reinterpret_cast<float4*>(fmri_dst); a.s1 = reinterpret_cast<const float4*>(fmri_src); a.n1 = (size_t)n4;
    if (tm) {
        a.tm = *tm;
        hipLaunchKernelGGL(stage_inputs_aug_kernel<true>, dim3((unsigned)(npack + ncopy)), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(stage_inputs_aug_kernel<false>, dim3((unsigned)(npack + ncopy)), dim3(256), 0, st, a);
    }
    return mm_check_launch(who);
}

}  // namespace

extern "C" {

int mm_eeg_augment_plan(const float* x, uint32_t* plan, int64_t plan_words, int B, int C, int T, float p_noise, float p_drop,
                        int n_drop, uint32_t s_noise, uint32_t s_drop, uint32_t s_keys, hipStream_t st) {
    if (int rc = aug_check_shape("eeg_augment_plan", B, C, T)) return rc;
    MM_REQUIRE(x && plan && ((uintptr_t)plan & 7) == 0, "eeg_augment_plan: null batch or plan (the plan is 8-byte aligned)");
    MM_REQUIRE(p_noise >= 0.f && p_noise <= 1.f && p_drop >= 0.f && p_drop <= 1.f, "eeg_augment_plan: probabilities lie in [0, 1]");
    MM_REQUIRE(n_drop >= 1 && n_drop <= C, "eeg_augment_plan: n_drop must lie in [1, C]");
    const AugShape s = aug_shape(B, C, T);
    MM_REQUIRE(plan_words >= s.words, "eeg_augment_plan: the plan needs %lld words", (long long)s.words);
    MM_REQUIRE((int64_t)B * s.nchunk < (1ll << 31), "eeg_augment_plan: too many workgroups");
    PlanArgs a;
    a.x = x; a.plan = plan; a.B = B; a.C = C; a.T = T; a.stride = s.stride; a.chunk = s.chunk; a.nchunk = s.nchunk;
    a.n_drop = n_drop;
    a.vec = ((int64_t)C * T) % 4 == 0 && ((uintptr_t)x & 15) == 0;
    a.t_noise = aug_thresh(p_noise); a.t_drop = aug_thresh(p_drop);
    a.s_noise = s_noise; a.s_drop = s_drop; a.s_keys = s_keys;
    hipLaunchKernelGGL(eeg_augment_plan_kernel, dim3(B * s.nchunk), dim3(256), 0, st, a);
    return mm_check_launch("eeg_augment_plan");
}

int mm_stage_inputs_aug(const float* eeg, uint32_t* plan, int64_t plan_words, void* eeg_packed_bf16, float* eeg_out_f32, int B,
                        int C, int T, int Cp, float noise_factor, uint32_t s_gauss_a, uint32_t s_gauss_b, float* fmri_dst,
                        const float* fmri_src, int64_t fmri_n, hipStream_t st) {
    return stage_aug_launch("stage_inputs_aug", nullptr, eeg, plan, plan_words, eeg_packed_bf16, eeg_out_f32, B, C, T, Cp, noise_factor,
                            s_gauss_a, s_gauss_b, fmri_dst, fmri_src, fmri_n, st);
}

int mm_stage_inputs_taug(const float* eeg, uint32_t* plan, int64_t plan_words, void* eeg_packed_bf16, float* eeg_out_f32, int B,
                         int C, int T, int Cp, float noise_factor, uint32_t s_gauss_a, uint32_t s_gauss_b, float p_shift,
                         int max_shift, float p_scale, float scale_range, float p_invert, float p_mask, int mask_len,
                         uint32_t s_shift, uint32_t s_shift_amt, uint32_t s_scale, uint32_t s_scale_u, uint32_t s_invert,
                         uint32_t s_mask, uint32_t s_mask_start, int32_t* time_plan, float* fmri_dst, const float* fmri_src,
                         int64_t fmri_n, hipStream_t st) {
    MM_REQUIRE(B > 0 && C > 0 && T > 0, "stage_inputs_taug: bad shape");
    MM_REQUIRE(p_shift >= 0.f && p_shift <= 1.f && p_scale >= 0.f && p_scale <= 1.f && p_invert >= 0.f && p_invert <= 1.f &&
               p_mask >= 0.f && p_mask <= 1.f, "stage_inputs_taug: probabilities lie in [0, 1]");
    MM_REQUIRE(max_shift >= 0 && max_shift < T, "stage_inputs_taug: max_shift must lie in [0, T)");
    MM_REQUIRE(scale_range >= 0.f && scale_range < 1.f, "stage_inputs_taug: scale_range must lie in [0, 1)");
    MM_REQUIRE(mask_len >= 1 && mask_len <= T, "stage_inputs_taug: the mask length must lie in [1, T]");
    if (eeg && eeg_out_f32) {                        // the shift is a gather: it cannot run in place, or into a part of its source
        const uintptr_t x0 = (uintptr_t)eeg, o0 = (uintptr_t)eeg_out_f32, n = (uintptr_t)B * C * T * sizeof(float);
        MM_REQUIRE(x0 + n <= o0 || o0 + n <= x0, "stage_inputs_taug: the batch and the fp32 output overlap (the shift is a gather)");
    }
    TimeAugArgs tm;
    tm.t_shift = aug_thresh(p_shift); tm.t_scale = aug_thresh(p_scale); tm.t_invert = aug_thresh(p_invert); tm.t_mask = aug_thresh(p_mask);
    tm.s_shift = s_shift; tm.s_shift_amt = s_shift_amt; tm.s_scale = s_scale; tm.s_scale_u = s_scale_u; tm.s_invert = s_invert;
    tm.s_mask = s_mask; tm.s_mask_start = s_mask_start;
    tm.max_shift = max_shift; tm.mask_len = mask_len; tm.scale_range = scale_range; tm.time_plan = time_plan;
    return stage_aug_launch("stage_inputs_taug", &tm, eeg, plan, plan_words, eeg_packed_bf16, eeg_out_f32, B, C, T, Cp, noise_factor,
                            s_gauss_a, s_gauss_b, fmri_dst, fmri_src, fmri_n, st);
}

}  // extern "C"
