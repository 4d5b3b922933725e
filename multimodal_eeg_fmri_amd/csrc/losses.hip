// The three classification losses with their logit gradients, one workgroup each (B is a batch size): class-weighted
// cross entropy, focal loss, label-smoothed cross entropy.  Callers: small_autograd.py (weighted_ce, focal_loss,
// smoothed_ce).
// Labels: every kernel compares the 64-bit label with [0, C) before anything is indexed with it (label_ok); a row whose
// label is outside (-100, C, 2^32 + 1) is dropped: nothing read through the label, no loss term, a zero gradient row.
#include "common.h"

namespace {
__device__ __forceinline__ bool label_ok(long long t, int C) { return t >= 0 && t < (long long)C; }

// nn.CrossEntropyLoss(weight=w): loss = sum_b w[t_b] nll_b / sum_b w[t_b]   (single block, B small); both sums run over
// the rows with a label in [0, C) only (ignore_index for every label outside)
__global__ void weighted_ce_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                   const float* __restrict__ cw, float* __restrict__ out, float* __restrict__ dlogits,
                                   int B, int C) {
    __shared__ float wsum_s;
    if (threadIdx.x == 0) {
        float ws = 0.f, ls = 0.f;
        for (int b = 0; b < B; ++b) {
            const float* z = logits + (size_t)b * C;
            float m = -INFINITY;
            for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += __expf(z[c] - m);
            const long long t = target[b];
            if (!label_ok(t, C)) continue;                   // dropped row: weight 0 in both sums (ignore_index)
            const float w = cw ? cw[t] : 1.f;
            ws += w; ls += w * (m + __logf(se) - z[t]);
        }
        wsum_s = ws;
        out[0] += ls / ws;
    }
    __syncthreads();
    if (!dlogits) return;
    for (int i = threadIdx.x; i < B * C; i += blockDim.x) {
        const int b = i / C, c = i % C;
        const long long t = target[b];
        if (!label_ok(t, C)) { dlogits[i] = 0.f; continue; }
        const float* z = logits + (size_t)b * C;
        float m = -INFINITY;
        for (int k = 0; k < C; ++k) m = fmaxf(m, z[k]);
        float se = 0.f;
        for (int k = 0; k < C; ++k) se += __expf(z[k] - m);
        const float w = cw ? cw[t] : 1.f;
        dlogits[i] = w * (__expf(z[c] - m) / se - (c == t ? 1.f : 0.f)) / wsum_s;
    }
}
}  // namespace

extern "C" {
int mm_weighted_ce(const float* logits, const void* target_i64, const float* class_weight, float* loss_out,
                   float* dlogits, int B, int C, hipStream_t st) {
    MM_REQUIRE(logits && target_i64 && loss_out && B > 0 && C > 0, "weighted_ce: bad args");
    hipLaunchKernelGGL(weighted_ce_kernel, dim3(1), dim3(256), 0, st, logits, (const long long*)target_i64, class_weight,
                       loss_out, dlogits, B, C);
    return mm_check_launch("weighted_ce");
}
}  // extern "C"

namespace {
// FocalLoss (CrossModal_EEG_scr.ipynb cell 20): ce_b = lse(z_b) - z_b[t_b]; pt = exp(-ce);
// fl_b = alpha (1 - pt)^gamma ce.  out[0] += scale * sum_b fl_b; per_sample[b] = fl_b (optional);
// dlogits[b][c] = d fl_b / d z_bc (un-reduced; the caller applies the reduction's factor).
__global__ void focal_loss_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                  float* __restrict__ out, float* __restrict__ per_sample,
                                  float* __restrict__ dlogits, int B, int C, float alpha, float gamma, float scale) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const long long t = target[b];
        if (!label_ok(t, C)) {                               // dropped row: fl_b = 0, zero gradient row
            if (per_sample) per_sample[b] = 0.f;
            if (dlogits)
                for (int c = 0; c < C; ++c) dlogits[(size_t)b * C + c] = 0.f;
            continue;
        }
        const float* z = logits + (size_t)b * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(z[c] - m);
        const float ce = m + __logf(se) - z[t];
        const float pt = __expf(-ce), q = fmaxf(1.f - pt, 0.f);
        const float qg = (gamma == 0.f) ? 1.f : powf(q, gamma);
        const float fl = alpha * qg * ce;
        if (per_sample) per_sample[b] = fl;
        acc += fl;
        if (dlogits) {
            const float qg1 = (gamma == 0.f || q <= 0.f) ? 0.f : gamma * powf(q, gamma - 1.f) * pt * ce;
            const float dce = alpha * (qg + qg1);
            for (int c = 0; c < C; ++c)
                dlogits[(size_t)b * C + c] = dce * (__expf(z[c] - m) / se - (c == t ? 1.f : 0.f));
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] += scale * red[0];
}
}  // namespace

extern "C" {
int mm_focal_loss(const float* logits, const void* target_i64, float* loss_out, float* per_sample, float* dlogits,
                  int B, int C, float alpha, float gamma, float scale, hipStream_t st) {
    MM_REQUIRE(logits && target_i64 && loss_out && B > 0 && C > 0, "focal_loss: bad args");
    hipLaunchKernelGGL(focal_loss_kernel, dim3(1), dim3(256), 0, st, logits, (const long long*)target_i64, loss_out,
                       per_sample, dlogits, B, C, alpha, gamma, scale);
    return mm_check_launch("focal_loss");
}
}  // extern "C"

namespace {
// LabelSmoothingCrossEntropy (crossmodal_v4_enhancements.py:665-677): loss = mean_b[(1-s)*nll + s*mean_c(-logp)]
// out[0] += loss ; dlogits[b][c] = (softmax - (1-s)*onehot - s/C) / B
__global__ void smoothed_ce_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                   float* __restrict__ out, float* __restrict__ dlogits, int B, int C, float smoothing) {
    // one block (B is a batch size): per-thread partial sums over rows b = tid, tid + 256, ..., then a
    // fixed-order tree over the 256 partials - the loss is bit-reproducible
    __shared__ float red[256];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const long long t = target[b];
        if (!label_ok(t, C)) {                               // dropped row: no term (the divisor stays B), zero gradient row
            if (dlogits)
                for (int c = 0; c < C; ++c) dlogits[(size_t)b * C + c] = 0.f;
            continue;
        }
        const float* z = logits + (size_t)b * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
        float se = 0.f, sz = 0.f;
        for (int c = 0; c < C; ++c) { se += __expf(z[c] - m); sz += z[c]; }
        const float lse = m + __logf(se);
        const float nll = lse - z[t], smooth = lse - sz / (float)C;
        acc += ((1.f - smoothing) * nll + smoothing * smooth) / (float)B;
        if (dlogits)
            for (int c = 0; c < C; ++c) {
                const float p = __expf(z[c] - m) / se;       // not exp(z - lse): lse is rounded at the size of |m|
                dlogits[(size_t)b * C + c] = (p - (c == t ? 1.f - smoothing : 0.f) - smoothing / (float)C) / (float)B;
            }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] += red[0];
}
}  // namespace

extern "C" {
int mm_smoothed_ce(const float* logits, const void* target_i64, float* loss_out, float* dlogits, int B, int C,
                   float smoothing, hipStream_t st) {
    MM_REQUIRE(logits && target_i64 && loss_out && B > 0 && C > 0 && smoothing >= 0.f && smoothing < 1.f, "smoothed_ce: bad args");
    hipLaunchKernelGGL(smoothed_ce_kernel, dim3(1), dim3(256), 0, st, logits, (const long long*)target_i64,
                       loss_out, dlogits, B, C, smoothing);
    return mm_check_launch("smoothed_ce");
}
}  // extern "C"
