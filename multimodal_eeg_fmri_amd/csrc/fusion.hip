// The modality-fusion kernels of the tabular / bridge / V4 classifiers (forward and backward, fp32): the two-way
// softmax-weighted concat, LearnedFusionModule's mix, the one-query cross-attention cores (two keys; K <= 4 keys) and
// HybridFusionModule's gate.  Callers: ops.py (the eval-mode forwards) and small_autograd.py (the training tape).
#include "common.h"

namespace {
// out[b] = [ w0 * a[b][:Ha] | w1 * c[b][:Hc] ],  (w0, w1) = softmax(pa[0], pc[0])   (fmri_utils.py:93-96)
__global__ void softmax2_concat_kernel(const float* __restrict__ a, const float* __restrict__ c,
                                       const float* __restrict__ pa, const float* __restrict__ pc,
                                       float* __restrict__ out, int B, int Ha, int Hc) {
    const float m = fmaxf(pa[0], pc[0]);
    const float ea = __expf(pa[0] - m), ec = __expf(pc[0] - m);
    const float w0 = ea / (ea + ec), w1 = ec / (ea + ec);
    const int H = Ha + Hc;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * H; i += gridDim.x * blockDim.x) {
        const int b = i / H, j = i % H;
        out[i] = j < Ha ? w0 * a[(size_t)b * Ha + j] : w1 * c[(size_t)b * Hc + (j - Ha)];
    }
}
}  // namespace

extern "C" {
int mm_softmax2_concat(const float* a, const float* c, const float* pa, const float* pc, float* out, int B, int Ha,
                       int Hc, hipStream_t st) {
    MM_REQUIRE(a && c && pa && pc && out && B > 0 && Ha > 0 && Hc > 0, "softmax2_concat: null");
    hipLaunchKernelGGL(softmax2_concat_kernel, dim3(grid_for((size_t)B * (Ha + Hc), 2048)), dim3(256), 0, st, a, c, pa, pc, out, B, Ha, Hc);
    return mm_check_launch("softmax2_concat");
}
}  // extern "C"

namespace {
// backward of softmax2_concat: d a, d c and the two scalar weight-logit gradients
__global__ void softmax2_concat_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ a,
                                           const float* __restrict__ c, const float* __restrict__ pa,
                                           const float* __restrict__ pc, float* __restrict__ da, float* __restrict__ dc,
                                           float* __restrict__ dpa, float* __restrict__ dpc, int B, int Ha, int Hc) {
    const float m = fmaxf(pa[0], pc[0]);
    const float ea = __expf(pa[0] - m), ec = __expf(pc[0] - m);
    const float w0 = ea / (ea + ec), w1 = ec / (ea + ec);
    const int H = Ha + Hc;
    float s0 = 0.f, s1 = 0.f;
    for (int i = threadIdx.x; i < B * H; i += blockDim.x) {
        const int b = i / H, j = i % H;
        const float g = dout[i];
        if (j < Ha) { da[(size_t)b * Ha + j] = w0 * g; s0 += g * a[(size_t)b * Ha + j]; }
        else { dc[(size_t)b * Hc + (j - Ha)] = w1 * g; s1 += g * c[(size_t)b * Hc + (j - Ha)]; }
    }
    __shared__ float r0[16], r1[16];
    s0 = wave_sum(s0); s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) { r0[threadIdx.x >> 6] = s0; r1[threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t0 = 0.f, t1 = 0.f;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { t0 += r0[k]; t1 += r1[k]; }
        const float dot = w0 * t0 + w1 * t1;
        dpa[0] += w0 * (t0 - dot);
        dpc[0] += w1 * (t1 - dot);
    }
}
}  // namespace

extern "C" {
int mm_softmax2_concat_bwd(const float* dout, const float* a, const float* c, const float* pa, const float* pc,
                           float* da, float* dc, float* dpa, float* dpc, int B, int Ha, int Hc, hipStream_t st) {
    MM_REQUIRE(dout && a && c && pa && pc && da && dc && dpa && dpc && B > 0 && Ha > 0 && Hc > 0, "softmax2_concat_bwd: null");
    hipLaunchKernelGGL(softmax2_concat_bwd_kernel, dim3(1), dim3(1024), 0, st, dout, a, c, pa, pc, da, dc, dpa, dpc, B, Ha, Hc);
    return mm_check_launch("softmax2_concat_bwd");
}
}  // extern "C"

namespace {
// LearnedFusionModule tail (enhanced_models_v4.py:468-484): w = 0.5 softmax(logits/T) +
// 0.5 softmax(dyn[b]/T); fused[b] = sum_m w[b][m] feat_m[b].   M <= 4, one wave per row.
__global__ void learned_fusion_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                      const float* __restrict__ f2, const float* __restrict__ dyn,
                                      const float* __restrict__ logits, const float* __restrict__ temp,
                                      float* __restrict__ fused, float* __restrict__ wout, int B, int H, int M) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const float T = temp[0];
    float st[4], dy[4], w[4];
    float ms = -INFINITY, md = -INFINITY;
    for (int m = 0; m < M; ++m) {
        st[m] = logits[m] / T; dy[m] = dyn[(size_t)row * M + m] / T;
        ms = fmaxf(ms, st[m]); md = fmaxf(md, dy[m]);
    }
    float ss = 0.f, sd = 0.f;
    for (int m = 0; m < M; ++m) { st[m] = __expf(st[m] - ms); dy[m] = __expf(dy[m] - md); ss += st[m]; sd += dy[m]; }
    for (int m = 0; m < M; ++m) w[m] = 0.5f * st[m] / ss + 0.5f * dy[m] / sd;
    const float* fs[3] = {f0, f1, f2};
    for (int h = lane; h < H; h += 64) {
        float acc = 0.f;
        for (int m = 0; m < M; ++m) acc += w[m] * fs[m][(size_t)row * H + h];
        fused[(size_t)row * H + h] = acc;
    }
    if (lane < M && wout) wout[(size_t)row * M + lane] = w[lane];
}
}  // namespace

extern "C" {
int mm_learned_fusion(const float* f0, const float* f1, const float* f2, const float* dyn, const float* logits,
                      const float* temperature, float* fused, float* weights, int B, int H, int M, hipStream_t st) {
    MM_REQUIRE(f0 && f1 && dyn && logits && temperature && fused && B > 0 && H > 0, "learned_fusion: null");
    MM_REQUIRE(M >= 2 && M <= 3 && (M == 2 || f2), "learned_fusion: M=%d (2 or 3)", M);
    hipLaunchKernelGGL(learned_fusion_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, st, f0, f1, f2, dyn, logits,
                       temperature, fused, weights, B, H, M);
    return mm_check_launch("learned_fusion");
}
}  // extern "C"

namespace {
// backward of learned_fusion_kernel.  ONE block of 16 waves, a wave walks rows w, w + 16, ...; the parameter
// gradients (logits [M], temperature) are per-wave partials summed in wave order (no atomics: bit-reproducible).
__global__ __launch_bounds__(1024) void learned_fusion_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                          const float* __restrict__ f2, const float* __restrict__ dyn,
                                          const float* __restrict__ logits, const float* __restrict__ temp,
                                          const float* __restrict__ dfused, float* __restrict__ df0,
                                          float* __restrict__ df1, float* __restrict__ df2, float* __restrict__ ddyn,
                                          float* __restrict__ dlogits, float* __restrict__ dtemp, int B, int H, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const float T = temp[0];
    __shared__ float part[16][5];
    float pl[4] = {0.f, 0.f, 0.f, 0.f}, pT = 0.f;
    for (int row = wave; row < B; row += nwave) {
        float us[4], ud[4], st[4], dy[4], w[4], dw[4] = {0.f, 0.f, 0.f, 0.f};
        float ms = -INFINITY, md = -INFINITY;
        for (int m = 0; m < M; ++m) {
            us[m] = logits[m] / T; ud[m] = dyn[(size_t)row * M + m] / T;
            ms = fmaxf(ms, us[m]); md = fmaxf(md, ud[m]);
        }
        float ss = 0.f, sd = 0.f;
        for (int m = 0; m < M; ++m) { st[m] = __expf(us[m] - ms); dy[m] = __expf(ud[m] - md); ss += st[m]; sd += dy[m]; }
        for (int m = 0; m < M; ++m) { st[m] /= ss; dy[m] /= sd; w[m] = 0.5f * st[m] + 0.5f * dy[m]; }
        const float* fs[3] = {f0, f1, f2};
        float* dfs[3] = {df0, df1, df2};
        for (int h = lane; h < H; h += 64) {
            const float g = dfused[(size_t)row * H + h];
            for (int m = 0; m < M; ++m) {
                dw[m] += g * fs[m][(size_t)row * H + h];
                dfs[m][(size_t)row * H + h] = w[m] * g;
            }
        }
        for (int m = 0; m < M; ++m) dw[m] = wave_sum(dw[m]);
        if (lane == 0) {
            float dots = 0.f, dotd = 0.f;
            for (int m = 0; m < M; ++m) { dots += st[m] * dw[m]; dotd += dy[m] * dw[m]; }
            float dT = 0.f;
            for (int m = 0; m < M; ++m) {
                const float gs = 0.5f * st[m] * (dw[m] - dots);      // d L / d (logits_m / T)
                const float gd = 0.5f * dy[m] * (dw[m] - dotd);      // d L / d (dyn_m / T)
                ddyn[(size_t)row * M + m] = gd / T;
                pl[m] += gs / T;
                dT -= (gs * us[m] + gd * ud[m]) / T;
            }
            pT += dT;
        }
    }
    if (lane == 0) {
        for (int m = 0; m < 4; ++m) part[wave][m] = pl[m];
        part[wave][4] = pT;
    }
    __syncthreads();
    if (threadIdx.x <= M) {                              // threads 0..M-1: dlogits[m]; thread M: dtemp
        const int j = (int)threadIdx.x == M ? 4 : (int)threadIdx.x;
        float s = 0.f;
        for (int wv = 0; wv < nwave; ++wv) s += part[wv][j];
        if ((int)threadIdx.x == M) dtemp[0] += s;
        else dlogits[threadIdx.x] += s;
    }
}
}  // namespace

extern "C" {
int mm_learned_fusion_bwd(const float* f0, const float* f1, const float* f2, const float* dyn, const float* logits,
                          const float* temperature, const float* dfused, float* df0, float* df1, float* df2,
                          float* ddyn, float* dlogits, float* dtemp, int B, int H, int M, hipStream_t st) {
    MM_REQUIRE(f0 && f1 && dyn && logits && temperature && dfused && df0 && df1 && ddyn && dlogits && dtemp &&
               B > 0 && H > 0, "learned_fusion_bwd: null");
    MM_REQUIRE(M >= 2 && M <= 3 && (M == 2 || (f2 && df2)), "learned_fusion_bwd: M=%d", M);
    hipLaunchKernelGGL(learned_fusion_bwd_kernel, dim3(1), dim3(1024), 0, st, f0, f1, f2, dyn, logits,
                       temperature, dfused, df0, df1, df2, ddyn, dlogits, dtemp, B, H, M);
    return mm_check_launch("learned_fusion_bwd");
}
}  // extern "C"

namespace {
// bridge cross-attention core (bridge_utils.py:75-82): one query (EEG token) over two
// keys [EEG, fMRI], nhead heads of dh.  pe / pf = in_proj outputs [B][3E] (q|k|v) of the
// two tokens.  ctx [B][E], attw [B][2] = head-averaged probabilities.  Attention-probability
// dropout p (thresh != 0) is applied to the two probabilities before mixing, recomputed from
// (seed, b, h, key).  backward:
//   d proj_e [B][3E] = [dq | dk_e | dv_e],  d proj_f [B][3E] = [0 | dk_f | dv_f]
__global__ void attn_1x2_fused_kernel(const float* __restrict__ pe, const float* __restrict__ pf,
                                      const float* __restrict__ dctx, float* __restrict__ ctx,
                                      float* __restrict__ attw, float* __restrict__ dpe, float* __restrict__ dpf,
                                      int B, int E, int nhead, uint32_t thresh, uint32_t seed, float inv_keep,
                                      const uint32_t* epoch, int backward) {
    seed = mm_eff_seed(seed, epoch);
    const int b = blockIdx.x;
    const int dh = E / nhead;
    __shared__ float p0s[16], p1s[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* q = pe + (size_t)b * 3 * E;
    const float* ke = q + E; const float* ve = q + 2 * E;
    const float* kf = pf + (size_t)b * 3 * E + E; const float* vf = kf + E;
    const float isq = rsqrtf((float)dh);
    for (int h = wave; h < nhead; h += (blockDim.x >> 6)) {
        float s0 = 0.f, s1 = 0.f;
        for (int d = lane; d < dh; d += 64) { s0 += q[h * dh + d] * ke[h * dh + d]; s1 += q[h * dh + d] * kf[h * dh + d]; }
        s0 = wave_sum(s0) * isq; s1 = wave_sum(s1) * isq;
        const float m = fmaxf(s0, s1);
        const float e0 = __expf(s0 - m), e1 = __expf(s1 - m);
        const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
        float k0 = 1.f, k1 = 1.f;
        if (thresh) {
            k0 = dropout_scale(seed, (uint32_t)((b * nhead + h) * 2), thresh, inv_keep);
            k1 = dropout_scale(seed, (uint32_t)((b * nhead + h) * 2 + 1), thresh, inv_keep);
        }
        if (!backward) {
            for (int d = lane; d < dh; d += 64)
                ctx[(size_t)b * E + h * dh + d] = p0 * k0 * ve[h * dh + d] + p1 * k1 * vf[h * dh + d];
            if (lane == 0) { p0s[h] = p0; p1s[h] = p1; }
        } else {
            const float* dc = dctx + (size_t)b * E + h * dh;
            float dp0 = 0.f, dp1 = 0.f;
            for (int d = lane; d < dh; d += 64) { dp0 += dc[d] * ve[h * dh + d]; dp1 += dc[d] * vf[h * dh + d]; }
            dp0 = wave_sum(dp0) * k0; dp1 = wave_sum(dp1) * k1;
            const float dot = p0 * dp0 + p1 * dp1;
            const float ds0 = p0 * (dp0 - dot) * isq, ds1 = p1 * (dp1 - dot) * isq;
            float* dq = dpe + (size_t)b * 3 * E;
            float* dkf_ = dpf + (size_t)b * 3 * E;
            for (int d = lane; d < dh; d += 64) {
                const int i = h * dh + d;
                dq[i] = ds0 * ke[i] + ds1 * kf[i];
                dq[E + i] = ds0 * q[i];
                dq[2 * E + i] = p0 * k0 * dc[d];
                dkf_[i] = 0.f;
                dkf_[E + i] = ds1 * q[i];
                dkf_[2 * E + i] = p1 * k1 * dc[d];
            }
        }
    }
    if (!backward) {
        __syncthreads();
        if (threadIdx.x == 0 && attw) {
            float a0 = 0.f, a1 = 0.f;
            for (int h = 0; h < nhead; ++h) { a0 += p0s[h]; a1 += p1s[h]; }
            attw[2 * b] = a0 / nhead; attw[2 * b + 1] = a1 / nhead;
        }
    }
}
}  // namespace

extern "C" {
int mm_attn_1x2(const float* proj_e, const float* proj_f, float* ctx, float* attw, int B, int E, int nhead,
                hipStream_t st) {
    MM_REQUIRE(proj_e && proj_f && ctx && attw && B > 0 && nhead > 0 && nhead <= 16 && E % nhead == 0, "attn_1x2: bad args");
    hipLaunchKernelGGL(attn_1x2_fused_kernel, dim3(B), dim3(256), 0, st, proj_e, proj_f, nullptr, ctx, attw, nullptr, nullptr,
                       B, E, nhead, 0u, 0u, 1.f, nullptr, 0);          // no dropout, forward
    return mm_check_launch("attn_1x2");
}

int mm_attn_1x2_train(const float* proj_e, const float* proj_f, const float* dctx, float* ctx, float* attw,
                      float* dproj_e, float* dproj_f, int B, int E, int nhead, float drop_p, uint32_t seed,
                      const uint32_t* seed_epoch, int backward, hipStream_t st) {
    MM_REQUIRE(proj_e && proj_f && B > 0 && nhead > 0 && nhead <= 16 && E % nhead == 0, "attn_1x2_train: bad args");
    MM_REQUIRE(backward ? (dctx && dproj_e && dproj_f) : (ctx != nullptr), "attn_1x2_train: outputs");
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(attn_1x2_fused_kernel, dim3(B), dim3(256), 0, st, proj_e, proj_f, dctx, ctx, attw, dproj_e,
                       dproj_f, B, E, nhead, d.thresh, seed, d.inv_keep, seed_epoch, backward);
    return mm_check_launch("attn_1x2_train");
}
}  // extern "C"

namespace {
// nn.MultiheadAttention core with ONE query token and K <= 4 key/value tokens per sample (the
// modality-level cross attention of the V4 classifiers: crossmodal_v4_enhancements.py:366-372 K = 3,
// :448-456 K = 2).  p[j] = in_proj(token_j) [B][3E] = [q | k | v]; the query is token 0's q.
// Attention-probability dropout as in the 1x2 kernel (index (b * nhead + h) * K + j).
struct Attn1xKArgs {
    const float* p[4]; float* dp[4];
    const float* dctx; float* ctx; float* attw;
    int B, E, nhead, K; uint32_t thresh, seed; float inv_keep; const uint32_t* epoch; int backward;
};
__global__ __launch_bounds__(256) void attn_1xk_kernel(Attn1xKArgs a) {
    const uint32_t seed = mm_eff_seed(a.seed, a.epoch);
    const int b = blockIdx.x, E = a.E, K = a.K;
    const int dh = E / a.nhead;
    __shared__ float ps[16][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* q = a.p[0] + (size_t)b * 3 * E;
    const float isq = rsqrtf((float)dh);
    for (int h = wave; h < a.nhead; h += (blockDim.x >> 6)) {
        float s[4], pr[4], keep[4];
        float m = -INFINITY;
        for (int j = 0; j < K; ++j) {
            const float* kj = a.p[j] + (size_t)b * 3 * E + E;
            float acc = 0.f;
            for (int d = lane; d < dh; d += 64) acc += q[h * dh + d] * kj[h * dh + d];
            s[j] = wave_sum(acc) * isq;
            m = fmaxf(m, s[j]);
        }
        float den = 0.f;
        for (int j = 0; j < K; ++j) { pr[j] = __expf(s[j] - m); den += pr[j]; }
        for (int j = 0; j < K; ++j) {
            pr[j] /= den;
            keep[j] = a.thresh ? dropout_scale(seed, (uint32_t)((b * a.nhead + h) * K + j), a.thresh, a.inv_keep) : 1.f;
        }
        if (!a.backward) {
            for (int d = lane; d < dh; d += 64) {
                float acc = 0.f;
                for (int j = 0; j < K; ++j) acc += pr[j] * keep[j] * a.p[j][(size_t)b * 3 * E + 2 * E + h * dh + d];
                a.ctx[(size_t)b * E + h * dh + d] = acc;
            }
            if (lane == 0)
                for (int j = 0; j < K; ++j) ps[h][j] = pr[j];
        } else {
            const float* dc = a.dctx + (size_t)b * E + h * dh;
            float dp[4], dot = 0.f;
            for (int j = 0; j < K; ++j) {
                const float* vj = a.p[j] + (size_t)b * 3 * E + 2 * E + h * dh;
                float acc = 0.f;
                for (int d = lane; d < dh; d += 64) acc += dc[d] * vj[d];
                dp[j] = wave_sum(acc) * keep[j];
                dot += pr[j] * dp[j];
            }
            for (int d = lane; d < dh; d += 64) {
                const int i = h * dh + d;
                float dq = 0.f;
                for (int j = 0; j < K; ++j) {
                    const float ds = pr[j] * (dp[j] - dot) * isq;
                    dq += ds * a.p[j][(size_t)b * 3 * E + E + i];
                    float* o = a.dp[j] + (size_t)b * 3 * E;
                    if (j > 0) o[i] = 0.f;
                    o[E + i] = ds * q[i];
                    o[2 * E + i] = pr[j] * keep[j] * dc[d];
                }
                a.dp[0][(size_t)b * 3 * E + i] = dq;
            }
        }
    }
    if (!a.backward && a.attw) {
        __syncthreads();
        if (threadIdx.x < K) {
            float s = 0.f;
            for (int h = 0; h < a.nhead; ++h) s += ps[h][threadIdx.x];
            a.attw[(size_t)b * K + threadIdx.x] = s / a.nhead;
        }
    }
}
}  // namespace

extern "C" {
int mm_attn_1xk(const float* p0, const float* p1, const float* p2, const float* p3, int K, const float* dctx,
                float* ctx, float* attw, float* dp0, float* dp1, float* dp2, float* dp3, int B, int E, int nhead,
                float drop_p, uint32_t seed, const uint32_t* seed_epoch, int backward, hipStream_t st) {
    MM_REQUIRE(K >= 1 && K <= 4 && B > 0 && nhead > 0 && nhead <= 16 && E % nhead == 0, "attn_1xk: K=%d nhead=%d E=%d", K, nhead, E);
    Attn1xKArgs a{};
    const float* p[4] = {p0, p1, p2, p3};
    float* dp[4] = {dp0, dp1, dp2, dp3};
    for (int j = 0; j < K; ++j) {
        MM_REQUIRE(p[j] && (!backward || dp[j]), "attn_1xk: null token %d", j);
        a.p[j] = p[j]; a.dp[j] = dp[j];
    }
    MM_REQUIRE(backward ? dctx != nullptr : ctx != nullptr, "attn_1xk: outputs");
    a.dctx = dctx; a.ctx = ctx; a.attw = attw; a.B = B; a.E = E; a.nhead = nhead; a.K = K;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.seed = seed; a.inv_keep = d.inv_keep; a.epoch = seed_epoch; a.backward = backward;
    hipLaunchKernelGGL(attn_1xk_kernel, dim3(B), dim3(256), 0, st, a);
    return mm_check_launch("attn_1xk");
}
}  // extern "C"

namespace {
// HybridFusionModule mix (crossmodal_v4_enhancements.py:787-797):
// gate = softmax(g[b][0:2]); comb[b] = [ gate0*erp + gate1*pw | conn * boost ]
__global__ void gate2_mix_kernel(const float* __restrict__ g, const float* __restrict__ erp, const float* __restrict__ pw,
                                 const float* __restrict__ conn, float* __restrict__ comb, float* __restrict__ gate,
                                 int B, int H, float boost) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * 2 * H; i += gridDim.x * blockDim.x) {
        const int b = i / (2 * H), j = i % (2 * H);
        const float g0 = g[2 * b], g1 = g[2 * b + 1], m = fmaxf(g0, g1);
        const float e0 = expf(g0 - m), e1 = expf(g1 - m);    // expf: __expf is off by |x| 2^-24 relative, a far gate logit's weight
        const float w0 = e0 / (e0 + e1), w1 = e1 / (e0 + e1);
        comb[i] = j < H ? w0 * erp[(size_t)b * H + j] + w1 * pw[(size_t)b * H + j] : conn[(size_t)b * H + (j - H)] * boost;
        if (j == 0 && gate) { gate[2 * b] = w0; gate[2 * b + 1] = w1; }
    }
}
}  // namespace

extern "C" {
int mm_gate2_mix(const float* g, const float* erp, const float* pw, const float* conn, float* comb, float* gate, int B,
                 int H, float boost, hipStream_t st) {
    MM_REQUIRE(g && erp && pw && conn && comb && B > 0 && H > 0, "gate2_mix: null");
    hipLaunchKernelGGL(gate2_mix_kernel, dim3(grid_for((size_t)B * 2 * H, 2048)), dim3(256), 0, st, g, erp, pw, conn, comb, gate, B, H, boost);
    return mm_check_launch("gate2_mix");
}
}  // extern "C"

namespace {
// backward of gate2_mix: given d comb [B][2H] -> d erp, d pw, d conn [B][H], d gate logits [B][2]
__global__ void gate2_mix_bwd_kernel(const float* __restrict__ dcomb, const float* __restrict__ g,
                                     const float* __restrict__ erp, const float* __restrict__ pw,
                                     float* __restrict__ derp, float* __restrict__ dpw, float* __restrict__ dconn,
                                     float* __restrict__ dg, int B, int H, float boost) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const float g0 = g[2 * b], g1 = g[2 * b + 1], m = fmaxf(g0, g1);
    const float e0 = expf(g0 - m), e1 = expf(g1 - m);        // the forward's expression: the same weights
    const float w0 = e0 / (e0 + e1), w1 = e1 / (e0 + e1);
    float a0 = 0.f, a1 = 0.f;
    for (int h = lane; h < H; h += 64) {
        const float dm = dcomb[(size_t)b * 2 * H + h];
        derp[(size_t)b * H + h] = w0 * dm;
        dpw[(size_t)b * H + h] = w1 * dm;
        dconn[(size_t)b * H + h] = boost * dcomb[(size_t)b * 2 * H + H + h];
        a0 += dm * erp[(size_t)b * H + h];
        a1 += dm * pw[(size_t)b * H + h];
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1);
    if (lane == 0) {
        const float dot = w0 * a0 + w1 * a1;
        dg[2 * b] = w0 * (a0 - dot);
        dg[2 * b + 1] = w1 * (a1 - dot);
    }
}
}  // namespace

extern "C" {
int mm_gate2_mix_bwd(const float* dcomb, const float* g, const float* erp, const float* pw, float* derp, float* dpw,
                     float* dconn, float* dg, int B, int H, float boost, hipStream_t st) {
    MM_REQUIRE(dcomb && g && erp && pw && derp && dpw && dconn && dg && B > 0 && H > 0, "gate2_mix_bwd: null");
    hipLaunchKernelGGL(gate2_mix_bwd_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, st, dcomb, g, erp, pw, derp, dpw, dconn, dg, B, H, boost);
    return mm_check_launch("gate2_mix_bwd");
}
}  // extern "C"
