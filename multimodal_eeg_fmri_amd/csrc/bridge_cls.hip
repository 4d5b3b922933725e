// Classification branch of the EEG<->fMRI bridge (bridge_utils.py:22-114 of the reference: the EEG token attends over
// [EEG, fMRI], LearnedFusionModule, Linear -> LayerNorm -> ReLU -> Dropout -> Linear, class-weighted cross-entropy) on
// the rows the projection heads already produced: ONE forward launch (a workgroup per sample) and TWO backward
// launches (rows, then weights).  fp32 throughout, no floating-point atomics: every gradient element has one writer and
// every sum over rows runs in row order.  The eager composition this stands in for
// (ops.bridge_forward's train branch) is ~19 launches forward and more backward and cannot sit in the captured step.
// Callers: ops.bridge_cls_forward_impl, autograd.bridge_cls_bwd.
//
// Dropout sites and their element indices (three seeds of their own, the same hash as everywhere: common.h):
//   attention probabilities  (b * H + h) * 2 + key      (the convention of mm_attn_1x2_train, fusion.hip)
//   gate hidden (p = 0.2)    b * N + n
//   classifier hidden        b * (N / 2) + n
// The two input tokens a_e / a_f are NOT a second evaluation of the projection heads: they are recomputed from the
// saved LayerNorm output `hn` of mm_proj_heads_fwd with its expression, seeds and indices (b * N + n).
#include "common.h"

namespace {
constexpr int CLS_MAXN = 256, CLS_MAXC = 16, CLS_MAXH = 16;

// per-row layout of the forward's save buffer (floats) ...
struct SaveL {
    int N, ae, att, af, pe, pf, ctx, g1, g, fused, c1, h, sm, stride;
    __host__ __device__ explicit SaveL(int n) : N(n) {
        ae = 0; att = n; af = 2 * n;                       // att | af adjacent = the gate net's concatenated input
        pe = 3 * n; pf = 6 * n; ctx = 9 * n; g1 = 10 * n; g = 11 * n; fused = 12 * n; c1 = 13 * n; h = 13 * n + n / 2;
        sm = 14 * n; stride = 14 * n + 48;
    }
};
// small values of a row at `sm`: p0[16] p1[16] (un-dropped probabilities per head), then
enum { SM_P0 = 0, SM_P1 = 16, SM_DYN = 32, SM_MEAN = 34, SM_RSTD = 35, SM_LSE = 36, SM_WNLL = 37, SM_W = 38, SM_OK = 39 };
// ... and of the rows launch's gradient buffer: the gradient at every Linear's output plus the per-row pieces of the
// LayerNorm / fusion_logits / temperature gradients
struct GradL {
    int dpe, dpf, datt, dg1, dc1, dgam, dbet, dlog, ddyn, dfl, dT, stride;
    __host__ __device__ explicit GradL(int n) {
        dpe = 0; dpf = 3 * n; datt = 6 * n; dg1 = 7 * n; dc1 = 8 * n; dgam = 8 * n + n / 2; dbet = 9 * n;
        dlog = 9 * n + n / 2; ddyn = dlog + 16; dfl = dlog + 18; dT = dlog + 20; stride = dlog + 24;
    }
};

struct ClsDrop { uint32_t thresh; float inv_keep; uint32_t seed; };
struct ClsParams {
    const float *in_w, *in_b, *out_w, *out_b, *g0_w, *g0_b, *g3_w, *g3_b, *fl, *temp, *c0_w, *c0_b, *ln_g, *ln_b, *c4_w, *c4_b;
};
struct ClsFwdArgs {
    const float* hn; ClsParams p; const int* labels; const float* cw; float ce_weight;
    float *logits, *fw, *aw, *save, *loss; int* ticket;
    int B, N, H, C; float eps;
    ClsDrop dhead; uint32_t seed_e, seed_f; ClsDrop datt, dgate, dcls; const uint32_t* epoch;
};

__device__ __forceinline__ float cls_block_sum(float v, float* red /* [4] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// y[r] = W[r][:] . x (+ bias[r]) for r < R, and the same row against x2 when given; x / x2 in LDS, K % 4 == 0.  Sixteen
// lanes share a row (256 contiguous bytes per load round) and the row sum is four DPP adds; a thread works on EIGHT rows
// at a time (128 per pass) so that eight independent loads are in flight per round: the chain is load latency, not flops.
__device__ __forceinline__ float4 ld4(const float* p, bool v4) {
    if (v4) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);              // a weight inside a flat bucket may sit at any float
}
template <class Store>
__device__ __forceinline__ void dense_rows(const float* __restrict__ W, const float* __restrict__ bias, const float* x,
                                           const float* x2, int R, int K, Store&& store) {
    constexpr int U = 8;
    const int part = threadIdx.x & 15, r0 = threadIdx.x >> 4;
    const bool v4 = (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    for (int base = 0; base < R; base += 16 * U) {
        float a[U], a2[U];
        const float* wr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = base + u * 16 + r0;
            a[u] = 0.f; a2[u] = 0.f;
            wr[u] = W + (size_t)(r < R ? r : R - 1) * K;      // (rows past the end re-read the last one; never stored)
        }
        for (int k = part * 4; k < K; k += 64) {
            float4 w4[U];
#pragma unroll
            for (int u = 0; u < U; ++u) w4[u] = ld4(wr[u] + k, v4);
            const float x0 = x[k], x1 = x[k + 1], x2_ = x[k + 2], x3 = x[k + 3];
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] += w4[u].x * x0 + w4[u].y * x1 + w4[u].z * x2_ + w4[u].w * x3;
            if (x2) {
                const float y0 = x2[k], y1 = x2[k + 1], y2 = x2[k + 2], y3 = x2[k + 3];
#pragma unroll
                for (int u = 0; u < U; ++u) a2[u] += w4[u].x * y0 + w4[u].y * y1 + w4[u].z * y2 + w4[u].w * y3;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = base + u * 16 + r0;
            const float s1 = row16_sum(a[u]), s2 = row16_sum(a2[u]);
            if (r < R && part == 0) {
                const float bv = bias ? bias[r] : 0.f;
                store(r, s1 + bv, s2 + bv);
            }
        }
    }
}

// static half of the fusion weights and the dynamic half of one row (learned_fusion_kernel's expressions, M = 2)
struct Fus2 { float T, us[2], ud[2], st[2], dy[2], w[2]; };
__device__ __forceinline__ Fus2 fusion2(const float* fl, const float* temp, float dyn0, float dyn1) {
    Fus2 f;
    f.T = temp[0];
    f.us[0] = fl[0] / f.T; f.us[1] = fl[1] / f.T; f.ud[0] = dyn0 / f.T; f.ud[1] = dyn1 / f.T;
    const float ms = fmaxf(f.us[0], f.us[1]), md = fmaxf(f.ud[0], f.ud[1]);
    f.st[0] = __expf(f.us[0] - ms); f.st[1] = __expf(f.us[1] - ms);
    f.dy[0] = __expf(f.ud[0] - md); f.dy[1] = __expf(f.ud[1] - md);
    const float ss = f.st[0] + f.st[1], sd = f.dy[0] + f.dy[1];
    for (int m = 0; m < 2; ++m) { f.st[m] /= ss; f.dy[m] /= sd; f.w[m] = 0.5f * f.st[m] + 0.5f * f.dy[m]; }
    return f;
}

__global__ __launch_bounds__(256) void bridge_cls_fwd_kernel(ClsFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ae[CLS_MAXN], cat[2 * CLS_MAXN], pe[3 * CLS_MAXN], pf[3 * CLS_MAXN],
        ctx[CLS_MAXN], g[CLS_MAXN], fused[CLS_MAXN], c1s[CLS_MAXN / 2], hs[CLS_MAXN / 2];
    __shared__ float lg[CLS_MAXC], p0s[CLS_MAXH], p1s[CLS_MAXH], pk0[CLS_MAXH], pk1[CLS_MAXH], dyn[2], red[4];
    __shared__ int last;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, N2 = a.N / 2, H = a.H, C = a.C, B = a.B;
    const SaveL L(N);
    float* sv = a.save + (size_t)b * L.stride;
    const ClsParams& p = a.p;
    // 1. the two tokens, as proj_heads_fwd_kernel formed them
    if (tid < N) {
        const float he = a.hn[((size_t)0 * B + b) * N + tid], hf = a.hn[((size_t)1 * B + b) * N + tid];
        float ve = gelu_erf(he), vf = gelu_erf(hf);
        if (a.dhead.thresh) {
            ve *= dropout_scale(mm_eff_seed(a.seed_e, a.epoch), (uint32_t)(b * N + tid), a.dhead.thresh, a.dhead.inv_keep);
            vf *= dropout_scale(mm_eff_seed(a.seed_f, a.epoch), (uint32_t)(b * N + tid), a.dhead.thresh, a.dhead.inv_keep);
        }
        ae[tid] = ve; cat[N + tid] = vf;
        sv[L.ae + tid] = ve; sv[L.af + tid] = vf;
    }
    __syncthreads();
    // 2. in_proj of both tokens: pe = [q | k_e | v_e], pf = [(unused) | k_f | v_f]
    dense_rows(p.in_w, p.in_b, ae, cat + N, 3 * N, N, [&](int r, float ye, float yf) {
        pe[r] = ye; pf[r] = yf; sv[L.pe + r] = ye; sv[L.pf + r] = yf;
    });
    __syncthreads();
    // 3. 1 x 2 attention per head: sixteen lanes per head
    {
        const int h = tid >> 4, part = tid & 15, dh = N / H;
        float s0 = 0.f, s1 = 0.f;
        if (h < H)
            for (int d = part; d < dh; d += 16) {
                const int i = h * dh + d;
                s0 += pe[i] * pe[N + i]; s1 += pe[i] * pf[N + i];
            }
        s0 = row16_sum(s0); s1 = row16_sum(s1);
        if (h < H && part == 0) {
            const float isq = rsqrtf((float)dh);
            s0 *= isq; s1 *= isq;
            const float m = fmaxf(s0, s1), e0 = __expf(s0 - m), e1 = __expf(s1 - m);
            const float p0 = e0 / (e0 + e1), p1 = e1 / (e0 + e1);
            float k0 = 1.f, k1 = 1.f;
            if (a.datt.thresh) {
                const uint32_t seed = mm_eff_seed(a.datt.seed, a.epoch);
                k0 = dropout_scale(seed, (uint32_t)((b * H + h) * 2), a.datt.thresh, a.datt.inv_keep);
                k1 = dropout_scale(seed, (uint32_t)((b * H + h) * 2 + 1), a.datt.thresh, a.datt.inv_keep);
            }
            p0s[h] = p0; p1s[h] = p1; pk0[h] = p0 * k0; pk1[h] = p1 * k1;
            sv[L.sm + SM_P0 + h] = p0; sv[L.sm + SM_P1 + h] = p1;
        }
    }
    __syncthreads();
    if (tid < N) {
        const int h = tid / (N / H);
        const float c = pk0[h] * pe[2 * N + tid] + pk1[h] * pf[2 * N + tid];
        ctx[tid] = c; sv[L.ctx + tid] = c;
    }
    if (tid == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int h = 0; h < H; ++h) { a0 += p0s[h]; a1 += p1s[h]; }
        a.aw[2 * b] = a0 / H; a.aw[2 * b + 1] = a1 / H;
    }
    __syncthreads();
    // 4. out_proj -> the attended EEG token, first half of the gate net's input
    dense_rows(p.out_w, p.out_b, ctx, nullptr, N, N, [&](int r, float y, float) { cat[r] = y; sv[L.att + r] = y; });
    __syncthreads();
    // 5. gate net: Linear(2N -> N), GELU, Dropout, Linear(N -> 2)
    {
        const uint32_t seed = mm_eff_seed(a.dgate.seed, a.epoch);
        dense_rows(p.g0_w, p.g0_b, cat, nullptr, N, 2 * N, [&](int r, float y, float) {
            float v = gelu_erf(y);
            if (a.dgate.thresh) v *= dropout_scale(seed, (uint32_t)(b * N + r), a.dgate.thresh, a.dgate.inv_keep);
            g[r] = v; sv[L.g1 + r] = y; sv[L.g + r] = v;
        });
    }
    __syncthreads();
    dense_rows(p.g3_w, p.g3_b, g, nullptr, 2, N, [&](int r, float y, float) { dyn[r] = y; sv[L.sm + SM_DYN + r] = y; });
    __syncthreads();
    // 6. fusion weights and the fused row
    {
        const Fus2 f = fusion2(p.fl, p.temp, dyn[0], dyn[1]);
        if (tid < N) {
            const float v = f.w[0] * cat[tid] + f.w[1] * cat[N + tid];
            fused[tid] = v; sv[L.fused + tid] = v;
        }
        if (tid < 2) a.fw[2 * b + tid] = f.w[tid];
    }
    __syncthreads();
    // 7. classifier: Linear -> LayerNorm -> ReLU -> Dropout -> Linear
    dense_rows(p.c0_w, p.c0_b, fused, nullptr, N2, N, [&](int r, float y, float) { c1s[r] = y; sv[L.c1 + r] = y; });
    __syncthreads();
    {
        const bool on = tid < N2;
        const float x1 = on ? c1s[tid] : 0.f;
        const float mean = cls_block_sum(x1, red) / N2;
        const float dlt = on ? x1 - mean : 0.f;
        const float rstd = rsqrtf(cls_block_sum(dlt * dlt, red) / N2 + a.eps);
        if (on) {
            float v = fmaxf(dlt * rstd * p.ln_g[tid] + p.ln_b[tid], 0.f);
            if (a.dcls.thresh)
                v *= dropout_scale(mm_eff_seed(a.dcls.seed, a.epoch), (uint32_t)(b * N2 + tid), a.dcls.thresh, a.dcls.inv_keep);
            hs[tid] = v; sv[L.h + tid] = v;
        }
        if (tid == 0) { sv[L.sm + SM_MEAN] = mean; sv[L.sm + SM_RSTD] = rstd; }
    }
    __syncthreads();
    dense_rows(p.c4_w, p.c4_b, hs, nullptr, C, N2, [&](int r, float y, float) { lg[r] = y; a.logits[(size_t)b * C + r] = y; });
    __syncthreads();
    // 8. the row's cross-entropy terms; the block that finishes last sums them over the rows in row order
    if (tid == 0) {
        float mx = lg[0];
        int am = 0;
        for (int c = 1; c < C; ++c) if (lg[c] > mx) { mx = lg[c]; am = c; }       // first maximum, as torch.argmax
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(lg[c] - mx);
        const float lse = mx + __logf(se);
        sv[L.sm + SM_LSE] = lse;
        int is_last = 0;
        if (a.labels) {
            const int y = a.labels[b];
            const bool ok = y >= 0 && y < C;                   // a label outside [0, C) indexes nothing: the row weighs 0
            const float w = ok ? (a.cw ? a.cw[y] : 1.f) : 0.f;
            sv[L.sm + SM_W] = w;
            sv[L.sm + SM_WNLL] = ok ? w * (lse - lg[y]) : 0.f;
            sv[L.sm + SM_OK] = ok && am == y ? 1.f : 0.f;
            __threadfence();
            is_last = atomicAdd(a.ticket, 1) == B - 1;         // integer ticket; the arithmetic below has a fixed order
        }
        last = is_last;
    }
    __syncthreads();
    if (last && tid == 0) {
        __threadfence();
        float sn = 0.f, sw = 0.f, ok = 0.f;
        for (int r = 0; r < B; ++r) {                          // other blocks' stores: read past this CU's vector cache
            const float* q = a.save + (size_t)r * L.stride + L.sm;
            sn += __hip_atomic_load(q + SM_WNLL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sw += __hip_atomic_load(q + SM_W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok += __hip_atomic_load(q + SM_OK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const float ce = sw > 0.f ? sn / sw : 0.f;
        a.loss[0] = ce; a.loss[1] = ok; a.loss[2] = sw; a.loss[3] = a.ce_weight * ce;
        a.ticket[0] = 0;                                       // ready for the next launch (and the next graph replay)
    }
}

static bool cls_shape_ok(int B, int N, int H, int C) {
    return B > 0 && N >= 32 && N <= CLS_MAXN && N % 32 == 0 && H > 0 && H <= CLS_MAXH && N % H == 0 && C >= 2 && C <= CLS_MAXC;
}
static ClsDrop cls_drop(float p, uint32_t seed) {
    const DropH d = mm_drop(p);
    return ClsDrop{d.thresh, d.inv_keep, seed};
}
}  // namespace

extern "C" {
// floats per row of the forward's save buffer (which = 0) and of the backward's gradient-row workspace (which = 1)
int mm_bridge_cls_ws_floats(int B, int N, int which, int* out, hipStream_t) {
    MM_REQUIRE(out && B > 0 && N >= 32 && N <= CLS_MAXN && N % 32 == 0 && (which == 0 || which == 1), "bridge_cls_ws_floats: B=%d bridge_dim=%d", B, N);
    *out = B * (which == 0 ? SaveL(N).stride : GradL(N).stride);
    return MM_OK;
}

int mm_bridge_cls_fwd(const float* hn, float drop_p, uint32_t seed_e, uint32_t seed_f, const float* in_w,
                      const float* in_b, const float* out_w, const float* out_b, const float* g0_w, const float* g0_b,
                      const float* g3_w, const float* g3_b, const float* fusion_logits, const float* temperature,
                      const float* c0_w, const float* c0_b, const float* ln_g, const float* ln_b, const float* c4_w,
                      const float* c4_b, const int* labels, const float* class_weight, float ce_weight, float* logits,
                      float* fusion_w, float* attn_w, float* save, float* loss, int* ticket, int B, int N, int nhead,
                      int C, float ln_eps, float attn_p, uint32_t seed_attn, float gate_p, uint32_t seed_gate,
                      float cls_p, uint32_t seed_cls, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(hn && in_w && in_b && out_w && out_b && g0_w && g0_b && g3_w && g3_b && fusion_logits && temperature &&
               c0_w && c0_b && ln_g && ln_b && c4_w && c4_b && logits && fusion_w && attn_w && save, "bridge_cls_fwd: null");
    MM_REQUIRE(cls_shape_ok(B, N, nhead, C), "bridge_cls_fwd: B=%d bridge_dim=%d (multiple of 32 in [32, 256]) heads=%d (<= 16, dividing it) classes=%d (2..16)", B, N, nhead, C);
    MM_REQUIRE(!labels || (loss && ticket), "bridge_cls_fwd: labels need the loss outputs and the ticket word");
    for (float p : {drop_p, attn_p, gate_p, cls_p}) MM_REQUIRE(p >= 0.f && p < 1.f, "bridge_cls_fwd: drop_p");
    ClsFwdArgs a{};
    a.hn = hn;
    a.p = ClsParams{in_w, in_b, out_w, out_b, g0_w, g0_b, g3_w, g3_b, fusion_logits, temperature, c0_w, c0_b, ln_g, ln_b, c4_w, c4_b};
    a.labels = labels; a.cw = class_weight; a.ce_weight = ce_weight;
    a.logits = logits; a.fw = fusion_w; a.aw = attn_w; a.save = save; a.loss = loss; a.ticket = ticket;
    a.B = B; a.N = N; a.H = nhead; a.C = C; a.eps = ln_eps;
    a.dhead = cls_drop(drop_p, 0); a.seed_e = seed_e; a.seed_f = seed_f;
    a.datt = cls_drop(attn_p, seed_attn); a.dgate = cls_drop(gate_p, seed_gate); a.dcls = cls_drop(cls_p, seed_cls);
    a.epoch = seed_epoch;
    hipLaunchKernelGGL(bridge_cls_fwd_kernel, dim3(B), dim3(256), 0, st, a);
    return mm_check_launch("bridge_cls_fwd");
}
}  // extern "C"

namespace {
struct ClsBwdArgs {
    const float *save, *logits, *loss; const int* labels; float ce_weight;
    const float *in_w, *out_w, *g0_w, *g3_w, *fl, *temp, *c0_w, *ln_g, *ln_b, *c4_w;
    float *grad, *da; const float* loss_in; float* loss_total;
    int B, N, H, C; ClsDrop datt, dgate, dcls; const uint32_t* epoch;
};

// out[k] = sum_r gy[r] W[r][k] for k < K (gy in LDS; K % 4 == 0, K <= 512).  A thread owns four consecutive columns
// (float4 loads along a row of W, coalesced), the 256 / (K / 4) thread groups split the rows between them with eight
// loads in flight each; the groups' partial sums meet in LDS (`part`, 1024 floats) and are added in group order.
template <class Store>
__device__ __forceinline__ void dense_cols(const float* __restrict__ W, const float* gy, int R, int K, float* part,
                                           Store&& store) {
    constexpr int U = 8;
    const int kq = K >> 2, G = 256 / kq;                     // G * K <= 1024
    const int c = threadIdx.x % kq, grp = threadIdx.x / kq;
    const bool v4 = (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    if (grp < G) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int r0 = grp; r0 < R; r0 += U * G) {
            float4 w4[U];
            float gv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = r0 + u * G;
                w4[u] = ld4(W + (size_t)(r < R ? r : R - 1) * K + 4 * c, v4);
                gv[u] = r < R ? gy[r] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc.x += gv[u] * w4[u].x; acc.y += gv[u] * w4[u].y; acc.z += gv[u] * w4[u].z; acc.w += gv[u] * w4[u].w;
            }
        }
        float* dst = part + grp * K + 4 * c;
        dst[0] = acc.x; dst[1] = acc.y; dst[2] = acc.z; dst[3] = acc.w;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        float sum = 0.f;
        for (int g = 0; g < G; ++g) sum += part[g * K + k];
        store(k, sum);
    }
    __syncthreads();                                         // `part` is free again
}

// rows launch: a workgroup per sample backpropagates d (ce_weight * ce) from the logits to the two input tokens
__global__ __launch_bounds__(256) void bridge_cls_bwd_rows_kernel(ClsBwdArgs a) {
    __shared__ float dpe[3 * CLS_MAXN], dpf[3 * CLS_MAXN], datt[CLS_MAXN], daf[CLS_MAXN], dfused[CLS_MAXN], dg1[CLS_MAXN],
        dctx[CLS_MAXN], dc1[CLS_MAXN / 2], dlog[CLS_MAXC], red[4], ddyn[2], part[1024];
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, N2 = a.N / 2, H = a.H, C = a.C;
    const SaveL L(N);
    const GradL G(N);
    const float* sv = a.save + (size_t)b * L.stride;
    float* gr = a.grad + (size_t)b * G.stride;
    // 1. d logits = ce_weight * w_b / sum w * (softmax - onehot); a row of weight 0 (a label outside [0, C)) gets zeros
    if (tid < C) {
        const int y = a.labels[b];
        const float w = sv[L.sm + SM_W], sw = a.loss[2];
        const float coef = (w > 0.f && sw > 0.f) ? a.ce_weight * w / sw : 0.f;
        const float v = coef * (__expf(a.logits[(size_t)b * C + tid] - sv[L.sm + SM_LSE]) - (tid == y ? 1.f : 0.f));
        dlog[tid] = v; gr[G.dlog + tid] = v;
    }
    if (b == 0 && tid == 0 && a.loss_total) a.loss_total[0] = (a.loss_in ? a.loss_in[0] : 0.f) + a.ce_weight * a.loss[0];
    __syncthreads();
    // 2. classifier.4 -> dropout / ReLU -> LayerNorm backward
    {
        const bool on = tid < N2;
        float gd = 0.f, xh = 0.f, rstd = sv[L.sm + SM_RSTD];
        if (on) {
            float dh = 0.f;
            for (int c = 0; c < C; ++c) dh += dlog[c] * a.c4_w[(size_t)c * N2 + tid];
            const float mean = sv[L.sm + SM_MEAN], gam = a.ln_g[tid];
            xh = (sv[L.c1 + tid] - mean) * rstd;
            // ReLU' and the dropout mask are the forward's own: its saved h is > 0 exactly where it kept a positive value
            dh = sv[L.h + tid] > 0.f ? dh * a.dcls.inv_keep : 0.f;
            gr[G.dgam + tid] = dh * xh; gr[G.dbet + tid] = dh;
            gd = dh * gam;
        }
        const float m1 = cls_block_sum(gd, red) / N2, m2 = cls_block_sum(gd * xh, red) / N2;
        if (on) {
            const float v = rstd * (gd - m1 - xh * m2);
            dc1[tid] = v; gr[G.dc1 + tid] = v;
        }
    }
    __syncthreads();
    // 3. classifier.0 -> d fused
    dense_cols(a.c0_w, dc1, N2, N, part, [&](int k, float v) { dfused[k] = v; });
    __syncthreads();
    // 4. fusion backward (learned_fusion_bwd_kernel's expressions, M = 2)
    {
        const bool on = tid < N;
        const float df = on ? dfused[tid] : 0.f;
        const float dw0 = cls_block_sum(on ? df * sv[L.att + tid] : 0.f, red);
        const float dw1 = cls_block_sum(on ? df * sv[L.af + tid] : 0.f, red);
        const Fus2 f = fusion2(a.fl, a.temp, sv[L.sm + SM_DYN], sv[L.sm + SM_DYN + 1]);
        const float dw[2] = {dw0, dw1};
        const float dots = f.st[0] * dw0 + f.st[1] * dw1, dotd = f.dy[0] * dw0 + f.dy[1] * dw1;
        float dT = 0.f, gdy[2], gst[2];
        for (int m = 0; m < 2; ++m) {
            const float gs = 0.5f * f.st[m] * (dw[m] - dots), gd = 0.5f * f.dy[m] * (dw[m] - dotd);
            gst[m] = gs / f.T; gdy[m] = gd / f.T;
            dT -= (gs * f.us[m] + gd * f.ud[m]) / f.T;
        }
        if (tid == 0) {
            ddyn[0] = gdy[0]; ddyn[1] = gdy[1];
            gr[G.ddyn] = gdy[0]; gr[G.ddyn + 1] = gdy[1]; gr[G.dfl] = gst[0]; gr[G.dfl + 1] = gst[1]; gr[G.dT] = dT;
        }
        if (on) { datt[tid] = f.w[0] * df; daf[tid] = f.w[1] * df; }
    }
    __syncthreads();
    // 5. gate net backward
    if (tid < N) {
        float v = ddyn[0] * a.g3_w[tid] + ddyn[1] * a.g3_w[N + tid];
        if (a.dgate.thresh)
            v *= dropout_scale(mm_eff_seed(a.dgate.seed, a.epoch), (uint32_t)(b * N + tid), a.dgate.thresh, a.dgate.inv_keep);
        v *= gelu_erf_grad(sv[L.g1 + tid]);
        dg1[tid] = v; gr[G.dg1 + tid] = v;
    }
    __syncthreads();
    dense_cols(a.g0_w, dg1, N, 2 * N, part, [&](int k, float v) { if (k < N) datt[k] += v; else daf[k - N] += v; });
    __syncthreads();
    if (tid < N) gr[G.datt + tid] = datt[tid];
    // 6. out_proj -> d ctx, then the 1 x 2 attention (attn_1x2_fused_kernel's backward), sixteen lanes per head
    dense_cols(a.out_w, datt, N, N, part, [&](int k, float v) { dctx[k] = v; });
    __syncthreads();
    {
        const int h = tid >> 4, part = tid & 15, dh = N / H;
        const float* pe = sv + L.pe;
        const float* pf = sv + L.pf;
        float dp0 = 0.f, dp1 = 0.f;
        if (h < H)
            for (int d = part; d < dh; d += 16) {
                const int i = h * dh + d;
                dp0 += dctx[i] * pe[2 * N + i]; dp1 += dctx[i] * pf[2 * N + i];
            }
        dp0 = row16_sum(dp0); dp1 = row16_sum(dp1);
        if (h < H) {
            float k0 = 1.f, k1 = 1.f;
            if (a.datt.thresh) {
                const uint32_t seed = mm_eff_seed(a.datt.seed, a.epoch);
                k0 = dropout_scale(seed, (uint32_t)((b * H + h) * 2), a.datt.thresh, a.datt.inv_keep);
                k1 = dropout_scale(seed, (uint32_t)((b * H + h) * 2 + 1), a.datt.thresh, a.datt.inv_keep);
            }
            const float p0 = sv[L.sm + SM_P0 + h], p1 = sv[L.sm + SM_P1 + h], isq = rsqrtf((float)dh);
            dp0 *= k0; dp1 *= k1;
            const float dot = p0 * dp0 + p1 * dp1;
            const float ds0 = p0 * (dp0 - dot) * isq, ds1 = p1 * (dp1 - dot) * isq;
            for (int d = part; d < dh; d += 16) {
                const int i = h * dh + d;
                dpe[i] = ds0 * pe[N + i] + ds1 * pf[N + i];
                dpe[N + i] = ds0 * pe[i];
                dpe[2 * N + i] = p0 * k0 * dctx[i];
                dpf[i] = 0.f;
                dpf[N + i] = ds1 * pe[i];
                dpf[2 * N + i] = p1 * k1 * dctx[i];
            }
        }
    }
    __syncthreads();
    for (int r = tid; r < 3 * N; r += 256) { gr[G.dpe + r] = dpe[r]; gr[G.dpf + r] = dpf[r]; }
    // 7. in_proj -> the gradient of both tokens (the q rows see a_e only)
    dense_cols(a.in_w, dpe, 3 * N, N, part, [&](int k, float v) { a.da[((size_t)0 * a.B + b) * N + k] = v; });
    dense_cols(a.in_w + (size_t)N * N, dpf + N, 2 * N, N, part, [&](int k, float v) { a.da[((size_t)1 * a.B + b) * N + k] = daf[k] + v; });
}

// weights launch: every parameter gradient element is owned by one thread, which sums its rows' terms in row order
// and adds the sum to its bucket target.  grid = (chunks of 256 elements, job): the job is uniform over a workgroup
struct WJob {
    const float *gy, *x, *gy2, *x2;         // row b: gy[b * gs + r], x[b * xs + k] (and a second pair: in_proj's fMRI token)
    float *dW, *db;
    int R, K;                               // R * K weight elements, then R bias elements
};
constexpr int CLS_NJOBS = 10;
struct ClsWArgs { WJob j[CLS_NJOBS]; int B, gs, xs; };

__global__ __launch_bounds__(256) void bridge_cls_bwd_weights_kernel(ClsWArgs a) {
    const WJob J = a.j[blockIdx.y];
    const int B = a.B, nw = J.R * J.K;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nw + J.R) return;
    float acc = 0.f;
    if (e < nw) {
        if (!J.dW) return;
        const int r = e / J.K, k = e - r * J.K;
        const float* gy = J.gy + r;
        const float* x = J.x + k;
#pragma unroll 8
        for (int b = 0; b < B; ++b) acc += gy[(size_t)b * a.gs] * x[(size_t)b * a.xs];
        if (J.gy2) {
            const float* gy2 = J.gy2 + r;
            const float* x2 = J.x2 + k;
#pragma unroll 8
            for (int b = 0; b < B; ++b) acc += gy2[(size_t)b * a.gs] * x2[(size_t)b * a.xs];
        }
        J.dW[e] += acc;
    } else {
        if (!J.db) return;
        const int r = e - nw;
        for (int b = 0; b < B; ++b) acc += J.gy[(size_t)b * a.gs + r];
        if (J.gy2)
            for (int b = 0; b < B; ++b) acc += J.gy2[(size_t)b * a.gs + r];
        J.db[r] += acc;
    }
}
}  // namespace

extern "C" {
int mm_bridge_cls_bwd(const float* save, const float* logits, const float* loss, const int* labels, float ce_weight,
                      const float* in_w, const float* out_w, const float* g0_w, const float* g3_w,
                      const float* fusion_logits, const float* temperature, const float* c0_w, const float* ln_g,
                      const float* ln_b, const float* c4_w, float* grad_rows, float* da, float* d_in_w, float* d_in_b,
                      float* d_out_w, float* d_out_b, float* d_g0_w, float* d_g0_b, float* d_g3_w, float* d_g3_b,
                      float* d_fusion_logits, float* d_temperature, float* d_c0_w, float* d_c0_b, float* d_ln_g,
                      float* d_ln_b, float* d_c4_w, float* d_c4_b, const float* loss_in, float* loss_total, int phase, int B,
                      int N, int nhead, int C, float attn_p, uint32_t seed_attn, float gate_p, uint32_t seed_gate, float cls_p,
                      uint32_t seed_cls, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(save && logits && loss && labels && in_w && out_w && g0_w && g3_w && fusion_logits && temperature && c0_w &&
               ln_g && ln_b && c4_w && grad_rows && da, "bridge_cls_bwd: null");
    MM_REQUIRE(cls_shape_ok(B, N, nhead, C), "bridge_cls_bwd: B=%d bridge_dim=%d (multiple of 32 in [32, 256]) heads=%d (<= 16, dividing it) classes=%d (2..16)", B, N, nhead, C);
    for (float p : {attn_p, gate_p, cls_p}) MM_REQUIRE(p >= 0.f && p < 1.f, "bridge_cls_bwd: drop_p");
    MM_REQUIRE(phase == 0 || phase == 1, "bridge_cls_bwd: phase %d (0 = rows, 1 = weights)", phase);
    if (phase == 0) {
    ClsBwdArgs a{};
    a.save = save; a.logits = logits; a.loss = loss; a.labels = labels; a.ce_weight = ce_weight;
    a.in_w = in_w; a.out_w = out_w; a.g0_w = g0_w; a.g3_w = g3_w; a.fl = fusion_logits; a.temp = temperature;
    a.c0_w = c0_w; a.ln_g = ln_g; a.ln_b = ln_b; a.c4_w = c4_w;
    a.grad = grad_rows; a.da = da; a.loss_in = loss_in; a.loss_total = loss_total;
    a.B = B; a.N = N; a.H = nhead; a.C = C;
    a.datt = cls_drop(attn_p, seed_attn); a.dgate = cls_drop(gate_p, seed_gate); a.dcls = cls_drop(cls_p, seed_cls);
    a.epoch = seed_epoch;
    hipLaunchKernelGGL(bridge_cls_bwd_rows_kernel, dim3(B), dim3(256), 0, st, a);
    return mm_check_launch("bridge_cls_bwd (rows)");
    }
    const SaveL L(N);
    const GradL G(N);
    const int N2 = N / 2;
    ClsWArgs w{};
    w.B = B; w.gs = G.stride; w.xs = L.stride;
    const float* g = grad_rows;
    int most = 0, n = 0;
    auto job = [&](const float* gy, const float* x, float* dW, float* db, int R, int K, const float* gy2 = nullptr,
                   const float* x2 = nullptr) {
        most = R * K + R > most ? R * K + R : most;
        w.j[n++] = WJob{gy, x, gy2, x2, dW, db, R, K};
    };
    job(g + G.dpe, save + L.ae, d_in_w, d_in_b, 3 * N, N, g + G.dpf, save + L.af);
    job(g + G.datt, save + L.ctx, d_out_w, d_out_b, N, N);
    job(g + G.dg1, save + L.att, d_g0_w, d_g0_b, N, 2 * N);
    job(g + G.ddyn, save + L.g, d_g3_w, d_g3_b, 2, N);
    job(g + G.dc1, save + L.fused, d_c0_w, d_c0_b, N2, N);
    job(g + G.dlog, save + L.h, d_c4_w, d_c4_b, C, N2);
    job(g + G.dgam, nullptr, nullptr, d_ln_g, N2, 0);
    job(g + G.dbet, nullptr, nullptr, d_ln_b, N2, 0);
    job(g + G.dfl, nullptr, nullptr, d_fusion_logits, 2, 0);
    job(g + G.dT, nullptr, nullptr, d_temperature, 1, 0);
    hipLaunchKernelGGL(bridge_cls_bwd_weights_kernel, dim3(ceil_div(most, 256), CLS_NJOBS), dim3(256), 0, st, w);
    return mm_check_launch("bridge_cls_bwd (weights)");
}
}  // extern "C"
