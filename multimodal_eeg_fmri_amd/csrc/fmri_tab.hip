// Feature half of the tabular fMRI net (fMRI_CODE/fmri_utils.py:23-108: two Linear-BN-ReLU-Dropout x 2 encoders on the ROI
// activation statistics and the flattened PPI connectivity, softmax-weighted concat, Linear-BN-ReLU-Dropout fusion) in
// ONE forward and ONE backward launch.  fp32 inputs, outputs and gradients; what BatchNorm over a small batch amplifies
// - the Linear's sums, the batch statistics and the BatchNorm backward's sums - is accumulated in fp64 (tab_slice,
// tab_bn_bwd).  No floating-point atomics, every sum in a fixed order.
// Callers: ops._tab_forward_impl, autograd.fmri_tab_bwd.
//
// Input x [B][A + C] = [activation | connectivity].  Five layers, in this order everywhere (arguments, seeds, save):
//   0 a1: A -> 2H    1 a2: 2H -> H    2 c1: C -> 2H    3 c2: 2H -> H    4 f: [wa * a2 | wc * c2] (2H) -> H
// with (wa, wc) = softmax(activation_weight, connectivity_weight).  Weights in PyTorch layout [out][in].
//
// Dropout: one site after each BN-ReLU, five seeds of their own in the layer order above, the same hash as everywhere
// (common.h); the element index is the flat row-major index b * width + f of the layer's (B, width) output.
//
// Forward decomposition.  BatchNorm statistics are per feature over the batch, so a workgroup that owns eight output
// features of a layer for ALL rows needs nobody else inside that layer: grid = 2 branches x (2H / 8) slices of the wide
// first layers.  No workgroup ever waits for another: the slices of a branch take a ticket (int32 word, agent-scope
// add behind an agent-scope release); the one that arrives last runs the branch's second layer, takes a second ticket
// with the other branch, and the last of those two runs the fusion layer.  Each last arriver leaves its word at zero.
//
// Backward decomposition: no ticket.  Everything from d fused down to d pre1 involves only B x (H | 2H) tensors; every
// workgroup recomputes the part its branch needs, in a fixed order, in a scratch area of its own (4 B H floats).  Then a
// workgroup owns 64 columns k of one branch's first layer - dW1[:, k], dx[:, k] - and three more workgroups own the small
// matrices: one per branch (second layer, both BatchNorms, first-layer bias) and one for the fusion layer and the two
// fusion scalars.  Every product goes through tab_gemm (64 x 64 output tiles, operand tiles staged in LDS, k ascending).
// Every gradient element has ONE writer and is a plain store.
#include "common.h"

namespace {
constexpr int TAB_FS = 8;          // output features a first-layer slice (one workgroup) owns
constexpr int TAB_FMAX = 64;       // most features a last arriver's slice holds: rows x features <= TAB_PAIRS
constexpr int TAB_PAIRS = 2048;    // (row, feature) pairs of a slice: eight per thread
constexpr int TAB_KT = 32;         // reduction tile staged in LDS
constexpr int TAB_RB = 256;        // rows per pass (train mode: the whole batch)
constexpr int TAB_KS = 64;         // first-layer input columns a backward workgroup owns

// layout of the forward's save buffer (floats): pre-activations (the Linear's output) `x*` and post-dropout outputs `h*`
// per layer (the fusion layer's output is the launch's `out`), then the five layers' means and inverse standard
// deviations as the forward used them (batch statistics in train mode, running statistics when frozen)
struct TabL {
    size_t xa1, ha1, xa2, ha2, xc1, hc1, xc2, hc2, xf, mean, rstd;       // (13 B H + 14 H floats in all)
    int H;
    __host__ __device__ TabL(int B, int h) : H(h) {
        const size_t n = (size_t)B * h;
        xa1 = 0; ha1 = 2 * n; xa2 = 4 * n; ha2 = 5 * n; xc1 = 6 * n; hc1 = 8 * n; xc2 = 10 * n; hc2 = 11 * n; xf = 12 * n;
        mean = 13 * n; rstd = mean + 7 * (size_t)h;
    }
    __host__ __device__ size_t pre(int l) const { const size_t o[5] = {xa1, xa2, xc1, xc2, xf}; return o[l]; }
    __host__ __device__ size_t hout(int l) const { const size_t o[5] = {ha1, ha2, hc1, hc2, 0}; return o[l]; }   // (l < 4)
    __host__ __device__ size_t st(int l) const { const int o[5] = {0, 2, 3, 5, 6}; return (size_t)o[l] * H; }
    __host__ __device__ size_t mu(int l) const { return mean + st(l); }
    __host__ __device__ size_t rs(int l) const { return rstd + st(l); }
};

struct TabLayer { const float *w, *b, *g, *be; float *rm, *rv; long long* nbt; };
struct TabFwdArgs {
    const float* x; TabLayer lay[5]; const float *aw, *cw;
    float *out, *save; int* tickets;
    int B, A, C, H, train; float eps, momentum;
    uint32_t thresh; float inv_keep; uint32_t seed[5]; const uint32_t* epoch;
};

struct TabSmem {
    float x[TAB_RB][TAB_KT + 1];           // (+1: a wave's rows fall on different banks)
    float w[TAB_FMAX][TAB_KT + 1];
    double pre[TAB_PAIRS];                 // [feature][row]: fp64 until xhat has been formed
    double part[128];                      // [feature][lane]: 128 / features lanes per feature
    double mean[TAB_FMAX], rstd[TAB_FMAX];
};

// features per slice for a last arriver (second layers, fusion layer): as many as eight pairs per thread allow, so that
// a small batch re-reads its input once, not once per eight features
__device__ __forceinline__ int tab_slice_width(int B, int width) {
    const int nb = B < TAB_RB ? B : TAB_RB;
    int n = TAB_FS;
    while (2 * n <= TAB_FMAX && 2 * n <= width && 2 * n * nb <= TAB_PAIRS) n *= 2;
    return n;
}

__device__ __forceinline__ float ld_agent(const float* p) {          // bytes another workgroup of this launch stored
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// softmax of the two fusion scalars
__device__ __forceinline__ void tab_fusion_w(const float* aw, const float* cw, float& wa, float& wc) {
    const float a = aw[0], c = cw[0], m = fmaxf(a, c);
    const float ea = __expf(a - m), ec = __expf(c - m);
    wa = ea / (ea + ec); wc = ec / (ea + ec);
}

// One slice of a layer: features [f0, f0 + nfs) of Linear(K -> width) + BatchNorm + ReLU + Dropout for all B rows
// (nfs a power of two in [8, 64], rows x nfs <= 2048).
// ld(b, k) = the layer's input.  Train mode (B <= 256): batch statistics, running statistics updated by this, the only
// workgroup that owns the features.  Frozen: running statistics, any B (256 rows per pass).  A thread owns up to eight
// (row, feature) pairs p = tid + 256 j -> (b = p % rows, f = p / rows); its sum over k runs in ascending k, the exact
// fp32 products added in fp64: with a handful of rows a feature's batch deviation can be a hundredth of its values, and
// 1 / deviation multiplies whatever rounding the pre-activation carries into xhat and every gradient behind it.
template <class Load>
__device__ __forceinline__ void tab_slice(TabSmem& s, Load&& ld, int B, int K, const TabLayer& L, int width, int f0,
                                          int nfs, const TabFwdArgs& a, uint32_t seed, float* pre, float* h, float* mean_out,
                                          float* rstd_out) {
    const int tid = threadIdx.x;
    for (int b0 = 0; b0 < B; b0 += TAB_RB) {
        const int nb = B - b0 < TAB_RB ? B - b0 : TAB_RB, np = nb * nfs;
        double acc[TAB_FS];
        int pb[TAB_FS], pf[TAB_FS];
#pragma unroll
        for (int j = 0; j < TAB_FS; ++j) {
            const int p = tid + 256 * j;
            acc[j] = 0.0;
            pf[j] = p < np ? p / nb : 0;
            pb[j] = p < np ? p - pf[j] * nb : 0;
        }
        for (int k0 = 0; k0 < K; k0 += TAB_KT) {
            const int kt = K - k0 < TAB_KT ? K - k0 : TAB_KT;
            for (int i = tid; i < nb * TAB_KT; i += 256) {
                const int r = i / TAB_KT, kk = i % TAB_KT;
                s.x[r][kk] = kk < kt ? ld(b0 + r, k0 + kk) : 0.f;
            }
            for (int i = tid; i < nfs * TAB_KT; i += 256) {
                const int f = i / TAB_KT, kk = i % TAB_KT;
                s.w[f][kk] = kk < kt ? L.w[(size_t)(f0 + f) * K + k0 + kk] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TAB_FS; ++j) {
                if (tid + 256 * j < np) {
                    double v = acc[j];
#pragma unroll
                    for (int kk = 0; kk < TAB_KT; ++kk) v += (double)s.x[pb[j]][kk] * (double)s.w[pf[j]][kk];
                    acc[j] = v;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < TAB_FS; ++j)
            if (tid + 256 * j < np) s.pre[pf[j] * nb + pb[j]] = acc[j] + (double)L.b[f0 + pf[j]];
        __syncthreads();
        {                                                          // 128 / nfs lanes per feature: rows lane, lane + lanes, ...
            const int lp = 128 / nfs;
            const bool on = tid < 128;
            const int f = on ? tid / lp : 0, lane = tid % lp;
            const double* pr = s.pre + f * nb;
            if (a.train) {                                         // (uniform: the barriers below are met by every thread)
                if (on) {
                    double sm = 0.0;
                    for (int b = lane; b < nb; b += lp) sm += pr[b];
                    s.part[tid] = sm;
                }
                __syncthreads();
                double mean = 0.0;
                if (on) {
                    for (int l = 0; l < lp; ++l) mean += s.part[f * lp + l];
                    mean /= nb;
                }
                __syncthreads();
                if (on) {
                    double sq = 0.0;
                    for (int b = lane; b < nb; b += lp) { const double d = pr[b] - mean; sq += d * d; }
                    s.part[tid] = sq;
                }
                __syncthreads();
                if (on && lane == 0) {
                    double var = 0.0;
                    for (int l = 0; l < lp; ++l) var += s.part[f * lp + l];
                    var /= nb;
                    const double rstd = 1.0 / sqrt(var + (double)a.eps);
                    s.mean[f] = mean; s.rstd[f] = rstd;
                    mean_out[f0 + f] = (float)mean; rstd_out[f0 + f] = (float)rstd;
                    L.rm[f0 + f] = (1.f - a.momentum) * L.rm[f0 + f] + a.momentum * (float)mean;
                    L.rv[f0 + f] = (1.f - a.momentum) * L.rv[f0 + f] + a.momentum * (float)(var * nb / (nb - 1));
                    if (f0 + f == 0 && L.nbt) L.nbt[0] += 1;
                }
            } else if (on && lane == 0) {
                const float rstd = rsqrtf(L.rv[f0 + f] + a.eps);
                s.mean[f] = L.rm[f0 + f]; s.rstd[f] = rstd;
                if (b0 == 0) { mean_out[f0 + f] = L.rm[f0 + f]; rstd_out[f0 + f] = rstd; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TAB_FS; ++j) {
            if (tid + 256 * j < np) {
                const int f = pf[j], b = b0 + pb[j];
                const double z = s.pre[f * nb + pb[j]];
                const float xh = (float)((z - s.mean[f]) * s.rstd[f]);
                float v = fmaxf(fmaf(xh, L.g[f0 + f], L.be[f0 + f]), 0.f);
                const size_t e = (size_t)b * width + f0 + f;
                if (a.thresh) v *= dropout_scale(seed, (uint32_t)e, a.thresh, a.inv_keep);
                pre[e] = (float)z; h[e] = v;
            }
        }
        __syncthreads();                                           // `s` is free again
    }
}

// Ticket of `n` workgroups on `word`: true in the workgroup that arrives last (which resets the word).  Every wave
// drains its stores, one lane releases them at agent scope and adds; the last arriver acquires at agent scope before
// any thread of its workgroup goes on to read what the others stored.
__device__ __forceinline__ bool tab_arrive_last(int* word, int n, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int last = __hip_atomic_fetch_add(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n - 1;
        if (last) {
            __hip_atomic_store(word, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next launch / replay
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

__global__ __launch_bounds__(256) void fmri_tab_fwd_kernel(TabFwdArgs a) {
    __shared__ TabSmem s;
    __shared__ int flag;
    const int H = a.H, W1 = 2 * H, nsl = W1 / TAB_FS, B = a.B;
    const int br = blockIdx.x / nsl, sl = blockIdx.x % nsl, nfs = tab_slice_width(B, H);
    const TabL L(B, H);
    // 1. this workgroup's slice of its branch's first layer
    {
        const int K = br ? a.C : a.A, xoff = br ? a.A : 0, Kt = a.A + a.C, l = 2 * br;
        const float* x = a.x;
        tab_slice(s, [=](int b, int k) { return x[(size_t)b * Kt + xoff + k]; }, B, K, a.lay[l], W1, sl * TAB_FS, TAB_FS, a,
                  mm_eff_seed(a.seed[l], a.epoch), a.save + L.pre(l), a.save + L.hout(l), a.save + L.mu(l), a.save + L.rs(l));
    }
    if (!tab_arrive_last(a.tickets + br, nsl, &flag)) return;
    // 2. the branch's last arriver: its second layer
    {
        const int l = 2 * br + 1;
        const float* h1 = a.save + L.hout(l - 1);
        for (int f0 = 0; f0 < H; f0 += nfs)
            tab_slice(s, [=](int b, int k) { return ld_agent(h1 + (size_t)b * W1 + k); }, B, W1, a.lay[l], H, f0, nfs, a,
                      mm_eff_seed(a.seed[l], a.epoch), a.save + L.pre(l), a.save + L.hout(l), a.save + L.mu(l), a.save + L.rs(l));
    }
    if (!tab_arrive_last(a.tickets + 2, 2, &flag)) return;
    // 3. the last of the two: softmax-weighted concat and the fusion layer
    {
        float wa, wc;
        tab_fusion_w(a.aw, a.cw, wa, wc);
        const float* ha = a.save + L.ha2;
        const float* hc = a.save + L.hc2;
        for (int f0 = 0; f0 < H; f0 += nfs)
            tab_slice(s, [=](int b, int k) { return k < H ? wa * ld_agent(ha + (size_t)b * H + k) : wc * ld_agent(hc + (size_t)b * H + k - H); },
                      B, W1, a.lay[4], H, f0, nfs, a, mm_eff_seed(a.seed[4], a.epoch), a.save + L.pre(4), a.out, a.save + L.mu(4),
                      a.save + L.rs(4));
    }
}

// ------------------------------------------------------------------------------------------------------- backward
struct TabBwdArgs {
    const float *dout, *x, *out, *save;
    const float *w[5], *g[5], *aw, *cw;        // weights and BatchNorm gammas, layer order
    float *scratch, *dx;
    float *dw[5], *db[5], *dg[5], *dbe[5], *daw, *dcw;
    int B, A, C, H, train; float inv_keep, eps;
};

// C(m, n) = sum_k A(m, k) B(k, n) for m < M, n < N through 64 x 64 output tiles: (64 x 64) tiles of both operands staged in
// LDS, a thread owns a 4 x 4 block and adds its products in ascending k (fp32).  la(m, k) / lb(k, n) read the operands,
// st(m, n, value) takes a result; AK: consecutive k of A are consecutive in memory (else consecutive m are).
constexpr int TAB_GT = 64, TAB_GK = 64;
struct __attribute__((aligned(16))) TabGemmSmem { float a[TAB_GK][TAB_GT + 4], b[TAB_GK][TAB_GT + 4]; };
template <bool AK, class LA, class LB, class ST>
__device__ __forceinline__ void tab_gemm(TabGemmSmem& s, int M, int N, int K, LA&& la, LB&& lb, ST&& st) {
    const int tid = threadIdx.x, tm = (tid >> 4) * 4, tn = (tid & 15) * 4;
    for (int m0 = 0; m0 < M; m0 += TAB_GT)
        for (int n0 = 0; n0 < N; n0 += TAB_GT) {
            float acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
            for (int k0 = 0; k0 < K; k0 += TAB_GK) {
                __syncthreads();                                   // the tiles of the step before have been read
                for (int i = tid; i < TAB_GK * TAB_GT; i += 256) {
                    const int kk = AK ? i % TAB_GK : i / TAB_GT, m = AK ? i / TAB_GK : i % TAB_GT;
                    s.a[kk][m] = (m0 + m < M && k0 + kk < K) ? la(m0 + m, k0 + kk) : 0.f;
                    const int kb = i / TAB_GT, n = i % TAB_GT;
                    s.b[kb][n] = (n0 + n < N && k0 + kb < K) ? lb(k0 + kb, n0 + n) : 0.f;
                }
                __syncthreads();
#pragma unroll 8
                for (int kk = 0; kk < TAB_GK; ++kk) {
                    const float4 av = *reinterpret_cast<const float4*>(&s.a[kk][tm]);
                    const float4 bv = *reinterpret_cast<const float4*>(&s.b[kk][tn]);
                    const float ar[4] = {av.x, av.y, av.z, av.w}, bc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(ar[u], bc[v], acc[u][v]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (m0 + tm + u < M && n0 + tn + v < N) st(m0 + tm + u, n0 + tn + v, acc[u][v]);
        }
    __syncthreads();
}

// BatchNorm backward over the columns of g (B, W), in place: in = the gradient at the BatchNorm's output, out = at the
// Linear's output.  W <= 256: 256 / W threads share a feature (rows grp, grp + groups, ...), their partial sums meet in
// LDS and are added in group order.  Train: the batch statistics are formed again from the saved pre-activations and
// everything up to the final rounding runs in fp64 - the result is a difference of nearly equal terms wherever BatchNorm
// passes little gradient (two rows; one input column), and fp32 statistics leave only three digits of it.  Frozen: a
// scale by the saved (running) statistics.  dgamma / dbeta / dbias (nullable): this workgroup owns them.
__device__ __forceinline__ void tab_bn_bwd(double* red /* [4][256] */, float* g, const float* pre, const float* mean,
                                           const float* rstd, const float* gamma, int B, int W, bool train, float eps,
                                           float* dgamma, float* dbeta, float* dbias) {
    const int tid = threadIdx.x, G = 256 / W, j = tid % W, grp = tid / W;
    __syncthreads();
    double t[4] = {0.0, 0.0, 0.0, 0.0};                            // sums of pre, pre^2, g, g * pre
#pragma unroll 4
    for (int b = grp; b < B; b += G) {
        const double p = pre[(size_t)b * W + j], v = g[(size_t)b * W + j];
        t[0] += p; t[1] += p * p; t[2] += v; t[3] += v * p;
    }
    for (int q = 0; q < 4; ++q) red[q * 256 + tid] = t[q];
    __syncthreads();
    for (int q = 0; q < 4; ++q) {
        double sum = 0.0;
        for (int gg = 0; gg < G; ++gg) sum += red[q * 256 + gg * W + j];
        t[q] = sum;
    }
    double mu = mean[j], rs = rstd[j];
    if (train) {
        mu = t[0] / B;
        const double var = t[1] / B - mu * mu;
        rs = 1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)eps);
    }
    const double s1 = t[2], s2 = rs * (t[3] - mu * t[2]);          // sum g, sum g * xhat
    if (grp == 0) {
        if (dgamma) dgamma[j] = (float)s2;
        if (dbeta) dbeta[j] = (float)s1;
    }
    const double sc = rs * (double)gamma[j], m1 = train ? s1 / B : 0.0, m2 = train ? s2 / B : 0.0;
    double sb = 0.0;
    __syncthreads();                                               // every thread has read `red`
#pragma unroll 4
    for (int b = grp; b < B; b += G) {
        const size_t e = (size_t)b * W + j;
        const double v = sc * ((double)g[e] - m1 - (((double)pre[e] - mu) * rs) * m2);
        g[e] = (float)v; sb += v;
    }
    red[tid] = sb;
    __syncthreads();
    if (grp == 0 && dbias) {
        double sum = 0.0;
        for (int gg = 0; gg < G; ++gg) sum += red[gg * W + j];
        dbias[j] = (float)sum;
    }
    __syncthreads();
}

__device__ __forceinline__ float tab_block_sum(float v, float* red /* [4] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void fmri_tab_bwd_kernel(TabBwdArgs a) {
    __shared__ TabGemmSmem gs;
    __shared__ double red64[4 * 256];
    __shared__ float red[4];
    const int B = a.B, H = a.H, W1 = 2 * H, Kt = a.A + a.C, tid = threadIdx.x;
    const int nsa = (a.A + TAB_KS - 1) / TAB_KS, nsc = (a.C + TAB_KS - 1) / TAB_KS;
    const TabL L(B, H);
    // role: a 64-column slice of a branch's first layer, or one of the three small-matrix owners
    int bid = blockIdx.x, br, slice = -1;
    bool small = false, fus = false;
    if (bid < nsa) { br = 0; slice = bid; }
    else if (bid < nsa + nsc) { br = 1; slice = bid - nsa; }
    else { br = bid - nsa - nsc; small = true; if (br == 2) { fus = true; br = 0; } }
    float* S1 = a.scratch + (size_t)blockIdx.x * 4 * B * H;        // d pre of the fusion layer (B, H)
    float* S2 = S1 + (size_t)B * H;                                // of the branch's second layer (B, H)
    float* S3 = S2 + (size_t)B * H;                                // of its first layer (B, 2H)
    const float* sv = a.save;
    float wa, wc;
    tab_fusion_w(a.aw, a.cw, wa, wc);
    // 1. fusion layer: ReLU' and the dropout mask are the forward's own (its output is > 0 exactly where it kept a
    //    positive value), then BatchNorm
    for (int e = tid; e < B * H; e += 256) S1[e] = a.out[e] > 0.f ? a.dout[e] * a.inv_keep : 0.f;
    tab_bn_bwd(red64, S1, sv + L.pre(4), sv + L.mu(4), sv + L.rs(4), a.g[4], B, H, a.train, a.eps, fus ? a.dg[4] : nullptr,
               fus ? a.dbe[4] : nullptr, fus ? a.db[4] : nullptr);
    if (fus) {
        // d W_f = d pre^T [wa * a2 | wc * c2]; the two scalars' gradients are sums over the same products
        const float* ha = sv + L.ha2;
        const float* hc = sv + L.hc2;
        const float* wf = a.w[4];
        float* dwf = a.dw[4];
        float pa = 0.f, pc = 0.f;
        tab_gemm<false>(gs, H, W1, B, [=](int i, int b) { return S1[(size_t)b * H + i]; },
                        [=](int b, int j) { return j < H ? ha[(size_t)b * H + j] : hc[(size_t)b * H + j - H]; },
                        [&](int i, int j, float m) {
                            const float w = wf[(size_t)i * W1 + j];
                            if (j < H) pa = fmaf(w, m, pa); else pc = fmaf(w, m, pc);
                            if (dwf) dwf[(size_t)i * W1 + j] = (j < H ? wa : wc) * m;
                        });
        const float dwa = tab_block_sum(pa, red), dwc = tab_block_sum(pc, red);
        const float dot = wa * dwa + wc * dwc;
        if (tid == 0) {
            if (a.daw) a.daw[0] = wa * (dwa - dot);
            if (a.dcw) a.dcw[0] = wc * (dwc - dot);
        }
        return;
    }
    // 2. the branch's half of d comb, scaled by its fusion weight, through ReLU / dropout and the second BatchNorm
    const int l1 = 2 * br, l2 = 2 * br + 1;
    {
        const float* h2 = sv + L.hout(l2);
        const float* wf = a.w[4] + (size_t)br * H;
        const float wbr = br ? wc : wa, ik = a.inv_keep;
        tab_gemm<true>(gs, B, H, H, [=](int b, int f) { return S1[(size_t)b * H + f]; },
                       [=](int f, int j) { return wf[(size_t)f * W1 + j]; }, [=](int b, int j, float v) {
                           const size_t e = (size_t)b * H + j;
                           S2[e] = h2[e] > 0.f ? wbr * v * ik : 0.f;
                       });
        tab_bn_bwd(red64, S2, sv + L.pre(l2), sv + L.mu(l2), sv + L.rs(l2), a.g[l2], B, H, a.train, a.eps,
                   small ? a.dg[l2] : nullptr, small ? a.dbe[l2] : nullptr, small ? a.db[l2] : nullptr);
    }
    // 3. through the second Linear, ReLU / dropout and the first BatchNorm
    {
        const float* h1 = sv + L.hout(l1);
        const float* w2 = a.w[l2];
        const float ik = a.inv_keep;
        tab_gemm<true>(gs, B, W1, H, [=](int b, int j) { return S2[(size_t)b * H + j]; },
                       [=](int j, int i) { return w2[(size_t)j * W1 + i]; }, [=](int b, int i, float v) {
                           const size_t e = (size_t)b * W1 + i;
                           S3[e] = h1[e] > 0.f ? v * ik : 0.f;
                       });
        tab_bn_bwd(red64, S3, sv + L.pre(l1), sv + L.mu(l1), sv + L.rs(l1), a.g[l1], B, W1, a.train, a.eps,
                   small ? a.dg[l1] : nullptr, small ? a.dbe[l1] : nullptr, small ? a.db[l1] : nullptr);
    }
    if (small) {                                                   // d W2 = d pre2^T h1
        const float* h1 = sv + L.hout(l1);
        float* dw2 = a.dw[l2];
        if (dw2)
            tab_gemm<false>(gs, H, W1, B, [=](int j, int b) { return S2[(size_t)b * H + j]; },
                            [=](int b, int i) { return h1[(size_t)b * W1 + i]; },
                            [=](int j, int i, float m) { dw2[(size_t)j * W1 + i] = m; });
        return;
    }
    // 4. this workgroup's columns of the first layer: d W1[:, k] and d x[:, k]
    {
        const int K = br ? a.C : a.A, xoff = br ? a.A : 0, k0 = slice * TAB_KS;
        const int nk = K - k0 < TAB_KS ? K - k0 : TAB_KS;
        const float* x = a.x + xoff + k0;
        const float* w1 = a.w[l1] + k0;
        float* dw1 = a.dw[l1];
        if (dw1)
            tab_gemm<false>(gs, W1, nk, B, [=](int i, int b) { return S3[(size_t)b * W1 + i]; },
                            [=](int b, int k) { return x[(size_t)b * Kt + k]; },
                            [=](int i, int k, float m) { dw1[(size_t)i * K + k0 + k] = m; });
        if (a.dx) {
            float* dx = a.dx + xoff + k0;
            tab_gemm<true>(gs, B, nk, W1, [=](int b, int i) { return S3[(size_t)b * W1 + i]; },
                           [=](int i, int k) { return w1[(size_t)i * K + k]; },
                           [=](int b, int k, float v) { dx[(size_t)b * Kt + k] = v; });
        }
    }
}

static bool tab_shape_ok(int B, int A, int C, int H, int train) {
    return B >= 1 && A >= 1 && C >= 1 && (H == 32 || H == 64 || H == 128) && (!train || (B >= 2 && B <= TAB_RB));
}
}  // namespace

extern "C" {
int mm_fmri_tab_fwd(const float* x, int B, int A, int C, int H,
                    const float* a1_w, const float* a1_b, const float* a1_g, const float* a1_be, float* a1_rm, float* a1_rv, int64_t* a1_nbt,
                    const float* a2_w, const float* a2_b, const float* a2_g, const float* a2_be, float* a2_rm, float* a2_rv, int64_t* a2_nbt,
                    const float* c1_w, const float* c1_b, const float* c1_g, const float* c1_be, float* c1_rm, float* c1_rv, int64_t* c1_nbt,
                    const float* c2_w, const float* c2_b, const float* c2_g, const float* c2_be, float* c2_rm, float* c2_rv, int64_t* c2_nbt,
                    const float* f_w, const float* f_b, const float* f_g, const float* f_be, float* f_rm, float* f_rv, int64_t* f_nbt,
                    const float* activation_weight, const float* connectivity_weight, float* out, float* save, int* tickets,
                    int train, float eps, float momentum, float drop_p, uint32_t seed_a1, uint32_t seed_a2, uint32_t seed_c1,
                    uint32_t seed_c2, uint32_t seed_f, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(tab_shape_ok(B, A, C, H, train), "fmri_tab_fwd: B=%d (train: 2..256) activation_dim=%d connectivity_dim=%d (>= 1) hidden_dim=%d (32, 64 or 128)", B, A, C, H);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f && (train || drop_p == 0.f), "fmri_tab_fwd: drop_p (0 with frozen BatchNorm)");
    TabFwdArgs a{};
    a.x = x;
    a.lay[0] = TabLayer{a1_w, a1_b, a1_g, a1_be, a1_rm, a1_rv, (long long*)a1_nbt};
    a.lay[1] = TabLayer{a2_w, a2_b, a2_g, a2_be, a2_rm, a2_rv, (long long*)a2_nbt};
    a.lay[2] = TabLayer{c1_w, c1_b, c1_g, c1_be, c1_rm, c1_rv, (long long*)c1_nbt};
    a.lay[3] = TabLayer{c2_w, c2_b, c2_g, c2_be, c2_rm, c2_rv, (long long*)c2_nbt};
    a.lay[4] = TabLayer{f_w, f_b, f_g, f_be, f_rm, f_rv, (long long*)f_nbt};
    for (const TabLayer& l : a.lay) MM_REQUIRE(l.w && l.b && l.g && l.be && l.rm && l.rv, "fmri_tab_fwd: null layer argument");
    MM_REQUIRE(x && activation_weight && connectivity_weight && out && save && tickets, "fmri_tab_fwd: null");
    a.aw = activation_weight; a.cw = connectivity_weight; a.out = out; a.save = save; a.tickets = tickets;
    a.B = B; a.A = A; a.C = C; a.H = H; a.train = train; a.eps = eps; a.momentum = momentum;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.inv_keep = d.inv_keep;
    a.seed[0] = seed_a1; a.seed[1] = seed_a2; a.seed[2] = seed_c1; a.seed[3] = seed_c2; a.seed[4] = seed_f;
    a.epoch = seed_epoch;
    hipLaunchKernelGGL(fmri_tab_fwd_kernel, dim3(2 * (2 * H / TAB_FS)), dim3(256), 0, st, a);
    return mm_check_launch("fmri_tab_fwd");
}

int mm_fmri_tab_bwd(const float* dout, const float* x, const float* out, const float* save, int B, int A, int C, int H,
                    const float* a1_w, const float* a1_g, const float* a2_w, const float* a2_g, const float* c1_w,
                    const float* c1_g, const float* c2_w, const float* c2_g, const float* f_w, const float* f_g,
                    const float* activation_weight, const float* connectivity_weight, float* scratch, float* dx,
                    float* d_a1_w, float* d_a1_b, float* d_a1_g, float* d_a1_be, float* d_a2_w, float* d_a2_b, float* d_a2_g,
                    float* d_a2_be, float* d_c1_w, float* d_c1_b, float* d_c1_g, float* d_c1_be, float* d_c2_w, float* d_c2_b,
                    float* d_c2_g, float* d_c2_be, float* d_f_w, float* d_f_b, float* d_f_g, float* d_f_be,
                    float* d_activation_weight, float* d_connectivity_weight, int train, float eps, float drop_p, hipStream_t st) {
    MM_REQUIRE(tab_shape_ok(B, A, C, H, train), "fmri_tab_bwd: B=%d (train: 2..256) activation_dim=%d connectivity_dim=%d (>= 1) hidden_dim=%d (32, 64 or 128)", B, A, C, H);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f && (train || drop_p == 0.f), "fmri_tab_bwd: drop_p (0 with frozen BatchNorm)");
    MM_REQUIRE(dout && x && out && save && a1_w && a1_g && a2_w && a2_g && c1_w && c1_g && c2_w && c2_g && f_w && f_g &&
               activation_weight && connectivity_weight && scratch, "fmri_tab_bwd: null");
    TabBwdArgs a{};
    a.dout = dout; a.x = x; a.out = out; a.save = save;
    const float* w[5] = {a1_w, a2_w, c1_w, c2_w, f_w};
    const float* g[5] = {a1_g, a2_g, c1_g, c2_g, f_g};
    float* dw[5] = {d_a1_w, d_a2_w, d_c1_w, d_c2_w, d_f_w};
    float* db[5] = {d_a1_b, d_a2_b, d_c1_b, d_c2_b, d_f_b};
    float* dg[5] = {d_a1_g, d_a2_g, d_c1_g, d_c2_g, d_f_g};
    float* dbe[5] = {d_a1_be, d_a2_be, d_c1_be, d_c2_be, d_f_be};
    for (int l = 0; l < 5; ++l) { a.w[l] = w[l]; a.g[l] = g[l]; a.dw[l] = dw[l]; a.db[l] = db[l]; a.dg[l] = dg[l]; a.dbe[l] = dbe[l]; }
    a.aw = activation_weight; a.cw = connectivity_weight; a.scratch = scratch; a.dx = dx;
    a.daw = d_activation_weight; a.dcw = d_connectivity_weight;
    a.B = B; a.A = A; a.C = C; a.H = H; a.train = train; a.inv_keep = mm_drop(drop_p).inv_keep; a.eps = eps;
    hipLaunchKernelGGL(fmri_tab_bwd_kernel, dim3(ceil_div(A, TAB_KS) + ceil_div(C, TAB_KS) + 3), dim3(256), 0, st, a);
    return mm_check_launch("fmri_tab_bwd");
}
}  // extern "C"
