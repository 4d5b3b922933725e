// Small fp32 row kernels at the ends of the encoders and the tabular models: the dense layer (fwd/bwd), elementwise
// activation, BatchNorm1d column statistics, both projection heads of the contrastive bridge in one launch each way, the
// pooled output head of the EEG encoders, and the loose drop_path / mean-pool / add / mul helpers.  Batches here are tens
// of rows: these kernels are latency-bound, kept in fp32 end-to-end (they sit right before the parity-checked outputs)
// and use wave-level shuffles for every row reduction.  Callers: ops.py (small_linear, act_f32, proj_heads_fwd,
// pooled_head_fwd, meanpool_bf16), small_autograd.py (the tabular tape), autograd.py (proj_heads_bwd, pooled_head_bwd*).
// The losses, the optimizer, the fusion kernels and the power front end are next door: clip_loss.hip, losses.hip,
// optim.hip, fusion.hip, power_front.hip.
#include "common.h"

namespace {
// y[b][n] = dropout(act(x[b][:] . W[n][:] + bias[n])); one wave per (b, 64 outputs)
__global__ void small_linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                        const float* __restrict__ bias, const float* __restrict__ scale,
                                        const float* __restrict__ shift, float* __restrict__ y,
                                        float* __restrict__ pre, int B, int K, int N, int act,
                                        uint32_t thresh, uint32_t seed, float inv_keep, const uint32_t* epoch) {
    seed = mm_eff_seed(seed, epoch);
    extern __shared__ float xs[];                   // one input row
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += blockDim.x) xs[k] = x[(size_t)b * K + k];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int n = blockIdx.y * nw + wave; n < N; n += gridDim.y * nw) {
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += xs[k] * W[(size_t)n * K + k];
        s = wave_sum(s);
        if (lane == 0) {
            s += bias ? bias[n] : 0.f;
            if (scale) s = s * scale[n] + shift[n];
            const size_t idx = (size_t)b * N + n;
            if (pre) pre[idx] = s;
            s = apply_act(s, act);
            if (thresh) s *= dropout_scale(seed, (uint32_t)idx, thresh, inv_keep);
            y[idx] = s;
        }
    }
}
}  // namespace

extern "C" {
int mm_small_linear_fwd(const float* x, const float* W, const float* bias, const float* scale, const float* shift,
                        float* y, float* pre, int B, int K, int N, int act, float drop_p, uint32_t seed,
                        const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(x && W && y && B > 0 && K > 0 && N > 0, "small_linear_fwd: null/invalid");
    MM_REQUIRE((scale == nullptr) == (shift == nullptr), "small_linear_fwd: scale/shift come in pairs");
    MM_REQUIRE((size_t)K * 4 <= 64 * 1024, "small_linear_fwd: K=%d too large", K);
    const int gy = ceil_div(N, 4) < 64 ? ceil_div(N, 4) : 64;
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(small_linear_fwd_kernel, dim3(B, gy), dim3(256), K * sizeof(float), st, x, W, bias, scale, shift,
                       y, pre, B, K, N, act, d.thresh, seed, d.inv_keep, seed_epoch);
    return mm_check_launch("small_linear_fwd");
}
}  // extern "C"

namespace {
// dx[b][k] = sum_n dy[b][n] W[n][k]           (grid.x = B, threads over k)
__global__ void small_linear_dx_kernel(const float* __restrict__ dy, const float* __restrict__ W,
                                       float* __restrict__ dx, int B, int K, int N) {
    extern __shared__ float ds[];
    const int b = blockIdx.x;
    for (int n = threadIdx.x; n < N; n += blockDim.x) ds[n] = dy[(size_t)b * N + n];
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += ds[n] * W[(size_t)n * K + k];
        dx[(size_t)b * K + k] = s;
    }
}

// dW[n][k] += sum_b dy[b][n] x[b][k];  db[n] += sum_b dy[b][n]   (unique owner per element)
__global__ void small_linear_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                       float* __restrict__ dW, float* __restrict__ db, int B, int K, int N) {
    const int n = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dy[(size_t)b * N + n] * x[(size_t)b * K + k];
        dW[(size_t)n * K + k] += s;
    }
    if (db && threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dy[(size_t)b * N + n];
        db[n] += s;
    }
}
}  // namespace

extern "C" {
int mm_small_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, int B, int K,
                        int N, hipStream_t st) {
    MM_REQUIRE(dy && x && W && B > 0 && K > 0 && N > 0, "small_linear_bwd: null/invalid");
    MM_REQUIRE((size_t)N * 4 <= 64 * 1024, "small_linear_bwd: N=%d too large", N);
    if (dx) hipLaunchKernelGGL(small_linear_dx_kernel, dim3(B), dim3(256), N * sizeof(float), st, dy, W, dx, B, K, N);
    if (dW) hipLaunchKernelGGL(small_linear_dw_kernel, dim3(N), dim3(128), 0, st, dy, x, dW, db, B, K, N);
    return mm_check_launch("small_linear_bwd");
}
}  // extern "C"

namespace {
__global__ void act_f32_kernel(const float* __restrict__ z, float* __restrict__ y, size_t n, int act,
                               uint32_t thresh, uint32_t seed, float inv_keep, const uint32_t* epoch) {
    seed = mm_eff_seed(seed, epoch);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = apply_act(z[i], act);
        if (thresh) v *= dropout_scale(seed, (uint32_t)i, thresh, inv_keep);
        y[i] = v;
    }
}
}  // namespace

extern "C" {
int mm_act_f32(const float* z, float* y, int64_t n, int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
               hipStream_t st) {
    MM_REQUIRE(z && y && n > 0, "act_f32: null");
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(act_f32_kernel, dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, z, y, (size_t)n, act, d.thresh, seed,
                       d.inv_keep, seed_epoch);
    return mm_check_launch("act_f32");
}
}  // extern "C"

namespace {
__global__ void act_bwd_f32_kernel(const float* __restrict__ g, const float* __restrict__ z, float* __restrict__ out,
                                   size_t n, int act, uint32_t thresh, uint32_t seed, float inv_keep,
                                   const uint32_t* epoch) {
    seed = mm_eff_seed(seed, epoch);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = g[i];
        if (thresh) v *= dropout_scale(seed, (uint32_t)i, thresh, inv_keep);
        if (z) v *= act_grad(z[i], act);
        out[i] = v;
    }
}
}  // namespace

extern "C" {
int mm_act_bwd_f32(const float* g, const float* z, float* out, int64_t n, int act, float drop_p, uint32_t seed,
                   const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(g && out && n > 0, "act_bwd_f32: null");
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(act_bwd_f32_kernel, dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, g, z, out, (size_t)n, act,
                       d.thresh, seed, d.inv_keep, seed_epoch);
    return mm_check_launch("act_bwd_f32");
}
}  // extern "C"

namespace {
// column sum / sum-of-squares of fp32 [B][N]  (BatchNorm1d over a (B, N) batch)
__global__ void colstats_kernel(const float* __restrict__ x, float* __restrict__ stats, int B, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f, q = 0.f;
    for (int b = 0; b < B; ++b) { const float v = x[(size_t)b * N + n]; s += v; q += v * v; }
    // replica 0 of a statistics accumulator workspace (the input of mm_bn_finalize); the other replicas stay zero
    mm_acc_t* acc = reinterpret_cast<mm_acc_t*>(stats);
    acc[n] = acc_encode<MM_ACC_STAT>(s);
    acc[N + n] = acc_encode<MM_ACC_STAT>(q);
}
}  // namespace

extern "C" {
int mm_colstats(const float* x, float* stats, int B, int N, hipStream_t st) {
    MM_REQUIRE(x && stats && B > 0 && N > 0, "colstats: null");
    hipLaunchKernelGGL(colstats_kernel, dim3(ceil_div(N, 64)), dim3(64), 0, st, x, stats, B, N);
    return mm_check_launch("colstats");
}
}  // extern "C"

namespace {
// ---------------------------------------------------------------------------
// Both projection heads of the contrastive bridge in ONE launch each way
// (bridge_utils.py:34-45: Linear -> LayerNorm -> GELU -> Dropout, then F.normalize).
// At B = 32 the eleven separate launches of this chain each way were ~130 us of
// pure launch latency on the step's critical path.  grid = (B rows, 2 heads).
// ---------------------------------------------------------------------------
struct HeadSide {
    const float* x; const float* W; const float* bias; const float* gamma; const float* beta;
    float* dx; float* dW; float* dbias; float* dgamma; float* dbeta;
    int K; uint32_t seed;
};
struct HeadsArgs {
    HeadSide s[2];
    float* z1; float* hn; float* stat;        // [2][B][N], [2][B][N], [2][B][2]   saved for backward
    float* z; float* nrm;                     // [B][2N] packed embeddings, [2][B]
    const float* dz;                          // [B][2N]
    const float* da;                          // [2][B][N] more gradient at the heads' outputs (proj_heads_bwd_da), or null
    int B, N; float eps; uint32_t thresh; float inv_keep; const uint32_t* epoch;
};
constexpr int HEAD_MAXK = 1024, HEAD_MAXN = 256;

__device__ __forceinline__ float block_sum256(float v, float* red /* [4] */) {
    v = wave_sum(v);
    __syncthreads();                          // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void proj_heads_fwd_kernel(HeadsArgs a) {
    __shared__ float xs[HEAD_MAXK], v[HEAD_MAXN], red[4];
    const int b = blockIdx.x, m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HeadSide s = a.s[m];
    const int N = a.N, K = s.K;
    for (int k = tid; k < K; k += 256) xs[k] = s.x[(size_t)b * K + k];
    __syncthreads();
    // T = 256 / N lanes share one output; each issues its float4 loads of the weight row back to
    // back (a wave-per-output loop waits out one global-load round trip per output: 36 us at N = 128)
    const int T = N <= 64 ? 4 : (N <= 128 ? 2 : 1);
    {
        const int n = tid / T, part = tid % T;
        float acc = 0.f;
        if (n < N) {
            const float* wr = s.W + (size_t)n * K;
            if ((K & 3) == 0) {
#pragma unroll 8
                for (int k = part * 4; k < K; k += 4 * T) {
                    const float4 w4 = *reinterpret_cast<const float4*>(wr + k);
                    acc += w4.x * xs[k] + w4.y * xs[k + 1] + w4.z * xs[k + 2] + w4.w * xs[k + 3];
                }
            } else {
                for (int k = part; k < K; k += T) acc += wr[k] * xs[k];
            }
        }
        if (T >= 2) acc += __shfl_xor(acc, 1, 64);
        if (T >= 4) acc += __shfl_xor(acc, 2, 64);
        if (n < N && part == 0) v[n] = acc + (s.bias ? s.bias[n] : 0.f);
    }
    (void)lane; (void)wave;
    __syncthreads();
    const bool on = tid < N;
    const float x1 = on ? v[tid] : 0.f;
    const float mean = block_sum256(x1, red) / N;
    const float dlt = on ? x1 - mean : 0.f;
    const float rstd = rsqrtf(block_sum256(dlt * dlt, red) / N + a.eps);
    float act = 0.f, hn = 0.f;
    const size_t o = ((size_t)m * a.B + b) * N + tid;
    if (on) {
        hn = dlt * rstd * s.gamma[tid] + s.beta[tid];
        act = gelu_erf(hn);
        if (a.thresh) act *= dropout_scale(mm_eff_seed(s.seed, a.epoch), (uint32_t)(b * N + tid), a.thresh, a.inv_keep);
        if (a.z1) { a.z1[o] = x1; a.hn[o] = hn; }
    }
    const float nr = fmaxf(sqrtf(block_sum256(act * act, red)), 1e-12f);
    if (on) a.z[(size_t)b * 2 * N + m * N + tid] = act / nr;
    if (tid == 0) {
        a.nrm[m * a.B + b] = nr;
        if (a.stat) { a.stat[((size_t)m * a.B + b) * 2] = mean; a.stat[((size_t)m * a.B + b) * 2 + 1] = rstd; }
    }
}
}  // namespace

extern "C" {
int mm_proj_heads_fwd(const float* x_e, const float* W_e, const float* b_e, const float* g_e, const float* be_e, int K_e,
                      const float* x_f, const float* W_f, const float* b_f, const float* g_f, const float* be_f, int K_f,
                      float* z1, float* hn, float* stat, float* z, float* nrm, int B, int N, float eps, float drop_p,
                      uint32_t seed_e, uint32_t seed_f, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(x_e && W_e && g_e && be_e && x_f && W_f && g_f && be_f && z && nrm, "proj_heads_fwd: null");
    MM_REQUIRE((!z1 && !hn && !stat) || (z1 && hn && stat), "proj_heads_fwd: z1/hn/stat go together");
    MM_REQUIRE(B > 0 && N > 0 && N <= HEAD_MAXN && K_e > 0 && K_e <= HEAD_MAXK && K_f > 0 && K_f <= HEAD_MAXK,
               "proj_heads_fwd: B=%d N=%d K=%d/%d", B, N, K_e, K_f);
    HeadsArgs a{};
    a.s[0].x = x_e; a.s[0].W = W_e; a.s[0].bias = b_e; a.s[0].gamma = g_e; a.s[0].beta = be_e; a.s[0].K = K_e; a.s[0].seed = seed_e;
    a.s[1].x = x_f; a.s[1].W = W_f; a.s[1].bias = b_f; a.s[1].gamma = g_f; a.s[1].beta = be_f; a.s[1].K = K_f; a.s[1].seed = seed_f;
    a.z1 = z1; a.hn = hn; a.stat = stat; a.z = z; a.nrm = nrm; a.B = B; a.N = N; a.eps = eps;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.inv_keep = d.inv_keep; a.epoch = seed_epoch;
    hipLaunchKernelGGL(proj_heads_fwd_kernel, dim3(B, 2), dim3(256), 0, st, a);
    return mm_check_launch("proj_heads_fwd");
}
}  // extern "C"

namespace {
// Backward of both heads, bit-reproducible: no gradient element has more than one writer.  grid = (B, 2 heads),
// 16 waves.  EVERY block recomputes d z1 of all rows (a wave per row, two rows in flight per wave: a few hundred
// flops each, the same bits in every block), then block j writes dx of row j and the j-th slice of dW, each element
// summed over the rows in order; block 0 adds the bias and LayerNorm-parameter gradients (per-wave partials combined
// in wave order).  NE = ceil(N / 64) elements per lane.
// DA: a second gradient at the post-dropout activations, `a.da` (the classification branch reads the same rows), joins
// the F.normalize term before the dropout mask and GELU'.
constexpr int HB_RC = 32;                                   // rows per LDS chunk (= 2 per wave)
template <int NE, bool DA>
__global__ __launch_bounds__(1024) void proj_heads_bwd_kernel(HeadsArgs a) {
    __shared__ float d1[HB_RC][HEAD_MAXN];                  // 32 KB; re-used for the LayerNorm partials at the end
    __shared__ float px[1024];                              // dx partials [part][k]
    const int j = blockIdx.x, m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HeadSide s = a.s[m];
    const int N = a.N, K = s.K, B = a.B, G = gridDim.x;
    const int NK = N * K, S = (NK + G - 1) / G;
    const uint32_t seed = mm_eff_seed(s.seed, a.epoch);
    float ag[NE], ab[NE], gam[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        ag[e] = 0.f; ab[e] = 0.f;
        gam[e] = lane + 64 * e < N ? s.gamma[lane + 64 * e] : 0.f;
    }
    for (int b0 = 0; b0 < B; b0 += HB_RC) {
        const int nb = B - b0 < HB_RC ? B - b0 : HB_RC;
        __syncthreads();                                    // the previous chunk is consumed
        // rows wave and wave + 16 of the chunk: every load of both rows is issued before the first use
        float dzv[2][NE], zv[2][NE], hnv[2][NE], z1v[2][NE], dav[2][NE], mean[2], rstd[2], nr[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = wave + 16 * q;
            const bool row_on = r < nb;
            const int b = row_on ? b0 + r : b0;
            const size_t o = ((size_t)m * B + b) * N, oz = (size_t)b * 2 * N + m * N;
            mean[q] = a.stat[((size_t)m * B + b) * 2]; rstd[q] = a.stat[((size_t)m * B + b) * 2 + 1];
            nr[q] = a.nrm[m * B + b];
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int n = lane + 64 * e;
                const bool on = row_on && n < N;
                dzv[q][e] = on ? a.dz[oz + n] : 0.f;
                zv[q][e] = on ? a.z[oz + n] : 0.f;
                hnv[q][e] = on ? a.hn[o + n] : 0.f;
                z1v[q][e] = on ? a.z1[o + n] : 0.f;
                dav[q][e] = DA && on ? a.da[o + n] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = wave + 16 * q;
            if (r >= nb) continue;                          // (wave-uniform)
            const int b = b0 + r;
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) dot += dzv[q][e] * zv[q][e];
            dot = wave_sum(dot);
            float gd[NE], xh[NE], s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int n = lane + 64 * e;
                gd[e] = 0.f; xh[e] = 0.f;
                if (n < N) {
                    // F.normalize backward: da = (dz - z (z . dz)) / ||a||
                    float g = (dzv[q][e] - zv[q][e] * dot) / nr[q];
                    if (DA) g += dav[q][e];
                    if (a.thresh) g *= dropout_scale(seed, (uint32_t)(b * N + n), a.thresh, a.inv_keep);
                    const float dh = g * gelu_erf_grad(hnv[q][e]);
                    xh[e] = (z1v[q][e] - mean[q]) * rstd[q];
                    gd[e] = dh * gam[e];
                    ag[e] += dh * xh[e];
                    ab[e] += dh;
                }
                s1 += gd[e]; s2 += gd[e] * xh[e];
            }
            const float m1 = wave_sum(s1) / N, m2 = wave_sum(s2) / N;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int n = lane + 64 * e;
                if (n < N) d1[r][n] = rstd[q] * (gd[e] - m1 - xh[e] * m2);
            }
        }
        __syncthreads();
        // dx of the rows this block owns: 1024 / K threads share one output (strided over n), partials summed in order
        if (s.dx) {
            const int nparts = 1024 / K > 0 ? 1024 / K : 1;                 // K <= 1024 (host-checked)
            for (int b = j; b < b0 + nb; b += G) {
                if (b < b0) continue;
                const int k = tid % K, part = tid / K;
                if (part < nparts) {
                    float acc = 0.f;
#pragma unroll 4
                    for (int n = part; n < N; n += nparts) acc += d1[b - b0][n] * s.W[(size_t)n * K + k];
                    px[part * K + k] = acc;
                }
                __syncthreads();
                if (tid < K) {
                    float acc = 0.f;
                    for (int q = 0; q < nparts; ++q) acc += px[q * K + tid];
                    s.dx[(size_t)b * K + tid] = acc;
                }
                __syncthreads();
            }
        }
        if (s.dW) {
            const int hi = (j + 1) * S < NK ? (j + 1) * S : NK;
            for (int i = j * S + tid; i < hi; i += 1024) {
                const int n = i / K, k = i % K;
                const float* xc = s.x + (size_t)b0 * K + k;
                float acc = 0.f;
#pragma unroll 8
                for (int r = 0; r < nb; ++r) acc += d1[r][n] * xc[(size_t)r * K];
                s.dW[i] += acc;
            }
        }
        if (j == 0 && s.dbias && tid < N) {
            float acc = 0.f;
            for (int r = 0; r < nb; ++r) acc += d1[r][tid];
            s.dbias[tid] += acc;
        }
    }
    if (j == 0 && (s.dgamma || s.dbeta)) {
        __syncthreads();
        float (*pg)[2][HEAD_MAXN] = reinterpret_cast<float (*)[2][HEAD_MAXN]>(&d1[0][0]);     // [16 waves][dgamma | dbeta][N]
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int n = lane + 64 * e;
            if (n < N) { pg[wave][0][n] = ag[e]; pg[wave][1][n] = ab[e]; }
        }
        __syncthreads();
        if (tid < 2 * N) {
            const int which = tid / N, n = tid % N;
            float acc = 0.f;
            for (int w = 0; w < 16; ++w) acc += pg[w][which][n];
            float* dst = which ? s.dbeta : s.dgamma;
            if (dst) dst[n] += acc;
        }
    }
}
}  // namespace

extern "C" {
static int proj_heads_bwd_common(const float* dz, const float* da, const float* z, const float* nrm, const float* hn,
                                 const float* z1, const float* stat, const float* x_e, const float* W_e, const float* g_e,
                                 int K_e, const float* x_f, const float* W_f, const float* g_f, int K_f, float* dx_e,
                                 float* dW_e, float* db_e, float* dg_e, float* dbe_e, float* dx_f, float* dW_f, float* db_f,
                                 float* dg_f, float* dbe_f, int B, int N, float drop_p, uint32_t seed_e, uint32_t seed_f,
                                 const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(dz && z && nrm && hn && z1 && stat && x_e && W_e && g_e && x_f && W_f && g_f, "proj_heads_bwd: null");
    MM_REQUIRE(B > 0 && N > 0 && N <= HEAD_MAXN && K_e > 0 && K_e <= HEAD_MAXK && K_f > 0 && K_f <= HEAD_MAXK,
               "proj_heads_bwd: B=%d N=%d K=%d/%d", B, N, K_e, K_f);
    HeadsArgs a{};
    a.s[0].x = x_e; a.s[0].W = W_e; a.s[0].gamma = g_e; a.s[0].K = K_e; a.s[0].seed = seed_e;
    a.s[0].dx = dx_e; a.s[0].dW = dW_e; a.s[0].dbias = db_e; a.s[0].dgamma = dg_e; a.s[0].dbeta = dbe_e;
    a.s[1].x = x_f; a.s[1].W = W_f; a.s[1].gamma = g_f; a.s[1].K = K_f; a.s[1].seed = seed_f;
    a.s[1].dx = dx_f; a.s[1].dW = dW_f; a.s[1].dbias = db_f; a.s[1].dgamma = dg_f; a.s[1].dbeta = dbe_f;
    a.z1 = const_cast<float*>(z1); a.hn = const_cast<float*>(hn); a.stat = const_cast<float*>(stat);
    a.z = const_cast<float*>(z); a.nrm = const_cast<float*>(nrm); a.dz = dz; a.da = da; a.B = B; a.N = N;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.inv_keep = d.inv_keep; a.epoch = seed_epoch;
#define MM_HEADS_BWD(NE)                                                                                  \
    if (da) hipLaunchKernelGGL((proj_heads_bwd_kernel<NE, true>), dim3(B, 2), dim3(1024), 0, st, a);      \
    else hipLaunchKernelGGL((proj_heads_bwd_kernel<NE, false>), dim3(B, 2), dim3(1024), 0, st, a)
    switch (ceil_div(N, 64)) {
        case 1: MM_HEADS_BWD(1); break;
        case 2: MM_HEADS_BWD(2); break;
        case 3: MM_HEADS_BWD(3); break;
        default: MM_HEADS_BWD(4); break;
    }
#undef MM_HEADS_BWD
    return mm_check_launch("proj_heads_bwd");
}

int mm_proj_heads_bwd(const float* dz, const float* z, const float* nrm, const float* hn, const float* z1,
                      const float* stat, const float* x_e, const float* W_e, const float* g_e, int K_e,
                      const float* x_f, const float* W_f, const float* g_f, int K_f, float* dx_e, float* dW_e,
                      float* db_e, float* dg_e, float* dbe_e, float* dx_f, float* dW_f, float* db_f, float* dg_f,
                      float* dbe_f, int B, int N, float drop_p, uint32_t seed_e, uint32_t seed_f,
                      const uint32_t* seed_epoch, hipStream_t st) {
    return proj_heads_bwd_common(dz, nullptr, z, nrm, hn, z1, stat, x_e, W_e, g_e, K_e, x_f, W_f, g_f, K_f, dx_e, dW_e, db_e,
                                 dg_e, dbe_e, dx_f, dW_f, db_f, dg_f, dbe_f, B, N, drop_p, seed_e, seed_f, seed_epoch, st);
}

// mm_proj_heads_bwd with one more gradient at the heads' outputs: da (2, B, N) = d loss / d (the post-GELU/dropout
// activations a_e, a_f) from a second consumer of those rows (mm_bridge_cls_bwd), added to the F.normalize-backward
// term before the dropout mask and GELU'.  The same kernel, compiled with the extra load.
int mm_proj_heads_bwd_da(const float* dz, const float* da, const float* z, const float* nrm, const float* hn,
                         const float* z1, const float* stat, const float* x_e, const float* W_e, const float* g_e, int K_e,
                         const float* x_f, const float* W_f, const float* g_f, int K_f, float* dx_e, float* dW_e,
                         float* db_e, float* dg_e, float* dbe_e, float* dx_f, float* dW_f, float* db_f, float* dg_f,
                         float* dbe_f, int B, int N, float drop_p, uint32_t seed_e, uint32_t seed_f,
                         const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(da, "proj_heads_bwd_da: null");
    return proj_heads_bwd_common(dz, da, z, nrm, hn, z1, stat, x_e, W_e, g_e, K_e, x_f, W_f, g_f, K_f, dx_e, dW_e, db_e,
                                 dg_e, dbe_e, dx_f, dW_f, db_f, dg_f, dbe_f, B, N, drop_p, seed_e, seed_f, seed_epoch, st);
}
}  // extern "C"

namespace {
// ---------------------------------------------------------------------------
// Encoder output head on the pooled token (enhanced_models_v4.py:161-167, 188-191): Linear(D -> N) ->
// act -> Dropout on pooled[b] (the mean over time arrives already reduced), fp32 FMAs, one workgroup
// per sample.  Backward: dz = dout * mask * act'(z); d pooled = dz W; every token of the sample gets
// d pooled / L (the mean's gradient), optionally with a second, dropout-masked bf16 copy for the GEMM
// that consumes it next.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pooled_head_fwd_kernel(const float* __restrict__ pooled, const mm_acc_t* __restrict__ pooled_acc,
                                                             const float* __restrict__ W,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             bf16* __restrict__ z_pre, bf16* __restrict__ pooled_bf16,
                                                             int D, int N, int act, uint32_t thresh, float inv_keep,
                                                             uint32_t seed, const uint32_t* __restrict__ epoch) {
    __shared__ float xs[1024];
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < D; k += 256) {
        const float v = pooled ? pooled[(size_t)b * D + k] : acc_val<MM_ACC_GRAD>(pooled_acc[(size_t)b * D + k]);
        xs[k] = v;
        if (pooled_bf16) pooled_bf16[(size_t)b * D + k] = (bf16)v;
    }
    __syncthreads();
    seed = mm_eff_seed(seed, epoch);
    for (int n = threadIdx.x; n < N; n += 256) {
        const float* wr = W + (size_t)n * D;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int k = 0;
        for (; k + 64 <= D; k += 64) {                      // sixteen independent float4 loads per round (see pooled_head_bwd_kernel)
            float4 w4[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w4[q] = *reinterpret_cast<const float4*>(wr + k + q * 4);
#pragma unroll
            for (int q = 0; q < 16; ++q)
                acc[q & 3] += w4[q].x * xs[k + q * 4] + w4[q].y * xs[k + q * 4 + 1] + w4[q].z * xs[k + q * 4 + 2] +
                              w4[q].w * xs[k + q * 4 + 3];
        }
        for (; k < D; k += 16) {                            // four independent float4 loads per round
            float4 w4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w4[q] = *reinterpret_cast<const float4*>(wr + k + q * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[q] += w4[q].x * xs[k + q * 4] + w4[q].y * xs[k + q * 4 + 1] + w4[q].z * xs[k + q * 4 + 2] +
                          w4[q].w * xs[k + q * 4 + 3];
        }
        const float z = (acc[0] + acc[1]) + (acc[2] + acc[3]) + (bias ? bias[n] : 0.f);
        const size_t idx = (size_t)b * N + n;
        if (z_pre) z_pre[idx] = (bf16)z;
        float v = apply_act(z, act);
        if (thresh) v *= dropout_scale(seed, (uint32_t)idx, thresh, inv_keep);
        out[idx] = v;
    }
}
}  // namespace

extern "C" {
int mm_pooled_head_fwd(const float* pooled, const float* pooled_acc, const float* W, const float* bias, float* out, void* z_pre_bf16,
                       void* pooled_bf16, int B, int D, int N, int act, float drop_p, uint32_t seed,
                       const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE((pooled != nullptr) != (pooled_acc != nullptr) && W && out && B > 0, "pooled_head_fwd: null (exactly one of pooled / pooled_acc)");
    MM_REQUIRE(D > 0 && D <= 1024 && D % 16 == 0 && N > 0, "pooled_head_fwd: D=%d (multiple of 16, <= 1024)", D);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "pooled_head_fwd: drop_p");
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(pooled_head_fwd_kernel, dim3(B), dim3(256), 0, st, pooled, reinterpret_cast<const mm_acc_t*>(pooled_acc), W, bias, out, (bf16*)z_pre_bf16,
                       (bf16*)pooled_bf16, D, N, act, d.thresh, d.inv_keep, seed, seed_epoch);
    return mm_check_launch("pooled_head_fwd");
}
}  // extern "C"

namespace {
__global__ __launch_bounds__(256) void pooled_head_bwd_kernel(const float* __restrict__ dout, const bf16* __restrict__ z_pre,
                                                             const float* __restrict__ W, bf16* __restrict__ dz_bf16,
                                                             float* __restrict__ dx, bf16* __restrict__ dx_bf16, int L, int D,
                                                             int N, int rows_per_wg, int act, uint32_t thresh, float inv_keep,
                                                             uint32_t seed, uint32_t thresh2, float inv_keep2, uint32_t seed2,
                                                             const uint32_t* __restrict__ epoch, float* __restrict__ rows_out) {
    __shared__ float dz[1024];
    __shared__ __attribute__((aligned(16))) float dp[1024];
    const int b = blockIdx.x, l0 = blockIdx.y * rows_per_wg;
    seed = mm_eff_seed(seed, epoch);
    seed2 = mm_eff_seed(seed2, epoch);
    for (int n = threadIdx.x; n < N; n += 256) {
        const size_t idx = (size_t)b * N + n;
        float g = dout[idx] * act_grad((float)z_pre[idx], act);
        if (thresh) g *= dropout_scale(seed, (uint32_t)idx, thresh, inv_keep);
        dz[n] = g;
        if (blockIdx.y == 0 && dz_bf16) dz_bf16[idx] = (bf16)g;
    }
    __syncthreads();
    const float invL = 1.f / (float)L;
    for (int k = threadIdx.x; k < D; k += 256) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int n = 0;
        // coalesced across k; four chains, SIXTEEN loads in flight per round: this loop is a chain of L2 round trips with one
        // workgroup per sample on the chip (13 us for N = 128 at four per round, alone in the serial heads section of the step)
        for (; n + 16 <= N; n += 16) {
            float w[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = W[(size_t)(n + q) * D + k];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q & 3] += dz[n + q] * w[q];
        }
        for (; n < N; n += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += dz[n + q] * W[(size_t)(n + q) * D + k];
        }
        dp[k] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) * invL;
        if (rows_out && blockIdx.y == 0) rows_out[(size_t)b * D + k] = dp[k];     // the ONE row every token of the sample receives
    }
    __syncthreads();
    const int vec = D / 4;                                  // float4 groups per row
    const int lend = min(L, l0 + rows_per_wg);
    for (int i = threadIdx.x; i < (lend - l0) * vec; i += 256) {
        const int l = l0 + i / vec, k4 = (i % vec) * 4;
        const float4 v = *reinterpret_cast<const float4*>(dp + k4);
        const size_t base = ((size_t)b * L + l) * D + k4;
        if (dx) *reinterpret_cast<float4*>(dx + base) = v;
        if (dx_bf16) {
            const float vs[4] = {v.x, v.y, v.z, v.w};
            bf16x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                o[c] = (bf16)(thresh2 ? vs[c] * dropout_scale(seed2, (uint32_t)(base + c), thresh2, inv_keep2) : vs[c]);
            *reinterpret_cast<bf16x4*>(dx_bf16 + base) = o;
        }
    }
}
}  // namespace

extern "C" {
static int pooled_head_bwd_common(const float* dout, const void* z_pre_bf16, const float* W, void* dz_bf16, float* dx,
                                  void* dx_bf16, float* rows_out, int B, int L, int D, int N, int act, float drop_p,
                                  uint32_t seed, float emit_drop_p, uint32_t emit_seed, const uint32_t* seed_epoch,
                                  hipStream_t st) {
    MM_REQUIRE(dout && z_pre_bf16 && W && (dx || dx_bf16) && B > 0 && L > 0, "pooled_head_bwd: null");
    MM_REQUIRE(D > 0 && D <= 1024 && D % 4 == 0 && N > 0 && N <= 1024 && N % 4 == 0, "pooled_head_bwd: D=%d N=%d", D, N);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f && emit_drop_p >= 0.f && emit_drop_p < 1.f, "pooled_head_bwd: drop_p");
    const int rows = 32;
    const DropH d1 = mm_drop(drop_p), d2 = mm_drop(emit_drop_p);
    hipLaunchKernelGGL(pooled_head_bwd_kernel, dim3(B, (L + rows - 1) / rows), dim3(256), 0, st, dout, (const bf16*)z_pre_bf16, W,
                       (bf16*)dz_bf16, dx, (bf16*)dx_bf16, L, D, N, rows, act, d1.thresh, d1.inv_keep, seed,
                       d2.thresh, d2.inv_keep, emit_seed, seed_epoch, rows_out);
    return mm_check_launch("pooled_head_bwd");
}

int mm_pooled_head_bwd(const float* dout, const void* z_pre_bf16, const float* W, void* dz_bf16, float* dx, void* dx_bf16,
                       int B, int L, int D, int N, int act, float drop_p, uint32_t seed, float emit_drop_p,
                       uint32_t emit_seed, const uint32_t* seed_epoch, hipStream_t st) {
    return pooled_head_bwd_common(dout, z_pre_bf16, W, dz_bf16, dx, dx_bf16, nullptr, B, L, D, N, act, drop_p, seed, emit_drop_p,
                                  emit_seed, seed_epoch, st);
}

// mm_pooled_head_bwd without the fp32 (B, L, D) token gradients: every token of sample b receives rows_out[b] (B, D), so a
// consumer that takes the row (mm_linear_dgrad_ln_bwd_gemm2's dres_rows_per_sample, mm_bn_act_bwd_*_bcast) needs only that;
// dx_bf16 (B, L, D) = the rows under the consumer's dropout mask (emit_drop_p, emit_seed), as before.
int mm_pooled_head_bwd_rows(const float* dout, const void* z_pre_bf16, const float* W, void* dz_bf16, float* rows_out,
                            void* dx_bf16, int B, int L, int D, int N, int act, float drop_p, uint32_t seed,
                            float emit_drop_p, uint32_t emit_seed, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(rows_out && dx_bf16, "pooled_head_bwd_rows: null");
    return pooled_head_bwd_common(dout, z_pre_bf16, W, dz_bf16, nullptr, dx_bf16, rows_out, B, L, D, N, act, drop_p, seed,
                                  emit_drop_p, emit_seed, seed_epoch, st);
}
}  // extern "C"

namespace {
// drop_path / stochastic depth (crossmodal_v4_enhancements.py:639-650): sample b is kept with
// probability 1 - p and scaled by 1 / (1 - p); the mask depends on (seed, b) only, so the same
// launch on the upstream gradient is the backward.
__global__ void drop_path_kernel(const float* __restrict__ x, float* __restrict__ o, size_t n, size_t inner,
                                 uint32_t thresh, float inv_keep, uint32_t base, const uint32_t* __restrict__ epoch) {
    const uint32_t seed = mm_eff_seed(base, epoch);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        o[i] = x[i] * dropout_scale(seed, (uint32_t)(i / inner), thresh, inv_keep);
}
}  // namespace

extern "C" {
int mm_drop_path(const float* x, float* out, int64_t B, int64_t inner, float drop_p, uint32_t seed,
                 const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(x && out && B > 0 && inner > 0 && drop_p >= 0.f && drop_p < 1.f, "drop_path: bad args");
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(drop_path_kernel, dim3(grid_for((size_t)(B * inner), 2048)), dim3(256), 0, st, x, out, (size_t)(B * inner),
                       (size_t)inner, d.thresh, d.inv_keep, seed, seed_epoch);
    return mm_check_launch("drop_path");
}
}  // extern "C"

namespace {
// mean over S of bf16 [R][S][N] -> fp32 [R][N]   (AdaptiveAvgPool1d(1) of the Lite encoders)
__global__ void meanpool_bf16_kernel(const bf16* __restrict__ x, float* __restrict__ out, int S, int N) {
    const int r = blockIdx.x;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float s = 0.f;
        for (int t = 0; t < S; ++t) s += (float)x[((size_t)r * S + t) * N + n];
        out[(size_t)r * N + n] = s / (float)S;
    }
}
}  // namespace

extern "C" {
int mm_meanpool_bf16(const void* x, float* out, int R, int S, int N, hipStream_t st) {
    MM_REQUIRE(x && out && R > 0 && S > 0 && N > 0, "meanpool_bf16: null");
    hipLaunchKernelGGL(meanpool_bf16_kernel, dim3(R), dim3(128), 0, st, (const bf16*)x, out, S, N);
    return mm_check_launch("meanpool_bf16");
}
}  // extern "C"

namespace {
__global__ void add_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) o[i] = a[i] + b[i];
}
}  // namespace

extern "C" {
int mm_add_f32(const float* a, const float* b, float* out, int64_t n, hipStream_t st) {
    MM_REQUIRE(a && b && out && n > 0, "add_f32: null");
    hipLaunchKernelGGL(add_f32_kernel, dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, a, b, out, (size_t)n);
    return mm_check_launch("add_f32");
}
}  // extern "C"

namespace {
__global__ void mul_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ o, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) o[i] = a[i] * b[i];
}
}  // namespace

extern "C" {
int mm_mul_f32(const float* a, const float* b, float* out, int64_t n, hipStream_t st) {
    MM_REQUIRE(a && b && out && n > 0, "mul_f32: null");
    hipLaunchKernelGGL(mul_f32_kernel, dim3(grid_for((size_t)n, 2048)), dim3(256), 0, st, a, b, out, (size_t)n);
    return mm_check_launch("mul_f32");
}
}  // extern "C"
