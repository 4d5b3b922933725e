// Tails of the EEG notebook's single-modality baselines (EEG_CODE/CrossModal_EEG_scr.ipynb: PWOnlyNet, ERPOnlyNet): a
// 1 x 1 projection of every time step of the 128-wide third conv block, then a pooling over time that collapses the
// sequence.  The projected (B, L, P) tensor is never written, read or differentiated as a tensor:
//   max tail (PWOnlyNet: proj -> Dropout -> AdaptiveMaxPool1d(1)): the projection runs on the bf16 MFMA and the running
//     (max, arg-max) over time lives in the accumulator layout; the backward is a gather through the arg-max.
//   avg tail (ERPOnlyNet: step_proj -> AdaptiveAvgPool1d(bins) -> Flatten): the projection is affine and nothing sits
//     between it and the pooling, so the time bins are averaged FIRST and `bins` rows per sample are projected (fp32).
// No floating-point atomics anywhere: every sum has one owner and a fixed order, so two runs give the same bits.
// Callers: small_autograd.py (PWOnlyFn, ERPOnlyFn), ops.py (eeg_baseline_forward).  DESIGN.md 5o.
#include "common.h"
#include "mmeeg_hip.h"

namespace {
constexpr int TP_K = 128;              // the encoders' fixed third width
constexpr int TP_PMAX = 512;
constexpr int TP_CT = 64;              // max tail: columns of one workgroup = 4 MFMA column tiles
constexpr int TP_WAVES = 4;            // ... and its waves; a time chunk = 16 rows per wave = 64 rows
constexpr int TP_BINS_MAX = 8;
constexpr int TP_RB = 64;              // backward: rows of dx per workgroup

// candidate (v, t) beats the held (bv, bt): larger value, or the same value earlier in time (torch's rule: the first
// maximum); a NaN wins over every number, as in torch.max
__device__ __forceinline__ bool tp_beats(float v, int t, float bv, int bt) {
    if (v != v) return bv == bv || t < bt;
    return v > bv || (v == bv && t < bt);
}

// one workgroup per (sample, 64-column tile); the weight tile stays in registers for the whole time loop.
// mfma_f32_16x16x32_bf16: A = 16 time rows of x (lane l: row l & 15, k = 8 (l >> 4) + j), B = w^T (lane l: column l & 15,
// same k), C: column l & 15 on the lane, rows 4 (l >> 4) + r in the registers - a lane sees its column's rows in
// ascending time order, so a strict > keeps the first maximum.
__global__ __launch_bounds__(64 * TP_WAVES) void timepool_max_fwd_kernel(
        const bf16* __restrict__ x, const bf16* __restrict__ w, const float* __restrict__ bias,
        float* __restrict__ pooled, int* __restrict__ arg, int L, int P, uint32_t thresh, uint32_t seed, float inv_keep,
        const uint32_t* epoch) {
    seed = mm_eff_seed(seed, epoch);
    const int b = blockIdx.x, n0 = blockIdx.y * TP_CT;
    const int nt = (P - n0) / 16 < 4 ? (P - n0) / 16 : 4;          // column tiles of this workgroup (P % 16 == 0)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lg = lane >> 4;
    bf16x8 wfr[4][4];                                               // [column tile][k step]
    float bs[4], best[4];
    int bt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + lc;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 z = {};
            wfr[j][ks] = j < nt ? *reinterpret_cast<const bf16x8*>(w + (size_t)n * TP_K + 32 * ks + 8 * lg) : z;
        }
        bs[j] = (j < nt && bias) ? bias[n] : 0.f;
        best[j] = -INFINITY;
        bt[j] = 0;
    }
    const bf16* xb = x + (size_t)b * L * TP_K;
    for (int t0 = 16 * wave; t0 < L; t0 += 16 * TP_WAVES) {
        const int tr = t0 + lc;
        bf16x8 a[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            bf16x8 z = {};
            a[ks] = tr < L ? *reinterpret_cast<const bf16x8*>(xb + (size_t)tr * TP_K + 32 * ks + 8 * lg) : z;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nt) break;                                     // uniform over the workgroup
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], wfr[j][ks], c, 0, 0, 0);
            const uint32_t n = (uint32_t)(n0 + 16 * j + lc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + 4 * lg + r;
                if (t >= L) continue;
                float y = c[r] + bs[j];
                if (thresh) y *= dropout_scale(seed, ((uint32_t)b * (uint32_t)L + (uint32_t)t) * (uint32_t)P + n, thresh, inv_keep);
                if (y > best[j] || (y != y && best[j] == best[j])) { best[j] = y; bt[j] = t; }
            }
        }
    }
    // merge the 16 partial (max, t) of a column - 4 lane groups x 4 waves - through LDS, scanned in slot order
    __shared__ float sv[4 * TP_WAVES][TP_CT];
    __shared__ int st[4 * TP_WAVES][TP_CT];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sv[4 * wave + lg][16 * j + lc] = best[j];
        st[4 * wave + lg][16 * j + lc] = bt[j];
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < 16 * nt) {
        float bv = sv[0][c];
        int bi = st[0][c];
        for (int s = 1; s < 4 * TP_WAVES; ++s)
            if (tp_beats(sv[s][c], st[s][c], bv, bi)) { bv = sv[s][c]; bi = st[s][c]; }
        pooled[(size_t)b * P + n0 + c] = bv;
        arg[(size_t)b * P + n0 + c] = bi;
    }
}

// g[b][n] = dpooled[b][n] * keep-scale at the winner; an arg outside [0, L) (never written by the forward) reads as "no row"
__device__ __forceinline__ float tp_g(const float* dpooled, int b, int n, int a, int L, int P, uint32_t thresh, uint32_t seed,
                                      float inv_keep) {
    float g = dpooled[(size_t)b * P + n];
    if (thresh) g *= dropout_scale(seed, ((uint32_t)b * (uint32_t)L + (uint32_t)a) * (uint32_t)P + (uint32_t)n, thresh, inv_keep);
    return g;
}

// dx[b][t][:] = sum over the columns won by row t of g[b][n] w[n][:], n ascending; one workgroup per (sample, 64 rows).
// The columns are rank-sorted by (arg, n) in LDS, the first sorted position of every row of the chunk goes into a table,
// and EVERY row is written (most with zeros).
__global__ __launch_bounds__(256) void timepool_max_bwd_dx_kernel(
        const float* __restrict__ dpooled, const int* __restrict__ arg, const bf16* __restrict__ w, bf16* __restrict__ dx,
        int L, int P, uint32_t thresh, uint32_t seed, float inv_keep, const uint32_t* epoch) {
    seed = mm_eff_seed(seed, epoch);
    __shared__ int ta[TP_PMAX], sn[TP_PMAX], stt[TP_PMAX], first[TP_RB];
    __shared__ float sg[TP_PMAX];
    const int b = blockIdx.x, t0 = blockIdx.y * TP_RB;
    for (int n = threadIdx.x; n < P; n += blockDim.x) {
        const int a = arg[(size_t)b * P + n];
        const bool ok = a >= 0 && a < L;
        ta[n] = ok ? a : L;
        sg[n] = ok ? tp_g(dpooled, b, n, a, L, P, thresh, seed, inv_keep) : 0.f;
    }
    if (threadIdx.x < TP_RB) first[threadIdx.x] = P;                 // no column
    __syncthreads();
    for (int n = threadIdx.x; n < P; n += blockDim.x) {
        const int a = ta[n];
        int r = 0;
        for (int m = 0; m < P; ++m) r += (ta[m] < a || (ta[m] == a && m < n)) ? 1 : 0;
        sn[r] = n;
        stt[r] = a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int a = stt[i];
        if (a >= t0 && a < t0 + TP_RB && (i == 0 || stt[i - 1] != a)) first[a - t0] = i;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int t = t0 + wave; t < L && t < t0 + TP_RB; t += nw) {
        // fp64: a product fp32 x bf16 is exact in it, so a row whose terms cancel still rounds to bf16 ONCE (in fp32 the
        // rounding of the first product alone can exceed a bf16 ulp of a small sum); a row has a handful of terms
        double a0 = 0.0, a1 = 0.0;
        for (int i = first[t - t0]; i < P && stt[i] == t; ++i) {
            const int n = sn[i];
            const bf16x2 wv = *reinterpret_cast<const bf16x2*>(w + (size_t)n * TP_K + 2 * lane);
            a0 += (double)sg[n] * (double)(float)wv[0];
            a1 += (double)sg[n] * (double)(float)wv[1];
        }
        bf16x2 o = {(bf16)(float)a0, (bf16)(float)a1};
        *reinterpret_cast<bf16x2*>(dx + ((size_t)b * L + t) * TP_K + 2 * lane) = o;
    }
}

// dw[n][:] += sum_b g[b][n] x[b][arg[b][n]][:], dbias[n] += sum_b g[b][n], b ascending; one workgroup per column.  The
// winners and g of up to 256 samples are staged in LDS first, so the x rows of consecutive samples load independently
// (eight in flight) instead of behind their own arg / dpooled loads
__global__ __launch_bounds__(TP_K) void timepool_max_bwd_dw_kernel(
        const float* __restrict__ dpooled, const int* __restrict__ arg, const bf16* __restrict__ x, float* __restrict__ dw,
        float* __restrict__ dbias, int B, int L, int P, uint32_t thresh, uint32_t seed, float inv_keep, const uint32_t* epoch) {
    seed = mm_eff_seed(seed, epoch);
    __shared__ int sa[256];
    __shared__ float sgg[256];
    const int n = blockIdx.x, k = threadIdx.x;
    float s = 0.f, sb = 0.f;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int nb = B - b0 < 256 ? B - b0 : 256;
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += blockDim.x) {
            const int a = arg[(size_t)(b0 + i) * P + n];
            const bool ok = a >= 0 && a < L;
            sa[i] = ok ? a : -1;
            sgg[i] = ok ? tp_g(dpooled, b0 + i, n, a, L, P, thresh, seed, inv_keep) : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < nb; ++i) {
            const int a = sa[i];
            const float xv = (float)x[((size_t)(b0 + i) * L + (a < 0 ? 0 : a)) * TP_K + k];
            s += sgg[i] * (a < 0 ? 0.f : xv);
            sb += sgg[i];
        }
    }
    if (dw) dw[(size_t)n * TP_K + k] += s;
    if (dbias && k == 0) dbias[n] += sb;
}

// torch's adaptive bins: [floor(i L / bins), ceil((i + 1) L / bins)); they overlap when bins does not divide L
__device__ __forceinline__ int tp_bin_start(int i, int L, int bins) { return (int)(((long long)i * L) / bins); }
__device__ __forceinline__ int tp_bin_end(int i, int L, int bins) { return (int)((((long long)i + 1) * L + bins - 1) / bins); }

// one workgroup per (sample, bin): the bin's mean (ascending t) -> LDS and xbin, then pooled[b][p bins + i] = xbin[i] . w[p] + bias[p]
__global__ __launch_bounds__(256) void timepool_avg_fwd_kernel(
        const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ xbin,
        float* __restrict__ pooled, int L, int P, int bins) {
    __shared__ float xs[TP_K];
    const int b = blockIdx.x, i = blockIdx.y;
    if (threadIdx.x < TP_K) {
        const int k = threadIdx.x, t0 = tp_bin_start(i, L, bins), t1 = tp_bin_end(i, L, bins);
        const float* xb = x + (size_t)b * L * TP_K + k;
        float s = 0.f;
#pragma unroll 8
        for (int t = t0; t < t1; ++t) s += xb[(size_t)t * TP_K];
        s /= (float)(t1 - t0);
        xs[k] = s;
        xbin[((size_t)b * bins + i) * TP_K + k] = s;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        const float4* wr = reinterpret_cast<const float4*>(w + (size_t)p * TP_K);
        float s = 0.f;
#pragma unroll 8
        for (int q = 0; q < TP_K / 4; ++q) {
            const float4 wv = wr[q];
            s += xs[4 * q] * wv.x;
            s += xs[4 * q + 1] * wv.y;
            s += xs[4 * q + 2] * wv.z;
            s += xs[4 * q + 3] * wv.w;
        }
        pooled[((size_t)b * P + p) * bins + i] = s + (bias ? bias[p] : 0.f);
    }
}

// one workgroup per (sample, 64 rows): u[i][:] = (sum_p dpooled[p bins + i] w[p][:]) / len_i (p ascending) for the bins that
// reach into the chunk, then dx[t][:] = sum over the bins that hold t of u[i][:] (i ascending); every row of dx is written
__global__ __launch_bounds__(256) void timepool_avg_bwd_dx_kernel(
        const float* __restrict__ dpooled, const float* __restrict__ w, float* __restrict__ dx, int L, int P, int bins) {
    __shared__ float dp[TP_PMAX * TP_BINS_MAX];
    __shared__ float us[TP_BINS_MAX * TP_K];
    const int b = blockIdx.x, t0 = blockIdx.y * TP_RB, t1 = t0 + TP_RB < L ? t0 + TP_RB : L;
    for (int o = threadIdx.x; o < P * bins; o += blockDim.x) dp[o] = dpooled[(size_t)b * P * bins + o];
    __syncthreads();
    for (int e = threadIdx.x; e < bins * TP_K; e += blockDim.x) {
        const int i = e / TP_K, k = e % TP_K;
        const int s0 = tp_bin_start(i, L, bins), s1 = tp_bin_end(i, L, bins);
        if (s1 <= t0 || s0 >= t1) continue;                          // no row of this chunk reads it
        float s = 0.f;
#pragma unroll 8
        for (int p = 0; p < P; ++p) s += dp[p * bins + i] * w[(size_t)p * TP_K + k];
        us[e] = s / (float)(s1 - s0);
    }
    __syncthreads();
    float* dxb = dx + (size_t)b * L * TP_K;
    for (int e = t0 * TP_K + threadIdx.x; e < t1 * TP_K; e += blockDim.x) {
        const int t = e / TP_K, k = e % TP_K;
        float s = 0.f;
        for (int i = 0; i < bins; ++i)
            if (t >= tp_bin_start(i, L, bins) && t < tp_bin_end(i, L, bins)) s += us[i * TP_K + k];
        dxb[e] = s;
    }
}

// dw[p][:] += sum_b sum_i dpooled[b][p bins + i] xbin[b][i][:], dbias[p] += sum_{b, i} dpooled[b][p bins + i]
__global__ __launch_bounds__(TP_K) void timepool_avg_bwd_dw_kernel(
        const float* __restrict__ dpooled, const float* __restrict__ xbin, float* __restrict__ dw, float* __restrict__ dbias,
        int B, int P, int bins) {
    const int p = blockIdx.x, k = threadIdx.x;
    float s = 0.f, sb = 0.f;
#pragma unroll 8
    for (int j = 0; j < B * bins; ++j) {                             // j = b bins + i: xbin's row index
        const float g = dpooled[((size_t)(j / bins) * P + p) * bins + j % bins];
        s += g * xbin[(size_t)j * TP_K + k];
        sb += g;
    }
    if (dw) dw[(size_t)p * TP_K + k] += s;
    if (dbias && k == 0) dbias[p] += sb;
}

int tp_sizes(const char* who, int B, int L, int K, int P) {
    if (K != TP_K) return mm_fail(MM_ERR_UNSUPPORTED, "%s: K=%d (the kernels serve K = %d)", who, K, TP_K);
    if (P < 16 || P > TP_PMAX || P % 16) return mm_fail(MM_ERR_UNSUPPORTED, "%s: P=%d (a multiple of 16 up to %d)", who, P, TP_PMAX);
    if (B < 1 || L < 1) return mm_fail(MM_ERR_UNSUPPORTED, "%s: B=%d L=%d (both >= 1)", who, B, L);
    if (L > TP_RB * 65535) return mm_fail(MM_ERR_UNSUPPORTED, "%s: L=%d (at most %d: one grid row per %d time steps)", who, L, TP_RB * 65535, TP_RB);
    if ((unsigned long long)B * (unsigned long long)L * (unsigned long long)P > 0xFFFFFFFFull)
        return mm_fail(MM_ERR_UNSUPPORTED, "%s: B*L*P = %d*%d*%d exceeds the 32-bit dropout index", who, B, L, P);
    return MM_OK;
}
}  // namespace

extern "C" {
int mm_timepool_max_fwd(const void* x_bf16, const void* w_bf16, const float* bias, float* pooled, int* arg, int B, int L,
                        int K, int P, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(x_bf16 && w_bf16 && pooled && arg, "timepool_max_fwd: null");
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "timepool_max_fwd: drop_p=%g", (double)drop_p);
    if (int rc = tp_sizes("timepool_max_fwd", B, L, K, P)) return rc;
    const DropH d = mm_drop(drop_p);
    hipLaunchKernelGGL(timepool_max_fwd_kernel, dim3(B, ceil_div(P, TP_CT)), dim3(64 * TP_WAVES), 0, st, (const bf16*)x_bf16,
                       (const bf16*)w_bf16, bias, pooled, arg, L, P, d.thresh, seed, d.inv_keep, seed_epoch);
    return mm_check_launch("timepool_max_fwd");
}

int mm_timepool_max_bwd(const float* dpooled, const int* arg, const void* x_bf16, const void* w_bf16, void* dx_bf16,
                        float* dw, float* dbias, int B, int L, int K, int P, float drop_p, uint32_t seed,
                        const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(dpooled && arg && x_bf16 && w_bf16, "timepool_max_bwd: null");
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "timepool_max_bwd: drop_p=%g", (double)drop_p);
    if (int rc = tp_sizes("timepool_max_bwd", B, L, K, P)) return rc;
    const DropH d = mm_drop(drop_p);
    if (dx_bf16)
        hipLaunchKernelGGL(timepool_max_bwd_dx_kernel, dim3(B, ceil_div(L, TP_RB)), dim3(256), 0, st, dpooled, arg, (const bf16*)w_bf16,
                           (bf16*)dx_bf16, L, P, d.thresh, seed, d.inv_keep, seed_epoch);
    if (dw || dbias)
        hipLaunchKernelGGL(timepool_max_bwd_dw_kernel, dim3(P), dim3(TP_K), 0, st, dpooled, arg, (const bf16*)x_bf16, dw,
                           dbias, B, L, P, d.thresh, seed, d.inv_keep, seed_epoch);
    return mm_check_launch("timepool_max_bwd");
}

int mm_timepool_avg_fwd(const float* x_f32, const float* w, const float* bias, float* xbin, float* pooled, int B, int L,
                        int K, int P, int bins, hipStream_t st) {
    MM_REQUIRE(x_f32 && w && xbin && pooled, "timepool_avg_fwd: null");
    if (int rc = tp_sizes("timepool_avg_fwd", B, L, K, P)) return rc;
    if (bins < 1 || bins > TP_BINS_MAX) return mm_fail(MM_ERR_UNSUPPORTED, "timepool_avg_fwd: bins=%d (1 .. %d)", bins, TP_BINS_MAX);
    hipLaunchKernelGGL(timepool_avg_fwd_kernel, dim3(B, bins), dim3(256), 0, st, x_f32, w, bias, xbin, pooled, L, P, bins);
    return mm_check_launch("timepool_avg_fwd");
}

int mm_timepool_avg_bwd(const float* dpooled, const float* xbin, const float* w, float* dx_f32, float* dw, float* dbias,
                        int B, int L, int K, int P, int bins, hipStream_t st) {
    MM_REQUIRE(dpooled && xbin && w, "timepool_avg_bwd: null");
    if (int rc = tp_sizes("timepool_avg_bwd", B, L, K, P)) return rc;
    if (bins < 1 || bins > TP_BINS_MAX) return mm_fail(MM_ERR_UNSUPPORTED, "timepool_avg_bwd: bins=%d (1 .. %d)", bins, TP_BINS_MAX);
    if (dx_f32)
        hipLaunchKernelGGL(timepool_avg_bwd_dx_kernel, dim3(B, ceil_div(L, TP_RB)), dim3(256), 0, st, dpooled, w, dx_f32, L, P, bins);
    if (dw || dbias)
        hipLaunchKernelGGL(timepool_avg_bwd_dw_kernel, dim3(P), dim3(TP_K), 0, st, dpooled, xbin, dw, dbias, B, P, bins);
    return mm_check_launch("timepool_avg_bwd");
}
}  // extern "C"
