// Read-out of the self-attention probabilities of csrc/attention.hip (eval mode: no dropout), from what a saving
// forward keeps: the packed projections and the log-sum-exp of every query row.
//
// qkv : [B][L][3E] bf16 (q | k | v, head h owns columns h*dh .. h*dh+dh-1 of each E-wide third), E = H*dh
// lse : [B][H][L]  fp32, natural log (mm_attn_fwd / mm_attn_fwd_hd)
//     P[b][h][i][j] = exp(scale * q_i . k_j + mask[i][j] - lse[b][h][i])
//
//   mm_attn_weights  : w   = P per head, (B, H, L, L), or its mean over the heads, (B, L, L)
//   mm_attn_received : out[b][j] = sw * r[b][j] + (1 - sw) * sum_i r[b][i] * (1/H) sum_h P[b][h][i][j]   - no score
//                      matrix is stored; sw = 0.5 is one step of attention rollout taken as a row-vector product
//
// Orientation (that of attn_bwd_dkv_kernel): a lane owns a KEY, its 16 accumulator registers run along the QUERIES,
//     S[q][key] = Q_tile . K^T          (A = Q rows from LDS, B = K^T from registers)
// so a store of `w` is 32 consecutive floats of one query row per half wave, the sum over the queries is 16 in-register
// adds per tile plus ONE exchange with lane ^ 32 at the very end, and lse / r are per-query scalars read from LDS
// (one address per half wave: a broadcast).  One workgroup = 4 waves = 128 keys; queries are staged in chunks of 128 rows,
// row stride DHP + 8 elements as in attention.hip (the A-fragment reads are its dkv kernel's).
//
// Head dims as attention.hip: multiples of 8 in [16, 64] on a padded width DHP in {32, 64}; columns dh .. DHP-1 are zero
// in registers and LDS.  Nothing here adds across workgroups with atomics: every sum has a fixed order, two calls on the
// same inputs give the same bits.  A fully masked row has lse = -inf (or NaN) and gives NaN, as in the forward: in `w`
// the NaN stays in that row, in `out` it reaches every column of that batch element (every key sums over that query).
#include <limits.h>

#include "common.h"

namespace {

constexpr int QCH = 128;                 // queries staged per chunk
constexpr int KTILE = 128;               // keys per workgroup (32 per wave)
constexpr float LOG2E = 1.4426950408889634f;

template <int DHP>
struct Hd {
    static_assert(DHP == 32 || DHP == 64, "padded head width");
    static constexpr int NS = DHP / 16;  // 16-deep reduction steps of S over the head dim
    static constexpr int KS = DHP + 8;   // row stride (elements) of the row-major LDS tile (+16 B pad)
    static constexpr int NG = DHP / 8;   // 16-byte column groups per row
};

__device__ __forceinline__ void zero8(bf16x8& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
}
// v_exp_f32 as is (attention.hip): a result below 2^-126 may flush to zero
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// rows q0 .. q0 + 127 of head h's Q (zero beyond L and beyond dh) -> Qs; their lse in log2 units -> Ls (+inf beyond L:
// such a row's probabilities are exp2(-inf) = 0); their row weight -> Rs (0 beyond L) when asked for
template <int DHP>
__device__ __forceinline__ void stage_queries(const bf16* __restrict__ qbase, const float* __restrict__ lse_bh,
                                              const float* __restrict__ rw_b, float r_const, bool want_r, bf16* Qs, float* Ls,
                                              float* Rs, int q0, int L, int E3, int dh, int tid) {
    using T = Hd<DHP>;
    const int qn = min(QCH, L - q0);
#pragma unroll
    for (int i = 0; i < QCH * T::NG / 256; ++i) {
        const int s = tid + i * 256, qi = s / T::NG, sg = s % T::NG;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (qi < qn && sg * 8 < dh) v = *reinterpret_cast<const uint4*>(qbase + (size_t)(q0 + qi) * E3 + sg * 8);
        *reinterpret_cast<uint4*>(Qs + qi * T::KS + sg * 8) = v;
    }
    if (tid < QCH) {
        const bool ok = tid < qn;
        Ls[tid] = ok ? lse_bh[q0 + tid] * LOG2E : INFINITY;
        if (want_r) Rs[tid] = ok ? (rw_b ? rw_b[q0 + tid] : r_const) : 0.f;
    }
}

// the 32 x 32 probability tile of queries qt .. qt + 31 of the staged chunk against this lane's key: register r is query
// qt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  amask_q0: the mask row of the chunk's first query at this lane's key column.
template <int DHP, bool MASK>
__device__ __forceinline__ void prob_tile(const bf16* Qs, const float* Ls, const bf16x8* kf, int qt, int qn, bool kok,
                                          float scale_log2, const float* __restrict__ amask_q0, int L, int lr, int lh,
                                          f32x16& p) {
    using T = Hd<DHP>;
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
    bf16x8 qar[T::NS];
#pragma unroll
    for (int s = 0; s < T::NS; ++s) qar[s] = *reinterpret_cast<const bf16x8*>(Qs + (qt + lr) * T::KS + 16 * s + 8 * lh);
#pragma unroll
    for (int s = 0; s < T::NS; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qar[s], kf[s], sacc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qi = qt + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float sc = fmaf(sacc[r], scale_log2, -Ls[qi]);
        if (MASK && kok && qi < qn) sc += amask_q0[(size_t)qi * L] * LOG2E;
        p[r] = fast_exp2(sc);
    }
}

template <int DHP>
__device__ __forceinline__ void load_key(const bf16* __restrict__ kbase, int key, bool kok, int E3, int dh, int lh, bf16x8* kf) {
#pragma unroll
    for (int s = 0; s < Hd<DHP>::NS; ++s) {
        zero8(kf[s]);
        if (kok && 16 * s + 8 * lh < dh) kf[s] = *reinterpret_cast<const bf16x8*>(kbase + (size_t)key * E3 + 16 * s + 8 * lh);
    }
}

// grid (key tiles, query chunks [x H when per_head], B).  The head mean is formed inside the workgroup, heads in the order
// 0 .. H-1; every element of `w` is written once.
template <int DHP, bool MASK>
__global__ __launch_bounds__(256) void attn_weights_kernel(const bf16* __restrict__ qkv, const float* __restrict__ lse,
                                                           float* __restrict__ w, int L, int H, int dh, float scale_log2,
                                                           const float* __restrict__ amask, size_t amask_bh, int per_head) {
    using T = Hd<DHP>;
    __shared__ __attribute__((aligned(16))) bf16 Qs[QCH * T::KS];
    __shared__ float Ls[QCH];
    const int E = H * dh, E3 = 3 * E;
    const int nqc = (L + QCH - 1) / QCH;
    const int b = blockIdx.z, qc = blockIdx.y % nqc, hsel = blockIdx.y / nqc;
    const int h0 = per_head ? hsel : 0, h1 = per_head ? hsel + 1 : H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int key = blockIdx.x * KTILE + wave * 32 + lr;
    const bool kok = key < L;
    const int q0 = qc * QCH, qn = min(QCH, L - q0);

    f32x16 acc[QCH / 32];
#pragma unroll
    for (int t = 0; t < QCH / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int h = h0; h < h1; ++h) {
        const bf16* base = qkv + (size_t)b * L * E3 + h * dh;
        bf16x8 kf[T::NS];
        load_key<DHP>(base + E, key, kok, E3, dh, lh, kf);
        __syncthreads();                                  // the previous head's tiles were read
        stage_queries<DHP>(base, lse + ((size_t)b * H + h) * L, nullptr, 0.f, false, Qs, Ls, nullptr, q0, L, E3, dh, tid);
        __syncthreads();
        const float* am = MASK ? amask + (size_t)(b * H + h) * amask_bh + (size_t)q0 * L + (kok ? key : 0) : nullptr;
#pragma unroll
        for (int t = 0; t < QCH / 32; ++t) {
            if (32 * t >= qn) continue;                   // (workgroup-uniform)
            f32x16 p;
            prob_tile<DHP, MASK>(Qs, Ls, kf, 32 * t, qn, kok, scale_log2, am, L, lr, lh, p);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] += p[r];
        }
    }
    if (!kok) return;
    const float inv = per_head ? 1.f : 1.f / (float)H;
    float* wb = w + (per_head ? ((size_t)b * H + h0) : (size_t)b) * L * L;
#pragma unroll
    for (int t = 0; t < QCH / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qi = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (qi < qn) wb[(size_t)(q0 + qi) * L + key] = acc[t][r] * inv;
        }
}

// grid (key tiles, H, B): slot[b][h][key] = sum_i r[b][i] P[b][h][i][key], queries in ascending chunks, tiles and
// registers, the two halves of the wave last
template <int DHP, bool MASK>
__global__ __launch_bounds__(256) void attn_received_kernel(const bf16* __restrict__ qkv, const float* __restrict__ lse,
                                                            const float* __restrict__ row_w, float* __restrict__ slots, int L,
                                                            int H, int dh, float scale_log2, const float* __restrict__ amask,
                                                            size_t amask_bh) {
    using T = Hd<DHP>;
    __shared__ __attribute__((aligned(16))) bf16 Qs[QCH * T::KS];
    __shared__ float Ls[QCH], Rs[QCH];
    const int E = H * dh, E3 = 3 * E;
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int key = blockIdx.x * KTILE + wave * 32 + lr;
    const bool kok = key < L;
    const bf16* base = qkv + (size_t)b * L * E3 + h * dh;
    bf16x8 kf[T::NS];
    load_key<DHP>(base + E, key, kok, E3, dh, lh, kf);
    const float* am_bh = MASK ? amask + (size_t)(b * H + h) * amask_bh + (kok ? key : 0) : nullptr;
    const float r_const = 1.f / (float)L;
    float col = 0.f;
    for (int q0 = 0; q0 < L; q0 += QCH) {
        const int qn = min(QCH, L - q0);
        __syncthreads();
        stage_queries<DHP>(base, lse + ((size_t)b * H + h) * L, row_w ? row_w + (size_t)b * L : nullptr, r_const, true, Qs, Ls,
                           Rs, q0, L, E3, dh, tid);
        __syncthreads();
        for (int qt = 0; qt < qn; qt += 32) {
            f32x16 p;
            prob_tile<DHP, MASK>(Qs, Ls, kf, qt, qn, kok, scale_log2, MASK ? am_bh + (size_t)q0 * L : nullptr, L, lr, lh, p);
#pragma unroll
            for (int r = 0; r < 16; ++r) col = fmaf(Rs[qt + (r & 3) + 8 * (r >> 2) + 4 * lh], p[r], col);
        }
    }
    col = xhalf_sum(col);
    if (kok && lh == 0) slots[((size_t)b * H + h) * L + key] = col;
}

// out[b][j] = sw * r[b][j] + (1 - sw) * (1/H) * (slot[b][0][j] + ... + slot[b][H-1][j])
__global__ __launch_bounds__(256) void attn_received_finish_kernel(const float* __restrict__ slots, const float* __restrict__ row_w,
                                                                   float* __restrict__ out, int B, int L, int H, float sw) {
    const size_t n = (size_t)B * L;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t b = i / L, j = i % L;
        float s = 0.f;
        for (int h = 0; h < H; ++h) s += slots[(b * H + h) * L + j];
        const float r = row_w ? row_w[i] : 1.f / (float)L;
        out[i] = sw * r + (1.f - sw) * (s * (1.f / (float)H));
    }
}

bool hd_supported(int dh) { return dh >= 16 && dh <= 64 && dh % 8 == 0; }

// what both entries check alike; the grid's y and z extents are 16-bit
int readout_check(const char* who, const void* qkv, const float* lse, const void* dst, int B, int L, int H, int head_dim) {
    MM_REQUIRE(hd_supported(head_dim), "%s: head_dim=%d (supported: multiples of 8 in [16, 64])", who, head_dim);
    MM_REQUIRE(qkv && lse && dst && B > 0 && L > 0 && H > 0, "%s: null/invalid", who);
    MM_REQUIRE(B <= 65535 && (long long)H * ((L + QCH - 1) / QCH) <= 65535, "%s: B=%d, H=%d, L=%d exceed the launch grid", who, B, H, L);
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_attn_weights(const void* qkv, const float* lse, float* w, int B, int L, int H, int head_dim, float scale,
                    const float* attn_mask, int attn_mask_per_head, int per_head, hipStream_t st) {
    const int rc = readout_check("attn_weights", qkv, lse, w, B, L, H, head_dim);
    if (rc) return rc;
    MM_REQUIRE(per_head == 0 || per_head == 1, "attn_weights: per_head=%d (0 = head mean, 1 = every head)", per_head);
    const size_t mask_bh = attn_mask && attn_mask_per_head ? (size_t)L * L : 0;
    auto kern = head_dim <= 32 ? (attn_mask ? attn_weights_kernel<32, true> : attn_weights_kernel<32, false>)
                               : (attn_mask ? attn_weights_kernel<64, true> : attn_weights_kernel<64, false>);
    const int nqc = ceil_div(L, QCH);
    hipLaunchKernelGGL(kern, dim3(ceil_div(L, KTILE), nqc * (per_head ? H : 1), B), dim3(256), 0, st, (const bf16*)qkv, lse, w,
                       L, H, head_dim, scale * LOG2E, attn_mask, mask_bh, per_head);
    return mm_check_launch("attn_weights");
}

int mm_attn_received_ws_floats(int B, int L, int H, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host, "attn_received_ws_floats: null floats_host");
    MM_REQUIRE(B > 0 && L > 0 && H > 0, "attn_received_ws_floats: invalid B=%d, L=%d, H=%d", B, L, H);
    const long long n = (long long)B * H * L;             // one slot per (batch element, head, key)
    MM_REQUIRE(n <= INT_MAX, "attn_received_ws_floats: workspace of %lld floats overflows int", n);
    *floats_host = (int)n;
    return MM_OK;
}

int mm_attn_received(const void* qkv, const float* lse, const float* row_w, float self_weight, float* out, float* ws,
                     int B, int L, int H, int head_dim, float scale, const float* attn_mask, int attn_mask_per_head,
                     hipStream_t st) {
    int rc = readout_check("attn_received", qkv, lse, out, B, L, H, head_dim);
    if (rc) return rc;
    MM_REQUIRE(ws, "attn_received: null ws (mm_attn_received_ws_floats)");
    MM_REQUIRE(self_weight >= 0.f && self_weight <= 1.f, "attn_received: self_weight outside [0, 1]");
    const size_t mask_bh = attn_mask && attn_mask_per_head ? (size_t)L * L : 0;
    auto kern = head_dim <= 32 ? (attn_mask ? attn_received_kernel<32, true> : attn_received_kernel<32, false>)
                               : (attn_mask ? attn_received_kernel<64, true> : attn_received_kernel<64, false>);
    hipLaunchKernelGGL(kern, dim3(ceil_div(L, KTILE), H, B), dim3(256), 0, st, (const bf16*)qkv, lse, row_w, ws, L, H, head_dim,
                       scale * LOG2E, attn_mask, mask_bh);
    rc = mm_check_launch("attn_received");
    if (rc) return rc;
    hipLaunchKernelGGL(attn_received_finish_kernel, dim3(grid_for((size_t)B * L, 1024)), dim3(256), 0, st, ws, row_w, out, B, L,
                       H, self_weight);
    return mm_check_launch("attn_received_finish");
}

}  // extern "C"
