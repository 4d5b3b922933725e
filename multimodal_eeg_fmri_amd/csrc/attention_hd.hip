// Multi-head self-attention for every head_dim dh that is a multiple of 8 in [16, 64], on bf16 MFMA, fp32 softmax.
//
// The kernels of attention.hip (same layouts, same products, same dropout hash and mask semantics - read its header
// comment first), templated on a PADDED head width DHP in {32, 64} with the runtime head_dim dh <= DHP:
//   * Q / K / V / dO columns dh .. DHP-1 are zero in registers and LDS: they add nothing to S = Q K^T or dP = dO V^T,
//     and the rows dh .. DHP-1 of the transposed outputs (O^T, dQ^T, dK^T, dV^T) are computed but never stored;
//   * every row starts on a 16-byte boundary (E = H * dh and h * dh are multiples of 8 elements), and a 16-byte column
//     group is either wholly inside dh or wholly outside it;
//   * S / dP take DHP / 16 MFMAs of 32x32x16 per 32-key tile; the transposed outputs are DHP / 32 accumulator tiles;
//   * the tiles read transposed (ds_read_b64_tr_b16, tr_frag32) are stored as DHP / 32 column blocks of [rows][32], so
//     that every block keeps the 64-byte, bank-conflict-free row stride of attention.hip.
// dh = 16 and 24 run the DHP = 32 kernels (a 16-wide S product would halve one MFMA of three per tile; the softmax,
// which is the same work at every dh, dominates).  head_dim 32 through this file computes what attention.hip computes;
// the default model keeps calling attention.hip (mm_attn_fwd / mm_attn_bwd).
#include "attention_common.h"

namespace {

constexpr int KCH = 128;                 // keys staged per chunk (forward, dq)
constexpr int QCH = 128;                 // queries staged per chunk (dkv)

template <int DHP>
struct Hd {
    static_assert(DHP == 32 || DHP == 64, "padded head width");
    static constexpr int NS = DHP / 16;  // 16-deep reduction steps of S / dP over the head dim
    static constexpr int NT = DHP / 32;  // 32-row tiles of the transposed outputs (and column blocks of the tr tiles)
    static constexpr int KS = DHP + 8;   // row stride (elements) of the row-major LDS tiles (+16 B pad)
    static constexpr int NG = DHP / 8;   // 16-byte column groups per row
    // LDS offset of row `row`, column group `sg` in a transposed tile of `rows` rows ([NT][rows][VR])
    static __device__ __forceinline__ int tr_off(int rows, int row, int sg) { return (sg >> 2) * rows * VR + row * VR + (sg & 3) * 8; }
};

__device__ __forceinline__ void zero8(bf16x8& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
}

template <int DHP, bool DROP, bool FULL, bool MASK>
__global__ __launch_bounds__(256) void attn_hd_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out,
                                                          float* __restrict__ lse, int L, int H, int dh, float scale_log2,
                                                          uint32_t dthresh, uint32_t dseed, float dinv,
                                                          const uint32_t* epoch, const float* __restrict__ amask, size_t amask_bh) {
    using T = Hd<DHP>;
    constexpr int NS = T::NS, NT = T::NT, KS = T::KS, NG = T::NG;
    dseed = mm_eff_seed(dseed, epoch);
    if (MASK) amask += (size_t)(blockIdx.z * H + blockIdx.y) * amask_bh;
    __shared__ __attribute__((aligned(16))) bf16 Ks[KCH * KS];
    __shared__ __attribute__((aligned(16))) bf16 Vs[NT * KCH * VR];      // V, row = vperm(key), NT column blocks
    const int E = H * dh, E3 = 3 * E;
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const bf16* base = qkv + (size_t)b * L * E3 + h * dh;

    bf16x8 qf[NS];                                       // Q^T fragments (B operand): lane holds Q[q][16s + 8*lh .. +8]
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        zero8(qf[s]);
        if (q < L && 16 * s + 8 * lh < dh) qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)q * E3 + 16 * s + 8 * lh);
    }
    f32x16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    constexpr int NI = KCH * NG / 256;
    uint4 kreg[NI], vreg[NI];
    auto load_chunk = [&](int k0) __attribute__((always_inline)) {
        const int kn = min(KCH, L - k0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = tid + i * 256, key = s / NG, sg = s % NG;
            kreg[i] = make_uint4(0, 0, 0, 0); vreg[i] = make_uint4(0, 0, 0, 0);
            if (key < kn && sg * 8 < dh) {
                const bf16* row = base + (size_t)(k0 + key) * E3;
                kreg[i] = *reinterpret_cast<const uint4*>(row + E + sg * 8);
                vreg[i] = *reinterpret_cast<const uint4*>(row + 2 * E + sg * 8);
            }
        }
    };
    load_chunk(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : : "v"(qf[s]));      // (attention.hip: no wait inside the tile loop)
    for (int k0 = 0; k0 < L; k0 += KCH) {
        const int kn = min(KCH, L - k0);
        const int kn32 = (kn + 31) & ~31;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = tid + i * 256, key = s / NG, sg = s % NG;
            if (key >= kn32) continue;
            *reinterpret_cast<uint4*>(Ks + key * KS + sg * 8) = kreg[i];
            *reinterpret_cast<uint4*>(Vs + T::tr_off(KCH, vperm(key), sg)) = vreg[i];
        }
        __syncthreads();
        if (k0 + KCH < L) load_chunk(k0 + KCH);
        bf16x8 kfr[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) kfr[s] = *reinterpret_cast<const bf16x8*>(Ks + lr * KS + 16 * s + 8 * lh);
        for (int kt = 0; kt < kn32; kt += 32) {
            f32x16 sacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[s], qf[s], sacc, 0, 0, 0);
            bf16x8 vfr[NT][2];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) vfr[t][s] = tr_frag32(Vs + t * KCH * VR, kt + 16 * s, lane);
            if (kt + 32 < kn32)
#pragma unroll
                for (int s = 0; s < NS; ++s) kfr[s] = *reinterpret_cast<const bf16x8*>(Ks + (kt + 32 + lr) * KS + 16 * s + 8 * lh);
            const float sc2 = MASK ? 1.f : scale_log2;
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                float sc = sacc[r];
                if (MASK) {
                    sc *= scale_log2;
                    if (key < kn) sc += amask[(size_t)min(q, L - 1) * L + k0 + key] * 1.4426950408889634f;
                }
                sacc[r] = (FULL || key < kn) ? sc : -INFINITY;
                mx = fmaxf(mx, sacc[r]);
            }
            mx = xhalf_max(mx);
            if (__builtin_amdgcn_ballot_w64(mx * sc2 > m_run + 8.f)) {      // lazy running maximum, as in attention.hip
                const float m_new = fmaxf(m_run, mx * sc2);
                const float alpha = fast_exp2(m_run - ((MASK && m_new == -INFINITY) ? 0.f : m_new));
                l_run *= alpha;
                m_run = m_new;
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
            }
            const float m_neg = (MASK && m_run == -INFINITY) ? 0.f : -m_run;
            float ps = 0.f;
            union { bf16x8 v[2]; bf16x2 h[8]; } pu;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                float p0 = fast_exp2(fmaf(sacc[r], sc2, m_neg)), p1 = fast_exp2(fmaf(sacc[r + 1], sc2, m_neg));
                ps += p0;
                ps += p1;
                if (DROP) {
                    bool kp0, kp1;
                    attn_keep2<true>(dseed, b * H + h, q, k0 + kt + (r & 3) + 8 * (r >> 2) + 4 * lh, L, dthresh, kp0, kp1);
                    p0 = kp0 ? p0 : 0.f; p1 = kp1 ? p1 : 0.f;
                }
                typedef __attribute__((ext_vector_type(2))) float f32x2_t;
                pu.h[r >> 1] = __builtin_convertvector((f32x2_t){p0, p1}, bf16x2);
            }
            l_run += ps;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[t][s], pu.v[s], o[t], 0, 0, 0);
        }
    }
    const float l_tot = xhalf_sum(l_run);
    const float inv = (DROP ? dinv : 1.f) / l_tot;
    if (q < L) {
        bf16* orow = out + ((size_t)b * L + q) * E + h * dh;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {                   // rows d = 32t + 8g + 4*lh + {0..3}
                const int d = 32 * t + 8 * g + 4 * lh;
                if (d >= dh) continue;
                bf16x4 v = {(bf16)(o[t][4 * g] * inv), (bf16)(o[t][4 * g + 1] * inv), (bf16)(o[t][4 * g + 2] * inv), (bf16)(o[t][4 * g + 3] * inv)};
                *reinterpret_cast<bf16x4*>(orow + d) = v;
            }
        if (lse && lh == 0) lse[((size_t)b * H + h) * L + q] = (m_run + log2f(l_tot)) * 0.6931471805599453f;
    }
}

// Backward: the two passes of attention.hip (dq kernel also writes delta; dkv kernel sweeps the queries), no atomics.
template <int DHP, bool DROP, bool FULL, bool MASK>
__global__ __launch_bounds__(256) void attn_hd_bwd_dq_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ out,
                                                             const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                             bf16* __restrict__ dqkv, float* __restrict__ delta,
                                                             int L, int H, int dh, float scale, uint32_t dthresh,
                                                             uint32_t dseed, float dinv, const uint32_t* epoch,
                                                             const float* __restrict__ amask, size_t amask_bh) {
    using T = Hd<DHP>;
    constexpr int NS = T::NS, NT = T::NT, KS = T::KS, NG = T::NG;
    dseed = mm_eff_seed(dseed, epoch);
    if (MASK) amask += (size_t)(blockIdx.z * H + blockIdx.y) * amask_bh;
    __shared__ __attribute__((aligned(16))) bf16 Ks[KCH * KS];
    __shared__ __attribute__((aligned(16))) bf16 Vs[KCH * KS];
    __shared__ __attribute__((aligned(16))) bf16 Kr[NT * KCH * VR];      // K again, row = vperm(key), NT column blocks
    const int E = H * dh, E3 = 3 * E;
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int q = blockIdx.x * 128 + wave * 32 + lr;
    const bool qok = q < L;
    const bf16* base = qkv + (size_t)b * L * E3 + h * dh;
    const float scale_log2 = scale * 1.4426950408889634f;

    bf16x8 qf[NS], dof[NS];
    float dl = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        zero8(qf[s]); zero8(dof[s]);
        if (qok && 16 * s + 8 * lh < dh) {
            qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)q * E3 + 16 * s + 8 * lh);
            const size_t oi = ((size_t)b * L + q) * E + h * dh + 16 * s + 8 * lh;
            dof[s] = *reinterpret_cast<const bf16x8*>(dout + oi);
            const bf16x8 of = *reinterpret_cast<const bf16x8*>(out + oi);
#pragma unroll
            for (int j = 0; j < 8; ++j) dl += (float)dof[s][j] * (float)of[j];
        }
    }
    dl = xhalf_sum(dl);
    const float lse2 = qok ? lse[((size_t)b * H + h) * L + q] * 1.4426950408889634f : 0.f;
    if (qok && lh == 0) delta[((size_t)b * H + h) * L + q] = dl;

    f32x16 dq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[t][r] = 0.f;

    constexpr int NI = KCH * NG / 256;
    uint4 kreg[NI], vreg[NI];
    auto load_chunk = [&](int k0) __attribute__((always_inline)) {
        const int kn = min(KCH, L - k0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = tid + i * 256, key = s / NG, sg = s % NG;
            kreg[i] = make_uint4(0, 0, 0, 0); vreg[i] = make_uint4(0, 0, 0, 0);
            if (key < kn && sg * 8 < dh) {
                const bf16* row = base + (size_t)(k0 + key) * E3;
                kreg[i] = *reinterpret_cast<const uint4*>(row + E + sg * 8);
                vreg[i] = *reinterpret_cast<const uint4*>(row + 2 * E + sg * 8);
            }
        }
    };
    load_chunk(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : : "v"(qf[s]), "v"(dof[s]));
    asm volatile("" : : "v"(dl), "v"(lse2));
    for (int k0 = 0; k0 < L; k0 += KCH) {
        const int kn = min(KCH, L - k0);
        const int kn32 = (kn + 31) & ~31;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = tid + i * 256, key = s / NG, sg = s % NG;
            if (key >= kn32) continue;
            *reinterpret_cast<uint4*>(Ks + key * KS + sg * 8) = kreg[i];
            *reinterpret_cast<uint4*>(Vs + key * KS + sg * 8) = vreg[i];
            *reinterpret_cast<uint4*>(Kr + T::tr_off(KCH, vperm(key), sg)) = kreg[i];
        }
        __syncthreads();
        if (k0 + KCH < L) load_chunk(k0 + KCH);
        for (int kt = 0; kt < kn32; kt += 32) {
            f32x16 sacc, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
            bf16x8 kfr[NS], vfr[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                kfr[s] = *reinterpret_cast<const bf16x8*>(Ks + (kt + lr) * KS + 16 * s + 8 * lh);
                vfr[s] = *reinterpret_cast<const bf16x8*>(Vs + (kt + lr) * KS + 16 * s + 8 * lh);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[s], qf[s], sacc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[s], dof[s], dp, 0, 0, 0);
            }
            bf16x8 ktfr[NT][2];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) ktfr[t][s] = tr_frag32(Kr + t * KCH * VR, kt + 16 * s, lane);
            bf16x8 dsf[2];
            bool kp[16];
            if (DROP)
#pragma unroll
                for (int r = 0; r < 16; r += 2)
                    attn_keep2<true>(dseed, b * H + h, q, k0 + kt + (r & 3) + 8 * (r >> 2) + 4 * lh, L, dthresh, kp[r], kp[r + 1]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                float sc = fmaf(sacc[r], scale_log2, -lse2);
                if (MASK && key < kn) sc += amask[(size_t)min(q, L - 1) * L + k0 + key] * 1.4426950408889634f;
                const float p = (FULL || key < kn) ? fast_exp2(sc) : 0.f;
                float dpr = dp[r];
                if (DROP) dpr = fmaf(kp[r] ? dpr : 0.f, dinv, -dl);
                else dpr -= dl;
                dsf[r >> 3][r & 7] = (bf16)(p * dpr);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) dq[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktfr[t][s], dsf[s], dq[t], 0, 0, 0);
        }
    }
    if (qok) {
        bf16* drow = dqkv + ((size_t)b * L + q) * E3 + h * dh;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * t + 8 * g + 4 * lh;
                if (d >= dh) continue;
                bf16x4 v = {(bf16)(dq[t][4 * g] * scale), (bf16)(dq[t][4 * g + 1] * scale), (bf16)(dq[t][4 * g + 2] * scale), (bf16)(dq[t][4 * g + 3] * scale)};
                *reinterpret_cast<bf16x4*>(drow + d) = v;
            }
    }
}

template <int DHP, bool DROP, bool FULL, bool MASK>
__global__ __launch_bounds__(256) void attn_hd_bwd_dkv_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                              bf16* __restrict__ dqkv, int L, int H, int dh, float scale,
                                                              uint32_t dthresh, uint32_t dseed, float dinv,
                                                              const uint32_t* epoch, const float* __restrict__ amask, size_t amask_bh) {
    using T = Hd<DHP>;
    constexpr int NS = T::NS, NT = T::NT, KS = T::KS, NG = T::NG;
    dseed = mm_eff_seed(dseed, epoch);
    if (MASK) amask += (size_t)(blockIdx.z * H + blockIdx.y) * amask_bh;
    __shared__ __attribute__((aligned(16))) bf16 Qs[QCH * KS];
    __shared__ __attribute__((aligned(16))) bf16 Ds[QCH * KS];
    __shared__ __attribute__((aligned(16))) bf16 Qr[NT * QCH * VR];      // Q and dO again, row = vperm(query), NT column
    __shared__ __attribute__((aligned(16))) bf16 Dr[NT * QCH * VR];      // blocks, for the transposed products
    __shared__ float Ls[QCH], Dl[QCH];
    const int E = H * dh, E3 = 3 * E;
    const int b = blockIdx.z, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int key = blockIdx.x * 128 + wave * 32 + lr;
    const bool kok = key < L;
    const bf16* base = qkv + (size_t)b * L * E3 + h * dh;
    const float scale_log2 = scale * 1.4426950408889634f;

    bf16x8 kf[NS], vf[NS];                               // K^T / V^T fragments as B operands
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        zero8(kf[s]); zero8(vf[s]);
        if (kok && 16 * s + 8 * lh < dh) {
            kf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)key * E3 + E + 16 * s + 8 * lh);
            vf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)key * E3 + 2 * E + 16 * s + 8 * lh);
        }
    }
    f32x16 dk[NT], dv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[t][r] = 0.f; dv[t][r] = 0.f; }

    constexpr int NI = QCH * NG / 256;
    static_assert(QCH <= 256, "one lse / delta value per thread");
    uint4 qreg[NI], dreg[NI];
    float lreg = INFINITY, dlreg = 0.f;
    auto load_chunk = [&](int q0) __attribute__((always_inline)) {
        const int qn = min(QCH, L - q0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = tid + i * 256, qi = s / NG, sg = s % NG;
            qreg[i] = make_uint4(0, 0, 0, 0); dreg[i] = make_uint4(0, 0, 0, 0);
            if (qi < qn && sg * 8 < dh) {
                qreg[i] = *reinterpret_cast<const uint4*>(base + (size_t)(q0 + qi) * E3 + sg * 8);
                dreg[i] = *reinterpret_cast<const uint4*>(dout + ((size_t)b * L + q0 + qi) * E + h * dh + sg * 8);
            }
        }
        const bool ok = tid < qn;
        lreg = ok ? lse[((size_t)b * H + h) * L + q0 + tid] : INFINITY;
        dlreg = ok ? delta[((size_t)b * H + h) * L + q0 + tid] : 0.f;
    };
    load_chunk(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("" : : "v"(kf[s]), "v"(vf[s]));
    for (int q0 = 0; q0 < L; q0 += QCH) {
        const int qn = min(QCH, L - q0);
        const int qn32 = (qn + 31) & ~31;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int s = tid + i * 256, qi = s / NG, sg = s % NG;
            if (qi >= qn32) continue;
            *reinterpret_cast<uint4*>(Qs + qi * KS + sg * 8) = qreg[i];
            *reinterpret_cast<uint4*>(Ds + qi * KS + sg * 8) = dreg[i];
            *reinterpret_cast<uint4*>(Qr + T::tr_off(QCH, vperm(qi), sg)) = qreg[i];
            *reinterpret_cast<uint4*>(Dr + T::tr_off(QCH, vperm(qi), sg)) = dreg[i];
        }
        if (tid < qn32) { Ls[tid] = lreg * 1.4426950408889634f; Dl[tid] = dlreg; }
        __syncthreads();
        if (q0 + QCH < L) load_chunk(q0 + QCH);
        for (int qt = 0; qt < qn32; qt += 32) {
            f32x16 sacc, dp;                             // S[q][key], dP[q][key]: rows = q (registers), column = this lane's key
#pragma unroll
            for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
            bf16x8 qar[NS], dar[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                qar[s] = *reinterpret_cast<const bf16x8*>(Qs + (qt + lr) * KS + 16 * s + 8 * lh);
                dar[s] = *reinterpret_cast<const bf16x8*>(Ds + (qt + lr) * KS + 16 * s + 8 * lh);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qar[s], kf[s], sacc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dar[s], vf[s], dp, 0, 0, 0);
            }
            bf16x8 dtar[NT][2], qtar[NT][2];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    dtar[t][s] = tr_frag32(Dr + t * QCH * VR, qt + 16 * s, lane);
                    qtar[t][s] = tr_frag32(Qr + t * QCH * VR, qt + 16 * s, lane);
                }
            bf16x8 pf[2], dsf[2];
            bool kp[16];
            if (DROP)
#pragma unroll
                for (int r = 0; r < 16; r += 2)
                    attn_keep2<false>(dseed, b * H + h, key, q0 + qt + (r & 3) + 8 * (r >> 2) + 4 * lh, L, dthresh, kp[r], kp[r + 1]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = qt + (r & 3) + 8 * (r >> 2) + 4 * lh;
                float sc = fmaf(sacc[r], scale_log2, -Ls[qi]);
                if (MASK && kok && qi < qn) sc += amask[(size_t)(q0 + qi) * L + key] * 1.4426950408889634f;
                const float p = (FULL || kok) ? fast_exp2(sc) : 0.f;
                pf[r >> 3][r & 7] = (bf16)((!DROP || kp[r]) ? p : 0.f);
                const float u = DROP ? fmaf(kp[r] ? dp[r] : 0.f, dinv, -Dl[qi]) : dp[r] - Dl[qi];
                dsf[r >> 3][r & 7] = (bf16)(p * u);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dtar[t][s], pf[s], dv[t], 0, 0, 0);
                    dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtar[t][s], dsf[s], dk[t], 0, 0, 0);
                }
        }
    }
    if (kok) {
        bf16* krow = dqkv + ((size_t)b * L + key) * E3 + E + h * dh;
        bf16* vrow = krow + E;
        const float dvs = DROP ? dinv : 1.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * t + 8 * g + 4 * lh;
                if (d >= dh) continue;
                bf16x4 a = {(bf16)(dk[t][4 * g] * scale), (bf16)(dk[t][4 * g + 1] * scale), (bf16)(dk[t][4 * g + 2] * scale), (bf16)(dk[t][4 * g + 3] * scale)};
                bf16x4 c = {(bf16)(dv[t][4 * g] * dvs), (bf16)(dv[t][4 * g + 1] * dvs), (bf16)(dv[t][4 * g + 2] * dvs), (bf16)(dv[t][4 * g + 3] * dvs)};
                *reinterpret_cast<bf16x4*>(krow + d) = a;
                *reinterpret_cast<bf16x4*>(vrow + d) = c;
            }
    }
}

bool hd_supported(int dh) { return dh >= 16 && dh <= 64 && dh % 8 == 0; }

template <int DHP>
void launch_fwd(const void* qkv, void* out, float* lse, int B, int L, int H, int dh, float scale, uint32_t dth,
                uint32_t seed, const uint32_t* seed_epoch, const float* attn_mask, size_t mask_bh, hipStream_t st) {
    const bool full = L % KCH == 0;
    auto kern = dth ? (full ? attn_hd_fwd_kernel<DHP, true, true, false> : attn_hd_fwd_kernel<DHP, true, false, false>)
                    : (full ? attn_hd_fwd_kernel<DHP, false, true, false> : attn_hd_fwd_kernel<DHP, false, false, false>);
    if (attn_mask) kern = dth ? attn_hd_fwd_kernel<DHP, true, false, true> : attn_hd_fwd_kernel<DHP, false, false, true>;
    hipLaunchKernelGGL(kern, dim3(ceil_div(L, 128), H, B), dim3(256), 0, st, (const bf16*)qkv, (bf16*)out, lse, L, H, dh,
                       scale * 1.4426950408889634f, dth, seed, attn_keep_scale(dth), seed_epoch, attn_mask, mask_bh);
}

template <int DHP>
int launch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
               int B, int L, int H, int dh, float scale, uint32_t dth, uint32_t seed, const uint32_t* seed_epoch,
               const float* attn_mask, size_t mask_bh, hipStream_t st) {
    const float dinv = attn_keep_scale(dth);
    const bool full = L % KCH == 0 && L % QCH == 0;
    auto kdq = dth ? (full ? attn_hd_bwd_dq_kernel<DHP, true, true, false> : attn_hd_bwd_dq_kernel<DHP, true, false, false>)
                   : (full ? attn_hd_bwd_dq_kernel<DHP, false, true, false> : attn_hd_bwd_dq_kernel<DHP, false, false, false>);
    auto kdkv = dth ? (full ? attn_hd_bwd_dkv_kernel<DHP, true, true, false> : attn_hd_bwd_dkv_kernel<DHP, true, false, false>)
                    : (full ? attn_hd_bwd_dkv_kernel<DHP, false, true, false> : attn_hd_bwd_dkv_kernel<DHP, false, false, false>);
    if (attn_mask) {
        kdq = dth ? attn_hd_bwd_dq_kernel<DHP, true, false, true> : attn_hd_bwd_dq_kernel<DHP, false, false, true>;
        kdkv = dth ? attn_hd_bwd_dkv_kernel<DHP, true, false, true> : attn_hd_bwd_dkv_kernel<DHP, false, false, true>;
    }
    const dim3 grid(ceil_div(L, 128), H, B);
    hipLaunchKernelGGL(kdq, grid, dim3(256), 0, st, (const bf16*)qkv, (const bf16*)out, (const bf16*)dout, lse,
                       (bf16*)dqkv, delta_ws, L, H, dh, scale, dth, seed, dinv, seed_epoch, attn_mask, mask_bh);
    int rc = mm_check_launch("attn_bwd_hd_dq");
    if (rc) return rc;
    hipLaunchKernelGGL(kdkv, grid, dim3(256), 0, st, (const bf16*)qkv, (const bf16*)dout, lse, delta_ws, (bf16*)dqkv,
                       L, H, dh, scale, dth, seed, dinv, seed_epoch, attn_mask, mask_bh);
    return mm_check_launch("attn_bwd_hd_dkv");
}

}  // namespace

extern "C" {

int mm_attn_fwd_hd(const void* qkv, void* out, float* lse, int B, int L, int H, int head_dim, float scale,
                   float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* attn_mask, int attn_mask_per_head,
                   hipStream_t st) {
    MM_REQUIRE(hd_supported(head_dim), "attn_fwd_hd: head_dim=%d (supported: multiples of 8 in [16, 64])", head_dim);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "attn_fwd_hd: drop_p");
    MM_REQUIRE(qkv && out && B > 0 && L > 0 && H > 0, "attn_fwd_hd: null/invalid");
    const size_t mask_bh = attn_mask && attn_mask_per_head ? (size_t)L * L : 0;
    const uint32_t dth = attn_thresh(drop_p);
    if (head_dim <= 32) launch_fwd<32>(qkv, out, lse, B, L, H, head_dim, scale, dth, seed, seed_epoch, attn_mask, mask_bh, st);
    else launch_fwd<64>(qkv, out, lse, B, L, H, head_dim, scale, dth, seed, seed_epoch, attn_mask, mask_bh, st);
    return mm_check_launch("attn_fwd_hd");
}

int mm_attn_bwd_hd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, float* delta_ws,
                   int B, int L, int H, int head_dim, float scale, float drop_p, uint32_t seed,
                   const uint32_t* seed_epoch, const float* attn_mask, int attn_mask_per_head, hipStream_t st) {
    MM_REQUIRE(hd_supported(head_dim), "attn_bwd_hd: head_dim=%d (supported: multiples of 8 in [16, 64])", head_dim);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "attn_bwd_hd: drop_p");
    MM_REQUIRE(qkv && out && dout && lse && dqkv && delta_ws && B > 0 && L > 0 && H > 0, "attn_bwd_hd: null/invalid");
    const size_t mask_bh = attn_mask && attn_mask_per_head ? (size_t)L * L : 0;
    const uint32_t dth = attn_thresh(drop_p);
    if (head_dim <= 32)
        return launch_bwd<32>(qkv, out, dout, lse, dqkv, delta_ws, B, L, H, head_dim, scale, dth, seed, seed_epoch, attn_mask, mask_bh, st);
    return launch_bwd<64>(qkv, out, dout, lse, dqkv, delta_ws, B, L, H, head_dim, scale, dth, seed, seed_epoch, attn_mask, mask_bh, st);
}

}  // extern "C"
