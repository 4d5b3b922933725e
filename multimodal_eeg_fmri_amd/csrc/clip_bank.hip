// Symmetric InfoNCE of a batch against the batch AND a cross-batch memory of earlier embeddings (Wang et al., "Cross-Batch
// Memory for Embedding Learning"), with its gradients, and the ring push that feeds the memory.  Callers:
// ops.clip_bank_loss, ops.clip_bank_push, ops.clip_bank_ws_floats (bridge_trainer.py's step with bank_size > 0,
// autograd.py's ClipBankLossFn); ops.clip_key_loss, ops.clip_key_ws_floats (the step with key_encoder=True, ClipKeyLossFn).
#include "common.h"

namespace {
// ---------------------------------------------------------------------------
// z [B][2N] = [ze | zf] own rows (queries AND keys); bank [K][2N] = the same rows of earlier steps (keys only, constants);
// state int32 {head, filled, pushes, 0}.  n = pushes >= warmup ? filled : 0 valid bank rows, read ON THE DEVICE: the same
// launch arguments (and the same captured graph) serve every fill level.  Key index t in [0, B + n): t < B is batch row t,
// else bank slot t - B (the ring never wraps before it is full, so slots [0, filled) are the valid ones).
//   e->f: query ze_r over keys zf_t        f->e: query zf_r over keys ze_t         s = exp(logit_scale)
//   P(r) = {t : gid_t = gid_r} (gid NULL: {r}, no bank row is ever a positive)
//   l_dir(r) = LSE_t(s x[r][t]) - LSE_{t in P(r)}(s x[r][t])        loss = 1/B sum_r (l_e2f(r) + l_f2e(r)) / 2
//   G_dir[r][t] = 0.5 s / B (softmax_t - [t in P(r)] softmax over P(r))        (= d loss / d x_dir[r][t])
//   dze_r = sum_{t < B + n} G_e2f[r][t] zf_t + sum_{j < B} G_f2e[j][r] zf_j      (query term + key term; bank rows get nothing)
//   dzf_r = sum_{t < B + n} G_f2e[r][t] ze_t + sum_{j < B} G_e2f[j][r] ze_j
// Two launches, no workgroup waits for or reads anything another workgroup of the same launch writes:
//   bank_scores_kernel (one workgroup per chunk of KC keys and tile of 8 queries; the grid follows the CAPACITY B + K,
//     workgroups whose chunk starts at or past B + n exit): both score blocks of the chunk against its queries -> ws (the
//     rows kernel reads them back instead of recomputing), and per (query, direction) the chunk's partial {max m,
//     sum exp(s (x - m)), the same sum weighted by x - m, and the same three over the positives} -> ws.
//   bank_rows_kernel (grid (B, column slabs of 64)): folds the partials of EVERY query in chunk order (each workgroup
//     for itself: 2 B serial chains with many loads in flight, cheaper than a third launch at the trainer's shapes;
//     profiles/clip_bank_ab.txt), then forms G for its row from the stored scores and its 64 columns of dz; workgroup
//     (0, 0) also sums the rows' scalars in a fixed order -> scal4.
// Scores are plain fp32 FMA chains (8 lanes per key, ascending n within a lane, then a fixed 3-step butterfly), not MFMA:
// 8 queries x 64 keys x N is far too little work per workgroup for the matrix pipe to matter, the launches are bound by
// latency, and no comparison here needs retrieval.hip's bit-exact score (top-1 compares scores of ONE chain with each
// other).  Every sum runs in a fixed order and there are no float atomics: same inputs + same state -> same bits.
// Rows at or beyond n are never loaded (their chunk's workgroup exits; inside the last chunk they are masked by index).
//
// mm_clip_key_loss: the same loss with the keys of the batch taken from a SECOND set of rows k [B][2N] = [ke | kf] (a
// momentum key encoder's embeddings of the same pairs; He et al., "Momentum Contrast") - queries q are never keys, keys
// are constants:
//   e->f: query qe_r over keys kf_t        f->e: query qf_r over keys ke_t         (t < B: k's row t, else bank slot t - B)
//   dqe_r = sum_{t < B + n} G_e2f[r][t] kf_t        dqf_r = sum_{t < B + n} G_f2e[r][t] ke_t        (no key term)
// Three launches, none of whose workgroups waits for another (the third's last arrivers read what the others stored, behind
// an integer ticket):
//   bank_scores_kernel, as above, its batch key rows read from k instead of z.
//   key_fold_kernel (one WAVE per (direction, query), four per workgroup): the fold of the chunks' partials, ONCE per launch
//     and direction: lane i takes chunks i, i + 64, ... in ascending order (first their maxima, then their sums relative
//     to the wave's maximum), the lanes meet in the fixed butterfly of wave_max / wave_sum -> {M, log S, PM, log PS} and
//     {l, top-1 flag, d / d logit_scale} of the query -> ws.  One load per lane and field at up to 4096 + 64 keys, where
//     the rows kernel above walks a chain of 65 in each of its workgroups.
//   key_dq_kernel (grid (tiles of 8 queries, column slabs of 32, tiles of 512 keys)): G of its 8 queries for its key tile
//     from the stored scores -> LDS (only the direction(s) its columns need), then every thread adds its key rows' float4 -
//     all loaded at once, ONCE - into the accumulators of all 8 queries: a key row is read once per query tile, not once
//     per query row.  8 lanes x 32 key phases; a thread's keys ascend, the phases are summed in phase order.  One key tile
//     by capacity: that sum is dq.  More: each workgroup stores its sums and takes an integer ticket of its (query tile,
//     slab) - the fold launch zeroed it -, and the last arriver adds the valid tiles' sums in tile order (agent-scope
//     loads); nobody waits.  A serial walk over the key tiles in one workgroup, the first build, was one wave per SIMD with
//     nothing to hide its two load latencies per tile behind: 88 us at K = 4096 (profiles/clip_key_ab.txt).  Workgroup
//     (0, 0, 0) also sums the queries' scalars in a fixed order -> scal4 (dq NULL: that workgroup alone).
// ---------------------------------------------------------------------------
constexpr int KC = 64;             // keys per chunk (two passes of 32 keys x 8 lanes)
constexpr int KCP = KC + 1;        // padded LDS row of a chunk's scores
constexpr int PF = 12;             // partial fields per (chunk, query): {m, sum, centred esum, pm, psum, centred pesum} x 2 directions
constexpr int KT = 1024;           // keys per coefficient tile of the rows kernel
constexpr int DZ_U = 16;           // key rows a rows-kernel thread keeps in flight
constexpr int SLAB = 64;           // dz columns per rows-kernel workgroup (16 float4 lanes x 16 key phases)

__device__ __forceinline__ int bank_valid(const int* state, int K, int warmup) {
    const int filled = state[1], pushes = state[2];
    const int n = pushes >= warmup ? filled : 0;
    return n < 0 ? 0 : (n > K ? K : n);                      // (a corrupt word must not become an out-of-bounds read)
}
// sum / maximum over each aligned group of 8 lanes: the first three steps of row16_sum's butterfly
__device__ __forceinline__ float oct_sum(float v) {
    v += dpp_f32<DPP_XOR1>(v);
    v += dpp_f32<DPP_XOR2>(v);
    v += dpp_f32<DPP_HALF_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float oct_max(float v) {
    v = fmaxf(v, dpp_f32<DPP_XOR1>(v));
    v = fmaxf(v, dpp_f32<DPP_XOR2>(v));
    v = fmaxf(v, dpp_f32<DPP_HALF_MIRROR>(v));
    return v;
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    acc += a.x * b.x; acc += a.y * b.y; acc += a.z * b.z; acc += a.w * b.w;
    return acc;
}
__device__ __forceinline__ const float* key_row(const float* z, const float* bank, int t, int B, int LD) {
    return t < B ? z + (size_t)t * LD : bank + (size_t)(t - B) * LD;
}

// NV > 0: a lane keeps its NV float4 of each half of its key row in registers (N <= 32 NV); 0: it reloads them per query
template <int NV>
__global__ __launch_bounds__(256) void bank_scores_kernel(const float* __restrict__ z, const float* __restrict__ kz,
                                                          const int* __restrict__ gid, const float* __restrict__ bank, const int* __restrict__ bank_gid,
                                                          const int* __restrict__ state, const float* __restrict__ logit_scale,
                                                          float* __restrict__ ws, int B, int K, int N, int warmup, int QT) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int LD = 2 * N, W = B + K, tid = threadIdx.x, sub = tid & 7, grp = tid >> 3;
    const int nk = B + bank_valid(state, K, warmup);
    const int k0 = blockIdx.x * KC;
    if (k0 >= nk) return;                                    // a chunk past the valid keys: no effect
    const int kv = min(KC, nk - k0);
    float* sq = sm;                                          // [QT][2N] the query tile
    float* sc = sq + (size_t)QT * LD;                        // [2][QT][KCP] the tile's scores
    int* kg = reinterpret_cast<int*>(sc + 2 * QT * KCP);     // [KC] the chunk's key ids
    float* Se = ws;
    float* Sf = ws + (size_t)B * W;
    float* part = ws + 2 * (size_t)B * W + (size_t)blockIdx.x * PF * B;
    const float s = expf(logit_scale[0]);
    if (gid && tid < kv) { const int t = k0 + tid; kg[tid] = t < B ? gid[t] : bank_gid[t - B]; }
    {                                                        // this workgroup's query tile
        const int q0 = blockIdx.y * QT;
        const int qn = min(QT, B - q0);
        {
            const float4* src = reinterpret_cast<const float4*>(z + (size_t)q0 * LD);
            float4* dst = reinterpret_cast<float4*>(sq);
            for (int i = tid; i < qn * (LD / 4); i += 256) dst[i] = src[i];
        }
        __syncthreads();
        for (int pass = 0; pass < KC / 32; ++pass) {
            const int kk = pass * 32 + grp, t = k0 + kk;
            const bool valid = kk < kv;
            const float* row = valid ? key_row(kz, bank, t, B, LD) : z;    // (a masked lane reads row 0 of z: in bounds)
            [[maybe_unused]] float4 ke[NV > 0 ? NV : 1], kf[NV > 0 ? NV : 1];
            if constexpr (NV > 0) {
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int n = sub * 4 + 32 * i;
                    ke[i] = kf[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (n < N) { ke[i] = *reinterpret_cast<const float4*>(row + n); kf[i] = *reinterpret_cast<const float4*>(row + N + n); }
                }
            }
            for (int r = 0; r < qn; ++r) {
                const float* qr = sq + (size_t)r * LD;
                float a = 0.f, c = 0.f;                      // a = ze_r . zf_t (e->f), c = zf_r . ze_t (f->e)
                if constexpr (NV > 0) {
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const int n = sub * 4 + 32 * i;
                        if (n < N) {
                            a = dot4(*reinterpret_cast<const float4*>(qr + n), kf[i], a);
                            c = dot4(*reinterpret_cast<const float4*>(qr + N + n), ke[i], c);
                        }
                    }
                } else {
                    for (int n = sub * 4; n < N; n += 32) {
                        a = dot4(*reinterpret_cast<const float4*>(qr + n), *reinterpret_cast<const float4*>(row + N + n), a);
                        c = dot4(*reinterpret_cast<const float4*>(qr + N + n), *reinterpret_cast<const float4*>(row + n), c);
                    }
                }
                a = oct_sum(a); c = oct_sum(c);
                if (sub == 0 && valid) {
                    sc[r * KCP + kk] = a; sc[(QT + r) * KCP + kk] = c;
                    Se[(size_t)(q0 + r) * W + t] = a; Sf[(size_t)(q0 + r) * W + t] = c;
                }
            }
        }
        __syncthreads();
        // the chunk's partials of this tile's queries: 8 lanes per (direction, query), 8 consecutive keys per lane
        for (int task = grp; task < 2 * qn; task += 32) {
            const int dir = task / qn, r = task - dir * qn, q = q0 + r;
            const float* x = sc + (size_t)(dir * QT + r) * KCP;
            const int gq = gid ? gid[q] : 0;
            float v[8];
            bool pos[8];
            float m = -INFINITY, pm = -INFINITY;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kk = sub * 8 + i;
                const bool in = kk < kv;
                v[i] = in ? x[kk] : -INFINITY;
                pos[i] = in && (gid ? kg[kk] == gq : k0 + kk == q);
                m = fmaxf(m, v[i]);
                if (pos[i]) pm = fmaxf(pm, v[i]);
            }
            m = oct_max(m); pm = oct_max(pm);                // (m is finite: kv >= 1)
            float se = 0.f, ee = 0.f, ps = 0.f, pe = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (sub * 8 + i < kv) {
                    const float p = expf(s * (v[i] - m));
                    se += p; ee += p * (v[i] - m);
                    if (pos[i]) { const float qv = expf(s * (v[i] - pm)); ps += qv; pe += qv * (v[i] - pm); }
                }
            }
            se = oct_sum(se); ee = oct_sum(ee); ps = oct_sum(ps); pe = oct_sum(pe);
            if (sub == 0) {
                float* p = part + (size_t)dir * 6 * B + q;
                p[0] = m; p[B] = se; p[2 * (size_t)B] = ee; p[3 * (size_t)B] = pm; p[4 * (size_t)B] = ps; p[5 * (size_t)B] = pe;
            }
        }
    }
}

// one chunk's partial f = {m, sum, centred esum, pm, psum, centred pesum} into the running sums relative to (M, PM)
__device__ __forceinline__ void bank_fold(const float (&f)[6], float s, float M, float PM, float& S, float& E, float& PS,
                                          float& PE) {
    const float w = expf(s * (f[0] - M));
    S += f[1] * w; E += (f[2] + f[1] * (f[0] - M)) * w;
    if (f[4] > 0.f) {                                        // (a chunk without a positive has pm = -inf)
        const float wp = expf(s * (f[3] - PM));
        PS += f[4] * wp; PE += (f[5] + f[4] * (f[3] - PM)) * wp;
    }
}

__global__ __launch_bounds__(256) void bank_rows_kernel(const float* __restrict__ z, const int* __restrict__ gid,
                                                        const float* __restrict__ bank, const int* __restrict__ bank_gid,
                                                        const int* __restrict__ state, const float* __restrict__ logit_scale,
                                                        const float* __restrict__ ws, float* __restrict__ scal,
                                                        float* __restrict__ dz, int B, int K, int N, int warmup) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int LD = 2 * N, W = B + K, tid = threadIdx.x;
    const int nk = B + bank_valid(state, K, warmup);
    const int nch = (nk + KC - 1) / KC;
    float* red = sm;                                         // [16 phases][16 lanes] float4 (first: 16-byte aligned)
    float* coef = red + 16 * 16 * 4;                         // [2][KT]
    float* nrm = coef + 2 * KT;                              // [2 directions][4][B]: {M, log S, PM, log PS} of every query
    float* rowv = nrm + 8 * (size_t)B;                       // [2 directions][3][B]: {l, top-1 flag, d / d logit_scale}
    const float* Se = ws;
    const float* Sf = ws + (size_t)B * W;
    const float* part = ws + 2 * (size_t)B * W;
    const float s = expf(logit_scale[0]);
    const size_t cs = (size_t)PF * B;                        // floats per chunk of partials
    for (int task = tid; task < 2 * B; task += 256) {        // fold the chunks' partials, in chunk order
        const int dir = task / B, j = task - dir * B;
        const float* p = part + (size_t)dir * 6 * B + j;
        float M = -INFINITY, PM = -INFINITY;
        int c = 0;
        for (; c + 16 <= nch; c += 16) {                     // (each thread walks its chunks alone: keep many loads in flight)
            float a[16], b[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { a[u] = p[(c + u) * cs]; b[u] = p[(c + u) * cs + 3 * (size_t)B]; }
#pragma unroll
            for (int u = 0; u < 16; ++u) { M = fmaxf(M, a[u]); PM = fmaxf(PM, b[u]); }
        }
        for (; c < nch; ++c) { M = fmaxf(M, p[c * cs]); PM = fmaxf(PM, p[c * cs + 3 * (size_t)B]); }
        float S = 0.f, E = 0.f, PS = 0.f, PE = 0.f;
        c = 0;
        for (; c + 8 <= nch; c += 8) {                       // 48 loads in flight, added in chunk order
            float f[8][6];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int q = 0; q < 6; ++q) f[u][q] = p[(c + u) * cs + q * (size_t)B];
#pragma unroll
            for (int u = 0; u < 8; ++u) bank_fold(f[u], s, M, PM, S, E, PS, PE);
        }
        for (; c < nch; ++c) {
            float f[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) f[q] = p[c * cs + q * (size_t)B];
            bank_fold(f, s, M, PM, S, E, PS, PE);
        }
        // the normalisers stay SPLIT into (maximum, log of the sum relative to it): s (x - M) - log S keeps the rounding of
        // a small argument where s x - (s M + log S) has that of the large s M
        const float LS = logf(S), LPS = logf(PS);
        float* o = nrm + (size_t)dir * 4 * B + j;
        o[0] = M; o[B] = LS; o[2 * (size_t)B] = PM; o[3 * (size_t)B] = LPS;
        rowv[(dir * 3 + 0) * B + j] = s * (M - PM) + (LS - LPS);
        rowv[(dir * 3 + 1) * B + j] = PM >= M ? 1.f : 0.f;   // the best positive reaches the maximum over all keys (a tie FOR it)
        rowv[(dir * 3 + 2) * B + j] = s * ((E / S - PE / PS) + (M - PM));
    }
    __syncthreads();
    const float invB = 1.f / (float)B;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < 64) {    // the rows' scalars, summed in a fixed order
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < B; r0 += 64) {
            const int j = r0 + tid;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (j < B) {
                v[0] = 0.5f * (rowv[j] + rowv[3 * B + j]);
                v[1] = rowv[B + j];
                v[2] = rowv[4 * B + j];
                v[3] = 0.5f * (rowv[2 * B + j] + rowv[5 * B + j]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += wave_sum(v[q]);
        }
        if (tid < 4) scal[tid] = (tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : acc[3]) * invB;
    }
    if (!dz) return;
    const int r = blockIdx.x;
    const int lane4 = tid & 15, phase = tid >> 4;
    const int col = blockIdx.y * SLAB + lane4 * 4;           // first of this lane's four dz columns
    const bool active = col < LD, first = col < N;
    const int src = first ? N + col : col - N;               // dze sums zf columns, dzf sums ze columns
    const float* cf = coef + (first ? 0 : KT);
    const float* n0 = nrm;                                   // e->f normalisers, n1: f->e
    const float* n1 = nrm + 4 * (size_t)B;
    const float M0 = n0[r], L0 = n0[B + r], Q0 = n0[2 * B + r], QL0 = n0[3 * B + r];
    const float M1 = n1[r], L1 = n1[B + r], Q1 = n1[2 * B + r], QL1 = n1[3 * B + r];
    const int gr = gid ? gid[r] : 0;
    const float k = 0.5f * invB * s;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t0 = 0; t0 < nk; t0 += KT) {
        const int tn = min(KT, nk - t0);
        for (int i = tid; i < tn; i += 256) {
            const int t = t0 + i;
            const float xe = Se[(size_t)r * W + t], xf = Sf[(size_t)r * W + t];
            const bool pos = gid ? (t < B ? gid[t] : bank_gid[t - B]) == gr : t == r;
            // G = P - [pos] Q with P / Q = exp(-l): a positive's P - Q = Q expm1(-l), without the cancellation of two
            // probabilities near 1.  The query terms G_e2f[r][t], G_f2e[r][t] ...
            float ce, cfv;
            if (pos) {
                ce = expf(s * (xe - Q0) - QL0) * expm1f(-rowv[r]);
                cfv = expf(s * (xf - Q1) - QL1) * expm1f(-rowv[3 * B + r]);
            } else {
                ce = expf(s * (xe - M0) - L0);
                cfv = expf(s * (xf - M1) - L1);
            }
            if (t < B) {                                     // ... and the key terms G_f2e[t][r] (x = ze_r . zf_t too), G_e2f[t][r]
                if (pos) {
                    ce += expf(s * (xe - n1[2 * B + t]) - n1[3 * B + t]) * expm1f(-rowv[3 * B + t]);
                    cfv += expf(s * (xf - n0[2 * B + t]) - n0[3 * B + t]) * expm1f(-rowv[t]);
                } else {
                    ce += expf(s * (xe - n1[t]) - n1[B + t]);
                    cfv += expf(s * (xf - n0[t]) - n0[B + t]);
                }
            }
            coef[i] = k * ce; coef[KT + i] = k * cfv;
        }
        __syncthreads();
        if (active) {
            int i = phase;
            for (; i + 16 * (DZ_U - 1) < tn; i += 16 * DZ_U) {   // DZ_U loads in flight (the loop is L2-latency bound), added in key order
                float4 v[DZ_U];
#pragma unroll
                for (int u = 0; u < DZ_U; ++u) v[u] = *reinterpret_cast<const float4*>(key_row(z, bank, t0 + i + 16 * u, B, LD) + src);
#pragma unroll
                for (int u = 0; u < DZ_U; ++u) {
                    const float g = cf[i + 16 * u];
                    acc.x += g * v[u].x; acc.y += g * v[u].y; acc.z += g * v[u].z; acc.w += g * v[u].w;
                }
            }
            for (; i < tn; i += 16) {
                const float4 v = *reinterpret_cast<const float4*>(key_row(z, bank, t0 + i, B, LD) + src);
                const float g = cf[i];
                acc.x += g * v.x; acc.y += g * v.y; acc.z += g * v.z; acc.w += g * v.w;
            }
        }
        __syncthreads();
    }
    reinterpret_cast<float4*>(red)[phase * 16 + lane4] = acc;
    __syncthreads();
    if (tid < 16 && active) {                                // the 16 key phases, in phase order
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ph = 0; ph < 16; ++ph) {
            const float4 v = reinterpret_cast<const float4*>(red)[ph * 16 + tid];
            o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
        }
        *reinterpret_cast<float4*>(dz + (size_t)r * LD + col) = o;
    }
}

// ONE workgroup: every thread reads the state words, all rows are copied, and only behind the barrier does thread 0
// advance the words - no other workgroup exists that could read a word already advanced
__global__ __launch_bounds__(256) void bank_push_kernel(const float* __restrict__ z, const int* __restrict__ gid,
                                                        float* __restrict__ bank, int* __restrict__ bank_gid, int* state,
                                                        int B, int K, int N) {
    const int tid = threadIdx.x, L4 = N / 2;                 // float4 per row
    int head = state[0];
    const int filled = state[1], pushes = state[2];
    head = ((head % K) + K) % K;                             // (a corrupt word must not become an out-of-bounds store)
    const float4* src = reinterpret_cast<const float4*>(z);
    float4* dst = reinterpret_cast<float4*>(bank);
    for (int i = tid; i < B * L4; i += 256) {
        const int row = i / L4, c = i - row * L4;
        int slot = head + row;
        if (slot >= K) slot -= K;
        dst[(size_t)slot * L4 + c] = src[i];
    }
    if (gid)
        for (int i = tid; i < B; i += 256) {
            int slot = head + i;
            if (slot >= K) slot -= K;
            bank_gid[slot] = gid[i];
        }
    __syncthreads();
    if (tid == 0) {
        state[0] = (head + B) % K;
        state[1] = min(max(filled, 0) + B, K);
        state[2] = pushes + 1;
    }
}

// ---- mm_clip_key_loss: launches two and three (the first is bank_scores_kernel) ----
constexpr int FQ = 14;             // folded floats per query: nrm [2 directions][4][B] then rowv [2 directions][3][B]
constexpr int DQ_QT = 8;           // queries per dq workgroup
constexpr int DQ_KT = 512;         // keys per coefficient tile
constexpr int DQ_L = 8;            // float4 lanes per column slab (32 columns)
constexpr int DQ_PH = 256 / DQ_L;  // key phases
constexpr int DQ_U = DQ_KT / DQ_PH;  // key rows a thread keeps in flight: all of its tile's

__global__ __launch_bounds__(256) void key_fold_kernel(const int* __restrict__ state, const float* __restrict__ logit_scale,
                                                       const float* __restrict__ part, float* __restrict__ fold,
                                                       int* __restrict__ tickets, int n_tickets, int B, int K, int warmup) {
    if (blockIdx.x == 0)                                     // the next launch's tickets (ws comes uninitialised); NULL: none
        for (int i = threadIdx.x; i < n_tickets; i += 256) tickets[i] = 0;
    const int lane = threadIdx.x & 63;
    const int task = blockIdx.x * 4 + (threadIdx.x >> 6);    // (wave-uniform)
    if (task >= 2 * B) return;
    const int nk = B + bank_valid(state, K, warmup);
    const int nch = (nk + KC - 1) / KC;
    const float s = expf(logit_scale[0]);
    const size_t cs = (size_t)PF * B;                        // floats per chunk of partials
    const int dir = task / B, j = task - dir * B;
    const float* p = part + (size_t)dir * 6 * B + j;
    float M = -INFINITY, PM = -INFINITY;
    for (int c = lane; c < nch; c += 64) { M = fmaxf(M, p[c * cs]); PM = fmaxf(PM, p[c * cs + 3 * (size_t)B]); }
    M = wave_max(M); PM = wave_max(PM);                      // (finite: chunk 0 exists and holds the query's own pair)
    float S = 0.f, E = 0.f, PS = 0.f, PE = 0.f;
    for (int c = lane; c < nch; c += 64) {
        float f[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) f[q] = p[c * cs + q * (size_t)B];
        bank_fold(f, s, M, PM, S, E, PS, PE);
    }
    S = wave_sum(S); E = wave_sum(E); PS = wave_sum(PS); PE = wave_sum(PE);
    if (lane == 0) {                                         // (split normalisers: see bank_rows_kernel)
        const float LS = logf(S), LPS = logf(PS);
        float* o = fold + (size_t)dir * 4 * B + j;
        o[0] = M; o[B] = LS; o[2 * (size_t)B] = PM; o[3 * (size_t)B] = LPS;
        float* rowv = fold + 8 * (size_t)B + (size_t)dir * 3 * B + j;
        rowv[0] = s * (M - PM) + (LS - LPS);
        rowv[B] = PM >= M ? 1.f : 0.f;                       // the best positive reaches the maximum over all keys (a tie FOR it)
        rowv[2 * (size_t)B] = s * ((E / S - PE / PS) + (M - PM));
    }
}

// grid (tiles of DQ_QT queries, slabs of 4 DQ_L columns, tiles of DQ_KT keys by the CAPACITY B + K).  gridDim.z == 1: the
// workgroup's sums are dq; else they go to dqp [key tile][B][2N] and the LAST workgroup of a (query tile, slab) to take its
// integer ticket adds the valid key tiles' sums in tile order -> dq (it waits for nobody; a key tile past B + n adds nothing
// but takes its ticket)
__global__ __launch_bounds__(256) void key_dq_kernel(const float* __restrict__ kz, const int* __restrict__ gid,
                                                     const float* __restrict__ bank, const int* __restrict__ bank_gid,
                                                     const int* __restrict__ state, const float* __restrict__ logit_scale,
                                                     const float* __restrict__ ws, const float* __restrict__ fold,
                                                     float* dqp, int* tickets, float* __restrict__ scal,
                                                     float* __restrict__ dq, int B, int K, int N, int warmup) {
    __shared__ __attribute__((aligned(16))) float coef[2 * DQ_QT * DQ_KT];   // [2 directions][DQ_QT][DQ_KT]; then the phases' sums
    __shared__ float qs[2][5][DQ_QT];                        // {M, log S, PM, log PS, expm1(-l)} of the tile's queries
    __shared__ int qg[DQ_QT];
    __shared__ float4 red2[256];                             // [DQ_QT][4 phase groups][DQ_L]
    __shared__ int last;
    const int LD = 2 * N, W = B + K, tid = threadIdx.x;
    const int nk = B + bank_valid(state, K, warmup);
    const float* rowv = fold + 8 * (size_t)B;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid < 64) {     // the queries' scalars, summed in a fixed order
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < B; r0 += 64) {
            const int j = r0 + tid;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (j < B) {
                v[0] = 0.5f * (rowv[j] + rowv[3 * (size_t)B + j]);
                v[1] = rowv[B + j];
                v[2] = rowv[4 * (size_t)B + j];
                v[3] = 0.5f * (rowv[2 * (size_t)B + j] + rowv[5 * (size_t)B + j]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += wave_sum(v[q]);
        }
        // a division, not a product with 1 / B: a top-1 word is count / B rounded once (5 / 6 is not 5 * fl(1 / 6))
        if (tid < 4) scal[tid] = (tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : acc[3]) / (float)B;
    }
    if (!dq) return;
    const int q0 = blockIdx.x * DQ_QT;
    const int qn = min(DQ_QT, B - q0);
    const int lane4 = tid & (DQ_L - 1), phase = tid / DQ_L;
    const int c0 = blockIdx.y * DQ_L * 4;                    // first column of the slab
    const int col = c0 + lane4 * 4;                          // first of this lane's four dq columns
    const bool active = col < LD, first = col < N;
    const bool need_e = c0 < N, need_f = c0 + DQ_L * 4 > N;  // dqe columns take G_e2f, dqf columns G_f2e (a slab may hold both)
    const int src = first ? N + col : col - N;               // dqe sums kf columns, dqf sums ke columns
    const int t0 = blockIdx.z * DQ_KT;
    const int tn = min(DQ_KT, nk - t0);                      // (<= 0: a key tile past the valid keys)
    const bool split = gridDim.z > 1;
    if (tn > 0) {
        const float* Se = ws;
        const float* Sf = ws + (size_t)B * W;
        const float s = expf(logit_scale[0]);
        // this thread's key rows first - they depend on nothing computed here, so their latency runs beside the
        // normalisers', the scores' and the exponentials' (a row past the tile's end: row t0, weighted by a zero below)
        float4 v[DQ_U];
#pragma unroll
        for (int u = 0; u < DQ_U; ++u) {
            const int i = phase + DQ_PH * u;
            v[u] = *reinterpret_cast<const float4*>(key_row(kz, bank, t0 + (i < tn ? i : 0), B, LD) + (active ? src : 0));
        }
        if (tid < 2 * 5 * DQ_QT) {
            const int dir = tid / (5 * DQ_QT), f = tid / DQ_QT % 5, r = tid % DQ_QT;
            if (r < qn) qs[dir][f][r] = f < 4 ? fold[((size_t)dir * 4 + f) * B + q0 + r] : expm1f(-rowv[(size_t)dir * 3 * B + q0 + r]);
        }
        if (gid && tid < qn) qg[tid] = gid[q0 + tid];
        float xe[DQ_KT / 256][DQ_QT], xf[DQ_KT / 256][DQ_QT];   // (all score loads of the tile's queries at once: one latency, not qn)
        int kgid[DQ_KT / 256];
#pragma unroll
        for (int j = 0; j < DQ_KT / 256; ++j) {
            const int i = tid + 256 * j, t = t0 + i;
            kgid[j] = gid && i < tn ? (t < B ? gid[t] : bank_gid[t - B]) : 0;
#pragma unroll
            for (int r = 0; r < DQ_QT; ++r) {
                xe[j][r] = need_e && r < qn && i < tn ? Se[(size_t)(q0 + r) * W + t] : 0.f;
                xf[j][r] = need_f && r < qn && i < tn ? Sf[(size_t)(q0 + r) * W + t] : 0.f;
            }
        }
        __syncthreads();
        const float k = 0.5f / (float)B * s;
#pragma unroll
        for (int j = 0; j < DQ_KT / 256; ++j) {
            const int i = tid + 256 * j, t = t0 + i;
#pragma unroll
            for (int r = 0; r < DQ_QT; ++r) {
                // G = P - [pos] Q with P / Q = exp(-l): a positive's P - Q = Q expm1(-l) (see bank_rows_kernel); keys past the
                // tile's end and queries past the batch's get a zero
                const bool in = r < qn && i < tn;
                const bool pos = gid ? kgid[j] == qg[r < qn ? r : 0] : t == q0 + r;
                // (one expf either way: the positives' normalisers and factor are selected, not a second exponential)
                if (need_e)
                    coef[r * DQ_KT + i] = !in ? 0.f : k * expf(s * (xe[j][r] - qs[0][pos ? 2 : 0][r]) - qs[0][pos ? 3 : 1][r]) * (pos ? qs[0][4][r] : 1.f);
                if (need_f)
                    coef[(DQ_QT + r) * DQ_KT + i] = !in ? 0.f : k * expf(s * (xf[j][r] - qs[1][pos ? 2 : 0][r]) - qs[1][pos ? 3 : 1][r]) * (pos ? qs[1][4][r] : 1.f);
            }
        }
        __syncthreads();
        const float* cf = coef + (first ? 0 : DQ_QT * DQ_KT);
        float4 acc[DQ_QT];
#pragma unroll
        for (int r = 0; r < DQ_QT; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active) {
#pragma unroll
            for (int u = 0; u < DQ_U; ++u) {                 // added in key order
                const int i = phase + DQ_PH * u;
                if (i >= tn) break;
#pragma unroll
                for (int r = 0; r < DQ_QT; ++r) {
                    const float g = cf[r * DQ_KT + i];
                    acc[r].x += g * v[u].x; acc[r].y += g * v[u].y; acc[r].z += g * v[u].z; acc[r].w += g * v[u].w;
                }
            }
        }
        __syncthreads();
        float4* red = reinterpret_cast<float4*>(coef);       // [DQ_QT][DQ_PH][DQ_L] (the coefficients are done with: barrier above)
#pragma unroll
        for (int r = 0; r < DQ_QT; ++r) red[(r * DQ_PH + phase) * DQ_L + lane4] = acc[r];
        __syncthreads();
        {                                                    // the key phases: four groups of DQ_PH / 4 in phase order ...
            const int r = tid / (4 * DQ_L), pg = tid / DQ_L % 4, l = tid % DQ_L;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int ph = pg * (DQ_PH / 4); ph < (pg + 1) * (DQ_PH / 4); ++ph) {
                const float4 v = red[(r * DQ_PH + ph) * DQ_L + l];
                o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
            }
            red2[tid] = o;
        }
        __syncthreads();
        if (tid < DQ_QT * DQ_L) {                            // ... then the four groups, in group order
            const int r = tid / DQ_L, l = tid % DQ_L, c = c0 + l * 4;
            if (r < qn && c < LD) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int pg = 0; pg < 4; ++pg) {
                    const float4 v = red2[(r * 4 + pg) * DQ_L + l];
                    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
                }
                float* dst = split ? dqp + (size_t)blockIdx.z * B * LD : dq;
                *reinterpret_cast<float4*>(dst + (size_t)(q0 + r) * LD + c) = o;
            }
        }
    }
    if (!split) return;
    __threadfence();                                         // this workgroup's sums, before its ticket
    __syncthreads();
    if (tid == 0) last = atomicAdd(tickets + blockIdx.x * gridDim.y + blockIdx.y, 1) == (int)gridDim.z - 1;   // integer ticket
    __syncthreads();
    if (!last) return;
    __threadfence();
    {                                                        // the valid key tiles' sums, in tile order: one float per thread
        const int r = tid / (4 * DQ_L), c = c0 + tid % (4 * DQ_L);
        if (r < qn && c < LD) {
            const int nt = (nk + DQ_KT - 1) / DQ_KT;
            const float* p = dqp + (size_t)(q0 + r) * LD + c;
            const size_t zs = (size_t)B * LD;
            float o = 0.f;
            for (int z0 = 0; z0 < nt; z0 += 16) {            // other workgroups' stores: read past this CU's vector cache,
                float t[16];                                 // 16 loads in flight (one round trip at up to 8192 keys)
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    t[u] = z0 + u < nt ? __hip_atomic_load(p + (z0 + u) * zs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u) o += t[u];      // (the padding adds +0: the sum is the tiles' in tile order)
            }
            dq[(size_t)(q0 + r) * LD + c] = o;
        }
    }
}
}  // namespace

extern "C" {
static int bank_chunks(int B, int K) { return (B + K + KC - 1) / KC; }

static int bank_check_shape(const char* who, int B, int K, int N) {
    MM_REQUIRE(N > 0 && N % 4 == 0, "%s: N=%d must be a positive multiple of 4 (16-byte row loads)", who, N);
    MM_REQUIRE(B >= 1 && B <= K, "%s: need 1 <= B <= K (B=%d K=%d)", who, B, K);
    MM_REQUIRE((long long)B * (B + (long long)K) < (1ll << 30), "%s: B=%d K=%d too large", who, B, K);
    return 0;
}

int mm_clip_bank_ws_floats(int B, int K, int N, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host, "clip_bank_ws_floats: null");
    int rc = bank_check_shape("clip_bank_ws_floats", B, K, N);
    if (rc) return rc;
    const long long n = 2ll * B * (B + K) + (long long)bank_chunks(B, K) * PF * B;
    MM_REQUIRE(n < (1ll << 31), "clip_bank_ws_floats: B=%d K=%d too large", B, K);
    *floats_host = (int)n;
    return 0;
}

int mm_clip_bank_loss(const float* z, const int* gid, const float* bank, const int* bank_gid, const int* state,
                      const float* logit_scale, float* scal4, float* dz, float* ws, int B, int K, int N, int warmup,
                      hipStream_t st) {
    MM_REQUIRE(z && bank && state && logit_scale && scal4 && ws, "clip_bank_loss: null");
    MM_REQUIRE(!gid || bank_gid, "clip_bank_loss: group ids need a bank that carries ids (bank_gid is null)");
    MM_REQUIRE(warmup >= 0, "clip_bank_loss: warmup=%d", warmup);
    int rc = bank_check_shape("clip_bank_loss", B, K, N);
    if (rc) return rc;
    MM_REQUIRE(((uintptr_t)z | (uintptr_t)bank | (uintptr_t)dz | (uintptr_t)ws) % 16 == 0, "clip_bank_loss: z, bank, dz and ws must be 16-byte aligned");
    // the scores kernel's query tile: 8 rows (a workgroup is latency-bound: short loops on many workgroups), fewer when
    // 48 KB of LDS do not hold them beside the tile's scores
    const int LD = 2 * N;
    int QT = (12288 - KC) / (LD + 2 * KCP);
    QT = QT > 8 ? 8 : QT;
    QT = QT > B ? B : QT;
    MM_REQUIRE(QT >= 1, "clip_bank_loss: N=%d too large for LDS", N);
    const size_t lds_a = ((size_t)QT * LD + 2 * (size_t)QT * KCP + KC) * sizeof(float);
    const size_t lds_b = (14 * (size_t)B + 2 * KT + 16 * 16 * 4) * sizeof(float);
    MM_REQUIRE(lds_b <= 64 * 1024, "clip_bank_loss: B=%d too large for LDS", B);
    const auto scores = N <= 128 ? bank_scores_kernel<4> : bank_scores_kernel<0>;
    hipLaunchKernelGGL(scores, dim3(bank_chunks(B, K), (B + QT - 1) / QT), dim3(256), lds_a, st, z, z, gid, bank, bank_gid, state, logit_scale, ws,
                       B, K, N, warmup, QT);
    rc = mm_check_launch("clip_bank_loss(scores)");
    if (rc) return rc;
    const dim3 grid = dz ? dim3(B, (LD + SLAB - 1) / SLAB) : dim3(1, 1);
    hipLaunchKernelGGL(bank_rows_kernel, grid, dim3(256), lds_b, st, z, gid, bank, bank_gid, state, logit_scale, ws, scal4, dz,
                       B, K, N, warmup);
    return mm_check_launch("clip_bank_loss(rows)");
}

// ws of mm_clip_key_loss = [scores | chunk partials | folded FQ B, padded to 4 floats | dq sums per key tile (more than one
// tile only) | one ticket per (query tile, column slab)]
static long long key_fold_offset(int B, int K) { return 2ll * B * (B + K) + (long long)bank_chunks(B, K) * PF * B; }
static int key_tiles(int B, int K) { return (B + K + DQ_KT - 1) / DQ_KT; }
static long long key_dqp_offset(int B, int K) { return (key_fold_offset(B, K) + (long long)FQ * B + 3) / 4 * 4; }
static int key_tickets(int B, int N) { return ((B + DQ_QT - 1) / DQ_QT) * ((2 * N + DQ_L * 4 - 1) / (DQ_L * 4)); }
static long long key_ws_floats(int B, int K, int N) {
    const int nt = key_tiles(B, K);
    return key_dqp_offset(B, K) + (nt > 1 ? (long long)nt * B * 2 * N + key_tickets(B, N) : 0);
}

int mm_clip_key_ws_floats(int B, int K, int N, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host, "clip_key_ws_floats: null");
    int rc = bank_check_shape("clip_key_ws_floats", B, K, N);
    if (rc) return rc;
    const long long n = key_ws_floats(B, K, N);
    MM_REQUIRE(n < (1ll << 31), "clip_key_ws_floats: B=%d K=%d too large", B, K);
    *floats_host = (int)n;
    return 0;
}

int mm_clip_key_loss(const float* q, const float* k, const int* gid, const float* bank, const int* bank_gid, const int* state,
                     const float* logit_scale, float* scal4, float* dq, float* ws, int B, int K, int N, int warmup,
                     hipStream_t st) {
    MM_REQUIRE(q && k && bank && state && logit_scale && scal4 && ws, "clip_key_loss: null");
    MM_REQUIRE(!gid || bank_gid, "clip_key_loss: group ids need a bank that carries ids (bank_gid is null)");
    MM_REQUIRE(warmup >= 0, "clip_key_loss: warmup=%d", warmup);
    int rc = bank_check_shape("clip_key_loss", B, K, N);
    if (rc) return rc;
    MM_REQUIRE(key_ws_floats(B, K, N) < (1ll << 31), "clip_key_loss: B=%d K=%d too large", B, K);
    MM_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)bank | (uintptr_t)dq | (uintptr_t)ws) % 16 == 0,
               "clip_key_loss: q, k, bank, dq and ws must be 16-byte aligned");
    const int LD = 2 * N;
    int QT = (12288 - KC) / (LD + 2 * KCP);                  // the scores kernel's query tile, as in mm_clip_bank_loss
    QT = QT > 8 ? 8 : QT;
    QT = QT > B ? B : QT;
    MM_REQUIRE(QT >= 1, "clip_key_loss: N=%d too large for LDS", N);
    const size_t lds_a = ((size_t)QT * LD + 2 * (size_t)QT * KCP + KC) * sizeof(float);
    const auto scores = N <= 128 ? bank_scores_kernel<4> : bank_scores_kernel<0>;
    hipLaunchKernelGGL(scores, dim3(bank_chunks(B, K), (B + QT - 1) / QT), dim3(256), lds_a, st, q, k, gid, bank, bank_gid, state, logit_scale,
                       ws, B, K, N, warmup, QT);
    rc = mm_check_launch("clip_key_loss(scores)");
    if (rc) return rc;
    const float* part = ws + 2 * (size_t)B * (B + K);
    float* fold = ws + key_fold_offset(B, K);
    const int nt = key_tiles(B, K);
    const bool split = dq && nt > 1;                         // more than one key tile: their sums meet behind a ticket
    float* dqp = ws + key_dqp_offset(B, K);
    int* tickets = reinterpret_cast<int*>(dqp + (size_t)nt * B * LD);
    hipLaunchKernelGGL(key_fold_kernel, dim3((2 * B + 3) / 4), dim3(256), 0, st, state, logit_scale, part, fold,
                       split ? tickets : nullptr, split ? key_tickets(B, N) : 0, B, K, warmup);
    rc = mm_check_launch("clip_key_loss(fold)");
    if (rc) return rc;
    const dim3 grid = dq ? dim3((B + DQ_QT - 1) / DQ_QT, (LD + DQ_L * 4 - 1) / (DQ_L * 4), nt) : dim3(1, 1, 1);
    hipLaunchKernelGGL(key_dq_kernel, grid, dim3(256), 0, st, k, gid, bank, bank_gid, state, logit_scale, ws, fold,
                       split ? dqp : nullptr, split ? tickets : nullptr, scal4, dq, B, K, N, warmup);
    return mm_check_launch("clip_key_loss(dq)");
}

int mm_clip_bank_push(const float* z, const int* gid, float* bank, int* bank_gid, int* state, int B, int K, int N,
                      hipStream_t st) {
    MM_REQUIRE(z && bank && state, "clip_bank_push: null");
    MM_REQUIRE(!gid || bank_gid, "clip_bank_push: group ids need a bank that carries ids (bank_gid is null)");
    int rc = bank_check_shape("clip_bank_push", B, K, N);
    if (rc) return rc;
    MM_REQUIRE(((uintptr_t)z | (uintptr_t)bank) % 16 == 0, "clip_bank_push: z and bank must be 16-byte aligned");
    hipLaunchKernelGGL(bank_push_kernel, dim3(1), dim3(256), 0, st, z, gid, bank, bank_gid, state, B, K, N);
    return mm_check_launch("clip_bank_push");
}
}  // extern "C"
