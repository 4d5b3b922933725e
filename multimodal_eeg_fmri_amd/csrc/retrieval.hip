// Gallery-scale retrieval: for every query row of Q [Nq][D] against a gallery G [Ng][D] (fp32), the rank of its
// positive and/or its top-k matches, without ever storing the Nq x Ng score matrix (include/mmeeg_hip.h,
// mm_retrieval; DESIGN.md "Gallery-scale retrieval").
//
// Scores come from the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32): each score is ONE ascending-d fmaf chain from
// +0, the same bits wherever the pair sits in a tile.  The positive's score is computed by the same instruction in the
// same order (pos_score_kernel), so an exact duplicate of the positive scores bit-equal to it and counts against the
// query - the tie rule.  (The in-batch top-1 of clip_loss.hip's clip_lse_kernel counts a tie FOR the query; see there.)
//
// Pass 1 (pos_score_kernel): s(q, pos[q]) for every query.
// Pass 2 (retr_tile_kernel<RANK, TOPK>): workgroup (query block of 128, gallery slice) walks its slice in 128-wide
//   tiles.  4 waves, each a 64 x 64 quarter of the 128 x 128 tile as 2 x 2 accumulators of 32 x 32; K streams through
//   LDS in chunks of 16 (next chunk prefetched into registers while the current one is multiplied).  Epilogue per tile:
//   integer count of {j != pos : s >= s_pos} per row; top-k candidates that beat the row's current k-th entry go to a
//   per-row LDS buffer and one thread per row merges them into the row's sorted list (rounds until every candidate is
//   placed).  At the end of the slice: per-(slice, query) count and list to the workspace.
// Pass 3 (retr_finish_kernel): one thread per query adds its slices' counts (integers) and merges their lists in slice
//   order.  No float atomics: same inputs -> same bits.
//
// Grouped positives (mm_retrieval_grouped): gallery row j is a positive of query q when ggid[j] == qgid[q], and the rank
// is that of the best-placed positive.  Pass 1 becomes a sweep of the same tiles (retr_tile_kernel<false, false,
// GRP_MAX>): per (slice, query) the maximum score over the slice's positives; retr_best_kernel folds the slices into
// s*(q).  The counting sweep (GRP_COUNT) then counts {j : ggid[j] != qgid[q], s >= s*} and pass 3 is unchanged.  Both
// sweeps score with the same MFMA chain, so a duplicate of the best positive ties with it bit for bit.
//
// Ignored temporal neighbours (mm_retrieval_masked): the ids are positions on a timeline and, with the radius R >= 0 and
// d = |ggid[j] - qgid[q]| (an unsigned difference, retr_id_dist), d == 0 is a positive, 0 < d <= R is ignored and d > R a
// negative.  The maxima sweep is the grouped one (equality needs no radius).  The counting sweep runs in a fourth mode
// (GRP_MASK): it counts {j : d > R, s >= s*} and, with NEG, {j : d > R} (ids only), and - for the first time together with
// group ids - keeps top-k lists, which a candidate enters only when d == 0 or d > R.  Pass 3 also adds the second count.
#include "common.h"
#include "mmeeg_hip.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int QB = 128;                 // queries per workgroup
constexpr int GB = 128;                 // gallery columns per tile
constexpr int KC = 16;                  // K chunk through LDS
constexpr int LDS_STRIDE = QB + 36;     // [k][row] image: column reads conflict-free up to 4 banks, float4-row stores conflict-free
constexpr int KMAX = MM_RETRIEVAL_KMAX;
constexpr int LSTR = KMAX + 1;          // per-row list stride in LDS (odd: one thread per row, no 16-way conflicts)
constexpr int CAP = 16;                 // top-k candidates per row per merge round
constexpr int TARGET_WG = 512;          // 2 workgroups per CU on 256 CUs
constexpr int GRP_NONE = 0, GRP_MAX = 1, GRP_COUNT = 2, GRP_MASK = 3;     // retr_tile_kernel's group modes (see the file comment)

// max that ignores NaN: a NaN b leaves a; NaN only when both are
__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || a != a) ? b : a; }
__device__ __forceinline__ float half32_nanmax(float v) {      // over each aligned group of 32 lanes (fixed pairing)
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) v = nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

// |a - b| of two int32 ids in [0, 2^32): the unsigned difference of the larger and the smaller cannot wrap (clip_loss.hip's
// clip_id_dist)
__device__ __forceinline__ unsigned retr_id_dist(int a, int b) {
    return a >= b ? (unsigned)a - (unsigned)b : (unsigned)b - (unsigned)a;
}

__device__ __forceinline__ bool beats(float s, int j, float ts, int tj) {
    // total order of the top-k lists: score descending, then index ascending; NaN never beats anything
    return s > ts || (s == ts && j < tj);
}

// insert (s, j) into a sorted list of k entries (stride 1); false if it does not make the list
__device__ __forceinline__ void list_insert(float* ls, int* li, int k, float s, int j) {
    if (!beats(s, j, ls[k - 1], li[k - 1])) return;
    int p = k - 1;
    while (p > 0 && beats(s, j, ls[p - 1], li[p - 1])) {
        ls[p] = ls[p - 1];
        li[p] = li[p - 1];
        --p;
    }
    ls[p] = s;
    li[p] = j;
}

// s(q, pos[q]) through the same MFMA chain as the tiles: one wave per 32 queries computes Q[q] . G[pos[q]] for all 32 x 32
// (query, positive) pairs and keeps the diagonal.  Rows beyond Nq are clamped (not written).
__global__ __launch_bounds__(64) void pos_score_kernel(const float* __restrict__ Q, const float* __restrict__ G,
                                                        const int* __restrict__ pos, float* __restrict__ spos, int Nq, int Ng, int D) {
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int q = min(blockIdx.x * 32 + i, Nq - 1);
    const int p_in = pos ? pos[q] : q;
    const bool p_bad = p_in < 0 || p_in >= Ng;          // outside the gallery: never read; NaN score -> rank Ng
    const int p = p_bad ? 0 : p_in;
    const float* qa = Q + (size_t)q * D + h;
    const float* gb = G + (size_t)p * D + h;
    f32x16 acc = {};
    for (int d = 0; d < D; d += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[d], gb[d], acc, 0, 0, 0);
    // C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 h: the diagonal element of column i sits in the lane
    // half h = (i >> 2) & 1, register (i & 3) + 4 (i >> 3)
    if (h == ((i >> 2) & 1)) {
        const int reg = (i & 3) + 4 * (i >> 3);
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) v = r == reg ? acc[r] : v;
        const int qq = blockIdx.x * 32 + i;
        if (qq < Nq) spos[qq] = p_bad ? __builtin_nanf("") : v;
    }
}

struct RetrPlan {
    int qblocks, ntiles, tps, nslices;
};
static RetrPlan retr_plan(int Nq, int Ng) {
    RetrPlan p;
    p.qblocks = ceil_div(Nq, QB);
    p.ntiles = ceil_div(Ng, GB);
    const int want = max(1, min(p.ntiles, ceil_div(TARGET_WG, p.qblocks)));
    p.tps = ceil_div(p.ntiles, want);
    p.nslices = ceil_div(p.ntiles, p.tps);      // every slice holds >= 1 tile
    return p;
}

struct RetrArgs {
    const float* Q; const float* G; const int* pos; const float* spos;
    const int* qgid; const int* ggid;       // grouped positives (GRP_MAX / GRP_COUNT / GRP_MASK), else null
    float* smax;       // [nslices][Nq] per-slice maxima over the positives (GRP_MAX)
    int* cnt;          // [nslices][Nq]
    float* tks;        // [nslices][Nq][k]
    int* tki;          // [nslices][Nq][k]
    int Nq, Ng, D, k, tps, ntiles;
    int radius;        // GRP_MASK: 0 < d <= radius is ignored (unread in the other modes)
    int* ncnt;         // [nslices][Nq] per-slice #{j : d > radius} (NEG)
    int* negatives;    // [Nq] (NEG)
};

template <bool RANK, bool TOPK, int GRP = GRP_NONE, bool NEG = false>
__global__ __launch_bounds__(256, TOPK ? 1 : 2) void retr_tile_kernel(RetrArgs a) {
    __shared__ float qs[KC * LDS_STRIDE];
    __shared__ float gs[KC * LDS_STRIDE];
    __shared__ float lst_s[TOPK ? QB * LSTR : 1];
    __shared__ int lst_i[TOPK ? QB * LSTR : 1];
    __shared__ float cand_s[TOPK ? QB * CAP : 1];
    __shared__ int cand_i[TOPK ? QB * CAP : 1];
    __shared__ int ccount[TOPK ? QB : 1];
    __shared__ int part[RANK ? 2 * QB : 1];
    __shared__ float sp_s[RANK ? QB : 1];
    __shared__ int pq_s[RANK || GRP ? QB : 1];         // the positive's index, or the query's group id
    __shared__ float pmax[GRP == GRP_MAX ? 2 * QB : 1];
    __shared__ int npart[NEG ? 2 * QB : 1];
    static_assert(!NEG || GRP == GRP_MASK, "the id-only count belongs to the masked sweep");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;       // row half / column half of the 128 x 128 tile
    const int q0 = blockIdx.x * QB;
    const int slice = blockIdx.y;
    const int t_begin = slice * a.tps, t_end = min(a.ntiles, t_begin + a.tps);
    const int D = a.D, k = a.k;
    const int nchunk = (D + KC - 1) / KC;

    // rows this lane's accumulator registers hold: tile row of (rt, reg) = wr * 64 + 32 rt + (reg & 3) + 8 (reg >> 2) + 4 h.
    // Positive score / index per row in LDS (read per tile: registers go to the accumulators and the counts)
    int cnt[2][16];
    int ncnt[2][16];
    float mx[2][16];
    if constexpr (GRP == GRP_MAX) {
        if (tid < QB) pq_s[tid] = a.qgid[min(q0 + tid, a.Nq - 1)];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[rt][r] = __builtin_nanf("");
    }
    if constexpr (GRP == GRP_MASK) {
        if (!RANK && tid < QB) pq_s[tid] = a.qgid[min(q0 + tid, a.Nq - 1)];
        if constexpr (NEG) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) ncnt[rt][r] = 0;
        }
    }
    if (RANK) {
        if (tid < QB) {
            const int q = min(q0 + tid, a.Nq - 1);
            sp_s[tid] = a.spos[q];
            if constexpr (GRP == GRP_COUNT || GRP == GRP_MASK) pq_s[tid] = a.qgid[q];
            else pq_s[tid] = a.pos ? a.pos[q] : q;
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) cnt[rt][r] = 0;
    }
    if (TOPK) {
        for (int e = tid; e < QB * LSTR; e += 256) { lst_s[e] = -INFINITY; lst_i[e] = INT_MAX; }
        if (tid < QB) ccount[tid] = 0;
    }

    // global -> register prefetch: thread covers float4 (row = idx >> 2, k4 = idx & 3) of the Q and G chunks, idx = tid, tid + 256
    float4 rq[2], rg[2];
    auto fetch = [&](int t, int c) {
        const int j0 = t * GB, k0 = c * KC;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, row = idx >> 2, kk = k0 + 4 * (idx & 3);
            const int q = q0 + row, j = j0 + row;
            const bool kin = kk < D;
            rq[u] = (kin && q < a.Nq) ? *reinterpret_cast<const float4*>(a.Q + (size_t)q * D + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
            rg[u] = (kin && j < a.Ng) ? *reinterpret_cast<const float4*>(a.G + (size_t)j * D + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, row = idx >> 2, kb = 4 * (idx & 3);
            qs[(kb + 0) * LDS_STRIDE + row] = rq[u].x; qs[(kb + 1) * LDS_STRIDE + row] = rq[u].y;
            qs[(kb + 2) * LDS_STRIDE + row] = rq[u].z; qs[(kb + 3) * LDS_STRIDE + row] = rq[u].w;
            gs[(kb + 0) * LDS_STRIDE + row] = rg[u].x; gs[(kb + 1) * LDS_STRIDE + row] = rg[u].y;
            gs[(kb + 2) * LDS_STRIDE + row] = rg[u].z; gs[(kb + 3) * LDS_STRIDE + row] = rg[u].w;
        }
    };

    fetch(t_begin, 0);
    for (int t = t_begin; t < t_end; ++t) {
        f32x16 acc[2][2] = {};
        int gg[2] = {0, 0};                        // group ids of this lane's two columns (loaded under the MFMA loop)
        if constexpr (GRP != GRP_NONE) {
            const int j0 = t * GB + wc * 64 + li;
            gg[0] = j0 < a.Ng ? a.ggid[j0] : 0;
            gg[1] = j0 + 32 < a.Ng ? a.ggid[j0 + 32] : 0;
        }
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();                       // every wave is done reading the previous chunk
            stash();
            __syncthreads();
            if (c + 1 < nchunk) fetch(t, c + 1);
            else if (t + 1 < t_end) fetch(t + 1, 0);
            const int steps = min(KC, D - c * KC) >> 1;      // D % 4 == 0: whole steps; zero-filled k never enter a chain
            const float* qa = qs + h * LDS_STRIDE + wr * 64 + li;
            const float* gb = gs + h * LDS_STRIDE + wc * 64 + li;
            for (int s = 0; s < steps; ++s) {
                // k-slot 0 (lanes 0-31) = d, k-slot 1 (lanes 32-63) = d + 1: one ascending fmaf chain per element
                const float a0 = qa[2 * s * LDS_STRIDE], a1 = qa[2 * s * LDS_STRIDE + 32];
                const float b0 = gb[2 * s * LDS_STRIDE], b1 = gb[2 * s * LDS_STRIDE + 32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        const int jb = t * GB + wc * 64 + li;          // gallery index of column tile ct: jb + 32 ct
        if constexpr (GRP == GRP_MASK && (RANK || NEG)) {
            const bool in0 = jb < a.Ng, in1 = jb + 32 < a.Ng;
            const unsigned R = (unsigned)a.radius;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int pq = pq_s[row];
                    const bool far0 = in0 & (retr_id_dist(gg[0], pq) > R), far1 = in1 & (retr_id_dist(gg[1], pq) > R);
                    if (RANK) {
                        const float sp = sp_s[row];
                        cnt[rt][r] += (far0 & (acc[rt][0][r] >= sp)) + (far1 & (acc[rt][1][r] >= sp));
                    }
                    if constexpr (NEG) ncnt[rt][r] += far0 + far1;
                }
        }
        if (RANK && GRP != GRP_MASK) {
            const bool in0 = jb < a.Ng, in1 = jb + 32 < a.Ng;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = wr * 64 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float sp = sp_s[row];
                    const int pq = pq_s[row];
                    if constexpr (GRP == GRP_COUNT)
                        cnt[rt][r] += (in0 & (acc[rt][0][r] >= sp) & (gg[0] != pq)) + (in1 & (acc[rt][1][r] >= sp) & (gg[1] != pq));
                    else
                        cnt[rt][r] += (in0 & (acc[rt][0][r] >= sp) & (jb != pq)) + (in1 & (acc[rt][1][r] >= sp) & (jb + 32 != pq));
                }
        }
        if constexpr (GRP == GRP_MAX) {
            const bool in0 = jb < a.Ng, in1 = jb + 32 < a.Ng;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pq = pq_s[wr * 64 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h];
                    if (in0 && gg[0] == pq) mx[rt][r] = nanmax(mx[rt][r], acc[rt][0][r]);
                    if (in1 && gg[1] == pq) mx[rt][r] = nanmax(mx[rt][r], acc[rt][1][r]);
                }
        }
        if (TOPK) {
            // candidates: beat the row's current k-th entry; placed in rounds of at most CAP per row, one 32 x 32 block at a time
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int j = jb + 32 * ct;
                    const int rbase = wr * 64 + 32 * rt + 4 * h;
                    unsigned pend = (j < a.Ng) ? 0xFFFFu : 0u;
                    if constexpr (GRP == GRP_MASK) {       // an ignored row (0 < d <= radius) is never a candidate
                        const unsigned R = (unsigned)a.radius;
                        unsigned adm = 0u;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const unsigned d = retr_id_dist(gg[ct], pq_s[rbase + (r & 3) + 8 * (r >> 2)]);
                            adm |= (unsigned)(d == 0u || d > R) << r;
                        }
                        pend &= adm;
                    }
                    while (true) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = rbase + (r & 3) + 8 * (r >> 2);
                            if ((pend >> r) & 1u) {
                                const float sc = acc[rt][ct][r];
                                if (!beats(sc, j, lst_s[row * LSTR + k - 1], lst_i[row * LSTR + k - 1])) {
                                    pend &= ~(1u << r);
                                } else {
                                    const int slot = atomicAdd(&ccount[row], 1);
                                    if (slot < CAP) {
                                        cand_s[row * CAP + slot] = sc;
                                        cand_i[row * CAP + slot] = j;
                                        pend &= ~(1u << r);
                                    }
                                }
                            }
                        }
                        __syncthreads();
                        if (tid < QB) {
                            const int n = min(ccount[tid], CAP);
                            for (int e = 0; e < n; ++e)
                                list_insert(lst_s + tid * LSTR, lst_i + tid * LSTR, k, cand_s[tid * CAP + e], cand_i[tid * CAP + e]);
                            ccount[tid] = 0;
                        }
                        if (!__syncthreads_or(pend != 0)) break;
                    }
                }
        }
    }

    if (RANK) {
        // 32 lanes of a half hold the same rows: add over them (exact: counts < 2^24 in fp32), then over the two column waves
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = half32_sum((float)cnt[rt][r]);
                if (li == 0) part[wc * QB + wr * 64 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h] = (int)v;
            }
        __syncthreads();
        if (tid < QB && q0 + tid < a.Nq) a.cnt[(size_t)slice * a.Nq + q0 + tid] = part[tid] + part[QB + tid];
    }
    if constexpr (NEG) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = half32_sum((float)ncnt[rt][r]);
                if (li == 0) npart[wc * QB + wr * 64 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h] = (int)v;
            }
        __syncthreads();
        if (tid < QB && q0 + tid < a.Nq) a.ncnt[(size_t)slice * a.Nq + q0 + tid] = npart[tid] + npart[QB + tid];
    }
    if constexpr (GRP == GRP_MAX) {
        // the 32 lanes of a half hold the same rows: fold over them, then over the two column waves
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = half32_nanmax(mx[rt][r]);
                if (li == 0) pmax[wc * QB + wr * 64 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * h] = v;
            }
        __syncthreads();
        if (tid < QB && q0 + tid < a.Nq) a.smax[(size_t)slice * a.Nq + q0 + tid] = nanmax(pmax[tid], pmax[QB + tid]);
    }
    if (TOPK) {
        __syncthreads();
        for (int e = tid; e < QB * k; e += 256) {
            const int row = e / k, m = e - row * k;
            if (q0 + row < a.Nq) {
                const size_t o = ((size_t)slice * a.Nq + q0 + row) * k + m;
                a.tks[o] = lst_s[row * LSTR + m];
                a.tki[o] = lst_i[row * LSTR + m];
            }
        }
    }
}

// one thread per query: ranks = 1 + the slices' counts (Ng for a NaN positive score); top-k = the slices' lists merged;
// NEG: negatives = the slices' id-only counts, in slice order
template <bool NEG = false>
__global__ __launch_bounds__(64) void retr_finish_kernel(RetrArgs a, int nslices, int* __restrict__ ranks,
                                                         int* __restrict__ topk_idx, float* __restrict__ topk_score) {
    __shared__ float ls[64 * LSTR];
    __shared__ int lj[64 * LSTR];
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Nq) return;
    if constexpr (NEG) {
        int n = 0;
        for (int s = 0; s < nslices; ++s) n += a.ncnt[(size_t)s * a.Nq + q];
        a.negatives[q] = n;
    }
    if (ranks) {
        int n = 0;
        for (int s = 0; s < nslices; ++s) n += a.cnt[(size_t)s * a.Nq + q];
        ranks[q] = isnan(a.spos[q]) ? a.Ng : 1 + n;
    }
    if (topk_idx) {
        const int k = a.k;
        float* l_s = ls + threadIdx.x * LSTR;
        int* l_i = lj + threadIdx.x * LSTR;
        for (int m = 0; m < k; ++m) { l_s[m] = -INFINITY; l_i[m] = INT_MAX; }
        for (int s = 0; s < nslices; ++s) {
            const size_t o = ((size_t)s * a.Nq + q) * k;
            for (int m = 0; m < k; ++m) {
                const float v = a.tks[o + m];
                const int j = a.tki[o + m];
                if (!beats(v, j, l_s[k - 1], l_i[k - 1])) break;     // the slice's list is sorted: the rest cannot enter
                list_insert(l_s, l_i, k, v, j);
            }
        }
        for (int m = 0; m < k; ++m) {
            const bool filled = l_i[m] != INT_MAX;
            topk_idx[(size_t)q * k + m] = filled ? l_i[m] : -1;
            topk_score[(size_t)q * k + m] = filled ? l_s[m] : -INFINITY;
        }
    }
}

// one thread per query: s*(q) = the slices' maxima folded in slice order (NaN: no positive with a number for a score)
__global__ __launch_bounds__(64) void retr_best_kernel(const float* __restrict__ smax, float* __restrict__ spos, int nslices, int Nq) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= Nq) return;
    float v = __builtin_nanf("");
    for (int s = 0; s < nslices; ++s) v = nanmax(v, smax[(size_t)s * Nq + q]);
    spos[q] = v;
}

// masked: one more per-slice count (the id-only count behind `negatives`)
static int64_t retr_ws(const RetrPlan& p, int Nq, int k, bool masked = false) {
    return (int64_t)Nq * (1 + (int64_t)p.nslices * (1 + (masked ? 1 : 0) + 2 * (int64_t)k));
}

static int retr_check_shape(const char* who, int Nq, int Ng, int D, int k, bool masked = false) {
    MM_REQUIRE(Nq >= 1 && Nq <= MM_RETRIEVAL_NMAX && Ng >= 1 && Ng <= MM_RETRIEVAL_NMAX,
               "%s: need 1 <= Nq, Ng <= %d (got Nq=%d Ng=%d)", who, MM_RETRIEVAL_NMAX, Nq, Ng);
    MM_REQUIRE(D >= 4 && D <= 1024 && D % 4 == 0, "%s: D must be a multiple of 4 in [4, 1024] (got %d)", who, D);
    MM_REQUIRE(k >= 0 && k <= MM_RETRIEVAL_KMAX && k <= Ng, "%s: k must be in [0, min(%d, Ng)] (got k=%d, Ng=%d)",
               who, MM_RETRIEVAL_KMAX, k, Ng);
    const int64_t ws = retr_ws(retr_plan(Nq, Ng), Nq, k, masked);
    MM_REQUIRE(ws <= INT_MAX, "%s: workspace of %lld floats overflows int", who, (long long)ws);
    return MM_OK;
}

}  // namespace

extern "C" int mm_retrieval_ws_floats(int Nq, int Ng, int D, int k, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host, "mm_retrieval_ws_floats: null floats_host");
    const int rc = retr_check_shape("mm_retrieval_ws_floats", Nq, Ng, D, k);
    if (rc) return rc;
    *floats_host = (int)retr_ws(retr_plan(Nq, Ng), Nq, k);
    return MM_OK;
}

extern "C" int mm_retrieval(const float* Q, const float* G, const int* pos, int* ranks, int* topk_idx, float* topk_score,
                            float* ws, int Nq, int Ng, int D, int k, hipStream_t stream) {
    MM_REQUIRE(Q && G && ws, "mm_retrieval: null Q, G or ws");
    MM_REQUIRE(ranks || k > 0, "mm_retrieval: nothing to compute (ranks is null and k == 0)");
    MM_REQUIRE(k == 0 || (topk_idx && topk_score), "mm_retrieval: k = %d needs topk_idx and topk_score", k);
    const int rc = retr_check_shape("mm_retrieval", Nq, Ng, D, k);
    if (rc) return rc;
    MM_REQUIRE(pos || !ranks || Nq <= Ng, "mm_retrieval: pos = NULL means pos[q] = q, which needs Nq <= Ng (got Nq=%d Ng=%d)", Nq, Ng);
    MM_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)G % 16) == 0, "mm_retrieval: Q and G must be 16-byte aligned");

    const RetrPlan p = retr_plan(Nq, Ng);
    RetrArgs a = {};
    a.Q = Q; a.G = G; a.pos = pos;
    float* spos = ws;
    int* cnt = reinterpret_cast<int*>(ws + Nq);
    float* tks = ws + Nq + (size_t)p.nslices * Nq;
    int* tki = reinterpret_cast<int*>(tks + (size_t)p.nslices * Nq * k);
    a.spos = spos; a.cnt = cnt; a.tks = tks; a.tki = tki;
    a.Nq = Nq; a.Ng = Ng; a.D = D; a.k = k; a.tps = p.tps; a.ntiles = p.ntiles;

    if (ranks) {
        pos_score_kernel<<<ceil_div(Nq, 32), 64, 0, stream>>>(Q, G, pos, spos, Nq, Ng, D);
        if (int e = mm_check_launch("mm_retrieval: positive scores")) return e;
    }
    const dim3 grid(p.qblocks, p.nslices);
    if (ranks && k > 0) retr_tile_kernel<true, true><<<grid, 256, 0, stream>>>(a);
    else if (ranks) retr_tile_kernel<true, false><<<grid, 256, 0, stream>>>(a);
    else retr_tile_kernel<false, true><<<grid, 256, 0, stream>>>(a);
    if (int e = mm_check_launch("mm_retrieval: tiles")) return e;
    retr_finish_kernel<false><<<ceil_div(Nq, 64), 64, 0, stream>>>(a, p.nslices, ranks, k > 0 ? topk_idx : nullptr, topk_score);
    return mm_check_launch("mm_retrieval: finish");
}

extern "C" int mm_retrieval_grouped_ws_floats(int Nq, int Ng, int D, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host, "mm_retrieval_grouped_ws_floats: null floats_host");
    const int rc = retr_check_shape("mm_retrieval_grouped_ws_floats", Nq, Ng, D, 0);
    if (rc) return rc;
    *floats_host = (int)retr_ws(retr_plan(Nq, Ng), Nq, 0);
    return MM_OK;
}

extern "C" int mm_retrieval_grouped(const float* Q, const float* G, const int* qgid, const int* ggid, int* ranks, float* ws,
                                    int Nq, int Ng, int D, hipStream_t stream) {
    MM_REQUIRE(Q && G && qgid && ggid && ranks && ws, "mm_retrieval_grouped: null argument");
    const int rc = retr_check_shape("mm_retrieval_grouped", Nq, Ng, D, 0);
    if (rc) return rc;
    MM_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)G % 16) == 0, "mm_retrieval_grouped: Q and G must be 16-byte aligned");

    const RetrPlan p = retr_plan(Nq, Ng);
    RetrArgs a = {};
    a.Q = Q; a.G = G; a.qgid = qgid; a.ggid = ggid;
    float* spos = ws;
    // the per-slice maxima and the per-slice counts share one region: retr_best_kernel has read the maxima before the
    // counting sweep writes its counts (stream order)
    a.smax = ws + Nq;
    a.cnt = reinterpret_cast<int*>(ws + Nq);
    a.spos = spos;
    a.Nq = Nq; a.Ng = Ng; a.D = D; a.k = 0; a.tps = p.tps; a.ntiles = p.ntiles;

    const dim3 grid(p.qblocks, p.nslices);
    retr_tile_kernel<false, false, GRP_MAX><<<grid, 256, 0, stream>>>(a);
    if (int e = mm_check_launch("mm_retrieval_grouped: positive maxima")) return e;
    retr_best_kernel<<<ceil_div(Nq, 64), 64, 0, stream>>>(a.smax, spos, p.nslices, Nq);
    if (int e = mm_check_launch("mm_retrieval_grouped: best positive")) return e;
    retr_tile_kernel<true, false, GRP_COUNT><<<grid, 256, 0, stream>>>(a);
    if (int e = mm_check_launch("mm_retrieval_grouped: tiles")) return e;
    retr_finish_kernel<false><<<ceil_div(Nq, 64), 64, 0, stream>>>(a, p.nslices, ranks, nullptr, nullptr);
    return mm_check_launch("mm_retrieval_grouped: finish");
}

extern "C" int mm_retrieval_masked_ws_floats(int Nq, int Ng, int D, int k, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host, "mm_retrieval_masked_ws_floats: null floats_host");
    const int rc = retr_check_shape("mm_retrieval_masked_ws_floats", Nq, Ng, D, k, true);
    if (rc) return rc;
    *floats_host = (int)retr_ws(retr_plan(Nq, Ng), Nq, k, true);
    return MM_OK;
}

namespace {

// the counting sweep of mm_retrieval_masked: RANK and / or TOPK, with or without the id-only count
template <bool NEG>
static void retr_masked_sweep(const RetrArgs& a, bool rank, dim3 grid, hipStream_t stream) {
    if (rank && a.k > 0) retr_tile_kernel<true, true, GRP_MASK, NEG><<<grid, 256, 0, stream>>>(a);
    else if (rank) retr_tile_kernel<true, false, GRP_MASK, NEG><<<grid, 256, 0, stream>>>(a);
    else retr_tile_kernel<false, true, GRP_MASK, NEG><<<grid, 256, 0, stream>>>(a);
}

}  // namespace

extern "C" int mm_retrieval_masked(const float* Q, const float* G, const int* qgid, const int* ggid, int radius, int* ranks,
                                   int* negatives, int* topk_idx, float* topk_score, float* ws, int Nq, int Ng, int D, int k,
                                   hipStream_t stream) {
    MM_REQUIRE(Q && G && qgid && ggid && ws, "mm_retrieval_masked: null Q, G, qgid, ggid or ws");
    MM_REQUIRE(radius >= 0, "mm_retrieval_masked: radius=%d must be >= 0", radius);
    MM_REQUIRE(ranks || k > 0, "mm_retrieval_masked: nothing to compute (ranks is null and k == 0)");
    MM_REQUIRE(k == 0 || (topk_idx && topk_score), "mm_retrieval_masked: k = %d needs topk_idx and topk_score", k);
    const int rc = retr_check_shape("mm_retrieval_masked", Nq, Ng, D, k, true);
    if (rc) return rc;
    MM_REQUIRE(((uintptr_t)Q % 16) == 0 && ((uintptr_t)G % 16) == 0, "mm_retrieval_masked: Q and G must be 16-byte aligned");

    const RetrPlan p = retr_plan(Nq, Ng);
    const size_t per_slice = (size_t)p.nslices * Nq;
    RetrArgs a = {};
    a.Q = Q; a.G = G; a.qgid = qgid; a.ggid = ggid; a.radius = radius;
    // ws: spos [Nq] | maxima, then counts [nslices][Nq] (one region, as mm_retrieval_grouped) | id-only counts [nslices][Nq] |
    // list scores [nslices][Nq][k] | list indices [nslices][Nq][k]
    float* spos = ws;
    a.spos = spos;
    a.smax = ws + Nq;
    a.cnt = reinterpret_cast<int*>(ws + Nq);
    a.ncnt = reinterpret_cast<int*>(ws + Nq + per_slice);
    a.tks = ws + Nq + 2 * per_slice;
    a.tki = reinterpret_cast<int*>(a.tks + per_slice * k);
    a.negatives = negatives;
    a.Nq = Nq; a.Ng = Ng; a.D = D; a.k = k; a.tps = p.tps; a.ntiles = p.ntiles;

    const dim3 grid(p.qblocks, p.nslices);
    if (ranks) {
        retr_tile_kernel<false, false, GRP_MAX><<<grid, 256, 0, stream>>>(a);
        if (int e = mm_check_launch("mm_retrieval_masked: positive maxima")) return e;
        retr_best_kernel<<<ceil_div(Nq, 64), 64, 0, stream>>>(a.smax, spos, p.nslices, Nq);
        if (int e = mm_check_launch("mm_retrieval_masked: best positive")) return e;
    }
    if (negatives) retr_masked_sweep<true>(a, ranks != nullptr, grid, stream);
    else retr_masked_sweep<false>(a, ranks != nullptr, grid, stream);
    if (int e = mm_check_launch("mm_retrieval_masked: tiles")) return e;
    if (negatives) retr_finish_kernel<true><<<ceil_div(Nq, 64), 64, 0, stream>>>(a, p.nslices, ranks, k > 0 ? topk_idx : nullptr, topk_score);
    else retr_finish_kernel<false><<<ceil_div(Nq, 64), 64, 0, stream>>>(a, p.nslices, ranks, k > 0 ? topk_idx : nullptr, topk_score);
    return mm_check_launch("mm_retrieval_masked: finish");
}
