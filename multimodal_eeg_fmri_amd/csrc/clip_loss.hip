// The fused batch-pairwise cosine-similarity / symmetric InfoNCE loss of the contrastive bridge with its gradients, for
// plain, for subject-grouped positives and for grouped positives with ignored temporal neighbours (MASKED): one kernel pair,
// six entry points; and the pairwise sigmoid (SigLIP) loss on the same inputs and helpers in the same three modes: two
// kernels, four entry points.  Callers: ops.clip_loss_own_rows*, ops.clip_loss*_ws_floats, ops.sigmoid_loss_own_rows and
// ops.sigmoid_loss_ws_floats (bridge_trainer.py's step, autograd.py's tape).
#include "common.h"

namespace {
// ---------------------------------------------------------------------------
// symmetric InfoNCE over the gathered batch, bit-reproducible (no float atomics).
//   C[r][j] = ze_r . zf_j  (cosines; Bg x Bg),  s = exp(logit_scale)
//   e->f problem = row softmax of s C, f->e problem = column softmax of s C
//   loss_r = 0.5 * (CE(row r, target r) + CE(column r, target r))
// This rank owns rows/columns [row0, row0 + B).  Its step loss is mean_r loss_r over its own r; the
// gradient it needs is that of the SUM over all ranks' losses w.r.t. its own embeddings (what a
// reduce-scatter of every rank's d loss_rank / d z_all would deliver; AdamW applies the 1/world):
//   dL/dC[r][j] = 0.5/B * s * (P_row[r][j] + P_col[r][j] - 2 delta_rj)
//   dze_r = sum_j dL/dC[r][j] zf_j        dzf_r = sum_j dL/dC[j][r] ze_j
// P_col[r][j] needs column j's normaliser, P_row[j][r] row j's: a global dependency, so two launches:
//   clip_lse_kernel  (one workgroup per GLOBAL row r): row r and column r of C -> their log-sum-exp,
//                     the row's loss / top-1 flags / d loss_r / d logit_scale            -> ws[6][Bg]
//   clip_rows_kernel (one workgroup per OWN row): recomputes its row and column of C, forms dL/dC from
//                     ws, writes dz[own row] with plain stores; workgroup 0 also sums the own rows'
//                     scalars in a fixed order into scal[4] = {loss, top1 e->f, top1 f->e, d/d logit_scale}.
// Every sum runs in a fixed order (lane-strided partials, xor-shuffle trees, fixed wave order).
//
// GROUPED: the same InfoNCE with subject-grouped positives (MIL-NCE, "log of the positive mass").  gid[Bg] int32: pairs
// with equal ids are positives of each other; P(r) = {j : gid_j = gid_r} always holds r.
//   l_row(r) = LSE_j(s C[r][j]) - LSE_{j in P(r)}(s C[r][j]),  l_col(r) the same over column r,  loss_r = 0.5 (l_row + l_col)
//   dL/dC[r][j] = 0.5/B * s * (P_row + P_col - [gid_r = gid_j] (Q_row + Q_col))[r][j]
// Q = the softmax restricted to the positive set: Q_row[r][j] = exp(s C[r][j] - LSE_P(row r)), Q_col[r][j] =
// exp(s C[r][j] - LSE_P(column j)).  Same two launches and rules as above; ws[8][Bg] = the six rows of the ungrouped
// layout (row / column LSE, loss, top-1 flags, d loss / d logit_scale) + the positive-set LSE of every row and column.
// With all-distinct ids every positive-set LSE is s C[r][r] + log 1 and the result is the ungrouped one (in exact
// arithmetic: the ungrouped instantiation keeps its own formulas).  gid is the LAST kernel argument: the ungrouped
// instantiation never reads it (null there), and its other arguments keep their offsets.
//
// MASKED: the ids are positions on a timeline and a third relation joins positive and negative.  With the radius R >= 0 and
// d = |gid_j - gid_r| (as an unsigned difference: INT_MIN and INT_MAX are 2^32 - 1 apart, see clip_id_dist):
//   d == 0 positive (P(r), as GROUPED)      0 < d <= R ignored      d > R negative      A(r) = {j : d == 0 or d > R}
//   l_row(r) = LSE_{j in A(r)}(s C[r][j]) - LSE_{j in P(r)}(s C[r][j]),  l_col(r) the same over column r
//   dL/dC[r][j] = 0.5/B * s * ([j in A(r)] (P_row + P_col) - [d == 0] (Q_row + Q_col))[r][j]
// P_row / P_col normalised over the admitted sets (the relation is symmetric: j in A(r) <=> r in A(j), so P_col[r][j] is
// only ever formed for a member of column j's sum).  An ignored key takes no part in any maximum, sum or top-1 test and its
// coefficient is stored as 0.f, not computed.  ws[11][Bg]: the eight rows of GROUPED with the admitted-set maximum / LSE in
// place of the all-keys one + one flag per row, 1.f when the row admits no negative (A = P; the relation is symmetric, so
// the flag serves row and column, and every member of P(r) carries it too) + l_row and l_col of every row.  A flagged
// row's loss, d / d logit_scale and every coefficient are STORED as 0.f: LSE_A - LSE_P evaluated in fp32 is only 0 to
// rounding (the compiler contracts s C - LSE into an FMA at some uses and not at others), the
// contract asks for exactly 0.  The same cancellation is kept out of a trained row's positives and of d / d logit_scale
// (see the two comments in the kernels): ignoring the near neighbours leaves rows whose admitted negatives are all far.
// The radius follows gid as the last kernel argument (unread in the other two modes).
// ---------------------------------------------------------------------------
enum { CLIP_PLAIN = 0, CLIP_GROUPED = 1, CLIP_MASKED = 2 };
// |a - b| of two int32 ids in [0, 2^32): the unsigned difference of the larger and the smaller cannot wrap
__device__ __forceinline__ unsigned clip_id_dist(int a, int b) {
    return a >= b ? (unsigned)a - (unsigned)b : (unsigned)b - (unsigned)a;
}
__device__ __forceinline__ bool clip_ignored(int a, int b, int radius) {
    const unsigned d = clip_id_dist(a, b);
    return d != 0u && d <= (unsigned)radius;
}
struct ClipShared {
    float *qe, *qf, *cr, *cc, *red;
};
__device__ __forceinline__ ClipShared clip_shared(float* sm, int N, int Bg) {
    ClipShared s;
    s.qe = sm; s.qf = sm + N; s.cr = s.qf + N; s.cc = s.cr + Bg; s.red = s.cc + Bg;
    return s;
}
// cr[j] = ze_r . zf_j, cc[j] = ze_j . zf_r for all j (8 lanes per column, float4 strides); returns the
// two maxima in every thread
__device__ __forceinline__ void clip_cosines(const float* __restrict__ z_all, int r, int Bg, int N, const ClipShared& sh,
                                             float& mxr, float& mxc) {
    const int LD = 2 * N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int n = tid; n < N; n += 256) { sh.qe[n] = z_all[(size_t)r * LD + n]; sh.qf[n] = z_all[(size_t)r * LD + N + n]; }
    __syncthreads();
    float a_mx = -INFINITY, c_mx = -INFINITY;
    const int sub = tid & 7, n32 = N & ~31;                // the float4 sweep covers whole 32-element chunks only
    for (int j = tid >> 3; j < Bg; j += 32) {
        float a = 0.f, c = 0.f;
        const float* re = z_all + (size_t)j * LD;
        const float* rf = re + N;
        for (int n = sub * 4; n < n32; n += 32) {
            const float4 vf = *reinterpret_cast<const float4*>(rf + n);
            const float4 ve = *reinterpret_cast<const float4*>(re + n);
            a += sh.qe[n] * vf.x + sh.qe[n + 1] * vf.y + sh.qe[n + 2] * vf.z + sh.qe[n + 3] * vf.w;
            c += sh.qf[n] * ve.x + sh.qf[n + 1] * ve.y + sh.qf[n + 2] * ve.z + sh.qf[n + 3] * ve.w;
        }
        for (int n = n32 + sub; n < N; n += 8) { a += sh.qe[n] * rf[n]; c += sh.qf[n] * re[n]; }   // N % 32 tail
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
        if (sub == 0) { sh.cr[j] = a; sh.cc[j] = c; }
        a_mx = fmaxf(a_mx, a); c_mx = fmaxf(c_mx, c);
    }
    a_mx = wave_max(a_mx); c_mx = wave_max(c_mx);
    if (lane == 0) { sh.red[wave] = a_mx; sh.red[4 + wave] = c_mx; }
    __syncthreads();
    mxr = fmaxf(fmaxf(sh.red[0], sh.red[1]), fmaxf(sh.red[2], sh.red[3]));
    mxc = fmaxf(fmaxf(sh.red[4], sh.red[5]), fmaxf(sh.red[6], sh.red[7]));
    __syncthreads();
}
// fixed-order workgroup sum / maximum of two values (4 waves)
__device__ __forceinline__ void clip_sum2(float& a, float& c, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum(a); c = wave_sum(c);
    if (lane == 0) { red[wave] = a; red[4 + wave] = c; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    c = (red[4] + red[5]) + (red[6] + red[7]);
    __syncthreads();
}
__device__ __forceinline__ void clip_max2(float& a, float& c, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_max(a); c = wave_max(c);
    if (lane == 0) { red[wave] = a; red[4 + wave] = c; }
    __syncthreads();
    a = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    c = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    __syncthreads();
}

// one row of dz from the row's dL/dC in LDS: orow[0, N) = dze = sum_j cr[j] zf_j, orow[N, 2N) = dzf = sum_j cc[j] ze_j;
// every sum in ascending j, plain stores
__device__ __forceinline__ void clip_dz_row(const float* __restrict__ z_all, const ClipShared& sh, float* __restrict__ orow,
                                            int Bg, int N) {
    const int LD = 2 * N;
    for (int n = threadIdx.x; n < 2 * N; n += 256) {        // first half: dze (columns of zf), second half: dzf
        const bool first = n < N;
        const float* g = first ? sh.cr : sh.cc;
        const float* col = z_all + (first ? N + n : n - N);
        float acc = 0.f;
        int j = 0;
        for (; j + 8 <= Bg; j += 8) {                       // 8 loads in flight, summed in order
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = col[(size_t)(j + q) * LD];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc += g[j + q] * v[q];
        }
        for (; j < Bg; ++j) acc += g[j] * col[(size_t)j * LD];
        orow[n] = acc;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void clip_lse_kernel(const float* __restrict__ z_all, const float* __restrict__ logit_scale,
                                                       float* __restrict__ ws, int Bg, int N, const int* __restrict__ gid,
                                                       int radius) {
    constexpr bool GROUPED = MODE != CLIP_PLAIN, MASKED = MODE == CLIP_MASKED;
    extern __shared__ float sm[];
    const ClipShared sh = clip_shared(sm, N, Bg);
    const int r = blockIdx.x, tid = threadIdx.x;
    const float s = __expf(logit_scale[0]);
    int gr = 0;
    if constexpr (GROUPED) gr = gid[r];
    float mxr, mxc;
    clip_cosines(z_all, r, Bg, N, sh, mxr, mxc);
    float pmr = -INFINITY, pmc = -INFINITY;                  // maxima over the positive set (the top-1 test and the stable LSE)
    bool no_negative = false;                                // MASKED: A(r) = P(r)
    if constexpr (MASKED) {                                  // and over the admitted set, in place of those over all keys
        mxr = -INFINITY; mxc = -INFINITY;
        float negative = 0.f, none = 0.f;                    // (a flag through the maximum the file already has)
        for (int j = tid; j < Bg; j += 256) {
            const int gj = gid[j];
            if (clip_ignored(gj, gr, radius)) continue;
            mxr = fmaxf(mxr, sh.cr[j]); mxc = fmaxf(mxc, sh.cc[j]);
            if (gj == gr) { pmr = fmaxf(pmr, sh.cr[j]); pmc = fmaxf(pmc, sh.cc[j]); }
            else negative = 1.f;
        }
        clip_max2(negative, none, sh.red);
        no_negative = negative == 0.f;
        clip_max2(mxr, mxc, sh.red);
        clip_max2(pmr, pmc, sh.red);
    } else if constexpr (GROUPED) {
        for (int j = tid; j < Bg; j += 256)
            if (gid[j] == gr) { pmr = fmaxf(pmr, sh.cr[j]); pmc = fmaxf(pmc, sh.cc[j]); }
        clip_max2(pmr, pmc, sh.red);
    }
    float se = 0.f, sf = 0.f, ee = 0.f, ef = 0.f;           // all (MASKED: admitted) columns: sum exp, sum exp * cos
    float qe = 0.f, qf = 0.f, qee = 0.f, qef = 0.f;         // the positive set
    for (int j = tid; j < Bg; j += 256) {
        if constexpr (MASKED) {
            if (clip_ignored(gid[j], gr, radius)) continue;
        }
        const float a = sh.cr[j], c = sh.cc[j];
        const float pa = __expf(s * (a - mxr)), pc = __expf(s * (c - mxc));
        se += pa; sf += pc; ee += pa * a; ef += pc * c;
        if constexpr (GROUPED) {
            if (gid[j] == gr) {
                const float qa = __expf(s * (a - pmr)), qc = __expf(s * (c - pmc));
                qe += qa; qf += qc; qee += qa * a; qef += qc * c;
            }
        }
    }
    clip_sum2(se, sf, sh.red);
    clip_sum2(ee, ef, sh.red);
    if constexpr (GROUPED) {
        clip_sum2(qe, qf, sh.red);
        clip_sum2(qee, qef, sh.red);
    }
    // MASKED: E_A[cos] - E_P[cos] = sum over the admitted NEGATIVES of P_j (cos_j - E_P[cos]) (the positives' terms cancel
    // exactly): small terms summed, not the difference of two means near 1, whose rounding times s exceeds a trained loss
    float ne = 0.f, nf = 0.f;
    if constexpr (MASKED) {
        const float mu_r = qee / qe, mu_c = qef / qf;
        for (int j = tid; j < Bg; j += 256) {
            const int gj = gid[j];
            if (gj == gr || clip_ignored(gj, gr, radius)) continue;
            const float a = sh.cr[j], c = sh.cc[j];
            ne += __expf(s * (a - mxr)) * (a - mu_r); nf += __expf(s * (c - mxc)) * (c - mu_c);
        }
        clip_sum2(ne, nf, sh.red);
    }
    if (tid == 0) {
        // the row's loss = LSE - LSE_P as s (max - max_P) + (log sum - log sum_P), ungrouped s (max - diag) + log sum: never
        // the difference of two numbers near s, whose rounding (4e-6 at s = 100) is the size of a trained model's loss
        if constexpr (GROUPED) {
            const float lg_r = __logf(se), lg_c = __logf(sf), lq_r = __logf(qe), lq_c = __logf(qf);
            const float lsp_r = s * pmr + lq_r, lsp_c = s * pmc + lq_c;
            ws[r] = s * mxr + lg_r;
            ws[Bg + r] = s * mxc + lg_c;
            ws[2 * Bg + r] = 0.5f * ((s * (mxr - pmr) + (lg_r - lq_r)) + (s * (mxc - pmc) + (lg_c - lq_c)));
            ws[3 * Bg + r] = pmr >= mxr ? 1.f : 0.f;         // the best positive reaches the row maximum (a tie counts FOR it)
            ws[4 * Bg + r] = pmc >= mxc ? 1.f : 0.f;
            if constexpr (MASKED) ws[5 * Bg + r] = no_negative ? 0.f : s * 0.5f * (ne / se + nf / sf);
            else ws[5 * Bg + r] = s * 0.5f * ((ee / se - qee / qe) + (ef / sf - qef / qf));
            ws[6 * Bg + r] = lsp_r;
            ws[7 * Bg + r] = lsp_c;
            if constexpr (MASKED) {
                ws[8 * Bg + r] = no_negative ? 1.f : 0.f;
                if (no_negative) ws[2 * Bg + r] = 0.f;
                ws[9 * Bg + r] = s * (mxr - pmr) + (lg_r - lq_r);       // l_row(r), l_col(r): LSE_A - LSE_P without cancellation
                ws[10 * Bg + r] = s * (mxc - pmc) + (lg_c - lq_c);
            }
        } else {
            const float diag = sh.cr[r];
            const float lg_r = __logf(se), lg_c = __logf(sf);
            ws[r] = s * mxr + lg_r;
            ws[Bg + r] = s * mxc + lg_c;
            ws[2 * Bg + r] = 0.5f * ((s * (mxr - diag) + lg_r) + (s * (mxc - sh.cc[r]) + lg_c));
            // top-1: a tie with the row maximum counts FOR the pair (diag >= max).  mm_retrieval's rank counts a tie
            // AGAINST the query (csrc/retrieval.hip), so a collapsed encoder ranks Ng there but scores top-1 = 1 here.
            ws[3 * Bg + r] = diag >= mxr ? 1.f : 0.f;
            ws[4 * Bg + r] = sh.cc[r] >= mxc ? 1.f : 0.f;
            // d loss_r / d logit_scale = s * 0.5 * (E_row[cos] - cos_rr + E_col[cos] - cos_rr)
            ws[5 * Bg + r] = s * 0.5f * ((ee / se - diag) + (ef / sf - sh.cc[r]));
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void clip_rows_kernel(const float* __restrict__ z_all, const float* __restrict__ logit_scale,
                                                        const float* __restrict__ ws, float* __restrict__ scal,
                                                        float* __restrict__ dz, int B, int Bg, int N, int row0,
                                                        const int* __restrict__ gid, int radius) {
    constexpr bool GROUPED = MODE != CLIP_PLAIN, MASKED = MODE == CLIP_MASKED;
    extern __shared__ float sm[];
    const ClipShared sh = clip_shared(sm, N, Bg);
    const int i = blockIdx.x, gi = row0 + i, tid = threadIdx.x, LD = 2 * N;
    const float s = __expf(logit_scale[0]);
    const float invB = 1.f / (float)B;
    if (i == 0 && tid < 64) {                               // the own rows' scalars, summed in a fixed order
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < B; r0 += 64) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (r0 + tid < B) ? ws[(size_t)(2 + q) * Bg + row0 + r0 + tid] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += wave_sum(v[q]);
        }
        // divided, not scaled by a rounded 1/B: the top-1 fractions are count / B rounded once, whatever B is
        if (tid < 4) scal[tid] = (tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : acc[3]) / (float)B;
    }
    if (!dz) return;
    float mxr, mxc;
    clip_cosines(z_all, gi, Bg, N, sh, mxr, mxc);
    // dL/dC[gi][j] -> cr[j],  dL/dC[j][gi] -> cc[j]
    const float lse_rg = ws[gi], lse_cg = ws[Bg + gi];
    float lsp_rg = 0.f, lsp_cg = 0.f;
    int gg = 0;
    if constexpr (GROUPED) { lsp_rg = ws[6 * Bg + gi]; lsp_cg = ws[7 * Bg + gi]; gg = gid[gi]; }
    const float k = 0.5f * invB * s;
    bool no_negative = false;
    float l_rg = 0.f, l_cg = 0.f;
    if constexpr (MASKED) {
        no_negative = ws[8 * Bg + gi] != 0.f;                            // A(gi) = P(gi): uniform over the workgroup
        l_rg = ws[9 * Bg + gi]; l_cg = ws[10 * Bg + gi];
    }
    for (int j = tid; j < Bg; j += 256) {
        if constexpr (MASKED) {                                          // an ignored pair: exactly no gradient, either way;
            if (no_negative || clip_ignored(gid[j], gg, radius)) { sh.cr[j] = 0.f; sh.cc[j] = 0.f; continue; }   // A = P: P - Q = 0
            if (gid[j] == gg) {
                // a positive key: P - Q = Q (exp(-(LSE_A - LSE_P)) - 1) = Q expm1(-l) with l from the lse kernel's split form,
                // not exp(a - LSE_A) - exp(a - LSE_P): two numbers near 1 whose roundings (ulp(s) each) are a trained row's gradient
                const float a = s * sh.cr[j], c = s * sh.cc[j];
                const float ga = __expf(a - lsp_rg) * expm1f(-l_rg) + __expf(a - ws[7 * Bg + j]) * expm1f(-ws[10 * Bg + j]);
                const float gc = __expf(c - ws[6 * Bg + j]) * expm1f(-ws[9 * Bg + j]) + __expf(c - lsp_cg) * expm1f(-l_cg);
                sh.cr[j] = k * ga; sh.cc[j] = k * gc;
                continue;
            }
        }
        const float a = s * sh.cr[j], c = s * sh.cc[j];
        float ga = __expf(a - lse_rg) + __expf(a - ws[Bg + j]);          // P_row[gi][j] + P_col[gi][j]
        float gc = __expf(c - ws[j]) + __expf(c - lse_cg);               // P_row[j][gi] + P_col[j][gi]
        if constexpr (GROUPED && !MASKED) {
            if (gid[j] == gg) {
                ga -= __expf(a - lsp_rg) + __expf(a - ws[7 * Bg + j]);   // Q_row[gi][j] + Q_col[gi][j]
                gc -= __expf(c - ws[6 * Bg + j]) + __expf(c - lsp_cg);   // Q_row[j][gi] + Q_col[j][gi]
            }
        } else if constexpr (!GROUPED) {
            if (j == gi) { ga -= 2.f; gc -= 2.f; }
        }
        sh.cr[j] = k * ga; sh.cc[j] = k * gc;
    }
    __syncthreads();
    clip_dz_row(z_all, sh, dz + (size_t)i * LD, Bg, N);
}

// ---------------------------------------------------------------------------
// pairwise sigmoid loss (Zhai et al., "Sigmoid Loss for Language Image Pre-Training") over the gathered batch: every
// (EEG r, fMRI j) pair is its own binary problem, so no row or column normaliser and no pass over other rows' results.
//   u[r][j] = s C[r][j] + b   (s = exp(logit_scale), b = logit_bias)      y[r][j] = +1 for a positive pair, else -1
//   l[r][j] = softplus(-y u)    loss_r = sum_j l[r][j]    G[r][j] = d l / d C = -y s sigmoid(-y u)
//   dze_r = 1/B sum_j G[r][j] zf_j    dzf_r = 1/B sum_j G[j][r] ze_j    (column r's terms belong to other ranks' rows and
//   are evaluated here from the gathered batch: the sum over ranks of their losses, as for InfoNCE)
// sigmoid_rows_kernel (one workgroup per OWN row gi): row gi and column gi of C, one sweep over j -> G[gi][j], G[j][gi]
//   in LDS and the row's {loss, top-1 e->f, top-1 f->e, d/d logit_scale, d/d logit_bias} -> ws[5][B]; then its dz row.
// sigmoid_sum_kernel (one wave): the own rows' scalars summed in a fixed order -> scal[5].  A second launch and not a
//   last-arriving workgroup: stream order is the only ordering the result then depends on.
// softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigmoid(x) from the same exp(-|x|); expf / log1pf, not the fast forms:
// well-separated pairs have losses of 1e-7 each, which log(1 + e) would quantise to multiples of 2^-24.
// MASKED (relations as for InfoNCE above): an ignored pair has l = 0 and G = 0, stored, not computed, and takes no part in
// the maximum of the top-1 test; everything else, the 1/B included, as GROUPED.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sigmoid_pair(float u, bool pos, float& l, float& dl_du) {
    const float x = pos ? -u : u;                             // -y u
    const float e = expf(-fabsf(x));
    l = fmaxf(x, 0.f) + log1pf(e);
    const float sg = (x >= 0.f ? 1.f : e) / (1.f + e);        // sigmoid(x)
    dl_du = pos ? -sg : sg;                                   // -y sigmoid(-y u)
}

template <int MODE>
__global__ __launch_bounds__(256) void sigmoid_rows_kernel(const float* __restrict__ z_all, const float* __restrict__ logit_scale,
                                                           const float* __restrict__ logit_bias, float* __restrict__ ws,
                                                           float* __restrict__ dz, int B, int Bg, int N, int row0,
                                                           const int* __restrict__ gid, int radius) {
    constexpr bool GROUPED = MODE != CLIP_PLAIN, MASKED = MODE == CLIP_MASKED;
    extern __shared__ float sm[];
    const ClipShared sh = clip_shared(sm, N, Bg);
    const int i = blockIdx.x, gi = row0 + i, tid = threadIdx.x;
    const float s = expf(logit_scale[0]), b = logit_bias[0];
    const float invB = 1.f / (float)B;
    int gg = 0;
    if constexpr (GROUPED) gg = gid[gi];
    float mxr, mxc;
    clip_cosines(z_all, gi, Bg, N, sh, mxr, mxc);
    float pmr = -INFINITY, pmc = -INFINITY;                  // maxima over the positive set (the top-1 test, as for InfoNCE)
    if constexpr (MASKED) {                                  // and over the admitted set, in place of those over all keys
        mxr = -INFINITY; mxc = -INFINITY;
        for (int j = tid; j < Bg; j += 256) {
            const int gj = gid[j];
            if (clip_ignored(gj, gg, radius)) continue;
            mxr = fmaxf(mxr, sh.cr[j]); mxc = fmaxf(mxc, sh.cc[j]);
            if (gj == gg) { pmr = fmaxf(pmr, sh.cr[j]); pmc = fmaxf(pmc, sh.cc[j]); }
        }
        clip_max2(mxr, mxc, sh.red);
        clip_max2(pmr, pmc, sh.red);
    } else if constexpr (GROUPED) {
        for (int j = tid; j < Bg; j += 256)
            if (gid[j] == gg) { pmr = fmaxf(pmr, sh.cr[j]); pmc = fmaxf(pmc, sh.cc[j]); }
        clip_max2(pmr, pmc, sh.red);
    } else {
        pmr = sh.cr[gi]; pmc = sh.cc[gi];
        __syncthreads();                                     // the sweep below overwrites cr / cc
    }
    float loss = 0.f, ds = 0.f, db = 0.f, none = 0.f;
    for (int j = tid; j < Bg; j += 256) {
        if constexpr (MASKED) {                              // an ignored pair: no loss, exactly no gradient, either way
            if (clip_ignored(gid[j], gg, radius)) {
                if (dz) { sh.cr[j] = 0.f; sh.cc[j] = 0.f; }
                continue;
            }
        }
        const float a = sh.cr[j], c = sh.cc[j];
        bool pos;
        if constexpr (GROUPED) pos = gid[j] == gg; else pos = j == gi;
        float l, g;
        sigmoid_pair(s * a + b, pos, l, g);                  // pair (gi, j): the row's loss and scalar gradients
        loss += l; db += g; ds += s * g * a;
        if (dz) {
            sh.cr[j] = invB * s * g;
            sigmoid_pair(s * c + b, pos, l, g);              // pair (j, gi): row j's term in dzf of gi
            sh.cc[j] = invB * s * g;
        }
    }
    clip_sum2(loss, ds, sh.red);                             // (its barriers also publish cr / cc to the dz pass)
    clip_sum2(db, none, sh.red);
    if (tid == 0) {
        ws[i] = loss;
        ws[B + i] = pmr >= mxr ? 1.f : 0.f;                  // the best positive reaches the row maximum (a tie counts FOR it)
        ws[2 * B + i] = pmc >= mxc ? 1.f : 0.f;
        ws[3 * B + i] = ds;
        ws[4 * B + i] = db;
    }
    if (dz) clip_dz_row(z_all, sh, dz + (size_t)i * 2 * N, Bg, N);
}

__global__ __launch_bounds__(64) void sigmoid_sum_kernel(const float* __restrict__ ws, float* __restrict__ scal, int B) {
    const int tid = threadIdx.x;
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < B; r0 += 64) {                     // 64 rows at a time, chunks in ascending order
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = (r0 + tid < B) ? ws[(size_t)q * B + r0 + tid] : 0.f;
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q] += wave_sum(v[q]);
    }
    if (tid < 5)
        scal[tid] = (tid == 0 ? acc[0] : tid == 1 ? acc[1] : tid == 2 ? acc[2] : tid == 3 ? acc[3] : acc[4]) / (float)B;
}
}  // namespace

extern "C" {
// floats-per-Bg rows of the loss workspace: the only place the count is written (layout: see clip_lse_kernel)
static int clip_ws_rows(bool grouped, bool masked = false) { return masked ? 11 : grouped ? 8 : 6; }

// the shape checks of every loss entry point of this file -> the launches' LDS bytes (ClipShared)
static int clip_check_shape(const char* who, int B, int Bg, int N, int row0, size_t* lds) {
    MM_REQUIRE(B > 0 && Bg >= B && row0 >= 0 && row0 + B <= Bg && N > 0, "%s: B=%d Bg=%d row0=%d", who, B, Bg, row0);
    MM_REQUIRE(N % 4 == 0, "%s: N=%d must be a multiple of 4 (16-byte row loads)", who, N);
    *lds = (size_t)(2 * N + 2 * Bg + 32) * sizeof(float);
    MM_REQUIRE(*lds <= 64 * 1024, "%s: N/Bg too large for LDS", who);
    return 0;
}

// the checks and the two launches of the three InfoNCE entry points; gid = nullptr: the ungrouped loss, radius < 0: no
// ignore relation (the grouped loss), radius >= 0: the masked one
static int clip_loss_launch(const char* who, const float* z_all, const int* gid, const float* logit_scale, float* scal4,
                            float* dz_local, float* ws, int B, int Bg, int N, int row0, int radius, hipStream_t st) {
    size_t lds;
    int rc = clip_check_shape(who, B, Bg, N, row0, &lds);
    if (rc) return rc;
    const auto lse = !gid ? clip_lse_kernel<CLIP_PLAIN> : radius < 0 ? clip_lse_kernel<CLIP_GROUPED> : clip_lse_kernel<CLIP_MASKED>;
    const auto rows = !gid ? clip_rows_kernel<CLIP_PLAIN> : radius < 0 ? clip_rows_kernel<CLIP_GROUPED> : clip_rows_kernel<CLIP_MASKED>;
    hipLaunchKernelGGL(lse, dim3(Bg), dim3(256), lds, st, z_all, logit_scale, ws, Bg, N, gid, radius);
    char what[64];
    snprintf(what, sizeof what, "%s(lse)", who);
    rc = mm_check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(rows, dim3(B), dim3(256), lds, st, z_all, logit_scale, ws, scal4, dz_local, B, Bg, N, row0, gid, radius);
    snprintf(what, sizeof what, "%s(rows)", who);
    return mm_check_launch(what);
}

int mm_clip_loss_ws_floats(int B, int Bg, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host && B > 0 && Bg >= B, "clip_loss_ws_floats: bad args");
    *floats_host = clip_ws_rows(false) * Bg;
    return 0;
}

int mm_clip_loss_own_rows(const float* z_all, const float* logit_scale, float* scal4, float* dz_local, float* ws, int B,
                          int Bg, int N, int row0, hipStream_t st) {
    MM_REQUIRE(z_all && logit_scale && scal4 && ws, "clip_loss_own_rows: null");
    return clip_loss_launch("clip_loss_own_rows", z_all, nullptr, logit_scale, scal4, dz_local, ws, B, Bg, N, row0, -1, st);
}

int mm_clip_loss_grouped_ws_floats(int B, int Bg, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host && B > 0 && Bg >= B, "clip_loss_grouped_ws_floats: bad args");
    *floats_host = clip_ws_rows(true) * Bg;
    return 0;
}

int mm_clip_loss_own_rows_grouped(const float* z_all, const int* gid_all, const float* logit_scale, float* scal4, float* dz_local,
                                  float* ws, int B, int Bg, int N, int row0, hipStream_t st) {
    MM_REQUIRE(z_all && gid_all && logit_scale && scal4 && ws, "clip_loss_own_rows_grouped: null");
    return clip_loss_launch("clip_loss_own_rows_grouped", z_all, gid_all, logit_scale, scal4, dz_local, ws, B, Bg, N, row0, -1, st);
}

int mm_clip_loss_masked_ws_floats(int B, int Bg, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host && B > 0 && Bg >= B, "clip_loss_masked_ws_floats: bad args");
    *floats_host = clip_ws_rows(true, true) * Bg;
    return 0;
}

int mm_clip_loss_own_rows_masked(const float* z_all, const int* gid_all, const float* logit_scale, float* scal4, float* dz_local,
                                 float* ws, int B, int Bg, int N, int row0, int radius, hipStream_t st) {
    MM_REQUIRE(z_all && gid_all && logit_scale && scal4 && ws, "clip_loss_own_rows_masked: null");
    MM_REQUIRE(radius >= 0, "clip_loss_own_rows_masked: radius=%d must be >= 0", radius);
    return clip_loss_launch("clip_loss_own_rows_masked", z_all, gid_all, logit_scale, scal4, dz_local, ws, B, Bg, N, row0, radius, st);
}

int mm_sigmoid_loss_ws_floats(int B, int Bg, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host && B > 0 && Bg >= B, "sigmoid_loss_ws_floats: bad args");
    *floats_host = 5 * B;                                    // layout: see sigmoid_rows_kernel
    return 0;
}

// the shape checks and the two launches of both sigmoid entry points; gid / radius as for clip_loss_launch
static int sigmoid_loss_launch(const char* who, const float* z_all, const int* gid, const float* logit_scale,
                               const float* logit_bias, float* scal5, float* dz_local, float* ws, int B, int Bg, int N, int row0,
                               int radius, hipStream_t st) {
    size_t lds;
    int rc = clip_check_shape(who, B, Bg, N, row0, &lds);
    if (rc) return rc;
    const auto rows = !gid ? sigmoid_rows_kernel<CLIP_PLAIN> : radius < 0 ? sigmoid_rows_kernel<CLIP_GROUPED> : sigmoid_rows_kernel<CLIP_MASKED>;
    hipLaunchKernelGGL(rows, dim3(B), dim3(256), lds, st, z_all, logit_scale, logit_bias, ws, dz_local, B, Bg, N, row0, gid, radius);
    char what[64];
    snprintf(what, sizeof what, "%s(rows)", who);
    rc = mm_check_launch(what);
    if (rc) return rc;
    hipLaunchKernelGGL(sigmoid_sum_kernel, dim3(1), dim3(64), 0, st, ws, scal5, B);
    snprintf(what, sizeof what, "%s(sum)", who);
    return mm_check_launch(what);
}

int mm_sigmoid_loss_own_rows(const float* z_all, const int* gid_all, const float* logit_scale, const float* logit_bias,
                             float* scal5, float* dz_local, float* ws, int B, int Bg, int N, int row0, hipStream_t st) {
    MM_REQUIRE(z_all && logit_scale && logit_bias && scal5 && ws, "sigmoid_loss_own_rows: null");
    return sigmoid_loss_launch("sigmoid_loss_own_rows", z_all, gid_all, logit_scale, logit_bias, scal5, dz_local, ws, B, Bg, N,
                               row0, -1, st);
}

int mm_sigmoid_loss_masked_ws_floats(int B, int Bg, int* floats_host, hipStream_t) {
    MM_REQUIRE(floats_host && B > 0 && Bg >= B, "sigmoid_loss_masked_ws_floats: bad args");
    *floats_host = 5 * B;                                    // the layout of mm_sigmoid_loss_ws_floats
    return 0;
}

int mm_sigmoid_loss_own_rows_masked(const float* z_all, const int* gid_all, const float* logit_scale, const float* logit_bias,
                                    float* scal5, float* dz_local, float* ws, int B, int Bg, int N, int row0, int radius,
                                    hipStream_t st) {
    MM_REQUIRE(z_all && gid_all && logit_scale && logit_bias && scal5 && ws, "sigmoid_loss_own_rows_masked: null");
    MM_REQUIRE(radius >= 0, "sigmoid_loss_own_rows_masked: radius=%d must be >= 0", radius);
    return sigmoid_loss_launch("sigmoid_loss_own_rows_masked", z_all, gid_all, logit_scale, logit_bias, scal5, dz_local, ws, B,
                               Bg, N, row0, radius, st);
}
}  // extern "C"
