// What the forward kernel and the fused transformer-row kernels of igemm1d.hip share: the launch argument structs, the
// epilogue feature masks, the epilogues that run on a finished C tile in LDS, the second GEMM behind them, and the host
// functions that check an entry point's arguments and fill a ConvArgs (the caller launches).
// Everything lives in the including file's anonymous namespace.
#pragma once
#include "common.h"

namespace {

constexpr int KPAD = 8;       // +16 B per LDS row
constexpr int A2S = 128 + KPAD; // row stride (elements) of the second GEMM's LDS operand tile (32 rows of 128 bf16)

// BatchNorm-backward reduce pass of the layer BELOW, fused behind the data-gradient GEMM that produces that layer's
// d(out) (epilogue_bn_reduce): the tile's bf16 d(out) values are routed through dropout / pool / act' exactly as
// elementwise.hip's bn_act_bwd_kernel<false> does and summed into the same accumulator workspace
struct BnRed {
    const float* y = nullptr;      // [B][T * pool][N] pre-BatchNorm activations of that layer (nullptr = off)
    const float* out4 = nullptr;   // [4][N] scale, shift, mean, rstd
    float* sums = nullptr;         // [MM_REPL][2][N] workspace (zeroed by the caller): sum dz | sum dz * xhat
    int act = 0, pool = 1, drop_first = 0;
    uint32_t thresh = 0, seed = 0;
    float inv_keep = 1.f;
    const uint32_t* epoch = nullptr;
    uint32_t thresh2 = 0, seed2 = 0;   // the dropout BEHIND the block (PositionalEncoding's), applied to d(out) first:
    float inv_keep2 = 1.f;             // epilogue_ln_bwd only (fp32 d(out))
};

struct EpiArgs {
    const float* scale = nullptr;       // [N] multiply (nullptr = 1)
    const float* shift = nullptr;       // [N] add (bias / folded BN shift) (nullptr = 0)
    const float* residual = nullptr;    // [M][N] fp32 added after activation (nullptr)
    const float* pe = nullptr;          // [>=T][N] fp32 positional table added per t (nullptr)
    float* stats = nullptr;             // [2][N] sum / sum-of-squares of v (atomics) (nullptr)
    float* out_f32 = nullptr;           // [M/pool][N]
    bf16* out_bf16 = nullptr;           // [M/pool][N]
    bf16* out_pre = nullptr;            // [M][N] pre-activation copy (nullptr)
    int act = 0;
    int pool = 1;                       // 1 or 2 (max over adjacent t pairs, after act)
    uint32_t drop_thresh = 0;           // 0 = no dropout
    uint32_t drop_seed = 0;
    float drop_inv_keep = 1.f;
    const uint32_t* drop_epoch = nullptr;
    const bf16* gradz = nullptr;        // backward fusion: v *= act'(gradz[idx]) (nullptr = off)
    int gradz_act = 0;
    // LayerNorm-128 backward fused behind a data-gradient GEMM (ln_x != nullptr): the tile rows are
    // d(LN output); residual = gradient of the skip path; out_f32 / out_bf16 = d(LN input) (bf16 copy
    // carries the consumer's dropout mask); ln_dgb = [REPL][2][128] {dgamma, dbeta} replicas
    const float* ln_x = nullptr;
    const float* ln_stat = nullptr;     // [M][2] mean, rstd
    const float* ln_gamma = nullptr;
    float* ln_dgb = nullptr;
    // mean over groups of pool_rows consecutive output rows, fused: pool_out[row / pool_rows][n] += out * pool_scale
    float* pool_out = nullptr;
    int pool_rows = 0;
    float pool_scale = 0.f;
    // LayerNorm-128 of every finished output row (the NEXT sub-layer's pre-norm), fused: lnf_out bf16 rows,
    // lnf_stat [M][2] mean / rstd (nullable)
    bf16* lnf_out = nullptr;
    float* lnf_stat = nullptr;
    const float* lnf_gamma = nullptr;
    const float* lnf_beta = nullptr;
    float lnf_eps = 0.f;
    BnRed bn;
    // second GEMM behind epilogue_ln_bwd (BM = 32, BN = 128): out2 (M, 128) bf16 = out_bf16 rows @ w2 (a 128 x 128 data-
    // gradient weight image) - the data gradient of the Linear whose output, after dropout, was added to this LayerNorm's
    // input (the attention out-projection under norm2): its operand never leaves the workgroup
    const bf16* w2 = nullptr;
    bf16* out2 = nullptr;
    const float* bias2 = nullptr;   // (n2) added to the second GEMM's columns (nullptr = 0)
    int n2 = 128;                   // its output width: w2 is n2 rows of 128 (a multiple of 128)
    int act2 = 0;                   // activation of the second GEMM's output, then dropout (thresh2 / seed2 / inv_keep2, index
    uint32_t thresh2 = 0, seed2 = 0; float inv_keep2 = 1.f;      // row * n2 + column as a launch of its own would use)
    bf16* pre2 = nullptr;           // pre-activation copy (M, n2) bf16 (nullptr = none)
    int res_rows = 0;            // epilogue_ln_bwd: > 0 = `residual` is (M / res_rows, 128): one row for res_rows consecutive rows
};

struct ConvArgs {
    const bf16* x = nullptr;
    const bf16* w = nullptr;
    int B = 0, T = 0, Cin = 0, Cout = 0, taps = 0, pad = 0;
    EpiArgs e;
    // split-K (few output tiles, long reduction: config #5's 192-channel k = 7 convolution over ~6 000 input channels is
    // 96 tiles of 98 chunks): workgroup z reduces input channels [z * csplit, (z + 1) * csplit) and stores its raw fp32
    // tile to partial[z][b][t][n]; conv1d_splitk_epilogue_kernel adds the slices in order and runs the epilogue
    float* partial = nullptr;
    int csplit = 0;
};

// Epilogue feature mask of a launch: which of epilogue_rows' optional steps it needs, the activation in bits 16-19 and
// the fused activation derivative in bits 20-23.  The kernel is compiled once per tile shape with every step behind a
// run-time test (FEAT = EF_ANY) and once more for each combination the training step uses, with the unused steps and
// the activation switch compiled out: the generic epilogue cost ~2.4 us per million outputs in branches and dead work
// (FFN-1 forward, 8.4 M outputs: 25.7 us generic, 17.5 us specialised).
enum : unsigned { EF_RES = 1, EF_PE = 2, EF_PRE = 4, EF_GRADZ = 8, EF_STATS = 16, EF_POOLOUT = 32, EF_LNF = 64, EF_POOL2 = 128,
                  EF_DROP = 256, EF_SCALE = 512, EF_F32 = 1024, EF_BF16 = 2048, EF_SHIFT = 4096, EF_LNBWD = 8192,
                  EF_BNRED = 16384, EF_BNPOOL2 = 32768 /* bits 24-27: the fused BatchNorm-backward's activation */,
                  EF_GEMM2 = 1u << 28,
                  // the second GEMM's own epilogue: GELU, pre-activation copy, dropout (none of them: bias only)
                  EF_G2ACT = 1u << 29, EF_G2PRE = 1u << 30, EF_G2DROP = 1u << 31, EF_G2FFN1 = EF_G2ACT | EF_G2PRE | EF_G2DROP,
                  EF_ANY = 0xFFFFFFFFu };
// the three activation fields (4 bits each, at these bit offsets): the epilogue's own, the fused activation
// derivative's, the fused BatchNorm-backward's
enum : int { EFA_OUT = 16, EFA_GRADZ = 20, EFA_BN = 24 };
constexpr unsigned ef_act(int act, int field = EFA_OUT) { return (unsigned)act << field; }
static unsigned epi_mask(const EpiArgs& e) {
    return (e.residual ? EF_RES : 0) | (e.pe ? EF_PE : 0) | (e.out_pre ? EF_PRE : 0) | (e.gradz ? EF_GRADZ : 0) | (e.stats ? EF_STATS : 0) |
           (e.pool_out ? EF_POOLOUT : 0) | (e.lnf_out ? EF_LNF : 0) | (e.pool == 2 ? EF_POOL2 : 0) | (e.drop_thresh ? EF_DROP : 0) |
           (e.scale ? EF_SCALE : 0) | (e.out_f32 ? EF_F32 : 0) | (e.out_bf16 ? EF_BF16 : 0) | (e.shift ? EF_SHIFT : 0) | (e.ln_x ? EF_LNBWD : 0) |
           ef_act(e.act) | ef_act(e.gradz ? e.gradz_act : 0, EFA_GRADZ) |
           (e.bn.y ? (EF_BNRED | (e.bn.pool == 2 ? EF_BNPOOL2 : 0) | ef_act(e.bn.act, EFA_BN)) : 0) |
           (e.w2 ? (EF_GEMM2 | (e.act2 ? EF_G2ACT : 0) | (e.pre2 ? EF_G2PRE : 0) | (e.thresh2 ? EF_G2DROP : 0)) : 0);
}
// bytes of the 32 x 128 tile's epilogue LDS: the fp32 C tile and its column sums, then the second GEMM's operand rows
constexpr size_t CT32 = (size_t)(32 * (128 + 4) + 2 * 128) * sizeof(float), A2B = (size_t)32 * A2S * sizeof(bf16);
static_assert(2 * A2B <= CT32, "the second GEMM's two staging tiles fit the dead C tile");

// one optional step of an epilogue: behind its run-time test (FEAT = EF_ANY), else compiled in or out by the launch's mask
#define EF_ON(bit, runtime) (ANY ? (bool)(runtime) : ((FEAT & (bit)) != 0))

// Epilogue through LDS: the accumulator tile is parked as fp32 [BM][BN+4], then
// every thread owns one 4-column group (fixed per thread) and walks rows, so
// residual / positional loads and all stores are 16-byte, row-contiguous.
template <int BM, int BN, unsigned FEAT>
__device__ __forceinline__ void epilogue_rows(const float* Cs, const EpiArgs& e, int tid, int b, int t0, int T,
                                              int n0, int N, float* sstat, bf16* a2 = nullptr) {
    // no implicit FMA contraction in here: which multiply-adds get fused would depend on what a specialisation folds
    // away, and the variants of one op must agree bit for bit (tests compare them); the two intended FMAs are explicit
#pragma clang fp contract(off)
    constexpr bool ANY = FEAT == EF_ANY;
    const int act = ANY ? e.act : (int)((FEAT >> 16) & 15u);
    const int gradz_act = ANY ? e.gradz_act : (int)((FEAT >> 20) & 15u);
    constexpr int LDC = BN + 4;
    constexpr int CG = BN / 4;                 // column groups
    constexpr int RPP = 256 / CG;              // rows per pass
    const int cg = tid % CG, rr = tid / CG;
    const int n = n0 + cg * 4;
    const bool nok = n < N;                    // N % 4 == 0 is required
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nok) {
        if (EF_ON(EF_SCALE, e.scale)) sc = *reinterpret_cast<const float4*>(e.scale + n);
        if (EF_ON(EF_SHIFT, e.shift)) sh = *reinterpret_cast<const float4*>(e.shift + n);
    }
    const float scs[4] = {sc.x, sc.y, sc.z, sc.w}, shs[4] = {sh.x, sh.y, sh.z, sh.w};
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0}, pp[4] = {0, 0, 0, 0};
    const bool drop = EF_ON(EF_DROP, e.drop_thresh);
    const uint32_t dseed = drop ? mm_eff_seed(e.drop_seed, e.drop_epoch) : 0u;
    const int step = ANY ? e.pool : ((FEAT & EF_POOL2) ? 2 : 1);      // rows consumed per item
    const int To = T / step;
    for (int r0 = rr * step; r0 < BM; r0 += RPP * step) {
        float o[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        bool any = false;
        for (int q = 0; q < step; ++q) {
            const int row = r0 + q, t = t0 + row;
            if (t >= T || !nok) continue;
            any = true;
            const float4 a4 = *reinterpret_cast<const float4*>(Cs + row * LDC + cg * 4);
            float v[4] = {a4.x, a4.y, a4.z, a4.w};
            const size_t idx = ((size_t)b * T + t) * N + n;
            float4 res = make_float4(0.f, 0.f, 0.f, 0.f), pe = res;
            if (EF_ON(EF_RES, e.residual)) res = *reinterpret_cast<const float4*>(e.residual + idx);
            if (EF_ON(EF_PE, e.pe)) pe = *reinterpret_cast<const float4*>(e.pe + (size_t)t * N + n);
            const float rs[4] = {res.x, res.y, res.z, res.w}, ps[4] = {pe.x, pe.y, pe.z, pe.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float val = __builtin_fmaf(v[c], scs[c], shs[c]);
                if (EF_ON(EF_STATS, e.stats)) { s1[c] += val; s2[c] = __builtin_fmaf(val, val, s2[c]); }
                v[c] = val;
            }
            if (EF_ON(EF_PRE, e.out_pre)) {
                bf16x4 pv = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                *reinterpret_cast<bf16x4*>(e.out_pre + idx) = pv;
            }
            if (EF_ON(EF_GRADZ, e.gradz)) {
                const bf16x4 zz = *reinterpret_cast<const bf16x4*>(e.gradz + idx);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] *= act_grad((float)zz[c], gradz_act);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float val = apply_act(v[c], act);
                const float rp = rs[c] + ps[c];
                if (drop) val = __builtin_fmaf(val, dropout_scale(dseed, (uint32_t)(idx + c), e.drop_thresh, e.drop_inv_keep), rp);
                else val += rp;
                o[c] = fmaxf(o[c], val);
            }
        }
        if (!any) continue;
        if (EF_ON(EF_POOLOUT, e.pool_out))
#pragma unroll
            for (int c = 0; c < 4; ++c) pp[c] += o[c];
        const int t = t0 + r0;
        const size_t oi = ((size_t)b * To + t / step) * N + n;
        if constexpr (BN == 128) {
            if (EF_ON(EF_LNF, e.lnf_out)) {                       // host guarantees N == 128, pool == 1: 32 lanes hold this row
                float sm = (o[0] + o[1]) + (o[2] + o[3]);
                sm = half32_sum(sm);
                const float mean = sm * (1.f / 128.f);
                const float d0 = o[0] - mean, d1 = o[1] - mean, d2 = o[2] - mean, d3 = o[3] - mean;
                float sq = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                sq = half32_sum(sq);
                const float rstd = rsqrtf(sq * (1.f / 128.f) + e.lnf_eps);
                const float4 g4 = *reinterpret_cast<const float4*>(e.lnf_gamma + n);
                const float4 b4 = *reinterpret_cast<const float4*>(e.lnf_beta + n);
                bf16x4 hv = {(bf16)(d0 * rstd * g4.x + b4.x), (bf16)(d1 * rstd * g4.y + b4.y),
                             (bf16)(d2 * rstd * g4.z + b4.z), (bf16)(d3 * rstd * g4.w + b4.w)};
                *reinterpret_cast<bf16x4*>(e.lnf_out + oi) = hv;
                if (a2) *reinterpret_cast<bf16x4*>(a2 + r0 * A2S + cg * 4) = hv;              // operand tile of the second GEMM
                if (e.lnf_stat && cg == 0) {
                    const size_t m = (size_t)b * To + t;
                    e.lnf_stat[2 * m] = mean; e.lnf_stat[2 * m + 1] = rstd;
                }
            }
        }
        if (EF_ON(EF_F32, e.out_f32)) *reinterpret_cast<float4*>(e.out_f32 + oi) = make_float4(o[0], o[1], o[2], o[3]);
        if (EF_ON(EF_BF16, e.out_bf16)) {
            bf16x4 ov = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
            *reinterpret_cast<bf16x4*>(e.out_bf16 + oi) = ov;
        }
    }
    if (EF_ON(EF_POOLOUT, e.pool_out)) {
        // fused mean over rows (all rows of this tile belong to one group: pool_rows % BM == 0, host-checked)
        __syncthreads();
        float* part = const_cast<float*>(Cs);              // [RPP][BN]
        *reinterpret_cast<float4*>(part + rr * BN + cg * 4) = make_float4(pp[0], pp[1], pp[2], pp[3]);
        __syncthreads();
        const size_t grp = ((size_t)b * T + t0) / e.pool_rows;
        for (int i = tid; i < BN; i += 256)
            if (n0 + i < N) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < RPP; ++r) s += part[r * BN + i];
                acc_add<MM_ACC_GRAD>(reinterpret_cast<mm_acc_t*>(e.pool_out) + grp * N + n0 + i, s * e.pool_scale);
            }
        if (EF_ON(EF_STATS, e.stats)) __syncthreads();
    }
    if (EF_ON(EF_STATS, e.stats)) {
        // block reduction of the per-thread column sums: plain stores into the (now dead) C tile, then a
        // column walk.  LDS float atomics with RPP-way same-address conflicts cost ~2 us per workgroup.
        __syncthreads();                                   // every thread is done reading Cs
        float* part = const_cast<float*>(Cs);              // [RPP][2][BN]  (RPP * 2 * BN = 2048 floats <= BM * LDC)
        static_assert(RPP * 2 * BN <= BM * LDC, "partials fit the C tile");
        *reinterpret_cast<float4*>(part + (rr * 2 + 0) * BN + cg * 4) = make_float4(s1[0], s1[1], s1[2], s1[3]);
        *reinterpret_cast<float4*>(part + (rr * 2 + 1) * BN + cg * 4) = make_float4(s2[0], s2[1], s2[2], s2[3]);
        __syncthreads();
        mm_acc_t* rep = acc_rep(e.stats, blockIdx.x % MM_ACC_REPL, 2 * (size_t)N);
        for (int i = tid; i < 2 * BN; i += 256) {
            const int which = i / BN, col = i % BN;
            if (n0 + col < N) {
                float s = 0.f;
#pragma unroll
                for (int r = 0; r < RPP; ++r) s += part[(r * 2 + which) * BN + col];
                acc_add<MM_ACC_STAT>(&rep[which * N + n0 + col], s);
            }
        }
    }
}

// dgrad GEMM -> bf16 d(out) of the layer below + that layer's BatchNorm-backward reduce pass (host: no scale / shift /
// activation / pooling of this GEMM's own, Cout == the BatchNorm's channel count).  Thread layout as epilogue_rows: one
// 4-column group per thread, BM / RPP rows; the rows' pre-BN values are fetched before the first row is touched.
struct BnDz { int act, pool, drop_first; uint32_t thresh, seed; float inv_keep; };
template <int BM, int BN, unsigned FEAT>
__device__ __forceinline__ void epilogue_bn_reduce(const float* Cs, const EpiArgs& e, int tid, int b, int t0, int T,
                                                   int n0, int N) {
#pragma clang fp contract(off)
    constexpr bool ANY = FEAT == EF_ANY;
    constexpr int LDC = BN + 4, CG = BN / 4, RPP = 256 / CG, NR = BM / RPP;
    const int cg = tid % CG, rr = tid / CG;
    const int n = n0 + cg * 4;
    const bool nok = n < N;
    BnDz bn;
    bn.act = ANY ? e.bn.act : (int)((FEAT >> 24) & 15u);
    bn.pool = ANY ? e.bn.pool : ((FEAT & EF_BNPOOL2) ? 2 : 1);
    bn.drop_first = e.bn.drop_first; bn.thresh = e.bn.thresh; bn.inv_keep = e.bn.inv_keep;
    bn.seed = mm_eff_seed(e.bn.seed, e.bn.epoch);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 y0[NR], y1[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int t = t0 + rr + k * RPP;
        const bool ok = nok && t < T;                    // rows / columns outside the tensor read element 0 (unused below)
        const size_t in0 = ok ? ((size_t)b * T + t) * bn.pool * N + n : 0;
        y0[k] = *reinterpret_cast<const float4*>(e.bn.y + in0);
        y1[k] = *reinterpret_cast<const float4*>(e.bn.y + in0 + (bn.pool == 2 ? N : 0));
    }
    float4 c4[4] = {z4, z4, z4, z4};
    if (nok)
#pragma unroll
        for (int q = 0; q < 4; ++q) c4[q] = *reinterpret_cast<const float4*>(e.bn.out4 + (size_t)q * N + n);
    const float scs[4] = {c4[0].x, c4[0].y, c4[0].z, c4[0].w}, shs[4] = {c4[1].x, c4[1].y, c4[1].z, c4[1].w};
    const float mus[4] = {c4[2].x, c4[2].y, c4[2].z, c4[2].w}, rss[4] = {c4[3].x, c4[3].y, c4[3].z, c4[3].w};
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int row = rr + k * RPP, t = t0 + row;
        if (!nok || t >= T) continue;
        const float4 a4 = *reinterpret_cast<const float4*>(Cs + row * LDC + cg * 4);
        const size_t oi = ((size_t)b * T + t) * N + n;
        const size_t in0 = ((size_t)b * T + t) * bn.pool * N + n;
        const bf16x4 ov = {(bf16)a4.x, (bf16)a4.y, (bf16)a4.z, (bf16)a4.w};
        *reinterpret_cast<bf16x4*>(e.out_bf16 + oi) = ov;
        const float y0s[4] = {y0[k].x, y0[k].y, y0[k].z, y0[k].w}, y1s[4] = {y1[k].x, y1[k].y, y1[k].z, y1[k].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float d0, d1;                                   // the stand-alone pass reads the bf16 d(out): so does this one
            bn_dz_pair<-1, 0>(bn, y0s[c], y1s[c], scs[c], shs[c], (float)ov[c], (uint32_t)(in0 + c), (uint32_t)(in0 + N + c),
                              (uint32_t)(oi + c), d0, d1);
            const float xh0 = (y0s[c] - mus[c]) * rss[c], xh1 = (y1s[c] - mus[c]) * rss[c];
            s1[c] += d0 + d1;
            s2[c] += d0 * xh0 + d1 * xh1;
        }
    }
    __syncthreads();                                       // every thread is done reading Cs
    float* part = const_cast<float*>(Cs);                  // [RPP][2][BN]
    static_assert(RPP * 2 * BN <= BM * LDC, "partials fit the C tile");
    *reinterpret_cast<float4*>(part + (rr * 2 + 0) * BN + cg * 4) = make_float4(s1[0], s1[1], s1[2], s1[3]);
    *reinterpret_cast<float4*>(part + (rr * 2 + 1) * BN + cg * 4) = make_float4(s2[0], s2[1], s2[2], s2[3]);
    __syncthreads();
    mm_acc_t* rep = acc_rep(e.bn.sums, blockIdx.x % MM_ACC_REPL, 2 * (size_t)N);
    for (int i = tid; i < 2 * BN; i += 256) {
        const int which = i / BN, col = i % BN;
        if (n0 + col < N) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < RPP; ++r) s += part[(r * 2 + which) * BN + col];
            acc_add<MM_ACC_GRAD>(&rep[which * N + n0 + col], s);
        }
    }
}

// dgrad GEMM -> LayerNorm backward in one pass (N == BN == 128, T % BM == 0: checked on the host).
// 32 lanes own one row (4 columns each): the two row means are 5-step half-wave shuffles; every
// thread keeps its 4 columns' dgamma / dbeta partial sums over the rows it walks.
template <int BM, int BN, unsigned FEAT>
__device__ __forceinline__ void epilogue_ln_bwd(const float* Cs, const EpiArgs& e, int tid, int b, int t0, int T,
                                                float* sstat, bf16* a2 = nullptr) {
    static_assert(BN == 128, "LayerNorm-128 epilogue");
    constexpr bool ANY = FEAT == EF_ANY;
    constexpr int LDC = BN + 4;
    const int cg = tid & 31, rr = tid >> 5;
    const float4 gg = *reinterpret_cast<const float4*>(e.ln_gamma + cg * 4);
    const float gam[4] = {gg.x, gg.y, gg.z, gg.w};
    float sh[4] = {0.f, 0.f, 0.f, 0.f};
    if (EF_ON(EF_SHIFT, e.shift)) {
        const float4 s4 = *reinterpret_cast<const float4*>(e.shift + cg * 4);
        sh[0] = s4.x; sh[1] = s4.y; sh[2] = s4.z; sh[3] = s4.w;
    }
    const bool drop = EF_ON(EF_DROP, e.drop_thresh);
    const uint32_t dseed = drop ? mm_eff_seed(e.drop_seed, e.drop_epoch) : 0u;
    float ag[4] = {0, 0, 0, 0}, ab[4] = {0, 0, 0, 0};
    // BatchNorm-backward reduce of the conv block whose output (+ positional table, dropout) IS this LayerNorm's input:
    // the rows leaving here are that block's fp32 d(out) (EnhancedERPEncoder: conv block 3 under the first transformer block)
    const bool bnred = EF_ON(EF_BNRED, e.bn.y);
    BnDz bn;
    bn.act = ANY ? e.bn.act : (int)((FEAT >> 24) & 15u);
    bn.pool = 1; bn.drop_first = 1; bn.thresh = e.bn.thresh; bn.inv_keep = e.bn.inv_keep;
    bn.seed = bnred ? mm_eff_seed(e.bn.seed, e.bn.epoch) : 0u;
    const uint32_t bseed2 = bnred ? mm_eff_seed(e.bn.seed2, e.bn.epoch) : 0u;
    float4 by[BM / 8];
    float bsc[4] = {0, 0, 0, 0}, bsh[4] = {0, 0, 0, 0}, bmu[4] = {0, 0, 0, 0}, brs[4] = {0, 0, 0, 0};
    float t1[4] = {0, 0, 0, 0}, t2[4] = {0, 0, 0, 0};
    if (bnred) {
#pragma unroll
        for (int k = 0; k < BM / 8; ++k)
            by[k] = *reinterpret_cast<const float4*>(e.bn.y + ((size_t)b * T + t0 + rr + 8 * k) * 128 + cg * 4);
        const float4 c0 = *reinterpret_cast<const float4*>(e.bn.out4 + cg * 4), c1 = *reinterpret_cast<const float4*>(e.bn.out4 + 128 + cg * 4);
        const float4 c2 = *reinterpret_cast<const float4*>(e.bn.out4 + 256 + cg * 4), c3 = *reinterpret_cast<const float4*>(e.bn.out4 + 384 + cg * 4);
        bsc[0] = c0.x; bsc[1] = c0.y; bsc[2] = c0.z; bsc[3] = c0.w; bsh[0] = c1.x; bsh[1] = c1.y; bsh[2] = c1.z; bsh[3] = c1.w;
        bmu[0] = c2.x; bmu[1] = c2.y; bmu[2] = c2.z; bmu[3] = c2.w; brs[0] = c3.x; brs[1] = c3.y; brs[2] = c3.z; brs[3] = c3.w;
    }
#pragma unroll
    for (int row = rr; row < BM; row += 8) {
        const size_t m = (size_t)b * T + t0 + row;
        const size_t base = m * 128 + cg * 4;
        const float4 a4 = *reinterpret_cast<const float4*>(Cs + row * LDC + cg * 4);
        const float4 xv = *reinterpret_cast<const float4*>(e.ln_x + base);
        float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (EF_ON(EF_RES, e.residual))
            rv = *reinterpret_cast<const float4*>(e.residual + (e.res_rows ? (size_t)((unsigned)m / (unsigned)e.res_rows) * 128 + cg * 4 : base));
        const float2 st = *reinterpret_cast<const float2*>(e.ln_stat + 2 * m);
        const float dyv[4] = {a4.x + sh[0], a4.y + sh[1], a4.z + sh[2], a4.w + sh[3]};
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, rs[4] = {rv.x, rv.y, rv.z, rv.w};
        float xh[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xh[c] = (xs[c] - st.x) * st.y;
            const float gh = dyv[c] * gam[c];
            s1 += gh; s2 += gh * xh[c];
            ag[c] += dyv[c] * xh[c]; ab[c] += dyv[c];
        }
        s1 = half32_sum(s1); s2 = half32_sum(s2);
        s1 *= (1.f / 128.f); s2 *= (1.f / 128.f);
        float o4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) o4[c] = st.y * (dyv[c] * gam[c] - s1 - xh[c] * s2) + rs[c];
        if (EF_ON(EF_F32, e.out_f32)) *reinterpret_cast<float4*>(e.out_f32 + base) = make_float4(o4[0], o4[1], o4[2], o4[3]);
        if (EF_ON(EF_BF16, e.out_bf16)) {
            bf16x4 ob;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                ob[c] = (bf16)(drop ? o4[c] * dropout_scale(dseed, (uint32_t)(base + c), e.drop_thresh, e.drop_inv_keep)
                                             : o4[c]);
            *reinterpret_cast<bf16x4*>(e.out_bf16 + base) = ob;
            if (a2) *reinterpret_cast<bf16x4*>(a2 + row * A2S + cg * 4) = ob;
        }
        if (bnred) {
            const float4 yv = by[(row - rr) / 8];
            const float ys[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float g = o4[c];
                if (e.bn.thresh2) g *= dropout_scale(bseed2, (uint32_t)(base + c), e.bn.thresh2, e.bn.inv_keep2);
                float d0, d1;
                bn_dz_pair<-1, 1>(bn, ys[c], ys[c], bsc[c], bsh[c], g, (uint32_t)(base + c), 0u, 0u, d0, d1);
                t1[c] += d0;
                t2[c] += d0 * ((ys[c] - bmu[c]) * brs[c]);
            }
        }
    }
    if (bnred) {
        __syncthreads();                                   // every thread is done reading Cs
        float* part = const_cast<float*>(Cs);              // [8 row groups][sum dz 128 | sum dz xhat 128]
        *reinterpret_cast<float4*>(part + rr * 256 + cg * 4) = make_float4(t1[0], t1[1], t1[2], t1[3]);
        *reinterpret_cast<float4*>(part + rr * 256 + 128 + cg * 4) = make_float4(t2[0], t2[1], t2[2], t2[3]);
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s += part[r * 256 + tid];
        acc_add<MM_ACC_GRAD>(acc_rep(e.bn.sums, blockIdx.x % MM_ACC_REPL, 256) + tid, s);
    }
    if (e.ln_dgb) {
        __syncthreads();                                   // every thread is done reading Cs
        float* part = const_cast<float*>(Cs);              // [8 row groups][dgamma 128 | dbeta 128]
        static_assert(8 * 256 <= BM * LDC, "partials fit the C tile");
        *reinterpret_cast<float4*>(part + rr * 256 + cg * 4) = make_float4(ag[0], ag[1], ag[2], ag[3]);
        *reinterpret_cast<float4*>(part + rr * 256 + 128 + cg * 4) = make_float4(ab[0], ab[1], ab[2], ab[3]);
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s += part[r * 256 + tid];
        acc_add<MM_ACC_GRAD>(acc_rep(e.ln_dgb, blockIdx.x % MM_ACC_REPL, 256) + tid, s);
    }
}

// out2[32 rows][n2] = a2[32][128] (bf16 rows this workgroup has just finished, in LDS) x w2 (+ bias2): wave wn owns columns
// 128 j + 32 wn .. of every 128-column group j; B fragments straight from the L2-resident weight image, k ascending as the
// main loop's, fp32 accumulate, one rounding to bf16 - bit-identical to a launch of its own on the same rows.
// The fragments of group j + 1 are requested before the MFMAs of group j.  A finished group is parked in LDS (the MFMA
// layout gives a lane ONE column: straight from the registers the outputs left as 2-byte column stores) and leaves as
// 16-byte stores, 16 lanes to a 256-byte row segment.  The staging tiles are double-buffered, so a group costs one barrier.
//   FEAT   EF_ANY: bias / pre-activation copy / activation / dropout behind run-time tests; otherwise EF_G2ACT (GELU),
//          EF_G2PRE and EF_G2DROP say what is compiled in (none of them: bias only)
//   KEEP   ost is the whole 32 x n2 output tile (row stride n2 + KPAD) and stays in LDS for the caller (out2 may be null:
//          nothing written); otherwise ost is two 32 x A2S staging tiles
//   pst    two 32 x A2S staging tiles of the pre-activation copy (used with pre2 only)
template <unsigned FEAT, bool KEEP>
__device__ __forceinline__ void second_gemm(const bf16* a2, const EpiArgs& e, size_t row0, int tid, int wn, int lr, int lh,
                                            bf16* ost, bf16* pst) {
#pragma clang fp contract(off)
    constexpr bool ANY = FEAT == EF_ANY;
    const int act = ANY ? e.act2 : ((FEAT & EF_G2ACT) ? (int)MM_ACT_GELU : 0);
    const bool pre = ANY ? e.pre2 != nullptr : (FEAT & EF_G2PRE) != 0;
    const bool drop = ANY ? e.thresh2 != 0 : (FEAT & EF_G2DROP) != 0;
    const bool store_out = !KEEP || e.out2 != nullptr;
    const int OS = KEEP ? e.n2 + KPAD : A2S;
    const uint32_t dseed = drop ? mm_eff_seed(e.seed2, e.drop_epoch) : 0u;
    bf16x8 af[8], bnx[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) af[ks] = *reinterpret_cast<const bf16x8*>(a2 + lr * A2S + ks * 16 + lh * 8);
    const bf16* wlane = e.w2 + (size_t)(32 * wn + lr) * 128 + lh * 8;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wlane + ks * 16);
    const int ng = e.n2 / 128;
    for (int j = 0; j < ng; ++j) {
        const int n = 128 * j + 32 * wn + lr;
        bf16x8 bfr[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bfr[ks] = bnx[ks];
        if (j + 1 < ng) {
            const bf16* wrow = wlane + (size_t)(j + 1) * 128 * 128;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wrow + ks * 16);
        }
        const float bias = e.bias2 ? e.bias2[n] : 0.f;
        f32x16 c2;
#pragma unroll
        for (int r = 0; r < 16; ++r) c2[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], bfr[ks], c2, 0, 0, 0);
        bf16* os = KEEP ? ost + 128 * j : ost + (j & 1) * (32 * A2S);
        bf16* ps = pst + (j & 1) * (32 * A2S);
        // bias -> pre-activation copy -> activation -> dropout, the arithmetic of epilogue_rows (FFN-1 forward)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const size_t idx = (row0 + row) * e.n2 + n;
            const float v = e.bias2 ? c2[r] + bias : c2[r];
            if (pre) ps[row * A2S + 32 * wn + lr] = (bf16)v;
            float val = apply_act(v, act);
            if (drop) val = __builtin_fmaf(val, dropout_scale(dseed, (uint32_t)idx, e.thresh2, e.inv_keep2), 0.f);
            os[row * OS + 32 * wn + lr] = (bf16)val;
        }
        if (!store_out && !pre) continue;              // (uniform) the tile only stays in LDS: the caller's barrier covers it
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = q * 16 + (tid >> 4), sg = (tid & 15) * 8;
            const size_t oi = (row0 + row) * e.n2 + 128 * j + sg;
            if (store_out) *reinterpret_cast<uint4*>(e.out2 + oi) = *reinterpret_cast<const uint4*>(os + row * OS + sg);
            if (pre) *reinterpret_cast<uint4*>(e.pre2 + oi) = *reinterpret_cast<const uint4*>(ps + row * A2S + sg);
        }
    }
}

// ------------------------------------------------------------------ host: an entry point's arguments -> ConvArgs
// Each builder checks the arguments, fills `a` (a fresh ConvArgs) and launches nothing.
static int conv1d_fwd_args(ConvArgs& a, const void* x, const void* w, int B, int T, int Cin, int Cout, int taps, int pad,
                           const float* scale, const float* shift, int act, const float* residual, const float* pe,
                           int pool, float* stats, float* out_f32, void* out_bf16, void* out_pre,
                           float drop_p, uint32_t drop_seed, const uint32_t* seed_epoch, const void* gradz, int gradz_act) {
    MM_REQUIRE(x && w, "conv1d_fwd: null operand");
    MM_REQUIRE(B > 0 && T > 0 && Cout > 0 && taps >= 1 && taps <= 9 && pad >= 0 && pad < taps, "conv1d_fwd: bad dims");
    MM_REQUIRE(Cin > 0 && Cin % 16 == 0, "conv1d_fwd: Cin=%d must be a multiple of 16", Cin);
    MM_REQUIRE(pool == 1 || (pool == 2 && T % 2 == 0), "conv1d_fwd: pool=%d T=%d", pool, T);
    MM_REQUIRE(out_f32 || out_bf16 || out_pre, "conv1d_fwd: no output");
    MM_REQUIRE(Cout % 4 == 0, "conv1d_fwd: Cout=%d must be a multiple of 4", Cout);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "conv1d_fwd: drop_p");
    a.x = (const bf16*)x; a.w = (const bf16*)w;
    a.B = B; a.T = T; a.Cin = Cin; a.Cout = Cout; a.taps = taps; a.pad = pad;
    a.e.scale = scale; a.e.shift = shift; a.e.residual = residual; a.e.pe = pe; a.e.stats = stats;
    a.e.out_f32 = out_f32; a.e.out_bf16 = (bf16*)out_bf16; a.e.out_pre = (bf16*)out_pre;
    a.e.act = act; a.e.pool = pool;
    const DropH d = mm_drop(drop_p);
    a.e.drop_thresh = d.thresh; a.e.drop_inv_keep = d.inv_keep; a.e.drop_seed = drop_seed; a.e.drop_epoch = seed_epoch;
    a.e.gradz = (const bf16*)gradz; a.e.gradz_act = gradz_act;
    return 0;
}

// y = dropout(x W^T + b) + residual, fp32 rows of width 128 (a transformer sub-layer's output), with up to two
// fused consumers of the finished rows: the mean over each group of rows_per_group rows (the encoder's pooling
// step, pool_out zeroed by the caller) and LayerNorm-128 (the next sub-layer's pre-norm: bf16 rows + mean/rstd).
// g2 (w != nullptr): the second GEMM on the LayerNorm rows - out = dropout(act(rows @ w^T + bias)) (M, n) bf16, pre (nullable)
// its pre-activation copy.  keep: the caller's kernel keeps the output tile in LDS (second_gemm<F, true>), so out may be null.
struct Gemm2H { const void* w = nullptr; const float* bias = nullptr; int n = 0; void* out = nullptr; int act = 0;
                float drop_p = 0.f; uint32_t seed = 0; void* pre = nullptr; bool keep = false; };
static int linear128_fwd_args(ConvArgs& a, const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                              float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch, float* pool_out,
                              int rows_per_group, const float* ln_gamma, const float* ln_beta, float ln_eps, void* ln_out,
                              float* ln_stat, const Gemm2H& g2 = {}) {
    MM_REQUIRE(x && w && out_f32 && M > 0 && M % 32 == 0 && K > 0 && K % 16 == 0, "linear128_fwd: M=%d (x32) K=%d (x16)", M, K);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "linear128_fwd: drop_p");
    MM_REQUIRE(!pool_out || (rows_per_group > 0 && rows_per_group % 32 == 0 && M % rows_per_group == 0),
               "linear128_fwd: rows_per_group=%d must be a multiple of 32 dividing M=%d", rows_per_group, M);
    MM_REQUIRE(!ln_out || (ln_gamma && ln_beta), "linear128_fwd: LayerNorm parameters");
    a.x = (const bf16*)x; a.w = (const bf16*)w;
    a.B = 1; a.T = M; a.Cin = K; a.Cout = 128; a.taps = 1; a.pad = 0;
    a.e.shift = bias; a.e.residual = residual; a.e.out_f32 = out_f32;
    const DropH d = mm_drop(drop_p);
    a.e.drop_thresh = d.thresh; a.e.drop_inv_keep = d.inv_keep; a.e.drop_seed = seed; a.e.drop_epoch = seed_epoch;
    if (pool_out) { a.e.pool_out = pool_out; a.e.pool_rows = rows_per_group; a.e.pool_scale = 1.f / (float)rows_per_group; }
    a.e.lnf_out = (bf16*)ln_out; a.e.lnf_stat = ln_stat; a.e.lnf_gamma = ln_gamma; a.e.lnf_beta = ln_beta; a.e.lnf_eps = ln_eps;
    if (g2.w) {
        MM_REQUIRE(ln_out && (g2.out || g2.keep) && g2.n > 0 && g2.n % 128 == 0, "linear128_fwd: the second GEMM needs the LayerNorm rows, an output and n2 %% 128 == 0 (n2=%d)", g2.n);
        MM_REQUIRE(g2.drop_p >= 0.f && g2.drop_p < 1.f && (size_t)M * g2.n < (1ull << 32), "linear128_fwd: second GEMM dropout / 32-bit indices");
        a.e.w2 = (const bf16*)g2.w; a.e.bias2 = g2.bias; a.e.n2 = g2.n; a.e.out2 = (bf16*)g2.out;
        a.e.act2 = g2.act; a.e.pre2 = (bf16*)g2.pre;
        const DropH d2 = mm_drop(g2.drop_p);
        a.e.thresh2 = d2.thresh; a.e.inv_keep2 = d2.inv_keep; a.e.seed2 = g2.seed;
    }
    return 0;
}

// dx = LayerNorm128_backward(dy @ W^T) + dres in one launch: the data-gradient GEMM of the Linear that
// consumed LN(x) (dy (M, K) bf16, w = that Linear's dgrad image (128 rows of K)) with the LayerNorm
// backward as its epilogue.  Same results as mm_conv1d_fwd followed by mm_layernorm_bwd, except that the
// d(LN output) rows stay fp32 instead of a bf16 round trip.
static int linear_dgrad_ln_bwd_args(ConvArgs& a, const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                                    const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgb_repl,
                                    float drop_p, uint32_t seed, const uint32_t* seed_epoch, const BnRed* bn = nullptr,
                                    const void* w2 = nullptr, void* out2 = nullptr, int res_rows = 0) {
    MM_REQUIRE(dy && w && x && stat && gamma && (dx || dx_bf16), "linear_dgrad_ln_bwd: null");
    MM_REQUIRE(!w2 || (out2 && dx_bf16), "linear_dgrad_ln_bwd: the second GEMM needs the bf16 rows and an output");
    MM_REQUIRE(M > 0 && M % 32 == 0 && K > 0 && K % 16 == 0, "linear_dgrad_ln_bwd: M=%d (multiple of 32) K=%d (multiple of 16)", M, K);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "linear_dgrad_ln_bwd: drop_p");
    a.x = (const bf16*)dy; a.w = (const bf16*)w;
    a.B = 1; a.T = M; a.Cin = K; a.Cout = 128; a.taps = 1; a.pad = 0;
    a.e.residual = dres; a.e.out_f32 = dx; a.e.out_bf16 = (bf16*)dx_bf16;
    const DropH d = mm_drop(drop_p);
    a.e.drop_thresh = d.thresh; a.e.drop_inv_keep = d.inv_keep; a.e.drop_seed = seed; a.e.drop_epoch = seed_epoch;
    a.e.ln_x = x; a.e.ln_stat = stat; a.e.ln_gamma = gamma; a.e.ln_dgb = dgb_repl;
    if (bn) a.e.bn = *bn;
    a.e.w2 = (const bf16*)w2; a.e.out2 = (bf16*)out2;
    MM_REQUIRE(res_rows >= 0 && (!res_rows || (dres && M % res_rows == 0 && (size_t)M < (1ull << 32))), "linear_dgrad_ln_bwd: res_rows=%d", res_rows);
    a.e.res_rows = res_rows;
    return 0;
}

}  // namespace

#undef EF_ON
