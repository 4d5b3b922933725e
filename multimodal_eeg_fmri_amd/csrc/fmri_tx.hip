// The encoders of the fMRI notebook's transformer fusion model (fMRI_CODE/CrossModal_fmri_scr.ipynb, cell "# ENCODER
// BLOCKS": ActivationEncoder / ConnectivityEncoder = Linear(in_dim -> H), nn.TransformerEncoder of L post-norm
// nn.TransformerEncoderLayer(d_model = H, nhead = 4, dim_feedforward = 4H, ReLU, batch_first) on a sequence of length ONE,
// LayerNorm(H)) as ONE forward launch and TWO backward launches for up to two stacks (both encoders of fMRIFusionNet).
// fp32 operands, fp32 accumulation, every sum in a fixed (ascending) order, no atomics, no workgroup waits for another
// (DESIGN.md section 5n).  Callers: ops.tab_tx_forward_impl, small_autograd.TabTxFn.
//
// With a single key the softmax is identically 1, so per layer and row h (H floats):
//   v  = Wv h + bv                        Wv = in_proj_weight[2H:3H], bv = in_proj_bias[2H:3H]
//   sa = Wo (keep_attn * v) + bo          keep_attn: one keep / scale value per (row, head), over the head's H / 4 columns
//   h  = LN1(h + drop1(sa))               eps 1e-5
//   ff = W2 drop(relu(W1 h + b1)) + b2
//   h  = LN2(h + drop2(ff))
// and the encoder's final LayerNorm after the last layer.  The query / key rows of in_proj never reach the output: the
// backward WRITES ZEROS to their gradients (torch leaves ~1e-18 there, and AdamW's weight decay then acts on them alone).
//
// Parameter table of a stack (host array of device pointers, `params`; the gradient table `grads` has the same layout,
// every entry nullable) = the module's parameters() order, 4 + 12 L entries:
//   0 project.weight [H][in]  1 project.bias
//   2 + 12 l + {0 in_proj_weight [3H][H], 1 in_proj_bias, 2 out_proj.weight [H][H], 3 out_proj.bias, 4 linear1.weight [4H][H],
//               5 linear1.bias, 6 linear2.weight [H][4H], 7 linear2.bias, 8 norm1.weight, 9 norm1.bias, 10 norm2.weight,
//               11 norm2.bias}
//   2 + 12 L norm.weight, 3 + 12 L norm.bias
// Two stacks: the second stack's table follows the first.
//
// Dropout (common.h's counter hash, seeds through mm_eff_seed): 4 L seeds per stack, layer order then site order
//   0 attention: element index b * 4 + head          1 dropout1: b * H + f
//   2 FFN middle: b * 4H + f                         3 dropout2: b * H + f
// Two stacks: the second stack's seeds follow the first's.
//
// Save buffer (forward -> backward), floats, per stack (1 + 9 L) B H, the second stack behind the first:
//   h0 [B][H] (project output), then per layer: mv [B][H] (keep_attn * v), y1 [B][H] (LN1 input), h1 [B][H] (LN1 output),
//   mid [B][4H] (post ReLU and dropout), y2 [B][H] (LN2 input), h2 [B][H] (LN2 output = the next layer's input).
// Scratch (backward pass 1 -> pass 2), floats, per stack (3 + 11 L) B H: the gradient at every Linear's output and, per
// LayerNorm, dy and dy * xhat:
//   dh0 [B][H], per layer: dv [H], dsa [H], dpre1 [4H], dff [H], ln1 dy [H], ln1 dy*xhat [H], ln2 dy [H], ln2 dy*xhat [H]
//   (each x B rows), then the final norm's dy, dy*xhat.
//
// Forward: grid (ceil(B / 16), stacks); a workgroup owns 16 rows of one stack, keeps their activations in LDS and streams
// every weight matrix through a 64 x 32 LDS tile, k ascending.  Backward pass 1 has the same decomposition and runs the
// chain in reverse (dx [B][in], optional, is its last product).  Backward pass 2: a workgroup owns one 64 x 64 tile of one
// weight gradient (sum over rows ascending), or the column sums (biases, LayerNorm parameters) of one layer, where it also
// zeroes the query / key rows.  Every gradient element has one writer and is a plain store.
#include "common.h"

namespace {
constexpr int TX_R = 16;           // rows a workgroup owns
constexpr int TX_NT = 64;          // output columns per weight tile
constexpr int TX_KT = 32;          // reduction tile
constexpr int TX_LMAX = 8;
constexpr int TX_PMAX = 4 + 12 * TX_LMAX;
constexpr int TX_HMAX = 128;
constexpr float TX_EPS = 1e-5f;
// the H / 16 <= 8 columns a thread holds of its row: a fixed trip count, so that they stay in registers
#define TX_COLS(i, nc) _Pragma("unroll") for (int i = 0; i < TX_HMAX / 16; ++i) if (i < (nc))

struct TxStack { const float* p[TX_PMAX]; uint32_t seed[4 * TX_LMAX]; };
struct TxGrads { float* g[TX_PMAX]; };

__host__ __device__ inline size_t tx_save_floats(int B, int H, int L) { return (size_t)(1 + 9 * L) * B * H; }
__host__ __device__ inline size_t tx_scratch_floats(int B, int H, int L) { return (size_t)(3 + 11 * L) * B * H; }
// offsets inside a stack's save area, in units of B * H
enum { SV_MV = 0, SV_Y1 = 1, SV_H1 = 2, SV_MID = 3, SV_Y2 = 7, SV_H2 = 8 };
__host__ __device__ inline size_t tx_sv(int B, int H, int l, int what) { return (size_t)(1 + 9 * l + what) * B * H; }
// offsets inside a stack's scratch area, in units of B * H
enum { G_DV = 0, G_DSA = 1, G_DPRE1 = 2, G_DFF = 6, G_LN1 = 7, G_LN1X = 8, G_LN2 = 9, G_LN2X = 10 };
__host__ __device__ inline size_t tx_g(int B, int H, int l, int what) { return (size_t)(1 + 11 * l + what) * B * H; }

struct __attribute__((aligned(16))) TxSmem {
    float a[TX_R][TX_HMAX];            // forward: h          backward: the running gradient
    float b[TX_R][TX_HMAX];            // forward: mv         backward: the residual branch's gradient
    float m[TX_R][4 * TX_HMAX];        // forward: x tile, FFN middle       backward: d mid / d v
    float w[TX_NT][TX_KT + 4];         // (+4: rows stay 16-byte aligned; a quarter wave's float4 reads fall on distinct banks)
};

// out(r, n) = sum_k in(r, k) Wt(n, k) for r < 16, n < N, k ascending (fp32 FMA).  Wt(n, k) = W[n * ldw + k], or with TR
// W[k * ldw + n] (the transposed product of a backward).  in(r, k, kk): the address of four consecutive k of row r in LDS
// (16-byte aligned), valid for k < round_up(K, 32) (weights beyond K are staged as zeros).  stage(k0, kt): the caller's own staging before the tile's barrier.  A thread owns
// column n0 + tid % 64 for the four rows 4 (tid / 64) ..; epi(r, n, sum) takes the result.
template <bool TR, class Stage, class In, class Epi>
__device__ __forceinline__ void tx_gemm(TxSmem& s, int N, int K, const float* W, int ldw, Stage&& stage, In&& in, Epi&& epi) {
    const int tid = threadIdx.x, n = tid & 63, r0 = (tid >> 6) * 4;
    for (int n0 = 0; n0 < N; n0 += TX_NT) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K; k0 += TX_KT) {
            const int kt = K - k0 < TX_KT ? K - k0 : TX_KT;
            __syncthreads();                                       // the tile before has been read; LDS inputs are written
            for (int i = tid; i < TX_NT * TX_KT; i += 256) {
                const int nn = TR ? i % TX_NT : i / TX_KT, kk = TR ? i / TX_NT : i % TX_KT;
                const bool ok = n0 + nn < N && kk < kt;
                s.w[nn][kk] = ok ? (TR ? W[(size_t)(k0 + kk) * ldw + n0 + nn] : W[(size_t)(n0 + nn) * ldw + k0 + kk]) : 0.f;
            }
            stage(k0, kt);
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < TX_KT; kk += 4) {                // four k per LDS read of either operand
                const float4 w = *reinterpret_cast<const float4*>(&s.w[n][kk]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 x = *reinterpret_cast<const float4*>(in(r0 + j, k0 + kk, kk));
                    acc[j] = fmaf(x.x, w.x, acc[j]);
                    acc[j] = fmaf(x.y, w.y, acc[j]);
                    acc[j] = fmaf(x.z, w.z, acc[j]);
                    acc[j] = fmaf(x.w, w.w, acc[j]);
                }
            }
        }
        if (n0 + n < N) {
#pragma unroll
            for (int j = 0; j < 4; ++j) epi(r0 + j, n0 + n, acc[j]);
        }
    }
    __syncthreads();
}

// sum over the 16 lanes that share a row (tid / 16 = row): DPP adds in a fixed pairing
__device__ __forceinline__ float tx_row_sum(float v) { return row16_sum(v); }

// LayerNorm of the 16 rows of buf (in place), H / 16 columns per thread: two passes (mean, then the centred squares)
__device__ __forceinline__ void tx_ln_rows(float (*buf)[TX_HMAX], int H, const float* gamma, const float* beta) {
    const int r = threadIdx.x >> 4, l = threadIdx.x & 15, nc = H >> 4;
    float v[TX_HMAX / 16], sm = 0.f;
    TX_COLS(i, nc) { v[i] = buf[r][l + 16 * i]; sm += v[i]; }
    const float mean = tx_row_sum(sm) / H;
    float sq = 0.f;
    TX_COLS(i, nc) { const float d = v[i] - mean; sq = fmaf(d, d, sq); }
    const float rstd = 1.f / sqrtf(tx_row_sum(sq) / H + TX_EPS);
    TX_COLS(i, nc) {
        const int j = l + 16 * i;
        buf[r][j] = fmaf((v[i] - mean) * rstd, gamma[j], beta[j]);
    }
}

// 16 rows of an LDS buffer -> global [B][W] (rows b0 + r < B)
__device__ __forceinline__ void tx_store_rows(const float* buf, int ld, float* dst, int W, int b0, int B) {
    for (int i = threadIdx.x; i < TX_R * W; i += 256) {
        const int r = i / W, j = i - r * W;
        if (b0 + r < B) dst[(size_t)(b0 + r) * W + j] = buf[r * ld + j];
    }
}

struct TxFwdArgs {
    TxStack st[2];
    const float* x[2]; float* out[2]; float* save;
    int in[2], B, H, L;
    uint32_t thresh; float inv_keep; const uint32_t* epoch;
};

__global__ __launch_bounds__(256) void tab_tx_fwd_kernel(TxFwdArgs a) {
    __shared__ TxSmem s;
    const int sk = blockIdx.y, b0 = blockIdx.x * TX_R, B = a.B, H = a.H, H4 = 4 * a.H, L = a.L, K0 = a.in[sk];
    const TxStack& S = a.st[sk];
    const float* x = a.x[sk];
    float* sv = a.save ? a.save + (size_t)sk * tx_save_floats(B, H, L) : nullptr;
    const uint32_t thresh = a.thresh;
    const float ik = a.inv_keep;
    const int dh = H / 4;
    auto none = [](int, int) {};
    // project: the x tile [16][32] is staged in s.m (rows beyond B as zeros)
    {
        const float* pb = S.p[1];
        tx_gemm<false>(s, H, K0, S.p[0], K0,
                       [&](int k0, int kt) {
                           for (int i = threadIdx.x; i < TX_R * TX_KT; i += 256) {
                               const int r = i / TX_KT, kk = i % TX_KT;
                               s.m[r][kk] = (b0 + r < B && kk < kt) ? x[(size_t)(b0 + r) * K0 + k0 + kk] : 0.f;
                           }
                       },
                       [&](int r, int, int kk) { return &s.m[r][kk]; },
                       [&](int r, int n, float v) { s.a[r][n] = v + pb[n]; });
        if (sv) tx_store_rows(&s.a[0][0], TX_HMAX, sv, H, b0, B);
    }
    for (int l = 0; l < L; ++l) {
        const float* const* P = S.p + 2 + 12 * l;
        const uint32_t sd0 = mm_eff_seed(S.seed[4 * l], a.epoch), sd1 = mm_eff_seed(S.seed[4 * l + 1], a.epoch),
                       sd2 = mm_eff_seed(S.seed[4 * l + 2], a.epoch), sd3 = mm_eff_seed(S.seed[4 * l + 3], a.epoch);
        {   // mv = keep_attn * (Wv h + bv)
            const float* bv = P[1] + 2 * H;
            tx_gemm<false>(s, H, H, P[0] + (size_t)2 * H * H, H, none, [&](int r, int k, int) { return &s.a[r][k]; },
                           [&](int r, int n, float v) {
                               v += bv[n];
                               if (thresh) v *= dropout_scale(sd0, (uint32_t)((b0 + r) * 4 + n / dh), thresh, ik);
                               s.b[r][n] = v;
                           });
            if (sv) tx_store_rows(&s.b[0][0], TX_HMAX, sv + tx_sv(B, H, l, SV_MV), H, b0, B);
        }
        {   // y1 = h + drop1(Wo mv + bo), in place
            const float* bo = P[3];
            tx_gemm<false>(s, H, H, P[2], H, none, [&](int r, int k, int) { return &s.b[r][k]; },
                           [&](int r, int n, float v) {
                               v += bo[n];
                               if (thresh) v *= dropout_scale(sd1, (uint32_t)((b0 + r) * H + n), thresh, ik);
                               s.a[r][n] += v;
                           });
            if (sv) tx_store_rows(&s.a[0][0], TX_HMAX, sv + tx_sv(B, H, l, SV_Y1), H, b0, B);
            __syncthreads();
            tx_ln_rows(s.a, H, P[8], P[9]);
            __syncthreads();
            if (sv) tx_store_rows(&s.a[0][0], TX_HMAX, sv + tx_sv(B, H, l, SV_H1), H, b0, B);
        }
        {   // mid = drop(relu(W1 h + b1))
            const float* b1 = P[5];
            tx_gemm<false>(s, H4, H, P[4], H, none, [&](int r, int k, int) { return &s.a[r][k]; },
                           [&](int r, int n, float v) {
                               v = fmaxf(v + b1[n], 0.f);
                               if (thresh) v *= dropout_scale(sd2, (uint32_t)((b0 + r) * H4 + n), thresh, ik);
                               s.m[r][n] = v;
                           });
            if (sv) tx_store_rows(&s.m[0][0], 4 * TX_HMAX, sv + tx_sv(B, H, l, SV_MID), H4, b0, B);
        }
        {   // y2 = h + drop2(W2 mid + b2), in place
            const float* b2 = P[7];
            tx_gemm<false>(s, H, H4, P[6], H4, none, [&](int r, int k, int) { return &s.m[r][k]; },
                           [&](int r, int n, float v) {
                               v += b2[n];
                               if (thresh) v *= dropout_scale(sd3, (uint32_t)((b0 + r) * H + n), thresh, ik);
                               s.a[r][n] += v;
                           });
            if (sv) tx_store_rows(&s.a[0][0], TX_HMAX, sv + tx_sv(B, H, l, SV_Y2), H, b0, B);
            __syncthreads();
            tx_ln_rows(s.a, H, P[10], P[11]);
            __syncthreads();
            if (sv) tx_store_rows(&s.a[0][0], TX_HMAX, sv + tx_sv(B, H, l, SV_H2), H, b0, B);
        }
    }
    __syncthreads();
    tx_ln_rows(s.a, H, S.p[2 + 12 * L], S.p[3 + 12 * L]);
    __syncthreads();
    tx_store_rows(&s.a[0][0], TX_HMAX, a.out[sk], H, b0, B);
}

// ------------------------------------------------------------------------------------------------- backward, pass 1
struct TxBwdArgs {
    TxStack st[2];
    const float* dout[2]; float* dx[2];
    const float* save; float* scratch;
    int in[2], B, H, L;
    uint32_t thresh; float inv_keep; const uint32_t* epoch;
};

// LayerNorm backward of the 16 rows in s.a (the gradient at the LayerNorm's output), y = its saved input [B][H]:
// dy and dy * xhat go to the scratch (pass 2 sums their columns); the gradient at the input is left in s.b, and times the
// dropout mask of (seed, b * H + j) - the gradient at the residual branch's output - in s.a and in `dbranch`.
__device__ __forceinline__ void tx_ln_bwd_rows(TxSmem& s, int H, int B, int b0, const float* y, const float* gamma, float* dy_out,
                                               float* dyx_out, float* dbranch, bool masked, uint32_t seed, uint32_t thresh, float ik) {
    const int r = threadIdx.x >> 4, l = threadIdx.x & 15, nc = H >> 4, b = b0 + r;
    const bool live = b < B;
    float v[TX_HMAX / 16], g[TX_HMAX / 16], sm = 0.f;
    TX_COLS(i, nc) {
        const int j = l + 16 * i;
        v[i] = live ? y[(size_t)b * H + j] : 0.f;
        g[i] = s.a[r][j];
        sm += v[i];
    }
    const float mean = tx_row_sum(sm) / H;
    float sq = 0.f;
    TX_COLS(i, nc) { v[i] -= mean; sq = fmaf(v[i], v[i], sq); }
    const float rstd = 1.f / sqrtf(tx_row_sum(sq) / H + TX_EPS);
    float s1 = 0.f, s2 = 0.f;
    TX_COLS(i, nc) {
        const int j = l + 16 * i;
        v[i] *= rstd;                                              // xhat
        if (live) { dy_out[(size_t)b * H + j] = g[i]; dyx_out[(size_t)b * H + j] = g[i] * v[i]; }
        g[i] *= gamma[j];
        s1 += g[i]; s2 = fmaf(g[i], v[i], s2);
    }
    const float m1 = tx_row_sum(s1) / H, m2 = tx_row_sum(s2) / H;
    TX_COLS(i, nc) {
        const int j = l + 16 * i;
        const float d = rstd * (g[i] - m1 - v[i] * m2);
        s.b[r][j] = d;
        if (masked) {
            const float dm = thresh ? d * dropout_scale(seed, (uint32_t)(b * H + j), thresh, ik) : d;
            s.a[r][j] = dm;
            if (live) dbranch[(size_t)b * H + j] = dm;
        }
    }
}

__global__ __launch_bounds__(256) void tab_tx_bwd_rows_kernel(TxBwdArgs a) {
    __shared__ TxSmem s;
    const int sk = blockIdx.y, b0 = blockIdx.x * TX_R, B = a.B, H = a.H, H4 = 4 * a.H, L = a.L, K0 = a.in[sk];
    const TxStack& S = a.st[sk];
    const float* sv = a.save + (size_t)sk * tx_save_floats(B, H, L);
    float* G = a.scratch + (size_t)sk * tx_scratch_floats(B, H, L);
    const uint32_t thresh = a.thresh;
    const float ik = a.inv_keep;
    const int dh = H / 4;
    const size_t BH = (size_t)B * H;
    auto none = [](int, int) {};
    for (int i = threadIdx.x; i < TX_R * H; i += 256) {
        const int r = i / H, j = i - r * H;
        s.a[r][j] = b0 + r < B ? a.dout[sk][(size_t)(b0 + r) * H + j] : 0.f;
    }
    __syncthreads();
    // final norm: its input is the last layer's h2 (h0 when there were no layers - L >= 1 always)
    tx_ln_bwd_rows(s, H, B, b0, sv + tx_sv(B, H, L - 1, SV_H2), S.p[2 + 12 * L], G + tx_g(B, H, L, 0), G + tx_g(B, H, L, 0) + BH,
                   nullptr, false, 0u, 0u, 1.f);
    __syncthreads();
    for (int i = threadIdx.x; i < TX_R * H; i += 256) { const int r = i / H, j = i - r * H; s.a[r][j] = s.b[r][j]; }
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
        const float* const* P = S.p + 2 + 12 * l;
        const uint32_t sd0 = mm_eff_seed(S.seed[4 * l], a.epoch), sd1 = mm_eff_seed(S.seed[4 * l + 1], a.epoch),
                       sd3 = mm_eff_seed(S.seed[4 * l + 3], a.epoch);
        // LN2: s.b = d y2, s.a = d ff = d y2 * mask2
        tx_ln_bwd_rows(s, H, B, b0, sv + tx_sv(B, H, l, SV_Y2), P[10], G + tx_g(B, H, l, G_LN2), G + tx_g(B, H, l, G_LN2X),
                       G + tx_g(B, H, l, G_DFF), true, sd3, thresh, ik);
        {   // d pre1 = (W2^T d ff) * relu' * mask (read off the saved middle: positive exactly where kept and positive)
            const float* mid = sv + tx_sv(B, H, l, SV_MID);
            float* dpre = G + tx_g(B, H, l, G_DPRE1);
            tx_gemm<true>(s, H4, H, P[6], H4, none, [&](int r, int k, int) { return &s.a[r][k]; },
                          [&](int r, int n, float v) {
                              const int b = b0 + r;
                              const float d = (b < B && mid[(size_t)b * H4 + n] > 0.f) ? v * ik : 0.f;
                              s.m[r][n] = d;
                              if (b < B) dpre[(size_t)b * H4 + n] = d;
                          });
        }
        // d h1 = W1^T d pre1 + d y2
        tx_gemm<true>(s, H, H4, P[4], H, none, [&](int r, int k, int) { return &s.m[r][k]; },
                      [&](int r, int n, float v) { s.a[r][n] = v + s.b[r][n]; });
        // LN1: s.b = d y1, s.a = d sa = d y1 * mask1
        tx_ln_bwd_rows(s, H, B, b0, sv + tx_sv(B, H, l, SV_Y1), P[8], G + tx_g(B, H, l, G_LN1), G + tx_g(B, H, l, G_LN1X),
                       G + tx_g(B, H, l, G_DSA), true, sd1, thresh, ik);
        {   // d v = keep_attn * (Wo^T d sa)
            float* dv = G + tx_g(B, H, l, G_DV);
            tx_gemm<true>(s, H, H, P[2], H, none, [&](int r, int k, int) { return &s.a[r][k]; },
                          [&](int r, int n, float v) {
                              const int b = b0 + r;
                              if (thresh) v *= dropout_scale(sd0, (uint32_t)(b * 4 + n / dh), thresh, ik);
                              s.m[r][n] = v;
                              if (b < B) dv[(size_t)b * H + n] = v;
                          });
        }
        // d h_in = Wv^T d v + d y1
        tx_gemm<true>(s, H, H, P[0] + (size_t)2 * H * H, H, none, [&](int r, int k, int) { return &s.m[r][k]; },
                      [&](int r, int n, float v) { s.a[r][n] = v + s.b[r][n]; });
    }
    tx_store_rows(&s.a[0][0], TX_HMAX, G, H, b0, B);               // d h0
    if (a.dx[sk]) {
        float* dx = a.dx[sk];
        tx_gemm<true>(s, K0, H, S.p[0], K0, none, [&](int r, int k, int) { return &s.a[r][k]; },
                      [&](int r, int n, float v) { if (b0 + r < B) dx[(size_t)(b0 + r) * K0 + n] = v; });
    }
}

// ------------------------------------------------------------------------------------------------- backward, pass 2
struct TxParArgs {
    TxGrads gr[2];
    const float* x[2];
    const float* save; const float* scratch;
    int in[2], B, H, L;
};

struct __attribute__((aligned(16))) TxTileSmem { float a[64][64 + 4], b[64][64 + 4]; };

// one 64 x 64 tile (m0, n0) of C[m][n] = sum_b A[b * lda + m] Bm[b * ldb + n], b ascending, to dst[m * N + n]
__device__ __forceinline__ void tx_wgrad_tile(TxTileSmem& s, float* dst, int M, int N, const float* A, int lda, const float* Bm,
                                              int ldb, int B, int m0, int n0) {
    if (!dst) return;
    const int tid = threadIdx.x, tm = (tid >> 4) * 4, tn = (tid & 15) * 4;
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
    for (int k0 = 0; k0 < B; k0 += 64) {
        __syncthreads();
        for (int i = tid; i < 64 * 64; i += 256) {
            const int kk = i >> 6, c = i & 63;
            const bool row = k0 + kk < B;
            s.a[kk][c] = (row && m0 + c < M) ? A[(size_t)(k0 + kk) * lda + m0 + c] : 0.f;
            s.b[kk][c] = (row && n0 + c < N) ? Bm[(size_t)(k0 + kk) * ldb + n0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) {
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
            if (m0 + tm + u < M && n0 + tn + v < N) dst[(size_t)(m0 + tm + u) * N + n0 + tn + v] = acc[u][v];
}

// column sums dst[j] = sum_b src[b * W + j], b ascending, for a list of (dst, src, W): one thread per column of the whole
// list, eight rows' loads in flight at a time and added in row order
struct TxColSum { float* dst; const float* src; int W; };
template <int N>
__device__ __forceinline__ void tx_colsums(const TxColSum (&cs)[N], int B) {
    int total = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) total += cs[q].W;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        int j = idx, W = 0;
        float* dst = nullptr;
        const float* src = nullptr;
        bool found = false;
#pragma unroll
        for (int q = 0; q < N; ++q) {
            if (!found && j < cs[q].W) { dst = cs[q].dst; src = cs[q].src; W = cs[q].W; found = true; }
            if (!found) j -= cs[q].W;
        }
        if (!dst) continue;
        float acc = 0.f;
        int b = 0;
        for (; b + 8 <= B; b += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(b + u) * W + j];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; b < B; ++b) acc += src[(size_t)b * W + j];
        dst[j] = acc;
    }
}

__host__ __device__ inline int tx_tiles(int n) { return (n + 63) / 64; }
// workgroups of pass 2 for one stack: project tiles, per layer (Wv, Wo, W1, W2 tiles + one for the column sums), one for
// the project bias and the final norm
__host__ __device__ inline int tx_par_blocks(int in, int H, int L) {
    const int tH = tx_tiles(H), t4 = tx_tiles(4 * H);
    return tH * tx_tiles(in) + L * (2 * tH * tH + 2 * tH * t4 + 1) + 1;
}

__global__ __launch_bounds__(256) void tab_tx_bwd_par_kernel(TxParArgs a) {
    __shared__ TxTileSmem s;
    const int sk = blockIdx.y, B = a.B, H = a.H, H4 = 4 * a.H, L = a.L, K0 = a.in[sk];
    int bid = blockIdx.x;
    if (bid >= tx_par_blocks(K0, H, L)) return;
    const float* sv = a.save + (size_t)sk * tx_save_floats(B, H, L);
    const float* G = a.scratch + (size_t)sk * tx_scratch_floats(B, H, L);
    float* const* gr = a.gr[sk].g;
    const size_t BH = (size_t)B * H;
    const int tH = tx_tiles(H), t4 = tx_tiles(H4), tI = tx_tiles(K0);
    if (bid < tH * tI) {                                           // d project.weight = d h0^T x
        tx_wgrad_tile(s, gr[0], H, K0, G, H, a.x[sk], K0, B, (bid / tI) * 64, (bid % tI) * 64);
        return;
    }
    bid -= tH * tI;
    const int per = 2 * tH * tH + 2 * tH * t4 + 1;
    if (bid < L * per) {
        const int l = bid / per;
        int t = bid % per;
        float* const* g = gr + 2 + 12 * l;
        const float* hin = l ? sv + tx_sv(B, H, l - 1, SV_H2) : sv;
        if (t < tH * tH) {                                         // d Wv = d v^T h_in
            tx_wgrad_tile(s, g[0] ? g[0] + (size_t)2 * H * H : nullptr, H, H, G + tx_g(B, H, l, G_DV), H, hin, H, B,
                          (t / tH) * 64, (t % tH) * 64);
            return;
        }
        t -= tH * tH;
        if (t < tH * tH) {                                         // d Wo = d sa^T mv
            tx_wgrad_tile(s, g[2], H, H, G + tx_g(B, H, l, G_DSA), H, sv + tx_sv(B, H, l, SV_MV), H, B, (t / tH) * 64, (t % tH) * 64);
            return;
        }
        t -= tH * tH;
        if (t < t4 * tH) {                                         // d W1 = d pre1^T h1
            tx_wgrad_tile(s, g[4], H4, H, G + tx_g(B, H, l, G_DPRE1), H4, sv + tx_sv(B, H, l, SV_H1), H, B, (t / tH) * 64, (t % tH) * 64);
            return;
        }
        t -= t4 * tH;
        if (t < tH * t4) {                                         // d W2 = d ff^T mid
            tx_wgrad_tile(s, g[6], H, H4, G + tx_g(B, H, l, G_DFF), H, sv + tx_sv(B, H, l, SV_MID), H4, B, (t / t4) * 64, (t % t4) * 64);
            return;
        }
        // the layer's column sums; the query / key rows of in_proj get zeros
        if (g[0]) for (int i = threadIdx.x; i < 2 * H * H; i += 256) g[0][i] = 0.f;
        if (g[1]) for (int i = threadIdx.x; i < 2 * H; i += 256) g[1][i] = 0.f;
        const TxColSum cs[8] = {{g[1] ? g[1] + 2 * H : nullptr, G + tx_g(B, H, l, G_DV), H}, {g[3], G + tx_g(B, H, l, G_DSA), H},
                                {g[5], G + tx_g(B, H, l, G_DPRE1), H4}, {g[7], G + tx_g(B, H, l, G_DFF), H},
                                {g[8], G + tx_g(B, H, l, G_LN1X), H}, {g[9], G + tx_g(B, H, l, G_LN1), H},
                                {g[10], G + tx_g(B, H, l, G_LN2X), H}, {g[11], G + tx_g(B, H, l, G_LN2), H}};
        tx_colsums(cs, B);
        return;
    }
    const TxColSum cs[3] = {{gr[1], G, H}, {gr[2 + 12 * L], G + tx_g(B, H, L, 0) + BH, H}, {gr[3 + 12 * L], G + tx_g(B, H, L, 0), H}};
    tx_colsums(cs, B);                                             // project bias, final norm
}

static bool tx_shape_ok(int nstacks, int B, int in0, int in1, int H, int L) {
    return (nstacks == 1 || nstacks == 2) && B >= 1 && in0 >= 1 && (nstacks == 1 || in1 >= 1) &&
           (H == 32 || H == 64 || H == 128) && L >= 1 && L <= TX_LMAX;
}

static bool tx_fill_stacks(TxStack* st, int nstacks, int L, const void* params_host, const uint32_t* seeds_host, bool seeded) {
    const int np = 4 + 12 * L;
    const float* const* p = static_cast<const float* const*>(params_host);
    for (int s = 0; s < nstacks; ++s) {
        for (int i = 0; i < np; ++i) {
            if (!p[s * np + i]) return false;
            st[s].p[i] = p[s * np + i];
        }
        for (int i = 0; i < 4 * L; ++i) st[s].seed[i] = seeded ? seeds_host[s * 4 * L + i] : 0u;
    }
    return true;
}
}  // namespace

extern "C" {
int mm_tab_tx_fwd(const float* x0, const float* x1, int nstacks, int B, int in0, int in1, int H, int L, const void* params_host,
                  float* out0, float* out1, float* save, float drop_p, const uint32_t* seeds_host, const uint32_t* seed_epoch,
                  hipStream_t st) {
    MM_REQUIRE(tx_shape_ok(nstacks, B, in0, in1, H, L), "tab_tx_fwd: stacks=%d (1 or 2) B=%d (>= 1) in_dim=%d, %d (>= 1) hidden_dim=%d (32, 64 or 128) num_layers=%d (1..8)", nstacks, B, in0, in1, H, L);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "tab_tx_fwd: drop_p");
    MM_REQUIRE(x0 && out0 && (nstacks == 1 || (x1 && out1)) && params_host && (drop_p == 0.f || seeds_host), "tab_tx_fwd: null");
    MM_REQUIRE((size_t)B * 4 * H < (1ull << 31), "tab_tx_fwd: B too large for the dropout index");
    TxFwdArgs a{};
    MM_REQUIRE(tx_fill_stacks(a.st, nstacks, L, params_host, seeds_host, drop_p > 0.f), "tab_tx_fwd: null parameter");
    a.x[0] = x0; a.x[1] = x1; a.out[0] = out0; a.out[1] = out1; a.save = save;
    a.in[0] = in0; a.in[1] = in1; a.B = B; a.H = H; a.L = L;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.inv_keep = d.inv_keep; a.epoch = seed_epoch;
    hipLaunchKernelGGL(tab_tx_fwd_kernel, dim3(ceil_div(B, TX_R), nstacks), dim3(256), 0, st, a);
    return mm_check_launch("tab_tx_fwd");
}

int mm_tab_tx_bwd(const float* dout0, const float* dout1, const float* x0, const float* x1, int nstacks, int B, int in0, int in1,
                  int H, int L, const void* params_host, const void* grads_host, const float* save, float* scratch, float* dx0,
                  float* dx1, float drop_p, const uint32_t* seeds_host, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(tx_shape_ok(nstacks, B, in0, in1, H, L), "tab_tx_bwd: stacks=%d (1 or 2) B=%d (>= 1) in_dim=%d, %d (>= 1) hidden_dim=%d (32, 64 or 128) num_layers=%d (1..8)", nstacks, B, in0, in1, H, L);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "tab_tx_bwd: drop_p");
    MM_REQUIRE(dout0 && x0 && (nstacks == 1 || (dout1 && x1)) && params_host && grads_host && save && scratch &&
               (drop_p == 0.f || seeds_host), "tab_tx_bwd: null");
    MM_REQUIRE((size_t)B * 4 * H < (1ull << 31), "tab_tx_bwd: B too large for the dropout index");
    TxBwdArgs a{};
    MM_REQUIRE(tx_fill_stacks(a.st, nstacks, L, params_host, seeds_host, drop_p > 0.f), "tab_tx_bwd: null parameter");
    a.dout[0] = dout0; a.dout[1] = dout1; a.dx[0] = dx0; a.dx[1] = nstacks == 2 ? dx1 : nullptr;
    a.save = save; a.scratch = scratch;
    a.in[0] = in0; a.in[1] = in1; a.B = B; a.H = H; a.L = L;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.inv_keep = d.inv_keep; a.epoch = seed_epoch;
    hipLaunchKernelGGL(tab_tx_bwd_rows_kernel, dim3(ceil_div(B, TX_R), nstacks), dim3(256), 0, st, a);
    int rc = mm_check_launch("tab_tx_bwd (rows)");
    if (rc) return rc;
    TxParArgs q{};
    const int np = 4 + 12 * L;
    float* const* g = static_cast<float* const*>(grads_host);
    for (int s = 0; s < nstacks; ++s)
        for (int i = 0; i < np; ++i) q.gr[s].g[i] = g[s * np + i];
    q.x[0] = x0; q.x[1] = x1; q.save = save; q.scratch = scratch;
    q.in[0] = in0; q.in[1] = in1; q.B = B; q.H = H; q.L = L;
    int blocks = tx_par_blocks(in0, H, L);
    if (nstacks == 2 && tx_par_blocks(in1, H, L) > blocks) blocks = tx_par_blocks(in1, H, L);
    hipLaunchKernelGGL(tab_tx_bwd_par_kernel, dim3(blocks, nstacks), dim3(256), 0, st, q);
    return mm_check_launch("tab_tx_bwd (parameters)");
}
}  // extern "C"
