// Weight gradient of the 1-D implicit-GEMM family (igemm1d.hip) and what turns its workspaces into parameter gradients:
//   wgrad   : dW[n,tap,c] = sum_{b,t} dY[b,t,n] * X[b, t+tap-pad, c]
// the GEMM (per-workgroup slots, one or many problems per launch), the slot sums (scatter), the accumulator reductions
// and the one-launch gradient flush.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------
// weight gradient:  dW[n][tap][c] += sum_{t in chunk} dY[b,t,n] * X[b,t+tap-pad,c]
// MFMA view: D[i=n][j=c] = sum_k A[i][k] B[k][j] with k = t, so both operands
// are k-strided in memory.  The dY tile [64 t][64 n] and the X halo tile
// [64+taps-1][64 c] are staged row-major and read with ds_read_b64_tr_b16
// (hardware transpose): each 16-lane group fetches a 4(t) x 16(col) block and
// every lane receives its column's 4 consecutive t values.  Row stride 192 B
// (== 192 mod 256) puts the 4 rows x 64 B a half-wave touches on 64 distinct
// banks.  A workgroup's partial sums leave as plain stores into its own slot of a
// workspace (arbitrary element strides sn/sc/stap; one writer per element, no
// atomics); the scatter / flush kernels below add the slots into the gradient.
// ---------------------------------------------------------------------------
constexpr int WG_MK = 64;          // t rows per LDS tile
constexpr int WG_LD = 96;          // LDS row stride in elements (192 B)

__device__ __forceinline__ bf16x8 tr_frag(const bf16* tile, int row0, int col0, int lane) {
    // rows row0 + 8*(lane>>5) + {0..7}, column col0 + (lane & 31)
    const int li = lane & 15, g = lane >> 4;
    const bf16* p = tile + (row0 + 8 * (g >> 1) + (li >> 2)) * WG_LD + col0 + (g & 1) * 16 + 4 * (li & 3);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * WG_LD));
    union { s16x4 s[2]; bf16x8 v; } u;
    u.s[0] = lo; u.s[1] = hi;
    return u.v;
}

struct WgradArgs {
    const bf16* dy; const bf16* x; float* dw; float* dbias;
    int B, T, Cin, Cout, pad, Cin_real, rows_per_wg, nrep;
    long sn, sc, stap, rep_stride;
    int slot_mode;            // 1: workgroup x stores its partial tile into slot blockIdx.x (no atomics)
    int bgroup;               // samples one workgroup accumulates over (> 1 only when a sample is a single row chunk)
};

template <int TAPS>
__device__ __forceinline__ void conv1d_wgrad_body(const WgradArgs& a, const int bx, const int by, const int bz) {
    __shared__ __attribute__((aligned(16))) bf16 Ys[WG_MK * WG_LD];
    __shared__ __attribute__((aligned(16))) bf16 Xs[(WG_MK + TAPS - 1) * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wc = wave & 1;
    const int chunksT = (a.T + a.rows_per_wg - 1) / a.rows_per_wg;
    // samples [b0, b1) of this workgroup: one, or - short sequences with many output tiles (config #5: 33 frames x 6 272
    // channels) - a group of them, so that the number of SLOTS (each a full weight-shaped fp32 image that the flush has to
    // sum: 33.7 MB there) does not grow with the batch
    const int b0 = (bx / chunksT) * a.bgroup, b1 = min(a.B, b0 + a.bgroup);
    const int tbeg = (bx % chunksT) * a.rows_per_wg;
    const int tend = min(a.T, tbeg + a.rows_per_wg);
    const int n0 = by * 64, c0 = bz * 64;

    f32x16 acc[TAPS];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;
    float bsum = 0.f;

    // tiles are fetched into registers one work item (sample, row tile) ahead (all loads in flight
    // before any LDS write, and in flight during the previous tile's MFMAs)
    constexpr int YREG = WG_MK * 8 / 256;                           // 2
    constexpr int XREG = ((WG_MK + TAPS - 1) * 8 + 255) / 256;      // 3
    uint4 yv[YREG], xv[XREG];
    auto fetch = [&](int b, int t0) {
        const bf16* dyb = a.dy + (size_t)b * a.T * a.Cout;
        const bf16* xb = a.x + (size_t)b * a.T * a.Cin;
#pragma unroll
        for (int i = 0; i < YREG; ++i) {
            const int s = tid + i * 256, r = s >> 3, sg = s & 7;
            const int t = t0 + r, n = n0 + sg * 8;
            yv[i] = (t < tend && n < a.Cout) ? *reinterpret_cast<const uint4*>(dyb + (size_t)t * a.Cout + n) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < XREG; ++i) {
            const int s = tid + i * 256, r = s >> 3, sg = s & 7;
            const int t = t0 - a.pad + r, c = c0 + sg * 8;
            xv[i] = (s < (WG_MK + TAPS - 1) * 8 && t >= 0 && t < a.T && c < a.Cin)
                        ? *reinterpret_cast<const uint4*>(xb + (size_t)t * a.Cin + c) : make_uint4(0, 0, 0, 0);
        }
    };
    int b = b0, t0 = tbeg;
    if (b < b1 && tbeg < tend) fetch(b, t0);
    while (b < b1 && tbeg < tend) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < YREG; ++i) {
            const int s = tid + i * 256;
            *reinterpret_cast<uint4*>(Ys + (s >> 3) * WG_LD + (s & 7) * 8) = yv[i];
        }
#pragma unroll
        for (int i = 0; i < XREG; ++i) {
            const int s = tid + i * 256;
            if (s < (WG_MK + TAPS - 1) * 8) *reinterpret_cast<uint4*>(Xs + (s >> 3) * WG_LD + (s & 7) * 8) = xv[i];
        }
        __syncthreads();
        int nb = b, nt = t0 + WG_MK;                                // next work item
        if (nt >= tend) { ++nb; nt = tbeg; }
        if (nb < b1) fetch(nb, nt);
#pragma unroll
        for (int kk = 0; kk < WG_MK; kk += 16) {
            const bf16x8 af = tr_frag(Ys, kk, wn * 32, lane);
            if (a.dbias && bz == 0 && wc == 0)
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum += (float)af[j];
#pragma unroll
            for (int tp = 0; tp < TAPS; ++tp) {
                const bf16x8 bfr = tr_frag(Xs, kk + tp, wc * 32, lane);
                acc[tp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[tp], 0, 0, 0);
            }
        }
        b = nb; t0 = nt;
    }
    // D[i = n][j = c]: lane owns column c, rows n = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const int c = c0 + wc * 32 + (lane & 31);
    float* dwr = a.dw + (size_t)bx * a.rep_stride;
    if (c < a.Cin_real) {
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n < a.Cout) dwr[n * a.sn + c * a.sc + tp * a.stap] = acc[tp][r];   // this (slot, tile) element has one writer
            }
    }
    if (a.dbias && bz == 0 && wc == 0) {
        bsum += __shfl_xor(bsum, 32, 64);
        const int n = n0 + wn * 32 + (lane & 31);
        if ((lane >> 5) == 0 && n < a.Cout) acc_add<MM_ACC_GRAD>(acc_rep(a.dbias, bx % MM_ACC_REPL, a.Cout) + n, bsum);
    }
}

template <int TAPS>
__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(WgradArgs a) {
    conv1d_wgrad_body<TAPS>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// several independent Linear (taps = 1) weight gradients in ONE launch: workgroup id -> (problem,
// its own 3-D block index).  The transformer blocks' eight weight-gradient GEMMs have nothing waiting
// on them but the final slot sum, so a trainer collects them and issues them once, off the chain.
constexpr int WM_MAX = 12;
struct WgradTable { WgradArgs a[WM_MAX]; int first[WM_MAX + 1]; int gx[WM_MAX], gy[WM_MAX]; int n; };
// Linear (taps = 1) weight gradient on a 128 (n) x 128 (c) workgroup tile: wave (wn, wc) owns 64 x 64 = 2 x 2
// MFMA tiles, so a k-step is 4 transposed LDS fragment reads for 4 MFMAs (the 64 x 64 tile: 2 for 1) and
// the operands are fetched from global memory half as often.  Each operand tile lives in LDS as two
// 64-column halves with the 192-byte row stride tr_frag is laid out for.  Slot mode only.
__device__ __forceinline__ void linear_wgrad128_body(const WgradArgs& a, const int bx, const int by, const int bz) {
    __shared__ __attribute__((aligned(16))) bf16 Ys[2][WG_MK * WG_LD];
    __shared__ __attribute__((aligned(16))) bf16 Xs[2][WG_MK * WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wc = wave & 1;
    const int chunksT = (a.T + a.rows_per_wg - 1) / a.rows_per_wg;
    const int b = bx / chunksT;
    const int tbeg = (bx % chunksT) * a.rows_per_wg;
    const int tend = min(a.T, tbeg + a.rows_per_wg);
    const int n0 = by * 128, c0 = bz * 128;
    const bf16* dyb = a.dy + (size_t)b * a.T * a.Cout;
    const bf16* xb = a.x + (size_t)b * a.T * a.Cin;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float bsum[2] = {0.f, 0.f};

    constexpr int NREG = WG_MK * 16 / 256;                          // 4 x 16-byte chunks per operand per thread
    uint4 yv[NREG], xv[NREG];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int i = 0; i < NREG; ++i) {
            const int s = tid + i * 256, r = s >> 4, sg = s & 15;
            const int t = t0 + r, n = n0 + sg * 8, c = c0 + sg * 8;
            yv[i] = (t < tend && n < a.Cout) ? *reinterpret_cast<const uint4*>(dyb + (size_t)t * a.Cout + n) : make_uint4(0, 0, 0, 0);
            xv[i] = (t < tend && c < a.Cin) ? *reinterpret_cast<const uint4*>(xb + (size_t)t * a.Cin + c) : make_uint4(0, 0, 0, 0);
        }
    };
    if (tbeg < tend) fetch(tbeg);
    for (int t0 = tbeg; t0 < tend; t0 += WG_MK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NREG; ++i) {
            const int s = tid + i * 256, r = s >> 4, sg = s & 15;
            *reinterpret_cast<uint4*>(Ys[sg >> 3] + r * WG_LD + (sg & 7) * 8) = yv[i];
            *reinterpret_cast<uint4*>(Xs[sg >> 3] + r * WG_LD + (sg & 7) * 8) = xv[i];
        }
        __syncthreads();
        if (t0 + WG_MK < tend) fetch(t0 + WG_MK);
#pragma unroll
        for (int kk = 0; kk < WG_MK; kk += 16) {
            bf16x8 af[2], bfr[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = tr_frag(Ys[wn], kk, i * 32, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = tr_frag(Xs[wc], kk, j * 32, lane);
            if (a.dbias && bz == 0 && wc == 0)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) bsum[i] += (float)af[i][j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    // D[i = n][j = c]: lane owns column c, rows n = (r&3) + 8*(r>>2) + 4*(lane>>5); every (slot, element) has one writer
    float* dwr = a.dw + (size_t)bx * a.rep_stride;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + wc * 64 + j * 32 + (lane & 31);
        if (c >= a.Cin_real) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n < a.Cout) dwr[n * a.sn + c * a.sc] = acc[i][j][r];
            }
    }
    if (a.dbias && bz == 0 && wc == 0)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v = bsum[i] + __shfl_xor(bsum[i], 32, 64);
            const int n = n0 + wn * 64 + i * 32 + (lane & 31);
            if ((lane >> 5) == 0 && n < a.Cout) acc_add<MM_ACC_GRAD>(acc_rep(a.dbias, bx % MM_ACC_REPL, a.Cout) + n, v);
        }
}

__global__ __launch_bounds__(256) void conv1d_wgrad_many_kernel(WgradTable tab) {
    int p = 0;
    while (p + 1 < tab.n && (int)blockIdx.x >= tab.first[p + 1]) ++p;
    const int local = blockIdx.x - tab.first[p];
    const int gx = tab.gx[p], gy = tab.gy[p];
    linear_wgrad128_body(tab.a[p], local % gx, (local / gx) % gy, local / (gx * gy));
}

// dw[n][c][tap] += sum_rep ws[rep][n][tap][c]   (replicated contiguous-atomics workspace -> PyTorch layout)
__global__ void wgrad_scatter_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Cout, int Cin, int taps,
                                     int Cinp, int nrep) {
    const size_t rstride = (size_t)Cout * taps * Cinp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rstride; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cinp);
        if (c >= Cin) continue;
        const int tap = (int)((i / Cinp) % taps);
        const int n = (int)(i / ((size_t)Cinp * taps));
        float s = 0.f;
        int r = 0;
        for (; r + 8 <= nrep; r += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = ws[(r + q) * rstride + i];      // coalesced along c
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; r < nrep; ++r) s += ws[r * rstride + i];
        dw[((size_t)n * Cin + c) * taps + tap] += s;
    }
}

// every conv weight-gradient workspace of a backward pass in one launch (blockIdx.y = tensor)
// taps: bits 0-7 the taps of the gradient tensor, bits 8-15 the first workspace tap it takes, bits 16-23 the taps of the
// workspace rows (0 = the same): a descriptor may take a WINDOW of the workspace's taps (the k = 3 / 5 branches of
// EnhancedPowerEncoder's merged k = 7 convolution: their gradients are the centre taps of their 64 output channels)
struct ScatterDesc { const float* ws; float* dw; int Cout, Cin, taps, Cinp, nrep, cout_all; };
__device__ __host__ inline int scatter_taps(const ScatterDesc& d) { return d.taps & 255; }
__device__ __host__ inline int scatter_tap0(const ScatterDesc& d) { return (d.taps >> 8) & 255; }
__device__ __host__ inline int scatter_ws_taps(const ScatterDesc& d) { return (d.taps >> 16) & 255 ? (d.taps >> 16) & 255 : (d.taps & 255); }
static bool scatter_desc_ok(const ScatterDesc& d) {
    return d.ws && d.dw && d.Cout > 0 && d.Cin > 0 && scatter_taps(d) > 0 && d.Cinp >= d.Cin && d.nrep >= 1 &&
           scatter_tap0(d) + scatter_taps(d) <= scatter_ws_taps(d) && (d.cout_all == 0 || d.cout_all >= d.Cout);
}
// cout_all: 0, or the output channels of the WHOLE workspace when the descriptor covers a slice of them (replica stride)
constexpr int SM_MAX = 64;
struct ScatterTable { ScatterDesc d[SM_MAX]; };
// wide layers (Cin >= 256: config #5's merged convolution has 6 272 input channels, 8.4 M weights): the strided
// read-modify-write of the plain form below ran at 0.6 TB/s (168 us).  Here a workgroup takes one output channel x 256
// input channels, reads the workspace rows of every tap coalesced, turns the [tap][c] block into [c][tap] through LDS and
// adds it to a CONTIGUOUS range of the gradient.  Same replica order as the plain form: same bits.
__device__ __forceinline__ void scatter_body_tiled(const ScatterDesc& d, int blk, int nblk) {
    __shared__ float tile[256 * 9];
    const int taps = scatter_taps(d), tap0 = scatter_tap0(d), tws = scatter_ws_taps(d);
    const size_t rstride = (size_t)(d.cout_all ? d.cout_all : d.Cout) * tws * d.Cinp;
    const int cch = (d.Cin + 255) / 256, items = d.Cout * cch, ts = taps | 1, tid = threadIdx.x;
    for (int item = blk; item < items; item += nblk) {
        const int n = item / cch, c0 = (item - n * cch) * 256;
        const int cn = min(256, d.Cin - c0);
        if (tid < cn)
            for (int tap = 0; tap < taps; ++tap) {
                const float* src = d.ws + ((size_t)n * tws + tap0 + tap) * d.Cinp + c0 + tid;
                float s = 0.f;
                int r = 0;
                for (; r + 8 <= d.nrep; r += 8) {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = src[(r + q) * rstride];
#pragma unroll
                    for (int q = 0; q < 8; ++q) s += v[q];
                }
                for (; r < d.nrep; ++r) s += src[r * rstride];
                tile[tid * ts + tap] = s;
            }
        __syncthreads();
        float* dst = d.dw + ((size_t)n * d.Cin + c0) * taps;
        for (int j = tid; j < cn * taps; j += 256) {
            const int cl = j / taps;
            dst[j] += tile[cl * ts + (j - cl * taps)];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void scatter_body(const ScatterDesc& d, int blk, int nblk) {
    const int taps = scatter_taps(d), tap0 = scatter_tap0(d), tws = scatter_ws_taps(d);
    if (taps > 1 && taps <= 8 && d.Cin >= 256) return scatter_body_tiled(d, blk, nblk);      // (uniform per descriptor)
    // walk the workspace in ITS order (channel-contiguous: the nrep replica reads coalesce) and
    // scatter one strided write per element, not nrep strided reads
    const size_t rstride = (size_t)(d.cout_all ? d.cout_all : d.Cout) * tws * d.Cinp;
    const size_t count = (size_t)d.Cout * taps * d.Cinp;
    for (size_t i = (size_t)blk * blockDim.x + threadIdx.x; i < count; i += (size_t)nblk * blockDim.x) {
        const int c = (int)(i % d.Cinp);
        if (c >= d.Cin) continue;
        const int tap = (int)((i / d.Cinp) % taps);
        const int n = (int)(i / ((size_t)d.Cinp * taps));
        const size_t e = ((size_t)n * tws + tap0 + tap) * d.Cinp + c;      // (= i for a whole-kernel descriptor)
        float s = 0.f;
        int r = 0;
        for (; r + 8 <= d.nrep; r += 8) {                   // eight independent loads at a time, not a latency chain
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = d.ws[(r + q) * rstride + e];
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; r < d.nrep; ++r) s += d.ws[r * rstride + e];
        d.dw[((size_t)n * d.Cin + c) * taps + tap] += s;
    }
}
__global__ void scatter_many_kernel(ScatterTable tab) { scatter_body(tab.d[blockIdx.y], blockIdx.x, gridDim.x); }

// dst[k] += sum_rep src[rep][k]
// one replica per lane (32 lanes per output), one shuffle reduction: a single
// load round trip instead of a 32-deep dependent chain
__global__ void reduce_replicas_kernel(const float* __restrict__ src, float* __restrict__ dst, int K, int nrep,
                                       long rep_stride) {
    const int k = blockIdx.x * 8 + (threadIdx.x >> 5);
    const int r0 = threadIdx.x & 31;
    float s = 0.f;
    if (k < K)
        for (int r = r0; r < nrep; r += 32) s += src[(size_t)r * rep_stride + k];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (k < K && r0 == 0) dst[k] += s;
}

// dst[k] += 2^-MM_ACC_GRAD * sum_rep acc[rep][k]: fixed-point accumulator workspace (common.h) -> fp32.
// One replica per lane (16 lanes per output), integer shuffle reduction.
__device__ __forceinline__ void acc_reduce_rows(const mm_acc_t* __restrict__ src, float* __restrict__ dst, long K,
                                                long rep_stride, long kfirst, long kstep) {
    const int r0 = threadIdx.x & 15;
    for (long k = kfirst + (threadIdx.x >> 4); k < ((K + 15) / 16) * 16; k += kstep) {
        mm_acc_t s = k < K ? src[r0 * rep_stride + k] : 0;
        s = acc_sum_lanes16(s);
        if (k < K && r0 == 0) dst[k] += acc_val<MM_ACC_GRAD>(s);
    }
}
__global__ void acc_reduce_kernel(const mm_acc_t* __restrict__ src, float* __restrict__ dst, int K, long rep_stride) {
    acc_reduce_rows(src, dst, K, rep_stride, (long)blockIdx.x * 16, (long)gridDim.x * 16);
}

template <int TAPS>
int launch_wgrad(const WgradArgs& a, hipStream_t st) {
    const int chunksT = ceil_div(a.T, a.rows_per_wg);
    dim3 grid(ceil_div(a.B, a.bgroup) * chunksT, ceil_div(a.Cout, 64), ceil_div(a.Cin, 64));
    hipLaunchKernelGGL(conv1d_wgrad_kernel<TAPS>, grid, dim3(256), 0, st, a);
    return mm_check_launch("conv1d_wgrad");
}

}  // namespace

// ============================================================================
// C ABI (declared in include/mmeeg_hip.h)
// ============================================================================
extern "C" {

// rows of T per workgroup.  Atomic mode: every workgroup ends with 64 x 64 x taps fp32 atomics, so for
// the k > 1 convs few, long workgroups win (sweep on the three EEG convs: 32 / 30 / 20 us at 384
// workgroups, 16 / 19 / 13 us at ~100).  Slot mode has no atomics: parallelism alone decides.
static int wgrad_rows_per_wg(int B, int T, int Cin, int Cout, int taps, int slot_mode) {
    const int tiles = ceil_div(Cout, 64) * ceil_div(Cin, 64);
    const int tilesT = ceil_div(T, WG_MK);
    constexpr int slot_target = 128;   // slot mode, k > 1: 384 1.116, 192 1.107, 128 1.106, 64 1.111 ms/step
    int want_chunks = ceil_div((taps > 1 && !slot_mode) ? 112 : (taps > 1 ? slot_target : 384), tiles * B);
    if (want_chunks < 1) want_chunks = 1;
    if (want_chunks > tilesT) want_chunks = tilesT;
    return ceil_div(tilesT, want_chunks) * WG_MK;
}

// samples per workgroup (conv1d_wgrad_body): 1 unless a sample is a single row chunk AND the output tiles alone fill the chip
static int wgrad_bgroup(int B, int T, int Cin, int Cout, int taps, int slot_mode) {
    const int rows = wgrad_rows_per_wg(B, T, Cin, Cout, taps, slot_mode);
    if (ceil_div(T, rows) != 1) return 1;
    const int tiles = ceil_div(Cout, 64) * ceil_div(Cin, 64);
    int nsl = 384 / tiles;                                          // slots wanted: ~384 workgroups in all
    if (nsl < 1) nsl = 1;
    if (nsl > B) nsl = B;
    return ceil_div(B, nsl);
}

// grouped launches (mm_conv1d_wgrad_many) get their parallelism from the number of problems, so each
// problem is cut into far fewer row chunks: ~32 workgroups per problem instead of 384 (round-1 sweep: 384 1.127, 128 1.124,
// 64 1.120, 32 1.158 ms/step; end of round 2, with the launch on the side stream beside the chain: 128 0.880, 96 0.873,
// 64 0.870, 48 0.866, 32 0.865, 24 0.864, 16 0.887 - fewer workgroups also leave more of the chip to the chain), i.e. 12x less
// slot memory to write and to sum afterwards
constexpr int WGRAD_MANY_TARGET = 32;
static int wgrad_many_rows_per_wg(int T, int Cin, int Cout) {
    const int tiles = ceil_div(Cout, 128) * ceil_div(Cin, 128);
    const int tilesT = ceil_div(T, WG_MK);
    int want_chunks = ceil_div(WGRAD_MANY_TARGET, tiles);
    if (want_chunks < 1) want_chunks = 1;
    if (want_chunks > tilesT) want_chunks = tilesT;
    return ceil_div(tilesT, want_chunks) * WG_MK;
}

int mm_conv1d_wgrad_many_slots(int B, int T, int Cin, int Cout, int* slots_host, hipStream_t) {
    MM_REQUIRE(slots_host && B > 0 && T > 0 && Cin > 0 && Cout > 0, "conv1d_wgrad_many_slots: bad args");
    *slots_host = B * ceil_div(T, wgrad_many_rows_per_wg(T, Cin, Cout));
    return 0;
}

int mm_conv1d_wgrad_slots(int B, int T, int Cin, int Cout, int taps, int* slots_host, hipStream_t) {
    MM_REQUIRE(slots_host && B > 0 && T > 0 && Cin > 0 && Cout > 0, "conv1d_wgrad_slots: bad args");
    *slots_host = ceil_div(B, wgrad_bgroup(B, T, Cin, Cout, taps, 1)) * ceil_div(T, wgrad_rows_per_wg(B, T, Cin, Cout, taps, 1));
    return 0;
}

int mm_conv1d_wgrad(const void* dy, const void* x, float* dw, float* dbias, int B, int T, int Cin, int Cout,
                    int taps, int pad, int Cin_real, int64_t sn, int64_t sc, int64_t stap, int nrep,
                    int64_t rep_stride, int slot_mode, hipStream_t st) {
    MM_REQUIRE(dy && x && dw && B > 0 && T > 0, "conv1d_wgrad: null/invalid");
    MM_REQUIRE(slot_mode == 1 && nrep >= 1, "conv1d_wgrad: slot_mode must be 1 (the fp32-atomics mode is gone: results are order-free)");
    MM_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0, "conv1d_wgrad: Cin=%d Cout=%d must be multiples of 8", Cin, Cout);
    MM_REQUIRE(Cin_real > 0 && Cin_real <= Cin, "conv1d_wgrad: Cin_real");
    WgradArgs a;
    a.dy = (const bf16*)dy; a.x = (const bf16*)x; a.dw = dw; a.dbias = dbias;
    a.B = B; a.T = T; a.Cin = Cin; a.Cout = Cout; a.pad = pad; a.Cin_real = Cin_real;
    a.sn = sn; a.sc = sc; a.stap = stap; a.nrep = nrep; a.rep_stride = rep_stride; a.slot_mode = slot_mode;
    a.rows_per_wg = wgrad_rows_per_wg(B, T, Cin, Cout, taps, slot_mode);
    a.bgroup = wgrad_bgroup(B, T, Cin, Cout, taps, slot_mode);
    MM_REQUIRE(!slot_mode || nrep >= ceil_div(B, a.bgroup) * ceil_div(T, a.rows_per_wg),
               "conv1d_wgrad: slot mode needs %d slots (mm_conv1d_wgrad_slots), got %d", ceil_div(B, a.bgroup) * ceil_div(T, a.rows_per_wg), nrep);
    switch (taps) {
        case 1: return launch_wgrad<1>(a, st);
        case 3: return launch_wgrad<3>(a, st);
        case 5: return launch_wgrad<5>(a, st);
        case 7: return launch_wgrad<7>(a, st);
        default: return mm_fail(MM_ERR_UNSUPPORTED, "conv1d_wgrad: taps=%d (1,3,5,7)", taps);
    }
}

// desc (host, 64 bytes each): {dy, x, dw(workspace), dbias (nullable)} pointers, then int B, T, Cin, Cout,
// Cin_real, nslots, 2 x pad.  Linear layers only (taps 1, pad 0), slot mode, workspace layout [slot][n][c].
struct WgradManyDesc { const void* dy; const void* x; float* dw; float* dbias; int B, T, Cin, Cout, Cin_real, nslots, p0, p1; };
int mm_conv1d_wgrad_many(const void* desc_host, int n, hipStream_t st) {
    MM_REQUIRE(desc_host && n > 0, "conv1d_wgrad_many: bad args");
    const WgradManyDesc* d = (const WgradManyDesc*)desc_host;
    for (int base = 0; base < n; base += WM_MAX) {
        WgradTable tab;
        tab.n = (n - base < WM_MAX) ? n - base : WM_MAX;
        int total = 0;
        for (int i = 0; i < tab.n; ++i) {
            const WgradManyDesc& q = d[base + i];
            MM_REQUIRE(q.dy && q.x && q.dw && q.B > 0 && q.T > 0, "conv1d_wgrad_many: null/invalid");
            MM_REQUIRE(q.Cin % 8 == 0 && q.Cout % 8 == 0 && q.Cin_real > 0 && q.Cin_real <= q.Cin,
                       "conv1d_wgrad_many: Cin=%d Cout=%d", q.Cin, q.Cout);
            WgradArgs& a = tab.a[i];
            a.dy = (const bf16*)q.dy; a.x = (const bf16*)q.x; a.dw = q.dw; a.dbias = q.dbias;
            a.B = q.B; a.T = q.T; a.Cin = q.Cin; a.Cout = q.Cout; a.pad = 0; a.Cin_real = q.Cin_real;
            a.sn = q.Cin; a.sc = 1; a.stap = q.Cin; a.nrep = q.nslots; a.rep_stride = (long)q.Cout * q.Cin; a.slot_mode = 1;
            a.rows_per_wg = wgrad_many_rows_per_wg(q.T, q.Cin, q.Cout);
            a.bgroup = 1;
            const int chunks = q.B * ceil_div(q.T, a.rows_per_wg);
            MM_REQUIRE(q.nslots == chunks, "conv1d_wgrad_many: needs exactly %d slots (mm_conv1d_wgrad_many_slots), got %d",
                       chunks, q.nslots);
            tab.first[i] = total;
            tab.gx[i] = chunks; tab.gy[i] = ceil_div(q.Cout, 128);
            total += chunks * tab.gy[i] * ceil_div(q.Cin, 128);
        }
        tab.first[tab.n] = total;
        hipLaunchKernelGGL(conv1d_wgrad_many_kernel, dim3(total), dim3(256), 0, st, tab);
        const int rc = mm_check_launch("conv1d_wgrad_many");
        if (rc) return rc;
    }
    return 0;
}

// many independent reductions into parameter gradients in one launch: desc[i] = {src, dst, K, nrep, stride};
// nrep = MM_ACC_REPL: src is a fixed-point accumulator workspace (stride in 64-bit elements);
// nrep = 1: src is a compact fp32 vector (plain dst[k] += src[k]);
// nrep = -R: src is R fp32 rows `stride` floats apart (per-sample partial rows, one writer each): dst[k] += their sum in
// ascending row order
struct ReduceDesc { const void* src; float* dst; long K, nrep, stride; };
static bool reduce_desc_ok(const ReduceDesc& d) {
    return d.src && d.dst && d.K > 0 && d.stride >= d.K && (d.nrep == 1 || d.nrep < 0 || (d.nrep == MM_ACC_REPL && ((uintptr_t)d.src & 7) == 0));
}
constexpr int RM_MAX = 64;
struct ReduceTable { ReduceDesc d[RM_MAX]; };      // passed BY VALUE (kernel argument): no memcpy node,
                                                   // so the launch can be recorded in a hipGraph
__device__ __forceinline__ void reduce_body(const ReduceDesc& d, int blk, int nblk) {
    if (d.nrep == 1) {
        const float* src = reinterpret_cast<const float*>(d.src);
        for (long k = (long)blk * 256 + threadIdx.x; k < d.K; k += (long)nblk * 256) d.dst[k] += src[k];
        return;
    }
    if (d.nrep < 0) {
        const float* src = reinterpret_cast<const float*>(d.src);
        for (long k = (long)blk * 256 + threadIdx.x; k < d.K; k += (long)nblk * 256) {
            float s = src[k];
            for (long r = 1; r < -d.nrep; ++r) s += src[r * d.stride + k];
            d.dst[k] += s;
        }
        return;
    }
    acc_reduce_rows(reinterpret_cast<const mm_acc_t*>(d.src), d.dst, d.K, d.stride, (long)blk * 16, (long)nblk * 16);
}
__global__ void reduce_many_kernel(ReduceTable tab) { reduce_body(tab.d[blockIdx.y], blockIdx.x, gridDim.x); }

// the slot sums AND the accumulator reductions of one gradient flush in ONE launch (they are independent; two graph
// nodes cost ~5 us of latency each on the stream that flushes): blocks [0, 256 ns) scatter, the rest reduce
constexpr int FM_MAX = 48, FM_SB = 256, FM_RB = 16;
struct FlushTable { ScatterDesc s[FM_MAX]; ReduceDesc r[FM_MAX]; int ns, nr; };
__global__ void flush_many_kernel(FlushTable tab) {
    const int b = blockIdx.x;
    if (b < tab.ns * FM_SB) scatter_body(tab.s[b / FM_SB], b % FM_SB, FM_SB);
    else reduce_body(tab.r[(b - tab.ns * FM_SB) / FM_RB], (b - tab.ns * FM_SB) % FM_RB, FM_RB);
}

int mm_reduce_many(const void* desc_host, int ndesc, hipStream_t st) {
    MM_REQUIRE(desc_host && ndesc > 0, "reduce_many: bad args");
    const ReduceDesc* src = (const ReduceDesc*)desc_host;
    for (int base = 0; base < ndesc; base += RM_MAX) {
        ReduceTable tab;
        const int n = ndesc - base < RM_MAX ? ndesc - base : RM_MAX;
        for (int i = 0; i < n; ++i) {
            tab.d[i] = src[base + i];
            MM_REQUIRE(reduce_desc_ok(tab.d[i]), "reduce_many: descriptor %d (nrep = 1 fp32 vector, or %d accumulator replicas)", base + i,
                       MM_ACC_REPL);
        }
        hipLaunchKernelGGL(reduce_many_kernel, dim3(16, n), dim3(256), 0, st, tab);
    }
    return mm_check_launch("reduce_many");
}

int mm_reduce_replicas(const float* src, float* dst, int K, int nrep, int64_t rep_stride, hipStream_t st) {
    MM_REQUIRE(src && dst && K > 0 && nrep >= 1 && rep_stride >= K, "reduce_replicas: bad args");
    hipLaunchKernelGGL(reduce_replicas_kernel, dim3(ceil_div(K, 8)), dim3(256), 0, st, src, dst, K, nrep, (long)rep_stride);
    return mm_check_launch("reduce_replicas");
}

int mm_flush_many(const void* scatter_desc_host, int nscatter, const void* reduce_desc_host, int nreduce, hipStream_t st) {
    MM_REQUIRE(nscatter >= 0 && nreduce >= 0 && nscatter + nreduce > 0 && (scatter_desc_host || !nscatter) &&
                   (reduce_desc_host || !nreduce), "flush_many: bad args");
    const ScatterDesc* sd_in = (const ScatterDesc*)scatter_desc_host;
    const ReduceDesc* rd = (const ReduceDesc*)reduce_desc_host;
    static_assert(sizeof(FlushTable) <= 4096, "kernel arguments");
    // every scatter descriptor gets FM_SB workgroups: a big workspace (config #5's merged convolution: 8.4 M weights) is dealt
    // out as up to 8 descriptors over slices of its output channels, so that it gets 8 x the workgroups
    constexpr int EXP_MAX = 1024;
    static thread_local ScatterDesc expanded[EXP_MAX];
    int nexp = 0;
    for (int i = 0; i < nscatter; ++i) {
        const ScatterDesc& d = sd_in[i];
        MM_REQUIRE(scatter_desc_ok(d), "flush_many: scatter descriptor %d", i);
        const int tws = scatter_ws_taps(d);
        const size_t elems = (size_t)d.Cout * scatter_taps(d) * d.Cinp;
        int parts = (int)((elems + (1u << 20) - 1) >> 20);
        if (parts > 8) parts = 8;
        if (parts > d.Cout) parts = d.Cout;
        if (parts < 1) parts = 1;
        MM_REQUIRE(nexp + parts <= EXP_MAX, "flush_many: too many scatter descriptors");
        for (int q = 0; q < parts; ++q) {
            const int o0 = (int)((long)d.Cout * q / parts), o1 = (int)((long)d.Cout * (q + 1) / parts);
            ScatterDesc e = d;
            e.ws = d.ws + (size_t)o0 * tws * d.Cinp;
            e.dw = d.dw + (size_t)o0 * d.Cin * scatter_taps(d);
            e.Cout = o1 - o0;
            e.cout_all = d.cout_all ? d.cout_all : d.Cout;
            expanded[nexp++] = e;
        }
    }
    const ScatterDesc* sd = expanded;
    nscatter = nexp;
    for (int sb = 0, rb = 0; sb < nscatter || rb < nreduce; sb += FM_MAX, rb += FM_MAX) {
        FlushTable tab;
        tab.ns = nscatter - sb > FM_MAX ? FM_MAX : (nscatter - sb > 0 ? nscatter - sb : 0);
        tab.nr = nreduce - rb > FM_MAX ? FM_MAX : (nreduce - rb > 0 ? nreduce - rb : 0);
        for (int i = 0; i < tab.ns; ++i) tab.s[i] = sd[sb + i];
        for (int i = 0; i < tab.nr; ++i) {
            const ReduceDesc& d = rd[rb + i];
            MM_REQUIRE(reduce_desc_ok(d), "flush_many: reduce descriptor %d (nrep = 1 fp32 vector, or %d accumulator replicas)", rb + i,
                       MM_ACC_REPL);
            tab.r[i] = d;
        }
        hipLaunchKernelGGL(flush_many_kernel, dim3(tab.ns * FM_SB + tab.nr * FM_RB), dim3(256), 0, st, tab);
    }
    return mm_check_launch("flush_many");
}

int mm_acc_reduce(const float* acc, float* dst, int K, int64_t rep_stride, hipStream_t st) {
    MM_REQUIRE(acc && dst && K > 0 && rep_stride >= K, "acc_reduce: bad args");
    MM_REQUIRE(((uintptr_t)acc & 7) == 0, "acc_reduce: workspace must be 8-byte aligned");
    hipLaunchKernelGGL(acc_reduce_kernel, dim3(ceil_div(K, 16)), dim3(256), 0, st, reinterpret_cast<const mm_acc_t*>(acc), dst, K,
                       (long)rep_stride);
    return mm_check_launch("acc_reduce");
}

int mm_wgrad_scatter(const float* ws, float* dw, int Cout, int Cin, int taps, int Cinp, int nrep, hipStream_t st) {
    MM_REQUIRE(ws && dw && Cout > 0 && Cin > 0 && taps > 0 && Cinp >= Cin && nrep >= 1, "wgrad_scatter: bad args");
    const size_t total = (size_t)Cout * Cin * taps;
    int grid = (int)((total + 255) / 256);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(wgrad_scatter_kernel, dim3(grid), dim3(256), 0, st, ws, dw, Cout, Cin, taps, Cinp, nrep);
    return mm_check_launch("wgrad_scatter");
}

int mm_scatter_many(const void* desc_host, int ndesc, hipStream_t st) {
    MM_REQUIRE(desc_host && ndesc > 0, "scatter_many: bad args");
    const ScatterDesc* src = (const ScatterDesc*)desc_host;
    for (int base = 0; base < ndesc; base += SM_MAX) {
        ScatterTable tab;
        const int n = ndesc - base < SM_MAX ? ndesc - base : SM_MAX;
        for (int i = 0; i < n; ++i) {
            const ScatterDesc& d = src[base + i];
            MM_REQUIRE(scatter_desc_ok(d), "scatter_many: descriptor %d", base + i);
            tab.d[i] = d;
        }
        hipLaunchKernelGGL(scatter_many_kernel, dim3(256, n), dim3(256), 0, st, tab);
    }
    return mm_check_launch("scatter_many");
}

}  // extern "C"
