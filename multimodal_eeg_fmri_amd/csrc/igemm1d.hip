// 1-D implicit-GEMM family on bf16 MFMA (fp32 accumulate), channels-last.
//
//   forward : Y[b,t,n]  = sum_{tap,c} X[b, t+tap-pad, c] * W[n, tap, c]
//   (a Linear layer is the taps == 1 case; data-gradient is the same kernel
//    run on dY with the flipped/transposed weight image)
//   wgrad   : dW[n,tap,c] = sum_{b,t} dY[b,t,n] * X[b, t+tap-pad, c]
//
// Layouts: X [B][T][Cin] bf16 (Cin % 16 == 0), W [Cout][taps][Cin] bf16,
// Y [B][T/pool][Cout].  One workgroup = 256 threads = 4 waves computes a
// BM x BN output tile of ONE batch item: the (BM + taps - 1) x KC halo tile of
// X is staged once per Cin-chunk into LDS and every tap reads it at a row
// offset (the im2col matrix is never materialised); W for the chunk sits
// beside it.  Rows are padded by 16 B so the 16-lane groups of ds_read_b128
// hit 16 distinct 16-B slots (row stride = odd multiple of 16 B).
//
// This file: the forward / data-gradient kernel, its split-K second half and the tile dispatch, then the two fused
// transformer-row kernels (ffn_rows_*), each of the two groups with its entry points below it.  igemm1d.h has the argument structs, the
// epilogues and the host argument builders; igemm1d_pack.hip the layout packers and weight images; igemm1d_wgrad.hip the
// weight gradient.
#include "igemm1d.h"

#include <cstdio>
#include <cstdlib>

namespace {

// FEAT: epilogue combination (EF_ANY = all run-time); TAPS > 0: compiled for that tap count (1 = the Linear layers)
template <int BM, int BN, int WM, int WN, int KCT, unsigned FEAT, int TAPS>
__global__ __launch_bounds__(256, 2) void conv1d_fwd_kernel(ConvArgs a) {
    if (TAPS > 0) a.taps = TAPS;
    constexpr int TM = BM / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    static_assert(WM * WN == 4, "4 waves");
    constexpr int AS = KCT + KPAD;                // LDS row stride (elements)
    constexpr int SEGS = KCT / 8;                 // 16-B segments per row
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tilesT = (a.T + BM - 1) / BM;
    const int b = blockIdx.x / tilesT;
    const int t0 = (blockIdx.x % tilesT) * BM;
    const int n0 = blockIdx.y * BN;
    const int arows = BM + a.taps - 1;
    bf16* As = reinterpret_cast<bf16*>(smem);
    bf16* Ws = As + arows * AS;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const bf16* xb = a.x + (size_t)b * a.T * a.Cin;
    const int lr = lane & 31, lh = lane >> 5;
    const int wrows = BN * a.taps;
    const int wvalid = (a.Cout - n0) * a.taps;    // rows >= wvalid are beyond Cout -> zeros

    // staging goes through register batches: all loads of a batch are in flight before the first LDS
    // write (a load->store loop serialises on load latency).  The first activation batch and the first
    // weight batch are issued TOGETHER (one global round trip per K chunk for the Linear layers instead of
    // two); whatever does not fit (k > 1 convs) follows in further batches.
    // (only the 32-row Linear tile: at 64 rows the 12 staging registers sets cost the third wave per SIMD)
    constexpr bool MERGE = BM == 32;
    constexpr int NA = MERGE ? 2 : 4, NB = 8;
    const bf16* wb = a.w + (size_t)n0 * a.taps * a.Cin;
    const int nA = arows * SEGS, nW = wrows * SEGS;
    auto load_a = [&](int s, int c0) {
        const int r = s / SEGS, sg = s % SEGS;
        const int t = t0 - a.pad + r;
        return (s < nA && t >= 0 && t < a.T) ? *reinterpret_cast<const uint4*>(xb + (size_t)t * a.Cin + c0 + sg * 8)
                                             : make_uint4(0, 0, 0, 0);
    };
    auto load_w = [&](int s, int c0) {
        const int r = s / SEGS, sg = s % SEGS;             // r = n_local * taps + tap
        return (s < nW && r < wvalid) ? *reinterpret_cast<const uint4*>(wb + (size_t)r * a.Cin + c0 + sg * 8)
                                      : make_uint4(0, 0, 0, 0);
    };
    const int c_lo = a.partial ? (int)blockIdx.z * a.csplit : 0;
    const int c_hi = a.partial ? min(a.Cin, c_lo + a.csplit) : a.Cin;
    for (int c0 = c_lo; c0 < c_hi; c0 += KCT) {
        if (c0 != c_lo) __syncthreads();
        if constexpr (MERGE) {
            uint4 va[NA], vw[NB];
#pragma unroll
            for (int i = 0; i < NA; ++i) va[i] = load_a(i * 256 + tid, c0);
#pragma unroll
            for (int i = 0; i < NB; ++i) vw[i] = load_w(i * 256 + tid, c0);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int s = i * 256 + tid;
                if (s < nA) *reinterpret_cast<uint4*>(As + (s / SEGS) * AS + (s % SEGS) * 8) = va[i];
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int s = i * 256 + tid;
                if (s < nW) *reinterpret_cast<uint4*>(Ws + (s / SEGS) * AS + (s % SEGS) * 8) = vw[i];
            }
        }
        for (int base = MERGE ? NA * 256 : 0; base < nA; base += NA * 256) {
            uint4 v[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) v[i] = load_a(base + i * 256 + tid, c0);
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int s = base + i * 256 + tid;
                if (s < nA) *reinterpret_cast<uint4*>(As + (s / SEGS) * AS + (s % SEGS) * 8) = v[i];
            }
        }
        for (int base = MERGE ? NB * 256 : 0; base < nW; base += NB * 256) {
            uint4 v[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) v[i] = load_w(base + i * 256 + tid, c0);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int s = base + i * 256 + tid;
                if (s < nW) *reinterpret_cast<uint4*>(Ws + (s / SEGS) * AS + (s % SEGS) * 8) = v[i];
            }
        }
        __syncthreads();
        for (int tap = 0; tap < a.taps; ++tap) {
#pragma unroll
            for (int ks = 0; ks < KCT; ks += 16) {
                bf16x8 af[TM], bfr[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int row = (wm * TM + i) * 32 + lr + tap;
                    af[i] = *reinterpret_cast<const bf16x8*>(As + row * AS + ks + lh * 8);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int nl = (wn * TN + j) * 32 + lr;
                    bfr[j] = *reinterpret_cast<const bf16x8*>(Ws + (nl * a.taps + tap) * AS + ks + lh * 8);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    __syncthreads();                               // staging LDS is dead: reuse as the C tile
    constexpr int LDC = BN + 4;
    float* Cs = reinterpret_cast<float*>(smem);
    float* sstat = Cs + BM * LDC;                  // [2][BN]
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                Cs[row * LDC + (wn * TN + j) * 32 + lr] = acc[i][j][r];
            }
    if (a.partial) {                               // split-K: the raw tile of this channel range, no epilogue
        __syncthreads();
        float* dst = a.partial + ((size_t)blockIdx.z * a.B + b) * a.T * a.Cout;
        for (int i = tid; i < BM * (BN / 4); i += 256) {
            const int row = i / (BN / 4), n = n0 + (i % (BN / 4)) * 4;
            if (t0 + row < a.T && n < a.Cout)
                *reinterpret_cast<float4*>(dst + (size_t)(t0 + row) * a.Cout + n) = *reinterpret_cast<const float4*>(Cs + row * LDC + (n - n0));
        }
        return;
    }
    if (a.e.stats || a.e.ln_dgb)
        for (int i = tid; i < 2 * BN; i += 256) sstat[i] = 0.f;
    __syncthreads();
    if constexpr (BM == 32 && BN == 128) {
        if ((FEAT == EF_ANY && a.e.ln_x) || (FEAT != EF_ANY && (FEAT & EF_LNBWD))) {
            const bool gemm2 = FEAT == EF_ANY ? a.e.w2 != nullptr : (FEAT & EF_GEMM2) != 0;
            bf16* a2 = gemm2 ? reinterpret_cast<bf16*>(smem + (BM * LDC + 2 * BN) * sizeof(float)) : nullptr;   // behind the C tile
            epilogue_ln_bwd<BM, BN, FEAT>(Cs, a.e, tid, b, t0, a.T, sstat, a2);
            if (gemm2) {
                __syncthreads();                  // the C tile is dead: it stages the outputs, the copy's tiles follow a2
                second_gemm<FEAT, false>(a2, a.e, (size_t)b * a.T + t0, tid, wn, lr, lh, reinterpret_cast<bf16*>(smem), a2 + 32 * A2S);
            }
            return;
        }
    }
    if constexpr (BM == 64 && BN == 64) {
        if ((FEAT == EF_ANY && a.e.bn.y) || (FEAT != EF_ANY && (FEAT & EF_BNRED))) {
            epilogue_bn_reduce<BM, BN, FEAT>(Cs, a.e, tid, b, t0, a.T, n0, a.Cout);
            return;
        }
    }
    if constexpr (BM == 32 && BN == 128) {
        // forward: the LayerNorm rows of the fused next pre-norm (EF_LNF) feed a second GEMM (the next block's QKV projection)
        const bool gemm2 = FEAT == EF_ANY ? a.e.w2 != nullptr : (FEAT & EF_GEMM2) != 0;
        if (gemm2) {
            bf16* a2 = reinterpret_cast<bf16*>(smem + (BM * LDC + 2 * BN) * sizeof(float));
            epilogue_rows<BM, BN, FEAT>(Cs, a.e, tid, b, t0, a.T, n0, a.Cout, sstat, a2);
            __syncthreads();
            second_gemm<FEAT, false>(a2, a.e, (size_t)b * a.T + t0, tid, wn, lr, lh, reinterpret_cast<bf16*>(smem), a2 + 32 * A2S);
            return;
        }
    }
    epilogue_rows<BM, BN, FEAT>(Cs, a.e, tid, b, t0, a.T, n0, a.Cout, sstat);
}

// second half of a split-K launch: the slices are added in slice order (same bits every run) into the C tile, then the
// ordinary epilogue runs on it (generic form: every step behind its run-time test, bit-equal to the compiled-in forms)
template <int BM, int BN>
__global__ __launch_bounds__(256) void conv1d_splitk_epilogue_kernel(ConvArgs a, int nsplit) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int LDC = BN + 4;
    float* Cs = reinterpret_cast<float*>(smem);
    float* sstat = Cs + BM * LDC;
    const int tid = threadIdx.x;
    const int tilesT = (a.T + BM - 1) / BM;
    const int b = blockIdx.x / tilesT, t0 = (blockIdx.x % tilesT) * BM, n0 = blockIdx.y * BN;
    const size_t slice = (size_t)a.B * a.T * a.Cout;
    const float* src = a.partial + (size_t)b * a.T * a.Cout;
    for (int i = tid; i < BM * (BN / 4); i += 256) {
        const int row = i / (BN / 4), n = n0 + (i % (BN / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + row < a.T && n < a.Cout) {
            const float* p = src + (size_t)(t0 + row) * a.Cout + n;
            v = *reinterpret_cast<const float4*>(p);
            for (int z = 1; z < nsplit; ++z) {
                const float4 u = *reinterpret_cast<const float4*>(p + z * slice);
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
        }
        *reinterpret_cast<float4*>(Cs + row * LDC + (n - n0)) = v;
    }
    if (a.e.stats || a.e.ln_dgb)
        for (int i = tid; i < 2 * BN; i += 256) sstat[i] = 0.f;
    __syncthreads();
    epilogue_rows<BM, BN, EF_ANY>(Cs, a.e, tid, b, t0, a.T, n0, a.Cout, sstat);
}

template <int BM, int BN, int WM, int WN, int KCT, unsigned FEAT, int TAPS = 0>
int launch_fwd_feat(const ConvArgs& a, hipStream_t st) {
    const size_t stage = (size_t)(BM + a.taps - 1 + BN * a.taps) * (KCT + KPAD) * sizeof(bf16);
    const size_t ctile = (size_t)(BM * (BN + 4) + 2 * BN) * sizeof(float);
    size_t need = stage > ctile ? stage : ctile;
    // second GEMM: its operand rows behind the C tile, then (pre-activation copy only) that copy's two staging tiles
    const size_t g2 = ctile + A2B + (a.e.pre2 ? 2 * A2B : 0);
    if (a.e.w2 && need < g2) need = g2;
    if (need > 160 * 1024) return mm_fail(MM_ERR_UNSUPPORTED, "conv1d_fwd: LDS %zu B > 160 KiB", need);
    auto kern = conv1d_fwd_kernel<BM, BN, WM, WN, KCT, FEAT, TAPS>;
    if (need > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    dim3 grid(a.B * ceil_div(a.T, BM), ceil_div(a.Cout, BN));
    if (a.partial) {
        const int nsplit = ceil_div(a.Cin, a.csplit);
        grid.z = nsplit;
        hipLaunchKernelGGL(kern, grid, dim3(256), need, st, a);
        int rc = mm_check_launch("conv1d_fwd(split-K)");
        if (rc) return rc;
        grid.z = 1;
        hipLaunchKernelGGL((conv1d_splitk_epilogue_kernel<BM, BN>), grid, dim3(256), ctile, st, a, nsplit);
        return mm_check_launch("conv1d_fwd(split-K epilogue)");
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), need, st, a);
    return mm_check_launch("conv1d_fwd");
}

// the combinations of the contrastive training step, each on the tile shape it runs on;
// everything else takes the generic epilogue
template <int BM, int BN, int WM, int WN, int KCT>
int launch_fwd(const ConvArgs& a, hipStream_t st) {
    const unsigned m = epi_mask(a.e);
    if (getenv("MM_EPI_GENERIC") || a.partial || (a.e.w2 && a.e.act2 && a.e.act2 != MM_ACT_GELU)) return launch_fwd_feat<BM, BN, WM, WN, KCT, EF_ANY>(a, st);      // tests: generic vs compiled-in epilogues; split-K
#define EPI_CASE(mask) case (mask): return launch_fwd_feat<BM, BN, WM, WN, KCT, (mask), LT>(a, st);
    if constexpr (BM == 64 && BN == 128 && KCT == 128) {
        constexpr int LT = 1;                 // the Linear layers: one tap
        if (a.taps == 1) switch (m) {
            EPI_CASE(EF_SHIFT | EF_BF16)   // QKV projection: bias, bf16 out
            EPI_CASE(EF_SHIFT | EF_BF16 | EF_DROP | EF_PRE | ef_act(MM_ACT_GELU))   // FFN-1 forward: bias, GELU, dropout, pre-activation copy, bf16 out
            EPI_CASE(EF_BF16 | EF_DROP | EF_GRADZ | ef_act(MM_ACT_GELU, EFA_GRADZ))   // FFN-2 data gradient: GELU', dropout mask, bf16 out
            default: break;
        }
    } else if constexpr (BM == 32 && BN == 128 && KCT == 128) {
        constexpr int LT = 1;
        if (a.taps == 1) switch (m) {
            EPI_CASE(EF_SHIFT | EF_F32 | EF_DROP | EF_RES | EF_LNF)   // out-proj / FFN-2 forward: bias, dropout, residual, fp32 out, LayerNorm of the result
            EPI_CASE(EF_SHIFT | EF_F32 | EF_DROP | EF_RES | EF_LNF | EF_GEMM2)   // ... and the next block's QKV projection of those LayerNorm rows (second GEMM)
            EPI_CASE(EF_SHIFT | EF_F32 | EF_DROP | EF_RES | EF_LNF | EF_GEMM2 | EF_G2FFN1)   // out-projection, norm2 and the first FFN Linear of those rows (second GEMM: GELU, dropout, pre-activation copy)
            EPI_CASE(EF_SHIFT | EF_F32 | EF_DROP | EF_RES | EF_POOLOUT)   // last FFN-2 forward: ... and the mean over tokens instead of the LayerNorm
            EPI_CASE(EF_BF16)   // plain data gradient, bf16 out
            EPI_CASE(EF_LNBWD | EF_RES | EF_F32 | EF_BF16 | EF_DROP)   // data gradient + LayerNorm backward: skip gradient in, fp32 and masked bf16 out
            EPI_CASE(EF_LNBWD | EF_RES | EF_F32 | EF_BF16 | EF_DROP | EF_GEMM2)   // ... and the data gradient of the Linear under that LayerNorm's skip path (second GEMM)
            EPI_CASE(EF_LNBWD | EF_RES | EF_F32)   // the same without the bf16 copy (first block)
            EPI_CASE(EF_LNBWD | EF_RES | EF_F32 | EF_BNRED | ef_act(MM_ACT_GELU, EFA_BN))   // ... + the BatchNorm-backward reduce of the conv block below the stack (GELU)
            default: break;
        }
    } else if constexpr (BM == 64 && BN == 64 && KCT == 64) {
        constexpr int LT = 0;                 // k = 3, 5, 7 convolutions: tap count at run time
        switch (m) {
            EPI_CASE(EF_SHIFT | EF_F32 | EF_STATS)   // conv block forward: bias, BatchNorm sums, fp32 out
            EPI_CASE(EF_BF16)   // conv data gradient, bf16 out
            EPI_CASE(EF_BF16 | EF_BNRED | ef_act(MM_ACT_GELU, EFA_BN))   // ... + the BatchNorm-backward reduce of the layer below (GELU)
            EPI_CASE(EF_BF16 | EF_BNRED | EF_BNPOOL2 | ef_act(MM_ACT_GELU, EFA_BN))   // ... the same below a MaxPool1d(2)
            default: break;
        }
    }
#undef EPI_CASE
    return launch_fwd_feat<BM, BN, WM, WN, KCT, EF_ANY>(a, st);
}

// K-chunk width: full-K staging for the linears (taps == 1), else the widest of 64 / 32 / 16 that divides Cin
static int fwd_kchunk(int taps, int Cin) {
    return (taps == 1 && Cin % 128 == 0) ? 128 : (Cin % 64 == 0 ? 64 : (Cin % 32 == 0 ? 32 : 16));
}

template <int BM, int BN, int WM, int WN>
int launch_fwd_tile(const ConvArgs& a, hipStream_t st) {
    switch (fwd_kchunk(a.taps, a.Cin)) {
        case 16: return launch_fwd<BM, BN, WM, WN, 16>(a, st);
        case 32: return launch_fwd<BM, BN, WM, WN, 32>(a, st);
        case 64: return launch_fwd<BM, BN, WM, WN, 64>(a, st);
        default: return launch_fwd<BM, BN, WM, WN, 128>(a, st);
    }
}

static int conv1d_dispatch(const ConvArgs& a, hipStream_t st) {
    // tile choice: BN = 64 for the k>1 convs (64-wide chunks) so that two workgroups fit one CU's LDS
    if (a.Cout <= 64 || a.taps > 1) return launch_fwd_tile<64, 64, 2, 2>(a, st);
    // few row tiles (M <= 16k): halve BM so that >= 2 workgroups share a CU and overlap
    if ((long)a.B * ceil_div(a.T, 64) * ceil_div(a.Cout, 128) <= 512) return launch_fwd_tile<32, 128, 1, 4>(a, st);
    return launch_fwd_tile<64, 128, 2, 2>(a, st);
}

// split-K plan of a forward launch: only the k > 1 convolutions on the 64 x 64 x 64 tile, when the output tiles do not
// fill the chip and the reduction is long.  -> number of channel slices (1 = run it whole)
static int conv1d_splitk_slices(int B, int T, int Cin, int Cout, int taps) {
    if (taps == 1 || Cin % 64) return 1;
    const long tiles = (long)B * ceil_div(T, 64) * ceil_div(Cout, 64);
    const int chunks = Cin / 64;
    if (tiles >= 192 || chunks < 16) return 1;
    long n = 512 / tiles;                       // ~2 workgroups per CU
    if (n > chunks / 8) n = chunks / 8;         // >= 8 chunks per slice
    if (n > 8) n = 8;
    return n < 2 ? 1 : (int)n;
}

// a Linear with 128 outputs on the 32 x 128 tile (the fused LayerNorm epilogues hold a whole row in one workgroup),
// at the widest chunk that divides K
static int launch_fwd_32x128(const ConvArgs& a, hipStream_t st) { return launch_fwd_tile<32, 128, 1, 4>(a, st); }

}  // namespace

// ============================================================================
// C ABI (declared in include/mmeeg_hip.h)
// ============================================================================
extern "C" {

int mm_conv1d_fwd_splitk_plan(int B, int T, int Cin, int Cout, int taps, int* nsplit_host, int64_t* ws_floats_host, hipStream_t) {
    MM_REQUIRE(nsplit_host && ws_floats_host && B > 0 && T > 0 && Cin > 0 && Cout > 0 && taps >= 1, "conv1d_fwd_splitk_plan: bad args");
    const int n = conv1d_splitk_slices(B, T, Cin, Cout, taps);
    *nsplit_host = n;
    *ws_floats_host = n > 1 ? (int64_t)n * B * T * Cout : 0;
    return 0;
}

int mm_conv1d_fwd_splitk(const void* x, const void* w, int B, int T, int Cin, int Cout, int taps, int pad,
                         const float* scale, const float* shift, int act, const float* residual, const float* pe,
                         int pool, float* stats, float* out_f32, void* out_bf16, void* out_pre,
                         float drop_p, uint32_t drop_seed, const uint32_t* seed_epoch, const void* gradz, int gradz_act,
                         float* ws, int nsplit, hipStream_t st) {
    ConvArgs a;
    int rc = conv1d_fwd_args(a, x, w, B, T, Cin, Cout, taps, pad, scale, shift, act, residual, pe, pool, stats, out_f32, out_bf16,
                             out_pre, drop_p, drop_seed, seed_epoch, gradz, gradz_act);
    if (rc) return rc;
    MM_REQUIRE(ws && nsplit >= 2 && nsplit <= 64, "conv1d_fwd_splitk: workspace / nsplit=%d", nsplit);
    MM_REQUIRE(taps > 1 && Cin % 64 == 0, "conv1d_fwd_splitk: k > 1 convolutions with Cin %% 64 == 0 only (taps=%d Cin=%d)", taps, Cin);
    const int chunks = Cin / 64;
    a.csplit = ceil_div(chunks, nsplit) * 64;
    MM_REQUIRE(ceil_div(Cin, a.csplit) >= 2, "conv1d_fwd_splitk: nsplit=%d leaves one slice", nsplit);
    a.partial = ws;                               // ceil(Cin / csplit) <= nsplit slices of B * T * Cout floats
    return conv1d_dispatch(a, st);
}

// Generic forward implicit GEMM.  See include/mmeeg_hip.h for the contract.
int mm_conv1d_fwd(const void* x, const void* w, int B, int T, int Cin, int Cout, int taps, int pad,
                  const float* scale, const float* shift, int act, const float* residual, const float* pe,
                  int pool, float* stats, float* out_f32, void* out_bf16, void* out_pre,
                  float drop_p, uint32_t drop_seed, const uint32_t* seed_epoch, const void* gradz, int gradz_act,
                  hipStream_t st) {
    ConvArgs a;
    int rc = conv1d_fwd_args(a, x, w, B, T, Cin, Cout, taps, pad, scale, shift, act, residual, pe, pool, stats, out_f32, out_bf16,
                             out_pre, drop_p, drop_seed, seed_epoch, gradz, gradz_act);
    return rc ? rc : conv1d_dispatch(a, st);
}

// Data-gradient convolution of a conv block (dy (B, T, Cin) bf16 x that block's dgrad weight image -> dx (B, T, Cout)
// bf16) with the BatchNorm-backward REDUCE pass of the block below as its epilogue: dx is that block's d(out), and its
// sums (sum dz | sum dz * xhat over the B * T * pool pre-BN rows y_below) land in sums_below exactly as
// mm_bn_act_bwd_reduce(y_below, out4_below, dx, nullptr, sums_below, B, T * pool, Cout, ...) would leave them.
int mm_conv1d_dgrad_bn_reduce(const void* dy, const void* w_dgrad, int B, int T, int Cin, int Cout, int taps, int pad,
                              void* dx_bf16, const float* y_below, const float* out4_below, float* sums_below, int act,
                              int pool, int drop_first, float drop_p, uint32_t seed, const uint32_t* seed_epoch,
                              hipStream_t st) {
    MM_REQUIRE(dy && w_dgrad && dx_bf16 && y_below && out4_below && sums_below, "conv1d_dgrad_bn_reduce: null");
    MM_REQUIRE(B > 0 && T > 0 && Cout > 0 && taps >= 1 && taps <= 9 && pad >= 0 && pad < taps, "conv1d_dgrad_bn_reduce: bad dims");
    MM_REQUIRE(Cin > 0 && Cin % 16 == 0 && Cout % 4 == 0, "conv1d_dgrad_bn_reduce: Cin=%d (x16) Cout=%d (x4)", Cin, Cout);
    MM_REQUIRE(taps > 1 || Cout <= 64, "conv1d_dgrad_bn_reduce: the fused reduce runs on the 64 x 64 tile (taps > 1 or Cout <= 64)");
    MM_REQUIRE(pool == 1 || pool == 2, "conv1d_dgrad_bn_reduce: pool=%d", pool);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "conv1d_dgrad_bn_reduce: drop_p");
    MM_REQUIRE((size_t)B * T * pool * Cout < (1ull << 32), "conv1d_dgrad_bn_reduce: 32-bit dropout indices");
    ConvArgs a;
    a.x = (const bf16*)dy; a.w = (const bf16*)w_dgrad;
    a.B = B; a.T = T; a.Cin = Cin; a.Cout = Cout; a.taps = taps; a.pad = pad;
    a.e.out_bf16 = (bf16*)dx_bf16;
    a.e.bn.y = y_below; a.e.bn.out4 = out4_below; a.e.bn.sums = sums_below;
    a.e.bn.act = act; a.e.bn.pool = pool; a.e.bn.drop_first = drop_first;
    const DropH d = mm_drop(drop_p);
    a.e.bn.thresh = d.thresh; a.e.bn.inv_keep = d.inv_keep; a.e.bn.seed = seed; a.e.bn.epoch = seed_epoch;
    return conv1d_dispatch(a, st);
}

int mm_linear_fwd_meanpool(const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                           float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch, float* pool_out,
                           int rows_per_group, hipStream_t st) {
    MM_REQUIRE(pool_out, "linear_fwd_meanpool: null pool_out");
    ConvArgs a;
    const int rc = linear128_fwd_args(a, x, w, M, K, bias, residual, out_f32, drop_p, seed, seed_epoch, pool_out, rows_per_group,
                                      nullptr, nullptr, 0.f, nullptr, nullptr);
    return rc ? rc : launch_fwd_32x128(a, st);
}

int mm_linear_fwd_ln(const void* x, const void* w, int M, int K, const float* bias, const float* residual, float* out_f32,
                     float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* ln_gamma, const float* ln_beta,
                     float ln_eps, void* ln_out_bf16, float* ln_stat, hipStream_t st) {
    MM_REQUIRE(ln_out_bf16, "linear_fwd_ln: null ln_out");
    ConvArgs a;
    const int rc = linear128_fwd_args(a, x, w, M, K, bias, residual, out_f32, drop_p, seed, seed_epoch, nullptr, 0, ln_gamma, ln_beta,
                                      ln_eps, ln_out_bf16, ln_stat);
    return rc ? rc : launch_fwd_32x128(a, st);
}

// mm_linear_fwd_ln followed, inside the launch, by out2 = ln_out @ w2^T + bias2 (M x 128 x n2): the projection that
// consumes the fused LayerNorm's rows (the next TemporalTransformerBlock's in_proj: n2 = 384).  w2 = that Linear's forward
// weight image (n2 rows of 128); bit-identical to mm_conv1d_fwd(ln_out, w2, 1, M, 128, n2, 1, 0, NULL, bias2, ..., bf16 out).
int mm_linear_fwd_ln_gemm2(const void* x, const void* w, int M, int K, const float* bias, const float* residual, float* out_f32,
                           float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* ln_gamma, const float* ln_beta,
                           float ln_eps, void* ln_out_bf16, float* ln_stat, const void* w2, const float* bias2, int n2,
                           void* out2_bf16, hipStream_t st) {
    MM_REQUIRE(ln_out_bf16 && w2 && out2_bf16, "linear_fwd_ln_gemm2: null");
    ConvArgs a;
    const int rc = linear128_fwd_args(a, x, w, M, K, bias, residual, out_f32, drop_p, seed, seed_epoch, nullptr, 0, ln_gamma, ln_beta,
                                      ln_eps, ln_out_bf16, ln_stat, {w2, bias2, n2, out2_bf16});
    return rc ? rc : launch_fwd_32x128(a, st);
}

// mm_linear_fwd_ln_gemm2 with an epilogue on the second GEMM: out2 = dropout(act(ln_out @ w2^T + bias2)), pre2 (nullable) =
// the bf16 pre-activation - the first FFN Linear (128 -> n2 = 512, GELU, Dropout) on the rows of the norm2 that the attention
// out-projection's launch has just formed.  Bit-identical to mm_conv1d_fwd(ln_out, w2, 1, M, 128, n2, 1, 0, NULL, bias2, act,
// ..., out_bf16 = out2, out_pre = pre2, drop2_p, seed2, seed_epoch, ...).
int mm_linear_fwd_ln_gemm2_act(const void* x, const void* w, int M, int K, const float* bias, const float* residual,
                               float* out_f32, float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* ln_gamma,
                               const float* ln_beta, float ln_eps, void* ln_out_bf16, float* ln_stat, const void* w2,
                               const float* bias2, int n2, void* out2_bf16, void* pre2_bf16, int act2, float drop2_p,
                               uint32_t seed2, hipStream_t st) {
    MM_REQUIRE(ln_out_bf16 && w2 && out2_bf16, "linear_fwd_ln_gemm2_act: null");
    ConvArgs a;
    const int rc = linear128_fwd_args(a, x, w, M, K, bias, residual, out_f32, drop_p, seed, seed_epoch, nullptr, 0, ln_gamma, ln_beta,
                                      ln_eps, ln_out_bf16, ln_stat, {w2, bias2, n2, out2_bf16, act2, drop2_p, seed2, pre2_bf16});
    return rc ? rc : launch_fwd_32x128(a, st);
}

int mm_linear_dgrad_ln_bwd(const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                           const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgb_repl,
                           float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t st) {
    ConvArgs a;
    const int rc = linear_dgrad_ln_bwd_args(a, dy, w, M, K, x, stat, gamma, dres, dx, dx_bf16, dgb_repl, drop_p, seed, seed_epoch);
    return rc ? rc : launch_fwd_32x128(a, st);
}

// mm_linear_dgrad_ln_bwd followed, inside the launch, by do = dx_bf16 @ w2 (M x 128 x 128): the data gradient of the
// Linear(128 -> 128) whose dropped-out output entered this LayerNorm's input through the residual add (the attention
// out-projection: x1 = x0 + drop(o Wo^T + bo), norm2(x1)) - dx_bf16 carries exactly that dropout mask (drop_p, seed).
// w2 = that Linear's data-gradient weight image (128 rows of 128); do (M, 128) bf16, bit-identical to
// mm_conv1d_fwd(dx_bf16, w2, ...) with a bf16 output.  dres_rows_per_sample > 0: dres is (M / that, 128) - ONE skip-gradient
// row for that many consecutive rows (the backward of a mean over a sample's tokens, mm_pooled_head_bwd_rows).
int mm_linear_dgrad_ln_bwd_gemm2(const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                                 const float* gamma, const float* dres, float* dx, void* dx_bf16, float* dgb_repl,
                                 float drop_p, uint32_t seed, const uint32_t* seed_epoch, const void* w2, void* do_bf16,
                                 int dres_rows_per_sample, hipStream_t st) {
    MM_REQUIRE(w2 && do_bf16 && dx_bf16, "linear_dgrad_ln_bwd_gemm2: null");
    ConvArgs a;
    const int rc = linear_dgrad_ln_bwd_args(a, dy, w, M, K, x, stat, gamma, dres, dx, dx_bf16, dgb_repl, drop_p, seed, seed_epoch,
                                            nullptr, w2, do_bf16, dres_rows_per_sample);
    return rc ? rc : launch_fwd_32x128(a, st);
}

// mm_linear_dgrad_ln_bwd whose rows dx are the fp32 d(out) of a 128-channel, un-pooled conv block (Conv1d -> BatchNorm1d
// -> act -> Dropout(p) -> + positional table -> Dropout(p2)): that block's BatchNorm-backward reduce pass rides in the same
// launch.  y_below (M, 128) fp32, out4_below, sums_below (zeroed [32][2][128] workspace) and act / drop_p / seed / drop2_p /
// seed2 as in mm_bn_act_bwd_reduce(y_below, out4_below, NULL, dx, sums_below, 1, M, 128, act, 1, 1, ...).
int mm_linear_dgrad_ln_bwd_bn_reduce(const void* dy, const void* w, int M, int K, const float* x, const float* stat,
                                     const float* gamma, const float* dres, float* dx, float* dgb_repl,
                                     const uint32_t* seed_epoch, const float* y_below, const float* out4_below,
                                     float* sums_below, int act, float bn_drop_p, uint32_t bn_seed, float bn_drop2_p,
                                     uint32_t bn_seed2, hipStream_t st) {
    MM_REQUIRE(dx && y_below && out4_below && sums_below, "linear_dgrad_ln_bwd_bn_reduce: null");
    MM_REQUIRE(bn_drop_p >= 0.f && bn_drop_p < 1.f && bn_drop2_p >= 0.f && bn_drop2_p < 1.f, "linear_dgrad_ln_bwd_bn_reduce: drop_p");
    MM_REQUIRE((size_t)M * 128 < (1ull << 32), "linear_dgrad_ln_bwd_bn_reduce: 32-bit dropout indices");
    BnRed bn;
    bn.y = y_below; bn.out4 = out4_below; bn.sums = sums_below; bn.act = act; bn.pool = 1; bn.drop_first = 1;
    const DropH d = mm_drop(bn_drop_p), d2 = mm_drop(bn_drop2_p);
    bn.thresh = d.thresh; bn.inv_keep = d.inv_keep; bn.seed = bn_seed;
    bn.thresh2 = d2.thresh; bn.inv_keep2 = d2.inv_keep; bn.seed2 = bn_seed2;
    bn.epoch = seed_epoch;
    ConvArgs a;
    const int rc = linear_dgrad_ln_bwd_args(a, dy, w, M, K, x, stat, gamma, dres, dx, nullptr, dgb_repl, 0.f, 0u, seed_epoch, &bn);
    return rc ? rc : launch_fwd_32x128(a, st);
}

}  // extern "C"

// ------------------------------------------------------------------ fused transformer rows
// The row-wise part of a width-128 transformer block between two attention kernels, one launch each way: out-projection,
// norm2 and both FFN Linears forward (mm_ffn_rows_fwd), their data gradients and norm2's backward (mm_ffn_rows_bwd).  The
// 32 x n1 hidden tile stays in LDS between the GEMMs.  The epilogues, the second GEMM and the argument builders are those
// of the stand-alone launches (igemm1d.h), so every output keeps the bits of the launches it replaces.  In one translation
// unit with the forward kernel on purpose: profiles/igemm1d_split_ab.txt, section 9.
namespace {
// Everything row-wise between two attention kernels of a width-128 transformer block, one launch: the out-projection
// (+ dropout, residual, norm2) as conv1d_fwd_kernel<32, 128, 1, 4, 128, ..., 1> runs it, the first FFN Linear as its second
// GEMM with the whole 32 x n1 hidden tile KEPT in LDS, then the second FFN Linear on that tile (W2's fragments from its
// L2-resident forward image one 128-chunk ahead, k ascending in 16-steps into one accumulator: the bits of the stand-alone
// launch's 128-chunks), whose C tile goes through the unchanged epilogue_rows with the x1 rows this workgroup has just
// written as its residual.  c = the first launch's arguments (Cin == Cout == 128, taps 1, B 1), t = the FFN-2 epilogue's.
struct FfnRowsArgs { ConvArgs c; const bf16* w3; EpiArgs t; };
// SPEC: the training step's epilogue combinations compiled in (else every step behind its run-time test)
// TAIL: what consumes the finished rows - 0 LayerNorm, 1 LayerNorm + a second GEMM on its rows, 2 the mean over tokens
template <bool SPEC, int TAIL>
__global__ __launch_bounds__(256, 2) void ffn_rows_fwd_kernel(FfnRowsArgs fa) {
    constexpr int BM = 32, BN = 128, AS = 128 + KPAD, LDC = BN + 4;
    constexpr unsigned F_HEAD = SPEC ? (EF_SHIFT | EF_F32 | EF_DROP | EF_RES | EF_LNF | EF_GEMM2 | EF_G2FFN1) : EF_ANY;
    constexpr unsigned F_TAIL = !SPEC ? EF_ANY : (EF_SHIFT | EF_F32 | EF_DROP | EF_RES | (TAIL == 2 ? EF_POOLOUT : EF_LNF) | (TAIL == 1 ? EF_GEMM2 : 0));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ConvArgs& a = fa.c;
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int t0 = blockIdx.x * BM;
    bf16* As = reinterpret_cast<bf16*>(smem);
    bf16* Ws = As + BM * AS;
    {   // 32 x 128 rows and the 128 x 128 weight image: one round trip (T % 32 == 0, host-checked)
        uint4 va[2], vw[8];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int s = i * 256 + tid;
            va[i] = *reinterpret_cast<const uint4*>(a.x + (size_t)(t0 + s / 16) * 128 + (s % 16) * 8);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int s = i * 256 + tid;
            vw[i] = *reinterpret_cast<const uint4*>(a.w + (size_t)(s / 16) * 128 + (s % 16) * 8);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int s = i * 256 + tid;
            *reinterpret_cast<uint4*>(As + (s / 16) * AS + (s % 16) * 8) = va[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int s = i * 256 + tid;
            *reinterpret_cast<uint4*>(Ws + (s / 16) * AS + (s % 16) * 8) = vw[i];
        }
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 128; ks += 16) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(As + lr * AS + ks + lh * 8);
        const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(Ws + (wn * 32 + lr) * AS + ks + lh * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc, 0, 0, 0);
    }
    __syncthreads();                               // staging LDS is dead: reuse as the C tile
    float* Cs = reinterpret_cast<float*>(smem);
    float* sstat = Cs + BM * LDC;
    bf16* a2 = reinterpret_cast<bf16*>(smem + CT32);   // the second GEMMs' operand rows (norm2's, then the next norm1's)
    bf16* Gs = a2 + 32 * A2S;                          // [32][n1 + KPAD] hidden tile
    auto park = [&]() {
#pragma unroll
        for (int r = 0; r < 16; ++r) Cs[((r & 3) + 8 * (r >> 2) + 4 * lh) * LDC + wn * 32 + lr] = acc[r];
    };
    park();
    __syncthreads();
    epilogue_rows<BM, BN, F_HEAD>(Cs, a.e, tid, 0, t0, a.T, 0, 128, sstat, a2);
    __syncthreads();                               // the C tile is dead: it stages the pre-activation copy
    second_gemm<F_HEAD, true>(a2, a.e, (size_t)t0, tid, wn, lr, lh, Gs, reinterpret_cast<bf16*>(smem));
    __syncthreads();                               // the hidden tile is complete; every staged copy has left
    {
        const int n1 = a.e.n2, GS = n1 + KPAD;
        const bf16* wlane = fa.w3 + (size_t)(32 * wn + lr) * n1 + lh * 8;
        bf16x8 bnx[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wlane + ks * 16);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int c0 = 0; c0 < n1; c0 += 128) {
            bf16x8 bfr[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) bfr[ks] = bnx[ks];
            if (c0 + 128 < n1)
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wlane + c0 + 128 + ks * 16);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(Gs + lr * GS + c0 + ks * 16 + lh * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[ks], acc, 0, 0, 0);
            }
        }
    }
    park();
    __syncthreads();
    epilogue_rows<BM, BN, F_TAIL>(Cs, fa.t, tid, 0, t0, a.T, 0, 128, sstat, TAIL == 1 ? a2 : nullptr);
    if constexpr (TAIL == 1) {
        __syncthreads();
        second_gemm<SPEC ? EF_GEMM2 : EF_ANY, false>(a2, fa.t, (size_t)t0, tid, wn, lr, lh, reinterpret_cast<bf16*>(smem), nullptr);
    }
}

// a finished 128-column group of ffn_rows_bwd_kernel's dz tile leaves as 16-byte stores, 16 lanes to a 256-byte row segment
__device__ __forceinline__ void store_dz_group(bf16* dz, const bf16* Gs, int GS, int t0, int n1, int j, int srow, int scol) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int row = q * 16 + srow;
        *reinterpret_cast<uint4*>(dz + (size_t)(t0 + row) * n1 + 128 * j + scol) = *reinterpret_cast<const uint4*>(Gs + row * GS + 128 * j + scol);
    }
}

// The backward of those rows, one launch: the second FFN Linear's data gradient (dy2 x W2d, * act'(z) * the hidden
// dropout's mask -> dz) with the whole 32 x n1 tile KEPT in LDS (and stored: linear1's weight gradient reads it), the first
// FFN Linear's data gradient on that tile (W1d's fragments from its L2-resident image one 128-chunk ahead, k ascending in
// 16-steps into one accumulator: the bits of the stand-alone launch's 128-chunks), then norm2's backward and the
// out-projection's data gradient exactly as conv1d_fwd_kernel<32, 128, 1, 4, 128, ..., 1> runs them behind that GEMM.
// g = the FFN-2 data gradient's epilogue arguments (gradz, its activation, dropout, out_bf16 = dz), e = the second launch's.
struct FfnRowsBwdArgs { const bf16* dy2; const bf16* w2d; const bf16* w1d; int M, n1; EpiArgs g; EpiArgs e; };
// SPEC: the training step's epilogue combination compiled in (GELU', both dropouts, skip gradient, fp32 rows)
template <bool SPEC>
__global__ __launch_bounds__(256, 2) void ffn_rows_bwd_kernel(FfnRowsBwdArgs fa) {
#pragma clang fp contract(off)
    constexpr int BM = 32, BN = 128, LDC = BN + 4;
    constexpr unsigned F_LN = SPEC ? (EF_LNBWD | EF_RES | EF_F32 | EF_BF16 | EF_DROP | EF_GEMM2) : EF_ANY;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int t0 = blockIdx.x * BM;
    const int n1 = fa.n1, GS = n1 + KPAD, ng = n1 / 128;
    float* Cs = reinterpret_cast<float*>(smem);
    float* sstat = Cs + BM * LDC;
    bf16* zs = reinterpret_cast<bf16*>(smem);          // two 32 x A2S staging tiles of z (the C tile is not live yet)
    bf16* a2 = reinterpret_cast<bf16*>(smem + CT32);   // dy2's rows, later norm2's masked d(input) rows
    bf16* Gs = a2 + 32 * A2S;                          // [32][n1 + KPAD] dz tile
    const EpiArgs& g = fa.g;
    const int act = SPEC ? (int)MM_ACT_GELU : g.gradz_act;
    const bool drop = SPEC ? true : g.drop_thresh != 0;
    const uint32_t dseed = drop ? mm_eff_seed(g.drop_seed, g.drop_epoch) : 0u;
    // 16-byte row segments: thread -> rows srow and srow + 16, columns scol .. scol + 7 of a 128-column group
    const int srow = tid >> 4, scol = (tid & 15) * 8;
    bf16x8 zreg[2];
    {
        uint4 va[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            va[q] = *reinterpret_cast<const uint4*>(fa.dy2 + (size_t)(t0 + q * 16 + srow) * 128 + scol);
            zreg[q] = *reinterpret_cast<const bf16x8*>(g.gradz + (size_t)(t0 + q * 16 + srow) * n1 + scol);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<uint4*>(a2 + (q * 16 + srow) * A2S + scol) = va[q];
    }
    bf16x8 bnx[8];
    {
        const bf16* wlane = fa.w2d + (size_t)(32 * wn + lr) * 128 + lh * 8;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wlane + ks * 16);
    }
    __syncthreads();
    {
        bf16x8 af[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) af[ks] = *reinterpret_cast<const bf16x8*>(a2 + lr * A2S + ks * 16 + lh * 8);
        const bf16* wlane = fa.w2d + (size_t)(32 * wn + lr) * 128 + lh * 8;
        for (int j = 0; j < ng; ++j) {
            bf16x8 bfr[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) bfr[ks] = bnx[ks];
            bf16* zt = zs + (j & 1) * (32 * A2S);      // last read two groups ago: a barrier lies between
#pragma unroll
            for (int q = 0; q < 2; ++q) *reinterpret_cast<bf16x8*>(zt + (q * 16 + srow) * A2S + scol) = zreg[q];
            if (j + 1 < ng) {                          // the next group's weight fragments and z rows fly during this group's MFMAs
                const bf16* wrow = wlane + (size_t)(j + 1) * 128 * 128;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wrow + ks * 16);
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    zreg[q] = *reinterpret_cast<const bf16x8*>(g.gradz + (size_t)(t0 + q * 16 + srow) * n1 + 128 * (j + 1) + scol);
            }
            f32x16 c2;
#pragma unroll
            for (int r = 0; r < 16; ++r) c2[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], bfr[ks], c2, 0, 0, 0);
            __syncthreads();                           // z's tile is staged; the previous group's columns of the dz tile are complete
            if (j > 0) store_dz_group(g.out_bf16, Gs, GS, t0, n1, j - 1, srow, scol);
            // scale 1, shift 0 -> act'(z) -> dropout, the arithmetic of epilogue_rows (FFN-2 data gradient)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int col = 128 * j + 32 * wn + lr;
                const size_t idx = (size_t)(t0 + row) * n1 + col;
                float v = __builtin_fmaf(c2[r], 1.f, 0.f);
                v *= act_grad((float)zt[row * A2S + 32 * wn + lr], act);
                if (drop) v = __builtin_fmaf(v, dropout_scale(dseed, (uint32_t)idx, g.drop_thresh, g.drop_inv_keep), 0.f);
                else v += 0.f;
                Gs[row * GS + col] = (bf16)fmaxf(-INFINITY, v);
            }
        }
    }
    __syncthreads();                                   // the dz tile is complete; z's staging tiles are dead
    store_dz_group(g.out_bf16, Gs, GS, t0, n1, ng - 1, srow, scol);
    f32x16 acc;
    {
        const bf16* wlane = fa.w1d + (size_t)(32 * wn + lr) * n1 + lh * 8;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wlane + ks * 16);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int c0 = 0; c0 < n1; c0 += 128) {
            bf16x8 bfr[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) bfr[ks] = bnx[ks];
            if (c0 + 128 < n1)
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) bnx[ks] = *reinterpret_cast<const bf16x8*>(wlane + c0 + 128 + ks * 16);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const bf16x8 af = *reinterpret_cast<const bf16x8*>(Gs + lr * GS + c0 + ks * 16 + lh * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr[ks], acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) Cs[((r & 3) + 8 * (r >> 2) + 4 * lh) * LDC + wn * 32 + lr] = acc[r];
    __syncthreads();
    epilogue_ln_bwd<BM, BN, F_LN>(Cs, fa.e, tid, 0, t0, fa.M, sstat, a2);
    __syncthreads();                                   // the C tile is dead: it stages the outputs
    second_gemm<F_LN, false>(a2, fa.e, (size_t)t0, tid, wn, lr, lh, reinterpret_cast<bf16*>(smem), a2 + 32 * A2S);
}

}  // namespace

extern "C" {
// mm_linear_fwd_ln_gemm2_act followed, inside the launch, by the second FFN Linear on the hidden rows and that Linear's
// own consumers: y = dropout(g W2^T + b2) + x1, then LayerNorm rows (+ stats) of y, optionally their projection wq (the next
// block's in_proj), or - pool_out != NULL - the mean over groups of rows_per_group rows.  The 32 x n1 hidden tile never
// leaves the workgroup: g_out / z_out (both nullable) are written only for a backward pass.  See include/mmeeg_hip.h.
int mm_ffn_rows_fwd(const void* x, const void* w, int M, int K, const float* bias, const float* residual, float* x1_f32,
                    float drop_p, uint32_t seed, const uint32_t* seed_epoch, const float* ln_gamma, const float* ln_beta,
                    float ln_eps, void* ln_out_bf16, float* ln_stat, const void* w1, const float* bias1, int n1,
                    void* g_bf16, void* z_bf16, int act1, float drop1_p, uint32_t seed1, const void* w2, const float* bias2,
                    float* y_f32, float drop2_p, uint32_t seed2, const float* nln_gamma, const float* nln_beta, float nln_eps,
                    void* nln_out_bf16, float* nln_stat, const void* wq, const float* biasq, int nq, void* q_bf16,
                    float* pool_out, int rows_per_group, hipStream_t st) {
    MM_REQUIRE(ln_out_bf16 && w1 && w2 && y_f32 && x1_f32, "ffn_rows_fwd: null");
    MM_REQUIRE(K == 128, "ffn_rows_fwd: the out-projection is 128 -> 128 (K=%d)", K);
    MM_REQUIRE(n1 > 0 && n1 % 128 == 0, "ffn_rows_fwd: n1=%d must be a multiple of 128", n1);
    MM_REQUIRE((pool_out != nullptr) != (nln_out_bf16 != nullptr), "ffn_rows_fwd: one consumer - LayerNorm rows or pool_out");
    MM_REQUIRE(!wq || (nln_out_bf16 && q_bf16), "ffn_rows_fwd: the projection needs the LayerNorm rows and an output");
    FfnRowsArgs fa;
    int rc = linear128_fwd_args(fa.c, x, w, M, K, bias, residual, x1_f32, drop_p, seed, seed_epoch, nullptr, 0, ln_gamma, ln_beta,
                                ln_eps, ln_out_bf16, ln_stat, {w1, bias1, n1, g_bf16, act1, drop1_p, seed1, z_bf16, /*keep*/ true});
    if (rc) return rc;
    ConvArgs t;
    // (x: never read, the operand is the LDS tile; g_bf16 may be null and the builder wants an operand)
    rc = linear128_fwd_args(t, g_bf16 ? g_bf16 : w2, w2, M, n1, bias2, x1_f32, y_f32, drop2_p, seed2, seed_epoch, pool_out,
                            rows_per_group, nln_gamma, nln_beta, nln_eps, nln_out_bf16, nln_stat, {wq, biasq, nq, q_bf16});
    if (rc) return rc;
    fa.t = t.e; fa.w3 = (const bf16*)w2;
    const size_t stage = (size_t)(32 + 128) * (128 + KPAD) * sizeof(bf16);
    size_t need = CT32 + A2B + (size_t)32 * (n1 + KPAD) * sizeof(bf16);
    if (need < stage) need = stage;
    MM_REQUIRE(need <= 64 * 1024, "ffn_rows_fwd: n1=%d needs %zu B of LDS (two workgroups per CU: 64 KiB each)", n1, need);
    const EpiArgs& h = fa.c.e;
    const bool spec = !getenv("MM_EPI_GENERIC") && h.shift && h.residual && h.drop_thresh && h.act2 == MM_ACT_GELU && h.pre2 &&
                      h.thresh2 && fa.t.shift && fa.t.drop_thresh;
    const int tail = pool_out ? 2 : (wq ? 1 : 0);
    const dim3 grid(M / 32);
#define FFN_CASE(S, T_) if (spec == S && tail == T_) hipLaunchKernelGGL((ffn_rows_fwd_kernel<S, T_>), grid, dim3(256), need, st, fa);
    FFN_CASE(true, 0) FFN_CASE(true, 1) FFN_CASE(true, 2) FFN_CASE(false, 0) FFN_CASE(false, 1) FFN_CASE(false, 2)
#undef FFN_CASE
    return mm_check_launch("ffn_rows_fwd");
}

// The FFN-2 data gradient (-> dz) followed, inside the launch, by mm_linear_dgrad_ln_bwd_gemm2 on the dz rows, which never
// leave the workgroup between the two GEMMs (dz_bf16 is still written: linear1's weight gradient reads it).  See
// include/mmeeg_hip.h.
int mm_ffn_rows_bwd(const void* dy2, const void* w2d, int M, int n1, const void* z_bf16, int act1, float drop1_p, uint32_t seed1,
                    void* dz_bf16, const void* w1d, const float* x1, const float* stat2, const float* gamma2, const float* dres,
                    int dres_rows_per_sample, float* dx1, void* dyo_bf16, float* dgb_repl, float drop_p, uint32_t seed,
                    const uint32_t* seed_epoch, const void* wo_d, void* do_bf16, hipStream_t st) {
    MM_REQUIRE(dy2 && w2d && z_bf16 && dz_bf16 && w1d && x1 && stat2 && gamma2 && dx1 && dyo_bf16 && wo_d && do_bf16, "ffn_rows_bwd: null");
    MM_REQUIRE(M > 0 && M % 32 == 0, "ffn_rows_bwd: M=%d must be a multiple of 32", M);
    MM_REQUIRE(n1 > 0 && n1 % 128 == 0 && n1 <= 512, "ffn_rows_bwd: n1=%d must be a multiple of 128 up to 512", n1);
    MM_REQUIRE(act1 >= MM_ACT_NONE && act1 <= MM_ACT_SIGMOID, "ffn_rows_bwd: act1=%d", act1);
    MM_REQUIRE(drop1_p >= 0.f && drop1_p < 1.f && drop_p >= 0.f && drop_p < 1.f, "ffn_rows_bwd: drop_p");
    MM_REQUIRE((size_t)M * n1 < (1ull << 32), "ffn_rows_bwd: 32-bit dropout indices");
    MM_REQUIRE(dres_rows_per_sample >= 0 && (!dres_rows_per_sample || (dres && M % dres_rows_per_sample == 0)),
               "ffn_rows_bwd: dres_rows_per_sample=%d must divide M=%d", dres_rows_per_sample, M);
    ConvArgs c;
    int rc = conv1d_fwd_args(c, dy2, w2d, 1, M, 128, n1, 1, 0, nullptr, nullptr, 0, nullptr, nullptr, 1, nullptr, nullptr, dz_bf16,
                             nullptr, drop1_p, seed1, seed_epoch, z_bf16, act1);
    if (rc) return rc;
    ConvArgs l;
    rc = linear_dgrad_ln_bwd_args(l, dz_bf16, w1d, M, n1, x1, stat2, gamma2, dres, dx1, dyo_bf16, dgb_repl, drop_p, seed, seed_epoch,
                                  nullptr, wo_d, do_bf16, dres_rows_per_sample);
    if (rc) return rc;
    FfnRowsBwdArgs fa;
    fa.dy2 = (const bf16*)dy2; fa.w2d = (const bf16*)w2d; fa.w1d = (const bf16*)w1d; fa.M = M; fa.n1 = n1;
    fa.g = c.e; fa.e = l.e;
    const size_t need = CT32 + A2B + (size_t)32 * (n1 + KPAD) * sizeof(bf16);
    MM_REQUIRE(need <= 64 * 1024, "ffn_rows_bwd: n1=%d needs %zu B of LDS (two workgroups per CU: 64 KiB each)", n1, need);
    // the combination both replaced launches compile in: GELU' and the hidden dropout; skip gradient, fp32 rows, out_proj's dropout
    const bool spec = !getenv("MM_EPI_GENERIC") && act1 == MM_ACT_GELU && fa.g.drop_thresh && dres && fa.e.drop_thresh;
    const dim3 grid(M / 32);
    if (spec) hipLaunchKernelGGL((ffn_rows_bwd_kernel<true>), grid, dim3(256), need, st, fa);
    else hipLaunchKernelGGL((ffn_rows_bwd_kernel<false>), grid, dim3(256), need, st, fa);
    return mm_check_launch("ffn_rows_bwd");
}
}  // extern "C"
