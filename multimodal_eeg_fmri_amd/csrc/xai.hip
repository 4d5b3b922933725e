// Attribution (explainability) kernels: the interpolation path of integrated gradients as one batch, the
// per-input gradient accumulator, the attribution / per-channel reduction, and the matched-pair score with its
// gradient seed.  All four are bandwidth-bound: 16-byte accesses per lane where the row length allows it, one
// writer per output element, every sum formed in a fixed order (the same inputs give the same bits).
#include "common.h"
#include "mmeeg_hip.h"

// HIP compiles device code with -ffp-contract=fast, __fmul_rn / __fadd_rn are plain operators there, and the backend
// fuses whatever a source pragma leaves apart: build.sh compiles THIS file with -ffp-contract=off.  Without it the
// interpolation becomes v_fma_f32 and is no longer torch's bits (tests/test_xai_kernels_gpu.py compares them).

namespace {

constexpr int XAI_THREADS = 256;
constexpr int XAI_MAX_GRID = 256 * 8;         // grid-stride loops: 256 CUs x 8 workgroups of 4 waves = 8 waves per SIMD in flight

// alpha_s of np.linspace(0, 1, n_steps) rounded to fp32: arange(n) * (1 / (n - 1)) in fp64, the last point exactly 1
__device__ __forceinline__ float xai_alpha(int s, int n_steps) {
    if (n_steps <= 1) return 0.f;
    if (s == n_steps - 1) return 1.f;
    return (float)((double)s * (1.0 / (double)(n_steps - 1)));
}

// base + alpha * (x - base), each operation rounded on its own (no contraction into an FMA): torch's bits
__device__ __forceinline__ float xai_lerp(float x, float b, float alpha) {
    return __fadd_rn(b, __fmul_rn(alpha, __fsub_rn(x, b)));
}

// out[s - s0][r][i] for s in [s0, s0 + gridDim.y); base_rows: 0 (no baseline = zeros), 1 (one row for every sample), rows
template <bool VEC>
__global__ __launch_bounds__(XAI_THREADS) void xai_interp_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                                 float* __restrict__ out, int n_steps, int s0, size_t rows,
                                                                 size_t inner, int base_rows) {
    const float alpha = xai_alpha(s0 + (int)blockIdx.y, n_steps);
    const size_t n = rows * inner;
    float* o = out + (size_t)blockIdx.y * n;
    const size_t stride = (size_t)gridDim.x * XAI_THREADS;
    if (VEC) {
        const size_t nv = n / 4, iv = inner / 4;
        for (size_t v = (size_t)blockIdx.x * XAI_THREADS + threadIdx.x; v < nv; v += stride) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(x)[v];
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (base_rows) bv = reinterpret_cast<const f32x4*>(base)[base_rows == 1 ? v % iv : v];
            f32x4 r;
            r[0] = xai_lerp(xv[0], bv[0], alpha); r[1] = xai_lerp(xv[1], bv[1], alpha);
            r[2] = xai_lerp(xv[2], bv[2], alpha); r[3] = xai_lerp(xv[3], bv[3], alpha);
            reinterpret_cast<f32x4*>(o)[v] = r;
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * XAI_THREADS + threadIdx.x; i < n; i += stride) {
            const float b = base_rows ? base[base_rows == 1 ? i % inner : i] : 0.f;
            o[i] = xai_lerp(x[i], b, alpha);
        }
    }
}

// acc[i] = (((acc[i] + g[0][i]) + g[1][i]) + ...): ascending step order, so the result does not depend on how the
// steps were cut into chunks
template <bool VEC>
__global__ __launch_bounds__(XAI_THREADS) void xai_accum_kernel(const float* __restrict__ grad, float* __restrict__ acc, int steps, size_t n) {
    const size_t stride = (size_t)gridDim.x * XAI_THREADS;
    if (VEC) {
        const size_t nv = n / 4;
        for (size_t v = (size_t)blockIdx.x * XAI_THREADS + threadIdx.x; v < nv; v += stride) {
            f32x4 a = reinterpret_cast<f32x4*>(acc)[v];
            for (int s = 0; s < steps; ++s) {
                const f32x4 g = reinterpret_cast<const f32x4*>(grad + (size_t)s * n)[v];
                a[0] = __fadd_rn(a[0], g[0]); a[1] = __fadd_rn(a[1], g[1]); a[2] = __fadd_rn(a[2], g[2]); a[3] = __fadd_rn(a[3], g[3]);
            }
            reinterpret_cast<f32x4*>(acc)[v] = a;
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * XAI_THREADS + threadIdx.x; i < n; i += stride) {
            float a = acc[i];
            for (int s = 0; s < steps; ++s) a = __fadd_rn(a, grad[(size_t)s * n + i]);
            acc[i] = a;
        }
    }
}

// mode 0: |(x - base) * (acc / n_steps)|   (integrated gradients; acc = the sum over the steps)
// mode 1: |acc|                            (gradient saliency; acc = the gradient)
// mode 2: |acc| * |x|                      (gradient x input)
__device__ __forceinline__ float xai_attr(float x, float b, float a, int n_steps, int mode) {
    if (mode == 1) return fabsf(a);
    if (mode == 2) return __fmul_rn(fabsf(a), fabsf(x));
    return fabsf(__fmul_rn(__fsub_rn(x, b), __fdiv_rn(a, (float)n_steps)));
}
__device__ __forceinline__ f32x4 xai_attr4(f32x4 x, f32x4 b, f32x4 a, int n_steps, int mode) {
    f32x4 r;
    r[0] = xai_attr(x[0], b[0], a[0], n_steps, mode); r[1] = xai_attr(x[1], b[1], a[1], n_steps, mode);
    r[2] = xai_attr(x[2], b[2], a[2], n_steps, mode); r[3] = xai_attr(x[3], b[3], a[3], n_steps, mode);
    return r;
}

template <bool VEC>
__global__ __launch_bounds__(XAI_THREADS) void xai_finish_flat_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                                      const float* __restrict__ acc, float* __restrict__ attr,
                                                                      size_t n, size_t inner, int base_rows, int n_steps, int mode) {
    const size_t stride = (size_t)gridDim.x * XAI_THREADS;
    if (VEC) {
        const size_t nv = n / 4, iv = inner / 4;
        for (size_t v = (size_t)blockIdx.x * XAI_THREADS + threadIdx.x; v < nv; v += stride) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (base_rows) bv = reinterpret_cast<const f32x4*>(base)[base_rows == 1 ? v % iv : v];
            reinterpret_cast<f32x4*>(attr)[v] = xai_attr4(reinterpret_cast<const f32x4*>(x)[v], bv, reinterpret_cast<const f32x4*>(acc)[v], n_steps, mode);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * XAI_THREADS + threadIdx.x; i < n; i += stride) {
            const float b = base_rows ? base[base_rows == 1 ? i % inner : i] : 0.f;
            attr[i] = xai_attr(x[i], b, acc[i], n_steps, mode);
        }
    }
}

// one workgroup per (sample, channel) row of T values: attr row + chan[row] = mean_t attr.  Every thread adds its
// elements in ascending t, the wave sum is the xor butterfly, the four wave totals are added in wave order.
template <bool VEC>
__global__ __launch_bounds__(XAI_THREADS) void xai_finish_rows_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                                      const float* __restrict__ acc, float* __restrict__ attr,
                                                                      float* __restrict__ chan, int C, size_t T, int base_rows,
                                                                      int n_steps, int mode) {
    __shared__ float part[XAI_THREADS / 64];
    const size_t row = blockIdx.x;
    const size_t off = row * T;
    const size_t boff = base_rows == 1 ? (row % (size_t)C) * T : off;
    float sum = 0.f;
    if (VEC) {
        for (size_t t = 4 * (size_t)threadIdx.x; t < T; t += 4 * XAI_THREADS) {
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (base_rows) bv = *reinterpret_cast<const f32x4*>(base + boff + t);
            const f32x4 v = xai_attr4(*reinterpret_cast<const f32x4*>(x + off + t), bv, *reinterpret_cast<const f32x4*>(acc + off + t), n_steps, mode);
            *reinterpret_cast<f32x4*>(attr + off + t) = v;
            sum = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(sum, v[0]), v[1]), v[2]), v[3]);
        }
    } else {
        for (size_t t = threadIdx.x; t < T; t += XAI_THREADS) {
            const float b = base_rows ? base[boff + t] : 0.f;
            const float v = xai_attr(x[off + t], b, acc[off + t], n_steps, mode);
            attr[off + t] = v;
            sum = __fadd_rn(sum, v);
        }
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = part[0];
        for (int w = 1; w < XAI_THREADS / 64; ++w) s = __fadd_rn(s, part[w]);
        chan[row] = __fdiv_rn(s, (float)T);
    }
}

// z (B, 2N) = [ze | zf]: score[b] = ze_b . zf_b (one wave per row, fixed order) and seed (B, 2N) = [zf | ze], the
// gradient of the score with respect to z
__global__ __launch_bounds__(64) void xai_pair_score_kernel(const float* __restrict__ z, float* __restrict__ score,
                                                            float* __restrict__ seed, int N) {
    const float* zr = z + (size_t)blockIdx.x * 2 * N;
    float* sr = seed ? seed + (size_t)blockIdx.x * 2 * N : nullptr;
    float sum = 0.f;
    for (int j = threadIdx.x; j < N; j += 64) {
        const float e = zr[j], f = zr[N + j];
        sum = __fadd_rn(sum, __fmul_rn(e, f));
        if (sr) { sr[j] = f; sr[N + j] = e; }
    }
    sum = wave_sum(sum);
    if (threadIdx.x == 0) score[blockIdx.x] = sum;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int flat_grid(size_t work) {
    size_t g = (work + XAI_THREADS - 1) / XAI_THREADS;
    return (int)(g < 1 ? 1 : (g > (size_t)XAI_MAX_GRID ? (size_t)XAI_MAX_GRID : g));
}

}  // namespace

extern "C" {

int mm_xai_interp(const float* x, const float* base, int base_rows, float* out, int n_steps, int s0, int steps,
                  int64_t rows, int64_t inner, hipStream_t st) {
    MM_REQUIRE(x && out, "xai_interp: null x / out");
    MM_REQUIRE(rows > 0 && inner > 0 && rows <= (1ll << 40) / inner, "xai_interp: rows=%lld inner=%lld", (long long)rows, (long long)inner);
    MM_REQUIRE(n_steps >= 1 && s0 >= 0 && steps >= 1 && steps <= 65535 && s0 + (int64_t)steps <= n_steps,
               "xai_interp: steps [%d, %d + %d) of %d", s0, s0, steps, n_steps);
    MM_REQUIRE((base == nullptr) == (base_rows == 0) && (base_rows == 0 || base_rows == 1 || base_rows == rows),
               "xai_interp: base_rows=%d (0 with a null baseline, 1 = one row for all, or rows=%lld)", base_rows, (long long)rows);
    const size_t n = (size_t)rows * (size_t)inner;
    const bool vec = inner % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(base);
    const dim3 grid(flat_grid(vec ? n / 4 : n), steps);
    if (vec)
        hipLaunchKernelGGL(xai_interp_kernel<true>, grid, dim3(XAI_THREADS), 0, st, x, base, out, n_steps, s0, (size_t)rows, (size_t)inner, base_rows);
    else
        hipLaunchKernelGGL(xai_interp_kernel<false>, grid, dim3(XAI_THREADS), 0, st, x, base, out, n_steps, s0, (size_t)rows, (size_t)inner, base_rows);
    return mm_check_launch("xai_interp");
}

int mm_xai_accum(const float* grad, float* acc, int steps, int64_t n, hipStream_t st) {
    MM_REQUIRE(grad && acc, "xai_accum: null grad / acc");
    MM_REQUIRE(steps >= 1 && n > 0 && n <= (1ll << 40) / steps, "xai_accum: steps=%d n=%lld", steps, (long long)n);
    const bool vec = n % 4 == 0 && aligned16(grad) && aligned16(acc);
    if (vec)
        hipLaunchKernelGGL(xai_accum_kernel<true>, dim3(flat_grid((size_t)n / 4)), dim3(XAI_THREADS), 0, st, grad, acc, steps, (size_t)n);
    else
        hipLaunchKernelGGL(xai_accum_kernel<false>, dim3(flat_grid((size_t)n)), dim3(XAI_THREADS), 0, st, grad, acc, steps, (size_t)n);
    return mm_check_launch("xai_accum");
}

int mm_xai_finish(const float* x, const float* base, int base_rows, const float* acc, float* attr, float* chan,
                  int B, int C, int64_t T, int n_steps, int mode, hipStream_t st) {
    MM_REQUIRE(x && acc && attr, "xai_finish: null x / acc / attr");
    MM_REQUIRE(B > 0 && C > 0 && T > 0 && (int64_t)B * C <= (1ll << 31) - 1 && (int64_t)B * C <= (1ll << 40) / T,
               "xai_finish: B=%d C=%d T=%lld", B, C, (long long)T);
    MM_REQUIRE(mode >= 0 && mode <= 2, "xai_finish: mode=%d (0 integrated gradients, 1 |grad|, 2 |grad| * |x|)", mode);
    MM_REQUIRE(n_steps >= 1, "xai_finish: n_steps=%d", n_steps);
    MM_REQUIRE((base == nullptr) == (base_rows == 0) && (base_rows == 0 || base_rows == 1 || base_rows == B),
               "xai_finish: base_rows=%d (0 with a null baseline, 1 = one sample for all, or B=%d)", base_rows, B);
    const size_t inner = (size_t)C * (size_t)T, n = (size_t)B * inner;
    const bool vec = T % 4 == 0 && aligned16(x) && aligned16(base) && aligned16(acc) && aligned16(attr);
    const dim3 rows((unsigned)((size_t)B * C)), thr(XAI_THREADS);
    if (chan && vec)
        hipLaunchKernelGGL(xai_finish_rows_kernel<true>, rows, thr, 0, st, x, base, acc, attr, chan, C, (size_t)T, base_rows, n_steps, mode);
    else if (chan)
        hipLaunchKernelGGL(xai_finish_rows_kernel<false>, rows, thr, 0, st, x, base, acc, attr, chan, C, (size_t)T, base_rows, n_steps, mode);
    else if (vec)
        hipLaunchKernelGGL(xai_finish_flat_kernel<true>, dim3(flat_grid(n / 4)), thr, 0, st, x, base, acc, attr, n, inner, base_rows, n_steps, mode);
    else
        hipLaunchKernelGGL(xai_finish_flat_kernel<false>, dim3(flat_grid(n)), thr, 0, st, x, base, acc, attr, n, inner, base_rows, n_steps, mode);
    return mm_check_launch("xai_finish");
}

int mm_xai_pair_score(const float* z, float* score, float* seed, int B, int N, hipStream_t st) {
    MM_REQUIRE(z && score, "xai_pair_score: null z / score");
    MM_REQUIRE(B > 0 && N > 0 && N <= (1 << 20), "xai_pair_score: B=%d N=%d", B, N);
    hipLaunchKernelGGL(xai_pair_score_kernel, dim3(B), dim3(64), 0, st, z, score, seed, N);
    return mm_check_launch("xai_pair_score");
}

}  // extern "C"
