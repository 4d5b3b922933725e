// Lag attention pooling over the frame features of an fMRI sequence: one learned query scores the
// F frames of a sample, a softmax over the frames weighs them, the weighted sum is the sample's feature.
//   s[b][f] = (x[b][f] . q) / sqrt(N) + c[f],  a[b] = softmax_f(s[b]),  out[b] = sum_f a[b][f] x[b][f]
// 16 K floats at the trainer's shapes: latency, not bandwidth.  ONE WAVE PER SAMPLE (a workgroup of 64 lanes): lane l holds
// the float4 chunks l, l + 64, ... of a feature row (N <= 1024 = 4 chunks per lane) and, once the dot products are
// reduced, the score of frame l (F <= 64).  Every reduction is the DPP / permlane butterfly of common.h: no LDS, no
// barrier, no atomics, a fixed order; a sample's wave reads and writes that sample alone, so a row's bits do not depend on
// the batch it is in.
#include "common.h"
#include "mmeeg_hip.h"

namespace {

constexpr int LP_MAX_F = 64, LP_MAX_N = 1024;

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// q is a parameter: a view into a trainer's flat bucket at any float offset, so it is read with 4-byte loads (N floats per
// wave, once); the activations are allocations of their own and travel as 16-byte chunks
__device__ __forceinline__ f32x4 load4(const float* p) { return f32x4{p[0], p[1], p[2], p[3]}; }

// NV = float4 chunks per lane = ceil(N / 256)
template <int NV>
__global__ __launch_bounds__(64) void lagpool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ q,
                                                         const float* __restrict__ c, float* __restrict__ out,
                                                         float* __restrict__ attw, int F, int N, float scale) {
    const int b = blockIdx.x, lane = threadIdx.x, n4 = N >> 2;
    const f32x4* xb = reinterpret_cast<const f32x4*>(x + (size_t)b * F * N);
    f32x4 qv[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int i = lane + 64 * j;
        qv[j] = i < n4 ? load4(q + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool live = lane < F;
    float u = 0.f;                                   // lane f: (x[b][f] . q) / sqrt(N)
    for (int f = 0; f < F; ++f) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            if (i < n4) p = dot4(xb[(size_t)f * n4 + i], qv[j], p);
        }
        p = wave_sum(p);
        if (lane == f) u = p * scale;
    }
    const float cf = live ? c[lane] : 0.f;
    // the pivot is the frame of the largest score; the exponent is formed from DIFFERENCES to it, (u - u_p) + (c - c_p):
    // a common offset of c (of any size) drops out exactly instead of eating the low bits of u + c
    const float s = live ? u + cf : -__builtin_inff();
    const float m = wave_max(s);
    const unsigned long long at_max = __ballot(live && s == m);
    const int piv = at_max ? __ffsll((long long)at_max) - 1 : 0;        // (no lane equals a NaN maximum: the row is NaN anyway)
    const float t = (u - __shfl(u, piv, 64)) + (cf - __shfl(cf, piv, 64));
    const float e = live ? expf(t) : 0.f;
    const float a = e / wave_sum(e);                 // F == 1: exp(0) / 1 = 1 exactly
    if (live) attw[(size_t)b * F + lane] = a;
    f32x4 acc[NV];
    for (int f = 0; f < F; ++f) {
        const float af = __shfl(a, f, 64);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            if (i < n4) {
                const f32x4 v = xb[(size_t)f * n4 + i];
                // the first frame is a product, not 0 + product: with a == 1 (F == 1) the row is x bit for bit
                acc[j] = f == 0 ? v * af : f32x4{fmaf(v.x, af, acc[j].x), fmaf(v.y, af, acc[j].y), fmaf(v.z, af, acc[j].z),
                                                  fmaf(v.w, af, acc[j].w)};
            }
        }
    }
    f32x4* ob = reinterpret_cast<f32x4*>(out + (size_t)b * N);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int i = lane + 64 * j;
        if (i < n4) ob[i] = acc[j];
    }
}

template <int NV>
__global__ __launch_bounds__(64) void lagpool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                                                         const float* __restrict__ attw, const float* __restrict__ q,
                                                         float* __restrict__ dx, float* __restrict__ dparts, int F, int N,
                                                         float scale) {
    const int b = blockIdx.x, lane = threadIdx.x, n4 = N >> 2;
    const f32x4* xb = reinterpret_cast<const f32x4*>(x + (size_t)b * F * N);
    f32x4* dxb = reinterpret_cast<f32x4*>(dx + (size_t)b * F * N);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(dout + (size_t)b * N);
    f32x4 qv[NV], g[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int i = lane + 64 * j;
        qv[j] = i < n4 ? load4(q + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
        g[j] = i < n4 ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool live = lane < F;
    float da = 0.f;                                  // lane f: dout[b] . x[b][f]
    for (int f = 0; f < F; ++f) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            if (i < n4) p = dot4(xb[(size_t)f * n4 + i], g[j], p);
        }
        p = wave_sum(p);
        if (lane == f) da = p;
    }
    const float a = live ? attw[(size_t)b * F + lane] : 0.f;
    // ds[f] = a[f] (da[f] - sum_g a[g] da[g]), evaluated as a[f] sum_g a[g] (da[f] - da[g]) in ascending g: the same number
    // (sum_g a[g] = 1) without the cancellation that zeroes the dominant frame's score gradient when the softmax is
    // nearly one-hot (its true value is minus the sum of the others').  F == 1: 1 * 1 * (da - da) = 0
    float dev = 0.f;
    for (int g2 = 0; g2 < F; ++g2) dev = fmaf(__shfl(a, g2, 64), da - __shfl(da, g2, 64), dev);
    const float ds = a * dev;
    float* part = dparts + (size_t)b * (N + F);      // (dq_b | dc_b); N + F need not be a multiple of 4: scalar stores
    if (live) part[N + lane] = ds;
    f32x4 dq[NV];
    for (int f = 0; f < F; ++f) {
        const float af = __shfl(a, f, 64), dsf = __shfl(ds, f, 64);
        const float k = dsf * scale;                 // wave-uniform
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int i = lane + 64 * j;
            if (i < n4) {
                const f32x4 v = xb[(size_t)f * n4 + i];
                f32x4 d = g[j] * af;
                // a zero score gradient adds nothing, not + 0.0f: with F == 1 the row is dout bit for bit
                if (k != 0.f) d = f32x4{fmaf(qv[j].x, k, d.x), fmaf(qv[j].y, k, d.y), fmaf(qv[j].z, k, d.z), fmaf(qv[j].w, k, d.w)};
                dxb[(size_t)f * n4 + i] = d;
                dq[j] = f == 0 ? v * dsf : f32x4{fmaf(v.x, dsf, dq[j].x), fmaf(v.y, dsf, dq[j].y), fmaf(v.z, dsf, dq[j].z),
                                                  fmaf(v.w, dsf, dq[j].w)};
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int i = lane + 64 * j;
        if (i < n4) {
            part[4 * i + 0] = dq[j].x * scale;
            part[4 * i + 1] = dq[j].y * scale;
            part[4 * i + 2] = dq[j].z * scale;
            part[4 * i + 3] = dq[j].w * scale;
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int lagpool_shape(const char* who, int B, int F, int N) {
    MM_REQUIRE(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    MM_REQUIRE(F >= 1 && F <= LP_MAX_F, "%s: F must be in 1..%d frames (got %d)", who, LP_MAX_F, F);
    MM_REQUIRE(N >= 4 && N <= LP_MAX_N && N % 4 == 0, "%s: N must be a multiple of 4 in 4..%d (got %d)", who, LP_MAX_N, N);
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_lagpool_fwd(const float* x, const float* q, const float* c, float* out, float* attw, int B, int F, int N,
                   hipStream_t st) {
    if (const int rc = lagpool_shape("lagpool_fwd", B, F, N)) return rc;
    MM_REQUIRE(x && q && c && out && attw, "lagpool_fwd: null pointer");
    MM_REQUIRE(aligned16(x) && aligned16(out), "lagpool_fwd: x and out must be 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)N);
    const dim3 grid(B), block(64);
    switch ((N + 255) / 256) {
        case 1: hipLaunchKernelGGL(lagpool_fwd_kernel<1>, grid, block, 0, st, x, q, c, out, attw, F, N, scale); break;
        case 2: hipLaunchKernelGGL(lagpool_fwd_kernel<2>, grid, block, 0, st, x, q, c, out, attw, F, N, scale); break;
        case 3: hipLaunchKernelGGL(lagpool_fwd_kernel<3>, grid, block, 0, st, x, q, c, out, attw, F, N, scale); break;
        default: hipLaunchKernelGGL(lagpool_fwd_kernel<4>, grid, block, 0, st, x, q, c, out, attw, F, N, scale); break;
    }
    return mm_check_launch("lagpool_fwd");
}

int mm_lagpool_bwd(const float* dout, const float* x, const float* attw, const float* q, float* dx, float* dparts, int B,
                   int F, int N, hipStream_t st) {
    if (const int rc = lagpool_shape("lagpool_bwd", B, F, N)) return rc;
    MM_REQUIRE(dout && x && attw && q && dx && dparts, "lagpool_bwd: null pointer");
    MM_REQUIRE(aligned16(dout) && aligned16(x) && aligned16(dx), "lagpool_bwd: dout, x and dx must be 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)N);
    const dim3 grid(B), block(64);
    switch ((N + 255) / 256) {
        case 1: hipLaunchKernelGGL(lagpool_bwd_kernel<1>, grid, block, 0, st, dout, x, attw, q, dx, dparts, F, N, scale); break;
        case 2: hipLaunchKernelGGL(lagpool_bwd_kernel<2>, grid, block, 0, st, dout, x, attw, q, dx, dparts, F, N, scale); break;
        case 3: hipLaunchKernelGGL(lagpool_bwd_kernel<3>, grid, block, 0, st, dout, x, attw, q, dx, dparts, F, N, scale); break;
        default: hipLaunchKernelGGL(lagpool_bwd_kernel<4>, grid, block, 0, st, dout, x, attw, q, dx, dparts, F, N, scale); break;
    }
    return mm_check_launch("lagpool_bwd");
}

}  // extern "C"
