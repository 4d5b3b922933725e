// The power encoder's front end: multi-scale STFT power spectra (direct DFT and radix-2 FFT in LDS) and their backward,
// the per-sample z-score (one workgroup per sample, or chunked with fp64 partials) and its backward, and the builder of
// the merged k = 3 | 5 | 7 convolution weight.  Callers: ops.stft_power_features and ops.power_merge* (forward),
// autograd.py (mm_stft_power_bwd, mm_sample_zscore_bwd).
#include "common.h"

namespace {
// ---------------------------------------------------------------------------
// multi-scale STFT power front-end (extension a-X3; torch.stft(center=True, reflect,
// periodic Hann) semantics): x (B, C, T) fp32 -> power written CHANNELS-LAST as bf16
// out[b][frame][ch_off + c*F + f] = |sum_n w[n] x[b,c,frame*hop + n - nfft/2] e^{-2 pi i f n / nfft}|^2
// so the result is directly the (B, L, Cin) activation of the Power encoder's first
// conv.  One workgroup per (b, c, frame-block); twiddles and the windowed frame in LDS.
// ---------------------------------------------------------------------------
__global__ void stft_power_kernel(const float* __restrict__ x, bf16* __restrict__ out, float* __restrict__ out_f32,
                                  int C, int T, int nfft, int hop, int frames, int ch_off, int ch_total) {
    extern __shared__ float sm[];
    float* tw_c = sm;                  // [nfft]
    float* tw_s = tw_c + nfft;         // [nfft]
    float* win = tw_s + nfft;          // [nfft] periodic Hann window
    float* fr = win + nfft;            // [8][nfft] windowed frames
    const int b = blockIdx.z, c = blockIdx.y;
    const int F = nfft / 2 + 1;
    for (int n = threadIdx.x; n < nfft; n += blockDim.x) {
        float s, co;
        __sincosf(6.283185307179586f * (float)n / (float)nfft, &s, &co);
        tw_c[n] = co; tw_s[n] = s;
        win[n] = 0.5f - 0.5f * __cosf(6.283185307179586f * (float)n / (float)nfft);
    }
    const float* xr = x + ((size_t)b * C + c) * T;
    // the workgroup walks its share of the frame blocks (gridDim.x = 1 for short sequences: 10 240 tiny workgroups - twiddles,
    // window and launch overhead per 8 frames - were 133 us per scale at config #5; one workgroup per (b, c) now)
    for (int f0 = blockIdx.x * 8; f0 < frames; f0 += gridDim.x * 8) {
        __syncthreads();                                    // twiddles ready / the previous block's frames consumed
        for (int i = threadIdx.x; i < 8 * nfft; i += blockDim.x) {
            const int fi = i / nfft, n = i % nfft;
            const int frame = f0 + fi;
            float v = 0.f;
            if (frame < frames) {
                int t = frame * hop + n - nfft / 2;
                if (t < 0) t = -t;                              // reflect padding
                if (t >= T) t = 2 * (T - 1) - t;
                v = xr[t] * win[n];
            }
            fr[i] = v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 8 * F; i += blockDim.x) {
            const int fi = i / F, f = i % F;
            const int frame = f0 + fi;
            if (frame >= frames) continue;
            float re = 0.f, im = 0.f;
            const float* fv = fr + fi * nfft;
            for (int n = 0; n < nfft; ++n) {
                const int k = (f * n) & (nfft - 1);             // nfft is a power of two
                re += fv[n] * tw_c[k];
                im -= fv[n] * tw_s[k];
            }
            const float p = re * re + im * im;
            const size_t o = ((size_t)b * frames + frame) * ch_total + ch_off + (size_t)c * F + f;
            if (out) out[o] = (bf16)p;
            if (out_f32) out_f32[o] = p;
        }
    }
}

// The same spectra by a radix-2 FFT (nfft <= 256): one workgroup per (b, c), each of its four waves transforms one frame at
// a time in its own LDS scratch (decimation in time on the bit-reversed, windowed frame; log2(nfft) butterfly stages of
// nfft / 2 butterflies, lanes = butterflies).  The direct DFT above costs nfft MACs per (frame, bin) - 705 M MAC pairs at
// config #5 (64 ch x 1024 samples, nfft 64 + 128, hop 32): 145 us per scale; the FFT needs nfft / 2 * log2(nfft) butterflies
// per frame.  fp32 throughout; twiddles from __sincosf (as the DFT's).
template <int LOG2N>
__global__ __launch_bounds__(256) void stft_power_fft_kernel(const float* __restrict__ x, bf16* __restrict__ out,
                                                             float* __restrict__ out_f32, int C, int T, int hop, int frames,
                                                             int ch_off, int ch_total) {
    constexpr int N = 1 << LOG2N, H = N / 2, F = H + 1;
    __shared__ float tw_c[H], tw_s[H], win[N];
    __shared__ float re[4][N], im[4][N];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int n = tid; n < N; n += 256) {
        float sn, cs;
        __sincosf(6.283185307179586f * (float)n / (float)N, &sn, &cs);
        if (n < H) { tw_c[n] = cs; tw_s[n] = sn; }             // e^{-2 pi i n / N} = tw_c - i tw_s
        win[n] = 0.5f - 0.5f * cs;                              // periodic Hann
    }
    __syncthreads();
    const float* xr = x + ((size_t)b * C + c) * T;
    float* r = re[wave];
    float* q = im[wave];
    // Every wave owns its frame and its own LDS arrays: after the twiddle tables nothing is shared between waves, so the
    // stages are ordered by WAVE-level fences only (a wave's LDS operations execute in issue order; the fence keeps the
    // compiler from moving them).  With a workgroup barrier per stage the four waves advanced in lock-step: ten barriers per
    // frame round in a kernel that is nothing but latency (45 us for nfft = 128 at config #5).
    auto wave_sync = []() __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    const int rounds = (frames + 3) / 4;
    // the samples of the NEXT round's frame are requested before this round's butterflies (a frame's global round trip was
    // as long as its whole transform)
    constexpr int PER = (N + 63) / 64;
    float nxt[PER];
    auto fetch = [&](int frame) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int n = lane + 64 * u;
            int t = frame * hop + n - H;
            if (t < 0) t = -t;                                  // reflect padding (torch.stft center = True)
            if (t >= T) t = 2 * (T - 1) - t;
            nxt[u] = (n < N && frame < frames) ? xr[t] : 0.f;
        }
    };
    fetch(wave);
    for (int it = 0; it < rounds; ++it) {
        const int frame = it * 4 + wave;
        const bool live = frame < frames;
        // bit-reversed store of the windowed frame
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int n = lane + 64 * u;
            if (n < N) {
                const int rv = (int)(__brev((unsigned)n) >> (32 - LOG2N));
                r[rv] = nxt[u] * win[n];
                q[rv] = 0.f;
            }
        }
        if (it + 1 < rounds) fetch(frame + 4);
        wave_sync();
#pragma unroll
        for (int sgm = 0; sgm < LOG2N; ++sgm) {
            const int m = 1 << sgm;                             // half size of this stage's butterflies
            for (int j = lane; j < H; j += 64) {
                const int k = j & (m - 1);
                const int i0 = ((j >> sgm) << (sgm + 1)) + k, i1 = i0 + m;
                const int tk = k << (LOG2N - 1 - sgm);          // twiddle index k * N / (2 m)
                const float wc = tw_c[tk], ws = tw_s[tk];
                const float ar = r[i1], ai = q[i1];
                const float tr = ar * wc + ai * ws, ti = ai * wc - ar * ws;     // (ar + i ai) (wc - i ws)
                const float br = r[i0], bi = q[i0];
                r[i0] = br + tr; q[i0] = bi + ti;
                r[i1] = br - tr; q[i1] = bi - ti;
            }
            wave_sync();
        }
        if (live) {
            const size_t o = ((size_t)b * frames + frame) * ch_total + ch_off + (size_t)c * F;
            for (int f = lane; f < F; f += 64) {
                const float p = r[f] * r[f] + q[f] * q[f];
                if (out) out[o + f] = (bf16)p;
                if (out_f32) out_f32[o + f] = p;
            }
        }
        wave_sync();
    }
}
}  // namespace

extern "C" {
int mm_stft_power(const float* x, void* out_bf16, float* out_f32, int B, int C, int T, int nfft, int hop, int ch_off,
                  int ch_total, hipStream_t st) {
    MM_REQUIRE(x && (out_bf16 || out_f32) && B > 0 && C > 0 && T > 0, "stft_power: null/invalid");
    MM_REQUIRE(nfft >= 8 && nfft <= 1024 && (nfft & (nfft - 1)) == 0 && hop > 0 && T > nfft / 2, "stft_power: nfft=%d hop=%d", nfft, hop);
    const int frames = T / hop + 1;
    const int F = nfft / 2 + 1;
    MM_REQUIRE(ch_off >= 0 && ch_off + C * F <= ch_total, "stft_power: channel window");
    if (nfft <= 256) {                // the FFT form
        const dim3 grid(1, C, B);
        switch (nfft) {
            case 8: hipLaunchKernelGGL((stft_power_fft_kernel<3>), grid, dim3(256), 0, st, x, (bf16*)out_bf16, out_f32, C, T, hop, frames, ch_off, ch_total); break;
            case 16: hipLaunchKernelGGL((stft_power_fft_kernel<4>), grid, dim3(256), 0, st, x, (bf16*)out_bf16, out_f32, C, T, hop, frames, ch_off, ch_total); break;
            case 32: hipLaunchKernelGGL((stft_power_fft_kernel<5>), grid, dim3(256), 0, st, x, (bf16*)out_bf16, out_f32, C, T, hop, frames, ch_off, ch_total); break;
            case 64: hipLaunchKernelGGL((stft_power_fft_kernel<6>), grid, dim3(256), 0, st, x, (bf16*)out_bf16, out_f32, C, T, hop, frames, ch_off, ch_total); break;
            case 128: hipLaunchKernelGGL((stft_power_fft_kernel<7>), grid, dim3(256), 0, st, x, (bf16*)out_bf16, out_f32, C, T, hop, frames, ch_off, ch_total); break;
            default: hipLaunchKernelGGL((stft_power_fft_kernel<8>), grid, dim3(256), 0, st, x, (bf16*)out_bf16, out_f32, C, T, hop, frames, ch_off, ch_total); break;
        }
        return mm_check_launch("stft_power");
    }
    const size_t lds = (size_t)(3 * nfft + 8 * nfft) * sizeof(float);
    // (b, c) pairs fill the chip by themselves at the encoder's sizes: one workgroup each walks all its frame blocks; only a
    // small problem is also split over the frame blocks
    const int fblocks = ceil_div(frames, 8);
    const int gx = (long)B * C >= 1024 ? 1 : (fblocks < 8 ? fblocks : 8);
    hipLaunchKernelGGL(stft_power_kernel, dim3(gx, C, B), dim3(256), lds, st, x, (bf16*)out_bf16, out_f32,
                       C, T, nfft, hop, frames, ch_off, ch_total);
    return mm_check_launch("stft_power");
}
}  // extern "C"

namespace {
// ---------------------------------------------------------------------------
// backward of stft_power_kernel: dx[b, c, t] += sum over the (frame, n) that read sample t (directly or through the
// reflect padding) of win[n] * dv[frame][n],   dv[n] = 2 sum_f gP[f] (re_f cos(2 pi f n / N) - im_f sin(2 pi f n / N)).
// One workgroup per (b, c): frames in blocks of 8 - windowed frames and their DFT recomputed in LDS, the gradient of
// the windowed frame formed by the inverse sum, then every thread GATHERS the contributions to the samples it owns
// in a fixed order (frame ascending; direct, left-reflected, right-reflected position): no atomics, bit-reproducible.
// gP fp32 [B][frames][ch_total] (channels ch_off + c * F + f); dx fp32 [B][C][T] is ADDED to (one launch per scale).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stft_power_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gP,
                                                             float* __restrict__ dx, int C, int T, int nfft, int hop,
                                                             int frames, int ch_off, int ch_total) {
    extern __shared__ float sm[];
    const int F = nfft / 2 + 1;
    float* tw_c = sm;                  // [nfft]
    float* tw_s = tw_c + nfft;         // [nfft]
    float* win = tw_s + nfft;          // [nfft]
    float* fr = win + nfft;            // [8][nfft] windowed frames, then their gradient
    float* cr = fr + 8 * nfft;         // [8][F]  2 gP re
    float* ci = cr + 8 * F;            // [8][F]  2 gP im
    float* acc = ci + 8 * F;           // [T]
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    for (int n = tid; n < nfft; n += 256) {
        float s, co;
        __sincosf(6.283185307179586f * (float)n / (float)nfft, &s, &co);
        tw_c[n] = co; tw_s[n] = s;
        win[n] = 0.5f - 0.5f * __cosf(6.283185307179586f * (float)n / (float)nfft);
    }
    for (int t = tid; t < T; t += 256) acc[t] = 0.f;
    const float* xr = x + ((size_t)b * C + c) * T;
    __syncthreads();
    for (int f0 = 0; f0 < frames; f0 += 8) {
        for (int i = tid; i < 8 * nfft; i += 256) {
            const int fi = i / nfft, n = i % nfft, frame = f0 + fi;
            float v = 0.f;
            if (frame < frames) {
                int t = frame * hop + n - nfft / 2;
                if (t < 0) t = -t;
                if (t >= T) t = 2 * (T - 1) - t;
                v = xr[t] * win[n];
            }
            fr[i] = v;
        }
        __syncthreads();
        for (int i = tid; i < 8 * F; i += 256) {
            const int fi = i / F, f = i % F, frame = f0 + fi;
            float re = 0.f, im = 0.f;
            if (frame < frames) {
                const float* fv = fr + fi * nfft;
                for (int n = 0; n < nfft; ++n) {
                    const int k = (f * n) & (nfft - 1);
                    re += fv[n] * tw_c[k];
                    im -= fv[n] * tw_s[k];
                }
                const float g2 = 2.f * gP[((size_t)b * frames + frame) * ch_total + ch_off + (size_t)c * F + f];
                re *= g2; im *= g2;
            }
            cr[i] = re; ci[i] = im;
        }
        __syncthreads();
        for (int i = tid; i < 8 * nfft; i += 256) {             // gradient of the windowed frame, times the window
            const int fi = i / nfft, n = i % nfft;
            float dv = 0.f;
            const float *pr = cr + fi * F, *pi = ci + fi * F;
            for (int f = 0; f < F; ++f) {
                const int k = (f * n) & (nfft - 1);
                dv += pr[f] * tw_c[k] - pi[f] * tw_s[k];
            }
            fr[i] = dv * win[n];
        }
        __syncthreads();
        for (int t0 = tid; t0 < T; t0 += 256) {
            float a = acc[t0];
            for (int fi = 0; fi < 8; ++fi) {
                const int frame = f0 + fi;
                if (frame >= frames) break;
                const int base = nfft / 2 - frame * hop;
                int n = t0 + base;                                              // read directly
                if (n >= 0 && n < nfft) a += fr[fi * nfft + n];
                n = -t0 + base;                                                 // read as the left reflection of t = -t0
                if (t0 > 0 && n >= 0 && n < nfft) a += fr[fi * nfft + n];
                n = 2 * (T - 1) - t0 + base;                                    // right reflection
                if (t0 < T - 1 && n >= 0 && n < nfft) a += fr[fi * nfft + n];
            }
            acc[t0] = a;
        }
        __syncthreads();
    }
    float* dr = dx + ((size_t)b * C + c) * T;
    for (int t = tid; t < T; t += 256) dr[t] += acc[t];
}
}  // namespace

extern "C" {
int mm_stft_power_bwd(const float* x, const float* g_power, float* dx, int B, int C, int T, int nfft, int hop, int ch_off,
                      int ch_total, hipStream_t st) {
    MM_REQUIRE(x && g_power && dx && B > 0 && C > 0 && T > 0, "stft_power_bwd: null/invalid");
    MM_REQUIRE(nfft >= 8 && nfft <= 1024 && (nfft & (nfft - 1)) == 0 && hop > 0 && T > nfft / 2, "stft_power_bwd: nfft=%d hop=%d", nfft, hop);
    const int frames = T / hop + 1;
    const int F = nfft / 2 + 1;
    MM_REQUIRE(ch_off >= 0 && ch_off + C * F <= ch_total, "stft_power_bwd: channel window");
    const size_t lds = (size_t)(3 * nfft + 8 * nfft + 16 * F + T) * sizeof(float);
    if (lds > 160 * 1024) return mm_fail(MM_ERR_UNSUPPORTED, "stft_power_bwd: T=%d nfft=%d needs %zu bytes of LDS", T, nfft, lds);
    auto kern = stft_power_bwd_kernel;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(C, B), dim3(256), lds, st, x, g_power, dx, C, T, nfft, hop, frames, ch_off, ch_total);
    return mm_check_launch("stft_power_bwd");
}
}  // extern "C"

namespace {
// ---------------------------------------------------------------------------
// normalize_modality (run_training_lite.py:48-51, applied to every sample's power features at :162):
// x[b] <- (x[b] - mean(x[b])) / (std(x[b]) + eps), population std (the reference z-scores numpy arrays: ddof = 0), over ALL elements of sample b, fp32 in ->
// bf16 channels-last out (the Power encoder's first-conv operand).  x [B][rows][ch_total]; only channels
// < ch_valid count (the padding channels stay zero).  One workgroup per sample, two sweeps; fixed-order
// sums (bit-reproducible); the mean is subtracted before squaring (two-pass variance).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sample_zscore_kernel(const float* __restrict__ x, bf16* __restrict__ out,
                                                             int rows, int ch_valid, int ch_total, float eps) {
    __shared__ float red[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xs = x + (size_t)b * rows * ch_total;
    bf16* os = out + (size_t)b * rows * ch_total;
    const size_t n = (size_t)rows * ch_total;
    const float cnt = (float)rows * (float)ch_valid;
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += red[w];
        return t;
    };
    if (ch_valid == ch_total && (ch_total & 3) == 0 && n < (1ull << 31)) {
        // no padding channels (config #5: 6 272 of 6 272): three float4 sweeps with 32-bit indices.  (The general path's 64-bit
        // modulo per ELEMENT and scalar loads made this one-workgroup-per-sample kernel 200 us at config #5.)
        const unsigned n4 = (unsigned)(n >> 2);
        const float4* x4 = reinterpret_cast<const float4*>(xs);
        float s = 0.f;
        for (unsigned i = tid; i < n4; i += 1024) { const float4 v = x4[i]; s += (v.x + v.y) + (v.z + v.w); }
        const float mean = block_sum(s) / cnt;
        float q = 0.f;
        for (unsigned i = tid; i < n4; i += 1024) {
            const float4 v = x4[i];
            const float a = v.x - mean, c = v.y - mean, d = v.z - mean, e = v.w - mean;
            q += (a * a + c * c) + (d * d + e * e);
        }
        const float inv = 1.f / (sqrtf(block_sum(q) / cnt) + eps);   // population std: the reference z-scores numpy arrays (ddof = 0)
        for (unsigned i = tid; i < n4; i += 1024) {
            const float4 v = x4[i];
            bf16x4 o = {(bf16)((v.x - mean) * inv), (bf16)((v.y - mean) * inv), (bf16)((v.z - mean) * inv), (bf16)((v.w - mean) * inv)};
            *reinterpret_cast<bf16x4*>(os + 4 * (size_t)i) = o;
        }
        return;
    }
    float s = 0.f;
    for (size_t i = tid; i < n; i += 1024) s += ((int)(i % ch_total) < ch_valid) ? xs[i] : 0.f;
    const float mean = block_sum(s) / cnt;
    float q = 0.f;
    for (size_t i = tid; i < n; i += 1024) {
        const float d = ((int)(i % ch_total) < ch_valid) ? xs[i] - mean : 0.f;
        q += d * d;
    }
    const float inv = 1.f / (sqrtf(block_sum(q) / cnt) + eps);       // population std: the reference z-scores numpy arrays (ddof = 0)
    for (size_t i = tid; i < n; i += 1024) os[i] = (bf16)(((int)(i % ch_total) < ch_valid) ? (xs[i] - mean) * inv : 0.f);
}

// The same z-score with the sample's elements dealt out over ZS_CHUNKS workgroups (config #5: 33 frames x 6 272 channels per
// sample - one workgroup per sample was 32 workgroups on 256 CUs, 41 us for 40 MB).  Pass 1: every workgroup leaves the sum
// and the sum of squares of its chunk in DOUBLE precision (the variance is then E[x^2] - mean^2 without the two-pass form's
// second sweep; fp64 keeps the cancellation harmless); pass 2: every workgroup adds the sample's partials in chunk order -
// the same value in all of them, the same bits every run - and writes its chunk.  No-padding layouts only (the fast path above).
constexpr int ZS_CHUNKS = 32;
__global__ __launch_bounds__(256) void zscore_partial_kernel(const float* __restrict__ x, double* __restrict__ part, unsigned n4) {
    __shared__ double red[8];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const float4* x4 = reinterpret_cast<const float4*>(x) + (size_t)b * n4;
    const unsigned lo = (unsigned)((unsigned long long)n4 * c / ZS_CHUNKS), hi = (unsigned)((unsigned long long)n4 * (c + 1) / ZS_CHUNKS);
    double s = 0.0, q = 0.0;
    for (unsigned i = lo + tid; i < hi; i += 256) {
        const float4 v = x4[i];
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        q += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6] = s; red[4 + (tid >> 6)] = q; }
    __syncthreads();
    if (tid == 0) {
        double* p = part + ((size_t)b * ZS_CHUNKS + c) * 2;
        p[0] = (red[0] + red[1]) + (red[2] + red[3]);
        p[1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}
__global__ __launch_bounds__(256) void zscore_apply_kernel(const float* __restrict__ x, const double* __restrict__ part,
                                                          bf16* __restrict__ out, unsigned n4, float cnt, float eps) {
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < ZS_CHUNKS; ++k) { s += part[((size_t)b * ZS_CHUNKS + k) * 2]; q += part[((size_t)b * ZS_CHUNKS + k) * 2 + 1]; }
    const double mean_d = s / (double)cnt;
    const double var = fmax(q / (double)cnt - mean_d * mean_d, 0.0);
    const float mean = (float)mean_d, inv = 1.f / ((float)sqrt(var) + eps);
    const float4* x4 = reinterpret_cast<const float4*>(x) + (size_t)b * n4;
    bf16* os = out + (size_t)b * n4 * 4;
    const unsigned lo = (unsigned)((unsigned long long)n4 * c / ZS_CHUNKS), hi = (unsigned)((unsigned long long)n4 * (c + 1) / ZS_CHUNKS);
    for (unsigned i = lo + tid; i < hi; i += 256) {
        const float4 v = x4[i];
        bf16x4 o = {(bf16)((v.x - mean) * inv), (bf16)((v.y - mean) * inv), (bf16)((v.z - mean) * inv), (bf16)((v.w - mean) * inv)};
        *reinterpret_cast<bf16x4*>(os + 4 * (size_t)i) = o;
    }
}
}  // namespace

extern "C" {
int mm_sample_zscore_bf16(const float* x, void* out_bf16, double* ws, int B, int rows, int ch_valid, int ch_total, float eps,
                          hipStream_t st) {
    MM_REQUIRE(x && out_bf16 && B > 0 && rows > 0 && ch_valid > 0 && ch_valid <= ch_total, "sample_zscore: null/invalid");
    const size_t n = (size_t)rows * ch_total;
    if (ws && ch_valid == ch_total && (n & 3) == 0 && n < (1ull << 31) && n >= (1u << 16)) {
        // big unpadded samples: ZS_CHUNKS workgroups per sample, partial sums in ws (MM_ZSCORE_WS_DOUBLES per sample)
        MM_REQUIRE(((uintptr_t)ws & 7) == 0, "sample_zscore: workspace alignment");
        hipLaunchKernelGGL(zscore_partial_kernel, dim3(ZS_CHUNKS, B), dim3(256), 0, st, x, ws, (unsigned)(n >> 2));
        hipLaunchKernelGGL(zscore_apply_kernel, dim3(ZS_CHUNKS, B), dim3(256), 0, st, x, (const double*)ws, (bf16*)out_bf16,
                           (unsigned)(n >> 2), (float)rows * (float)ch_valid, eps);
        return mm_check_launch("sample_zscore(chunked)");
    }
    hipLaunchKernelGGL(sample_zscore_kernel, dim3(B), dim3(1024), 0, st, x, (bf16*)out_bf16, rows, ch_valid, ch_total, eps);
    return mm_check_launch("sample_zscore");
}
}  // extern "C"

namespace {
// backward of sample_zscore_kernel: y = (x - mean) / d, d = std + eps (population std over the cnt valid elements):
//   dx_i = (g_i - mean(g)) / d - y_i * mean(g * y) / std        (padding channels: 0)
// g = bf16 gradient w.r.t. the z-scored (bf16) tensor, same layout; dx fp32.  Fixed-order block sums.
__global__ __launch_bounds__(1024) void sample_zscore_bwd_kernel(const float* __restrict__ x, const bf16* __restrict__ g,
                                                                 float* __restrict__ dx, int rows, int ch_valid, int ch_total,
                                                                 float eps) {
    __shared__ float red[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = (size_t)rows * ch_total;
    const float* xs = x + (size_t)b * n;
    const bf16* gs = g + (size_t)b * n;
    float* os = dx + (size_t)b * n;
    const float cnt = (float)rows * (float)ch_valid;
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += red[w];
        return t;
    };
    auto valid = [&](size_t i) { return (int)(i % ch_total) < ch_valid; };
    float s = 0.f;
    for (size_t i = tid; i < n; i += 1024) s += valid(i) ? xs[i] : 0.f;
    const float mean = block_sum(s) / cnt;
    float q = 0.f;
    for (size_t i = tid; i < n; i += 1024) {
        const float d = valid(i) ? xs[i] - mean : 0.f;
        q += d * d;
    }
    const float sd = sqrtf(block_sum(q) / cnt);
    const float inv = 1.f / (sd + eps);
    float sg = 0.f, sgy = 0.f;
    for (size_t i = tid; i < n; i += 1024)
        if (valid(i)) {
            const float gi = (float)gs[i];
            sg += gi;
            sgy += gi * (xs[i] - mean) * inv;
        }
    const float mg = block_sum(sg) / cnt;
    const float mgy = block_sum(sgy) / cnt;
    const float c2 = mgy / fmaxf(sd, 1e-30f);
    for (size_t i = tid; i < n; i += 1024)
        os[i] = valid(i) ? ((float)gs[i] - mg) * inv - (xs[i] - mean) * inv * c2 : 0.f;
}
}  // namespace

extern "C" {
int mm_sample_zscore_bwd(const float* x, const void* g_bf16, float* dx, int B, int rows, int ch_valid, int ch_total, float eps,
                         hipStream_t st) {
    MM_REQUIRE(x && g_bf16 && dx && B > 0 && rows > 0 && ch_valid > 0 && ch_valid <= ch_total, "sample_zscore_bwd: null/invalid");
    hipLaunchKernelGGL(sample_zscore_bwd_kernel, dim3(B), dim3(1024), 0, st, x, (const bf16*)g_bf16, dx, rows, ch_valid, ch_total, eps);
    return mm_check_launch("sample_zscore_bwd");
}
}  // extern "C"

namespace {
// ---------------------------------------------------------------------------
// EnhancedPowerEncoder's three parallel Conv1d(C -> 64, k = 3 | 5 | 7) + BatchNorm1d(64) branches
// (enhanced_models_v4.py:210-234) run as ONE Conv1d(C -> 192, k = 7) + BatchNorm1d(192).  The merged tensors are built
// from the parts, their running statistics handed back, and their gradients added back into the parts' - each in one
// launch (the host glue was ~55 tiny torch launches per training step: pads, cats, slice copies, slice adds).
//   mode 0: parts -> merged      W[o][c][t] = w_i[o % 64][c][t - lo_i] inside the branch's taps, else 0  (i = o / 64,
//                                 lo_i = (7 - k_i) / 2: the shorter kernels sit around the centre tap);  vectors concatenated
//   mode 1: merged running mean / var -> the parts';  batches_tracked += 1
//   mode 2: parts' gradient sinks += their slices of the merged gradients (null part = frozen parameter: skipped)
//   mode 3: as mode 0, but the merged WEIGHT is written as the forward kernel's bf16 image [192][7][cinp] (what
//           mm_prep_conv_weight would make of the fp32 merged weight, which is then never materialised: 33 MB written and
//           read back per step at config #5); W points to that image
// ---------------------------------------------------------------------------
struct PowerMergeArgs {
    float* w[3]; float* b[3]; float* gamma[3]; float* beta[3]; float* run_mean[3]; float* run_var[3];
    long long* tracked[3];
    float* W; float* B; float* Gamma; float* Beta; float* Run_mean; float* Run_var;
    int cin, k[3], cinp, reserved;
};

template <int MODE>
__global__ void power_merge_kernel(PowerMergeArgs a) {
    const size_t per_o = (size_t)a.cin * 7, total = 192 * per_o;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid < 192) {                                          // the per-channel vectors
        const int i = (int)gid / 64, j = (int)gid % 64;
        if (MODE == 0 || MODE == 3) {
            a.B[gid] = a.b[i][j]; a.Gamma[gid] = a.gamma[i][j]; a.Beta[gid] = a.beta[i][j];
            a.Run_mean[gid] = a.run_mean[i][j]; a.Run_var[gid] = a.run_var[i][j];
        } else if (MODE == 1) {
            a.run_mean[i][j] = a.Run_mean[gid]; a.run_var[i][j] = a.Run_var[gid];
            if (j == 0 && a.tracked[i]) a.tracked[i][0] += 1;
        } else {
            if (a.b[i] && a.B) a.b[i][j] += a.B[gid];
            if (a.gamma[i] && a.Gamma) a.gamma[i][j] += a.Gamma[gid];
            if (a.beta[i] && a.Beta) a.beta[i][j] += a.Beta[gid];
        }
    }
    if (MODE == 1 || (MODE == 2 && !a.W)) return;
    if (MODE == 3) {
        // image element (o, t, c): channel-contiguous stores; the fp32 reads of a branch stride by its kernel size
        bf16* img = reinterpret_cast<bf16*>(a.W);
        const size_t per_oi = (size_t)7 * a.cinp, itotal = 192 * per_oi;
        for (size_t e = gid; e < itotal; e += (size_t)gridDim.x * blockDim.x) {
            const int o = (int)(e / per_oi);
            const int r = (int)(e - (size_t)o * per_oi);
            const int t = r / a.cinp, c = r - t * a.cinp;
            const int i = o / 64, k = a.k[i], lo = (7 - k) >> 1;
            const bool in = c < a.cin && t >= lo && t < lo + k;
            img[e] = (bf16)(in ? a.w[i][((size_t)(o - 64 * i) * a.cin + c) * k + (t - lo)] : 0.f);
        }
        return;
    }
    for (size_t e = gid; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int o = (int)(e / per_o);
        const int r = (int)(e - (size_t)o * per_o);
        const int c = r / 7, t = r - 7 * c;
        const int i = o / 64, k = a.k[i], lo = (7 - k) >> 1;
        const bool in = t >= lo && t < lo + k;
        const size_t pe = ((size_t)(o - 64 * i) * a.cin + c) * k + (t - lo);
        if (MODE == 0) a.W[e] = in ? a.w[i][pe] : 0.f;
        else if (in && a.w[i]) a.w[i][pe] += a.W[e];
    }
}
}  // namespace

extern "C" {
int mm_power_merge(const void* desc_host, int mode, hipStream_t st) {
    MM_REQUIRE(desc_host && mode >= 0 && mode <= 3, "power_merge: null / mode");
    const PowerMergeArgs a = *static_cast<const PowerMergeArgs*>(desc_host);
    MM_REQUIRE(a.cin > 0, "power_merge: cin");
    for (int i = 0; i < 3; ++i) MM_REQUIRE(a.k[i] == 3 || a.k[i] == 5 || a.k[i] == 7, "power_merge: kernel sizes must be 3, 5 or 7");
    if (mode == 0 || mode == 3) {
        for (int i = 0; i < 3; ++i)
            MM_REQUIRE(a.w[i] && a.b[i] && a.gamma[i] && a.beta[i] && a.run_mean[i] && a.run_var[i], "power_merge(0): null part");
        MM_REQUIRE(a.W && a.B && a.Gamma && a.Beta && a.Run_mean && a.Run_var, "power_merge(0): null merged tensor");
        MM_REQUIRE(mode == 0 || (a.cinp >= a.cin && a.cinp % 16 == 0), "power_merge(3): cinp=%d", a.cinp);
    } else if (mode == 1) {
        for (int i = 0; i < 3; ++i) MM_REQUIRE(a.run_mean[i] && a.run_var[i], "power_merge(1): null part");
        MM_REQUIRE(a.Run_mean && a.Run_var, "power_merge(1): null merged statistics");
    }
    const size_t total = (size_t)192 * a.cin * 7;
    const int grid = mode == 1 ? 1 : grid_for(total, 2048);
    if (mode == 3) hipLaunchKernelGGL(power_merge_kernel<3>, dim3(grid), dim3(256), 0, st, a);
    else if (mode == 0) hipLaunchKernelGGL(power_merge_kernel<0>, dim3(grid), dim3(256), 0, st, a);
    else if (mode == 1) hipLaunchKernelGGL(power_merge_kernel<1>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(power_merge_kernel<2>, dim3(grid), dim3(256), 0, st, a);
    return mm_check_launch("power_merge");
}
}  // extern "C"
