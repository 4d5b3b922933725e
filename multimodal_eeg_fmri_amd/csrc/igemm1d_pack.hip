// Layout packers and weight images of the 1-D implicit-GEMM family (igemm1d.hip): (B, C, T) fp32 <-> channels-last bf16
// operands, a step's inputs into its static buffers in one launch, and a conv / Linear weight -> its forward and
// data-gradient bf16 images, one tensor or a whole model's per launch.
#include "common.h"

namespace {
// (B, C, T) fp32  ->  (B, T, Cp) bf16, channels zero-padded to Cp
__global__ void pack_nct_kernel(const float* __restrict__ x, bf16* __restrict__ y, int C, int T, int Cp) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 256 threads: 32 x 8
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, t = t0 + tx;
        tile[i][tx] = (c < C && t < T) ? x[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, c = c0 + tx;
        if (t < T && c < Cp) y[((size_t)b * T + t) * Cp + c] = (bf16)tile[tx][i];
    }
}
}  // namespace

extern "C" {
int mm_pack_nct_bf16(const float* x, void* y, int B, int C, int T, int Cp, hipStream_t st) {
    MM_REQUIRE(x && y && B > 0 && C > 0 && T > 0 && Cp >= C && Cp % 16 == 0, "pack_nct: bad args");
    dim3 grid(ceil_div(T, 32), ceil_div(Cp, 32), B);
    hipLaunchKernelGGL(pack_nct_kernel, grid, dim3(256), 0, st, x, (bf16*)y, C, T, Cp);
    return mm_check_launch("pack_nct");
}
}  // extern "C"

namespace {
// A step's inputs into the static buffers of a captured step, ONE launch: the EEG batch (B, C, T) fp32 is packed straight
// into the channels-last bf16 operand (B, T, Cp) of the first convolution (and, optionally, copied as fp32), the fMRI
// batch is copied.  Workgroups [0, npack) are pack_nct tiles, the rest copy.
__global__ void stage_inputs_kernel(const float* __restrict__ x, bf16* __restrict__ y, float* __restrict__ x_copy, int B, int C,
                                    int T, int Cp, int npack, float4* __restrict__ d1, const float4* __restrict__ s1, size_t n1) {
    __shared__ float tile[32][33];
    if ((int)blockIdx.x >= npack) {
        const size_t nb = gridDim.x - npack;
        for (size_t i = (size_t)(blockIdx.x - npack) * blockDim.x + threadIdx.x; i < n1; i += nb * blockDim.x) d1[i] = s1[i];
        return;
    }
    const int tt = (T + 31) / 32, tc = (Cp + 31) / 32;
    const int b = blockIdx.x / (tt * tc), rem = blockIdx.x % (tt * tc);
    const int t0 = (rem % tt) * 32, c0 = (rem / tt) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, t = t0 + tx;
        const float v = (c < C && t < T) ? x[((size_t)b * C + c) * T + t] : 0.f;
        tile[i][tx] = v;
        if (x_copy && c < C && t < T) x_copy[((size_t)b * C + c) * T + t] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, c = c0 + tx;
        if (t < T && c < Cp) y[((size_t)b * T + t) * Cp + c] = (bf16)tile[tx][i];
    }
}
}  // namespace

extern "C" {
int mm_stage_inputs(const float* eeg, void* eeg_packed_bf16, float* eeg_copy, int B, int C, int T, int Cp, float* fmri_dst,
                    const float* fmri_src, int64_t fmri_n, hipStream_t st) {
    MM_REQUIRE(eeg && eeg_packed_bf16 && B > 0 && C > 0 && T > 0 && Cp >= C && Cp % 16 == 0, "stage_inputs: bad EEG args");
    MM_REQUIRE(fmri_dst && fmri_src && fmri_n > 0 && fmri_n % 4 == 0 && (((uintptr_t)fmri_dst | (uintptr_t)fmri_src) & 15) == 0,
               "stage_inputs: fMRI copy needs 16-byte alignment and a multiple of 4 floats");
    const int npack = B * ceil_div(T, 32) * ceil_div(Cp, 32);
    const long n4 = fmri_n / 4;
    const int ncopy = (int)((n4 + 1023) / 1024 < 1024 ? (n4 + 1023) / 1024 : 1024);
    hipLaunchKernelGGL(stage_inputs_kernel, dim3(npack + ncopy), dim3(256), 0, st, eeg, (bf16*)eeg_packed_bf16, eeg_copy, B, C, T, Cp,
                       npack, reinterpret_cast<float4*>(fmri_dst), reinterpret_cast<const float4*>(fmri_src), (size_t)n4);
    return mm_check_launch("stage_inputs");
}
}  // extern "C"

namespace {
// (B, T, Cp) (bf16 grads) -> (B, C, T) fp32  (input-gradient un-pack)
__global__ void unpack_ntc_kernel(const bf16* __restrict__ g, float* __restrict__ dx, int C, int T, int Cp) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, c = c0 + tx;
        tile[i][tx] = (t < T && c < Cp) ? (float)g[((size_t)b * T + t) * Cp + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, t = t0 + tx;
        if (c < C && t < T) dx[((size_t)b * C + c) * T + t] = tile[tx][i];
    }
}
}  // namespace

extern "C" {
int mm_unpack_ntc_f32(const void* g, float* dx, int B, int C, int T, int Cp, hipStream_t st) {
    MM_REQUIRE(g && dx && B > 0 && C > 0 && T > 0 && Cp >= C, "unpack_ntc: bad args");
    dim3 grid(ceil_div(T, 32), ceil_div(Cp, 32), B);
    hipLaunchKernelGGL(unpack_ntc_kernel, grid, dim3(256), 0, st, (const bf16*)g, dx, C, T, Cp);
    return mm_check_launch("unpack_ntc");
}
}  // extern "C"

namespace {
// conv weight (Cout, Cin, k) fp32 -> forward image [Cout][k][Cinp] bf16 and
// data-gradient image [Cinp16][k (flipped)][Coutp] bf16 (Coutp = Cout padded to 16)
__global__ void prep_weight_kernel(const float* __restrict__ w, bf16* __restrict__ wf, bf16* __restrict__ wd,
                                   int Cout, int Cin, int k, int Cinp, int Coutp) {
    const int total_f = Cout * k * Cinp;
    const int CinRows = Cinp;
    const int total_d = wd ? CinRows * k * Coutp : 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total_f + total_d; i += gridDim.x * blockDim.x) {
        if (i < total_f) {
            const int c = i % Cinp, tap = (i / Cinp) % k, n = i / (Cinp * k);
            wf[conv_image_index(Cout, k, Cinp, n, tap, c)] = (bf16)(c < Cin ? w[((size_t)n * Cin + c) * k + tap] : 0.f);
        } else {
            const int d = i - total_f;
            const int n = d % Coutp, tap = (d / Coutp) % k, c = d / (Coutp * k);
            const float v = (c < Cin && n < Cout) ? w[((size_t)n * Cin + c) * k + (k - 1 - tap)] : 0.f;
            wd[conv_image_index(CinRows, k, Coutp, c, tap, n)] = (bf16)v;
        }
    }
}
}  // namespace

extern "C" {
int mm_prep_conv_weight(const float* w, void* w_fwd, void* w_dgrad, int Cout, int Cin, int k,
                        int Cinp, int Coutp, hipStream_t st) {
    MM_REQUIRE(w && w_fwd && Cinp % 16 == 0 && Cinp >= Cin && (!w_dgrad || (Coutp % 16 == 0 && Coutp >= Cout)),
               "prep_conv_weight: bad args");
    const int total = Cout * k * Cinp + (w_dgrad ? Cinp * k * Coutp : 0);
    hipLaunchKernelGGL(prep_weight_kernel, dim3(ceil_div(total, 256) < 1024 ? ceil_div(total, 256) : 1024), dim3(256),
                       0, st, w, (bf16*)w_fwd, (bf16*)w_dgrad, Cout, Cin, k, Cinp, Coutp);
    return mm_check_launch("prep_conv_weight");
}
}  // extern "C"

namespace {
// every weight image of a model in one launch (blockIdx.y = tensor): a training step repacks ~40
// small tensors after each optimizer update, and as separate ~5 us nodes they sat on the critical
// path of the step's graph
struct PrepDesc { const float* w; bf16* wf; bf16* wd; int Cout, Cin, k, Cinp, Coutp, pad_; };
constexpr int PM_MAX = 64;
// first[t] = first workgroup of tensor t: workgroups are dealt out in proportion to the elements (PM_EPB per
// workgroup).  128 workgroups per tensor left the step's two largest images (13 elements per thread, gathered with
// a stride of k floats) as a 12 us tail on the chain while the small ones idled.
constexpr int PM_EPB = 1024;
struct PrepTable { PrepDesc d[PM_MAX]; int first[PM_MAX + 1]; };          // by value, as ReduceTable
__global__ void prep_many_kernel(PrepTable tab, int ndesc, float4* __restrict__ zero, long nzero4) {
    if ((int)blockIdx.x >= tab.first[ndesc]) {
        // the step's accumulator arena is zeroed by the same launch (a fill node of its own cost ~5 us on the chain)
        const long b = blockIdx.x - tab.first[ndesc], nb = gridDim.x - tab.first[ndesc];
        for (long i = b * blockDim.x + threadIdx.x; i < nzero4; i += nb * blockDim.x) zero[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    int t = 0;
    while (t + 1 < ndesc && (int)blockIdx.x >= tab.first[t + 1]) ++t;      // (uniform: <= 64 scalar compares)
    const PrepDesc d = tab.d[t];
    const int blk = blockIdx.x - tab.first[t], nblk = tab.first[t + 1] - tab.first[t];
    // one item = 8 consecutive elements of an image's innermost index (c of the forward image, n of the data-gradient
    // image; both padded widths are multiples of 16 and both layouts keep an aligned group of 8 contiguous): two integer
    // divisions and one 16-byte store per 8 elements (three divisions and a 2-byte store per ELEMENT made this launch -
    // the first of the step, in front of both streams - VALU-bound at 10 us)
    const int cg = d.Cinp / 8, ng = d.wd ? d.Coutp / 8 : 0;
    const int items_f = d.Cout * d.k * cg, items_d = d.wd ? d.Cinp * d.k * ng : 0;
    for (int i = blk * blockDim.x + threadIdx.x; i < items_f + items_d; i += nblk * blockDim.x) {
        bf16x8 v;
        if (i < items_f) {
            const int c0 = (i % cg) * 8, r = i / cg, tap = r % d.k, n = r / d.k;
            const float* src = d.w + ((size_t)n * d.Cin + c0) * d.k + tap;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (bf16)(c0 + j < d.Cin ? src[(size_t)j * d.k] : 0.f);
            *reinterpret_cast<bf16x8*>(d.wf + conv_image_index(d.Cout, d.k, d.Cinp, n, tap, c0)) = v;
        } else {
            const int e = i - items_f;
            const int n0 = (e % ng) * 8, r = e / ng, tap = r % d.k, c = r / d.k;
            const float* src = d.w + ((size_t)n0 * d.Cin + c) * d.k + (d.k - 1 - tap);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (bf16)((c < d.Cin && n0 + j < d.Cout) ? src[(size_t)j * d.Cin * d.k] : 0.f);
            *reinterpret_cast<bf16x8*>(d.wd + conv_image_index(d.Cinp, d.k, d.Coutp, c, tap, n0)) = v;
        }
    }
}
}  // namespace

extern "C" {
int mm_prep_many_zero(const void* desc_host, int ndesc, float* zero, int64_t nzero, hipStream_t st) {
    MM_REQUIRE(desc_host && ndesc > 0, "prep_many: bad args");
    MM_REQUIRE(nzero >= 0 && (zero || !nzero) && nzero % 4 == 0 && ((uintptr_t)zero & 15) == 0,
               "prep_many_zero: the zeroed range must be 16-byte aligned and a multiple of 4 floats");
    const PrepDesc* src = (const PrepDesc*)desc_host;
    for (int base = 0; base < ndesc; base += PM_MAX) {
        PrepTable tab;
        const int n = ndesc - base < PM_MAX ? ndesc - base : PM_MAX;
        for (int i = 0; i < n; ++i) {
            const PrepDesc& d = src[base + i];
            MM_REQUIRE(d.w && d.wf && d.Cinp % 16 == 0 && d.Cinp >= d.Cin && d.Cout > 0 && d.k > 0 &&
                       (!d.wd || (d.Coutp % 16 == 0 && d.Coutp >= d.Cout)), "prep_many: descriptor %d", base + i);
            tab.d[i] = d;
        }
        static_assert(sizeof(PrepTable) + 8 <= 4096, "kernel arguments");
        int nblocks = 0;
        for (int i = 0; i < n; ++i) {
            const PrepDesc& d = tab.d[i];
            const long total = (long)d.Cout * d.k * d.Cinp + (d.wd ? (long)d.Cinp * d.k * d.Coutp : 0);
            MM_REQUIRE(total < (1l << 31), "prep_many: descriptor %d too large", base + i);
            tab.first[i] = nblocks;
            nblocks += (int)((total + PM_EPB - 1) / PM_EPB);
        }
        tab.first[n] = nblocks;
        const bool last = base + PM_MAX >= ndesc;                     // the fill rides in the last launch
        const long nz4 = last ? nzero / 4 : 0;
        const int zblocks = (int)((nz4 + 2047) / 2048 < 1024 ? (nz4 + 2047) / 2048 : 1024);
        hipLaunchKernelGGL(prep_many_kernel, dim3(nblocks + zblocks), dim3(256), 0, st, tab, n, reinterpret_cast<float4*>(zero), nz4);
    }
    return mm_check_launch("prep_many");
}

int mm_prep_many(const void* desc_host, int ndesc, hipStream_t st) { return mm_prep_many_zero(desc_host, ndesc, nullptr, 0, st); }
}  // extern "C"
