// On-device fMRI volume augmentation (the reference has no volume code, SURVEY section 0: the transform is this package's
// own): per sample of a (B, 1, D, H, W) fp32 batch, each with a probability of its own, a mirror of the W
// axis, an integer translation, an intensity scale, Gaussian noise of noise_factor * std(sample), and one cuboid erased.
// It sits beside the EEG augmenter (augment.hip) and follows it: counter-based draws, no state on the device, two launches.
//
// ---- the random stream: h(stream, idx), stream(seed, step, rank, purpose), thresh(p), the uniform draw and the scale
// factor are aug_stream.h's (tests/test_volume_augment_*.py carry an fp64 replica).  This file's
// purposes, one per decision and per drawn quantity:
//     5 flip decision   6 shift decision   7 dz   8 dy   9 dx   10 scale decision   11 scale u   12 noise decision
//     13 gauss a   14 gauss b   15 erase decision   16 erase z   17 erase y   18 erase x
//   every draw of sample b is h(stream_k, b) (the noise: of the pair index below):
//     dz, dy, dx = uniform[0, 2 * max_shift + 1) - max_shift           (0, 0, 0 when the shift is off)
//     factor = aug_scale_factor(scale_range, h)                        (1.0f when off)
//     erase corner (ez, ey, ex) = uniform[0, D - ed + 1), [0, H - eh + 1), [0, W - ew + 1);  the extents ed, eh, ew
//     = max(1, int(erase_fraction * D)), ... are formed on the host
//   output voxel (z, y, x) of sample b, v = (z * H + y) * W + x, V = D * H * W:
//     inside the erased cuboid                               -> fill, exactly
//     (zs, ys, xs) = (z - dz, y - dy, x - dx) outside the volume -> fill, exactly (no scale, no noise)
//     else  val = src[zs][ys][flip ? W - 1 - xs : xs]
//           val = val * factor                               if the scale is on (one fp32 rounding)
//           val = val + z_v * ns                             if ns != 0: ns = noise_factor * std_b in fp32 when the noise
//                                                            is on, else 0 (two fp32 roundings: the product, the sum)
//     std_b = the unbiased standard deviation of the ORIGINAL sample over its V voxels
//     voxels (v, v + 1), v even, share the Box-Muller pair idx = b * ceil(V / 2) + v / 2:
//           u1 = (h(stream13, idx) + 1) * 2^-32 in (0, 1],  u2 = h(stream14, idx) * 2^-32
//           z_v = sqrt(-2 ln u1) cos(2 pi u2),  z_{v+1} = sqrt(-2 ln u1) sin(2 pi u2);  an odd V uses z_v alone at the end
//   A sample with no decision on - or with the noise alone and std_b = 0 - passes through bit for bit.
//
// ---- the two launches -----------------------------------------------------------------------------------------------
// mm_volume_augment_plan: workgroup (b, k) sums chunk k of sample b as fp64 {sum, sum of squares} partials, the scheme of
//   eeg_augment_plan_kernel (4096 values per workgroup, doubled until a sample has at most 64 chunks; fixed order, no
//   atomics).  A thread adds whole groups of four consecutive values, in order; a group is ONE 16-byte load when the
//   sample's base address allows it and four 4-byte loads otherwise (V is usually no multiple of 4: 91 x 109 x 91 is odd),
//   so std_b has the same bits whatever the alignment.  Workgroup (b, 0) also writes the sample's header.
// mm_volume_augment: a workgroup handles 2048 Box-Muller pairs (4096 output voxels) of one sample; consecutive threads take
//   consecutive pairs, so a wave writes one contiguous run and reads contiguous (flipped: reversed) runs of source rows.
//   Every workgroup adds its sample's partials in chunk order (<= 64 pairs of doubles, the same bits in every workgroup);
//   the sample's first workgroup stores the noise scale and std_b into the plan.
//
// plan (32-bit words; include/mmeeg_hip.h): per sample 16 words -
//   [0] flags (bit 0 flip, 1 shift, 2 scale, 3 noise, 4 erase)   [1] dz  [2] dy  [3] dx (int32)   [4] factor (fp32)
//   [5] ez  [6] ey  [7] ex   [8] ed  [9] eh  [10] ew (0 when the erase is off)   [11] ns (fp32)   [12] std_b (fp32)
//   [13..15] 0 - then, from word 16 * B, the partials double[B][nchunk][2].  Words 11 and 12 are mm_volume_augment's.
#include <cmath>

#include "aug_stream.h"
#include "common.h"
#include "mmeeg_hip.h"

// the contract is the replica's fp32 operations, each rounded on its own: val * factor + z * ns must not become an FMA
#pragma clang fp contract(off)

namespace {

constexpr int VOL_HDR = 16;
constexpr int VOL_PAIRS = 2048;                    // Box-Muller pairs per workgroup of mm_volume_augment (8 per thread)
enum : uint32_t { VF_FLIP = 1, VF_SHIFT = 2, VF_SCALE = 4, VF_NOISE = 8, VF_ERASE = 16 };

struct VolShape { int chunk, nchunk; int64_t words; };
// the layout of the plan for (B, V): ops.volume_augment_plan_layout computes the same
inline VolShape vol_shape(int B, int64_t V) {
    VolShape s;
    const AugChunks k = aug_chunks(V);
    s.chunk = k.chunk;
    s.nchunk = k.nchunk;
    s.words = (int64_t)B * VOL_HDR + 4 * (int64_t)B * s.nchunk;
    return s;
}
inline bool prob_ok(float p) { return p >= 0.f && p <= 1.f; }

struct VolPlanArgs {
    const float* x; uint32_t* plan;
    int B, D, H, W, chunk, nchunk, max_shift, ed, eh, ew;
    uint32_t V;
    float scale_range;
    uint64_t t_flip, t_shift, t_scale, t_noise, t_erase;
    uint32_t s_flip, s_shift, s_dz, s_dy, s_dx, s_scale, s_scale_u, s_noise, s_erase, s_ez, s_ey, s_ex;
};

__global__ void __launch_bounds__(256) volume_augment_plan_kernel(VolPlanArgs a) {
    __shared__ double red[4][2];
    const int b = blockIdx.x / a.nchunk, k = blockIdx.x % a.nchunk;
    const int tid = threadIdx.x;
    const float* xs = a.x + (size_t)b * a.V;
    const uint32_t lo = (uint32_t)k * (uint32_t)a.chunk;                        // (a multiple of 4)
    const uint32_t hi = a.V - lo > (uint32_t)a.chunk ? lo + (uint32_t)a.chunk : a.V;
    const bool aligned = ((uintptr_t)xs & 15) == 0;
    double s = 0.0, q = 0.0;
    // groups of four consecutive values, the same order on both paths (a ragged last group is the scalar path's)
#pragma unroll 4
    for (uint32_t g = lo / 4 + tid; g * 4 < hi; g += 256) {
        const uint32_t i = g * 4;
        if (aligned && hi - i >= 4) {
            const float4 v = *reinterpret_cast<const float4*>(xs + i);
            s += (double)v.x; q += (double)v.x * (double)v.x;
            s += (double)v.y; q += (double)v.y * (double)v.y;
            s += (double)v.z; q += (double)v.z * (double)v.z;
            s += (double)v.w; q += (double)v.w * (double)v.w;
        } else {
            const uint32_t n = hi - i < 4 ? hi - i : 4;
            for (uint32_t j = 0; j < n; ++j) {
                const double v = (double)xs[i + j];
                s += v; q += v * v;
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6][0] = s; red[tid >> 6][1] = q; }
    __syncthreads();
    if (tid != 0) return;
    double* part = reinterpret_cast<double*>(a.plan + (size_t)a.B * VOL_HDR) + ((size_t)b * a.nchunk + k) * 2;
    part[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    part[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    if (k != 0) return;
    // the sample's header
    uint32_t* hdr = a.plan + (size_t)b * VOL_HDR;
    const uint32_t ub = (uint32_t)b;
    uint32_t flags = 0;
    if ((uint64_t)aug_hash(a.s_flip, ub) < a.t_flip) flags |= VF_FLIP;
    if ((uint64_t)aug_hash(a.s_shift, ub) < a.t_shift) flags |= VF_SHIFT;
    if ((uint64_t)aug_hash(a.s_scale, ub) < a.t_scale) flags |= VF_SCALE;
    if ((uint64_t)aug_hash(a.s_noise, ub) < a.t_noise) flags |= VF_NOISE;
    if ((uint64_t)aug_hash(a.s_erase, ub) < a.t_erase) flags |= VF_ERASE;
    const bool sh = flags & VF_SHIFT, er = flags & VF_ERASE;
    const uint32_t span = 2u * (uint32_t)a.max_shift + 1u;
    hdr[0] = flags;
    hdr[1] = (uint32_t)(sh ? (int)aug_uniform(aug_hash(a.s_dz, ub), span) - a.max_shift : 0);
    hdr[2] = (uint32_t)(sh ? (int)aug_uniform(aug_hash(a.s_dy, ub), span) - a.max_shift : 0);
    hdr[3] = (uint32_t)(sh ? (int)aug_uniform(aug_hash(a.s_dx, ub), span) - a.max_shift : 0);
    float factor = 1.0f;
    if (flags & VF_SCALE) factor = aug_scale_factor(a.scale_range, aug_hash(a.s_scale_u, ub));
    hdr[4] = __float_as_uint(factor);
    hdr[5] = er ? aug_uniform(aug_hash(a.s_ez, ub), (uint32_t)(a.D - a.ed + 1)) : 0u;
    hdr[6] = er ? aug_uniform(aug_hash(a.s_ey, ub), (uint32_t)(a.H - a.eh + 1)) : 0u;
    hdr[7] = er ? aug_uniform(aug_hash(a.s_ex, ub), (uint32_t)(a.W - a.ew + 1)) : 0u;
    hdr[8] = er ? (uint32_t)a.ed : 0u;
    hdr[9] = er ? (uint32_t)a.eh : 0u;
    hdr[10] = er ? (uint32_t)a.ew : 0u;
    hdr[11] = 0u; hdr[12] = 0u;                     // (mm_volume_augment's words)
    hdr[13] = 0u; hdr[14] = 0u; hdr[15] = 0u;
}

struct VolAugArgs {
    const float* x; const uint32_t* plan; uint32_t* plan_w; float* out;
    int B, D, H, W, nchunk, nblk;
    uint32_t V, half;
    float noise_factor, fill;
    uint32_t s_ga, s_gb;
};

struct VolSample {
    bool flip, scale, erase;
    int dz, dy, dx;
    uint32_t ez, ey, ex, ed, eh, ew;
    float factor, ns, fill;
};

__device__ __forceinline__ float vol_voxel(const VolAugArgs& a, const VolSample& p, const float* src, uint32_t v, float zn) {
    const uint32_t x = v % (uint32_t)a.W, t = v / (uint32_t)a.W;
    const uint32_t y = t % (uint32_t)a.H, z = t / (uint32_t)a.H;
    if (p.erase && z - p.ez < p.ed && y - p.ey < p.eh && x - p.ex < p.ew) return p.fill;         // (unsigned: one compare per side pair)
    const int zs = (int)z - p.dz, ys = (int)y - p.dy, xs = (int)x - p.dx;
    if ((unsigned)zs >= (unsigned)a.D || (unsigned)ys >= (unsigned)a.H || (unsigned)xs >= (unsigned)a.W) return p.fill;
    const int sx = p.flip ? a.W - 1 - xs : xs;
    float val = src[((size_t)zs * a.H + ys) * a.W + sx];
    if (p.scale) val = val * p.factor;
    if (p.ns != 0.f) val = val + zn * p.ns;
    return val;
}

__global__ void __launch_bounds__(256) volume_augment_kernel(VolAugArgs a) {
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x % a.nblk;
    const uint32_t* hdr = a.plan + (size_t)b * VOL_HDR;
    // std_b from the chunk partials, in chunk order
    const double* part = reinterpret_cast<const double*>(a.plan + (size_t)a.B * VOL_HDR) + (size_t)b * a.nchunk * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < a.nchunk; ++k) { s1 += part[2 * k]; s2 += part[2 * k + 1]; }
    const double n = (double)a.V;
    double var = (s2 - s1 * (s1 / n)) / (n - 1.0);
    var = var < 0.0 ? 0.0 : var;                                   // (a NaN stays a NaN)
    const float std_b = (float)sqrt(var);
    const uint32_t flags = hdr[0];
    VolSample p;
    p.flip = flags & VF_FLIP; p.scale = flags & VF_SCALE; p.erase = flags & VF_ERASE;
    p.dz = (int)hdr[1]; p.dy = (int)hdr[2]; p.dx = (int)hdr[3];
    p.factor = __uint_as_float(hdr[4]);
    p.ez = hdr[5]; p.ey = hdr[6]; p.ex = hdr[7]; p.ed = hdr[8]; p.eh = hdr[9]; p.ew = hdr[10];
    p.ns = (flags & VF_NOISE) ? a.noise_factor * std_b : 0.f;
    p.fill = a.fill;
    if (blk == 0 && threadIdx.x == 0) {
        uint32_t* w = a.plan_w + (size_t)b * VOL_HDR;
        w[11] = __float_as_uint(p.ns); w[12] = __float_as_uint(std_b);
    }
    const float* src = a.x + (size_t)b * a.V;
    float* dst = a.out + (size_t)b * a.V;
    const uint32_t p0 = (uint32_t)blk * VOL_PAIRS + threadIdx.x;
    for (int j = 0; j < VOL_PAIRS / 256; ++j) {                     // a thread: the two voxels of one Box-Muller pair
        const uint32_t pi = p0 + (uint32_t)j * 256u;
        if (pi >= a.half) break;
        const uint32_t v = 2u * pi;
        const bool two = v + 1u < a.V;
        float z0 = 0.f, z1 = 0.f;
        if (p.ns != 0.f) {
            const uint32_t idx = (uint32_t)b * a.half + pi;
            const float u1 = ((float)aug_hash(a.s_ga, idx) + 1.0f) * 2.3283064365386963e-10f;   // 2^-32
            const float w2 = (float)aug_hash(a.s_gb, idx) * 4.6566128730773926e-10f;            // 2 u2
            const float r = sqrtf(-2.0f * logf(u1));
            float sn, cs;
            sincospif(w2, &sn, &cs);
            z0 = r * cs; z1 = r * sn;
        }
        dst[v] = vol_voxel(a, p, src, v, z0);
        if (two) dst[v + 1u] = vol_voxel(a, p, src, v + 1u, z1);
    }
}

int vol_check_shape(const char* who, int B, int D, int H, int W) {
    MM_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "%s: bad shape", who);
    const int64_t V = (int64_t)D * H * W;
    MM_REQUIRE(V >= 2, "%s: a sample needs D * H * W >= 2 voxels for its standard deviation", who);
    MM_REQUIRE(V < (1ll << 31), "%s: D * H * W must be below 2^31 (the voxel index)", who);
    MM_REQUIRE((int64_t)B * ((V + 1) / 2) < (1ll << 32), "%s: B * ceil(D * H * W / 2) must be below 2^32 (the stream's index)", who);
    return MM_OK;
}

}  // namespace

extern "C" {

int mm_volume_augment_plan(const float* x, uint32_t* plan, int64_t plan_words, int B, int D, int H, int W, float p_flip,
                           float p_shift, int max_shift, float p_scale, float scale_range, float p_noise, float p_erase, int ed,
                           int eh, int ew, uint32_t s_flip, uint32_t s_shift, uint32_t s_dz, uint32_t s_dy, uint32_t s_dx,
                           uint32_t s_scale, uint32_t s_scale_u, uint32_t s_noise, uint32_t s_erase, uint32_t s_ez, uint32_t s_ey,
                           uint32_t s_ex, hipStream_t st) {
    if (int rc = vol_check_shape("volume_augment_plan", B, D, H, W)) return rc;
    MM_REQUIRE(x && plan && ((uintptr_t)plan & 7) == 0, "volume_augment_plan: null batch or plan (the plan is 8-byte aligned)");
    MM_REQUIRE(prob_ok(p_flip) && prob_ok(p_shift) && prob_ok(p_scale) && prob_ok(p_noise) && prob_ok(p_erase),
               "volume_augment_plan: probabilities lie in [0, 1]");
    const int dmin = D < H ? (D < W ? D : W) : (H < W ? H : W);
    MM_REQUIRE(max_shift >= 0 && max_shift < dmin, "volume_augment_plan: max_shift must lie in [0, min(D, H, W))");
    MM_REQUIRE(scale_range >= 0.f && scale_range < 1.f, "volume_augment_plan: scale_range must lie in [0, 1)");
    MM_REQUIRE(ed >= 1 && ed <= D && eh >= 1 && eh <= H && ew >= 1 && ew <= W,
               "volume_augment_plan: the erased cuboid's extents must lie in [1, D] x [1, H] x [1, W]");
    const int64_t V = (int64_t)D * H * W;
    const VolShape s = vol_shape(B, V);
    MM_REQUIRE(plan_words >= s.words, "volume_augment_plan: the plan needs %lld words", (long long)s.words);
    MM_REQUIRE((int64_t)B * s.nchunk < (1ll << 31), "volume_augment_plan: too many workgroups");
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)B * V * 4, q0 = (uintptr_t)plan, q1 = q0 + (size_t)s.words * 4;
    MM_REQUIRE(x1 <= q0 || q1 <= x0, "volume_augment_plan: the plan overlaps the batch");
    VolPlanArgs a;
    a.x = x; a.plan = plan; a.B = B; a.D = D; a.H = H; a.W = W; a.V = (uint32_t)V; a.chunk = s.chunk; a.nchunk = s.nchunk;
    a.max_shift = max_shift; a.ed = ed; a.eh = eh; a.ew = ew; a.scale_range = scale_range;
    a.t_flip = aug_thresh(p_flip); a.t_shift = aug_thresh(p_shift); a.t_scale = aug_thresh(p_scale);
    a.t_noise = aug_thresh(p_noise); a.t_erase = aug_thresh(p_erase);
    a.s_flip = s_flip; a.s_shift = s_shift; a.s_dz = s_dz; a.s_dy = s_dy; a.s_dx = s_dx; a.s_scale = s_scale;
    a.s_scale_u = s_scale_u; a.s_noise = s_noise; a.s_erase = s_erase; a.s_ez = s_ez; a.s_ey = s_ey; a.s_ex = s_ex;
    hipLaunchKernelGGL(volume_augment_plan_kernel, dim3(B * s.nchunk), dim3(256), 0, st, a);
    return mm_check_launch("volume_augment_plan");
}

int mm_volume_augment(const float* x, uint32_t* plan, int64_t plan_words, float* out, int B, int D, int H, int W,
                      float noise_factor, float fill, uint32_t s_gauss_a, uint32_t s_gauss_b, hipStream_t st) {
    if (int rc = vol_check_shape("volume_augment", B, D, H, W)) return rc;
    MM_REQUIRE(x && out && plan && ((uintptr_t)plan & 7) == 0, "volume_augment: null batch, output or plan (the plan is 8-byte aligned)");
    MM_REQUIRE(std::isfinite(noise_factor) && std::isfinite(fill), "volume_augment: noise_factor and fill must be finite");
    const int64_t V = (int64_t)D * H * W;
    const VolShape s = vol_shape(B, V);
    MM_REQUIRE(plan_words >= s.words, "volume_augment: the plan needs %lld words", (long long)s.words);
    const size_t bytes = (size_t)B * V * 4;
    const uintptr_t x0 = (uintptr_t)x, o0 = (uintptr_t)out, q0 = (uintptr_t)plan, q1 = q0 + (size_t)s.words * 4;
    MM_REQUIRE(x0 + bytes <= o0 || o0 + bytes <= x0,
               "volume_augment: source and destination overlap (the shift is a gather: augment into another buffer)");
    MM_REQUIRE((x0 + bytes <= q0 || q1 <= x0) && (o0 + bytes <= q0 || q1 <= o0), "volume_augment: the plan overlaps a batch");
    VolAugArgs a;
    a.half = (uint32_t)((V + 1) / 2);
    a.nblk = (int)((a.half + VOL_PAIRS - 1) / VOL_PAIRS);
    MM_REQUIRE((int64_t)B * a.nblk < (1ll << 31), "volume_augment: too many workgroups");
    a.x = x; a.plan = plan; a.plan_w = plan; a.out = out; a.B = B; a.D = D; a.H = H; a.W = W; a.nchunk = s.nchunk; a.V = (uint32_t)V;
    a.noise_factor = noise_factor; a.fill = fill; a.s_ga = s_gauss_a; a.s_gb = s_gauss_b;
    hipLaunchKernelGGL(volume_augment_kernel, dim3(B * a.nblk), dim3(256), 0, st, a);
    return mm_check_launch("volume_augment");
}

}  // extern "C"
