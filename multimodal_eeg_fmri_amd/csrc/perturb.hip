// Perturbation attribution kernels: the masked copies of a batch as one big batch (occlusion, Shapley coalitions), the
// matching score of every perturbed row against the intact other modality, and the Shapley average over sampled
// permutations.  fp32, contiguous tensors, one writer per output element, every sum formed in a fixed order (the same
// inputs give the same bits).  The expansion is the one bandwidth-sized kernel: 16-byte accesses per lane where the
// innermost length allows it; the other two read a few kilobytes.
#include "common.h"
#include "mmeeg_hip.h"

namespace {

constexpr int PERTURB_THREADS = 256;
constexpr int PERTURB_MAX_GRID = 256 * 8;     // as XAI_MAX_GRID (xai.hip): 256 CUs x 8 workgroups of 4 waves per grid row

// how one sample is cut into units; kind 0: rows of (n0, n1); 1: windows of `size` along n1; 2: size^3 blocks of (n1, n2, n3)
struct PerturbGeom {
    int kind;
    unsigned n1, n2, n3, size, gh, gw;
};

// the unit of element i of ONE sample (i < n0 * n1 [* n2 * n3])
__device__ __forceinline__ unsigned perturb_unit(const PerturbGeom& g, unsigned i) {
    if (g.kind == 0) return i / g.n1;
    if (g.kind == 1) return (i % g.n1) / g.size;
    const unsigned w = i % g.n3, r = i / g.n3, h = r % g.n2, d = (r / g.n2) % g.n1;
    return ((d / g.size) * g.gh + h / g.size) * g.gw + w / g.size;
}

// out[blockIdx.y][e] = mask[unit(e % inner)] ? x[e] : base[...] for the n = B * inner elements e of the batch; `mask` is
// row m0 + blockIdx.y of the table.  No arithmetic: a copy of x's or the baseline's bits, or +0.0f.
// VEC: four elements per lane; ONE_UNIT: the four share a unit (rows, or a window / block edge length that is a
// multiple of 4), so one look-up and ONE of the two loads serve them
template <bool VEC, bool ONE_UNIT>
__global__ __launch_bounds__(PERTURB_THREADS) void perturb_expand_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                                         const int* __restrict__ masks, float* __restrict__ out,
                                                                         unsigned n, unsigned inner, int base_rows, int U, PerturbGeom g) {
    const int* mk = masks + (size_t)blockIdx.y * (size_t)U;
    float* o = out + (size_t)blockIdx.y * (size_t)n;
    const unsigned stride = gridDim.x * PERTURB_THREADS;
    if (VEC) {
        const unsigned nv = n / 4;
        for (unsigned v = blockIdx.x * PERTURB_THREADS + threadIdx.x; v < nv; v += stride) {
            const unsigned e = 4 * v, i = e % inner;
            const f32x4* bp = base_rows ? reinterpret_cast<const f32x4*>(base + (base_rows == 1 ? i : e)) : nullptr;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 r;
            if (ONE_UNIT) {
                r = mk[perturb_unit(g, i)] ? reinterpret_cast<const f32x4*>(x)[v] : (bp ? *bp : zero);
            } else {
                const f32x4 xv = reinterpret_cast<const f32x4*>(x)[v];
                const f32x4 bv = bp ? *bp : zero;
                r[0] = mk[perturb_unit(g, i)] ? xv[0] : bv[0];
                r[1] = mk[perturb_unit(g, i + 1)] ? xv[1] : bv[1];
                r[2] = mk[perturb_unit(g, i + 2)] ? xv[2] : bv[2];
                r[3] = mk[perturb_unit(g, i + 3)] ? xv[3] : bv[3];
            }
            reinterpret_cast<f32x4*>(o)[v] = r;
        }
    } else {
        for (unsigned e = blockIdx.x * PERTURB_THREADS + threadIdx.x; e < n; e += stride) {
            const unsigned i = e % inner;
            o[e] = mk[perturb_unit(g, i)] ? x[e] : (base_rows ? base[base_rows == 1 ? i : e] : 0.f);
        }
    }
}

// v[r] = z[r] . z_other[r % B] for the m * B rows r (mask-major): one wave per row, lane l adds elements l, l + 64, ...
// in ascending order, then the xor butterfly (xai_pair_score_kernel's order)
__global__ __launch_bounds__(64) void perturb_pair_scores_kernel(const float* __restrict__ z, const float* __restrict__ z_other,
                                                                 float* __restrict__ v, int B, int N) {
    const float* zr = z + (size_t)blockIdx.x * N;
    const float* zo = z_other + (size_t)(blockIdx.x % (unsigned)B) * N;
    float sum = 0.f;
    for (int j = threadIdx.x; j < N; j += 64) sum = __fadd_rn(sum, __fmul_rn(zr[j], zo[j]));
    sum = wave_sum(sum);
    if (threadIdx.x == 0) v[blockIdx.x] = sum;
}

// one thread per (u, b), b fastest (the scores are [..][B]): the marginal contribution of unit u in permutation q is
// v(q, pos) - v(q, pos - 1), exact in fp64 (both are fp32 values); the P of them are added in ascending q in fp64 and
// the mean is rounded to fp32 once.  A place outside 1..U (never produced by the host side) gives NaN, not a read
// outside v.
__global__ __launch_bounds__(PERTURB_THREADS) void perturb_shapley_kernel(const float* __restrict__ v, const float* __restrict__ v_empty,
                                                                          const float* __restrict__ v_full, const int* __restrict__ pos,
                                                                          float* __restrict__ phi, int B, int U, int P) {
    const unsigned idx = blockIdx.x * PERTURB_THREADS + threadIdx.x;
    if (idx >= (unsigned)B * (unsigned)U) return;
    const int u = idx / (unsigned)B, b = idx % (unsigned)B;
    double sum = 0.0;
    bool bad = false;
    for (int q = 0; q < P; ++q) {
        const int p = pos[(size_t)q * U + u];
        if (p < 1 || p > U) { bad = true; continue; }
        const float* vq = v + (size_t)q * (size_t)(U - 1) * (size_t)B;       // (only read when U > 1: 1 < p or p < U)
        const float hi = p == U ? v_full[b] : vq[(size_t)(p - 1) * B + b];
        const float lo = p == 1 ? v_empty[b] : vq[(size_t)(p - 2) * B + b];
        sum += (double)hi - (double)lo;
    }
    phi[(size_t)b * U + u] = bad ? __builtin_nanf("") : (float)(sum / (double)P);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int flat_grid(size_t work) {
    size_t g = (work + PERTURB_THREADS - 1) / PERTURB_THREADS;
    return (int)(g < 1 ? 1 : (g > (size_t)PERTURB_MAX_GRID ? (size_t)PERTURB_MAX_GRID : g));
}

}  // namespace

extern "C" {

int mm_perturb_expand(const float* x, const float* base, int base_rows, const int* masks, float* out, int B, int kind,
                      int n0, int n1, int n2, int n3, int size, int U, int m0, int m, hipStream_t st) {
    MM_REQUIRE(x && masks && out, "perturb_expand: null x / masks / out");
    MM_REQUIRE(kind >= 0 && kind <= 2, "perturb_expand: kind=%d (0 rows, 1 windows, 2 blocks)", kind);
    MM_REQUIRE(B > 0 && n0 > 0 && n1 > 0 && size >= 1, "perturb_expand: B=%d n0=%d n1=%d size=%d", B, n0, n1, size);
    MM_REQUIRE(kind == 2 ? (n2 > 0 && n3 > 0) : (n2 == 1 && n3 == 1),
               "perturb_expand: n2=%d n3=%d (positive for blocks, 1 otherwise)", n2, n3);
    const int64_t inner = (int64_t)n0 * n1 * n2 * n3;
    MM_REQUIRE(inner <= (1ll << 31) - 1 && (int64_t)B * inner <= (1ll << 31) - 1,
               "perturb_expand: B=%d samples of %lld values (the batch must stay below 2^31 elements)", B, (long long)inner);
    const int64_t gd = ((int64_t)n1 + size - 1) / size, gh = ((int64_t)n2 + size - 1) / size, gw = ((int64_t)n3 + size - 1) / size;
    const int64_t units = kind == 0 ? n0 : (kind == 1 ? gd : gd * gh * gw);
    MM_REQUIRE(U == units, "perturb_expand: U=%d but kind %d of (%d, %d, %d, %d) with size %d has %lld units", U, kind, n0, n1,
               n2, n3, size, (long long)units);
    MM_REQUIRE(m0 >= 0 && m >= 1 && m <= 65535 && (int64_t)m0 + m <= (1ll << 31) - 1, "perturb_expand: masks [%d, %d + %d)", m0, m0, m);
    MM_REQUIRE((base == nullptr) == (base_rows == 0) && (base_rows == 0 || base_rows == 1 || base_rows == B),
               "perturb_expand: base_rows=%d (0 with a null baseline, 1 = one sample for all, or B=%d)", base_rows, B);
    const unsigned n = (unsigned)((int64_t)B * inner);
    const int last = kind == 2 ? n3 : n1;
    const bool vec = last % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(base);
    const bool one_unit = kind == 0 || size % 4 == 0;
    const int* mk = masks + (size_t)m0 * (size_t)U;
    PerturbGeom g{kind, (unsigned)n1, (unsigned)n2, (unsigned)n3, (unsigned)size, (unsigned)gh, (unsigned)gw};
    const dim3 grid(flat_grid(vec ? n / 4 : n), m), thr(PERTURB_THREADS);
    if (vec && one_unit)
        hipLaunchKernelGGL((perturb_expand_kernel<true, true>), grid, thr, 0, st, x, base, mk, out, n, (unsigned)inner, base_rows, U, g);
    else if (vec)
        hipLaunchKernelGGL((perturb_expand_kernel<true, false>), grid, thr, 0, st, x, base, mk, out, n, (unsigned)inner, base_rows, U, g);
    else
        hipLaunchKernelGGL((perturb_expand_kernel<false, false>), grid, thr, 0, st, x, base, mk, out, n, (unsigned)inner, base_rows, U, g);
    return mm_check_launch("perturb_expand");
}

int mm_perturb_pair_scores(const float* z, const float* z_other, float* v, int B, int m, int N, hipStream_t st) {
    MM_REQUIRE(z && z_other && v, "perturb_pair_scores: null z / z_other / v");
    MM_REQUIRE(B > 0 && m > 0 && N > 0 && N <= (1 << 20) && (int64_t)B * m <= (1ll << 31) - 1, "perturb_pair_scores: B=%d m=%d N=%d", B, m, N);
    hipLaunchKernelGGL(perturb_pair_scores_kernel, dim3((unsigned)((int64_t)B * m)), dim3(64), 0, st, z, z_other, v, B, N);
    return mm_check_launch("perturb_pair_scores");
}

int mm_perturb_shapley(const float* v, const float* v_empty, const float* v_full, const int* pos, float* phi, int B, int U,
                       int P, hipStream_t st) {
    MM_REQUIRE(v_empty && v_full && pos && phi, "perturb_shapley: null v_empty / v_full / pos / phi");
    MM_REQUIRE(B > 0 && U > 0 && P > 0 && (int64_t)B * U <= (1ll << 31) - 1 && (int64_t)P * U <= (1ll << 31) - 1,
               "perturb_shapley: B=%d U=%d P=%d", B, U, P);
    MM_REQUIRE(v || U == 1, "perturb_shapley: null v with U=%d (only a single unit has no intermediate coalition)", U);
    const unsigned work = (unsigned)((int64_t)B * U);
    hipLaunchKernelGGL(perturb_shapley_kernel, dim3((work + PERTURB_THREADS - 1) / PERTURB_THREADS), dim3(PERTURB_THREADS), 0, st,
                       v, v_empty, v_full, pos, phi, B, U, P);
    return mm_check_launch("perturb_shapley");
}

}  // extern "C"
