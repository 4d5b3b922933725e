// GATv2 graph attention (Brody et al. 2022) over ONE static graph shared by every sample of the batch: the layer
// of GNNConnectivityEncoder (EEG_CODE/enhanced_models_v4.py:292-413).  The reference walks the batch one sample per
// call; here a layer is one launch with a workgroup per (sample, head).
//
//   e[i <- j]  = sum_c att[h][c] * leaky_relu(xl[j][h][c] + xr[i][h][c])
//   alpha      = softmax over the incoming edges of i  (* dropout keep / (1 - p), not renormalised)
//   out[i][h]  = act(sum_j alpha * xl[j][h] + bias[h])
//
// fp32 throughout; this is VALU / latency work (N <= 128 nodes, C <= 64 channels per head), no MFMA.  The graph
// comes in as CSR by target (rowptr, col = source) and, for the backward, a CSC view of the same edges (colptr,
// row = target, perm = CSR position), so that every sum - over the sources of a target, the targets of a source,
// nodes and batch - is formed in a fixed order without atomics: two runs give the same bits.
//
// Workgroup = 4 waves; the (sample, head) slice of xl sits in LDS with rows padded to C + 1 words (score phase:
// one lane per edge, every lane walks the channels of its own source row - the odd stride spreads the rows over the
// banks).  A wave owns one target at a time:
//   score phase      lane = edge           e, running max / sum through wave reductions
//   aggregate phase  lane = (group, c)     64 / C groups split the edges of a 64-edge chunk, rows read contiguously
// LDS: N (C + 1) + C + 4 x 64 x 4 words  <= 128 x 65 x 4 + 256 + 4096 B = 37.6 KB.
//
// Edge features (template parameter DP > 0, the mm_gatv2_edge_* entry points): the score becomes
//   e[i <- j]  = sum_c att[h][c] * leaky_relu((xl[j][h][c] + xr[i][h][c]) + sum_d We[h][c][d] * ea[e][d])
// with ea (B | 1, E', D) the raw attributes in CSR order (D <= 8; DP = D rounded up to 1, 2, 4 or 8, the tail zero) and
// We = lin_edge.weight.  The head's We slice [C][DP] sits in LDS in front of xs (<= 2 KB; every lane of the score loop
// reads the same word: a broadcast), the D attributes of a lane's edge in registers: the projection happens inside
// the score loop, a (B, E', H C) image is never formed.  z is (xl + xr) + edge term in that order, so We = 0 gives
// the bits of the plain kernel.  The backward also stages the attributes of a 64-edge chunk per wave ([64][DP]).
#include "common.h"

namespace {

constexpr int GAT_WAVES = 4;

struct GatArgs {
    const float* xl; const float* xr; int ld;
    const float* att; const float* bias;
    const int* rowptr; const int* col;
    const int* colptr; const int* row; const int* perm;
    float* out; float* pre; float* alpha;                  // forward outputs (alpha: read by the backward)
    const float* dout; float* dxl; float* dxr;             // backward
    float* ds; float* dz; float* part;                     // backward workspaces
    int B, N, H, C, E; float slope; int act;
    uint32_t thresh, seed; float inv_keep; const uint32_t* epoch;
    // edge variant only (DP > 0)
    const float* we; const float* ea; size_t ea_bs; int D;  // We [H*C][D]; ea [B | 1][E][D], batch stride ea_bs (0: shared)
    float* dea; float* pwe;                                // backward: per-head d ea [B][H][E][D] (nullable), d We partials [B][H*C][D]
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the 64 / C lane groups (lanes c, c + C, c + 2 C, ...): every lane ends with the total, fixed pairing
template <int C> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = C; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int C> __device__ __forceinline__ void load_slice(const GatArgs& a, int b, int h, float* xs, float* atts) {
    constexpr int LDC = C + 1;
    for (int idx = threadIdx.x; idx < a.N * C; idx += blockDim.x) {
        const int n = idx / C, c = idx % C;
        xs[n * LDC + c] = a.xl[((size_t)b * a.N + n) * a.ld + h * C + c];
    }
    if (threadIdx.x < C) atts[threadIdx.x] = a.att[h * C + threadIdx.x];
}

// ---- edge variant helpers: We slice [C][DP] at the start of the dynamic LDS (16-byte aligned rows)
template <int C, int DP> __device__ __forceinline__ void load_we(const GatArgs& a, int h, float* wes) {
    for (int idx = threadIdx.x; idx < C * DP; idx += blockDim.x) {
        const int k = idx / DP, d = idx % DP;
        wes[idx] = d < a.D ? a.we[(size_t)(h * C + k) * a.D + d] : 0.f;
    }
}

template <int DP> __device__ __forceinline__ void load_row(const float* __restrict__ p, float (&w)[DP]) {
    if constexpr (DP == 1) {
        w[0] = p[0];
    } else if constexpr (DP == 2) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < DP; q += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + q);
            w[q] = v.x; w[q + 1] = v.y; w[q + 2] = v.z; w[q + 3] = v.w;
        }
    }
}

// the D raw attributes of CSR edge e of sample b (global), zero beyond D
template <int DP> __device__ __forceinline__ void load_ea(const GatArgs& a, int b, int e, float (&ev)[DP]) {
    const float* p = a.ea + (size_t)b * a.ea_bs + (size_t)e * a.D;
#pragma unroll
    for (int d = 0; d < DP; ++d) ev[d] = d < a.D ? p[d] : 0.f;
}

template <int DP> __device__ __forceinline__ float edge_term(const float (&w)[DP], const float (&ev)[DP]) {
    float t = w[0] * ev[0];
#pragma unroll
    for (int d = 1; d < DP; ++d) t += w[d] * ev[d];
    return t;
}

template <int C, int DP = 0>
__global__ __launch_bounds__(64 * GAT_WAVES) void gatv2_fwd_kernel(GatArgs a) {
    constexpr int LDC = C + 1, G = 64 / C;
    extern __shared__ float smem[];
    float* xs = smem + C * DP;                             // [N][C + 1]  (edge variant: We slice [C][DP] in front)
    float* atts = xs + a.N * LDC;                          // [C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* xri = atts + C + wave * 256;                    // per wave: xr row of the target [64]
    float* wa = xri + 64;                                  //           alpha * keep of a chunk [64]
    int* wj = reinterpret_cast<int*>(wa + 64);             //           source of a chunk [64]
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
    const uint32_t seed = mm_eff_seed(a.seed, a.epoch);
    load_slice<C>(a, b, h, xs, atts);
    if constexpr (DP > 0) load_we<C, DP>(a, h, smem);
    __syncthreads();
    const int g = lane / C, c = lane % C, HC = a.H * C;
    float* alpha = a.alpha + (size_t)bh * a.E;
    for (int i = wave; i < a.N; i += GAT_WAVES) {
        const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
        const size_t node = (size_t)b * a.N + i;
        if (lane < C) xri[lane] = a.xr[node * a.ld + h * C + lane];
        wave_sync();
        float m = -INFINITY;
        for (int e = e0 + lane; e < e1; e += 64) {
            const float* xj = xs + a.col[e] * LDC;
            float s = 0.f;
            if constexpr (DP > 0) {
                float ev[DP], w[DP];
                load_ea<DP>(a, b, e, ev);
#pragma unroll 4
                for (int k = 0; k < C; ++k) {
                    load_row<DP>(smem + k * DP, w);
                    const float z = (xj[k] + xri[k]) + edge_term<DP>(w, ev);
                    s += atts[k] * (z > 0.f ? z : a.slope * z);
                }
            } else {
#pragma unroll 8
                for (int k = 0; k < C; ++k) {
                    const float z = xj[k] + xri[k];
                    s += atts[k] * (z > 0.f ? z : a.slope * z);
                }
            }
            alpha[e] = s;
            m = fmaxf(m, s);
        }
        m = wave_max(m);
        float sum = 0.f;
        for (int e = e0 + lane; e < e1; e += 64) sum += expf(alpha[e] - m);
        sum = wave_sum(sum);
        const float inv = 1.f / sum;
        float acc = 0.f;
        for (int base = e0; base < e1; base += 64) {
            const int e = base + lane;
            if (e < e1) {
                const float p = expf(alpha[e] - m) * inv;
                alpha[e] = p;
                const float keep = a.thresh ? dropout_scale(seed, (uint32_t)((size_t)bh * a.E + e), a.thresh, a.inv_keep) : 1.f;
                wa[lane] = p * keep;
                wj[lane] = a.col[e];
            }
            wave_sync();
            const int cnt = e1 - base < 64 ? e1 - base : 64;
            for (int t = g; t < cnt; t += G) acc += wa[t] * xs[wj[t] * LDC + c];
            wave_sync();
        }
        acc = group_sum<C>(acc);
        if (lane < C) {
            float v = acc + (a.bias ? a.bias[h * C + c] : 0.f);
            const size_t o = node * HC + h * C + c;
            if (a.pre) a.pre[o] = v;
            a.out[o] = apply_act(v, a.act);
        }
    }
}

// backward, one launch: phase 1 walks the targets (d alpha -> d score, d xr, d att, d bias), phase 2 the sources
// (d xl).  d score of every edge crosses from phase 1 to phase 2 through `ds` (global, the workgroup's own slice).
//
// Edge variant: LDS starts with the We slice [C][DP] and a per-wave stage of a chunk's attributes [64][DP]; a lane of
// the aggregate loop keeps the We row of its channel in registers.  d We: per-lane sums over the edges, group_sum,
// block combine through the (then idle) stages, one partial per (sample, head) to `pwe`.  d ea crosses heads, which
// are separate workgroups: lane = edge forms sum_c d z[e][c] We[c][d] for its head and writes it to `dea`
// [B][H][E][D]; gatv2_edge_dea_kernel adds the heads in order.
template <int C, int DP = 0>
__global__ __launch_bounds__(64 * GAT_WAVES) void gatv2_bwd_kernel(GatArgs a) {
    constexpr int LDC = C + 1, G = 64 / C;
    extern __shared__ float smem[];
    float* xs = smem + (C + 64 * GAT_WAVES) * DP;
    float* atts = xs + a.N * LDC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* red = atts + C;                                 // [GAT_WAVES][2][C] block combine of d att / d bias (<= 512 words)
    float* xri = red + 512 + wave * 256;
    float* dpi = xri + 64;                                 // d pre-activation row of the target [64]
    float* wa = dpi + 64;
    int* wj = reinterpret_cast<int*>(wa + 64);
    const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
    const uint32_t seed = mm_eff_seed(a.seed, a.epoch);
    load_slice<C>(a, b, h, xs, atts);
    if constexpr (DP > 0) load_we<C, DP>(a, h, smem);
    __syncthreads();
    const int g = lane / C, c = lane % C, HC = a.H * C;
    [[maybe_unused]] float* wea = smem + (C + 64 * wave) * DP;              // edge variant, per wave: attributes of a chunk [64][DP]
    [[maybe_unused]] float wc[DP > 0 ? DP : 1], dwe[DP > 0 ? DP : 1];       // We row of channel c; d We[c][:] / att[c] of this lane's edges
    if constexpr (DP > 0) {
        load_row<DP>(smem + c * DP, wc);
#pragma unroll
        for (int d = 0; d < DP; ++d) dwe[d] = 0.f;
    }
    const float* alpha = a.alpha + (size_t)bh * a.E;
    float* ds = a.ds + (size_t)bh * a.E;
    const float* dzsrc = a.act != MM_ACT_NONE ? a.dz : a.dout;
    float datt = 0.f, dbias = 0.f;
    for (int i = wave; i < a.N; i += GAT_WAVES) {
        const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
        const size_t node = (size_t)b * a.N + i;
        if (lane < C) {
            xri[lane] = a.xr[node * a.ld + h * C + lane];
            const size_t o = node * HC + h * C + lane;
            float d = a.dout[o];
            if (a.act != MM_ACT_NONE) {
                d *= act_grad(a.pre[o], a.act);
                a.dz[o] = d;
            }
            dpi[lane] = d;
            dbias += d;
        }
        wave_sync();
        // d (alpha * keep) of every edge, and S = sum alpha * d alpha
        float S = 0.f;
        for (int e = e0 + lane; e < e1; e += 64) {
            const float* xj = xs + a.col[e] * LDC;
            float s = 0.f;
#pragma unroll 8
            for (int k = 0; k < C; ++k) s += dpi[k] * xj[k];
            if (a.thresh) s *= dropout_scale(seed, (uint32_t)((size_t)bh * a.E + e), a.thresh, a.inv_keep);
            ds[e] = s;
            S += alpha[e] * s;
        }
        S = wave_sum(S);
        float dxr = 0.f;
        for (int base = e0; base < e1; base += 64) {
            const int e = base + lane;
            if (e < e1) {
                const float d = alpha[e] * (ds[e] - S);
                ds[e] = d;
                wa[lane] = d;
                wj[lane] = a.col[e];
                if constexpr (DP > 0) {
                    float ev[DP];
                    load_ea<DP>(a, b, e, ev);
#pragma unroll
                    for (int q = 0; q < DP; ++q) wea[lane * DP + q] = ev[q];
                    if (a.dea) {                           // d ea[e][:] of this head = sum_c d z[e][c] We[c][:]
                        const float* xj = xs + a.col[e] * LDC;
                        float de[DP], w[DP];
#pragma unroll
                        for (int q = 0; q < DP; ++q) de[q] = 0.f;
#pragma unroll 4
                        for (int k = 0; k < C; ++k) {
                            load_row<DP>(smem + k * DP, w);
                            const float z = (xj[k] + xri[k]) + edge_term<DP>(w, ev);
                            const float gz = d * atts[k] * (z > 0.f ? 1.f : a.slope);
#pragma unroll
                            for (int q = 0; q < DP; ++q) de[q] += gz * w[q];
                        }
                        float* o = a.dea + ((size_t)bh * a.E + e) * a.D;
#pragma unroll
                        for (int q = 0; q < DP; ++q)
                            if (q < a.D) o[q] = de[q];
                    }
                }
            }
            wave_sync();
            const int cnt = e1 - base < 64 ? e1 - base : 64;
            const float xr_c = xri[c];
            for (int t = g; t < cnt; t += G) {
                float z = xs[wj[t] * LDC + c] + xr_c;
                if constexpr (DP > 0) {
                    float ev[DP];
                    load_row<DP>(wea + t * DP, ev);
                    z += edge_term<DP>(wc, ev);
                    const float gz = wa[t] * (z > 0.f ? 1.f : a.slope);
#pragma unroll
                    for (int q = 0; q < DP; ++q) dwe[q] += gz * ev[q];
                }
                dxr += wa[t] * (z > 0.f ? 1.f : a.slope);
                datt += wa[t] * (z > 0.f ? z : a.slope * z);
            }
            wave_sync();
        }
        dxr = group_sum<C>(dxr);
        if (lane < C) a.dxr[node * a.ld + h * C + c] = dxr * atts[c];
    }
    datt = group_sum<C>(datt);
    if (lane < C) {
        red[(wave * 2 + 0) * C + c] = datt;
        red[(wave * 2 + 1) * C + c] = dbias;
    }
    if constexpr (DP > 0) {                                // the wave's stage is idle now: its d We partial [C][DP]
#pragma unroll
        for (int q = 0; q < DP; ++q) {
            const float v = group_sum<C>(dwe[q]);
            if (lane < C) wea[c * DP + q] = v;
        }
    }
    __threadfence_block();
    __syncthreads();
    if constexpr (DP > 0) {
        for (int idx = threadIdx.x; idx < C * DP; idx += blockDim.x) {
            const int cc = idx / DP, q = idx % DP;
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < GAT_WAVES; ++w) s += smem[(C + 64 * w) * DP + idx];
            if (q < a.D) a.pwe[((size_t)b * HC + h * C + cc) * a.D + q] = s * atts[cc];
        }
    }
    if (threadIdx.x < 2 * C) {
        const int k = threadIdx.x / C, cc = threadIdx.x % C;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < GAT_WAVES; ++w) s += red[(w * 2 + k) * C + cc];
        a.part[((size_t)b * 2 + k) * HC + h * C + cc] = s;
    }
    // phase 2: d xl[j] = sum over the edges j -> i of alpha keep d pre[i] + d score att leaky'(xl[j] + xr[i])
    for (int j = wave; j < a.N; j += GAT_WAVES) {
        const int t0 = a.colptr[j], t1 = a.colptr[j + 1];
        const float xl_c = xs[j * LDC + c], att_c = atts[c];
        float acc = 0.f;
        for (int t = t0 + g; t < t1; t += G) {
            const int i = a.row[t], e = a.perm[t];
            const size_t node = (size_t)b * a.N + i;
            float am = alpha[e];
            if (a.thresh) am *= dropout_scale(seed, (uint32_t)((size_t)bh * a.E + e), a.thresh, a.inv_keep);
            float z = xl_c + a.xr[node * a.ld + h * C + c];
            if constexpr (DP > 0) {
                float ev[DP];
                load_ea<DP>(a, b, e, ev);
                z += edge_term<DP>(wc, ev);
            }
            acc += am * dzsrc[node * HC + h * C + c] + ds[e] * att_c * (z > 0.f ? 1.f : a.slope);
        }
        acc = group_sum<C>(acc);
        if (lane < C) a.dxl[((size_t)b * a.N + j) * a.ld + h * C + c] = acc;
    }
}

// d att / d bias += sum over the batch of the per-(sample, head) partial sums, in batch order
__global__ void gatv2_param_grads_kernel(const float* __restrict__ part, float* __restrict__ datt,
                                         float* __restrict__ dbias, int B, int HC) {
    const int k = threadIdx.x;
    if (k >= HC) return;
    float sa = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        sa += part[((size_t)b * 2 + 0) * HC + k];
        sb += part[((size_t)b * 2 + 1) * HC + k];
    }
    if (datt) datt[k] += sa;
    if (dbias) dbias[k] += sb;
}

// d lin_edge.weight += sum over the batch of the per-(sample, head) partials [B][H*C*D], in batch order
__global__ void gatv2_edge_wgrad_kernel(const float* __restrict__ part, float* __restrict__ dwe, int B, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[(size_t)b * n + k];
    dwe[k] += s;
}

// d ea (CSR order) = the per-head partials [B][H][E*D] added in head order; shared attributes (Bo = 1): over the
// batch too, sample by sample
__global__ void gatv2_edge_dea_kernel(const float* __restrict__ part, float* __restrict__ dea, int B, int Bo, int H, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int bo = blockIdx.y;
    float s = 0.f;
    for (int b = (Bo == 1 ? 0 : bo); b < (Bo == 1 ? B : bo + 1); ++b)
        for (int h = 0; h < H; ++h) s += part[((size_t)b * H + h) * n + k];
    dea[(size_t)bo * n + k] = s;
}

// listed attributes [Bo][El][D] -> CSR order [Bo][E][D]; the appended self-loop of node i (the last edge of row i)
// gets the mean of the listed edges into i (0 without any) or a constant.  One thread per (sample, node, d).
__global__ void gatv2_edge_pack_kernel(const float* __restrict__ listed, const int* __restrict__ eid,
                                       const int* __restrict__ rowptr, const int* __restrict__ indeg,
                                       float* __restrict__ csr, int N, int El, int E, int D, int fill_mean, float fill) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * D) return;
    const int i = idx / D, d = idx % D;
    const float* src = listed + (size_t)blockIdx.y * El * D;
    float* dst = csr + (size_t)blockIdx.y * E * D;
    float s = 0.f;
    for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int l = eid[e];
        if (l >= 0) {
            const float v = src[(size_t)l * D + d];
            dst[(size_t)e * D + d] = v;
            s += v;
        } else {
            dst[(size_t)e * D + d] = fill_mean ? (indeg[i] > 0 ? s / (float)indeg[i] : 0.f) : fill;
        }
    }
}

// d listed[l] = d csr[pos(l)] + d csr[loop of l's target] / indeg  (0 for a dropped listed self-loop): a gather
__global__ void gatv2_edge_pack_bwd_kernel(const float* __restrict__ dcsr, const int* __restrict__ pos,
                                           const int* __restrict__ tgt, const int* __restrict__ rowptr,
                                           const int* __restrict__ indeg, float* __restrict__ dlisted, int El, int E,
                                           int D, int fill_mean) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= El * D) return;
    const int l = idx / D, d = idx % D;
    const float* src = dcsr + (size_t)blockIdx.y * E * D;
    const int e = pos[l];
    float v = 0.f;
    if (e >= 0) {
        v = src[(size_t)e * D + d];
        const int i = tgt[l];
        if (fill_mean) v += src[(size_t)(rowptr[i + 1] - 1) * D + d] / (float)indeg[i];
    }
    dlisted[(size_t)blockIdx.y * El * D + idx] = v;
}

// the fields every entry point fills; the callers add their own outputs and workspaces
GatArgs gat_args(const float* xl, const float* xr, int ld, const float* att, const float* w_edge, const float* edge_attr,
                 int ea_batched, const int* rowptr, const int* col, int B, int N, int H, int C, int E, int D, float slope,
                 int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch) {
    GatArgs a{};
    a.xl = xl; a.xr = xr; a.ld = ld; a.att = att; a.rowptr = rowptr; a.col = col;
    a.B = B; a.N = N; a.H = H; a.C = C; a.E = E; a.slope = slope; a.act = act;
    const DropH d = mm_drop(drop_p);
    a.thresh = d.thresh; a.seed = seed; a.inv_keep = d.inv_keep; a.epoch = seed_epoch;
    a.we = w_edge; a.ea = edge_attr; a.ea_bs = ea_batched ? (size_t)E * D : 0; a.D = D;
    return a;
}

// The one place the dynamic LDS of the two kernels is priced (in floats).  It follows their pointer arithmetic:
//   edge variant, in front:  forward  xs = smem + C * DP                       the We slice
//                            backward xs = smem + (C + 64 * GAT_WAVES) * DP    the We slice + every wave's attribute stage
//   then xs [N][C + 1], atts [C], backward only: red (512), and 256 words per wave (the 512 + GAT_WAVES * 256 tail)
constexpr size_t gat_lds_floats(int N, int C, int DP, bool bwd) {
    return (size_t)(bwd ? C + 64 * GAT_WAVES : C) * DP + (size_t)N * (C + 1) + C + (bwd ? 512 : 0) + GAT_WAVES * 256;
}

using GatKernel = void (*)(GatArgs);

// the one (C, DP) dispatch over the 3 x 5 instantiations of either kernel
template <bool BWD, int C, int DP> GatKernel gat_kernel_of() {
    if constexpr (BWD) return gatv2_bwd_kernel<C, DP>;
    else return gatv2_fwd_kernel<C, DP>;
}

template <bool BWD, int DP> GatKernel gat_kernel_c(int C) {
    return C == 16 ? gat_kernel_of<BWD, 16, DP>() : C == 32 ? gat_kernel_of<BWD, 32, DP>() : gat_kernel_of<BWD, 64, DP>();
}

template <bool BWD> GatKernel gat_kernel(int C, int DP) {
    switch (DP) {
        case 0: return gat_kernel_c<BWD, 0>(C);
        case 1: return gat_kernel_c<BWD, 1>(C);
        case 2: return gat_kernel_c<BWD, 2>(C);
        case 4: return gat_kernel_c<BWD, 4>(C);
        default: return gat_kernel_c<BWD, 8>(C);
    }
}

// The shared path of the four entry points; w_edge == nullptr, D = 0: the plain layer (DP = D rounded up to 1, 2, 4 or 8).
// Backward: the kernel, then the batch sums of the parameter gradients and, where asked for, the head sums of d ea.
int gat_run(const char* who, const GatArgs& a, float drop_p, bool bwd, hipStream_t st, float* datt = nullptr,
            float* dbias = nullptr, float* dw_edge = nullptr, float* dedge_attr = nullptr) {
    const int B = a.B, N = a.N, H = a.H, C = a.C, E = a.E, D = a.D, HC = H * C;
    MM_REQUIRE(B > 0 && H > 0, "%s: B=%d H=%d", who, B, H);
    MM_REQUIRE(N >= 1 && N <= 128, "%s: N=%d outside [1, 128]", who, N);
    MM_REQUIRE(C == 16 || C == 32 || C == 64, "%s: C=%d is not 16, 32 or 64", who, C);
    MM_REQUIRE(HC <= 256, "%s: H*C=%d above 256", who, HC);
    MM_REQUIRE(E >= N, "%s: E=%d edges for N=%d nodes (every node carries a self-loop)", who, E, N);
    MM_REQUIRE((unsigned long long)B * H * (unsigned long long)E < (1ull << 32), "%s: B*H*E does not fit the 32-bit mask index", who);
    MM_REQUIRE(a.ld >= HC, "%s: ld=%d below H*C=%d", who, a.ld, HC);
    MM_REQUIRE(a.act >= MM_ACT_NONE && a.act <= MM_ACT_SIGMOID, "%s: act=%d", who, a.act);
    MM_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%f", who, (double)drop_p);
    MM_REQUIRE(!a.we || (D >= 1 && D <= 8), "%s: D=%d outside [1, 8]", who, D);
    MM_REQUIRE(!bwd || a.act == MM_ACT_NONE || (a.pre && a.dz), "%s: an activation epilogue needs pre and dz_ws", who);
    MM_REQUIRE(!dedge_attr || a.dea, "%s: dedge_attr needs epart_ws", who);
    const int DP = D <= 2 ? D : D <= 4 ? 4 : 8, Bo = a.ea_bs ? B : 1;
    const GatKernel k = !bwd ? gat_kernel<false>(C, DP) : gat_kernel<true>(C, DP);
    hipLaunchKernelGGL(k, dim3(B * H), dim3(64 * GAT_WAVES), gat_lds_floats(N, C, DP, bwd) * sizeof(float), st, a);
    if (datt || dbias) hipLaunchKernelGGL(gatv2_param_grads_kernel, dim3(1), dim3(256), 0, st, a.part, datt, dbias, B, HC);
    if (dw_edge) hipLaunchKernelGGL(gatv2_edge_wgrad_kernel, dim3((HC * D + 255) / 256), dim3(256), 0, st, a.pwe, dw_edge, B, HC * D);
    if (dedge_attr)
        hipLaunchKernelGGL(gatv2_edge_dea_kernel, dim3((E * D + 255) / 256, Bo), dim3(256), 0, st, a.dea, dedge_attr, B, Bo, H, E * D);
    return mm_check_launch(who);
}

}  // namespace

extern "C" {

int mm_gatv2_fwd(const float* xl, const float* xr, int ld, const float* att, const float* bias, const int* rowptr,
                 const int* col, float* out, float* pre, float* alpha, int B, int N, int H, int C, int E,
                 float slope, int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(xl && xr && att && rowptr && col && out && alpha, "gatv2_fwd: null pointer");
    GatArgs a = gat_args(xl, xr, ld, att, nullptr, nullptr, 0, rowptr, col, B, N, H, C, E, 0, slope, act, drop_p, seed, seed_epoch);
    a.bias = bias; a.out = out; a.pre = pre; a.alpha = alpha;
    return gat_run("gatv2_fwd", a, drop_p, false, st);
}

int mm_gatv2_edge_fwd(const float* xl, const float* xr, int ld, const float* att, const float* bias,
                      const float* w_edge, const float* edge_attr, int ea_batched, const int* rowptr, const int* col,
                      float* out, float* pre, float* alpha, int B, int N, int H, int C, int E, int D, float slope,
                      int act, float drop_p, uint32_t seed, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(xl && xr && att && w_edge && edge_attr && rowptr && col && out && alpha, "gatv2_edge_fwd: null pointer");
    GatArgs a = gat_args(xl, xr, ld, att, w_edge, edge_attr, ea_batched, rowptr, col, B, N, H, C, E, D, slope, act, drop_p, seed,
                         seed_epoch);
    a.bias = bias; a.out = out; a.pre = pre; a.alpha = alpha;
    return gat_run("gatv2_edge_fwd", a, drop_p, false, st);
}

int mm_gatv2_bwd(const float* dout, const float* pre, const float* xl, const float* xr, int ld, const float* att,
                 const float* alpha, const int* rowptr, const int* col, const int* colptr, const int* row,
                 const int* perm, float* dxl, float* dxr, float* datt, float* dbias, float* ds_ws, float* dz_ws,
                 float* part_ws, int B, int N, int H, int C, int E, float slope, int act, float drop_p,
                 uint32_t seed, const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(dout && xl && xr && att && alpha && rowptr && col && colptr && row && perm && dxl && dxr && ds_ws && part_ws,
               "gatv2_bwd: null pointer");
    GatArgs a = gat_args(xl, xr, ld, att, nullptr, nullptr, 0, rowptr, col, B, N, H, C, E, 0, slope, act, drop_p, seed, seed_epoch);
    a.colptr = colptr; a.row = row; a.perm = perm; a.pre = const_cast<float*>(pre); a.alpha = const_cast<float*>(alpha);
    a.dout = dout; a.dxl = dxl; a.dxr = dxr; a.ds = ds_ws; a.dz = dz_ws; a.part = part_ws;
    return gat_run("gatv2_bwd", a, drop_p, true, st, datt, dbias);
}

int mm_gatv2_edge_bwd(const float* dout, const float* pre, const float* xl, const float* xr, int ld, const float* att,
                      const float* w_edge, const float* edge_attr, int ea_batched, const float* alpha,
                      const int* rowptr, const int* col, const int* colptr, const int* row, const int* perm,
                      float* dxl, float* dxr, float* datt, float* dbias, float* dw_edge, float* dedge_attr,
                      float* ds_ws, float* dz_ws, float* part_ws, float* wpart_ws, float* epart_ws, int B, int N,
                      int H, int C, int E, int D, float slope, int act, float drop_p, uint32_t seed,
                      const uint32_t* seed_epoch, hipStream_t st) {
    MM_REQUIRE(dout && xl && xr && att && w_edge && edge_attr && alpha && rowptr && col && colptr && row && perm && dxl &&
               dxr && ds_ws && part_ws && wpart_ws, "gatv2_edge_bwd: null pointer");
    GatArgs a = gat_args(xl, xr, ld, att, w_edge, edge_attr, ea_batched, rowptr, col, B, N, H, C, E, D, slope, act, drop_p, seed,
                         seed_epoch);
    a.colptr = colptr; a.row = row; a.perm = perm; a.pre = const_cast<float*>(pre); a.alpha = const_cast<float*>(alpha);
    a.dout = dout; a.dxl = dxl; a.dxr = dxr; a.ds = ds_ws; a.dz = dz_ws; a.part = part_ws;
    a.dea = dedge_attr ? epart_ws : nullptr; a.pwe = wpart_ws;
    return gat_run("gatv2_edge_bwd", a, drop_p, true, st, datt, dbias, dw_edge, dedge_attr);
}

int mm_gatv2_edge_pack(const float* listed, const int* eid, const int* rowptr, const int* indeg, float* csr, int Bo,
                       int N, int El, int E, int D, int fill_mean, float fill_value, hipStream_t st) {
    MM_REQUIRE(eid && rowptr && indeg && csr && (listed || El == 0), "gatv2_edge_pack: null pointer");
    MM_REQUIRE(Bo >= 1 && Bo <= 65535, "gatv2_edge_pack: B=%d outside [1, 65535]", Bo);
    MM_REQUIRE(N >= 1 && N <= 128, "gatv2_edge_pack: N=%d outside [1, 128]", N);
    MM_REQUIRE(D >= 1 && D <= 8, "gatv2_edge_pack: D=%d outside [1, 8]", D);
    MM_REQUIRE(El >= 0 && E >= N && E <= El + N, "gatv2_edge_pack: E=%d CSR edges for %d listed edges and N=%d nodes", E, El, N);
    hipLaunchKernelGGL(gatv2_edge_pack_kernel, dim3((N * D + 255) / 256, Bo), dim3(256), 0, st, listed, eid, rowptr, indeg,
                       csr, N, El, E, D, fill_mean, fill_value);
    return mm_check_launch("gatv2_edge_pack");
}

int mm_gatv2_edge_pack_bwd(const float* dcsr, const int* pos, const int* tgt, const int* rowptr, const int* indeg,
                           float* dlisted, int Bo, int N, int El, int E, int D, int fill_mean, hipStream_t st) {
    MM_REQUIRE(dcsr && rowptr && indeg && ((pos && tgt && dlisted) || El == 0), "gatv2_edge_pack_bwd: null pointer");
    MM_REQUIRE(Bo >= 1 && Bo <= 65535, "gatv2_edge_pack_bwd: B=%d outside [1, 65535]", Bo);
    MM_REQUIRE(N >= 1 && N <= 128, "gatv2_edge_pack_bwd: N=%d outside [1, 128]", N);
    MM_REQUIRE(D >= 1 && D <= 8, "gatv2_edge_pack_bwd: D=%d outside [1, 8]", D);
    MM_REQUIRE(El >= 0 && E >= N && E <= El + N, "gatv2_edge_pack_bwd: E=%d CSR edges for %d listed edges and N=%d nodes", E, El, N);
    if (El == 0) return MM_OK;
    hipLaunchKernelGGL(gatv2_edge_pack_bwd_kernel, dim3((El * D + 255) / 256, Bo), dim3(256), 0, st, dcsr, pos, tgt, rowptr,
                       indeg, dlisted, El, E, D, fill_mean);
    return mm_check_launch("gatv2_edge_pack_bwd");
}

}  // extern "C"
