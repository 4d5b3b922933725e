// Pieces shared by the self-attention kernels: attention.hip (head_dim 32) and attention_hd.hip (head_dim 16-64):
// the transposed LDS fragment read, the dropout block hash, the half-wave exchanges and the host-side dropout
// threshold.  One definition, so that every kernel draws the same dropout mask (oracle/dropout_replica.py).
#pragma once
#include "common.h"

namespace {

constexpr int VR = 32;                   // row stride (elements) of a row-major tile read through ds_read_b64_tr_b16: 64 B, NO
                                         // padding.  The instruction is served in two groups of 32 lanes; a group reads four
                                         // rows x two 32-byte column halves, i.e. eight 8-bank windows at (16 row + 8 half)
                                         // mod 64 - all distinct.  (The 96-byte stride of round 2 put row 3 / half 0 on the
                                         // banks of row 0 / half 1: SQ_LDS_BANK_CONFLICT = 0.36 of the LDS cycles,
                                         // profiles/r03_pmc_attn.summary.txt)

// MFMA A operand of a TRANSPOSED product from a row-major LDS tile [k][32] (row stride VR): row index = lane & 31 =
// tile column, k-slots 8 (lane >> 5) + {0..7} = tile rows row0 + 8 (lane >> 5) + {0..7} (hardware transpose, as in
// the weight-gradient kernels) - no scattered 2-byte writes into a transposed copy (they were 0.4 of the LDS cycles)
__device__ __forceinline__ bf16x8 tr_frag32(const bf16* tile, int row0, int lane) {
    const int li = lane & 15, g = lane >> 4;
    const bf16* p = tile + (row0 + 8 * (g >> 1) + (li >> 2)) * VR + (g & 1) * 16 + 4 * (li & 3);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    union { s16x4 s[2]; bf16x8 v; } u;
    u.s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
    u.s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * VR));
    return u.v;
}

__device__ __forceinline__ int vperm(int key) {       // swap bits 2 and 3 of the key index
    return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1);
}

// attention-probability dropout (nn.MultiheadAttention(dropout=p)): the softmax
// row sum uses the un-dropped probabilities, only the P operand of P.V is masked.
// The mask used to cost a quarter of these kernels (hash ~9 of ~20 VALU instructions per score, its 32-bit multiply
// quarter-rate; the dkv kernel, whose registers run along the queries, could not share the per-key-pair hash of the
// other two and hashed per score).  Now ONE hash serves the 2 x 2 block (queries 2i, 2i + 1) x (keys 2j, 2j + 1): byte
// 2 (q & 1) + (key & 1) of the word decides the score (keep iff byte >= round(p * 256): p is honoured to 1/256 and
// the keep scale is 256 / (256 - t), so the mask stays unbiased for the quantised p).  Every kernel then spends one
// hash per two scores whichever way its registers run: forward / dq lanes own a query and hold the two keys of a
// block in registers r, r + 1; dkv lanes own a key and hold the two queries.  The mixer's multiply is the full-rate
// 24-bit one (v_mul_u32_u24; constants chosen on the mask statistics: keep rate to 7e-4, lag / diagonal / head
// correlations <= 0.0022, row- and column-sum variance 0.97-1.04 of binomial; oracle/dropout_replica.py is the host
// replica).  Block index = (bh * ceil(L / 2) + q / 2) * ceil(L / 2) + key / 2.
__device__ __forceinline__ uint32_t attn_block_hash(uint32_t seed, int bh, int q, int key, int L) {
    const uint32_t Lh = ((uint32_t)L + 1u) >> 1;
    uint32_t x = (((uint32_t)bh * Lh + ((uint32_t)q >> 1)) * Lh + ((uint32_t)key >> 1)) * 0x9E3779B1u + seed;
    x ^= x >> 13;
    x = __umul24(x, 0xB5297Bu);
    x ^= x >> 15;
    return x;
}
// the two scores of a block that ONE lane owns: `mine` = the lane's own index (query in forward / dq, key in dkv),
// `other` = the EVEN index of the register pair (keys 2j, 2j + 1 resp. queries 2i, 2i + 1).  along_keys: the pair runs
// along the keys (forward, dq) or along the queries (dkv).
template <bool ALONG_KEYS>
__device__ __forceinline__ void attn_keep2(uint32_t seed, int bh, int mine, int other, int L, uint32_t thresh8, bool& k0, bool& k1) {
    if (ALONG_KEYS) {
        const uint32_t x = attn_block_hash(seed, bh, mine, other, L) >> (16 * (mine & 1));
        k0 = (x & 0xFFu) >= thresh8;
        k1 = ((x >> 8) & 0xFFu) >= thresh8;
    } else {
        const uint32_t x = attn_block_hash(seed, bh, other, mine, L) >> (8 * (mine & 1));
        k0 = (x & 0xFFu) >= thresh8;
        k1 = ((x >> 16) & 0xFFu) >= thresh8;
    }
}

// exchange between the two halves of a wave (lanes l and l ^ 32) without an LDS round trip: v_permlane32_swap (gfx950)
// leaves the lower half of its first operand / the upper half of its second in both halves
__device__ __forceinline__ float xhalf_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// v_exp_f32 as is: arguments are <= 0 here and a result below 2^-126 may flush to zero (softmax
// weights); exp2f() wraps the instruction in a compare / two selects / add / ldexp for denormal
// results, i.e. 6 extra VALU instructions per score in loops that are VALU-bound.
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

}  // namespace

// 8-bit drop threshold of one byte of the block hash (0 = dropout off: p < 1/512), and the keep scale that makes the
// mask unbiased for the quantised probability t / 256
static inline uint32_t attn_thresh(float p) { return p > 0.f ? (uint32_t)((double)p * 256.0 + 0.5) : 0u; }
static inline float attn_keep_scale(uint32_t t) { return t ? 256.f / (256.f - (float)t) : 1.f; }
