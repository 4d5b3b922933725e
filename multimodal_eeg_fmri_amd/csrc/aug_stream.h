// The augmenters' random stream, device and host side: ONE definition for augment.hip and volume_augment.hip (its host
// replica is multimodal_eeg_fmri_amd/augment_stream.py; DESIGN.md 5i defines it).  Counter based, stateless on the device,
// independent of the dropout stream (mm_hash / ops._seed_state).
//
//   h(stream, idx):   x  = idx * 0x9E3779B1 + stream            (all arithmetic mod 2^32)
//                     x ^= x >> 16;  x *= 0x7FEB352D
//                     x ^= x >> 15;  x += rotl(stream, 16);  x *= 0x846CA68B
//                     x ^= x >> 16
//   (the two multiply-xorshift rounds of the "lowbias32" integer mixer; the stream word enters twice, so that two
//   streams are not index-shifted copies of each other)
//
//   stream(seed, step, rank, purpose), formed on the host in 64-bit arithmetic (mod 2^64):
//                     z  = seed * 0x9E3779B97F4A7C15 + step * 0xBF58476D1CE4E5B9 + rank * 0x94D049BB133111EB
//                          + (purpose + 1) * 0xD6E8FEB86659FD93
//                     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
//                     stream = (z ^ (z >> 32)) mod 2^32
//   purposes 0..4 are the EEG augmenter's, 5..18 the volume augmenter's, 19..25 the temporal EEG augmenter's
//   (augment_stream.PURPOSES, one table): the three are independent at equal seed and step.
//
//   every per-sample draw of sample b is h(stream_k, b):
//     decision on  iff  h < thresh(p), thresh(p) = (uint64)((double)p * 2^32) of the fp32 value p (p = 1: 2^32, always)
//     uniform integer in [0, n):  (h * n) >> 32 in 64-bit arithmetic
//     scale factor = fp32( 1 + (double)scale_range * (h * 2^-31 - 1) )   (fp64 in this order, rounded once)
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

__device__ __forceinline__ uint32_t aug_hash(uint32_t stream, uint32_t idx) {
    uint32_t x = idx * 0x9E3779B1u + stream;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x += (stream << 16) | (stream >> 16);
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t aug_uniform(uint32_t h, uint32_t n) { return (uint32_t)(((uint64_t)h * n) >> 32); }

// fp64 operations in the order above, each rounded on its own (no FMA)
__device__ __forceinline__ float aug_scale_factor(float scale_range, uint32_t h) {
#pragma clang fp contract(off)
    return (float)(1.0 + (double)scale_range * ((double)h * 4.656612873077392578125e-10 - 1.0));
}

inline uint64_t aug_thresh(float p) {
    return p <= 0.f ? 0ull : p >= 1.f ? (1ull << 32) : (uint64_t)((double)p * 4294967296.0);
}

// a sample of n values is summed in chunks of 4096, doubled until there are at most 64 (both plan kernels; ops.py's
// *_plan_layout compute the same)
struct AugChunks { int chunk, nchunk; };
inline AugChunks aug_chunks(int64_t n) {
    int64_t chunk = 4096;
    while ((n + chunk - 1) / chunk > 64) chunk *= 2;
    return {(int)chunk, (int)((n + chunk - 1) / chunk)};
}
