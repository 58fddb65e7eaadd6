// trackformer_amd/csrc/dropout_rng.h -- the counter-based generator behind the dropout of the training kernels (included from
// fused_ops.hip; include/tf_fused.h: DROPOUT INSIDE THE TRAINING KERNELS states the contract).
//
//   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): multipliers 0xD2511F53 /
//   0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.
//   key     = (seed low 32, seed high 32)
//   counter = (g low 32, g high 32, offset low 32, offset high 32),  g = the index of a group of four consecutive elements of the
//             flat tensor (C % 4 == 0: a group never straddles a row and is one 16-byte access)
//   output word j decides element 4 g + j:  kept iff word >= T,  T = floor(p 2^32) (dropout_threshold, on the host, in double)
//   survivors are multiplied by the float 1.0f / (1.0f - p) (dropout_scale)
//
// The decision is an integer comparison: a function of (seed, offset, p, element index) alone, whatever the launch geometry or the dtype
// of the data.  Plain C++ 64-bit multiplies; the compiler picks v_mul_lo_u32 / v_mul_hi_u32.
#ifndef TF_DROPOUT_RNG_H_
#define TF_DROPOUT_RNG_H_

#include <stdint.h>

namespace tfd {

struct Words {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

// what a kernel needs of the rng tensor (int64[2] = seed, offset on the device; read by every thread, never by the host)
struct Stream {
    uint32_t k0, k1, o0, o1;
};

__device__ __forceinline__ Stream load_stream(const long long *__restrict__ rng)
{
    const unsigned long long seed = (unsigned long long)rng[0], offset = (unsigned long long)rng[1];
    return Stream{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
}

// the four words of group g
__device__ __forceinline__ Words group_words(const Stream &s, unsigned long long g)
{
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), s.o0, s.o1, s.k0, s.k1);
}

// bit j: element 4 g + j is kept
__device__ __forceinline__ unsigned keep_bits(const Stream &s, unsigned long long g, uint32_t T)
{
    const Words w = group_words(s, g);
    return (w.w[0] >= T ? 1u : 0u) | (w.w[1] >= T ? 2u : 0u) | (w.w[2] >= T ? 4u : 0u) | (w.w[3] >= T ? 8u : 0u);
}

// host side of an entry point: p must be a finite number in (0, 1)
inline bool dropout_p_ok(float p) { return p > 0.f && p < 1.f; }
inline uint32_t dropout_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }   // floor: p < 1 keeps it below 2^32
inline float dropout_scale(float p) { return 1.0f / (1.0f - p); }

}  // namespace tfd

#endif /* TF_DROPOUT_RNG_H_ */
