/*
 * cc_device.h -- what api.cpp and cc.hip share of the K = 7 convolutional code:
 * the code's parameters, passed to the kernels by value, and the launchers.
 */
#ifndef POPORON_AMD_CC_DEVICE_H
#define POPORON_AMD_CC_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#define CC_STATES 64u
#define CC_BLOCK_MAX 4096u
#define CC_OVERLAP_MAX 1024u
#define CC_PERIOD_MAX 16u
#define CC_ENC_THREADS 256u

/* g0, g1 in [1, 127], invert in [0, 3]; keep0 / keep1: bit k = phase k, none at or above period; kept = the kept
 * outputs of one period.  block / overlap are the decoder's B and V. */
struct CcParams {
    uint32_t g0, g1, invert, period, keep0, keep1, kept, block, overlap;
};

/* kept symbols of the steps [0, t) */
static __host__ __device__ __forceinline__ uint64_t cc_symbols_before(const CcParams &p, uint64_t t)
{
    const uint32_t ph = (uint32_t)(t % p.period), below = (1u << ph) - 1u;
    return t / p.period * p.kept + (uint32_t)__builtin_popcount(p.keep0 & below) +
           (uint32_t)__builtin_popcount(p.keep1 & below);
}

/* 32-step groups of the largest window, and the LDS bytes of one decode workgroup: a decision word per lane and
 * group, the cost rows of 64 steps */
static __host__ __device__ __forceinline__ uint32_t cc_decode_groups(const CcParams &p)
{
    return (p.block + 2u * p.overlap + 31u) / 32u;
}
static inline size_t cc_decode_lds(const CcParams &p) { return (size_t)cc_decode_groups(p) * 256u + CC_STATES * 8u; }

/* blocks [first, first + n) of the count * blocks of a call, one wave each; n < 2^31 */
extern "C" hipError_t cck_decode(const CcParams *p, const int8_t *llr, size_t llr_stride, uint64_t nbits, uint64_t blocks,
                                 uint64_t first, uint32_t n, int start_state, int end_state, uint8_t *bits,
                                 size_t bits_stride, uint32_t *metric, hipStream_t s);
/* output words [first, first + n) of the count * words of a call (words = max(1, ceil(symbols / 32)) per frame) */
extern "C" hipError_t cck_encode(const CcParams *p, const uint8_t *bits, size_t bits_stride, uint64_t nbits,
                                 uint64_t symbols, uint64_t words, uint64_t first, uint64_t n, int start_state,
                                 uint8_t *sym, size_t sym_stride, uint8_t *end_state, hipStream_t s);

#endif
