/*
 * cc_device.h -- what api.cpp, cc.hip and cc_soft.hip share of the K = 7
 * convolutional code: the code's parameters, passed to the kernels by value, the
 * launchers, and the kernels' label and prefix-count helpers.
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

/* the soft decode (cc_soft.hip): 64-step segments of a window that is padded in front so that the block's first own
 * step starts a segment (one segment more than the window's own), and the LDS bytes of one workgroup: 32 rows of
 * 64 sums at a stride of CC_SOFT_ROW words, the cost rows of 64 steps, a checkpoint of the 64 metrics per segment */
#define CC_SOFT_ROW 68u
static __host__ __device__ __forceinline__ uint32_t cc_soft_segments(const CcParams &p)
{
    return (p.block + 2u * p.overlap + 63u) / 64u + 1u;
}
static inline size_t cc_soft_lds(const CcParams &p)
{
    return 32u * CC_SOFT_ROW * 4u + CC_STATES * 8u + (size_t)cc_soft_segments(p) * 256u;
}

#ifdef __HIP__ /* what the kernels of cc.hip and cc_soft.hip share */
#define CC_INF 0x10000000u /* a state no path reaches */

static __device__ __forceinline__ uint32_t cc_label(const CcParams &p, uint32_t r)
{
    const uint32_t l0 = ((uint32_t)__popc(r & p.g0) ^ p.invert) & 1u;
    const uint32_t l1 = ((uint32_t)__popc(r & p.g1) ^ (p.invert >> 1)) & 1u;
    return l0 | l1 << 1;
}

static __device__ __forceinline__ uint32_t cc_prefix(const CcParams &p, uint32_t ph)
{
    const uint32_t below = (1u << ph) - 1u;
    return (uint32_t)__popc(p.keep0 & below) + (uint32_t)__popc(p.keep1 & below);
}
#endif

/* blocks [first, first + n) of the count * blocks of a call, one wave each; n < 2^31 */
extern "C" hipError_t cck_decode(const CcParams *p, const int8_t *llr, size_t llr_stride, uint64_t nbits, uint64_t blocks,
                                 uint64_t first, uint32_t n, int start_state, int end_state, uint8_t *bits,
                                 size_t bits_stride, uint32_t *metric, hipStream_t s);
/* the same blocks, soft outputs: one int8 per info bit at soft + c * soft_stride + t; shift in [0, 8] */
extern "C" hipError_t cck_decode_soft(const CcParams *p, const int8_t *llr, size_t llr_stride, uint64_t nbits,
                                      uint64_t blocks, uint64_t first, uint32_t n, int start_state, int end_state,
                                      uint32_t shift, int8_t *soft, size_t soft_stride, hipStream_t s);
/* output words [first, first + n) of the count * words of a call (words = max(1, ceil(symbols / 32)) per frame) */
extern "C" hipError_t cck_encode(const CcParams *p, const uint8_t *bits, size_t bits_stride, uint64_t nbits,
                                 uint64_t symbols, uint64_t words, uint64_t first, uint64_t n, int start_state,
                                 uint8_t *sym, size_t sym_stride, uint8_t *end_state, hipStream_t s);

#endif
