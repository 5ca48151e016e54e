/*
 * rs_slot16.h -- 16-byte slots of a run of bytes at any alignment, shared by
 * the layout kernels (rs_interleave.hip, rs_conv.hip).  A run is cut at the
 * 16-byte boundaries of its own address: a lane takes one slot, as one uint4
 * access when the slot lies inside the run, byte by byte over the part inside
 * it at the run's head and tail.  Nothing outside a run is read or written.
 */
#ifndef POPORON_AMD_RS_SLOT16_H
#define POPORON_AMD_RS_SLOT16_H

#include <stdint.h>

#include <hip/hip_runtime.h>

/* the part [kb, ke) of 16-byte slot q of a region at p (len bytes) that lies
 * inside it; o0 = the slot's offset from p (negative in the head slot) */
static __device__ __forceinline__ bool ilv_slot(const uint8_t *p, uint32_t len, uint32_t q, int32_t &o0, uint32_t &kb,
                                                uint32_t &ke)
{
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    o0 = (int32_t)(q * 16u) - (int32_t)head;
    if (o0 >= (int32_t)len)
        return false;
    kb = o0 < 0 ? (uint32_t)(-o0) : 0u;
    ke = (int32_t)len - o0 < 16 ? (uint32_t)((int32_t)len - o0) : 16u;
    return kb < ke;
}

/* 16 bytes of slot [kb, ke) at p + o0: one uint4 load when whole, else its
 * bytes.  A wave takes the byte path whenever one of its 64 slots is a run's
 * head or tail, which at small depths is nearly every wave, so the 16 byte
 * loads carry no branch and do not wait for one another: byte k outside
 * [kb, ke) re-reads the nearest byte inside it (never one outside the run)
 * and is not used. */
static __device__ __forceinline__ uint4 ilv_load16(const uint8_t *p, int32_t o0, uint32_t kb, uint32_t ke)
{
    if (kb == 0u && ke == 16u)
        return *reinterpret_cast<const uint4 *>(p + o0);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        const uint32_t kk = k < kb ? kb : k >= ke ? ke - 1u : k;
        w[k >> 2] |= (uint32_t)p[o0 + (int32_t)kk] << (8u * (k & 3u));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

#endif
