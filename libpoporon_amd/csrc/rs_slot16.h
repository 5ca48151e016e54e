/*
 * rs_slot16.h -- the 16-byte slot walk of the layout kernels: a run of bytes
 * at any alignment is cut at the 16-byte boundaries of its own address, and a
 * lane takes one slot, as one uint4 access when the slot lies inside the run,
 * byte by byte over the part [kb, ke) inside it at the run's head and tail.
 * Nothing outside a run is read or written by any helper here.
 *
 *   slot16_part          where slot q of a run lies: its offset o0 from the
 *                        run's first byte (negative in the head slot) and the
 *                        part [kb, ke) inside the run; false, with kb >= ke,
 *                        for a slot that holds nothing of it.
 *   slot16_part_aligned  the same for a run known to start on a boundary.
 *   slot16_load          the slot's 16 bytes; bytes outside [kb, ke) are copies
 *                        of bytes inside it.
 *   slot16_store         the slot whole, or its bytes [kb, ke).
 *   slot16_divmod        i / d and i mod d by a reciprocal, i < 2^24.
 *   slot16_spread        a slot's bytes [kb, ke) to LDS bytes `step` apart;
 *   slot16_collect       the other way, bytes outside [kb, ke) zero.
 *   slot16_image_out     workgroup-wide: the LDS image of a run to the run;
 *   slot16_image_in      the run to its image.  Byte b of the run lies at LDS
 *                        byte (run address & 15) + b, so a slot of the run is
 *                        an aligned uint4 of LDS.
 *   slot16_batched       the loop that keeps BATCH global loads in flight per
 *                        lane: locate and load BATCH slots, then consume them.
 *
 * Users: rs_interleave.hip (part, load, store, spread, image_out, batched),
 * rs_conv.hip (part, load, store, divmod, spread, batched), rs_planes.hip (all
 * of them), rs_product.hip (all but collect and store: its scatter writes a
 * partial slot as dwords and keeps the collect beside that store),
 * rs_soft.hip (part, load).  rs_report.hip keeps its own zero-filling load and
 * padded store: other contracts.
 */
#ifndef POPORON_AMD_RS_SLOT16_H
#define POPORON_AMD_RS_SLOT16_H

#include <stdint.h>

#include <hip/hip_runtime.h>

/* the part [kb, ke) of 16-byte slot q of a region at p (len bytes) that lies
 * inside it; o0 = the slot's offset from p (negative in the head slot) */
static __device__ __forceinline__ bool slot16_part(const uint8_t *p, uint32_t len, uint32_t q, int32_t &o0, uint32_t &kb,
                                                   uint32_t &ke)
{
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    o0 = (int32_t)(q * 16u) - (int32_t)head;
    kb = ke = 0u;
    if (o0 >= (int32_t)len)
        return false;
    kb = o0 < 0 ? (uint32_t)(-o0) : 0u;
    ke = (int32_t)len - o0 < 16 ? (uint32_t)((int32_t)len - o0) : 16u;
    return kb < ke;
}

/* the same for a run on a 16-byte boundary: no head, only the last slot can be partial */
static __device__ __forceinline__ bool slot16_part_aligned(uint32_t len, uint32_t q, int32_t &o0, uint32_t &kb,
                                                           uint32_t &ke)
{
    o0 = (int32_t)(q * 16u);
    kb = ke = 0u;
    if (o0 >= (int32_t)len)
        return false;
    ke = len - q * 16u < 16u ? len - q * 16u : 16u;
    return true;
}

/* 16 bytes of slot [kb, ke) at p + o0: one uint4 load when whole, else its
 * bytes.  A wave takes the byte path whenever one of its 64 slots is a run's
 * head or tail, which at small depths is nearly every wave, so the 16 byte
 * loads carry no branch and do not wait for one another: byte k outside
 * [kb, ke) re-reads the nearest byte inside it (never one outside the run)
 * and is not used. */
static __device__ __forceinline__ uint4 slot16_load(const uint8_t *p, int32_t o0, uint32_t kb, uint32_t ke)
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

/* one slot's store: whole as a uint4, else its bytes [kb, ke) */
static __device__ __forceinline__ void slot16_store(uint8_t *p, int32_t o0, uint32_t kb, uint32_t ke, const uint32_t w[4])
{
    if (kb == 0u && ke == 16u) {
        *reinterpret_cast<uint4 *>(p + o0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++)
            if (k >= kb && k < ke)
                p[o0 + (int32_t)k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
    }
}

/* quo = i / d, rem = i mod d for i < 2^24 and inv = 1.0f / d: i is exact in
 * float and the quotient estimate off by at most one.  A caller that wants the
 * remainder alone ignores quo. */
static __device__ __forceinline__ void slot16_divmod(uint32_t i, uint32_t d, float inv, uint32_t &quo, uint32_t &rem)
{
    quo = (uint32_t)((float)i * inv);
    int32_t r = (int32_t)(i - quo * d);
    if (r < 0) {
        r += (int32_t)d;
        quo--;
    } else if (r >= (int32_t)d) {
        r -= (int32_t)d;
        quo++;
    }
    rem = (uint32_t)r;
}

/* byte k of x -> c[k * step] for k in [kb, ke); c is where byte 0 would go (before the image only with kb > 0).  A
 * whole slot, nearly every one, is sixteen stores and no branch. */
static __device__ __forceinline__ void slot16_spread(uint8_t *c, int32_t step, const uint32_t x[4], uint32_t kb,
                                                     uint32_t ke)
{
    if (kb == 0u && ke == 16u) {
#pragma unroll
        for (int32_t k = 0; k < 16; k++)
            c[k * step] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int32_t k = 0; k < 16; k++)
            if ((uint32_t)k >= kb && (uint32_t)k < ke)
                c[k * step] = (uint8_t)(x[k >> 2] >> (8 * (k & 3)));
    }
}

/* the other way: x = the bytes c[k * step], k in [kb, ke), zero around them; a whole slot is sixteen loads in flight
 * and no branch */
static __device__ __forceinline__ void slot16_collect(uint32_t x[4], const uint8_t *c, int32_t step, uint32_t kb,
                                                      uint32_t ke)
{
    x[0] = x[1] = x[2] = x[3] = 0u;
    if (kb == 0u && ke == 16u) {
#pragma unroll
        for (int32_t k = 0; k < 16; k++)
            x[k >> 2] |= (uint32_t)c[k * step] << (8 * (k & 3));
    } else {
#pragma unroll
        for (int32_t k = 0; k < 16; k++)
            if ((uint32_t)k >= kb && (uint32_t)k < ke)
                x[k >> 2] |= (uint32_t)c[k * step] << (8 * (k & 3));
    }
}

/* LDS image -> the run of len bytes, by a workgroup of THREADS lanes: byte b of the run is LDS byte (run & 15) + b.
 * Whole slots move as uint4, the head and tail slot as their bytes inside the run.  The test for a whole slot comes
 * first and on its own: nearly every slot passes it (measured on the plane kernels, whose runs have no head). */
template <uint32_t THREADS>
static __device__ __forceinline__ void slot16_image_out(uint8_t *run, uint32_t len, const uint4 *lds128)
{
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u), end = head + len;
    const uint8_t *lds = reinterpret_cast<const uint8_t *>(lds128);
    for (uint32_t q = threadIdx.x; q * 16u < end; q += THREADS) {
        const uint32_t s0 = q * 16u, s1 = s0 + 16u; /* the slot is LDS bytes [s0, s1), the run [head, end) */
        if (s0 >= head && s1 <= end) {
            *reinterpret_cast<uint4 *>(run + (s0 - head)) = lds128[q];
        } else {
            const uint32_t b1 = s1 < end ? s1 : end;
            for (uint32_t b = s0 > head ? s0 : head; b < b1; b++)
                run[b - head] = lds[b];
        }
    }
}

/* the run -> its LDS image, the same walk */
template <uint32_t THREADS>
static __device__ __forceinline__ void slot16_image_in(uint4 *lds128, const uint8_t *run, uint32_t len)
{
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u), end = head + len;
    uint8_t *lds = reinterpret_cast<uint8_t *>(lds128);
    for (uint32_t q = threadIdx.x; q * 16u < end; q += THREADS) {
        const uint32_t s0 = q * 16u, s1 = s0 + 16u;
        if (s0 >= head && s1 <= end) {
            lds128[q] = *reinterpret_cast<const uint4 *>(run + (s0 - head));
        } else {
            const uint32_t b1 = s1 < end ? s1 : end;
            for (uint32_t b = s0 > head ? s0 : head; b < b1; b++)
                lds[b] = run[b - head];
        }
    }
}

/* one slot of a batch: where it lies, its part, and one dword of the caller's */
struct Slot16 {
    int32_t o0;
    uint32_t kb, ke, tag;
};

/* Items [0, total) over a workgroup of THREADS lanes, BATCH global loads in flight per lane: the loads' latency is
 * paid once per batch, not once per slot.  fetch(i, sl, v) locates item i's slot, loads it into v itself and leaves
 * kb >= ke (as it finds them) for a slot that holds nothing; use(sl, v) then consumes every slot with kb < ke.  Both
 * are lambdas at the call site and inline. */
template <uint32_t THREADS, uint32_t BATCH, typename Fetch, typename Use>
static __device__ __forceinline__ void slot16_batched(uint32_t total, Fetch fetch, Use use)
{
    for (uint32_t base = threadIdx.x; base < total; base += THREADS * BATCH) {
        Slot16 sl[BATCH];
        uint4 v[BATCH];
#pragma unroll
        for (uint32_t u = 0; u < BATCH; u++) {
            const uint32_t i = base + u * THREADS;
            sl[u] = Slot16{0, 0u, 0u, 0u};
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (i < total)
                fetch(i, sl[u], v[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < BATCH; u++)
            if (sl[u].kb < sl[u].ke)
                use(sl[u], v[u]);
    }
}

#endif
