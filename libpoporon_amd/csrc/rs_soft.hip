/*
 * rs_soft.hip -- Chase-2 soft-decision RS decode around the row decoders
 * (gfx950): the two kernels either side of launch_decode (api.cpp soft_run).
 *
 * A codeword arrives as W m int8 LLRs (W = size + nr symbols of m bits, MSB
 * first, negative = 1; poporon_amd.h has the contract).  Its hard row is the
 * signs; the `flips` least reliable bits are the smallest keys
 * (|llr| << 11 | bit index), unique, so ties go to the lower index and round k
 * of the selection is "the smallest key above round k-1's": nothing is
 * retired and no row is sorted.
 *
 *   rs_soft_expand_k  one wave per codeword, four per workgroup.  The LLR row
 *                     goes into LDS once (16-byte slots cut at the row's own
 *                     address, rs_slot16.h: whole slots as uint4, the head
 *                     and tail of an unaligned row byte by byte).  A lane
 *                     builds the hard symbols lane, lane + 64, ...; then it
 *                     holds 32 consecutive LLRs in registers and `flips`
 *                     rounds of a wave-wide minimum (shuffle butterfly) find
 *                     the picks.  The 2^flips candidate rows go out as whole
 *                     RS_ILV_ROW-byte staging rows, 16 lanes a row and four
 *                     rows a store: lane (r, q) holds slot q of the hard row
 *                     and the picks' bits that fall into it, and XORs in the
 *                     ones that candidate 4i + r flips.  Bytes W .. 255 of a
 *                     row are written as zeros.
 *   rs_soft_select_k  the same wave per codeword after the decode.  The hard
 *                     row is formed again from the LLRs, which the scores need
 *                     anyway: nothing but the candidates' rows and ok flags
 *                     passes between the two kernels.  Lane (r, q) reads slot
 *                     q of the decoded candidate 4i + r, and for every bit
 *                     that differs from the hard row adds that bit's
 *                     magnitude; 16 lanes add up to the candidate's score, and
 *                     the minimum of (score << 6 | p) over the ok candidates
 *                     is the winner, ties to the lowest p.  Its row (or the
 *                     hard row when no candidate decoded) goes to the caller's
 *                     rows byte by byte, at any alignment and stride.
 *
 * All integer arithmetic: the order of the lane reductions changes nothing.
 * Control flow around every shuffle is wave-uniform (a wave without a codeword
 * leaves only after the last workgroup barrier and before the first shuffle).
 * Nothing outside an LLR row's W m bytes is read; nothing outside the chunk's
 * staging rows, the callers' size + nr row bytes and result entries is written.
 */
#include "rs_device.h"
#include "rs_slot16.h"

#define RS_SOFT_THREADS 256u
#define RS_SOFT_WAVES 4u     /* codewords per workgroup */
#define RS_SOFT_LLR 2048u    /* LDS bytes of one LLR row: 255 symbols x 8 bits = 2040 at the most */
#define RS_SOFT_NONE 0xFFFFFFFFu

static __device__ __forceinline__ uint32_t soft_mag(uint32_t b)
{
    const int32_t v = (int8_t)b;
    return (uint32_t)(v < 0 ? -v : v); /* -128 -> 128 */
}

static __device__ __forceinline__ uint32_t soft_xor(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off); }

/* the len LLRs at p -> dst[0 .. len), by the wave */
static __device__ __forceinline__ void soft_load_llr(uint8_t *dst, const uint8_t *p, uint32_t len, uint32_t lane)
{
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u), slots = (head + len + 15u) / 16u;
    for (uint32_t q = lane; q < slots; q += 64u) {
        int32_t o0;
        uint32_t kb, ke;
        if (!slot16_part(p, len, q, o0, kb, ke))
            continue;
        const uint4 v = slot16_load(p, o0, kb, ke);
        if (head == 0u && kb == 0u && ke == 16u) {
            *reinterpret_cast<uint4 *>(dst + o0) = v;
        } else {
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++)
                if (k >= kb && k < ke)
                    dst[o0 + (int32_t)k] = (uint8_t)(x[k >> 2] >> (8u * (k & 3u)));
        }
    }
}

/* hard[s] for every s < 256: the signs of symbol s's m LLRs, MSB first; 0 from w on */
static __device__ __forceinline__ void soft_hard_row(const uint8_t *llr, uint8_t *hard, uint32_t w, uint32_t m,
                                                     uint32_t lane)
{
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t s = lane + 64u * i;
        uint32_t h = 0u;
        if (s < w)
            for (uint32_t j = 0; j < m; j++)
                h |= (uint32_t)(llr[s * m + j] >> 7) << (m - 1u - j);
        hard[s] = (uint8_t)h;
    }
}

__global__ __launch_bounds__(RS_SOFT_THREADS) void rs_soft_expand_k(const uint8_t *llr, size_t ls, uint8_t *rows,
                                                                    uint32_t w, uint32_t m, uint32_t flips, size_t n)
{
    __shared__ uint4 llr4[RS_SOFT_WAVES][RS_SOFT_LLR / 16u];
    __shared__ uint4 hard4[RS_SOFT_WAVES][16];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nbits = w * m;
    const size_t c = (size_t)blockIdx.x * RS_SOFT_WAVES + wv;
    const bool live = c < n;
    uint8_t *L = reinterpret_cast<uint8_t *>(llr4[wv]), *H = reinterpret_cast<uint8_t *>(hard4[wv]);
    if (live)
        soft_load_llr(L, llr + c * ls, nbits, lane);
    __syncthreads();
    if (live)
        soft_hard_row(L, H, w, m, lane);
    __syncthreads();
    if (!live)
        return;
    /* bits 32 lane .. 32 lane + 31 (LDS bytes from nbits on hold nothing: masked by their index) */
    const uint4 a = llr4[wv][2u * lane], b = llr4[wv][2u * lane + 1u];
    const uint32_t q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t slot = lane & 15u;
    uint4 fm[6]; /* pick k's bit where it falls into this lane's slot of a row */
    int32_t prev = -1;
#pragma unroll
    for (uint32_t k = 0; k < 6u; k++) {
        fm[k] = make_uint4(0u, 0u, 0u, 0u);
        if (k >= flips) /* (uniform) */
            continue;
        uint32_t mn = RS_SOFT_NONE;
#pragma unroll
        for (uint32_t i = 0; i < 32u; i++) {
            const uint32_t idx = 32u * lane + i, key = soft_mag((q[i >> 2] >> (8u * (i & 3u))) & 255u) << 11 | idx;
            if (idx < nbits && (int32_t)key > prev && key < mn)
                mn = key;
        }
#pragma unroll
        for (int off = 32; off; off >>= 1)
            mn = min(mn, soft_xor(mn, off));
        prev = (int32_t)mn; /* flips <= nbits: a key every round */
        const uint32_t idx = mn & 2047u, sym = idx / m, bit = m - 1u - (idx - sym * m);
        if ((sym >> 4) == slot) {
            const uint32_t v = 1u << (8u * (sym & 3u) + bit), d = (sym & 15u) >> 2;
            fm[k] = make_uint4(d == 0u ? v : 0u, d == 1u ? v : 0u, d == 2u ? v : 0u, d == 3u ? v : 0u);
        }
    }
    const uint4 base = hard4[wv][slot];
    uint4 *out = reinterpret_cast<uint4 *>(rows + (c << flips) * RS_ILV_ROW);
    const uint32_t np = 1u << flips;
    for (uint32_t p = lane >> 4; p < np; p += 4u) {
        uint4 x = base;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) {
            const uint32_t on = 0u - ((p >> k) & 1u);
            x.x ^= fm[k].x & on;
            x.y ^= fm[k].y & on;
            x.z ^= fm[k].z & on;
            x.w ^= fm[k].w & on;
        }
        out[p * (RS_ILV_ROW / 16u) + slot] = x;
    }
}

__global__ __launch_bounds__(RS_SOFT_THREADS) void rs_soft_select_k(const uint8_t *llr, size_t ls, const uint8_t *rows,
                                                                    const uint8_t *cok, uint32_t w, uint32_t size,
                                                                    uint32_t m, uint32_t flips, size_t n, uint8_t *data,
                                                                    size_t ds, uint8_t *par, size_t ps, uint8_t *ok,
                                                                    uint8_t *changed, uint8_t *pattern, uint32_t *score)
{
    __shared__ uint4 llr4[RS_SOFT_WAVES][RS_SOFT_LLR / 16u];
    __shared__ uint4 hard4[RS_SOFT_WAVES][16];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const size_t c = (size_t)blockIdx.x * RS_SOFT_WAVES + wv;
    const bool live = c < n;
    uint8_t *L = reinterpret_cast<uint8_t *>(llr4[wv]), *H = reinterpret_cast<uint8_t *>(hard4[wv]);
    if (live)
        soft_load_llr(L, llr + c * ls, w * m, lane);
    __syncthreads();
    if (live)
        soft_hard_row(L, H, w, m, lane);
    __syncthreads();
    if (!live)
        return;
    const uint32_t slot = lane & 15u, np = 1u << flips;
    const uint4 base = hard4[wv][slot];
    uint32_t vm[4]; /* the slot's bytes below w */
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) {
        vm[d] = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            if (16u * slot + 4u * d + k < w)
                vm[d] |= 0xFFu << (8u * k);
    }
    const uint8_t *cr = rows + (c << flips) * RS_ILV_ROW, *co = cok + (c << flips);
    uint32_t best = RS_SOFT_NONE;
    for (uint32_t p0 = 0; p0 < np; p0 += 4u) {
        const uint32_t p = p0 + (lane >> 4);
        const bool okp = p < np && co[p] != 0u;
        uint32_t sc = 0u;
        if (okp) {
            const uint4 y = reinterpret_cast<const uint4 *>(cr)[p * (RS_ILV_ROW / 16u) + slot];
            const uint32_t diff[4] = {(y.x ^ base.x) & vm[0], (y.y ^ base.y) & vm[1], (y.z ^ base.z) & vm[2],
                                      (y.w ^ base.w) & vm[3]};
#pragma unroll
            for (uint32_t d = 0; d < 4u; d++) {
                uint32_t x = diff[d];
                while (x) { /* a few symbols of a row at the most */
                    const uint32_t at = (uint32_t)__ffs((int)x) - 1u, bit = at & 7u;
                    x &= x - 1u;
                    if (bit < m)
                        sc += soft_mag(L[(16u * slot + 4u * d + (at >> 3)) * m + (m - 1u - bit)]);
                }
            }
        }
        sc += soft_xor(sc, 8);
        sc += soft_xor(sc, 4);
        sc += soft_xor(sc, 2);
        sc += soft_xor(sc, 1);
        if (okp) /* score <= 2040 * 128 < 2^18 */
            best = min(best, sc << 6 | p);
    }
    best = min(best, soft_xor(best, 16));
    best = min(best, soft_xor(best, 32));
    const bool win = best != RS_SOFT_NONE;
    const uint8_t *y = cr + (size_t)(best & 63u) * RS_ILV_ROW;
    uint32_t nch = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t s = lane + 64u * i;
        const uint8_t hs = H[s];
        uint8_t v = hs;
        if (s < w) {
            if (win)
                v = y[s];
            if (s < size)
                data[c * ds + s] = v;
            else
                par[c * ps + (s - size)] = v;
        }
        nch += (uint32_t)__popcll(__ballot(v != hs));
    }
    if (lane == 0u) {
        ok[c] = win ? 1u : 0u;
        if (changed)
            changed[c] = (uint8_t)nch;
        if (pattern)
            pattern[c] = win ? (uint8_t)(best & 63u) : (uint8_t)0u;
        if (score)
            score[c] = win ? best >> 6 : 0u;
    }
}

static bool soft_shape(const void *llr, size_t ls, const uint8_t *rows, uint32_t size, uint32_t nr, uint32_t m,
                       uint32_t flips, size_t n)
{
    const uint32_t w = size + nr;
    return llr && rows && !(reinterpret_cast<uintptr_t>(rows) & 15u) && size >= 1u && w <= 255u && m >= 1u && m <= 8u &&
           flips <= 6u && flips <= w * m && ls >= (size_t)w * m && (n + RS_SOFT_WAVES - 1u) / RS_SOFT_WAVES <= 0x7FFFFFFFu;
}

extern "C" hipError_t rsk_soft_expand(const int8_t *llr, size_t llr_stride, uint8_t *rows, uint32_t size, uint32_t nr,
                                      uint32_t m, uint32_t flips, size_t n, hipStream_t s)
{
    if (!soft_shape(llr, llr_stride, rows, size, nr, m, flips, n))
        return hipErrorInvalidValue;
    if (n == 0)
        return hipSuccess;
    const uint32_t grid = (uint32_t)((n + RS_SOFT_WAVES - 1u) / RS_SOFT_WAVES);
    RS_LAUNCH(rs_soft_expand_k, dim3(grid), dim3(RS_SOFT_THREADS), 0, s, reinterpret_cast<const uint8_t *>(llr),
              llr_stride, rows, size + nr, m, flips, n);
    return hipGetLastError();
}

extern "C" hipError_t rsk_soft_select(const int8_t *llr, size_t llr_stride, const uint8_t *rows, const uint8_t *cand_ok,
                                      uint32_t size, uint32_t nr, uint32_t m, uint32_t flips, size_t n, uint8_t *data,
                                      size_t ds, uint8_t *parity, size_t ps, uint8_t *ok, uint8_t *changed,
                                      uint8_t *pattern, uint32_t *score, hipStream_t s)
{
    if (!soft_shape(llr, llr_stride, rows, size, nr, m, flips, n) || !cand_ok || !data || !parity || !ok)
        return hipErrorInvalidValue;
    if (n == 0)
        return hipSuccess;
    const uint32_t grid = (uint32_t)((n + RS_SOFT_WAVES - 1u) / RS_SOFT_WAVES);
    RS_LAUNCH(rs_soft_select_k, dim3(grid), dim3(RS_SOFT_THREADS), 0, s, reinterpret_cast<const uint8_t *>(llr),
              llr_stride, rows, cand_ok, size + nr, size, m, flips, n, data, ds, parity, ps, ok, changed, pattern, score);
    return hipGetLastError();
}
