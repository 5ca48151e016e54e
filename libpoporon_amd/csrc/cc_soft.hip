/*
 * cc_soft.hip -- soft-output (max-log-MAP) decode of the K = 7 convolutional
 * code (gfx950): poporon_amd.h has the contract, tests/cc_soft_ref.py the model,
 * api.cpp the argument checks and the launch loop; code, puncturing, costs,
 * blocks and windows are those of cc.hip.
 *
 *   cc_soft_k  one wave per block of a frame, one wave per workgroup, lane =
 *              trellis state.  A window's forward metrics A do not fit the LDS
 *              (64 x 4 B per step), so the kernel keeps a checkpoint of them
 *              every 64 steps and computes them again where they are needed.
 *              The window is cut into segments of 64 steps, counted from `pad`
 *              steps before its first so that the block's first own step starts
 *              a segment: an own segment's 64 outputs are then 64 adjacent bytes
 *              of the frame, step r in lane r.
 *              1. Forward: cc_decode_k's add-compare-select (a lane writes the
 *                 four branch costs of one step of the segment to LDS, the next
 *                 segment's LLR loads are issued before the current one runs;
 *                 a step is two LDS reads, two ds_bpermute, two adds and a
 *                 minimum), without decisions; a lane stores its metric at the
 *                 start of every segment.
 *              2. Backward from t1, a segment at a time, down to the block's
 *                 first own step (the overlap in front is never walked).  Z runs
 *                 over the states' successors (state s goes to s >> 1 and to
 *                 32 + (s >> 1)) with the same costs.  A segment of the trailing
 *                 overlap only runs Z.  An own segment first runs A again from
 *                 its checkpoint and keeps the lane's 64 values in registers
 *                 (fully unrolled, no scratch), then runs Z down the segment and
 *                 writes A + Z of every step, 64 sums, as one row of LDS.
 *              3. The two 32-lane minima per step come from LDS, 32 steps at a
 *                 time: lane l takes step l % 32 and input bit l / 32 and reads
 *                 the 32 sums of that half of the row as eight 16-byte loads
 *                 (rows are CC_SOFT_ROW = 68 words apart: the lanes of one
 *                 16-byte access group fall on distinct banks); the other
 *                 bit's minimum comes from lane l ^ 32, and both lanes form the
 *                 output.  Lane r keeps the byte of step r of the segment.
 *              4. One byte store per lane: 64 adjacent bytes per segment, fewer
 *                 lanes at a frame's end.
 *
 * Sums are the contract's integers in 32 bits: "no path" is 2^28, a window costs
 * at most 6144 * 256, so A + Z stays below 2^30.  Nothing outside a frame's
 * symbols(nbits) LLRs is read, nothing outside its nbits output bytes is
 * written.  Control flow around every cross-lane operation and every barrier is
 * wave-uniform.
 */
#include "cc_device.h"

__global__ __launch_bounds__(CC_STATES) void cc_soft_k(CcParams p, const int8_t *llr, size_t ls, uint64_t nbits,
                                                       uint64_t blocks, uint64_t first, int start_state, int end_state,
                                                       uint32_t shift, int8_t *soft, size_t ss)
{
    extern __shared__ uint4 cc_soft_lds_[];
    const uint32_t lane = threadIdx.x;
    const uint64_t gb = first + blockIdx.x, c = gb / blocks, b = gb - c * blocks;
    const uint64_t e0 = b * p.block, e1 = e0 + p.block < nbits ? e0 + p.block : nbits;
    const uint64_t t0 = e0 > p.overlap ? e0 - p.overlap : 0u;
    const uint64_t t1 = e0 + p.block + p.overlap < nbits ? e0 + p.block + p.overlap : nbits;
    const uint32_t n = (uint32_t)(t1 - t0); /* 1 .. block + 2 overlap */
    /* window step i is step i + pad of the padded window; the block's own steps [i0, i0 + er) start segment ks */
    const uint32_t i0 = (uint32_t)(e0 - t0), er = (uint32_t)(e1 - e0);
    const uint32_t pad = (64u - (i0 & 63u)) & 63u, np = n + pad, segs = (np + 63u) >> 6;
    const uint32_t ks = (i0 + pad) >> 6, kown = ks + ((er + 63u) >> 6);

    uint32_t *sums = reinterpret_cast<uint32_t *>(cc_soft_lds_); /* [step % 32][CC_SOFT_ROW] */
    uint2 *cost2 = reinterpret_cast<uint2 *>(sums + 32u * CC_SOFT_ROW);
    const uint16_t *cost = reinterpret_cast<const uint16_t *>(cost2);
    uint32_t *ckpt = reinterpret_cast<uint32_t *>(cost2 + CC_STATES); /* [segment][lane] */

    /* forward: the lane's state s' has the predecessors pred0 and pred0 + 1 and the hypothesised input s' >> 5 */
    const uint32_t pred0 = (lane << 1) & 63u, reg = (lane >> 5) << 6 | pred0;
    const uint16_t *cp0 = cost + cc_label(p, reg), *cp1 = cost + cc_label(p, reg | 1u);
    const int bp0 = (int)(pred0 * 4u), bp1 = bp0 + 4;
    /* backward: the lane's state s has the successors s >> 1 (input 0) and 32 + (s >> 1) (input 1) */
    const uint16_t *cq0 = cost + cc_label(p, lane), *cq1 = cost + cc_label(p, 64u | lane);
    const int bq0 = (int)((lane >> 1) * 4u), bq1 = bq0 + 128;

    /* step t0 + i's kept symbols lie at base[off], off counted from the window's first; i outside [0, n) gives 0 */
    const uint32_t ph0 = (uint32_t)(t0 % p.period), pre0 = cc_prefix(p, ph0);
    const int8_t *base = llr + c * ls + cc_symbols_before(p, t0);
    auto fetch = [&](uint32_t i, int32_t &v0, int32_t &v1) {
        v0 = v1 = 0;
        if (i < n) {
            const uint32_t x = ph0 + i, q = x / p.period, ph = x - q * p.period;
            const uint32_t off = q * p.kept + cc_prefix(p, ph) - pre0, k0 = (p.keep0 >> ph) & 1u;
            if (k0)
                v0 = base[off];
            if ((p.keep1 >> ph) & 1u)
                v1 = base[off + k0];
        }
    };
    auto put_costs = [&](int32_t v0, int32_t v1) {
        const uint32_t a0 = (uint32_t)max(-v0, 0), a1 = (uint32_t)max(v0, 0);
        const uint32_t b0 = (uint32_t)max(-v1, 0), b1 = (uint32_t)max(v1, 0);
        cost2[lane] = make_uint2((a0 + b0) | (a1 + b0) << 16, (a0 + b1) | (a1 + b1) << 16);
    };
    auto fstep = [&](uint32_t a, uint32_t j) {
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_ds_bpermute(bp0, (int)a) + cp0[4u * j];
        const uint32_t m1 = (uint32_t)__builtin_amdgcn_ds_bpermute(bp1, (int)a) + cp1[4u * j];
        return min(m0, m1);
    };
    auto zstep = [&](uint32_t z, uint32_t j) {
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_ds_bpermute(bq0, (int)z) + cq0[4u * j];
        const uint32_t m1 = (uint32_t)__builtin_amdgcn_ds_bpermute(bq1, (int)z) + cq1[4u * j];
        return min(m0, m1);
    };

    /* ---- forward: A at the start of every segment ---- */
    uint32_t metric = t0 == 0u && start_state >= 0 && lane != (uint32_t)start_state ? CC_INF : 0u;
    int32_t v0, v1;
    fetch(lane - pad, v0, v1);
    for (uint32_t k = 0; k < segs; k++) {
        put_costs(v0, v1);
        __syncthreads();
        if (k + 1u < segs)
            fetch((k + 1u) * 64u + lane - pad, v0, v1);
        ckpt[k * 64u + lane] = metric;
        const uint32_t lo = k ? 0u : pad, hi = min(64u, np - k * 64u);
        if (lo == 0u && hi == 64u) {
#pragma unroll
            for (uint32_t j = 0; j < 64u; j++)
                metric = fstep(metric, j);
        } else {
            for (uint32_t j = lo; j < hi; j++)
                metric = fstep(metric, j);
        }
        __syncthreads();
    }

    /* ---- backward: Z from t1 down to the block's first own step ---- */
    uint32_t z = t1 == nbits && end_state >= 0 && lane != (uint32_t)end_state ? CC_INF : 0u;
    const uint32_t *mine = sums + (lane & 31u) * CC_SOFT_ROW + (lane >> 5) * 32u; /* the sums this lane reduces */
    int8_t *out = soft + c * ss + e0;
    fetch((segs - 1u) * 64u + lane - pad, v0, v1);
    for (uint32_t k = segs; k-- > ks;) {
        put_costs(v0, v1);
        __syncthreads();
        if (k > ks)
            fetch((k - 1u) * 64u + lane - pad, v0, v1);
        const uint32_t hi = min(64u, np - k * 64u); /* k >= ks: no padded step in the segment */
        if (k >= kown) { /* the trailing overlap */
            if (hi == 64u) {
#pragma unroll
                for (uint32_t j = 64u; j-- > 0u;)
                    z = zstep(z, j);
            } else {
                for (uint32_t j = hi; j-- > 0u;)
                    z = zstep(z, j);
            }
            __syncthreads();
            continue;
        }
        /* own steps: A after each step of the segment (steps at or past hi have zero costs and are not used) */
        uint32_t A[64];
        {
            uint32_t a = ckpt[k * 64u + lane];
#pragma unroll
            for (uint32_t j = 0; j < 64u; j++)
                A[j] = a = fstep(a, j);
        }
        int32_t val = 0;
#pragma unroll
        for (uint32_t half = 2u; half-- > 0u;) {
#pragma unroll
            for (uint32_t jj = 32u; jj-- > 0u;) {
                const uint32_t j = half * 32u + jj;
                if (j < hi) { /* the step's output takes A and Z after it */
                    sums[jj * CC_SOFT_ROW + lane] = A[j] + z;
                    z = zstep(z, j);
                }
            }
            __syncthreads();
            if (half * 32u < hi) {
                uint32_t m = 0xFFFFFFFFu;
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) {
                    const uint4 w = reinterpret_cast<const uint4 *>(mine)[q];
                    m = min(m, min(min(w.x, w.y), min(w.z, w.w)));
                }
                const uint32_t o = (uint32_t)__shfl_xor((int)m, 32);
                const int32_t x = lane < 32u ? (int32_t)(o - m) : (int32_t)(m - o); /* D_1 - D_0 */
                const int32_t mag = min(127, (x < 0 ? -x : x) >> shift);
                if ((lane >> 5) == half)
                    val = x > 0 ? mag : -mag;
            }
            __syncthreads();
        }
        if (lane < hi)
            out[(k - ks) * 64u + lane] = (int8_t)val;
    }
}

extern "C" hipError_t cck_decode_soft(const CcParams *p, const int8_t *llr, size_t llr_stride, uint64_t nbits,
                                      uint64_t blocks, uint64_t first, uint32_t n, int start_state, int end_state,
                                      uint32_t shift, int8_t *soft, size_t soft_stride, hipStream_t s)
{
    if (!p || !llr || !soft || !nbits || !blocks || n > 0x7FFFFFFFu || shift > 8u || p->block % 64u || p->block < 64u ||
        p->block > CC_BLOCK_MAX || p->overlap > CC_OVERLAP_MAX || !p->period || p->period > CC_PERIOD_MAX || !p->kept)
        return hipErrorInvalidValue;
    if (n == 0u)
        return hipSuccess;
    hipLaunchKernelGGL(cc_soft_k, dim3(n), dim3(CC_STATES), cc_soft_lds(*p), s, *p, llr, llr_stride, nbits, blocks, first,
                       start_state, end_state, shift, soft, soft_stride);
    return hipGetLastError();
}
