/*
 * cc.hip -- the K = 7, rate-1/2 convolutional code with puncturing (gfx950):
 * batch encode and blocked Viterbi decode (poporon_amd.h has the contract,
 * tests/cc_ref.py the model, api.cpp the argument checks and the launch loops).
 *
 *   cc_decode_k  one wave per block of a frame, one wave per workgroup, lane =
 *                trellis state.  The window [t0, t1) of a block runs forward 64
 *                steps at a time.  Per 64 steps a lane takes one step: it reads
 *                that step's one or two kept LLRs straight from the frame (the
 *                symbol index follows from the masks' prefix counts; the loads
 *                of the next 64 steps are issued before the current 64 run) and
 *                writes the step's four branch costs, one per label pair, as
 *                four uint16 into LDS.  A step of the add-compare-select loop
 *                is then two LDS reads at the lane's two labels (fixed per
 *                lane, computed once from g0 / g1), two ds_bpermute for the
 *                predecessors' metrics, two adds, one compare and one select.
 *                A lane keeps its own decisions, one bit per step, and writes
 *                them to LDS as one word per 32 steps: nothing per step (a
 *                per-step store of the compare's lane mask from one lane was
 *                measured first and cost a quarter of the throughput: the loop
 *                is bound by the LDS pipe).  Metrics are the contract's costs
 *                themselves in 32 bits: a window is at most 6144 steps of at
 *                most 256, far below the 2^28 that stands for "no such path".
 *                The traceback walks from t1 down to the block's first step.
 *                Per 32 steps every lane loads its word; a step's 64 decisions
 *                are the ballot of the lanes' bits, and the walk itself is
 *                wave-uniform (shift, and, or on the scalar unit) with no LDS
 *                access in the chain.  64 output bits, packed MSB first, land
 *                in one lane; after the walk lane k stores bytes 8k .. 8k+7 of
 *                the block's output as one uint64 where the address allows,
 *                else byte by byte.
 *   cc_encode_k  one thread per 32 output symbols (one big-endian word).  The
 *                thread finds the step of its first symbol from the prefix
 *                counts, rebuilds the state from the six input bits before it
 *                (start_state's bits before step 0) and runs the register until
 *                its word is full.  The thread of a frame's word 0 also writes
 *                the end state: the frame's last six input bits.
 *
 * Nothing outside a frame's symbols(nbits) LLRs or ceil(nbits / 8) input bytes
 * is read, nothing outside its ceil(n / 8) output bytes and its result entries
 * is written.  Control flow around every cross-lane operation is wave-uniform.
 */
#include "cc_device.h"

__global__ __launch_bounds__(CC_STATES) void cc_decode_k(CcParams p, const int8_t *llr, size_t ls, uint64_t nbits,
                                                         uint64_t blocks, uint64_t first, int start_state,
                                                         int end_state, uint8_t *bits, size_t bs, uint32_t *metric_out)
{
    extern __shared__ uint64_t cc_lds[];
    const uint32_t lane = threadIdx.x;
    const uint64_t gb = first + blockIdx.x, c = gb / blocks, b = gb - c * blocks;
    const uint64_t e0 = b * p.block, e1 = e0 + p.block < nbits ? e0 + p.block : nbits;
    const uint64_t t0 = e0 > p.overlap ? e0 - p.overlap : 0u;
    const uint64_t t1 = e0 + p.block + p.overlap < nbits ? e0 + p.block + p.overlap : nbits;
    const uint32_t n = (uint32_t)(t1 - t0); /* 1 .. block + 2 overlap */
    uint32_t *dec = reinterpret_cast<uint32_t *>(cc_lds); /* [32-step group of the window][lane] */
    uint2 *cost2 = reinterpret_cast<uint2 *>(dec + cc_decode_groups(p) * 64u);
    const uint16_t *cost = reinterpret_cast<const uint16_t *>(cost2);

    /* the lane's state s' has the predecessors pred0 and pred0 + 1 and the hypothesised input s' >> 5 */
    const uint32_t pred0 = (lane << 1) & 63u, reg = (lane >> 5) << 6 | pred0;
    const uint16_t *cp0 = cost + cc_label(p, reg), *cp1 = cost + cc_label(p, reg | 1u);
    const int bp0 = (int)(pred0 * 4u), bp1 = bp0 + 4;

    /* step t0 + i's kept symbols lie at base[off], off counted from the window's first */
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

    uint32_t metric = t0 == 0u && start_state >= 0 && lane != (uint32_t)start_state ? CC_INF : 0u;
    int32_t v0, v1;
    fetch(lane, v0, v1);
    for (uint32_t cb = 0; cb < n; cb += 64u) {
        {
            const uint32_t a0 = (uint32_t)max(-v0, 0), a1 = (uint32_t)max(v0, 0);
            const uint32_t b0 = (uint32_t)max(-v1, 0), b1 = (uint32_t)max(v1, 0);
            cost2[lane] = make_uint2((a0 + b0) | (a1 + b0) << 16, (a0 + b1) | (a1 + b1) << 16);
        }
        __syncthreads();
        if (cb + 64u < n)
            fetch(cb + 64u + lane, v0, v1);
        uint32_t *dc = dec + (cb >> 5) * 64u + lane; /* the lane's word of the 32-step group */
        uint32_t own = 0u;                           /* step 32 k + j of a group at bit 31 - j */
        auto step = [&](uint32_t j) {
            const uint32_t m0 = (uint32_t)__builtin_amdgcn_ds_bpermute(bp0, (int)metric) + cp0[4u * j];
            const uint32_t m1 = (uint32_t)__builtin_amdgcn_ds_bpermute(bp1, (int)metric) + cp1[4u * j];
            const bool d = m1 < m0; /* a tie goes to d = 0 */
            metric = d ? m1 : m0;
            own = own + own + (d ? 1u : 0u);
        };
        if (n - cb >= 64u) {
#pragma unroll
            for (uint32_t j = 0; j < 32u; j++)
                step(j);
            dc[0] = own;
#pragma unroll
            for (uint32_t j = 32u; j < 64u; j++)
                step(j);
            dc[64] = own;
        } else {
            const uint32_t rem = n - cb;
            for (uint32_t j = 0; j < rem; j++) {
                step(j);
                if (j == 31u)
                    dc[0] = own;
            }
            if (rem & 31u)
                dc[(rem >> 5) * 64u] = own << (32u - (rem & 31u));
        }
        __syncthreads();
    }

    /* where the traceback starts */
    uint32_t S;
    if (t1 == nbits && end_state >= 0) {
        S = (uint32_t)end_state;
    } else {
        uint32_t mn = metric;
#pragma unroll
        for (int off = 32; off; off >>= 1)
            mn = min(mn, (uint32_t)__shfl_xor((int)mn, off));
        S = (uint32_t)__ffsll((unsigned long long)__ballot(metric == mn)) - 1u; /* the lowest such state */
    }
    S = (uint32_t)__builtin_amdgcn_readfirstlane((int)S);
    const uint32_t ms = (uint32_t)__shfl((int)metric, (int)S);
    if (metric_out && lane == 0u)
        metric_out[gb] = ms;

    /* window step i is step r = i - i0 of the block, whose own steps are [0, er); the walk ends at r = 0 */
    const int32_t i0 = (int32_t)(e0 - t0), er = (int32_t)(e1 - e0);
    uint64_t mine = 0u, acc = 0u;
    int32_t i = (int32_t)n - 1;
    uint32_t own = dec[(uint32_t)(i >> 5) * 64u + lane];
    for (; i >= i0; i--) {
        /* the step's 64 decisions: every lane's bit of it */
        const uint64_t word = __ballot((own >> (31u - ((uint32_t)i & 31u))) & 1u);
        const int32_t r = i - i0;
        acc |= (uint64_t)(S >> 5) << (r & 63); /* the bit of the step: bit 5 of the state after it */
        S = ((S << 1) | (uint32_t)((word >> S) & 1u)) & 63u;
        if ((r & 63) == 0) { /* steps r .. r + 63 are complete */
            if (r < er) {
                if (er - r < 64)
                    acc &= (1ull << (er - r)) - 1ull; /* the window's steps behind the block; a frame's spare bits */
                /* step j of the 64 -> bit 7 - j % 8 of byte j / 8 */
                const uint64_t out = __builtin_bswap64(__brevll(acc));
                if (lane == (uint32_t)(r >> 6))
                    mine = out;
            }
            acc = 0u;
        }
        if (((uint32_t)i & 31u) == 0u && i > i0)
            own = dec[(uint32_t)((i - 1) >> 5) * 64u + lane];
    }
    const int32_t left = er - 64 * (int32_t)lane;
    if (left > 0) {
        const uint32_t nb = left >= 64 ? 8u : (uint32_t)(left + 7) / 8u;
        uint8_t *o = bits + c * bs + e0 / 8u + 8u * lane;
        if (nb == 8u && !(reinterpret_cast<uintptr_t>(o) & 7u)) {
            *reinterpret_cast<uint64_t *>(o) = mine;
        } else {
            for (uint32_t i = 0; i < nb; i++)
                o[i] = (uint8_t)(mine >> (8u * i));
        }
    }
}

__global__ __launch_bounds__(CC_ENC_THREADS) void cc_encode_k(CcParams p, const uint8_t *bits, size_t bs, uint64_t nbits,
                                                              uint64_t symbols, uint64_t words, uint64_t first,
                                                              uint64_t total, int start_state, uint8_t *sym, size_t ss,
                                                              uint8_t *end_state)
{
    const uint64_t at = (uint64_t)blockIdx.x * CC_ENC_THREADS + threadIdx.x;
    if (at >= total)
        return;
    const uint64_t idx = first + at, c = idx / words, w = idx - c * words;
    const uint8_t *in = bits + c * bs;
    /* input bit t; the six before step 0 are start_state's, newest (t = -1) at bit 5 */
    auto bit = [&](int64_t t) -> uint32_t {
        return t < 0 ? ((uint32_t)start_state >> (uint32_t)(6 + t)) & 1u
                     : ((uint32_t)in[(uint64_t)t >> 3] >> (7u - ((uint32_t)t & 7u))) & 1u;
    };
    auto state_before = [&](uint64_t t) {
        uint32_t st = 0u;
#pragma unroll
        for (int k = 1; k <= 6; k++)
            st |= bit((int64_t)t - k) << (6 - k);
        return st;
    };
    if (w == 0u && end_state)
        end_state[c] = (uint8_t)state_before(nbits);
    const uint64_t m0 = w * 32u;
    if (m0 >= symbols)
        return;
    const uint32_t cnt = symbols - m0 < 32u ? (uint32_t)(symbols - m0) : 32u;
    /* the step and the output of symbol m0 */
    const uint64_t q = m0 / p.kept;
    uint32_t r = (uint32_t)(m0 - q * p.kept), ph = 0u;
    for (; ph < p.period; ph++) {
        const uint32_t k = ((p.keep0 >> ph) & 1u) + ((p.keep1 >> ph) & 1u);
        if (r < k)
            break;
        r -= k;
    }
    uint64_t t = q * p.period + ph;
    uint32_t st = state_before(t), word = 0u, got = 0u;
    while (got < cnt) { /* t < nbits: the frame has `symbols` symbols */
        const uint32_t reg = bit((int64_t)t) << 6 | st, lab = cc_label(p, reg);
        if (((p.keep0 >> ph) & 1u) && r == 0u)
            word |= (lab & 1u) << (31u - got++);
        if (((p.keep1 >> ph) & 1u) && got < cnt)
            word |= (lab >> 1) << (31u - got++);
        r = 0u;
        st = reg >> 1;
        t++;
        ph = ph + 1u == p.period ? 0u : ph + 1u;
    }
    const uint32_t nb = (cnt + 7u) / 8u;
    uint8_t *o = sym + c * ss + w * 4u;
    if (nb == 4u && !(reinterpret_cast<uintptr_t>(o) & 3u)) {
        *reinterpret_cast<uint32_t *>(o) = __builtin_bswap32(word);
    } else {
        for (uint32_t i = 0; i < nb; i++)
            o[i] = (uint8_t)(word >> (24u - 8u * i));
    }
}

extern "C" hipError_t cck_decode(const CcParams *p, const int8_t *llr, size_t llr_stride, uint64_t nbits, uint64_t blocks,
                                 uint64_t first, uint32_t n, int start_state, int end_state, uint8_t *bits,
                                 size_t bits_stride, uint32_t *metric, hipStream_t s)
{
    if (!p || !llr || !bits || !nbits || !blocks || n > 0x7FFFFFFFu || p->block % 64u || p->block < 64u ||
        p->block > CC_BLOCK_MAX || p->overlap > CC_OVERLAP_MAX || !p->period || p->period > CC_PERIOD_MAX || !p->kept)
        return hipErrorInvalidValue;
    if (n == 0u)
        return hipSuccess;
    hipLaunchKernelGGL(cc_decode_k, dim3(n), dim3(CC_STATES), cc_decode_lds(*p), s, *p, llr, llr_stride, nbits, blocks,
                       first, start_state, end_state, bits, bits_stride, metric);
    return hipGetLastError();
}

extern "C" hipError_t cck_encode(const CcParams *p, const uint8_t *bits, size_t bits_stride, uint64_t nbits,
                                 uint64_t symbols, uint64_t words, uint64_t first, uint64_t n, int start_state,
                                 uint8_t *sym, size_t sym_stride, uint8_t *end_state, hipStream_t s)
{
    const uint64_t grid = (n + CC_ENC_THREADS - 1u) / CC_ENC_THREADS;
    if (!p || !bits || !sym || !nbits || !words || grid > 0x7FFFFFFFu || !p->period || p->period > CC_PERIOD_MAX ||
        !p->kept || start_state < 0 || start_state > 63)
        return hipErrorInvalidValue;
    if (n == 0u)
        return hipSuccess;
    hipLaunchKernelGGL(cc_encode_k, dim3((uint32_t)grid), dim3(CC_ENC_THREADS), 0, s, *p, bits, bits_stride, nbits,
                       symbols, words, first, n, start_state, sym, sym_stride, end_state);
    return hipGetLastError();
}
