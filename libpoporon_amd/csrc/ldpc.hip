/*
 * ldpc.hip -- LDPC batch encode, check and normalised min-sum decode for
 * gfx950, one workgroup per codeword (the reference: src/ldpc.c:635-778,
 * :925-1085 under ldpc_encode / ldpc_decode, src/encode.c:147-197,
 * src/decode.c:489-540).
 *
 * A workgroup of 256 lanes takes rows blockIdx.x, + gridDim.x, ...  The
 * graph (CSR rows, column view, interleaver tables) is read from device
 * memory and shared by every codeword.  The row's bits live in LDS as the
 * reference's byte image (bit i = byte i/8, mask 0x80 >> i%8).  Interleaving
 * is a gather through the host-built tables, whole output bytes per lane, so
 * no two lanes touch one byte.
 *
 * Decode keeps three int16 arrays per codeword: var_to_check and
 * check_to_var (one entry per edge) and llr_total (one per bit).  They sit
 * in LDS (ldpc_decode_k<true>) or in the workgroup's slice of a global
 * workspace (<false>).  One iteration is
 *   check update     a lane per check row: sign product, min1 / min2,
 *                    abs * 15 / 16, min2 to the edge that holds min1
 *   variable update  a lane per bit: channel + incoming in int32, saturated
 *                    to +/-32000; out = saturate(sum - incoming)
 *   syndrome         a lane per check row over the signs of llr_total
 * with a barrier between them.  All three are sums, minima and XORs over
 * fixed sets, so the integers equal the reference's sequential loops.  The
 * stop decision (__syncthreads_or) is uniform across the workgroup.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ldpc_device.h"
#include "rs_device.h" /* RS_LAUNCH */

#define L_WG 256
#define LLR_SAT 32000
#define LLR_HARD 30000

extern __shared__ __attribute__((aligned(16))) uint8_t ldpc_smem[];

/* bit k of the row [data | parity]; info_bits is a multiple of 8 */
__device__ static inline uint32_t row_bit(const LdpcDev &G, const uint8_t *d, const uint8_t *p, uint32_t k)
{
    const uint8_t b = k < G.info_bits ? d[k >> 3] : p[(k - G.info_bits) >> 3];
    return (b >> (7u - (k & 7u))) & 1u;
}

__device__ static inline uint32_t cw_bit(const uint8_t *cw, uint32_t k) { return (cw[k >> 3] >> (7u - (k & 7u))) & 1u; }

/* the received row, inner de-interleaved, into cw[codeword_bytes]: out bit i =
 * in bit forward[i] (deinterleave_bits scatters in[i] to inverse[i]); bits
 * past codeword_bits are 0.  Without the interleaver the bytes are copied,
 * spare bits of the last byte included, as the reference's memcpy does. */
__device__ static void load_codeword(const LdpcDev &G, const uint8_t *d, const uint8_t *p, uint8_t *cw)
{
    for (uint32_t b = threadIdx.x; b < G.codeword_bytes; b += L_WG) {
        uint32_t v = 0;
        if (!G.inner_forward) {
            v = b < G.info_bytes ? d[b] : p[b - G.info_bytes];
        } else {
            for (uint32_t k = 0; k < 8u; k++) {
                const uint32_t i = 8u * b + k;
                if (i < G.codeword_bits)
                    v |= row_bit(G, d, p, G.inner_forward[i]) << (7u - k);
            }
        }
        cw[b] = (uint8_t)v;
    }
}

/* nonzero when any check row of the byte image fails (a barrier; uniform) */
__device__ static int syndrome_bytes(const LdpcDev &G, const uint8_t *cw)
{
    uint32_t bad = 0;
    for (uint32_t r = threadIdx.x; r < G.num_checks; r += L_WG) {
        uint32_t x = 0;
        const uint32_t e1 = G.row_ptr[r + 1];
        for (uint32_t e = G.row_ptr[r]; e < e1; e++)
            x ^= cw_bit(cw, G.col_idx[e]);
        bad |= x;
    }
    return __syncthreads_or((int)bad);
}

__device__ static inline int sat(int v) { return v > LLR_SAT ? LLR_SAT : v < -LLR_SAT ? -LLR_SAT : v; }

/* ------------------------------------------------------------------------ */
/* encode                                                                   */
/* ------------------------------------------------------------------------ */

/* LDS: carry[L_WG] bytes, then the codeword's byte image */
__global__ __launch_bounds__(L_WG) void ldpc_encode_k(const LdpcDev G, uint8_t *data, size_t dstride, uint8_t *parity,
                                                      size_t pstride, size_t count)
{
    uint8_t *carry = ldpc_smem;
    uint8_t *cw = ldpc_smem + L_WG;
    uint8_t *cp = cw + G.info_bytes;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    /* the prefix pass gives every lane a run of whole parity bytes */
    const uint32_t run = (G.parity_bytes + L_WG - 1) / L_WG;
    const uint32_t b0 = min(tid * run, G.parity_bytes), b1 = min(b0 + run, G.parity_bytes);
    for (size_t c = blockIdx.x; c < count; c += gridDim.x) {
        uint8_t *d = data + c * dstride;
        uint8_t *p = parity + c * pstride;
        /* outer interleave: out[forward[i]] = in[i], gathered through the inverse */
        for (uint32_t k = tid; k < G.info_bytes; k += L_WG)
            cw[k] = d[G.outer_inverse ? G.outer_inverse[k] : k];
        __syncthreads();
        /* x_r = XOR of row r's info bits, a lane per row; a wave's 64 rows are
         * 8 parity bytes, packed from the ballot (row 8j is byte j's top bit) */
        for (uint32_t base = 0; base < G.parity_bits; base += L_WG) {
            const uint32_t r = base + tid;
            uint32_t x = 0;
            if (r < G.parity_bits) {
                const uint32_t e1 = G.row_ptr[r + 1];
                for (uint32_t e = G.row_ptr[r]; e < e1; e++) {
                    const uint32_t col = G.col_idx[e];
                    if (col < G.info_bits)
                        x ^= cw_bit(cw, col);
                }
            }
            const unsigned long long m = __ballot((int)x);
            const uint32_t byte = (base + (tid & ~63u)) / 8u + lane;
            if (lane < 8u && byte < G.parity_bytes)
                cp[byte] = (uint8_t)(__brev((uint32_t)(m >> (8u * lane)) & 0xFFu) >> 24);
        }
        __syncthreads();
        /* parity bit i = x_0 ^ ... ^ x_i (the dual diagonal): prefix XOR inside
         * each lane's run, then the carry of the runs before it */
        uint32_t acc = 0;
        for (uint32_t b = b0; b < b1; b++) {
            uint32_t v = cp[b];
            v ^= v >> 1;
            v ^= v >> 2;
            v ^= v >> 4;
            if (acc)
                v ^= 0xFFu;
            acc = v & 1u;
            cp[b] = (uint8_t)v;
        }
        carry[tid] = (uint8_t)acc;
        __syncthreads();
        uint32_t in = 0;
        for (uint32_t t = 0; t < tid; t++)
            in ^= carry[t];
        if (in)
            for (uint32_t b = b0; b < b1; b++)
                cp[b] ^= 0xFFu;
        __syncthreads();
        /* spare bits of the last parity byte are 0 */
        if (tid == 0 && (G.parity_bits & 7u))
            cp[G.parity_bytes - 1] &= (uint8_t)(0xFF00u >> (G.parity_bits & 7u));
        __syncthreads();
        if (G.inner_inverse) {
            /* inner interleave: out[forward[i]] = in[i]; data and parity both rewritten */
            for (uint32_t b = tid; b < G.codeword_bytes; b += L_WG) {
                uint32_t v = 0;
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t i = 8u * b + k;
                    if (i < G.codeword_bits)
                        v |= cw_bit(cw, G.inner_inverse[i]) << (7u - k);
                }
                if (b < G.info_bytes)
                    d[b] = (uint8_t)v;
                else
                    p[b - G.info_bytes] = (uint8_t)v;
            }
        } else {
            if (G.outer_inverse)
                for (uint32_t k = tid; k < G.info_bytes; k += L_WG)
                    d[k] = cw[k];
            for (uint32_t k = tid; k < G.parity_bytes; k += L_WG)
                p[k] = cp[k];
        }
        __syncthreads();
    }
}

/* ------------------------------------------------------------------------ */
/* check                                                                    */
/* ------------------------------------------------------------------------ */

__global__ __launch_bounds__(L_WG) void ldpc_check_k(const LdpcDev G, const uint8_t *data, size_t dstride,
                                                     const uint8_t *parity, size_t pstride, size_t count,
                                                     uint8_t *dirty)
{
    uint8_t *cw = ldpc_smem;
    for (size_t c = blockIdx.x; c < count; c += gridDim.x) {
        load_codeword(G, data + c * dstride, parity + c * pstride, cw);
        __syncthreads();
        const int bad = syndrome_bytes(G, cw);
        if (threadIdx.x == 0)
            dirty[c] = bad ? 1 : 0;
        __syncthreads();
    }
}

/* ------------------------------------------------------------------------ */
/* decode                                                                   */
/* ------------------------------------------------------------------------ */

/* messages per codeword, int16: var_to_check[E], check_to_var[E], llr_total[N] */
__host__ __device__ static inline size_t msg_bytes(const LdpcDev &G)
{
    return (((size_t)2 * G.num_edges + G.num_bits) * sizeof(int16_t) + 15) & ~(size_t)15;
}

template <bool LDS>
__global__ __launch_bounds__(L_WG) void ldpc_decode_k(const LdpcDev G, uint8_t *data, size_t dstride,
                                                      const uint8_t *parity, size_t pstride, const int8_t *llr,
                                                      size_t lstride, size_t count, uint8_t *ok_out,
                                                      uint32_t *iter_out, uint8_t *hard, size_t hstride,
                                                      uint32_t max_iter, uint8_t *ws)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t E = G.num_edges, N = G.num_bits;
    int16_t *v2c;
    uint8_t *cw;
    if (LDS) {
        v2c = reinterpret_cast<int16_t *>(ldpc_smem);
        cw = ldpc_smem + msg_bytes(G);
    } else {
        v2c = reinterpret_cast<int16_t *>(ws + (size_t)blockIdx.x * msg_bytes(G));
        cw = ldpc_smem;
    }
    int16_t *c2v = v2c + E;
    int16_t *tot = c2v + E;

    for (size_t c = blockIdx.x; c < count; c += gridDim.x) {
        uint8_t *d = data + c * dstride;
        const int8_t *l = llr ? llr + c * lstride : nullptr;
        bool ok = false, run = true;
        uint32_t iters = 0;
        if (!l) {
            /* hard path: a clean row leaves at iteration 0; else every bit starts at +/-30000 */
            load_codeword(G, d, parity + c * pstride, cw);
            __syncthreads();
            if (!syndrome_bytes(G, cw)) {
                ok = true;
                run = false;
            } else {
                for (uint32_t i = tid; i < N; i += L_WG)
                    tot[i] = cw_bit(cw, i) ? (int16_t)-LLR_HARD : (int16_t)LLR_HARD;
            }
        } else {
            /* soft path: the row's bits are not read; llr de-interleaved by gather */
            for (uint32_t i = tid; i < N; i += L_WG)
                tot[i] = (int16_t)sat((int)l[G.inner_forward ? G.inner_forward[i] : i] * 256);
        }
        if (run) { /* uniform */
            __syncthreads();
            for (uint32_t e = tid; e < E; e += L_WG)
                v2c[e] = tot[G.col_idx[e]];
            __syncthreads();
            iters = max_iter;
            for (uint32_t it = 0; it < max_iter; it++) {
                for (uint32_t r = tid; r < G.num_checks; r += L_WG) {
                    const uint32_t e0 = G.row_ptr[r], e1 = G.row_ptr[r + 1];
                    int min1 = LLR_SAT, min2 = LLR_SAT;
                    uint32_t at = 0, neg = 0;
                    for (uint32_t e = e0; e < e1; e++) {
                        const int m = v2c[e];
                        neg ^= (uint32_t)(m < 0);
                        const int a = m < 0 ? -m : m;
                        if (a < min1) {
                            min2 = min1;
                            min1 = a;
                            at = e;
                        } else if (a < min2) {
                            min2 = a;
                        }
                    }
                    const int a1 = min1 * 15 / 16, a2 = min2 * 15 / 16;
                    for (uint32_t e = e0; e < e1; e++) {
                        const int a = e == at ? a2 : a1;
                        c2v[e] = (int16_t)((neg ^ (uint32_t)(v2c[e] < 0)) ? -a : a);
                    }
                }
                __syncthreads();
                for (uint32_t i = tid; i < N; i += L_WG) {
                    /* channel: the llr again (unsaturated), or on the hard path the previous total */
                    int sum = l ? (int)l[G.inner_forward ? G.inner_forward[i] : i] * 256 : (int)tot[i];
                    const uint32_t j0 = G.col_ptr[i], j1 = G.col_ptr[i + 1];
                    for (uint32_t j = j0; j < j1; j++)
                        sum += c2v[G.edge_idx[j]];
                    tot[i] = (int16_t)sat(sum);
                    for (uint32_t j = j0; j < j1; j++) {
                        const uint32_t e = G.edge_idx[j];
                        v2c[e] = (int16_t)sat(sum - c2v[e]);
                    }
                }
                __syncthreads();
                uint32_t bad = 0;
                for (uint32_t r = tid; r < G.num_checks; r += L_WG) {
                    uint32_t x = 0;
                    const uint32_t e1 = G.row_ptr[r + 1];
                    for (uint32_t e = G.row_ptr[r]; e < e1; e++)
                        x ^= (uint32_t)(tot[G.col_idx[e]] < 0);
                    bad |= x;
                }
                if (!__syncthreads_or((int)bad)) {
                    ok = true;
                    iters = it + 1;
                    break;
                }
            }
            /* hard decisions of the last iteration */
            for (uint32_t b = tid; b < G.codeword_bytes; b += L_WG) {
                uint32_t v = 0;
                for (uint32_t k = 0; k < 8u; k++) {
                    const uint32_t i = 8u * b + k;
                    if (i < N && tot[i] < 0)
                        v |= 0x80u >> k;
                }
                cw[b] = (uint8_t)v;
            }
            __syncthreads();
        }
        if (tid == 0) {
            ok_out[c] = ok ? 1 : 0;
            if (iter_out)
                iter_out[c] = iters;
        }
        if (hard)
            for (uint32_t b = tid; b < G.codeword_bytes; b += L_WG)
                hard[c * hstride + b] = cw[b];
        if (ok) /* outer de-interleave: out[inverse[i]] = in[i]; a failed row keeps its data */
            for (uint32_t k = tid; k < G.info_bytes; k += L_WG)
                d[k] = cw[G.outer_forward ? G.outer_forward[k] : k];
        __syncthreads();
    }
}

/* ------------------------------------------------------------------------ */
/* launchers                                                                */
/* ------------------------------------------------------------------------ */

static size_t cw_lds(const LdpcDev *prm) { return ((size_t)prm->codeword_bytes + 15) & ~(size_t)15; }

extern "C" size_t ldpck_decode_lds_bytes(const LdpcDev *prm) { return msg_bytes(*prm) + cw_lds(prm); }
extern "C" size_t ldpck_slice_bytes(const LdpcDev *prm) { return msg_bytes(*prm); }

/* LDS the compiler gives ldpc_decode_k<true> on its own (__syncthreads_or keeps words there):
 * it comes out of the same 160 KiB as the dynamic bytes.  Nothing fits where it cannot be read. */
static size_t decode_static_lds()
{
    static const size_t bytes = [] {
        hipFuncAttributes a;
        if (hipFuncGetAttributes(&a, reinterpret_cast<const void *>(ldpc_decode_k<true>)) != hipSuccess)
            return (size_t)LDPC_LDS_MAX;
        return (size_t)a.sharedSizeBytes;
    }();
    return bytes;
}

extern "C" size_t ldpck_decode_lds_room(void) { return LDPC_LDS_MAX - std::min<size_t>(LDPC_LDS_MAX, decode_static_lds()); }

static uint32_t rows_grid(size_t count, size_t cap)
{
    return (uint32_t)std::max<size_t>(1, std::min(count, std::max<size_t>(cap, 1)));
}

extern "C" uint32_t ldpck_decode_grid(const LdpcDev *prm, size_t count, int num_cu, bool lds)
{
    const size_t cu = (size_t)(num_cu > 0 ? num_cu : 256);
    if (lds) /* as many workgroups per CU as its LDS and its 32 waves hold */
        return rows_grid(count, cu * std::min<size_t>(8, std::max<size_t>(1, LDPC_LDS_MAX / ldpck_decode_lds_bytes(prm))));
    /* global messages: the workspace stays below 512 MiB */
    return rows_grid(count, std::min<size_t>(cu * 4, ((size_t)512 << 20) / ldpck_slice_bytes(prm)));
}

/* more than 64 KiB of dynamic LDS has to be asked for once per kernel */
template <typename K> static hipError_t allow_lds(K kernel, size_t bytes)
{
    if (bytes <= 64u * 1024u)
        return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

extern "C" hipError_t ldpck_encode(const LdpcDev *prm, uint8_t *data, size_t dstride, uint8_t *parity, size_t pstride,
                                   size_t count, int num_cu, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    const size_t cu = (size_t)(num_cu > 0 ? num_cu : 256);
    RS_LAUNCH(ldpc_encode_k, dim3(rows_grid(count, cu * 8)), dim3(L_WG), L_WG + cw_lds(prm), stream, *prm, data,
              dstride, parity, pstride, count);
    return hipGetLastError();
}

extern "C" hipError_t ldpck_check(const LdpcDev *prm, const uint8_t *data, size_t dstride, const uint8_t *parity,
                                  size_t pstride, size_t count, uint8_t *dirty, int num_cu, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    const size_t cu = (size_t)(num_cu > 0 ? num_cu : 256);
    RS_LAUNCH(ldpc_check_k, dim3(rows_grid(count, cu * 8)), dim3(L_WG), cw_lds(prm), stream, *prm, data, dstride,
              parity, pstride, count, dirty);
    return hipGetLastError();
}

extern "C" hipError_t ldpck_decode(const LdpcDev *prm, uint8_t *data, size_t dstride, const uint8_t *parity,
                                   size_t pstride, const int8_t *llr, size_t lstride, size_t count, uint8_t *ok,
                                   uint32_t *iterations, uint8_t *hard, size_t hstride, uint32_t max_iterations,
                                   bool lds, uint8_t *ws, uint32_t grid, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    if (max_iterations == 0)
        max_iterations = 50; /* src/ldpc.c:981-983 */
    if (lds) {
        const size_t bytes = ldpck_decode_lds_bytes(prm);
        if (bytes > ldpck_decode_lds_room())
            return hipErrorInvalidValue;
        const hipError_t e = allow_lds(ldpc_decode_k<true>, bytes);
        if (e != hipSuccess)
            return e;
        RS_LAUNCH(ldpc_decode_k<true>, dim3(grid), dim3(L_WG), bytes, stream, *prm, data, dstride, parity, pstride,
                  llr, lstride, count, ok, iterations, hard, hstride, max_iterations, (uint8_t *)nullptr);
    } else {
        if (!ws)
            return hipErrorInvalidValue;
        RS_LAUNCH(ldpc_decode_k<false>, dim3(grid), dim3(L_WG), cw_lds(prm), stream, *prm, data, dstride, parity,
                  pstride, llr, lstride, count, ok, iterations, hard, hstride, max_iterations, ws);
    }
    return hipGetLastError();
}
