/*
 * rs_conv.hip -- Forney convolutional interleaver streams <-> codeword rows
 * (gfx950).
 *
 * The interleaver has I branches, branch b a FIFO of b*M bytes (DVB: I = 12,
 * M = 17; ATSC: I = 52, M = 4).  With the code bytes of a batch numbered
 * serially, n = c*W + s (codeword c, symbol s, W = size + nr), byte n travels
 * on branch b = (phase + n) mod I and leaves at stream offset
 *
 *     p(n) = n + b*D,   D = M*I.
 *
 * D is a multiple of I, so p alone gives the branch back: b = (phase + p) mod
 * I, n = p - b*D.  A batch of `count` codewords occupies a span of count*W + H
 * bytes, H = (I-1)*D; the H offsets whose n falls outside [0, count*W) are
 * holes, bytes of the codewords before and after the batch, never written.
 *
 *   rs_conv_gather_k    stream -> rows.  A workgroup of 256 lanes takes a tile
 *                       of T consecutive codewords.  Their bytes lie in the
 *                       stream window [c0*W, (c0+T)*W + H): it is loaded into
 *                       LDS as 16-byte slots of the stream's own address
 *                       (rs_slot16.h; four loads in flight per lane), and the
 *                       rows are written from LDS through p(n), a 16-byte
 *                       slot of a row region per lane.  Neighbouring tiles
 *                       re-read H bytes each.
 *   rs_conv_scatter_k   rows -> stream.  A workgroup owns P contiguous bytes
 *                       of the stream, cut at the 16-byte boundaries of the
 *                       stream's address.  The bytes it needs are the serial
 *                       numbers [p0 - H, p1): the whole rows that hold them
 *                       are loaded into LDS, and each lane puts together one
 *                       16-byte slot of the stream through n(p).  A slot that
 *                       holds no hole and lies inside the span is one uint4
 *                       store, any other is stored byte by byte over the
 *                       bytes the call owns.  Holes exist only in the first
 *                       and last H bytes of the span.
 *   rs_conv_gather_direct_k, rs_conv_scatter_direct_k
 *                       the plain path for geometries whose window does not
 *                       fit the LDS (H up to 4.1 MB): a lane takes a 16-byte
 *                       slot of a row region and reads or writes the stream
 *                       byte by byte at p(n).
 *
 * Row regions: codeword c's message is `size` bytes at data + c*ds, its
 * parity nr bytes at par + c*ps (par NULL: no parity region; those symbols are
 * not delivered, their stream bytes not written).  Wire rows (par = data +
 * size, both strides W) are one run of bytes per tile, so that only the tile's
 * first and last slot are partial; any other placement is cut per region.
 *
 * The branch of a slot's first byte is one reciprocal multiplication
 * (slot16_divmod); from byte to byte branch and index are stepped: no division in
 * the inner step.  Everything inside a workgroup's window is indexed in 32
 * bits relative to the window; the window's own offset is size_t.
 *
 * LDS banking of the byte side: consecutive lanes hold slots 16 serial bytes
 * apart, so their k-th bytes lie 16 + (16 mod I)*D bytes apart in the window
 * image (minus I*D on a wrap).  DVB (I 12, D 204): the branch takes three
 * values 4 apart, byte addresses 16 l + 816 (l mod 3), dword banks 4 l + 12
 * (l mod 3) mod 32: eight banks among 32 lanes, 4-way.  ATSC (I 52, D 208):
 * 16 + 16*208 = 3344 B = 836 dwords = 4 mod 32, again eight banks, 4-way.  At
 * 4-way a ds_read_u8 wave-instruction takes 8 LDS cycles for 64 bytes: 8 B per
 * clock and CU, 4.9 TB/s over the chip, above what HBM leaves a kernel that
 * reads and writes every byte (3 TB/s each way).
 */
#include "rs_device.h"
#include "rs_slot16.h"

#define RS_CONV_THREADS 256
#define RS_CONV_BATCH 4u /* 16-byte global loads a lane keeps in flight */

struct RsConvArgs {
    uint8_t *data, *par; /* row regions; par NULL: none */
    size_t ds, ps;
    uint8_t *stream;     /* span offset 0 */
    size_t count;        /* codewords */
    uint32_t size, nr;
    uint32_t nb, d;      /* I and D = M*I */
    uint32_t phase;
    uint32_t tile;       /* gather and the direct kernels: codewords per workgroup; scatter: stream bytes */
    uint32_t wire;       /* rows are wire rows: one run per tile */
    float inv;           /* 1 / I */
};

/* the 16-byte slots of the row regions of codewords [c0, c0 + tc): slot idx of
 * `total` is the part [kb, ke) of the slot at p + o0, whose first byte inside
 * has serial number nrel relative to c0*W */
struct ConvRows {
    uint32_t w, tc, nq_d, nq_p, n_d, total;
    bool wire;
};

static __device__ __forceinline__ ConvRows conv_rows(const RsConvArgs &a, uint32_t tc)
{
    ConvRows r;
    r.w = a.size + a.nr;
    r.tc = tc;
    r.wire = a.wire != 0u;
    if (r.wire) {
        r.nq_d = tc * r.w / 16u + 2u;
        r.n_d = r.nq_d;
        r.nq_p = 0u;
    } else {
        r.nq_d = a.size / 16u + 2u;
        r.n_d = tc * r.nq_d;
        r.nq_p = a.par ? a.nr / 16u + 2u : 0u;
    }
    r.total = r.n_d + tc * r.nq_p;
    return r;
}

static __device__ __forceinline__ bool conv_rows_slot(const RsConvArgs &a, const ConvRows &r, size_t c0, uint32_t idx,
                                                      uint8_t *&p, int32_t &o0, uint32_t &kb, uint32_t &ke,
                                                      uint32_t &nrel)
{
    uint32_t len, q, base;
    if (r.wire) {
        p = a.data + c0 * r.w;
        len = r.tc * r.w;
        q = idx;
        base = 0u;
    } else if (idx < r.n_d) {
        const uint32_t row = idx / r.nq_d;
        q = idx - row * r.nq_d;
        p = a.data + (c0 + row) * a.ds;
        len = a.size;
        base = row * r.w;
    } else {
        const uint32_t row = (idx - r.n_d) / r.nq_p;
        q = idx - r.n_d - row * r.nq_p;
        p = a.par + (c0 + row) * a.ps;
        len = a.nr;
        base = row * r.w + a.size;
    }
    if (!slot16_part(p, len, q, o0, kb, ke))
        return false;
    nrel = base + (uint32_t)(o0 + (int32_t)kb);
    return true;
}

/* rows out of a window image: byte nrel of the tile at src[nrel + b*D], b = (ph0 + nrel) mod I.  src is the LDS image
 * (gather) or the stream itself at the tile's first byte (direct gather). */
static __device__ __forceinline__ void conv_rows_out(const RsConvArgs &a, const uint8_t *src, size_t c0, uint32_t tc,
                                                     uint32_t ph0)
{
    const ConvRows r = conv_rows(a, tc);
    const uint32_t step = a.d + 1u, back = a.nb * a.d;
    for (uint32_t idx = threadIdx.x; idx < r.total; idx += RS_CONV_THREADS) {
        uint8_t *p;
        int32_t o0;
        uint32_t kb, ke, nrel;
        if (!conv_rows_slot(a, r, c0, idx, p, o0, kb, ke, nrel))
            continue;
        uint32_t turn, b;
        slot16_divmod(ph0 + nrel, a.nb, a.inv, turn, b);
        uint32_t i = nrel + b * a.d;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            if (k >= kb && k < ke) {
                w[k >> 2] |= (uint32_t)src[i] << (8u * (k & 3u));
                i += step;
                if (++b == a.nb) {
                    b = 0u;
                    i -= back;
                }
            }
        }
        slot16_store(p, o0, kb, ke, w);
    }
}

/* the tile of workgroup blockIdx.x: its first codeword, how many, and the branch of its first byte */
static __device__ __forceinline__ bool conv_tile(const RsConvArgs &a, size_t &c0, uint32_t &tc, uint32_t &ph0)
{
    c0 = (size_t)blockIdx.x * a.tile;
    if (c0 >= a.count)
        return false;
    tc = a.count - c0 < a.tile ? (uint32_t)(a.count - c0) : a.tile;
    ph0 = (uint32_t)((a.phase + c0 * (a.size + a.nr)) % a.nb);
    return true;
}

__global__ __launch_bounds__(RS_CONV_THREADS) void rs_conv_gather_k(RsConvArgs a)
{
    extern __shared__ uint4 conv_lds[];
    size_t c0;
    uint32_t tc, ph0;
    if (!conv_tile(a, c0, tc, ph0))
        return;
    const uint32_t w = a.size + a.nr, len = tc * w + (a.nb - 1u) * a.d; /* the window */
    const uint8_t *run = a.stream + c0 * w;
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u);
    const uint32_t nq = (head + len + 15u) / 16u;
    /* a partial slot goes to LDS whole: the bytes outside the window are copies of bytes inside it, and are not used */
    slot16_batched<RS_CONV_THREADS, RS_CONV_BATCH>(
        nq,
        [&](uint32_t q, Slot16 &sl, uint4 &v) {
            sl.tag = q;
            if (slot16_part(run, len, q, sl.o0, sl.kb, sl.ke))
                v = slot16_load(run, sl.o0, sl.kb, sl.ke);
        },
        [&](const Slot16 &sl, const uint4 &v) { conv_lds[sl.tag] = v; });
    __syncthreads();
    conv_rows_out(a, reinterpret_cast<const uint8_t *>(conv_lds) + head, c0, tc, ph0);
}

__global__ __launch_bounds__(RS_CONV_THREADS) void rs_conv_gather_direct_k(RsConvArgs a)
{
    size_t c0;
    uint32_t tc, ph0;
    if (!conv_tile(a, c0, tc, ph0))
        return;
    conv_rows_out(a, a.stream + c0 * (a.size + a.nr), c0, tc, ph0);
}

/* rows -> stream, a row-region slot per lane, the stream byte by byte: every byte written is a p(n) of the call */
__global__ __launch_bounds__(RS_CONV_THREADS) void rs_conv_scatter_direct_k(RsConvArgs a)
{
    size_t c0;
    uint32_t tc, ph0;
    if (!conv_tile(a, c0, tc, ph0))
        return;
    const ConvRows r = conv_rows(a, tc);
    uint8_t *dst = a.stream + c0 * r.w;
    const uint32_t step = a.d + 1u, back = a.nb * a.d;
    for (uint32_t idx = threadIdx.x; idx < r.total; idx += RS_CONV_THREADS) {
        uint8_t *p;
        int32_t o0;
        uint32_t kb, ke, nrel;
        if (!conv_rows_slot(a, r, c0, idx, p, o0, kb, ke, nrel))
            continue;
        const uint4 v = slot16_load(p, o0, kb, ke);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t turn, b;
        slot16_divmod(ph0 + nrel, a.nb, a.inv, turn, b);
        uint32_t i = nrel + b * a.d;
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            if (k >= kb && k < ke) {
                dst[i] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
                i += step;
                if (++b == a.nb) {
                    b = 0u;
                    i -= back;
                }
            }
        }
    }
}

__global__ __launch_bounds__(RS_CONV_THREADS) void rs_conv_scatter_k(RsConvArgs a)
{
    extern __shared__ uint4 conv_lds[];
    const uint32_t w = a.size + a.nr;
    const size_t h = (size_t)(a.nb - 1u) * a.d, nw = a.count * w, span = nw + h;
    const uint32_t shead = (uint32_t)(reinterpret_cast<uintptr_t>(a.stream) & 15u);
    /* the piece [pa, pa + tile) of span offsets starts on a 16-byte boundary of the stream's address; the call owns
     * [plo, phi) of it */
    const int64_t pa = (int64_t)((size_t)blockIdx.x * a.tile) - (int64_t)shead;
    const size_t plo = pa < 0 ? 0 : (size_t)pa;
    const size_t phi = (size_t)(pa + (int64_t)a.tile) < span ? (size_t)(pa + (int64_t)a.tile) : span;
    if (plo >= phi)
        return;
    /* the serial numbers that land in it, and the whole rows [ca, cb) that hold them */
    const size_t nlo = plo > h ? plo - h : 0, nhi = phi < nw ? phi : nw;
    if (nlo >= nhi)
        return; /* holes only */
    const size_t ca = nlo / w, cb = (nhi + w - 1u) / w;
    const uint32_t tc = (uint32_t)(cb - ca), rows_len = tc * w;
    const size_t nbase = ca * w;
    /* rows into LDS: byte nrel of the rows at LDS byte lh + nrel; wire rows are one run copied slot by slot */
    const ConvRows r = conv_rows(a, tc);
    const uint32_t lh = r.wire ? (uint32_t)(reinterpret_cast<uintptr_t>(a.data + nbase) & 15u) : 0u;
    uint8_t *lds = reinterpret_cast<uint8_t *>(conv_lds) + lh;
    slot16_batched<RS_CONV_THREADS, RS_CONV_BATCH>(
        r.total,
        [&](uint32_t idx, Slot16 &sl, uint4 &v) {
            uint8_t *p;
            if (conv_rows_slot(a, r, ca, idx, p, sl.o0, sl.kb, sl.ke, sl.tag)) /* the tag: nrel */
                v = slot16_load(p, sl.o0, sl.kb, sl.ke);
        },
        [&](const Slot16 &sl, const uint4 &v) {
            if (sl.kb == 0u && sl.ke == 16u && ((lh + sl.tag) & 15u) == 0u) {
                *reinterpret_cast<uint4 *>(lds + sl.tag) = v;
            } else {
                const uint32_t x[4] = {v.x, v.y, v.z, v.w};
                slot16_spread(lds + sl.tag - sl.kb, 1, x, sl.kb, sl.ke); /* byte kb is serial number nrel */
            }
        });
    __syncthreads();
    /* the stream out: offset p holds serial number p - b*D, b = (phase + p) mod I; a hole where that is outside the
     * batch, and where it is a parity symbol without a parity region */
    const uint32_t ph0 = (uint32_t)((a.phase + nbase) % a.nb);
    const uint32_t back = a.nb * a.d;
    const bool nopar = a.par == nullptr;
    uint8_t *piece = a.stream + pa; /* 16-byte aligned; never dereferenced outside [plo, phi) */
    const int64_t lo = (int64_t)plo - pa, hi = (int64_t)phi - pa;
    for (uint32_t q = threadIdx.x; q < a.tile / 16u; q += RS_CONV_THREADS) {
        const int32_t s0 = (int32_t)(q * 16u);
        if (s0 + 16 <= lo || s0 >= hi)
            continue;
        const uint32_t kb = s0 < lo ? (uint32_t)(lo - s0) : 0u, ke = hi - s0 < 16 ? (uint32_t)(hi - s0) : 16u;
        const uint32_t prel = (uint32_t)(pa + s0 + (int64_t)kb - (int64_t)nbase); /* >= 0: nbase <= plo */
        uint32_t turn, b;
        slot16_divmod(ph0 + prel, a.nb, a.inv, turn, b);
        int32_t n = (int32_t)prel - (int32_t)(b * a.d);
        uint32_t x[4] = {0u, 0u, 0u, 0u}, ok = 0u;
        /* offsets [H, count*W) hold no hole: a whole slot there (all but the two ends of the span) is 16 bytes of
         * the rows, each inside the image, and one store */
        const int64_t p0 = pa + s0;
        if (kb == 0u && ke == 16u && !nopar && p0 >= (int64_t)h && p0 + 16 <= (int64_t)nw) {
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++) {
                x[k >> 2] |= (uint32_t)lds[n] << (8u * (k & 3u));
                n += 1 - (int32_t)a.d;
                if (++b == a.nb) {
                    b = 0u;
                    n += (int32_t)back;
                }
            }
            *reinterpret_cast<uint4 *>(piece + s0) = make_uint4(x[0], x[1], x[2], x[3]);
            continue;
        }
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            if (k >= kb && k < ke) {
                bool in = n >= 0 && n < (int32_t)rows_len;
                if (in && nopar) {
                    uint32_t row, sym;
                    slot16_divmod((uint32_t)n, w, 1.0f / (float)w, row, sym);
                    in = sym < a.size;
                }
                if (in) {
                    x[k >> 2] |= (uint32_t)lds[n] << (8u * (k & 3u));
                    ok |= 1u << k;
                }
                n += 1 - (int32_t)a.d;
                if (++b == a.nb) {
                    b = 0u;
                    n += (int32_t)back;
                }
            }
        }
        if (ok == 0xFFFFu) {
            *reinterpret_cast<uint4 *>(piece + s0) = make_uint4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++)
                if (ok & (1u << k))
                    piece[s0 + (int32_t)k] = (uint8_t)(x[k >> 2] >> (8u * (k & 3u)));
        }
    }
}

/* Codewords per workgroup of the tile kernels for rows of w bytes: enough that the H bytes a tile re-reads are at
 * most a quarter of its own (at least RS_CONV_TILE_MIN), as far as RS_CONV_LDS holds window and slack; 0 where not
 * even one row fits (the direct kernels take such a geometry). */
extern "C" uint32_t rsk_conv_tile(uint32_t w, uint32_t branches, uint32_t cell)
{
    if (w == 0u || w > 255u || branches < 1u || branches > RS_CONV_MAX_BRANCHES || cell < 1u ||
        cell > RS_CONV_MAX_CELL)
        return 0u;
    const uint64_t h = (uint64_t)(branches - 1u) * cell * branches;
    const uint64_t fixed = h + 2u * w + RS_CONV_LDS_SLACK;
    if (fixed + w > RS_CONV_LDS)
        return 0u;
    const uint64_t fit = (RS_CONV_LDS - fixed) / w, quarter = (4u * h + w - 1u) / w;
    const uint64_t want = quarter > RS_CONV_TILE_MIN ? quarter : RS_CONV_TILE_MIN;
    return (uint32_t)(want < fit ? want : fit);
}

static hipError_t conv_launch(bool gather, uint8_t *stream, uint32_t branches, uint32_t cell, uint32_t phase,
                              uint8_t *data, size_t ds, uint8_t *par, size_t ps, uint32_t size, uint32_t nr,
                              size_t count, int path, hipStream_t s)
{
    const uint32_t w = size + nr;
    if (size == 0u || w > 255u || branches < 1u || branches > RS_CONV_MAX_BRANCHES || cell < 1u ||
        cell > RS_CONV_MAX_CELL || phase >= branches || !stream || !data || ds < size || (par && ps < nr))
        return hipErrorInvalidValue;
    const uint32_t t = rsk_conv_tile(w, branches, cell);
    if (path == RS_CONV_PATH_TILE && t == 0u)
        return hipErrorInvalidConfiguration;
    const bool tile = path != RS_CONV_PATH_DIRECT && t != 0u;
    if (count == 0)
        return hipSuccess;
    RsConvArgs a;
    a.data = data;
    a.par = par;
    a.ds = ds;
    a.ps = ps;
    a.stream = stream;
    a.count = count;
    a.size = size;
    a.nr = nr;
    a.nb = branches;
    a.d = cell * branches;
    a.phase = phase;
    a.wire = par == data + size && ds == w && ps == w ? 1u : 0u;
    a.inv = 1.0f / (float)branches;
    const size_t h = (size_t)(branches - 1u) * a.d;
    size_t grid;
    uint32_t lds = 0u;
    if (tile) {
        lds = (uint32_t)((t * w + h + 2u * w + RS_CONV_LDS_SLACK + 15u) & ~(size_t)15);
        if (gather) {
            a.tile = t;
            grid = (count + t - 1u) / t;
        } else {
            a.tile = t * w >= 16u ? (t * w) & ~15u : 16u;
            grid = (count * w + h + 15u + a.tile - 1u) / a.tile; /* 15: the stream's address within its slot */
        }
    } else {
        a.tile = RS_CONV_TILE_MIN;
        grid = (count + a.tile - 1u) / a.tile;
    }
    if (grid > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    if (tile && gather)
        RS_LAUNCH(rs_conv_gather_k, dim3((uint32_t)grid), dim3(RS_CONV_THREADS), lds, s, a);
    else if (tile)
        RS_LAUNCH(rs_conv_scatter_k, dim3((uint32_t)grid), dim3(RS_CONV_THREADS), lds, s, a);
    else if (gather)
        RS_LAUNCH(rs_conv_gather_direct_k, dim3((uint32_t)grid), dim3(RS_CONV_THREADS), 0, s, a);
    else
        RS_LAUNCH(rs_conv_scatter_direct_k, dim3((uint32_t)grid), dim3(RS_CONV_THREADS), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t rsk_conv_gather(const uint8_t *stream, uint32_t branches, uint32_t cell, uint32_t phase,
                                      uint8_t *data, size_t ds, uint8_t *parity, size_t ps, uint32_t size, uint32_t nr,
                                      size_t count, int path, hipStream_t s)
{
    return conv_launch(true, const_cast<uint8_t *>(stream), branches, cell, phase, data, ds, parity, ps, size, nr,
                       count, path, s);
}

extern "C" hipError_t rsk_conv_scatter(const uint8_t *data, size_t ds, const uint8_t *parity, size_t ps, uint32_t size,
                                       uint32_t nr, size_t count, uint32_t branches, uint32_t cell, uint32_t phase,
                                       uint8_t *stream, int path, hipStream_t s)
{
    return conv_launch(false, stream, branches, cell, phase, const_cast<uint8_t *>(data), ds,
                       const_cast<uint8_t *>(parity), ps, size, nr, count, path, s);
}
