/*
 * rs_product.hip -- product-code blocks <-> codeword rows (gfx950).
 *
 * A block is n2 rows of n1 bytes, byte (i, j) at blocks + b*bstride + i*pitch
 * + j (poporon_amd.h).  Axis 0's codewords are the block's rows, axis 1's its
 * columns.  The codec kernels work on wire rows, w bytes back to back per
 * codeword, so a layout pass moves the block's bytes between its rows in the
 * caller's buffer -- runs of at most 255 bytes, `pitch` apart -- and the
 * staging rows, where codeword (b, c) lies at (b*cw + c)*w.
 *
 *   rs_prod_gather_k   blocks -> rows.  A workgroup of 256 lanes takes a tile:
 *                      g whole blocks when a block's codewords are small, else
 *                      the codewords [c0, c0 + u) of one block.  On axis 1
 *                      that is a run of u columns: block row i gives u bytes
 *                      at i*pitch + c0, the plane kernel's geometry
 *                      (rs_planes.hip) with the plane pointer computed and not
 *                      tabled.  On axis 0 it is the rows c0 .. c0 + u - 1
 *                      themselves.  A run is cut at the 16-byte boundaries of
 *                      its own address (rs_slot16.h); a lane takes one slot as
 *                      one uint4 load, four loads in flight, and puts its
 *                      bytes into the LDS image: down symbol column m of the
 *                      image on axis 1 (a step of w), side by side on axis 0.
 *                      The image IS the tile's staging rows.  Their run starts
 *                      at any byte, (b*cw + c0)*w, so the image sits in LDS at
 *                      that address mod 16: an LDS uint4 and a staging uint4
 *                      cover the same bytes, and the row side is a straight
 *                      uint4 copy with a byte path in the run's first and last
 *                      slot, which it shares with the neighbouring tiles.
 *   rs_prod_scatter_k  rows -> blocks, the same tile backwards.
 *   rs_prod_lists_k    the coupling of a decode schedule: one wave per block
 *                      compacts the other axis's dirty flags (at most 255) to
 *                      an ascending list by ballot and rank, applies the
 *                      threshold rule (poporon_amd.h) and writes the list and
 *                      its count for every codeword of the block.
 *   rs_prod_ok_k       d_block_ok[b] = no flag of block b is set.
 *
 * The gather loads a run's head and tail slot whole too when the 16 bytes lie
 * inside the chunk's blocks (first byte of the first block to the last byte of
 * the last): what it reads beside the run -- the neighbouring row's bytes, or
 * a pitch or stride gap -- is dropped, and only the very first and last slot
 * of a chunk go byte by byte.  The scatter never writes beside a run: a head
 * or tail slot goes out as the dwords that lie inside the run and the bytes
 * around them.
 *
 * Only the symbols [m0, m1) of a codeword move: the message on the way into
 * an encode, the parity on the way out, everything around a decode.  Image
 * bytes outside [m0, m1) of a gather are not initialised; the encoders that
 * follow such a gather overwrite them and the scatter takes only the parity.
 *
 * Lanes map to slots slot-major (item i = q*NR + r over the tile's NR runs):
 * neighbouring lanes take the same slot of neighbouring runs.  On axis 1 those
 * are neighbouring symbols of the same codewords, one byte apart in the image,
 * so the 32 lanes of an LDS group touch eight consecutive dwords at each of
 * the sixteen steps whatever w is.  Run-major, as the plane kernel has it, the
 * slots of one run lie 16 w bytes apart, and for a w that is a multiple of 8
 * (DVD's 208) every slot of a run falls on one bank.
 *
 * Every index inside a tile is 32 bits (the image is at most 32 KiB); offsets
 * into the blocks and the rows are size_t.  Nothing outside a block's n2 x n1
 * rectangle or the chunk's rows is written, and nothing outside the chunk's
 * blocks or rows is read.
 */
#include "rs_device.h"
#include "rs_slot16.h"

#define RS_PROD_THREADS 256
#define RS_PROD_BATCH 4u /* 16-byte global loads a lane keeps in flight */

struct RsProdArgs {
    uint8_t *rows;   /* the chunk's staging rows, 16-byte aligned */
    uint8_t *blocks; /* the chunk's first block */
    size_t pitch, bstride;
    size_t count;    /* blocks of the chunk */
    size_t span;     /* bytes from `blocks` to the end of the last codeword's last symbol */
    uint32_t axis;   /* 0: codewords are block rows, 1: block columns */
    uint32_t w;      /* bytes of a codeword */
    uint32_t cw;     /* codewords of a block in the rows */
    uint32_t g;      /* tpb == 1: whole blocks per tile */
    uint32_t u;      /* tpb > 1: codewords per tile */
    uint32_t tpb;    /* tiles per block */
    uint32_t m0, m1; /* the symbols that move */
    uint32_t s;      /* slots per run */
};

struct RsProdTile {
    size_t b0;       /* first block */
    uint32_t nb;     /* blocks */
    uint32_t c0, nc; /* codewords [c0, c0 + nc) of each */
    uint32_t nr, rpb; /* runs of the tile, runs per block */
    uint32_t len;    /* bytes of a run */
    uint32_t head;   /* the image's offset in LDS = its staging address mod 16 */
    uint32_t bytes;  /* bytes of the image */
    size_t off;      /* the image's offset in the rows */
};

static __device__ __forceinline__ bool prod_tile(const RsProdArgs &a, RsProdTile &t)
{
    if (a.tpb == 1u) {
        t.b0 = (size_t)blockIdx.x * a.g;
        if (t.b0 >= a.count)
            return false;
        t.nb = a.count - t.b0 < a.g ? (uint32_t)(a.count - t.b0) : a.g;
        t.c0 = 0u;
        t.nc = a.cw;
    } else {
        t.b0 = blockIdx.x / a.tpb;
        t.c0 = (blockIdx.x % a.tpb) * a.u;
        if (t.b0 >= a.count || t.c0 >= a.cw)
            return false;
        t.nb = 1u;
        t.nc = a.cw - t.c0 < a.u ? a.cw - t.c0 : a.u;
    }
    t.rpb = a.axis ? a.m1 - a.m0 : t.nc;
    t.len = a.axis ? t.nc : a.m1 - a.m0;
    t.nr = t.nb * t.rpb;
    t.off = (t.b0 * a.cw + t.c0) * a.w;
    t.head = (uint32_t)(t.off & 15u);
    t.bytes = t.nb * t.nc * a.w;
    return true;
}

/* run r of the tile: its address in the blocks, and where its byte 0 lies in the image; byte k lies `step` further */
static __device__ __forceinline__ uint8_t *prod_run(const RsProdArgs &a, const RsProdTile &t, uint32_t r, float inv_rpb,
                                                    uint32_t &img0)
{
    uint32_t bb, x;
    slot16_divmod(r, t.rpb, inv_rpb, bb, x);
    uint8_t *blk = a.blocks + (t.b0 + bb) * a.bstride;
    if (a.axis) {
        img0 = bb * a.cw * a.w + a.m0 + x;
        return blk + (size_t)(a.m0 + x) * a.pitch + t.c0;
    }
    img0 = (bb * a.cw + x) * a.w + a.m0;
    return blk + (size_t)(t.c0 + x) * a.pitch + a.m0;
}

__global__ __launch_bounds__(RS_PROD_THREADS) void rs_prod_gather_k(RsProdArgs a)
{
    extern __shared__ uint4 prod_lds[];
    RsProdTile t;
    if (!prod_tile(a, t))
        return;
    uint8_t *img = reinterpret_cast<uint8_t *>(prod_lds) + t.head;
    const int32_t step = a.axis ? (int32_t)a.w : 1;
    const float inv_nr = 1.0f / (float)t.nr, inv_rpb = 1.0f / (float)t.rpb;
    /* item i -> slot q = i / nr of run r = i mod nr; the tag is where the run's byte 0 lies in the image */
    slot16_batched<RS_PROD_THREADS, RS_PROD_BATCH>(
        t.nr * a.s,
        [&](uint32_t i, Slot16 &sl, uint4 &v) {
            uint32_t q, r;
            slot16_divmod(i, t.nr, inv_nr, q, r);
            const uint8_t *p = prod_run(a, t, r, inv_rpb, sl.tag);
            if (!slot16_part(p, t.len, q, sl.o0, sl.kb, sl.ke))
                return;
            if (p + sl.o0 >= a.blocks && p + sl.o0 + 16 <= a.blocks + a.span)
                v = *reinterpret_cast<const uint4 *>(p + sl.o0); /* a head or tail slot inside the blocks: whole */
            else
                v = slot16_load(p, sl.o0, sl.kb, sl.ke);
        },
        [&](const Slot16 &sl, const uint4 &v) {
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
            slot16_spread(img + (int32_t)sl.tag + sl.o0 * step, step, x, sl.kb, sl.ke); /* o0 < 0 only with kb > 0 */
        });
    __syncthreads();
    slot16_image_out<RS_PROD_THREADS>(a.rows + t.off, t.bytes, prod_lds);
}

__global__ __launch_bounds__(RS_PROD_THREADS) void rs_prod_scatter_k(RsProdArgs a)
{
    extern __shared__ uint4 prod_lds[];
    RsProdTile t;
    if (!prod_tile(a, t))
        return;
    slot16_image_in<RS_PROD_THREADS>(prod_lds, a.rows + t.off, t.bytes);
    __syncthreads();
    const uint8_t *img = reinterpret_cast<const uint8_t *>(prod_lds) + t.head;
    const int32_t step = a.axis ? (int32_t)a.w : 1;
    const uint32_t total = t.nr * a.s;
    const float inv_nr = 1.0f / (float)t.nr, inv_rpb = 1.0f / (float)t.rpb;
    for (uint32_t i = threadIdx.x; i < total; i += RS_PROD_THREADS) {
        uint32_t q, r, at, kb, ke;
        int32_t o0;
        slot16_divmod(i, t.nr, inv_nr, q, r);
        uint8_t *p = prod_run(a, t, r, inv_rpb, at);
        if (!slot16_part(p, t.len, q, o0, kb, ke))
            continue;
        const uint8_t *c = img + (int32_t)at + o0 * step;
        /* the collect is written out here, each branch ending in its own store: through slot16_collect this kernel
         * measured 3 to 8 % slower */
        uint32_t x[4] = {0u, 0u, 0u, 0u};
        if (kb == 0u && ke == 16u) { /* sixteen loads in flight and no branch */
#pragma unroll
            for (int32_t k = 0; k < 16; k++)
                x[k >> 2] |= (uint32_t)c[k * step] << (8 * (k & 3));
            *reinterpret_cast<uint4 *>(p + o0) = make_uint4(x[0], x[1], x[2], x[3]);
        } else { /* a run's head or tail: whole dwords where they lie inside the run, bytes around them */
#pragma unroll
            for (int32_t k = 0; k < 16; k++)
                if ((uint32_t)k >= kb && (uint32_t)k < ke)
                    x[k >> 2] |= (uint32_t)c[k * step] << (8 * (k & 3));
#pragma unroll
            for (uint32_t d = 0; d < 4u; d++) {
                if (kb <= 4u * d && 4u * d + 4u <= ke) {
                    *reinterpret_cast<uint32_t *>(p + o0 + (int32_t)(4u * d)) = x[d];
                } else {
#pragma unroll
                    for (uint32_t k = 4u * d; k < 4u * d + 4u; k++)
                        if (k >= kb && k < ke)
                            p[o0 + (int32_t)k] = (uint8_t)(x[d] >> (8u * (k & 3u)));
                }
            }
        }
    }
}

/* flags: nf per block, the other axis's; pos: cwa rows of `stride` bytes per block (a multiple of 16, <= 256) on a
 * 16-byte boundary; a wave per block */
__global__ __launch_bounds__(RS_PROD_THREADS) void rs_prod_lists_k(const uint8_t *flags, uint32_t nf, uint32_t ra,
                                                                   uint32_t cwa, uint8_t *pos, uint32_t stride,
                                                                   uint8_t *cnt, size_t nblocks)
{
    __shared__ uint4 row4[RS_PROD_THREADS / 64][16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint8_t *row = reinterpret_cast<uint8_t *>(row4[wave]);
    const uint32_t spr = stride / 16u, total = cwa * spr;
    for (size_t base = (size_t)blockIdx.x * 4u; base < nblocks; base += (size_t)gridDim.x * 4u) {
        const size_t b = base + wave;
        const bool active = b < nblocks;
        if (lane < 16u)
            row4[wave][lane] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        uint32_t n = 0u;
        for (uint32_t t0 = 0; t0 < 256u; t0 += 64u) {
            const uint32_t t = t0 + lane;
            const bool f = active && t < nf && flags[b * nf + t] != 0u;
            const unsigned long long m = __ballot(f);
            if (f)
                row[n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint8_t)t;
            n += (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (active) {
            const bool use = n > ra / 2u && n <= ra;
            uint4 *dst = reinterpret_cast<uint4 *>(pos) + b * total;
            for (uint32_t i = lane; i < total; i += 64u)
                dst[i] = use ? row4[wave][i % spr] : make_uint4(0u, 0u, 0u, 0u);
            for (uint32_t c = lane; c < cwa; c += 64u)
                cnt[b * cwa + c] = use ? (uint8_t)n : (uint8_t)0u;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RS_PROD_THREADS) void rs_prod_ok_k(const uint8_t *rowf, uint32_t n2, const uint8_t *colf,
                                                                uint32_t n1, uint8_t *ok, size_t nblocks)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (size_t base = (size_t)blockIdx.x * 4u; base < nblocks; base += (size_t)gridDim.x * 4u) {
        const size_t b = base + wave;
        if (b >= nblocks)
            continue;
        uint32_t any = 0u;
        for (uint32_t t = lane; t < n2; t += 64u)
            any |= rowf[b * n2 + t];
        for (uint32_t t = lane; t < n1; t += 64u)
            any |= colf[b * n1 + t];
        const unsigned long long m = __ballot(any != 0u);
        if (lane == 0u)
            ok[b] = m ? 0u : 1u;
    }
}

/* The tile of a layout pass over blocks of cw codewords of w bytes: g whole blocks while they fit RS_PROD_LDS_PACK
 * (small blocks keep every lane busy and the workgroups many), one block up to RS_PROD_LDS, else the block in tpb
 * tiles of u codewords, u a multiple of 16 and the tiles near equal. */
extern "C" bool rsk_prod_tile(uint32_t w, uint32_t cw, uint32_t *g, uint32_t *u, uint32_t *tpb)
{
    if (w == 0u || w > 255u || cw == 0u || cw > 255u)
        return false;
    const uint32_t per = w * cw;
    *g = 1u;
    *u = cw;
    *tpb = 1u;
    if (per <= RS_PROD_LDS_PACK) {
        *g = RS_PROD_LDS_PACK / per;
    } else if (per > RS_PROD_LDS) {
        const uint32_t umax = (RS_PROD_LDS / w) & ~15u; /* >= 128 */
        const uint32_t parts = (cw + umax - 1u) / umax;
        *u = ((cw + parts - 1u) / parts + 15u) & ~15u;
        *tpb = (cw + *u - 1u) / *u;
    }
    return true;
}

static hipError_t prod_launch(bool gather, uint8_t *blocks, size_t pitch, size_t bstride, size_t count, uint32_t axis,
                              uint32_t w, uint32_t cw, uint32_t m0, uint32_t m1, uint8_t *rows, hipStream_t s)
{
    RsProdArgs a;
    if (!rsk_prod_tile(w, cw, &a.g, &a.u, &a.tpb) || !blocks || !rows || (reinterpret_cast<uintptr_t>(rows) & 15u) ||
        m0 > m1 || m1 > w || axis > 1u)
        return hipErrorInvalidValue;
    if (count == 0 || m0 == m1)
        return hipSuccess;
    a.rows = rows;
    a.blocks = blocks;
    a.pitch = pitch;
    a.bstride = bstride;
    a.count = count;
    /* axis 1: w rows of cw columns move at the most; axis 0: cw rows of w */
    a.span = (count - 1u) * bstride + (size_t)((axis ? w : cw) - 1u) * pitch + (axis ? cw : w);
    a.axis = axis;
    a.w = w;
    a.cw = cw;
    a.m0 = m0;
    a.m1 = m1;
    const uint32_t lmax = axis ? a.u : m1 - m0; /* the longest run; at any alignment it spans (lmax + 30) / 16 slots */
    a.s = (lmax + 30u) / 16u;
    const size_t grid = a.tpb == 1u ? (count + a.g - 1u) / a.g : count * a.tpb;
    if (grid > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    const uint32_t lds = (a.g * a.u * w + 15u + 15u) & ~15u; /* the image behind a head of at most 15 bytes */
    if (gather)
        RS_LAUNCH(rs_prod_gather_k, dim3((uint32_t)grid), dim3(RS_PROD_THREADS), lds, s, a);
    else
        RS_LAUNCH(rs_prod_scatter_k, dim3((uint32_t)grid), dim3(RS_PROD_THREADS), lds, s, a);
    return hipGetLastError();
}

extern "C" hipError_t rsk_prod_gather(const uint8_t *blocks, size_t pitch, size_t bstride, size_t count, uint32_t axis,
                                      uint32_t w, uint32_t cw, uint32_t m0, uint32_t m1, uint8_t *rows, hipStream_t s)
{
    return prod_launch(true, const_cast<uint8_t *>(blocks), pitch, bstride, count, axis, w, cw, m0, m1, rows, s);
}

extern "C" hipError_t rsk_prod_scatter(const uint8_t *rows, uint8_t *blocks, size_t pitch, size_t bstride, size_t count,
                                       uint32_t axis, uint32_t w, uint32_t cw, uint32_t m0, uint32_t m1, hipStream_t s)
{
    return prod_launch(false, blocks, pitch, bstride, count, axis, w, cw, m0, m1, const_cast<uint8_t *>(rows), s);
}

extern "C" hipError_t rsk_prod_lists(const uint8_t *flags, uint32_t nf, uint32_t ra, uint32_t cwa, uint8_t *pos,
                                     uint32_t stride, uint8_t *cnt, size_t nblocks, hipStream_t s)
{
    if (!flags || !pos || !cnt || nf == 0u || nf > 255u || cwa == 0u || cwa > 255u || stride == 0u || stride > 256u ||
        (stride & 15u) || ra > stride || (reinterpret_cast<uintptr_t>(pos) & 15u))
        return hipErrorInvalidValue;
    if (nblocks == 0)
        return hipSuccess;
    const size_t want = (nblocks + 3u) / 4u;
    const uint32_t grid = (uint32_t)(want < 8192u ? want : 8192u);
    RS_LAUNCH(rs_prod_lists_k, dim3(grid), dim3(RS_PROD_THREADS), 0, s, flags, nf, ra, cwa, pos, stride, cnt, nblocks);
    return hipGetLastError();
}

extern "C" hipError_t rsk_prod_ok(const uint8_t *rowf, uint32_t n2, const uint8_t *colf, uint32_t n1, uint8_t *ok,
                                  size_t nblocks, hipStream_t s)
{
    if (!rowf || !colf || !ok)
        return hipErrorInvalidValue;
    if (nblocks == 0)
        return hipSuccess;
    const size_t want = (nblocks + 3u) / 4u;
    RS_LAUNCH(rs_prod_ok_k, dim3((uint32_t)(want < 8192u ? want : 8192u)), dim3(RS_PROD_THREADS), 0, s, rowf, n2, colf,
              n1, ok, nblocks);
    return hipGetLastError();
}
