/*
 * rs_planes.hip -- plane layout <-> codeword rows (gfx950).
 *
 * A stripe is W = size + nr planes, each a buffer of its own; codeword c has
 * symbol j at plane[j][c] (storage shards: poporon_amd.h).  The codec kernels
 * work on wire rows, W bytes back to back per codeword, so a layout pass is a
 * W x count byte transpose between W far-apart runs and one contiguous run.
 *
 *   rs_plane_gather_k   planes -> rows.  A workgroup of 256 lanes takes a tile
 *                       of T consecutive codewords [t0, t0 + T).  On the plane
 *                       side that is W runs of T bytes: each is cut at the
 *                       16-byte boundaries of its own address (rs_slot16.h), a
 *                       lane takes one slot (plane j, codewords o0 .. o0 + 15)
 *                       as one uint4 load, four loads in flight, and writes its
 *                       bytes down column j of the LDS image.  The image IS
 *                       the tile's rows (byte (c, j) at c*W + j), so the row
 *                       side is a straight copy: the run starts on a 16-byte
 *                       boundary (rows 16-byte aligned, t0 a multiple of 16)
 *                       and goes out as uint4, the last tile's tail as bytes.
 *                       Planes outside [first, last), lost planes and NULL
 *                       entries are never read: their columns are zero-filled.
 *   rs_plane_scatter_k  rows -> planes, the same tile backwards: the run into
 *                       LDS as uint4, then a lane puts together one 16-byte
 *                       slot of a plane from column j and stores it whole, or
 *                       byte by byte at a run's head and tail.  Planes outside
 *                       [first, last) and NULL entries are not written.
 *   rs_plane_lists_k    the erasure lists of a rebuild: every codeword gets
 *                       the same list, the set bits of the lost mask ascending
 *                       and zeros behind them, and the same count.
 *
 * <true> (ALIGNED): every plane run of the chunk starts on a 16-byte boundary
 * (decided once on the host), so a run of T bytes is T/16 whole slots; the
 * head arithmetic and the extra slot per plane are gone, and only the last
 * tile of a count that is no multiple of 16 has a partial slot.
 *
 * The table of W pointers and the 256-bit lost mask travel by value in the
 * kernel arguments (2,120 bytes of HIP's 4 KiB): no device table, no copy.
 *
 * Lanes map to slots plane by plane (item i = j*S + q, S slots per run), so a
 * wave's 64 loads cover whole 128-byte lines of a few planes.  LDS banking of
 * the byte side: at step k lane (j, q) touches byte (16 q + k) W + j.  The
 * slots of one plane lie 16 W bytes = 4 W dwords apart, so for odd W (255: 28
 * mod 32) eight neighbouring slots fall on eight banks 4 apart and the up to
 * four planes of a 32-lane group share a dword; W = 14: bank step 24, 2-way;
 * a W that is a multiple of 8 puts every slot of a plane on one bank (8-way
 * at T = 128).  The byte accesses were measured, not tuned: DESIGN section 16.
 *
 * Every index inside a tile is 32 bits (T W <= 32 KiB); the tile's offsets
 * into the planes and the rows are size_t.  Nothing outside [base, base +
 * count) of a plane or outside the chunk's rows is read or written.
 */
#include "rs_device.h"
#include "rs_slot16.h"

#define RS_PLANE_THREADS 256
#define RS_PLANE_BATCH 4u /* 16-byte global loads a lane keeps in flight */

struct RsPlaneArgs {
    uint8_t *rows;         /* the chunk's wire rows, 16-byte aligned */
    size_t base;           /* the chunk's first codeword within the planes */
    size_t count;          /* codewords of the chunk */
    uint32_t w, tile;      /* planes; codewords per workgroup (a multiple of 16) */
    uint32_t first, last;  /* the planes that move */
    float inv;             /* 1 / slots per plane run */
    uint32_t lost[8];      /* gather: planes never read */
    uint8_t *plane[255];
};

struct RsPlaneLost {
    uint32_t m[8];
};

/* the part [kb, ke) of slot q of a plane run of len bytes at p that lies inside it (p NULL: a run on a boundary) */
template <bool AL>
static __device__ __forceinline__ bool plane_slot(const uint8_t *p, uint32_t len, uint32_t q, int32_t &o0, uint32_t &kb,
                                                  uint32_t &ke)
{
    return AL ? slot16_part_aligned(len, q, o0, kb, ke) : slot16_part(p, len, q, o0, kb, ke);
}

template <bool AL> __global__ __launch_bounds__(RS_PLANE_THREADS) void rs_plane_gather_k(RsPlaneArgs a)
{
    extern __shared__ uint4 plane_lds[];
    uint8_t *img = reinterpret_cast<uint8_t *>(plane_lds);
    const size_t t0 = (size_t)blockIdx.x * a.tile;
    if (t0 >= a.count)
        return;
    const uint32_t tc = a.count - t0 < a.tile ? (uint32_t)(a.count - t0) : a.tile;
    const uint32_t s = a.tile / 16u + (AL ? 0u : 1u);
    /* item i -> plane j = i / s (the tag), slot q = i mod s; a plane that is not read gives zeros */
    slot16_batched<RS_PLANE_THREADS, RS_PLANE_BATCH>(
        a.w * s,
        [&](uint32_t i, Slot16 &sl, uint4 &v) {
            uint32_t j, q;
            slot16_divmod(i, s, a.inv, j, q);
            sl.tag = j;
            const uint8_t *p = nullptr;
            if (j >= a.first && j < a.last && !((a.lost[j >> 5] >> (j & 31u)) & 1u) && a.plane[j])
                p = a.plane[j] + a.base + t0;
            if (plane_slot<AL>(p, tc, q, sl.o0, sl.kb, sl.ke))
                v = p ? slot16_load(p, sl.o0, sl.kb, sl.ke) : make_uint4(0u, 0u, 0u, 0u);
        },
        [&](const Slot16 &sl, const uint4 &v) {
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
            /* down column j of the image; o0 < 0 only with kb > 0 */
            slot16_spread(img + sl.o0 * (int32_t)a.w + (int32_t)sl.tag, (int32_t)a.w, x, sl.kb, sl.ke);
        });
    __syncthreads();
    slot16_image_out<RS_PLANE_THREADS>(a.rows + t0 * a.w, tc * a.w, plane_lds);
}

template <bool AL> __global__ __launch_bounds__(RS_PLANE_THREADS) void rs_plane_scatter_k(RsPlaneArgs a)
{
    extern __shared__ uint4 plane_lds[];
    const uint8_t *img = reinterpret_cast<const uint8_t *>(plane_lds);
    const size_t t0 = (size_t)blockIdx.x * a.tile;
    if (t0 >= a.count)
        return;
    const uint32_t tc = a.count - t0 < a.tile ? (uint32_t)(a.count - t0) : a.tile;
    slot16_image_in<RS_PLANE_THREADS>(plane_lds, a.rows + t0 * a.w, tc * a.w);
    __syncthreads();
    const uint32_t s = a.tile / 16u + (AL ? 0u : 1u), total = (a.last - a.first) * s;
    for (uint32_t i = threadIdx.x; i < total; i += RS_PLANE_THREADS) {
        uint32_t j, q, kb, ke, x[4];
        int32_t o0;
        slot16_divmod(i, s, a.inv, j, q);
        j += a.first;
        if (!a.plane[j])
            continue;
        uint8_t *p = a.plane[j] + a.base + t0;
        if (!plane_slot<AL>(p, tc, q, o0, kb, ke))
            continue;
        slot16_collect(x, img + o0 * (int32_t)a.w + (int32_t)j, (int32_t)a.w, kb, ke);
        slot16_store(p, o0, kb, ke, x);
    }
}

/* pos: n rows of `stride` bytes (a multiple of 16, <= 256) on a 16-byte boundary */
__global__ __launch_bounds__(RS_PLANE_THREADS) void rs_plane_lists_k(RsPlaneLost l, uint32_t lost_count, uint8_t *pos,
                                                                     uint32_t stride, uint8_t *cnt, size_t n)
{
    __shared__ uint4 row4[16];
    uint8_t *row = reinterpret_cast<uint8_t *>(row4);
    const uint32_t t = threadIdx.x;
    row[t] = 0u;
    __syncthreads();
    if ((l.m[t >> 5] >> (t & 31u)) & 1u) {
        uint32_t rank = __popc(l.m[t >> 5] & ((1u << (t & 31u)) - 1u));
        for (uint32_t k = 0; k < (t >> 5); k++)
            rank += __popc(l.m[k]);
        row[rank] = (uint8_t)t;
    }
    __syncthreads();
    const uint32_t spr = stride / 16u;
    const size_t slots = n * spr, step = (size_t)gridDim.x * RS_PLANE_THREADS;
    for (size_t i = (size_t)blockIdx.x * RS_PLANE_THREADS + t; i < slots; i += step)
        reinterpret_cast<uint4 *>(pos)[i] = row4[i % spr];
    for (size_t c = (size_t)blockIdx.x * RS_PLANE_THREADS + t; c < n; c += step)
        cnt[c] = (uint8_t)lost_count;
}

/* Codewords per workgroup for rows of w bytes: the image of T rows within RS_PLANE_LDS, T a multiple of 16, at
 * most RS_PLANE_TILE_MAX, which leaves 2^20 codewords of a narrow code 2,048 workgroups, eight per compute unit
 * (all the waves a CU holds); 0 for a w that is no row. */
extern "C" uint32_t rsk_plane_tile(uint32_t w)
{
    if (w == 0u || w > 255u)
        return 0u;
    const uint32_t fit = (RS_PLANE_LDS / w) & ~15u;
    return fit < RS_PLANE_TILE_MAX ? fit : RS_PLANE_TILE_MAX;
}

static hipError_t plane_launch(bool gather, uint8_t *const *planes, const uint32_t *lost, uint32_t w, uint32_t first,
                               uint32_t last, size_t base, uint8_t *rows, size_t count, bool aligned, hipStream_t s)
{
    const uint32_t t = rsk_plane_tile(w);
    if (t == 0u || !planes || !rows || (reinterpret_cast<uintptr_t>(rows) & 15u) || first > last || last > w)
        return hipErrorInvalidValue;
    if (count == 0 || first == last)
        return hipSuccess;
    RsPlaneArgs a;
    a.rows = rows;
    a.base = base;
    a.count = count;
    a.w = w;
    a.tile = t;
    a.first = first;
    a.last = last;
    a.inv = 1.0f / (float)(t / 16u + (aligned ? 0u : 1u));
    for (uint32_t k = 0; k < 8u; k++)
        a.lost[k] = lost ? lost[k] : 0u;
    for (uint32_t j = 0; j < 255u; j++)
        a.plane[j] = j < w ? planes[j] : nullptr;
    const size_t grid = (count + t - 1u) / t;
    if (grid > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    const uint32_t lds = (t * w + 15u) & ~15u;
    if (gather && aligned)
        RS_LAUNCH(rs_plane_gather_k<true>, dim3((uint32_t)grid), dim3(RS_PLANE_THREADS), lds, s, a);
    else if (gather)
        RS_LAUNCH(rs_plane_gather_k<false>, dim3((uint32_t)grid), dim3(RS_PLANE_THREADS), lds, s, a);
    else if (aligned)
        RS_LAUNCH(rs_plane_scatter_k<true>, dim3((uint32_t)grid), dim3(RS_PLANE_THREADS), lds, s, a);
    else
        RS_LAUNCH(rs_plane_scatter_k<false>, dim3((uint32_t)grid), dim3(RS_PLANE_THREADS), lds, s, a);
    return hipGetLastError();
}

extern "C" hipError_t rsk_plane_gather(const uint8_t *const *planes, const uint32_t *lost, uint32_t w, uint32_t first,
                                       uint32_t last, size_t base, uint8_t *rows, size_t count, bool aligned,
                                       hipStream_t s)
{
    return plane_launch(true, const_cast<uint8_t *const *>(planes), lost, w, first, last, base, rows, count, aligned, s);
}

extern "C" hipError_t rsk_plane_scatter(const uint8_t *rows, uint8_t *const *planes, uint32_t w, uint32_t first,
                                        uint32_t last, size_t base, size_t count, bool aligned, hipStream_t s)
{
    return plane_launch(false, planes, nullptr, w, first, last, base, const_cast<uint8_t *>(rows), count, aligned, s);
}

extern "C" hipError_t rsk_plane_lists(const uint32_t *lost, uint32_t lost_count, uint8_t *pos, uint32_t stride,
                                      uint8_t *cnt, size_t n, hipStream_t s)
{
    if (!lost || !pos || !cnt || stride == 0u || stride > 256u || (stride & 15u) ||
        (reinterpret_cast<uintptr_t>(pos) & 15u))
        return hipErrorInvalidValue;
    if (n == 0)
        return hipSuccess;
    RsPlaneLost l;
    for (uint32_t k = 0; k < 8u; k++)
        l.m[k] = lost[k];
    const size_t want = (n * (stride / 16u) + RS_PLANE_THREADS - 1u) / RS_PLANE_THREADS;
    const uint32_t grid = (uint32_t)(want < 4096u ? want : 4096u);
    RS_LAUNCH(rs_plane_lists_k, dim3(grid), dim3(RS_PLANE_THREADS), 0, s, l, lost_count, pos, stride, cnt, n);
    return hipGetLastError();
}
