/*
 * rs_interleave.hip -- symbol-interleaved frames <-> codeword rows (gfx950).
 *
 * A frame of depth D holds D codewords of W = size + nr symbols: byte j*D + i
 * of its message region is message symbol j of codeword i, byte p*D + i of its
 * parity region parity symbol p.  The codec kernels take rows, so the
 * interleaved entry points (api.cpp) move a chunk of frames into a staging
 * buffer of wire rows (W bytes back to back, parity at byte `size`: the row
 * layout the codec kernels are measured on, and the one their block apply
 * takes), run the row kernels there and move the results back:
 *
 *   rs_ilv_gather_k   frames -> rows   (message only, or message and parity)
 *   rs_ilv_scatter_k  rows -> frames   (parity only, or message and parity)
 *
 * Both are byte-matrix transposes [W][D] <-> [D][W] per frame.  A workgroup
 * of 256 lanes takes a tile of whole frames whose rows fit RS_ILV_LDS bytes
 * of LDS, so that several groups share a CU.
 *
 * Both sides of a tile are contiguous runs of bytes at any alignment: a
 * frame's region, and the tile's rows in the staging buffer.  A run is cut at
 * the 16-byte boundaries of its own address: a lane takes one 16-byte slot,
 * as one uint4 access when the slot lies inside the run, byte by byte over
 * the part inside it at the run's head and tail (nothing outside a run is
 * read or written).
 *
 * LDS holds the image of the tile's staging rows, byte t of the run at LDS
 * byte (run address & 15) + t, so a 16-byte slot of the run is a 16-byte
 * aligned slot of LDS and the row side is uint4 copies (ds_read_b128 /
 * ds_write_b128, consecutive lanes on consecutive slots).  On the frame side
 * the 16 bytes of a slot go to / come from LDS one by one at the transposed
 * index r*W + j.  The byte accesses bank as dword accesses do, (a / 4) mod 32
 * within a 32-lane half, and the lanes of a half hold 32 consecutive slots,
 * 512 bytes of a region.  For D = 4, 8 and 16 their k-th bytes are one
 * codeword's symbols 4, 2 and 1 apart: one row, consecutive dwords (1, 2 and
 * 4 lanes per dword).  For D = 64 they fall in four rows 16 apart, 16 W bytes:
 * with W = 255 that is 1020 dwords, banks 0, 28, 24 and 20, two or three
 * dwords each, so they meet on no bank; the row pitch W is the padding (an
 * odd W never puts rows 16 apart on one bank; a shortened code whose W is a
 * multiple of 8 does, up to 4-way at D = 64).
 *
 * Wire form (poporon_amd_set_wire_form): the mapped variants
 * rs_ilv_gather_map_k / rs_ilv_scatter_map_k are the same bodies compiled with
 * MAP = true.  The byte step on the frame side then goes through a 256-byte
 * table held in LDS beside the tile (to_code on the way in, to_wire on the way
 * out), and the gather XORs each 16-byte frame slot with the 16 bytes of the
 * receive sequence that fall on it before the lookup.  The sequence comes from
 * a device image ext[i] = seq[i mod xlen], i < xlen + 20: a slot whose first
 * byte has block offset b takes ext[b mod xlen .. + 16), one division per slot
 * and five aligned dword loads, shifted into place.  With MAP = false the
 * bodies pass an empty struct around and nothing of this is compiled in.
 */
#include "rs_device.h"
#include "rs_slot16.h"

#define RS_ILV_THREADS 256
#define RS_ILV_BATCH 4u /* 16-byte global loads a lane keeps in flight */

/* what the mapped variants add: the LDS table, the sequence image (xlen 0:
 * none) and the block offset of the region's first byte; nothing without a
 * form, so that the plain kernels pass nothing */
template <bool MAP> struct IlvWire {
};
template <> struct IlvWire<true> {
    const uint8_t *lut;
    const uint32_t *ext;
    uint32_t xlen, boff;
};

/* the 16 sequence bytes on the slot whose byte 0 has block offset boff + o0
 * (o0 >= -15: the head slot starts before the region) */
static __device__ __forceinline__ uint4 ilv_seq16(const IlvWire<true> &wf, int32_t o0)
{
    const uint32_t ph = (uint32_t)((int32_t)(wf.boff + 16u * wf.xlen) + o0) % wf.xlen;
    const uint32_t *e = wf.ext + (ph >> 2);
    const uint32_t sh = 8u * (ph & 3u);
    uint32_t d[5], w[4];
#pragma unroll
    for (uint32_t i = 0; i < 5u; i++)
        d[i] = e[i];
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++)
        w[i] = (uint32_t)((((uint64_t)d[i + 1u] << 32) | d[i]) >> sh);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* frames -> LDS rows (row pitch `pitch` bytes): region of nsym symbols per
 * codeword (nsym * depth bytes per frame, `stride` apart), LDS columns col0 ..
 * col0 + nsym.  A lane loads RS_ILV_BATCH slots before it spreads the first:
 * the loads' latency is paid once per batch, not once per slot. */
template <bool MAP>
static __device__ void ilv_region_in(uint8_t *lds, uint32_t pitch, const uint8_t *reg, size_t stride, uint32_t nsym,
                                     uint32_t depth, uint32_t col0, uint32_t f0, uint32_t fc, IlvWire<MAP> wf)
{
    const uint32_t len = nsym * depth;
    const uint32_t nq = len / 16u + 2u; /* slots a region can touch at the worst alignment */
    slot16_batched<RS_ILV_THREADS, RS_ILV_BATCH>(
        fc * nq,
        [&](uint32_t idx, Slot16 &sl, uint4 &v) {
            sl.tag = idx / nq; /* the frame within the tile */
            const uint8_t *p = reg + (size_t)(f0 + sl.tag) * stride;
            if (!slot16_part(p, len, idx - sl.tag * nq, sl.o0, sl.kb, sl.ke))
                return;
            v = slot16_load(p, sl.o0, sl.kb, sl.ke);
            if constexpr (MAP) {
                if (wf.xlen) {
                    const uint4 x = ilv_seq16(wf, sl.o0);
                    v = make_uint4(v.x ^ x.x, v.y ^ x.y, v.z ^ x.z, v.w ^ x.w);
                }
            }
        },
        [&](const Slot16 &sl, const uint4 &v) {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint32_t o = (uint32_t)(sl.o0 + (int32_t)sl.kb);
            uint32_t j = o / depth, i = o - j * depth;
            const uint32_t r0 = sl.tag * depth;
#pragma unroll
            for (uint32_t k = 0; k < 16u; k++) {
                if (k >= sl.kb && k < sl.ke) {
                    uint8_t b = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
                    if constexpr (MAP)
                        b = wf.lut[b];
                    lds[(r0 + i) * pitch + col0 + j] = b;
                    if (++i == depth) {
                        i = 0u;
                        j++;
                    }
                }
            }
        });
}

/* LDS rows -> frames, the same walk */
template <bool MAP>
static __device__ void ilv_region_out(const uint8_t *lds, uint32_t pitch, uint8_t *reg, size_t stride, uint32_t nsym,
                                      uint32_t depth, uint32_t col0, uint32_t f0, uint32_t fc, IlvWire<MAP> wf)
{
    const uint32_t len = nsym * depth;
    const uint32_t nq = len / 16u + 2u;
    for (uint32_t idx = threadIdx.x; idx < fc * nq; idx += RS_ILV_THREADS) {
        const uint32_t fi = idx / nq, q = idx - fi * nq;
        uint8_t *p = reg + (size_t)(f0 + fi) * stride;
        int32_t o0;
        uint32_t kb, ke;
        if (!slot16_part(p, len, q, o0, kb, ke))
            continue;
        const uint32_t o = (uint32_t)(o0 + (int32_t)kb);
        uint32_t j = o / depth, i = o - j * depth;
        const uint32_t r0 = fi * depth;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            if (k >= kb && k < ke) {
                if constexpr (MAP)
                    w[k >> 2] |= (uint32_t)wf.lut[lds[(r0 + i) * pitch + col0 + j]] << (8u * (k & 3u));
                else
                    w[k >> 2] |= (uint32_t)lds[(r0 + i) * pitch + col0 + j] << (8u * (k & 3u));
                if (++i == depth) {
                    i = 0u;
                    j++;
                }
            }
        }
        slot16_store(p, o0, kb, ke, w);
    }
}

struct RsIlvArgs {
    uint8_t *data, *parity; /* frame f's regions at data + f * dstride, parity + f * pstride */
    size_t dstride, pstride;
    uint8_t *rows;          /* staging: row c at rows + c * (size + nr), c = f * depth + i */
    uint32_t size, nr, depth;
    uint32_t nframes;       /* frames of this launch */
    uint32_t tile;          /* frames per workgroup */
    uint32_t both;          /* gather: the parity region too; scatter: the message region too */
};

/* the mapped variants' arguments: the handle's device image, to_code at byte
 * 0, to_wire at byte 256, the sequence image from byte 512 (xlen 0: none) */
struct RsIlvMapArgs {
    RsIlvArgs a;
    const uint8_t *wire;
    uint32_t xlen;
};

/* 256 table bytes from global memory into LDS, a dword per lane */
static __device__ __forceinline__ void ilv_lut_in(uint32_t *lut, const uint8_t *tab)
{
    if (threadIdx.x < 64u)
        lut[threadIdx.x] = reinterpret_cast<const uint32_t *>(tab)[threadIdx.x];
}

template <bool MAP>
static __device__ __forceinline__ void ilv_gather_body(uint4 *lds128, const RsIlvArgs &a, IlvWire<MAP> wf)
{
    const uint32_t f0 = blockIdx.x * a.tile;
    if (f0 >= a.nframes)
        return;
    const uint32_t fc = a.nframes - f0 < a.tile ? a.nframes - f0 : a.tile;
    const uint32_t w = a.size + a.nr, len = fc * a.depth * w;
    uint8_t *run = a.rows + (size_t)f0 * a.depth * w; /* the tile's rows */
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u);
    uint8_t *lds = reinterpret_cast<uint8_t *>(lds128) + head;
    ilv_region_in<MAP>(lds, w, a.data, a.dstride, a.size, a.depth, 0u, f0, fc, wf);
    if constexpr (MAP)
        wf.boff = a.size * a.depth; /* wire-block order wherever the parity region lies */
    if (a.both)
        ilv_region_in<MAP>(lds, w, a.parity, a.pstride, a.nr, a.depth, a.size, f0, fc, wf);
    __syncthreads();
    /* rows out (without the parity region its columns carry whatever LDS held:
     * they are the rows' own bytes, which the encode then writes) */
    slot16_image_out<RS_ILV_THREADS>(run, len, lds128);
}

__global__ __launch_bounds__(RS_ILV_THREADS) void rs_ilv_gather_k(RsIlvArgs a)
{
    __shared__ uint4 lds128[RS_ILV_LDS / 16];
    ilv_gather_body<false>(lds128, a, IlvWire<false>{});
}

__global__ __launch_bounds__(RS_ILV_THREADS) void rs_ilv_gather_map_k(RsIlvMapArgs m)
{
    __shared__ uint4 lds128[RS_ILV_LDS / 16];
    __shared__ uint32_t lut[64];
    ilv_lut_in(lut, m.wire);
    __syncthreads();
    ilv_gather_body<true>(lds128, m.a,
                          IlvWire<true>{reinterpret_cast<const uint8_t *>(lut),
                                        reinterpret_cast<const uint32_t *>(m.wire + 512), m.xlen, 0u});
}

template <bool MAP>
static __device__ __forceinline__ void ilv_scatter_body(uint4 *lds128, const RsIlvArgs &a, IlvWire<MAP> wf)
{
    const uint32_t f0 = blockIdx.x * a.tile;
    if (f0 >= a.nframes)
        return;
    const uint32_t fc = a.nframes - f0 < a.tile ? a.nframes - f0 : a.tile;
    const uint32_t w = a.size + a.nr, len = fc * a.depth * w;
    const uint8_t *run = a.rows + (size_t)f0 * a.depth * w;
    const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u);
    uint8_t *lds = reinterpret_cast<uint8_t *>(lds128) + head;
    /* rows in, RS_ILV_BATCH loads in flight per lane; parity only: the slots
     * that hold message bytes alone are passed by */
    const uint32_t nq = (head + len + 15u) / 16u;
    slot16_batched<RS_ILV_THREADS, RS_ILV_BATCH>(
        nq,
        [&](uint32_t q, Slot16 &sl, uint4 &v) {
            sl.tag = q;
            if (!slot16_part(run, len, q, sl.o0, sl.kb, sl.ke))
                return;
            if (!a.both && (uint32_t)(sl.o0 + (int32_t)sl.kb) % w + (sl.ke - sl.kb) <= a.size)
                sl.kb = sl.ke = 0u;
            else
                v = slot16_load(run, sl.o0, sl.kb, sl.ke);
        },
        [&](const Slot16 &sl, const uint4 &v) {
            if (sl.kb == 0u && sl.ke == 16u) {
                lds128[sl.tag] = v;
            } else {
                const uint32_t x[4] = {v.x, v.y, v.z, v.w};
                slot16_spread(lds + sl.o0, 1, x, sl.kb, sl.ke);
            }
        });
    __syncthreads();
    if (a.both)
        ilv_region_out<MAP>(lds, w, a.data, a.dstride, a.size, a.depth, 0u, f0, fc, wf);
    ilv_region_out<MAP>(lds, w, a.parity, a.pstride, a.nr, a.depth, a.size, f0, fc, wf);
}

__global__ __launch_bounds__(RS_ILV_THREADS) void rs_ilv_scatter_k(RsIlvArgs a)
{
    __shared__ uint4 lds128[RS_ILV_LDS / 16];
    ilv_scatter_body<false>(lds128, a, IlvWire<false>{});
}

/* the table is read after the body's barrier between rows in and frames out */
__global__ __launch_bounds__(RS_ILV_THREADS) void rs_ilv_scatter_map_k(RsIlvMapArgs m)
{
    __shared__ uint4 lds128[RS_ILV_LDS / 16];
    __shared__ uint32_t lut[64];
    ilv_lut_in(lut, m.wire + 256);
    ilv_scatter_body<true>(lds128, m.a, IlvWire<true>{reinterpret_cast<const uint8_t *>(lut), nullptr, 0u, 0u});
}

/* whole frames per workgroup for a code of w = size + nr symbols at `depth`:
 * their rows, and up to 15 bytes of alignment before them, in RS_ILV_LDS bytes
 * (one frame of 64 rows of 255 symbols: 16,320 B) */
static bool ilv_tile(uint32_t w, uint32_t depth, uint32_t &tile)
{
    if (w == 0u || w > RS_ILV_ROW - 1u || depth == 0u || depth > RS_ILV_MAX_DEPTH)
        return false;
    tile = (RS_ILV_LDS - 16u) / (w * depth);
    return tile >= 1u;
}

static hipError_t ilv_launch(bool gather, uint8_t *data, size_t dstride, uint8_t *parity, size_t pstride, uint8_t *rows,
                             uint32_t size, uint32_t nr, uint32_t depth, size_t nframes, bool both,
                             const uint8_t *wire, uint32_t xlen, hipStream_t stream)
{
    RsIlvArgs a;
    a.data = data;
    a.parity = parity;
    a.dstride = dstride;
    a.pstride = pstride;
    a.rows = rows;
    a.size = size;
    a.nr = nr;
    a.depth = depth;
    a.both = both ? 1u : 0u;
    if (!ilv_tile(size + nr, depth, a.tile) || nframes > 0x7FFFFFFFu / RS_ILV_MAX_DEPTH)
        return hipErrorInvalidValue;
    if (nframes == 0)
        return hipSuccess;
    a.nframes = (uint32_t)nframes;
    const uint32_t grid = (a.nframes + a.tile - 1u) / a.tile;
    if (wire) {
        const RsIlvMapArgs m = {a, wire, xlen};
        if (gather)
            RS_LAUNCH(rs_ilv_gather_map_k, dim3(grid), dim3(RS_ILV_THREADS), 0, stream, m);
        else
            RS_LAUNCH(rs_ilv_scatter_map_k, dim3(grid), dim3(RS_ILV_THREADS), 0, stream, m);
    } else if (gather) {
        RS_LAUNCH(rs_ilv_gather_k, dim3(grid), dim3(RS_ILV_THREADS), 0, stream, a);
    } else {
        RS_LAUNCH(rs_ilv_scatter_k, dim3(grid), dim3(RS_ILV_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}

extern "C" hipError_t rsk_ilv_gather(const uint8_t *data, size_t dstride, const uint8_t *parity, size_t pstride,
                                     uint8_t *rows, uint32_t size, uint32_t nr, uint32_t depth, size_t nframes,
                                     bool with_parity, hipStream_t stream)
{
    return ilv_launch(true, const_cast<uint8_t *>(data), dstride, const_cast<uint8_t *>(parity), pstride, rows, size,
                      nr, depth, nframes, with_parity, nullptr, 0u, stream);
}

extern "C" hipError_t rsk_ilv_scatter(const uint8_t *rows, uint8_t *data, size_t dstride, uint8_t *parity,
                                      size_t pstride, uint32_t size, uint32_t nr, uint32_t depth, size_t nframes,
                                      bool with_data, hipStream_t stream)
{
    return ilv_launch(false, data, dstride, parity, pstride, const_cast<uint8_t *>(rows), size, nr, depth, nframes,
                      with_data, nullptr, 0u, stream);
}

/* the mapped variants; `wire` is RS_ILV_WIRE_BYTES(xlen) bytes of device memory
 * (rs_device.h), xlen 0 for no sequence (an encode passes 0) */
extern "C" hipError_t rsk_ilv_gather_map(const uint8_t *data, size_t dstride, const uint8_t *parity, size_t pstride,
                                         uint8_t *rows, uint32_t size, uint32_t nr, uint32_t depth, size_t nframes,
                                         bool with_parity, const uint8_t *wire, uint32_t xlen, hipStream_t stream)
{
    if (!wire || xlen > RS_ILV_XOR_MAX)
        return hipErrorInvalidValue;
    return ilv_launch(true, const_cast<uint8_t *>(data), dstride, const_cast<uint8_t *>(parity), pstride, rows, size,
                      nr, depth, nframes, with_parity, wire, xlen, stream);
}

extern "C" hipError_t rsk_ilv_scatter_map(const uint8_t *rows, uint8_t *data, size_t dstride, uint8_t *parity,
                                          size_t pstride, uint32_t size, uint32_t nr, uint32_t depth, size_t nframes,
                                          bool with_data, const uint8_t *wire, hipStream_t stream)
{
    if (!wire)
        return hipErrorInvalidValue;
    return ilv_launch(false, data, dstride, parity, pstride, const_cast<uint8_t *>(rows), size, nr, depth, nframes,
                      with_data, wire, 0u, stream);
}
