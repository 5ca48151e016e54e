/*
 * rs_report.hip -- sparse bytes of codeword-shaped regions -> ascending lists (gfx950).
 *
 * Two callers (api.cpp), one problem: compact the few non-zero bytes of a
 * region of `w` bytes per codeword into a list of at most nr entries per
 * codeword, ascending by position, the slots behind the count zero.
 *
 *   rs_snapshot_k    strided rows -> wire rows (size + nr bytes back to back) in
 *                    the handle's snapshot buffer, before a decode
 *   rs_report_k      rows after the decode against the snapshot: the bytes the
 *                    decode changed, as positions and before ^ after
 *   rs_mask_lists_k  a per-symbol flag plane in the layout of the (possibly
 *                    interleaved) message regions -> erasure lists and counts
 *
 * rs_report_k and rs_mask_lists_k share one shape.  A workgroup of 256 lanes
 * takes a tile of whole codewords (frames), in three phases:
 *
 *  1 the tile streams into LDS.  Both kernels read *runs*: contiguous bytes at
 *    any alignment (the tile's wire rows; a tile of contiguous frames, or one
 *    frame of a strided plane).  A run is cut at the 16-byte boundaries of its
 *    own address, a lane takes one slot as one uint4 load (the slots at a run's
 *    two ends, byte by byte over the part inside it: two slots per tile or
 *    frame, not two per row), and byte t of the run lands in LDS at byte
 *    head + t + 4 r e: r = t / w its row, head = run address & 15, e = 0 or 1
 *    padding dwords per row.  So an aligned dword of the run is an aligned
 *    dword of LDS and the stores are ds_write_b32 of whole dwords; a dword
 *    that holds bytes of two rows (or more, w < 4) is stored once per row, at
 *    either offset: the bytes of the other row in it are never looked at.
 *    e makes the row pitch (w + 4e) / 4 dwords round to an odd number, so the
 *    lanes of phase 2 start on different banks: w = 128 (RS(255,223) at size
 *    96) has pitch 33, not 32 (32 lanes on one bank); w = 255 has 64.75 (two
 *    lanes per bank at worst), not 63.75 (four).
 *    rs_report_k stores snapshot ^ rows.  The snapshot run is 16-byte aligned
 *    (tiles are multiples of 16 rows).  Rows that are themselves a 16-byte
 *    aligned run of wire rows (the staging rows of the interleaved calls, a
 *    caller's block of wire rows) are loaded the same way and XORed in
 *    registers.  Any other placement takes a second pass: the rows' regions as
 *    dwords (bases and strides 4-byte aligned) or bytes, XORed into the LDS
 *    image byte by byte.
 *  2 lane = codeword.  It walks its row in dwords and looks at the bytes of
 *    the non-zero ones only, in order, so the list comes out ascending without
 *    a sort; the lists are built in LDS (pitch an odd number of dwords).
 *    rs_mask_lists_k at depth > 1 walks symbol j of its codeword at byte
 *    j * depth + i of the frame instead.
 *  3 the tile's lists go out as dwords (4-byte aligned base and stride) or
 *    bytes, consecutive lanes on consecutive bytes: with a stride of nr the
 *    tile's lists are one run.  Bytes nr .. stride of a slot row are never
 *    written.
 *
 * Nothing outside the regions named above is read or written, with one
 * exception on the library's own buffers: the last 16-byte slot of a snapshot
 * run is read and written whole (the snapshot buffer has 256 bytes per
 * codeword and at least 64 codewords, api.cpp ensure_rep).
 */
#include <algorithm>

#include "rs_device.h"

#define RS_REP_THREADS 256
#define RS_REP_IMAGE 34816u /* LDS bytes of a tile's image: 128 rows of 260 B, 256 rows of 132 B */
#define RS_REP_LDS 65536u   /* image and lists */

/* 16 bytes at p + o0 of a run of len bytes at p: one uint4 load when they lie
 * inside it (p + o0 is 16-byte aligned), else the bytes inside, the rest 0 */
static __device__ __forceinline__ uint4 rep_load16(const uint8_t *p, int32_t o0, uint32_t len)
{
    if (o0 >= 0 && o0 + 16 <= (int32_t)len)
        return *reinterpret_cast<const uint4 *>(p + o0);
    uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int32_t k = 0; k < 16; k++) {
        const int32_t o = o0 + k;
        if (o >= 0 && o < (int32_t)len)
            x[k >> 2] |= (uint32_t)p[o] << (8 * (k & 3));
    }
    return make_uint4(x[0], x[1], x[2], x[3]);
}

/* the slot's four dwords into the LDS image (dwords dw0 .. dw0 + 3 before the
 * row padding): dword k holds run bytes o0 + 4k .. + 3, and goes to the place
 * of every row (w bytes each) that has a byte in it */
static __device__ __forceinline__ void rep_put16(uint32_t *img, uint4 x, int32_t o0, uint32_t dw0, uint32_t len,
                                                 uint32_t w, uint32_t e)
{
    if (o0 >= (int32_t)len)
        return;
    const uint32_t v[4] = {x.x, x.y, x.z, x.w};
    uint32_t r = (o0 < 0 ? 0u : (uint32_t)o0) / w, rend = (r + 1u) * w; /* rend: the next row's first byte */
#pragma unroll
    for (int32_t k = 0; k < 4; k++) {
        const int32_t t = o0 + 4 * k;
        if (t + 3 < 0 || t >= (int32_t)len)
            continue;
        const uint32_t lo = t < 0 ? 0u : (uint32_t)t;
        const uint32_t hi = (uint32_t)(t + 3) < len - 1u ? (uint32_t)(t + 3) : len - 1u;
        while (lo >= rend) {
            r++;
            rend += w;
        }
        uint32_t rr = r, re = rend;
        for (;;) {
            img[dw0 + (uint32_t)k + rr * e] = v[k];
            if (hi < re)
                break;
            rr++;
            re += w;
        }
    }
}

/* lane = codeword: the non-zero bytes of the w bytes at LDS byte b0, ascending,
 * the first nr of them into lpos (and lval); returns how many were listed,
 * total = how many there are */
template <bool VALS>
static __device__ __forceinline__ uint32_t rep_scan_row(const uint32_t *img, uint32_t b0, uint32_t w, uint32_t nr,
                                                        uint8_t *lpos, uint8_t *lval, uint32_t &total)
{
    uint32_t n = 0u;
    total = 0u;
    const uint32_t last = b0 + w - 1u, d0 = b0 >> 2, d1 = last >> 2;
    for (uint32_t d = d0; d <= d1; d++) {
        uint32_t x = img[d];
        if (d == d0)
            x &= 0xFFFFFFFFu << (8u * (b0 & 3u));
        if (d == d1)
            x &= 0xFFFFFFFFu >> (8u * (3u - (last & 3u)));
        /* one turn per non-zero byte, lowest first: the lanes of a wave hold
         * different rows, and at the usual error counts some lane has a byte
         * in nearly every dword, but rarely two */
        while (x) {
            const uint32_t k = (uint32_t)(__ffs((int)x) - 1) >> 3;
            if (n < nr) {
                lpos[n] = (uint8_t)(d * 4u + k - b0);
                if (VALS)
                    lval[n] = (uint8_t)(x >> (8u * k));
                n++;
            }
            total++;
            x &= ~(0xFFu << (8u * k));
        }
    }
    return n;
}

/* the tile's lists (LDS, lp bytes apart, zero behind the counts) to
 * out[(c0 + r) * stride .. + nr) for r < fc */
static __device__ void rep_lists_out(const uint8_t *lst, uint32_t lp, uint8_t *out, size_t stride, uint32_t nr,
                                     size_t c0, uint32_t fc)
{
    const uint32_t nq = (nr + 3u) / 4u;
    const bool al = ((reinterpret_cast<uintptr_t>(out) | stride) & 3u) == 0u;
    for (uint32_t idx = threadIdx.x; idx < fc * nq; idx += RS_REP_THREADS) {
        const uint32_t r = idx / nq, j = 4u * (idx - r * nq);
        const uint32_t v = *reinterpret_cast<const uint32_t *>(lst + r * lp + j);
        uint8_t *o = out + (c0 + r) * stride + j;
        if (al && j + 4u <= nr) {
            *reinterpret_cast<uint32_t *>(o) = v;
        } else {
            for (uint32_t k = 0; k < 4u && j + k < nr; k++)
                o[k] = (uint8_t)(v >> (8u * k));
        }
    }
}

/* n bytes per row at reg + (c0 + r) * stride, XORed into columns col0 .. of the
 * LDS image's rows (head 0): dword loads when base and stride are 4-byte aligned */
static __device__ void rep_region_xor(uint8_t *imgb, const uint8_t *reg, size_t stride, uint32_t n, uint32_t col0,
                                      size_t c0, uint32_t fc, uint32_t w, uint32_t e)
{
    const uint32_t nq = (n + 3u) / 4u;
    const bool al = ((reinterpret_cast<uintptr_t>(reg) | stride) & 3u) == 0u;
    for (uint32_t idx = threadIdx.x; idx < fc * nq; idx += RS_REP_THREADS) {
        const uint32_t r = idx / nq, j = 4u * (idx - r * nq);
        const uint32_t cnt = n - j < 4u ? n - j : 4u;
        const uint8_t *p = reg + (c0 + r) * stride + j;
        uint32_t v = 0u;
        if (al && cnt == 4u) {
            v = *reinterpret_cast<const uint32_t *>(p);
        } else {
            for (uint32_t k = 0; k < cnt; k++)
                v |= (uint32_t)p[k] << (8u * k);
        }
        uint8_t *b = imgb + r * (w + 4u * e) + col0 + j;
        for (uint32_t k = 0; k < cnt; k++)
            b[k] ^= (uint8_t)(v >> (8u * k));
    }
}

struct RsRepArgs {
    const uint8_t *data, *parity; /* the rows after the decode */
    size_t ds, ps;
    const uint8_t *snap;          /* the rows before it: wire rows, 16-byte aligned */
    uint8_t *num, *pos, *val;
    size_t rstride;
    uint32_t size, nr, count;
    uint32_t tile;                /* codewords per workgroup, a multiple of 16 */
    uint32_t e, lp, img;          /* padding dwords per row, list pitch (bytes), image dwords */
    uint32_t run;                 /* the rows are a 16-byte aligned run of wire rows at data */
};

extern __shared__ uint4 rep_lds[];

__global__ __launch_bounds__(RS_REP_THREADS) void rs_report_k(RsRepArgs a)
{
    const uint32_t c0 = blockIdx.x * a.tile;
    if (c0 >= a.count)
        return;
    const uint32_t fc = a.count - c0 < a.tile ? a.count - c0 : a.tile;
    const uint32_t w = a.size + a.nr, len = fc * w;
    uint32_t *img = reinterpret_cast<uint32_t *>(rep_lds);
    uint8_t *lpos = reinterpret_cast<uint8_t *>(img + a.img), *lval = lpos + a.tile * a.lp;
    for (uint32_t i = threadIdx.x; i < a.tile * a.lp / 2u; i += RS_REP_THREADS)
        reinterpret_cast<uint32_t *>(lpos)[i] = 0u; /* both lists */
    const uint8_t *snap = a.snap + (size_t)c0 * w;
    const uint32_t nq = (len + 15u) / 16u;
    if (a.run) {
        /* two slots of either side in flight per lane */
        const uint8_t *now = a.data + (size_t)c0 * w;
        for (uint32_t q = threadIdx.x; q < nq; q += 2u * RS_REP_THREADS) {
            const uint32_t q1 = q + RS_REP_THREADS;
            const int32_t o0 = (int32_t)(q * 16u), o1 = (int32_t)(q1 * 16u);
            uint4 s0 = *reinterpret_cast<const uint4 *>(snap + o0), s1 = make_uint4(0u, 0u, 0u, 0u), n1 = s1;
            const uint4 n0 = rep_load16(now, o0, len);
            if (q1 < nq) {
                s1 = *reinterpret_cast<const uint4 *>(snap + o1);
                n1 = rep_load16(now, o1, len);
            }
            rep_put16(img, make_uint4(s0.x ^ n0.x, s0.y ^ n0.y, s0.z ^ n0.z, s0.w ^ n0.w), o0, q * 4u, len, w, a.e);
            if (q1 < nq)
                rep_put16(img, make_uint4(s1.x ^ n1.x, s1.y ^ n1.y, s1.z ^ n1.z, s1.w ^ n1.w), o1, q1 * 4u, len, w,
                          a.e);
        }
    } else {
        for (uint32_t q = threadIdx.x; q < nq; q += RS_REP_THREADS)
            rep_put16(img, *reinterpret_cast<const uint4 *>(snap + q * 16u), (int32_t)(q * 16u), q * 4u, len, w, a.e);
        __syncthreads();
        rep_region_xor(reinterpret_cast<uint8_t *>(img), a.data, a.ds, a.size, 0u, c0, fc, w, a.e);
        rep_region_xor(reinterpret_cast<uint8_t *>(img), a.parity, a.ps, a.nr, a.size, c0, fc, w, a.e);
    }
    __syncthreads();
    if (threadIdx.x < fc) {
        const uint32_t r = threadIdx.x;
        uint32_t total;
        const uint32_t n = rep_scan_row<true>(img, r * (w + 4u * a.e), w, a.nr, lpos + r * a.lp, lval + r * a.lp, total);
        a.num[(size_t)c0 + r] = (uint8_t)n;
    }
    __syncthreads();
    rep_lists_out(lpos, a.lp, a.pos, a.rstride, a.nr, c0, fc);
    rep_lists_out(lval, a.lp, a.val, a.rstride, a.nr, c0, fc);
}

struct RsSnapArgs {
    const uint8_t *data, *parity;
    size_t ds, ps;
    uint8_t *snap;
    uint32_t size, nr;
    size_t count;
};

/* strided rows -> wire rows: a lane gathers one 16-byte slot of the snapshot
 * (bytes behind the last row: 0) and stores it whole */
__global__ __launch_bounds__(RS_REP_THREADS) void rs_snapshot_k(RsSnapArgs a)
{
    const uint32_t w = a.size + a.nr;
    const size_t q = (size_t)blockIdx.x * RS_REP_THREADS + threadIdx.x, t0 = q * 16u;
    if (t0 >= a.count * w)
        return;
    size_t r = t0 / w;
    uint32_t col = (uint32_t)(t0 - r * w);
    uint32_t x[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        if (r < a.count) {
            const uint8_t b = col < a.size ? a.data[r * a.ds + col] : a.parity[r * a.ps + (col - a.size)];
            x[k >> 2] |= (uint32_t)b << (8u * (k & 3u));
        }
        if (++col == w) {
            col = 0u;
            r++;
        }
    }
    *reinterpret_cast<uint4 *>(a.snap + t0) = make_uint4(x[0], x[1], x[2], x[3]);
}

struct RsMaskArgs {
    const uint8_t *mask; /* frame f's size * depth flags at mask + f * mstride */
    size_t mstride;
    uint8_t *pos, *cnt, *over;
    size_t pstride;
    uint32_t size, depth, nr, nframes;
    uint32_t tile;         /* frames per workgroup: tile * depth <= 256 */
    uint32_t e, lp, img;
    uint32_t fpd;          /* strided plane: LDS dwords per frame (odd); 0: the frames are one run */
};

__global__ __launch_bounds__(RS_REP_THREADS) void rs_mask_lists_k(RsMaskArgs a)
{
    const uint32_t f0 = blockIdx.x * a.tile;
    if (f0 >= a.nframes)
        return;
    const uint32_t fc = a.nframes - f0 < a.tile ? a.nframes - f0 : a.tile;
    const uint32_t fb = a.size * a.depth;
    uint32_t *img = reinterpret_cast<uint32_t *>(rep_lds);
    uint8_t *lpos = reinterpret_cast<uint8_t *>(img + a.img);
    for (uint32_t i = threadIdx.x; i < a.tile * a.depth * a.lp / 4u; i += RS_REP_THREADS)
        reinterpret_cast<uint32_t *>(lpos)[i] = 0u;
    const uint8_t *run = a.mask + (size_t)f0 * a.mstride;
    if (!a.fpd) {
        const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u), len = fc * fb;
        const uint32_t nq = (head + len + 15u) / 16u;
        for (uint32_t q = threadIdx.x; q < nq; q += 2u * RS_REP_THREADS) {
            const uint32_t q1 = q + RS_REP_THREADS;
            const int32_t o0 = (int32_t)(q * 16u) - (int32_t)head, o1 = (int32_t)(q1 * 16u) - (int32_t)head;
            const uint4 x0 = rep_load16(run, o0, len);
            uint4 x1 = make_uint4(0u, 0u, 0u, 0u);
            if (q1 < nq)
                x1 = rep_load16(run, o1, len);
            rep_put16(img, x0, o0, q * 4u, len, fb, a.e);
            if (q1 < nq)
                rep_put16(img, x1, o1, q1 * 4u, len, fb, a.e);
        }
    } else {
        const uint32_t nq = fb / 16u + 2u; /* slots a frame can touch at the worst alignment */
        for (uint32_t idx = threadIdx.x; idx < fc * nq; idx += RS_REP_THREADS) {
            const uint32_t fl = idx / nq, q = idx - fl * nq;
            const uint8_t *p = run + (size_t)fl * a.mstride;
            const int32_t o0 = (int32_t)(q * 16u) - (int32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
            if (o0 < (int32_t)fb)
                rep_put16(img + fl * a.fpd, rep_load16(p, o0, fb), o0, q * 4u, fb, fb, 0u);
        }
    }
    __syncthreads();
    if (threadIdx.x < fc * a.depth) {
        const uint32_t cl = threadIdx.x, fl = cl / a.depth, i = cl - fl * a.depth;
        /* LDS byte of the frame's first flag */
        const uint32_t fs = a.fpd ? fl * a.fpd * 4u +
                                        (uint32_t)(reinterpret_cast<uintptr_t>(run + (size_t)fl * a.mstride) & 15u)
                                  : (uint32_t)(reinterpret_cast<uintptr_t>(run) & 15u) + fl * (fb + 4u * a.e);
        uint8_t *lp = lpos + cl * a.lp;
        uint32_t n = 0u, total = 0u;
        if (a.depth == 1u) {
            n = rep_scan_row<false>(img, fs, a.size, a.nr, lp, nullptr, total);
        } else {
            const uint8_t *fbytes = reinterpret_cast<const uint8_t *>(img) + fs + i;
            for (uint32_t j = 0; j < a.size; j++) {
                if (fbytes[j * a.depth]) {
                    if (n < a.nr)
                        lp[n++] = (uint8_t)j;
                    total++;
                }
            }
        }
        const size_t c = (size_t)f0 * a.depth + cl;
        a.cnt[c] = (uint8_t)n;
        if (a.over)
            a.over[c] = total > a.nr ? 1u : 0u;
    }
    __syncthreads();
    rep_lists_out(lpos, a.lp, a.pos, a.pstride, a.nr, (size_t)f0 * a.depth, fc * a.depth);
}

/* row padding that rounds the pitch (w + 4e) / 4 dwords to an odd number */
static uint32_t rep_pad(uint32_t w) { return (((w + 2u) / 4u) & 1u) ? 0u : 1u; }
/* list pitch: nr bytes in an odd number of dwords */
static uint32_t rep_list_pitch(uint32_t nr) { return (((nr + 3u) / 4u) | 1u) * 4u; }

extern "C" hipError_t rsk_snapshot(const uint8_t *data, size_t ds, const uint8_t *parity, size_t ps, uint8_t *snap,
                                   uint32_t size, uint32_t nr, size_t count, hipStream_t stream)
{
    const uint32_t w = size + nr;
    if (w == 0u || w > 255u || (reinterpret_cast<uintptr_t>(snap) & 15u))
        return hipErrorInvalidValue;
    if (count == 0)
        return hipSuccess;
    const size_t nq = (count * w + 15u) / 16u, grid = (nq + RS_REP_THREADS - 1u) / RS_REP_THREADS;
    if (grid > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    RsSnapArgs a = {data, parity, ds, ps, snap, size, nr, count};
    RS_LAUNCH(rs_snapshot_k, dim3((uint32_t)grid), dim3(RS_REP_THREADS), 0, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t rsk_report(const uint8_t *data, size_t ds, const uint8_t *parity, size_t ps, const uint8_t *snap,
                                 uint32_t size, uint32_t nr, size_t count, uint8_t *num, uint8_t *pos, uint8_t *val,
                                 size_t rstride, hipStream_t stream)
{
    const uint32_t w = size + nr;
    if (size == 0u || nr == 0u || w > 255u || rstride < nr || count > 0x7FFFFFFFu ||
        (reinterpret_cast<uintptr_t>(snap) & 15u))
        return hipErrorInvalidValue;
    if (count == 0)
        return hipSuccess;
    RsRepArgs a;
    a.data = data;
    a.parity = parity;
    a.ds = ds;
    a.ps = ps;
    a.snap = snap;
    a.num = num;
    a.pos = pos;
    a.val = val;
    a.rstride = rstride;
    a.size = size;
    a.nr = nr;
    a.count = (uint32_t)count;
    a.e = rep_pad(w);
    a.lp = rep_list_pitch(nr);
    a.tile = std::min(256u, RS_REP_IMAGE / (w + 4u * a.e)) & ~15u;
    auto image = [&](uint32_t tile) { return ((tile * w + 3u) / 4u + tile * a.e + 3u) & ~3u; };
    while (a.tile > 16u && image(a.tile) * 4u + 2u * a.tile * a.lp > RS_REP_LDS)
        a.tile -= 16u;
    a.img = image(a.tile);
    const uint32_t lds = a.img * 4u + 2u * a.tile * a.lp;
    if (a.tile < 16u || lds > RS_REP_LDS)
        return hipErrorInvalidValue;
    a.run = parity == data + size && ds == w && ps == w && !(reinterpret_cast<uintptr_t>(data) & 15u) ? 1u : 0u;
    const uint32_t grid = (a.count + a.tile - 1u) / a.tile;
    RS_LAUNCH(rs_report_k, dim3(grid), dim3(RS_REP_THREADS), lds, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t rsk_mask_lists(const uint8_t *mask, size_t mstride, uint32_t size, uint32_t depth, uint32_t nr,
                                     size_t nframes, uint8_t *pos, size_t pstride, uint8_t *cnt, uint8_t *over,
                                     hipStream_t stream)
{
    const uint32_t fb = size * depth;
    if (size == 0u || size > 254u || nr == 0u || nr > 254u || depth == 0u || depth > RS_ILV_MAX_DEPTH ||
        mstride < fb || pstride < nr || nframes > 0x7FFFFFFFu / RS_ILV_MAX_DEPTH)
        return hipErrorInvalidValue;
    if (nframes == 0)
        return hipSuccess;
    RsMaskArgs a;
    a.mask = mask;
    a.mstride = mstride;
    a.pos = pos;
    a.cnt = cnt;
    a.over = over;
    a.pstride = pstride;
    a.size = size;
    a.depth = depth;
    a.nr = nr;
    a.nframes = (uint32_t)nframes;
    a.lp = rep_list_pitch(nr);
    const bool run = mstride == fb;
    a.e = run ? rep_pad(fb) : 0u;
    a.fpd = run ? 0u : ((fb + 15u + 3u) / 4u) | 1u;
    /* image dwords: a run of tile frames behind a head of up to 15 bytes, or tile frames of fpd dwords */
    auto image = [&](uint32_t tile) {
        return run ? ((15u + tile * fb + 3u) / 4u + tile * a.e + 3u) & ~3u : (tile * a.fpd + 3u) & ~3u;
    };
    a.tile = std::max(1u, std::min(RS_REP_THREADS / depth, RS_REP_IMAGE / (fb + 20u)));
    while (a.tile > 1u && image(a.tile) * 4u + a.tile * depth * a.lp > RS_REP_LDS)
        a.tile--;
    a.img = image(a.tile);
    const uint32_t lds = a.img * 4u + a.tile * depth * a.lp;
    if (lds > RS_REP_LDS)
        return hipErrorInvalidValue;
    const uint32_t grid = (a.nframes + a.tile - 1u) / a.tile;
    RS_LAUNCH(rs_mask_lists_k, dim3(grid), dim3(RS_REP_THREADS), lds, stream, a);
    return hipGetLastError();
}
