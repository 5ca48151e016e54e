"""RS x RS product-code blocks against the oracle's row batches (helper, no tests).

A block is n2 rows of n1 bytes: every row a codeword of the row code (k1 message symbols, r1 roots),
every column a codeword of the column code (k2, r2) (include/poporon_amd.h).  The reference has no
notion of a block, so its answer is its row batch answer on the block's rows and on its transposed
columns.  ``Model`` is the definition of the product calls: numpy and ``oracle.Oracle`` alone, nothing
of the library under test.  ``decode`` follows the header's three numbered steps literally.

``tile_rule`` / ``tile_model`` restate the index arithmetic of the layout kernels (rs_product.hip) in
numpy with every bound asserted; tests/test_product_cpu.py sweeps them.
"""
import numpy as np

DVD_ROW = (8, 0x11D, 0, 1, 10)  # RS(182,172)
DVD_COL = (8, 0x11D, 0, 1, 16)  # RS(208,192)
DVD_K1, DVD_K2 = 172, 192


def codewords(blocks, axis):
    """u8[count, n2, n1] -> the axis's codewords as rows: u8[count*n2, n1] or u8[count*n1, n2]"""
    b = np.asarray(blocks, dtype=np.uint8)
    count, n2, n1 = b.shape
    if axis == 0:
        return np.ascontiguousarray(b.reshape(count * n2, n1))
    return np.ascontiguousarray(b.transpose(0, 2, 1).reshape(count * n1, n2))


def from_codewords(rows, axis, count):
    """the inverse of codewords()"""
    r = np.asarray(rows, dtype=np.uint8)
    if axis == 0:
        return np.ascontiguousarray(r.reshape(count, -1, r.shape[1]))
    return np.ascontiguousarray(r.reshape(count, -1, r.shape[1]).transpose(0, 2, 1))


def coupling_lists(other_flags, r_a, cw_a):
    """step 1 of a pass: other_flags u8[count, n_other], the other axis's dirty flags per block ->
    (positions u32[count*cw_a, r_a], counts u32[count*cw_a])"""
    f = np.asarray(other_flags)
    count = f.shape[0]
    pos = np.zeros((count, cw_a, r_a), np.uint32)
    cnt = np.zeros((count, cw_a), np.uint32)
    for b in range(count):
        e = np.nonzero(f[b])[0]
        if r_a // 2 < len(e) <= r_a:
            pos[b, :, :len(e)] = e[None, :]
            cnt[b, :] = len(e)
    return pos.reshape(count * cw_a, r_a), cnt.reshape(-1)


class Model:
    def __init__(self, row, col, threads=0):
        from oracle import Oracle
        self.o = (Oracle(*row), Oracle(*col))
        self.r = (row[4], col[4])
        self.threads = threads

    def shape(self, k1, k2):
        return k1 + self.r[0], k2 + self.r[1]

    def _encode_axis(self, blocks, axis, k, ncw):
        """parity of the first ncw codewords of every block along the axis, written in place"""
        count = blocks.shape[0]
        if axis == 0:
            rows = np.ascontiguousarray(blocks[:, :ncw, :k]).reshape(count * ncw, k)
            blocks[:, :ncw, k:] = self.o[0].encode_batch(rows, threads=self.threads).reshape(count, ncw, -1)
        else:
            cols = np.ascontiguousarray(blocks[:, :k, :ncw].transpose(0, 2, 1)).reshape(count * ncw, k)
            par = self.o[1].encode_batch(cols, threads=self.threads).reshape(count, ncw, -1)
            blocks[:, k:, :ncw] = par.transpose(0, 2, 1)

    def encode(self, messages, rows_first=False):
        """u8[count, k2, k1] -> u8[count, n2, n1]: column parity of the message columns, then row parity of
        every row (rows_first: row parity of the message rows, then column parity of every column)"""
        m = np.asarray(messages, dtype=np.uint8)
        count, k2, k1 = m.shape
        n1, n2 = self.shape(k1, k2)
        out = np.zeros((count, n2, n1), np.uint8)
        out[:, :k2, :k1] = m
        if rows_first:
            self._encode_axis(out, 0, k1, k2)
            self._encode_axis(out, 1, k2, n1)
        else:
            self._encode_axis(out, 1, k2, k1)
            self._encode_axis(out, 0, k1, n2)
        return out

    def flags(self, blocks, axis, k):
        rows = codewords(blocks, axis)
        return self.o[axis].syndrome_batch(rows[:, :k], rows[:, k:])[0].reshape(blocks.shape[0], -1)

    def check(self, blocks, k1, k2):
        """(row_dirty u8[count, n2], col_dirty u8[count, n1], block_ok u8[count])"""
        rd, cd = self.flags(blocks, 0, k1), self.flags(blocks, 1, k2)
        return rd, cd, (~(rd.any(1) | cd.any(1))).astype(np.uint8)

    def decode(self, blocks, k1, k2, first_axis=0, passes=2, couple=1):
        """(blocks', row_dirty, col_dirty, block_ok) of the schedule"""
        assert first_axis in (0, 1) and 1 <= passes <= 16
        b = np.array(blocks, dtype=np.uint8, copy=True)
        count = b.shape[0]
        k = (k1, k2)
        flag = [None, None]
        a = first_axis
        for p in range(passes):
            rows = codewords(b, a)
            d, par = rows[:, :k[a]], rows[:, k[a]:]
            if couple and p > 0:  # 1. lists
                pos, cnt = coupling_lists(flag[a ^ 1], self.r[a], rows.shape[0] // count)
                res = self.o[a].decode_batch(d, par, pos, cnt, threads=self.threads)
            else:
                res = self.o[a].decode_batch(d, par, threads=self.threads)
            rows = np.concatenate([res[2], res[3]], 1)  # 2. decode, as the row call leaves every codeword
            flag[a] = self.o[a].syndrome_batch(res[2], res[3])[0].reshape(count, -1)  # 3. flags: dirty after the pass
            b = from_codewords(rows, a, count)
            a ^= 1
        flag[a] = self.flags(b, a, k[a])  # the other axis, once, on the block as returned
        return b, flag[0], flag[1], (~(flag[0].any(1) | flag[1].any(1))).astype(np.uint8)


# ---- the kernels' index arithmetic ---------------------------------------------------------

LDS_BYTES = 32768
LDS_PACK = 16384


def tile_rule(w, cw):
    """rsk_prod_tile restated: (whole blocks per tile, codewords per tile, tiles per block) for blocks of cw
    codewords of w bytes; None for no block"""
    if not (1 <= w <= 255 and 1 <= cw <= 255):
        return None
    per, g, u, tpb = w * cw, 1, cw, 1
    if per <= LDS_PACK:
        g = LDS_PACK // per
    elif per > LDS_BYTES:
        umax = (LDS_BYTES // w) & ~15
        parts = -(-cw // umax)
        u = (-(-cw // parts) + 15) & ~15
        tpb = -(-cw // u)
    return g, u, tpb


def tiles(w, cw, count):
    g, u, tpb = tile_rule(w, cw)
    return -(-count // g) if tpb == 1 else count * tpb


def _div(i, d):
    """the kernels' float estimate of i / d and its correction, asserted against divmod"""
    assert i.size == 0 or int(i.max()) < 1 << 24
    q = (i.astype(np.float32) * (np.float32(1.0) / np.float32(d))).astype(np.int64)
    r = i - q * d
    lo, hi = r < 0, r >= d
    q, r = q - lo + hi, r + lo * d - hi * d
    assert ((q == i // d) & (r == i % d)).all()
    return q, r


def _slots(addr, length, q):
    """slot16_part for arrays: slot q of runs of `length` bytes at addr -> (o0, kb, ke, valid)"""
    o0 = 16 * q - (addr & 15)
    kb = np.where(o0 < 0, -o0, 0)
    ke = np.minimum(16, length - o0)
    return o0, kb, ke, (o0 < length) & (kb < ke)


def tile_model(axis, w, cw, m0, m1, pitch, bstride, base, count, t):
    """Workgroup t of a layout pass over `count` blocks at address `base`, as the kernels index it (the staging
    rows at address 0).  Returns None for a workgroup with no tile, else a dict: mem = block-side byte addresses
    touched, img = the image byte of each, rows = staging bytes the row side touches, lds = LDS bytes allocated.
    Asserts: uint4 accesses aligned, every LDS index inside the allocation, every image index inside the image."""
    g, u, tpb = tile_rule(w, cw)
    if tpb == 1:
        b0 = t * g
        if b0 >= count:
            return None
        nb, c0, nc = min(g, count - b0), 0, cw
    else:
        b0, c0 = t // tpb, (t % tpb) * u
        if b0 >= count or c0 >= cw:
            return None
        nb, nc = 1, min(u, cw - c0)
    rpb = m1 - m0 if axis else nc
    length = nc if axis else m1 - m0
    nr = nb * rpb
    off = (b0 * cw + c0) * w
    head, nbytes = off & 15, nb * nc * w
    s = ((u if axis else m1 - m0) + 30) // 16
    lds = (g * u * w + 30) & ~15
    assert lds <= LDS_BYTES + 16 and head + nbytes <= lds
    q, r = _div(np.arange(nr * s, dtype=np.int64), nr)
    bb, x = _div(r, rpb)
    if axis:
        at, step = bb * cw * w + m0 + x, w
        p = base + (b0 + bb) * bstride + (m0 + x) * pitch + c0
    else:
        at, step = (bb * cw + x) * w + m0, 1
        p = base + (b0 + bb) * bstride + (c0 + x) * pitch + m0
    o0, kb, ke, valid = _slots(p, length, q)
    whole = valid & (kb == 0) & (ke == 16)
    # every slot is cut on a 16-byte boundary: the whole ones move as uint4, and the gather also loads a head or
    # tail slot whole when it lies inside the chunk's blocks (the bytes beside the run are dropped)
    assert ((p + o0)[valid] % 16 == 0).all()
    k = np.arange(16)[None, :]
    m = valid[:, None] & (k >= kb[:, None]) & (k < ke[:, None])
    mem = ((p + o0)[:, None] + k)[m]
    img = (at[:, None] + (o0[:, None] + k) * step)[m]
    assert img.size == 0 or (0 <= img.min() and img.max() < nbytes)
    # the row side: the image's run in the staging rows, slots cut at the run's own address
    nq = -(-(head + nbytes) // 16)
    qq = np.arange(nq, dtype=np.int64)
    ro0, rkb, rke, rvalid = _slots(np.full(nq, off, np.int64), nbytes, qq)
    rwhole = rvalid & (rkb == 0) & (rke == 16)
    assert ((off + ro0)[rwhole] % 16 == 0).all() and rvalid.all()
    rm = (k >= rkb[:, None]) & (k < rke[:, None])
    rows = ((off + ro0)[:, None] + k)[rm]
    ldsi = (qq[:, None] * 16 + k)[rm]
    assert (ldsi < lds).all() and (ldsi - head == rows - off).all()  # an LDS uint4 and a staging uint4: the same bytes
    return {"mem": mem, "img": img, "rows": rows, "lds": lds, "off": off, "bytes": nbytes, "b0": b0, "nb": nb,
            "c0": c0, "nc": nc}


def expected_image(axis, w, cw, m0, m1, tile):
    """the image bytes a pass with symbols [m0, m1) moves for a tile (relative to the image)"""
    nb, nc = tile["nb"], tile["nc"]
    c = np.arange(nb * nc)
    bb, cc = c // nc, c % nc
    start = (bb * cw + cc) * w if nb > 1 or nc == cw else cc * w
    return np.sort((start[:, None] + np.arange(m0, m1)[None, :]).reshape(-1))


def expected_mem(axis, w, cw, m0, m1, pitch, bstride, base, count):
    """the block bytes a pass moves: codewords [0, cw) of every block, symbols [m0, m1)"""
    b = np.arange(count)[:, None, None]
    c = np.arange(cw)[None, :, None]
    m = np.arange(m0, m1)[None, None, :]
    i, j = (m, c) if axis else (c, m)
    return np.sort((base + b * bstride + i * pitch + j).reshape(-1))


# ---- DVD blocks and the corruption patterns of the tests ------------------------------------

def dvd_blocks(model, count, seed):
    rng = np.random.default_rng([seed, count])
    return model.encode(rng.integers(0, 256, (count, DVD_K2, DVD_K1), dtype=np.uint8))


def _scatter_errors(rng, block, rows, nerr):
    """nerr (int or per-row array) errors at distinct columns of each listed row of one block"""
    n1 = block.shape[1]
    for i, e in zip(rows, np.broadcast_to(nerr, len(rows))):
        cols = rng.choice(n1, int(e), replace=False)
        block[i, cols] ^= rng.integers(1, 256, int(e), dtype=np.uint8)


def dvd_pattern(name, clean, seed):
    """clean u8[count, 208, 182] -> (corrupted copy, first_axis, passes, couple, repaired) for the named pattern;
    repaired: the schedule gives the original block back (tests/test_product_cpu.py checks it on the model)"""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    bad = clean.copy()
    count, n2, n1 = bad.shape
    sched = (0, 2, 1, True)
    for b in range(count):
        blk = bad[b]
        if name == "errors5":
            _scatter_errors(rng, blk, np.arange(n2), rng.integers(0, 6, n2))
            sched = (0, 1, 1, True)
        elif name.startswith("rows"):  # rows16, rows16_nocouple, rows8, rows9, rows17
            nrows = int(name[4:].split("_")[0])
            rows = rng.choice(n2, nrows, replace=False)
            blk[rows] = rng.integers(0, 256, (nrows, n1), dtype=np.uint8)
            couple = 0 if name.endswith("_nocouple") else 1
            # coupled: lists from 9 to 16 flagged rows; below that the column pass is the erasure-mode call with
            # count 0, which does not repair errors; uncoupled: the column code's t = 8
            sched = (0, 2, couple, 8 < nrows <= 16 if couple else nrows <= 8)
        elif name.startswith("cols"):  # cols12, cols10
            ncols = int(name[4:])
            cols = rng.choice(n1, ncols, replace=False)
            blk[:, cols] = rng.integers(0, 256, (n2, ncols), dtype=np.uint8)
            sched = (1, 2, 1, ncols <= 10)
        elif name == "burst":
            r0 = int(rng.integers(0, n2 - 10))
            blk[r0:r0 + 10] = rng.integers(0, 256, (10, n1), dtype=np.uint8)
            _scatter_errors(rng, blk, [i for i in range(n2) if not r0 <= i < r0 + 10], 3)
            sched = (0, 3, 1, True)
        elif name == "planted":
            rows = rng.choice(n2, 10, replace=False)
            blk[rows[:9]] = rng.integers(0, 256, (9, n1), dtype=np.uint8)
            other = clean[(b + 1) % count] if count > 1 else clean[b]
            blk[rows[9]] = other[(rows[9] + 1) % n2]  # a clean row codeword that is not this row's
            sched = (0, 2, 1, None)  # quirk Q2 territory: the model decides
        elif name == "clean":
            sched = (0, 2, 1, True)
        else:
            raise KeyError(name)
    return (bad,) + sched


DVD_PATTERNS = ("errors5", "rows16", "rows16_nocouple", "rows8", "rows8_nocouple", "rows9", "rows17", "cols12",
                "cols10", "burst",
                "planted", "clean")
