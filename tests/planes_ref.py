"""Plane-layout stripes against the oracle's row batches (helper, no tests).

A stripe is W = size + nroots planes of `count` bytes; codeword c has symbol j at planes[j, c]
(include/poporon_amd.h).  The reference has no notion of a plane, so its answer for a stripe is its
row batch answer on the transpose: ``expect_*`` below, on ``oracle.Oracle``'s ``encode_batch`` /
``decode_batch`` / ``syndrome_batch``.  A rebuild zeroes the lost columns (lost planes are never
read) and gives every row the same erasure list: the lost plane indices ascending, zeros behind
them up to nroots, and the count.

``tile_model`` restates the index arithmetic of the layout kernels (rs_planes.hip) for one tile in
plain Python, with every bound asserted; tests/test_planes_cpu.py sweeps it.
"""
import numpy as np


def planes_to_rows(planes):
    """u8[W, count] -> u8[count, W]"""
    return np.ascontiguousarray(np.asarray(planes, dtype=np.uint8).T)


def rows_to_planes(rows):
    """u8[count, W] -> u8[W, count]"""
    return np.ascontiguousarray(np.asarray(rows, dtype=np.uint8).T)


def lost_lists(lost, nroots, count):
    """(positions u32[count, nroots], counts u32[count]): the list every codeword of a rebuild gets"""
    lost = list(lost)
    assert len(lost) <= nroots and all(a < b for a, b in zip(lost, lost[1:]))
    pos = np.zeros((count, nroots), np.uint32)
    pos[:, :len(lost)] = np.asarray(lost, dtype=np.uint32)[None, :]
    return pos, np.full(count, len(lost), np.uint32)


def staged_rows(planes, lost=()):
    """the rows a decode works on: the transpose with the lost columns zero"""
    rows = planes_to_rows(planes)
    rows[:, list(lost)] = 0
    return rows


def expect_encode(oracle, data_planes, threads=0):
    """parity planes u8[nroots, count] of message planes u8[size, count]"""
    return rows_to_planes(oracle.encode_batch(planes_to_rows(data_planes), threads=threads))


def expect_decode(oracle, planes, lost=(), threads=0):
    """(ok u8[count], corrected u32[count], planes' u8[W, count], dirty u8[count]) of a stripe; planes'
    holds what the row call left in every column, the lost ones included"""
    p = np.asarray(planes, dtype=np.uint8)
    W, count = p.shape
    size = W - oracle.nroots
    rows = staged_rows(p, lost)
    if len(lost):
        pos, cnt = lost_lists(lost, oracle.nroots, count)
        ok, cor, d, par = oracle.decode_batch(rows[:, :size], rows[:, size:], pos, cnt, threads=threads)
    else:
        ok, cor, d, par = oracle.decode_batch(rows[:, :size], rows[:, size:], threads=threads)
    dirty = oracle.syndrome_batch(d, par)[0]
    return ok, cor, rows_to_planes(np.concatenate([d, par], 1)), dirty


def expect_check(oracle, planes):
    """dirty u8[count]: the oracle's nonzero-syndrome flag per codeword"""
    rows = planes_to_rows(planes)
    size = rows.shape[1] - oracle.nroots
    return oracle.syndrome_batch(rows[:, :size], rows[:, size:])[0]


# ---- the kernels' index arithmetic ---------------------------------------------------------

LDS_BYTES = 32768
TILE_MAX = 512


def tile(W):
    """poporon_amd_plane_tile restated"""
    if W < 1 or W > 255:
        return 0
    return min(LDS_BYTES // W & ~15, TILE_MAX)


def _slot(addr, length, q, aligned):
    """the part [kb, ke) of 16-byte slot q of a run of `length` bytes at address addr, and the slot's offset o0 from
    the run's start (negative in the head slot); None where the slot holds no byte of the run"""
    head = 0 if aligned else addr & 15
    o0 = q * 16 - head
    if o0 >= length:
        return None
    kb = -o0 if o0 < 0 else 0
    ke = min(16, length - o0)
    return (o0, kb, ke) if kb < ke else None


def tile_model(W, T, count, t0, addrs, used, aligned):
    """One workgroup's tile [t0, t0 + T) of a chunk of `count` codewords, as the kernels index it.
    addrs[j]: the address of plane j's byte t0 (any int); used[j]: the plane moves.
    Returns (lds i64[tc*W], moves): lds[b] = how often LDS image byte b was touched from the plane side,
    moves = list of (plane, first byte relative to t0, last + 1, whole) per global access of the plane side.
    Asserts: every LDS index inside the image, every plane byte inside [0, tc)."""
    assert T % 16 == 0 and T * W <= LDS_BYTES and t0 % 16 == 0 and t0 < count
    tc = min(T, count - t0)
    s = T // 16 + (0 if aligned else 1)
    inv = np.float32(1.0) / np.float32(s)
    lds = np.zeros(tc * W, np.int64)
    moves = []
    for i in range(W * s):
        j = int(np.float32(i) * inv)      # the kernels' float estimate and its correction
        r = i - j * s
        if r < 0:
            r, j = r + s, j - 1
        elif r >= s:
            r, j = r - s, j + 1
        assert (j, r) == divmod(i, s)
        if aligned:
            assert not used[j] or addrs[j] % 16 == 0
        sl = _slot(addrs[j] if used[j] else 0, tc, r, aligned)
        if sl is None:
            continue
        o0, kb, ke = sl
        for k in range(kb, ke):
            c = o0 + k
            assert 0 <= c < tc
            b = c * W + j
            assert 0 <= b < tc * W <= T * W
            lds[b] += 1
        if used[j]:
            whole = kb == 0 and ke == 16
            assert not whole or (addrs[j] + o0) % 16 == 0  # a uint4 access is aligned
            moves.append((j, o0 + kb, o0 + ke, whole))
    return lds, moves


def row_side_model(W, tc):
    """the 16-byte pieces of a tile's contiguous run of tc*W row bytes: (first, last + 1, whole)"""
    n = tc * W
    out = []
    q = 0
    while q * 16 < n:
        out.append((q * 16, min(q * 16 + 16, n), q * 16 + 16 <= n))
        q += 1
    return out
