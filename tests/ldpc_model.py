"""A plain numpy model of the LDPC codec (not a test module): encode, check and
normalised min-sum decode as DESIGN.md section 11 and the header of
csrc/ldpc.hip describe them, written for a whole batch of rows at once in int64.

A graph is a dict with row_ptr, col_idx (CSR rows of H = [A | D]), info_bits and
the optional tables inner_forward (bits) and outer_forward (bytes); graph()
below builds one.  Nothing here keeps state and nothing calls the library: the
tests feed it the reference's recorded graph, or a handle's graph after it was
compared with the recorded SHA-256s.

Bit i of a row is byte i // 8, mask 0x80 >> i % 8.  Both interleavers scatter
on encode (out[forward[i]] = in[i]) and gather on decode (out[i] = in[forward[i]]).
"""
from __future__ import annotations

import numpy as np

LLR_SAT = 32000
LLR_HARD = 30000


def graph(row_ptr, col_idx, info_bits, inner_forward=None, outer_forward=None):
    i64 = lambda a: None if a is None else np.asarray(a, dtype=np.int64)  # noqa: E731
    g = dict(row_ptr=i64(row_ptr), col_idx=i64(col_idx), info_bits=int(info_bits), inner_forward=i64(inner_forward),
             outer_forward=i64(outer_forward))
    g["num_checks"] = g["row_ptr"].size - 1
    g["num_bits"] = g["info_bits"] + g["num_checks"]
    g["num_edges"] = int(g["row_ptr"][-1])
    assert (np.diff(g["row_ptr"]) >= 1).all(), "every check row holds its diagonal edge"
    assert g["col_idx"].size == g["num_edges"] and g["col_idx"].max() < g["num_bits"]
    # the column view: edges sorted by bit, and where each bit's run starts and ends
    g["by_col"] = np.argsort(g["col_idx"], kind="stable")
    g["col_ptr"] = np.searchsorted(g["col_idx"][g["by_col"]], np.arange(g["num_bits"] + 1))
    g["row_of"] = np.repeat(np.arange(g["num_checks"]), np.diff(g["row_ptr"]))
    return g


def _sizes(g):
    n = g["num_bits"]
    return g["info_bits"] // 8, (n + 7) // 8, n


def _bits(rows, n=None):
    b = np.unpackbits(np.ascontiguousarray(rows, dtype=np.uint8), axis=1)
    return b if n is None else b[:, :n]


def _bytes(bits, nbytes):
    out = np.zeros((bits.shape[0], 8 * nbytes), np.uint8)
    out[:, :bits.shape[1]] = bits
    return np.packbits(out, axis=1)


def _row_xor(g, edge_bits):
    """XOR of a 0/1 value per edge over every check row: [rows, num_checks]."""
    return np.bitwise_xor.reduceat(edge_bits, g["row_ptr"][:-1], axis=1)


def encode(g, data):
    """(data', parity): data' differs from data when an interleaver is on."""
    ib, cb, n = _sizes(g)
    d = np.ascontiguousarray(data, dtype=np.uint8)
    assert d.shape[1] == ib
    if g["outer_forward"] is not None:
        o = np.empty_like(d)
        o[:, g["outer_forward"]] = d
        d = o
    info = _bits(d)
    col = g["col_idx"]
    on_info = col < g["info_bits"]
    x = _row_xor(g, np.where(on_info, info[:, np.where(on_info, col, 0)], 0).astype(np.uint8))
    parity = np.bitwise_xor.accumulate(x, axis=1)  # the dual diagonal: p_i = x_0 ^ ... ^ x_i
    cw = np.concatenate([info, parity], axis=1)
    if g["inner_forward"] is not None:
        o = np.empty_like(cw)
        o[:, g["inner_forward"]] = cw
        cw = o
    out = _bytes(cw, cb)  # spare bits of the last byte are 0
    return np.ascontiguousarray(out[:, :ib]), np.ascontiguousarray(out[:, ib:])


def received(g, data, parity):
    """The received row's byte image after the inner de-interleave.  With the interleaver the
    spare bits are 0; without it the bytes are copied, spare bits included."""
    ib, cb, n = _sizes(g)
    rows = np.concatenate([np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(parity, dtype=np.uint8)],
                          axis=1)
    assert rows.shape[1] == cb
    if g["inner_forward"] is None:
        return rows
    return _bytes(_bits(rows)[:, g["inner_forward"]], cb)


def _dirty(g, bits):
    return _row_xor(g, bits[:, g["col_idx"]]).any(axis=1)


def check(g, data, parity):
    """1 where some check row of the de-interleaved row fails."""
    return _dirty(g, _bits(received(g, data, parity), g["num_bits"])).astype(np.uint8)


def _iterate(g, tot, channel, max_iterations):
    """Min-sum on rows that all start dirty.  tot: [rows, N] start totals; channel: the
    unsaturated llr * 256 (soft path) or None (hard path: the previous total).
    Returns (ok, iterations, last totals)."""
    rows = tot.shape[0]
    rp, col, by_col, cp, row_of = g["row_ptr"][:-1], g["col_idx"], g["by_col"], g["col_ptr"], g["row_of"]
    e_idx = np.arange(g["num_edges"])
    ok = np.zeros(rows, bool)
    iters = np.full(rows, max_iterations, np.int64)
    tot = tot.copy()
    live = np.arange(rows)
    t = tot
    v2c = t[:, col]
    for it in range(max_iterations):
        if live.size == 0:
            break
        # check update
        neg = v2c < 0
        mag = np.abs(v2c)
        min1 = np.minimum(np.minimum.reduceat(mag, rp, axis=1), LLR_SAT)
        # the first edge of the row at min1, when that is below the start value; else edge 0 of the graph
        hit = (mag == min1[:, row_of]) & (min1[:, row_of] < LLR_SAT)
        at = np.minimum.reduceat(np.where(hit, e_idx, g["num_edges"]), rp, axis=1)
        at = np.where(at == g["num_edges"], 0, at)
        holder = e_idx == at[:, row_of]
        min2 = np.minimum(np.minimum.reduceat(np.where(holder, LLR_SAT, mag), rp, axis=1), LLR_SAT)
        a = np.where(holder, min2[:, row_of], min1[:, row_of]) * 15 // 16
        flip = np.bitwise_xor.reduceat(neg.astype(np.uint8), rp, axis=1)[:, row_of].astype(bool) ^ neg
        c2v = np.where(flip, -a, a)
        # variable update: channel + incoming, each output saturated on its own
        run = np.concatenate([np.zeros((len(live), 1), np.int64), np.cumsum(c2v[:, by_col], axis=1)], axis=1)
        total = (t if channel is None else channel[live]) + run[:, cp[1:]] - run[:, cp[:-1]]
        t = np.clip(total, -LLR_SAT, LLR_SAT)
        v2c = np.clip(total[:, col] - c2v, -LLR_SAT, LLR_SAT)
        # syndrome over the signs of the totals
        clean = ~_dirty(g, (t < 0).astype(np.uint8))
        tot[live] = t
        ok[live[clean]] = True
        iters[live[clean]] = it + 1
        live, t, v2c = live[~clean], t[~clean], v2c[~clean]
    return ok, iters, tot


def decode(g, data, parity, llr=None, max_iterations=0):
    """(ok u8, iterations u32, data', hard) of every row.  llr (int8, channel order) selects
    the soft path, which reads neither data nor parity and never leaves at iteration 0."""
    ib, cb, n = _sizes(g)
    if max_iterations == 0:
        max_iterations = 50
    data = np.ascontiguousarray(data, dtype=np.uint8)
    rows = data.shape[0]
    ok = np.zeros(rows, bool)
    iters = np.zeros(rows, np.int64)
    hard = np.zeros((rows, cb), np.uint8)
    if llr is None:
        image = received(g, data, parity)
        bits = _bits(image, n)
        todo = _dirty(g, bits)
        ok[~todo], hard[~todo] = True, image[~todo]  # a clean row leaves at once, its byte image as it is
        tot, channel = np.where(bits[todo] != 0, -LLR_HARD, LLR_HARD).astype(np.int64), None
    else:
        l = np.ascontiguousarray(llr, dtype=np.int8).astype(np.int64)
        assert l.shape == (rows, n)
        if g["inner_forward"] is not None:
            l = l[:, g["inner_forward"]]
        todo = np.ones(rows, bool)
        channel = l * 256
        tot = np.clip(channel, -LLR_SAT, LLR_SAT)
    if todo.any():
        ok[todo], iters[todo], tot = _iterate(g, tot, channel, max_iterations)
        hard[todo] = _bytes((tot < 0).astype(np.uint8), cb)
    out = data.copy()  # a failed row keeps its data
    won = hard[ok][:, :ib]
    out[ok] = won if g["outer_forward"] is None else won[:, g["outer_forward"]]
    return ok.astype(np.uint8), iters.astype(np.uint32), out, hard
