"""The soft-decision RS decode (Chase-2 over int8 bit LLRs, include/poporon_amd.h) as a numpy model
over the oracle's row decode, and the LLR rows the soft tests are built from.  No tests in here.

The contract, steps 1 to 6 of the header: the hard row is the signs of the LLRs (negative = 1, MSB
first); the `flips` picked bits are the first in ascending order of (|llr|, bit index); candidate p
flips pick k where bit k of p is set; every candidate goes through the errors-only row decode, and
failed ones are ignored; a candidate's score is the sum of |llr| over the bits in which its decoded
row differs from the hard row; the smallest score wins, ties to the lowest p; no winner gives the
hard row back with ok = 0 and zeros."""
import numpy as np

MAX_FLIPS = 6
HIGH = 100  # a reliable bit of a built row


def bit_weights(m):
    return (1 << np.arange(m - 1, -1, -1)).astype(np.uint8)


def hard_rows(llr, W, m):
    """(count, W) uint8: the signs of (count, >= W*m) int8 LLRs, MSB first"""
    L = np.asarray(llr, np.int8)[:, :W * m].reshape(-1, W, m)
    return ((L < 0) * bit_weights(m)).sum(2).astype(np.uint8)


def magnitudes(llr, W, m):
    """(count, W*m) int32: |llr|, -128 -> 128"""
    return np.abs(np.asarray(llr, np.int8)[:, :W * m].astype(np.int32))


def picks(llr, W, m, flips):
    """(count, flips) bit indices: ascending (magnitude, index)"""
    mag = magnitudes(llr, W, m)
    key = mag * 4096 + np.arange(W * m)[None, :]
    return np.argsort(key, 1, kind="stable")[:, :flips]


def candidates(llr, W, m, flips):
    """(count, 2^flips, W) uint8"""
    hard = hard_rows(llr, W, m)
    count, P = hard.shape[0], 1 << flips
    pick = picks(llr, W, m, flips)
    cand = np.repeat(hard[:, None, :], P, 1)
    rows, ps = np.arange(count)[:, None], np.arange(P)[None, :]
    for k in range(flips):
        sym, bit = pick[:, k] // m, m - 1 - pick[:, k] % m
        on = ((np.arange(P) >> k) & 1).astype(np.uint8)
        cand[rows, ps, sym[:, None]] ^= (on[None, :] << bit[:, None]).astype(np.uint8)
    return cand


def soft_decode(orc, llr, size, m, flips, threads=0):
    """The model.  llr: (count, >= (size + nroots)*m) int8.  Returns a dict: ok u8[count], rows
    u8[count, W] (message then parity), changed, pattern, score (int64[count]), and cand_ok
    u8[count, 2^flips]."""
    assert 0 <= flips <= MAX_FLIPS
    W = size + orc.nroots
    hard = hard_rows(llr, W, m)
    mag = magnitudes(llr, W, m)
    count, P = hard.shape[0], 1 << flips
    flat = candidates(llr, W, m, flips).reshape(count * P, W)
    ok, _, d, p = orc.decode_batch(flat[:, :size], flat[:, size:], threads=threads)
    out = np.concatenate([d, p], 1).reshape(count, P, W)
    ok = (ok.reshape(count, P) != 0)
    diff = out ^ hard[:, None, :]
    dbits = (diff[..., None] >> np.arange(m - 1, -1, -1)) & 1
    score = (dbits * mag.reshape(count, 1, W, m)).sum((2, 3)).astype(np.int64)
    score = np.where(ok, score, np.int64(1) << 40)
    best = score.argmin(1)  # the first minimum: the lowest p
    win = ok.any(1)
    idx = np.arange(count)
    rows = np.where(win[:, None], out[idx, best], hard)
    return {"ok": win.astype(np.uint8), "rows": rows, "changed": (rows != hard).sum(1),
            "pattern": np.where(win, best, 0), "score": np.where(win, score[idx, best], 0),
            "cand_ok": ok.astype(np.uint8), "hard": hard}


def soft_decode_literal(orc, llr_row, size, m, flips):
    """One codeword, as the header words it: loops, and one Oracle.decode per candidate"""
    W = size + orc.nroots
    llr_row = [int(v) for v in np.asarray(llr_row, np.int8)[:W * m]]
    hard = [0] * W
    for s in range(W):
        for j in range(m):
            if llr_row[s * m + j] < 0:
                hard[s] |= 1 << (m - 1 - j)
    order = sorted(range(W * m), key=lambda b: (abs(llr_row[b]), b))[:flips]
    winner = None
    for p in range(1 << flips):
        cand = list(hard)
        for k, b in enumerate(order):
            if (p >> k) & 1:
                cand[b // m] ^= 1 << (m - 1 - b % m)
        ok, _, d, par = orc.decode(np.array(cand[:size], np.uint8), np.array(cand[size:], np.uint8))
        if not ok:
            continue
        y = [int(v) for v in d] + [int(v) for v in par]
        score = 0
        for s in range(W):
            for j in range(m):
                if ((y[s] ^ hard[s]) >> (m - 1 - j)) & 1:
                    score += abs(llr_row[s * m + j])
        if winner is None or score < winner[0]:
            winner = (score, p, y)
    if winner is None:
        return 0, hard, 0, 0, 0
    score, p, y = winner
    return 1, y, sum(a != b for a, b in zip(y, hard)), p, score


# ---- LLR rows ------------------------------------------------------------------------------

def codewords(orc, size, m, count, rng):
    msg = rng.integers(0, 1 << m, (count, size), dtype=np.uint8)
    return np.concatenate([msg, orc.encode_batch(msg)], 1)


def clean_llr(cw, m, high=HIGH):
    """(count, W*m) int32: +-high by the codewords' bits"""
    bits = (cw[..., None] >> np.arange(m - 1, -1, -1)) & 1
    return np.where(bits == 1, -high, high).astype(np.int32).reshape(cw.shape[0], -1)


def built_rows(orc, size, m, count, weak, rng, total=None):
    """`count` codewords and their LLR rows with `total` (default t + weak, t = nroots // 2) symbol errors
    each, reliable bits at +-HIGH: `weak` of them single-bit flips of magnitude 1..7, the rest multi-bit
    (any non-zero symbol error) of magnitude 10..59.  Returns (codewords u8[count, W], llr int8[count, W*m])."""
    nr = orc.nroots
    W = size + nr
    total = nr // 2 + weak if total is None else total
    total = min(total, W)
    weak = min(weak, total)
    cw = codewords(orc, size, m, count, rng)
    llr = clean_llr(cw, m).reshape(count, W, m)
    for c in range(count):
        for i, s in enumerate(rng.choice(W, total, replace=False)):
            if i < weak:
                b = rng.integers(m)
                llr[c, s, b] = -np.sign(llr[c, s, b]) * rng.integers(1, 8)
            else:
                e = int(rng.integers(1, 1 << m))
                for b in range(m):
                    if (e >> (m - 1 - b)) & 1:
                        llr[c, s, b] = -np.sign(llr[c, s, b]) * rng.integers(10, 60)
    return cw, llr.reshape(count, W * m).astype(np.int8)


def awgn_llr(cw, m, ebn0_db, rate, rng, scale=32.0):
    """BPSK over AWGN: bit 0 -> +1, bit 1 -> -1, y = x + n at the given Eb/N0 for a code of `rate`;
    LLR = rint(scale * y) clipped to +-127.  int8[count, W*m]."""
    bits = ((cw[..., None] >> np.arange(m - 1, -1, -1)) & 1).reshape(cw.shape[0], -1)
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (ebn0_db / 10.0)))
    y = (1.0 - 2.0 * bits) + sigma * rng.standard_normal(bits.shape)
    return np.clip(np.rint(scale * y), -127, 127).astype(np.int8)
