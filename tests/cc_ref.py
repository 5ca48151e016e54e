"""numpy model of the K = 7 convolutional code of include/poporon_amd.h (poporon_cc_encode_device,
poporon_cc_decode_device): a restatement of the header's contract, nothing shared with cc.hip.

A code is (g0, g1, invert), a puncture pattern (period, keep0, keep1).  Bits and symbols are arrays of 0 / 1
here (pack / unpack give the MSB-first bytes of the calls), LLRs int8 arrays of the kept symbols.  The
decoder's add-compare-select runs over the 64 states and over all blocks of a frame at once, with a
Python loop over the at most B + 2V steps of a window."""
import numpy as np

CCSDS = (0o171, 0o133, 2)
DVB = (0o171, 0o133, 0)
RATE_1_2 = (1, 0b1, 0b1)
DVB_2_3 = (2, 0b01, 0b11)
DVB_3_4 = (3, 0b101, 0b011)
DVB_5_6 = (5, 0b10101, 0b01011)
DVB_7_8 = (7, 0b1010001, 0b0101111)
INF = 1 << 40  # a state no path reaches


def _parity(x):
    return bin(int(x)).count("1") & 1


def outputs(code, u, s):
    """(output 0, output 1, next state) for input bit u in state s"""
    g0, g1, inv = code
    r = (u << 6) | s
    return _parity(r & g0) ^ (inv & 1), _parity(r & g1) ^ ((inv >> 1) & 1), r >> 1


def kept(punct, t):
    """which of step t's two outputs are transmitted"""
    period, k0, k1 = punct
    return (k0 >> (t % period)) & 1, (k1 >> (t % period)) & 1


def n_symbols(punct, nbits):
    """kept symbols of nbits steps (plain Python integers: any nbits)"""
    period, k0, k1 = punct
    per = [((k0 >> k) & 1) + ((k1 >> k) & 1) for k in range(period)]
    return nbits // period * sum(per) + sum(per[:nbits % period])


def n_blocks(block, nbits):
    return -(-nbits // block)


def pack(bits):
    """0 / 1 array -> MSB-first bytes, spare low bits 0"""
    return np.packbits(np.asarray(bits, np.uint8))


def unpack(data, n):
    return np.unpackbits(np.asarray(data, np.uint8))[:n]


def encode(code, punct, bits, start_state=0):
    """(kept symbols as 0 / 1, end state): encode_literal over whole arrays"""
    g0, g1, inv = code
    period, k0, k1 = punct
    bits = np.asarray(bits, np.uint8)
    n = len(bits)
    x = np.concatenate([[(start_state >> i) & 1 for i in range(6)], bits]).astype(np.uint8)  # x[6 + t] = input t
    out = np.zeros((n, 2), np.uint8)
    for j, g in enumerate((g0, g1)):
        out[:, j] = (inv >> j) & 1
        for k in range(7):  # register bit 6 - k holds input t - k
            if (g >> (6 - k)) & 1:
                out[:, j] ^= x[6 - k:6 - k + n]
    t = np.arange(n)
    keep = np.stack([(k0 >> (t % period)) & 1, (k1 >> (t % period)) & 1], 1).astype(bool)
    return out[keep], sum(int(x[n + i]) << i for i in range(6))


def encode_literal(code, punct, bits, start_state=0):
    """(kept symbols as 0 / 1, end state), step by step"""
    s, out = start_state, []
    for t, u in enumerate(np.asarray(bits).tolist()):
        o0, o1, s = outputs(code, u, s)
        k0, k1 = kept(punct, t)
        if k0:
            out.append(o0)
        if k1:
            out.append(o1)
    return np.array(out, np.uint8), s


def depuncture(punct, llr, nbits):
    """int64[nbits, 2]: the received value of every output of every step, 0 where punctured"""
    period, k0, k1 = punct
    t = np.arange(nbits)
    keep = np.stack([(k0 >> (t % period)) & 1, (k1 >> (t % period)) & 1], 1).astype(bool)
    v = np.zeros((nbits, 2), np.int64)
    assert int(keep.sum()) == len(llr) == n_symbols(punct, nbits)
    v[keep] = np.asarray(llr, np.int64)  # row-major: a step's output 0 before its output 1
    return v


def _tables(code):
    """pred[d][s'], label[d][s'] = output 0 + 2 * output 1 of the branch from pred[d][s'] to s'"""
    pred = np.zeros((2, 64), np.int64)
    lab = np.zeros((2, 64), np.int64)
    for s2 in range(64):
        for d in (0, 1):
            p = ((s2 << 1) | d) & 63
            o0, o1, nxt = outputs(code, s2 >> 5, p)
            assert nxt == s2
            pred[d, s2], lab[d, s2] = p, o0 + 2 * o1
    return pred, lab


def _costs(v):
    """int64[..., 4]: the cost of the label o0 + 2 * o1 for the received pair v[..., 2]"""
    c = [np.where(v < 0, -v, 0), np.where(v > 0, v, 0)]  # c[b]: the cost of hypothesising bit b
    return np.stack([c[l & 1][..., 0] + c[l >> 1][..., 1] for l in range(4)], -1)


def decode(code, punct, llr, nbits, block, overlap, start_state=-1, end_state=-1):
    """one frame: (bits uint8[nbits], metric int64[blocks])"""
    pred, lab = _tables(code)
    v = depuncture(punct, llr, nbits)
    nb = n_blocks(block, nbits)
    e0 = np.arange(nb, dtype=np.int64) * block
    e1 = np.minimum(nbits, e0 + block)
    t0 = np.maximum(0, e0 - overlap)
    t1 = np.minimum(nbits, e0 + block + overlap)
    n = t1 - t0
    metric = np.zeros((nb, 64), np.int64)
    if start_state >= 0:
        first = t0 == 0
        metric[first] = INF
        metric[first, start_state] = 0
    steps = int(n.max())
    dec = np.zeros((steps, nb), np.uint64)
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    rows = np.arange(nb)[:, None]
    for i in range(steps):
        live = i < n
        cost = _costs(v[np.minimum(t0 + i, nbits - 1)])  # [nb, 4]
        m0 = metric[:, pred[0]] + cost[rows, lab[0][None, :]]
        m1 = metric[:, pred[1]] + cost[rows, lab[1][None, :]]
        d = m1 < m0  # a tie goes to d = 0
        metric = np.where(live[:, None], np.where(d, m1, m0), metric)
        dec[i] = (d * weights).sum(1, dtype=np.uint64)
    state = np.argmin(metric, 1)  # the first of the least: ties to the lowest state
    if end_state >= 0:
        state = np.where(t1 == nbits, end_state, state)
    out_metric = metric[np.arange(nb), state]
    bits = np.zeros(nbits, np.uint8)
    for i in range(steps - 1, -1, -1):
        live = i < n
        t = t0 + i
        emit = live & (t >= e0) & (t < e1)
        bits[t[emit]] = (state[emit] >> 5).astype(np.uint8)
        dbit = ((dec[i] >> state.astype(np.uint64)) & np.uint64(1)).astype(np.int64)
        state = np.where(live, ((state << 1) | dbit) & 63, state)
    return bits, out_metric


def path_cost(code, punct, llr, bits, start_state):
    """the contract's metric of the path that `bits` takes from start_state; also its end state"""
    v = depuncture(punct, llr, len(bits))
    s, total = start_state, 0
    for t, u in enumerate(np.asarray(bits).tolist()):
        o0, o1, s = outputs(code, u, s)
        for o, x in ((o0, int(v[t, 0])), (o1, int(v[t, 1]))):
            if x != 0 and (x < 0) != bool(o):
                total += abs(x)
    return total, s


# ---- builders of LLR frames ------------------------------------------------------------------

def llr_clean(symbols, rng=None, low=1, high=127):
    """noise-free: the sign says the symbol (negative = 1), magnitudes random in [low, high] (or all `high`)"""
    n = len(symbols)
    mag = np.full(n, high, np.int64) if rng is None else rng.integers(low, high + 1, n)
    return np.where(np.asarray(symbols) != 0, -mag, mag).astype(np.int8)


def llr_awgn(symbols, rng, sigma, scale=32.0):
    """BPSK over AWGN: y = (1 - 2 symbol) + sigma * noise, rint(scale * y) clipped to +-127"""
    y = 1.0 - 2.0 * np.asarray(symbols, np.float64) + sigma * rng.standard_normal(len(symbols))
    return np.clip(np.rint(scale * y), -127, 127).astype(np.int8)


def llr_ties(symbols, rng, flip=0.2, top=2):
    """crafted ties: magnitudes 0 .. top, a fraction `flip` of the signs wrong"""
    n = len(symbols)
    mag = rng.integers(0, top + 1, n)
    sym = np.asarray(symbols) ^ (rng.random(n) < flip)
    return np.where(sym != 0, -mag, mag).astype(np.int8)
