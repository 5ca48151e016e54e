"""Host batches past one pipeline chunk (api.cpp: poporon_encode_batch,
poporon_decode_batch and their _multi forms).

A host batch is cut into chunks of 2^18 codewords that cycle through three
pinned slots; a slot's results are scattered back to the caller only when the
slot is needed again.  These cases reach the second chunk, a partial tail (which
takes another kernel route inside the same call), slot reuse (four chunks), the
c0 offsets into every caller array, the aligned erasure layout of a chunk,
corrected == NULL and the whole-row fast path (parity == data + size with equal
strides, which the ctypes wrapper can never produce: called directly here).

Inputs are built so that the expected result of every row is known without
the library: `clean` rows come from the CPU oracle's encoder, row c gets e_c
errors (e_c cycles through 0..t, so the row decodes to clean[c] with
corrected == e_c), every 997th row gets t + 1 .. t + 4 errors and is judged by
the oracle's decoder, and the four rows around every chunk boundary carry
pairwise different error counts, so a row that lands in the wrong place shows
in `corrected` as well as in the bytes.  Every row is compared.

Two kinds of rows do not follow from their construction, because the
reference itself does not return them clean, and are judged by the oracle's
decoder instead: rows that carry errors beside an erasure list (the reference
reports success but applies the magnitudes to the bytes the list names by
root index, quirks Q1 and Q2), and all rows of the (8, 0x187, 5, 7, 48) code,
most of which the reference gives up on.
"""
import ctypes as C

import numpy as np
import pytest

import libpoporon_amd as P
from oracle import BchOracle, Oracle

pytestmark = pytest.mark.gpu

CHUNK = 1 << 18  # kPipeChunk (api.cpp)
K, NR, N = 223, 32, 255
THREADS = 16


def _need_gpu():
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")


def _ptr(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _call(ok, what):
    assert ok, f"{what} failed: {P.last_error()}"


def _clean_rows(o, count, size, seed):
    rng = np.random.default_rng(seed)
    rows = np.empty((count, size + o.nroots), np.uint8)
    rows[:, :size] = rng.integers(0, 256, (count, size), dtype=np.uint8)
    rows[:, size:] = o.encode_batch(rows[:, :size], threads=THREADS)
    rows.setflags(write=False)
    return rows


@pytest.fixture(scope="module")
def clean255():
    """3 * 2^18 + 2^14 + 5 RS(255,223) codewords from the oracle's encoder"""
    return _clean_rows(Oracle(), 3 * CHUNK + (1 << 14) + 5, K, 0xC1EA)


@pytest.fixture(scope="module")
def clean72():
    """2 * (3 * 2^18) + 74 codewords of the code shortened to 40 data bytes"""
    return _clean_rows(Oracle(), 2 * 3 * CHUNK + 74, 40, 0xC1EB)


def _error_counts(count, t, bounds):
    """e_c: c mod (t + 1); t + 1 .. t + 4 on every 997th row; pairwise different
    nonzero counts on the rows c0 - 2 .. c0 + 1 around every boundary c0"""
    c = np.arange(count)
    ne = c % (t + 1)
    heavy = c % 997 == 996
    ne[heavy] = t + 1 + (c[heavy] // 997) % 4
    for c0 in bounds:
        for d, e in zip((-2, -1, 0, 1), (t, 1, t - 3, 2)):
            if 0 <= c0 + d < count:
                ne[c0 + d] = e
                heavy[c0 + d] = False
    return ne, heavy


def _inject(rng, rows, ne, step, lo=0, span=None):
    """XOR ne[c] nonzero bytes into row c at lo + (a_c + j * step) mod span, j < ne[c]
    (step coprime to span: the positions of a row are distinct)"""
    count = rows.shape[0]
    span = rows.shape[1] - lo if span is None else span
    assert np.gcd(step, span) == 1 and ne.max() <= span
    a = rng.integers(0, span, count)
    for j in range(int(ne.max())):
        sel = np.nonzero(ne > j)[0]
        rows[sel, lo + (a[sel] + j * step) % span] ^= rng.integers(1, 256, sel.size, dtype=np.uint8)


def _channel(o, clean, size, seed, step, bounds, by_construction=True):
    """(received rows, expected ok, expected corrected, expected rows).  Rows of
    at most t errors are expected back clean with corrected == e_c; the heavy
    rows (all rows where by_construction is off) are judged by the oracle."""
    count = clean.shape[0]
    t = o.nroots // 2
    rng = np.random.default_rng(seed)
    ne, heavy = _error_counts(count, t, bounds)
    bad = clean.copy()
    _inject(rng, bad, ne, step)
    ok = np.ones(count, np.uint8)
    cor = ne.astype(np.uint8)
    rows = clean.copy()
    h = np.nonzero(heavy)[0] if by_construction else np.arange(count)
    hok, hcor, hd, hp = o.decode_batch(bad[h, :size], bad[h, size:], threads=THREADS)
    assert not hok.all()  # failures (rows left as received) are among them
    ok[h], cor[h] = hok, hcor
    rows[h, :size], rows[h, size:] = hd, hp
    return bad, ok, cor, rows


def _bounds(count, first=0):
    """chunk boundaries of a range of `count` rows starting at row `first`"""
    return [first + c0 for c0 in range(CHUNK, count, CHUNK)]


def _compare(what, got, want):
    """every row: ok, corrected (where given) and all bytes; names the first row and its chunk"""
    for name, g, w in zip(("ok", "corrected", "rows"), got, want):
        if g is None:
            continue
        bad = (g != w) if g.ndim == 1 else (g != w).any(1)
        if bad.any():
            c = int(np.nonzero(bad)[0][0])
            pytest.fail(f"{what}: {name} differs at row {c} (chunk {c // CHUNK}, offset {c % CHUNK}); "
                        f"{int(bad.sum())} rows differ; got {g[c][:8] if g.ndim > 1 else g[c]}, "
                        f"expected {w[c][:8] if w.ndim > 1 else w[c]}")


# ---------------------------------------------------------------------------
# wire rows, 4 chunks: the `rows` branch, slot reuse, a 37-codeword tail
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_corrected", [True, False])
def test_wire_rows_four_chunks(clean255, with_corrected):
    """RS(255,223), 3 * 2^18 + 37 rows of one [count, 255] array, parity ==
    data + 223 and both strides 255: whole rows move (the `rows` branch), slot
    0 is reused for the 37-codeword tail, which decodes on the small-batch
    kernel while the chunks before it took the split kernels."""
    _need_gpu()
    count = 3 * CHUNK + 37
    o = Oracle()
    bad, wok, wcor, wrows = _channel(o, clean255[:count], K, 11, 37, _bounds(count))
    h = P.Poporon.default()
    buf = bad.copy()
    ok = np.full(count + 64, 0xEE, np.uint8)
    cor = np.full(count + 64, 0xEE, np.uint8)
    _call(P.load_library().poporon_decode_batch(h.h, _ptr(buf), N, _ptr(buf, K), N, K, count, None, 0, None, _ptr(ok),
                                                _ptr(cor) if with_corrected else None), "poporon_decode_batch")
    _compare("wire rows", (ok[:count], cor[:count] if with_corrected else None, buf), (wok, wcor, wrows))
    assert (ok[count:] == 0xEE).all() and (cor[count if with_corrected else 0:] == 0xEE).all()


# ---------------------------------------------------------------------------
# separate arrays, padded strides, a shortened code, a one-codeword second chunk
# ---------------------------------------------------------------------------
def test_padded_strides_one_row_tail(clean72):
    """size 40 in rows 48 bytes apart, parity in an array of its own 37 bytes
    apart, 2^18 + 1 rows: the second chunk is one codeword.  The pad bytes
    start out random and stay as they were, through encode and decode."""
    _need_gpu()
    size, ds, ps = 40, 48, 37
    count = CHUNK + 1
    o = Oracle()
    clean = clean72[:count]
    lib = P.load_library()
    h = P.Poporon.default()
    rng = np.random.default_rng(21)
    data = rng.integers(0, 256, (count + 1, ds), dtype=np.uint8)  # one guard row behind
    par = rng.integers(0, 256, (count + 1, ps), dtype=np.uint8)
    data[:count, :size] = clean[:, :size]
    d0, p0 = data.copy(), par.copy()
    _call(lib.poporon_encode_batch(h.h, _ptr(data), ds, _ptr(par), ps, size, count), "poporon_encode_batch")
    want_p = p0.copy()
    want_p[:count, :NR] = clean[:, size:]
    _compare("padded encode", (None, None, par), (None, None, want_p))
    assert (data == d0).all(), "encode wrote the data array"
    # decode the same layout
    bad, wok, wcor, wrows = _channel(o, clean, size, 22, 7, _bounds(count))
    data[:count, :size], par[:count, :NR] = bad[:, :size], bad[:, size:]
    want_d, want_p = data.copy(), par.copy()
    want_d[:count, :size], want_p[:count, :NR] = wrows[:, :size], wrows[:, size:]
    ok = np.full(count + 64, 0xEE, np.uint8)
    cor = np.full(count + 64, 0xEE, np.uint8)
    _call(lib.poporon_decode_batch(h.h, _ptr(data), ds, _ptr(par), ps, size, count, None, 0, None, _ptr(ok),
                                   _ptr(cor)), "poporon_decode_batch")
    _compare("padded decode (data array)", (ok[:count], cor[:count], data), (wok, wcor, want_d))
    _compare("padded decode (parity array)", (None, None, par), (None, None, want_p))
    assert (ok[count:] == 0xEE).all() and (cor[count:] == 0xEE).all()


# ---------------------------------------------------------------------------
# erasures across chunks
# ---------------------------------------------------------------------------
def _erasure_channel(o, clean, size, seed, pstride, bounds):
    """Row c: cnt_c in (0, 1, 8, 16, 31, 32) sorted distinct erasure slots in
    [0, size) whose bytes are replaced by different ones; slots past the count
    stay 0 (quirk Q2).  Every fifth row, and the rows around a boundary, also
    get e_c errors in the parity bytes, 2 e_c + cnt_c <= 32.

    Returns (received rows, positions, counts, expected ok, corrected, rows).
    A row with erasures only comes back clean with corrected == cnt_c.  With an
    erasure list attached the reference reports success on a row that has
    errors too but puts their magnitudes at the bytes the list names by root
    index (quirks Q1, Q2), so those rows do not come back clean: they, every
    256th row and the boundary rows are judged by the oracle's decoder."""
    count = clean.shape[0]
    rng = np.random.default_rng(seed)
    c = np.arange(count)
    cnt = np.array([0, 1, 8, 16, 31, 32])[c % 6]
    ne = np.where(c % 5 == 2, np.minimum((c // 30) % 17, (NR - cnt) // 2), 0)
    edge = np.zeros(count, bool)
    for c0 in bounds:  # rows around a boundary: pairwise different (count, errors)
        for d, (k, e) in zip((-2, -1, 0, 1), ((8, 12), (16, 8), (1, 15), (31, 0))):
            if 0 <= c0 + d < count:
                cnt[c0 + d], ne[c0 + d], edge[c0 + d] = k, e, True
    gap = 1 + (c // 36) % max(1, (size - 1) // 31)  # slot j at a_c + j * gap, the last one < size
    a = rng.integers(0, size, count) % (size - 31 * gap)
    pos = np.zeros((count, pstride), np.uint8)
    bad = clean.copy()
    for j in range(NR):
        sel = np.nonzero(cnt > j)[0]
        p = a[sel] + j * gap[sel]
        pos[sel, j] = p
        bad[sel, p] ^= rng.integers(1, 256, sel.size, dtype=np.uint8)
    _inject(rng, bad, ne, 5, lo=size, span=NR)
    cnt = cnt.astype(np.uint8)
    ok, cor, rows = np.ones(count, np.uint8), cnt.copy(), clean.copy()
    r = np.nonzero((ne > 0) | edge | (c % 256 == 0) | (c == count - 1))[0]
    ook, ocor, od, op = o.decode_batch(bad[r, :size], bad[r, size:], pos[r].astype(np.uint32),
                                       cnt[r].astype(np.uint32), threads=THREADS)
    assert ook.all()  # within capacity: the reference says yes, whatever it wrote
    pure = ne[r] == 0
    assert (ocor[pure] == cnt[r][pure]).all() and (od[pure] == clean[r[pure], :size]).all()
    ok[r], cor[r] = ook, ocor
    rows[r, :size], rows[r, size:] = od, op
    assert (rows[r] != clean[r]).any(1).sum() > len(r) // 4  # the quirk rows are among them
    return bad, pos, cnt, ok, cor, rows


def test_erasures_across_chunks(clean255):
    """RS(255,223), 3 * 2^18 + 2^14 + 5 rows (a tail that takes the split
    kernels too), positions 40 bytes apart: the c0 offsets into positions and
    counts and the 16-byte-aligned position block of every chunk."""
    _need_gpu()
    count = clean255.shape[0]
    bad, pos, cnt, wok, wcor, wrows = _erasure_channel(Oracle(), clean255, K, 31, 40, _bounds(count))
    h = P.Poporon.default()
    ok, cor, d, p = h.decode_batch(bad[:, :K], bad[:, K:], pos, cnt)
    _compare("erasures", (ok, cor, np.concatenate([d, p], 1)), (wok, wcor, wrows))


# ---------------------------------------------------------------------------
# a general-parameter code (rs_generic.hip) and BCH through the same pipeline
# ---------------------------------------------------------------------------
def test_general_code_two_chunks():
    """(8, 0x187, 5, 7, 48): full-length rows of 207 + 48 bytes, 2^18 + 300 of
    them, through the Poporon wrapper.  The reference does not decode this
    code up to t = 24: it gives up on about 30 % of the rows with one error and
    on most rows with more (the oracle and the compiled reference agree on
    that, row for row), so no row's result follows from its construction and
    every row is judged by the oracle's decoder."""
    _need_gpu()
    params = (8, 0x187, 5, 7, 48)
    o = Oracle(*params)
    size, count = 255 - 48, CHUNK + 300
    clean = _clean_rows(o, count, size, 41)
    h = P.Poporon(*params)
    assert (h.encode_batch(clean[:, :size]) == clean[:, size:]).all()
    bad, wok, wcor, wrows = _channel(o, clean, size, 42, 37, _bounds(count), by_construction=False)
    assert wok[CHUNK:].any() and wok.sum() > count // 20 and wcor[wok == 1].max() > 4
    ok, cor, d, p = h.decode_batch(bad[:, :size], bad[:, size:])
    _compare("general code", (ok, cor, np.concatenate([d, p], 1)), (wok, wcor, wrows))


def test_bch_two_chunks():
    """BCH (5, 0x25, 3), 2^18 + 300 rows: the pipeline's row width comes from
    par_bytes(), which is not num_roots here.  Codewords with c mod 6 bit
    errors and, on every eighth row, a uniform word; all against the oracle."""
    _need_gpu()
    o = BchOracle(5, 0x25, 3)
    count = CHUNK + 300
    rng = np.random.default_rng(51)
    msgs = rng.integers(0, 1 << o.k, count, dtype=np.uint64)
    data = o.word_images(msgs << np.uint64(o.pbits), junk=np.arange(count))[0]
    par = o.encode_batch(data)
    h = P.Bch(5, 0x25, 3)
    assert (h.parity_size, h.info_size) == (o.parity_bytes, o.data_bytes)
    assert (h.encode_batch(data) == par).all()
    pv = np.zeros(count, np.uint64)
    for i in range(o.parity_bytes):
        pv = (pv << np.uint64(8)) | par[:, i].astype(np.uint64)
    words = (msgs << np.uint64(o.pbits)) | pv
    c = np.arange(count)
    ne = c % 6
    a = rng.integers(0, 31, count)
    for j in range(5):
        words ^= np.where(ne > j, np.uint64(1) << ((a + 7 * j) % 31).astype(np.uint64), np.uint64(0))
    uni = c % 8 == 7
    words[uni] = rng.integers(0, 1 << 31, int(uni.sum()), dtype=np.uint64)
    rd, rp = o.word_images(words, junk=c)
    wok, wcor, wout = o.decode_batch(rd, rp)
    # by construction: up to 3 flipped bits are corrected, to the message sent
    near = ~uni & (ne <= 3)
    assert wok[near].all() and (wcor[near] == ne[near]).all()
    assert (wout[near] == o.word_images(msgs[near] << np.uint64(o.pbits))[0]).all()
    assert not wok.all()
    ok, cor, d, p = h.decode_batch(rd, rp)
    _compare("BCH", (ok, cor, d), (wok, wcor.astype(np.uint8), wout))
    assert (p == rp).all()


# ---------------------------------------------------------------------------
# multi: two handles on one device, each range four chunks with a tail
# ---------------------------------------------------------------------------
def test_multi_two_handles(clean72):
    """P.Multi(devices=[0, 0]) over 2 * (3 * 2^18) + 74 rows of size 40: each
    handle's range is 3 * 2^18 + 37 rows, so both pipelines reuse a slot and
    end on a tail, on their own host threads.  Results equal the single
    handle's expectation: encode, decode, decode with erasures."""
    _need_gpu()
    size = 40
    count = clean72.shape[0]
    half = count // 2
    assert P.shard_range(count, 1, 2) == (half, count) and half == 3 * CHUNK + 37
    bounds = _bounds(half) + [half] + _bounds(count - half, half)
    o = Oracle()
    m = P.Multi(devices=[0, 0])
    assert m.devices == 2
    par = m.encode_batch(clean72[:, :size])
    _compare("multi encode", (None, None, par), (None, None, clean72[:, size:]))
    bad, wok, wcor, wrows = _channel(o, clean72, size, 61, 7, bounds)
    ok, cor, d, p = m.decode_batch(bad[:, :size], bad[:, size:])
    _compare("multi decode", (ok, cor, np.concatenate([d, p], 1)), (wok, wcor, wrows))
    del bad, wrows, d, p
    bad, pos, cnt, wok, wcor, wrows = _erasure_channel(o, clean72, size, 62, 36, bounds)
    ok, cor, d, p = m.decode_batch(bad[:, :size], bad[:, size:], pos, cnt)
    _compare("multi erasures", (ok, cor, np.concatenate([d, p], 1)), (wok, wcor, wrows))
