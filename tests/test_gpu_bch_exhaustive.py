"""The binary BCH codec (bch.hip) on every input there is, and on the launch
shapes no other test reaches.

bch_decode_k restates the reference's Berlekamp-Massey with tracked degree
bounds and rotating LDS buffers, and poporon_create accepts every t in 1..16
for symbol sizes 3..5: the degenerate codes too (k = 1, k = 0 with an empty
data image, 2t larger than the codeword).  The codeword spaces of m = 3 and 4
are tiny, so every received word of every accepted code is decoded, through the
host batch and the device API, and compared bit for bit with the CPU oracle
(oracle/bch_oracle.c, itself compared with the compiled reference on the same
words by tests/test_oracle_golden.py): the bool, corrected_num and the data
bytes.  m = 5 gets structured and random words; two codes get the grid-stride
loop, the block edges and strided layouts.

Every expected value comes from the oracle or from how the input was built.
"""
import itertools

import numpy as np
import pytest

import libpoporon_amd as P
from oracle import BchOracle

pytestmark = pytest.mark.gpu

SMALL = [(m, poly, t) for m, poly in ((3, 0x0B), (3, 0x0D), (4, 0x13), (4, 0x19)) for t in range(1, 17)]
M5 = [(5, 0x25, t) for t in range(1, 17)] + [(5, 0x3D, t) for t in (1, 4, 8, 16)]
SHAPES = [(4, 0x13, 3), (5, 0x25, 7)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _handle(m, poly, t):
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    # the reference serves every one of these codes: a refusal here is a finding
    return P.Bch(m, poly, t)


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _first(bad):
    return int(np.nonzero(bad)[0][0])


def _same(what, code, words, got, want):
    """(ok, corrected, data') of the library == the oracle's; names the first word that differs"""
    for name, g, w in zip(("ok", "corrected", "data"), got, want):
        bad = (g != w) if g.ndim == 1 else (g != w).any(1)
        if bad.any():
            c = _first(bad)
            pytest.fail(f"{what} {name} differs: (m, poly, t) = {code}, row {c}, word {int(words[c]):#x}: "
                        f"got {g[c]}, oracle {w[c]} ({int(bad.sum())} rows differ)")


def _decode_both(torch, h, o, code, words, junk=None):
    """Decode the words through the host batch and the device API (packed rows
    [data | parity]) and compare both with the oracle.  Returns the oracle's result."""
    data, parity = o.word_images(words, junk=np.arange(len(words)) if junk is None else junk)
    n, size = data.shape
    pb = o.parity_bytes
    want = o.decode_batch(data, parity)
    wok = want[0].astype(bool)
    # the yardstick itself: a failed row is left as received, with corrected 0
    assert (want[2][~wok] == data[~wok]).all() and not want[1][~wok].any()
    ok, cor, d, p = h.decode_batch(data, parity)
    _same("host batch", code, words, (ok, cor, d), want)
    assert (p == parity).all(), "host batch wrote parity bytes"
    rows = torch.from_numpy(np.concatenate([data, parity], 1)).cuda()
    okd = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    cord = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    h.decode_batch_device(rows.data_ptr(), size + pb, rows.data_ptr() + size, size + pb, size, n, okd.data_ptr(),
                          cord.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    out = rows.cpu().numpy()
    _same("device batch", code, words, (okd.cpu().numpy(), cord.cpu().numpy(), out[:, :size]), want)
    assert (out[:, size:] == parity).all(), "device batch wrote parity bytes"
    return want


def _encode_both(torch, h, o, code, msgs):
    """msgs: message values < 2^k.  Host batch and device API == oracle parity."""
    data = o.word_images(np.asarray(msgs, np.uint64) << np.uint64(o.pbits), junk=np.arange(len(msgs)))[0]
    n, size = data.shape
    pb = o.parity_bytes
    want = o.encode_batch(data)
    got = h.encode_batch(data)
    assert got.shape == want.shape
    assert (got == want).all(), (code, "host", _first((got != want).any(1)))
    rows = torch.from_numpy(np.concatenate([data, np.full((n, pb), 0xEE, np.uint8)], 1)).cuda()
    h.encode_batch_device(rows.data_ptr(), size + pb, rows.data_ptr() + size, size + pb, size, n, _stream(torch))
    torch.cuda.synchronize()
    out = rows.cpu().numpy()
    assert (out[:, size:] == want).all(), (code, "device", _first((out[:, size:] != want).any(1)))
    assert (out[:, :size] == data).all(), "encode wrote data bytes"
    return data, want


# ---------------------------------------------------------------------------
# 1. every received word of every accepted code, m = 3 and 4
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,poly,t", SMALL)
def test_bch_every_word(torch_cuda, m, poly, t):
    """All 2^nn received words (unused high bits of the top data and parity
    bytes set on odd rows) and all 2^k messages.  The k = 0 codes (one
    codeword, an empty data image) follow the reference: size must still be
    >= 1 and that data byte is left alone."""
    code = (m, poly, t)
    o, h = BchOracle(m, poly, t), _handle(m, poly, t)
    assert (h.parity_size, h.info_size) == (o.parity_bytes, o.data_bytes)
    nn = (1 << m) - 1
    words = np.arange(1 << nn, dtype=np.uint64)
    ok, cor, out = _decode_both(torch_cuda, h, o, code, words)
    # by construction: every word within distance t of the zero codeword decodes to it
    weight = np.array([bin(int(w)).count("1") for w in words])
    near = weight <= t
    assert ok[near].all() and (cor[near] == weight[near]).all()
    if o.k:  # a successful write clears the unused high bits too
        assert not out[near].any()
    _encode_both(torch_cuda, h, o, code, np.arange(1 << o.k, dtype=np.uint64))


# ---------------------------------------------------------------------------
# 2. m = 5: structured and random words
# ---------------------------------------------------------------------------
def _weight_patterns(rng, n, w):
    """n random 31-bit patterns of weight w"""
    idx = np.argsort(rng.random((n, 31)), axis=1)[:, :w].astype(np.uint64)
    return (np.uint64(1) << idx).sum(1, dtype=np.uint64)


@pytest.fixture(scope="module")
def m5_shared():
    """every error pattern of weight 0..3 (4992) and 2^16 uniform 31-bit words"""
    low = [0]
    for w in (1, 2, 3):
        low += [sum(1 << b for b in bits) for bits in itertools.combinations(range(31), w)]
    low = np.array(low, dtype=np.uint64)
    assert low.size == 4992
    return low, np.random.default_rng(0xB5).integers(0, 1 << 31, 1 << 16, dtype=np.uint64)


def _m5_words(o, t, shared, per_weight=2048):
    """(words, codeword of each row or -1, error weight of each row or -1)"""
    low, uniform = shared
    rng = np.random.default_rng(1000 * t + o.k)
    msgs = rng.integers(0, 1 << o.k, 32, dtype=np.uint64)
    msgs[0], msgs[1] = 0, (1 << o.k) - 1
    data = o.word_images(msgs << np.uint64(o.pbits))[0]
    par = o.encode_batch(data)
    pv = np.zeros(32, np.uint64)
    for i in range(o.parity_bytes):
        pv = (pv << np.uint64(8)) | par[:, i].astype(np.uint64)
    cw = (msgs << np.uint64(o.pbits)) | pv
    words = [(cw[:, None] ^ low[None, :]).ravel()]
    base = [np.repeat(cw, low.size)]
    wt = [np.tile(np.array([bin(int(x)).count("1") for x in low]), 32)]
    for w in (t, t + 1, min(31, -(-(t + 31) // 2))):
        w = min(w, 31)
        words.append(np.repeat(cw, per_weight) ^ _weight_patterns(rng, 32 * per_weight, w))
        base.append(np.repeat(cw, per_weight))
        wt.append(np.full(32 * per_weight, w))
    words.append(uniform)
    base.append(np.full(uniform.size, -1, np.int64).astype(np.uint64))
    wt.append(np.full(uniform.size, -1))
    return np.concatenate(words), np.concatenate(base), np.concatenate(wt)


@pytest.mark.parametrize("m,poly,t", M5)
def test_bch_m5_structured(torch_cuda, m5_shared, m, poly, t):
    """32 codewords (the all-zero and all-ones messages among them) under every
    error pattern of weight 0..3, 2048 random patterns each of weight t, t + 1
    and ceil((t + 31) / 2), and 2^16 uniform words: about 4.2e5 rows a code."""
    code = (m, poly, t)
    o, h = BchOracle(m, poly, t), _handle(m, poly, t)
    assert (h.parity_size, h.info_size) == (o.parity_bytes, o.data_bytes)
    words, base, wt = _m5_words(o, t, m5_shared)
    assert words.size == 32 * 4992 + 3 * 32 * 2048 + (1 << 16)
    ok, cor, out = _decode_both(torch_cuda, h, o, code, words)
    # by construction: at most t errors on a codeword are corrected, to that codeword
    near = (wt >= 0) & (wt <= t)
    assert ok[near].all() and (cor[near] == wt[near]).all()
    clean = o.word_images(base[near])[0]
    if o.k:
        assert (out[near] == clean).all()
    # failures are among the rows too, except on the two perfect codes (Hamming, 31-fold repetition)
    assert ok.any() and (t in (1, 15) or not ok.all())
    msgs = np.random.default_rng(t).integers(0, 1 << o.k, 4096, dtype=np.uint64)
    msgs[0], msgs[1] = 0, (1 << o.k) - 1
    _encode_both(torch_cuda, h, o, code, msgs)


# ---------------------------------------------------------------------------
# 3. launch shapes
# ---------------------------------------------------------------------------
def _shape_words(m, t, o, shared):
    if m == 4:
        return np.arange(1 << 15, dtype=np.uint64)
    return _m5_words(o, t, shared, per_weight=128)[0][::7]


@pytest.fixture(scope="module")
def tiled_4_13_3():
    """the exhaustive (4, 0x13, 3) set and its oracle result, computed once"""
    o = BchOracle(4, 0x13, 3)
    words = np.arange(1 << 15, dtype=np.uint64)
    data, parity = o.word_images(words, junk=words)
    return o, words, data, parity, o.decode_batch(data, parity)


def test_bch_grid_stride(torch_cuda, tiled_4_13_3):
    """2^20 + 3 rows: past 8 x 256 CUs x 256 lanes = 524288, so every lane of
    the capped grid decodes at least two codewords and reuses its LDS arrays
    (syndromes, the three polynomial buffers, positions) from the one before."""
    torch = torch_cuda
    o, words, data, parity, (wok, wcor, wout) = tiled_4_13_3
    h = _handle(4, 0x13, 3)
    n = (1 << 20) + 3
    # every word 32 times or more; rows c and c + 524288 (one lane's sequence) hold different words
    idx = np.arange(n)
    sel = (idx * 7 + idx // words.size) % words.size
    rows_np = np.concatenate([data, parity], 1)[sel]
    size, pb = data.shape[1], parity.shape[1]
    rows = torch.from_numpy(rows_np).cuda()
    okd = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    cord = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    h.decode_batch_device(rows.data_ptr(), size + pb, rows.data_ptr() + size, size + pb, size, n, okd.data_ptr(),
                          cord.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    out, ok, cor = rows.cpu().numpy(), okd.cpu().numpy(), cord.cpu().numpy()
    _same("grid-stride", (4, 0x13, 3), words[sel], (ok[:n], cor[:n], out[:, :size]), (wok[sel], wcor[sel], wout[sel]))
    assert (out[:, size:] == rows_np[:, size:]).all()
    assert (ok[n:] == 0xEE).all() and (cor[n:] == 0xEE).all()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("m,poly,t", SHAPES)
def test_bch_small_counts(torch_cuda, m5_shared, m, poly, t, count):
    """The cw < count guard on both sides of a 256-lane block: rows, ok and
    corrected past the count stay as they were."""
    torch = torch_cuda
    o, h = BchOracle(m, poly, t), _handle(m, poly, t)
    allw = _shape_words(m, t, o, m5_shared)
    words = allw[np.random.default_rng(count).permutation(allw.size)[: count + 300]]
    data, parity = o.word_images(words, junk=np.arange(words.size))
    size, pb = data.shape[1], parity.shape[1]
    wok, wcor, wout = o.decode_batch(data[:count], parity[:count])
    rows_np = np.concatenate([data, parity], 1)
    rows = torch.from_numpy(rows_np).cuda()
    okd = torch.full((count + 300,), 0xEE, dtype=torch.uint8, device="cuda")
    cord = torch.full((count + 300,), 0xEE, dtype=torch.uint8, device="cuda")
    h.decode_batch_device(rows.data_ptr(), size + pb, rows.data_ptr() + size, size + pb, size, count, okd.data_ptr(),
                          cord.data_ptr(), stream=_stream(torch))
    torch.cuda.synchronize()
    out, ok, cor = rows.cpu().numpy(), okd.cpu().numpy(), cord.cpu().numpy()
    _same("small count", (m, poly, t), words, (ok[:count], cor[:count], out[:count, :size]), (wok, wcor, wout))
    assert (out[count:] == rows_np[count:]).all() and (out[:, size:] == parity).all()
    assert (ok[count:] == 0xEE).all() and (cor[count:] == 0xEE).all()
    # encode of the same rows' data images
    enc = torch.from_numpy(np.concatenate([data, np.full_like(parity, 0xEE)], 1)).cuda()
    h.encode_batch_device(enc.data_ptr(), size + pb, enc.data_ptr() + size, size + pb, size, count, _stream(torch))
    torch.cuda.synchronize()
    e = enc.cpu().numpy()
    assert (e[:count, size:] == o.encode_batch(data[:count])).all()
    assert (e[count:, size:] == 0xEE).all() and (e[:, :size] == data).all()


@pytest.mark.parametrize("m,poly,t", SHAPES)
def test_bch_odd_layout(torch_cuda, m5_shared, m, poly, t):
    """Data rows image + 3 + 5 bytes apart from a base 3 bytes in, parity in a
    buffer of its own (stride image + 2, base 1 byte in), size = info image + 3
    (the reference reads and writes only the first info bytes and accepts any
    larger size), no corrected array.  Both buffers start out random; after
    decode only the data images of the rows that decoded may differ, after
    encode only the parity images."""
    torch = torch_cuda
    o, h = BchOracle(m, poly, t), _handle(m, poly, t)
    words = _shape_words(m, t, o, m5_shared)
    n = words.size
    data, parity = o.word_images(words, junk=np.arange(n))
    ib, pb = o.data_bytes, o.parity_bytes
    size, ds, ps, d0, p0 = ib + 3, ib + 3 + 5, pb + 2, 3, 1
    rng = np.random.default_rng(m * 100 + t)
    dbuf = rng.integers(0, 256, d0 + n * ds + 7, dtype=np.uint8)
    pbuf = rng.integers(0, 256, p0 + n * ps + 7, dtype=np.uint8)
    dview = dbuf[d0:d0 + n * ds].reshape(n, ds)
    pview = pbuf[p0:p0 + n * ps].reshape(n, ps)
    dview[:, :ib] = data
    pview[:, :pb] = parity
    wok, wcor, wout = o.decode_batch(data, parity)
    assert 0 < wok.sum() < n
    want_d = dbuf.copy()
    want_d[d0:d0 + n * ds].reshape(n, ds)[:, :ib] = wout
    dd, dp = torch.from_numpy(dbuf).cuda(), torch.from_numpy(pbuf).cuda()
    okd = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    h.decode_batch_device(dd.data_ptr() + d0, ds, dp.data_ptr() + p0, ps, size, n, okd.data_ptr(), None,
                          stream=_stream(torch))
    torch.cuda.synchronize()
    ok = okd.cpu().numpy()
    bad = ok[:n] != wok
    assert not bad.any(), ((m, poly, t), _first(bad))
    assert (ok[n:] == 0xEE).all()
    got_d = dd.cpu().numpy()
    if (got_d != want_d).any():
        at = _first(got_d != want_d)
        pytest.fail(f"decode: byte {at} (row {(at - d0) // ds}, column {(at - d0) % ds}) got {got_d[at]}, "
                    f"expected {want_d[at]}")
    assert (dp.cpu().numpy() == pbuf).all(), "decode wrote the parity buffer"
    # encode the same layout: parity images only
    want_p = pbuf.copy()
    want_p[p0:p0 + n * ps].reshape(n, ps)[:, :pb] = o.encode_batch(data)
    dd = torch.from_numpy(dbuf).cuda()
    h.encode_batch_device(dd.data_ptr() + d0, ds, dp.data_ptr() + p0, ps, size, n, _stream(torch))
    torch.cuda.synchronize()
    got_p = dp.cpu().numpy()
    if (got_p != want_p).any():
        at = _first(got_p != want_p)
        pytest.fail(f"encode: parity byte {at} (row {(at - p0) // ps}, column {(at - p0) % ps}) got {got_p[at]}, "
                    f"expected {want_p[at]}")
    assert (dd.cpu().numpy() == dbuf).all(), "encode wrote the data buffer"
