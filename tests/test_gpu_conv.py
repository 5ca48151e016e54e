"""Convolutional-interleaver streams on the GPU (poporon_*_conv_*, rs_conv.hip around the row
kernels), bit-exact against the index formula of tests/conv_ref.py and the oracle's row batches
on the de-interleaved rows: stream, rows, parity, ok, corrected, dirty and reports, failed rows
included.

Every call runs on device buffers pre-filled with 0xA5: the holes of a span, the padding of a row
stride and 64 guard bytes on either side of every buffer, and whole buffers are compared
afterwards, so a byte written outside what a call owns shows.  Row placements: wire rows (parity
behind the message, both strides W) and separate buffers with strides size + 3 / nr + 1 at base
offsets +1 / +3.  Stream base offsets 0, 1 and 15 from a 64-byte boundary.  Counts are sized by
the tile the library reports (poporon_amd_conv_tile)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child-process tests run this file as a program
    sys.path.insert(0, ROOT)

import libpoporon_amd as P
import conv_ref as R

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5

DVB = (8, 0x11D, 0, 1, 16)     # RS(204,188): fewer roots
ATSC = (8, 0x11D, 0, 1, 20)    # RS(207,187)
RS223 = (8, 0x11D, 1, 1, 32)   # fast kernels
RS15 = (4, 0x13, 1, 1, 8)      # general kernels, m = 4
RS155 = (8, 0x11D, 1, 1, 100)  # 100 roots
# (params, size): the default code also at a shortened size whose W = 248 is a multiple of 8
CODES = [(DVB, 188), (ATSC, 187), (RS223, 223), (RS223, 216), (RS15, 7), (RS155, 155)]
TILED = [(12, 17), (52, 4), (1, 3), (2, 1), (5, 1), (64, 1), (128, 2)]
DIRECT = [(64, 64), (128, 255)]  # the window does not fit the LDS


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_handles, _oracles = {}, {}


def _handle(params):
    if params not in _handles:
        _handles[params] = P.Poporon(*params)
        assert _handles[params].supported
    return _handles[params]


def _oracle(params):
    from oracle import Oracle
    if params not in _oracles:
        _oracles[params] = Oracle(*params)
    return _oracles[params]


def _phases(I):
    return sorted({0, 1 % I, I - 1})


def _counts(W, I, M):
    """1, 2, I-1, I, and around the tile: T-1, T, T+1, 3T+1 (the direct path: 1..3)"""
    t = P.conv_tile(W, I, M)
    if t == 0:
        return [1, 2, 3]
    return sorted({1, 2, max(I - 1, 1), I, max(t - 1, 1), t, t + 1, 3 * t + 1})


class Rows:
    """where the rows of `count` codewords lie in 0xA5-filled buffers"""

    def __init__(self, kind, size, nr, count):
        self.size, self.nr, self.count = size, nr, count
        if kind == "wire":
            self.ds = self.ps = size + nr
            self.lens = [2 * G + count * self.ds]
            self.dloc, self.ploc = (0, G), (0, G + size)
        else:
            self.ds, self.ps = size + 3, nr + 1
            self.lens = [2 * G + 1 + count * self.ds, 2 * G + 3 + count * self.ps]
            self.dloc, self.ploc = (0, G + 1), (1, G + 3)

    def image(self, data=None, par=None):
        bufs = [np.full(n, FILL, np.uint8) for n in self.lens]
        for reg, (b, off), stride, w in ((data, self.dloc, self.ds, self.size), (par, self.ploc, self.ps, self.nr)):
            if reg is not None:
                v = np.lib.stride_tricks.as_strided(bufs[b][off:], (self.count, w), (stride, 1))
                v[...] = reg
        return bufs

    def upload(self, torch, bufs):
        dev = [torch.from_numpy(b).cuda() for b in bufs]
        return dev, dev[self.dloc[0]].data_ptr() + self.dloc[1], dev[self.ploc[0]].data_ptr() + self.ploc[1]


def _stream_image(stream, off):
    """a span (u8[span], holes and all) between guards, `off` bytes past a 64-byte boundary"""
    buf = np.full(G + off + stream.size + G, FILL, np.uint8)
    buf[G + off: G + off + stream.size] = stream
    return buf


def _same(dev, want):
    return all((d.cpu().numpy() == w).all() for d, w in zip(dev, want))


def _layout_case(torch, h, size, nr, I, M, phase, count, kind, off, rng, with_parity=True, crc=None):
    """interleave and deinterleave of random rows in one placement, whole buffers compared"""
    W = size + nr
    rows = rng.integers(0, 256, (count, W), dtype=np.uint8)
    L = Rows(kind, size, nr, count)
    span = P.conv_span(W, count, I, M)
    assert span == R.span(W, count, I, M)
    # rows -> stream: the batch's bytes appear, holes and guards keep 0xA5, the rows are unchanged
    rimg = L.image(rows[:, :size], rows[:, size:])
    dev, dp, pp = L.upload(torch, rimg)
    st = torch.from_numpy(_stream_image(np.full(span, FILL, np.uint8), off)).cuda()
    torch.cuda.synchronize()
    h.conv_interleave_device(dp, L.ds, pp if with_parity else None, L.ps, size, count, I, M, phase,
                             st.data_ptr() + G + off)
    torch.cuda.synchronize()
    src = rows if with_parity else np.concatenate([rows[:, :size], np.full((count, nr), FILL, np.uint8)], 1)
    want = _stream_image(R.rows_to_stream(src, I, M, phase, FILL), off)
    got = st.cpu().numpy()
    assert (got == want).all(), ("interleave", I, M, phase, count, kind, off, np.nonzero(got != want)[0][:8])
    assert _same(dev, rimg), "interleave wrote rows"
    # stream -> rows, from a stream whose holes hold other codewords' bytes
    full = rng.integers(0, 256, span, dtype=np.uint8)
    simg = _stream_image(full, off)
    st = torch.from_numpy(simg).cuda()
    dev, dp, pp = L.upload(torch, L.image())
    torch.cuda.synchronize()
    h.conv_deinterleave_device(st.data_ptr() + G + off, I, M, phase, dp, L.ds, pp if with_parity else None, L.ps, size,
                               count)
    torch.cuda.synchronize()
    back = R.stream_to_rows(full, W, count, I, M, phase)
    wimg = L.image(back[:, :size], back[:, size:] if with_parity else None)
    out = [d.cpu().numpy() for d in dev]
    assert all((a == b).all() for a, b in zip(out, wimg)), ("deinterleave", I, M, phase, count, kind, off)
    assert (st.cpu().numpy() == simg).all(), "deinterleave wrote the stream"
    if crc is not None:
        for a in [got] + out:
            crc[0] = zlib.crc32(a.tobytes(), crc[0])


def _sweep(torch, params, size, I, M, crc=None, counts=None):
    """every count and phase of one geometry; placement, base offset and the NULL-parity forms rotate"""
    h = _handle(params)
    nr = params[4]
    rng = np.random.default_rng([size, nr, I, M])
    k = 0
    for count in counts or _counts(size + nr, I, M):
        for phase in _phases(I):
            _layout_case(torch, h, size, nr, I, M, phase, count, ("wire", "split")[k % 2], (0, 1, 15)[k % 3], rng,
                         with_parity=k % 5 != 4, crc=crc)
            k += 1


@pytest.mark.parametrize("I,M", TILED)
@pytest.mark.parametrize("params,size", CODES)
def test_layout_calls(torch_cuda, params, size, I, M):
    _sweep(torch_cuda, params, size, I, M)


@pytest.mark.parametrize("I,M", DIRECT)
@pytest.mark.parametrize("params,size", [(DVB, 188), (RS223, 216), (RS15, 7)])
def test_layout_calls_direct_path(torch_cuda, params, size, I, M):
    assert P.conv_tile(size + params[4], I, M) == 0
    _sweep(torch_cuda, params, size, I, M)


@pytest.mark.parametrize("params,size,I,M", [(DVB, 188, 12, 17), (ATSC, 187, 52, 4)])
def test_every_placement(torch_cuda, params, size, I, M):
    """wire and separate rows x stream offsets 0, 1, 15 x with and without parity, W % I == 0 (DVB)
    and != 0 (ATSC), at one tile + 1"""
    h = _handle(params)
    rng = np.random.default_rng(5)
    count = P.conv_tile(size + params[4], I, M) + 1
    for kind in ("wire", "split"):
        for off in (0, 1, 15):
            for wp in (True, False):
                _layout_case(torch_cuda, h, size, params[4], I, M, I - 1, count, kind, off, rng, with_parity=wp)


def _path_cases(torch):
    """the layout sweep over geometries that fit the LDS, as one CRC of every output buffer"""
    crc = [0]
    for params, size in ((DVB, 188), (RS15, 7)):
        for I, M in ((12, 17), (5, 1), (128, 2)):
            t = P.conv_tile(size + params[4], I, M)
            _sweep(torch, params, size, I, M, crc=crc, counts=[1, I, min(t, 70) + 1])
    return crc[0]


def test_both_paths_give_identical_buffers(torch_cuda):
    """POPORON_AMD_CONV_PATH=direct and =tile in child processes against the default path here"""
    want = _path_cases(torch_cuda)
    for path in ("direct", "tile"):
        env = dict(os.environ, POPORON_AMD_CONV_PATH=path)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "paths"], env=env, capture_output=True,
                           text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0 and f"conv paths crc {want}" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_interleave_then_deinterleave_and_adjacent_windows(torch_cuda):
    """n1 codewords, then n2 at base + n1*W with the advanced phase, write the stream one call on
    n1 + n2 writes; de-interleaving it gives the rows back"""
    torch = torch_cuda
    for params, size, I, M, phase in ((DVB, 188, 12, 17, 7), (ATSC, 187, 52, 4, 51), (RS15, 7, 5, 1, 2)):
        h = _handle(params)
        nr = params[4]
        W = size + nr
        t = P.conv_tile(W, I, M)
        n1, n2 = t + 3, 2 * t - 1
        rng = np.random.default_rng([I, M, size])
        rows = torch.from_numpy(rng.integers(0, 256, (n1 + n2, W), dtype=np.uint8)).cuda()
        span = P.conv_span(W, n1 + n2, I, M)
        one = torch.full((span + 2 * G,), FILL, dtype=torch.uint8, device="cuda")
        two = torch.full((span + 2 * G,), FILL, dtype=torch.uint8, device="cuda")
        rp = rows.data_ptr()
        h.conv_interleave_device(rp, W, rp + size, W, size, n1 + n2, I, M, phase, one.data_ptr() + G)
        h.conv_interleave_device(rp, W, rp + size, W, size, n1, I, M, phase, two.data_ptr() + G)
        h.conv_interleave_device(rp + n1 * W, W, rp + n1 * W + size, W, size, n2, I, M, (phase + n1 * W) % I,
                                 two.data_ptr() + G + n1 * W)
        back = torch.full((n1 + n2, W), FILL, dtype=torch.uint8, device="cuda")
        h.conv_deinterleave_device(two.data_ptr() + G, I, M, phase, back.data_ptr(), W, back.data_ptr() + size, W,
                                   size, n1 + n2)
        torch.cuda.synchronize()
        assert torch.equal(one, two)
        assert (one.cpu().numpy()[G:G + span] == R.rows_to_stream(rows.cpu().numpy(), I, M, phase, FILL)).all()
        assert torch.equal(back, rows)


# ---- the codec calls ----------------------------------------------------------------------

_cases = {}


def _case(params, size, I, M, phase, count, seed=0):
    """clean and received stream of one case with the oracle's answers (computed once)"""
    key = (params, size, I, M, phase, count, seed)
    if key in _cases:
        return _cases[key]
    m, nr = params[0], params[4]
    nn, t, W = (1 << m) - 1, nr // 2, size + nr
    o = _oracle(params)
    th = 8 if count > 4096 else 0
    rng = np.random.default_rng([seed, size, I, M, phase, count])
    msg = rng.integers(0, nn + 1, (count, size), dtype=np.uint8)
    par = R.expect_encode(o, msg, threads=th)
    clean = R.rows_to_stream(np.concatenate([msg, par], 1), I, M, phase, FILL)
    # holes carry the neighbours' bytes on a real link
    holes = R.hole_mask(W, count, I, M, phase)
    clean[holes] = rng.integers(0, nn + 1, int(holes.sum()), dtype=np.uint8)
    recv = clean.copy()
    off = R.offsets(W, count, I, M, phase).reshape(count, W)
    ne = (3 + 5 * np.arange(count)) % (t + 3)  # 0 .. t + 2 errors: past the capability too
    ne[1::4] = 0
    for c in np.nonzero(ne)[0][:4096]:
        pos = rng.permutation(W)[:min(ne[c], W)]
        recv[off[c, pos]] ^= rng.integers(1, nn + 1, pos.size).astype(np.uint8)
    burst = None
    if m == 8 and count * W >= 4 * I * 8:
        # a burst of I*8 consecutive stream bytes past the head of the span, over clean codewords
        b0 = (I - 1) * M * I + (count * W // 3)
        b0 = min(b0, clean.size - (I - 1) * M * I - I * 8)
        burst = np.arange(b0, b0 + I * 8)
        recv[burst] = clean[burst] ^ 0x5A
    res = dict(msg=msg, par=par, clean=clean, recv=recv, burst=burst,
               dirty=R.expect_check(o, recv, size, count, I, M, phase),
               dec=R.expect_decode(o, recv, size, count, I, M, phase, threads=th))
    _cases[key] = res
    return res


def _burst_errors_per_codeword(c, W, count, I, M, phase):
    """how many bytes of the burst fall in each codeword, from the model"""
    where = np.full(R.span(W, count, I, M), -1, np.int64)
    where[R.offsets(W, count, I, M, phase)] = np.arange(count * W) // W
    hit = where[c["burst"]]
    return np.bincount(hit[hit >= 0], minlength=count)


def _decode(torch, h, c, size, nr, I, M, phase, count, kind, off, stream=0, **kw):
    """decode_conv of the case's received stream; returns (rows buffers, ok/corrected, layout)"""
    L = Rows(kind, size, nr, count)
    simg = _stream_image(c["recv"], off)
    st = torch.from_numpy(simg).cuda()
    dev, dp, pp = L.upload(torch, L.image())
    okc = torch.full((2, count + 2 * G), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.decode_conv_device(st.data_ptr() + G + off, I, M, phase, dp, L.ds, pp, L.ps, size, count, okc[0].data_ptr() + G,
                         okc[1].data_ptr() + G, stream=stream, **kw)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == simg).all(), "decode wrote the stream"
    got = okc.cpu().numpy()
    assert (got[:, :G] == FILL).all() and (got[:, G + count:] == FILL).all()
    return dev, got[:, G:G + count], L


def _run_codec(torch, params, size, I, M, phase, count, kind="wire", off=0, stream=0):
    """encode_conv, check_conv and decode_conv of one case, everything compared"""
    h = _handle(params)
    nr = params[4]
    W = size + nr
    c = _case(params, size, I, M, phase, count)
    L = Rows(kind, size, nr, count)
    span = P.conv_span(W, count, I, M)
    # encode: the parity rows and the batch's bytes of the stream appear, nothing else moves
    dev, dp, pp = L.upload(torch, L.image(c["msg"]))
    st = torch.from_numpy(_stream_image(np.full(span, FILL, np.uint8), off)).cuda()
    torch.cuda.synchronize()
    h.encode_conv_device(dp, L.ds, pp, L.ps, size, count, I, M, phase, st.data_ptr() + G + off, stream=stream)
    torch.cuda.synchronize()
    assert _same(dev, L.image(c["msg"], c["par"])), "encode: parity rows"
    want = R.rows_to_stream(np.concatenate([c["msg"], c["par"]], 1), I, M, phase, FILL)
    assert (st.cpu().numpy() == _stream_image(want, off)).all(), "encode: stream"
    # check: reads only
    simg = _stream_image(c["recv"], off)
    st = torch.from_numpy(simg).cuda()
    dirty = torch.full((count + 2 * G,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.check_conv_device(st.data_ptr() + G + off, I, M, phase, size, count, dirty.data_ptr() + G, stream=stream)
    torch.cuda.synchronize()
    got = dirty.cpu().numpy()
    assert (got[G:G + count] == c["dirty"]).all(), "dirty"
    assert (got[:G] == FILL).all() and (got[G + count:] == FILL).all()
    assert (st.cpu().numpy() == simg).all(), "check wrote the stream"
    # decode into the caller's rows
    ook, ocor, od, op = c["dec"]
    dev, okc, _ = _decode(torch, h, c, size, nr, I, M, phase, count, kind, off, stream=stream)
    assert (okc[0] == ook).all(), "ok"
    assert (okc[1] == ocor).all(), "corrected"
    assert _same(dev, L.image(od, op)), "decode"
    # a failed codeword comes out as received
    recv = R.stream_to_rows(c["recv"], W, count, I, M, phase)
    bad = ook == 0
    assert (np.concatenate([od, op], 1)[bad] == recv[bad]).all()
    return c


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("params,size,I,M", [(DVB, 188, 12, 17), (ATSC, 187, 52, 4), (RS223, 223, 12, 17),
                                             (RS223, 216, 52, 4), (RS15, 7, 5, 1), (RS155, 155, 64, 1),
                                             (DVB, 188, 128, 2), (ATSC, 187, 64, 64)])
def test_codec_calls(torch_cuda, params, size, I, M, kind):
    W = size + params[4]
    t = P.conv_tile(W, I, M)
    counts = (1, 3) if t == 0 else (1, I, t + 1, 3 * t + 1)
    for k, count in enumerate(counts):
        c = _run_codec(torch_cuda, params, size, I, M, _phases(I)[k % len(_phases(I))], count, kind, (0, 1, 15)[k % 3])
    if t:
        assert 0 < c["dec"][0].sum() < counts[-1]  # corrected rows and failed rows both present


def test_a_burst_is_spread_over_the_codewords(torch_cuda):
    """a burst of I*8 consecutive stream bytes is at most 8 errors per codeword, which DVB's t = 8
    and ATSC's t = 10 correct: the point of the interleaver"""
    for params, size, I, M in ((DVB, 188, 12, 17), (ATSC, 187, 52, 4)):
        W = size + params[4]
        count = 3 * P.conv_tile(W, I, M) + 1
        c = _case(params, size, I, M, 1, count)
        per = _burst_errors_per_codeword(c, W, count, I, M, 1)
        assert c["burst"].size == I * 8 and per.sum() == I * 8 and 0 < per.max() <= 8  # from the model
        hit = per > 0
        _run_codec(torch_cuda, params, size, I, M, 1, count)
        ook = c["dec"][0]
        only_burst = hit & ((3 + 5 * np.arange(count)) % (params[4] // 2 + 3) + per <= params[4] // 2)
        assert only_burst.any() and ook[only_burst].all()


def test_past_the_split_threshold(torch_cuda):
    """16,385 codewords: the decode behind the gather is routed as a large batch (the default code
    takes the split kernels there; DVB's goes wherever the row call sends it)"""
    for params, size in ((RS223, 223), (DVB, 188)):
        h = _handle(params)
        h.timing(True)
        _run_codec(torch_cuda, params, size, 12, 17, 5, 16385)
        bm, g, s = (h.timing_read(k)[1] for k in (P.KERNEL_BM, P.KERNEL_CONV_GATHER, P.KERNEL_CONV_SCATTER))
        h.timing(False)
        assert bm >= 1 or params != RS223, "the split kernels did not run"
        assert (g, s) == (2, 1)  # check and decode gather once each, the encode scatters once


def test_decode_equals_the_row_call_on_deinterleaved_rows(torch_cuda):
    torch = torch_cuda
    for params, size, I, M, phase, count in ((DVB, 188, 12, 17, 3, 200), (RS223, 223, 52, 4, 9, 300)):
        h = _handle(params)
        nr = params[4]
        c = _case(params, size, I, M, phase, count)
        for kind in ("wire", "split"):
            dev, okc, L = _decode(torch, h, c, size, nr, I, M, phase, count, kind, 1)
            st = torch.from_numpy(c["recv"]).cuda()
            dev2, dp, pp = L.upload(torch, L.image())
            ok2 = torch.full((2, count), FILL, dtype=torch.uint8, device="cuda")
            h.conv_deinterleave_device(st.data_ptr(), I, M, phase, dp, L.ds, pp, L.ps, size, count)
            h.decode_batch_device(dp, L.ds, pp, L.ps, size, count, ok2[0].data_ptr(), ok2[1].data_ptr())
            torch.cuda.synchronize()
            assert (ok2.cpu().numpy() == okc).all()
            assert all(torch.equal(a, b) for a, b in zip(dev, dev2))


@pytest.mark.parametrize("params,size,I,M", [(DVB, 188, 12, 17), (RS223, 223, 52, 4)])
def test_erasure_lists_from_a_flag_stream(torch_cuda, params, size, I, M):
    """per-symbol flags travel as a stream of their own: deinterleave with d_parity NULL, then
    poporon_amd_erasures_from_mask_device at depth 1, then decode_conv with those lists"""
    torch = torch_cuda
    h = _handle(params)
    o = _oracle(params)
    nr = params[4]
    W, phase, count = size + nr, 2, 150
    rng = np.random.default_rng([nr, I])
    msg = rng.integers(0, 256, (count, size), dtype=np.uint8)
    cw = np.concatenate([msg, o.encode_batch(msg)], 1)
    flags = np.zeros((count, W), np.uint8)
    for c in range(count):
        ne = c % (nr + 3)  # more than num_roots flagged symbols too
        e = rng.permutation(W)[:ne]
        flags[c, e] = 1 + c % 255
        cw[c, e] = rng.integers(0, 256, ne)
        nerr = (c // (nr + 3)) % 3
        p = rng.permutation(W)[:nerr]
        cw[c, p] ^= rng.integers(1, 256, nerr).astype(np.uint8)
    recv = R.rows_to_stream(cw, I, M, phase, 0x11)
    fstream = R.rows_to_stream(flags, I, M, phase, 0xFF)  # the holes are other codewords' flags
    # the lists the chain must build: the first num_roots flagged message symbols, ascending
    pos, cnt = np.zeros((count, nr), np.uint8), np.zeros(count, np.uint8)
    for c in range(count):
        e = np.nonzero(flags[c, :size])[0][:nr]
        pos[c, :e.size], cnt[c] = e, e.size
    want = R.expect_decode(o, recv, size, count, I, M, phase, pos, cnt)
    assert 0 < want[0].sum() < count
    fs, rs = torch.from_numpy(fstream).cuda(), torch.from_numpy(recv).cuda()
    mask = torch.full((count, size + 5), FILL, dtype=torch.uint8, device="cuda")
    dpos = torch.full((count, nr), FILL, dtype=torch.uint8, device="cuda")
    dcnt = torch.full((count,), FILL, dtype=torch.uint8, device="cuda")
    h.conv_deinterleave_device(fs.data_ptr(), I, M, phase, mask.data_ptr(), size + 5, None, 0, size, count)
    h.erasures_from_mask_device(mask.data_ptr(), size + 5, size, 1, count, dpos.data_ptr(), nr, dcnt.data_ptr())
    rows = torch.full((count, W), FILL, dtype=torch.uint8, device="cuda")
    okc = torch.full((2, count), FILL, dtype=torch.uint8, device="cuda")
    h.decode_conv_device(rs.data_ptr(), I, M, phase, rows.data_ptr(), W, rows.data_ptr() + size, W, size, count,
                         okc[0].data_ptr(), okc[1].data_ptr(), d_positions=dpos.data_ptr(), positions_stride=nr,
                         d_counts=dcnt.data_ptr())
    torch.cuda.synchronize()
    m = mask.cpu().numpy()
    assert (m[:, :size] == flags[:, :size]).all() and (m[:, size:] == FILL).all()
    assert (dpos.cpu().numpy() == pos).all() and (dcnt.cpu().numpy() == cnt).all()
    got = okc.cpu().numpy()
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    assert (rows.cpu().numpy() == np.concatenate([want[2], want[3]], 1)).all()


def test_a_callers_stream(torch_cuda):
    s = torch_cuda.cuda.Stream()
    assert s.cuda_stream != 0
    _run_codec(torch_cuda, DVB, 188, 12, 17, 4, 77, "split", 15, stream=s.cuda_stream)


def test_a_wire_form_on_the_handle_is_not_applied(torch_cuda):
    h = P.Poporon(*RS223)
    h.set_wire_form_ccsds(True, True)
    size, I, M, phase, count = 223, 12, 17, 6, 90
    c = _case(RS223, size, I, M, phase, count)
    dev, okc, L = _decode(torch_cuda, h, c, size, 32, I, M, phase, count, "wire", 0)
    assert (okc[0] == c["dec"][0]).all() and (okc[1] == c["dec"][1]).all()
    assert _same(dev, L.image(c["dec"][2], c["dec"][3]))
    h.close()


@pytest.mark.parametrize("params,size,I,M", [(DVB, 188, 12, 17), (RS223, 223, 52, 4)])
def test_report_equals_the_row_report(torch_cuda, params, size, I, M):
    torch = torch_cuda
    h = _handle(params)
    nr = params[4]
    phase, count = 1, 260
    c = _case(params, size, I, M, phase, count)
    st = torch.from_numpy(c["recv"]).cuda()
    outs = []
    for conv in (True, False):
        L = Rows("split", size, nr, count)
        dev, dp, pp = L.upload(torch, L.image())
        okc = torch.full((3, count), FILL, dtype=torch.uint8, device="cuda")
        rep = torch.full((2, count, nr + 2), FILL, dtype=torch.uint8, device="cuda")
        args = (dp, L.ds, pp, L.ps, size, count, okc[0].data_ptr(), okc[2].data_ptr(), rep[0].data_ptr(),
                rep[1].data_ptr(), nr + 2)
        if conv:
            h.decode_conv_report_device(st.data_ptr(), I, M, phase, *args, d_corrected=okc[1].data_ptr())
        else:
            h.conv_deinterleave_device(st.data_ptr(), I, M, phase, dp, L.ds, pp, L.ps, size, count)
            h.decode_batch_report_device(*args, d_corrected=okc[1].data_ptr())
        torch.cuda.synchronize()
        outs.append([d.cpu().numpy() for d in dev] + [okc.cpu().numpy(), rep.cpu().numpy()])
    assert all((a == b).all() for a, b in zip(*outs))
    okc, rep = outs[0][-2:]
    assert (okc[0] == c["dec"][0]).all() and (okc[1] == c["dec"][1]).all()
    assert _same([torch.from_numpy(b) for b in outs[0][:2]], L.image(c["dec"][2], c["dec"][3]))
    # the report is the diff of the rows: XORed into the returned rows it gives the received rows
    recv = R.stream_to_rows(c["recv"], size + nr, count, I, M, phase)
    back = np.concatenate([c["dec"][2], c["dec"][3]], 1)
    for r in range(count):
        n = okc[2][r]
        back[r, rep[0, r, :n]] ^= rep[1, r, :n]
    assert (back == recv).all() and (rep[:, :, nr:] == FILL).all() and okc[2].sum() > 0


# ---- check_conv: chunks, the staging buffer, timing ---------------------------------------

def _chunk_child(chunk):
    """POPORON_AMD_ILV_CHUNK=<chunk> is in this process's environment: counts that give 1, 2 and 3
    chunks and a remainder, each chunk its own window of the stream"""
    import torch
    assert os.environ.get("POPORON_AMD_ILV_CHUNK") == str(chunk) and torch.cuda.is_available()
    for params, size, I, M, phase in ((DVB, 188, 12, 17, 11), (ATSC, 187, 52, 4, 50)):
        h = _handle(params)
        for count in (chunk - 1, chunk, chunk + 1, 2 * chunk, 3 * chunk, 3 * chunk + 7):
            c = _case(params, size, I, M, phase, count)
            st = torch.from_numpy(c["recv"]).cuda()
            dirty = torch.full((count,), FILL, dtype=torch.uint8, device="cuda")
            h.timing(True)
            h.check_conv_device(st.data_ptr(), I, M, phase, size, count, dirty.data_ptr())
            torch.cuda.synchronize()
            assert (dirty.cpu().numpy() == c["dirty"]).all(), (chunk, count)
            chunks = -(-count // chunk)
            assert h.timing_read(P.KERNEL_CONV_GATHER)[1] == chunks, (chunk, count)
            assert h.timing_read(P.KERNEL_CHECK)[1] == chunks
            assert h.timing_read(P.KERNEL_CONV_SCATTER)[1] == 0
            h.timing(False)
    print(f"conv chunks of {chunk} ok")


@pytest.mark.parametrize("chunk", [64, 100])
def test_check_in_chunks_in_a_child_process(torch_cuda, chunk):
    env = dict(os.environ, POPORON_AMD_ILV_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks", str(chunk)], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and f"conv chunks of {chunk} ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_reserved_staging_does_not_grow(torch_cuda):
    """after poporon_amd_reserve_interleaved a check allocates nothing: the device's free memory
    does not drop by the 48 MiB of staging rows that 196,608 codewords take (8 MiB of slack for
    whatever else the runtime does).  The device is shared, so a fresh handle gets up to three
    attempts: a staging buffer that grows does so on every one of them."""
    torch = torch_cuda
    count, size, I, M = 196608, 188, 12, 17
    st = torch.zeros(P.conv_span(204, count, I, M), dtype=torch.uint8, device="cuda")
    dirty = torch.full((count,), FILL, dtype=torch.uint8, device="cuda")
    drops = []
    for _ in range(3):
        h = P.Poporon(*DVB)
        h.reserve_interleaved(count)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        h.check_conv_device(st.data_ptr(), I, M, 0, size, count, dirty.data_ptr())
        torch.cuda.synchronize()
        drops.append(free0 - torch.cuda.mem_get_info()[0])
        h.close()
        assert not dirty.any()  # the all-zero word is a codeword
        if drops[-1] < 8 << 20:
            break
    assert drops[-1] < 8 << 20, drops


def test_timing_ids(torch_cuda):
    """20 and 21 record one launch per layout pass and none for the row calls"""
    torch = torch_cuda
    h = P.Poporon(*DVB)
    size, nr, I, M, phase, count = 188, 16, 12, 17, 0, 130
    c = _case(DVB, size, I, M, phase, count)
    W = size + nr
    rows = torch.from_numpy(np.concatenate([c["msg"], c["par"]], 1)).cuda()
    st = torch.from_numpy(c["recv"]).cuda()
    okc = torch.zeros((2, count), dtype=torch.uint8, device="cuda")
    rp = rows.data_ptr()

    def launches():
        torch.cuda.synchronize()
        n = [h.timing_read(k)[1] for k in (P.KERNEL_CONV_GATHER, P.KERNEL_CONV_SCATTER)]
        ms = [h.timing_read(k)[0] for k in (P.KERNEL_CONV_GATHER, P.KERNEL_CONV_SCATTER)]
        h.timing(True)
        return n, ms

    h.timing(True)
    h.encode_batch_device(rp, W, rp + size, W, size, count)
    h.check_batch_device(rp, W, rp + size, W, size, count, okc[0].data_ptr())
    h.decode_batch_device(rp, W, rp + size, W, size, count, okc[0].data_ptr(), okc[1].data_ptr())
    assert launches()[0] == [0, 0]
    h.conv_interleave_device(rp, W, rp + size, W, size, count, I, M, phase, st.data_ptr())
    n, ms = launches()
    assert n == [0, 1] and ms[1] > 0
    h.conv_deinterleave_device(st.data_ptr(), I, M, phase, rp, W, rp + size, W, size, count)
    n, ms = launches()
    assert n == [1, 0] and ms[0] > 0
    h.encode_conv_device(rp, W, rp + size, W, size, count, I, M, phase, st.data_ptr())
    assert launches()[0] == [0, 1]
    h.decode_conv_device(st.data_ptr(), I, M, phase, rp, W, rp + size, W, size, count, okc[0].data_ptr())
    assert launches()[0] == [1, 0]
    h.check_conv_device(st.data_ptr(), I, M, phase, size, count, okc[0].data_ptr())
    assert launches()[0] == [1, 0]
    h.timing(False)
    h.close()


# ---- offsets past 2^32 ---------------------------------------------------------------------

def test_stream_offsets_past_4_gib(torch_cuda):
    """DVB rows whose span exceeds 2^32 bytes: the stream is filled on the device, and the first
    and last 1,024 rows and 4,096 random rows of the de-interleave are compared on the device
    through a torch index gather; the same rows of an interleave, and the end of its span"""
    torch = torch_cuda
    size, nr, I, M, phase = 188, 16, 12, 17, 7
    W = size + nr
    count = (1 << 32) // W + 1000
    span = P.conv_span(W, count, I, M)
    assert span > 1 << 32
    try:
        st = torch.empty(span, dtype=torch.uint8, device="cuda")
        rows = torch.full((count, W), FILL, dtype=torch.uint8, device="cuda")
        st2 = torch.full((span,), FILL, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # torch.cuda.OutOfMemoryError is one
        pytest.skip(f"no 13 GB of device memory for a span past 2^32: {e}")
    step = 1 << 26
    for a in range(0, span, step):  # byte i = bits 13.. of i * 2654435761
        i = torch.arange(a, min(a + step, span), dtype=torch.int64, device="cuda")
        st[a:a + i.numel()] = ((i * 2654435761) >> 13).to(torch.uint8)
    del i
    h = _handle(DVB)
    h.conv_deinterleave_device(st.data_ptr(), I, M, phase, rows.data_ptr(), W, rows.data_ptr() + size, W, size, count)
    h.conv_interleave_device(rows.data_ptr(), W, rows.data_ptr() + size, W, size, count, I, M, phase, st2.data_ptr())
    torch.cuda.synchronize()
    rng = np.random.default_rng(11)
    sel = np.unique(np.concatenate([np.arange(1024), np.arange(count - 1024, count),
                                    rng.integers(0, count, 4096)])).astype(np.int64)
    n = torch.from_numpy(sel[:, None] * W + np.arange(W)[None, :]).cuda()
    p = n + ((phase + n) % I) * (M * I)
    assert int(p.max()) > 1 << 32
    assert torch.equal(st[p], rows[torch.from_numpy(sel).cuda()])
    assert torch.equal(st2[p], st[p])
    # the last 4,096 offsets of the span: the batch's bytes, and 0xA5 in the holes
    tail = torch.arange(span - 4096, span, dtype=torch.int64, device="cuda")
    hole = (tail - ((phase + tail) % I) * (M * I)) >= count * W
    assert bool(hole.any()) and bool((~hole).any())
    assert torch.equal(st2[tail], torch.where(hole, torch.full_like(st[tail], FILL), st[tail]))


if __name__ == "__main__":
    import torch as _torch
    if sys.argv[1] == "paths":
        print(f"conv paths crc {_path_cases(_torch)}")
    else:
        _chunk_child(int(sys.argv[2]))
