"""Symbol-interleaved frames on the GPU (poporon_*_interleaved*, rs_interleave.hip
around the row kernels), bit-exact against the oracle's row batches on the
de-interleaved codewords (tests/interleave_ref.py): parity, data, ok, corrected
and dirty, failed rows included.

Every call runs on device buffers whose stride padding and 64 guard bytes on
either side hold 0xA5, and the whole buffers are compared afterwards, so a
byte written outside a region shows.  Placements: the CCSDS wire block (parity
aliased behind the data, odd frame sizes giving every alignment) and separate
buffers with strides size*depth + 3 / nr*depth + 1 at base offsets +1 / +3."""
import numpy as np
import pytest

import libpoporon_amd as P
from interleave_ref import expect_check, expect_decode, expect_encode, frames_to_rows, rows_to_frames

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5
DEPTHS = (1, 2, 3, 4, 5, 7, 8, 16, 64)

RS223 = (8, 0x11D, 1, 1, 32)   # fast kernels
RS239 = (8, 0x11D, 1, 1, 16)   # fewer roots
RS15 = (4, 0x13, 1, 1, 8)      # general kernels, m = 4
RS155 = (8, 0x11D, 1, 1, 100)  # 100 roots


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_handles, _oracles, _cases = {}, {}, {}


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


class Layout:
    """where the regions of `count` frames lie in 0xA5-filled buffers"""

    def __init__(self, kind, size, nr, depth, count):
        self.db, self.pb, self.count = size * depth, nr * depth, count
        if kind == "wire":
            self.ds = self.ps = self.db + self.pb
            self.lens = [2 * G + count * self.ds]
            self.dloc, self.ploc = (0, G), (0, G + self.db)
        else:
            self.ds, self.ps = self.db + 3, self.pb + 1
            self.lens = [2 * G + 1 + count * self.ds, 2 * G + 3 + count * self.ps]
            self.dloc, self.ploc = (0, G + 1), (1, G + 3)

    def image(self, dreg=None, preg=None):
        bufs = [np.full(n, FILL, np.uint8) for n in self.lens]
        for reg, (b, off), stride, w in ((dreg, self.dloc, self.ds, self.db), (preg, self.ploc, self.ps, self.pb)):
            if reg is not None:
                for f in range(self.count):
                    bufs[b][off + f * stride: off + f * stride + w] = reg[f]
        return bufs

    def upload(self, torch, bufs):
        dev = [torch.from_numpy(b).cuda() for b in bufs]
        return dev, dev[self.dloc[0]].data_ptr() + self.dloc[1], dev[self.ploc[0]].data_ptr() + self.ploc[1]


def _same(dev, want):
    return all((d.cpu().numpy() == w).all() for d, w in zip(dev, want))


def _case(params, size, depth, count, seed=0):
    """clean and received frames of one case with the oracle's answers (computed once)"""
    key = (params, size, depth, count, seed)
    if key in _cases:
        return _cases[key]
    m, nr = params[0], params[4]
    nn, t = (1 << m) - 1, nr // 2
    o = _oracle(params)
    rng = np.random.default_rng([seed, size, depth, count, nr])
    ncw = count * depth
    rows = rng.integers(0, nn + 1, (ncw, size), dtype=np.uint8)
    dreg = rows_to_frames(rows, depth)
    preg = expect_encode(o, dreg, depth, threads=8 if ncw > 4096 else 0)
    cw = np.concatenate([rows, frames_to_rows(preg, depth)], 1)
    for c in range(ncw):
        f, i = divmod(c, depth)
        ne = (3 + 5 * c) % (t + 3)  # 0 .. t + 2: past the capability too, so some rows fail
        if count >= 2 and f % 4 == 1:
            ne = 0  # a whole frame of clean codewords
        elif count >= 3 and f % 4 == 2:
            ne = max(ne, 1) if i == depth - 1 else 0  # only the frame's last codeword dirty
        ne = min(ne, size + nr)
        pos = rng.permutation(size + nr)[:ne]
        cw[c, pos] ^= rng.integers(1, nn + 1, ne).astype(np.uint8)
    rd, rp = rows_to_frames(cw[:, :size], depth), rows_to_frames(cw[:, size:], depth)
    th = 8 if ncw > 4096 else 0
    res = dict(dreg=dreg, preg=preg, rd=rd, rp=rp, dirty=expect_check(o, rd, rp, depth),
               dec=expect_decode(o, rd, rp, depth, threads=th))
    _cases[key] = res
    return res


def _run(torch, h, params, size, depth, count, kind, stream=0, case=None):
    """encode, check and decode of one case in one placement, everything compared"""
    nr = params[4]
    c = case or _case(params, size, depth, count)
    L = Layout(kind, size, nr, depth, count)
    ncw = count * depth
    sync = torch.cuda.synchronize
    # encode: parity regions appear, nothing else moves
    dev, dp, pp = L.upload(torch, L.image(c["dreg"]))
    sync()
    h.encode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, stream=stream)
    sync()
    assert _same(dev, L.image(c["dreg"], c["preg"])), "encode"
    # check: reads only
    recv = L.image(c["rd"], c["rp"])
    dev, dp, pp = L.upload(torch, recv)
    dirty = torch.full((ncw + 2 * G,), FILL, dtype=torch.uint8, device="cuda")
    sync()
    h.check_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, dirty.data_ptr() + G, stream=stream)
    sync()
    got = dirty.cpu().numpy()
    assert (got[G:G + ncw] == c["dirty"]).all(), "dirty"
    assert (got[:G] == FILL).all() and (got[G + ncw:] == FILL).all()
    assert _same(dev, recv), "check wrote"
    # decode in place
    ook, ocor, od, op = c["dec"]
    okc = torch.full((2, ncw + 2 * G), FILL, dtype=torch.uint8, device="cuda")
    sync()
    h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr() + G,
                                okc[1].data_ptr() + G, stream=stream)
    sync()
    got = okc.cpu().numpy()
    assert (got[0, G:G + ncw] == ook).all(), "ok"
    assert (got[1, G:G + ncw] == ocor).all(), "corrected"
    assert (got[:, :G] == FILL).all() and (got[:, G + ncw:] == FILL).all()
    assert _same(dev, L.image(od, op)), "decode"
    return c


# count * depth lands on 1, 63, 64, 65 and 1023 codewords where the depth divides them
_TARGETS = [(d, n // d) for n in (1, 63, 64, 65, 1023) for d in DEPTHS if n % d == 0]


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("depth,count", _TARGETS + [(64, 3)])
def test_rs255_223_full_size(torch_cuda, depth, count, kind):
    c = _run(torch_cuda, _handle(RS223), RS223, 223, depth, count, kind)
    if count * depth >= 63:
        assert 0 < c["dec"][0].sum() < count * depth  # corrected rows and failed rows both present


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("size", [222, 2, 1])
@pytest.mark.parametrize("depth", DEPTHS)
def test_rs255_223_shortened(torch_cuda, depth, size, kind):
    _run(torch_cuda, _handle(RS223), RS223, size, depth, 3, kind)


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("params,size", [(RS239, 239), (RS15, 7), (RS155, 155)])
def test_other_codes(torch_cuda, params, size, depth, kind):
    """the fewer-roots, general (m = 4) and 100-root kernels behind the same layout kernels"""
    _run(torch_cuda, _handle(params), params, size, depth, 65 // depth + 2, kind)


def test_past_the_split_threshold(torch_cuda):
    """depth 8 x 2049 frames = 16,392 codewords: the chunk takes the split decode"""
    h = _handle(RS223)
    h.timing(True)
    _run(torch_cuda, h, RS223, 223, 8, 2049, "wire")
    bm = h.timing_read(P.KERNEL_BM)[1]
    h.timing(False)
    assert bm >= 1, "the split kernels did not run"


def _erasure_case(params, size, depth, count, all_sorted):
    """counts 0 .. num_roots of erased message symbols mixed with errors (or num_roots sorted
    erasures everywhere), with the oracle's answer"""
    nr = params[4]
    o = _oracle(params)
    rng = np.random.default_rng([nr, depth, count, int(all_sorted)])
    ncw = count * depth
    rows = rng.integers(0, 256, (ncw, size), dtype=np.uint8)
    cw = np.concatenate([rows, o.encode_batch(rows)], 1)
    pos = np.zeros((ncw, nr), np.uint8)
    cnt = np.zeros(ncw, np.uint8)
    for c in range(ncw):
        ne = nr if all_sorted else c % (nr + 1)
        e = rng.permutation(size)[:ne]
        if all_sorted:
            e = np.sort(e)
        pos[c, :ne], cnt[c] = e, ne
        cw[c, e] = rng.integers(0, 256, ne)
        nerr = 0 if all_sorted else (c // (nr + 1)) % ((nr - ne) // 2 + 2)  # up to one past what is left
        p = rng.permutation(size + nr)[:nerr]
        cw[c, p] ^= rng.integers(1, 256, nerr).astype(np.uint8)
    rd, rp = rows_to_frames(cw[:, :size], depth), rows_to_frames(cw[:, size:], depth)
    return rd, rp, pos, cnt, expect_decode(o, rd, rp, depth, pos, cnt)


@pytest.mark.parametrize("params,size,all_sorted", [(RS223, 223, False), (RS239, 239, False), (RS223, 223, True)])
def test_erasures_depth_4(torch_cuda, params, size, all_sorted):
    torch = torch_cuda
    nr, depth, count = params[4], 4, 16 if all_sorted else 50
    h = _handle(params)
    rd, rp, pos, cnt, (ook, ocor, od, op) = _erasure_case(params, size, depth, count, all_sorted)
    assert 0 < ook.sum() and (all_sorted or ook.sum() < ook.size)
    ncw = count * depth
    for kind in ("wire", "split"):
        L = Layout(kind, size, nr, depth, count)
        dev, dp, pp = L.upload(torch, L.image(rd, rp))
        dpos, dcnt = torch.from_numpy(pos).cuda(), torch.from_numpy(cnt).cuda()
        okc = torch.full((2, ncw), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr(), okc[1].data_ptr(),
                                    d_positions=dpos.data_ptr(), positions_stride=nr, d_counts=dcnt.data_ptr())
        torch.cuda.synchronize()
        got = okc.cpu().numpy()
        assert (got[0] == ook).all() and (got[1] == ocor).all(), kind
        assert _same(dev, L.image(od, op)), kind
        assert (dpos.cpu().numpy() == pos).all() and (dcnt.cpu().numpy() == cnt).all()


def test_depth_1_is_the_row_call(torch_cuda):
    """depth 1 equals poporon_*_batch_device on the same buffers byte for byte"""
    torch = torch_cuda
    h = _handle(RS223)
    size, count = 223, 65
    c = _case(RS223, size, 1, count)
    for kind in ("wire", "split"):
        L = Layout(kind, size, 32, 1, count)
        out = []
        for ilv in (False, True):
            dev, dp, pp = L.upload(torch, L.image(c["dreg"]))
            torch.cuda.synchronize()
            if ilv:
                h.encode_interleaved_device(dp, L.ds, pp, L.ps, size, 1, count)
            else:
                h.encode_batch_device(dp, L.ds, pp, L.ps, size, count)
            torch.cuda.synchronize()
            enc = [d.cpu().numpy() for d in dev]
            dev, dp, pp = L.upload(torch, L.image(c["rd"], c["rp"]))
            res = torch.full((3, count), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if ilv:
                h.check_interleaved_device(dp, L.ds, pp, L.ps, size, 1, count, res[2].data_ptr())
                h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, 1, count, res[0].data_ptr(), res[1].data_ptr())
            else:
                h.check_batch_device(dp, L.ds, pp, L.ps, size, count, res[2].data_ptr())
                h.decode_batch_device(dp, L.ds, pp, L.ps, size, count, res[0].data_ptr(), res[1].data_ptr())
            torch.cuda.synchronize()
            out.append(enc + [d.cpu().numpy() for d in dev] + [res.cpu().numpy()])
        assert all((a == b).all() for a, b in zip(*out)), kind


def test_chunking(torch_cuda, monkeypatch):
    """POPORON_AMD_ILV_CHUNK=96: depth 5 x 100 frames runs in chunks of 19 frames, depth 64 x 3
    frames one frame at a time, with the unchunked handle's results"""
    monkeypatch.setenv("POPORON_AMD_ILV_CHUNK", "96")
    hc = P.Poporon(*RS223)
    monkeypatch.delenv("POPORON_AMD_ILV_CHUNK")
    for depth, count, chunks in ((5, 100, 6), (64, 3, 3)):
        hc.timing(True)
        c = _run(torch_cuda, hc, RS223, 223, depth, count, "wire")
        # encode, check and decode: a gather per chunk each; encode and decode: a scatter per chunk
        assert hc.timing_read(P.KERNEL_ILV_GATHER)[1] == 3 * chunks
        assert hc.timing_read(P.KERNEL_ILV_SCATTER)[1] == 2 * chunks
        hc.timing(False)
        h = _handle(RS223)
        h.timing(True)
        _run(torch_cuda, h, RS223, 223, depth, count, "split", case=c)
        assert h.timing_read(P.KERNEL_ILV_GATHER)[1] == 3
        h.timing(False)
    hc.close()


def test_reserve_and_timing(torch_cuda):
    torch = torch_cuda
    h = P.Poporon(*RS223)
    h.reserve_interleaved(4096)
    size, depth, count = 223, 4, 1024
    c = _case(RS223, size, depth, count)
    L = Layout("wire", size, 32, depth, count)
    h.timing(True)
    dev, dp, pp = L.upload(torch, L.image(c["rd"], c["rp"]))
    okc = torch.zeros((2, count * depth), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr(), okc[1].data_ptr())
    torch.cuda.synchronize()
    assert h.timing_read(P.KERNEL_ILV_GATHER)[1] == 1 and h.timing_read(P.KERNEL_ILV_SCATTER)[1] == 1
    assert h.timing_read(P.KERNEL_ILV_GATHER)[0] > 0 and h.timing_read(P.KERNEL_ILV_SCATTER)[0] > 0
    assert (okc[0].cpu().numpy() == c["dec"][0]).all() and _same(dev, L.image(c["dec"][2], c["dec"][3]))
    h.reserve_interleaved(100)  # a second, smaller reserve
    h.timing(True)
    dev, dp, pp = L.upload(torch, L.image(c["dreg"]))
    torch.cuda.synchronize()
    h.encode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count)
    torch.cuda.synchronize()
    assert h.timing_read(P.KERNEL_ILV_SCATTER)[1] == 1 and h.timing_read(P.KERNEL_ENCODE)[1] == 1
    assert _same(dev, L.image(c["dreg"], c["preg"]))
    h.close()


def test_host_forms(torch_cuda):
    """encode_interleaved / decode_interleaved on numpy frames, depth 5 x 300 frames, and x 6503
    frames: the host forms move 8 MiB of slot bytes at a time, 6502 such frames, so the last
    frame is a second chunk of its own"""
    h = _handle(RS223)
    for count in (300, 6503):
        c = _case(RS223, 223, 5, count)
        assert (h.encode_interleaved(c["dreg"], 5) == c["preg"]).all()
        ok, cor, d, p = h.decode_interleaved(c["rd"], c["rp"], 5)
        ook, ocor, od, op = c["dec"]
        assert (ok == ook).all() and (cor == ocor).all() and (d == od).all() and (p == op).all()
    # erasure form through the host path
    rd, rp, pos, cnt, (ook, ocor, od, op) = _erasure_case(RS223, 223, 4, 50, False)
    ok, cor, d, p = h.decode_interleaved(rd, rp, 4, positions=pos, counts=cnt)
    assert (ok == ook).all() and (cor == ocor).all() and (d == od).all() and (p == op).all()


def test_non_null_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    _run(torch, _handle(RS223), RS223, 223, 5, 13, "split", stream=s.cuda_stream)
