"""GPU parity of the fused tail of the split decode (rs_fast.hip:
rs_forney_apply_k, Forney magnitudes and the block apply in one kernel)
against the pinned oracle, the golden vectors and the two-kernel tail
(POPORON_AMD_DECODE_TAIL=split: rs_forney_k, then rs_apply_k<16>).

POPORON_AMD_DECODE_PATH=split forces the split kernels at any batch size
(every stage its own kernel, unless POPORON_AMD_DECODE_TAIL=fused asks for
the fused tail, which batches routed by their size take by default), so the
batches stay tiny: 229 codewords are three whole waves, which take the
block path on the wire layout (255-byte rows back to back, 16-byte aligned),
and a tail of 37 that corrects byte by byte.  Bytes, ok and corrected_num are
compared bit-exactly, and so is every byte around the batch: each buffer
carries 4,080 random guard bytes (16 rows) before and after the rows, and
the bytes between strided rows are guards too.
"""
import functools

import numpy as np
import pytest

import libpoporon_amd as P

pytestmark = pytest.mark.gpu

DEFAULT = (8, 0x11D, 1, 1, 32)
GUARD = 16 * 255  # a multiple of 16, so the guard in front keeps the rows aligned
TAILS = ["fused", "split"]
_handles = {}


def _handle(monkeypatch, tail, params=DEFAULT):
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    if (tail, params) not in _handles:
        monkeypatch.setenv("POPORON_AMD_DECODE_PATH", "split")
        monkeypatch.setenv("POPORON_AMD_DECODE_TAIL", tail)
        h = P.Poporon(*params)
        assert h.supported
        _handles[(tail, params)] = h
    return _handles[(tail, params)]


@functools.lru_cache(maxsize=None)
def _oracle(params):
    from oracle import Oracle
    return Oracle(*params)


def _boundary_pairs(lane, first):
    """Positions on both sides of eight of the 16-byte chunk boundaries that
    the row of `lane` straddles inside its wave's block (row bytes 255 lane +
    p): the first eight or the last eight."""
    ps = [p for p in range(1, 255) if (255 * lane + p) % 16 == 0]
    ps = ps[:8] if first else ps[-8:]
    return np.array([q for p in ps for q in (p - 1, p)])


@functools.lru_cache(maxsize=None)
def _case(params, size, nmax, special):
    """229 received words (n, size + nr) and the oracle's (ok, cor, data,
    parity).  Every row gets 0..nmax random errors; with `special` (full
    length, 32 roots) wave 1 is clean, every row of wave 2 has 16 errors on
    both sides of eight chunk boundaries, and the rows at the quarter-block
    edges of wave 0 and some of the tail have errors at bytes 0 and 254."""
    o = _oracle(params)
    nr = params[4]
    L = size + nr
    n = 229
    rng = np.random.default_rng(size * 1000 + nr * 10 + params[2] + nmax)
    data = rng.integers(0, 256, (n, size), dtype=np.uint8)
    cw = np.concatenate([data, o.encode_batch(data)], 1)
    for c in range(n):
        if special and 64 <= c < 128:
            continue
        if special and 128 <= c < 192:
            pos = _boundary_pairs(c - 128, c % 2 == 0)
        elif special and c in (0, 15, 16, 31, 32, 47, 48, 63, 192, 200, 228):
            ne = int(rng.integers(0, 15))
            pos = np.concatenate([[0, 254], 1 + rng.permutation(253)[:ne]])
        else:
            pos = rng.permutation(L)[:int(rng.integers(0, nmax + 1))]
        cw[c, pos] ^= rng.integers(1, 256, len(pos)).astype(np.uint8)
    want = o.decode_batch(cw[:, :size], cw[:, size:])
    for a in (cw,) + tuple(want):
        a.setflags(write=False)
    return cw, want


def _run(h, cw, want, size, layout, tail):
    """Decode cw[:n] on the device in `layout`; compares ok, corrected_num and
    the whole buffers (rows and guards) with what the oracle expects."""
    import torch
    n, L = cw.shape
    nr = L - size
    rng = np.random.default_rng(n + len(layout))
    off = 1 if layout == "off1" else 0
    if layout == "separate":
        dstride, pstride = size, nr
        dbuf = rng.integers(0, 256, 2 * GUARD + n * size, dtype=np.uint8)
        pbuf = rng.integers(0, 256, 2 * GUARD + n * nr, dtype=np.uint8)
        dview = dbuf[GUARD:GUARD + n * size].reshape(n, size)
        pview = pbuf[GUARD:GUARD + n * nr].reshape(n, nr)
        bufs = [dbuf, pbuf]
    else:
        dstride = pstride = L + 1 if layout == "stride256" else L
        dbuf = rng.integers(0, 256, 2 * GUARD + off + n * dstride, dtype=np.uint8)
        rows = dbuf[GUARD + off:GUARD + off + n * dstride].reshape(n, dstride)
        dview, pview = rows[:, :size], rows[:, size:L]
        bufs = [dbuf]
    dview[:], pview[:] = cw[:, :size], cw[:, size:]
    dev = [torch.from_numpy(b).cuda() for b in bufs]
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    cor = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dptr = dev[0].data_ptr() + GUARD + off
    pptr = dev[1].data_ptr() + GUARD if layout == "separate" else dptr + size
    if layout == "wire":
        assert dptr % 16 == 0 and L == 255
    h.timing(True)
    h.decode_batch_device(dptr, dstride, pptr, pstride, size, n, ok.data_ptr(), cor.data_ptr(),
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t = {k: h.timing_read(k)[1] for k in (P.KERNEL_BM, P.KERNEL_FORNEY, P.KERNEL_APPLY)}
    h.timing(False)
    assert t[P.KERNEL_BM] == 1 and t[P.KERNEL_APPLY] == 1, t  # the split route, and one launch of its tail
    assert t[P.KERNEL_FORNEY] == (1 if tail == "split" else 0), t
    gok, gcor = ok.cpu().numpy(), cor.cpu().numpy()
    got = [d.cpu().numpy() for d in dev]
    assert (gok == want[0][:n]).all(), np.nonzero(gok != want[0][:n])[0][:8]
    assert (gcor == want[1][:n]).all(), np.nonzero(gcor != want[1][:n])[0][:8]
    dview[:], pview[:] = want[2][:n], want[3][:n]  # bufs: now the expected images, guards as they were
    for g, b in zip(got, bufs):
        assert (g == b).all(), np.nonzero(g != b)[0][:8]
    return gok, gcor, got


def _both(monkeypatch, params, cw, want, size, layout):
    res = [_run(_handle(monkeypatch, tail, params), cw, want, size, layout, tail) for tail in TAILS]
    (ok0, cor0, b0), (ok1, cor1, b1) = res
    assert (ok0 == ok1).all() and (cor0 == cor1).all()
    assert all((x == y).all() for x, y in zip(b0, b1))


@pytest.mark.parametrize("n", [229, 64, 5])
def test_wire(monkeypatch, n):
    """Three whole waves (mixed; all clean: the block is skipped; 16 errors
    in every row) and a 37-codeword tail; one whole wave; five codewords."""
    cw, want = _case(DEFAULT, 223, 20, True)
    assert want[0][64:128].all() and not want[1][64:128].any()
    assert (want[1][128:192] == 16).all()
    assert (want[0][:64] == 0).any() and (want[0][:64] == 1).any()  # list and fast codewords share a wave
    _both(monkeypatch, DEFAULT, cw[:n], want, 223, "wire")


@pytest.mark.parametrize("layout", ["off1", "stride256", "separate"])
def test_not_wire(monkeypatch, layout):
    """The same rows where the block path does not apply: byte by byte."""
    cw, want = _case(DEFAULT, 223, 20, True)
    _both(monkeypatch, DEFAULT, cw, want, 223, layout)


def test_shortened(monkeypatch):
    """size 100 (pad = 123), rows of 132 bytes back to back."""
    cw, want = _case(DEFAULT, 100, 20, False)
    assert want[1].max() == 16
    _both(monkeypatch, DEFAULT, cw, want, 100, "rows")


def test_nrsplit_wire(monkeypatch):
    """RS(255,239): 16 roots, positions below size + npar, wire layout."""
    params = (8, 0x11D, 1, 1, 16)
    cw, want = _case(params, 239, 10, False)
    assert want[1].max() == 8 and (want[0] == 0).any()
    _both(monkeypatch, params, cw, want, 239, "wire")


def test_fcr0_wire(monkeypatch):
    """fcr = 0: the kernels' general-exponent form (P11 = false)."""
    params = (8, 0x11D, 0, 1, 32)
    cw, want = _case(params, 223, 20, False)
    assert want[1].max() == 16
    _both(monkeypatch, params, cw, want, 223, "wire")


def test_golden_wire(monkeypatch, golden):
    """The golden vectors of full length (constructed miscorrections and
    beyond-capacity failures among them), repeated over 229 rows."""
    sel = np.nonzero(golden["dec_size"] == 223)[0]
    idx = np.resize(sel, 229)
    cw = golden["dec_in"][idx, :255]
    out = golden["dec_out"][idx, :255]
    want = (golden["dec_ok"][idx], golden["dec_cor"][idx], out[:, :223], out[:, 223:])
    _both(monkeypatch, DEFAULT, cw, want, 223, "wire")


def test_default_route_is_fused(monkeypatch):
    """With nothing set, a batch large enough for the split kernels (16,384
    codewords) ends with the fused kernel: one launch under the apply's id,
    none under Forney's; the forced split path keeps every stage its own
    kernel unless the tail is asked for."""
    import torch
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    cw, want = _case(DEFAULT, 223, 20, True)
    n = 16384
    idx = np.resize(np.arange(229), n)
    for path, forney in ((None, 0), ("split", 1)):
        monkeypatch.delenv("POPORON_AMD_DECODE_TAIL", raising=False)
        if path:
            monkeypatch.setenv("POPORON_AMD_DECODE_PATH", path)
        else:
            monkeypatch.delenv("POPORON_AMD_DECODE_PATH", raising=False)
        h = P.Poporon(*DEFAULT)
        d = torch.from_numpy(cw[idx]).cuda()
        ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        cor = torch.zeros(n, dtype=torch.uint8, device="cuda")
        h.timing(True)
        h.decode_batch_device(d.data_ptr(), 255, d.data_ptr() + 223, 255, 223, n, ok.data_ptr(), cor.data_ptr(),
                              stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        t = {k: h.timing_read(k)[1] for k in (P.KERNEL_BM, P.KERNEL_FORNEY, P.KERNEL_APPLY)}
        h.timing(False)
        assert t == {P.KERNEL_BM: 1, P.KERNEL_FORNEY: forney, P.KERNEL_APPLY: 1}, (path, t)
        out = d.cpu().numpy()
        assert (ok.cpu().numpy() == want[0][idx]).all() and (cor.cpu().numpy() == want[1][idx]).all()
        assert (out[:, :223] == want[2][idx]).all() and (out[:, 223:] == want[3][idx]).all()
