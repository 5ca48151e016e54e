"""Wire forms on the GPU (poporon_amd_set_wire_form, the mapped layout kernels of
rs_interleave.hip): every interleaved call with a symbol map, a receive-side XOR sequence or
both, bit-exact against the oracle on the code bytes (tests/wire_ref.py around
tests/interleave_ref.py): parity, both regions, ok, corrected and dirty, failed codewords
included.

As in tests/test_gpu_interleaved.py every call runs on device buffers whose stride padding and
64 guard bytes on either side hold 0xA5, and whole buffers are compared.  Placements: the wire
block, and separate regions with strides size*depth + 3 / nr*depth + 1 at base offsets +1 / +3
(the parity region's sequence phase size*depth is then no multiple of 16 for odd sizes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the chunking test runs this file as a program
    sys.path.insert(0, ROOT)

import libpoporon_amd as P
import interleave_ref as R
import wire_ref as W

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5
DEPTHS = (1, 2, 3, 4, 5, 7, 8, 64)

CCSDS = (8, 0x187, 112, 11, 32)  # fast kernels
RS223 = (8, 0x11D, 1, 1, 32)     # fast kernels, primitive element 1
RS239 = (8, 0x11D, 1, 1, 16)     # fewer roots
RS155 = (8, 0x11D, 1, 1, 100)    # general kernels

FORMS = ("dual", "seq255", "seq7", "seq1", "seq65536", "ccsds", "perm", "perm7")


def _form(name):
    """(to_code, to_wire, xor_seq) of a named form; None: not given"""
    rng = np.random.default_rng(list(name.encode()))
    if name == "none":
        return None, None, None
    if name == "dual":
        return P.ccsds_dual_basis() + (None,)
    if name == "ccsds":
        return P.ccsds_dual_basis() + (P.ccsds_randomizer(),)
    if name.startswith("seq"):
        return None, None, rng.integers(1, 256, int(name[3:]), dtype=np.uint8)
    # a random bijection that is not GF(2)-linear: a linear-only shortcut in the kernels fails here
    to_code = rng.permutation(256).astype(np.uint8)
    to_wire = np.zeros(256, np.uint8)
    to_wire[to_code] = np.arange(256, dtype=np.uint8)
    assert (to_code[1] ^ to_code[2]) != (to_code[3] ^ to_code[0])
    return to_code, to_wire, (rng.integers(1, 256, 7, dtype=np.uint8) if name == "perm7" else None)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_handles, _oracles, _cases, _set = {}, {}, {}, {}


def _handle(params, fname):
    """the shared handle of a code with the named form set"""
    if params not in _handles:
        _handles[params] = P.Poporon(*params)
        assert _handles[params].supported
    h = _handles[params]
    if _set.get(params) != fname:
        h.set_wire_form(*_form(fname))
        _set[params] = fname
    return h


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


def _case(params, size, depth, count, fname, seed=0):
    """clean and received frames of one case in wire form with the oracle's answers (computed once).
    Errors are XORed into the wire bytes: 0 .. t+2 per codeword, a clean frame, a frame whose last
    codeword alone is dirty."""
    key = (params, size, depth, count, fname, seed)
    if key in _cases:
        return _cases[key]
    to_code, to_wire, seq = _form(fname)
    nr = params[4]
    t = nr // 2
    o = _oracle(params)
    rng = np.random.default_rng([seed, size, depth, count, nr])
    ncw = count * depth
    th = 8 if ncw > 4096 else 0
    rows = rng.integers(0, 256, (ncw, size), dtype=np.uint8)
    cmsg = R.rows_to_frames(rows, depth)                        # code bytes
    cpar = R.expect_encode(o, cmsg, depth, threads=th)
    wmsg = cmsg if to_wire is None else to_wire[cmsg]           # what an encode is given: no sequence
    wpar = W.expect_encode(o, wmsg, depth, to_code, to_wire, threads=th)
    assert (wpar == (cpar if to_wire is None else to_wire[cpar])).all()
    sd, sp = W.to_wire_frames(cmsg, cpar, depth, to_wire, seq)  # the block as sent
    cw = np.concatenate([R.frames_to_rows(sd, depth), R.frames_to_rows(sp, depth)], 1)
    for c in range(ncw):
        f, i = divmod(c, depth)
        ne = (3 + 5 * c) % (t + 3)
        if count >= 2 and f % 4 == 1:
            ne = 0
        elif count >= 3 and f % 4 == 2:
            ne = max(ne, 1) if i == depth - 1 else 0
        ne = min(ne, size + nr)
        pos = rng.permutation(size + nr)[:ne]
        cw[c, pos] ^= rng.integers(1, 256, ne).astype(np.uint8)
    rd, rp = R.rows_to_frames(cw[:, :size], depth), R.rows_to_frames(cw[:, size:], depth)
    res = dict(wmsg=wmsg, wpar=wpar, rd=rd, rp=rp, dirty=W.expect_check(o, rd, rp, depth, to_code, seq),
               dec=W.expect_decode(o, rd, rp, depth, to_code, to_wire, seq, threads=th))
    _cases[key] = res
    return res


def _run(torch, h, params, size, depth, count, kind, fname, stream=0, case=None):
    """encode, check and decode of one case in one placement, everything compared"""
    nr = params[4]
    c = case or _case(params, size, depth, count, fname)
    L = Layout(kind, size, nr, depth, count)
    ncw = count * depth
    sync = torch.cuda.synchronize
    # encode: the message in wire symbols, the parity in wire symbols, no sequence anywhere
    dev, dp, pp = L.upload(torch, L.image(c["wmsg"]))
    sync()
    h.encode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, stream=stream)
    sync()
    assert _same(dev, L.image(c["wmsg"], c["wpar"])), "encode"
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
    ook, ocor, od, op = c["dec"][:4]
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


def _frames(depth):
    return 65 // depth + 2


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("fname", FORMS)
@pytest.mark.parametrize("params", [CCSDS, RS223])
def test_every_form_at_every_depth(torch_cuda, params, fname, depth, kind):
    """the CCSDS code, and the default code: with a primitive element other than 1 the reference
    corrects next to nothing (its codewords with errors come back failed and unchanged), so the
    bytes a decode changes are covered by the code with primitive element 1"""
    c = _run(torch_cuda, _handle(params, fname), params, 223, depth, _frames(depth), kind, fname)
    ok, cor = c["dec"][:2]
    assert 0 < ok.sum() < ok.size  # decoded codewords and failed codewords both present
    assert params[3] != 1 or (ok[cor > 0] == 1).any()  # ... and corrected ones
    # a failed codeword comes back derandomized and otherwise as received
    to_code, to_wire, seq = _form(fname)
    rd, rp = W.to_wire_frames(*W.to_code_frames(c["rd"], c["rp"], depth, to_code, seq), depth, to_wire, None)
    bad = np.nonzero(ok == 0)[0]
    for got, was in ((c["dec"][2], rd), (c["dec"][3], rp)):
        assert (R.frames_to_rows(got, depth)[bad] == R.frames_to_rows(was, depth)[bad]).all()


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("fname", ["ccsds", "perm7"])
@pytest.mark.parametrize("size", [222, 2, 1])
@pytest.mark.parametrize("depth", DEPTHS)
def test_shortened(torch_cuda, depth, size, fname, kind):
    _run(torch_cuda, _handle(CCSDS, fname), CCSDS, size, depth, 3, kind, fname)


# count * depth lands on 1, 63, 64 and 65 codewords where the depth divides them
_TARGETS = [(d, n // d) for n in (1, 63, 64, 65) for d in DEPTHS if n % d == 0]


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("depth,count", _TARGETS)
def test_codeword_counts(torch_cuda, depth, count, kind):
    _run(torch_cuda, _handle(CCSDS, "ccsds"), CCSDS, 223, depth, count, kind, "ccsds")


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("fname", ["ccsds", "perm7"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("params,size", [(RS239, 239), (RS155, 155)])
def test_other_codes(torch_cuda, params, size, depth, fname, kind):
    """the fewer-roots and the general kernels behind the mapped layout kernels"""
    _run(torch_cuda, _handle(params, fname), params, size, depth, _frames(depth), kind, fname)


@pytest.mark.parametrize("params", [CCSDS, RS223])
def test_past_the_split_threshold(torch_cuda, params):
    """depth 8 x 2049 frames = 16,392 codewords: the chunk of the default code takes the split
    decode (a code with another primitive element stays on the whole-batch kernel)"""
    h = _handle(params, "ccsds")
    h.timing(True)
    _run(torch_cuda, h, params, 223, 8, 2049, "wire", "ccsds")
    bm, whole = h.timing_read(P.KERNEL_BM)[1], h.timing_read(P.KERNEL_CORRECT)[1]
    h.timing(False)
    assert (bm >= 1 and whole == 0) if params[3] == 1 else (bm == 0 and whole == 1)


def test_encode_is_the_same_with_and_without_a_sequence(torch_cuda):
    torch = torch_cuda
    size, depth, count = 223, 5, 13
    c = _case(CCSDS, size, depth, count, "ccsds")
    out = []
    for fname in ("dual", "ccsds"):
        h = _handle(CCSDS, fname)
        L = Layout("split", size, 32, depth, count)
        dev, dp, pp = L.upload(torch, L.image(c["wmsg"]))
        torch.cuda.synchronize()
        h.encode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count)
        torch.cuda.synchronize()
        assert _same(dev, L.image(c["wmsg"], c["wpar"])), fname
        out.append([d.cpu().numpy() for d in dev])
    assert all((a == b).all() for a, b in zip(*out))


def _erasure_case(params, size, depth, count, all_sorted, fname):
    """counts 0 .. num_roots of erased message symbols mixed with errors (or num_roots sorted
    erasures everywhere) on frames in wire form, with the oracle's answer"""
    to_code, to_wire, seq = _form(fname)
    nr = params[4]
    o = _oracle(params)
    rng = np.random.default_rng([nr, depth, count, int(all_sorted)])
    ncw = count * depth
    rows = rng.integers(0, 256, (ncw, size), dtype=np.uint8)
    sd, sp = W.to_wire_frames(R.rows_to_frames(rows, depth), R.rows_to_frames(o.encode_batch(rows), depth), depth,
                              to_wire, seq)
    cw = np.concatenate([R.frames_to_rows(sd, depth), R.frames_to_rows(sp, depth)], 1)
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
    rd, rp = R.rows_to_frames(cw[:, :size], depth), R.rows_to_frames(cw[:, size:], depth)
    return rd, rp, pos, cnt, W.expect_decode(o, rd, rp, depth, to_code, to_wire, seq, pos, cnt)


@pytest.mark.parametrize("params,size,all_sorted", [(CCSDS, 223, False), (RS239, 239, False), (CCSDS, 223, True),
                                                    (RS223, 223, True)])
def test_erasures_depth_4(torch_cuda, params, size, all_sorted):
    """lists of 0 .. num_roots erasures with errors, and 32 sorted erasures.  With a primitive
    element other than 1 the reference's erasure decode fails nearly every codeword, and so does
    this one, bit for bit: the codes with primitive element 1 are where erasures get corrected"""
    torch = torch_cuda
    nr, depth, count = params[4], 4, 16 if all_sorted else 50
    h = _handle(params, "ccsds")
    rd, rp, pos, cnt, (ook, ocor, od, op, _, _) = _erasure_case(params, size, depth, count, all_sorted, "ccsds")
    assert params[3] != 1 or (0 < ook.sum() and (all_sorted or ook.sum() < ook.size))
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


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("params", [CCSDS, RS223])
def test_report_form(torch_cuda, params, depth):
    """the bytes are the plain mapped decode's; err_pos / err_val are the diff of the code bytes
    before and after the reference's decode; depth 1 goes through the staging rows too"""
    torch = torch_cuda
    size, nr, count, rs = 223, 32, 20, 35  # report stride past num_roots: bytes 32 .. 34 never written
    h = _handle(params, "ccsds")
    c = _case(params, size, depth, count, "ccsds")
    ook, ocor, od, op, (cd, cp), (dd, pp_) = c["dec"]
    before = np.concatenate([R.frames_to_rows(cd, depth), R.frames_to_rows(cp, depth)], 1)
    after = np.concatenate([R.frames_to_rows(dd, depth), R.frames_to_rows(pp_, depth)], 1)
    ncw = count * depth
    num, pos, val = np.zeros(ncw, np.uint8), np.full((ncw, rs), FILL, np.uint8), np.full((ncw, rs), FILL, np.uint8)
    pos[:, :nr] = val[:, :nr] = 0
    for r in range(ncw):
        at = np.nonzero(before[r] != after[r])[0]
        assert at.size <= nr
        num[r], pos[r, :at.size], val[r, :at.size] = at.size, at, (before[r] ^ after[r])[at]
    assert params[3] != 1 or (num > 8).any()
    for kind in ("wire", "split"):
        L = Layout(kind, size, nr, depth, count)
        plain, dp, pp = L.upload(torch, L.image(c["rd"], c["rp"]))
        okc = torch.full((2, ncw), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr(), okc[1].data_ptr())
        dev, dp, pp = L.upload(torch, L.image(c["rd"], c["rp"]))
        okr = torch.full((2, ncw), FILL, dtype=torch.uint8, device="cuda")
        rep = torch.full((ncw,), FILL, dtype=torch.uint8, device="cuda")
        rpv = torch.full((2, ncw, rs), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.timing(True)
        h.decode_interleaved_report_device(dp, L.ds, pp, L.ps, size, depth, count, okr[0].data_ptr(), rep.data_ptr(),
                                           rpv[0].data_ptr(), rpv[1].data_ptr(), rs, d_corrected=okr[1].data_ptr())
        torch.cuda.synchronize()
        launches = [h.timing_read(k)[1] for k in (P.KERNEL_ILV_GATHER, P.KERNEL_ILV_SCATTER, P.KERNEL_SNAPSHOT,
                                                  P.KERNEL_REPORT)]
        h.timing(False)
        assert launches == [1, 1, 1, 1], (kind, launches)
        assert _same(dev, L.image(od, op)) and _same(dev, [d.cpu().numpy() for d in plain]), kind
        assert (okr.cpu().numpy() == okc.cpu().numpy()).all() and (okr[0].cpu().numpy() == ook).all()
        assert (rep.cpu().numpy() == num).all(), kind
        got = rpv.cpu().numpy()
        assert (got[0] == pos).all() and (got[1] == val).all(), kind


def test_host_forms(torch_cuda):
    for params, fname, depth, count in ((CCSDS, "ccsds", 5, 300), (RS223, "perm7", 1, 100), (RS223, "seq65536", 8, 40)):
        h = _handle(params, fname)
        c = _case(params, 223, depth, count, fname)
        assert (h.encode_interleaved(c["wmsg"], depth) == c["wpar"]).all(), fname
        ok, cor, d, p = h.decode_interleaved(c["rd"], c["rp"], depth)
        ook, ocor, od, op = c["dec"][:4]
        assert (ok == ook).all() and (cor == ocor).all() and (d == od).all() and (p == op).all(), fname


def _chunk_child():
    """POPORON_AMD_ILV_CHUNK=96 is in this process's environment: chunks of 19 frames at depth 5,
    one frame at depth 64, 96 rows at depth 1; a sequence of 7 or 255 bytes restarts with every
    frame, whatever chunk it falls in"""
    import torch
    assert os.environ.get("POPORON_AMD_ILV_CHUNK") == "96" and torch.cuda.is_available()
    for params, fname in ((CCSDS, "ccsds"), (RS223, "perm7")):
        for depth, count, chunks in ((5, 100, 6), (64, 3, 3), (1, 200, 3)):
            h = _handle(params, fname)
            h.timing(True)
            _run(torch, h, params, 223, depth, count, "wire" if depth != 5 else "split", fname)
            # encode, check and decode: a gather per chunk each; encode and decode: a scatter per chunk
            assert h.timing_read(P.KERNEL_ILV_GATHER)[1] == 3 * chunks, (fname, depth)
            assert h.timing_read(P.KERNEL_ILV_SCATTER)[1] == 2 * chunks, (fname, depth)
            h.timing(False)
    print("chunked wire forms ok")


def test_chunking_in_a_child_process(torch_cuda):
    env = dict(os.environ, POPORON_AMD_ILV_CHUNK="96")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "chunked wire forms ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_a_callers_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    _run(torch, _handle(CCSDS, "ccsds"), CCSDS, 223, 5, 13, "split", "ccsds", stream=s.cuda_stream)


def _decode_only(torch, h, c, size, depth, count, kind="wire", stream=0):
    """enqueue one decode of the case; returns what to compare after a synchronise"""
    L = Layout(kind, size, 32, depth, count)
    dev, dp, pp = L.upload(torch, L.image(c["rd"], c["rp"]))
    okc = torch.full((2, count * depth), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return L, dev, dp, pp, okc


def _decoded(L, dev, okc, c):
    got = okc.cpu().numpy()
    return (got[0] == c["dec"][0]).all() and (got[1] == c["dec"][1]).all() and \
        _same(dev, L.image(c["dec"][2], c["dec"][3]))


def test_reserve_then_decode(torch_cuda):
    """the tables go up with poporon_amd_reserve_interleaved; the handle does not expose its staging
    capacity, so only the results are checked"""
    torch = torch_cuda
    h = P.Poporon(*CCSDS)
    h.set_wire_form(*_form("ccsds"))
    h.reserve_interleaved(1024)
    size, depth, count = 223, 4, 256
    for fname in ("ccsds", "seq65536"):  # the second form's image is larger than the first's
        h.set_wire_form(*_form(fname))
        c = _case(CCSDS, size, depth, count, fname)
        L, dev, dp, pp, okc = _decode_only(torch, h, c, size, depth, count)
        h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr(), okc[1].data_ptr())
        torch.cuda.synchronize()
        assert _decoded(L, dev, okc, c), fname
    h.close()


@pytest.mark.parametrize("params", [CCSDS, RS223])
def test_form_change_between_two_enqueued_decodes(torch_cuda, params):
    """set_wire_form between two decodes on a side stream, no synchronise in between: the library
    waits itself before it replaces its device tables"""
    torch = torch_cuda
    h = P.Poporon(*params)
    s = torch.cuda.Stream()
    size, depth, count = 223, 5, 400
    ca, cb = _case(params, size, depth, count, "ccsds"), _case(params, size, depth, count, "perm7")
    A = _decode_only(torch, h, ca, size, depth, count)
    B = _decode_only(torch, h, cb, size, depth, count)
    h.set_wire_form(*_form("ccsds"))
    for (L, dev, dp, pp, okc), fname in ((A, None), (B, "perm7")):
        if fname:
            h.set_wire_form(*_form(fname))
        h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr(), okc[1].data_ptr(),
                                    stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert _decoded(A[0], A[1], A[4], ca), "the decode enqueued before the change"
    assert _decoded(B[0], B[1], B[4], cb), "the decode enqueued after the change"
    h.close()


def _ilv_launches(h):
    return [h.timing_read(k)[1] for k in (P.KERNEL_ILV_GATHER, P.KERNEL_ILV_SCATTER)]


def test_depth_1_timing(torch_cuda):
    """with a form a depth-1 call is staged: one gather and one scatter per chunk; without: none"""
    torch = torch_cuda
    h = P.Poporon(*CCSDS)
    size, count = 223, 65
    for fname, want in (("none", [0, 0]), ("ccsds", [1, 1]), ("seq7", [1, 1])):
        h.set_wire_form(*_form(fname))
        c = _case(CCSDS, size, 1, count, fname)
        L, dev, dp, pp, okc = _decode_only(torch, h, c, size, 1, count)
        h.timing(True)
        h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, 1, count, okc[0].data_ptr(), okc[1].data_ptr())
        torch.cuda.synchronize()
        assert _ilv_launches(h) == want, fname
        h.timing(False)
        assert _decoded(L, dev, okc, c), fname
    h.close()


@pytest.mark.parametrize("depth", [1, 4])
def test_set_then_cleared(torch_cuda, depth):
    """a handle whose form was cleared behaves as one that never had a form: results and launches"""
    torch = torch_cuda
    size, count = 223, _frames(depth)
    used, fresh = P.Poporon(*CCSDS), P.Poporon(*CCSDS)
    used.set_wire_form(*_form("ccsds"))
    _run(torch, used, CCSDS, size, depth, count, "wire", "ccsds")
    used.set_wire_form()
    assert used.wire_form() is None
    counts = []
    for h in (used, fresh):
        h.timing(True)
        _run(torch, h, CCSDS, size, depth, count, "split", "none")
        counts.append(_ilv_launches(h))
        h.timing(False)
        h.close()
    assert counts[0] == counts[1] == ([0, 0] if depth == 1 else [3, 2])


@pytest.mark.parametrize("depth", [1, 5])
@pytest.mark.parametrize("params", [CCSDS, RS223])
def test_against_the_plain_call_around_a_host_transform(torch_cuda, params, depth):
    """the mapped decode equals numpy's to_code, the plain decode_interleaved_device and numpy's
    to_wire: bytes, d_ok and d_corrected"""
    torch = torch_cuda
    size, count = 223, _frames(depth)
    to_code, to_wire, seq = _form("ccsds")
    c = _case(params, size, depth, count, "ccsds")
    plain = P.Poporon(*params)
    L, dev, dp, pp, okc = _decode_only(torch, plain, c, size, depth, count)
    h = _handle(params, "ccsds")
    h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okc[0].data_ptr(), okc[1].data_ptr())
    cd, cp = W.to_code_frames(c["rd"], c["rp"], depth, to_code, seq)
    dev2, dp, pp = L.upload(torch, L.image(cd, cp))
    okp = torch.full((2, count * depth), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plain.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, okp[0].data_ptr(), okp[1].data_ptr())
    torch.cuda.synchronize()
    assert (okc.cpu().numpy() == okp.cpu().numpy()).all()
    back = [b.cpu().numpy() for b in dev2]
    lo, hi = G, G + count * L.ds  # the wire block: everything between the guards is region bytes
    back[0][lo:hi] = to_wire[back[0][lo:hi]]
    assert _same(dev, back)
    plain.close()


if __name__ == "__main__":
    _chunk_child()
