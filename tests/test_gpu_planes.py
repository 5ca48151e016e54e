"""Plane-layout stripes on the GPU (poporon_*_planes_*, rs_planes.hip around the row kernels),
bit-exact against tests/planes_ref.py: the oracle's row batches on the transposed stripe, with the
lost columns zero and one erasure list for every codeword.  Planes, ok, corrected, dirty and
reports are compared, failed codewords included.

Every call runs on device buffers pre-filled with 0xA5: the gaps of a plane stride and 64 guard
bytes around every plane, and whole buffers are compared afterwards, so a byte written outside
[0, count) of a plane shows.  Placements: strided from one buffer at base offsets 0 / 1 / 3 with
plane strides count, count + 1 and count + 13 (planes of differing alignment), a table of separate
allocations in shuffled order, each at its own offset 0..15, and a table of 16-byte aligned planes
(the kernels without a byte path).  Counts are sized by the tile the library reports
(poporon_amd_plane_tile)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child-process test runs this file as a program
    sys.path.insert(0, ROOT)

import libpoporon_amd as P
import planes_ref as R
import report_ref

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5

RS223 = (8, 0x11D, 1, 1, 32)    # fast kernels
RS239 = (8, 0x11D, 1, 1, 16)    # fewer roots
RS15 = (4, 0x13, 1, 1, 8)       # general kernels, m = 4
RS155 = (8, 0x11D, 1, 1, 100)   # 100 roots
STORAGE = (8, 0x11D, 1, 1, 4)   # the (14,10) shape
CODES = [(RS223, 223), (RS239, 239), (RS15, 7), (RS155, 155), (STORAGE, 10)]
KINDS = ["strided0", "strided1", "strided2", "table", "aligned"]


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


def _counts(W):
    t = P.plane_tile(W)
    return [1, 15, 16, 17, t - 1, t, t + 1, 2 * t + 5]


class Layout:
    """where the W planes of `count` bytes lie in 0xA5-filled buffers"""

    def __init__(self, kind, size, nr, count):
        W = size + nr
        self.size, self.nr, self.W, self.count, self.strided = size, nr, W, count, None
        rng = np.random.default_rng([W, count, len(kind)])
        if kind.startswith("strided"):
            v = int(kind[-1])
            ds, ps = count + (0, 1, 13)[v], count + (13, 0, 1)[v]
            doff = G + (0, 1, 3)[v]
            poff = doff + size * ds + 5 * v
            self.lens = [poff + nr * ps + G]
            self.loc = [(0, doff + j * ds) for j in range(size)] + [(0, poff + p * ps) for p in range(nr)]
            self.strided = (doff, ds, poff, ps)
        else:
            order = rng.permutation(W)  # plane j is allocation order[j]
            offs = rng.integers(0, 16, W) if kind == "table" else np.zeros(W, np.int64)
            self.lens = [0] * W
            self.loc = [None] * W
            for j in range(W):
                self.lens[order[j]] = G + int(offs[j]) + count + G
                self.loc[j] = (int(order[j]), G + int(offs[j]))

    def image(self, planes=None, rows=None):
        """buffers with planes[j] in place (rows: which planes, default all; the others stay 0xA5)"""
        bufs = [np.full(n, FILL, np.uint8) for n in self.lens]
        if planes is not None:
            for j in (range(self.W) if rows is None else rows):
                b, off = self.loc[j]
                bufs[b][off:off + self.count] = planes[j]
        return bufs

    def upload(self, torch, bufs):
        dev = [torch.from_numpy(b).cuda() for b in bufs]
        return dev, [dev[b].data_ptr() + off for b, off in self.loc]


def _same(dev, want):
    return all((d.cpu().numpy() == w).all() for d, w in zip(dev, want))


def _encode(h, L, ptrs, stream=0):
    if L.strided:
        _, ds, _, ps = L.strided
        h.encode_planes_strided_device(ptrs[0], ds, ptrs[L.size], ps, L.size, L.count, stream=stream)
    else:
        h.encode_planes_device(ptrs, L.size, L.count, stream=stream)


def _check(h, L, ptrs, d_dirty, stream=0):
    if L.strided:
        _, ds, _, ps = L.strided
        h.check_planes_strided_device(ptrs[0], ds, ptrs[L.size], ps, L.size, L.count, d_dirty, stream=stream)
    else:
        h.check_planes_device(ptrs, L.size, L.count, d_dirty, stream=stream)


def _decode(h, L, ptrs, d_ok, lost, d_cor, d_dirty, stream=0):
    if L.strided:
        _, ds, _, ps = L.strided
        h.decode_planes_strided_device(ptrs[0], ds, ptrs[L.size], ps, L.size, L.count, d_ok, lost=lost,
                                       d_corrected=d_cor, d_dirty=d_dirty, stream=stream)
    else:
        h.decode_planes_device(ptrs, L.size, L.count, d_ok, lost=lost, d_corrected=d_cor, d_dirty=d_dirty,
                               stream=stream)


_cases, _decodes = {}, {}


def _case(params, size, count, seed=0):
    """clean and received stripe of one case (computed once): 0 .. t + 2 errors per codeword by a pattern in
    c, over all W planes"""
    key = (params, size, count, seed)
    if key in _cases:
        return _cases[key]
    m, nr = params[0], params[4]
    nn, t, W = (1 << m) - 1, nr // 2, size + nr
    o = _oracle(params)
    th = 8 if count > 4096 else 0
    rng = np.random.default_rng([seed, size, nr, count])
    msg = rng.integers(0, nn + 1, (size, count), dtype=np.uint8)
    clean = np.concatenate([msg, R.expect_encode(o, msg, threads=th)])
    recv = clean.copy()
    ne = (3 + 5 * np.arange(count)) % (t + 3)
    ne[1::4] = 0
    for c in np.nonzero(ne)[0]:
        pos = rng.permutation(W)[:min(ne[c], W)]
        recv[pos, c] ^= rng.integers(1, nn + 1, pos.size).astype(np.uint8)
    _cases[key] = dict(msg=msg, clean=clean, recv=recv, dirty=R.expect_check(o, recv))
    return _cases[key]


def _expect(params, planes, lost, key=None):
    """planes_ref.expect_decode, remembered under key"""
    if key is not None and key in _decodes:
        return _decodes[key]
    res = R.expect_decode(_oracle(params), planes, lost, threads=8 if planes.shape[1] > 4096 else 0)
    if key is not None:
        _decodes[key] = res
    return res


def _flags(torch, n, count):
    return torch.full((n, count + 2 * G), FILL, dtype=torch.uint8, device="cuda")


def _flag_rows(f, count):
    got = f.cpu().numpy()
    assert (got[:, :G] == FILL).all() and (got[:, G + count:] == FILL).all(), "a flag array's guard bytes changed"
    return got[:, G:G + count]


def _run_decode(torch, h, params, L, planes, lost, want, null=(), stream=0, what=""):
    """one decode of `planes` in placement L: flags and whole buffers against want = (ok, cor, planes', dirty);
    lost planes in `null` have a NULL entry and no buffer contents of their own"""
    bufs = L.image(planes)
    dev, ptrs = L.upload(torch, bufs)
    ptrs = [None if j in null else p for j, p in enumerate(ptrs)]
    f = _flags(torch, 3, L.count)
    torch.cuda.synchronize()
    _decode(h, L, ptrs, f[0].data_ptr() + G, list(lost), f[1].data_ptr() + G, f[2].data_ptr() + G, stream=stream)
    torch.cuda.synchronize()
    got = _flag_rows(f, L.count)
    ok, cor, out, dirty = want
    assert (got[0] == ok).all(), ("ok", what, np.nonzero(got[0] != ok)[0][:8])
    assert (got[1] == cor.astype(np.uint8)).all(), ("corrected", what)
    assert (got[2] == dirty).all(), ("dirty", what)
    # every non-NULL plane holds the row call's symbols; a NULL entry's buffer is as it was
    exp = L.image(out, rows=[j for j in range(L.W) if j not in null])
    for j in null:
        b, off = L.loc[j]
        exp[b][off:off + L.count] = planes[j]
    assert _same(dev, exp), ("planes", what)
    return got


# ---- encode, check, scrub: every code, count and placement ----------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("params,size", CODES)
def test_encode_check_scrub(torch_cuda, params, size, kind):
    torch = torch_cuda
    h = _handle(params)
    nr = params[4]
    W = size + nr
    for k, count in enumerate(_counts(W)):
        c = _case(params, size, count)
        L = Layout(kind, size, nr, count)
        # encode: the parity planes appear, nothing else moves; table forms leave some parity entries out
        skip = () if L.strided or k % 2 == 0 else tuple(range(size + k % nr, W, 3))[:nr - 1]
        bufs = L.image(c["clean"], rows=range(size))
        dev, ptrs = L.upload(torch, bufs)
        torch.cuda.synchronize()
        _encode(h, L, [None if j in skip else p for j, p in enumerate(ptrs)])
        torch.cuda.synchronize()
        assert _same(dev, L.image(c["clean"], rows=[j for j in range(W) if j not in skip])), ("encode", count, skip)
        # check of the encoded stripe (parity left out above: of the clean one), and of the received one
        for name, planes, want in (("clean", c["clean"], np.zeros(count, np.uint8)), ("recv", c["recv"], c["dirty"])):
            bufs = L.image(planes)
            dev, ptrs = L.upload(torch, bufs)
            f = _flags(torch, 1, count)
            torch.cuda.synchronize()
            _check(h, L, ptrs, f[0].data_ptr() + G)
            torch.cuda.synchronize()
            assert (_flag_rows(f, count)[0] == want).all(), ("check", name, count)
            assert _same(dev, bufs), "check wrote a plane"
        # scrub: the errors-only decode
        want = _expect(params, c["recv"], (), key=(params, size, count, "scrub"))
        _run_decode(torch, h, params, L, c["recv"], (), want, what=("scrub", count))
    ok = want[0]
    assert 0 < ok.sum() < count and not want[3][ok == 1].any()  # corrected and failed codewords both present


@pytest.mark.parametrize("params,size", CODES)
def test_only_the_last_codeword_is_dirty(torch_cuda, params, size):
    torch = torch_cuda
    h = _handle(params)
    nr = params[4]
    for kind, count in (("table", P.plane_tile(size + nr) + 1), ("strided1", 17)):
        c = _case(params, size, count)
        planes = c["clean"].copy()
        planes[size // 2, count - 1] ^= 1
        L = Layout(kind, size, nr, count)
        dev, ptrs = L.upload(torch, L.image(planes))
        f = _flags(torch, 1, count)
        _check(h, L, ptrs, f[0].data_ptr() + G)
        torch.cuda.synchronize()
        want = np.zeros(count, np.uint8)
        want[-1] = 1
        assert (_flag_rows(f, count)[0] == want).all()
        got = _run_decode(torch, h, params, L, planes, (), _expect(params, planes, ()))
        assert got[0].all() and got[1][-1] == 1 and not got[1][:-1].any() and not got[2].any()


# ---- rebuild ------------------------------------------------------------------------------------

def _lost_sets(size, nr):
    W = size + nr
    sets = [[size // 2], [0], [W - 1], [size + nr // 2], list(range(1, 2 * nr, 2))[:nr] if size >= 2 * nr else
            list(range(min(nr, size))), list(range(size, W)), sorted({0, size - 1, size, W - 1})[:nr]]
    out = []
    for s in sets:
        s = sorted(set(s))[:nr]
        if s not in out:
            out.append(s)
    return out


@pytest.mark.parametrize("params,size", CODES)
def test_rebuild_lost_planes(torch_cuda, params, size):
    """clean survivors: the stripe comes back exactly, whatever the lost planes held (they are never read);
    then the same with NULL entries for the lost planes: nothing is written there and nothing else changes"""
    torch = torch_cuda
    h = _handle(params)
    nr = params[4]
    W = size + nr
    count = P.plane_tile(W) + 1
    c = _case(params, size, count)
    rng = np.random.default_rng([W, 77])
    done = []
    for k, lost in enumerate(_lost_sets(size, nr)):
        L = Layout(KINDS[k % len(KINDS)], size, nr, count)
        zero = c["clean"].copy()
        zero[lost] = 0
        junk = c["clean"].copy()
        junk[lost] = rng.integers(0, 256, (len(lost), count), dtype=np.uint8)
        want = _expect(params, zero, lost)
        assert want[0].all() and (want[2] == c["clean"]).all() and not want[3].any()  # the oracle rebuilds exactly
        a = _run_decode(torch, h, params, L, zero, lost, want, what=("zeros", lost))
        b = _run_decode(torch, h, params, L, junk, lost, want, what=("junk", lost))
        assert (a == b).all() and (a[1] == want[1]).all()
        done.append((lost, junk, want))
    # NULL lost entries, after the same cases have passed with real buffers; table forms only
    for k, (lost, junk, want) in enumerate(done):
        L = Layout(("table", "aligned")[k % 2], size, nr, count)
        null = lost if k % 2 else lost[::2]
        _run_decode(torch, h, params, L, junk, lost, want, null=null, what=("null", lost, null))


@pytest.mark.parametrize("params,size", CODES)
def test_lost_planes_and_errors_in_survivors(torch_cuda, params, size):
    """quirk Q2 and everything around it: whatever the oracle answers, with d_dirty its post-decode flag"""
    torch = torch_cuda
    h = _handle(params)
    nr = params[4]
    W = size + nr
    count = 2 * P.plane_tile(W) + 5
    c = _case(params, size, count)
    wrong_ok = flagged = 0
    for k, lost in enumerate(_lost_sets(size, nr)[:5]):
        L = Layout(KINDS[(k + 2) % len(KINDS)], size, nr, count)
        want = _expect(params, c["recv"], lost)
        _run_decode(torch, h, params, L, c["recv"], lost, want, what=("q2", lost))
        wrong = (want[0] == 1) & (want[2] != c["clean"]).any(0)  # ok = 1 with wrong bytes
        wrong_ok += int(wrong.sum())
        flagged += int(want[3][wrong].sum())
    # the cases hold what d_dirty is for: the oracle says ok, the bytes are wrong, and the flag shows it
    assert wrong_ok > 0 and flagged > 0, (wrong_ok, flagged)


# ---- the report form ------------------------------------------------------------------------

@pytest.mark.parametrize("params,size", [(RS223, 223), (STORAGE, 10), (RS15, 7)])
def test_report_positions_are_plane_indices(torch_cuda, params, size):
    torch = torch_cuda
    h = _handle(params)
    nr = params[4]
    W = size + nr
    count = P.plane_tile(W) + 17
    c = _case(params, size, count)
    for kind, lost in (("table", ()), ("strided2", ()), ("aligned", [1, size + 1]), ("table", [size - 1])):
        L = Layout(kind, size, nr, count)
        planes = c["recv"] if not lost else c["clean"].copy()
        if lost:  # clean survivors but for one bad shard in a quarter of the codewords
            planes[3, ::4] ^= 1
        want = _expect(params, planes, lost)
        before = R.staged_rows(planes, lost)
        num, pos, val = report_ref.expect_report(before, R.planes_to_rows(want[2]), nr)
        dev, ptrs = L.upload(torch, L.image(planes))
        f = _flags(torch, 4, count)
        rep = torch.full((2, count, nr + 2), FILL, dtype=torch.uint8, device="cuda")
        args = (f[0].data_ptr() + G, f[3].data_ptr() + G, rep[0].data_ptr(), rep[1].data_ptr(), nr + 2)
        h.decode_planes_report_device(ptrs, size, count, *args, lost=list(lost), d_corrected=f[1].data_ptr() + G,
                                      d_dirty=f[2].data_ptr() + G)
        torch.cuda.synchronize()
        got = _flag_rows(f, count)
        assert (got[0] == want[0]).all() and (got[1] == want[1].astype(np.uint8)).all() and (got[2] == want[3]).all()
        assert _same(dev, L.image(want[2]))
        r = rep.cpu().numpy()
        assert (got[3] == num).all() and (r[0, :, :nr] == pos).all() and (r[1, :, :nr] == val).all()
        assert (r[:, :, nr:] == FILL).all()
        assert not got[3][want[0] == 0].any()  # a failed codeword's report is empty
        if lost:  # rebuilt non-zero symbols are listed with their value, under their plane's index
            good = np.nonzero((want[0] == 1) & (want[3] == 0) & (num < nr))[0]
            assert good.size
            for cw in good[:64]:
                listed = dict(zip(pos[cw, :num[cw]].tolist(), val[cw, :num[cw]].tolist()))
                for j in lost:
                    if want[2][j, cw]:
                        assert listed[j] == want[2][j, cw]
        else:
            assert num.max() > 0 and pos.max() >= size  # parity planes are reported under size + p


# ---- large batches, chunks, reserve, timing, streams ------------------------------------------

def test_past_the_split_threshold(torch_cuda):
    """16,392 codewords of the default code: the decode behind the gather is routed as a large batch"""
    torch = torch_cuda
    h = _handle(RS223)
    size, nr, count = 223, 32, 16392
    c = _case(RS223, size, count)
    L = Layout("strided0", size, nr, count)  # stride 16,392: planes on alternating 8-byte boundaries
    h.timing(True)
    _run_decode(torch, h, RS223, L, c["recv"], (), _expect(RS223, c["recv"], (), key=(RS223, size, count, "scrub")))
    bm, g, s = (h.timing_read(k)[1] for k in (P.KERNEL_BM, P.KERNEL_PLANE_GATHER, P.KERNEL_PLANE_SCATTER))
    assert bm >= 1, "the split kernels did not run"
    assert (g, s) == (1, 1)
    lost = [7, 100, 230, 254]
    junk = c["recv"].copy()
    junk[lost] = 0x5A
    h.timing(True)
    _run_decode(torch, h, RS223, L, junk, lost, _expect(RS223, c["recv"], lost))
    h.timing(False)


def _chunk_child(chunk):
    """POPORON_AMD_ILV_CHUNK=<chunk> is in this process's environment: 3 chunks and a remainder"""
    import torch
    assert os.environ.get("POPORON_AMD_ILV_CHUNK") == str(chunk) and torch.cuda.is_available()
    count = 3 * chunk + 7
    chunks = 4
    for params, size, lost in ((STORAGE, 10, [2, 11]), (RS223, 223, [0, 100, 254])):
        h = _handle(params)
        nr = params[4]
        c = _case(params, size, count)
        for kind in ("strided1", "aligned"):
            L = Layout(kind, size, nr, count)

            def launches():
                torch.cuda.synchronize()
                n = [h.timing_read(k)[1] for k in (P.KERNEL_PLANE_GATHER, P.KERNEL_PLANE_SCATTER, P.KERNEL_CHECK)]
                h.timing(True)
                return n

            h.timing(True)
            dev, ptrs = L.upload(torch, L.image(c["clean"], rows=range(size)))
            _encode(h, L, ptrs)
            assert launches() == [chunks, chunks, 0]
            assert _same(dev, L.image(c["clean"]))
            f = _flags(torch, 1, count)
            dev, ptrs = L.upload(torch, L.image(c["recv"]))
            _check(h, L, ptrs, f[0].data_ptr() + G)
            assert launches() == [chunks, 0, chunks]
            assert (_flag_rows(f, count)[0] == c["dirty"]).all()
            _run_decode(torch, h, params, L, c["recv"], (), _expect(params, c["recv"], (), key=(params, "s")))
            assert launches()[:2] == [chunks, chunks]
            _run_decode(torch, h, params, L, c["recv"], lost, _expect(params, c["recv"], lost, key=(params, "l")))
            assert launches()[:2] == [chunks, chunks]
            h.timing(False)
    print(f"plane chunks of {chunk} ok")


def test_chunks_in_a_child_process(torch_cuda):
    env = dict(os.environ, POPORON_AMD_ILV_CHUNK="96")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks", "96"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "plane chunks of 96 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_reserve_then_timing_ids(torch_cuda):
    """after poporon_amd_reserve_planes (and _report) the calls allocate nothing: the device's free memory
    does not drop by the 32 MiB of staging rows that 131,072 codewords take (8 MiB of slack for whatever else
    the runtime does; the device is shared, so a fresh handle gets up to three attempts).  Then 22 and 23
    record one launch each per chunk: 22 only for a check, 23 only the parity planes for an encode."""
    torch = torch_cuda
    size, nr, count = 10, 4, 1 << 17
    W = size + nr
    buf = torch.zeros(W * count, dtype=torch.uint8, device="cuda")
    f = torch.full((3, count), FILL, dtype=torch.uint8, device="cuda")
    rep = torch.zeros((3, count, nr), dtype=torch.uint8, device="cuda")
    bp = buf.data_ptr()
    ptrs = [bp + j * count for j in range(W)]
    drops = []
    for _ in range(3):
        h = P.Poporon(*STORAGE)
        h.reserve_planes(count)
        h.reserve_report(count)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        h.check_planes_device(ptrs, size, count, f[0].data_ptr())
        h.decode_planes_report_device(ptrs, size, count, f[0].data_ptr(), rep[0].data_ptr(), rep[1].data_ptr(),
                                      rep[2].data_ptr(), nr, lost=[1, 12], d_corrected=f[1].data_ptr(),
                                      d_dirty=f[2].data_ptr())
        torch.cuda.synchronize()
        drops.append(free0 - torch.cuda.mem_get_info()[0])
        assert f[0].all() and not f[2].any() and not buf.any()  # the all-zero stripe is a codeword
        if drops[-1] < 8 << 20:
            break
        h.close()
    assert drops[-1] < 8 << 20, drops

    def launches():
        torch.cuda.synchronize()
        n = [h.timing_read(k)[1] for k in (P.KERNEL_PLANE_GATHER, P.KERNEL_PLANE_SCATTER)]
        ms = [h.timing_read(k)[0] for k in (P.KERNEL_PLANE_GATHER, P.KERNEL_PLANE_SCATTER)]
        h.timing(True)
        return n, ms

    h.timing(True)
    h.check_batch_device(bp, W, bp + size, W, size, 100, f[0].data_ptr())
    assert launches()[0] == [0, 0]
    h.check_planes_device(ptrs, size, count, f[0].data_ptr())
    n, ms = launches()
    assert n == [1, 0] and ms[0] > 0
    h.encode_planes_strided_device(bp, count, bp + size * count, count, size, count)
    n, ms = launches()
    assert n == [1, 1] and ms[1] > 0
    h.decode_planes_device(ptrs, size, count, f[0].data_ptr(), lost=[0, 13])
    assert launches()[0] == [1, 1]
    h.decode_planes_device(ptrs, size, count, f[0].data_ptr())
    assert launches()[0] == [1, 1]
    h.timing(False)
    assert not buf.any()
    h.close()


def test_a_callers_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    h = _handle(STORAGE)
    size, nr, count = 10, 4, 777
    c = _case(STORAGE, size, count)
    L = Layout("table", size, nr, count)
    dev, ptrs = L.upload(torch, L.image(c["clean"], rows=range(size)))
    torch.cuda.synchronize()
    _encode(h, L, ptrs, stream=s.cuda_stream)
    s.synchronize()
    assert _same(dev, L.image(c["clean"]))
    lost = [3, 12]
    _run_decode(torch, h, STORAGE, L, c["recv"], lost, _expect(STORAGE, c["recv"], lost), stream=s.cuda_stream)


def test_a_wire_form_on_the_handle_is_not_applied(torch_cuda):
    h = P.Poporon(*RS223)
    h.set_wire_form_ccsds(True, True)
    size, nr, count = 223, 32, 90
    c = _case(RS223, size, count)
    L = Layout("table", size, nr, count)
    _run_decode(torch_cuda, h, RS223, L, c["recv"], (), _expect(RS223, c["recv"], ()))
    h.close()


# ---- offsets past 2^32 ---------------------------------------------------------------------

def test_plane_offsets_past_4_gib(torch_cuda):
    """255 planes 2^25 bytes apart in one buffer from torch.empty: plane 128 and up lie past 2^32.  Only
    T + 1 bytes per plane and 64 guard bytes either side are touched"""
    torch = torch_cuda
    size, nr, W, stride = 223, 32, 255, 1 << 25
    count = P.plane_tile(W) + 1
    h = _handle(RS223)
    c = _case(RS223, size, count)
    buf = torch.empty((W - 1) * stride + count + 2 * G + 16, dtype=torch.uint8, device="cuda")
    base = G + 5
    assert (W - 1) * stride + base > 1 << 32
    wide = torch.as_strided(buf, (W, count + 2 * G), (stride, 1), base - G)  # every plane with its guards
    view = wide[:, G:G + count]

    def put(planes):
        wide.fill_(FILL)
        view.copy_(torch.from_numpy(planes).cuda())

    def got():
        torch.cuda.synchronize()
        w = wide.cpu().numpy()
        assert (w[:, :G] == FILL).all() and (w[:, G + count:] == FILL).all(), "guard bytes of a plane changed"
        return w[:, G:G + count]

    bp = buf.data_ptr() + base
    msg_only = c["clean"].copy()
    msg_only[size:] = FILL
    put(msg_only)
    h.encode_planes_strided_device(bp, stride, bp + size * stride, stride, size, count)
    assert (got() == c["clean"]).all()
    dirty = torch.full((count,), FILL, dtype=torch.uint8, device="cuda")
    put(c["recv"])
    h.check_planes_strided_device(bp, stride, bp + size * stride, stride, size, count, dirty.data_ptr())
    assert (got() == c["recv"]).all() and (dirty.cpu().numpy() == c["dirty"]).all()
    lost = [3, 130, 254]
    want = _expect(RS223, c["recv"], lost)
    f = torch.full((3, count), FILL, dtype=torch.uint8, device="cuda")
    h.decode_planes_strided_device(bp, stride, bp + size * stride, stride, size, count, f[0].data_ptr(), lost=lost,
                                   d_corrected=f[1].data_ptr(), d_dirty=f[2].data_ptr())
    assert (got() == want[2]).all()
    fl = f.cpu().numpy()
    assert (fl[0] == want[0]).all() and (fl[1] == want[1].astype(np.uint8)).all() and (fl[2] == want[3]).all()


if __name__ == "__main__":
    _chunk_child(int(sys.argv[2]))
