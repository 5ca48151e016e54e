"""Decode reports on the GPU (poporon_decode_*_report*, rs_report.hip around the
unchanged decode), against the CPU oracle: the decoded bytes, ok and corrected
are the oracle's and, byte for byte, a plain poporon_decode_batch_device run's;
the report is the diff of the oracle's input and output rows
(tests/report_ref.py), and XORing it into the output restores the input.

Every call runs on device buffers whose stride gaps and 64 guard bytes on
either side hold 0xA5, and the whole buffers are compared afterwards: data,
parity, ok, corrected, err_num, err_pos and err_val.  Placements: wire rows
(parity behind the message, 16-byte aligned: the report kernel's run path),
separate buffers with strides size + 3 / nr + 1 at base offsets +1 / +3 (its
byte path), and separate buffers with 4-byte aligned strides at +4 (its dword
path)."""
import numpy as np
import pytest

import libpoporon_amd as P
import rs_syndrome_rows as R
from interleave_ref import expect_decode, frames_to_rows, rows_to_frames
from report_ref import apply_report, expect_report

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5

RS223 = (8, 0x11D, 1, 1, 32)   # fast kernels
RS239 = (8, 0x11D, 1, 1, 16)   # fewer roots
RS15 = (4, 0x13, 1, 1, 8)      # general kernels, W = 15
RS155 = (8, 0x11D, 1, 1, 100)  # 100 slots, W = 255
K = {RS223: 223, RS239: 239, RS15: 7, RS155: 155}
KINDS = ("wire", "split", "split4")


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
    """where `count` regions of db and pb bytes (rows, or frames) lie in 0xA5-filled buffers"""

    def __init__(self, kind, db, pb, count):
        self.db, self.pb, self.count = db, pb, count
        if kind == "wire":
            self.ds = self.ps = db + pb
            self.lens = [2 * G + count * self.ds]
            self.dloc, self.ploc = (0, G), (0, G + db)
        elif kind == "split":
            self.ds, self.ps = db + 3, pb + 1
            self.lens = [2 * G + 1 + count * self.ds, 2 * G + 3 + count * self.ps]
            self.dloc, self.ploc = (0, G + 1), (1, G + 3)
        else:  # 4-byte aligned bases and strides
            self.ds, self.ps = (db + 3) // 4 * 4 + 4, (pb + 3) // 4 * 4
            self.lens = [2 * G + 4 + count * self.ds, 2 * G + 4 + count * self.ps]
            self.dloc, self.ploc = (0, G + 4), (1, G + 4)

    def image(self, dreg, preg):
        bufs = [np.full(n, FILL, np.uint8) for n in self.lens]
        for reg, (b, off), stride, w in ((dreg, self.dloc, self.ds, self.db), (preg, self.ploc, self.ps, self.pb)):
            for f in range(self.count):
                bufs[b][off + f * stride: off + f * stride + w] = reg[f]
        return bufs

    def upload(self, torch, bufs):
        dev = [torch.from_numpy(b).cuda() for b in bufs]
        return dev, dev[self.dloc[0]].data_ptr() + self.dloc[1], dev[self.ploc[0]].data_ptr() + self.ploc[1]


class Out:
    """ok, corrected, err_num (ncw bytes each) and err_pos, err_val (ncw slots of `rs` bytes, nr used)
    in guarded 0xA5-filled device buffers"""

    def __init__(self, torch, ncw, nr, rs):
        self.ncw, self.nr, self.rs = ncw, nr, rs
        self.flat = torch.full((3, ncw + 2 * G), FILL, dtype=torch.uint8, device="cuda")
        self.lists = torch.full((2, ncw * rs + 2 * G), FILL, dtype=torch.uint8, device="cuda")
        self.ok, self.cor, self.num = (self.flat[i].data_ptr() + G for i in range(3))
        self.pos, self.val = (self.lists[i].data_ptr() + G for i in range(2))

    def report_args(self):
        return self.num, self.pos, self.val, self.rs

    def expected(self, ok, cor, num, pos, val):
        flat = np.full((3, self.ncw + 2 * G), FILL, np.uint8)
        flat[0, G:G + self.ncw], flat[1, G:G + self.ncw], flat[2, G:G + self.ncw] = ok, cor, num
        lists = np.full((2, self.ncw * self.rs + 2 * G), FILL, np.uint8)
        for i, a in enumerate((pos, val)):
            v = lists[i, G:G + self.ncw * self.rs].reshape(self.ncw, self.rs)
            v[:, :self.nr] = a
        return flat, lists

    def got(self):
        flat, lists = self.flat.cpu().numpy(), self.lists.cpu().numpy()
        body = lists[:, G:G + self.ncw * self.rs].reshape(2, self.ncw, self.rs)
        return flat, lists, flat[2, G:G + self.ncw], body[0, :, :self.nr], body[1, :, :self.nr]


def _same(dev, want):
    return all((d.cpu().numpy() == w).all() for d, w in zip(dev, want))


def _answer(params, data, parity, pos=None, cnt=None):
    """the oracle's decode of the rows and the report that follows from it"""
    o = _oracle(params)
    th = 8 if len(data) > 4096 else 0
    if pos is not None:
        ok, cor, od, op = o.decode_batch(data, parity, pos.astype(np.uint32), cnt.astype(np.uint32), threads=th)
    else:
        ok, cor, od, op = o.decode_batch(data, parity, threads=th)
    num, epos, evl = expect_report(np.concatenate([data, parity], 1), np.concatenate([od, op], 1), params[4])
    return dict(data=data, parity=parity, pos=pos, cnt=cnt, ok=ok, cor=cor, od=od, op=op, num=num, epos=epos, evl=evl)


def _random_case(params, size, count, seed=0):
    """0 .. t + 2 random errors per row (as test_gpu_interleaved's _case), so failed rows are present"""
    key = ("random", params, size, count, seed)
    if key not in _cases:
        m, nr = params[0], params[4]
        nn, t = (1 << m) - 1, nr // 2
        o = _oracle(params)
        rng = np.random.default_rng([seed, size, count, nr])
        rows = rng.integers(0, nn + 1, (count, size), dtype=np.uint8)
        cw = np.concatenate([rows, o.encode_batch(rows, threads=8 if count > 4096 else 0)], 1)
        for c in range(count):
            ne = min((3 + 5 * c) % (t + 3), size + nr)
            pos = rng.permutation(size + nr)[:ne]
            cw[c, pos] ^= rng.integers(1, nn + 1, ne).astype(np.uint8)
        _cases[key] = _answer(params, np.ascontiguousarray(cw[:, :size]), np.ascontiguousarray(cw[:, size:]))
    return _cases[key]


def _family_case(params, size):
    """the positions and late_discrepancy families of tests/rs_syndrome_rows.py (8-bit codes)"""
    key = ("family", params, size)
    if key not in _cases:
        sm = R.SyndromeMap(_oracle(params), size)
        parts = [R.positions(sm), R.late_discrepancy(sm, draws=1)]
        _cases[key] = _answer(params, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    return _cases[key]


def _erasure_case(params, size, mode, count=70):
    """mode "full": nr sorted erasures, every erased value wrong; "half": every second one already
    right; "short": c % (nr + 1) erasures in insertion order, stale slots behind them and extra
    errors (quirks Q1 / Q2: judged by the oracle alone)"""
    key = ("erasure", params, size, mode, count)
    if key not in _cases:
        nr = params[4]
        o = _oracle(params)
        rng = np.random.default_rng([nr, size, count, len(mode)])
        rows = rng.integers(0, 256, (count, size), dtype=np.uint8)
        cw = np.concatenate([rows, o.encode_batch(rows)], 1)
        pos = np.zeros((count, nr), np.uint8)
        cnt = np.zeros(count, np.uint8)
        for c in range(count):
            if mode == "short":
                ne = min(c % (nr + 1), size)
                e = rng.permutation(size)[:ne]
                pos[c] = rng.integers(0, size, nr)  # stale slots
                nerr = (7 * c) % ((nr - ne) // 2 + 3)  # up to two past what is left
                p = rng.permutation(size + nr)[:nerr]
                cw[c, p] ^= rng.integers(1, 256, nerr).astype(np.uint8)
                cw[c, e] ^= rng.integers(1, 256, ne).astype(np.uint8)
            else:
                ne = nr
                e = np.sort(rng.permutation(size)[:ne])
                flip = rng.integers(1, 256, ne).astype(np.uint8)
                if mode == "half":
                    flip[1::2] = 0
                cw[c, e] ^= flip
            pos[c, :ne], cnt[c] = e, ne
        _cases[key] = _answer(params, np.ascontiguousarray(cw[:, :size]), np.ascontiguousarray(cw[:, size:]), pos, cnt)
    return _cases[key]


def _run(torch, h, params, size, c, kind, rs, stream=0, plain=True):
    """one report call on one case in one placement; everything compared"""
    nr = params[4]
    count = len(c["data"])
    L = Layout(kind, size, nr, count)
    recv = L.image(c["data"], c["parity"])
    dev, dp, pp = L.upload(torch, recv)
    out = Out(torch, count, nr, rs)
    kw = {}
    if c["pos"] is not None:
        dpos, dcnt = torch.from_numpy(c["pos"]).cuda(), torch.from_numpy(c["cnt"]).cuda()
        kw = dict(d_positions=dpos.data_ptr(), positions_stride=nr, d_counts=dcnt.data_ptr())
    torch.cuda.synchronize()
    h.decode_batch_report_device(dp, L.ds, pp, L.ps, size, count, out.ok, *out.report_args(), d_corrected=out.cor,
                                 stream=stream, **kw)
    torch.cuda.synchronize()
    flat, lists, num, epos, evl = out.got()
    wflat, wlists = out.expected(c["ok"], c["cor"], c["num"], c["epos"], c["evl"])
    assert (flat[0] == wflat[0]).all(), "ok"
    assert (flat[1] == wflat[1]).all(), "corrected"
    assert (flat[2] == wflat[2]).all(), "err_num"
    assert (lists[0] == wlists[0]).all(), "err_pos"
    assert (lists[1] == wlists[1]).all(), "err_val"
    assert _same(dev, L.image(c["od"], c["op"])), "decoded rows"
    if kw:
        assert (dpos.cpu().numpy() == c["pos"]).all() and (dcnt.cpu().numpy() == c["cnt"]).all()
    # the report XORed into the output gives the input back
    got = np.concatenate([c["od"], c["op"]], 1)
    assert (apply_report(got, num, epos, evl) == np.concatenate([c["data"], c["parity"]], 1)).all(), "restore"
    if plain:  # a plain decode of the same input: the same bytes everywhere
        dev2, dp2, pp2 = L.upload(torch, recv)
        okc = torch.full((2, count + 2 * G), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h.decode_batch_device(dp2, L.ds, pp2, L.ps, size, count, okc[0].data_ptr() + G, okc[1].data_ptr() + G,
                              stream=stream, **kw)
        torch.cuda.synchronize()
        assert all((a.cpu().numpy() == b.cpu().numpy()).all() for a, b in zip(dev, dev2)), "plain decode differs"
        assert (okc.cpu().numpy() == flat[:2]).all(), "plain ok / corrected differ"
    return out


def _tile_counts(size, nr):
    """one workgroup's tile of rs_report_k - 1 / tile / tile + 1"""
    return (127, 128, 129) if size + nr > 128 else (255, 256, 257)


_SIZES = [(p, s) for p in (RS223, RS239, RS15, RS155) for s in (K[p], K[p] - 1, 1)] + [(RS223, 96)]


@pytest.mark.parametrize("count", [1, 63, 64, 65, "tile-1", "tile", "tile+1"])
@pytest.mark.parametrize("params,size", _SIZES)
def test_random_errors(torch_cuda, params, size, count):
    nr = params[4]
    if isinstance(count, str):
        count = _tile_counts(size, nr)[("tile-1", "tile", "tile+1").index(count)]
    c = _random_case(params, size, count)
    h = _handle(params)
    for i, kind in enumerate(KINDS):
        for rs in (nr, nr + 3):
            _run(torch_cuda, h, params, size, c, kind, rs, plain=rs == nr)
    if count >= 63 and size > 1:
        assert 0 < c["ok"].sum() < count          # corrected rows and failed rows
        both = (c["epos"][:, 0] < size) & (c["epos"].max(1) >= size) & (c["num"] > 1)
        assert both.any()                           # entries in both message and parity


@pytest.mark.parametrize("params", [RS223, RS239])
def test_past_the_split_threshold(torch_cuda, params):
    """16,392 wire rows: the chunk takes the split decode"""
    h = _handle(params)
    c = _random_case(params, K[params], 16392)
    h.timing(True)
    _run(torch_cuda, h, params, K[params], c, "wire", params[4])
    bm, snap, rep = (h.timing_read(k)[1] for k in (P.KERNEL_BM, P.KERNEL_SNAPSHOT, P.KERNEL_REPORT))
    h.timing(False)
    assert bm >= 1, "the split kernels did not run"
    assert snap == 1 and rep == 1


# family sizes: where the oracle shows failed rows with corrected_num > 0 that come back unchanged
_FAMILY = [(RS223, 223), (RS223, 100), (RS223, 96), (RS239, 239), (RS239, 50), (RS155, 155)]


@pytest.mark.parametrize("params,size", _FAMILY)
def test_families(torch_cuda, params, size):
    """one error at every byte of the row (positions 0, size - 1, size and W - 1), runs of t, and
    late discrepancies: failures whose corrected_num counts magnitudes that were never applied"""
    nr = params[4]
    c = _family_case(params, size)
    h = _handle(params)
    for kind, rs in (("wire", nr), ("split", nr + 3), ("split4", nr)):
        _run(torch_cuda, h, params, size, c, kind, rs, plain=kind == "wire")
    single = c["num"] == 1
    assert set(c["epos"][single, 0].tolist()) == set(range(size + nr))  # every position is reported once
    assert (c["ok"] == 0).any()


@pytest.mark.parametrize("params", [RS223, RS239, RS155])
def test_vacuity_conditions(params):
    """what keeps the set above from being vacuous, on the oracle's answers: per 8-bit code a failed
    row, a row with an empty report and corrected_num > 0, a row with entries in both message and
    parity, a row with err_num == num_roots"""
    nr = params[4]
    fam = [_family_case(p, s) for p, s in _FAMILY if p == params]
    assert any((c["ok"] == 0).any() for c in fam)
    assert any(((c["num"] == 0) & (c["cor"] > 0)).any() for c in fam)
    assert any(((c["epos"][:, 0] < s) & (c["epos"].max(1) >= s) & (c["num"] > 1)).any()
               for (p, s), c in zip([x for x in _FAMILY if x[0] == params], fam))
    full = _erasure_case(params, K[params], "full")
    assert (full["num"] == nr).all() and (full["cor"] == nr).all() and full["ok"].all()
    half = _erasure_case(params, K[params], "half")
    assert (half["num"] == nr // 2).all() and (half["cor"] == nr // 2).all() and half["ok"].all()


@pytest.mark.parametrize("params,mode", [(p, m) for p in (RS223, RS239, RS155) for m in ("full", "half", "short")]
                         + [(RS15, "short")])  # 7 message symbols hold no 8 erasures
def test_erasure_mode(torch_cuda, params, mode):
    c = _erasure_case(params, K[params], mode)
    h = _handle(params)
    for kind in ("wire", "split"):
        _run(torch_cuda, h, params, K[params], c, kind, params[4])
    assert c["ok"].any()
    if mode == "short" and params != RS155:
        assert not c["ok"].all()  # rows past what the list leaves fail


# ---- interleaved frames ------------------------------------------------------------------

def _frame_case(params, size, depth, count):
    key = ("frames", params, size, depth, count)
    if key not in _cases:
        rows = _random_case(params, size, count * depth, seed=depth)
        rd, rp = rows_to_frames(rows["data"], depth), rows_to_frames(rows["parity"], depth)
        ok, cor, od, op = expect_decode(_oracle(params), rd, rp, depth)
        num, epos, evl = expect_report(np.concatenate([rows["data"], rows["parity"]], 1),
                                       np.concatenate([frames_to_rows(od, depth), frames_to_rows(op, depth)], 1),
                                       params[4])
        _cases[key] = dict(rd=rd, rp=rp, ok=ok, cor=cor, od=od, op=op, num=num, epos=epos, evl=evl)
    return _cases[key]


def _run_frames(torch, h, params, size, depth, count, kind, rs, report=True):
    nr = params[4]
    c = _frame_case(params, size, depth, count)
    L = Layout(kind, size * depth, nr * depth, count)
    dev, dp, pp = L.upload(torch, L.image(c["rd"], c["rp"]))
    out = Out(torch, count * depth, nr, rs)
    torch.cuda.synchronize()
    if report:
        h.decode_interleaved_report_device(dp, L.ds, pp, L.ps, size, depth, count, out.ok, *out.report_args(),
                                           d_corrected=out.cor)
    else:
        h.decode_interleaved_device(dp, L.ds, pp, L.ps, size, depth, count, out.ok, out.cor)
    torch.cuda.synchronize()
    flat, lists = out.got()[:2]
    if report:
        wflat, wlists = out.expected(c["ok"], c["cor"], c["num"], c["epos"], c["evl"])
        assert (flat == wflat).all() and (lists == wlists).all(), "ok / corrected / report"
    else:
        assert (flat[2] == FILL).all() and (lists == FILL).all()
    assert _same(dev, L.image(c["od"], c["op"])), "decoded frames"
    return [d.cpu().numpy() for d in dev], flat[:2]


@pytest.mark.parametrize("kind", ["wire", "split"])
@pytest.mark.parametrize("depth", [2, 5, 8, 64])
@pytest.mark.parametrize("params,size", [(RS223, 223), (RS223, 96), (RS239, 239), (RS15, 7), (RS155, 155)])
def test_interleaved_report(torch_cuda, params, size, depth, kind):
    h = _handle(params)
    count = 130 // depth + 2
    with_report = _run_frames(torch_cuda, h, params, size, depth, count, kind, params[4] + (3 if kind == "split" else 0))
    # the call without a report does exactly what it did: the same frames, ok and corrected
    without = _run_frames(torch_cuda, h, params, size, depth, count, kind, params[4], report=False)
    assert all((a == b).all() for a, b in zip(with_report[0], without[0])) and (with_report[1] == without[1]).all()


def test_depth_1_is_the_row_report(torch_cuda):
    torch = torch_cuda
    h = _handle(RS223)
    size, count, nr = 223, 65, 32
    c = _random_case(RS223, size, count)
    for kind in ("wire", "split"):
        L = Layout(kind, size, nr, count)
        res = []
        for ilv in (False, True):
            dev, dp, pp = L.upload(torch, L.image(c["data"], c["parity"]))
            out = Out(torch, count, nr, nr + 3)
            torch.cuda.synchronize()
            if ilv:
                h.decode_interleaved_report_device(dp, L.ds, pp, L.ps, size, 1, count, out.ok, *out.report_args(),
                                                   d_corrected=out.cor)
            else:
                h.decode_batch_report_device(dp, L.ds, pp, L.ps, size, count, out.ok, *out.report_args(),
                                             d_corrected=out.cor)
            torch.cuda.synchronize()
            res.append([d.cpu().numpy() for d in dev] + list(out.got()[:2]))
        assert all((a == b).all() for a, b in zip(*res)), kind
        assert (res[0][-2][2, G:G + count] == c["num"]).all()


# ---- chunks, streams, reserve, timing, the host form ---------------------------------------

def test_chunking(torch_cuda, monkeypatch):
    """POPORON_AMD_REPORT_CHUNK=96: 250 codewords run as chunks of 96, 96 and 58"""
    monkeypatch.setenv("POPORON_AMD_REPORT_CHUNK", "96")
    hc = P.Poporon(*RS223)
    monkeypatch.delenv("POPORON_AMD_REPORT_CHUNK")
    c = _random_case(RS223, 223, 250)
    for kind in ("wire", "split"):
        hc.timing(True)
        _run(torch_cuda, hc, RS223, 223, c, kind, 35, plain=False)
        assert hc.timing_read(P.KERNEL_SNAPSHOT)[1] == 3 and hc.timing_read(P.KERNEL_REPORT)[1] == 3
        hc.timing(False)
    hc.close()


def test_timing_ids(torch_cuda):
    """17 (snapshot: a device copy for wire rows, rs_snapshot_k otherwise) and 18 (rs_report_k) record one
    launch per call, with time"""
    h = _handle(RS223)
    c = _random_case(RS223, 223, 129)
    for kind in KINDS:
        h.timing(True)
        _run(torch_cuda, h, RS223, 223, c, kind, 32, plain=False)
        for k in (P.KERNEL_SNAPSHOT, P.KERNEL_REPORT):
            ms, n = h.timing_read(k)
            assert n == 1 and ms > 0, (kind, k)
        assert h.timing_read(P.KERNEL_MASK_LISTS)[1] == 0
        h.timing(False)


def test_non_null_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    _run(torch, _handle(RS223), RS223, 223, _random_case(RS223, 223, 129), "split", 35, stream=s.cuda_stream)


def test_two_streams_without_synchronisation(torch_cuda):
    """four report calls of one handle, alternating between two streams, nothing between them: the
    snapshot buffer they share is ordered by the library"""
    torch = torch_cuda
    h = _handle(RS223)
    size, nr, count = 223, 32, 4000
    cases = [_random_case(RS223, size, count, seed=s) for s in (1, 2, 3, 4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    L = Layout("wire", size, nr, count)
    runs = []
    for c in cases:
        dev, dp, pp = L.upload(torch, L.image(c["data"], c["parity"]))
        runs.append((dev, dp, pp, Out(torch, count, nr, nr)))
    torch.cuda.synchronize()
    for i, (dev, dp, pp, out) in enumerate(runs):
        h.decode_batch_report_device(dp, L.ds, pp, L.ps, size, count, out.ok, *out.report_args(),
                                     d_corrected=out.cor, stream=streams[i % 2].cuda_stream)
    torch.cuda.synchronize()
    for c, (dev, dp, pp, out) in zip(cases, runs):
        flat, lists = out.got()[:2]
        wflat, wlists = out.expected(c["ok"], c["cor"], c["num"], c["epos"], c["evl"])
        assert (flat == wflat).all() and (lists == wlists).all()
        assert _same(dev, L.image(c["od"], c["op"]))


def test_reserve_report(torch_cuda):
    h = P.Poporon(*RS223)
    h.reserve_report(4096)
    c = _random_case(RS223, 223, 257)
    _run(torch_cuda, h, RS223, 223, c, "wire", 32)
    h.reserve_report(100)  # a second, smaller reserve
    _run(torch_cuda, h, RS223, 223, c, "split", 35, plain=False)
    h.close()


def test_host_form(torch_cuda):
    """decode_batch_report on numpy rows, error and erasure mode; 25,972 rows are two chunks (the host
    form moves 8 MiB of slot bytes at a time: 25,971 rows of 255 + 4 + 64 bytes), the second of one row"""
    h = _handle(RS223)
    for c in (_random_case(RS223, 223, 257), _erasure_case(RS223, 223, "short"), _random_case(RS223, 223, 25972)):
        d, p, ok, cor, num, epos, evl = h.decode_batch_report(c["data"], c["parity"], c["pos"], c["cnt"])
        for got, want in ((d, "od"), (p, "op"), (ok, "ok"), (cor, "cor"), (num, "num"), (epos, "epos"), (evl, "evl")):
            assert (got == c[want]).all(), want
