"""RS x RS product-code blocks on the GPU (poporon_*_product*, rs_product.hip around the row kernels),
bit-exact against the model of tests/product_ref.py: the oracle's row batches along the rows and the
columns, the schedule of include/poporon_amd.h followed literally.

Every call runs on a device buffer pre-filled with 0xA5 -- every pitch gap, every stride gap and a
64-byte guard band either side -- and the whole buffer is compared afterwards, so a byte written outside
a block's n2 x n1 rectangle shows.  Placements: tight (pitch n1, stride n1*n2: the row code runs in
place), pitch n1+3 with stride n2*pitch (in place, with gaps), and a stride that is no multiple of the
pitch (the staged row route); base offsets 0, 1 and 15.  Block counts are 1, 2, 3 and the counts around
one tile as the library reports it (poporon_amd_product_tile)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child-process test runs this file as a program
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import libpoporon_amd as P
import product_ref as R

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5
SEED = 20

# (row params, column params, row_size, col_size)
PAIRS = {
    "dvd": (R.DVD_ROW, R.DVD_COL, 172, 192),
    "gf16": ((4, 0x13, 1, 1, 4), (4, 0x13, 1, 1, 6), 11, 9),            # general kernels, several blocks per tile
    "full": ((8, 0x11D, 1, 1, 32), (8, 0x11D, 1, 1, 16), 223, 239),     # full width and height, fast kernels
    "roots100": ((8, 0x11D, 1, 1, 4), (8, 0x11D, 1, 1, 100), 16, 20),   # columns RS(120,20) over rows RS(20,16)
    "dvd_row1": (R.DVD_ROW, R.DVD_COL, 1, 192),
    "dvd_col1": (R.DVD_ROW, R.DVD_COL, 172, 1),
}
KINDS = ("tight", "pitch3", "ragged")
OFFS = (0, 1, 15)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_products, _models, _memo = {}, {}, {}


def _product(pair):
    if pair not in _products:
        _products[pair] = P.Product(*PAIRS[pair][:2])
    return _products[pair]


def _model(pair):
    if pair not in _models:
        _models[pair] = R.Model(*PAIRS[pair][:2], threads=8)
    return _models[pair]


def _once(key, f):
    """a reference result, computed once and shared"""
    if key not in _memo:
        _memo[key] = f()
    return _memo[key]


def _counts(pair):
    """1, 2, 3 and the counts around one tile of either axis"""
    row, col, k1, k2 = PAIRS[pair]
    n1, n2 = k1 + row[4], k2 + col[4]
    out = {1, 2, 3}
    for w, cw in ((n2, n1), (n1, n2), (n2, k1)):  # column passes, row passes, the encode's column pass
        g = P.product_tile(w, cw)[0]
        out |= {max(1, g - 1), g, g + 1}
    return sorted(out)


class Place:
    """where `count` blocks of n2 x n1 lie in a 0xA5-filled buffer"""

    def __init__(self, kind, off, n1, n2, count):
        self.n1, self.n2, self.count, self.off = n1, n2, count, G + off
        self.pitch = n1 if kind == "tight" else n1 + 3
        self.stride = n2 * self.pitch + (7 if kind == "ragged" else 0)
        self.len = self.off + count * self.stride + G
        self.inplace = kind != "ragged"

    def image(self, blocks, rows=None, cols=None):
        """the buffer with blocks[b, :rows, :cols] in place; everything else stays 0xA5"""
        buf = np.full(self.len, FILL, np.uint8)
        rows, cols = self.n2 if rows is None else rows, self.n1 if cols is None else cols
        for b in range(self.count):
            for i in range(rows):
                at = self.off + b * self.stride + i * self.pitch
                buf[at:at + cols] = blocks[b, i, :cols]
        return buf

    def args(self, dev):
        return dev.data_ptr() + self.off, self.pitch, self.stride


def _case(pair, count):
    """clean blocks of a pair and a corrupted copy: per block a few rows past the row code's t, the rest with
    0 .. t1 errors, so that a row pass and a coupled column pass both have work"""
    def make():
        row, col, k1, k2 = PAIRS[pair]
        m = _model(pair)
        n1, n2 = m.shape(k1, k2)
        rng = np.random.default_rng([SEED, k1, k2, count])
        msg = rng.integers(0, 1 << row[0], (count, k2, k1), dtype=np.uint8)
        clean = m.encode(msg)
        bad = clean.copy()
        t1, r2 = row[4] // 2, col[4]
        for b in range(count):
            heavy = rng.choice(n2, min(n2, (r2 // 2 + 1 + b % (r2 // 2 + 1))), replace=False)
            for i in range(n2):
                ne = min(n1, t1 + 2) if i in heavy else int(rng.integers(0, t1 + 1)) if (i + b) % 3 else 0
                pos = rng.choice(n1, ne, replace=False)
                bad[b, i, pos] ^= rng.integers(1, 1 << row[0], ne, dtype=np.uint8)
        return msg, clean, bad
    return _once(("case", pair, count), make)


def _flags(torch, count, n1, n2):
    return (torch.full((count * n2,), FILL, dtype=torch.uint8, device="cuda"),
            torch.full((count * n1,), FILL, dtype=torch.uint8, device="cuda"),
            torch.full((count,), FILL, dtype=torch.uint8, device="cuda"))


def _decode_and_compare(torch, pair, pl, bad, want, first, passes, couple, stream=0, prod=None):
    """decode `bad` in place pl; compare the whole buffer and the three outputs with want = Model.decode(...)"""
    row, col, k1, k2 = PAIRS[pair]
    p = prod or _product(pair)
    dev = torch.from_numpy(pl.image(bad)).cuda()
    rd, cd, ok = _flags(torch, pl.count, pl.n1, pl.n2)
    p.decode_device(*pl.args(dev), k1, k2, pl.count, first, passes, couple, rd.data_ptr(), cd.data_ptr(),
                    ok.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    exp = pl.image(want[0])
    assert (got == exp).all(), np.nonzero(got != exp)[0][:8]
    assert (rd.cpu().numpy() == want[1].reshape(-1)).all()
    assert (cd.cpu().numpy() == want[2].reshape(-1)).all()
    assert (ok.cpu().numpy() == want[3]).all()


# ---- every pair, placement and count: encode, check, decode ---------------------------------

@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_encode_check_decode(torch_cuda, pair, kind, off):
    torch = torch_cuda
    row, col, k1, k2 = PAIRS[pair]
    p, m = _product(pair), _model(pair)
    n1, n2 = p.shape(k1, k2)
    for count in _counts(pair):
        msg, clean, bad = _case(pair, count)
        pl = Place(kind, off, n1, n2, count)
        # encode: only the message rectangle is read (the parity area holds 0xA5 on the way in)
        dev = torch.from_numpy(pl.image(clean, rows=k2, cols=k1)).cuda()
        p.encode_device(*pl.args(dev), k1, k2, count)
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == pl.image(clean)).all(), (pair, kind, off, count)
        # check: clean, then the corrupted copy
        rd, cd, ok = _flags(torch, count, n1, n2)
        p.check_device(*pl.args(dev), k1, k2, count, rd.data_ptr(), cd.data_ptr(), ok.data_ptr())
        torch.cuda.synchronize()
        assert not rd.any() and not cd.any() and ok.all()
        assert (dev.cpu().numpy() == pl.image(clean)).all()
        dev = torch.from_numpy(pl.image(bad)).cuda()
        p.check_device(*pl.args(dev), k1, k2, count, rd.data_ptr(), cd.data_ptr(), ok.data_ptr())
        torch.cuda.synchronize()
        want = _once(("check", pair, count), lambda: m.check(bad, k1, k2))
        assert (rd.cpu().numpy() == want[0].reshape(-1)).all() and (cd.cpu().numpy() == want[1].reshape(-1)).all()
        assert (ok.cpu().numpy() == want[2]).all() and (dev.cpu().numpy() == pl.image(bad)).all()
        # decode: row, column with lists; and column first
        for first in (0, 1):
            want = _once(("dec", pair, count, first), lambda: m.decode(bad, k1, k2, first, 2, 1))
            _decode_and_compare(torch, pair, pl, bad, want, first, 2, 1)
        # the check call on the decoded block says what the decode said
        rd, cd, ok = _flags(torch, count, n1, n2)
        dev = torch.from_numpy(pl.image(want[0])).cuda()
        p.check_device(*pl.args(dev), k1, k2, count, rd.data_ptr(), cd.data_ptr(), ok.data_ptr())
        torch.cuda.synchronize()
        assert (rd.cpu().numpy() == want[1].reshape(-1)).all() and (cd.cpu().numpy() == want[2].reshape(-1)).all()
        assert (ok.cpu().numpy() == want[3]).all()


# ---- the patterns on DVD ---------------------------------------------------------------------

def _dvd_clean(count):
    return _once(("dvd", count), lambda: R.dvd_blocks(_model("dvd"), count, SEED))


@pytest.mark.parametrize("kind", ("tight", "ragged"))
@pytest.mark.parametrize("name", R.DVD_PATTERNS)
def test_dvd_patterns(torch_cuda, name, kind):
    """rows16 against rows16_nocouple is the pair that fails if the lists are not built or not used: coupled,
    the block comes back whole; uncoupled, the same schedule leaves it dirty with exactly the model's flags"""
    m = _model("dvd")
    clean = _dvd_clean(2)
    bad, first, passes, couple, repaired = _once(("pat", name), lambda: R.dvd_pattern(name, clean, SEED))
    want = _once(("patdec", name), lambda: m.decode(bad, R.DVD_K1, R.DVD_K2, first, passes, couple))
    if repaired is True:  # (tests/test_product_cpu.py: the model gives the original back)
        assert (want[0] == clean).all() and want[3].all()
    elif repaired is False:
        assert not want[3].any()
    pl = Place(kind, 1, 182, 208, 2)
    _decode_and_compare(torch_cuda, "dvd", pl, bad, want, first, passes, couple)
    # d_block_ok is truthful about the returned bytes
    assert (want[3] == m.check(want[0], R.DVD_K1, R.DVD_K2)[2]).all()


@pytest.mark.parametrize("first", (0, 1))
@pytest.mark.parametrize("passes", (1, 2, 3, 4, 16))
def test_schedules(torch_cuda, passes, first):
    m = _model("dvd")
    clean = _dvd_clean(2)
    for name, couple in (("burst", 1), ("rows16", 1), ("burst", 0)):
        bad = _once(("pat", name), lambda: R.dvd_pattern(name, clean, SEED))[0]
        want = _once(("sched", name, couple, first, passes),
                     lambda: m.decode(bad, R.DVD_K1, R.DVD_K2, first, passes, couple))
        _decode_and_compare(torch_cuda, "dvd", Place("tight" if passes & 1 else "ragged", 15, 182, 208, 2), bad, want,
                            first, passes, couple)


def test_any_output_may_be_null(torch_cuda):
    torch = torch_cuda
    p, m = _product("dvd"), _model("dvd")
    clean = _dvd_clean(2)
    bad = _once(("pat", "rows16"), lambda: R.dvd_pattern("rows16", clean, SEED))[0]
    want = _once(("patdec", "rows16"), lambda: m.decode(bad, R.DVD_K1, R.DVD_K2, 0, 2, 1))
    pl = Place("pitch3", 0, 182, 208, 2)
    for keep in range(3):
        dev = torch.from_numpy(pl.image(bad)).cuda()
        out = _flags(torch, 2, 182, 208)
        ptr = [o.data_ptr() if k == keep else None for k, o in enumerate(out)]
        p.decode_device(*pl.args(dev), R.DVD_K1, R.DVD_K2, 2, 0, 2, 1, *ptr)
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == pl.image(want[0])).all()
        for k, o in enumerate(out):
            exp = want[1 + k].reshape(-1) if k == keep else np.full(o.numel(), FILL, np.uint8)
            assert (o.cpu().numpy() == exp).all()


# ---- large and chunked -----------------------------------------------------------------------

def _workload(count):
    """the bench's corruption: 16 overwritten rows plus 2 errors in every other row"""
    def make():
        clean = _dvd_clean(count)
        rng = np.random.default_rng([SEED, count, 7])
        bad = clean.copy()
        for b in range(count):
            rows = rng.choice(208, 16, replace=False)
            bad[b, rows] = rng.integers(0, 256, (16, 182), dtype=np.uint8)
            R._scatter_errors(rng, bad[b], [i for i in range(208) if i not in set(rows)], 2)
        return clean, bad
    return _once(("work", count), make)


def test_79_dvd_blocks_past_the_split_threshold(torch_cuda):
    """16,432 row codewords and 14,378 column codewords, 3 MB: the row pass is routed as a large batch"""
    m = _model("dvd")
    clean, bad = _workload(79)
    want = _once(("work79",), lambda: m.decode(bad, R.DVD_K1, R.DVD_K2, 0, 3, 1))
    # An overwritten row is within 5 symbols of some row codeword with probability about C(182,5) 255^5 / 256^10
    # = 1.4e-3; the row pass then "corrects" it to that codeword, 15 flags and one wrong row are more than 16 roots
    # take, and the block stays dirty.  That is 0.02 per block, under two of 79: most blocks come back whole.
    assert want[3].sum() >= 70 and (want[0][want[3] == 1] == clean[want[3] == 1]).all()
    _decode_and_compare(torch_cuda, "dvd", Place("tight", 0, 182, 208, 79), bad, want, 0, 3, 1)
    _decode_and_compare(torch_cuda, "dvd", Place("ragged", 1, 182, 208, 79), bad, want, 0, 3, 1)


def _chunk_child(chunk):
    """POPORON_AMD_ILV_CHUNK=<chunk> is in this process's environment: three chunks and a remainder"""
    import torch
    assert os.environ.get("POPORON_AMD_ILV_CHUNK") == str(chunk) and torch.cuda.is_available()
    for pair, kind in (("dvd", "tight"), ("dvd", "ragged"), ("gf16", "pitch3")):
        row, col, k1, k2 = PAIRS[pair]
        p, m = _product(pair), _model(pair)
        n1, n2 = p.shape(k1, k2)
        per = chunk // max(n1, n2)
        count = 3 * per + 1
        msg, clean, bad = _case(pair, count)
        pl = Place(kind, 1, n1, n2, count)
        dev = torch.from_numpy(pl.image(clean, rows=k2, cols=k1)).cuda()
        for axis in (0, 1):
            p.handle(axis).timing(True)
        p.encode_device(*pl.args(dev), k1, k2, count)
        torch.cuda.synchronize()
        assert (dev.cpu().numpy() == pl.image(clean)).all()
        n = [[p.handle(a).timing_read(k)[1] for k in (P.KERNEL_PROD_GATHER, P.KERNEL_PROD_SCATTER)] for a in (0, 1)]
        assert n == [[0, 0] if pl.inplace else [4, 4], [4, 4]], n  # one launch per chunk and staged pass
        for axis in (0, 1):
            p.handle(axis).timing(False)
        for first in (0, 1):
            _decode_and_compare(torch, pair, pl, bad, m.decode(bad, k1, k2, first, 3, 1), first, 3, 1)
        rd, cd, ok = _flags(torch, count, n1, n2)
        dev = torch.from_numpy(pl.image(bad)).cuda()
        p.check_device(*pl.args(dev), k1, k2, count, rd.data_ptr(), cd.data_ptr(), ok.data_ptr())
        torch.cuda.synchronize()
        want = m.check(bad, k1, k2)
        assert (rd.cpu().numpy() == want[0].reshape(-1)).all() and (cd.cpu().numpy() == want[1].reshape(-1)).all()
        assert (ok.cpu().numpy() == want[2]).all()
    print(f"product chunks of {chunk} ok")


def test_chunks_in_a_child_process(torch_cuda):
    env = dict(os.environ, POPORON_AMD_ILV_CHUNK="416")  # two DVD blocks, 27 GF(16) blocks
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks", "416"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "product chunks of 416 ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- reserve, timing ids, streams ------------------------------------------------------------

def test_reserve_then_timing_ids(torch_cuda):
    """after poporon_amd_product_reserve the calls allocate nothing: the device's free memory does not drop by the
    staging rows of 512 blocks (2 x 26 MiB; 8 MiB of slack for whatever else the runtime does; the device is shared,
    so a fresh object gets up to three attempts).  Then the ids: 24 / 25 per staged pass on the axis's handle and
    none on the in-place row route, 26 per coupled pass and for d_block_ok."""
    torch = torch_cuda
    count, k1, k2 = 512, R.DVD_K1, R.DVD_K2
    tight, ragged = Place("tight", 0, 182, 208, count), Place("ragged", 0, 182, 208, count)
    buf = torch.zeros(ragged.len, dtype=torch.uint8, device="cuda")  # all-zero blocks are clean
    rd, cd, ok = _flags(torch, count, 182, 208)
    outs = (rd.data_ptr(), cd.data_ptr(), ok.data_ptr())
    drops = []
    for _ in range(3):
        p = P.Product(R.DVD_ROW, R.DVD_COL)
        p.reserve(k1, k2, count)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        p.encode_device(*ragged.args(buf), k1, k2, count)
        p.check_device(*ragged.args(buf), k1, k2, count, *outs)
        p.decode_device(*ragged.args(buf), k1, k2, count, 0, 3, 1, None, None, outs[2])
        p.decode_device(*tight.args(buf), k1, k2, count, 1, 3, 1, *outs)
        torch.cuda.synchronize()
        drops.append(free0 - torch.cuda.mem_get_info()[0])
        assert ok.all() and not rd.any() and not cd.any() and not buf.any()
        if drops[-1] < 8 << 20:
            break
        p.close()
    assert drops[-1] < 8 << 20, drops
    h = [p.handle(0), p.handle(1)]
    ids = (P.KERNEL_PROD_GATHER, P.KERNEL_PROD_SCATTER, P.KERNEL_PROD_LISTS)

    def launches():
        torch.cuda.synchronize()
        n = [[x.timing_read(k)[1] for k in ids] for x in h]
        ms = [[x.timing_read(k)[0] for k in ids] for x in h]
        for x in h:
            x.timing(True)
        return n, ms

    for x in h:
        x.timing(True)
    # the in-place row route records neither 24 nor 25 on the row handle
    p.decode_device(*tight.args(buf), k1, k2, count, 0, 2, 1, *outs)
    n, ms = launches()
    assert n == [[0, 0, 1], [1, 1, 1]] and min(ms[1]) > 0 and ms[0][2] > 0, n
    p.decode_device(*tight.args(buf), k1, k2, count, 0, 2, 0, outs[0], outs[1], None)  # no lists, no block-ok
    assert launches()[0] == [[0, 0, 0], [1, 1, 0]]
    p.encode_device(*tight.args(buf), k1, k2, count)
    assert launches()[0] == [[0, 0, 0], [1, 1, 0]]
    p.check_device(*tight.args(buf), k1, k2, count, *outs)
    assert launches()[0] == [[0, 0, 1], [1, 0, 0]]
    # the staged row route: row, column, row, then the column check
    p.decode_device(*ragged.args(buf), k1, k2, count, 0, 3, 1, *outs)
    assert launches()[0] == [[2, 2, 2], [2, 1, 1]]
    p.encode_device(*ragged.args(buf), k1, k2, count)
    assert launches()[0] == [[1, 1, 0], [1, 1, 0]]
    p.check_device(*ragged.args(buf), k1, k2, count, *outs)
    assert launches()[0] == [[1, 0, 1], [1, 0, 0]]
    for x in h:
        x.timing(False)
    assert not buf.any() and ok.all()
    p.close()


def test_a_clean_block_comes_back_untouched(torch_cuda):
    m = _model("dvd")
    clean = _dvd_clean(2)
    want = (clean, np.zeros((2, 208), np.uint8), np.zeros((2, 182), np.uint8), np.ones(2, np.uint8))
    for kind in KINDS:
        _decode_and_compare(torch_cuda, "dvd", Place(kind, 15, 182, 208, 2), clean, want, 0, 3, 1)


def test_a_callers_stream_and_two_decodes_back_to_back(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    p, m = _product("dvd"), _model("dvd")
    clean = _dvd_clean(2)
    jobs = []
    for name in ("rows16", "burst"):
        bad, first, passes, couple, _ = _once(("pat", name), lambda: R.dvd_pattern(name, clean, SEED))
        want = _once(("patdec", name), lambda: m.decode(bad, R.DVD_K1, R.DVD_K2, first, passes, couple))
        pl = Place("ragged" if name == "burst" else "tight", 1, 182, 208, 2)
        jobs.append((pl, torch.from_numpy(pl.image(bad)).cuda(), _flags(torch, 2, 182, 208), want, first, passes))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for pl, dev, out, want, first, passes in jobs:  # the second reuses the staging rows, lists and flags
            p.decode_device(*pl.args(dev), R.DVD_K1, R.DVD_K2, 2, first, passes, 1, *[o.data_ptr() for o in out],
                            stream=s.cuda_stream)
    s.synchronize()
    for pl, dev, out, want, first, passes in jobs:
        assert (dev.cpu().numpy() == pl.image(want[0])).all()
        for o, w in zip(out, want[1:]):
            assert (o.cpu().numpy() == w.reshape(-1)).all()


# ---- host forms ------------------------------------------------------------------------------

def test_host_forms(torch_cuda):
    for pair, count in (("dvd", 225), ("gf16", 100)):  # 225 DVD blocks: two pinned chunks
        row, col, k1, k2 = PAIRS[pair]
        p, m = _product(pair), _model(pair)
        if pair == "dvd":
            clean, bad = _workload(count)
            assert (p.encode(clean[:, :k2, :k1]) == clean).all()
        else:
            msg, clean, bad = _case(pair, count)
            assert (p.encode(msg) == clean).all()
        want = m.decode(bad, k1, k2, 0, 3, 1)
        got = p.decode(bad, k1, k2, 0, 3, 1)
        for g, w in zip(got, want):
            assert (g == w).all()
    # pitches and strides in host memory; bytes between rows and blocks stay
    p, m = _product("dvd"), _model("dvd")
    clean = _dvd_clean(2)
    bad = _once(("pat", "rows16"), lambda: R.dvd_pattern("rows16", clean, SEED))[0]
    pl = Place("ragged", 3, 182, 208, 2)
    buf = pl.image(bad)
    rd, cd, ok = np.zeros(416, np.uint8), np.zeros(364, np.uint8), np.zeros(2, np.uint8)
    at = buf.ctypes.data + pl.off
    assert p.lib.poporon_decode_product(p.h, at, pl.pitch, pl.stride, R.DVD_K1, R.DVD_K2, 2, 0, 2, 1, rd.ctypes.data,
                                        cd.ctypes.data, ok.ctypes.data), P.last_error()
    assert (buf == pl.image(clean)).all() and ok.all() and not rd.any() and not cd.any()
    buf = pl.image(clean, rows=R.DVD_K2, cols=R.DVD_K1)
    assert p.lib.poporon_encode_product(p.h, buf.ctypes.data + pl.off, pl.pitch, pl.stride, R.DVD_K1, R.DVD_K2, 2)
    assert (buf == pl.image(clean)).all()


if __name__ == "__main__":
    _chunk_child(int(sys.argv[2]))
