"""Reed-Solomon decode on every syndrome vector of the small-root codes.

Every RS decoder here -- rsg_decode_k (one codeword per lane), rsgw_decode_k
(4 .. 64 lanes per codeword), the nr-root split kernels (rsk_bm_nr / rsk_ebm_nr,
rsk_chien32, rsk_forney32_nr, the applies, the list hand-off) and the
one-workgroup rs_dec1_k -- follows its syndromes through a chain of
data-dependent branches that restates the reference's integer behaviour:
erasure locator, Berlekamp-Massey, Chien with the "root in the padding"
refusal, Omega, Forney (corrected_num counted before the re-syndrome check can
fail), the check, the apply with its "location outside the row" refusal.  The
outcome depends on the syndromes, the padding and the erasure list alone, and
random error patterns reach most of those branches rarely.

A code of nr roots over GF(2^m) has 2^(m nr) syndrome vectors, and adding
every value of the nr parity symbols to one codeword produces each of them
exactly once (Oracle.syndrome_sweep).  These tests decode such a table for
every code listed in TABLES -- 2 .. 8-bit symbols, 1 .. 6 roots, odd root
counts, fcr 0 .. 2000, prim 1 .. 37, full length and shortened down to one
byte -- through every kernel family that serves the code, the host batch and
the device batch (strided rows between guard bytes), and compare the bool,
corrected_num and every byte with the CPU oracle (oracle/rs_oracle.c, itself
compared with the compiled reference on the same tables by
tests/test_oracle_golden.py).  The same tables run through the syndrome, check,
external-syndrome and single-call entry points, and, crossed with every short
erasure list, through the erasure decoders.

Every expected value comes from the oracle or from how the input was built;
no row is ever left out.
"""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import libpoporon_amd as P
from oracle import Oracle

pytestmark = pytest.mark.gpu

THREADS = 8  # oracle batches


# ---------------------------------------------------------------------------
# the codes: (symbol_size, field polynomial, fcr, prim, num_roots) -> message sizes
# ---------------------------------------------------------------------------
def _k(code):
    return (1 << code[0]) - 1 - code[4]


def _every_size(code):
    return list(range(1, _k(code) + 1))


def _three_sizes(code):
    return sorted({1, _k(code) // 2, _k(code)})


TABLES = {}
for _c in [(2, 7, 1, 1, 1), (2, 7, 1, 1, 2), (2, 7, 0, 2, 1)]:
    TABLES[_c] = _every_size(_c)
for _c in ([(3, poly, 1, 1, nr) for nr in range(1, 7) for poly in (0xB, 0xD)]
           + [(3, 0xB, 0, 3, 3), (3, 0xD, 5, 2, 6), (3, 0xB, 6, 5, 4)]):
    TABLES[_c] = _every_size(_c)
for _c in [(4, 0x13, 1, 2, nr) for nr in range(1, 5)] + [(4, 0x19, 0, 7, 3)]:
    TABLES[_c] = _three_sizes(_c)
TABLES[(4, 0x13, 0, 1, 5)] = [10]  # 2^20 rows
for _c in [(5, 0x25, 3, 1, nr) for nr in range(1, 4)]:
    TABLES[_c] = _three_sizes(_c)
TABLES[(5, 0x25, 3, 1, 4)] = [27]  # 2^20 rows
for _c in [(6, 0x43, 1, 1, nr) for nr in range(1, 4)]:
    TABLES[_c] = _three_sizes(_c)
for _c in [(7, 0x89, 1, 1, nr) for nr in range(1, 3)]:
    TABLES[_c] = _three_sizes(_c)
TABLES[(7, 0x89, 1, 1, 3)] = [1]  # 2^21 rows of 4 bytes
# byte symbols, 2 roots: the nr-root split kernels (api.cpp params_nrsplit) ...
NRSPLIT = [(8, 0x11D, 0, 1, 2), (8, 0x11D, 1, 1, 2), (8, 0x187, 5, 7, 2), (8, 0x171, 1, 11, 2)]
# ... one set past their exponent bound and a 1-root code: the general kernels
for _c in NRSPLIT + [(8, 0x11D, 2000, 37, 2), (8, 0x11D, 1, 1, 1)]:
    TABLES[_c] = _three_sizes(_c)
CODES = list(TABLES)

# tables in which the oracle must show the rare branches (conditions on the oracle's result alone)
COUNTED_FAILURES = {((3, 0xB, 1, 1, 4), 3), ((4, 0x13, 1, 2, 4), 11), ((5, 0x25, 3, 1, 4), 27)}
PAST_HALF = {((3, 0xB, 1, 1, 3), 4)}

ROUTE_ENV = {"default": {}, "generic-wave": {"POPORON_AMD_GENERIC": "wave"},
             "generic-lane": {"POPORON_AMD_GENERIC": "lane"}, "path-split": {"POPORON_AMD_DECODE_PATH": "split"},
             "path-single": {"POPORON_AMD_DECODE_PATH": "single"}, "path-wave": {"POPORON_AMD_DECODE_PATH": "wave"}}


def _routes(code):
    if code[0] <= 7:
        return ["default", "generic-wave", "generic-lane"]
    if code in NRSPLIT:
        return ["default", "path-split", "path-single", "path-wave"]
    return ["default"]


def _id(v):
    if isinstance(v, tuple):
        return "m{}-{:#x}-fcr{}-prim{}-nr{}".format(*v)
    return str(v)


CASES = [(code, route) for code in CODES for route in _routes(code)]  # code-major: the tables are built once a code


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _handle(code, route, monkeypatch, **kw):
    """The environment is read at poporon_create: set it, then create."""
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    for name in ("POPORON_AMD_GENERIC", "POPORON_AMD_DECODE_PATH", "POPORON_AMD_DECODE_TAIL",
                 "POPORON_AMD_FORCE_VERIFY"):
        monkeypatch.delenv(name, raising=False)
    for name, value in ROUTE_ENV[route].items():
        monkeypatch.setenv(name, value)
    # the reference serves every one of these codes: a refusal here is a finding
    h = P.Poporon(*code, **kw)
    assert h.supported
    return h


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _first(bad):
    return int(np.nonzero(bad)[0][0])


def _ran(h):
    """names of the kernel timers that recorded launches since timing(True)"""
    return [P.KERNEL_NAMES[k] for k in sorted(P.KERNEL_NAMES) if h.timing_read(k)[1]]


# ---------------------------------------------------------------------------
# the tables and the oracle's results, built once for each code
# ---------------------------------------------------------------------------
_CACHE = {}


def _table(code, size):
    """The sweep of (code, size), its syndromes and the oracle's decode, read-only.
    Kept for the code in hand (the cases run code-major)."""
    if _CACHE.get("code") != code:
        _CACHE.clear()
        _CACHE["code"] = code
    if size in _CACHE:
        return _CACHE[size]
    m, nr = code[0], code[4]
    o = Oracle(*code)
    data, parity = o.syndrome_sweep(size)
    n = 1 << (m * nr)
    assert data.shape == (n, size) and parity.shape == (n, nr)  # complete: one row for every syndrome vector
    flag, syn = o.syndrome_batch(data, parity)
    ok, cor, od, op = o.decode_batch(data, parity, threads=THREADS)
    t = SimpleNamespace(code=code, size=size, n=n, data=data, parity=parity, flag=flag, syn=syn,
                        want=(ok, cor, od, op), lists=None)
    for a in (data, parity, flag, syn, ok, cor, od, op):
        a.setflags(write=False)
    # -- conditions on the oracle's result alone --
    key = np.zeros(n, np.int64)
    for j in range(nr):
        key += syn[:, j].astype(np.int64) << (m * j)
    assert (np.bincount(key, minlength=n) == 1).all(), (code, size, "every syndrome vector exactly once")
    assert int((flag == 0).sum()) == 1 and flag[0] == 0
    assert ok[0] == 1 and cor[0] == 0 and (od[0] == data[0]).all() and (op[0] == parity[0]).all()
    failed = ok == 0
    assert (od[failed] == data[failed]).all() and (op[failed] == parity[failed]).all(), "a failed row was modified"
    if not (nr == 1 and size == _k(code)):
        assert failed.any(), (code, size, "no failing row")
    if (code, size) in COUNTED_FAILURES:
        assert (failed & (cor > 0)).any(), (code, size, "no failure with corrected_num counted")
    if (code, size) in PAST_HALF:
        assert (~failed & (cor > nr // 2)).any(), (code, size, "no success past nr / 2 corrections")
    _CACHE[size] = t
    return t


def _describe(t, c):
    s = f"code {_id(t.code)}, size {t.size}, row {c}, syndromes {t.syn[c % t.n].tolist()}"
    if t.lists is not None:
        s += f", erasure list {t.lists[c // t.n]}"
    return s


def _same(what, t, got, want, rows=None):
    """(ok, corrected, data', parity') of the library == the oracle's; names the first row that differs.
    rows: the table row of each compared row (default: row c is table row c)."""
    for name, g, w in zip(("ok", "corrected_num", "data", "parity"), got, want):
        bad = (g != w) if g.ndim == 1 else (g != w).any(1)
        if bad.any():
            c = _first(bad)
            r = c if rows is None else int(rows[c])
            pytest.fail(f"{what}: {name} differs: {_describe(t, r)}: got {g[c]}, oracle {w[c]} "
                        f"({int(bad.sum())} rows differ)")


def _host(h, t, data, parity, want, slots=None, counts=None, rows=None, what="host batch"):
    if slots is None:
        got = h.decode_batch(data, parity)
    else:
        got = h.decode_batch(data, parity, slots, counts)
    _same(what, t, got, want, rows)


def _device(torch, h, t, data, parity, want, count=None, slots=None, counts=None, slot_stride=0, rows=None,
            what="device batch"):
    """decode_batch_device on rows size + nr + 5 bytes apart, the first 3 bytes into a buffer of
    random guard bytes; ok / corrected pre-filled with 0xEE and 5 bytes longer than the batch.
    `count` rows are decoded (default all); the rest of the rows and flags must stay as they were.
    The whole buffer is compared: the rows with the oracle's, every other byte with what it held."""
    n, size = data.shape
    nr = parity.shape[1]
    count = n if count is None else count
    w, off = size + nr + 5, 3
    rng = np.random.default_rng(size * 131 + nr)
    buf = rng.integers(0, 256, off + n * w + 11, dtype=np.uint8)
    view = buf[off:off + n * w].reshape(n, w)
    view[:, :size] = data
    view[:, size:size + nr] = parity
    expect = buf.copy()
    ev = expect[off:off + n * w].reshape(n, w)
    ev[:count, :size] = want[2][:count]
    ev[:count, size:size + nr] = want[3][:count]
    dev = torch.from_numpy(buf).cuda()
    okd = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    cord = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    kw = {}
    if slots is not None:
        sl = rng.integers(0, 256, (n, slot_stride), dtype=np.uint8)  # junk between the rows of slots
        sl[:, :nr] = slots
        dsl = torch.from_numpy(sl).cuda()
        dcn = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint8)).cuda()
        kw = dict(d_positions=dsl.data_ptr(), positions_stride=slot_stride, d_counts=dcn.data_ptr())
    b = dev.data_ptr() + off
    h.decode_batch_device(b, w, b + size, w, size, count, okd.data_ptr(), cord.data_ptr(), stream=_stream(torch), **kw)
    torch.cuda.synchronize()
    got, ok, cor = dev.cpu().numpy(), okd.cpu().numpy(), cord.cpu().numpy()
    for name, g, wv in (("ok", ok, want[0]), ("corrected_num", cor, want[1])):
        bad = g[:count] != wv[:count]
        if bad.any():
            c = _first(bad)
            r = c if rows is None else int(rows[c])
            pytest.fail(f"{what}: {name} differs: {_describe(t, r)}: got {g[c]}, oracle {wv[c]} "
                        f"({int(bad.sum())} rows differ)")
        assert (g[count:] == 0xEE).all(), f"{what}: {name} written past the count ({_id(t.code)}, count {count})"
    if (got != expect).any():
        at = _first(got != expect)
        c, col = (at - off) // w, (at - off) % w
        where = "a guard byte"
        if off <= at < off + n * w and col < size + nr:
            r = c if rows is None else int(rows[c])
            where = ("data" if col < size else "parity") + f" byte {col if col < size else col - size} of " + (
                _describe(t, r) if c < count else f"row {c}, past the count {count}")
        pytest.fail(f"{what}: buffer byte {at} ({where}) got {got[at]}, expected {expect[at]} "
                    f"({_id(t.code)}, size {size}; {int((got != expect).sum())} bytes differ)")
    if slots is not None:
        assert (dsl.cpu().numpy() == sl).all() and (dcn.cpu().numpy() == counts).all(), "the erasure lists were written"


# ---------------------------------------------------------------------------
# 1. errors-only decode of every table through every route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code,route", CASES, ids=_id)
def test_rs_every_syndrome(torch_cuda, code, route, monkeypatch):
    """Host batch and device batch of every size's table against the oracle.  The kernel
    timers name the kernels that ran: on the default and the path-split runs of the four
    nr-root-split codes the split kernels (the Berlekamp-Massey timer), elsewhere not."""
    h = _handle(code, route, monkeypatch)
    ran = set()
    for size in TABLES[code]:
        t = _table(code, size)
        h.timing(True)
        _host(h, t, t.data, t.parity, t.want)
        bm_host = h.timing_read(P.KERNEL_BM)[1]
        ran.update(_ran(h))
        h.timing(True)
        _device(torch_cuda, h, t, t.data, t.parity, t.want)
        bm_dev = h.timing_read(P.KERNEL_BM)[1]
        ran.update(_ran(h))
        h.timing(False)
        split = code in NRSPLIT and route in ("default", "path-split")
        assert (bm_host > 0) == split and (bm_dev > 0) == split, (code, route, size, bm_host, bm_dev)
    print(f"\n[timers] {_id(code)} {route}: {sorted(ran)}")
    h.close()


# ---------------------------------------------------------------------------
# 2. batch counts at the edges of a block, of the grouped wave kernel and of the routing threshold
# ---------------------------------------------------------------------------
EDGES = [((4, 0x13, 1, 2, 4), 11), ((8, 0x11D, 1, 1, 2), 253)]


@pytest.mark.parametrize("count", [255, 256, 257, 271, 16383, 16384, 16385])
@pytest.mark.parametrize("code,size", EDGES, ids=_id)
def test_rs_count_edges(torch_cuda, code, size, count, monkeypatch):
    """The table (in a seeded order) cut to count + 16 rows, `count` of them decoded
    under the default routing: from 256 codewords on (GW_GROUP_MIN) a 15-symbol code takes
    4 lanes a codeword, 16 codewords a wave (a last wave of 0, 1 and 15 codewords; 255: one
    codeword a wave), the routing looks at the count again at 16,384, and the split
    kernels' blocks end at multiples of 256.  Rows, ok and corrected_num past the count
    stay untouched."""
    t = _table(code, size)
    sel = np.random.default_rng(count).permutation(t.n)[:count + 16]
    want = tuple(a[sel] for a in t.want)
    h = _handle(code, "default", monkeypatch)
    _device(torch_cuda, h, t, t.data[sel], t.parity[sel], want, count=count, rows=sel, what=f"count {count}")
    h.close()


# ---------------------------------------------------------------------------
# 3. the same tables through the other entry points (one size a code, default routing)
# ---------------------------------------------------------------------------
def _one_size(code):
    sizes = TABLES[code]
    return sizes[len(sizes) // 2]


@pytest.mark.parametrize("code", CODES, ids=_id)
def test_rs_every_syndrome_other_entry_points(torch_cuda, code, monkeypatch):
    """poporon_syndrome_batch_device / poporon_check_batch_device: every log-form syndrome
    vector and dirty flag equals the oracle's, so across the table the output takes every
    possible value once.  poporon_decode_batch_syndrome_device fed with those syndromes:
    the errors-only results; one row in 64 carries a value above 2^m - 1 and is refused
    (ok 0, corrected_num 0, bytes untouched: include/poporon_amd.h).  poporon_decode on
    every row of the tables of up to 4096 rows (every 16th row of the 65,536-row tables
    of the nr-root-split codes, whose single calls run on one workgroup, rs_dec1_k)."""
    torch = torch_cuda
    m, nr = code[0], code[4]
    nn = (1 << m) - 1
    size = _one_size(code)
    t = _table(code, size)
    n, w = t.n, size + nr
    h = _handle(code, "default", monkeypatch)
    s = _stream(torch)
    wire = np.concatenate([t.data, t.parity], 1)
    dev = torch.from_numpy(wire).cuda()
    b = dev.data_ptr()
    dirty = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    nz = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    syn = torch.full((n + 1, nr), -1, dtype=torch.int16, device="cuda")
    h.check_batch_device(b, w, b + size, w, size, n, dirty.data_ptr(), s)
    h.syndrome_batch_device(b, w, b + size, w, size, n, syn.data_ptr(), nr, nz.data_ptr(), s)
    torch.cuda.synchronize()
    gsyn = syn.cpu().numpy().view(np.uint16)
    for name, g in (("dirty flag", dirty.cpu().numpy()), ("nonzero flag", nz.cpu().numpy())):
        bad = g[:n] != t.flag
        if bad.any():
            pytest.fail(f"{name} differs: {_describe(t, _first(bad))}: got {g[_first(bad)]} ({int(bad.sum())} rows)")
        assert (g[n:] == 0xEE).all(), name
    bad = (gsyn[:n] != t.syn).any(1)
    if bad.any():
        c = _first(bad)
        pytest.fail(f"syndromes differ: {_describe(t, c)}: got {gsyn[c].tolist()} ({int(bad.sum())} rows)")
    assert (gsyn[n] == 0xFFFF).all() and (dev.cpu().numpy() == wire).all()

    # external syndromes: the row's own, one row in 64 with a value past the field
    xs = t.syn.copy()
    refused = np.arange(37, n, 64)
    xs[refused, (refused // 64) % nr] = nn + 1 + refused % 300
    want = [a.copy() for a in t.want]
    want[0][refused], want[1][refused] = 0, 0
    want[2][refused], want[3][refused] = t.data[refused], t.parity[refused]
    dsy = torch.from_numpy(xs.view(np.int16)).cuda()
    okd = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    cord = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    h.decode_batch_syndrome_device(b, w, b + size, w, size, n, dsy.data_ptr(), nr, okd.data_ptr(), cord.data_ptr(), s)
    torch.cuda.synchronize()
    got, ok, cor = dev.cpu().numpy(), okd.cpu().numpy(), cord.cpu().numpy()
    _same("external syndromes", t, (ok[:n], cor[:n], got[:, :size], got[:, size:]), want)
    assert (ok[n:] == 0xEE).all() and (cor[n:] == 0xEE).all()

    # single calls
    step = 1 if n <= 4096 else 16 if code in NRSPLIT else 0
    for c in range(0, n, step) if step else ():
        sok, sn, sd, sp = h.decode(t.data[c], t.parity[c])
        if not (sok == bool(t.want[0][c]) and sn == t.want[1][c] and (sd == t.want[2][c]).all()
                and (sp == t.want[3][c]).all()):
            pytest.fail(f"poporon_decode differs: {_describe(t, c)}: got {(sok, sn, sd, sp)}, oracle "
                        f"{tuple(a[c] for a in t.want)}")
    h.close()


# ---------------------------------------------------------------------------
# 4. erasure mode: the sweep crossed with every short erasure list
# ---------------------------------------------------------------------------
def _tuples(npos, nmax, distinct=False):
    """every ordered tuple of 0 .. nmax positions below npos (repeats included unless distinct)"""
    out = []
    for e in range(nmax + 1):
        out += list(itertools.permutations(range(npos), e) if distinct else itertools.product(range(npos), repeat=e))
    return out


def _m8_lists(size):
    """the empty list; single positions; pairs ascending, descending, repeated and across
    the data / parity edge"""
    mid, last = size // 2, size - 1
    return [(), (0,), (mid,), (last,), (size,), (size + 1,), (5, mid), (mid, 5), (mid, mid), (last, size),
            (size, last), (size, size + 1), (size + 1, size + 1), (0, size + 1), (last, 0)]


# (code, size, every list, parts the lists are dealt over)
ERA_TABLES = [((3, 0xB, 1, 1, 3), 4, _tuples(7, 3), 1), ((3, 0xB, 1, 1, 3), 1, _tuples(4, 3), 1),
              ((3, 0xB, 1, 1, 4), 3, _tuples(7, 4, distinct=True), 4), ((2, 7, 1, 1, 2), 1, _tuples(3, 2), 1),
              ((4, 0x13, 1, 2, 2), 13, _tuples(15, 2), 1)]
assert [len(x[2]) for x in ERA_TABLES] == [400, 85, 1100, 13, 241]
ERA8_TABLES = [((8, 0x11D, 1, 1, 2), 253, 3), ((8, 0x11D, 0, 1, 2), 100, 3)]


def _slot_rows(lists, first, nr, width):
    """nr slots for each list: its positions, then in-range stale values from a fixed formula
    of the list's index (the apply reads them when the locator's degree passes the count)"""
    slots = np.zeros((len(lists), nr), np.uint8)
    counts = np.zeros(len(lists), np.uint8)
    for i, lst in enumerate(lists):
        li = first + i
        slots[i] = [(5 * li + 3 * j + 1) % width for j in range(nr)]
        slots[i, :len(lst)] = lst
        counts[i] = len(lst)
    assert (slots < width).all()
    return slots, counts


def _erasure_table(code, size, lists, first):
    """The sweep of (code, size) under each list, list-major, and the oracle's erasure decode."""
    nr = code[4]
    base = _table(code, size)
    slots, counts = _slot_rows(lists, first, nr, size + nr)
    data, parity = np.tile(base.data, (len(lists), 1)), np.tile(base.parity, (len(lists), 1))
    slots, counts = np.repeat(slots, base.n, axis=0), np.repeat(counts, base.n)
    want = Oracle(*code).decode_batch(data, parity, slots.astype(np.uint32), counts.astype(np.uint32), threads=THREADS)
    assert len(want[0]) == base.n * len(lists)  # complete: every syndrome vector under every list
    failed = want[0] == 0
    assert (want[2][failed] == data[failed]).all() and (want[3][failed] == parity[failed]).all()
    t =SimpleNamespace(code=code, size=size, n=base.n, syn=base.syn, lists=lists)
    return t, data, parity, slots, counts, want


ERA_CASES = [(code, size, part, route) for code, size, lists, parts in ERA_TABLES for part in range(parts)
             for route in ("default", "generic-wave", "generic-lane")]


@pytest.mark.parametrize("code,size,part,route", ERA_CASES, ids=_id)
def test_rs_every_syndrome_every_erasure_list(torch_cuda, code, size, part, route, monkeypatch):
    """u8 slots through the host batch (rows of nr slots) and the device batch (rows nr + 3
    apart, junk between).  Under the default routing the 3-bit tables also send every 97th
    row through an erasure object and poporon_decode: the object filled with the row's nr
    slots, reset, and the real positions added, so the stale slots stay readable behind
    the count as in the reference."""
    lists, parts = next((x[2], x[3]) for x in ERA_TABLES if x[0] == code and x[1] == size)
    per = -(-len(lists) // parts)
    first = part * per
    t, data, parity, slots, counts, want = _erasure_table(code, size, lists[first:first + per], first)
    t.lists = lists[first:first + per]
    nr = code[4]
    h = _handle(code, route, monkeypatch)
    _host(h, t, data, parity, want, slots, counts, what="erasure host batch")
    _device(torch_cuda, h, t, data, parity, want, slots=slots, counts=counts, slot_stride=nr + 3,
            what="erasure device batch")
    h.close()
    if code[0] == 3 and route == "default":
        er = P.Erasure(nr, nr)
        he = _handle(code, route, monkeypatch, erasure=er)
        loaded = -1
        for c in range(0, len(counts), 97):
            if c // t.n != loaded:
                loaded = c // t.n
                er.set(slots[c])
                er.set(slots[c][:counts[c]])
            sok, sn, sd, sp = he.decode(data[c], parity[c])
            if not (sok == bool(want[0][c]) and sn == want[1][c] and (sd == want[2][c]).all()
                    and (sp == want[3][c]).all()):
                pytest.fail(f"poporon_decode with an erasure object differs: {_describe(t, c)}: got "
                            f"{(sok, sn, sd, sp)}, oracle {tuple(a[c] for a in want)}")
        he.close()


@pytest.mark.parametrize("code,size,part", [(c, s, p) for c, s, parts in ERA8_TABLES for p in range(parts)], ids=_id)
def test_rs_every_syndrome_erasure_lists_m8(torch_cuda, code, size, part, monkeypatch):
    """The 65,536-row tables of two byte-symbol codes under 15 erasure lists.  Device rows
    of slots 4 bytes apart take the errata split kernels with npar = 2 (rsk_ebm_nr,
    rsk_chien32, rsk_forney32_nr, rsk_apply_era_nr: the Berlekamp-Massey timer counts
    them); the host batch hands over rows of nr slots, which the general kernel takes,
    as does every batch of a handle created with POPORON_AMD_DECODE_PATH=single."""
    nr = code[4]
    all_lists = _m8_lists(size)
    per = -(-len(all_lists) // ERA8_TABLES[0][2])
    h = _handle(code, "default", monkeypatch)
    hs = _handle(code, "path-single", monkeypatch)
    for li in range(part * per, min(len(all_lists), (part + 1) * per)):
        t, data, parity, slots, counts, want = _erasure_table(code, size, all_lists[li:li + 1], li)
        t.lists = all_lists[li:li + 1]
        for hh, split in ((h, True), (hs, False)):
            _host(hh, t, data, parity, want, slots, counts, what="erasure host batch")
            hh.timing(True)
            _device(torch_cuda, hh, t, data, parity, want, slots=slots, counts=counts, slot_stride=4,
                    what="erasure device batch" + ("" if split else " (single)"))
            bm = hh.timing_read(P.KERNEL_BM)[1]
            if li == 0:
                print(f"\n[timers] {_id(code)} erasures {'default' if split else 'path-single'}: {_ran(hh)}")
            hh.timing(False)
            assert (bm > 0) == split, (code, li, bm)
    h.close()
    hs.close()
