"""The split Reed-Solomon decode kernels on rows built from chosen syndromes and on
batches whose waves are alike.

rs_bm_k<false> / rs_bm_k<true>, rs_chien_k, rs_forney_apply_k, rs_forney_k + rs_apply_k and
the hand-off list into the general kernels claim bit-exact agreement with the reference,
its failures and their corrected_num included, on branches that random error patterns
reach about once in 256 Berlekamp-Massey steps or never (runs of zero discrepancies, a
jump of L, L > 16, a locator that would pass x^16, deg != L, a root in the padding of a
shortened row), and they take wave-uniform shortcuts (the clean-wave exit, the wave
maxima that bound the coefficient loops, the degmax == 16 Omega, the "no fast row in
this wave" exits) that batches of independently drawn rows never leave.

tests/rs_syndrome_rows.py builds rows for the first and layouts for the second, from the
CPU oracle and GF(2) linear algebra alone; tests/test_rs_syndrome_rows_cpu.py compares the
oracle with the compiled reference on the same rows.  Here every route through the
library decodes them, and ok, corrected_num and every byte must equal the oracle's.  No
row is left out and nothing is approximate.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import libpoporon_amd as P
import rs_syndrome_rows as R
from oracle import Oracle

pytestmark = pytest.mark.gpu

THREADS = 8  # oracle batches

# (symbol_size, field polynomial, fcr, prim, num_roots) -> the family conditions the code is
# excused from, as in tests/test_rs_syndrome_rows_cpu.py.  The reasons are written there, and
# so is why every code, the 32-root ones included, has single syndromes S_j (j + 1 = 17, 15
# or 5, a divisor of 255 above t) that a full-length row "corrects" in j + 1 places.
DEFAULT = (8, 0x11D, 1, 1, 32)
CODES = {
    DEFAULT: (),
    (8, 0x11D, 0, 1, 32): (),
    (8, 0x11D, 5, 7, 32): (),
    (8, 0x187, 5, 1, 31): (),
    (8, 0x11D, 1, 1, 16): (),
    (8, 0x11D, 3, 1, 8): ("late_fails",),
}

# POPORON_AMD_DECODE_PATH x POPORON_AMD_DECODE_TAIL (the tail matters on the split kernels only)
ROUTES = {"default": {}, "default+tail-split": {"POPORON_AMD_DECODE_TAIL": "split"},
          "default+tail-fused": {"POPORON_AMD_DECODE_TAIL": "fused"},
          "split": {"POPORON_AMD_DECODE_PATH": "split"},
          "split+tail-split": {"POPORON_AMD_DECODE_PATH": "split", "POPORON_AMD_DECODE_TAIL": "split"},
          "split+tail-fused": {"POPORON_AMD_DECODE_PATH": "split", "POPORON_AMD_DECODE_TAIL": "fused"},
          "single": {"POPORON_AMD_DECODE_PATH": "single"}, "wave": {"POPORON_AMD_DECODE_PATH": "wave"}}


def _id(v):
    if isinstance(v, tuple):
        return "m{}-{:#x}-fcr{}-prim{}-nr{}".format(*v)
    return str(v)


def _k(code):
    return 255 - code[4]


def _short(code):
    """a shortened size with at least 64 bytes of padding, no multiple of 4 or 16"""
    return {32: 101, 31: 61, 16: 150, 8: 37}[code[4]]


def _takes_split(code, route):
    """The split kernels serve a code whose verification exponents stay below 2^15
    (api.cpp: RsCorrParams.vfast), on the default route and under DECODE_PATH=split."""
    fcr, prim, nr = code[2:]
    path = ROUTES[route].get("POPORON_AMD_DECODE_PATH")
    return (fcr + nr - 1) * prim * 254 < 32768 and path not in ("single", "wave")


def _by_size_only(code, route):
    """32-root codes take the split kernels on the default route from SPLIT_MIN_COUNT rows on"""
    return code[4] == 32 and "POPORON_AMD_DECODE_PATH" not in ROUTES[route]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _handle(code, route, monkeypatch):
    """The environment is read at poporon_create: set it, then create."""
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    for name in ("POPORON_AMD_GENERIC", "POPORON_AMD_DECODE_PATH", "POPORON_AMD_DECODE_TAIL",
                 "POPORON_AMD_FORCE_VERIFY"):
        monkeypatch.delenv(name, raising=False)
    for name, value in ROUTES[route].items():
        monkeypatch.setenv(name, value)
    h = P.Poporon(*code)
    assert h.supported
    return h


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _first(bad):
    return int(np.nonzero(bad)[0][0])


# ---------------------------------------------------------------------------
# the pools and the oracle's results, built once for each (code, size)
# ---------------------------------------------------------------------------
_CACHE = {}
ORDINARY_ROWS = R.BM_WORKGROUP  # of each error count 0 .. t + 1: uniform_blocks repeats no row
ZERO_RUN_DRAWS = 4  # rows of each (k, w): whole waves of zero_run rows in the sorted layout


def _pool(code, size):
    """Every family and ORDINARY_ROWS rows of each error count, their syndromes (log form)
    and the oracle's decode, read-only."""
    if (code, size) in _CACHE:
        return _CACHE[(code, size)]
    o = Oracle(*code)
    k = _k(code)
    full_key = ("map", code)
    if full_key not in _CACHE:
        _CACHE[full_key] = R.SyndromeMap(o, k)
    full = _CACHE[full_key]
    sm = full if size == k else R.SyndromeMap(o, size)
    t = sm.t
    pool = R.Pool.concat([R.family_pool(sm, full, zero_run_draws=ZERO_RUN_DRAWS)] +
                         [R.ordinary(sm, e, ORDINARY_ROWS) for e in range(t + 2)])
    flag, syn = o.syndrome_batch(pool.data, pool.parity)
    want = o.decode_batch(pool.data, pool.parity, threads=THREADS)
    # -- conditions on the oracle alone: no family has quietly become trivial --
    seen = R.family_conditions(pool, want, CODES[code])
    assert ("padding_roots" in seen) == (size < k)
    assert size < k or seen["sparse"][1] >= 15  # sparse(): successes with more than t corrections
    e_of = np.array([g.e if g.family == "ordinary" else -1 for g in pool.tags])
    assert (flag[e_of == 0] == 0).all() and (flag[e_of != 0] == 1).all()
    within = (e_of >= 0) & (e_of <= t)
    assert (want[0][within] == 1).all() and (want[1][within] == np.minimum(e_of, size + code[4])[within]).all()
    assert len(R.list_rows(pool, t)) >= 30  # lone_lane repeats them to fill a wave
    for a in (pool.data, pool.parity, flag, syn) + tuple(want):
        a.setflags(write=False)
    pc = SimpleNamespace(code=code, size=size, t=t, pool=pool, syn=syn, want=want, o=o, lists=None)
    _CACHE[(code, size)] = pc
    return pc


def _describe(pc, r):
    s = f"code {_id(pc.code)}, size {pc.size}, pool row {r}, {pc.pool.tags[r]!r}, syndromes {pc.syn[r].tolist()}"
    if pc.lists is not None:
        s += f", erasure list {pc.lists[r]}"
    return s


def _take(pc, order, want=None):
    want = pc.want if want is None else want
    return pc.pool.data[order], pc.pool.parity[order], tuple(a[order] for a in want)


def _same(what, pc, got, want, rows):
    """(ok, corrected, data', parity') of the library == the oracle's; names the first row that
    differs.  rows: the pool row of each compared row."""
    for name, g, w in zip(("ok", "corrected_num", "data", "parity"), got, want):
        bad = (g != w) if g.ndim == 1 else (g != w).any(1)
        if bad.any():
            c = _first(bad)
            pytest.fail(f"{what}: {name} differs at batch row {c}: {_describe(pc, int(rows[c]))}: got {g[c]}, "
                        f"oracle {w[c]} ({int(bad.sum())} rows differ)")


def _host(h, pc, order, what="host batch", slots=None, counts=None, want=None):
    data, parity, want = _take(pc, order, want)
    got = h.decode_batch(data, parity) if slots is None else h.decode_batch(data, parity, slots, counts)
    _same(what, pc, got, want, order)


def _device(torch, h, pc, order, count=None, extra=5, off=3, slots=None, counts=None, slot_stride=0, ext_syn=None,
            want=None, what="device batch"):
    """decode_batch_device on rows size + nr + extra bytes apart, `off` bytes into a buffer of
    random guard bytes (extra 0: the wire layout); ok / corrected pre-filled with 0xEE and 5
    bytes longer than the batch.  `count` rows are decoded (default all); the rest of the
    rows and flags must stay as they were.  The whole buffer is compared: the rows with the
    oracle's, every other byte with what it held.  ext_syn: log-form syndromes of every row,
    for decode_batch_syndrome_device."""
    data, parity, want = _take(pc, order, want)
    n, size = data.shape
    nr = parity.shape[1]
    count = n if count is None else count
    w = size + nr + extra
    rng = np.random.default_rng(size * 131 + nr + extra)
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
    b = dev.data_ptr() + off
    if ext_syn is not None:
        dsy = torch.from_numpy(np.ascontiguousarray(ext_syn).view(np.int16)).cuda()
        h.decode_batch_syndrome_device(b, w, b + size, w, size, count, dsy.data_ptr(), nr, okd.data_ptr(),
                                       cord.data_ptr(), _stream(torch))
    else:
        kw = {}
        if slots is not None:
            sl = rng.integers(0, 256, (n, slot_stride), dtype=np.uint8)  # junk between the rows of slots
            sl[:, :nr] = slots
            dsl = torch.from_numpy(sl).cuda()
            dcn = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint8)).cuda()
            kw = dict(d_positions=dsl.data_ptr(), positions_stride=slot_stride, d_counts=dcn.data_ptr())
        h.decode_batch_device(b, w, b + size, w, size, count, okd.data_ptr(), cord.data_ptr(), stream=_stream(torch),
                              **kw)
    torch.cuda.synchronize()
    got, ok, cor = dev.cpu().numpy(), okd.cpu().numpy(), cord.cpu().numpy()
    for name, g, wv in (("ok", ok, want[0]), ("corrected_num", cor, want[1])):
        bad = g[:count] != wv[:count]
        if bad.any():
            c = _first(bad)
            pytest.fail(f"{what}: {name} differs at batch row {c}: {_describe(pc, int(order[c]))}: got {g[c]}, "
                        f"oracle {wv[c]} ({int(bad.sum())} rows differ)")
        assert (g[count:] == 0xEE).all(), f"{what}: {name} written past the count ({_id(pc.code)}, count {count})"
    if (got != expect).any():
        at = _first(got != expect)
        c, col = (at - off) // w, (at - off) % w
        where = "a guard byte"
        if off <= at < off + n * w and col < size + nr:
            where = ("data" if col < size else "parity") + f" byte {col if col < size else col - size} of " + (
                f"batch row {c}: " + _describe(pc, int(order[c])) if c < count else f"row {c}, past the count {count}")
        pytest.fail(f"{what}: buffer byte {at} ({where}) got {got[at]}, expected {expect[at]} "
                    f"({_id(pc.code)}, size {size}; {int((got != expect).sum())} bytes differ)")
    if slots is not None:
        assert (dsl.cpu().numpy() == sl).all() and (dcn.cpu().numpy() == counts).all(), "the erasure lists were written"


def _timed(h, fn):
    """launches of the Berlekamp-Massey timer (the split kernels) during fn()"""
    h.timing(True)
    fn()
    n = h.timing_read(P.KERNEL_BM)[1]
    h.timing(False)
    return n


# ---------------------------------------------------------------------------
# 1. every family, grouped and shuffled, through every route
# ---------------------------------------------------------------------------
SIZED = [(code, size) for code in CODES for size in (_k(code), _short(code))] + [(DEFAULT, 1)]
CHOSEN = [(code, size, route) for code, size in SIZED for route in ROUTES]


@pytest.mark.parametrize("code,size,route", CHOSEN, ids=_id)
def test_chosen_syndromes(torch_cuda, code, size, route, monkeypatch):
    """All families and the ordinary rows in the sorted_by_tag layout (whole waves of one
    family, whole waves on the list) and the shuffled one: the host batch, and the device
    batch on strided rows between guard bytes.  On the default route a 32-root batch is
    repeated up to SPLIT_MIN_COUNT rows, below which it would not reach the split kernels.
    The Berlekamp-Massey timer says whether the split kernels ran."""
    pc = _pool(code, size)
    h = _handle(code, route, monkeypatch)
    for name, order in (("sorted_by_tag", R.sorted_by_tag(pc.pool)), ("shuffled", R.shuffled(pc.pool))):
        if _by_size_only(code, route):
            order = R.pad_to(order)
        bm_host = _timed(h, lambda: _host(h, pc, order, what=f"host batch, {name}"))
        bm_dev = _timed(h, lambda: _device(torch_cuda, h, pc, order, what=f"device batch, {name}"))
        split = _takes_split(code, route)
        assert (bm_host > 0) == split and (bm_dev > 0) == split, (code, size, route, name, bm_host, bm_dev)
    h.close()


# ---------------------------------------------------------------------------
# 2. waves whose rows are alike
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code,route", [(code, route) for code in CODES for route in ROUTES], ids=_id)
def test_wave_composition(torch_cuda, code, route, monkeypatch):
    """uniform_blocks (512 rows of each error count 0 .. t + 1: a workgroup of rs_bm_k, 8
    waves of one degree; clean waves between dirty ones) and lone_lane (one row of another
    kind at lane 0, 31, 32, 63), at the full count and at counts 64 q + 1 and 64 q + 63, each
    in the wire layout (rows size + nr apart, the block apply) at size k and on a padded
    stride at the shortened size; the host batch at an odd count.  Default route of a
    32-root code: repeated past SPLIT_MIN_COUNT."""
    for size, extra, off in ((_k(code), 0, 0), (_short(code), 9, 1)):
        pc = _pool(code, size)
        h = _handle(code, route, monkeypatch)
        order = np.concatenate([R.uniform_blocks(pc.pool, pc.t), R.lone_lane(pc.pool, pc.t)])
        assert len(order) % R.BM_WORKGROUP == 0
        if _by_size_only(code, route):
            order = R.pad_to(order, R.SPLIT_MIN_COUNT + R.WAVE)
        c1, c63 = R.odd_counts(len(order))
        assert c1 % 64 == 1 and c63 % 64 == 63 and (not _by_size_only(code, route) or c63 >= R.SPLIT_MIN_COUNT)
        for count in (len(order), c1, c63):
            bm = _timed(h, lambda: _device(torch_cuda, h, pc, order, count=count, extra=extra, off=off,
                                           what=f"count {count}, rows {size + code[4] + extra} apart"))
            assert (bm > 0) == _takes_split(code, route), (code, size, route, count, bm)
        _host(h, pc, order[:c63 if extra == 0 else c1], what="host batch")
        h.close()


# ---------------------------------------------------------------------------
# 3. the same syndrome vectors as external syndromes
# ---------------------------------------------------------------------------
EXTERNAL_ROWS = 200  # of each family


@pytest.mark.parametrize("route", ["default", "split", "split+tail-fused", "single", "wave"])
@pytest.mark.parametrize("code", [DEFAULT, (8, 0x11D, 1, 1, 16)], ids=_id)
def test_chosen_syndromes_external(torch_cuda, code, route, monkeypatch):
    """The families' syndromes, log form, fed to decode_batch_syndrome_device on clean rows
    (the codewords the family rows were built on), against Oracle.decode(..., ext_syn=...)
    row by row: up to EXTERNAL_ROWS rows of each family, grouped by family and then
    shuffled."""
    size = _k(code)
    pc = _pool(code, size)
    key = ("external", code)
    if key not in _CACHE:
        fam = pc.pool.families()
        rng = np.random.default_rng(code[4])
        sel = np.concatenate([rng.permutation(np.nonzero(fam == f)[0])[:EXTERNAL_ROWS] for f in np.unique(fam)])
        sel = np.concatenate([sel, rng.permutation(sel)])
        data = np.ascontiguousarray(pc.pool.clean[sel, :size])
        parity = np.ascontiguousarray(pc.pool.clean[sel, size:])
        assert not pc.o.syndrome_batch(data, parity)[0].any()
        res = [pc.o.decode(data[c], parity[c], ext_syn=pc.syn[sel[c]]) for c in range(len(sel))]
        want = (np.array([r[0] for r in res], np.uint8), np.array([r[1] for r in res], np.uint32),
                np.array([r[2] for r in res]), np.array([r[3] for r in res]))
        assert want[0].any() and not want[0].all()
        assert ((want[2] != data).any(1) | (want[3] != parity).any(1))[want[0] == 1].any()
        _CACHE[key] = (sel, data, parity, want)
    sel, data, parity, want = _CACHE[key]
    idx = np.arange(len(sel))
    if _by_size_only(code, route):
        idx = R.pad_to(idx)
    h = _handle(code, route, monkeypatch)
    # _device indexes data / parity / want through `order`: hand it the batch as its own pool
    view = SimpleNamespace(code=code, size=size, lists=None, syn=pc.syn[sel], want=want,
                           pool=SimpleNamespace(data=data, parity=parity, tags=[pc.pool.tags[r] for r in sel]))
    bm = _timed(h, lambda: _device(torch_cuda, h, view, idx, ext_syn=pc.syn[sel][idx], what="external syndromes"))
    assert (bm > 0) == _takes_split(code, route), (code, route, bm)
    h.close()


# ---------------------------------------------------------------------------
# 4. the exotic rows with part of their errors named as erasures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["split", "single"])
@pytest.mark.parametrize("size", [_k(DEFAULT), _short(DEFAULT)])
def test_chosen_syndromes_with_erasures(torch_cuda, size, route, monkeypatch):
    """zero_run and late_discrepancy rows of the default code, each three times: with 1, 2
    and w of its true error positions as its erasure list (late_discrepancy: of its e
    ordinary errors; fewer where the row has fewer), the other slots stale.  Host batch
    and device batch (slot rows 32 bytes apart: the errata split kernels under
    DECODE_PATH=split) against Oracle.decode_batch(..., erasures, counts)."""
    code, nr = DEFAULT, DEFAULT[4]
    pc = _pool(code, size)
    key = ("erasures", size)
    if key not in _CACHE:
        rows = pc.pool.where(lambda g: g.family in ("zero_run", "late_discrepancy"))
        order, slots, counts = [], [], []
        for r in rows:
            g = pc.pool.tags[r]
            w = g.w if g.family == "zero_run" else g.e
            for f in (1, 2, w):
                f = min(f, w)
                sl = [(5 * r + 3 * j + 1) % (size + nr) for j in range(nr)]  # stale, in range
                sl[:f] = g.positions[:f]
                order.append(r)
                slots.append(sl)
                counts.append(f)
        order = np.array(order)
        slots, counts = np.array(slots, np.uint8), np.array(counts, np.uint8)
        want = pc.o.decode_batch(pc.pool.data[order], pc.pool.parity[order], slots.astype(np.uint32),
                                 counts.astype(np.uint32), threads=THREADS)
        assert (want[0] == 1).any() and (want[0] == 0).any(), "some rows succeed and some fail"
        failed = want[0] == 0
        assert (want[2][failed] == pc.pool.data[order][failed]).all()
        assert (want[3][failed] == pc.pool.parity[order][failed]).all()
        _CACHE[key] = (order, slots, counts, want)
    order, slots, counts, want = _CACHE[key]
    lists = [s[:c].tolist() for s, c in zip(slots, counts)]
    view = SimpleNamespace(code=code, size=size, syn=pc.syn[order], lists=lists,
                           pool=SimpleNamespace(data=pc.pool.data[order], parity=pc.pool.parity[order],
                                                tags=[pc.pool.tags[r] for r in order]), want=want)
    idx = np.arange(len(order))
    h = _handle(code, route, monkeypatch)
    _host(h, view, idx, what="erasure host batch", slots=slots, counts=counts)
    bm = _timed(h, lambda: _device(torch_cuda, h, view, idx, slots=slots, counts=counts, slot_stride=nr,
                                   what="erasure device batch"))
    assert (bm > 0) == (route == "split"), (size, route, bm)
    h.close()
