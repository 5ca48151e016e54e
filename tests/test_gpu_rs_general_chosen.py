"""The general Reed-Solomon kernels (rs_generic.hip) on rows built from chosen syndromes, on
waves whose codeword groups are alike or all but one, and on chosen pairs.

rsgw_decode_k<PosT, GL> runs a codeword on GL lanes, the groups of a wave diverging per
codeword around DPP shifts, readlane, __ballot and gw_sync(); its Berlekamp-Massey starts on
one or two register slots and hands over to two or four at the first iteration at which B
holds a nonzero at index GL NQ - 1 (with a list: only when ne < GL or ne < 2 GL); with GL 64 in
errors mode two codewords share a wave, their BM loops interleaved and the hand-off taken when
either asks for it (gw_decode_pair / gw_bm2); rsg_decode_k runs a codeword per lane.  Batches
of independently drawn rows reach the hand-off of a short code never (15 symbols), a refusal
on a long one never, and leave every wave mixed.

tests/rs_syndrome_rows.py builds the rows (general_pool with the handoff family,
general_errata_pool) and the layouts (group_layout, pair_layout) from the CPU oracle, GF(2)
linear algebra and a Berlekamp-Massey trace that only tags rows;
tests/test_rs_general_rows_cpu.py names the codes and compares the oracle with the compiled
reference on the same rows, lists and external syndromes.  Here the library decodes them
and ok, corrected_num and every byte must equal the oracle's, between 0xA5 guard bytes that
must stay.  No row is left out and nothing is approximate.

Which kernel form a batch takes, from the launcher (rsgw_decode_launch, gw_grid,
rsgw_decode_k) and api.cpp (gen_wave), not from any probe:
  POPORON_AMD_GENERIC=lane   rsg_decode_k, a codeword per lane, at every count
  default (below 16,384 rows) and POPORON_AMD_GENERIC=wave: rsgw_decode_k with
    count < 256              GL 64 whatever the code (the batches named "below 256")
    count >= 256             GL 4 / 8 / 16 / 32 / 64 for codes of up to 15 / 31 / 63 / 127 / 255
                             symbols: 16 .. 1 codewords a wave, 64 .. 4 a workgroup
    GL 64, errors mode, 8 <= nr < 128, count > stride = min(ceil(count / 4), 8 CUs) 4:
                             rows e and e + stride in one wave (gw_decode_pair) for
                             e < count - stride, the rest alone
  single calls: rsgw_decode_k<uint32_t, 64> on one codeword, slots from the erasure object
"""
import numpy as np
import pytest

import libpoporon_amd as P
import rs_syndrome_rows as R
from oracle import Oracle
from test_rs_general_rows_cpu import CODES, _nn, external_cases

pytestmark = pytest.mark.gpu


def _id(v):
    return "m{}-{:#x}-fcr{}-prim{}-nr{}".format(*v) if isinstance(v, tuple) else str(v)



ROUTES = {"default": None, "wave": "wave", "lane": "lane"}  # POPORON_AMD_GENERIC, read at poporon_create
GUARD = 0xA5
SMALL = 252  # rows of a batch below GW_GROUP_MIN: whole workgroups of four codewords


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _handle(code, route, monkeypatch, **kw):
    """The environment is read at poporon_create: set it, then create."""
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    for name in ("POPORON_AMD_GENERIC", "POPORON_AMD_DECODE_PATH", "POPORON_AMD_DECODE_TAIL", "POPORON_AMD_FORCE_VERIFY"):
        monkeypatch.delenv(name, raising=False)
    if ROUTES[route]:
        monkeypatch.setenv("POPORON_AMD_GENERIC", ROUTES[route])
    h = P.Poporon(*code, **kw)
    assert h.supported
    return h


_CACHE = {}


def _case(code, size):
    """rs_syndrome_rows.general_case of (code, size), built once; read-only"""
    if (code, size) not in _CACHE:
        o = Oracle(*code)
        if ("map", code) not in _CACHE:
            _CACHE[("map", code)] = R.SyndromeMap(o, _nn(code) - code[4])
        pc = R.general_case(o, size, _CACHE[("map", code)], CODES[code])
        pc.code = code
        _CACHE[(code, size)] = pc
    return _CACHE[(code, size)]


def _external(code, size):
    if ("external", code, size) not in _CACHE:
        got = external_cases(_case(code, size))
        for a in got[:3] + tuple(got[3]):
            a.setflags(write=False)
        _CACHE[("external", code, size)] = got
    return _CACHE[("external", code, size)]


def _sizes(code):
    return R.general_sizes(_nn(code), code[4])


def _grouped(code):
    return R.group_lanes(_nn(code))


def _first(bad):
    return int(np.nonzero(bad)[0][0])


class Rows:
    """A set of rows to decode with what the oracle makes of them: data, parity, want (ok,
    corrected_num, data', parity'), and describe(c) for a failure's message."""

    def __init__(self, code, data, parity, want, describe, slots=None, counts=None, syn=None):
        self.code, self.data, self.parity, self.want, self.describe = code, data, parity, want, describe
        self.slots, self.counts, self.syn = slots, counts, syn

    def take(self, order):
        pick = lambda a: None if a is None else a[order]  # noqa: E731
        return Rows(self.code, self.data[order], self.parity[order], tuple(a[order] for a in self.want),
                    lambda c: self.describe(int(order[c])), pick(self.slots), pick(self.counts), pick(self.syn))

    def __len__(self):
        return len(self.data)


def _errors(pc):
    return Rows(pc.code, pc.pool.data, pc.pool.parity, pc.want,
                lambda r: f"pool row {r}, {pc.pool.tags[r]!r}, syndromes {pc.syn[r].tolist()}")


def _lists(pc):
    ep = pc.epool
    return Rows(pc.code, ep.data, ep.parity, pc.ewant,
                lambda r: f"list row {r}, {ep.tags[r]!r}, list {ep.tags[r].slots[:ep.tags[r].count]} + stale "
                          f"{ep.tags[r].slots[ep.tags[r].count:]}", slots=ep.slots, counts=ep.counts)


def _device(torch, h, rows, what, count=None, extra=5, off=3, apart=False, slot_stride=None):
    """One device batch of `rows` between guard bytes of 0xA5: rows size + nr + extra bytes apart
    `off` bytes into one buffer (parity behind the data), or with apart: data rows size + extra
    apart in one buffer and parity rows nr + extra + 2 apart in another.  ok and corrected_num
    are 5 flags longer than the batch; `count` rows are decoded (default all).  Whole buffers
    are compared: the decoded rows with the oracle's, every other byte with the guard."""
    data, parity, want = rows.data, rows.parity, rows.want
    n, size = data.shape
    nr = parity.shape[1]
    count = n if count is None else count
    assert 0 < count <= n
    where = f"{what}, count {count}, {_id(rows.code)}, size {size}"
    if apart:
        wd, wp = size + extra, nr + extra + 2
        bufs = [np.full(off + n * wd + 11, GUARD, np.uint8), np.full(off + 1 + n * wp + 7, GUARD, np.uint8)]
        views = [bufs[0][off:off + n * wd].reshape(n, wd)[:, :size], bufs[1][off + 1:off + 1 + n * wp].reshape(n, wp)[:, :nr]]
    else:
        wd = wp = size + nr + extra
        bufs = [np.full(off + n * wd + 11, GUARD, np.uint8)]
        v = bufs[0][off:off + n * wd].reshape(n, wd)
        views = [v[:, :size], v[:, size:size + nr]]
    views[0][:], views[1][:] = data, parity
    dev = [torch.from_numpy(b).cuda() for b in bufs]
    views[0][:count], views[1][:count] = want[2][:count], want[3][:count]  # bufs: now what must come back
    okd = torch.full((n + 5,), GUARD, dtype=torch.uint8, device="cuda")
    cord = torch.full((n + 5,), GUARD, dtype=torch.uint8, device="cuda")
    bd = dev[0].data_ptr() + off
    bp = dev[1].data_ptr() + off + 1 if apart else bd + size
    stream = torch.cuda.current_stream().cuda_stream
    sl = dsl = dcn = None
    if rows.syn is not None:
        ss = nr + 3  # u16 values between rows: 0xA5A5, out of every table
        sy = np.full((n, ss), GUARD * 257, np.uint16)
        sy[:, :nr] = rows.syn
        dsy = torch.from_numpy(sy.view(np.int16)).cuda()
        h.decode_batch_syndrome_device(bd, wd, bp, wp, size, count, dsy.data_ptr(), ss, okd.data_ptr(), cord.data_ptr(),
                                       stream)
    elif rows.slots is not None:
        slot_stride = nr if slot_stride is None else slot_stride
        sl = np.full((n, slot_stride), GUARD, np.uint8)
        sl[:, :nr] = rows.slots
        dsl = torch.from_numpy(sl).cuda()
        dcn = torch.from_numpy(np.ascontiguousarray(rows.counts, dtype=np.uint8)).cuda()
        h.decode_batch_device(bd, wd, bp, wp, size, count, okd.data_ptr(), cord.data_ptr(), d_positions=dsl.data_ptr(),
                              positions_stride=slot_stride, d_counts=dcn.data_ptr(), stream=stream)
    else:
        h.decode_batch_device(bd, wd, bp, wp, size, count, okd.data_ptr(), cord.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    ok, cor = okd.cpu().numpy(), cord.cpu().numpy()
    for name, g, wv in (("ok", ok, want[0]), ("corrected_num", cor, want[1])):
        bad = g[:count] != wv[:count]
        if bad.any():
            c = _first(bad)
            pytest.fail(f"{where}: {name} differs at batch row {c}: {rows.describe(c)}: got {g[c]}, oracle {wv[c]} "
                        f"({int(bad.sum())} rows differ)")
        assert (g[count:] == GUARD).all(), f"{where}: {name} written past the count"
    for which, (d, b, w) in enumerate(zip(dev, bufs, (wd, wp))):
        got = d.cpu().numpy()
        if (got != b).any():
            at = _first(got != b)
            o = off + (1 if apart and which else 0)
            c, col = (at - o) // w, (at - o) % w
            row = rows.describe(c) if o <= at and c < count else "no decoded row"
            pytest.fail(f"{where}: {'parity' if which else 'data'} buffer byte {at} (batch row {c}, column {col}; {row}) "
                        f"got {got[at]}, expected {b[at]} ({int((got != b).sum())} bytes differ)")
    if sl is not None:
        assert (dsl.cpu().numpy() == sl).all() and (dcn.cpu().numpy() == rows.counts).all(), "the erasure lists were written"


def _host(h, rows, what):
    got = h.decode_batch(rows.data, rows.parity) if rows.slots is None else \
        h.decode_batch(rows.data, rows.parity, rows.slots, rows.counts)
    for name, g, w in zip(("ok", "corrected_num", "data", "parity"), got, rows.want):
        bad = (g != w) if g.ndim == 1 else (g != w).any(1)
        if bad.any():
            c = _first(bad)
            pytest.fail(f"{what}, {_id(rows.code)}: {name} differs at batch row {c}: {rows.describe(c)}: got {g[c]}, "
                        f"oracle {w[c]} ({int(bad.sum())} rows differ)")


def _odd(n):
    return n if n % 2 else n - 1


def _at_least(order, n=R.GW_GROUP_MIN + 65):
    """`order` repeated up to n rows: the grouped form and more than one workgroup"""
    return order if len(order) >= n else np.resize(order, n)


def _batches(torch, h, code, rows, order, what, turn=0):
    """The rows `order` as one batch of 256 rows or more at an odd count (the last wave and
    the last workgroup partial) and, for a code of fewer than 255 symbols, as batches below
    256 rows (GL 64 whatever the code); parity behind the data and apart from it by turns."""
    big = _at_least(order)
    _device(torch, h, rows.take(big), what, count=_odd(len(big)), extra=(5, 0, 9)[turn % 3], off=turn % 4,
            apart=turn % 2 == 1, slot_stride=None if turn % 2 else code[4] + 3)
    if code[0] < 8 or turn == 0:
        for n, start in enumerate(range(0, len(order) if code[0] < 8 else SMALL, SMALL)):
            part = order[start:start + SMALL]
            _device(torch, h, rows.take(part), what + " below 256", count=len(part) if n % 2 else _odd(len(part)),
                    extra=n % 3, off=1, apart=(turn + n) % 2 == 0)


SET = [(code, route) for code in CODES for route in ROUTES]


# ---------------------------------------------------------------------------
# 1. errors only: every family, sorted and shuffled
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code,route", SET, ids=_id)
def test_general_errors(torch_cuda, code, route, monkeypatch):
    """Every row of general_pool at full length, at a shortened size and at size 1 on one
    handle: sorted by family (whole waves of one family), shuffled with two seeds; the host
    batch; single calls on every 29th row."""
    h = _handle(code, route, monkeypatch)
    for size in _sizes(code):
        pc = _case(code, size)
        rows = _errors(pc)
        for turn, (name, order) in enumerate((("sorted_by_tag", R.sorted_by_tag(pc.pool)), ("shuffled", R.shuffled(pc.pool)),
                                              ("shuffled, seed 1", R.shuffled(pc.pool, 1)))):
            _batches(torch_cuda, h, code, rows, order, name, turn)
        _host(h, rows.take(R.shuffled(pc.pool, 2)), "host batch")
        for r in range(0, len(rows), 29):
            got = h.decode(rows.data[r], rows.parity[r])
            assert got[0] == bool(pc.want[0][r]) and got[1] == pc.want[1][r] and (got[2] == pc.want[2][r]).all() and \
                (got[3] == pc.want[3][r]).all(), f"single call, {_id(code)}, size {size}: {rows.describe(r)}"
    h.close()


# ---------------------------------------------------------------------------
# 2. waves and workgroups whose codeword groups are alike, or all but one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code,route", SET, ids=_id)
def test_general_groups(torch_cuda, code, route, monkeypatch):
    """group_layout for the code's GL at 256 rows or more (at the full count and one less: the
    last group of the last wave missing) and, for a code of fewer than 255 symbols, for GL 64 in
    batches below 256 rows that are whole workgroups of four."""
    h = _handle(code, route, monkeypatch)
    for turn, size in enumerate(_sizes(code)):
        pc = _case(code, size)
        rows = _errors(pc)
        gl = _grouped(code)
        order, pieces = R.group_layout(pc.pool, pc.want, gl)
        assert len(order) >= R.GW_GROUP_MIN or gl == 64
        for count in (len(order), len(order) - 1):
            _device(torch_cuda, h, rows.take(order), f"group_layout GL {gl}", count=count, extra=turn, off=turn,
                    apart=(turn + count) % 2 == 0)
        if gl != 64:
            order, pieces = R.group_layout(pc.pool, pc.want, 64)
            for start in range(0, len(order), SMALL):
                _device(torch_cuda, h, rows.take(order[start:start + SMALL]), "group_layout GL 64 below 256", extra=3, off=2,
                        apart=start % 2 == 1)
    h.close()


# ---------------------------------------------------------------------------
# 3. two codewords on one wave
# ---------------------------------------------------------------------------
PAIRED = [c for c in CODES if c[0] == 8 and 8 <= c[4] < 128]


@pytest.mark.parametrize("code,route", [(code, route) for code in PAIRED for route in ROUTES], ids=_id)
def test_general_pairs(torch_cuda, code, route, monkeypatch):
    """pair_layout: more rows than one grid pass, so rows e and e + stride share a wave, with
    the chosen (A, B) at some e and ordinary rows elsewhere; the stride is gw_grid's, from the
    device's CU count.  (POPORON_AMD_GENERIC=lane: the same batch on rsg_decode_k.)"""
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    h = _handle(code, route, monkeypatch)
    for turn, size in enumerate(_sizes(code)):
        pc = _case(code, size)
        order, stride, pairs = R.pair_layout(pc.pool, pc.want, cus)
        assert stride == R.pair_stride(len(order), cus) and len(order) > stride and len(order) % 2 == 1
        assert all(e + stride < len(order) for _, e in pairs) and len(order) <= 20000
        _device(torch_cuda, h, _errors(pc).take(order), f"pair_layout, stride {stride}", extra=(0, 7, 2)[turn], off=turn,
                apart=turn == 1)
    h.close()


# ---------------------------------------------------------------------------
# 4. erasure lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code,route", SET, ids=_id)
def test_general_erasures(torch_cuda, code, route, monkeypatch):
    """Every row of general_errata_pool (counts around GL - 1, GL, 2 GL - 1, 2 GL, nr - 1 and nr,
    repeated slots, slots outside the row, idle slots, count 0) under its list: u8 slots in
    the device batch, rows of slots nr and nr + 3 bytes apart, and in the host batch; u32 slots
    through the erasure object in single calls on every 41st row, the stale slots behind the
    count in the object as in the reference."""
    nr = code[4]
    h = _handle(code, route, monkeypatch)
    er = P.Erasure(nr, nr)
    he = _handle(code, route, monkeypatch, erasure=er)
    for size in _sizes(code):
        pc = _case(code, size)
        rows = _lists(pc)
        for turn, (name, order) in enumerate((("sorted_by_tag", R.sorted_by_tag(pc.epool)), ("shuffled", R.shuffled(pc.epool)))):
            _batches(torch_cuda, h, code, rows, order, "lists, " + name, turn)
        _host(h, rows.take(R.shuffled(pc.epool, 1)), "host batch with lists")
        for r in range(0, len(rows), 41):
            er.set(rows.slots[r].astype(np.uint32))
            er.set(rows.slots[r][:rows.counts[r]].astype(np.uint32))
            got = he.decode(rows.data[r], rows.parity[r])
            w = pc.ewant
            assert got[0] == bool(w[0][r]) and got[1] == w[1][r] and (got[2] == w[2][r]).all() and \
                (got[3] == w[3][r]).all(), f"single call with a list, {_id(code)}, size {size}: {rows.describe(r)}"
    he.close()
    h.close()


# ---------------------------------------------------------------------------
# 5. external syndromes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code,route", SET, ids=_id)
def test_general_external(torch_cuda, code, route, monkeypatch):
    """Each pool row's syndrome vector, log form, straight to decode_batch_syndrome_device: with
    the row it belongs to and with an unrelated clean row (every Berlekamp-Massey branch of the
    pool without a row that has those syndromes), in that order and shuffled."""
    h = _handle(code, route, monkeypatch)
    for turn, size in enumerate(_sizes(code)):
        pc = _case(code, size)
        data, parity, syn, want = _external(code, size)
        n = len(pc.pool)
        rows = Rows(code, data, parity, want,
                    lambda c: f"{'its own row' if c < n else 'a clean row'}, pool row {c % n}, {pc.pool.tags[c % n]!r}, "
                              f"syndromes {syn[c].tolist()}", syn=syn)
        _batches(torch_cuda, h, code, rows, np.arange(len(rows)), "external syndromes", turn)
        _batches(torch_cuda, h, code, rows, np.random.default_rng(size).permutation(len(rows)), "external syndromes, shuffled",
                 turn + 1)
    h.close()


# ---------------------------------------------------------------------------
# 6. one handle across sizes and modes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_general_handle_reuse(torch_cuda, code, monkeypatch):
    """One handle, default route: errors, lists and external syndromes in a row at each size,
    then the sizes backwards in the other order of modes, small and large batches by turns."""
    h = _handle(code, "default", monkeypatch)
    sizes = _sizes(code)
    for lap, seq in enumerate((sizes, sizes[::-1])):
        for size in seq:
            pc = _case(code, size)
            data, parity, syn, want = _external(code, size)
            n = len(pc.pool)
            modes = [("errors", _errors(pc)), ("lists", _lists(pc)),
                     ("external", Rows(code, data, parity, want, lambda c: f"pool row {c % n}, {pc.pool.tags[c % n]!r}", syn=syn))]
            for k, (name, rows) in enumerate(modes[::-1] if lap else modes):
                order = R.shuffled(rows, 3 + lap)
                order = order[:SMALL - 1] if (k + lap) % 2 else _at_least(order)[:R.GW_GROUP_MIN + 65]
                _device(torch_cuda, h, rows.take(order), f"one handle, lap {lap}, {name}", extra=k, off=lap, apart=k == 1)
    h.close()
