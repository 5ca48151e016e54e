"""The Reed-Solomon errata decode kernels on rows with chosen erasure lists and on batches
whose waves are alike.

rs_ebm_k, rs_chien32_k and rs_forney32_k (rs_errata.hip), rs_era_bp_k with its pending flag
and its list (rs_fast.hip), and the rsk_ebm_nr / rsk_forney32_nr forms of the codes with
fewer than 32 roots take wave-wide shortcuts that a batch of independently drawn rows never
leaves: the trip count of the erasure-locator loop (the wave's largest count), the first
Berlekamp-Massey block (its smallest), the coefficient groups per step, the widths 16 / 24 /
32 of the root search and 8 / 12 / 16 of the magnitude sums (the wave's largest degree), a
degree of 32 carried as 0 in five bits, and "nothing pending in this batch", on which all
three errata kernels return at once and leave the handle's last records in the workspace.

tests/rs_syndrome_rows.py builds the rows (errata_* families) and the layouts (uniform_ne,
lone_ne, degree_brackets, bp_mixes) from the CPU oracle alone;
tests/test_rs_syndrome_rows_cpu.py compares the oracle with the compiled reference on the
same rows.  Here the library decodes them on every route and in every form of the rows of
slots, and ok, corrected_num and every byte must equal the oracle's; the guard bytes around
the rows and the flags stay as they were.  No row is left out and nothing is approximate.

The rows of slots are u8 throughout: no batch entry point of the library takes u32 slots.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import libpoporon_amd as P
import rs_syndrome_rows as R
from oracle import Oracle
from test_gpu_rs_chosen_syndromes import CODES as ERROR_CODES
from test_gpu_rs_chosen_syndromes import DEFAULT, ROUTES, THREADS, _device, _handle, _host, _id, _k, _short

pytestmark = pytest.mark.gpu

# (symbol_size, field polynomial, fcr, prim, num_roots) -> the errata conditions the code is
# excused from: none (tests/test_rs_syndrome_rows_cpu.py says how the promises are stated)
CODES = {code: () for code in ERROR_CODES}
PATHS = ("default", "split", "single", "wave")  # the tail settings do not reach the errata routes (api.cpp: launch_errata)
# rows of slots: 32 bytes apart (16-byte rows: rs_era_bp_k first), 40 (the errata kernels alone), 33 (the record kernel)
STRIDES = (32, 40, 33)
WATCHED = (P.KERNEL_ERASURE, P.KERNEL_BM, P.KERNEL_CHIEN, P.KERNEL_FORNEY, P.KERNEL_LIST, P.KERNEL_APPLY,
           P.KERNEL_CORRECT, P.KERNEL_WAVE)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _kernels(code, route, stride, count):
    """decode_route of api.cpp restated for a device batch with u8 slots in 4-byte aligned
    rows `stride` apart: the launches (in WATCHED's order) that the library's kernel timers
    must show.  The list kernel is launched on every errata route, list rows or not."""
    fcr, prim, nr = code[2:]
    path = ROUTES[route].get("POPORON_AMD_DECODE_PATH")
    vfast = (fcr + nr - 1) * prim * 254 < 32768
    rows4 = stride % 4 == 0 and stride >= nr
    errata = {True: (1, 1, 1, 1, 1, 1, 0, 0), False: (0, 1, 1, 1, 1, 1, 0, 0)}
    correct, wave = (0, 0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 0, 0, 1)
    assert count > 1
    if nr < 32:  # rsk_ebm_nr and rsk_forney32_nr at every batch size, else the general kernel
        return errata[False] if rows4 and vfast and path in (None, "split") else correct
    if path == "wave" or (path is None and count < R.SPLIT_MIN_COUNT):
        return wave
    if not vfast or path == "single":
        return correct
    if prim == 1 and stride % 16 == 0:
        return errata[True]
    return errata[False] if rows4 else (0, 0, 0, 0, 0, 1, 1, 0)


def _launches(h, fn):
    h.timing(True)
    fn()
    n = tuple(h.timing_read(k)[1] for k in WATCHED)
    h.timing(False)
    return n


def _pads(code, route):
    """a 32-root batch takes the errata kernels on the default route from SPLIT_MIN_COUNT rows on"""
    return code[4] == 32 and "POPORON_AMD_DECODE_PATH" not in ROUTES[route]


# ---------------------------------------------------------------------------
# the pools and the oracle's results, built once for each (code, size)
# ---------------------------------------------------------------------------
_CACHE = {}


def _pool(code, size):
    """Every errata family, the oracle's decode of each row under its list (once: the layouts
    index it), and the conditions on the oracle alone; read-only."""
    if (code, size) in _CACHE:
        return _CACHE[(code, size)]
    o = Oracle(*code)
    k = _k(code)
    if ("map", code) not in _CACHE:
        _CACHE[("map", code)] = R.SyndromeMap(o, k)
    full = _CACHE[("map", code)]
    sm = full if size == k else R.SyndromeMap(o, size)
    pool = R.errata_pool(sm, full)
    want = R.decode_lists(o, pool, threads=THREADS)
    seen = R.errata_conditions(pool, want, sm, CODES[code])
    assert set(seen) == set(R.ERRATA_FAMILIES) - (set() if size < k else {"errata_padding"})
    syn = o.syndrome_batch(pool.data, pool.parity)[1]
    for a in (pool.data, pool.parity, pool.slots, pool.counts, syn) + tuple(want):
        a.setflags(write=False)
    pc = SimpleNamespace(code=code, size=size, pool=pool, syn=syn, want=want, o=o,
                         lists=[f"{t.slots[:t.count]} + stale {t.slots[t.count:]}" for t in pool.tags])
    _CACHE[(code, size)] = pc
    return pc


def _run(torch, h, pc, order, stride, route, what, count=None, extra=5, off=3, kernels=True):
    """One device batch of the pool's rows `order` under their lists, rows of slots `stride`
    apart with junk between them; with the launches that the route must show."""
    count = len(order) if count is None else count
    got = _launches(h, lambda: _device(torch, h, pc, order, count=count, extra=extra, off=off,
                                       slots=pc.pool.slots[order], counts=pc.pool.counts[order], slot_stride=stride,
                                       what=f"{what}, slots {stride} apart, count {count}"))
    if kernels:
        assert got == _kernels(pc.code, route, stride, count), (what, pc.code, pc.size, route, stride, count, got)


# ---------------------------------------------------------------------------
# 1. every family, grouped and shuffled, on every route and in every form of the slot rows
# ---------------------------------------------------------------------------
SIZED = [(code, size) for code in CODES for size in (_k(code), _short(code), 1)]


@pytest.mark.parametrize("route", PATHS)
@pytest.mark.parametrize("code,size", SIZED, ids=_id)
def test_errata_families(torch_cuda, code, size, route, monkeypatch):
    """All errata families in the sorted_by_tag layout (whole waves of one family) and the
    shuffled one: the device batch at each stride of the slot rows, between guard bytes, and
    the host batch.  The 31-root code reads a 32nd byte with each row of slots: every batch
    runs twice with different junk there and must give the oracle's rows both times.  On the
    default route a 32-root batch is repeated up to SPLIT_MIN_COUNT rows."""
    pc = _pool(code, size)
    h = _handle(code, route, monkeypatch)
    for name, order in (("sorted_by_tag", R.sorted_by_tag(pc.pool)), ("shuffled", R.shuffled(pc.pool))):
        if _pads(code, route):
            order = R.pad_to(order)
        for stride in STRIDES:
            _run(torch_cuda, h, pc, order, stride, route, name)
            if code[4] == 31:  # (_device seeds its junk by the rows' stride)
                _run(torch_cuda, h, pc, order, stride, route, name + ", other junk", extra=6)
    order = R.shuffled(pc.pool, seed=1)
    _host(h, pc, order, what="host batch", slots=pc.pool.slots[order], counts=pc.pool.counts[order])
    h.close()


# ---------------------------------------------------------------------------
# 2. waves whose rows are alike
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", PATHS)
@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_errata_wave_composition(torch_cuda, code, route, monkeypatch):
    """uniform_ne (a wave of each count, workgroups of some: the bounds nemax and nemin at both
    ends, no Berlekamp-Massey block at all for nr unsorted slots), lone_ne (one row of
    another count, a clean row, a list row at lane 0, 31, 32, 63), degree_brackets (the
    widths of rs_chien32_k and rs_forney32_k at 16 | 17 and 24 | 25, degree 32 alone among
    low degrees) and bp_mixes, at the full count and at counts 64 q + 1 and 64 q + 63, in
    the wire layout at size k and on padded strides at the shortened size and at size 1.  The
    31-root code runs each batch twice, with other junk in the 32nd byte of its slot rows."""
    for size, extra, off in ((_k(code), 0, 0), (_short(code), 9, 1), (1, 4, 2)):
        pc = _pool(code, size)
        h = _handle(code, route, monkeypatch)
        order = np.concatenate([R.uniform_ne(pc.pool, pc.want), R.lone_ne(pc.pool, pc.want),
                                R.degree_brackets(pc.pool, pc.want)] + list(R.bp_mixes(pc.pool, pc.want).values()))
        assert len(order) % R.WAVE == 0
        if _pads(code, route):
            order = R.pad_to(order, R.SPLIT_MIN_COUNT + R.WAVE)
        c1, c63 = R.odd_counts(len(order))
        assert c1 % 64 == 1 and c63 % 64 == 63 and (not _pads(code, route) or c63 >= R.SPLIT_MIN_COUNT)
        for count in (len(order), c1, c63):
            for stride in STRIDES[:2] if count == len(order) else (32 if count == c1 else 40,):
                _run(torch_cuda, h, pc, order, stride, route, "waves", count=count, extra=extra, off=off)
                if code[4] == 31:  # the 32nd byte of each row of slots: other junk, the same rows
                    _run(torch_cuda, h, pc, order, stride, route, "waves, other junk", count=count, extra=extra + 1,
                         off=off)
        sel = order[:c63 if extra == 0 else c1]
        _host(h, pc, sel, what="host batch", slots=pc.pool.slots[sel], counts=pc.pool.counts[sel])
        h.close()


# ---------------------------------------------------------------------------
# 3. what one batch leaves in the handle's workspace for the next
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["k", "short"])
@pytest.mark.parametrize("code", [DEFAULT, (8, 0x11D, 0, 1, 32)], ids=_id)
def test_errata_state_between_batches(torch_cuda, code, size, monkeypatch):
    """On one handle (DECODE_PATH=split, slot rows 32 bytes apart: rs_era_bp_k first): a
    batch of pending and list rows, then batches in which rs_era_bp_k leaves nothing pending
    (nr sorted slots throughout; the same with one clean row) and the three errata kernels
    return at once, over the meta, ext and roots that the first batch left, then the first
    batch again; on a second handle the other way round.  The batches have the same number
    of rows, so every row of one meets the records of the other."""
    size = _k(code) if size == "k" else _short(code)
    pc = _pool(code, size)
    mixes = R.bp_mixes(pc.pool, pc.want)
    first = R.sorted_by_tag(pc.pool)
    first = first[:len(first) // R.WAVE * R.WAVE - 1]
    quiet = [np.resize(mixes[name], len(first)) for name in ("solved", "one_clean")]
    for turn in ([first] + quiet + [first, mixes["pending_last"], first], quiet + [first] + quiet):
        h = _handle(code, "split", monkeypatch)
        for n, order in enumerate(turn):
            _run(torch_cuda, h, pc, order, 32, "split", f"batch {n} on one handle", extra=0, off=0)
        h.close()
