"""The rows of tests/rs_syndrome_rows.py on the CPU: the syndrome map round trip, what
each family promises, and the oracle's decode of every family row against the compiled
reference (the GPU tests compare with the oracle alone, on these same rows).
"""
import numpy as np
import pytest

import rs_syndrome_rows as R
from oracle import Oracle, Reference, reference_available
from test_oracle_golden import _assert_rows_equal, _reference_rows

# (symbol_size, field polynomial, fcr, prim, num_roots) -> the family conditions the code is
# excused from (rs_syndrome_rows.family_conditions), with the reason.
#
# No code, the 32-root ones included, meets "every single S_j fails with corrected_num 0"
# (sparse singles, and late_discrepancy with e = 0, which is the same row) as first stated:
# S_j = d alone with j >= t leaves the locator 1 + d' x^(j+1), and where j + 1 divides 255
# (17 for 32 and 31 roots, 15 for 16, 5 for 8) x^(j+1) = 1 / d' has all j + 1 roots for one
# d in j + 1: 15 of the 255 values for j + 1 = 17.  On a full-length row oracle and
# reference then "correct" j + 1 > t symbols and return true.  So the condition every code
# is held to is: a single fails with corrected_num 0, or j + 1 > t divides 255 and it
# succeeds with corrected_num j + 1; sparse() draws all 255 values of d at those j, and
# the full-length pools must show at least 15 such successes.  The other three conditions
# hold for the 32-, 31- and 16-root codes at every size as stated.
CODES = {
    (8, 0x11D, 1, 1, 32): (),  # 15 singles S_16 "corrected" in 17 places at size 223, none at 55 and 1
    (8, 0x11D, 0, 1, 32): (),  # the same
    (8, 0x11D, 5, 7, 32): (),  # the same
    (8, 0x187, 5, 1, 31): (),  # 15 singles S_16 at size 224
    (8, 0x11D, 1, 1, 16): (),  # 17 singles S_14 (and the e = 0, j = 14 row) in 15 places at size 239
    # t = 4: about one syndrome vector in 25 belongs to a locator of degree <= 4 with all its
    # roots, so late_discrepancy rows are now and then "corrected" (at size 247 the row with
    # e = 1, j = 6 is, with corrected_num 6; oracle and reference agree on it)
    (8, 0x11D, 3, 1, 8): ("late_fails",),
}


def _id(code):
    return "m{}-{:#x}-fcr{}-prim{}-nr{}".format(*code)


def _sizes(code):
    k = 255 - code[4]
    return (k, k // 4, 1)


@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_parity_for_round_trip(code):
    """The syndromes of parity_for(S) are S, on 500 random vectors at sizes k, k / 4 and 1,
    on the zero row and on random base messages."""
    o = Oracle(*code)
    nr = code[4]
    for size in _sizes(code):
        sm = R.SyndromeMap(o, size)
        rng = np.random.default_rng([size, nr])
        S = rng.integers(0, 256, (500, nr), dtype=np.uint8)
        S[0] = 0
        par = sm.parity_for(S)
        assert (sm.syndromes(np.zeros((500, size), np.uint8), par) == S).all(), (code, size)
        assert not par[0].any()
        rows, clean = sm.rows_for(rng, S)
        assert not sm.syndromes(clean[:, :size], clean[:, size:]).any()
        assert (sm.syndromes(rows[:, :size], rows[:, size:]) == S).all(), (code, size)


@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_zero_run_syndromes_vanish(code):
    """A zero_run row without its `a` ordinary errors (those bytes taken back from the
    clean row it was built on) has S_0 .. S_(k-1) = 0, and all of its w pattern bytes are
    in error."""
    o = Oracle(*code)
    for size in _sizes(code):
        sm = R.SyndromeMap(o, size)
        data, parity, tags = R.zero_run(sm, draws=1)
        assert len(tags) == sum(min(sm.t, sm.width) - k for k in range(1, sm.t))
        rows, clean = np.concatenate([data, parity], 1), np.array([g.base for g in tags])
        assert not sm.syndromes(clean[:, :size], clean[:, size:]).any()  # codewords
        for c, g in enumerate(tags):
            extra = list(g.positions[g.w:])
            rows[c, extra] = clean[c, extra]
            assert (rows[c, list(g.positions[:g.w])] != clean[c, list(g.positions[:g.w])]).all()
        S = sm.syndromes(rows[:, :size], rows[:, size:])
        for c, g in enumerate(tags):
            assert not S[c, :g.k].any(), (code, size, g, S[c].tolist())
            assert S[c].any()


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built here")
@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_families_oracle_vs_reference(code):
    """Every family row and ordinary rows of 0 .. t + 1 errors: the oracle's decode equals
    the compiled reference's row by row (bool, corrected_num, every byte), and the families
    are what they claim (family_conditions, on the oracle's results alone)."""
    o, r = Oracle(*code), Reference(*code)
    k = 255 - code[4]
    full = R.SyndromeMap(o, k)
    for size in _sizes(code):
        sm = full if size == k else R.SyndromeMap(o, size)
        pool = R.Pool.concat([R.family_pool(sm, full)] + [R.ordinary(sm, e, 8) for e in range(sm.t + 2)])
        want = o.decode_batch(pool.data, pool.parity)
        _assert_rows_equal((code, size), want, _reference_rows(r, pool.data, pool.parity))
        seen = R.family_conditions(pool, want, CODES[code])
        print(f"\n[families] {_id(code)} size {size}: {len(pool)} rows, {seen}")
        assert ("padding_roots" in seen) == (size < k)
        if size == k:  # sparse(): 15 values of the S_j whose j + 1 > t divides 255 are "corrected" past t
            assert seen["sparse"][1] >= 15
    r.close()


def test_layouts():
    """The layouts on a small pool: what each wave holds."""
    o = Oracle()
    sm = R.SyndromeMap(o, 60)
    t = sm.t
    pool = R.Pool.concat([R.late_discrepancy(sm, draws=1)] + [R.ordinary(sm, e, 70) for e in range(t + 2)])
    e_of = np.array([g.params.get("e", -1) if g.family == "ordinary" else -1 for g in pool.tags])
    ub = R.uniform_blocks(pool, t)
    assert ub.size == (t + 2) * R.BM_WORKGROUP
    assert (e_of[ub].reshape(t + 2, R.BM_WORKGROUP) == np.arange(t + 2)[:, None]).all()
    ll = R.lone_lane(pool, t).reshape(-1, R.WAVE)
    assert ll.shape[0] == 24
    fam = pool.families()
    for w, lane in enumerate([0, 31, 32, 63] * 6):
        rest = np.delete(ll[w], lane)
        kind = [(t, 1), (1, t), (1, 0), (0, 1)]
        if w < 16:
            many, one = kind[w // 4]
            assert (e_of[rest] == many).all() and e_of[ll[w, lane]] == one
        elif w < 20:
            assert (fam[rest] == "late_discrepancy").all() and 1 <= e_of[ll[w, lane]] <= t
        else:
            assert (1 <= e_of[rest]).all() and (e_of[rest] <= t).all() and fam[ll[w, lane]] == "late_discrepancy"
    st = R.sorted_by_tag(pool)
    assert sorted(st.tolist()) == list(range(len(pool))) and (np.diff((fam[st] == "ordinary").astype(int)) >= 0).all()
    sh = R.shuffled(pool)
    assert sorted(sh.tolist()) == list(range(len(pool))) and (sh != np.arange(len(pool))).any()
    assert R.odd_counts(1000) == [961, 959] and R.odd_counts(len(pool))[0] % 64 == 1
    assert len(R.pad_to(sh)) == R.SPLIT_MIN_COUNT and (R.pad_to(sh)[:len(sh)] == sh).all()


# ---------------------------------------------------------------------------
# rows with erasure lists
# ---------------------------------------------------------------------------
# (symbol_size, field polynomial, fcr, prim, num_roots) -> the errata conditions the code is
# excused from (rs_syndrome_rows.errata_conditions), with the reason.  None is: every promise
# holds for every code at every size as errata_conditions states it.  Two promises are
# stated there more narrowly than a first reading suggests, for every code alike:
#  - a corrected row equals its clean row only where the list names the damaged positions in
#    the order of the reference's root search, the errors' positions in the stale slots
#    (magnitude n goes to slot n: quirks Q1 - Q3), so errata_zero_run promises the clean row
#    on its even rows and ok with corrected_num == ne + w on all;
#  - errata_degrees names the degrees 15 .. 32 that nr reaches, and nr - 1 and nr: a code of
#    16 or 8 roots has no locator of degree 17.
ERRATA_CODES = {code: () for code in CODES}


def _errata_sizes(code):
    """k, a shortened size that is no multiple of 4, and 1"""
    return (255 - code[4], {32: 101, 31: 61, 16: 150, 8: 37}[code[4]], 1)


def _reference_lists(r, pool, guard=64):
    """poporon_decode of the compiled reference (erasure mode) on every row under its list,
    stale slots included: the whole row of slots is added first and stays in the object
    behind the count.  Each row lies as [data | parity | guard] in one buffer: the
    reference applies a slot p as data[p] whatever p is, so a slot in size .. size + nr - 1
    lands in the parity, as the oracle and the library define it, and one past the codeword
    (up to 255) in the guard, where the oracle drops it.  (ok, corrected_num, data', parity')"""
    import ctypes as C
    fn = r.lib.poporon_decode
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
    n, size = pool.data.shape
    nr = pool.parity.shape[1]
    w = max(size + nr, 256) + guard
    buf = np.zeros((n, w), np.uint8)
    buf[:, :size], buf[:, size:size + nr] = pool.data, pool.parity
    ok, cor = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    num = C.c_size_t(0)
    ref, b0 = C.byref(num), buf.ctypes.data
    for c in range(n):
        r.set_erasures(pool.slots[c])
        r.set_erasures(pool.slots[c, :pool.counts[c]])
        num.value = 0
        ok[c] = fn(r.h, b0 + c * w, size, b0 + c * w + size, ref)
        cor[c] = num.value
    return ok, cor, buf[:, :size].copy(), buf[:, size:size + nr].copy()


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built here")
@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_errata_families_oracle_vs_reference(code):
    """Every row of every errata family at sizes k, a shortened size that is no multiple of
    4, and 1: the oracle's erasure-mode decode equals the compiled reference's row by row
    (bool, corrected_num, every byte) under the same list and stale slots, and the families
    are what they claim (errata_conditions, on the oracle's results alone)."""
    o, r = Oracle(*code), Reference(*code, erasure=True)
    k = 255 - code[4]
    full = R.SyndromeMap(o, k)
    for size in _errata_sizes(code):
        sm = full if size == k else R.SyndromeMap(o, size)
        pool = R.errata_pool(sm, full)
        want = R.decode_lists(o, pool)
        _assert_rows_equal((code, size), want, _reference_lists(r, pool))
        seen = R.errata_conditions(pool, want, sm, ERRATA_CODES[code])
        print(f"\n[errata families] {_id(code)} size {size}: {len(pool)} rows, {seen}")
        assert ("errata_padding" in seen) == (size < k)
        assert set(seen) == set(R.ERRATA_FAMILIES) - (set() if size < k else {"errata_padding"})
    r.close()


@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_errata_zero_run_syndromes_vanish(code):
    """An errata_zero_run row with its erased symbols put back to the clean row's has
    S_0 .. S_(k-1) = 0 and S_k != 0, k > ne, and ne + 2w <= nr."""
    o = Oracle(*code)
    for size in _errata_sizes(code):
        sm = R.SyndromeMap(o, size)
        data, parity, tags, slots, counts = R.errata_zero_run(sm, draws=1)
        rows, clean = np.concatenate([data, parity], 1), np.array([g.base for g in tags])
        assert len(tags) and (counts == [g.ne for g in tags]).all()
        for c, g in enumerate(tags):
            era = list(g.slots[:g.count])
            assert sorted(era) == sorted(g.positions[:g.ne]) and g.ne < g.k < g.w and g.ne + 2 * g.w <= sm.nr
            rows[c, era] = clean[c, era]
        S = sm.syndromes(rows[:, :size], rows[:, size:])
        for c, g in enumerate(tags):
            assert not S[c, :g.k].any() and S[c, g.k], (code, size, g, S[c].tolist())


def test_root_search_order():
    """SyndromeMap.visit against the oracle: the position tried last, and for prim 7 the
    order of a sample of pairs."""
    for code in ((8, 0x11D, 1, 1, 32), (8, 0x11D, 5, 7, 32), (8, 0x11D, 3, 1, 8)):
        o = Oracle(*code)
        for size in (255 - code[4], 37):
            sm = R.SyndromeMap(o, size)
            assert sm.last_visited() == sm.width - 1  # location 254, the point i = 255, whatever prim is
            rng = np.random.default_rng(size)
            for _ in range(40):
                p, q = (int(x) for x in rng.permutation(sm.width)[:2])
                row = np.zeros(sm.width, np.uint8)
                row[p], row[q] = 1, 2
                assert sm._count0(row, [p, q]) == bool(sm.visit(p) < sm.visit(q)), (code, size, p, q)


def test_errata_layouts():
    """The layouts of a pool with lists: what each wave holds."""
    o = Oracle()
    sm = R.SyndromeMap(o, 101)
    nr, W = sm.nr, sm.width
    pool = R.errata_pool(sm, R.SyndromeMap(o, 223))
    want = R.decode_lists(o, pool)
    cnt, fam = pool.counts.astype(int), pool.families()
    asc = np.array([R._ascending(t, W) for t in pool.tags])
    un = R.uniform_ne(pool, want)
    waves = un[:(nr + 1) * R.WAVE].reshape(nr + 1, R.WAVE)
    assert (cnt[waves] == np.arange(nr + 1)[:, None]).all() and not asc[waves[nr]].any()
    groups = un[(nr + 1) * R.WAVE:].reshape(-1, R.EBM_WORKGROUP)
    assert [int(cnt[g][0]) for g in groups] == [0, 1, 16, 28, 29, 31, 32]
    assert all((cnt[g] == cnt[g][0]).all() for g in groups)
    assert not asc[groups[-1]].any()
    ll = R.lone_ne(pool, want).reshape(-1, R.WAVE)
    assert ll.shape[0] == 32
    for w, lane in enumerate(R.LANES * 4):
        many, one = ((nr, 0), (0, nr), (nr - 3, 3), (3, nr - 3))[w // 4]
        assert (cnt[np.delete(ll[w], lane)] == many).all() and cnt[ll[w, lane]] == one
    dirty = (np.concatenate([pool.data, pool.parity], 1) != pool.clean).any(1)
    for w, lane in enumerate(R.LANES * 2):
        rest, one = np.delete(ll[16 + w], lane), ll[16 + w, lane]
        assert (dirty[rest] != (w < 4)).all() and dirty[one] == (w < 4)
    for w, lane in enumerate(R.LANES * 2):
        rest, one = np.delete(ll[24 + w], lane), ll[24 + w, lane]
        assert ((fam[rest] == "errata_outside") == (w < 4)).all() and (fam[one] == "errata_outside") == (w >= 4)
    # the final degree, from the oracle alone: the nonzero magnitudes of a success and the idle erased
    # symbols, on rows within the code's reach (beyond it a success is a miscorrection)
    reach = np.array([t.family in ("errata_grid", "errata_degrees") and t.ne + 2 * t.e <= nr for t in pool.tags])
    deg = np.where(reach & (want[0] == 1) & dirty, want[1].astype(np.int64) + [len(t.idle) for t in pool.tags], -1)
    assert (deg == R._kinds(pool, want)["degree"]).all()
    db = R.degree_brackets(pool, want).reshape(-1, R.WAVE)
    assert db.shape[0] == 3 + 16
    for w, (lo, hi) in enumerate(((1, 16), (17, 24), (25, 32))):
        assert (deg[db[w]] >= lo).all() and (deg[db[w]] <= hi).all() and want[0][db[w]].all()
    assert {1, 16} <= set(deg[db[0]]) and {17, 24} <= set(deg[db[1]]) and {25, 32} <= set(deg[db[2]])
    for w, (D, lane) in enumerate((D, lane) for D in (17, 24, 25, 32) for lane in R.LANES):
        assert deg[db[3 + w, lane]] == D and (deg[np.delete(db[3 + w], lane)] <= 16).all()
        assert (deg[db[3 + w]] >= 1).all()
    bp = R.bp_mixes(pool, want)
    solved = (cnt == nr) & asc & dirty
    assert solved[bp["solved"]].all() and len(bp["solved"]) == 4 * R.WAVE
    assert solved[bp["pending_last"][:-1]].all() and not solved[bp["pending_last"][-1]] and dirty[bp["pending_last"][-1]]
    assert (~solved[bp["one_clean"]]).sum() == 1 and (~dirty[bp["one_clean"]]).sum() == 1
    assert solved[bp["mix"][0::2]].all() and not solved[bp["mix"][1::2]].any() and dirty[bp["mix"]].all()
