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
