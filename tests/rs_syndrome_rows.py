"""Reed-Solomon rows built from chosen syndromes, and batch layouts with chosen waves.

A helper module of the tests (not a conftest, no fixtures).  No expected value comes
from field arithmetic of its own: everything comes from the CPU oracle
(oracle/rs_oracle.c) and from linear algebra over GF(2) on what the oracle answers.
The one exception is bm_trace, a Berlekamp-Massey replay on the oracle's tables that
only tags rows (which iteration the general kernels' narrow run stops at, the final L)
and is itself checked against the oracle (trace_conditions).

Symbols have m <= 8 bits, one per byte, nn = 2^m - 1 (m = 8, nn = 255 for the split and
errata suites).  The map from the nr parity symbols of a row to its nr syndrome values
is GF(2)-linear on the low m bits of each symbol, and invertible whenever the code's
roots are distinct.  SyndromeMap reads its m nr x m nr bit matrix off the oracle's
syndromes of the m nr one-bit parity perturbations of the all-zero row, inverts it, and
so turns any wanted syndrome vector S into the row [base | encode(base) ^ parity_for(S)].
The same idea on a set of symbol positions gives error patterns whose first k
syndromes vanish (SyndromeMap.vanishing).  Base messages are raw bytes: the codec masks
them to m bits.

The families below are rows that random error patterns produce once in 256
steps of Berlekamp-Massey or never: runs of zero discrepancies, a late jump of
L, locators that would pass x^t, sparse syndromes, roots in the padding of a
shortened row, every error position.  The layouts order a pool of rows so that
whole waves of 64 rows (and whole workgroups of 512) are alike, or differ in
one lane.  Everything is seeded; every row stands on a random base message.

The errata_* families further down are rows with erasure lists (a row of nr slot bytes,
a count, stale bytes after it) for the errata kernels, with their own conditions
(errata_conditions) and layouts (uniform_ne, lone_ne, degree_brackets, bp_mixes).

The last section serves the general kernels (rs_generic.hip), which run a codeword on
GL = 4 .. 64 lanes: the handoff family, general_pool / general_errata_pool (the
families above thinned for long codes), group_layout and pair_layout.
"""
import numpy as np

WAVE = 64
BM_WORKGROUP = 512  # rows of one rs_bm_k workgroup
SPLIT_MIN_COUNT = 16384  # api.cpp: a 32-root batch takes the split kernels by default from here on


# ---------------------------------------------------------------------------
# GF(2) linear algebra on uint8 0 / 1 matrices
# ---------------------------------------------------------------------------
def _reduce(a, ncols):
    """Row-reduce `a` (in place) on its first ncols columns; returns the pivot rows' count."""
    r = 0
    for c in range(ncols):
        hit = np.nonzero(a[r:, c])[0]
        if hit.size == 0:
            continue
        p = r + int(hit[0])
        if p != r:
            a[[r, p]] = a[[p, r]]
        rows = np.nonzero(a[:, c])[0]
        rows = rows[rows != r]
        a[rows] ^= a[r]
        r += 1
        if r == a.shape[0]:
            break
    return r


def gf2_inverse(m):
    """Inverse of a square 0 / 1 matrix over GF(2); ValueError if it is singular."""
    n = m.shape[0]
    a = np.concatenate([m.astype(np.uint8) & 1, np.eye(n, dtype=np.uint8)], 1)
    if _reduce(a, n) != n:
        raise ValueError("singular over GF(2)")
    return np.ascontiguousarray(a[:, n:])


def gf2_left_null_space(m):
    """Basis (rows) of {x : x m = 0} over GF(2)."""
    n, k = m.shape
    a = np.concatenate([m.astype(np.uint8) & 1, np.eye(n, dtype=np.uint8)], 1)
    rank = _reduce(a, k)
    assert not a[rank:, :k].any()
    return np.ascontiguousarray(a[rank:, k:])


def _bits(b, m=8):
    """(count, n) symbols -> (count, m n) bits: the low m bits of each, the highest first"""
    b = np.ascontiguousarray(b, dtype=np.uint8)
    x = np.unpackbits(b, axis=1)
    return x if m == 8 else np.ascontiguousarray(x.reshape(len(b), -1, 8)[:, :, 8 - m:]).reshape(len(b), -1)


def _bytes(x, m=8):
    """(count, m n) bits -> (count, n) symbols of m bits"""
    x = x.astype(np.uint8)
    if m == 8:
        return np.packbits(x, axis=1)
    sym = np.zeros((len(x), x.shape[1] // m, 8), np.uint8)
    sym[:, :, 8 - m:] = x.reshape(len(x), -1, m)
    return np.packbits(sym.reshape(len(x), -1), axis=1)


def _mul(x, m):
    """x m over GF(2), x (count, a) and m (a, b) of 0 / 1"""
    return (x.astype(np.float32) @ m.astype(np.float32)).astype(np.int64) & 1


# ---------------------------------------------------------------------------
# rows and their tags
# ---------------------------------------------------------------------------
class Tag:
    """How a row was built: its family and the parameters of its construction.
    positions: the byte positions of the errors put into the row (None where
    the row was built from syndromes alone).  base: the clean row
    [base | encode(base)] that the row was built on (set by the family).
    Rows with an erasure list: slots, the nr bytes of the row of slots (the list and the
    stale bytes after it); count, how many of them count; idle, the counted slots whose
    symbol is correct (the clean row's)."""
    __slots__ = ("family", "params", "positions", "base", "slots", "count", "idle")

    def __init__(self, family, positions=None, **params):
        self.family, self.params, self.positions, self.base = family, params, positions, None
        self.slots, self.count, self.idle = None, 0, ()  # the errata families: see _Listed.add

    def __getattr__(self, name):
        try:
            return self.params[name]
        except KeyError:
            raise AttributeError(name) from None

    def __repr__(self):
        return self.family + "(" + ", ".join(f"{k}={v}" for k, v in self.params.items()) + ")"


class Pool:
    """Rows of one (code, size): data (count, size), parity (count, nr), a Tag each;
    clean (count, size + nr): the codewords [base | encode(base)] the rows were built on;
    slots (count, nr) uint8 and counts (count,) uint8: the rows' erasure lists, stale bytes
    after the count filled in (all zero for rows that have no list)."""

    def __init__(self, data, parity, tags, slots=None, counts=None):
        assert len(data) == len(parity) == len(tags)
        self.data, self.parity, self.tags = data, parity, list(tags)
        self.slots = np.zeros(parity.shape, np.uint8) if slots is None else np.ascontiguousarray(slots, np.uint8)
        self.counts = np.zeros(len(tags), np.uint8) if counts is None else np.ascontiguousarray(counts, np.uint8)
        assert self.slots.shape == parity.shape and self.counts.shape == (len(tags),)
        self.clean = np.array([t.base for t in self.tags], np.uint8).reshape(len(self.tags), -1)
        assert self.clean.shape == (len(self.tags), data.shape[1] + parity.shape[1])

    def __len__(self):
        return len(self.tags)

    @staticmethod
    def concat(parts):
        parts = [p if isinstance(p, Pool) else Pool(*p) for p in parts]
        return Pool(np.concatenate([p.data for p in parts]), np.concatenate([p.parity for p in parts]),
                    [t for p in parts for t in p.tags], np.concatenate([p.slots for p in parts]),
                    np.concatenate([p.counts for p in parts]))

    def families(self):
        return np.array([t.family for t in self.tags])

    def where(self, pred):
        return np.array([i for i, t in enumerate(self.tags) if pred(t)], dtype=np.int64)


class SyndromeMap:
    """parity bytes <-> syndrome values of one code at one message size."""

    def __init__(self, oracle, size):
        self.o, self.size, self.nr = oracle, size, oracle.nroots
        self.m, self.nn = oracle.m, oracle.nn  # bits per symbol, 2^m - 1
        assert 2 <= self.m <= 8, "symbols of at most a byte"
        self.t = self.nr // 2
        self.width = size + self.nr
        self.pad = oracle.nn - self.nr - size  # the zero symbols a shortened row stands for
        self.alog = oracle.tables()[0]
        nb = self.m * self.nr
        par = _bytes(np.eye(nb, dtype=np.uint8), self.m)  # the m nr one-bit parity perturbations
        self.matrix = _bits(self.syndromes(np.zeros((nb, size), np.uint8), par), self.m)  # parity bits -> syndrome bits
        self.inverse = gf2_inverse(self.matrix)

    # -- syndromes as values (the oracle gives logs) --
    def syndromes(self, data, parity):
        """(count, nr) syndrome values of the rows"""
        _, syn = self.o.syndrome_batch(data, parity)
        return self.alog[syn].astype(np.uint8)

    def parity_for(self, S):
        """(count, nr) parity deltas whose syndromes (on zero data) are the value vectors S"""
        S = np.atleast_2d(np.asarray(S, dtype=np.uint8))
        return _bytes(_mul(_bits(S, self.m), self.inverse), self.m)

    def vanishing(self, positions, k):
        """Basis of the GF(2) null space of "values at these byte positions -> S_0 .. S_(k-1)":
        (m (w - k), m w) bits, w = len(positions); symbol i of a member goes to positions[i]."""
        w, m = len(positions), self.m
        unit = _bytes(np.eye(m * w, dtype=np.uint8), m)
        rows = np.zeros((m * w, self.width), np.uint8)
        for i, p in enumerate(positions):
            rows[:, p] = unit[:, i]
        syn = self.syndromes(rows[:, :self.size], rows[:, self.size:])
        basis = gf2_left_null_space(_bits(syn[:, :k], m))
        assert basis.shape == (m * max(w - k, 0), m * w), (basis.shape, w, k)
        return basis

    def vanishing_pattern(self, rng, positions, k):
        """A random null-space member with every byte nonzero: an error pattern of weight w
        whose first k syndromes are zero (w >= k + 1)."""
        basis = self.vanishing(positions, k)
        for _ in range(1000):
            v = _bytes(_mul(rng.integers(0, 2, (1, basis.shape[0])), basis), self.m)[0]
            if v.all():
                return v
        raise AssertionError("no full-weight pattern found")

    # -- rows --
    def base_rows(self, rng, n):
        data = rng.integers(0, 256, (n, self.size), dtype=np.uint8)  # raw bytes: the codec masks to m bits
        return np.concatenate([data, self.o.encode_batch(data)], 1)

    def _split(self, rows, tags, clean):
        """(data, parity, tags) of a family; every tag keeps its clean row"""
        assert clean.shape == rows.shape and len(tags) == len(rows)
        for c, g in enumerate(tags):
            g.base = clean[c]
        return np.ascontiguousarray(rows[:, :self.size]), np.ascontiguousarray(rows[:, self.size:]), tags

    def rows_for(self, rng, S):
        """rows [base | encode(base) ^ parity_for(S)] on random base messages, and the clean rows"""
        clean = self.base_rows(rng, len(S))
        rows = clean.copy()
        rows[:, self.size:] ^= self.parity_for(S)
        return rows, clean

    def _scatter(self, rng, rows, c, e, avoid=()):
        """e random nonzero values at random positions of row c outside `avoid`"""
        free = np.setdiff1d(np.arange(self.width), np.asarray(avoid, dtype=np.int64))
        pos = rng.permutation(free)[:e]
        rows[c, pos] ^= rng.integers(1, self.nn + 1, pos.size, dtype=np.uint8)
        return tuple(int(p) for p in pos)

    # -- the order of the reference's root search --
    def visit(self, pos):
        """When the reference's root search meets byte position pos of the row: it tries
        the points i = 1 .. nn in turn, and point i stands for location (i iprim - 1) mod
        nn, so location k = pos + pad is met at i = (k + 1) prim mod nn (0 read as nn; nn = 255
        for byte symbols).  Returned as i - 1, 0 .. nn - 1.  Integer arithmetic on exponents, no field arithmetic;
        last_visited() and every family row that promises its clean row back check it
        against the oracle.  Magnitude n, in this order, goes to list slot n: a list
        restores the row only when it names the damaged positions in this order."""
        return ((np.asarray(pos, dtype=np.int64) + self.pad + 1) * self.o.prim - 1) % self.o.nn

    def in_root_order(self, listed):
        return bool((np.diff(self.visit(listed)) > 0).all())

    def by_visit(self, pos):
        pos = np.asarray(pos, dtype=np.int64)
        return pos[np.argsort(self.visit(pos), kind="stable")]

    def last_visited(self):
        """The position whose root the reference tries last (its point i = nn), found from
        the oracle by trying each: on the zero codeword with two unlike errors at p and q,
        the erasure mode with count 0 hands magnitude 0 to slot 0 and magnitude 1 to slot 1
        (quirk Q3), so the list [q, p] restores the row exactly when q is met before p."""
        assert self.t >= 2
        zero = np.zeros(self.size, np.uint8)
        par = self.o.encode(zero)
        assert not par.any()
        best = 0
        for p in range(1, self.width):
            row = np.zeros(self.width, np.uint8)
            row[best], row[p] = 1, 2
            if self._count0(row, [best, p]):  # best is met before p
                best = p
        assert best == int(np.argmax(self.visit(np.arange(self.width)))), "visit() disagrees with the oracle"
        return best

    def _count0(self, row, first):
        sl = np.zeros((1, self.nr), np.uint32)
        sl[0, :len(first)] = first
        ok, n, d, p = self.o.decode_batch(row[None, :self.size], row[None, self.size:], sl, np.zeros(1, np.uint32))
        assert ok[0] == 1 and n[0] == 2
        return not d.any() and not p.any()


def _rng(sm, seed, family):
    o = sm.o
    return np.random.default_rng([seed, o.nroots, o.fcr, o.prim, sm.size, sum(family.encode())])


# ---------------------------------------------------------------------------
# families: (data, parity, tags)
# ---------------------------------------------------------------------------
def ordinary(sm, e, n, seed=0):
    """n rows with exactly e random errors (at most the row's width)"""
    rng = _rng(sm, seed + 1000 * e, "ordinary")
    clean = sm.base_rows(rng, n)
    rows = clean.copy()
    e_row = min(e, sm.width)
    pos = rng.permuted(np.tile(np.arange(sm.width), (n, 1)), axis=1)[:, :e_row]
    val = rng.integers(1, sm.nn + 1, (n, e_row), dtype=np.uint8)
    np.put_along_axis(rows, pos, np.take_along_axis(rows, pos, 1) ^ val, 1)
    return sm._split(rows, [Tag("ordinary", tuple(int(p) for p in pos[c]), e=e) for c in range(n)], clean)


def zero_run(sm, draws=1, seed=0, ks=None):
    """For every k in 1 .. t-1 (or in `ks`: long codes) and w in k+1 .. t: a vanishing pattern
    of weight w and a
    ordinary errors elsewhere, a <= min(t - w, k // 2).  Correctable; Berlekamp-Massey
    sees k - 2a zero discrepancies in a row and then lengthens by more than one."""
    rng = _rng(sm, seed, "zero_run")
    t = sm.t
    combos = [(k, w) for k in range(1, t) for w in range(k + 1, t + 1) if w <= sm.width]
    if ks is not None:  # (w: the least, the greatest and one between)
        combos = [(k, w) for k, w in combos if k in ks and w in (k + 1, (k + 1 + t) // 2, t)]
    combos = combos * draws
    clean = sm.base_rows(rng, len(combos))
    rows = clean.copy()
    tags = []
    for c, (k, w) in enumerate(combos):
        a = int(rng.integers(0, min(t - w, k // 2, sm.width - w) + 1))
        pos = rng.permutation(sm.width)[:w]
        rows[c, pos] ^= sm.vanishing_pattern(rng, pos, k)
        extra = sm._scatter(rng, rows, c, a, avoid=pos)
        tags.append(Tag("zero_run", tuple(int(p) for p in pos) + extra, k=k, w=w, a=a))
    return sm._split(rows, tags, clean)


def late_discrepancy(sm, draws=3, seed=0, es=None, js=None):
    """e ordinary errors, e in 0 .. t (or in `es`), then a nonzero value XORed into one syndrome
    S_j, for every j (or those in `js`): L jumps to j + 1 - e late, with B shifted many times."""
    rng = _rng(sm, seed, "late_discrepancy")
    t, nr = sm.t, sm.nr
    combos = [(e, j) for e in (range(t + 1) if es is None else es) for j in (range(nr) if js is None else js)] * draws
    n = len(combos)
    clean = sm.base_rows(rng, n)
    rows = clean.copy()
    S = np.zeros((n, nr), np.uint8)
    tags = []
    for c, (e, j) in enumerate(combos):
        pos = sm._scatter(rng, rows, c, min(e, sm.width))
        S[c, j] = rng.integers(1, sm.nn + 1)
        tags.append(Tag("late_discrepancy", pos, e=e, j=j))
    rows[:, sm.size:] ^= sm.parity_for(S)
    return sm._split(rows, tags, clean)


def sparse(sm, values=4, pairs=48, seed=0, js=None):
    """Exactly one nonzero syndrome S_j for every j (`values` values each), and exactly
    two for a seeded set of pairs.  A single S_j = d with j >= t leaves the locator
    1 + d' x^(j+1): j = t - 1 gives 1 + d' x^t, and where j + 1 divides 255 (17 for 32
    roots, 15 for 16, 5 for 8) the locator has j + 1 > t roots for one d in j + 1; the
    reference then "corrects" j + 1 symbols of a full-length row.  Those j get every d.
    (255: nn = 2^m - 1 for symbols of m bits.  js: the singles' j, for long codes.)"""
    rng = _rng(sm, seed, "sparse")
    nr = sm.nr
    S, tags = [], []
    for j in (range(nr) if js is None else js):
        every = j + 1 > sm.t and sm.nn % (j + 1) == 0
        for v in rng.permutation(np.arange(1, sm.nn + 1))[:sm.nn if every else values]:
            s = np.zeros(nr, np.uint8)
            s[j] = v
            S.append(s)
            tags.append(Tag("sparse", None, j=j))
    for _ in range(pairs):
        i, j = sorted(int(x) for x in rng.permutation(nr)[:2])
        s = np.zeros(nr, np.uint8)
        s[i], s[j] = rng.integers(1, sm.nn + 1, 2)
        S.append(s)
        tags.append(Tag("sparse", None, i=i, j=j))
    rows, clean = sm.rows_for(rng, np.array(S))
    return sm._split(rows, tags, clean)


def padding_roots(sm, full, seed=0, es=None):
    """Shortened sizes: the syndromes of e errors, e in 1 .. t, on the full-length code
    (`full`: the SyndromeMap of size k), 1 .. e of them inside the padding, transplanted
    onto the short row.  The locator is valid and all its roots are found, but a location
    lies before the row."""
    rng = _rng(sm, seed, "padding_roots")
    pad = full.size - sm.size
    assert pad > 0 and full.nr == sm.nr
    combos = [(e, p) for e in range(1, sm.t + 1) for p in range(1, e + 1) if p <= pad and e - p <= sm.width]
    if es is not None:  # long codes: these e, with one, half and all of the errors inside the padding
        combos = [(e, p) for e, p in combos if e in es and p in (1, (e + 1) // 2, min(e, pad))]
    err = np.zeros((len(combos), full.width), np.uint8)
    tags = []
    for c, (e, p) in enumerate(combos):
        pos = np.concatenate([rng.permutation(pad)[:p], pad + rng.permutation(sm.width)[:e - p]])
        err[c, pos] = rng.integers(1, sm.nn + 1, e, dtype=np.uint8)
        tags.append(Tag("padding_roots", None, e=e, inside=p))
    S = full.syndromes(err[:, :full.size], err[:, full.size:])
    rows, clean = sm.rows_for(rng, S)
    return sm._split(rows, tags, clean)


def positions(sm, seed=0):
    """One error at each position of the row; t errors on consecutive positions for every start."""
    rng = _rng(sm, seed, "positions")
    W, t = sm.width, min(sm.t, sm.width)
    clean = sm.base_rows(rng, W + (W - t + 1))
    rows = clean.copy()
    tags = []
    for p in range(W):
        rows[p, p] ^= rng.integers(1, sm.nn + 1)
        tags.append(Tag("positions", (p,), at=p, run=1))
    for s in range(W - t + 1):
        rows[W + s, s:s + t] ^= rng.integers(1, sm.nn + 1, t, dtype=np.uint8)
        tags.append(Tag("positions", tuple(range(s, s + t)), at=s, run=t))
    return sm._split(rows, tags, clean)


def family_pool(sm, full=None, zero_run_draws=1, late_draws=3, seed=0):
    """Every family of (code, size) in one pool; padding_roots where `full` is given."""
    parts = [zero_run(sm, zero_run_draws, seed), late_discrepancy(sm, late_draws, seed), sparse(sm, seed=seed),
             positions(sm, seed)]
    if full is not None and full.size > sm.size:
        parts.append(padding_roots(sm, full, seed))
    return Pool.concat(parts)


# ---------------------------------------------------------------------------
# conditions on the oracle's results alone: no family may quietly become trivial
# ---------------------------------------------------------------------------
def _all_refused(pool, want):
    """The condition "all_refused" of a code whose exponents pass 2^16: the reference's own
    check of a correction (its 16-bit exponent arithmetic) refuses every dirty row, with
    corrected_num counted where a locator was found, and passes every clean one."""
    ok, cor = want[0], want[1]
    dirty = (np.concatenate([pool.data, pool.parity], 1) != pool.clean).any(1)
    assert dirty.any() and not ok[dirty].any() and ok[~dirty].all(), "all_refused: a dirty row succeeds"
    assert (cor[dirty] > 0).any() and (cor[dirty] == 0).any()
    return {"all_refused": (int(dirty.sum()), int((cor[dirty] > 0).sum()))}


def family_conditions(pool, want, relaxed=(), nn=255):
    """pool: rows and tags; want: Oracle.decode_batch of them; nn: the field's 2^m - 1 (255 in
    the text below).  `relaxed` names the
    conditions a code is excused from (see the codes' entries in the tests):
      "late_fails"     no late_discrepancy row with e > 0 succeeds (e = 0 is a sparse single)
      "late_counted"   at least one late_discrepancy failure has corrected_num > 0
      "sparse_zero"    a sparse single S_j fails with corrected_num == 0, or j + 1 > t divides
                       255 and it succeeds with corrected_num == j + 1 (see sparse())
      "padding_fails"  padding_roots rows fail with corrected_num == 0
      "all_refused"    instead of all the above: see _all_refused
    Returns the counts it looked at, for the record."""
    ok, cor, od, op = want
    fam = pool.families()
    failed = ok == 0
    assert (od[failed] == pool.data[failed]).all() and (op[failed] == pool.parity[failed]).all(), \
        "a failed row was modified"
    if "all_refused" in relaxed:
        return _all_refused(pool, want)
    seen = {}
    size = pool.data.shape[1]
    tt = pool.parity.shape[1] // 2
    n = np.array([len(t.positions or ()) for t in pool.tags])
    restored = (od == pool.clean[:, :size]).all(1) & (op == pool.clean[:, size:]).all(1)
    damaged = (np.concatenate([pool.data, pool.parity], 1) != pool.clean).sum(1)
    z = fam == "zero_run"
    if z.any():
        assert all(t.w + t.a == len(t.positions) for t in pool.tags if t.family == "zero_run")
        assert (damaged[z] == n[z]).all(), "zero_run: a pattern byte is zero"
        assert (ok[z] == 1).all() and (cor[z] == n[z]).all() and restored[z].all(), \
            "zero_run: a row was not corrected in full (ok, corrected_num == w + a, bytes of the clean row)"
        seen["zero_run"] = int(z.sum())
    within = np.array([t.family == "ordinary" and t.e <= tt for t in pool.tags])
    if within.any():
        assert (damaged[within] == n[within]).all()
        assert (ok[within] == 1).all() and (cor[within] == n[within]).all() and restored[within].all(), \
            "ordinary: a row of at most t errors was not corrected in full"
        seen["ordinary"] = int(within.sum())
    ld = fam == "late_discrepancy"
    if ld.any():
        e0 = np.array([t.family == "late_discrepancy" and t.e == 0 for t in pool.tags])
        if "late_fails" not in relaxed:
            assert not ok[ld & ~e0].any(), f"late_discrepancy: {int(ok[ld & ~e0].sum())} rows succeed"
        if "late_counted" not in relaxed:
            assert (failed & ld & (cor > 0)).any(), "late_discrepancy: no failure with corrected_num counted"
        seen["late_discrepancy"] = (int(ld.sum()), int(ok[ld].sum()), int((failed & ld & (cor > 0)).sum()))
    single = np.array([(t.family == "sparse" and "i" not in t.params) or (t.family == "late_discrepancy" and t.e == 0)
                       for t in pool.tags])
    if single.any():
        j1 = np.array([t.j + 1 if s else 0 for t, s in zip(pool.tags, single)])
        full = single & (ok == 1) & (cor == j1) & (j1 > tt) & (nn % np.maximum(j1, 1) == 0)
        if "sparse_zero" not in relaxed:
            assert ((failed & (cor == 0)) | full)[single].all(), "sparse singles: a row succeeds or counts"
        seen["sparse"] = (int(single.sum()), int(ok[single].sum()), int((cor[single] > 0).sum()))
    pr = fam == "padding_roots"
    if pr.any():
        if "padding_fails" not in relaxed:
            assert not ok[pr].any() and not cor[pr].any(), "padding_roots: a row succeeds or counts"
        seen["padding_roots"] = (int(pr.sum()), int(ok[pr].sum()), int((cor[pr] > 0).sum()))
    po = fam == "positions"
    if po.any():
        assert (damaged[po] == n[po]).all()
        assert (ok[po] == 1).all() and (cor[po] == n[po]).all() and restored[po].all(), \
            "positions: a row was not corrected in full"
        seen["positions"] = int(po.sum())
    return seen


# ---------------------------------------------------------------------------
# rows with erasure lists: (data, parity, tags, slots, counts)
#
# The reference hands magnitude n, in the order of its root search, to list slot n, stale
# slots after the count included once the locator has more roots than the list has
# entries.  So ok and corrected_num do not depend on the order of a list, the bytes do, and
# a row comes back clean only when its nr slots begin with the damaged positions in that
# order (SyndromeMap.visit): the erased ones met first, the errors' in the stale slots.
# ---------------------------------------------------------------------------
ORDERS = ("ascending", "descending", "insertion")
NAMED_DEGREES = (15, 16, 17, 23, 24, 25, 31, 32)  # the brackets of rs_chien32_k and rs_forney32_k, and the 5-bit wrap


def named_degrees(nr):
    """The named final degrees that a code of nr roots can reach, and nr - 1 and nr."""
    return sorted({d for d in NAMED_DEGREES if d <= nr} | {nr - 1, nr})


def _ordered(pos, order):
    pos = [int(p) for p in pos]
    return sorted(pos) if order == "ascending" else sorted(pos, reverse=True) if order == "descending" else pos


class _Listed:
    """The rows of one errata family under construction: n random clean rows, stale slot
    bytes of junk (any byte value: a stale slot may lie past the codeword)."""

    def __init__(self, sm, rng, family, n):
        self.sm, self.rng, self.family = sm, rng, family
        self.clean = sm.base_rows(rng, n)
        self.rows = self.clean.copy()
        self.slots = rng.integers(0, 256, (n, sm.nr), dtype=np.uint8)
        self.counts = np.zeros(n, np.uint8)
        self.tags = []

    def damage(self, c, pos):
        pos = np.asarray(pos, dtype=np.int64)
        self.rows[c, pos] ^= self.rng.integers(1, self.sm.nn + 1, pos.size, dtype=np.uint8)

    def same_row(self, c, src):
        """row c: the clean row, the damage and the junk of row src"""
        self.clean[c], self.rows[c], self.slots[c] = self.clean[src], self.rows[src], self.slots[src]

    def add(self, listed, stale=(), idle=(), positions=None, **params):
        """The next row's list: `listed` counts, `stale` follows it, junk after that."""
        c, ne = len(self.tags), len(listed)
        assert ne + len(stale) <= self.sm.nr
        self.slots[c, :ne] = listed
        self.slots[c, ne:ne + len(stale)] = stale
        self.counts[c] = ne
        g = Tag(self.family, None if positions is None else tuple(int(p) for p in positions), **params)
        g.slots, g.count, g.idle = tuple(int(x) for x in self.slots[c]), ne, tuple(int(p) for p in idle)
        self.tags.append(g)
        return c

    def done(self):
        assert len(self.tags) == len(self.rows), (self.family, len(self.tags), len(self.rows))
        return self.sm._split(self.rows, self.tags, self.clean) + (self.slots, self.counts)


def _ne_range(sm, ne_range, lo=0):
    top = min(sm.nr, sm.width)
    return [ne for ne in (range(lo, top + 1) if ne_range is None else ne_range) if lo <= ne <= top]


def errata_grid(sm, ne_range=None, draws=1, seed=0):
    """ne erasures and e errors elsewhere for every (ne, e) with ne + 2e <= nr + 2: all that
    the code corrects and the two diagonals beyond.  Each damaged row three times, its list
    in ascending, descending and insertion order."""
    rng = _rng(sm, seed, "errata_grid")
    nr, W = sm.nr, sm.width
    cells = [(ne, e) for ne in _ne_range(sm, ne_range) for e in range((nr + 2 - ne) // 2 + 1) if ne + e <= W] * draws
    b = _Listed(sm, rng, "errata_grid", 3 * len(cells))
    for i, (ne, e) in enumerate(cells):
        pos = rng.permutation(W)[:ne + e]
        b.damage(3 * i, pos)
        for o, order in enumerate(ORDERS):
            b.same_row(3 * i + o, 3 * i)
            b.add(_ordered(pos[:ne], order), positions=pos, ne=ne, e=e, order=order, degree=ne + e)
    return b.done()


def idle_erasures(sm, ne_range=None, seed=0):
    """Counted slots whose symbols are correct: ne slots in the order of the root search
    (prim 1: ascending) of which v carry a nonzero value, v in 0 .. ne (ne = nr, v = 1: a
    single magnitude among nr sorted slots); the same with e errors elsewhere; and clean rows (v = 0, e = 0) whose list holds a slot
    past the codeword, size + nr or 255."""
    rng = _rng(sm, seed, "idle_erasures")
    nr, W = sm.nr, sm.width
    nes = _ne_range(sm, ne_range, 1)
    spec = [(ne, v, 0, None) for ne in nes for v in range(ne + 1)]
    spec += [(ne, 0, 0, out) for ne in nes for out in sorted({W, 255})]
    for ne in nes:
        top = min((nr - ne) // 2, W - ne)
        if top >= 1:
            spec.append((ne, int(rng.integers(0, ne + 1)), int(rng.integers(1, top + 1)), None))
    b = _Listed(sm, rng, "idle_erasures", len(spec))
    for c, (ne, v, e, out) in enumerate(spec):
        era = rng.permutation(W)[:ne]
        live = era[:v]
        b.damage(c, live)
        err = sm._scatter(rng, b.rows, c, e, avoid=era)
        listed = [int(p) for p in sm.by_visit(era)]  # (prim 1: ascending)
        if out is not None:
            listed[int(rng.integers(0, ne))] = out
            listed.sort()
        b.add(listed, idle=era[v:], positions=tuple(live) + err, ne=ne, v=v, e=e, outside=out)
    return b.done()


def errata_zero_run(sm, draws=2, seed=0):
    """ne erased positions with any values and, elsewhere, an error pattern of weight w
    whose plain syndromes S_0 .. S_(k-1) vanish and whose S_k does not (vanishing_pattern),
    ne < k < w, ne + 2w <= nr.  The erasure locator annihilates the erased positions' share
    of every discrepancy, so Berlekamp-Massey starts at r = ne + 1 with zero discrepancies
    up to r = k and then lengthens by more than one.  Even rows name the damage in the
    order of the root search (the errors' positions in the stale slots) and come back
    clean; odd rows name it in any order."""
    rng = _rng(sm, seed, "errata_zero_run")
    nr, W = sm.nr, sm.width
    combos = [(ne, k, w) for ne in range((nr - 4) // 3 + 1) for k in range(ne + 1, nr)
              for w in range(k + 1, (nr - ne) // 2 + 1) if ne + w <= W] * draws
    b = _Listed(sm, rng, "errata_zero_run", len(combos))
    for c, (ne, k, w) in enumerate(combos):
        pos = rng.permutation(W)[:ne + w]
        rooted = c % 2 == 0
        if rooted:
            pos = sm.by_visit(pos)
        era, err = pos[:ne], pos[ne:]
        for _ in range(100):
            v = sm.vanishing_pattern(rng, err, k)
            probe = np.zeros((1, W), np.uint8)
            probe[0, err] = v
            S = sm.syndromes(probe[:, :sm.size], probe[:, sm.size:])[0]
            assert not S[:k].any()
            if S[k]:
                break
        else:
            raise AssertionError("no pattern with S_k != 0")
        b.rows[c, err] ^= v
        b.damage(c, era)
        b.add(era, stale=err if rooted else (), positions=pos, ne=ne, k=k, w=w, rooted=rooted)
    return b.done()


def errata_late(sm, draws=1, seed=0):
    """ne erasures with values, e errors (ne + 2e <= nr), then a nonzero value XORed into
    one syndrome S_j, for every ne and j: deg != L, L past the bound, failures with and
    without a counted corrected_num."""
    rng = _rng(sm, seed, "errata_late")
    nr, W = sm.nr, sm.width
    combos = [(ne, j) for ne in _ne_range(sm, None) for j in range(nr)] * draws
    b = _Listed(sm, rng, "errata_late", len(combos))
    S = np.zeros((len(combos), nr), np.uint8)
    for c, (ne, j) in enumerate(combos):
        e = int(rng.integers(0, min((nr - ne) // 2, W - ne) + 1))
        pos = rng.permutation(W)[:ne + e]
        b.damage(c, pos)
        S[c, j] = rng.integers(1, sm.nn + 1)
        b.add(_ordered(pos[:ne], ORDERS[c % 3]), positions=pos, ne=ne, e=e, j=j)
    b.rows[:, sm.size:] ^= sm.parity_for(S)
    return b.done()


def errata_sparse(sm, seed=0):
    """Exactly one nonzero syndrome S_j under lists of every count, for every j; lists of
    nr slots sorted (the Vandermonde solve answers any syndromes) and unsorted."""
    rng = _rng(sm, seed, "errata_sparse")
    nr, W = sm.nr, sm.width
    combos = [(j, ne, (j + ne) % 2 == 0 or ne == nr) for j in range(nr) for ne in _ne_range(sm, None)]
    combos += [(j, nr, False) for j in range(nr) if nr <= W]
    b = _Listed(sm, rng, "errata_sparse", len(combos))
    S = np.zeros((len(combos), nr), np.uint8)
    for c, (j, ne, asc) in enumerate(combos):
        S[c, j] = rng.integers(1, sm.nn + 1)
        listed = rng.permutation(W)[:ne]
        if not asc and ne >= 2 and (np.diff(listed) > 0).all():
            listed = listed[::-1]
        b.add(_ordered(listed, "ascending" if asc else "insertion"), j=j, ne=ne, sorted=asc)
    b.rows[:, sm.size:] ^= sm.parity_for(S)
    return b.done()


def errata_degrees(sm, draws=1, seed=0):
    """Rows that succeed with final degree exactly D for every D of named_degrees(nr), in
    every split D = ne + e with ne + 2e <= nr; each split with every erased symbol in error
    and, for ne >= 1, with one of them idle.  D = nr also from nr slots in descending and
    in insertion order."""
    rng = _rng(sm, seed, "errata_degrees")
    nr, W = sm.nr, sm.width
    spec = []
    for D in named_degrees(nr):
        for e in range(min(nr - D, D) + 1):
            ne = D - e
            if D > W:
                continue
            spec.append((D, ne, e, 0, "ascending"))
            if ne >= 1:
                spec.append((D, ne, e, 1, "ascending"))
            if D == nr:
                spec += [(D, ne, e, 0, "descending"), (D, ne, e, 0, "insertion")]
    spec = spec * draws
    b = _Listed(sm, rng, "errata_degrees", len(spec))
    for c, (D, ne, e, idle, order) in enumerate(spec):
        pos = rng.permutation(W)[:D]
        if order == "insertion" and ne >= 2 and (np.diff(pos[:ne]) > 0).all():
            pos[:ne] = pos[:ne][::-1]
        b.damage(c, pos[idle:])
        b.add(_ordered(pos[:ne], order), idle=pos[:idle], positions=pos[idle:], degree=D, ne=ne, e=e, order=order)
    return b.done()


def errata_positions(sm, runs=None, seed=0):
    """One erasure at every position; one erasure at p with one error at p + 1 (named in the
    first stale slot), for every p; `runs` consecutive erased positions for every start
    (default 3 and nr); and the position whose root the reference tries last
    (last_visited), alone, beside an erasure at 0, and as an error beside it."""
    rng = _rng(sm, seed, "errata_positions")
    nr, W = sm.nr, sm.width
    runs = sorted({r for r in ((3, nr) if runs is None else runs) if 1 <= r <= min(nr, W)})
    last = sm.last_visited()
    spec = [("single", (p,), ()) for p in range(W)] + [("pair", (p,), (p + 1,)) for p in range(W - 1)]
    spec += [("run", tuple(range(s, s + r)), ()) for r in runs for s in range(W - r + 1)]
    spec += [("last", (last,), ()), ("last", (0, last), ()), ("last", (0,), (last,))]
    b = _Listed(sm, rng, "errata_positions", len(spec))
    for c, (kind, era, err) in enumerate(spec):
        b.damage(c, era + err)
        b.add(era, stale=err, positions=era + err, kind=kind, at=era[0], ne=len(era), e=len(err), last=last)
    return b.done()


def errata_padding(sm, full, seed=0):
    """Shortened sizes: padding_roots with an erasure list besides.  The errors' syndromes
    come from a row of the full-length code (`full`) with 1 .. e of its e errors inside the
    padding, ne + 2e <= nr; the ne erased positions of the short row carry values.  The
    locator is found, and one of its roots lies before the row."""
    rng = _rng(sm, seed, "errata_padding")
    nr, W, pad = sm.nr, sm.width, full.size - sm.size
    assert pad > 0 and full.nr == nr
    combos = [(ne, e, p) for e in range(1, nr // 2 + 1) for p in range(1, e + 1)
              for ne in sorted({0, 1, (nr - 2 * e) // 2, nr - 2 * e}) if p <= pad and ne + e - p <= W and 0 <= ne <= nr - 2 * e]
    b = _Listed(sm, rng, "errata_padding", len(combos))
    err = np.zeros((len(combos), full.width), np.uint8)
    for c, (ne, e, p) in enumerate(combos):
        short = rng.permutation(W)
        era, inside = short[:ne], short[ne:ne + e - p]
        at = np.concatenate([rng.permutation(pad)[:p], pad + inside])
        err[c, at] = rng.integers(1, sm.nn + 1, e, dtype=np.uint8)
        b.damage(c, era)
        b.add(_ordered(era, ORDERS[c % 3]), positions=tuple(era) + tuple(inside), ne=ne, e=e, inside=p)
    b.rows[:, sm.size:] ^= sm.parity_for(full.syndromes(err[:, :full.size], err[:, full.size:]))
    return b.done()


def errata_outside(sm, seed=0, ne_range=None):
    """A slot past the codeword, size + nr or 255, in threes on one damaged row (ne erasures
    and e errors, ne + e < nr): the plain list; the list with that slot counted besides;
    the plain list with that value in the last stale slot, which no magnitude reaches."""
    rng = _rng(sm, seed, "errata_outside")
    nr, W = sm.nr, sm.width
    spec = [(ne, out) for ne in _ne_range(sm, range(nr) if ne_range is None else [n for n in ne_range if n < nr])
            for out in sorted({W, 255})]
    b = _Listed(sm, rng, "errata_outside", 3 * len(spec))
    for i, (ne, out) in enumerate(spec):
        e = int(rng.integers(0, min((nr - 1 - ne) // 2, W - ne) + 1))
        pos = rng.permutation(W)[:ne + e]
        b.damage(3 * i, pos)
        b.slots[3 * i, nr - 1] = pos[0] if len(pos) else 0
        for o, kind in enumerate(("plain", "counted", "stale")):
            b.same_row(3 * i + o, 3 * i)
            if kind == "stale":
                b.slots[3 * i + o, nr - 1] = out
            b.add(_ordered(pos[:ne], "insertion") + ([out] if kind == "counted" else []), positions=pos, ne=ne, e=e,
                  kind=kind, outside=out)
    return b.done()


def errata_repeats(sm, seed=0, ne_range=None):
    """A slot counted twice, next to itself and apart; a counted slot repeated in the first
    stale slot; nr slots ascending but for one pair of equal neighbours, at every index."""
    rng = _rng(sm, seed, "errata_repeats")
    nr, W = sm.nr, sm.width
    spec = [(kind, ne, 0) for ne in _ne_range(sm, ne_range, 2) for kind in ("adjacent", "apart", "stale")
            if (kind != "apart" or ne >= 3) and (kind != "stale" or ne < nr)]
    spec += [("asc_pair", nr, i) for i in range(nr - 1) if nr <= W]
    b = _Listed(sm, rng, "errata_repeats", len(spec))
    for c, (kind, ne, i) in enumerate(spec):
        distinct = ne if kind == "stale" else ne - 1
        pos = rng.permutation(W)[:distinct]
        listed, stale = [int(p) for p in pos], ()
        if kind == "adjacent":
            i = int(rng.integers(0, distinct))
            listed.insert(i + 1, listed[i])
        elif kind == "apart":
            i = int(rng.integers(0, distinct - 1))
            listed.insert(int(rng.integers(i + 2, distinct + 1)), listed[i])
        elif kind == "stale":
            stale = (listed[int(rng.integers(0, ne))],)
        else:
            listed.sort()
            listed.insert(i + 1, listed[i])
        e = int(rng.integers(0, min((nr - ne) // 2, W - distinct) + 1)) if kind != "asc_pair" else 0
        b.damage(c, pos)
        extra = sm._scatter(rng, b.rows, c, e, avoid=pos)
        b.add(listed, stale=stale, positions=tuple(pos) + extra, kind=kind, ne=ne, e=e)
    return b.done()


def count_zero(sm, full=None, seed=0, src=None):
    """The rows of the errors-only family_pool (or of the pool `src`) under the erasure mode
    with count 0 and junk in the stale slots (quirk Q3: the magnitudes go to the stale slots)."""
    rng = _rng(sm, seed, "count_zero")
    src = family_pool(sm, full, seed=seed) if src is None else src
    tags = []
    slots = rng.integers(0, 256, (len(src), sm.nr), dtype=np.uint8)
    for c, t in enumerate(src.tags):
        g = Tag("count_zero", t.positions, origin=t.family)
        g.base, g.slots = t.base, tuple(int(x) for x in slots[c])
        tags.append(g)
    return src.data, src.parity, tags, slots, np.zeros(len(src), np.uint8)


def errata_pool(sm, full=None, draws=1, seed=0):
    """Every errata family of (code, size) in one pool; errata_padding where `full` is given.
    Three damaged rows for each cell of errata_grid: the uniform and lone waves draw on them."""
    parts = [errata_grid(sm, draws=3 * draws, seed=seed), idle_erasures(sm, seed=seed),
             errata_zero_run(sm, draws=2 * draws, seed=seed), errata_late(sm, draws=draws, seed=seed),
             errata_sparse(sm, seed), errata_degrees(sm, draws=draws, seed=seed), errata_positions(sm, seed=seed),
             errata_outside(sm, seed), errata_repeats(sm, seed), count_zero(sm, full, seed)]
    if full is not None and full.size > sm.size:
        parts.append(errata_padding(sm, full, seed))
    return Pool.concat(parts)


ERRATA_FAMILIES = ("errata_grid", "idle_erasures", "errata_zero_run", "errata_late", "errata_sparse", "errata_degrees",
                   "errata_positions", "errata_outside", "errata_repeats", "count_zero", "errata_padding")


def decode_lists(oracle, pool, rows=None, threads=0):
    """Oracle.decode_batch of the pool's rows under their erasure lists"""
    rows = np.arange(len(pool)) if rows is None else rows
    return oracle.decode_batch(pool.data[rows], pool.parity[rows], pool.slots[rows].astype(np.uint32),
                               pool.counts[rows].astype(np.uint32), threads=threads)


def errata_conditions(pool, want, sm, relaxed=()):
    """pool: rows with lists; want: decode_lists of them; sm: the pool's SyndromeMap (for the
    order of the root search alone).  What every family promises, on the oracle's results:
      every family      a failed row comes back unmodified
      errata_grid       ne + 2e <= nr: success with corrected_num == ne + e; e == 0 and the list
                        in the order of the root search: the clean row
      idle_erasures     ne + 2e <= nr by construction: success with corrected_num == v + e, the
                        nonzero magnitudes alone; v == 0 and e == 0: success with 0 and no byte
                        changed, a slot past the codeword in the list or not; e == 0 and the
                        list in root order: the clean row
      errata_zero_run   success with corrected_num == ne + w == the symbols that differ from the
                        clean row; the rooted rows: the clean row
      errata_late       at least one failure with corrected_num counted and one without
                        ("late_counted" excuses a code)
      errata_degrees    at least one success at each degree of named_degrees(nr) that the row's
                        width allows; corrected_num == degree - the idle symbols on every success
                        (a code of fewer than 32 roots has no degree above nr: named_degrees)
      errata_positions  success with corrected_num == the damaged symbols; a list in root order
                        with the errors in the stale slots: the clean row
      errata_padding    failure with corrected_num == 0 ("padding_fails" excuses a code)
      errata_outside    the row with the outside value in its last stale slot gives what the
                        plain row gives
    ("all_refused" in `relaxed`: _all_refused instead of all these.)
    Returns the counts it looked at, for the record."""
    ok, cor, od, op = want
    fam = pool.families()
    nr = pool.parity.shape[1]
    size = pool.data.shape[1]
    failed = ok == 0
    assert (od[failed] == pool.data[failed]).all() and (op[failed] == pool.parity[failed]).all(), \
        "a failed row was modified"
    if "all_refused" in relaxed:
        return _all_refused(pool, want)
    restored = (od == pool.clean[:, :size]).all(1) & (op == pool.clean[:, size:]).all(1)
    untouched = (od == pool.data).all(1) & (op == pool.parity).all(1)
    damaged = (np.concatenate([pool.data, pool.parity], 1) != pool.clean).sum(1)
    n = np.array([len(t.positions or ()) for t in pool.tags])
    par = lambda name, default=-1: np.array([t.params.get(name, default) for t in pool.tags])  # noqa: E731
    ne, e = par("ne"), par("e")
    rooted = np.array([t.slots is not None and t.positions is not None and len(t.positions) <= nr and
                       sorted(t.slots[:len(t.positions)]) == sorted(t.positions) and
                       sm.in_root_order(t.slots[:len(t.positions)]) for t in pool.tags])
    seen = {}

    def full(sel, what):
        assert (damaged[sel] == n[sel]).all(), what + ": a damaged symbol equals the clean row's"
        assert (ok[sel] == 1).all(), f"{what}: row {int(np.nonzero(sel & failed)[0][0])} fails"
        assert (cor[sel] == n[sel]).all(), what + ": corrected_num is not the number of damaged symbols"
        assert restored[sel & rooted].all(), what + ": a list in root order did not restore the row"

    g = fam == "errata_grid"
    if g.any():
        within = g & (ne + 2 * e <= nr)
        full(within, "errata_grid")
        assert (rooted & within & (e == 0) & (ne >= 2)).any() and (~rooted & within & (ne >= 2)).any()
        seen["errata_grid"] = (int(g.sum()), int(ok[g].sum()), int((restored & g).sum()))
    i = fam == "idle_erasures"
    if i.any():
        v = par("v")
        assert (ok[i] == 1).all() and (cor[i] == (v + e)[i]).all(), "idle_erasures: ok, corrected_num == v + e"
        assert (damaged[i] == (v + e)[i]).all()
        clean = i & (v == 0) & (e == 0)
        assert untouched[clean].all() and (par("outside", None)[clean] != None).any()  # noqa: E711
        live = i & (e == 0) & np.array([t.slots is not None and sm.in_root_order(t.slots[:t.count])
                                        for t in pool.tags])
        assert restored[live].all() and (live & (v > 0) & (v < ne)).any()
        seen["idle_erasures"] = (int(i.sum()), int(clean.sum()), int(live.sum()))
    z = fam == "errata_zero_run"
    if z.any():
        full(z, "errata_zero_run")
        assert ((ne + par("w"))[z] == n[z]).all() and (rooted & z).any() and (restored[z] == rooted[z]).mean() > 0.9
        seen["errata_zero_run"] = (int(z.sum()), int((restored & z).sum()))
    la = fam == "errata_late"
    if la.any():
        if "late_counted" not in relaxed:
            assert (la & failed & (cor > 0)).any() and (la & failed & (cor == 0)).any()
        seen["errata_late"] = (int(la.sum()), int(ok[la].sum()), int((la & failed & (cor > 0)).sum()))
    s = fam == "errata_sparse"
    if s.any():
        seen["errata_sparse"] = (int(s.sum()), int(ok[s].sum()), int((cor[s] > 0).sum()))
    d = fam == "errata_degrees"
    if d.any():
        deg = par("degree")
        idle = np.array([len(t.idle) for t in pool.tags])
        assert (cor[d & (ok == 1)] == (deg - idle)[d & (ok == 1)]).all(), "errata_degrees: corrected_num"
        assert (ok[d] == 1).all(), "errata_degrees: a row within the code's reach fails"
        at = {int(D): int((d & (ok == 1) & (deg == D)).sum()) for D in named_degrees(nr) if D <= size + nr}
        assert all(at.values()), f"errata_degrees: no success at some degree: {at}"
        assert all((d & (deg == D) & (idle == 0)).any() and (d & (deg == D) & (idle == 1)).any() for D in at)
        seen["errata_degrees"] = at
    po = fam == "errata_positions"
    if po.any():
        full(po, "errata_positions")
        assert restored[po & (par("kind", "") != "pair")].all() or sm.o.prim != 1
        seen["errata_positions"] = (int(po.sum()), int((restored & po).sum()))
    pr = fam == "errata_padding"
    if pr.any():
        if "padding_fails" not in relaxed:
            assert not ok[pr].any() and not cor[pr].any(), "errata_padding: a row succeeds or counts"
        seen["errata_padding"] = (int(pr.sum()), int(ok[pr].sum()), int((cor[pr] > 0).sum()))
    out = fam == "errata_outside"
    if out.any():
        kind = par("kind", "")
        plain, stale = np.nonzero(out & (kind == "plain"))[0], np.nonzero(out & (kind == "stale"))[0]
        assert (stale == plain + 2).all()
        assert (ok[plain] == ok[stale]).all() and (cor[plain] == cor[stale]).all() and \
            (od[plain] == od[stale]).all() and (op[plain] == op[stale]).all(), "errata_outside: a stale slot matters"
        counted = out & (kind == "counted")
        seen["errata_outside"] = (int(out.sum()), int(ok[plain].sum()), int(ok[counted].sum()))
    for name in ("errata_repeats", "count_zero"):
        m = fam == name
        if m.any():
            seen[name] = (int(m.sum()), int(ok[m].sum()), int((restored & m).sum()))
    return seen


# ---------------------------------------------------------------------------
# layouts: orders of a pool's rows (index arrays; a row may appear more than once)
# ---------------------------------------------------------------------------
def uniform_blocks(pool, t):
    """For each e in 0 .. t+1, BM_WORKGROUP consecutive rows of ordinary(e): one rs_bm_k
    workgroup, 8 waves of the same degree."""
    out = []
    for e in range(t + 2):
        idx = pool.where(lambda g: g.family == "ordinary" and g.e == e)
        assert idx.size, f"the pool has no ordinary({e}) rows"
        out.append(np.resize(idx, BM_WORKGROUP))
    return np.concatenate(out)


def list_rows(pool, t):
    """late_discrepancy rows whose L passes t (j + 1 - e > t): never on the fast path"""
    return pool.where(lambda g: g.family == "late_discrepancy" and g.j + 1 - g.e > t)


def lone_lane(pool, t):
    """Waves of 63 rows of one kind and one row of another at lane 0, 31, 32 and 63:
    1 error among t errors and the reverse, clean among 1 error and the reverse, fast rows
    (1 .. t errors) among list rows and the reverse."""
    def ordinary_e(lo, hi):
        return pool.where(lambda g: g.family == "ordinary" and lo <= g.e <= hi)
    kinds = {"one": ordinary_e(1, 1), "t": ordinary_e(t, t), "clean": ordinary_e(0, 0), "fast": ordinary_e(1, t),
             "list": list_rows(pool, t)}
    out = []
    for a, b in (("t", "one"), ("one", "t"), ("one", "clean"), ("clean", "one"), ("list", "fast"), ("fast", "list")):
        for n, lane in enumerate((0, 31, 32, 63)):
            assert kinds[a].size and kinds[b].size, (a, b)
            wave = np.resize(np.roll(kinds[a], -WAVE * n), WAVE)
            wave[lane] = kinds[b][n % kinds[b].size]
            out.append(wave)
    return np.concatenate(out)


def sorted_by_tag(pool):
    """The rows grouped by family, so whole waves are exotic and whole waves are on the list."""
    return np.argsort(pool.families(), kind="stable")


def shuffled(pool, seed=0):
    return np.random.default_rng([seed, len(pool)]).permutation(len(pool))


def odd_counts(n):
    """The largest counts 64 q + 1 and 64 q + 63 up to n"""
    return [c for c in ((n - 1) // WAVE * WAVE + 1, (n - 63) // WAVE * WAVE + 63) if 0 < c <= n]


def pad_to(order, n=SPLIT_MIN_COUNT):
    """`order` repeated up to at least n rows"""
    return order if len(order) >= n else np.resize(order, n)


# ---------------------------------------------------------------------------
# layouts of a pool of rows with erasure lists
# ---------------------------------------------------------------------------
EBM_WORKGROUP = 1024  # rows of one rs_ebm_k / rs_chien32_k / rs_forney32_k / rs_era_bp_k workgroup
LANES = (0, 31, 32, 63)


def _ascending(t, width):
    s = t.slots[:t.count]
    return all(a < b for a, b in zip(s, s[1:])) and (not s or s[-1] < width)


def _kinds(pool, want):
    """The rows of a pool by what the kernels make of them, from the tags and the oracle's
    results: index arrays."""
    ok = want[0]
    nr = pool.parity.shape[1]
    width = pool.data.shape[1] + nr
    dirty = ((pool.data != pool.clean[:, :pool.data.shape[1]]).any(1) | (pool.parity != pool.clean[:, -nr:]).any(1))
    grid = pool.where(lambda g: g.family == "errata_grid" and g.ne + 2 * g.e <= nr)
    k = {"grid": grid, "dirty": np.array([r for r in grid if dirty[r]], np.int64)}
    k["clean"] = pool.where(lambda g: g.family == "idle_erasures" and g.v == 0 and g.e == 0)
    for ne in range(nr + 1):
        k[ne] = np.array([r for r in grid if pool.counts[r] == ne and (ne < nr or not _ascending(pool.tags[r], width))],
                         np.int64)
    # nr sorted in-range slots on a dirty row: what rs_era_bp_k solves itself
    k["bp"] = np.array([r for r, t in enumerate(pool.tags) if t.count == nr and dirty[r] and _ascending(t, width)],
                       np.int64)
    # a counted slot past the codeword on a dirty row: refused by rs_ebm_k, the general kernel's
    k["list"] = np.array([r for r, t in enumerate(pool.tags) if t.family == "errata_outside" and dirty[r] and
                          t.kind == "counted"], np.int64)
    k["pending"] = np.array([r for r in grid if dirty[r] and 0 < pool.counts[r] < nr], np.int64)
    # the final degree of a row that succeeds within the code's reach (ne + 2e <= nr; beyond it a
    # success is a miscorrection at some other degree): the oracle's nonzero magnitudes and the idle
    # erased symbols, which must be the ne + e of the construction
    cor = want[1].astype(np.int64)
    deg = np.array([cor[r] + len(t.idle) if t.family in ("errata_grid", "errata_degrees") and ok[r] == 1 and dirty[r]
                    and t.ne + 2 * t.e <= nr else -1 for r, t in enumerate(pool.tags)])
    assert all(deg[r] == t.degree for r, t in enumerate(pool.tags) if deg[r] >= 0), "a degree is not ne + e"
    k["degree"] = deg
    return k


def _fill(idx, n, turn=0):
    assert len(idx), "no such rows in the pool"
    return np.resize(np.roll(idx, -turn), n)


def uniform_ne(pool, want, groups=None):
    """For each count ne in 0 .. nr a whole wave of errata_grid rows with that count (nr:
    unsorted), then whole workgroups of EBM_WORKGROUP rows for ne in 0, 1, 16, 28, 29, 31 and nr
    unsorted (the counts below nr that the code has, nr - 4, nr - 3 and nr - 1 among them)."""
    nr = pool.parity.shape[1]
    k = _kinds(pool, want)
    groups = sorted({g for g in (0, 1, 16, 28, 29, 31, nr - 4, nr - 3, nr - 1, nr) if 0 <= g <= nr} if groups is None
                    else groups)
    return np.concatenate([_fill(k[ne], WAVE) for ne in range(nr + 1)] +
                          [_fill(k[ne], EBM_WORKGROUP) for ne in groups])


def lone_ne(pool, want):
    """Waves of 63 rows of one kind and one of another at lane 0, 31, 32 and 63: nr unsorted
    slots and count 0, nr - 3 and 3 slots, clean and dirty rows, list rows (a counted slot
    past the codeword) and rows the errata kernels finish, each pair both ways."""
    nr = pool.parity.shape[1]
    k = _kinds(pool, want)
    pairs = ((nr, 0), (0, nr), (nr - 3, 3), (3, nr - 3), ("clean", "dirty"), ("dirty", "clean"), ("list", "grid"),
             ("grid", "list"))
    out = []
    for a, b in pairs:
        for n, lane in enumerate(LANES):
            wave = _fill(k[a], WAVE, WAVE * n)
            lone = [r for r in k[b] if pool.tags[r].params.get("e", 0) >= 1 or b == "clean"]
            wave[lane] = (lone or list(k[b]))[n % len(lone or k[b])]  # (a lone row with errors to find, if any)
            out.append(wave)
    return np.concatenate(out)


def degree_brackets(pool, want):
    """Waves whose rows all end at a degree of at most 16, all in 17 .. 24, all in 25 .. 32
    (the brackets the code's nr reaches), then 63 rows of degree at most 16 with one of
    degree 17, 24, 25 and 32 (those that nr reaches) at lane 0, 31, 32 and 63."""
    nr = pool.parity.shape[1]
    deg = _kinds(pool, want)["degree"]
    def spread(lo, hi):  # 64 rows across the bracket, both of its ends among them
        idx = np.nonzero((deg >= lo) & (deg <= hi))[0]
        idx = idx[np.argsort(deg[idx], kind="stable")]
        return idx[np.linspace(0, len(idx) - 1, WAVE).astype(np.int64)]

    low = np.nonzero((deg >= 1) & (deg <= 16))[0]
    out = [spread(1, 16)]
    for lo, hi in ((17, 24), (25, 32)):
        if nr >= lo:
            out.append(spread(lo, hi))
    for D in (17, 24, 25, 32):
        if D <= nr:
            for n, lane in enumerate(LANES):
                wave = _fill(low, WAVE, 7 * n + D)
                wave[lane] = _fill(np.nonzero(deg == D)[0], 1, n)[0]
                out.append(wave)
    return np.concatenate(out)


def bp_mixes(pool, want, waves=4):
    """Batches around rs_era_bp_k's pending flag, by name: "solved", rows of nr sorted in-range
    slots alone, nothing pending; "pending_last", such waves with one pending row at lane 63
    of the last wave; "one_clean", such waves with one clean row; "mix", solved and pending
    rows in turn."""
    k = _kinds(pool, want)
    n = waves * WAVE
    solved = _fill(k["bp"], n)
    last, clean, mix = solved.copy(), solved.copy(), solved.copy()
    last[-1] = k["pending"][0]
    clean[WAVE + 5] = k["clean"][0]
    mix[1::2] = _fill(k["pending"], n // 2)
    return {"solved": solved, "pending_last": last, "one_clean": clean, "mix": mix}


# ---------------------------------------------------------------------------
# the general kernels (rs_generic.hip): a codeword on GL lanes
#
# rsgw_decode_k<., GL> keeps index i = lane + GL q of the locator in register slot q, nq =
# (nr + GL) // GL slots.  With nq >= 2 Berlekamp-Massey starts narrow, on NQ = 1 (nq = 2) or
# 2 (nq >= 3) slots, and stops before the first iteration r at which B holds a nonzero at
# index GL NQ - 1 (gw_top_set); a run on all slots goes on from r: the hand-off.
# ---------------------------------------------------------------------------
GW_GROUP_MIN = 256  # rs_generic.hip: a batch below it runs every code on 64 lanes per codeword
GW_WORKGROUP = 256  # lanes of one rsgw_decode_k workgroup


def group_lanes(nn, count=GW_GROUP_MIN):
    """GL of a decode batch (rsgw_decode_launch)"""
    if count < GW_GROUP_MIN:
        return 64
    return 4 if nn <= 15 else 8 if nn <= 31 else 16 if nn <= 63 else 32 if nn <= 127 else 64


def narrow_top(nr, gl):
    """The index GL NQ - 1 of B that ends the narrow run, None where nq = 1 (no narrow run)."""
    nq = (nr + gl) // gl
    return None if nq < 2 else gl * (1 if nq == 2 else 2) - 1


def _spread(lo, hi, n, also=()):
    """About n integers across lo .. hi, both ends among them, and those of `also` in range"""
    if hi < lo:
        return []
    return sorted({int(x) for x in np.linspace(lo, hi, min(n, hi - lo + 1))} | {int(x) for x in also if lo <= x <= hi})


def bm_trace(sm, S, tops=()):
    """Berlekamp-Massey (errors only) on the syndrome values S (count, nr), on the oracle's log
    and antilog tables, all rows at once.  FOR TAGS AND COVERAGE CONDITIONS ONLY: no expected
    value of any test comes from here, and trace_conditions checks it against the oracle.
    Returns the final L (count,) and, for each T of `tops`, the first iteration r (1 .. nr) at
    whose start B[T] != 0, 0 where there is none or the row is clean (no BM runs on it)."""
    alog, log, _ = sm.o.tables()
    alog, log = alog.astype(np.int64), log.astype(np.int64)
    nn = sm.nn
    S = np.atleast_2d(np.asarray(S)).astype(np.int64)
    n, nr = S.shape

    def mul(a, b):
        return np.where((a == 0) | (b == 0), 0, alog[(log[a] + log[b]) % nn])

    lam = np.zeros((n, nr + 2), np.int64)
    lam[:, 0] = 1
    B, L = lam.copy(), np.zeros(n, np.int64)
    first = {T: np.zeros(n, np.int64) for T in tops}
    dirty = S.any(1)
    for r in range(1, nr + 1):
        for T in tops:
            first[T][(first[T] == 0) & (B[:, T] != 0) & dirty] = r
        disc = np.bitwise_xor.reduce(mul(lam[:, :r], S[:, r - 1::-1]), axis=1)  # sum of Lambda_i S_(r-1-i)
        Bm = np.zeros_like(B)
        Bm[:, 1:] = B[:, :-1]
        lengthen = (disc != 0) & (2 * L <= r - 1)
        inv = np.where(disc != 0, alog[(nn - log[disc]) % nn], 0)
        B = np.where(lengthen[:, None], mul(lam, inv[:, None]), Bm)
        lam = lam ^ mul(disc[:, None], Bm)
        L = np.where(lengthen, r - L, L)
    return L, first


def tag_trace(sm, pool, gls):
    """bm_trace of every row of an errors-only pool: each tag gets L (the final length) and
    handoff, {GL: the iteration at which the narrow run of that GL stops, 0 for none}."""
    assert not pool.counts.any()
    tops = sorted({narrow_top(sm.nr, gl) for gl in gls} - {None})
    L, first = bm_trace(sm, sm.syndromes(pool.data, pool.parity), tops)
    for c, g in enumerate(pool.tags):
        g.params["L"] = int(L[c])
        g.params["handoff"] = {gl: int(first[narrow_top(sm.nr, gl)][c]) if narrow_top(sm.nr, gl) is not None else 0
                               for gl in gls}
    return L


def trace_conditions(pool, want):
    """The trace against the oracle: on every row that the oracle corrects, the final L is its
    corrected_num (a clean row: both 0)."""
    ok, cor = want[0], want[1]
    L = np.array([g.L for g in pool.tags])
    bad = (ok == 1) & (L != cor)
    assert not bad.any(), f"bm_trace: L {L[bad][:5]} != corrected_num {cor[bad][:5]} at rows {np.nonzero(bad)[0][:5]}"
    return int((ok == 1).sum())


def handoff(sm, gl, per_r=6, seed=0):
    """Rows whose narrow run on GL = gl lanes stops at a chosen iteration r, for the earliest r
    (GL NQ: the first GL NQ - 1 syndromes zero, the next nonzero), the last (nr) and up to six
    between.  Candidates: e errors, e = 1 .. min(t, nr - GL NQ), whose B climbs one index an
    iteration once L has settled and reaches the top at r = GL NQ + e (they succeed); the same
    with a value XORed into one syndrome S_j, j >= r - 1, which the run on all slots meets
    after the hand-off (they fail, or are miscorrected); GL NQ - 1 zero syndromes, a nonzero one
    and random ones after it (the earliest r; they fail).  bm_trace says at which r each
    candidate stops, and nothing else; per_r rows are kept for each chosen r, half of them of
    the first kind where there are any."""
    T = narrow_top(sm.nr, gl)
    assert T is not None, "nq = 1: no narrow run"
    rng = _rng(sm, seed + gl, "handoff")
    nr, t, W = sm.nr, sm.t, sm.width
    es = [e for e in range(1, min(t, nr - T - 1, W) + 1)]
    spec = [("errors", e, None) for e in es] * 3
    spec += [("late", e, int(rng.integers(T + e, nr))) for e in [0] + es for _ in range(3)]
    spec += [("zeros", 0, None)] * 6
    n = len(spec)
    clean = sm.base_rows(rng, n)
    rows = clean.copy()
    S = np.zeros((n, nr), np.uint8)
    tags = []
    for c, (kind, e, j) in enumerate(spec):
        pos = sm._scatter(rng, rows, c, e)
        if kind == "late":
            S[c, j] = rng.integers(1, sm.nn + 1)
        elif kind == "zeros":
            S[c, T:] = rng.integers(1, sm.nn + 1, nr - T)
        tags.append(Tag("handoff", pos if kind != "zeros" else None, gl=gl, kind=kind, e=e, j=j))
    rows[:, sm.size:] ^= sm.parity_for(S)
    r = bm_trace(sm, sm.syndromes(rows[:, :sm.size], rows[:, sm.size:]), (T,))[1][T]
    found = sorted(set(r[r > 0].tolist()))
    assert found and found[0] >= T + 1, (found, T)
    chosen = [found[i] for i in _spread(0, len(found) - 1, 8)]
    keep = []
    for rr in chosen:
        at = np.nonzero(r == rr)[0]
        good = [c for c in at if spec[c][0] == "errors"][:per_r // 2]
        keep += good + [c for c in at if spec[c][0] != "errors"][:per_r - len(good)]
    for c in keep:
        tags[c].params["r"] = int(r[c])
    keep = np.array(keep)
    return sm._split(rows[keep], [tags[c] for c in keep], clean[keep])


def take(pool, idx):
    """The rows idx of a pool as a pool"""
    return Pool(pool.data[idx], pool.parity[idx], [pool.tags[i] for i in idx], pool.slots[idx], pool.counts[idx])


def general_pool(sm, full=None, gls=(64,), seed=0):
    """The errors-only families for a code of the general kernels, thinned where t > 8 (a long
    code has thousands of (k, w) and (e, j) cells): the parameters are spread over their range,
    both ends and the indices around every narrow top GL NQ - 1 among them; the handoff family
    for every GL of `gls` that has a narrow run; ordinary rows of 0 .. t + 1 errors.  Every
    tag carries the trace's L and handoff (tag_trace)."""
    nr, t = sm.nr, sm.t
    tops = sorted({narrow_top(nr, gl) for gl in gls} - {None})
    thin = t > 8
    around = [T + d for T in tops for d in (-1, 0, 1)]
    es = _spread(0, t, 6) if thin else None
    # (the singles S_j that a full-length row "corrects" in j + 1 > t places, see sparse(): past a narrow
    # top they are the rows whose success rests on the run after the hand-off)
    deep = [j for j in range(t, nr) if sm.nn % (j + 1) == 0]
    js = _spread(0, nr - 1, 8, around + deep + [t - 1, t]) if thin else None
    parts = []
    if t >= 2:
        parts.append(zero_run(sm, 1, seed, ks=_spread(1, t - 1, 5) if thin else None))
    parts += [late_discrepancy(sm, 1 if thin else 2, seed, es, js), sparse(sm, 2 if thin else 4, 16, seed, js),
              positions(sm, seed)]
    if full is not None and full.size > sm.size:
        parts.append(padding_roots(sm, full, seed, es=_spread(1, t, 6) if thin else None))
    done = set()
    for gl in gls:
        T = narrow_top(nr, gl)
        if T is not None and T not in done:
            done.add(T)
            parts.append(handoff(sm, gl, seed=seed))
    parts += [ordinary(sm, e, 6) for e in (_spread(0, t + 1, 8, (1, 2, t - 1, t)) if thin else range(t + 2))]
    pool = Pool.concat(parts)
    tag_trace(sm, pool, gls)
    return pool


def general_ne_range(sm, gls):
    """The erasure counts around the narrow run's conditions ne < GL and ne < 2 GL for each GL,
    0 .. 3, nr - 1 and nr, where the code and the row have them"""
    want = {0, 1, 2, 3, sm.nr - 1, sm.nr} | {x for gl in gls for x in (gl - 1, gl, 2 * gl - 1, 2 * gl)}
    return sorted(x for x in want if 0 <= x <= min(sm.nr, sm.width))


def _locator(sm, listed):
    """Coefficients (values, index 0 .. len(listed)) of the erasure locator prod (1 + X_l x), X_l =
    alpha^(prim (nn - 1 - (position + pad))), on the oracle's tables.  Like bm_trace: for choosing
    and tagging rows only."""
    alog, log, _ = sm.o.tables()
    nn = sm.nn
    lam = [1] + [0] * len(listed)
    for d, p in enumerate(listed):
        x = (sm.o.prim * (nn - 1 - (int(p) + sm.pad))) % nn
        for i in range(d + 1, 0, -1):
            if lam[i - 1]:
                lam[i] ^= int(alog[(int(log[lam[i - 1]]) + x) % nn])
    return lam


def errata_top_gap(sm, gls, draws=4, seed=0):
    """Lists of ne = GL NQ - 1 erased positions, for each narrow top of `gls`, whose locator has a
    zero at index ne - 1 and a nonzero at ne: the narrow run starts with B's top index set and the
    one below it clear, and must hand over before its first iteration.  The last position is
    solved for (the sum of the 1 / X_l vanishes).  Every erased symbol is damaged, with e = 1 ..
    errors elsewhere (ne + 2 e <= nr), so the locator grows past the top."""
    rng = _rng(sm, seed, "errata_top_gap")
    alog, log, _ = sm.o.tables()
    nn, nr, W = sm.nn, sm.nr, sm.width
    iprim = pow(int(sm.o.prim), -1, nn)
    spec = []
    for T in sorted({narrow_top(nr, gl) for gl in gls} - {None}):
        found = 0
        for _ in range(4000):
            if found == draws or T < 2 or T >= nr:
                break
            pos = [int(p) for p in rng.permutation(W)[:T - 1]]
            v = 0
            for p in pos:
                v ^= int(alog[(-sm.o.prim * (nn - 1 - (p + sm.pad))) % nn])
            if v == 0:
                continue
            last = (nn - 1 - (-int(log[v])) * iprim) % nn - sm.pad  # 1 / X_last = v
            if not 0 <= last < W or last in pos:
                continue
            listed = pos + [last]
            lam = _locator(sm, listed)
            assert lam[T] != 0 and lam[T - 1] == 0, (T, lam[T - 1:])
            e = 1 + found % max(1, min((nr - T) // 2, W - T))
            if T + 2 * e <= nr and T + e <= W:
                spec.append((T, listed, e))
                found += 1
    b = _Listed(sm, rng, "errata_top_gap", len(spec))
    for c, (T, listed, e) in enumerate(spec):
        b.damage(c, listed)
        extra = sm._scatter(rng, b.rows, c, e, avoid=listed)
        b.add(listed, positions=tuple(listed) + extra, ne=T, e=e, top=T)
    return b.done()


def general_errata_pool(sm, src, full=None, gls=(64,), seed=0):
    """errata_grid, idle_erasures, errata_outside, errata_repeats at the counts of
    general_ne_range, errata_top_gap, and count_zero of the rows `src` (an errors-only pool)"""
    nes = general_ne_range(sm, gls)
    parts = [errata_grid(sm, nes, seed=seed), idle_erasures(sm, nes, seed), errata_outside(sm, seed, nes),
             errata_repeats(sm, seed, nes), errata_top_gap(sm, gls, seed=seed), count_zero(sm, full, seed, src=src)]
    return Pool.concat([p for p in parts if len(p[2])])  # (errata_top_gap: none where no narrow top has room)


GENERAL_ERRATA_FAMILIES = ("errata_grid", "idle_erasures", "errata_outside", "errata_repeats", "count_zero")


def general_conditions(pool, want, sm, gls, excused=()):
    """Coverage of an errors-only general_pool, on the oracle's results and the tags alone;
    `excused` names what a code cannot meet (the tests give the reason with each):
      every family is there (padding_roots on a shortened size, handoff where some GL has nq >= 2)
      for each GL with nq >= 2: rows hand off at no fewer than 4 distinct r ("few_handoffs": the
        code has fewer than 4 iterations GL NQ .. nr, and rows at each of them), the earliest
        (GL NQ) and nr among them, and some of the rows that hand off succeed and some fail
        ("handoff_all_fail": GL NQ = nr, so a row hands off only when its first nr - 1
        syndromes vanish, and then L = nr > t)
      a shortened size has a padding_roots row refused with corrected_num 0 ("padding_fails")
    Returns what it saw, for the record."""
    ok, cor = want[0], want[1]
    fam = pool.families()
    need = {"late_discrepancy", "sparse", "positions", "ordinary"} | ({"zero_run"} if sm.t >= 2 else set())
    seen = {}
    for gl in gls:
        T = narrow_top(sm.nr, gl)
        if T is None:
            continue
        need.add("handoff")
        r = np.array([g.handoff[gl] for g in pool.tags])
        rs = sorted(set(r[r > 0].tolist()))
        assert rs and rs[0] == T + 1 and rs[-1] == sm.nr, (gl, rs)
        assert len(rs) >= 4 or ("few_handoffs" in excused and len(rs) == sm.nr - T), (gl, rs)
        if "handoff_all_fail" in excused:
            assert rs == [sm.nr] and not ok[r > 0].any(), (gl, rs)
        else:
            assert ok[r > 0].any() and not ok[r > 0].all(), \
                f"GL {gl}: the hand-off rows all {'succeed' if ok[r > 0].all() else 'fail'}"
        seen[f"handoff GL {gl}"] = (len(rs), int((r > 0).sum()), int(ok[r > 0].sum()))
    if sm.pad > 0:
        need.add("padding_roots")
        pr = fam == "padding_roots"
        assert "padding_fails" in excused or ((ok[pr] == 0) & (cor[pr] == 0)).any(), "no root-in-padding refusal"
    assert need <= set(fam), need - set(fam)
    return seen


def general_sizes(nn, nr):
    """full length, a shortened size with padding, and 1"""
    k = nn - nr
    return sorted({k, max(2, k // 3), 1}, reverse=True)


def general_case(o, size, full=None, excused=(), threads=8):
    """What the tests of the general kernels share for one (code, size): the errors-only pool
    with the oracle's decode and the rows' syndromes (log form), the pool of rows with lists
    (count_zero on every third row of the first) with the oracle's decode, and every
    condition on them (family_conditions, general_conditions, trace_conditions,
    errata_conditions; `excused`: the names a code is excused from), checked here."""
    from types import SimpleNamespace
    k = o.nn - o.nroots
    full = SyndromeMap(o, k) if full is None else full
    sm = full if size == k else SyndromeMap(o, size)
    gls = tuple(sorted({group_lanes(o.nn), 64}))
    pool = general_pool(sm, full, gls)
    want = o.decode_batch(pool.data, pool.parity, threads=threads)
    seen = family_conditions(pool, want, excused, nn=o.nn)
    seen.update(general_conditions(pool, want, sm, gls, excused))
    seen["traced"] = trace_conditions(pool, want)
    epool = general_errata_pool(sm, take(pool, np.arange(0, len(pool), 3)), full, gls)
    ewant = decode_lists(o, epool, threads=threads)
    eseen = errata_conditions(epool, ewant, sm, excused)
    assert "all_refused" in excused or set(eseen) == set(GENERAL_ERRATA_FAMILIES), set(eseen)
    # errata_top_gap: wherever a narrow top GL NQ - 1 leaves room for an error (GL NQ + 1 <= nr); corrected in full
    gap = epool.families() == "errata_top_gap"
    tops = {narrow_top(sm.nr, gl) for gl in gls} - {None}
    assert {g.top for g in epool.tags if g.family == "errata_top_gap"} == {T for T in tops if 2 <= T and T + 2 <= sm.nr}
    if "all_refused" not in excused:
        assert (ewant[0][gap] == 1).all() and (ewant[1][gap] == [g.ne + g.e for g in epool.tags if g.family == "errata_top_gap"]).all()
    eseen["errata_top_gap"] = int(gap.sum())
    assert set(epool.families()) - {"errata_top_gap"} == set(GENERAL_ERRATA_FAMILIES)
    syn = o.syndrome_batch(pool.data, pool.parity)[1]
    for a in (pool.data, pool.parity, epool.data, epool.parity, epool.slots, epool.counts, syn) + tuple(want) + tuple(ewant):
        a.setflags(write=False)
    return SimpleNamespace(o=o, sm=sm, size=size, gls=gls, pool=pool, want=want, syn=syn, seen=seen, epool=epool,
                           ewant=ewant, eseen=eseen)


# -- layouts --
def general_kinds(pool, want, gl):
    """The rows of an errors-only general_pool by what rsgw_decode_k<., gl> makes of them, from
    the tags and the oracle's results: name -> index array.  clean; e<n>: n ordinary errors
    (up to eight n, 1 and t among them); fail: dirty rows the oracle refuses that do
    not hand off; handoff<r>: rows whose narrow run stops at r (the earliest, the last and one
    between); handoff_fail: refused rows that hand off."""
    ok = want[0]
    t = pool.parity.shape[1] // 2
    e_of = np.array([g.e if g.family == "ordinary" else -1 for g in pool.tags])
    r = np.array([g.handoff.get(gl, 0) for g in pool.tags])
    kinds = {"clean": np.nonzero(e_of == 0)[0]}
    have = sorted(set(e_of[(e_of >= 1) & (e_of <= t)].tolist()))
    for e in [have[i] for i in _spread(0, len(have) - 1, 8)]:
        kinds[f"e{e}"] = np.nonzero(e_of == e)[0]
    dirty = (pool.data != pool.clean[:, :pool.data.shape[1]]).any(1) | (pool.parity != pool.clean[:, pool.data.shape[1]:]).any(1)
    kinds["fail"] = np.nonzero((ok == 0) & (r == 0) & dirty)[0]
    rs = sorted(set(r[r > 0].tolist()))
    for rr in [rs[i] for i in _spread(0, len(rs) - 1, 3)]:
        kinds[f"handoff{rr}"] = np.nonzero(r == rr)[0]
    if ((r > 0) & (ok == 0)).any():
        kinds["handoff_fail"] = np.nonzero((r > 0) & (ok == 0))[0]
    # handoff_wide: the oracle corrects more symbols than the narrow run has indices, so the row's
    # result rests on what the run on all slots does after the hand-off.  (Where a row that hands off
    # is corrected within the narrow indices, no discrepancy follows the hand-off; where it is refused,
    # it mostly is whatever became of the high coefficients.)
    T = narrow_top(pool.parity.shape[1], gl)
    if T is not None:
        kinds["handoff_wide"] = np.nonzero((r > 0) & (ok == 1) & (want[1] > T))[0]
    return {k: v for k, v in kinds.items() if len(v)}


def group_layout(pool, want, gl):
    """Batches in which the g = 64 // gl codewords of a wave, and the 256 // gl of a workgroup,
    are alike or all but one: for every kind of general_kinds in turn a whole workgroup of it;
    a workgroup of it with one codeword of the next kind at position 0, 1, half and the last;
    a wave of it; a wave of it with one codeword of the next kind at group 0, 1, g / 2 and
    g - 1.  (gl = 64: a wave is one codeword, and only the workgroups of four have a lone one.)
    The workgroups come first, so each starts a workgroup of the kernel; every piece is whole
    waves.  Returns the order and (name, start, length) of each piece."""
    g, wg = WAVE // gl, GW_WORKGROUP // gl
    kinds = general_kinds(pool, want, gl)
    names = list(kinds)
    out, pieces = [], []

    def piece(name, rows):
        pieces.append((name, sum(len(x) for x in out), len(rows)))
        out.append(rows)

    for width, label in ((wg, "workgroup"), (g, "wave")):
        for n, a in enumerate(names):
            piece(f"{label} of {a}", _fill(kinds[a], width, n))
            b = names[(n + 1) % len(names)]
            for k, at in enumerate(sorted({0, 1, width // 2, width - 1})):
                if width == 1:
                    continue
                rows = _fill(kinds[a], width, n + k + 1)
                rows[at] = kinds[b][k % len(kinds[b])]
                piece(f"{label} of {a}, {b} at {at}", rows)
    return np.concatenate(out), pieces


def pair_stride(count, cus):
    """The distance between the two codewords of a pass of rsgw_decode_k<., 64> (gw_grid: a
    grid of min(ceil(count / 4), 8 CUs) workgroups of four codewords)"""
    return min(-(-count // 4), 8 * cus) * 4


def pair_layout(pool, want, cus, reps=3):
    """A batch longer than one grid pass in which chosen codewords A and B share a wave
    (gw_decode_pair: rows e and e + stride): clean / dirty and dirty / clean; fail / ok and
    ok / fail; both at t errors; both clean; and where the code has a narrow run at GL 64,
    hand-off at rA != rB in both orders, hand-off in A alone and in B alone, a failing
    hand-off beside a correctable row and the reverse, and handoff_wide rows (general_kinds) as B
    beside an A that never hands off or does so later, and the reverse.  Ordinary rows everywhere else; the count
    is odd, so the last pass has rows without a partner.  Returns (order, stride, pairs), pairs:
    (name, e) of each chosen pair."""
    k = general_kinds(pool, want, 64)
    t = pool.parity.shape[1] // 2
    es = sorted(int(n[1:]) for n in k if n[0] == "e" and n[1:].isdigit())
    k["dirty"] = np.concatenate([k[f"e{e}"] for e in es])
    k["t"] = k[f"e{t}"]
    combos = [("clean", "dirty"), ("dirty", "clean"), ("t", "t"), ("clean", "clean")]
    if "fail" in k:  # (a code whose every dirty row the reference refuses has them under "dirty" too)
        combos += [("fail", "dirty"), ("dirty", "fail"), ("fail", "fail")]
    hs = sorted((int(n[7:]), n) for n in k if n.startswith("handoff") and n[7:].isdigit())
    if hs:
        quiet = np.array([r for r in k["dirty"] if pool.tags[r].handoff[64] == 0])
        assert len(quiet), "every dirty row hands off"
        k["quiet"] = quiet
        first, last = hs[0][1], hs[-1][1]
        combos += [(first, "quiet"), ("quiet", first), (last, "quiet"), ("quiet", last), (first, first)]
        if len(hs) > 1:
            combos += [(first, last), (last, first)]
            if len(hs) > 2:
                combos += [(hs[1][1], last), (first, hs[1][1])]
        if "handoff_fail" in k:
            combos += [("handoff_fail", "dirty"), ("dirty", "handoff_fail"), ("handoff_fail", last)]
        if "handoff_wide" in k:  # B alone hands off, or hands off first, and its result shows it
            combos += [("quiet", "handoff_wide"), ("handoff_wide", "quiet"), (last, "handoff_wide"), ("handoff_wide", last),
                       ("clean", "handoff_wide"), ("handoff_wide", "handoff_wide")]
    cap = pair_stride(1 << 30, cus)
    npairs = len(combos) * reps
    count = cap + npairs + 64 + (cap + npairs) % 2 + 1  # odd, and some filler rows have partners too
    stride = pair_stride(count, cus)
    assert stride == cap < count <= 2 * stride
    filler = pool.where(lambda g: g.family == "ordinary")
    order = _fill(filler, count)
    pairs = []
    for i, (a, b) in enumerate(combos * reps):
        e = 5 * i % npairs if npairs % 5 else i  # (scattered over the slots of the workgroups)
        order[e] = k[a][(i // len(combos)) % len(k[a])]
        order[e + stride] = k[b][(i // len(combos) + 1) % len(k[b])]
        pairs.append((f"{a} / {b}", e))
    return order, stride, pairs
