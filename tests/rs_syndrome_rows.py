"""Reed-Solomon rows built from chosen syndromes, and batch layouts with chosen waves.

A helper module of the tests (not a conftest, no fixtures).  It does no field
arithmetic of its own: everything comes from the CPU oracle (oracle/rs_oracle.c)
and from linear algebra over GF(2) on what the oracle answers.

The map from the nr parity bytes of a row to its nr syndrome values is
GF(2)-linear, and invertible whenever the code's roots are distinct.
SyndromeMap reads its 8 nr x 8 nr bit matrix off the oracle's syndromes of the
8 nr one-bit parity perturbations of the all-zero row, inverts it, and so turns
any wanted syndrome vector S into the row [base | encode(base) ^ parity_for(S)].
The same idea on a set of byte positions gives error patterns whose first k
syndromes vanish (SyndromeMap.vanishing).

The families below are rows that random error patterns produce once in 256
steps of Berlekamp-Massey or never: runs of zero discrepancies, a late jump of
L, locators that would pass x^t, sparse syndromes, roots in the padding of a
shortened row, every error position.  The layouts order a pool of rows so that
whole waves of 64 rows (and whole workgroups of 512) are alike, or differ in
one lane.  Everything is seeded; every row stands on a random base message.

The errata_* families further down are rows with erasure lists (a row of nr slot bytes,
a count, stale bytes after it) for the errata kernels, with their own conditions
(errata_conditions) and layouts (uniform_ne, lone_ne, degree_brackets, bp_mixes).
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


def _bits(b):
    """(count, n) bytes -> (count, 8 n) bits"""
    return np.unpackbits(np.ascontiguousarray(b, dtype=np.uint8), axis=1)


def _bytes(x):
    return np.packbits(x.astype(np.uint8), axis=1)


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
        assert oracle.m == 8, "byte symbols"
        self.t = self.nr // 2
        self.width = size + self.nr
        self.pad = oracle.nn - self.nr - size  # the zero symbols a shortened row stands for
        self.alog = oracle.tables()[0]
        nb = 8 * self.nr
        par = _bytes(np.eye(nb, dtype=np.uint8))  # the 8 nr one-bit parity perturbations
        self.matrix = _bits(self.syndromes(np.zeros((nb, size), np.uint8), par))  # parity bits -> syndrome bits
        self.inverse = gf2_inverse(self.matrix)

    # -- syndromes as values (the oracle gives logs) --
    def syndromes(self, data, parity):
        """(count, nr) syndrome values of the rows"""
        _, syn = self.o.syndrome_batch(data, parity)
        return self.alog[syn].astype(np.uint8)

    def parity_for(self, S):
        """(count, nr) parity deltas whose syndromes (on zero data) are the value vectors S"""
        S = np.atleast_2d(np.asarray(S, dtype=np.uint8))
        return _bytes(_mul(_bits(S), self.inverse))

    def vanishing(self, positions, k):
        """Basis of the GF(2) null space of "values at these byte positions -> S_0 .. S_(k-1)":
        (8 (w - k), 8 w) bits, w = len(positions); byte i of a member goes to positions[i]."""
        w = len(positions)
        unit = _bytes(np.eye(8 * w, dtype=np.uint8))
        rows = np.zeros((8 * w, self.width), np.uint8)
        for i, p in enumerate(positions):
            rows[:, p] = unit[:, i]
        syn = self.syndromes(rows[:, :self.size], rows[:, self.size:])
        basis = gf2_left_null_space(_bits(syn[:, :k]))
        assert basis.shape == (8 * max(w - k, 0), 8 * w), (basis.shape, w, k)
        return basis

    def vanishing_pattern(self, rng, positions, k):
        """A random null-space member with every byte nonzero: an error pattern of weight w
        whose first k syndromes are zero (w >= k + 1)."""
        basis = self.vanishing(positions, k)
        for _ in range(1000):
            v = _bytes(_mul(rng.integers(0, 2, (1, basis.shape[0])), basis))[0]
            if v.all():
                return v
        raise AssertionError("no full-weight pattern found")

    # -- rows --
    def base_rows(self, rng, n):
        data = rng.integers(0, 256, (n, self.size), dtype=np.uint8)
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
        rows[c, pos] ^= rng.integers(1, 256, pos.size, dtype=np.uint8)
        return tuple(int(p) for p in pos)

    # -- the order of the reference's root search --
    def visit(self, pos):
        """When the reference's root search meets byte position pos of the row: it tries
        the points i = 1 .. 255 in turn, and point i stands for location (i iprim - 1) mod
        255, so location k = pos + pad is met at i = (k + 1) prim mod 255 (0 read as 255).
        Returned as i - 1, 0 .. 254.  Integer arithmetic on exponents, no field arithmetic;
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
        """The position whose root the reference tries last (its point i = 255), found from
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
    val = rng.integers(1, 256, (n, e_row), dtype=np.uint8)
    np.put_along_axis(rows, pos, np.take_along_axis(rows, pos, 1) ^ val, 1)
    return sm._split(rows, [Tag("ordinary", tuple(int(p) for p in pos[c]), e=e) for c in range(n)], clean)


def zero_run(sm, draws=1, seed=0):
    """For every k in 1 .. t-1 and w in k+1 .. t: a vanishing pattern of weight w and a
    ordinary errors elsewhere, a <= min(t - w, k // 2).  Correctable; Berlekamp-Massey
    sees k - 2a zero discrepancies in a row and then lengthens by more than one."""
    rng = _rng(sm, seed, "zero_run")
    t = sm.t
    combos = [(k, w) for k in range(1, t) for w in range(k + 1, t + 1) if w <= sm.width] * draws
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


def late_discrepancy(sm, draws=3, seed=0):
    """e ordinary errors, e in 0 .. t, then a nonzero value XORed into one syndrome S_j,
    for every j: L jumps to j + 1 - e late, with B shifted many times."""
    rng = _rng(sm, seed, "late_discrepancy")
    t, nr = sm.t, sm.nr
    combos = [(e, j) for e in range(t + 1) for j in range(nr)] * draws
    n = len(combos)
    clean = sm.base_rows(rng, n)
    rows = clean.copy()
    S = np.zeros((n, nr), np.uint8)
    tags = []
    for c, (e, j) in enumerate(combos):
        pos = sm._scatter(rng, rows, c, min(e, sm.width))
        S[c, j] = rng.integers(1, 256)
        tags.append(Tag("late_discrepancy", pos, e=e, j=j))
    rows[:, sm.size:] ^= sm.parity_for(S)
    return sm._split(rows, tags, clean)


def sparse(sm, values=4, pairs=48, seed=0):
    """Exactly one nonzero syndrome S_j for every j (`values` values each), and exactly
    two for a seeded set of pairs.  A single S_j = d with j >= t leaves the locator
    1 + d' x^(j+1): j = t - 1 gives 1 + d' x^t, and where j + 1 divides 255 (17 for 32
    roots, 15 for 16, 5 for 8) the locator has j + 1 > t roots for one d in j + 1; the
    reference then "corrects" j + 1 symbols of a full-length row.  Those j get every d."""
    rng = _rng(sm, seed, "sparse")
    nr = sm.nr
    S, tags = [], []
    for j in range(nr):
        every = j + 1 > sm.t and 255 % (j + 1) == 0
        for v in rng.permutation(np.arange(1, 256))[:255 if every else values]:
            s = np.zeros(nr, np.uint8)
            s[j] = v
            S.append(s)
            tags.append(Tag("sparse", None, j=j))
    for _ in range(pairs):
        i, j = sorted(int(x) for x in rng.permutation(nr)[:2])
        s = np.zeros(nr, np.uint8)
        s[i], s[j] = rng.integers(1, 256, 2)
        S.append(s)
        tags.append(Tag("sparse", None, i=i, j=j))
    rows, clean = sm.rows_for(rng, np.array(S))
    return sm._split(rows, tags, clean)


def padding_roots(sm, full, seed=0):
    """Shortened sizes: the syndromes of e errors, e in 1 .. t, on the full-length code
    (`full`: the SyndromeMap of size k), 1 .. e of them inside the padding, transplanted
    onto the short row.  The locator is valid and all its roots are found, but a location
    lies before the row."""
    rng = _rng(sm, seed, "padding_roots")
    pad = full.size - sm.size
    assert pad > 0 and full.nr == sm.nr
    combos = [(e, p) for e in range(1, sm.t + 1) for p in range(1, e + 1) if p <= pad and e - p <= sm.width]
    err = np.zeros((len(combos), full.width), np.uint8)
    tags = []
    for c, (e, p) in enumerate(combos):
        pos = np.concatenate([rng.permutation(pad)[:p], pad + rng.permutation(sm.width)[:e - p]])
        err[c, pos] = rng.integers(1, 256, e, dtype=np.uint8)
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
        rows[p, p] ^= rng.integers(1, 256)
        tags.append(Tag("positions", (p,), at=p, run=1))
    for s in range(W - t + 1):
        rows[W + s, s:s + t] ^= rng.integers(1, 256, t, dtype=np.uint8)
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
def family_conditions(pool, want, relaxed=()):
    """pool: rows and tags; want: Oracle.decode_batch of them.  `relaxed` names the
    conditions a code is excused from (see the codes' entries in the tests):
      "late_fails"     no late_discrepancy row with e > 0 succeeds (e = 0 is a sparse single)
      "late_counted"   at least one late_discrepancy failure has corrected_num > 0
      "sparse_zero"    a sparse single S_j fails with corrected_num == 0, or j + 1 > t divides
                       255 and it succeeds with corrected_num == j + 1 (see sparse())
      "padding_fails"  padding_roots rows fail with corrected_num == 0
    Returns the counts it looked at, for the record."""
    ok, cor, od, op = want
    fam = pool.families()
    failed = ok == 0
    assert (od[failed] == pool.data[failed]).all() and (op[failed] == pool.parity[failed]).all(), \
        "a failed row was modified"
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
        full = single & (ok == 1) & (cor == j1) & (j1 > tt) & (255 % np.maximum(j1, 1) == 0)
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
        self.rows[c, pos] ^= self.rng.integers(1, 256, pos.size, dtype=np.uint8)

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
        S[c, j] = rng.integers(1, 256)
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
        S[c, j] = rng.integers(1, 256)
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
        err[c, at] = rng.integers(1, 256, e, dtype=np.uint8)
        b.damage(c, era)
        b.add(_ordered(era, ORDERS[c % 3]), positions=tuple(era) + tuple(inside), ne=ne, e=e, inside=p)
    b.rows[:, sm.size:] ^= sm.parity_for(full.syndromes(err[:, :full.size], err[:, full.size:]))
    return b.done()


def errata_outside(sm, seed=0):
    """A slot past the codeword, size + nr or 255, in threes on one damaged row (ne erasures
    and e errors, ne + e < nr): the plain list; the list with that slot counted besides;
    the plain list with that value in the last stale slot, which no magnitude reaches."""
    rng = _rng(sm, seed, "errata_outside")
    nr, W = sm.nr, sm.width
    spec = [(ne, out) for ne in _ne_range(sm, range(nr)) for out in sorted({W, 255})]
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


def errata_repeats(sm, seed=0):
    """A slot counted twice, next to itself and apart; a counted slot repeated in the first
    stale slot; nr slots ascending but for one pair of equal neighbours, at every index."""
    rng = _rng(sm, seed, "errata_repeats")
    nr, W = sm.nr, sm.width
    spec = [(kind, ne, 0) for ne in _ne_range(sm, None, 2) for kind in ("adjacent", "apart", "stale")
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


def count_zero(sm, full=None, seed=0):
    """The rows of the errors-only family_pool under the erasure mode with count 0 and junk
    in the stale slots (quirk Q3: the magnitudes go to the stale slots)."""
    rng = _rng(sm, seed, "count_zero")
    src = family_pool(sm, full, seed=seed)
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
    Returns the counts it looked at, for the record."""
    ok, cor, od, op = want
    fam = pool.families()
    nr = pool.parity.shape[1]
    size = pool.data.shape[1]
    failed = ok == 0
    assert (od[failed] == pool.data[failed]).all() and (op[failed] == pool.parity[failed]).all(), \
        "a failed row was modified"
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
