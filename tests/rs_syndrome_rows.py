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
    [base | encode(base)] that the row was built on (set by the family)."""
    __slots__ = ("family", "params", "positions", "base")

    def __init__(self, family, positions=None, **params):
        self.family, self.params, self.positions, self.base = family, params, positions, None

    def __getattr__(self, name):
        try:
            return self.params[name]
        except KeyError:
            raise AttributeError(name) from None

    def __repr__(self):
        return self.family + "(" + ", ".join(f"{k}={v}" for k, v in self.params.items()) + ")"


class Pool:
    """Rows of one (code, size): data (count, size), parity (count, nr), a Tag each;
    clean (count, size + nr): the codewords [base | encode(base)] the rows were built on."""

    def __init__(self, data, parity, tags):
        assert len(data) == len(parity) == len(tags)
        self.data, self.parity, self.tags = data, parity, list(tags)
        self.clean = np.array([t.base for t in self.tags], np.uint8).reshape(len(self.tags), -1)
        assert self.clean.shape == (len(self.tags), data.shape[1] + parity.shape[1])

    def __len__(self):
        return len(self.tags)

    @staticmethod
    def concat(parts):
        parts = [p if isinstance(p, Pool) else Pool(*p) for p in parts]
        return Pool(np.concatenate([p.data for p in parts]), np.concatenate([p.parity for p in parts]),
                    [t for p in parts for t in p.tags])

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
