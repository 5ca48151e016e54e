"""The rows of tests/rs_syndrome_rows.py for the general kernels, on the CPU: symbols of 4
to 8 bits through the syndrome map, the hand-off family and its Berlekamp-Massey trace, the
group and pair layouts, and the oracle's decode of every row, list and external syndrome
vector against the compiled reference (tests/test_gpu_rs_general_chosen.py compares the
library with the oracle alone, on these same rows).
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import rs_syndrome_rows as R
from oracle import Oracle, Reference, reference_available
from test_oracle_golden import _assert_rows_equal, _reference_rows
from test_rs_syndrome_rows_cpu import CODES as BYTE_CODES
from test_rs_syndrome_rows_cpu import _reference_lists

# (symbol_size, field polynomial, fcr, prim, num_roots) -> the conditions the code is excused from
# (rs_syndrome_rows.family_conditions, general_conditions, errata_conditions), with the reason.
#
# A code has one symbol size and one root count, so it sits in exactly one cell (GL, nq) of
# rsgw_decode_k at 256 rows or more (GL from nn, nq = (nr + GL) // GL), and the sixteen cells
# GL 4 x nq 2 3 4, GL 8 16 32 x nq 1 2 >= 3, GL 64 x nq 1 2 3 4 need sixteen codes; the one whose
# exponents pass 2^16 makes seventeen.  Below 256 rows every code runs on GL 64 (nq 1, or 2 for
# the 100-root code of 127 symbols).
#
#   late_fails        t <= 5: one syndrome vector in a few dozen belongs to a locator of degree
#                     <= t with all its roots, so a late_discrepancy row is now and then
#                     "corrected" at full length (oracle and reference agree on it)
#   few_handoffs      the narrow run can stop at r = GL NQ .. nr alone, fewer than 4 iterations:
#                     1 for RS(15,11) (4 .. 4) and RS(15,7) (8 .. 8), 2 for the 33-root code of 63
#                     symbols (32, 33), 3 for the 130-root code (128 .. 130); rows at each are asked
#   handoff_all_fail  GL NQ = nr: B reaches index nr - 1 before the last iteration only when the
#                     first nr - 1 syndromes vanish, and then L = nr > t
#   all_refused       (fcr + nr - 1) prim 254 is far past 2^16: the reference's check of a correction
#                     multiplies in 16 bits and refuses every dirty row, corrected_num counted
CODES = {
    (4, 0x13, 0, 1, 4): ("late_fails", "few_handoffs", "handoff_all_fail"),  # GL 4, nq 2
    (4, 0x13, 1, 2, 8): ("late_fails", "few_handoffs", "handoff_all_fail"),  # GL 4, nq 3; prim 2
    (4, 0x13, 1, 1, 12): (),  # GL 4, nq 4
    (5, 0x25, 3, 1, 6): ("late_fails",),  # GL 8, nq 1; fcr 3
    (5, 0x25, 1, 1, 12): (),  # GL 8, nq 2
    (5, 0x25, 0, 1, 20): (),  # GL 8, nq 3; fcr 0
    (6, 0x43, 1, 1, 10): ("late_fails",),  # GL 16, nq 1
    (6, 0x43, 1, 1, 20): (),  # GL 16, nq 2
    (6, 0x43, 2, 1, 33): ("few_handoffs",),  # GL 16, nq 3
    (7, 0x89, 1, 1, 20): (),  # GL 32, nq 1
    (7, 0x89, 1, 1, 40): (),  # GL 32, nq 2
    (7, 0x89, 1, 3, 100): (),  # GL 32, nq 4 (GL 64 below 256 rows: nq 2); prim 3
    (8, 0x11D, 0, 1, 48): (),  # GL 64, nq 1, pairs
    (8, 0x11D, 2000, 37, 32): ("all_refused",),  # GL 64, nq 1, pairs; the syndromes' Horner path
    (8, 0x11D, 1, 1, 100): (),  # GL 64, nq 2, pairs
    (8, 0x11D, 1, 1, 130): ("few_handoffs",),  # GL 64, nq 3
    (8, 0x11D, 3, 1, 200): (),  # GL 64, nq 4
}


def _id(code):
    return "m{}-{:#x}-fcr{}-prim{}-nr{}".format(*code)


def _nn(code):
    return (1 << code[0]) - 1


def test_codes_cover_the_cells():
    """The cells (GL, nq) of the grouped kernel that the codes stand for, pair-eligible codes
    among them, a code whose exponents pass 2^16, prim != 1, fcr 0 and fcr > 1."""
    def cell(c):
        gl = R.group_lanes(_nn(c))
        return gl, min((c[4] + gl) // gl, 4 if gl in (4, 64) else 3)  # (GL 8, 16, 32: nq >= 3 is one cell)

    cells = [cell(c) for c in CODES]
    assert len(set(cells)) == len(CODES) - 1  # (two pair-eligible codes at GL 64, nq 1)
    assert set(cells) == {(4, 2), (4, 3), (4, 4), (8, 1), (8, 2), (8, 3), (16, 1), (16, 2), (16, 3), (32, 1), (32, 2), (32, 3),
                     (64, 1), (64, 2), (64, 3), (64, 4)}
    pair = [c for c in CODES if c[0] == 8 and 8 <= c[4] < 128]
    assert {(c[4] + 64) // 64 for c in pair} == {1, 2}
    assert any((c[2] + c[4] - 1) * c[3] + _nn(c) - 1 >= 65536 for c in CODES)
    assert {c[3] for c in CODES} > {1} and 0 in {c[2] for c in CODES} and any(c[2] > 1 for c in CODES)


# sha256 of the byte-symbol pools as the module built them while it took byte symbols alone
# (data, parity, slots, counts, clean rows and tags): generalising it must not move a byte.
BYTE_POOLS = {
    (8, 0x11D, 1, 1, 32): "7f4adf9073aca4dd47cfd4c91a9cced1331f70d6c24ee7174059f2737dc19670",
    (8, 0x11D, 0, 1, 32): "2b8ce1fd4b759ed61f401d0d95317eccdd2559338eeacaca04d2b1450bef3382",
    (8, 0x11D, 5, 7, 32): "5e76e675a8f0f856be36b845014c939ec3898961ec9d56fad372499d5fed0007",
    (8, 0x187, 5, 1, 31): "7746f508dcf93fd3616b4313dcafb3fa9288b48dae5835b8c279015d9a9aaf00",
    (8, 0x11D, 1, 1, 16): "2455cb2fbc0f9ef0353d3dd5a79fa03d289e248757b4f37fc17f259c3f72a8d3",
    (8, 0x11D, 3, 1, 8): "975f3b03c0aea8398b4f97d3c7eb3d13f454014fe62033f5c6c106a2caee29d3",
}


def _digest(pool):
    m = hashlib.sha256()
    for a in (pool.data, pool.parity, pool.slots, pool.counts, pool.clean):
        m.update(np.ascontiguousarray(a).tobytes())
    m.update(repr([(repr(t), t.positions, t.slots, t.count, t.idle) for t in pool.tags]).encode())
    return m.hexdigest()


@pytest.mark.parametrize("code", list(BYTE_CODES), ids=_id)
def test_byte_pools_unchanged(code):
    """The errors-only families, ordinary rows and (8 roots: every errata family) of the six
    byte-symbol codes at a shortened size: byte for byte what they were."""
    o = Oracle(*code)
    sm, full = R.SyndromeMap(o, {32: 101, 31: 61, 16: 150, 8: 37}[code[4]]), R.SyndromeMap(o, 255 - code[4])
    parts = [R.family_pool(sm, full, zero_run_draws=2)] + [R.ordinary(sm, e, 8) for e in range(sm.t + 2)]
    if code[4] == 8:
        parts.append(R.errata_pool(sm, full))
    assert _digest(R.Pool.concat(parts)) == BYTE_POOLS[code]


@pytest.mark.parametrize("code", [c for c in CODES if c[0] < 8], ids=_id)
def test_parity_for_round_trip_short_symbols(code):
    """The syndromes of parity_for(S) are S for symbols of m < 8 bits, on the zero row and on
    raw-byte base messages (junk above bit m), at every size; the parity it returns has no
    bit above m."""
    o = Oracle(*code)
    nr, nn = code[4], _nn(code)
    for size in R.general_sizes(nn, nr):
        sm = R.SyndromeMap(o, size)
        rng = np.random.default_rng([size, nr])
        S = rng.integers(0, nn + 1, (300, nr), dtype=np.uint8)
        S[0] = 0
        par = sm.parity_for(S)
        assert (par <= nn).all() and not par[0].any()
        assert (sm.syndromes(np.zeros((300, size), np.uint8), par) == S).all(), (code, size)
        rows, clean = sm.rows_for(rng, S)
        assert (clean[:, :size] > nn).any()
        assert not sm.syndromes(clean[:, :size], clean[:, size:]).any()
        assert (sm.syndromes(rows[:, :size], rows[:, size:]) == S).all(), (code, size)


def _reference_external(code, data, parity, syn):
    """poporon_decode of the compiled reference with external syndromes (log form), one row
    at a time through one handle, which reads its syndrome array at every call."""
    nr = code[4]
    r = Reference(*code, ext_syn=np.zeros(nr, np.uint16))
    d, p = data.copy(), parity.copy()
    ok, cor = np.zeros(len(d), np.uint8), np.zeros(len(d), np.uint32)
    syn = np.ascontiguousarray(syn, dtype=np.uint16)
    for c in range(len(d)):
        C.memmove(r._syn, syn[c].ctypes.data, 2 * nr)
        ok[c], cor[c], d[c], p[c] = r.decode(d[c], p[c])
    r.close()
    return ok, cor, d, p


def external_cases(pc):
    """Each pool row's syndromes (log form) with the row itself and with the clean codeword of
    the next row but one (unrelated to it): data, parity, syndromes and the oracle's results."""
    pool, size = pc.pool, pc.size
    other = np.roll(pool.clean, -2, axis=0)
    data = np.concatenate([pool.data, other[:, :size]])
    parity = np.concatenate([pool.parity, other[:, size:]])
    syn = np.concatenate([pc.syn, pc.syn])
    res = [pc.o.decode(data[c], parity[c], ext_syn=syn[c]) for c in range(len(data))]
    want = (np.array([x[0] for x in res], np.uint8), np.array([x[1] for x in res], np.uint32),
            np.array([x[2] for x in res]), np.array([x[3] for x in res]))
    return data, parity, syn, want


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built here")
@pytest.mark.parametrize("code", list(CODES), ids=_id)
def test_general_rows_oracle_vs_reference(code):
    """Every row of general_pool, every row and list of general_errata_pool and every external
    syndrome vector (with its own row and with an unrelated clean one), at full length, at a
    shortened size and at size 1: the oracle equals the compiled reference (bool,
    corrected_num, every byte), and the conditions hold on the oracle and the tags alone
    (general_case: every family present, hand-off rows at 4 or more iterations with the
    earliest and nr among them, successes and failures among them, a root-in-padding refusal
    on each shortened size, the trace's L equal to corrected_num on every corrected row)."""
    o = Oracle(*code)
    nn, nr = _nn(code), code[4]
    full = R.SyndromeMap(o, nn - nr)
    r, re = Reference(*code), Reference(*code, erasure=True)
    for size in R.general_sizes(nn, nr):
        pc = R.general_case(o, size, full, CODES[code])
        _assert_rows_equal((code, size), pc.want, _reference_rows(r, pc.pool.data, pc.pool.parity))
        _assert_rows_equal((code, size, "lists"), pc.ewant, _reference_lists(re, pc.epool))
        data, parity, syn, want = external_cases(pc)
        _assert_rows_equal((code, size, "external"), want, _reference_external(code, data, parity, syn))
        fam, efam = pc.pool.families(), pc.epool.families()
        print(f"\n[general rows] {_id(code)} size {size}: {len(pc.pool)} rows "
              f"{ {str(f): int((fam == f).sum()) for f in sorted(set(fam))} }, {pc.seen}; {len(pc.epool)} rows with lists "
              f"{ {str(f): int((efam == f).sum()) for f in sorted(set(efam))} }, counts {R.general_ne_range(pc.sm, pc.gls)}; "
              f"external {len(data)} ({int(want[0].sum())} ok)")
    r.close()
    re.close()


def test_general_layouts():
    """group_layout and pair_layout on the 40-root code of 127 symbols and the 100-root byte
    code: what each wave, workgroup and pair holds."""
    code = (7, 0x89, 1, 1, 40)
    o = Oracle(*code)
    pc = R.general_case(o, 87, None, CODES[code])
    pool, want = pc.pool, pc.want
    for gl in (32, 64):
        g, wg = 64 // gl, 256 // gl
        kinds = R.general_kinds(pool, want, gl)
        assert {"clean", "e1", "e20", "fail"} <= set(kinds)
        assert ("handoff32" in kinds and "handoff40" in kinds and "handoff_fail" in kinds) == (gl == 32)
        member = {name: set(idx.tolist()) for name, idx in kinds.items()}
        order, pieces = R.group_layout(pool, want, gl)
        assert sum(n for _, _, n in pieces) == len(order) and len(order) % g == 0
        lone = 0
        for name, start, n in pieces:
            rows = order[start:start + n]
            assert n == (wg if name.startswith("workgroup") else g) and start % n == 0, (name, start, n)
            a = name.split(" of ")[1].split(",")[0]
            if "," in name:
                b, at = name.split(", ")[1].split(" at ")
                assert rows[int(at)] in member[b] and all(x in member[a] for x in np.delete(rows, int(at))), name
                lone += 1
            else:
                assert all(x in member[a] for x in rows), name
        assert lone == len(kinds) * sum(len({0, 1, w // 2, w - 1}) for w in (wg, g) if w > 1)
    code = (8, 0x11D, 1, 1, 100)
    o = Oracle(*code)
    pc = R.general_case(o, 155, None, CODES[code])  # (full length: the singles S_84 corrected in 85 places)
    order, stride, pairs = R.pair_layout(pc.pool, pc.want, cus=256)
    assert stride == 8192 == R.pair_stride(len(order), 256) and stride < len(order) <= 20000 and len(order) % 2 == 1
    assert R.pair_stride(300, 256) == 300 and R.pair_stride(301, 256) == 304 and R.pair_stride(10 ** 6, 64) == 2048
    kinds = R.general_kinds(pc.pool, pc.want, 64)
    names = {n for n, _ in pairs}
    assert {"clean / dirty", "dirty / clean", "fail / dirty", "dirty / fail", "t / t", "handoff64 / handoff100",
            "handoff100 / handoff64", "handoff64 / quiet", "quiet / handoff64", "handoff_fail / dirty",
            "dirty / handoff_fail", "quiet / handoff_wide", "handoff_wide / quiet", "handoff100 / handoff_wide"} <= names
    wide = kinds["handoff_wide"]
    assert len(wide) >= 3 and (pc.want[1][wide] == 85).all()
    r64 = np.array([g.handoff[64] for g in pc.pool.tags])
    for name, e in pairs:
        a, b = name.split(" / ")
        assert e + stride < len(order)
        for kind, row in ((a, order[e]), (b, order[e + stride])):
            if kind in kinds:
                assert row in kinds[kind], (name, e)
            if kind.startswith("handoff") and kind[7:].isdigit():
                assert r64[row] == int(kind[7:])
            if kind == "quiet":
                assert r64[row] == 0 and pc.want[0][row] == 1
    assert len({e for _, e in pairs}) == len(pairs)
