"""Wire forms without a GPU (poporon_amd_set_wire_form, include/poporon_amd.h): the CCSDS
tables from their definitions, in numpy (libpoporon_amd.ccsds_*) and in the library, the
argument checks of set and get, and the numpy model the GPU tests compare with
(tests/wire_ref.py)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import libpoporon_amd as P
import interleave_ref as R
import wire_ref as W

CCSDS = (8, 0x187, 112, 11, 32)


def _perm(seed):
    """a random bijection of the bytes that is not GF(2)-linear, and its inverse"""
    to_code = np.random.default_rng(seed).permutation(256).astype(np.uint8)
    to_wire = np.zeros(256, np.uint8)
    to_wire[to_code] = np.arange(256, dtype=np.uint8)
    return to_code, to_wire


def _raw_get(h):
    lib = P.load_library()
    tc, tw, seq = np.full(256, 0xA5, np.uint8), np.full(256, 0xA5, np.uint8), np.full(65536, 0xA5, np.uint8)
    n = C.c_size_t(12345)
    ok = lib.poporon_amd_get_wire_form(h.h, tc.ctypes.data, tw.ctypes.data, seq.ctypes.data, seq.size, C.byref(n))
    return ok, tc, tw, seq, n.value


# ---- the CCSDS tables -------------------------------------------------------------------

def test_dual_basis_from_the_definition():
    to_code, to_wire = P.ccsds_dual_basis()
    assert to_wire.dtype == np.uint8 and to_wire.shape == (256,)
    assert sorted(to_wire.tolist()) == list(range(256))
    v = np.arange(256)
    assert (to_code[to_wire] == v).all() and (to_wire[to_code] == v).all()
    a, b = np.meshgrid(v, v)
    assert (to_wire[a ^ b] == to_wire[a] ^ to_wire[b]).all()  # GF(2)-linear
    assert to_wire[[1, 2, 4, 8, 16, 32]].tolist() == [0x7B, 0xAF, 0x99, 0xFA, 0x86, 0xEC]
    assert zlib.crc32(to_wire.tobytes()) == 2066307702


def test_randomizer_from_the_definition():
    seq = P.ccsds_randomizer()
    assert seq.dtype == np.uint8 and seq.shape == (255,)
    assert seq[:10].tobytes() == bytes.fromhex("FF480EC09A0D70BC8E2C")
    assert zlib.crc32(seq.tobytes()) == 3426211836
    bits = np.unpackbits(seq)
    # one period of a maximal-length sequence of degree 8: 255 bits, repeated 8 times in 255 bytes
    assert (bits == np.tile(bits[:255], 8)).all()
    assert all((np.roll(bits[:255], -p) != bits[:255]).any() for p in range(1, 255))
    assert bits[:255].sum() == 128


def test_library_builds_the_same_tables():
    h = P.Poporon(*CCSDS)
    to_code, to_wire = P.ccsds_dual_basis()
    seq = P.ccsds_randomizer()
    ident = np.arange(256, dtype=np.uint8)
    for dual, rand in ((True, True), (True, False), (False, True)):
        h.set_wire_form_ccsds(dual, rand)
        tc, tw, s = h.wire_form()
        assert (tc == (to_code if dual else ident)).all() and (tw == (to_wire if dual else ident)).all()
        assert s.tobytes() == (seq.tobytes() if rand else b"")
    h.set_wire_form_ccsds(False, False)  # neither: cleared
    assert h.wire_form() is None
    # any symbol_size 8 handle takes them
    g = P.Poporon.default()
    g.set_wire_form_ccsds()
    assert (g.wire_form()[1] == to_wire).all()


# ---- set and get ------------------------------------------------------------------------

def test_set_get_set_get():
    h = P.Poporon.default()
    assert h.wire_form() is None
    ok, tc, tw, seq, n = _raw_get(h)
    assert ok is False and "no wire form" in P.last_error()
    assert (tc == 0xA5).all() and (seq == 0xA5).all() and n == 12345  # nothing written
    to_code, to_wire = _perm(1)
    s1 = np.random.default_rng(2).integers(0, 256, 65536, dtype=np.uint8)
    h.set_wire_form(to_code, to_wire, s1)
    tc, tw, s = h.wire_form()
    assert (tc == to_code).all() and (tw == to_wire).all() and (s == s1).all()
    # the tables were copied: the caller's arrays may change
    to_code[:] = 0
    s1[:] = 0
    assert h.wire_form()[0].any() and h.wire_form()[2].any()
    # a sequence alone: the maps come back as the identity
    h.set_wire_form(xor_seq=[7])
    tc, tw, s = h.wire_form()
    assert (tc == np.arange(256)).all() and (tw == np.arange(256)).all() and s.tolist() == [7]
    # a map alone: xor_len 0 and no sequence byte written
    to_code, to_wire = _perm(3)
    h.set_wire_form(to_code, to_wire)
    ok, tc, tw, seq, n = _raw_get(h)
    assert ok is True and n == 0 and (tc == to_code).all() and (tw == to_wire).all() and (seq == 0xA5).all()
    h.set_wire_form()
    assert h.wire_form() is None


def test_getter_pointers_are_optional():
    lib = P.load_library()
    h = P.Poporon.default()
    h.set_wire_form(xor_seq=np.arange(9))
    n = C.c_size_t(0)
    assert lib.poporon_amd_get_wire_form(h.h, None, None, None, 0, C.byref(n)) is True and n.value == 9
    assert lib.poporon_amd_get_wire_form(h.h, None, None, None, 0, None) is True
    buf = np.zeros(16, np.uint8)
    n = C.c_size_t(0)
    assert lib.poporon_amd_get_wire_form(h.h, None, None, buf.ctypes.data, 8, C.byref(n)) is False
    assert n.value == 9 and "xor_cap" in P.last_error() and not buf.any()
    assert lib.poporon_amd_get_wire_form(h.h, None, None, buf.ctypes.data, 9, None) is True
    assert buf.tolist() == list(range(9)) + [0] * 7


def test_bad_arguments_leave_the_form():
    lib = P.load_library()
    h = P.Poporon.default()
    to_code, to_wire = _perm(4)
    h.set_wire_form(to_code, to_wire, [1, 2, 3])
    seq = np.zeros(65537, np.uint8)
    ident = np.arange(256, dtype=np.uint8)
    broken = to_wire.copy()
    broken[[5, 9]] = broken[[9, 5]]
    p = lambda a: a.ctypes.data
    for args, word in (((p(to_code), p(broken), None, 0), "inverse"),
                       ((p(ident), p(np.zeros(256, np.uint8)), None, 0), "inverse"),
                       ((p(to_code), None, None, 0), "both"),
                       ((None, p(to_wire), None, 0), "both"),
                       ((None, None, p(seq), 0), "xor_len"),
                       ((None, None, None, 5), "xor_len"),
                       ((None, None, p(seq), 65537), "xor_len")):
        assert lib.poporon_amd_set_wire_form(h.h, *args) is False, word
        assert word in P.last_error(), (word, P.last_error())
    tc, tw, s = h.wire_form()
    assert (tc == to_code).all() and (tw == to_wire).all() and s.tolist() == [1, 2, 3]
    assert lib.poporon_amd_set_wire_form(h.h, None, None, p(seq), 65536) is True
    assert h.wire_form()[2].size == 65536


def test_handles_that_take_no_wire_form():
    lib = P.load_library()
    buf = np.zeros(256, np.uint8)
    n = C.c_size_t(0)
    for h, word in ((P.Bch.default(), "RS handles"), (P.Ldpc(128, P.LDPC_RATE_1_2), "RS handles"),
                    (P.Poporon(4, 0x13, 1, 1, 8), "symbol_size")):
        for call in (lambda: lib.poporon_amd_set_wire_form(h.h, None, None, buf.ctypes.data, 4),
                     lambda: lib.poporon_amd_set_wire_form(h.h, None, None, None, 0),
                     lambda: lib.poporon_amd_set_wire_form_ccsds(h.h, True, True),
                     lambda: lib.poporon_amd_get_wire_form(h.h, None, None, None, 0, C.byref(n))):
            assert call() is False
            assert word in P.last_error(), P.last_error()
    assert lib.poporon_amd_set_wire_form(None, None, None, None, 0) is False and "NULL" in P.last_error()
    assert lib.poporon_amd_set_wire_form_ccsds(None, True, True) is False and "NULL" in P.last_error()
    assert lib.poporon_amd_get_wire_form(None, None, None, None, 0, None) is False and "NULL" in P.last_error()


def test_python_wrapper_refuses_short_maps():
    h = P.Poporon.default()
    with pytest.raises(P.PoporonError):
        h.set_wire_form(np.arange(255), np.arange(255))
    with pytest.raises(P.PoporonError):
        h.set_wire_form(np.arange(256))  # one map without the other


def test_header_declares_the_three_calls():
    names = P.header_symbols()
    lib = P.load_library()
    for n in ("poporon_amd_set_wire_form", "poporon_amd_set_wire_form_ccsds", "poporon_amd_get_wire_form"):
        assert n in names and hasattr(lib, n) and n in P._SIGS


# ---- the numpy model --------------------------------------------------------------------

def test_model_maps_are_inverses_and_place_the_sequence():
    rng = np.random.default_rng(5)
    to_code, to_wire = _perm(6)
    for depth, size, nr in ((1, 223, 32), (5, 222, 32), (8, 1, 16), (3, 2, 100)):
        d = rng.integers(0, 256, (3, size * depth), dtype=np.uint8)
        p = rng.integers(0, 256, (3, nr * depth), dtype=np.uint8)
        for seq in (None, rng.integers(0, 256, 7, dtype=np.uint8), rng.integers(0, 256, 65536, dtype=np.uint8)):
            cd, cp = W.to_code_frames(d, p, depth, to_code, seq)
            wd, wp = W.to_wire_frames(cd, cp, depth, to_wire, seq)
            assert (wd == d).all() and (wp == p).all()
            # byte by byte from the definition: the block offset of a parity byte starts at size*depth
            block, code = np.concatenate([d, p], 1), np.concatenate([cd, cp], 1)
            for b in (0, 1, size * depth - 1, size * depth, block.shape[1] - 1):
                x = 0 if seq is None else int(seq[b % len(seq)])
                assert (code[:, b] == to_code[block[:, b] ^ x]).all()


class _XorOracle:
    """stands in for the oracle: 'parity' is the message's first bytes XOR 0x3C, a 'decode' clears byte 0"""

    def encode_batch(self, rows, threads=0):
        return rows[:, :2] ^ 0x3C

    def decode_batch(self, d, p, *pos, threads=0):
        dd = d.copy()
        dd[:, 0] = 0
        return np.ones(len(d), np.uint8), np.ones(len(d), np.uint32), dd, p.copy()

    def syndrome_batch(self, d, p):
        return [(d[:, 0] != 0).astype(np.uint8)]


def test_model_with_no_form_is_the_interleaved_model():
    rng = np.random.default_rng(7)
    o = _XorOracle()
    ident = np.arange(256, dtype=np.uint8)
    for depth in (1, 4, 5):
        d = rng.integers(0, 256, (6, 9 * depth), dtype=np.uint8)
        p = rng.integers(0, 256, (6, 2 * depth), dtype=np.uint8)
        for tc, tw in ((None, None), (ident, ident)):
            assert (W.expect_encode(o, d, depth, tc, tw) == R.expect_encode(o, d, depth)).all()
            got, want = W.expect_decode(o, d, p, depth, tc, tw, None), R.expect_decode(o, d, p, depth)
            assert all((a == b).all() for a, b in zip(got[:4], want))
            assert (W.expect_check(o, d, p, depth, tc, None) == R.expect_check(o, d, p, depth)).all()


def test_model_decode_is_derandomized_and_in_wire_symbols():
    rng = np.random.default_rng(8)
    o = _XorOracle()
    to_code, to_wire = _perm(9)
    seq = rng.integers(0, 256, 255, dtype=np.uint8)
    depth = 3
    d = rng.integers(0, 256, (4, 9 * depth), dtype=np.uint8)
    p = rng.integers(0, 256, (4, 2 * depth), dtype=np.uint8)
    ok, cor, wd, wp, (cd, cp), (dd, pp) = W.expect_decode(o, d, p, depth, to_code, to_wire, seq)
    assert (to_code[wd] == dd).all() and (to_code[wp] == pp).all()
    # the parity the stand-in left alone comes back derandomized, not as received
    assert (wp == p ^ W._seq_at(seq, 9 * depth, 2 * depth)).all()
    assert (dd[:, :depth] == 0).all() and (dd[:, depth:] == cd[:, depth:]).all()
