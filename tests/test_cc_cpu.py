"""The K = 7 convolutional code without a GPU (include/poporon_amd.h): the numpy model of tests/cc_ref.py
held to things it did not define itself (the impulse response of 171/133, noise-free frames, a brute-force
search over every message of short terminated frames, windows wider than the frame), then the library's
poporon_amd_cc_symbols / poporon_amd_cc_blocks against the definitions, every argument check of create
and of both calls (none of them reaches the GPU), and the count-0 return."""
import itertools

import numpy as np
import pytest

import libpoporon_amd as P
import cc_ref as R

X = 0x1000  # a non-NULL pointer that is never dereferenced
PUNCTURES = (R.RATE_1_2, R.DVB_2_3, R.DVB_3_4, R.DVB_5_6, R.DVB_7_8)


# ---- the model -------------------------------------------------------------------------------

def test_impulse_response_of_171_133():
    sym, end = R.encode(R.DVB, R.RATE_1_2, [1, 0, 0, 0, 0, 0, 0], 0)
    assert "".join(map(str, sym[0::2])) == "1111001" and "".join(map(str, sym[1::2])) == "1011011"
    assert end == 0
    inv, _ = R.encode(R.CCSDS, R.RATE_1_2, [1, 0, 0, 0, 0, 0, 0], 0)
    assert (inv[0::2] == sym[0::2]).all() and (inv[1::2] == 1 - sym[1::2]).all()  # CCSDS inverts output 1


def test_the_array_encoder_is_the_step_by_step_one():
    rng = np.random.default_rng(3)
    sym, end = R.encode_literal(R.DVB, R.RATE_1_2, [1, 0, 0, 0, 0, 0, 0], 0)
    assert "".join(map(str, sym[0::2])) == "1111001" and "".join(map(str, sym[1::2])) == "1011011" and end == 0
    for code in (R.DVB, R.CCSDS, (0o171, 0o132, 1), (1, 0o100, 3)):
        for punct in PUNCTURES + ((16, 0b1010000010010110, 0b0110000011010001),):
            for n in (1, 3, 6, 7, 50):
                msg = rng.integers(0, 2, n)
                start = int(rng.integers(64))
                a, b = R.encode(code, punct, msg, start), R.encode_literal(code, punct, msg, start)
                assert a[0].tolist() == b[0].tolist() and a[1] == b[1] and len(a[0]) == R.n_symbols(punct, n)


def test_the_library_constants_are_the_models():
    assert (P.CC_CODE_CCSDS, P.CC_CODE_DVB) == (R.CCSDS, R.DVB)
    assert (P.CC_PUNCTURE_NONE, P.CC_PUNCTURE_DVB_2_3, P.CC_PUNCTURE_DVB_3_4, P.CC_PUNCTURE_DVB_5_6,
            P.CC_PUNCTURE_DVB_7_8) == PUNCTURES


def test_packing_is_msb_first():
    assert R.pack([1, 0, 0, 0, 0, 0, 0, 0, 1, 1]).tolist() == [0x80, 0xC0]
    assert R.unpack([0x80, 0xC0], 10).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("code", [R.DVB, R.CCSDS])
def test_noise_free_frames_decode_to_the_message(code):
    # unknown start and end: both polynomials tap the oldest bit, so the state's every bit shows in the symbols
    rng = np.random.default_rng(40)
    for _ in range(12):
        start = int(rng.integers(64))
        msg = rng.integers(0, 2, 40).astype(np.uint8)
        sym, _ = R.encode(code, R.RATE_1_2, msg, start)
        llr = R.llr_clean(sym, rng)
        bits, metric = R.decode(code, R.RATE_1_2, llr, 40, 64, 0)
        assert metric.tolist() == [0] and (bits == msg).all()


@pytest.mark.parametrize("punct", PUNCTURES)
def test_terminated_frames_against_every_message(punct):
    rng = np.random.default_rng(list(punct))
    for trial in range(3):
        msg = np.concatenate([rng.integers(0, 2, 10), np.zeros(6, np.int64)]).astype(np.uint8)
        sym, end = R.encode(R.DVB, punct, msg, 0)
        assert end == 0
        llr = R.llr_ties(sym, rng)
        best = min(R.path_cost(R.DVB, punct, llr, list(m) + [0] * 6, 0)[0]
                   for m in itertools.product((0, 1), repeat=10))
        bits, metric = R.decode(R.DVB, punct, llr, 16, 64, 0, start_state=0, end_state=0)
        assert metric.tolist() == [best]
        assert R.path_cost(R.DVB, punct, llr, bits, 0) == (best, 0)
        assert not bits[10:].any()


@pytest.mark.parametrize("start,end", [(-1, -1), (5, -1), (5, "enc"), (-1, "enc")])
def test_blocks_with_an_overlap_wider_than_the_frame_are_one_window(start, end):
    rng = np.random.default_rng(7)
    nbits = 300
    msg = rng.integers(0, 2, nbits).astype(np.uint8)
    sym, last = R.encode(R.CCSDS, R.DVB_3_4, msg, max(start, 0))
    llr = R.llr_awgn(sym, rng, 0.7)
    end = last if end == "enc" else end
    one, m1 = R.decode(R.CCSDS, R.DVB_3_4, llr, nbits, 320, 0, start, end)
    for block, overlap in ((64, 300), (128, 1024)):
        bits, m = R.decode(R.CCSDS, R.DVB_3_4, llr, nbits, block, overlap, start, end)
        assert (bits == one).all() and (m == m1[0]).all() and len(m) == R.n_blocks(block, nbits)
    short, _ = R.decode(R.CCSDS, R.DVB_3_4, llr, nbits, 64, 0, start, end)
    assert (short != one).any()  # the overlap matters on this frame


# ---- the library: sizes ------------------------------------------------------------------------

def test_symbols_and_blocks_against_the_definitions():
    rng = np.random.default_rng(16)
    for period in range(1, 17):
        while True:
            k0, k1 = (int(x) for x in rng.integers(0, 1 << period, 2))
            if k0 | k1:
                break
        punct = (period, k0, k1)
        block = 64 * int(rng.integers(1, 65))
        cc = P.Cc(R.DVB, punct, block, 0)
        ns = set()
        for base in (0, period, 7 * period, block, 3 * block, 1 << 32, (1 << 32) // period * period,
                     (1 << 32) // block * block, 5 << 32):
            ns.update(n for n in range(base - 2, base + 3) if n >= 0)
        for n in sorted(ns):
            assert cc.symbols(n) == R.n_symbols(punct, n), (punct, n)
            assert cc.blocks(n) == R.n_blocks(block, n), (block, n)
        if period <= 8:  # the definition itself, step by step
            assert cc.symbols(3 * period + 1) == sum(sum(R.kept(punct, t)) for t in range(3 * period + 1))
        cc.close()


def test_the_default_selecting_values_give_a_consistent_handle():
    cc = P.Cc(R.DVB, R.RATE_1_2, P.CC_DEFAULT_BLOCK, P.CC_DEFAULT_OVERLAP)
    block = max(b for b in range(64, 4097, 64) if cc.blocks(b) == 1)
    for n in (1, block - 1, block, block + 1, 10 * block, 10 * block + 1, (1 << 32) + 5):
        assert cc.blocks(n) == R.n_blocks(block, n)
    assert cc.blocks(0) == 0 and cc.symbols(11) == 22


# ---- the library: argument checks --------------------------------------------------------------

GOOD = dict(g0=0o171, g1=0o133, invert=0, period=3, keep0=0b101, keep1=0b011, block=64, overlap=8)


@pytest.mark.parametrize("change,message", [
    (dict(g0=0), "polynomials"), (dict(g0=128), "polynomials"), (dict(g1=0), "polynomials"),
    (dict(g1=128), "polynomials"), (dict(invert=4), "invert 4 > 3"),
    (dict(period=0), "period 0 outside [1, 16]"), (dict(period=17), "period 17 outside [1, 16]"),
    (dict(keep0=0b1101), "at or above the period 3"), (dict(keep1=0b1000), "at or above the period 3"),
    (dict(keep0=0, keep1=0), "keep nothing"),
    (dict(block=32), "block 32 is no multiple of 64"), (dict(block=100), "block 100 is no multiple of 64"),
    (dict(block=4160), "block 4160 is no multiple of 64"), (dict(overlap=1025), "overlap 1025 > 1024"),
])
def test_create_refuses(change, message):
    lib = P.load_library()
    a = dict(GOOD, **change)
    h = lib.poporon_amd_cc_create(a["g0"], a["g1"], a["invert"], a["period"], a["keep0"], a["keep1"], a["block"],
                                  a["overlap"])
    assert not h and "poporon_amd_cc_create" in P.last_error() and message in P.last_error()


def test_create_accepts_the_edges():
    for change in (dict(block=4096, overlap=1024), dict(overlap=0), dict(g0=1, g1=127, invert=3),
                   dict(period=16, keep0=1 << 15, keep1=0), dict(period=1, keep0=1, keep1=0)):
        a = dict(GOOD, **change)
        P.Cc((a["g0"], a["g1"], a["invert"]), (a["period"], a["keep0"], a["keep1"]), a["block"], a["overlap"]).close()


def _enc(lib, handle, **kw):
    a = dict(cc=handle, bits=X, bs=13, nbits=100, count=2, start=0, sym=X, ss=17, end=X)
    a.update(kw)
    return lib.poporon_cc_encode_device(a["cc"], a["bits"], a["bs"], a["nbits"], a["count"], a["start"], a["sym"],
                                        a["ss"], a["end"], None)


def _dec(lib, handle, **kw):
    a = dict(cc=handle, llr=X, ls=134, nbits=100, count=2, start=-1, end=-1, bits=X, bs=13, metric=X)
    a.update(kw)
    return lib.poporon_cc_decode_device(a["cc"], a["llr"], a["ls"], a["nbits"], a["count"], a["start"], a["end"],
                                        a["bits"], a["bs"], a["metric"], None)


def test_the_calls_refuse_before_the_gpu():
    lib = P.load_library()
    c = P.Cc(R.DVB, R.DVB_3_4, 64, 8)  # 100 steps: 134 symbols, 13 bytes of bits, 17 bytes of symbols
    assert c.symbols(100) == 134
    for kw, message in ((dict(cc=None), "NULL handle"), (dict(nbits=0), "nbits is 0"),
                        (dict(start=-1), "start_state -1 outside [0, 63]"),
                        (dict(start=64), "start_state 64 outside [0, 63]"),
                        (dict(bs=12), "bits_stride 12 < the 13 bytes"),
                        (dict(ss=16), "symbols_stride 16 < the 17 bytes"),
                        (dict(bits=None), "NULL argument"), (dict(sym=None), "NULL argument")):
        assert not _enc(lib, c.h, **kw), kw
        assert "poporon_cc_encode_device" in P.last_error() and message in P.last_error(), (kw, P.last_error())
    for kw, message in ((dict(cc=None), "NULL handle"), (dict(nbits=0), "nbits is 0"),
                        (dict(start=-2), "start_state -2 outside [-1, 63]"),
                        (dict(start=64), "start_state 64 outside [-1, 63]"),
                        (dict(end=-2), "end_state -2 outside [-1, 63]"),
                        (dict(end=64), "end_state 64 outside [-1, 63]"),
                        (dict(ls=133), "llr_stride 133 < the 134 symbols"),
                        (dict(bs=12), "bits_stride 12 < the 13 bytes"),
                        (dict(llr=None), "NULL argument"), (dict(bits=None), "NULL argument")):
        assert not _dec(lib, c.h, **kw), kw
        assert "poporon_cc_decode_device" in P.last_error() and message in P.last_error(), (kw, P.last_error())
    with pytest.raises(P.PoporonError, match="nbits is 0"):
        c.decode(X, 134, 0, 2, X, 13)
    with pytest.raises(P.PoporonError, match="start_state 64"):
        c.encode(X, 13, 100, 2, X, 17, start_state=64)


def test_count_0_returns_true_without_a_gpu():
    lib = P.load_library()
    c = P.Cc(R.CCSDS, R.RATE_1_2, 128, 32)
    assert _enc(lib, c.h, count=0, bits=None, sym=None, end=None, ss=25)
    assert _dec(lib, c.h, count=0, llr=None, bits=None, metric=None, ls=200)
    c.encode(None, 13, 100, 0, None, 25)
    c.decode(None, 200, 100, 0, None, 13)
