"""The soft-output decode of the K = 7 code without a GPU (poporon_cc_decode_siso_device, include/poporon_amd.h):
the numpy model of tests/cc_soft_ref.py held to things it did not define itself -- a brute-force search over every
message of short frames (path costs by cc_ref.path_cost), the hard decode of cc_ref.decode (signs and block
metrics), hand-written rows for saturation and shift -- then every argument check of the call (none reaches the
GPU), the count-0 return and the Python binding."""
import numpy as np
import pytest

import libpoporon_amd as P
import cc_ref as R
import cc_soft_ref as S

X = 0x1000  # a non-NULL pointer that is never dereferenced
PARITY = np.array([bin(i).count("1") & 1 for i in range(128)], np.int64)


def _all_costs(code, punct, llr, n):
    """(cost, end state) int64[64, 2^n] of every message from every start state: cc_ref.path_cost over arrays;
    message k has bit t at bit n - 1 - t of k"""
    g0, g1, inv = code
    v = R.depuncture(punct, llr, n)
    k = np.arange(1 << n, dtype=np.int64)[None, :]
    s = np.broadcast_to(np.arange(64, dtype=np.int64)[:, None], (64, 1 << n)).copy()
    total = np.zeros((64, 1 << n), np.int64)
    for t in range(n):
        r = (((k >> (n - 1 - t)) & 1) << 6) | s
        for j, g in enumerate((g0, g1)):
            o = PARITY[r & g] ^ ((inv >> j) & 1)
            x = int(v[t, j])
            if x != 0:
                total += np.where((x < 0) != (o != 0), abs(x), 0)
        s = r >> 1
    return total, s


def _message(k, n):
    return [(k >> (n - 1 - t)) & 1 for t in range(n)]


def test_the_array_path_costs_are_cc_refs():
    rng = np.random.default_rng(11)
    for punct in (R.RATE_1_2, R.DVB_3_4):
        for n in (1, 4, 10):
            llr = rng.integers(-128, 128, R.n_symbols(punct, n)).astype(np.int8)
            total, end = _all_costs(R.DVB, punct, llr, n)
            for _ in range(40):
                s, k = int(rng.integers(64)), int(rng.integers(1 << n))
                assert R.path_cost(R.DVB, punct, llr, _message(k, n), s) == (total[s, k], end[s, k])


@pytest.mark.parametrize("punct", [R.RATE_1_2, R.DVB_3_4])
@pytest.mark.parametrize("known_start", [False, True])
@pytest.mark.parametrize("known_end", [False, True])
def test_short_frames_against_every_message(punct, known_start, known_end):
    """D_b of step t is the least path cost over the messages with bit t = b (2^28 where there is none); one
    window: the block is wider than the frame"""
    rng = np.random.default_rng([punct[0], known_start, known_end])
    for n in range(1, 11):
        for trial in range(2):
            start = int(rng.integers(64))
            msg = rng.integers(0, 2, n)
            sym, end = R.encode(R.DVB, punct, msg, start)
            llr = (R.llr_ties(sym, rng, top=3), R.llr_awgn(sym, rng, 0.9))[trial]
            total, last = _all_costs(R.DVB, punct, llr, n)
            if known_start:
                total, last = total[start:start + 1], last[start:start + 1]
            if known_end:
                total = np.where(last == end, total, S.NO_PATH)
            best = total.min(0)  # over the start states: per message
            k = np.arange(1 << n)
            want = np.array([[best[((k >> (n - 1 - t)) & 1) == b].min() for b in (0, 1)] for t in range(n)])
            soft, D = S.decode_soft(R.DVB, punct, llr, n, 64, 0, start if known_start else -1,
                                    end if known_end else -1)
            finite = want < S.NO_PATH
            assert (D[finite] == want[finite]).all() and (D[~finite] >= S.NO_PATH).all(), (n, trial)
            assert (soft == S.quantise(want[:, 1] - want[:, 0], 0)).all()


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("overlap", [0, 7, 64, 1024])
def test_signs_and_block_metrics_are_the_hard_decodes(block, overlap):
    """wherever the output is not 0 its sign is cc_ref.decode's bit, and min(D_0, D_1) of every own step of a
    block is that block's metric"""
    rng = np.random.default_rng([block, overlap])
    nbits = 300
    nonzero = 0
    for code, punct in ((R.DVB, R.RATE_1_2), (R.CCSDS, R.DVB_3_4)):
        msg = rng.integers(0, 2, nbits)
        sym, last = R.encode(code, punct, msg, 5)
        for llr in (R.llr_awgn(sym, rng, 0.85), R.llr_ties(sym, rng)):
            for start, end in ((-1, -1), (5, -1), (-1, last), (5, last)):
                bits, metric = R.decode(code, punct, llr, nbits, block, overlap, start, end)
                soft, D = S.decode_soft(code, punct, llr, nbits, block, overlap, start, end)
                assert ((soft < 0) == (bits == 1))[soft != 0].all()
                assert (D.min(1) == np.repeat(metric, block)[:nbits]).all()
                for shift in (3, 8):
                    again, _ = S.decode_soft(code, punct, llr, nbits, block, overlap, start, end, shift)
                    assert (again == S.quantise(D[:, 1] - D[:, 0], shift)).all()
                nonzero += int((soft != 0).sum())
    assert nonzero > nbits


def test_saturation_and_shift_on_hand_written_rows():
    x = [0, 1, -1, 7, -7, 8, -8, 127, -127, 128, -128, 1 << 28, -(1 << 28), (1 << 29) + 5]
    assert S.quantise(x, 0).tolist() == [0, 1, -1, 7, -7, 8, -8, 127, -127, 127, -127, 127, -127, 127]
    assert S.quantise(x, 3).tolist() == [0, 0, 0, 0, 0, 1, -1, 15, -15, 16, -16, 127, -127, 127]
    assert S.quantise(x, 8).tolist() == [0] * 9 + [0, 0, 127, -127, 127]
    # nothing received: every path costs 0, every output is 0
    erased = np.zeros(R.n_symbols(R.DVB_3_4, 100), np.int8)
    for start in (-1, 9):
        soft, D = S.decode_soft(R.CCSDS, R.DVB_3_4, erased, 100, 64, 7, start, -1)
        assert not soft.any() and not D.any()
    # ... but a known end state is the last six bits: no path with another bit there (state 0b000101: newest first)
    soft, D = S.decode_soft(R.CCSDS, R.DVB_3_4, erased, 100, 64, 7, -1, 0b000101)
    assert not soft[:94].any() and soft[94:].tolist() == [-127, 127, -127, 127, 127, 127]
    assert not D[:94].any() and (D[94:].max(1) >= S.NO_PATH).all() and not D[94:].min(1).any()
    # every symbol -128: from state 63 the all-ones message of 171/133 sends ones only (both polynomials have five
    # taps) and costs 0; another bit anywhere costs at least one symbol of 128
    llr = np.full(2 * 200, -128, np.int8)
    soft, D = S.decode_soft(R.DVB, R.RATE_1_2, llr, 200, 64, 32)
    assert (soft == -127).all() and (D[:, 1] == 0).all() and (D[:, 0] % 128 == 0).all()
    # away from the frame's ends a wrong bit costs the free distance, 10 symbols: 1280 >> 8 = 5
    soft, D = S.decode_soft(R.DVB, R.RATE_1_2, llr, 200, 64, 32, shift=8)
    assert (D[32:160, 0] == 1280).all() and (soft[32:160] == -5).all() and soft.min() >= -5 and soft.max() < 0
    soft, _ = S.decode_soft(R.DVB, R.RATE_1_2, llr, 200, 64, 32, start_state=0)  # state 0 sends zeros first
    assert soft.min() >= -127 and (soft[100:] == -127).all()


# ---- the library: argument checks, count 0, the binding ------------------------------------------

def _soft(lib, handle, **kw):
    a = dict(cc=handle, llr=X, ls=134, nbits=100, count=2, start=-1, end=-1, shift=0, soft=X, ss=100)
    a.update(kw)
    return lib.poporon_cc_decode_siso_device(a["cc"], a["llr"], a["ls"], a["nbits"], a["count"], a["start"], a["end"],
                                             a["shift"], a["soft"], a["ss"], None)


def test_the_call_refuses_before_the_gpu():
    lib = P.load_library()
    c = P.Cc(R.DVB, R.DVB_3_4, 64, 8)  # 100 steps: 134 symbols, 100 bytes of output
    for kw, message in ((dict(cc=None), "NULL handle"), (dict(nbits=0), "nbits is 0"),
                        (dict(start=-2), "start_state -2 outside [-1, 63]"),
                        (dict(start=64), "start_state 64 outside [-1, 63]"),
                        (dict(end=-2), "end_state -2 outside [-1, 63]"),
                        (dict(end=64), "end_state 64 outside [-1, 63]"),
                        (dict(shift=9), "shift 9 > 8"),
                        (dict(ls=133), "llr_stride 133 < the 134 symbols"),
                        (dict(ss=99), "soft_stride 99 < the 100 bytes"),
                        (dict(llr=None), "NULL argument"), (dict(soft=None), "NULL argument")):
        assert not _soft(lib, c.h, **kw), kw
        assert "poporon_cc_decode_siso_device" in P.last_error() and message in P.last_error(), (kw, P.last_error())
    # the order of the checks is the hard decode's: the earlier argument is the one reported
    assert not _soft(lib, c.h, nbits=0, start=99, shift=9) and "nbits is 0" in P.last_error()
    assert not _soft(lib, c.h, end=64, shift=9, ls=1) and "end_state 64" in P.last_error()
    assert not _soft(lib, c.h, shift=9, ls=1, ss=1) and "shift 9" in P.last_error()
    assert not _soft(lib, c.h, ls=1, ss=1, soft=None) and "llr_stride 1" in P.last_error()
    assert not _soft(lib, c.h, ss=1, soft=None) and "soft_stride 1" in P.last_error()
    with pytest.raises(P.PoporonError, match="shift 9 > 8"):
        c.decode_soft(X, 134, 100, 2, X, 100, shift=9)
    with pytest.raises(P.PoporonError, match="poporon_cc_decode_siso_device failed: .*soft_stride 99"):
        c.decode_soft(X, 134, 100, 2, X, 99)


def test_count_0_returns_true_without_a_gpu():
    lib = P.load_library()
    c = P.Cc(R.CCSDS, R.RATE_1_2, 128, 32)
    assert _soft(lib, c.h, count=0, llr=None, soft=None, ls=200, shift=8)
    c.decode_soft(None, 200, 100, 0, None, 100)
    c.decode_soft(None, 200, 100, 0, None, 100, start_state=0, end_state=63, shift=8, stream=0)
