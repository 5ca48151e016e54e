"""Plane-layout stripes without a GPU (poporon_*_planes_*, include/poporon_amd.h): the helper of
tests/planes_ref.py against a literal double loop, poporon_amd_plane_tile, the index arithmetic of
the layout kernels restated in Python (every used byte moved exactly once, no LDS index past the
image, no byte outside the tile), every argument check of every entry point (none of them reaches
the GPU), and the new kernel ids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libpoporon_amd as P
import planes_ref as R

RS223 = (8, 0x11D, 1, 1, 32)
STORAGE = (8, 0x11D, 1, 1, 4)  # the (14,10) shape
X = 0x1000  # a non-NULL pointer that is never dereferenced


def _oracle(params):
    from oracle import Oracle
    return Oracle(*params)


# ---- the helper ---------------------------------------------------------------------------

def test_transposes_against_a_double_loop():
    rng = np.random.default_rng(1)
    planes = rng.integers(0, 256, (14, 37), dtype=np.uint8)
    rows = R.planes_to_rows(planes)
    assert rows.shape == (37, 14) and rows.flags.c_contiguous
    for j in range(14):
        for c in range(37):
            assert rows[c, j] == planes[j, c]
    assert (R.rows_to_planes(rows) == planes).all()
    st = R.staged_rows(planes, [0, 5, 13])
    for c in range(37):
        for j in range(14):
            assert st[c, j] == (0 if j in (0, 5, 13) else planes[j, c])
    pos, cnt = R.lost_lists([2, 9, 12], 4, 5)
    assert pos.tolist() == [[2, 9, 12, 0]] * 5 and cnt.tolist() == [3] * 5
    with pytest.raises(AssertionError):
        R.lost_lists([9, 2], 4, 1)


def test_expectations_against_row_calls_in_a_loop():
    o = _oracle(STORAGE)
    rng = np.random.default_rng(2)
    size, nr, count = 10, 4, 23
    data = rng.integers(0, 256, (size, count), dtype=np.uint8)
    par = R.expect_encode(o, data)
    for c in range(count):
        assert (par[:, c] == o.encode(data[:, c])).all()
    clean = np.concatenate([data, par])
    assert not R.expect_check(o, clean).any()
    recv = clean.copy()
    recv[3, 4] ^= 0x11           # one error: corrected by the scrub
    recv[[1, 2, 12], 9] ^= 0x77  # three: past t = 2
    recv[13, 22] ^= 1
    assert R.expect_check(o, recv).tolist() == [int(c in (4, 9, 22)) for c in range(count)]
    ok, cor, out, dirty = R.expect_decode(o, recv)
    for c in range(count):
        want = o.decode(recv[:size, c], recv[size:, c])
        assert (ok[c], cor[c]) == (want[0], want[1])
        assert (out[:size, c] == want[2]).all() and (out[size:, c] == want[3]).all()
    assert ok[4] and ok[22] and not ok[9] and dirty[9] and not dirty[4]
    # a rebuild of two lost planes, one of them parity, from clean survivors: exact, whatever the lost planes held
    lost = [2, 11]
    junk = clean.copy()
    junk[lost] = rng.integers(0, 256, (2, count), dtype=np.uint8)
    ok, cor, out, dirty = R.expect_decode(o, junk, lost)
    assert ok.all() and not dirty.any() and (out == clean).all()
    # quirk Q2: a lost plane and one corrupted survivor: ok = 1 with wrong bytes, and the flag shows it
    bad = clean.copy()
    bad[5] ^= 0x3C
    ok, cor, out, dirty = R.expect_decode(o, bad, [1])
    assert ok.all() and (out != clean).any(1).any() and dirty.all()


# ---- poporon_amd_plane_tile and the index model ---------------------------------------------

def test_plane_tile():
    for W in range(2, 256):
        t = P.plane_tile(W)
        assert t == R.tile(W) and t % 16 == 0 and t >= 64 and t * W <= 32768, W
        assert (1 << 20) // t >= 2048  # a launch of 2^20 codewords: eight workgroups per compute unit of 256
    assert P.plane_tile(255) == 128 and P.plane_tile(14) == 512
    assert P.plane_tile(0) == 0 and P.plane_tile(256) == 0 and P.plane_tile(1 << 40) == 0 and P.plane_tile(-1) == 0


def _model_case(W, count, offs, used, t0=None):
    """every tile of a chunk: the used bytes of each plane are moved exactly once, the unused columns are
    filled, the row side covers the run exactly once"""
    T = R.tile(W)
    aligned = all(o % 16 == 0 for o, u in zip(offs, used) if u)
    for t0 in range(0, count, T):
        tc = min(T, count - t0)
        addrs = [0x7000 + o + t0 for o in offs]
        lds, moves = R.tile_model(W, T, count, t0, addrs, used, aligned)
        assert (lds == 1).all(), (W, count, t0)  # every image byte written exactly once (gather), read once (scatter)
        seen = np.zeros((W, tc), np.int64)
        for j, a, b, whole in moves:
            assert used[j] and 0 <= a < b <= tc and (not whole or b - a == 16)
            seen[j, a:b] += 1
        assert (seen[[j for j in range(W) if used[j]]] == 1).all() and not seen[[j for j in range(W) if not used[j]]].any()
        cover = np.zeros(tc * W, np.int64)
        for a, b, whole in R.row_side_model(W, tc):
            assert 0 <= a < b <= tc * W and (not whole or (b - a == 16 and a % 16 == 0))
            cover[a:b] += 1
        assert (cover == 1).all()
        assert (t0 * W) % 16 == 0  # the run of a tile starts on a 16-byte boundary of the rows


@pytest.mark.parametrize("W", [2, 3, 14, 15, 16, 33, 100, 248, 255])
def test_index_model(W):
    rng = np.random.default_rng(W)
    T = R.tile(W)
    for count in (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 5):
        all_used = [True] * W
        _model_case(W, count, [0] * W, all_used)                       # the aligned kernels
        _model_case(W, count, [16 * (j % 3) for j in range(W)], all_used)
        _model_case(W, count, list(rng.integers(0, 16, W)), all_used)  # every plane its own alignment
        for a in (1, 15):
            _model_case(W, count, [a] * W, all_used)
        used = [bool(b) for b in rng.integers(0, 2, W)]                # lost and NULL planes: zero-filled columns
        _model_case(W, count, list(rng.integers(0, 16, W)), used)
        _model_case(W, count, [0] * W, used)


# ---- argument checks: all of them fail before the GPU is touched -------------------------

def _table(W, null=()):
    return (C.c_void_p * W)(*[None if j in null else X + 0x100 * j for j in range(W)])


def _lost(lost):
    return (C.c_uint8 * max(1, len(lost)))(*lost)


def _calls(h, size=10, nr=4, count=4, null=(), lost=(), nlost=None, out=X, rep=X, rstride=None, table=True, buf=X):
    """every entry point as (name, thunk) with the given arguments"""
    lib = P.load_library()
    W = size + nr if 0 < size + nr < 300 else 14
    tab = _table(W, null) if table else None
    la, ln = _lost(lost), len(lost) if nlost is None else nlost
    rs = nr if rstride is None else rstride
    return [
        ("poporon_encode_planes_device", lambda: lib.poporon_encode_planes_device(h, tab, size, count, None)),
        ("poporon_decode_planes_device",
         lambda: lib.poporon_decode_planes_device(h, tab, size, count, la, ln, out, None, None, None)),
        ("poporon_decode_planes_report_device",
         lambda: lib.poporon_decode_planes_report_device(h, tab, size, count, la, ln, out, None, None, rep, rep, rep,
                                                         rs, None)),
        ("poporon_check_planes_device", lambda: lib.poporon_check_planes_device(h, tab, size, count, out, None)),
        ("poporon_encode_planes_strided_device",
         lambda: lib.poporon_encode_planes_strided_device(h, buf, 64, buf, 64, size, count, None)),
        ("poporon_decode_planes_strided_device",
         lambda: lib.poporon_decode_planes_strided_device(h, buf, 64, buf, 64, size, count, la, ln, out, None, None,
                                                          None)),
        ("poporon_check_planes_strided_device",
         lambda: lib.poporon_check_planes_strided_device(h, buf, 64, buf, 64, size, count, out, None)),
    ]


ENCODES = ("poporon_encode_planes_device", "poporon_encode_planes_strided_device")
DECODES = ("poporon_decode_planes_device", "poporon_decode_planes_report_device",
           "poporon_decode_planes_strided_device")
CHECKS = ("poporon_check_planes_device", "poporon_check_planes_strided_device")
TABLE = ("poporon_encode_planes_device", "poporon_decode_planes_device", "poporon_decode_planes_report_device",
         "poporon_check_planes_device")
STRIDED = (ENCODES[1], DECODES[2], CHECKS[1])
REPORT = ("poporon_decode_planes_report_device",)


def _all_fail(calls, word, only=None):
    n = 0
    for name, f in calls:
        if only is not None and name not in only:
            continue
        assert f() is False, name
        msg = P.last_error()
        assert name in msg and word in msg, (name, msg)
        n += 1
    assert n == (7 if only is None else len(only))


def test_null_handle_and_other_handles():
    _all_fail(_calls(None), "NULL handle")
    for h in (P.Bch.default(), P.Ldpc(32, P.LDPC_RATE_1_2)):
        _all_fail(_calls(h.h), "RS handles")
    lib = P.load_library()
    assert lib.poporon_amd_reserve_planes(None, 10) is False and "NULL handle" in P.last_error()
    assert lib.poporon_amd_reserve_planes(P.Bch.default().h, 10) is False and "RS handles" in P.last_error()


def test_size_out_of_range():
    h = P.Poporon(*STORAGE)
    _all_fail(_calls(h.h, size=0), "size")
    _all_fail(_calls(h.h, size=252), "size")  # 252 + 4 > 255
    _all_fail(_calls(h.h, size=252, count=0), "size")  # the limits hold at count 0 too


def test_lost_list():
    h = P.Poporon(*STORAGE)
    _all_fail(_calls(h.h, lost=[5, 2]), "ascending", DECODES)
    _all_fail(_calls(h.h, lost=[2, 2]), "ascending", DECODES)
    _all_fail(_calls(h.h, lost=[3, 14]), "lost plane index", DECODES)
    _all_fail(_calls(h.h, lost=[255]), "lost plane index", DECODES)
    _all_fail(_calls(h.h, lost=[0, 1, 2, 3, 4]), "lost_count", DECODES)
    _all_fail(_calls(h.h, lost=[5, 2], count=0), "ascending", DECODES)
    lib = P.load_library()
    assert lib.poporon_decode_planes_device(h.h, _table(14), 10, 4, None, 2, X, None, None, None) is False
    assert "NULL argument" in P.last_error()


def test_null_entries_and_arguments():
    h = P.Poporon(*STORAGE)
    _all_fail(_calls(h.h, table=False), "NULL argument", TABLE)
    _all_fail(_calls(h.h, buf=None), "NULL argument", STRIDED)
    _all_fail(_calls(h.h, out=None), "NULL argument", DECODES + CHECKS)
    _all_fail(_calls(h.h, rep=None), "NULL report array", REPORT)
    _all_fail(_calls(h.h, rstride=3), "report_stride", REPORT)
    # a surviving plane may not be NULL; a lost one may (the call then goes on to the GPU: not made here)
    _all_fail(_calls(h.h, null=(3,)), "NULL plane 3", TABLE)
    _all_fail(_calls(h.h, null=(12,)), "NULL plane 12", TABLE[1:])  # the encode takes a NULL parity entry
    _all_fail(_calls(h.h, null=(3,), lost=[4]), "NULL plane 3", TABLE[1:3])
    _all_fail(_calls(h.h, null=(10, 11, 12, 13)), "every parity plane is NULL", ENCODES[:1])


def test_count_zero_succeeds_without_a_gpu_call():
    h = P.Poporon(*STORAGE)
    for name, f in _calls(h.h, count=0, table=False, out=None, rep=None, buf=None):
        assert f() is True, (name, P.last_error())
    for name, f in _calls(h.h, count=0, lost=[1, 13], table=False, out=None, rep=None, buf=None):
        assert f() is True, (name, P.last_error())


# ---- names and ids ------------------------------------------------------------------------

def test_kernel_ids_and_names():
    text = open(os.path.join(P.INCLUDE_DIR, "poporon_amd.h")).read()
    ids = dict(re.findall(r"POPORON_AMD_KERNEL_(PLANE_\w+) = (\d+)", text))
    assert ids == {"PLANE_GATHER": "22", "PLANE_SCATTER": "23"}
    assert (P.KERNEL_PLANE_GATHER, P.KERNEL_PLANE_SCATTER) == (22, 23)
    assert sorted(P.PLANE_KERNEL_NAMES) == [22, 23]
    assert not set(P.PLANE_KERNEL_NAMES) & (set(P.KERNEL_NAMES) | set(P.CONV_KERNEL_NAMES))


def test_every_new_symbol_is_bound():
    names = [n for n in P.header_symbols() if "plane" in n]
    assert sorted(names) == sorted(["poporon_amd_plane_tile", "poporon_amd_reserve_planes",
                                    "poporon_encode_planes_device", "poporon_decode_planes_device",
                                    "poporon_decode_planes_report_device", "poporon_check_planes_device",
                                    "poporon_encode_planes_strided_device", "poporon_decode_planes_strided_device",
                                    "poporon_check_planes_strided_device"])
    lib = P.load_library()
    assert all(hasattr(lib, n) and n in P._SIGS for n in names)
