"""Symbol-interleaved frames without a GPU: the helper's two maps
(tests/interleave_ref.py), and the argument checks of the interleaved entry
points (include/poporon_amd.h), which all answer before any GPU
initialisation: false with a message naming what was wrong."""

import numpy as np
import pytest

import libpoporon_amd as P
from interleave_ref import frames_to_rows, rows_to_frames


def test_maps_are_inverses():
    rng = np.random.default_rng(1)
    for depth in (1, 2, 3, 4, 5, 7, 8, 16, 64):
        for nsym in (1, 2, 32, 223, 255):
            fr = rng.integers(0, 256, (3, nsym * depth), dtype=np.uint8)
            rows = frames_to_rows(fr, depth)
            assert rows.shape == (3 * depth, nsym)
            assert (rows_to_frames(rows, depth) == fr).all()
            assert (frames_to_rows(rows_to_frames(rows, depth), depth) == rows).all()
            # byte j*depth + i of frame f is symbol j of codeword f*depth + i
            f, j, i = 2, nsym - 1, depth - 1
            assert fr[f, j * depth + i] == rows[f * depth + i, j]


def test_depth_one_is_identity():
    rows = np.arange(5 * 9, dtype=np.uint8).reshape(5, 9)
    assert (rows_to_frames(rows, 1) == rows).all()
    assert (frames_to_rows(rows, 1) == rows).all()


def test_hand_written_2x3():
    # two codewords of three symbols, a0 a1 a2 and b0 b1 b2, in one frame of depth 2
    rows = np.array([[0xA0, 0xA1, 0xA2], [0xB0, 0xB1, 0xB2]], np.uint8)
    frame = np.array([[0xA0, 0xB0, 0xA1, 0xB1, 0xA2, 0xB2]], np.uint8)
    assert (rows_to_frames(rows, 2) == frame).all()
    assert (frames_to_rows(frame, 2) == rows).all()
    # two such frames: codewords 2 and 3 come from the second
    assert (frames_to_rows(np.concatenate([frame, frame ^ 0x0F]), 2)[2:] == rows ^ 0x0F).all()


# ---- argument checks ---------------------------------------------------------------

_BUF = np.zeros(1 << 16, np.uint8)
_PTR = _BUF.ctypes.data


def _calls(h, size, depth, count, ds=None, ps=None, data=_PTR, parity=_PTR, out=_PTR, pos=None, pos_stride=0,
           cnt=None, nr=32):
    """every interleaved entry point on one argument set: (name, thunk) pairs"""
    lib = P.load_library()
    ds = size * depth if ds is None else ds
    ps = nr * depth if ps is None else ps
    return [
        ("encode_device", lambda: lib.poporon_encode_interleaved_device(h, data, ds, parity, ps, size, depth, count,
                                                                        None)),
        ("decode_device", lambda: lib.poporon_decode_interleaved_device(h, data, ds, parity, ps, size, depth, count,
                                                                        pos, pos_stride, cnt, out, out, None)),
        ("check_device", lambda: lib.poporon_check_interleaved_device(h, data, ds, parity, ps, size, depth, count,
                                                                      out, None)),
        ("encode_host", lambda: lib.poporon_encode_interleaved(h, data, ds, parity, ps, size, depth, count)),
        ("decode_host", lambda: lib.poporon_decode_interleaved(h, data, ds, parity, ps, size, depth, count, pos,
                                                               pos_stride, cnt, out, out)),
    ]


def _refused(calls, word):
    for name, call in calls:
        assert call() is False, name
        msg = P.last_error()
        assert msg and word in msg, (name, msg)


def test_null_handle_and_pointers():
    h = P.Poporon.default()
    _refused(_calls(None, 223, 4, 1), "NULL")
    _refused(_calls(h.h, 223, 4, 1, data=None), "NULL")
    _refused(_calls(h.h, 223, 4, 1, parity=None), "NULL")
    lib = P.load_library()
    assert lib.poporon_decode_interleaved_device(h.h, _PTR, 892, _PTR, 128, 223, 4, 1, None, 0, None, None, None,
                                                 None) is False and "NULL" in P.last_error()
    assert lib.poporon_check_interleaved_device(h.h, _PTR, 892, _PTR, 128, 223, 4, 1, None, None) is False
    assert "NULL" in P.last_error()
    assert lib.poporon_amd_reserve_interleaved(None, 16) is False and "NULL" in P.last_error()


def test_non_rs_handles():
    for h in (P.Bch.default(), P.Ldpc(128, P.LDPC_RATE_1_2)):
        _refused(_calls(h.h, 4, 2, 1), "RS handles")
        assert P.load_library().poporon_amd_reserve_interleaved(h.h, 16) is False
        assert "RS handles" in P.last_error()


@pytest.mark.parametrize("depth", [0, 65, 1 << 20])
def test_depth_outside_1_64(depth):
    h = P.Poporon.default()
    _refused(_calls(h.h, 8, depth, 1, ds=1 << 30, ps=1 << 30), "depth")


@pytest.mark.parametrize("params,sizes", [((8, 0x11D, 1, 1, 32), (0, 224, 255, 70000)),
                                          ((8, 0x11D, 1, 1, 16), (0, 240)),
                                          ((4, 0x13, 1, 1, 8), (0, 8))])
def test_size_outside_the_code(params, sizes):
    """size in [1, field_size - num_roots] for all three calls, encode included"""
    h = P.Poporon(*params)
    for size in sizes:
        _refused(_calls(h.h, size, 4, 1, ds=1 << 30, nr=params[4]), "size")


def test_strides_below_the_regions():
    h = P.Poporon.default()
    _refused(_calls(h.h, 223, 4, 2, ds=223 * 4 - 1), "data_stride")
    _refused(_calls(h.h, 223, 4, 2, ps=32 * 4 - 1), "parity_stride")
    _refused(_calls(h.h, 1, 64, 2, ds=63), "data_stride")
    # a row-sized stride does not do for a frame
    _refused(_calls(h.h, 223, 5, 2, ds=255, ps=255), "data_stride")


def test_erasure_arguments_of_the_row_call():
    h = P.Poporon.default()
    lib = P.load_library()
    for fn, tail in ((lib.poporon_decode_interleaved_device, (None,)), (lib.poporon_decode_interleaved, ())):
        # positions without counts; a positions stride below num_roots
        assert fn(h.h, _PTR, 892, _PTR, 128, 223, 4, 1, _PTR, 32, None, _PTR, _PTR, *tail) is False
        assert "erasure" in P.last_error()
        assert fn(h.h, _PTR, 892, _PTR, 128, 223, 4, 1, _PTR, 31, _PTR, _PTR, _PTR, *tail) is False
        assert "erasure" in P.last_error()


def test_zero_frames_is_a_no_op():
    """count == 0 returns true and launches nothing (no GPU needed, NULL pointers allowed)"""
    h = P.Poporon.default()
    for name, call in _calls(h.h, 223, 4, 0, data=None, parity=None, out=None):
        assert call() is True, name
    # ... but the other arguments are still checked
    _refused(_calls(h.h, 223, 65, 0), "depth")


def test_python_wrappers_refuse_ragged_frames():
    h = P.Poporon.default()
    with pytest.raises(P.PoporonError):
        h.encode_interleaved(np.zeros((2, 223 * 4 + 1), np.uint8), 4)
    with pytest.raises(P.PoporonError):
        h.decode_interleaved(np.zeros((2, 10), np.uint8), np.zeros((2, 128), np.uint8), 4)
