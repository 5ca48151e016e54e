"""Convolutional-interleaver streams without a GPU (poporon_*_conv_*, include/poporon_amd.h): the
index formula of tests/conv_ref.py against the literal FIFO model, poporon_amd_conv_span, every
argument check of every entry point (none of them reaches the GPU), and the new kernel ids."""
import os
import re

import numpy as np
import pytest

import libpoporon_amd as P
import conv_ref as R

FILL = 0xA5
# (I, M, W, phases)
GEOMETRIES = [(12, 17, 204, range(12)), (52, 4, 207, (0, 1, 51)), (3, 2, 7, range(3)), (5, 1, 255, range(5)),
              (1, 4, 10, (0,)), (64, 1, 33, (0, 1, 31, 63)), (128, 1, 128, (0, 1, 127))]


@pytest.mark.parametrize("I,M,W,phases", GEOMETRIES)
def test_formula_is_the_fifo_interleaver(I, M, W, phases):
    rng = np.random.default_rng([I, M, W])
    for phase in phases:
        for count in (1, 2, 3, 9):
            rows = rng.integers(0, 256, (count, W), dtype=np.uint8)
            # values that cannot be mistaken for the fill: the holes must hold it and nothing else may
            rows[rows == FILL] = 0
            want = R.fifo_interleave(rows.reshape(-1), I, M, phase, FILL)
            got = R.rows_to_stream(rows, I, M, phase, FILL)
            assert got.size == R.span(W, count, I, M) == count * W + (I - 1) * M * I
            assert (got == want).all(), (phase, count)
            holes = R.hole_mask(W, count, I, M, phase)
            assert holes.sum() == (I - 1) * M * I and (got[holes] == FILL).all() and (got[~holes] != FILL).all()
            assert (R.stream_to_rows(got, W, count, I, M, phase) == rows).all()


@pytest.mark.parametrize("I,M,W,phases", GEOMETRIES)
def test_deinterleaver_fifo_returns_the_input_after_the_delay(I, M, W, phases):
    rng = np.random.default_rng([W, M, I])
    delay = (I - 1) * M * I
    for phase in phases:
        seq = rng.integers(0, 256, 3 * W, dtype=np.uint8)
        sent = R.fifo_interleave(seq, I, M, phase, FILL)
        back = R.fifo_deinterleave(sent, I, M, phase, FILL)
        assert back.size == seq.size + delay
        assert (back[delay:] == seq).all(), phase
        assert (back[:delay] == FILL).all()


def test_adjacent_windows_compose():
    """n1 codewords, then n2 at base + n1*W with the advanced phase, fill one stream as n1 + n2 do"""
    rng = np.random.default_rng(7)
    for I, M, W, phase, n1, n2 in ((12, 17, 204, 5, 3, 4), (52, 4, 207, 51, 1, 2), (5, 1, 255, 0, 2, 2)):
        rows = rng.integers(0, 256, (n1 + n2, W), dtype=np.uint8)
        whole = R.rows_to_stream(rows, I, M, phase, FILL)
        parts = np.full_like(whole, FILL)
        a = R.offsets(W, n1, I, M, phase)
        parts[a] = rows[:n1].reshape(-1)
        b = n1 * W + R.offsets(W, n2, I, M, (phase + n1 * W) % I)
        assert not np.intersect1d(a, b).size
        parts[b] = rows[n1:].reshape(-1)
        assert (parts == whole).all()


def test_conv_span():
    assert P.conv_span(204, 8, 12, 17) == 8 * 204 + 11 * 17 * 12
    assert P.conv_span(207, 1 << 20, 52, 4) == (207 << 20) + 51 * 4 * 52
    assert P.conv_span(255, 0, 128, 255) == 127 * 255 * 128
    assert P.conv_span(10, 3, 1, 4) == 30
    assert P.conv_span(188, 5, 12, 17) == 5 * 188 + 2244  # a flag stream's rows
    for bad in ((0, 1, 12, 17), (204, 1, 0, 17), (204, 1, 129, 17), (204, 1, 12, 0), (204, 1, 12, 256)):
        assert P.conv_span(*bad) == 0, bad
    top = (1 << 64) - 1
    assert P.conv_span(204, top // 204 + 1, 12, 17) == 0
    assert P.conv_span(204, (top - 2244) // 204, 12, 17) == (top - 2244) // 204 * 204 + 2244
    assert P.conv_span(204, (top - 2244) // 204 + 1, 12, 17) == 0
    assert P.conv_span(1, top, 1, 1) == top and P.conv_span(1, top, 2, 1) == 0
    assert P.conv_span(204, 1 << 64, 12, 17) == 0 and P.conv_span(-1, 1, 12, 17) == 0


def test_conv_tile():
    """the tile the GPU tests size their counts by: the window of a tile and its slack fit 64 KiB"""
    for W, I, M in ((204, 12, 17), (207, 52, 4), (255, 128, 2), (15, 128, 2), (255, 1, 3), (33, 64, 1)):
        t = P.conv_tile(W, I, M)
        assert t >= 1 and t * W + (I - 1) * M * I + 2 * W + 48 <= 65536, (W, I, M)
    assert P.conv_tile(204, 12, 17) == 64  # the smallest tile: 2,244 B re-read against 13,056
    assert P.conv_tile(207, 52, 4) == -(-4 * 51 * 208 // 207)  # re-read a quarter of the tile's own bytes
    assert P.conv_tile(204, 64, 64) == 0 and P.conv_tile(204, 128, 255) == 0  # the direct path
    assert P.conv_tile(256, 12, 17) == 0 and P.conv_tile(0, 12, 17) == 0


# ---- argument checks: all of them fail before the GPU is touched -------------------------

DVB = (8, 0x11D, 0, 1, 16)
X = 0x1000  # a non-NULL pointer that is never dereferenced


def _calls(h, size=188, count=4, I=12, M=17, phase=0, data=X, ds=None, par=X, ps=None, stream=X, out=X, pos=None,
           pstride=0, cnt=None, rep=X, rstride=16):
    """every entry point as (name, thunk) with the given arguments"""
    lib = P.load_library()
    ds = size if ds is None else ds
    ps = 16 if ps is None else ps
    return [
        ("poporon_amd_conv_interleave_device",
         lambda: lib.poporon_amd_conv_interleave_device(h, data, ds, par, ps, size, count, I, M, phase, stream, None)),
        ("poporon_amd_conv_deinterleave_device",
         lambda: lib.poporon_amd_conv_deinterleave_device(h, stream, I, M, phase, data, ds, par, ps, size, count,
                                                          None)),
        ("poporon_encode_conv_device",
         lambda: lib.poporon_encode_conv_device(h, data, ds, par, ps, size, count, I, M, phase, stream, None)),
        ("poporon_decode_conv_device",
         lambda: lib.poporon_decode_conv_device(h, stream, I, M, phase, data, ds, par, ps, size, count, pos, pstride,
                                                cnt, out, None, None)),
        ("poporon_decode_conv_report_device",
         lambda: lib.poporon_decode_conv_report_device(h, stream, I, M, phase, data, ds, par, ps, size, count, pos,
                                                       pstride, cnt, out, None, rep, rep, rep, rstride, None)),
        ("poporon_check_conv_device",
         lambda: lib.poporon_check_conv_device(h, stream, I, M, phase, size, count, out, None)),
    ]


def _all_fail(calls, word, only=None):
    for name, f in calls:
        if only is not None and name not in only:
            continue
        assert f() is False, name
        msg = P.last_error()
        assert name in msg and word in msg, (name, msg)


LAYOUT = ("poporon_amd_conv_interleave_device", "poporon_amd_conv_deinterleave_device")
CODEC = ("poporon_encode_conv_device", "poporon_decode_conv_device", "poporon_decode_conv_report_device")
DECODES = CODEC[1:]
ROWS = LAYOUT + CODEC


def test_limits():
    h = P.Poporon(*DVB)
    _all_fail(_calls(h.h, I=0), "branches")
    _all_fail(_calls(h.h, I=129), "branches")
    _all_fail(_calls(h.h, M=0), "cell")
    _all_fail(_calls(h.h, M=256), "cell")
    _all_fail(_calls(h.h, phase=12), "phase")
    _all_fail(_calls(h.h, I=1, phase=1), "phase")
    _all_fail(_calls(h.h, size=0), "size")
    _all_fail(_calls(h.h, size=240), "size")  # 240 + 16 > 255
    _all_fail(_calls(h.h, count=((1 << 64) - 1) // 204), "overflows")
    # the limits hold at count 0 too
    _all_fail(_calls(h.h, count=0, I=129), "branches")


def test_null_arguments():
    h = P.Poporon(*DVB)
    _all_fail(_calls(None), "NULL handle")
    _all_fail(_calls(h.h, stream=None), "NULL argument")
    _all_fail(_calls(h.h, data=None), "NULL argument", ROWS)
    _all_fail(_calls(h.h, par=None), "NULL argument", CODEC)  # the layout calls take a NULL parity
    _all_fail(_calls(h.h, out=None), "NULL argument", DECODES + ("poporon_check_conv_device",))
    _all_fail(_calls(h.h, rep=None), "NULL report array", ("poporon_decode_conv_report_device",))


def test_strides_and_erasure_arguments():
    h = P.Poporon(*DVB)
    _all_fail(_calls(h.h, ds=187), "data_stride", ROWS)
    _all_fail(_calls(h.h, ps=15), "parity_stride", ROWS)
    _all_fail(_calls(h.h, pos=X, pstride=15, cnt=X), "positions_stride", DECODES)
    _all_fail(_calls(h.h, pos=X, pstride=16, cnt=None), "counts", DECODES)
    _all_fail(_calls(h.h, rstride=15), "report_stride", ("poporon_decode_conv_report_device",))


def test_other_handles_are_refused():
    for h in (P.Bch.default(), P.Ldpc(32, P.LDPC_RATE_1_2)):
        _all_fail(_calls(h.h, size=4), "RS handles")


def test_count_zero_succeeds_without_a_gpu_call():
    h = P.Poporon(*DVB)
    for name, f in _calls(h.h, count=0, data=None, par=None, stream=None, out=None, rep=None):
        assert f() is True, (name, P.last_error())


def test_forced_tile_path_on_a_geometry_that_does_not_fit(monkeypatch):
    monkeypatch.setenv("POPORON_AMD_CONV_PATH", "tile")
    h = P.Poporon(*DVB)
    monkeypatch.delenv("POPORON_AMD_CONV_PATH")
    _all_fail(_calls(h.h, I=64, M=64), "does not fit the LDS")
    _all_fail(_calls(h.h, I=128, M=255), "does not fit the LDS")


# ---- names and ids ------------------------------------------------------------------------

def test_kernel_ids_and_names():
    text = open(os.path.join(P.INCLUDE_DIR, "poporon_amd.h")).read()
    ids = dict(re.findall(r"#define POPORON_AMD_KERNEL_(\w+) (\d+)", text))
    assert ids["CONV_GATHER"] == "20" and ids["CONV_SCATTER"] == "21"
    assert (P.KERNEL_CONV_GATHER, P.KERNEL_CONV_SCATTER) == (20, 21)
    assert sorted(P.CONV_KERNEL_NAMES) == [20, 21]
    assert not set(P.CONV_KERNEL_NAMES) & set(P.KERNEL_NAMES)
    assert len(set(ids.values())) == len(ids) == 22


def test_every_new_symbol_is_bound():
    names = [n for n in P.header_symbols() if "conv" in n]
    assert sorted(names) == sorted(["poporon_amd_conv_span", "poporon_amd_conv_tile",
                                    "poporon_amd_conv_interleave_device", "poporon_amd_conv_deinterleave_device",
                                    "poporon_encode_conv_device", "poporon_decode_conv_device",
                                    "poporon_decode_conv_report_device", "poporon_check_conv_device"])
    lib = P.load_library()
    assert all(hasattr(lib, n) and n in P._SIGS for n in names)
