"""Decode reports and mask-to-erasure-list calls without a GPU: the numpy helpers
(tests/report_ref.py) on hand-made rows, the argument checks of every new entry
point (include/poporon_amd.h), which all answer before any GPU initialisation,
and the new symbols in the header and the library.  On the CPU oracle: the
report is not corrected_num in another form."""

import numpy as np
import pytest

import libpoporon_amd as P
from report_ref import apply_report, expect_lists, expect_report

NEW = ("poporon_decode_batch_report_device", "poporon_decode_interleaved_report_device",
       "poporon_decode_batch_report", "poporon_amd_reserve_report", "poporon_amd_erasures_from_mask_device")


# ---- the helpers ---------------------------------------------------------------------

def test_report_of_hand_made_rows():
    before = np.zeros((4, 10), np.uint8)
    after = before.copy()
    after[1, 7] = 0x11            # one byte
    after[2, [9, 0, 4]] = (1, 2, 3)  # out of order: the list is ascending
    after[3, :] = np.arange(1, 11)   # more than nr = 4 changes: capped
    num, pos, val = expect_report(before, after, 4)
    assert num.tolist() == [0, 1, 3, 4]
    assert pos.tolist() == [[0, 0, 0, 0], [7, 0, 0, 0], [0, 4, 9, 0], [0, 1, 2, 3]]
    assert val.tolist() == [[0, 0, 0, 0], [0x11, 0, 0, 0], [2, 3, 1, 0], [1, 2, 3, 4]]
    # values are before ^ after, not after
    num, pos, val = expect_report(before ^ 0xF0, after ^ 0xF0, 4)
    assert val[1].tolist() == [0x11, 0, 0, 0]
    # XORing a report into the output restores the input (where nothing was capped)
    assert (apply_report(after[:3], num[:3], pos[:3], val[:3]) == before[:3]).all()
    assert not (apply_report(after[3:], num[3:], pos[3:], val[3:]) == before[3:]).all()


def test_report_position_zero_with_zero_slots():
    """a change at position 0 and the zero slots behind the count are told apart by err_num"""
    before = np.zeros((1, 6), np.uint8)
    after = before.copy()
    after[0, 0] = 5
    num, pos, val = expect_report(before, after, 3)
    assert num.tolist() == [1] and pos.tolist() == [[0, 0, 0]] and val.tolist() == [[5, 0, 0]]


def test_lists_of_hand_made_masks():
    m = np.zeros((5, 8), np.uint8)
    m[1, 0] = 1
    m[2, 7] = 0x80
    m[3, [1, 3, 5]] = 0xFF
    m[4, :] = 1
    pos, cnt, over = expect_lists(m, 3)
    assert cnt.tolist() == [0, 1, 1, 3, 3] and over.tolist() == [0, 0, 0, 0, 1]
    assert pos.tolist() == [[0, 0, 0], [0, 0, 0], [7, 0, 0], [1, 3, 5], [0, 1, 2]]


def test_report_is_not_corrected_num(oracle_default):
    """RS(255,223) at size 100, the late_discrepancy family (tests/rs_syndrome_rows.py): failed rows
    with corrected_num > 0 come back unchanged, so their report is empty; on ok rows the changed
    bytes equal corrected_num"""
    import rs_syndrome_rows as R
    o = oracle_default
    sm = R.SyndromeMap(o, 100)
    data, parity, _ = R.late_discrepancy(sm, draws=1)
    ok, cor, od, op = o.decode_batch(data, parity)
    num, _, _ = expect_report(np.concatenate([data, parity], 1), np.concatenate([od, op], 1), 32)
    stale = (ok == 0) & (cor > 0)
    assert stale.sum() >= 50 and (num[stale] == 0).all()
    assert (num[ok == 0] == 0).all()  # a failed row comes back unchanged
    data, parity, _ = R.positions(sm)  # corrected rows: the changed bytes are corrected_num
    ok, cor, od, op = o.decode_batch(data, parity)
    num, _, _ = expect_report(np.concatenate([data, parity], 1), np.concatenate([od, op], 1), 32)
    assert ok.all() and (num == cor).all() and set(num.tolist()) == {1, 16}


# ---- symbols -------------------------------------------------------------------------

def test_new_symbols_in_header_and_library():
    lib = P.load_library()
    names = P.header_symbols()
    for n in NEW:
        assert n in names, n
        assert hasattr(lib, n), n
    text = open(P.INCLUDE_DIR + "/poporon_amd.h").read()
    for macro, value in (("POPORON_AMD_KERNEL_SNAPSHOT", 17), ("POPORON_AMD_KERNEL_REPORT", 18),
                         ("POPORON_AMD_KERNEL_MASK_LISTS", 19)):
        assert f"#define {macro} {value}" in text
    assert (P.KERNEL_SNAPSHOT, P.KERNEL_REPORT, P.KERNEL_MASK_LISTS) == (17, 18, 19)
    for m in ("decode_batch_report_device", "decode_interleaved_report_device", "decode_batch_report",
              "reserve_report", "erasures_from_mask_device"):
        assert callable(getattr(P.Poporon, m))


# ---- argument checks -----------------------------------------------------------------

_BUF = np.zeros(1 << 16, np.uint8)
_PTR = _BUF.ctypes.data


def _report_calls(h, size=223, count=1, data=_PTR, parity=_PTR, ok=_PTR, pos=None, pos_stride=0, cnt=None,
                  num=_PTR, epos=_PTR, eval_=_PTR, rs=32, depth=4, ds=None, ps=None, nr=32):
    """the three report entry points on one argument set: (name, thunk) pairs"""
    lib = P.load_library()
    fds = size * depth if ds is None else ds
    fps = nr * depth if ps is None else ps
    return [
        ("row_device", lambda: lib.poporon_decode_batch_report_device(h, data, size, parity, nr, size, count, pos,
                                                                      pos_stride, cnt, ok, _PTR, num, epos, eval_, rs,
                                                                      None)),
        ("interleaved_device", lambda: lib.poporon_decode_interleaved_report_device(
            h, data, fds, parity, fps, size, depth, count, pos, pos_stride, cnt, ok, _PTR, num, epos, eval_, rs, None)),
        ("row_host", lambda: lib.poporon_decode_batch_report(h, data, size, parity, nr, size, count, pos, pos_stride,
                                                             cnt, ok, _PTR, num, epos, eval_, rs)),
    ]


def _mask_call(h, size=223, depth=4, count=1, mask=_PTR, ms=None, pos=_PTR, pstride=32, cnt=_PTR, over=_PTR):
    lib = P.load_library()
    ms = size * depth if ms is None else ms
    return [("mask", lambda: lib.poporon_amd_erasures_from_mask_device(h, mask, ms, size, depth, count, pos, pstride,
                                                                       cnt, over, None))]


def _refused(calls, word):
    for name, call in calls:
        assert call() is False, name
        msg = P.last_error()
        assert msg and word in msg, (name, msg)


def test_null_handle_and_pointers():
    h = P.Poporon.default()
    _refused(_report_calls(None) + _mask_call(None), "NULL")
    for kw in ({"data": None}, {"parity": None}, {"ok": None}, {"num": None}, {"epos": None}, {"eval_": None}):
        _refused(_report_calls(h.h, **kw), "NULL")
    for kw in ({"mask": None}, {"pos": None}, {"cnt": None}):
        _refused(_mask_call(h.h, **kw), "NULL")
    assert P.load_library().poporon_amd_reserve_report(None, 16) is False and "NULL" in P.last_error()


def test_non_rs_handles():
    for h in (P.Bch.default(), P.Ldpc(128, P.LDPC_RATE_1_2)):
        _refused(_report_calls(h.h, size=4, depth=2) + _mask_call(h.h, size=4, depth=2), "RS handles")
        assert P.load_library().poporon_amd_reserve_report(h.h, 16) is False
        assert "RS handles" in P.last_error()


@pytest.mark.parametrize("params", [(8, 0x11D, 1, 1, 32), (8, 0x11D, 1, 1, 16), (4, 0x13, 1, 1, 8)])
def test_strides_below_num_roots(params):
    h = P.Poporon(*params)
    nr = params[4]
    _refused(_report_calls(h.h, size=4, rs=nr - 1, nr=nr), "report_stride")
    _refused(_report_calls(h.h, size=4, rs=0, nr=nr), "report_stride")
    _refused(_mask_call(h.h, size=4, pstride=nr - 1), "positions_stride")
    # the erasure arguments of the decode calls: positions without counts, a stride below num_roots
    _refused(_report_calls(h.h, size=4, pos=_PTR, pos_stride=nr, cnt=None, rs=nr, nr=nr), "erasure")
    _refused(_report_calls(h.h, size=4, pos=_PTR, pos_stride=nr - 1, cnt=_PTR, rs=nr, nr=nr), "erasure")


def test_strides_below_a_region():
    h = P.Poporon.default()
    calls = dict(_report_calls(h.h, depth=4, ds=223 * 4 - 1))
    assert calls["interleaved_device"]() is False and "data_stride" in P.last_error()
    calls = dict(_report_calls(h.h, depth=4, ps=32 * 4 - 1))
    assert calls["interleaved_device"]() is False and "parity_stride" in P.last_error()
    _refused(_mask_call(h.h, size=223, depth=4, ms=223 * 4 - 1), "mask_stride")
    _refused(_mask_call(h.h, size=223, depth=5, ms=255), "mask_stride")  # a row-sized stride is no frame's


@pytest.mark.parametrize("depth", [0, 65, 1 << 20])
def test_depth_outside_1_64(depth):
    h = P.Poporon.default()
    calls = dict(_report_calls(h.h, size=8, depth=depth, ds=1 << 30, ps=1 << 30))
    assert calls["interleaved_device"]() is False and "depth" in P.last_error()
    _refused(_mask_call(h.h, size=8, depth=depth, ms=1 << 30), "depth")


@pytest.mark.parametrize("params,sizes", [((8, 0x11D, 1, 1, 32), (0, 224, 255, 70000)),
                                          ((8, 0x11D, 1, 1, 16), (0, 240)),
                                          ((4, 0x13, 1, 1, 8), (0, 8))])
def test_size_outside_the_code(params, sizes):
    h = P.Poporon(*params)
    nr = params[4]
    for size in sizes:
        _refused(_report_calls(h.h, size=size, ds=1 << 30, nr=nr, rs=nr) + _mask_call(h.h, size=size, ms=1 << 30),
                 "size")


def test_zero_count_is_a_no_op():
    """count == 0 returns true and launches nothing (no GPU needed, NULL pointers allowed) ..."""
    h = P.Poporon.default()
    for name, call in (_report_calls(h.h, count=0, data=None, parity=None, ok=None, num=None, epos=None, eval_=None)
                       + _mask_call(h.h, count=0, mask=None, pos=None, cnt=None, over=None)):
        assert call() is True, name
    # ... but the other arguments are still checked
    _refused(_report_calls(h.h, count=0, rs=31), "report_stride")
    _refused(_mask_call(h.h, count=0, depth=65, ms=1 << 30), "depth")
