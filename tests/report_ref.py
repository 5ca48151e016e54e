"""Decode reports and erasure lists in numpy (helper, no tests).

A report is the diff of a decode's input and output rows (include/poporon_amd.h):
for each codeword the positions that changed, ascending, and before ^ after,
capped at nr entries, the slots behind the count zero.  The expected report of
a batch is ``expect_report`` on the oracle's ``decode_batch`` input and output;
the library's own decode output is never the yardstick.  ``expect_lists`` is
the same compaction on a flag plane's rows: the first nr flagged symbol
indices, the count and whether there were more.
"""
import numpy as np


def _compact(hit, nr):
    """hit bool[count, w] -> (listed u8[count], pos u8[count, nr], total int[count]): per row the
    first nr True columns, ascending, zeros behind them"""
    hit = np.asarray(hit, dtype=bool)
    count, w = hit.shape
    assert w <= 256
    total = hit.sum(1)
    rank = np.cumsum(hit, 1) - 1                 # slot of a hit within its row
    keep = hit & (rank < nr)
    pos = np.zeros((count, nr), np.uint8)
    r, c = np.nonzero(keep)
    pos[r, rank[r, c]] = c
    return np.minimum(total, nr).astype(np.uint8), pos, total


def expect_report(before, after, nr):
    """before, after u8[count, size + nr] wire rows -> (err_num u8[count], err_pos u8[count, nr],
    err_val u8[count, nr])"""
    b, a = np.asarray(before, dtype=np.uint8), np.asarray(after, dtype=np.uint8)
    assert b.shape == a.shape
    x = b ^ a
    num, pos, _ = _compact(x != 0, nr)
    val = np.take_along_axis(x, pos.astype(np.int64), 1)
    val[np.arange(nr)[None, :] >= num[:, None]] = 0
    return num, pos, val


def expect_lists(mask_rows, nr):
    """mask_rows u8[count, size] (non-zero = flagged) -> (positions u8[count, nr], counts u8[count],
    over u8[count])"""
    cnt, pos, total = _compact(np.asarray(mask_rows) != 0, nr)
    return pos, cnt, (total > nr).astype(np.uint8)


def apply_report(rows, num, pos, val):
    """XOR a report into wire rows (a copy): on a decode's output this gives its input back"""
    out = np.array(rows, dtype=np.uint8, copy=True)
    live = np.arange(pos.shape[1])[None, :] < np.asarray(num)[:, None]
    r, k = np.nonzero(live)
    np.bitwise_xor.at(out, (r, pos[r, k].astype(np.int64)), val[r, k])
    return out
