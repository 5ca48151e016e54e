"""Symbol-interleaved frames against the oracle's row batches (helper, no tests).

A frame of depth D holds D codewords symbol by symbol: byte j*D + i of a
region is symbol j of codeword i (include/poporon_amd.h).  The reference has
no notion of a frame, so its answer for a batch of frames is its row batch
answer on the de-interleaved codewords, re-interleaved: ``expect_*`` below,
on ``oracle.Oracle``'s ``encode_batch`` / ``decode_batch`` /
``syndrome_batch``.  Codeword c = f*D + i everywhere.
"""
import numpy as np


def frames_to_rows(frames, depth):
    """u8[count, nsym*depth] regions -> u8[count*depth, nsym] rows (row f*depth + i)."""
    fr = np.asarray(frames, dtype=np.uint8)
    count, width = fr.shape
    assert depth >= 1 and width % depth == 0
    nsym = width // depth
    return np.ascontiguousarray(fr.reshape(count, nsym, depth).transpose(0, 2, 1)).reshape(count * depth, nsym)


def rows_to_frames(rows, depth):
    """u8[count*depth, nsym] rows -> u8[count, nsym*depth] regions."""
    r = np.asarray(rows, dtype=np.uint8)
    n, nsym = r.shape
    assert depth >= 1 and n % depth == 0
    count = n // depth
    return np.ascontiguousarray(r.reshape(count, depth, nsym).transpose(0, 2, 1)).reshape(count, nsym * depth)


def expect_encode(oracle, frames, depth, threads=0):
    """parity regions u8[count, nroots*depth] of message regions u8[count, size*depth]"""
    return rows_to_frames(oracle.encode_batch(frames_to_rows(frames, depth), threads=threads), depth)


def expect_decode(oracle, frames, parity, depth, positions=None, counts=None, threads=0):
    """(ok u8[count*depth], corrected u32[count*depth], frames', parity'); positions u8 or
    u32 [count*depth, >= nroots] slots with counts[count*depth] select the erasure decode."""
    d, p = frames_to_rows(frames, depth), frames_to_rows(parity, depth)
    if positions is not None:
        ok, cor, dd, pp = oracle.decode_batch(d, p, np.asarray(positions).astype(np.uint32),
                                              np.asarray(counts).astype(np.uint32), threads=threads)
    else:
        ok, cor, dd, pp = oracle.decode_batch(d, p, threads=threads)
    return ok, cor, rows_to_frames(dd, depth), rows_to_frames(pp, depth)


def expect_check(oracle, frames, parity, depth):
    """dirty u8[count*depth]: the oracle's nonzero-syndrome flag per codeword"""
    return oracle.syndrome_batch(frames_to_rows(frames, depth), frames_to_rows(parity, depth))[0]
