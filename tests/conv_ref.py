"""Convolutional-interleaver streams against the oracle's row batches (helper, no tests).

A Forney interleaver has I branches, branch b a FIFO of b*M bytes, one byte to each branch in
turn (EN 300 421 section 4.4.1: I = 12, M = 17).  With the code bytes of a batch numbered
serially, n = c*W + s, byte n travels on branch b = (phase + n) mod I and leaves at stream offset

    p(n) = n + b*M*I

(include/poporon_amd.h).  ``rows_to_stream`` / ``stream_to_rows`` apply that formula in numpy;
``fifo_interleave`` / ``fifo_deinterleave`` are the literal model, a deque per branch, which
tests/test_conv_cpu.py holds the formula against.  The reference has no notion of a stream, so its
answer for a stream is its row batch answer on the de-interleaved rows: ``expect_*`` below, on
``oracle.Oracle``'s ``encode_batch`` / ``decode_batch`` / ``syndrome_batch``.
"""
from collections import deque

import numpy as np


def span(W, count, I, M):
    """bytes of stream that `count` rows of W bytes occupy"""
    return count * W + (I - 1) * M * I


def offsets(W, count, I, M, phase):
    """i64[count*W]: p(n) of every byte of the batch"""
    n = np.arange(count * W, dtype=np.int64)
    return n + ((phase + n) % I) * (M * I)


def rows_to_stream(rows, I, M, phase, fill):
    """u8[count, W] rows -> u8[span]: every byte at its p(n), `fill` in the holes"""
    r = np.ascontiguousarray(rows, dtype=np.uint8)
    count, W = r.shape
    out = np.full(span(W, count, I, M), fill, np.uint8)
    out[offsets(W, count, I, M, phase)] = r.reshape(-1)
    return out


def stream_to_rows(stream, W, count, I, M, phase):
    """u8[span] -> u8[count, W] rows"""
    s = np.asarray(stream, dtype=np.uint8)
    assert s.size == span(W, count, I, M)
    return s[offsets(W, count, I, M, phase)].reshape(count, W)


def hole_mask(W, count, I, M, phase):
    """bool[span]: True at the offsets that are no p(n) of the batch"""
    m = np.ones(span(W, count, I, M), bool)
    m[offsets(W, count, I, M, phase)] = False
    return m


def fifo_interleave(seq, I, M, phase, fill):
    """The interleaver itself: input byte t enters branch (phase + t) mod I, a FIFO of b*M cells
    that hold `fill` at the start, and the byte the FIFO pushes out is output byte t (branch 0
    passes its byte on).  Returns len(seq) + (I-1)*M*I output bytes: the input is followed by
    enough `fill` to flush the longest branch."""
    fifos = [deque([fill] * (b * M)) for b in range(I)]
    out = []
    for t, v in enumerate(list(seq) + [fill] * ((I - 1) * M * I)):
        f = fifos[(phase + t) % I]
        f.append(v)
        out.append(f.popleft())
    return np.array(out, dtype=np.uint8)


def fifo_deinterleave(seq, I, M, phase, fill):
    """The de-interleaver: branch b is a FIFO of (I-1-b)*M cells, so that every byte has waited
    (I-1)*M in all.  Output byte t + (I-1)*M*I is interleaver input byte t."""
    fifos = [deque([fill] * ((I - 1 - b) * M)) for b in range(I)]
    out = []
    for t, v in enumerate(seq):
        f = fifos[(phase + t) % I]
        f.append(v)
        out.append(f.popleft())
    return np.array(out, dtype=np.uint8)


def expect_encode(oracle, rows, threads=0):
    """parity rows u8[count, nroots] of message rows u8[count, size]"""
    return oracle.encode_batch(rows, threads=threads)


def expect_decode(oracle, stream, size, count, I, M, phase, positions=None, counts=None, threads=0):
    """(ok u8[count], corrected u32[count], data', parity') of the de-interleaved rows"""
    r = stream_to_rows(stream, size + oracle.nroots, count, I, M, phase)
    if positions is not None:
        return oracle.decode_batch(r[:, :size], r[:, size:], np.asarray(positions).astype(np.uint32),
                                   np.asarray(counts).astype(np.uint32), threads=threads)
    return oracle.decode_batch(r[:, :size], r[:, size:], threads=threads)


def expect_check(oracle, stream, size, count, I, M, phase):
    """dirty u8[count]: the oracle's nonzero-syndrome flag per codeword"""
    r = stream_to_rows(stream, size + oracle.nroots, count, I, M, phase)
    return oracle.syndrome_batch(r[:, :size], r[:, size:])[0]
