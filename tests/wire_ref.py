"""Wire forms of the interleaved calls against the oracle (helper, no tests).

A handle's wire form (include/poporon_amd.h) is a symbol map to_code / to_wire
and a receive-side XOR sequence.  A byte of a frame at block offset b (message
region: its offset in the region; parity region: size*depth + its offset) is
the code byte to_code[wire ^ seq[b % len(seq)]].  ``to_code_frames`` and
``to_wire_frames`` are that map and its inverse in numpy; ``expect_*`` put
them around tests/interleave_ref.py, which holds the reference's answer on the
code bytes.  None for a map is the identity, None for the sequence is none.
"""
import numpy as np

import interleave_ref as R


def _seq_at(seq, start, n):
    seq = np.asarray(seq, dtype=np.uint8)
    return seq[(start + np.arange(n)) % seq.size]


def to_code_frames(frames, parity, depth, to_code=None, seq=None):
    """wire regions u8[count, size*depth], u8[count, nr*depth] -> the code bytes of both"""
    d, p = np.asarray(frames, dtype=np.uint8), np.asarray(parity, dtype=np.uint8)
    assert d.shape[1] % depth == 0 and p.shape[1] % depth == 0
    if seq is not None:
        d, p = d ^ _seq_at(seq, 0, d.shape[1]), p ^ _seq_at(seq, d.shape[1], p.shape[1])
    if to_code is not None:
        d, p = np.asarray(to_code, dtype=np.uint8)[d], np.asarray(to_code, dtype=np.uint8)[p]
    return d, p


def to_wire_frames(frames, parity, depth, to_wire=None, seq=None):
    """the inverse: code bytes -> wire regions (mapped, then randomized)"""
    d, p = np.asarray(frames, dtype=np.uint8), np.asarray(parity, dtype=np.uint8)
    assert d.shape[1] % depth == 0 and p.shape[1] % depth == 0
    if to_wire is not None:
        d, p = np.asarray(to_wire, dtype=np.uint8)[d], np.asarray(to_wire, dtype=np.uint8)[p]
    if seq is not None:
        d, p = d ^ _seq_at(seq, 0, d.shape[1]), p ^ _seq_at(seq, d.shape[1], p.shape[1])
    return d, p


def expect_encode(oracle, frames, depth, to_code=None, to_wire=None, threads=0):
    """parity regions in wire symbols of message regions in wire symbols; an encode uses no sequence"""
    fr = np.asarray(frames, dtype=np.uint8)
    code = fr if to_code is None else np.asarray(to_code, dtype=np.uint8)[fr]
    par = R.expect_encode(oracle, code, depth, threads=threads)
    return par if to_wire is None else np.asarray(to_wire, dtype=np.uint8)[par]


def expect_decode(oracle, frames, parity, depth, to_code=None, to_wire=None, seq=None, positions=None, counts=None,
                  threads=0):
    """(ok, corrected, frames', parity', code_in, code_out): both regions come back in wire symbols,
    derandomized and not re-randomized, failed codewords too; code_in / code_out are the (message,
    parity) regions in code bytes before and after the reference's decode"""
    cd, cp = to_code_frames(frames, parity, depth, to_code, seq)
    ok, cor, dd, pp = R.expect_decode(oracle, cd, cp, depth, positions, counts, threads=threads)
    wd, wp = to_wire_frames(dd, pp, depth, to_wire, None)
    return ok, cor, wd, wp, (cd, cp), (dd, pp)


def expect_check(oracle, frames, parity, depth, to_code=None, seq=None):
    """dirty u8[count*depth] of the code bytes"""
    return R.expect_check(oracle, *to_code_frames(frames, parity, depth, to_code, seq), depth)
