"""numpy model of poporon_cc_decode_siso_device (include/poporon_amd.h): a restatement of the header's
max-log-MAP contract, nothing shared with cc_soft.hip.  Tables, branch costs and depuncturing are those of
tests/cc_ref.py; "no path" is the contract's 2^28, added like any other cost (not cc_ref.INF).

The forward metrics A and the backward metrics Z run over the 64 states and over all blocks of a frame at once,
with a Python loop over the at most B + 2V steps of a window; A is kept for every step of the window."""
import numpy as np

import cc_ref as R

NO_PATH = 1 << 28


def _successors(code):
    """succ[u][s], label[u][s] of the branch that input u takes from state s"""
    pred, lab = R._tables(code)
    succ = np.zeros((2, 64), np.int64)
    slab = np.zeros((2, 64), np.int64)
    for s in range(64):
        for u in (0, 1):
            s2 = (u << 5) | (s >> 1)
            d = s & 1
            assert pred[d, s2] == s
            succ[u, s], slab[u, s] = s2, lab[d, s2]
    return succ, slab


def quantise(x, shift):
    """D_1 - D_0 -> the int8 of the contract"""
    x = np.asarray(x, np.int64)
    mag = np.minimum(127, np.abs(x) >> shift)
    return np.where(x > 0, mag, -mag).astype(np.int8)


def decode_soft(code, punct, llr, nbits, block, overlap, start_state=-1, end_state=-1, shift=0):
    """one frame: (soft int8[nbits], D int64[nbits, 2]) with D[t, b] the least A + Z of step t over input b"""
    pred, lab = R._tables(code)
    succ, slab = _successors(code)
    v = R.depuncture(punct, llr, nbits)
    nb = R.n_blocks(block, nbits)
    e0 = np.arange(nb, dtype=np.int64) * block
    e1 = np.minimum(nbits, e0 + block)
    t0 = np.maximum(0, e0 - overlap)
    t1 = np.minimum(nbits, e0 + block + overlap)
    n = t1 - t0
    steps = int(n.max())
    rows = np.arange(nb)[:, None]
    A = np.zeros((steps + 1, nb, 64), np.int64)
    if start_state >= 0:
        first = t0 == 0
        A[0, first] = NO_PATH
        A[0, first, start_state] = 0
    for i in range(steps):
        live = i < n
        cost = R._costs(v[np.minimum(t0 + i, nbits - 1)])  # [nb, 4]
        m0 = A[i][:, pred[0]] + cost[rows, lab[0][None, :]]
        m1 = A[i][:, pred[1]] + cost[rows, lab[1][None, :]]
        A[i + 1] = np.where(live[:, None], np.minimum(m0, m1), A[i])
    Z = np.zeros((nb, 64), np.int64)  # of a block whose window has fewer steps: Z_n until the loop reaches n - 1
    if end_state >= 0:
        last = t1 == nbits
        Z[last] = NO_PATH
        Z[last, end_state] = 0
    D = np.zeros((nbits, 2), np.int64)
    for i in range(steps - 1, -1, -1):
        live = i < n
        t = t0 + i
        emit = live & (t >= e0) & (t < e1)
        total = A[i + 1] + Z  # A and Z after step i
        D[t[emit], 0] = total[emit, :32].min(1)
        D[t[emit], 1] = total[emit, 32:].min(1)
        cost = R._costs(v[np.minimum(t, nbits - 1)])
        z0 = cost[rows, slab[0][None, :]] + Z[:, succ[0]]
        z1 = cost[rows, slab[1][None, :]] + Z[:, succ[1]]
        Z = np.where(live[:, None], np.minimum(z0, z1), Z)
    return quantise(D[:, 1] - D[:, 0], shift), D
