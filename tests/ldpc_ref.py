"""Shared by the LDPC tests and tools/gen_golden_ldpc.py (not a test module).

* CODES: the test codes A-H (+ M, a code whose messages need more than 64 KiB of LDS).
* SWEEP: the edge-shaped codes of tests/test_gpu_ldpc_sweep.py and their seeded rows.
* Seeded inputs (numpy Generators).  The golden file records the SHA-256 of
  every input array next to the reference's outputs, so a numpy whose streams
  differ fails loudly instead of comparing against the wrong rows.
* RefLdpc: ctypes binding of the real reference (oracle/_ref/libpoporon_ref.so,
  built by oracle/Makefile where the reference's sources are present) through its
  public API, with a layout mirror of its handle for the graph and the decoder's
  codeword buffer.  The tests use it live where it exists; the golden file alone
  is enough to run them.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libpoporon_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ldpc_golden.npz")

RANDOM, QC = 1, 2
# rate ids: 0 = 1/3, 1 = 1/2, 2 = 2/3, 3 = 3/4, 4 = 4/5, 5 = 5/6
CODES = {
    "A": dict(block=32, rate=1, matrix=RANDOM, weight=3, outer=False, inner=False, lifting=0, seed=0),
    "B": dict(block=32, rate=0, matrix=RANDOM, weight=3, outer=True, inner=True, lifting=0, seed=7),
    "C": dict(block=32, rate=5, matrix=QC, weight=4, outer=False, inner=False, lifting=0, seed=1),
    "D": dict(block=64, rate=2, matrix=QC, weight=3, outer=True, inner=False, lifting=16, seed=3),
    "E": dict(block=36, rate=3, matrix=RANDOM, weight=8, outer=True, inner=True, lifting=0, seed=9),
    "F": dict(block=32, rate=1, matrix=RANDOM, weight=7, outer=True, inner=True, lifting=0, seed=0),
    "G": dict(block=8192, rate=0, matrix=RANDOM, weight=8, outer=False, inner=False, lifting=0, seed=5),
    "H": dict(block=32, rate=5, matrix=RANDOM, weight=3, outer=False, inner=True, lifting=0, seed=0),
    # 98 KiB of messages: the LDS placement past the 64 KiB a kernel gets without asking
    "M": dict(block=512, rate=1, matrix=RANDOM, weight=3, outer=True, inner=True, lifting=0, seed=11),
}
SMALL = "ABCDEF"
SOFT = "ACF"
MAX_ITER = 20
ENC_ROWS = 257
FLIPS = (0, 1, 2, 4, 8, 16)
ROWS_PER_FLIP = 64
SIGMAS = (0.5, 0.8, 1.0)
SOFT_EXTRA = 16
SENT = 777

# The sweep codes (tests/golden/ldpc_sweep_golden.npz, tools/gen_golden_ldpc_sweep.py): shapes at
# which ldpc.hip takes paths of its own.  "depth" is poporon_ldpc_config_create's interleave_depth.
SWEEP_GOLDEN = os.path.join(ROOT, "tests", "golden", "ldpc_sweep_golden.npz")
SWEEP = {
    # inner interleaver with spare bits in parity and codeword (341 bits); a seed past 2^32
    "S1": dict(block=32, rate=3, matrix=RANDOM, weight=3, outer=True, inner=True, depth=11, lifting=0,
               seed=(1 << 32) + 17),
    # the same with QC; 117 check rows: one full wave and a partial one
    "S2": dict(block=44, rate=3, matrix=QC, weight=4, outer=False, inner=True, depth=7, lifting=0, seed=2),
    # fewer than 64 check rows; row degree up to 41
    "S3": dict(block=36, rate=5, matrix=RANDOM, weight=5, outer=True, inner=True, depth=15, lifting=0, seed=3),
    # 260 parity bytes: encode's prefix pass has runs of 2 bytes, lanes 130-255 empty
    "S4": dict(block=260, rate=1, matrix=RANDOM, weight=4, outer=True, inner=True, depth=65, lifting=0, seed=4),
    # weight 8; 512 check rows: two full passes of the encode loop
    "S5": dict(block=32, rate=0, matrix=RANDOM, weight=8, outer=False, inner=False, depth=0, lifting=0, seed=5),
    # a lifting factor that is no power of two, 4 x 24 > 80 check rows: edges are dropped
    "S6": dict(block=40, rate=4, matrix=QC, weight=3, outer=True, inner=False, depth=0, lifting=24, seed=6),
    # decode LDS 65,184 B (the last size that needs no attribute), 65,968 B (the first that does),
    # 163,744 B (96 B under LDPC_LDS_MAX, yet past what the kernel's static LDS leaves of it: the
    # workspace) and 164,512 B (past LDPC_LDS_MAX: the workspace)
    "W336": dict(block=336, rate=1, matrix=RANDOM, weight=3, outer=False, inner=False, depth=0, lifting=0, seed=7),
    "W340": dict(block=340, rate=1, matrix=RANDOM, weight=3, outer=False, inner=False, depth=0, lifting=0, seed=42),
    "W844": dict(block=844, rate=1, matrix=RANDOM, weight=3, outer=False, inner=False, depth=0, lifting=0, seed=9),
    # seed 30: a check row with a single edge
    "W848": dict(block=848, rate=1, matrix=RANDOM, weight=3, outer=True, inner=False, depth=0, lifting=0, seed=30),
    # 162,960 B: the largest block of this family whose messages do fit the LDS
    "W840": dict(block=840, rate=1, matrix=RANDOM, weight=3, outer=False, inner=False, depth=0, lifting=0, seed=10),
}
# W340 with the automatic inner depth: the table is no permutation, the handle is not served
SWEEP_REFUSED = dict(SWEEP["W340"], inner=True)
SWEEP_SEED = 0x53574550
SWEEP_SOFT_ROWS = 22


def sweep_large(code):
    return code["block"] > 200


def sweep_enc_inputs(name):
    code = SWEEP[name]
    rng = np.random.default_rng([SWEEP_SEED, list(SWEEP).index(name), 1])
    return rng.integers(0, 256, (12 if sweep_large(code) else 48, code["block"]), dtype=np.uint8)


def sweep_flip_one(name, enc_data, enc_parity, codeword_bits):
    """Every encoded row with one bit of the codeword flipped."""
    rng = np.random.default_rng([SWEEP_SEED, list(SWEEP).index(name), 2])
    bits = rng.integers(0, codeword_bits, enc_data.shape[0])
    row = np.concatenate([enc_data, enc_parity], axis=1)
    row[np.arange(len(row)), bits // 8] ^= (0x80 >> (bits % 8)).astype(np.uint8)
    ib = enc_data.shape[1]
    return np.ascontiguousarray(row[:, :ib]), np.ascontiguousarray(row[:, ib:])


def sweep_hard_rows(name, enc_data, enc_parity, seed=4):
    """flip_rows with the sweep's flip counts: 0, 1, 3, 8, 30 x 16 rows, or 0, 2, 20, 300 x 4 for
    the large blocks."""
    code = SWEEP[name]
    flips, per = ((0, 2, 20, 300), 4) if sweep_large(code) else ((0, 1, 3, 8, 30), 16)
    rng_seed = int(np.random.default_rng([SWEEP_SEED, list(SWEEP).index(name), seed]).integers(1 << 62))
    return flip_rows(enc_data, enc_parity, flips=flips, per=per, seed=rng_seed)


def sweep_soft_rows(name, enc_data, enc_parity, codeword_bits, seed=5):
    """22 LLR rows in channel order that reach the saturated regime (|llr| >= 126 gives
    |llr * 256| > 32000), and junk data / parity the soft path must not read:
      12  codeword signs at magnitude 127, 16 and 1, four rows each, 4 % of the positions negated
       4  codeword signs at 127, 3 % of the positions set to -128 or 0
       1  all 0;  1  all -128;  1  all 127
       3  drawn from {-128, -127, 127}"""
    rng = np.random.default_rng([SWEEP_SEED, list(SWEEP).index(name), seed])
    bits = np.unpackbits(np.concatenate([enc_data, enc_parity], axis=1), axis=1)[:, :codeword_bits].astype(np.int64)
    sign = 1 - 2 * bits[rng.integers(0, enc_data.shape[0], 16)]
    out = []
    for k, mag in enumerate((127, 16, 1)):
        s = sign[4 * k:4 * k + 4] * mag
        out.append(np.where(rng.random(s.shape) < 0.04, -s, s))
    s = sign[12:16] * 127
    hit = rng.random(s.shape) < 0.03
    out.append(np.where(hit, np.where(rng.random(s.shape) < 0.5, -128, 0), s))
    for v in (0, -128, 127):
        out.append(np.full((1, codeword_bits), v, np.int64))
    out.append(np.array([-128, -127, 127])[rng.integers(0, 3, (3, codeword_bits))])
    llr = np.ascontiguousarray(np.concatenate(out).astype(np.int8))
    assert llr.shape[0] == SWEEP_SOFT_ROWS
    junk_d = rng.integers(0, 256, (llr.shape[0], enc_data.shape[1]), dtype=np.uint8)
    junk_p = rng.integers(0, 256, (llr.shape[0], enc_parity.shape[1]), dtype=np.uint8)
    return llr, junk_d, junk_p


SINGLE_EDGE_LLR = (-117, -118, -119, -120, -125, -128)


def sweep_single_edge_rows(graph):
    """LLR rows in channel order for a graph (row_ptr, col_idx, inner_forward) with a check row of
    one edge.  Such a row has no second minimum: its edge gets the start value of the minima,
    32000 * 15 / 16 = +30000, every iteration.  The bit on that edge is given an LLR whose channel
    term, llr * 256, lies within a few hundred of -30000, every other bit 0 (and, in a second set,
    +1), so the sign of that bit's total is the sign of channel + 30000: a start value that is off
    by a little changes the hard decision."""
    row_ptr = np.asarray(graph["row_ptr"], dtype=np.int64)
    rows = np.nonzero(np.diff(row_ptr) == 1)[0]
    assert rows.size, "no check row with a single edge"
    bit = int(graph["col_idx"][row_ptr[rows[0]]])
    n = int(graph["num_bits"])
    pos = bit if graph["inner_forward"] is None else int(graph["inner_forward"][bit])
    llr = np.zeros((2 * len(SINGLE_EDGE_LLR), n), np.int8)
    llr[len(SINGLE_EDGE_LLR):] = 1
    llr[:, pos] = SINGLE_EDGE_LLR * 2
    return llr


def decode_lds_bytes(num_edges, num_bits):
    """Dynamic LDS of ldpc_decode_k<true>: three int16 arrays (two per edge, one per bit) and the
    row's byte image, each rounded up to 16 bytes."""
    r16 = lambda v: (v + 15) & ~15  # noqa: E731
    return r16(2 * (2 * num_edges + num_bits)) + r16((num_bits + 7) // 8)


_NUM = {0: (1, 2), 1: (1, 1), 2: (2, 1), 3: (3, 1), 4: (4, 1), 5: (5, 1)}


def sizes(block, rate):
    """(info_bytes, parity_bits, parity_bytes) of the issue's size rule."""
    i, p = _NUM[rate]
    pbits = block * 8 * p // i
    return block, pbits, (pbits + 7) // 8


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def config_args(code, max_iterations=MAX_ITER, soft=False, llr_ptr=None, llr_size=0):
    """poporon_ldpc_config_create's 13 arguments."""
    return (code["block"], code["rate"], code["matrix"], code["weight"], soft, code["outer"], code["inner"],
            code.get("depth", 0), code["lifting"], max_iterations, llr_ptr, llr_size, code["seed"])


# ---- seeded inputs ---------------------------------------------------------------------

def enc_inputs(name, rows=ENC_ROWS):
    return np.random.default_rng([ord(name), 10]).integers(0, 256, (rows, CODES[name]["block"]), dtype=np.uint8)


def flip_rows(enc_data, enc_parity, flips=FLIPS, per=ROWS_PER_FLIP, seed=1):
    """Received rows for the hard path: for every flip count, `per` encoded rows
    (drawn with replacement) with that many distinct bits flipped over all data
    and parity bytes.  Returns (src, data, parity, nflip)."""
    rng = np.random.default_rng(seed)
    ib, pb = enc_data.shape[1], enc_parity.shape[1]
    src, dd, pp, nf = [], [], [], []
    for f in flips:
        s = rng.integers(0, enc_data.shape[0], per)
        row = np.concatenate([enc_data[s], enc_parity[s]], axis=1)
        for r in range(per):
            for b in rng.permutation(8 * (ib + pb))[:f]:
                row[r, b // 8] ^= np.uint8(0x80 >> (b % 8))
        src.append(s)
        dd.append(row[:, :ib])
        pp.append(row[:, ib:])
        nf.append(np.full(per, f))
    return (np.concatenate(src), np.ascontiguousarray(np.concatenate(dd)), np.ascontiguousarray(np.concatenate(pp)),
            np.concatenate(nf))


def soft_rows(name, enc_data, enc_parity, codeword_bits):
    """LLR rows in channel order: clip(rint((1 - 2b + N(0, sigma)) * 16), -127, 127) over the
    bits b of encoded rows, 64 rows per sigma, then 16 rows of uniform int8 that start with
    -128, 0, 127; and junk data / parity rows the soft path must not read."""
    rng = np.random.default_rng([ord(name), 30])
    bits = np.unpackbits(np.concatenate([enc_data, enc_parity], axis=1), axis=1)[:, :codeword_bits].astype(np.float64)
    out = []
    for sg in SIGMAS:
        s = rng.integers(0, enc_data.shape[0], ROWS_PER_FLIP)
        y = 1.0 - 2.0 * bits[s] + rng.normal(0.0, sg, (ROWS_PER_FLIP, codeword_bits))
        out.append(np.clip(np.rint(y * 16.0), -127, 127).astype(np.int8))
    u = rng.integers(-128, 128, (SOFT_EXTRA, codeword_bits)).astype(np.int8)
    u[:, 0], u[:, 1], u[:, 2] = -128, 0, 127
    out.append(u)
    llr = np.ascontiguousarray(np.concatenate(out))
    junk_d = rng.integers(0, 256, (llr.shape[0], enc_data.shape[1]), dtype=np.uint8)
    junk_p = rng.integers(0, 256, (llr.shape[0], enc_parity.shape[1]), dtype=np.uint8)
    return llr, junk_d, junk_p


def g_inputs():
    """Code G: 2 messages; flips of row 0 (few) and row 1 (many) over the codeword bytes."""
    rng = np.random.default_rng(0x6)
    data = rng.integers(0, 256, (2, CODES["G"]["block"]), dtype=np.uint8)
    nbits = 8 * (8192 + 16384)
    flips = [rng.permutation(nbits)[:8], rng.permutation(nbits)[:2000]]
    return data, flips


def apply_flips(data, parity, flips):
    row = np.concatenate([data, parity])
    for b in flips:
        row[b // 8] ^= np.uint8(0x80 >> (b % 8))
    return row[:data.size].copy(), row[data.size:].copy()


def deinterleave(rows, inner_forward, codeword_bits):
    """The reference's deinterleave_bits on byte rows: out bit k = in bit forward[k]."""
    if inner_forward is None:
        return rows.copy()
    bits = np.unpackbits(rows, axis=1)
    out = np.zeros_like(bits)
    out[:, :codeword_bits] = bits[:, np.asarray(inner_forward, dtype=np.int64)]
    return np.packbits(out, axis=1)


# ---- the real reference ------------------------------------------------------------------

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_i16p = C.POINTER(C.c_int16)


class _Params(C.Structure):  # src/internal/ldpc.h:19-27
    _fields_ = [("matrix_type", C.c_int), ("column_weight", C.c_uint32), ("use_inner_interleave", C.c_bool),
                ("use_outer_interleave", C.c_bool), ("interleave_depth", C.c_uint32), ("lifting_factor", C.c_uint32),
                ("seed", C.c_uint64)]


class _Sparse(C.Structure):  # :51-57
    _fields_ = [("row_ptr", _u32p), ("col_idx", _u32p), ("num_checks", C.c_uint32), ("num_bits", C.c_uint32),
                ("num_edges", C.c_uint32)]


class _Cols(C.Structure):  # :59-63
    _fields_ = [("col_ptr", _u32p), ("row_idx", _u32p), ("edge_idx", _u32p)]


class _Msg(C.Structure):  # :65-69
    _fields_ = [("check_to_var", _i16p), ("var_to_check", _i16p), ("llr_total", _i16p)]


class _Inner(C.Structure):  # :71-76
    _fields_ = [("forward", _u32p), ("inverse", _u32p), ("size", C.c_size_t), ("depth", C.c_uint32)]


class _Outer(C.Structure):  # :78-82
    _fields_ = [("forward", _u32p), ("inverse", _u32p), ("size", C.c_size_t)]


class _RefLdpc(C.Structure):  # :84-103
    _fields_ = [("rate", C.c_int), ("config", _Params), ("info_bits", C.c_size_t), ("parity_bits", C.c_size_t),
                ("codeword_bits", C.c_size_t), ("info_bytes", C.c_size_t), ("parity_bytes", C.c_size_t),
                ("codeword_bytes", C.c_size_t), ("parity_matrix", _Sparse), ("parity_matrix_cols", _Cols),
                ("msg", _Msg), ("interleaver", _Inner), ("outer_interleaver", _Outer), ("temp_codeword", _u8p),
                ("temp_interleaved", _u8p), ("temp_outer", _u8p)]


class _RefHandle(C.Structure):  # src/internal/common.h:74-100 (fec_type + ctx.ldpc)
    _fields_ = [("fec_type", C.c_int), ("ldpc", C.POINTER(_RefLdpc)), ("soft_llr", C.c_void_p),
                ("soft_llr_size", C.c_size_t), ("max_iterations", C.c_uint32), ("last_iterations", C.c_uint32),
                ("use_soft_decode", C.c_bool)]


def reference_available(so=REF_SO):
    return os.path.exists(so)


def _buf(a):
    return a.ctypes.data_as(C.c_void_p)


class RefLdpc:
    """The reference's LDPC handle through poporon_ldpc_config_create / poporon_create /
    poporon_encode / poporon_decode.  soft=True gives the handle an LLR buffer (set_llr)."""

    def __init__(self, code, max_iterations=MAX_ITER, soft=False, so=REF_SO):
        lib = C.CDLL(so)
        self.lib = lib
        lib.poporon_ldpc_config_create.restype = C.c_void_p
        lib.poporon_ldpc_config_create.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_uint32, C.c_bool, C.c_bool,
                                                   C.c_bool, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                   C.c_size_t, C.c_uint64]
        lib.poporon_create.restype = C.POINTER(_RefHandle)
        lib.poporon_create.argtypes = [C.c_void_p]
        lib.poporon_config_destroy.argtypes = [C.c_void_p]
        lib.poporon_destroy.argtypes = [C.POINTER(_RefHandle)]
        for f in (lib.poporon_encode, lib.poporon_decode):
            f.restype = C.c_bool
        lib.poporon_encode.argtypes = [C.POINTER(_RefHandle), C.c_void_p, C.c_size_t, C.c_void_p]
        lib.poporon_decode.argtypes = [C.POINTER(_RefHandle), C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.POINTER(C.c_size_t)]
        lib.poporon_get_iterations_used.restype = C.c_uint32
        lib.poporon_get_iterations_used.argtypes = [C.POINTER(_RefHandle)]
        for f in (lib.poporon_get_parity_size, lib.poporon_get_info_size):
            f.restype = C.c_size_t
            f.argtypes = [C.POINTER(_RefHandle)]
        lib.poporon_ldpc_check.restype = C.c_bool
        lib.poporon_ldpc_check.argtypes = [C.POINTER(_RefLdpc), C.c_void_p]
        lib.poporon_ldpc_deinterleave.restype = C.c_bool
        lib.poporon_ldpc_deinterleave.argtypes = [C.POINTER(_RefLdpc), C.c_void_p, C.c_void_p]
        ib, pbits, pb = sizes(code["block"], code["rate"])
        self.llr = np.zeros(8 * ib + pbits, np.int8) if soft else None
        cfg = lib.poporon_ldpc_config_create(*config_args(code, max_iterations, soft,
                                                          _buf(self.llr) if soft else None,
                                                          self.llr.size if soft else 0))
        self.h = lib.poporon_create(cfg)
        lib.poporon_config_destroy(cfg)
        if not self.h:
            raise RuntimeError("reference poporon_create returned NULL")
        self.s = self.h.contents.ldpc.contents
        self.info_bytes, self.parity_bytes = int(self.s.info_bytes), int(self.s.parity_bytes)
        self.codeword_bits, self.codeword_bytes = int(self.s.codeword_bits), int(self.s.codeword_bytes)
        self.inner = bool(self.s.interleaver.forward)

    def close(self):
        if getattr(self, "h", None):
            self.lib.poporon_destroy(self.h)
            self.h = None

    __del__ = close

    def getters(self):
        return int(self.lib.poporon_get_parity_size(self.h)), int(self.lib.poporon_get_info_size(self.h))

    def graph(self):
        s = self.s
        arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if p else None  # noqa: E731
        row_ptr = arr(s.parity_matrix.row_ptr, s.parity_matrix.num_checks + 1)
        return dict(num_checks=int(s.parity_matrix.num_checks), num_bits=int(s.parity_matrix.num_bits),
                    num_edges=int(row_ptr[-1]), row_ptr=row_ptr, col_idx=arr(s.parity_matrix.col_idx, int(row_ptr[-1])),
                    inner_forward=arr(s.interleaver.forward, self.codeword_bits),
                    outer_forward=arr(s.outer_interleaver.forward, self.info_bytes))

    def encode(self, data):
        d = np.array(data, dtype=np.uint8, copy=True)
        p = np.zeros(self.parity_bytes, np.uint8)
        assert self.lib.poporon_encode(self.h, _buf(d), d.size, _buf(p))
        return d, p

    def set_llr(self, llr):
        self.llr[...] = llr

    def decode(self, data, parity, corrected_init=SENT):
        """(ok, corrected_num, iterations_used, data', hard): hard is the decoder's codeword
        buffer after poporon_ldpc_decode_hard / _soft (src/decode.c:501-513)."""
        d = np.array(data, dtype=np.uint8, copy=True)
        p = np.array(parity, dtype=np.uint8, copy=True)
        n = C.c_size_t(corrected_init)
        ok = bool(self.lib.poporon_decode(self.h, _buf(d), d.size, _buf(p), C.byref(n)))
        buf = self.s.temp_interleaved if (self.s.config.use_inner_interleave and self.s.temp_interleaved) \
            else self.s.temp_codeword
        hard = np.ctypeslib.as_array(buf, shape=(self.codeword_bytes,)).copy()
        return ok, int(n.value), int(self.lib.poporon_get_iterations_used(self.h)), d, hard

    def dirty(self, data, parity):
        """The de-interleaved row's syndrome is non-zero."""
        cw = np.concatenate([np.asarray(data, np.uint8), np.asarray(parity, np.uint8)])
        out = np.zeros_like(cw)
        assert self.lib.poporon_ldpc_deinterleave(self.h.contents.ldpc, _buf(cw), _buf(out))
        return not self.lib.poporon_ldpc_check(self.h.contents.ldpc, _buf(out))
