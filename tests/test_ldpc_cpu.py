"""LDPC host side without a device: config and handle creation, the getters, and
the graph (parity-check matrix, both interleavers) against the arrays recorded
from the reference's own handle (tests/golden/ldpc_golden.npz, written by
tools/gen_golden_ldpc.py), plus the live reference where oracle/_ref exists."""
import ctypes as C

import numpy as np
import pytest

import ldpc_ref as R
import libpoporon_amd as P


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


def make(code, **kw):
    args = dict(matrix_type=code["matrix"], column_weight=code["weight"], use_outer_interleave=code["outer"],
                use_inner_interleave=code["inner"], lifting_factor=code["lifting"], max_iterations=R.MAX_ITER,
                seed=code["seed"])
    args.update(kw)
    return P.Ldpc(code["block"], code["rate"], **args)


def test_getters_all_rates(gold):
    rows = gold["getters"]
    assert rows.shape == (18, 4)
    for block, rate, pb, ib in rows.tolist():
        h = P.Ldpc(block, rate)
        assert h.fec_type == P.POPORON_FEC_LDPC
        assert (h.parity_size, h.info_size) == (pb, ib)
        assert (ib, pb) == (R.sizes(block, rate)[0], R.sizes(block, rate)[2])
        assert h.iterations_used == 0
        assert h.supported
        h.close()
    assert R.sizes(32, 5) == (32, 51, 7)  # rate 5/6 at block 32: 51 parity bits in 7 bytes


@pytest.mark.parametrize("block,rate", [(28, 1), (34, 1), (8196, 1), (32, 6), (0, 1), (8192 + 4, 0)])
def test_create_refuses(block, rate):
    lib = P.load_library()
    cfg = lib.poporon_ldpc_config_create(block, rate, 1, 3, False, False, False, 0, 0, 0, None, 0, 0)
    assert cfg, "the config stores any arguments"
    assert not lib.poporon_create(cfg)
    lib.poporon_config_destroy(cfg)


def test_column_weight_clamped():
    for lo, hi, matrix in ((0, 3, R.RANDOM), (99, 8, R.RANDOM), (1, 3, R.QC), (9, 8, R.QC)):
        code = dict(R.CODES["A"], matrix=matrix)
        a, b = make(code, column_weight=lo).graph(), make(code, column_weight=hi).graph()
        assert a["num_edges"] == b["num_edges"]
        assert (a["row_ptr"] == b["row_ptr"]).all() and (a["col_idx"] == b["col_idx"]).all()


def _same_graph(g, want_dims, want):
    assert [g["num_checks"], g["num_bits"], g["num_edges"]] == list(want_dims[2:])
    for k in ("row_ptr", "col_idx", "inner_forward", "outer_forward"):
        if want(k) is None:
            assert g[k] is None, k
        else:
            assert g[k] is not None and g[k].shape == want(k).shape and (g[k] == want(k)).all(), k


@pytest.mark.parametrize("name", list(R.SMALL + "M"))
def test_graph_equals_recorded(gold, name):
    h = make(R.CODES[name])
    dims = gold[name + "_dims"].tolist()
    assert (h.parity_size, h.info_size) == tuple(dims[:2])
    g = h.graph()
    _same_graph(g, dims, lambda k: gold[f"{name}_{k}"] if f"{name}_{k}" in gold.files else None)
    assert g["row_ptr"][-1] == g["num_edges"] and g["col_idx"].max() < g["num_bits"]
    if name == "C":  # the QC builder dropped edges: fewer than info_bits * weight + 2 * parity_bits - 1
        assert g["num_edges"] < 256 * 4 + 2 * 51 - 1 and g["num_checks"] == 51
    if name == "A":
        assert g["num_edges"] == 1279
    if R.reference_available():
        ref = R.RefLdpc(R.CODES[name])
        rg = ref.graph()
        _same_graph(g, [0, 0, rg["num_checks"], rg["num_bits"], rg["num_edges"]], lambda k: rg[k])
        ref.close()


def test_graph_largest_code_hashes(gold):
    h = make(R.CODES["G"])
    g = h.graph()
    assert [h.parity_size, h.info_size, g["num_checks"], g["num_bits"], g["num_edges"]] == gold["G_dims"].tolist()
    assert g["num_edges"] == 786431 and g["num_bits"] == 196608
    assert g["inner_forward"] is None and g["outer_forward"] is None
    for k in ("row_ptr", "col_idx"):
        assert R.sha(g[k].astype(np.uint32)) == str(gold["G_" + k]), k


def test_explicit_interleave_depth_and_lifting_live():
    """Parameters the recorded codes do not cover, against the live reference
    (extra rows only: nothing to compare with where it was not built)."""
    if not R.reference_available():
        return
    for extra in (dict(block=64, rate=1, inner=True, outer=True, seed=(1 << 40) + 5),
                  dict(block=40, rate=4, matrix=R.QC, lifting=24, seed=2),
                  dict(block=128, rate=0, matrix=R.QC, weight=5, seed=0xFFFFFFFF)):
        code = dict(R.CODES["A"], **extra)
        ref = R.RefLdpc(code)
        rg = ref.graph()
        g = make(code).graph()
        _same_graph(g, [0, 0, rg["num_checks"], rg["num_bits"], rg["num_edges"]], lambda k: rg[k])
        ref.close()


def test_non_bijective_interleaver_is_not_served():
    """Code H: depth * width != codeword_bits, the inner forward table is no permutation."""
    h = make(R.CODES["H"])
    lib = h.lib
    assert h.h and h.fec_type == P.POPORON_FEC_LDPC
    assert (h.parity_size, h.info_size) == (7, 32)
    assert not h.supported
    f = h.graph()["inner_forward"]
    assert f.shape == (307,) and np.unique(f).size < f.size
    d, p = np.zeros(32, np.uint8), np.zeros(7, np.uint8)
    assert not lib.poporon_encode(h.h, d.ctypes.data, 32, p.ctypes.data)
    assert "permutation" in P.last_error()
    n = C.c_size_t(R.SENT)
    assert not lib.poporon_decode(h.h, d.ctypes.data, 32, p.ctypes.data, C.byref(n))
    assert n.value == R.SENT and "permutation" in P.last_error()
    dirty = np.zeros(1, np.uint8)
    assert not lib.poporon_ldpc_check_batch(h.h, d.ctypes.data, 32, p.ctypes.data, 7, 1, dirty.ctypes.data)
    assert "permutation" in P.last_error()
    # the same parameters with a depth that divides the codeword are served
    assert make(R.CODES["B"]).supported


def test_single_calls_refuse_wrong_size():
    h = make(R.CODES["A"])
    d, p = np.zeros(64, np.uint8), np.zeros(32, np.uint8)
    assert not h.lib.poporon_encode(h.h, d.ctypes.data, 31, p.ctypes.data)
    assert "info bytes" in P.last_error()
    n = C.c_size_t(R.SENT)
    assert not h.lib.poporon_decode(h.h, d.ctypes.data, 33, p.ctypes.data, C.byref(n))
    assert n.value == R.SENT


def test_rs_batch_calls_refuse_ldpc_handles():
    h = make(R.CODES["A"])
    lib, b = h.lib, np.zeros(256, np.uint8)
    q = b.ctypes.data
    assert not lib.poporon_encode_batch(h.h, q, 32, q, 32, 32, 1)
    assert "LDPC" in P.last_error()
    assert not lib.poporon_decode_batch(h.h, q, 32, q, 32, 32, 1, None, 0, None, q, q)
    assert not lib.poporon_encode_batch_device(h.h, q, 32, q, 32, 32, 1, None)
    assert not lib.poporon_decode_batch_device(h.h, q, 32, q, 32, 32, 1, None, 0, None, q, q, None)
    assert not lib.poporon_check_batch_device(h.h, q, 32, q, 32, 32, 1, q, None)
    assert not lib.poporon_amd_ldpc_graph(P.Bch().h, None, None, None, None, None, None, None)


def test_multi_handle_refuses_ldpc():
    lib = P.load_library()
    cfg = lib.poporon_ldpc_config_create(32, 1, 1, 3, False, False, False, 0, 0, 0, None, 0, 0)
    assert not lib.poporon_amd_multi_create(cfg, None, 0)
    lib.poporon_config_destroy(cfg)
