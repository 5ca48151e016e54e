"""The soft-decision RS decode without a GPU (poporon_decode_soft_batch_device, include/poporon_amd.h):
the numpy model of tests/soft_ref.py against a literal per-candidate loop of single oracle decodes, the
pick rule on hand-written rows, poporon_amd_soft_llr_row, every argument check of the call and of its
reserve (none of them reaches the GPU), the count-0 return, and the two new kernel ids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libpoporon_amd as P
import soft_ref as S

RS223 = (8, 0x11D, 1, 1, 32)
RS204 = (8, 0x11D, 0, 1, 16)  # RS(204,188)
RS15 = (4, 0x13, 1, 1, 4)     # RS(15,11) over GF(16)
X = 0x1000  # a non-NULL pointer that is never dereferenced
NAME = "poporon_decode_soft_batch_device"


def _oracle(params):
    from oracle import Oracle
    return Oracle(*params)


# ---- the model ----------------------------------------------------------------------------

@pytest.mark.parametrize("params,size", [(RS223, 223), (RS223, 40), (RS204, 188), (RS15, 11), (RS15, 1)])
def test_model_against_a_literal_loop(params, size):
    m, nr = params[0], params[4]
    o = _oracle(params)
    rng = np.random.default_rng([size, nr])
    for flips, weak, count in ((0, 0, 4), (0, 1, 4), (2, 2, 5), (2, 3, 5), (3, 1, 4), (4, 5, 3)):
        cw, llr = S.built_rows(o, size, m, count, weak, rng)
        llr[0, : min(6, llr.shape[1])] = 0  # ties among the least reliable bits
        got = S.soft_decode(o, llr, size, m, flips)
        for c in range(count):
            ok, y, changed, p, score = S.soft_decode_literal(o, llr[c], size, m, flips)
            assert (got["ok"][c], got["changed"][c], got["pattern"][c], got["score"][c]) == (ok, changed, p, score)
            assert got["rows"][c].tolist() == y
        if m == 8 and weak <= flips:  # within t after the right flips: the transmitted codeword
            assert got["ok"][1:].all() and (got["rows"][1:] == cw[1:]).all()


def test_flips_0_is_the_plain_decode_of_the_hard_rows():
    o = _oracle(RS223)
    rng = np.random.default_rng(5)
    cw, llr = S.built_rows(o, 223, 8, 12, 0, rng)
    _, over = S.built_rows(o, 223, 8, 4, 0, rng, total=17)
    llr = np.concatenate([llr, over])
    hard = S.hard_rows(llr, 255, 8)
    ok, _, d, p = o.decode_batch(hard[:, :223], hard[:, 223:])
    got = S.soft_decode(o, llr, 223, 8, 0)
    assert (got["ok"] == ok).all() and ok[:12].all() and not ok.all()
    good = ok != 0
    assert (got["rows"][good] == np.concatenate([d, p], 1)[good]).all()
    assert (got["rows"][~good] == hard[~good]).all() and not got["score"][~good].any()
    assert (got["pattern"] == 0).all()


def test_the_pick_rule_on_hand_written_rows():
    W, m = 15, 4
    n = W * m
    flat = np.full((1, n), 9, np.int8)  # all magnitudes equal: the lowest indices
    assert S.picks(flat, W, m, 6).tolist() == [[0, 1, 2, 3, 4, 5]]
    assert S.picks(-flat, W, m, 3).tolist() == [[0, 1, 2]]
    z = np.zeros((1, n), np.int8)  # zeros: bit 0 of every symbol is 0, the picks again the first
    assert S.picks(z, W, m, 4).tolist() == [[0, 1, 2, 3]] and not S.hard_rows(z, W, m).any()
    r = np.full((1, n), -128, np.int8)  # |-128| = 128, above 127
    r[0, 7] = 127
    r[0, 50] = -127
    r[0, 20] = 127
    assert S.picks(r, W, m, 4).tolist() == [[7, 20, 50, 0]]
    assert S.magnitudes(r, W, m)[0, 0] == 128 and (S.hard_rows(r, W, m)[0, 2:5] == 15).all()
    assert S.hard_rows(r, W, m)[0, 1] == 0b1110  # bit 7 = symbol 1's LSB, MSB first
    mixed = np.array([[5, -3, 3, 0, -1, 1, 3, -128] + [60] * (n - 8)], np.int8)
    assert S.picks(mixed, W, m, 6).tolist() == [[3, 4, 5, 1, 2, 6]]
    cand = S.candidates(mixed, W, m, 2)  # pick 0 = bit 3 (symbol 0, LSB), pick 1 = bit 4 (symbol 1, MSB)
    hard = S.hard_rows(mixed, W, m)[0]
    assert hard[:2].tolist() == [0b0100, 0b1001]
    assert [(c[:2] ^ hard[:2]).tolist() for c in cand[0]] == [[0, 0], [1, 0], [0, 8], [1, 8]]
    assert (cand[0][:, 2:] == hard[2:]).all()


# ---- poporon_amd_soft_llr_row ---------------------------------------------------------------

def test_soft_llr_row():
    lib = P.load_library()
    h = P.Poporon(*RS223)
    assert h.soft_llr_row(223) == 255 * 8 and h.soft_llr_row(1) == 33 * 8
    assert h.soft_llr_row(0) == 0 and h.soft_llr_row(224) == 0
    g = P.Poporon(*RS15)
    assert g.soft_llr_row(11) == 60 and g.soft_llr_row(1) == 20 and g.soft_llr_row(12) == 0
    assert lib.poporon_amd_soft_llr_row(None, 10) == 0
    assert lib.poporon_amd_soft_llr_row(P.Bch.default().h, 1) == 0
    assert lib.poporon_amd_soft_llr_row(P.Ldpc(32, P.LDPC_RATE_1_2).h, 1) == 0


# ---- argument checks ------------------------------------------------------------------------

def _call(h, llr=X, ls=2040, data=X, ds=223, par=X, ps=32, size=223, count=3, flips=2, ok=X, changed=None,
          pattern=None, score=None):
    return P.load_library().poporon_decode_soft_batch_device(h, llr, ls, data, ds, par, ps, size, count, flips, ok,
                                                             changed, pattern, score, None)


def _refused(word, *a, **k):
    assert _call(*a, **k) is False
    msg = P.last_error()
    assert NAME in msg and word in msg, msg


def test_null_handle_and_other_handles():
    lib = P.load_library()
    _refused("NULL handle", None)
    _refused("NULL handle", None, count=0)
    for h in (P.Bch.default(), P.Ldpc(32, P.LDPC_RATE_1_2)):
        _refused("RS handles", h.h)
        assert lib.poporon_amd_reserve_soft(h.h, 2, 10) is False and "RS handles" in P.last_error()
    assert lib.poporon_amd_reserve_soft(None, 2, 10) is False and "NULL handle" in P.last_error()


def test_size_and_flips():
    h = P.Poporon(*RS223)
    for size in (0, 224, 1 << 40):
        _refused("size %d outside [1, 223]" % size, h.h, size=size)
    _refused("size 0 outside", h.h, size=0, count=0)  # the limits hold at count 0 too
    _refused("flips 7 > 6", h.h, flips=7)
    _refused("flips 7 > 6", h.h, flips=7, count=0)
    _refused("flips 4294967295 > 6", h.h, flips=0xFFFFFFFF)
    tiny = P.Poporon(2, 0x7, 1, 1, 1)  # RS(3,2) over GF(4): a row of size 1 has 4 bits
    assert tiny.soft_llr_row(1) == 4
    _refused("flips 5 > the 4 bits of a codeword", tiny.h, size=1, flips=5, ls=4, ds=1, ps=1)
    lib = P.load_library()
    assert lib.poporon_amd_reserve_soft(h.h, 7, 10) is False
    assert "poporon_amd_reserve_soft" in P.last_error() and "flips 7 > 6" in P.last_error()


def test_strides():
    h = P.Poporon(*RS223)
    _refused("llr_stride 2039 < (size + num_roots) * symbol_size = 2040", h.h, ls=2039)
    _refused("llr_stride 0 <", h.h, ls=0, count=1)
    _refused("data_stride 222 < size 223", h.h, ds=222)
    _refused("parity_stride 31 < num_roots 32", h.h, ps=31)
    _refused("llr_stride 575 < (size + num_roots) * symbol_size = 576", h.h, size=40, ls=575, ds=40)
    g = P.Poporon(*RS15)
    _refused("llr_stride 59 <", g.h, size=11, ls=59, ds=11, ps=4)
    _refused("parity_stride 3 < num_roots 4", g.h, size=11, ls=60, ds=11, ps=3)


def test_null_arguments():
    h = P.Poporon(*RS223)
    for name in ("llr", "data", "par", "ok"):
        _refused("NULL argument", h.h, **{name: None})


def test_count_zero_succeeds_without_a_gpu_call():
    h = P.Poporon(*RS223)
    assert _call(h.h, count=0) is True, P.last_error()
    assert _call(h.h, count=0, llr=None, data=None, par=None, ok=None) is True, P.last_error()
    h.decode_soft_batch_device(0, 2040, 0, 223, 0, 32, 223, 0, 6, 0)
    with pytest.raises(P.PoporonError, match="flips 9 > 6"):
        h.decode_soft_batch_device(X, 2040, X, 223, X, 32, 223, 1, 9, X)


# ---- names and ids ------------------------------------------------------------------------

def test_kernel_ids_and_names():
    text = open(os.path.join(P.INCLUDE_DIR, "poporon_amd.h")).read()
    ids = dict(re.findall(r"POPORON_AMD_KERNEL_(SOFT_\w+) = (\d+)", text))
    assert ids == {"SOFT_EXPAND": "27", "SOFT_SELECT": "28"}
    assert not re.search(r"#define\s+POPORON_AMD_KERNEL_SOFT", text)
    assert (P.KERNEL_SOFT_EXPAND, P.KERNEL_SOFT_SELECT) == (27, 28)
    assert sorted(P.SOFT_KERNEL_NAMES) == [27, 28]
    others = set(P.KERNEL_NAMES) | set(P.CONV_KERNEL_NAMES) | set(P.PLANE_KERNEL_NAMES) | set(P.PROD_KERNEL_NAMES)
    assert not set(P.SOFT_KERNEL_NAMES) & others


def test_every_new_symbol_is_bound():
    names = [n for n in P.header_symbols() if "soft" in n]
    assert sorted(names) == sorted(["poporon_amd_soft_llr_row", "poporon_amd_reserve_soft",
                                    "poporon_decode_soft_batch_device"])
    lib = P.load_library()
    assert all(hasattr(lib, n) and n in P._SIGS for n in names)
    sig = P._SIGS["poporon_decode_soft_batch_device"]
    assert sig[0] is C.c_bool and len(sig[1]) == 15
