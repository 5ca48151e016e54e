"""The numpy LDPC model (tests/ldpc_model.py) pinned to the reference, without a device.

The GPU sweep (tests/test_gpu_ldpc_sweep.py) compares the kernels with the model, so the
model itself has to equal the reference: here it reproduces every recorded array of
tests/golden/ldpc_golden.npz for codes A-F and M (on the recorded graph: neither the
library nor the reference is needed), the whole sweep fixture
tests/golden/ldpc_sweep_golden.npz (tools/gen_golden_ldpc_sweep.py), and, where
oracle/_ref exists, the live reference on further rows.  The library's graph of every
sweep code is compared with the fixture's dims and SHA-256s.
"""
import numpy as np
import pytest

import ldpc_model as M
import ldpc_ref as R
import libpoporon_amd as P


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def sweep():
    return np.load(R.SWEEP_GOLDEN)


def _eq(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, recorded {want.shape}"
    bad = (got != want) if got.ndim == 1 else (got != want).any(1)
    assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0][:8].tolist()} differ ({int(bad.sum())} of {len(bad)})"


def _cor(ok, it):
    """corrected_num as the caller sees it: the iteration count, or the sentinel left in place."""
    return np.where(ok == 1, it, R.SENT)


# ---- the recorded codes ------------------------------------------------------------------

def _recorded_graph(gold, name):
    k = lambda s: gold[f"{name}_{s}"] if f"{name}_{s}" in gold.files else None  # noqa: E731
    dims = gold[name + "_dims"].tolist()
    g = M.graph(k("row_ptr"), k("col_idx"), 8 * dims[1], k("inner_forward"), k("outer_forward"))
    assert [g["num_checks"], g["num_bits"], g["num_edges"]] == dims[2:]
    return g


@pytest.mark.parametrize("name", list(R.SMALL + "M"))
def test_model_equals_recorded(gold, name):
    code = R.CODES[name]
    g = _recorded_graph(gold, name)
    k = lambda s: gold[f"{name}_{s}"]  # noqa: E731
    rows = R.ENC_ROWS if name != "M" else 8
    msgs = R.enc_inputs(name, rows)
    assert R.sha(msgs) == str(k("enc_in_sha"))
    enc_d, enc_p = M.encode(g, msgs)
    _eq("enc_parity", enc_p, k("enc_parity"))
    _eq("enc_data", enc_d, k("enc_data") if (code["inner"] or code["outer"]) else msgs)
    assert not M.check(g, enc_d, enc_p).any()
    bits = np.random.default_rng([ord(name), 20]).integers(0, 8 * enc_p.shape[1] + 8 * enc_d.shape[1], rows)
    row = np.concatenate([enc_d, enc_p], axis=1)
    row[np.arange(rows), bits // 8] ^= (0x80 >> (bits % 8)).astype(np.uint8)
    _eq("chk_dirty", M.check(g, row[:, :enc_d.shape[1]], row[:, enc_d.shape[1]:]), k("chk_dirty"))
    # hard path
    if name == "M":
        src, din, pin, nf = R.flip_rows(enc_d, enc_p, flips=(0, 4, 40, 400), per=2)
    else:
        src, din, pin, nf = R.flip_rows(enc_d, enc_p)
    assert R.sha(np.concatenate([din, pin], axis=1)) == str(k("hard_in_sha"))
    clean = R.deinterleave(np.concatenate([enc_d, enc_p], axis=1), g["inner_forward"], g["num_bits"])
    ok, it, dout, hard = M.decode(g, din, pin, max_iterations=R.MAX_ITER)
    _eq("hard_ok", ok, k("hard_ok"))
    _eq("hard_iter", it, k("hard_iter"))
    _eq("hard_cor", _cor(ok, it), k("hard_cor"))
    _eq("hard_data_x", dout ^ msgs[src], k("hard_data_x"))
    _eq("hard_hard_x", hard ^ clean[src], k("hard_hard_x"))
    if name == "A":
        sel = nf >= 8
        for limit in (0, 1):
            assert R.sha(np.concatenate([din[sel], pin[sel]], axis=1)) == str(gold[f"A_it{limit}_in_sha"])
            ok, it, dout, hard = M.decode(g, din[sel], pin[sel], max_iterations=limit)
            _eq(f"it{limit}_ok", ok, gold[f"A_it{limit}_ok"])
            _eq(f"it{limit}_iter", it, gold[f"A_it{limit}_iter"])
            _eq(f"it{limit}_cor", _cor(ok, it), gold[f"A_it{limit}_cor"])
            _eq(f"it{limit}_data_x", dout ^ msgs[src[sel]], gold[f"A_it{limit}_data_x"])
            _eq(f"it{limit}_hard_x", hard ^ clean[src[sel]], gold[f"A_it{limit}_hard_x"])
    if name in R.SOFT:
        llr, jd, jp = R.soft_rows(name, enc_d, enc_p, g["num_bits"])
        assert R.sha(llr) + R.sha(jd) + R.sha(jp) == str(k("soft_in_sha"))
        ok, it, dout, hard = M.decode(g, jd, jp, llr=llr, max_iterations=R.MAX_ITER)
        _eq("soft_ok", ok, k("soft_ok"))
        _eq("soft_iter", it, k("soft_iter"))
        _eq("soft_cor", _cor(ok, it), k("soft_cor"))
        _eq("soft_data", dout, k("soft_data"))
        _eq("soft_hard", hard, k("soft_hard"))


def test_every_recorded_array_is_compared(gold):
    """The list above against the file: a new array in the fixture needs a comparison here."""
    seen = {"getters"}
    for name in R.SMALL + "M":
        seen |= {f"{name}_{s}" for s in ("dims", "row_ptr", "col_idx", "inner_forward", "outer_forward", "enc_in_sha",
                                        "enc_parity", "enc_data", "chk_dirty", "hard_in_sha", "hard_ok", "hard_cor",
                                        "hard_iter", "hard_data_x", "hard_hard_x")}
    for name in R.SOFT:
        seen |= {f"{name}_soft_{s}" for s in ("in_sha", "ok", "cor", "iter", "data", "hard")}
    for limit in (0, 1):
        seen |= {f"A_it{limit}_{s}" for s in ("in_sha", "ok", "cor", "iter", "data_x", "hard_x")}
    assert {f for f in gold.files if not f.startswith("G_")} <= seen


# ---- the sweep codes ----------------------------------------------------------------------

def make(code, **kw):
    return P.Ldpc(code["block"], code["rate"], code["matrix"], code["weight"], False, code["outer"], code["inner"],
                  code["depth"], code["lifting"], R.MAX_ITER, None, 0, code["seed"], **kw)


def graph_sha(g):
    return [R.sha(g[k].astype(np.uint32)) if g[k] is not None else ""
            for k in ("row_ptr", "col_idx", "inner_forward", "outer_forward")]


def model_graph(h):
    g = h.graph()
    return M.graph(g["row_ptr"], g["col_idx"], 8 * h.info_bytes, g["inner_forward"], g["outer_forward"])


def single_edge_rows(h):
    """LLRs, junk data and junk parity of ldpc_ref.sweep_single_edge_rows for a handle."""
    el = R.sweep_single_edge_rows(h.graph())
    return el, np.full((len(el), h.info_bytes), 0x5A, np.uint8), np.full((len(el), h.parity_bytes), 0xC3, np.uint8)


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_sweep_graph_equals_recorded(sweep, name):
    """Explicit depth, explicit lifting and a seed above 2^32 among them."""
    code = R.SWEEP[name]
    h = make(code)
    assert h.supported
    g = h.graph()
    assert [h.parity_size, h.info_size, g["num_checks"], g["num_bits"], g["num_edges"]] == sweep[name + "_dims"].tolist()
    assert graph_sha(g) == sweep[name + "_graph_sha"].tolist()
    assert (g["inner_forward"] is not None) == code["inner"] and (g["outer_forward"] is not None) == code["outer"]
    if code["inner"]:
        assert g["num_bits"] % code["depth"] == 0 and np.unique(g["inner_forward"]).size == g["num_bits"]
    if name == "S1":
        assert code["seed"] >= 1 << 32 and g["num_bits"] % 8 and g["num_checks"] % 8
    if name == "S6":  # the QC builder dropped edges
        assert g["num_edges"] < 3 * 320 + 2 * 80 - 1
    if code["matrix"] == R.RANDOM:
        assert g["num_edges"] == code["weight"] * 8 * code["block"] + 2 * g["num_checks"] - 1
    if name == "W848":
        assert (np.diff(g["row_ptr"].astype(np.int64)) == 1).any(), "a check row with a single edge"
    if R.reference_available():
        ref = R.RefLdpc(code)
        assert graph_sha(ref.graph()) == graph_sha(g)
        ref.close()


def test_sweep_refused_variant(sweep):
    """W340 with the automatic inner depth: no permutation, not served."""
    h = make(R.SWEEP_REFUSED)
    g = h.graph()
    assert not h.supported
    assert [h.parity_size, h.info_size, g["num_checks"], g["num_bits"], g["num_edges"]] == sweep["refused_dims"].tolist()
    assert graph_sha(g) == sweep["refused_graph_sha"].tolist()
    assert np.unique(g["inner_forward"]).size < g["num_bits"]
    d, p = np.zeros(h.info_size, np.uint8), np.zeros(h.parity_size, np.uint8)
    assert not h.lib.poporon_encode(h.h, d.ctypes.data, d.size, p.ctypes.data)
    assert "permutation" in P.last_error()


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_model_equals_sweep_fixture(sweep, name):
    h = make(R.SWEEP[name])
    assert graph_sha(h.graph()) == sweep[name + "_graph_sha"].tolist()
    g = model_graph(h)
    k = lambda s: sweep[f"{name}_{s}"]  # noqa: E731
    in_sha = k("in_sha").tolist()
    msgs = R.sweep_enc_inputs(name)
    enc_d, enc_p = M.encode(g, msgs)
    assert R.sha(msgs) == in_sha[0] and [R.sha(enc_d), R.sha(enc_p)] == k("enc_sha").tolist()
    fd, fp = R.sweep_flip_one(name, enc_d, enc_p, g["num_bits"])
    assert R.sha(np.concatenate([fd, fp], axis=1)) == in_sha[1]
    assert not M.check(g, enc_d, enc_p).any()
    _eq("chk_dirty", M.check(g, fd, fp), k("chk_dirty"))
    src, din, pin, nf = R.sweep_hard_rows(name, enc_d, enc_p)
    assert R.sha(np.concatenate([din, pin], axis=1)) == in_sha[2]
    ok, it, dout, hard = M.decode(g, din, pin, max_iterations=R.MAX_ITER)
    _eq("hard_ok", ok, k("hard_ok"))
    _eq("hard_iter", it, k("hard_iter"))
    _eq("hard_cor", _cor(ok, it), k("hard_cor"))
    assert [R.sha(dout), R.sha(hard)] == k("hard_sha").tolist()
    llr, jd, jp = R.sweep_soft_rows(name, enc_d, enc_p, g["num_bits"])
    assert [R.sha(llr), R.sha(jd), R.sha(jp)] == in_sha[3:]
    assert (np.abs(llr[:4].astype(np.int64)) * 256 > M.LLR_SAT).all(), "rows in the saturated regime"
    ok, it, dout, hard = M.decode(g, jd, jp, llr=llr, max_iterations=R.MAX_ITER)
    _eq("soft_ok", ok, k("soft_ok"))
    _eq("soft_iter", it, k("soft_iter"))
    _eq("soft_cor", _cor(ok, it), k("soft_cor"))
    assert [R.sha(dout), R.sha(hard)] == k("soft_sha").tolist()
    assert (ok[:16] == 1).any(), "a row in the saturated regime decodes"
    if name + "_edge_ok" in sweep.files:
        el, ed, ep = single_edge_rows(h)
        ok, it, dout, hard = M.decode(g, ed, ep, llr=el, max_iterations=R.MAX_ITER)
        _eq("edge_ok", ok, k("edge_ok"))
        _eq("edge_iter", it, k("edge_iter"))
        _eq("edge_cor", _cor(ok, it), k("edge_cor"))
        assert [R.sha(el), R.sha(dout), R.sha(hard)] == k("edge_sha").tolist()
    else:
        assert (np.diff(g["row_ptr"]) > 1).all()


@pytest.mark.parametrize("name", list(R.SWEEP))
def test_model_equals_live_reference(name):
    """Further rows of every sweep code (nothing to compare with where the reference was not built)."""
    if not R.reference_available():
        return
    code = R.SWEEP[name]
    ref = R.RefLdpc(code)
    rg = ref.graph()
    g = M.graph(rg["row_ptr"], rg["col_idx"], 8 * ref.info_bytes, rg["inner_forward"], rg["outer_forward"])
    msgs = np.random.default_rng([R.SWEEP_SEED, len(name), 77]).integers(0, 256, (6, code["block"]), dtype=np.uint8)
    enc_d, enc_p = M.encode(g, msgs)
    for i in range(len(msgs)):
        wd, wp = ref.encode(msgs[i])
        assert (enc_d[i] == wd).all() and (enc_p[i] == wp).all(), f"encode, row {i}"
    src, din, pin, nf = R.sweep_hard_rows(name, enc_d, enc_p, seed=78)
    din, pin = din[::2], pin[::2]
    want = [ref.decode(din[i], pin[i]) for i in range(len(din))]
    ok, it, dout, hard = M.decode(g, din, pin, max_iterations=R.MAX_ITER)
    _eq("live hard ok", ok, np.array([w[0] for w in want], np.uint8))
    _eq("live hard cor", _cor(ok, it), np.array([w[1] for w in want]))
    _eq("live hard iter", it, np.array([w[2] for w in want], np.uint32))
    _eq("live hard data", dout, np.stack([w[3] for w in want]))
    _eq("live hard hard", hard, np.stack([w[4] for w in want]))
    _eq("live check", M.check(g, din, pin), np.array([ref.dirty(din[i], pin[i]) for i in range(len(din))], np.uint8))
    ref.close()
    rs = R.RefLdpc(code, soft=True)
    llr, jd, jp = R.sweep_soft_rows(name, enc_d, enc_p, rs.codeword_bits, seed=79)
    want = []
    for i in range(len(llr)):
        rs.set_llr(llr[i])
        want.append(rs.decode(jd[i], jp[i]))
    ok, it, dout, hard = M.decode(g, jd, jp, llr=llr, max_iterations=R.MAX_ITER)
    _eq("live soft ok", ok, np.array([w[0] for w in want], np.uint8))
    _eq("live soft iter", it, np.array([w[2] for w in want], np.uint32))
    _eq("live soft data", dout, np.stack([w[3] for w in want]))
    _eq("live soft hard", hard, np.stack([w[4] for w in want]))
    rs.close()
