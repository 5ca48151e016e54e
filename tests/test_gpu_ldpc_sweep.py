"""The LDPC kernels (ldpc.hip) against the numpy model (tests/ldpc_model.py) on codes
shaped for the kernels' own code paths: inner interleaver with spare bits, explicit
depth and lifting, fewer than 64 check rows, a partial run in encode's prefix pass, a
check row with a single edge, decode LDS sizes on both sides of 64 KiB and of
LDPC_LDS_MAX, and soft rows in the saturated regime (tests/ldpc_ref.py: SWEEP).

The chain is reference -> recorded fixture -> model -> kernels: the model equals the
reference on every row used here (tests/test_ldpc_model_cpu.py, no device), the handle's
graph is compared with the fixture's SHA-256s before any launch, and after every
comparison with the model, ok and iterations are compared with the arrays recorded
from the reference as well.  Every call runs on canary-filled buffers at odd offsets
and padded strides (tests/ldpc_dev.py).
"""
import re

import numpy as np
import pytest

import ldpc_model as M
import ldpc_ref as R
import libpoporon_amd as P
from ldpc_dev import Rows, _dev_check, _dev_decode, _dev_encode, _env, _same, _stream

pytestmark = pytest.mark.gpu

LDS_MAX = 160 * 1024  # LDPC_LDS_MAX
LDS_PLAIN = 64 * 1024  # more dynamic LDS than this is asked for with hipFuncSetAttribute
# dynamic LDS of ldpc_decode_k<true>, from the graph
LDS_BYTES = {"W336": 65184, "W340": 65968, "W840": 162960, "W844": 163744, "W848": 164512}
# W844 is under LDPC_LDS_MAX but past what the kernel's static LDS leaves of it, W848 is past both:
# forced into the LDS they are refused, and they also run the automatic choice (the workspace)
NO_LDS = ("W844", "W848")
PLACEMENTS = [(n, p) for n in R.SWEEP for p in (("global", None) if n in NO_LDS else ("lds", "global"))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def sweep():
    return np.load(R.SWEEP_GOLDEN)


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


def _make(code, path, max_iterations=R.MAX_ITER):
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    with _env(POPORON_AMD_LDPC_PATH=path):  # read at poporon_create
        return P.Ldpc(code["block"], code["rate"], code["matrix"], code["weight"], False, code["outer"], code["inner"],
                      code.get("depth", 0), code["lifting"], max_iterations, None, 0, code["seed"])


def _graph_sha(g):
    return [R.sha(g[k].astype(np.uint32)) if g[k] is not None else ""
            for k in ("row_ptr", "col_idx", "inner_forward", "outer_forward")]


def _handle(sweep, name, path):
    """A handle whose graph is known to be the reference's, before any launch."""
    h = _make(R.SWEEP[name], path)
    g = h.graph()
    assert h.supported and _graph_sha(g) == sweep[name + "_graph_sha"].tolist()
    lds = R.decode_lds_bytes(g["num_edges"], g["num_bits"])
    if name in LDS_BYTES:
        assert lds == LDS_BYTES[name]
    else:
        assert lds < LDS_PLAIN
    return h


_CASES = {}


def _case(sweep, name):
    """The rows of one sweep code and the model's results, computed once for every placement."""
    if name in _CASES:
        return _CASES[name]
    h = _make(R.SWEEP[name], None)
    hg = h.graph()
    assert _graph_sha(hg) == sweep[name + "_graph_sha"].tolist()
    g = M.graph(hg["row_ptr"], hg["col_idx"], 8 * h.info_bytes, hg["inner_forward"], hg["outer_forward"])
    sha = sweep[name + "_in_sha"].tolist()
    c = dict(g=g, msgs=R.sweep_enc_inputs(name))
    c["enc_d"], c["enc_p"] = M.encode(g, c["msgs"])
    c["fd"], c["fp"] = R.sweep_flip_one(name, c["enc_d"], c["enc_p"], g["num_bits"])
    c["dirty"] = M.check(g, c["fd"], c["fp"])
    _, c["din"], c["pin"], c["nflip"] = R.sweep_hard_rows(name, c["enc_d"], c["enc_p"])
    c["hard"] = M.decode(g, c["din"], c["pin"], max_iterations=R.MAX_ITER)
    c["llr"], c["jd"], c["jp"] = R.sweep_soft_rows(name, c["enc_d"], c["enc_p"], g["num_bits"])
    c["soft"] = M.decode(g, c["jd"], c["jp"], llr=c["llr"], max_iterations=R.MAX_ITER)
    assert [R.sha(c["msgs"]), R.sha(np.concatenate([c["fd"], c["fp"]], axis=1)),
            R.sha(np.concatenate([c["din"], c["pin"]], axis=1)), R.sha(c["llr"]), R.sha(c["jd"]), R.sha(c["jp"])] == sha, \
        "numpy's Generator stream differs from the recorded inputs"
    _CASES[name] = c
    return c


def _recorded(sweep, what, name, got):
    """ok and iterations against the arrays recorded from the reference, independent of the model."""
    assert (got[0] == sweep[f"{name}_{what}_ok"]).all(), f"{what} ok differs from the recorded reference on {name}"
    assert (got[1] == sweep[f"{name}_{what}_iter"]).all(), f"{what} iterations differ from the recorded reference on {name}"


# ---- per code and placement ----------------------------------------------------------------

@pytest.mark.parametrize("name,path", PLACEMENTS)
def test_encode_and_check(torch_cuda, sweep, name, path):
    c = _case(sweep, name)
    h = _handle(sweep, name, path)
    dd, pp = _dev_encode(torch_cuda, h, c["msgs"])
    _same("encode", name, (None, None, dd, None), (None, None, c["enc_d"], None))
    assert (pp == c["enc_p"]).all(), f"parity differs on rows {np.nonzero((pp != c['enc_p']).any(1))[0][:8]}"
    assert [R.sha(dd), R.sha(pp)] == sweep[name + "_enc_sha"].tolist()
    if h.codeword_bits % 8:  # spare bits of the last parity byte are 0
        assert not (pp[:, -1] & (0xFF >> (h.codeword_bits % 8))).any()
    assert not _dev_check(torch_cuda, h, dd, pp).any(), "freshly encoded rows are clean"
    dirty = _dev_check(torch_cuda, h, c["fd"], c["fp"])
    assert (dirty == c["dirty"]).all() and (dirty == sweep[name + "_chk_dirty"]).all()
    assert dirty.any()


@pytest.mark.parametrize("name,path", PLACEMENTS)
def test_hard_decode(torch_cuda, sweep, name, path):
    c = _case(sweep, name)
    h = _handle(sweep, name, path)
    got = _dev_decode(torch_cuda, h, c["din"], c["pin"])
    _same("hard decode", name, got, c["hard"])
    _recorded(sweep, "hard", name, got)
    assert [R.sha(got[2]), R.sha(got[3])] == sweep[name + "_hard_sha"].tolist()
    bad, it = got[0] == 0, got[1][got[0] == 1]
    assert (got[2][bad] == c["din"][bad]).all(), "a failed row's data is untouched"
    assert bad.any() and (it == 0).any() and (it == 1).any() and (it >= 3).any(), "every exit of the kernel"


@pytest.mark.parametrize("name,path", PLACEMENTS)
def test_soft_decode(torch_cuda, sweep, name, path):
    c = _case(sweep, name)
    h = _handle(sweep, name, path)
    assert (np.abs(c["llr"][:4].astype(np.int64)) * 256 > M.LLR_SAT).all(), "rows in the saturated regime"
    # junk in the row's data and parity: the soft path reads the llr alone
    got = _dev_decode(torch_cuda, h, c["jd"], c["jp"], llr=c["llr"])
    _same("soft decode", name, got, c["soft"])
    _recorded(sweep, "soft", name, got)
    assert [R.sha(got[2]), R.sha(got[3])] == sweep[name + "_soft_sha"].tolist()
    ok, it = got[0], got[1]
    assert (ok == 0).any() and (ok[:16] == 1).any()
    # all 0 and all 127 are the zero codeword after one iteration; all -128 never settles
    assert (ok[16], it[16], ok[17], it[17], ok[18], it[18]) == (1, 1, 0, R.MAX_ITER, 1, 1)
    assert (got[2][ok == 0] == c["jd"][ok == 0]).all()


@pytest.mark.parametrize("path", ("global", None))
def test_single_edge_check_row(torch_cuda, sweep, path):
    """W848 has a check row with one edge: no second minimum, so the edge gets the start value of
    the minima (32000 * 15 / 16 = 30000).  LLR rows that balance the edge's bit against that message."""
    name = "W848"
    c = _case(sweep, name)
    h = _handle(sweep, name, path)
    assert (np.diff(c["g"]["row_ptr"]) == 1).any()
    llr = R.sweep_single_edge_rows(h.graph())
    jd, jp = np.full((len(llr), h.info_bytes), 0x5A, np.uint8), np.full((len(llr), h.parity_bytes), 0xC3, np.uint8)
    want = M.decode(c["g"], jd, jp, llr=llr, max_iterations=R.MAX_ITER)
    got = _dev_decode(torch_cuda, h, jd, jp, llr=llr)
    _same("single-edge check row", name, got, want)
    _recorded(sweep, "edge", name, got)
    assert [R.sha(llr), R.sha(got[2]), R.sha(got[3])] == sweep[name + "_edge_sha"].tolist()
    assert (got[0] == 0).any() and (got[1][got[0] == 1] == 1).any() and (got[1][got[0] == 1] > 1).any()


@pytest.mark.parametrize("name", NO_LDS)
def test_lds_boundaries(torch_cuda, sweep, name):
    """The forced LDS placement refuses what does not fit, naming the kernel's own figures: the
    code's bytes (the ones this file computes from the graph), the room the kernel's static LDS
    leaves, and LDPC_LDS_MAX.  W844 is 96 B under LDPC_LDS_MAX and still does not fit; W840 does."""
    c = _case(sweep, name)
    assert LDS_BYTES["W336"] <= LDS_PLAIN < LDS_BYTES["W340"]
    assert LDS_BYTES["W840"] < LDS_BYTES["W844"] == LDS_MAX - 96 and LDS_MAX < LDS_BYTES["W848"]
    forced = _handle(sweep, name, "lds")
    ok = torch_cuda.zeros(len(c["din"]), dtype=torch_cuda.uint8, device="cuda")
    d, p = Rows(torch_cuda, c["din"]), Rows(torch_cuda, c["pin"])
    with pytest.raises(P.PoporonError, match="do not fit") as e:
        forced.decode_batch_device(d.ptr, d.stride, p.ptr, p.stride, d.n, ok.data_ptr(), stream=_stream(torch_cuda))
    need, room, whole = [int(v) for v in re.findall(r"(\d+) bytes", str(e.value))]
    assert (need, whole) == (LDS_BYTES[name], LDS_MAX) and LDS_BYTES["W840"] <= room < need
    torch_cuda.cuda.synchronize()
    assert (d.rows() == c["din"]).all() and d.canaries() and not ok.cpu().numpy().any()


# ---- the recorded codes: workspace growth, fresh rows --------------------------------------------

def _old_graph(gold, name, h):
    g = h.graph()
    for k in ("row_ptr", "col_idx", "inner_forward", "outer_forward"):
        want = gold[f"{name}_{k}"] if f"{name}_{k}" in gold.files else None
        assert (g[k] is None) == (want is None) and (want is None or (g[k] == want).all()), k
    return M.graph(g["row_ptr"], g["col_idx"], 8 * h.info_bytes, g["inner_forward"], g["outer_forward"])


def test_workspace_growth(torch_cuda, gold):
    """2 rows, then 600, then 2 on one global-path handle without reserve: the second call frees
    and reallocates the workspace while the first may still run (no synchronise between them)."""
    h = _make(R.CODES["A"], "global")
    g = _old_graph(gold, "A", h)
    enc_d, enc_p = M.encode(g, R.enc_inputs("A", 64))
    _, din, pin, _ = R.flip_rows(enc_d, enc_p, flips=(0, 2, 5, 9, 14), per=24, seed=41)
    want = M.decode(g, din, pin, max_iterations=R.MAX_ITER)
    assert (want[0] == 0).any() and (want[1][want[0] == 1] >= 3).any()
    slow = np.argsort(-want[1].astype(np.int64), kind="stable")[:2]  # the first call's rows take the longest
    picks = [slow, np.arange(600) % len(din), np.arange(2) + 50]
    bufs = []
    for k, idx in enumerate(picks):
        n = len(idx)
        bufs.append((Rows(torch_cuda, din[idx], 3 + k, 5), Rows(torch_cuda, pin[idx], 2 + k, 7),
                     Rows(torch_cuda, np.full((n, h.codeword_bytes), 0xA5, np.uint8), 1 + k, 4),
                     torch_cuda.full((n + 1,), 0xEE, dtype=torch_cuda.uint8, device="cuda"),
                     torch_cuda.full((n + 1,), -1, dtype=torch_cuda.int32, device="cuda")))
    s = _stream(torch_cuda)
    for k, (d, p, hd, ok, it) in enumerate(bufs):
        h.decode_batch_device(d.ptr, d.stride, p.ptr, p.stride, d.n, ok.data_ptr(), it.data_ptr(), hd.ptr, hd.stride,
                              stream=s)
        if k == 1:
            torch_cuda.cuda.synchronize()
    torch_cuda.cuda.synchronize()
    for k, (idx, (d, p, hd, ok, it)) in enumerate(zip(picks, bufs)):
        assert d.canaries() and p.canaries() and hd.canaries() and (p.rows() == pin[idx]).all()
        okh, ith = ok.cpu().numpy(), it.cpu().numpy().view(np.uint32)
        assert okh[-1] == 0xEE and ith[-1] == 0xFFFFFFFF
        _same(f"workspace growth, call {k}", "A", (okh[:-1], ith[:-1], d.rows(), hd.rows()), [w[idx] for w in want])


def _fresh_rows(name, g):
    """64 hard and 64 soft rows of a recorded code from seeds the fixtures do not use."""
    rng = np.random.default_rng([ord(name), 0x5EED])
    ib, n = g["info_bits"] // 8, g["num_bits"]
    enc_d, enc_p = M.encode(g, rng.integers(0, 256, (32, ib), dtype=np.uint8))
    _, din, pin, _ = R.flip_rows(enc_d, enc_p, flips=(0, 1, 3, 5, 7, 10, 13, 24), per=8, seed=int(rng.integers(1 << 40)))
    sign = 1.0 - 2.0 * np.unpackbits(np.concatenate([enc_d, enc_p], axis=1), axis=1)[:, :n]
    noisy = [np.clip(np.rint((sign[rng.integers(0, 32, 16)] + rng.normal(0.0, sg, (16, n))) * 16.0), -127, 127)
             for sg in (0.5, 0.8, 1.0)]
    strong = sign[rng.integers(0, 32, 16)] * np.repeat([127, 126, 125, 1], 4)[:, None]  # around llr * 256 = 32000
    noisy.append(np.where(rng.random(strong.shape) < 0.04, -strong, strong))
    llr = np.ascontiguousarray(np.concatenate(noisy).astype(np.int8))
    return din, pin, llr, rng.integers(0, 256, (64, ib), dtype=np.uint8), \
        rng.integers(0, 256, (64, enc_p.shape[1]), dtype=np.uint8)


@pytest.mark.parametrize("name", list(R.SMALL))
def test_fresh_rows_of_recorded_codes(torch_cuda, gold, name):
    """Rows the recorded file does not hold, on both placements."""
    g = None
    for path in ("lds", "global"):
        h = _make(R.CODES[name], path)
        if g is None:
            g = _old_graph(gold, name, h)
            din, pin, llr, jd, jp = _fresh_rows(name, g)
            assert din.shape[0] == 64 and llr.shape == (64, g["num_bits"])
            hard = M.decode(g, din, pin, max_iterations=R.MAX_ITER)
            soft = M.decode(g, jd, jp, llr=llr, max_iterations=R.MAX_ITER)
            assert (hard[0] == 0).any() and (hard[0] == 1).any() and (soft[0] == 1).any()
        _same(f"fresh hard rows ({path})", name, _dev_decode(torch_cuda, h, din, pin), hard)
        _same(f"fresh soft rows ({path})", name, _dev_decode(torch_cuda, h, jd, jp, llr=llr), soft)
        assert (_dev_check(torch_cuda, h, din, pin) == M.check(g, din, pin)).all()
