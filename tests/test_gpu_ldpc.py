"""LDPC batch encode, check and min-sum decode (ldpc.hip) against the reference,
bit for bit: parity bytes, rewritten data bytes, ok flag, iteration count and
hard decisions.

The checker is the reference itself: its outputs recorded in
tests/golden/ldpc_golden.npz (tools/gen_golden_ldpc.py) for seeded inputs that
tests/ldpc_ref.py rebuilds (their SHA-256 is recorded too), and, where
oracle/_ref was built, the live library on further rows.  Codes A-F and M run
with the decoder's messages in LDS and in the global workspace
(POPORON_AMD_LDPC_PATH); G, the largest code, takes the automatic choice.
"""
import ctypes as C

import numpy as np
import pytest

import ldpc_ref as R
import libpoporon_amd as P
from ldpc_dev import Rows, _dev_check, _dev_decode, _dev_encode, _env, _same, _stream

pytestmark = pytest.mark.gpu

PATHS = ("lds", "global")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


def _handle(name, path, max_iterations=R.MAX_ITER, soft=False, llr=None):
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    c = R.CODES[name]
    with _env(POPORON_AMD_LDPC_PATH=path):  # read at poporon_create
        return P.Ldpc(c["block"], c["rate"], c["matrix"], c["weight"], soft, c["outer"], c["inner"], 0, c["lifting"],
                      max_iterations, llr, 0, c["seed"])


_CASES = {}


def _case(gold, name):
    """The rows of one code: seeded inputs (hash-checked) and the reference's recorded outputs."""
    if name in _CASES:
        return _CASES[name]
    code = R.CODES[name]
    k = lambda s: gold[f"{name}_{s}"]  # noqa: E731
    c = dict(code=code)
    c["msgs"] = R.enc_inputs(name, R.ENC_ROWS if name != "M" else 8)
    assert R.sha(c["msgs"]) == str(k("enc_in_sha")), "numpy's Generator stream differs from the recorded inputs"
    c["enc_p"] = k("enc_parity")
    c["enc_d"] = k("enc_data") if (code["inner"] or code["outer"]) else c["msgs"]
    c["fwd"] = k("inner_forward") if code["inner"] else None
    c["nbits"] = int(k("dims")[3])
    c["clean"] = R.deinterleave(np.concatenate([c["enc_d"], c["enc_p"]], axis=1), c["fwd"], c["nbits"])
    if name == "M":
        src, din, pin, nf = R.flip_rows(c["enc_d"], c["enc_p"], flips=(0, 4, 40, 400), per=2)
    else:
        src, din, pin, nf = R.flip_rows(c["enc_d"], c["enc_p"])
    assert R.sha(np.concatenate([din, pin], axis=1)) == str(k("hard_in_sha"))
    c.update(src=src, din=din, pin=pin, nflip=nf, ok=k("hard_ok"), cor=k("hard_cor"), iter=k("hard_iter"),
             dout=k("hard_data_x") ^ c["msgs"][src], hard=k("hard_hard_x") ^ c["clean"][src])
    # the yardstick itself: a failed row keeps its data, corrected_num keeps the sentinel
    bad = c["ok"] == 0
    assert (c["dout"][bad] == din[bad]).all() and (c["cor"][bad] == R.SENT).all()
    assert (c["cor"][~bad] == c["iter"][~bad]).all() and (c["iter"][bad] == R.MAX_ITER).all()
    # the hard path leaves at iteration 0 exactly when the row's syndrome is clean
    c["dirty"] = ~((c["ok"] == 1) & (c["iter"] == 0))
    _CASES[name] = c
    return c


# ---- encode and check ---------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(R.SMALL + "M"))
def test_encode_and_check(torch_cuda, gold, name, path):
    c = _case(gold, name)
    h = _handle(name, path)
    dd, pp = _dev_encode(torch_cuda, h, c["msgs"])
    _same("encode", name, (None, None, dd, None), (None, None, c["enc_d"], None))
    assert (pp == c["enc_p"]).all(), f"parity differs on rows {np.nonzero((pp != c['enc_p']).any(1))[0][:8]}"
    if c["code"]["inner"] or c["code"]["outer"]:
        assert (dd != c["msgs"]).any(), "an interleaver is on: encode rewrites the data"
    assert not _dev_check(torch_cuda, h, dd, pp).any(), "freshly encoded rows are clean"
    bits = np.random.default_rng([ord(name), 20]).integers(0, 8 * h.codeword_bytes, len(dd))
    row = np.concatenate([dd, pp], axis=1)
    row[np.arange(len(dd)), bits // 8] ^= (0x80 >> (bits % 8)).astype(np.uint8)
    fd, fp = np.ascontiguousarray(row[:, :h.info_bytes]), np.ascontiguousarray(row[:, h.info_bytes:])
    dirty = _dev_check(torch_cuda, h, fd, fp)
    assert (dirty == gold[name + "_chk_dirty"]).all()
    assert dirty.any()
    # the host forms
    hd, hp = h.encode_batch(c["msgs"])
    assert (hd == c["enc_d"]).all() and (hp == c["enc_p"]).all()
    assert (h.check_batch(fd, fp) == dirty).all()
    if R.reference_available():
        ref = R.RefLdpc(c["code"])
        more = np.random.default_rng([ord(name), 11]).integers(0, 256, (24, h.info_bytes), dtype=np.uint8)
        gd, gp = _dev_encode(torch_cuda, h, more, off=0, pad=0)
        for i in range(len(more)):
            wd, wp = ref.encode(more[i])
            assert (gd[i] == wd).all() and (gp[i] == wp).all(), f"live reference, row {i}"
        for i in range(min(len(more), len(dirty))):
            assert bool(dirty[i]) == ref.dirty(fd[i], fp[i])
        ref.close()


# ---- hard decode ----------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(R.SMALL + "M"))
def test_hard_decode(torch_cuda, gold, name, path):
    c = _case(gold, name)
    h = _handle(name, path)
    got = _dev_decode(torch_cuda, h, c["din"], c["pin"])
    _same("hard decode", name, got, (c["ok"], c["iter"], c["dout"], c["hard"]))
    bad = c["ok"] == 0
    assert (got[2][bad] == c["din"][bad]).all(), "a failed row's data is untouched"
    if name != "M":  # every exit of the kernel is in the row set
        it = c["iter"][~bad]
        assert bad.any() and (it == 0).any() and (it == 1).any() and (it >= 3).any()
    if R.reference_available():
        ref = R.RefLdpc(c["code"])
        _, din, pin, _ = R.flip_rows(c["enc_d"], c["enc_p"], flips=(3, 6, 12), per=12, seed=2)
        want = [ref.decode(din[i], pin[i]) for i in range(len(din))]
        g = _dev_decode(torch_cuda, h, din, pin, off=0, pad=0)
        _same("hard decode (live reference)", name, g,
              (np.array([w[0] for w in want], np.uint8), np.array([w[2] for w in want], np.uint32),
               np.stack([w[3] for w in want]), np.stack([w[4] for w in want])))
        ref.close()


# ---- soft decode ----------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(R.SOFT))
def test_soft_decode(torch_cuda, gold, name, path):
    c = _case(gold, name)
    llr, jd, jp = R.soft_rows(name, c["enc_d"], c["enc_p"], c["nbits"])
    assert R.sha(llr) + R.sha(jd) + R.sha(jp) == str(gold[name + "_soft_in_sha"])
    assert (llr[-R.SOFT_EXTRA:, :3] == (-128, 0, 127)).all()
    k = lambda s: gold[f"{name}_soft_{s}"]  # noqa: E731
    h = _handle(name, path)
    # junk in the row's data and parity: the soft path reads the llr alone
    got = _dev_decode(torch_cuda, h, jd, jp, llr=llr)
    _same("soft decode", name, got, (k("ok"), k("iter"), k("data"), k("hard")))
    bad = k("ok") == 0
    assert bad[-R.SOFT_EXTRA:].all() and (k("iter")[bad] == R.MAX_ITER).all()
    assert (got[2][bad] == jd[bad]).all()
    assert k("ok")[:R.ROWS_PER_FLIP].sum() > R.ROWS_PER_FLIP // 2, "sigma 0.5 mostly decodes"
    # other junk, same result
    again = _dev_decode(torch_cuda, h, jd ^ 0x5A, jp ^ 0xC3, llr=llr, off=0, pad=0)
    _same("soft decode, other junk", name, (again[0], again[1], None, again[3]), (k("ok"), k("iter"), None, k("hard")))
    ho = h.decode_batch(jd, jp, llr=llr)
    _same("soft decode, host batch", name, ho, (k("ok"), k("iter"), k("data"), k("hard")))


# ---- iteration limits ------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("limit", (0, 1))
def test_iteration_limits(torch_cuda, gold, limit, path):
    c = _case(gold, "A")
    sel = c["nflip"] >= 8
    k = lambda s: gold[f"A_it{limit}_{s}"]  # noqa: E731
    h = _handle("A", path, max_iterations=limit)
    got = _dev_decode(torch_cuda, h, c["din"][sel], c["pin"][sel])
    want_d, want_h = k("data_x") ^ c["msgs"][c["src"][sel]], k("hard_x") ^ c["clean"][c["src"][sel]]
    _same(f"max_iterations {limit}", "A", got, (k("ok"), k("iter"), want_d, want_h))
    bad = k("ok") == 0
    assert bad.any() and (k("iter")[bad] == (50 if limit == 0 else 1)).all()


# ---- layout -----------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("count", (1, 2, 255, 4099))
def test_layout(torch_cuda, gold, count, path):
    """Row counts around the block and past the launch's grid cap (8 and 4 workgroups per CU:
    at most 2048 and 1024 on 256 CUs), mostly clean rows; NULL d_iterations, NULL d_hard."""
    c = _case(gold, "A")
    clean, dirty = np.nonzero(c["nflip"] == 0)[0], np.nonzero(c["nflip"] >= 4)[0]
    idx = np.where(np.arange(count) % 16 == 7, dirty[np.arange(count) % len(dirty)], clean[np.arange(count) % len(clean)])
    if count <= 2:
        idx = dirty[-count:]
    din, pin = c["din"][idx], c["pin"][idx]
    want = (c["ok"][idx], c["iter"][idx], c["dout"][idx], c["hard"][idx])
    h = _handle("A", path)
    h.reserve(count)
    _same("layout", "A", _dev_decode(torch_cuda, h, din, pin, off=1, pad=7), want)
    _same("layout, NULL d_iterations", "A", _dev_decode(torch_cuda, h, din, pin, want_iter=False, off=2, pad=1), want)
    _same("layout, NULL d_hard", "A", _dev_decode(torch_cuda, h, din, pin, want_hard=False, off=7, pad=0), want)
    _same("layout, NULL both", "A", _dev_decode(torch_cuda, h, din, pin, want_iter=False, want_hard=False), want)
    e = np.arange(count) % R.ENC_ROWS
    dd, pp = _dev_encode(torch_cuda, h, c["msgs"][e], off=7, pad=9)
    assert (dd == c["enc_d"][e]).all() and (pp == c["enc_p"][e]).all()
    assert (_dev_check(torch_cuda, h, din, pin) == c["dirty"][idx]).all()


@pytest.mark.parametrize("path", PATHS)
def test_rows_in_one_buffer(torch_cuda, gold, path):
    """[data | parity] rows of one buffer (the wire layout), decoded in place."""
    c = _case(gold, "B")
    h = _handle("B", path)
    ib, w = h.info_bytes, h.codeword_bytes
    r = Rows(torch_cuda, np.concatenate([c["din"], c["pin"]], axis=1), off=1, pad=2)
    n = r.n
    ok = torch_cuda.zeros(n, dtype=torch_cuda.uint8, device="cuda")
    h.decode_batch_device(r.ptr, r.stride, r.ptr + ib, r.stride, n, ok.data_ptr(), stream=_stream(torch_cuda))
    torch_cuda.cuda.synchronize()
    out = r.rows()
    assert r.canaries() and (ok.cpu().numpy() == c["ok"]).all()
    assert (out[:, :ib] == c["dout"]).all() and (out[:, ib:w] == c["pin"]).all()


# ---- drop-in single calls ---------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ("A", "B"))
def test_drop_in_hard(gold, name, path):
    c = _case(gold, name)
    h = _handle(name, path)
    for i in (0, 1, 100, 256):
        d, p = h.encode(c["msgs"][i])
        assert (d == c["enc_d"][i]).all() and (p == c["enc_p"][i]).all()
    rows = np.concatenate([np.nonzero(c["ok"] == 0)[0][:3], np.nonzero(c["iter"] == 0)[0][:2],
                           np.nonzero((c["ok"] == 1) & (c["iter"] >= 2))[0][:3]])
    assert (c["ok"][rows] == 0).any()
    for i in rows:
        ok, cor, d = h.decode(c["din"][i], c["pin"][i], R.SENT)
        assert (ok, cor) == (bool(c["ok"][i]), int(c["cor"][i])), f"row {i}"
        assert cor == (R.SENT if not ok else c["iter"][i])
        assert (d == c["dout"][i]).all()
        assert h.iterations_used == c["iter"][i]
    d, p = np.zeros(64, np.uint8), np.zeros(h.parity_bytes, np.uint8)
    n = C.c_size_t(R.SENT)
    assert not h.lib.poporon_encode(h.h, d.ctypes.data, h.info_bytes + 1, p.ctypes.data)
    assert not h.lib.poporon_decode(h.h, d.ctypes.data, h.info_bytes - 1, p.ctypes.data, C.byref(n))
    assert n.value == R.SENT


@pytest.mark.parametrize("path", PATHS)
def test_drop_in_soft(gold, path):
    c = _case(gold, "A")
    llr, jd, jp = R.soft_rows("A", c["enc_d"], c["enc_p"], c["nbits"])
    k = lambda s: gold[f"A_soft_{s}"]  # noqa: E731
    h = _handle("A", path, soft=True, llr=llr[0])
    rows = [0, 1, 70, 80, 130, 200]
    assert (k("ok")[rows] == 0).any() and (k("ok")[rows] == 1).any()
    for i in rows:
        h.set_llr(llr[i])
        ok, cor, d = h.decode(jd[i], jp[i], R.SENT)
        assert (ok, cor) == (bool(k("ok")[i]), int(k("cor")[i])), f"row {i}"
        assert (d == k("data")[i]).all() and h.iterations_used == k("iter")[i]
    # use_soft_decode without LLRs is the hard path (src/decode.c:509)
    hh = _handle("A", path, soft=True)
    i = int(np.nonzero(c["iter"] >= 2)[0][0])
    assert hh.decode(c["din"][i], c["pin"][i], R.SENT)[:2] == (bool(c["ok"][i]), int(c["cor"][i]))


# ---- host batch -----------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
def test_host_batch(gold, path):
    c = _case(gold, "D")
    h = _handle("D", path)
    idx = np.arange(300) % len(c["din"])
    idx[:84] = np.arange(300, 384)  # the 16-flip rows too
    got = h.decode_batch(c["din"][idx], c["pin"][idx])
    _same("host batch", "D", got, (c["ok"][idx], c["iter"][idx], c["dout"][idx], c["hard"][idx]))
    got = h.decode_batch(c["din"][idx], c["pin"][idx], want_hard=False)
    _same("host batch, NULL hard", "D", got, (c["ok"][idx], c["iter"][idx], c["dout"][idx], None))
    e = np.arange(300) % R.ENC_ROWS
    dd, pp = h.encode_batch(c["msgs"][e])
    assert (dd == c["enc_d"][e]).all() and (pp == c["enc_p"][e]).all()
    assert (h.check_batch(c["din"][idx], c["pin"][idx]) == c["dirty"][idx]).all()


def test_host_batch_past_one_chunk(gold):
    """The host forms move 8 MiB chunks: 45,000 rows of D with their hard decisions are two."""
    c = _case(gold, "D")
    h = _handle("D", None)
    n = 45000
    assert n * (2 * h.codeword_bytes + 9) > (8 << 20) > (n // 2) * (2 * h.codeword_bytes + 9)
    clean, rest = np.nonzero(c["nflip"] == 0)[0], np.nonzero(c["nflip"] > 0)[0]
    idx = np.where(np.arange(n) % 16 == 5, rest[np.arange(n) % len(rest)], clean[np.arange(n) % len(clean)])
    got = h.decode_batch(c["din"][idx], c["pin"][idx])
    _same("host batch, two chunks", "D", got, (c["ok"][idx], c["iter"][idx], c["dout"][idx], c["hard"][idx]))
    e = np.arange(n) % R.ENC_ROWS
    dd, pp = h.encode_batch(c["msgs"][e])
    assert (dd == c["enc_d"][e]).all() and (pp == c["enc_p"][e]).all()
    assert (h.check_batch(c["din"][idx], c["pin"][idx]) == c["dirty"][idx]).all()


# ---- timing ids -------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
def test_timing_ids(torch_cuda, gold, path):
    c = _case(gold, "A")
    h = _handle("A", path)
    h.timing(True)
    dd, pp = _dev_encode(torch_cuda, h, c["msgs"])
    _dev_check(torch_cuda, h, dd, pp)
    _dev_decode(torch_cuda, h, c["din"], c["pin"])
    t = {k: h.timing_read(k) for k in range(15)}
    h.timing(False)
    for k in (P.KERNEL_LDPC_ENCODE, P.KERNEL_LDPC_DECODE, P.KERNEL_LDPC_CHECK):
        assert t[k][1] == 1 and t[k][0] > 0, f"kernel id {k} ({P.LDPC_KERNEL_NAMES[k]}): {t[k]}"
    assert all(t[k][1] == 0 for k in range(12)), "an RS / BCH kernel id was charged"


# ---- the largest code ---------------------------------------------------------------------------------

def test_largest_code(torch_cuda, gold):
    """G: 786431 edges, 3.5 MB of messages per codeword: the workspace path by the
    automatic choice (the LDS placement refuses it), slices at multi-megabyte offsets."""
    msgs, flips = R.g_inputs()
    assert R.sha(msgs) == str(gold["G_enc_in_sha"])
    h = _handle("G", None, max_iterations=3)
    dd, pp = _dev_encode(torch_cuda, h, msgs)
    assert (dd == msgs).all() and R.sha(pp) == str(gold["G_enc_parity_sha"])
    rx = [R.apply_flips(dd[i], pp[i], flips[i]) for i in range(2)]
    din, pin = np.stack([r[0] for r in rx]), np.stack([r[1] for r in rx])
    assert (_dev_check(torch_cuda, h, din, pin) == gold["G_chk_dirty"]).all()
    ok, it, dout, hard = _dev_decode(torch_cuda, h, din, pin)
    assert ok.tolist() == gold["G_hard_ok"].tolist() and it.tolist() == gold["G_hard_iter"].tolist()
    for i in range(2):
        assert R.sha(dout[i]) == str(gold["G_hard_data_sha"][i]), f"data of row {i}"
        assert R.sha(hard[i]) == str(gold["G_hard_hard_sha"][i]), f"hard decisions of row {i}"
    assert (dout[1] == din[1]).all() and (dout[0] == msgs[0]).all()
    forced = _handle("G", "lds", max_iterations=3)
    okb = torch_cuda.zeros(2, dtype=torch_cuda.uint8, device="cuda")
    d, p = Rows(torch_cuda, din), Rows(torch_cuda, pin)
    with pytest.raises(P.PoporonError, match="do not fit"):
        forced.decode_batch_device(d.ptr, d.stride, p.ptr, p.stride, 2, okb.data_ptr())
    assert (d.rows() == din).all()
