"""The soft-decision RS decode on the GPU (poporon_decode_soft_batch_device, rs_soft.hip around the row
decoders), bit-exact against the model of tests/soft_ref.py over the oracle: rows, ok, changed, pattern
and score of every codeword, failed ones included.

Every call runs on device buffers pre-filled with 0xA5: the gaps of a row stride, the gaps of the LLR
stride and 64 guard bytes around every array; whole buffers are compared afterwards, so a byte written
outside a row or a result entry shows, and the LLR buffer is compared with its copy.  The rows a case
decodes are built: t + e symbol errors per codeword, e of them single weak bits, e cycling through 0, 1,
flips and flips + 1 along the batch (soft_ref.built_rows)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child-process test runs this file as a program
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import libpoporon_amd as P
import soft_ref as S

pytestmark = pytest.mark.gpu

G = 64       # guard bytes (entries of the score array)
FILL = 0xA5

RS223 = (8, 0x11D, 1, 1, 32)    # fast kernels
RS204 = (8, 0x11D, 0, 1, 16)    # RS(204,188): fewer roots
RS15 = (4, 0x13, 1, 1, 4)       # RS(15,11) over GF(16): general kernels, 4 LLRs per symbol
RS155 = (8, 0x11D, 1, 1, 100)   # 100 roots
COUNTS = (1, 63, 64, 65)
CASES = [(RS223, 223, f) for f in range(7)] + \
        [(p, s, f) for p, s in ((RS223, 222), (RS223, 40), (RS223, 1), (RS204, 188), (RS15, 11), (RS15, 1),
                                (RS155, 155)) for f in (0, 3, 6)]
KINDS = ("behind", "apart", "behind_padded", "apart_padded")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_handles, _oracles, _models = {}, {}, {}


def _handle(params):
    if params not in _handles:
        _handles[params] = P.Poporon(*params)
        assert _handles[params].supported
    return _handles[params]


def _oracle(params):
    from oracle import Oracle
    if params not in _oracles:
        _oracles[params] = Oracle(*params)
    return _oracles[params]


def _mixed(params, size, count, flips, seed=0):
    """`count` built rows, the number of weak single-bit errors cycling through 0, 1, flips, flips + 1; the
    model's answer for them (computed once per key).  Returns (codewords, llr, weak per row, model)."""
    key = (params, size, count, flips, seed)
    if key not in _models:
        m, o = params[0], _oracle(params)
        rng = np.random.default_rng([size, count, flips, params[4], seed])
        weak = np.array([(0, 1, flips, flips + 1)[c % 4] for c in range(count)])
        cw = np.zeros((count, size + params[4]), np.uint8)
        llr = np.zeros((count, (size + params[4]) * m), np.int8)
        for e in sorted(set(weak.tolist())):
            sel = np.nonzero(weak == e)[0]
            cw[sel], llr[sel] = S.built_rows(o, size, m, sel.size, e, rng)
        _models[key] = (cw, llr, weak, S.soft_decode(o, llr, size, m, flips, threads=8))
    return _models[key]


class Place:
    """where the rows of `count` codewords lie in 0xA5-filled buffers: parity behind the message in one
    buffer or apart from it in a second one, strides exact or padded, the first row `off` bytes past the
    guard"""

    def __init__(self, kind, size, nr, count, off=0):
        self.size, self.nr, self.count = size, nr, count
        W = size + nr
        pad = kind.endswith("_padded")
        if kind.startswith("behind"):
            self.ds = self.ps = W + (9 if pad else 0)
            self.lens = [G + off + (count - 1) * self.ds + W + G]
            self.d, self.p = (0, G + off), (0, G + off + size)
        else:
            self.ds, self.ps = size + (13 if pad else 0), nr + (5 if pad else 0)
            self.lens = [G + off + (count - 1) * self.ds + size + G, G + off + (count - 1) * self.ps + nr + G]
            self.d, self.p = (0, G + off), (1, G + off)

    def image(self, rows=None):
        bufs = [np.full(n, FILL, np.uint8) for n in self.lens]
        if rows is not None:
            for c in range(self.count):
                b, o = self.d
                bufs[b][o + c * self.ds:o + c * self.ds + self.size] = rows[c, :self.size]
                b, o = self.p
                bufs[b][o + c * self.ps:o + c * self.ps + self.nr] = rows[c, self.size:]
        return bufs


def _guarded(torch, n, dtype):
    fill = FILL if dtype == torch.uint8 else int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])
    return torch.full((G + n + G,), fill, dtype=dtype, device="cuda")


def _run(torch, h, params, size, llr, flips, want, kind="behind", off=0, llr_off=0, llr_pad=0, skip=(), stream=0,
         sync=True):
    """one call on fresh buffers; returns a check() that compares every buffer with what `want` (the model's
    dict, or a slice of it) says, after a synchronize"""
    m, nr = params[0], params[4]
    count, bits = llr.shape[0], (size + nr) * m
    assert llr.shape[1] == bits and h.soft_llr_row(size) == bits
    ls = bits + llr_pad
    host_llr = np.full(G + llr_off + (count - 1) * ls + bits + G, FILL, np.uint8).view(np.int8)
    for c in range(count):
        host_llr[G + llr_off + c * ls:G + llr_off + c * ls + bits] = llr[c]
    d_llr = torch.from_numpy(host_llr.copy()).cuda()
    pl = Place(kind, size, nr, count, off)
    dev = [torch.from_numpy(b).cuda() for b in pl.image()]
    outs = {k: _guarded(torch, count, torch.int32 if k == "score" else torch.uint8)
            for k in ("ok", "changed", "pattern", "score")}
    ptr = {k: 0 if k in skip else v.data_ptr() + G * v.element_size() for k, v in outs.items()}
    if stream:  # the fills above ran on the default stream
        torch.cuda.synchronize()
    h.decode_soft_batch_device(d_llr.data_ptr() + G + llr_off, ls, dev[pl.d[0]].data_ptr() + pl.d[1], pl.ds,
                               dev[pl.p[0]].data_ptr() + pl.p[1], pl.ps, size, count, flips, ptr["ok"],
                               changed_ptr=ptr["changed"], pattern_ptr=ptr["pattern"], score_ptr=ptr["score"],
                               stream=stream)

    def check():
        if sync:
            torch.cuda.synchronize()
        assert (d_llr.cpu().numpy() == host_llr).all(), "the LLR buffer changed"
        for got, exp in zip(dev, pl.image(want["rows"])):
            got = got.cpu().numpy()
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (kind, off, count, flips, bad[:8].tolist())
        for k, v in outs.items():
            got = v.cpu().numpy()
            if k == "score":
                got = got.view(np.uint32)
                exp = np.full(G + count + G, 0xA5A5A5A5, np.uint32)
            else:
                exp = np.full(G + count + G, FILL, np.uint8)
            if k not in skip:
                exp[G:G + count] = want[k]
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, (k, kind, count, flips, (bad[:8] - G).tolist(), got[bad[:8]].tolist(),
                                   exp[bad[:8]].tolist())

    return check


def _slice(model, a, b):
    return {k: v[a:b] for k, v in model.items()}


# ---- codes, flips and counts ---------------------------------------------------------------

@pytest.mark.parametrize("params,size,flips", CASES, ids=lambda v: str(v[4]) if isinstance(v, tuple) else str(v))
def test_codes_flips_counts(torch_cuda, params, size, flips):
    """the fast, fewer-roots, general and 100-root decoders behind the candidates; counts 1, 63, 64 and 65
    (a workgroup takes four codewords) are slices of one built batch"""
    torch = torch_cuda
    h = _handle(params)
    total = sum(COUNTS)
    cw, llr, weak, model = _mixed(params, size, total, flips)
    if params[0] == 8:  # within t once the weak bits are flipped: the transmitted codeword
        sure = weak <= flips
        assert model["ok"][sure].all() and (model["rows"][sure] == cw[sure]).all()
    a = 0
    for i, n in enumerate(COUNTS):
        kind = KINDS[(i + flips) % 4]
        _run(torch, h, params, size, llr[a:a + n], flips, _slice(model, a, a + n), kind=kind, off=(0, 1, 15, 0)[i],
             llr_off=(0, 15, 1, 0)[i], llr_pad=(0, 0, 7, 16)[i])()
        a += n


@pytest.mark.parametrize("flips,counts", [(6, (255, 256, 257)), (4, (1023, 1024, 1025))])
def test_candidate_rows_either_side_of_the_split_threshold(torch_cuda, flips, counts):
    """count << flips below, at and above 16,384 rows: the candidates decode on the one-codeword-per-wave
    kernel, then on the split kernels"""
    torch = torch_cuda
    h = _handle(RS223)
    cw, llr, weak, model = _mixed(RS223, 223, counts[-1], flips, seed=1)
    for n in counts:
        h.timing(True)
        _run(torch, h, RS223, 223, llr[:n], flips, _slice(model, 0, n))()
        wave, bm, ex, se = (h.timing_read(k)[1] for k in (P.KERNEL_WAVE, P.KERNEL_BM, P.KERNEL_SOFT_EXPAND,
                                                          P.KERNEL_SOFT_SELECT))
        h.timing(False)
        assert (ex, se) == (1, 1)
        assert (wave, bm) == ((1, 0) if n << flips < 16384 else (0, 1)), (n, wave, bm)


def test_awgn_rows(torch_cuda):
    """what a demodulator delivers: RS(255,223), BPSK over AWGN at Eb/N0 = 5.2 dB, LLR = rint(32 y) clipped to
    +-127; the picks are wherever the noise put them, and the winners' patterns are spread over 0 .. 2^flips - 1"""
    torch = torch_cuda
    h, o = _handle(RS223), _oracle(RS223)
    rng = np.random.default_rng(56)
    cw = S.codewords(o, 223, 8, 96, rng)
    llr = S.awgn_llr(cw, 8, 5.2, 223 / 255, rng)
    ok = None
    for flips in (0, 2, 4, 6):
        model = S.soft_decode(o, llr, 223, 8, flips, threads=8)
        assert ok is None or (model["ok"] >= ok).all()  # the candidates of fewer flips are among those of more
        ok = model["ok"]
        _run(torch, h, RS223, 223, llr, flips, model, kind=KINDS[flips % 4], llr_off=flips)()
    assert len(set(model["pattern"].tolist())) > 8 and (model["rows"][ok == 1] == cw[ok == 1]).all()


# ---- ties, and rows without a winner -------------------------------------------------------

@pytest.mark.parametrize("params,size", [(RS223, 223), (RS223, 40), (RS204, 188), (RS15, 11)])
def test_ties_and_rows_without_a_winner(torch_cuda, params, size):
    torch = torch_cuda
    m, nr = params[0], params[4]
    W, o, h = size + nr, _oracle(params), _handle(params)
    rng = np.random.default_rng(size)
    cw = S.codewords(o, size, m, 1, rng)
    flat = S.clean_llr(cw, m, 9).astype(np.int8)              # a codeword, every magnitude equal
    zero = np.zeros((1, W * m), np.int8)                      # the all-zero row: the zero codeword
    low = np.full((1, W * m), -128, np.int8)                  # every bit 1 at magnitude 128
    junk = np.where(rng.integers(0, 2, (5, W * m)) == 1, -90, 90).astype(np.int8)  # random hard rows
    junk[1, ::3] //= 90                                       # ... one with a third of its bits at +-1
    llr = np.concatenate([flat, zero, low, junk])
    for flips in (0, 1, 3, 6):
        model = S.soft_decode(o, llr, size, m, flips)
        assert model["ok"][0] and (model["rows"][0] == cw[0]).all() and (nr < 16 or model["cand_ok"][0].all())
        assert (model["pattern"][:2] == 0).all() and (model["score"][:2] == 0).all() and model["ok"][1]
        assert (S.picks(llr[:3], W, m, flips) == np.arange(flips)[None, :]).all()
        if nr >= 16:  # a random row of a long code decodes to nothing: it comes back as the hard row
            assert not model["ok"][3:].any() and (model["rows"][3:] == S.hard_rows(junk, W, m)).all()
            assert not model["changed"][3:].any()
        _run(torch, h, params, size, llr, flips, model, kind=KINDS[flips % 4], off=flips % 3)()


# ---- placements ------------------------------------------------------------------------------

@pytest.mark.parametrize("params,size", [(RS223, 40), (RS15, 11)])
def test_placements(torch_cuda, params, size):
    """parity behind the message and apart from it, exact and padded strides, the rows and the LLRs 0, 1 and 15
    bytes off a 16-byte boundary, an LLR stride above the row"""
    torch = torch_cuda
    h = _handle(params)
    flips, count = 3, 21
    cw, llr, weak, model = _mixed(params, size, count, flips, seed=2)
    checks = []
    for kind in KINDS:
        for off in (0, 1, 15):
            for llr_off, llr_pad in ((0, 0), (1, 0), (15, 3), (0, 16), (0, 5)):
                checks.append(_run(torch, h, params, size, llr, flips, model, kind=kind, off=off, llr_off=llr_off,
                                   llr_pad=llr_pad, sync=False))
    torch.cuda.synchronize()
    for check in checks:
        check()


def test_null_optional_outputs(torch_cuda):
    torch = torch_cuda
    h = _handle(RS223)
    flips, count = 2, 9
    cw, llr, weak, model = _mixed(RS223, 40, count, flips, seed=3)
    assert model["changed"].any() and model["pattern"].any() and model["score"].any()
    for skip in (("changed",), ("pattern",), ("score",), ("changed", "pattern", "score")):
        _run(torch, h, RS223, 40, llr, flips, model, skip=skip)()


# ---- flips = 0 -------------------------------------------------------------------------------

@pytest.mark.parametrize("params,size", [(RS223, 223), (RS204, 188), (RS15, 11)])
def test_flips_0_is_the_row_decode_of_the_hard_rows(torch_cuda, params, size):
    torch = torch_cuda
    m, nr = params[0], params[4]
    h = _handle(params)
    count = 65
    cw, llr, weak, model = _mixed(params, size, count, 0, seed=4)
    hard = S.hard_rows(llr, size + nr, m)
    assert (hard == model["hard"]).all() and model["ok"].any() and not model["ok"].all()
    _run(torch, h, params, size, llr, 0, model)()
    rows = torch.from_numpy(hard.copy()).cuda()
    f = torch.full((2, count), FILL, dtype=torch.uint8, device="cuda")
    h.decode_batch_device(rows.data_ptr(), size + nr, rows.data_ptr() + size, size + nr, size, count,
                          f[0].data_ptr(), d_corrected=f[1].data_ptr())
    torch.cuda.synchronize()
    ok = f[0].cpu().numpy()
    assert (ok == model["ok"]).all()
    good = ok != 0
    assert (rows.cpu().numpy()[good] == model["rows"][good]).all()
    assert (model["rows"][~good] == hard[~good]).all()


# ---- streams, timing ids, reserve, chunks --------------------------------------------------

def test_a_callers_stream_two_calls_back_to_back(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    h = _handle(RS223)
    a = _mixed(RS223, 223, 65, 3, seed=5)
    b = _mixed(RS223, 40, 64, 2, seed=6)
    torch.cuda.synchronize()
    ca = _run(torch, h, RS223, 223, a[1], 3, a[3], kind="apart", stream=s.cuda_stream, sync=False)
    cb = _run(torch, h, RS223, 40, b[1], 2, b[3], kind="behind_padded", off=1, stream=s.cuda_stream, sync=False)
    s.synchronize()
    ca()
    cb()
    # and behind them a call on the default stream: the staging rows are ordered across streams
    cc = _run(torch, h, RS223, 223, a[1], 3, a[3], stream=s.cuda_stream, sync=False)
    _run(torch, h, RS223, 40, b[1], 2, b[3])()
    cc()


def test_reserve_then_timing_ids(torch_cuda):
    """after poporon_amd_reserve_soft a call allocates nothing: the device's free memory does not drop by the
    32 MiB of staging rows that 8,192 codewords at flips = 4 take (8 MiB of slack for whatever else the runtime
    does; the device is shared, so a fresh handle gets up to three attempts).  Then 27 and 28 record one launch
    each per call of one chunk, and none for a row call."""
    torch = torch_cuda
    size, nr, m, count, flips = 11, 4, 4, 1 << 13, 4
    W = size + nr
    llr = torch.zeros(count * W * m, dtype=torch.int8, device="cuda")
    rows = torch.full((count * W,), FILL, dtype=torch.uint8, device="cuda")
    f = torch.full((3, count), FILL, dtype=torch.uint8, device="cuda")
    sc = torch.full((count,), -1, dtype=torch.int32, device="cuda")

    def call(h, fl=flips):
        h.decode_soft_batch_device(llr.data_ptr(), W * m, rows.data_ptr(), W, rows.data_ptr() + size, W, size, count,
                                   fl, f[0].data_ptr(), changed_ptr=f[1].data_ptr(), pattern_ptr=f[2].data_ptr(),
                                   score_ptr=sc.data_ptr())

    drops = []
    for _ in range(3):
        h = P.Poporon(*RS15)
        h.reserve_soft(flips, count)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        call(h)
        torch.cuda.synchronize()
        drops.append(free0 - torch.cuda.mem_get_info()[0])
        # the all-zero row is the zero codeword, whatever is flipped: candidate 0 wins at score 0
        assert f[0].all() and not f[1].any() and not f[2].any() and not sc.any() and not rows.any()
        if drops[-1] < 8 << 20:
            break
        h.close()
    assert drops[-1] < 8 << 20, drops

    def launches():
        torch.cuda.synchronize()
        n = [h.timing_read(k)[1] for k in (P.KERNEL_SOFT_EXPAND, P.KERNEL_SOFT_SELECT)]
        ms = [h.timing_read(k)[0] for k in (P.KERNEL_SOFT_EXPAND, P.KERNEL_SOFT_SELECT)]
        h.timing(True)
        return n, ms

    h.timing(True)
    h.decode_batch_device(rows.data_ptr(), W, rows.data_ptr() + size, W, size, 100, f[0].data_ptr())
    assert launches()[0] == [0, 0]
    call(h)
    n, ms = launches()
    assert n == [1, 1] and ms[0] > 0 and ms[1] > 0
    call(h, 0)
    assert launches()[0] == [1, 1]
    h.timing(False)
    h.close()


def _chunk_child():
    """POPORON_AMD_ILV_CHUNK=192 is in this process's environment: a chunk is max(1, 192 >> flips) codewords, so
    100 codewords at flips = 2 are three chunks of 48, 48 and 4, and 5 at flips = 6 two chunks of 3 and 2; a
    handle created under POPORON_AMD_ILV_CHUNK=32 has one codeword per chunk at flips = 6"""
    import torch
    assert os.environ.get("POPORON_AMD_ILV_CHUNK") == "192" and torch.cuda.is_available()

    def run(h, params, size, count, flips, chunks):
        cw, llr, weak, model = _mixed(params, size, count, flips, seed=7)
        h.timing(True)
        _run(torch, h, params, size, llr, flips, model, kind="apart_padded", off=1, llr_off=1, llr_pad=3)()
        n = [h.timing_read(k)[1] for k in (P.KERNEL_SOFT_EXPAND, P.KERNEL_SOFT_SELECT)]
        h.timing(False)
        assert n == [chunks, chunks], (count, flips, n)

    for params, size in ((RS223, 223), (RS15, 11)):
        h = P.Poporon(*params)
        run(h, params, size, 100, 2, 3)
        run(h, params, size, 5, 6, 2)
        run(h, params, size, 96, 1, 1)
        h.close()
    os.environ["POPORON_AMD_ILV_CHUNK"] = "32"  # read at poporon_create
    h = P.Poporon(*RS223)
    run(h, RS223, 223, 5, 6, 5)
    run(h, RS223, 223, 5, 5, 5)
    run(h, RS223, 223, 5, 4, 3)
    h.close()
    print("soft chunks ok")


def test_chunks_in_a_child_process(torch_cuda):
    env = dict(os.environ, POPORON_AMD_ILV_CHUNK="192")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "soft chunks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


if __name__ == "__main__":
    _chunk_child()
