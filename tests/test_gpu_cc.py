"""The K = 7 convolutional code on the GPU (poporon_cc_encode_device, poporon_cc_decode_device, cc.hip),
bit-exact against the model of tests/cc_ref.py: bits, metrics, symbols and end states.

Every call runs on device buffers pre-filled with 0xA5: the gaps of a stride and 64 guard bytes (entries of
the metric array) around every array; whole buffers are compared afterwards, so a byte written outside a
frame or a result entry shows, and the LLR and input buffers are compared with their copies.  The shapes
are the ones at which the kernels can go wrong: lengths around the 64 steps a wave runs at a time, around
a block and its overlap, windows wider than the block and wider than the frame, every base alignment."""
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
import cc_ref as R

pytestmark = pytest.mark.gpu

G = 64       # guard bytes (entries of the metric array)
FILL = 0xA5
FILL32 = 0xA5A5A5A5

P16 = (16, 0b1010000010010110, 0b0110000011010001)  # period 16; phases 3, 5 and 8 .. 12 keep nothing
ODD = (0o171, 0o132, 1)                             # the second polynomial does not tap the oldest bit
CONFIGS = [(R.CCSDS, R.RATE_1_2), (R.DVB, R.RATE_1_2), (R.DVB, R.DVB_2_3), (R.DVB, R.DVB_3_4), (R.DVB, R.DVB_5_6),
           (R.DVB, R.DVB_7_8), (R.DVB, P16), (ODD, R.DVB_3_4)]
OVERLAPS = (0, 1, 6, 7, 64, 200, 1024)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_handles, _models = {}, {}


def _handle(code, punct, block, overlap):
    key = (code, punct, block, overlap)
    if key not in _handles:
        _handles[key] = P.Cc(code, punct, block, overlap)
    return _handles[key]


def _model(code, punct, llr, nbits, block, overlap, start, end):
    key = (code, punct, llr.tobytes(), nbits, block, overlap, start, end)
    if key not in _models:
        _models[key] = R.decode(code, punct, llr, nbits, block, overlap, start, end)
    return _models[key]


def _frames(code, punct, nbits, count, seed, start=0, sigma=0.8):
    """`count` random messages from `start`: (messages, symbols, end states, AWGN LLRs)"""
    rng = np.random.default_rng([nbits, count, seed])
    msgs = rng.integers(0, 2, (count, nbits)).astype(np.uint8)
    enc = [R.encode(code, punct, m, start) for m in msgs]
    return msgs, [e[0] for e in enc], [e[1] for e in enc], [R.llr_awgn(e[0], rng, sigma) for e in enc]


def _image(rows, off, stride, dtype=np.uint8):
    """the rows at G + off + c * stride of a FILL-ed buffer with G bytes either side"""
    n = len(rows[0])
    img = np.full(G + off + (len(rows) - 1) * stride + n + G, FILL, np.uint8).view(dtype)
    for c, r in enumerate(rows):
        img[G + off + c * stride:G + off + c * stride + n] = r
    return img


def _decode(torch, code, punct, block, overlap, llrs, nbits, start=-1, end=-1, llr_off=0, llr_pad=0, off=0, pad=0,
            metric=True, stream=0, sync=True):
    """one decode call on fresh buffers; returns a check() that compares every buffer with the model's"""
    cc = _handle(code, punct, block, overlap)
    count, M, fb, nb = len(llrs), R.n_symbols(punct, nbits), -(-nbits // 8), R.n_blocks(block, nbits)
    assert cc.symbols(nbits) == M == len(llrs[0]) and cc.blocks(nbits) == nb
    ls, bs = M + llr_pad, fb + pad
    host_llr = _image(llrs, llr_off, ls, np.int8)
    d_llr = torch.from_numpy(host_llr.copy()).cuda()
    d_bits = torch.from_numpy(_image([np.full(fb, FILL, np.uint8)] * count, off, bs)).cuda()
    d_met = torch.full((G + count * nb + G,), int(np.array([FILL32], np.uint32).view(np.int32)[0]), dtype=torch.int32,
                       device="cuda")
    if stream:  # the fills above ran on the default stream
        torch.cuda.synchronize()
    cc.decode(d_llr.data_ptr() + G + llr_off, ls, nbits, count, d_bits.data_ptr() + G + off, bs, start, end,
              d_metric=d_met.data_ptr() + 4 * G if metric else None, stream=stream)

    def check():
        if sync:
            torch.cuda.synchronize()
        want = [_model(code, punct, l, nbits, block, overlap, start, end) for l in llrs]
        assert (d_llr.cpu().numpy() == host_llr).all(), "the LLR buffer changed"
        got, exp = d_bits.cpu().numpy(), _image([R.pack(w[0]) for w in want], off, bs)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, ("bits", nbits, block, overlap, (bad[:8] - G - off).tolist(), got[bad[:8]].tolist(),
                               exp[bad[:8]].tolist())
        got, exp = d_met.cpu().numpy().view(np.uint32), np.full(G + count * nb + G, FILL32, np.uint32)
        if metric:
            exp[G:G + count * nb] = np.concatenate([w[1] for w in want])
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, ("metric", nbits, block, overlap, (bad[:8] - G).tolist(), got[bad[:8]].tolist(),
                               exp[bad[:8]].tolist())
        return want

    return check


def _encode(torch, code, punct, msgs, start=0, off=0, pad=0, sym_off=0, sym_pad=0, end=True, stream=0):
    """one encode call on fresh buffers, compared with the model; returns the end states the GPU wrote"""
    cc = _handle(code, punct, 64, 0)
    count, nbits = len(msgs), len(msgs[0])
    M, fb = R.n_symbols(punct, nbits), -(-nbits // 8)
    sb = -(-M // 8)
    bs, ss = fb + pad, sb + sym_pad
    host_bits = _image([R.pack(m) for m in msgs], off, bs)
    d_bits = torch.from_numpy(host_bits.copy()).cuda()
    d_sym = torch.from_numpy(_image([np.full(sb, FILL, np.uint8)] * count, sym_off, ss)).cuda()
    d_end = torch.full((G + count + G,), FILL, dtype=torch.uint8, device="cuda")
    if stream:
        torch.cuda.synchronize()
    cc.encode(d_bits.data_ptr() + G + off, bs, nbits, count, d_sym.data_ptr() + G + sym_off, ss, start,
              d_end_state=d_end.data_ptr() + G if end else None, stream=stream)
    torch.cuda.synchronize()
    want = [R.encode(code, punct, m, start) for m in msgs]
    assert (d_bits.cpu().numpy() == host_bits).all(), "the input bits changed"
    got, exp = d_sym.cpu().numpy(), _image([R.pack(w[0]) for w in want], sym_off, ss)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("symbols", code, punct, nbits, (bad[:8] - G - sym_off).tolist(), got[bad[:8]].tolist(),
                           exp[bad[:8]].tolist())
    exp = np.full(G + count + G, FILL, np.uint8)
    if end:
        exp[G:G + count] = [w[1] for w in want]
    got = d_end.cpu().numpy()
    assert (got == exp).all(), ("end states", code, punct, nbits, got[G:G + count].tolist(), exp[G:G + count].tolist())
    return got[G:G + count].tolist()


def _lengths(block, overlap):
    return sorted({1, 5, 6, 7, 8, 9, 63, 64, 65, block - 1, block, block + 1, block + overlap,
                   2 * block + overlap + 1, 3 * block + 13})  # 3 B + 13: a last block of 13 steps, 5 in its last byte


# ---- lengths and overlaps --------------------------------------------------------------------

@pytest.mark.parametrize("overlap", OVERLAPS)
def test_lengths_and_overlaps(torch_cuda, overlap):
    """B = 64; the codes, the boundary states and the placements cycle along the lengths; the encoder runs on
    the same frames, and a terminated decode takes the end state the encoder wrote"""
    torch = torch_cuda
    block = 64
    checks = []
    for i, nbits in enumerate(_lengths(block, overlap)):
        code, punct = CONFIGS[(i + OVERLAPS.index(overlap)) % len(CONFIGS)]
        start = (0, 37, 63, 1)[i % 4]
        msgs, syms, ends, llrs = _frames(code, punct, nbits, 2, overlap, start)
        got_ends = _encode(torch, code, punct, msgs, start, off=i % 3, pad=(0, 3)[i % 2], sym_off=(0, 1, 15)[i % 3],
                           sym_pad=(0, 5)[(i // 2) % 2], end=i % 5 != 4)
        assert i % 5 == 4 or got_ends == ends
        for c in range(2):  # start and end go to a call by value: frames with their own end state, one at a time
            s, e = ((-1, -1), (start, -1), (-1, ends[c]), (start, ends[c]))[(i + c) % 4]
            checks.append(_decode(torch, code, punct, block, overlap, llrs[c:c + 1], nbits, s, e,
                                  llr_off=(0, 1, 15)[(i + c) % 3], off=(i + c) % 4, metric=(i + c) % 5 != 0, sync=False))
        checks.append(_decode(torch, code, punct, block, overlap, llrs, nbits, start, -1, llr_off=(15, 0, 1)[i % 3],
                              llr_pad=(0, 7)[i % 2], off=i % 2, pad=(0, 2, 9)[i % 3], sync=False))
    torch.cuda.synchronize()
    for check in checks:
        check()


def test_the_largest_window_and_the_largest_metrics(torch_cuda):
    """B = 4096, V = 1024, every LLR +-127 or -128 and random: windows of 6144 steps, metrics past what 17 bits hold"""
    torch = torch_cuda
    nbits = 2 * 4096 + 1500
    rng = np.random.default_rng(4096)
    llr = rng.choice(np.array([127, -127, -128], np.int8), 2 * nbits)
    want = _decode(torch, R.DVB, R.RATE_1_2, 4096, 1024, [llr], nbits, llr_off=1)()
    assert want[0][1].max() > 1 << 17 and len(want[0][1]) == 3


# ---- frames, strides, alignments ---------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 2, 5])
def test_frames_strides_and_alignments(torch_cuda, count):
    torch = torch_cuda
    code, punct, block, overlap, nbits = R.DVB, R.DVB_2_3, 128, 32, 300 + count
    msgs, syms, ends, llrs = _frames(code, punct, nbits, count, 1)
    checks = []
    for llr_off in (0, 1, 15):
        for llr_pad, off, pad in ((0, 0, 0), (3, 1, 0), (16, 7, 5), (1, 8, 1)):
            checks.append(_decode(torch, code, punct, block, overlap, llrs, nbits, 0, -1, llr_off=llr_off,
                                  llr_pad=llr_pad, off=off, pad=pad, sync=False))
            _encode(torch, code, punct, msgs, 0, off=llr_off, pad=llr_pad, sym_off=off, sym_pad=pad)
    torch.cuda.synchronize()
    for check in checks:
        check()


# ---- codes and puncturing ----------------------------------------------------------------------

@pytest.mark.parametrize("code,punct", CONFIGS)
def test_codes_and_patterns(torch_cuda, code, punct):
    torch = torch_cuda
    nbits, count = 333, 3
    msgs, syms, ends, llrs = _frames(code, punct, nbits, count, 2, start=21, sigma=0.5)
    assert _encode(torch, code, punct, msgs, 21) == ends
    _encode(torch, code, punct, msgs, 21, end=False, sym_off=3)
    want = _decode(torch, code, punct, 128, 40, llrs, nbits, 21, -1)()
    if (code, punct) in CONFIGS[:4]:  # rates up to 3/4 decode nearly clean at this noise
        assert sum(int((w[0] != m).sum()) for w, m in zip(want, msgs)) < 20
    _decode(torch, code, punct, 64, 200, llrs, nbits, -1, -1, metric=False)()


def test_round_trip(torch_cuda):
    """encode on the GPU, +-32 LLRs from the symbols it wrote, decode: the messages, at metric 0"""
    torch = torch_cuda
    for code, punct in CONFIGS[:6]:
        nbits, count = 1000, 4
        cc = _handle(code, punct, 256, 64)
        rng = np.random.default_rng(nbits)
        msgs = rng.integers(0, 2, (count, nbits)).astype(np.uint8)
        M, fb = cc.symbols(nbits), 125
        d_msg = torch.from_numpy(np.stack([R.pack(m) for m in msgs])).cuda()
        d_sym = torch.zeros((count, -(-M // 8)), dtype=torch.uint8, device="cuda")
        cc.encode(d_msg, fb, nbits, count, d_sym, d_sym.shape[1])
        sym = np.stack([R.unpack(r, M) for r in d_sym.cpu().numpy()])
        d_llr = torch.from_numpy(np.where(sym != 0, -32, 32).astype(np.int8)).cuda()
        d_out = torch.full((count, fb), FILL, dtype=torch.uint8, device="cuda")
        d_met = torch.full((count, cc.blocks(nbits)), -1, dtype=torch.int32, device="cuda")
        cc.decode(d_llr, M, nbits, count, d_out, fb, 0, -1, d_metric=d_met)
        torch.cuda.synchronize()
        assert torch.equal(d_out, d_msg) and not d_met.any()


# ---- ties and erasures -------------------------------------------------------------------------

@pytest.mark.parametrize("code,punct", [(R.DVB, R.RATE_1_2), (R.CCSDS, R.DVB_3_4), (ODD, R.DVB_7_8)])
def test_ties_and_erasures(torch_cuda, code, punct):
    torch = torch_cuda
    nbits, block, overlap = 400, 128, 16
    M = R.n_symbols(punct, nbits)
    rng = np.random.default_rng(M)
    msgs, syms, ends, llrs = _frames(code, punct, nbits, 3, 3)
    zero = np.zeros(M, np.int8)                                # nothing received: every path costs 0
    ones = R.llr_ties(syms[0], rng, flip=0.15, top=1)          # magnitudes 0 and 1
    unit = np.where(rng.integers(0, 2, M) == 1, -1, 1).astype(np.int8)  # magnitudes of 1 only, random signs
    third = llrs[1].copy()
    third[rng.permutation(M)[:M // 3]] = 0                     # a third of the symbols erased
    small = R.llr_ties(syms[2], rng)                           # magnitudes 0 .. 2, a fifth of the signs wrong
    for s, e in ((-1, -1), (0, -1)):
        want = _decode(torch, code, punct, block, overlap, [zero, ones, unit, third, small], nbits, s, e, llr_off=1)()
        assert not want[0][0].any() and not want[0][1].any()  # ties go to d = 0 and to state 0: the zero path
    _decode(torch, code, punct, block, 1024, [zero, unit], nbits, -1, 0, metric=False)()


# ---- optional outputs, a caller's stream -------------------------------------------------------

def test_a_callers_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    code, punct = R.CCSDS, R.DVB_5_6
    msgs, syms, ends, llrs = _frames(code, punct, 777, 3, 4)
    torch.cuda.synchronize()
    a = _decode(torch, code, punct, 256, 48, llrs, 777, 0, -1, stream=s.cuda_stream, sync=False)
    b = _decode(torch, code, punct, 64, 7, llrs, 777, -1, -1, metric=False, stream=s.cuda_stream, sync=False)
    s.synchronize()
    a()
    b()
    assert _encode(torch, code, punct, msgs, 0, stream=s.cuda_stream) == ends


# ---- the chunk edge ------------------------------------------------------------------------------

def _chunk_child():
    """POPORON_AMD_CC_CHUNK=3 is in this process's environment: a decode launch takes three blocks, an encode
    launch 192 threads"""
    import torch
    assert os.environ.get("POPORON_AMD_CC_CHUNK") == "3" and torch.cuda.is_available()
    code, punct = R.DVB, R.DVB_3_4
    for nbits, count in ((64 * 7 + 5, 2), (64, 5), (64 * 3, 2), (9000, 1)):
        msgs, syms, ends, llrs = _frames(code, punct, nbits, count, 5)
        assert _encode(torch, code, punct, msgs, 0, sym_off=1, sym_pad=2) == ends
        _decode(torch, code, punct, 64, 20, llrs, nbits, 0, -1, llr_off=1, pad=1)()
    print("cc chunks ok")


def test_the_chunk_edge_in_a_child_process(torch_cuda):
    env = dict(os.environ, POPORON_AMD_CC_CHUNK="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "cc chunks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- a long frame ------------------------------------------------------------------------------

def test_a_long_frame(torch_cuda):
    """2^20 bits at rate 3/4 over AWGN, B = 512, V = 64: 2048 blocks of one frame"""
    torch = torch_cuda
    nbits = 1 << 20
    msgs, syms, ends, llrs = _frames(R.DVB, R.DVB_3_4, nbits, 1, 6, sigma=0.4)
    assert _encode(torch, R.DVB, R.DVB_3_4, msgs, 0) == ends
    want = _decode(torch, R.DVB, R.DVB_3_4, 512, 64, llrs, nbits, 0, ends[0], llr_off=1)()
    assert int((want[0][0] != msgs[0]).sum()) < nbits // 1000


# ---- the chain, once ---------------------------------------------------------------------------

def test_the_receive_chain(torch_cuda):
    """RS(204,188) codewords through the DVB Forney interleaver (12 x 17) are the info bits of the inner code at
    3/4; a few dozen symbols arrive with the wrong sign; the Viterbi decode's output goes to
    poporon_decode_conv_device, and the messages come back"""
    torch = torch_cuda
    params, size, nr, I, M, phase, count = (8, 0x11D, 0, 1, 16), 188, 16, 12, 17, 0, 12
    W = size + nr
    h = P.Poporon(*params)
    rng = np.random.default_rng(204)
    msg = rng.integers(0, 256, (count, size), dtype=np.uint8)
    rows = torch.from_numpy(np.concatenate([msg, np.zeros((count, nr), np.uint8)], 1)).cuda()
    span = P.conv_span(W, count, I, M)
    stream = torch.zeros(span, dtype=torch.uint8, device="cuda")  # the holes of the span: zeros
    h.encode_conv_device(rows.data_ptr(), W, rows.data_ptr() + size, W, size, count, I, M, phase, stream.data_ptr())
    code, punct, nbits = R.DVB, R.DVB_3_4, 8 * span
    cc = _handle(code, punct, 512, 64)
    ns = cc.symbols(nbits)
    sym = torch.zeros(-(-ns // 8), dtype=torch.uint8, device="cuda")
    cc.encode(stream, span, nbits, 1, sym, sym.numel())
    torch.cuda.synchronize()
    sent = stream.cpu().numpy()
    hard = R.unpack(sym.cpu().numpy(), ns)
    assert (hard == R.encode(code, punct, R.unpack(sent, nbits), 0)[0]).all()
    llr = np.where(hard != 0, -32, 32).astype(np.int8)
    llr[rng.permutation(ns)[:40] // 50 * 50] *= -1  # up to 40 sign flips, at least 50 symbols apart
    bits, _ = R.decode(code, punct, llr, nbits, 512, 64, 0, -1)
    assert (R.pack(bits) == sent).all()  # the model alone returns the stream
    d_llr = torch.from_numpy(llr).cuda()
    back = torch.full((span,), FILL, dtype=torch.uint8, device="cuda")
    cc.decode(d_llr, ns, nbits, 1, back, span, 0, -1)
    out = torch.full((count, W), FILL, dtype=torch.uint8, device="cuda")
    okc = torch.full((2, count), FILL, dtype=torch.uint8, device="cuda")
    h.decode_conv_device(back.data_ptr(), I, M, phase, out.data_ptr(), W, out.data_ptr() + size, W, size, count,
                         okc[0].data_ptr(), okc[1].data_ptr())
    torch.cuda.synchronize()
    assert (back.cpu().numpy() == sent).all()
    assert okc[0].cpu().numpy().all() and (out.cpu().numpy()[:, :size] == msg).all()
    assert torch.equal(out, rows)
    h.close()


if __name__ == "__main__":
    _chunk_child()
