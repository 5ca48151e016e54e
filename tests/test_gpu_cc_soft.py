"""The soft-output decode of the K = 7 code on the GPU (poporon_cc_decode_siso_device, cc_soft.hip), bit-exact
against the model of tests/cc_soft_ref.py.

Every call runs on device buffers pre-filled with 0xA5: the gaps of a stride and 64 guard bytes around every
array; whole buffers are compared afterwards, so a byte written outside a frame shows, and the LLR buffer is
compared with its copy.  The shapes are the ones at which the kernel can go wrong: lengths around the 64 steps
of a segment, around a block and its overlap (the overlap in front of a block decides how far the kernel pads
its window), windows wider than the block and wider than the frame, every base alignment.  The outputs are held
against the unchanged hard decode on the GPU (signs), and feed poporon_decode_soft_batch_device."""
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
import cc_soft_ref as S

pytestmark = pytest.mark.gpu

G = 64       # guard bytes
FILL = 0xA5

P16 = (16, 0b1010000010010110, 0b0110000011010001)  # period 16; phases 3, 5 and 8 .. 12 keep nothing
ODD = (0o171, 0o132, 1)                             # the second polynomial does not tap the oldest bit
CONFIGS = [(R.CCSDS, R.RATE_1_2), (R.DVB, R.RATE_1_2), (R.DVB, R.DVB_2_3), (R.DVB, R.DVB_3_4), (R.DVB, R.DVB_5_6),
           (R.DVB, R.DVB_7_8), (R.DVB, P16), (ODD, R.DVB_3_4)]
OVERLAPS = (0, 1, 6, 7, 63, 64, 65, 200, 1024)
SHIFTS = (0, 3, 8)
RS223 = (8, 0x11D, 1, 1, 32)


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


def _model(code, punct, llr, nbits, block, overlap, start, end, shift):
    """the model's int8 row; D is computed once per frame and boundary states, whatever the shift"""
    key = (code, punct, llr.tobytes(), nbits, block, overlap, start, end)
    if key not in _models:
        _models[key] = S.decode_soft(code, punct, llr, nbits, block, overlap, start, end)[1]
    D = _models[key]
    return S.quantise(D[:, 1] - D[:, 0], shift)


def _frames(code, punct, nbits, count, seed, start=0, sigma=0.85, ties=False):
    """`count` random messages from `start`: (messages, end states, LLRs: AWGN, or magnitudes 0 .. 2)"""
    rng = np.random.default_rng([nbits, count, seed])
    msgs = rng.integers(0, 2, (count, nbits)).astype(np.uint8)
    enc = [R.encode(code, punct, m, start) for m in msgs]
    llrs = [R.llr_ties(e[0], rng) if ties else R.llr_awgn(e[0], rng, sigma) for e in enc]
    return msgs, [e[1] for e in enc], llrs


def _image(rows, off, stride, dtype=np.uint8):
    """the rows at G + off + c * stride of a FILL-ed buffer with G bytes either side"""
    n = len(rows[0])
    img = np.full(G + off + (len(rows) - 1) * stride + n + G, FILL, np.uint8).view(dtype)
    for c, r in enumerate(rows):
        img[G + off + c * stride:G + off + c * stride + n] = r
    return img


def _soft(torch, code, punct, block, overlap, llrs, nbits, start=-1, end=-1, shift=0, llr_off=0, llr_pad=0, off=0,
          pad=0, stream=0, sync=True):
    """one call on fresh buffers; returns a check() that compares every buffer with the model's and returns the
    model's rows"""
    cc = _handle(code, punct, block, overlap)
    count, M = len(llrs), R.n_symbols(punct, nbits)
    assert cc.symbols(nbits) == M == len(llrs[0])
    ls, ss = M + llr_pad, nbits + pad
    host_llr = _image(llrs, llr_off, ls, np.int8)
    d_llr = torch.from_numpy(host_llr.copy()).cuda()
    d_soft = torch.from_numpy(_image([np.full(nbits, FILL, np.uint8)] * count, off, ss)).cuda()
    if stream:  # the fills above ran on the default stream
        torch.cuda.synchronize()
    cc.decode_soft(d_llr.data_ptr() + G + llr_off, ls, nbits, count, d_soft.data_ptr() + G + off, ss, start, end, shift,
                   stream=stream)

    def check():
        if sync:
            torch.cuda.synchronize()
        want = [_model(code, punct, l, nbits, block, overlap, start, end, shift) for l in llrs]
        assert (d_llr.cpu().numpy() == host_llr).all(), "the LLR buffer changed"
        got, exp = d_soft.cpu().numpy().view(np.int8), _image(want, off, ss, np.int8)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, ("soft", code, punct, nbits, block, overlap, start, end, shift, bad.size,
                               (bad[:8] - G - off).tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
        return want

    return check


def _lengths(block, overlap):
    return sorted({1, 5, 6, 7, 63, 64, 65, 127, 128, 129, block - 1, block, block + 1, block + overlap - 1,
                   block + overlap + 1, 2 * block + overlap + 1, 3 * block})


# ---- lengths and overlaps --------------------------------------------------------------------

@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("block", [64, 128])
def test_lengths_and_overlaps(torch_cuda, block, overlap):
    """the codes, the boundary states, the shifts, the kinds of LLRs and the placements cycle along the lengths"""
    torch = torch_cuda
    checks = []
    for i, nbits in enumerate(_lengths(block, overlap)):
        k = i + OVERLAPS.index(overlap) + block // 64
        code, punct = CONFIGS[k % len(CONFIGS)]
        start = (0, 37, 63, 1)[i % 4]
        msgs, ends, llrs = _frames(code, punct, nbits, 1, overlap, start, ties=k % 3 == 2)
        s, e = ((-1, -1), (start, -1), (-1, ends[0]), (start, ends[0]))[k % 4]
        checks.append(_soft(torch, code, punct, block, overlap, llrs, nbits, s, e, SHIFTS[(k // 2) % 3],
                            llr_off=(0, 1, 15)[k % 3], off=(0, 1, 15, 2)[i % 4], sync=False))
    torch.cuda.synchronize()
    for check in checks:
        check()


def test_the_largest_window_and_the_largest_sums(torch_cuda):
    """B = 4096, V = 1024, every LLR +-127 or -128 and random: windows of 6144 steps, 96 segments and one of
    padding, sums past what 17 bits hold"""
    torch = torch_cuda
    nbits = 2 * 4096 + 1500
    rng = np.random.default_rng(4096)
    llr = rng.choice(np.array([127, -127, -128], np.int8), 2 * nbits)
    _soft(torch, R.DVB, R.RATE_1_2, 4096, 1024, [llr], nbits, llr_off=1, off=3)()
    D = _models[(R.DVB, R.RATE_1_2, llr.tobytes(), nbits, 4096, 1024, -1, -1)]
    assert D.min(1).max() > 1 << 17
    _soft(torch, R.DVB, R.RATE_1_2, 4096, 1024, [llr], nbits, 63, 0, shift=8)()


# ---- frames, strides, alignments ---------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 2, 5])
def test_frames_strides_and_alignments(torch_cuda, count):
    torch = torch_cuda
    code, punct, block, overlap, nbits = R.DVB, R.DVB_2_3, 128, 32, 300 + count
    msgs, ends, llrs = _frames(code, punct, nbits, count, 1)
    checks = []
    for llr_off in (0, 1, 15):
        for llr_pad, off, pad in ((0, 0, 0), (3, 1, 0), (16, 15, 5), (1, 8, 1)):
            checks.append(_soft(torch, code, punct, block, overlap, llrs, nbits, 0, -1, shift=(llr_off + off) % 2,
                                llr_off=llr_off, llr_pad=llr_pad, off=off, pad=pad, sync=False))
    torch.cuda.synchronize()
    for check in checks:
        check()


# ---- codes and puncturing; the hard decode's bits ------------------------------------------------

@pytest.mark.parametrize("code,punct", CONFIGS)
def test_codes_and_patterns_and_the_hard_decodes_signs(torch_cuda, code, punct):
    """every configuration at two settings; wherever the GPU's soft output is not 0, its sign is the bit that
    poporon_cc_decode_device returns for the same handle, frames and boundary states"""
    torch = torch_cuda
    nbits, count = 333, 3
    msgs, ends, llrs = _frames(code, punct, nbits, count, 2, start=21)
    M, fb = R.n_symbols(punct, nbits), -(-nbits // 8)
    nonzero = 0
    for block, overlap, start, shift in ((128, 40, 21, 0), (64, 200, -1, 3)):
        want = _soft(torch, code, punct, block, overlap, llrs, nbits, start, -1, shift)()
        cc = _handle(code, punct, block, overlap)
        d_llr = torch.from_numpy(np.stack(llrs)).cuda()
        d_soft = torch.zeros((count, nbits), dtype=torch.int8, device="cuda")
        d_bits = torch.zeros((count, fb), dtype=torch.uint8, device="cuda")
        cc.decode_soft(d_llr, M, nbits, count, d_soft, nbits, start, -1, shift)
        cc.decode(d_llr, M, nbits, count, d_bits, fb, start, -1)
        torch.cuda.synchronize()
        soft = d_soft.cpu().numpy()
        bits = np.stack([R.unpack(r, nbits) for r in d_bits.cpu().numpy()])
        assert (soft == np.stack(want)).all()
        assert ((soft < 0) == (bits == 1))[soft != 0].all()
        nonzero += int((soft != 0).sum())
    if (code, punct) in CONFIGS[:4]:  # rates up to 3/4 decode at this noise: most outputs say something
        assert nonzero > count * nbits


# ---- zeros, saturated values and the values between -----------------------------------------------

def test_ties_saturation_and_the_values_between(torch_cuda):
    """asserted on the model's rows: frames of magnitudes 0 .. 2 give outputs of 0, AWGN frames at shift 0 give
    +-127, a shift gives values strictly between, of both signs; an all-zero frame gives zeros only"""
    torch = torch_cuda
    nbits, block, overlap = 200, 64, 16
    code, punct = R.DVB, R.RATE_1_2
    _, _, ties = _frames(code, punct, nbits, 2, 7, ties=True)
    _, _, awgn = _frames(code, punct, nbits, 2, 8, sigma=0.85)
    zero = np.zeros(2 * nbits, np.int8)
    low = np.full(2 * nbits, -128, np.int8)
    rows = ties + awgn + [zero, low]
    want0 = np.stack(_soft(torch, code, punct, block, overlap, rows, nbits, llr_off=1)())
    want3 = np.stack(_soft(torch, code, punct, block, overlap, rows, nbits, shift=3, off=1, pad=2)())
    assert (want0[:2] == 0).sum() > 20
    assert (want0[2:4] == 127).sum() > 20 and (want0[2:4] == -127).sum() > 20
    between = want3[2:4][(np.abs(want3[2:4]) > 0) & (np.abs(want3[2:4]) < 127)]
    assert (between > 0).sum() > 20 and (between < 0).sum() > 20
    assert not want0[4].any() and (want0[5] == -127).all()
    for rows_of in (want0, want3):
        assert rows_of.min() >= -127
    _soft(torch, R.CCSDS, R.DVB_7_8, block, 1024, [np.zeros(R.n_symbols(R.DVB_7_8, nbits), np.int8)], nbits, -1, 0)()


# ---- a caller's stream -----------------------------------------------------------------------------

def test_a_callers_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    code, punct = R.CCSDS, R.DVB_5_6
    msgs, ends, llrs = _frames(code, punct, 777, 3, 4)
    torch.cuda.synchronize()
    a = _soft(torch, code, punct, 256, 48, llrs, 777, 0, -1, stream=s.cuda_stream, sync=False)
    b = _soft(torch, code, punct, 64, 7, llrs, 777, -1, -1, shift=3, stream=s.cuda_stream, sync=False)
    s.synchronize()
    a()
    b()


# ---- the chunk edge ------------------------------------------------------------------------------

def _chunk_child():
    """POPORON_AMD_CC_CHUNK=3 is in this process's environment: a launch takes three blocks"""
    import torch
    assert os.environ.get("POPORON_AMD_CC_CHUNK") == "3" and torch.cuda.is_available()
    code, punct = R.DVB, R.DVB_3_4
    for nbits, count in ((64 * 7 + 5, 2), (64, 5), (64 * 3, 2), (3000, 1)):
        msgs, ends, llrs = _frames(code, punct, nbits, count, 5)
        _soft(torch, code, punct, 64, 20, llrs, nbits, 0, -1, llr_off=1, pad=1)()
    print("cc soft chunks ok")


def test_the_chunk_edge_in_a_child_process(torch_cuda):
    env = dict(os.environ, POPORON_AMD_CC_CHUNK="3")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chunks"], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "cc soft chunks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- a long frame ------------------------------------------------------------------------------

def test_a_long_frame(torch_cuda):
    """2^16 bits at rate 3/4 over AWGN at the library's default block and overlap (512 / 96): 128 blocks"""
    torch = torch_cuda
    nbits = 1 << 16
    msgs, ends, llrs = _frames(R.DVB, R.DVB_3_4, nbits, 1, 6, sigma=0.5)
    _handles[(R.DVB, R.DVB_3_4, 512, 96)] = P.Cc(R.DVB, R.DVB_3_4, P.CC_DEFAULT_BLOCK, P.CC_DEFAULT_OVERLAP)
    want = _soft(torch, R.DVB, R.DVB_3_4, 512, 96, llrs, nbits, 0, ends[0], llr_off=1)()
    assert int(((want[0] < 0) != (msgs[0] == 1)).sum()) < nbits // 100


# ---- the soft chain ----------------------------------------------------------------------------

def _chain(torch, frames_of, nbits, flips_list, seed):
    """RS(255,223) codewords -> the frames' bytes by frames_of -> poporon_cc_encode_device (CCSDS, rate 1/2) ->
    AWGN LLRs -> the soft decode at shift 0 -> rows of 2040 LLRs by the inverse of frames_of, in torch ->
    poporon_decode_soft_batch_device; bit-exact against cc_soft_ref followed by soft_ref"""
    import soft_ref as SR
    from oracle import Oracle
    size, nr, W = 223, 32, 255
    orc, h = Oracle(*RS223), P.Poporon(*RS223)
    rng = np.random.default_rng(seed)
    cw = SR.codewords(orc, size, 8, 4, rng)
    frames, rows_of = frames_of(torch, cw)
    count, fb = frames.shape
    assert fb * 8 == nbits
    code, punct, block, overlap = R.CCSDS, R.RATE_1_2, 512, 96
    cc = _handle(code, punct, block, overlap)
    M = cc.symbols(nbits)
    d_msg = torch.from_numpy(frames).cuda()
    d_sym = torch.zeros((count, M // 8), dtype=torch.uint8, device="cuda")
    cc.encode(d_msg, fb, nbits, count, d_sym, M // 8)
    torch.cuda.synchronize()
    sym = [R.unpack(r, M) for r in d_sym.cpu().numpy()]
    assert all((s == R.encode(code, punct, R.unpack(f, nbits), 0)[0]).all() for s, f in zip(sym, frames))
    llrs = [R.llr_awgn(s, rng, 0.8) for s in sym]
    d_llr = torch.from_numpy(np.stack(llrs)).cuda()
    d_soft = torch.full((count, nbits), -128, dtype=torch.int8, device="cuda")
    cc.decode_soft(d_llr, M, nbits, count, d_soft, nbits, 0, -1, 0)
    soft = np.stack([_model(code, punct, l, nbits, block, overlap, 0, -1, 0) for l in llrs])
    assert (d_soft.cpu().numpy() == soft).all()
    d_rows = rows_of(d_soft).contiguous()               # (4, 2040) int8: a valid LLR row per codeword
    want_rows = rows_of(torch.from_numpy(soft)).contiguous().numpy()
    assert d_rows.shape == (4, W * 8) and h.soft_llr_row(size) == W * 8
    for flips in flips_list:
        model = SR.soft_decode(orc, want_rows, size, 8, flips, threads=8)
        out = torch.full((4, W), FILL, dtype=torch.uint8, device="cuda")
        res = {k: torch.full((4,), FILL, dtype=torch.int32 if k == "score" else torch.uint8, device="cuda")
               for k in ("ok", "changed", "pattern", "score")}
        h.decode_soft_batch_device(d_rows.data_ptr(), W * 8, out.data_ptr(), W, out.data_ptr() + size, W, size, 4,
                                   flips, res["ok"].data_ptr(), changed_ptr=res["changed"].data_ptr(),
                                   pattern_ptr=res["pattern"].data_ptr(), score_ptr=res["score"].data_ptr())
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == model["rows"]).all()
        for k, v in res.items():
            assert (v.cpu().numpy().astype(np.int64) == model[k]).all(), (k, flips)
    h.close()


def test_the_soft_chain_one_frame_per_codeword(torch_cuda):
    _chain(torch_cuda, lambda torch, cw: (cw.copy(), lambda soft: soft), 2040, (0, 4), 255)


def test_the_soft_chain_four_codewords_interleaved_in_one_frame(torch_cuda):
    """symbol j of codeword c is byte 4 j + c of the frame; the caller's de-interleave of the LLRs is a permute"""
    def frames_of(torch, cw):
        return (np.ascontiguousarray(cw.T).reshape(1, 4 * 255),
                lambda soft: soft.reshape(255, 4, 8).permute(1, 0, 2).reshape(4, 2040))
    _chain(torch_cuda, frames_of, 4 * 2040, (0, 4), 1020)


if __name__ == "__main__":
    _chunk_child()
