"""Erasure lists from a flag plane on the GPU (poporon_amd_erasures_from_mask_device,
rs_mask_lists_k) against tests/report_ref.py's expect_lists on the de-interleaved
plane, and end to end: a flagged burst in interleaved frames, mask -> lists ->
poporon_decode_interleaved_device, restores the clean frames, as the oracle says.

Planes, positions, counts and over lie in device buffers whose stride gaps and
64 guard bytes on either side hold 0xA5; the whole buffers are compared."""
import numpy as np
import pytest

import libpoporon_amd as P
from interleave_ref import expect_decode, expect_encode, frames_to_rows, rows_to_frames
from report_ref import expect_lists

pytestmark = pytest.mark.gpu

G = 64
FILL = 0xA5
NR = 32
RS223 = (8, 0x11D, 1, 1, 32)
RS239 = (8, 0x11D, 1, 1, 16)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


_handles = {}


def _handle(params=RS223):
    if params not in _handles:
        _handles[params] = P.Poporon(*params)
    return _handles[params]


def _plane(size, depth, ncw, nr, seed=0):
    """flag rows u8[ncw, size]: by codeword none, j = 0, j = size - 1, both ends, nr, nr + 1, all and
    a sparse random set of flags; values 1, 0x80 and 0xFF"""
    rng = np.random.default_rng([seed, size, depth, ncw, nr])
    rows = np.zeros((ncw, size), np.uint8)
    for c in range(ncw):
        mode = c % 8
        if mode == 1:
            j = [0]
        elif mode == 2:
            j = [size - 1]
        elif mode == 3:
            j = [0, size - 1]
        elif mode == 4:
            j = rng.permutation(size)[:nr]
        elif mode == 5:
            j = rng.permutation(size)[:nr + 1]
        elif mode == 6:
            j = np.arange(size)
        elif mode == 7:
            j = np.nonzero(rng.random(size) < 0.05)[0]
        else:
            j = []
        rows[c, j] = np.array([1, 0x80, 0xFF], np.uint8)[(np.arange(len(j)) + c) % 3]
    return rows


def _run(torch, h, nr, size, depth, nframes, pad, off, pstride, over=True, stream=0, rows=None):
    ncw = nframes * depth
    rows = _plane(size, depth, ncw, nr) if rows is None else rows
    frames = rows_to_frames(rows, depth)
    fb, ms = size * depth, size * depth + pad
    plane = np.full(2 * G + off + nframes * ms, FILL, np.uint8)
    for f in range(nframes):
        plane[G + off + f * ms: G + off + f * ms + fb] = frames[f]
    dplane = torch.from_numpy(plane).cuda()
    dpos = torch.full((2 * G + ncw * pstride,), FILL, dtype=torch.uint8, device="cuda")
    dflat = torch.full((2, 2 * G + ncw), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.erasures_from_mask_device(dplane.data_ptr() + G + off, ms, size, depth, nframes, dpos.data_ptr() + G, pstride,
                                dflat[0].data_ptr() + G, dflat[1].data_ptr() + G if over else None, stream=stream)
    torch.cuda.synchronize()
    wpos, wcnt, wover = expect_lists(rows, nr)
    want_pos = np.full(2 * G + ncw * pstride, FILL, np.uint8)
    want_pos[G:G + ncw * pstride].reshape(ncw, pstride)[:, :nr] = wpos
    want_flat = np.full((2, 2 * G + ncw), FILL, np.uint8)
    want_flat[0, G:G + ncw] = wcnt
    if over:
        want_flat[1, G:G + ncw] = wover
    assert (dplane.cpu().numpy() == plane).all(), "the plane was written"
    assert (dflat.cpu().numpy()[0] == want_flat[0]).all(), "counts"
    assert (dflat.cpu().numpy()[1] == want_flat[1]).all(), "over"
    assert (dpos.cpu().numpy() == want_pos).all(), "positions"
    return wcnt, wover


@pytest.mark.parametrize("target", [63, 65, 257, 600])
@pytest.mark.parametrize("size", [223, 222, 96, 2, 1])
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 8, 64])
def test_lists(torch_cuda, depth, size, target):
    """codeword counts around 64, around a tile of 256 lanes and over several workgroups; a
    contiguous plane at two alignments and a padded one; both output strides"""
    h = _handle()
    nframes = max(1, -(-target // depth))
    cnt, over = _run(torch_cuda, h, NR, size, depth, nframes, 0, 0, NR)
    _run(torch_cuda, h, NR, size, depth, nframes, 0, 7, NR + 3, over=False)
    _run(torch_cuda, h, NR, size, depth, nframes, 5, 1, NR + 3)
    _run(torch_cuda, h, NR, size, depth, nframes, 16 - (size * depth) % 16, 0, NR)  # 16-byte aligned frames
    if size > NR and nframes * depth >= 8:
        assert over.any() and (cnt == NR).any() and (cnt == 0).any() and (cnt == 1).any()


def test_fewer_roots_and_a_stream(torch_cuda):
    torch = torch_cuda
    s = torch.cuda.Stream()
    h = _handle(RS239)
    for depth in (1, 5):
        _run(torch, h, 16, 239, depth, 70, 3, 2, 16, stream=s.cuda_stream)
        _run(torch, h, 16, 50, depth, 70, 0, 0, 19, stream=s.cuda_stream)


def test_timing_id(torch_cuda):
    h = _handle()
    h.timing(True)
    _run(torch_cuda, h, NR, 223, 4, 70, 0, 0, NR)
    ms, n = h.timing_read(P.KERNEL_MASK_LISTS)
    h.timing(False)
    assert n == 1 and ms > 0


@pytest.mark.parametrize("depth", [1, 5, 8])
def test_burst_end_to_end(torch_cuda, depth):
    """clean frames; a burst of depth * nr consecutive bytes overwritten and flagged; mask -> lists ->
    decode_interleaved_device restores the clean frames; over is 0, and the oracle agrees"""
    torch = torch_cuda
    from oracle import Oracle
    o = Oracle(*RS223)
    h = _handle()
    size, nframes = 223, 40
    ncw = nframes * depth
    rng = np.random.default_rng([depth, 99])
    clean_d = rows_to_frames(rng.integers(0, 256, (ncw, size), dtype=np.uint8), depth)
    clean_p = expect_encode(o, clean_d, depth)
    rd = clean_d.copy()
    mask = np.zeros_like(rd)
    for f in range(nframes):
        s0 = int(rng.integers(0, size * depth - depth * NR + 1))
        rd[f, s0:s0 + depth * NR] = rng.integers(0, 256, depth * NR)
        mask[f, s0:s0 + depth * NR] = 0xFF
    # the lists
    dmask = torch.from_numpy(mask).cuda()
    dpos = torch.zeros((ncw, NR), dtype=torch.uint8, device="cuda")
    dcnt = torch.zeros(ncw, dtype=torch.uint8, device="cuda")
    dover = torch.full((ncw,), FILL, dtype=torch.uint8, device="cuda")
    assert dpos.data_ptr() % 16 == 0
    h.erasures_from_mask_device(dmask.data_ptr(), size * depth, size, depth, nframes, dpos.data_ptr(), NR,
                                dcnt.data_ptr(), dover.data_ptr())
    # straight into the decode, on the same stream
    dd, dpar = torch.from_numpy(rd).cuda(), torch.from_numpy(clean_p).cuda()
    okc = torch.zeros((2, ncw), dtype=torch.uint8, device="cuda")
    h.decode_interleaved_device(dd.data_ptr(), size * depth, dpar.data_ptr(), NR * depth, size, depth, nframes,
                                okc[0].data_ptr(), okc[1].data_ptr(), d_positions=dpos.data_ptr(),
                                positions_stride=NR, d_counts=dcnt.data_ptr())
    torch.cuda.synchronize()
    pos, cnt = dpos.cpu().numpy(), dcnt.cpu().numpy()
    wpos, wcnt, wover = expect_lists(frames_to_rows(mask, depth), NR)
    assert (pos == wpos).all() and (cnt == wcnt).all() and (cnt == NR).all()
    assert not wover.any() and not dover.cpu().numpy().any()
    ook, ocor, od, op = expect_decode(o, rd, clean_p, depth, pos, cnt)
    assert ook.all() and (od == clean_d).all() and (op == clean_p).all(), "the oracle does not restore the frames"
    assert (okc.cpu().numpy()[0] == 1).all() and (okc.cpu().numpy()[1] == ocor).all()
    assert (dd.cpu().numpy() == clean_d).all() and (dpar.cpu().numpy() == clean_p).all()
