"""The branches of rs_bm_k's iteration (csrc/rs_fast.hip) one by one: the
wave-uniform degree guards, the group of Lambda that lies past the wave's
bound when B is rewritten, the lengthen / update masks (uniform and mixed),
iterations with a zero discrepancy, the exits to the list past t and the
early exit of a clean wave -- on RS(255,223) (rs_bm_k<false>) and on
RS(255,239) (rs_bm_k<true>, 16 roots).

POPORON_AMD_DECODE_PATH=split sends these small batches to the split
kernels.  Counts 1, 63, 65 and 513: a lone lane (on RS(255,239); one
RS(255,223) codeword takes the single-call kernel whatever the override), a
ragged last wave, a wave plus one lane, and a ragged last workgroup.  The
inputs come from a fixed seed on the CPU; bytes, ok and the corrected count
are compared bit for bit with the oracle (oracle/rs_oracle.c, pinned to the compiled reference by
tests/test_oracle_golden.py), which restores every codeword with at most t
errors (test_oracle_restores_cases, no GPU)."""
import os

import numpy as np
import pytest

import libpoporon_amd as P

COUNTS = (1, 63, 65, 513)
CODES = {"rs223": (8, 0x11D, 1, 1, 32), "rs239": (8, 0x11D, 1, 1, 16)}
LANE_PERM = np.random.default_rng(0xB17).permutation(64)


def _cases(t):
    """name -> error count of codeword c (lane c % 64 of wave c // 64), t = 16 or 8"""
    lo, mid = (3, 8) if t == 16 else (2, 4)
    over = (t + 1, t + 2) if t == 16 else (t + 1, t + 1)  # 17 and 18 errors; 9 on the 16-root code

    def mixed(c):  # 0, 1, .., t in turn: some lanes leave the upper groups at zero
        return c % (t + 1) if t == 16 else c % 10

    def mixed_perm(c):
        return mixed((c & ~63) | LANE_PERM[c & 63])

    def zero_disc(c):  # few errors: late iterations without an update, beside lanes that update
        return np.choose(c % 4, [lo, mid, t, t - 5])

    def past_t(c):  # more than t errors beside correctable ones
        return np.choose(c % 8, [over[0], over[1], t, 5, over[0], 0, over[1], t - 7])

    def clean_wave(c):  # every second wave clean, between dirty ones
        return np.where((c // 64) % 2 == 1, 0, 1 + c % 7)

    return {
        "mixed": mixed,
        "mixed_perm": mixed_perm,
        "all_lengthen": lambda c: np.full_like(c, t),  # every lane lengthens in the same iterations
        "none_lengthen": lambda c: np.full_like(c, 1),  # no lane lengthens after the first
        "split_wave": lambda c: np.where((c & 63) < 32, t, 1),  # the mask mixed in almost every iteration
        "zero_disc": zero_disc,
        "past_t": past_t,
        "clean_wave": clean_wave,
    }


CASE_NAMES = tuple(_cases(16))


def _inputs(o, code, case, n):
    """clean codewords, the received ones and the error counts, from a fixed seed"""
    nr = CODES[code][4]
    k = 255 - nr
    rng = np.random.default_rng([0xB3, sorted(CODES).index(code), CASE_NAMES.index(case), n])
    data = rng.integers(0, 256, (n, k), dtype=np.uint8)
    clean = np.concatenate([data, o.encode_batch(data)], 1)
    ne = np.asarray(_cases(nr // 2)[case](np.arange(n)), dtype=np.int64)
    cw = clean.copy()
    for c in range(n):
        pos = rng.permutation(255)[:ne[c]]
        cw[c, pos] ^= rng.integers(1, 256, ne[c]).astype(np.uint8)
    return clean, cw, ne


@pytest.fixture(scope="module")
def oracles():
    from oracle import Oracle
    return {code: Oracle(*params) for code, params in CODES.items()}


@pytest.fixture(scope="module")
def handles():
    """handles that take the split kernels at every batch size (the route is read at creation)"""
    prev = os.environ.get("POPORON_AMD_DECODE_PATH")
    os.environ["POPORON_AMD_DECODE_PATH"] = "split"
    try:
        return {code: P.Poporon(*params) for code, params in CODES.items()}
    finally:
        if prev is None:
            del os.environ["POPORON_AMD_DECODE_PATH"]
        else:
            os.environ["POPORON_AMD_DECODE_PATH"] = prev


@pytest.mark.parametrize("code", sorted(CODES))
def test_oracle_restores_cases(oracles, code):
    """the reference side alone: every codeword with at most t errors comes
    back clean with its error count, every case and count"""
    o = oracles[code]
    nr = CODES[code][4]
    k, t = 255 - nr, nr // 2
    for case in CASE_NAMES:
        for n in COUNTS:
            clean, cw, ne = _inputs(o, code, case, n)
            ook, ocor, od, op = o.decode_batch(cw[:, :k], cw[:, k:])
            fit = ne <= t
            assert (ook[fit] == 1).all() and (ocor[fit] == ne[fit]).all(), (case, n)
            assert (od[fit] == clean[fit, :k]).all() and (op[fit] == clean[fit, k:]).all(), (case, n)
            if case == "past_t":  # past t the reference refuses or miscorrects, never restores
                assert not (np.concatenate([od, op], 1)[~fit] == clean[~fit]).all(1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("code", sorted(CODES))
def test_bm_paths_vs_oracle(oracles, handles, code, case, n):
    import torch
    o, h = oracles[code], handles[code]
    nr = CODES[code][4]
    k = 255 - nr
    clean, cw, ne = _inputs(o, code, case, n)
    ook, ocor, od, op = o.decode_batch(cw[:, :k], cw[:, k:])
    s = torch.cuda.current_stream().cuda_stream
    dev = torch.from_numpy(cw).cuda()
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    cor = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    b = dev.data_ptr()
    h.timing(True)
    h.decode_batch_device(b, 255, b + k, 255, k, n, ok.data_ptr(), cor.data_ptr(), stream=s)
    torch.cuda.synchronize()
    launches = h.timing_read(P.KERNEL_BM)[1]
    h.timing(False)
    # one RS(255,223) codeword is the single-call kernel's whatever the override (api.cpp decode_route):
    # that count checks the result alone, every other one must have run rs_bm_k
    if not (code == "rs223" and n == 1):
        assert launches == 1, "rs_bm_k did not run"
    got, gok, gcor = dev.cpu().numpy(), ok.cpu().numpy(), cor.cpu().numpy()
    assert (gok == ook).all(), np.nonzero(gok != ook)[0][:8]
    assert (gcor == ocor).all(), np.nonzero(gcor != ocor)[0][:8]
    bad = np.nonzero((got[:, :k] != od).any(1) | (got[:, k:] != op).any(1))[0]
    assert bad.size == 0, bad[:8]
