"""The route table of the RS / BCH batch decode.

Which kernels a decode call launches is decided on the host, from the code,
the batch size, the mode of the call (errors only, external syndromes, u8
erasure slots and how their rows are aligned) and the POPORON_AMD_*
switches read at poporon_create.  The launch counts that timing_read returns
per timing id are therefore a signature of the route taken.  Every case here
runs one decode with timing on, checks that the rows come back clean with ok
set, and compares the tuple of launch counts over KERNEL_NAMES with the one
recorded in tests/golden/decode_routes.json (recorded by this module's
__main__ block at the commit the file names, before the dispatch was
reshaped; never from the code under test).

Axes: four codes x counts 1, 2, 16383, 16384 (the two sides of every
threshold in the dispatch) x eleven environments x six modes; BCH has mode a
only (its entry points refuse erasures and external syndromes).

The general wave and lane kernels (rsgw_decode / rsg_decode) are charged to
one timing id, so the signature cannot tell them apart: which of the two runs
is covered by the result tests under POPORON_AMD_GENERIC
(tests/test_gpu_generic_wave.py).
"""
import json
import os

import numpy as np
import pytest

import libpoporon_amd as P

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_routes.json")
ENV_VARS = ("POPORON_AMD_DECODE_PATH", "POPORON_AMD_DECODE_TAIL", "POPORON_AMD_GENERIC", "POPORON_AMD_FORCE_VERIFY")
CODES = {"rs255_223": (8, 0x11D, 1, 1, 32), "rs255_239": (8, 0x11D, 1, 1, 16), "rs15_11": (4, 0x13, 1, 1, 4),
         "bch_default": None}
COUNTS = (1, 2, 16383, 16384)
ENVS = {
    "default": {},
    "path_split": {"POPORON_AMD_DECODE_PATH": "split"},
    "path_single": {"POPORON_AMD_DECODE_PATH": "single"},
    "path_wave": {"POPORON_AMD_DECODE_PATH": "wave"},
    "tail_split": {"POPORON_AMD_DECODE_TAIL": "split"},
    "tail_fused": {"POPORON_AMD_DECODE_TAIL": "fused"},
    "path_split_tail_split": {"POPORON_AMD_DECODE_PATH": "split", "POPORON_AMD_DECODE_TAIL": "split"},
    "path_split_tail_fused": {"POPORON_AMD_DECODE_PATH": "split", "POPORON_AMD_DECODE_TAIL": "fused"},
    "generic_lane": {"POPORON_AMD_GENERIC": "lane"},
    "generic_wave": {"POPORON_AMD_GENERIC": "wave"},
    "force_verify": {"POPORON_AMD_FORCE_VERIFY": "1"},
}
# a: errors only; b: external syndromes; c..f: u8 erasure slots in rows that are 16-byte aligned (c), a multiple
# of 4 but not of 16 bytes apart (d), num_roots + 1 bytes apart (e), 16-byte rows from a base one byte off (f)
MODES = "abcdef"
NMAX = max(COUNTS)
DIRTY = (0, 1, 7, 8191, 16382, 16383)  # rows that carry errors / erasures (those below the count)
KERNEL_IDS = sorted(P.KERNEL_NAMES)


def _make(code):
    if CODES[code] is None:
        return P.Bch.default()
    return P.Poporon(*CODES[code])


def _slot_stride(mode, nr):
    if mode == "d":
        s = (nr + 3) // 4 * 4
        return s if s % 16 else s + 4
    if mode == "e":
        return nr + 1
    return (nr + 15) // 16 * 16


_inputs = {}


def _code_inputs(torch, code):
    """Clean rows, rows with errors (mode a / b, with their own log-form
    syndromes), rows with erasures and their slots: made once per code, on
    the device, and never written."""
    if code in _inputs:
        return _inputs[code]
    h = _make(code)
    rng = np.random.default_rng(len(code) * 1000 + 17)
    bch = CODES[code] is None
    if bch:
        size, nr, q = h.info_size, h.parity_size, 1 << 5  # BCH(15, 5): five message bits in one byte
    else:
        m, _, _, _, nr = CODES[code]
        size, q = (1 << m) - 1 - nr, 1 << m
    data = rng.integers(0, q, (NMAX, size), dtype=np.uint8)
    clean = np.concatenate([data, h.encode_batch(data)], 1)
    w = size + nr
    err = clean.copy()
    era = clean.copy()
    slots = np.zeros((NMAX, nr), np.uint8)
    cnt = np.zeros(NMAX, np.uint8)
    for c in DIRTY:
        if bch:  # one flipped message bit (the decode writes data bytes only)
            err[c, size - 1] ^= 1
            continue
        pos = rng.permutation(w)[: nr // 2]
        err[c, pos] ^= rng.integers(1, q, pos.size, dtype=np.uint8)
        # erasures alone, in ascending order: the reference hands magnitude n to slot n (quirk Q1), so only
        # then do the bytes come back clean
        pos = np.sort(rng.permutation(size)[: nr // 2])
        era[c, pos] ^= rng.integers(1, q, pos.size, dtype=np.uint8)
        slots[c, : pos.size] = pos
        cnt[c] = pos.size
    inp = {"size": size, "nr": nr, "clean": torch.from_numpy(clean).cuda(), "err": torch.from_numpy(err).cuda(),
           "era": torch.from_numpy(era).cuda(), "slots": slots, "cnt": torch.from_numpy(cnt).cuda()}
    if not bch:
        syn = torch.zeros((NMAX, nr), dtype=torch.int16, device="cuda")
        b = inp["err"].data_ptr()
        h.syndrome_batch_device(b, w, b + size, w, size, NMAX, syn.data_ptr(), nr, None,
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        inp["syn"] = syn
        for mode in "cdef":
            st = _slot_stride(mode, nr)
            rows = np.zeros((NMAX, st), np.uint8)
            rows[:, :nr] = slots
            off = 1 if mode == "f" else 0
            inp["slots_" + mode] = torch.from_numpy(np.concatenate([np.zeros(off, np.uint8), rows.reshape(-1)])).cuda()
    h.close()
    _inputs[code] = inp
    return inp


def run_routes(torch, code):
    """One handle under the environment in force: {"count|mode": launch counts}
    of every count and mode, after checking each decode's result."""
    inp = _code_inputs(torch, code)
    h = _make(code)
    assert h.supported or CODES[code] is None
    size, nr = inp["size"], inp["nr"]
    w = size + nr
    s = torch.cuda.current_stream().cuda_stream
    routes = {}
    for count in COUNTS:
        for mode in (MODES if CODES[code] is not None else "a"):
            rows = inp["era" if mode in "cdef" else "err"][:count].clone()
            ok = torch.zeros(count, dtype=torch.uint8, device="cuda")
            cor = torch.zeros(count, dtype=torch.uint8, device="cuda")
            b = rows.data_ptr()
            h.timing(True)
            if mode == "a":
                h.decode_batch_device(b, w, b + size, w, size, count, ok.data_ptr(), cor.data_ptr(), stream=s)
            elif mode == "b":
                h.decode_batch_syndrome_device(b, w, b + size, w, size, count, inp["syn"].data_ptr(), nr,
                                               ok.data_ptr(), cor.data_ptr(), s)
            else:
                sl = inp["slots_" + mode]
                h.decode_batch_device(b, w, b + size, w, size, count, ok.data_ptr(), cor.data_ptr(),
                                      d_positions=sl.data_ptr() + (1 if mode == "f" else 0),
                                      positions_stride=_slot_stride(mode, nr), d_counts=inp["cnt"].data_ptr(),
                                      stream=s)
            torch.cuda.synchronize()
            launches = [int(h.timing_read(k)[1]) for k in KERNEL_IDS]
            h.timing(False)
            assert int(ok.sum()) == count, (code, count, mode, "ok")
            assert torch.equal(rows, inp["clean"][:count]), (code, count, mode, "rows")
            routes[f"{count}|{mode}"] = launches
    h.close()
    return routes


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("code", list(CODES))
def test_decode_route_table(monkeypatch, recorded, code, env):
    import torch
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    assert recorded["kernel_ids"] == KERNEL_IDS
    for v in ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    got = run_routes(torch, code)
    want = recorded["routes"][code][env]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, f"{code} under {env}: (launched, recorded) per count|mode over ids {KERNEL_IDS}: {wrong}"


if __name__ == "__main__":
    # recorder, run from the repository root at the commit whose routes are the record:
    #   PYTHONPATH=. python tests/test_gpu_decode_routes.py COMMIT [OUT]
    import sys

    import torch

    table = {}
    for code_ in CODES:
        table[code_] = {}
        for env_, sets in ENVS.items():
            for v_ in ENV_VARS:
                os.environ.pop(v_, None)
            os.environ.update(sets)
            table[code_][env_] = run_routes(torch, code_)
    out = {"recorded_at_commit": sys.argv[1], "kernel_ids": KERNEL_IDS,
           "kernel_names": [P.KERNEL_NAMES[k] for k in KERNEL_IDS], "routes": table}
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        f.write("{\n")
        f.write(f' "recorded_at_commit": {json.dumps(out["recorded_at_commit"])},\n')
        f.write(f' "kernel_ids": {json.dumps(out["kernel_ids"])},\n')
        f.write(f' "kernel_names": {json.dumps(out["kernel_names"])},\n')
        f.write(' "routes": {\n')
        for i, (code_, envs) in enumerate(table.items()):
            f.write(f'  {json.dumps(code_)}: {{\n')
            for j, (env_, r) in enumerate(envs.items()):
                f.write(f'   {json.dumps(env_)}: {json.dumps(r)}{"," if j + 1 < len(envs) else ""}\n')
            f.write(f'  }}{"," if i + 1 < len(table) else ""}\n')
        f.write(" }\n}\n")
