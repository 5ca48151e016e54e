#!/usr/bin/env python3
"""LDPC throughput: device-resident batch encode and hard decode on the GPU
against the reference on 16 CPU threads.  Reported, not gated.

Two codes, rows with 4 flipped bits each, max_iterations 20:
  A      block 32,   rate 1/2, RANDOM, weight 3   (messages in LDS)
  k1024  block 1024, rate 1/2, RANDOM, weight 3   (messages in the global workspace)

GPU: 2^16 rows resident in device memory; per step the received rows are
restored (untimed), then one poporon_ldpc_decode_batch_device call.  Kernel time
comes from the library's timing ids (12 encode, 13 decode: HIP events around the
launch), wall time from a host clock around call + synchronise.  Encoded parity,
ok flags and iteration counts are compared with the reference's on its slice.

CPU: oracle/_ref/libpoporon_ref_avx2.so through its public API, 16 processes
(one handle each, no GIL between them), each on its own slice of the same rows:
poporon_encode over the slice, then poporon_decode over the flipped slice, called
through ctypes on raw addresses (about a microsecond of call overhead per row).  The
rate is rows of all workers over the slowest worker's time.  It runs first, before
the GPU is opened.

  python tools/ldpc_bench.py [--rows 65536] [--steps 10] [--threads 16]
prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ldpc_ref as R  # noqa: E402

AVX2_SO = os.path.join(ROOT, "oracle", "_ref", "libpoporon_ref_avx2.so")
CODES = {
    "A": (dict(R.CODES["A"]), 4096),
    "k1024": (dict(block=1024, rate=1, matrix=R.RANDOM, weight=3, outer=False, inner=False, lifting=0, seed=0), 256),
}
NFLIP = 4


def rows_of(name, n):
    code = CODES[name][0]
    rng = np.random.default_rng([len(name), code["block"]])
    ib, _, pb = R.sizes(code["block"], code["rate"])
    msgs = rng.integers(0, 256, (n, ib), dtype=np.uint8)
    flips = rng.integers(0, 8 * (ib + pb), (n, NFLIP))
    while True:  # NFLIP distinct bits in every row
        srt = np.sort(flips, axis=1)
        dup = (srt[:, 1:] == srt[:, :-1]).any(axis=1)
        if not dup.any():
            break
        flips[dup] = rng.integers(0, 8 * (ib + pb), (int(dup.sum()), NFLIP))
    return msgs, flips


def flip(data, parity, flips):
    row = np.concatenate([data, parity], axis=1)
    r = np.arange(len(row))[:, None]
    np.bitwise_xor.at(row, (r, flips // 8), (0x80 >> (flips % 8)).astype(np.uint8))
    return np.ascontiguousarray(row[:, :data.shape[1]]), np.ascontiguousarray(row[:, data.shape[1]:])


def cpu_worker(args):
    name, lo, hi, total = args
    msgs, flips = rows_of(name, total)
    msgs, flips = msgs[lo:hi], flips[lo:hi]
    ref = R.RefLdpc(CODES[name][0], so=AVX2_SO)
    n, ib, pb = hi - lo, ref.info_bytes, ref.parity_bytes
    # raw addresses into contiguous arrays: a ctypes call costs about a microsecond per row
    enc, dec, used, hd = ref.lib.poporon_encode, ref.lib.poporon_decode, ref.lib.poporon_get_iterations_used, ref.h
    msgs = np.ascontiguousarray(msgs)
    par = np.zeros((n, pb), np.uint8)
    dp, pp = msgs.ctypes.data, par.ctypes.data
    t0 = time.perf_counter()
    for i in range(n):
        enc(hd, dp + i * ib, ib, pp + i * pb)
    t_enc = time.perf_counter() - t0
    din, pin = flip(msgs, par, flips)
    ok, it = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    dp, pp = din.ctypes.data, pin.ctypes.data
    cnt = C.c_size_t(0)
    pc = C.byref(cnt)
    okl, itl = [0] * n, [0] * n
    t0 = time.perf_counter()
    for i in range(n):
        okl[i] = dec(hd, dp + i * ib, ib, pp + i * pb, pc)
        itl[i] = used(hd)
    t_dec = time.perf_counter() - t0
    ok[:], it[:] = okl, itl
    return lo, hi, t_enc, t_dec, par, ok, it


def cpu_reference(name, total, threads):
    per = min(CODES[name][1], total // threads)
    jobs = [(name, t * per, (t + 1) * per, total) for t in range(threads)]
    with mp.get_context("fork").Pool(threads) as pool:
        res = pool.map(cpu_worker, jobs)
    n = per * threads
    return dict(rows=n, threads=threads, encode_rows_per_s=n / max(r[2] for r in res),
                decode_rows_per_s=n / max(r[3] for r in res)), res


def gpu(name, total, steps, res):
    import torch

    import libpoporon_amd as P
    code = CODES[name][0]
    h = P.Ldpc(code["block"], code["rate"], code["matrix"], code["weight"], False, code["outer"], code["inner"], 0,
               code["lifting"], R.MAX_ITER, None, 0, code["seed"], device=0)
    ib, pb = h.info_bytes, h.parity_bytes
    w = ib + pb
    msgs, flips = rows_of(name, total)
    s = torch.cuda.current_stream().cuda_stream
    rows = torch.zeros((total, w), dtype=torch.uint8, device="cuda")
    rows[:, :ib] = torch.from_numpy(msgs).cuda()
    ok = torch.zeros(total, dtype=torch.uint8, device="cuda")
    it = torch.zeros(total, dtype=torch.int32, device="cuda")
    h.reserve(total)

    def run(kernel, fn, restore):
        wall = []
        for step in range(steps + 1):  # the first step warms up
            restore()
            torch.cuda.synchronize()
            if step == 1:
                h.timing(True)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        ms, n = h.timing_read(kernel)
        h.timing(False)
        assert n == steps
        return dict(kernel_ms=ms / n, wall_ms=1e3 * float(np.median(wall[1:])), rows_per_s_kernel=total * n / (ms / 1e3),
                    rows_per_s_wall=total / float(np.median(wall[1:])))

    enc = run(P.KERNEL_LDPC_ENCODE, lambda: h.encode_batch_device(rows.data_ptr(), w, rows.data_ptr() + ib, w, total, s),
              lambda: None)
    host = rows.cpu().numpy()
    din, pin = flip(host[:, :ib], host[:, ib:], flips)
    rx = torch.from_numpy(np.concatenate([din, pin], axis=1)).cuda()
    dec = run(P.KERNEL_LDPC_DECODE,
              lambda: h.decode_batch_device(rows.data_ptr(), w, rows.data_ptr() + ib, w, total, ok.data_ptr(),
                                            it.data_ptr(), stream=s), lambda: rows.copy_(rx))
    gok, git = ok.cpu().numpy(), it.cpu().numpy().view(np.uint32)
    same = all((host[lo:hi, ib:] == par).all() and (gok[lo:hi] == o).all() and (git[lo:hi] == i).all()
               for lo, hi, _, _, par, o, i in res)
    return dict(rows=total, encode=enc, decode=dec, decode_ok=int(gok.sum()), mean_iterations=float(git.mean()),
                matches_reference=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--codes", default="A,k1024")
    ap.add_argument("--cpu-only", action="store_true", help="the reference's rates alone (no device needed)")
    a = ap.parse_args()
    if not os.path.exists(AVX2_SO):
        sys.exit("oracle/_ref/libpoporon_ref_avx2.so missing (oracle/Makefile builds it where the reference is)")
    names = a.codes.split(",")
    cpu = {n: cpu_reference(n, a.rows, a.threads) for n in names}  # before the GPU is opened
    if a.cpu_only:
        print(json.dumps(dict(tool="ldpc_bench", nflip=NFLIP, max_iterations=R.MAX_ITER,
                              **{n: dict(cpu=cpu[n][0]) for n in names})))
        return
    out = {}
    for n in names:
        g = gpu(n, a.rows, a.steps, cpu[n][1])
        c = cpu[n][0]
        out[n] = dict(gpu=g, cpu=c,
                      encode_speedup_kernel=g["encode"]["rows_per_s_kernel"] / c["encode_rows_per_s"],
                      decode_speedup_kernel=g["decode"]["rows_per_s_kernel"] / c["decode_rows_per_s"],
                      encode_speedup_wall=g["encode"]["rows_per_s_wall"] / c["encode_rows_per_s"],
                      decode_speedup_wall=g["decode"]["rows_per_s_wall"] / c["decode_rows_per_s"])
    print(json.dumps(dict(tool="ldpc_bench", nflip=NFLIP, max_iterations=R.MAX_ITER, **out)))


if __name__ == "__main__":
    main()
