#!/usr/bin/env python3
"""Cost of the decode report and of the mask-to-erasure-list call (diagnostic):
bench.py's workload -- 2^20 codewords of RS(255,223) as wire rows, 16 errors
each, resident on the device -- through poporon_decode_batch_report_device,
next to the plain poporon_decode_batch_device, to the interleaved report at
depth 4, to poporon_amd_erasures_from_mask_device at depths 1 and 8 with 32
flags per codeword, and to hipMemcpyAsync device-to-device copies of the
block's and of the mask's bytes: the yardsticks.  One process, the legs
alternating inside every step.

    python tools/report_bench.py [--steps 10] [--warmup 3] [--batch 1048576] [--size 223] [--out FILE]
                                 [--no-verify]

One JSON line (appended to --out): wall time of call + synchronise per leg
(median, min, max over the steps, us); per-kernel time per call from the
library's events in a second pass (ids 17 = snapshot, 18 = rs_report_k, 19 =
rs_mask_lists_k, and the codec ids); and the ratios DESIGN.md section 13 states:
the snapshot and rs_report_k against the block copy (the snapshot moves the
copy's bytes, rs_report_k reads them), rs_mask_lists_k against the copy of
the mask's bytes, the report call against the row decode."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import devdata  # noqa: E402
import libpoporon_amd as P  # noqa: E402

NR, NERR, ILV_DEPTH, MASK_DEPTH, FLAGS = 32, 16, 4, 8, 32


def hip_runtime():
    """the HIP runtime this process already runs on (torch's), not a second copy"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            lib.hipMemcpyAsync.restype = C.c_int
            return lib
    raise RuntimeError("no HIP runtime loaded")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2] * 1e6, 1), "min": round(s[0] * 1e6, 1), "max": round(s[-1] * 1e6, 1)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_us(h):
    names = {**P.KERNEL_NAMES, **P.ILV_KERNEL_NAMES, **P.REPORT_KERNEL_NAMES}
    out = {}
    for k in names:
        ms, n = h.timing_read(k)
        if n:
            out[str(k)] = {"name": names[k], "us_per_call": round(ms * 1e3, 1), "launches_per_call": n}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--size", type=int, default=223)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-verify", action="store_true",
                    help="do not check the results (experimental builds through POPORON_AMD_LIB)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip = hip_runtime()
    K, W = a.size, a.size + NR
    n = a.batch // (ILV_DEPTH * MASK_DEPTH) * (ILV_DEPTH * MASK_DEPTH)
    h = P.Poporon.default(device=0)
    s = torch.cuda.current_stream().cuda_stream
    clean = torch.zeros((n, W), dtype=torch.uint8, device=dev)
    clean[:, :K] = devdata.synth_bytes(bench.SEED, 0, n, K, dev)
    h.encode_batch_device(clean.data_ptr(), W, clean.data_ptr() + K, W, K, n, s)
    pos, mag = devdata.synth_errors(bench.SEED + 1, 0, n, NERR, W, dev)
    bad = clean.clone()
    devdata.channel(pos, mag, NERR, bad.data_ptr(), W, n, s)
    torch.cuda.synchronize()
    frames = n // ILV_DEPTH
    to_frames = lambda rows, d: rows.view(n // d, d, rows.shape[1]).transpose(1, 2).contiguous()  # noqa: E731
    f_clean, f_bad = to_frames(clean, ILV_DEPTH), to_frames(bad, ILV_DEPTH)
    # flag planes: FLAGS distinct symbols per codeword
    flags = min(FLAGS, K)
    mrows = torch.zeros((n, K), dtype=torch.uint8, device=dev)
    hop = 7  # coprime to 223 and to 96: (c + 7 k) mod K are distinct symbols for k < K
    idx = (torch.arange(n, device=dev)[:, None] + hop * torch.arange(flags, device=dev)[None, :]) % K
    mrows.scatter_(1, idx, 1)
    m1, m8 = mrows, to_frames(mrows, MASK_DEPTH)
    h.reserve_report(n)
    h.reserve_interleaved(n)
    rw, pw, fw = bad.clone(), bad.clone(), f_bad.clone()
    cp, cpm = torch.empty_like(rw), torch.empty_like(m1)
    ok = torch.zeros((3, n), dtype=torch.uint8, device=dev)
    num = torch.zeros((2, n), dtype=torch.uint8, device=dev)
    lst = torch.zeros((4, n, NR), dtype=torch.uint8, device=dev)
    mpos = torch.zeros((n, NR), dtype=torch.uint8, device=dev)
    mcnt = torch.zeros((2, n), dtype=torch.uint8, device=dev)
    rp, pp, fp, fb = rw.data_ptr(), pw.data_ptr(), fw.data_ptr(), W * ILV_DEPTH
    legs = {
        "row_decode": lambda: h.decode_batch_device(rp, W, rp + K, W, K, n, ok[0].data_ptr(), stream=s),
        "report_decode": lambda: h.decode_batch_report_device(pp, W, pp + K, W, K, n, ok[1].data_ptr(),
                                                              num[0].data_ptr(), lst[0].data_ptr(), lst[1].data_ptr(),
                                                              NR, stream=s),
        "memcpy_block": lambda: hip.hipMemcpyAsync(cp.data_ptr(), rp, n * W, 3, s),
        "ilv_report_d4": lambda: h.decode_interleaved_report_device(fp, fb, fp + K * ILV_DEPTH, fb, K, ILV_DEPTH,
                                                                    frames, ok[2].data_ptr(), num[1].data_ptr(),
                                                                    lst[2].data_ptr(), lst[3].data_ptr(), NR,
                                                                    stream=s),
        "mask_d1": lambda: h.erasures_from_mask_device(m1.data_ptr(), K, K, 1, n, mpos.data_ptr(), NR,
                                                       mcnt[0].data_ptr(), mcnt[1].data_ptr(), stream=s),
        "mask_d8": lambda: h.erasures_from_mask_device(m8.data_ptr(), K * MASK_DEPTH, K, MASK_DEPTH, n // MASK_DEPTH,
                                                       mpos.data_ptr(), NR, mcnt[0].data_ptr(), mcnt[1].data_ptr(),
                                                       stream=s),
        "memcpy_mask": lambda: hip.hipMemcpyAsync(cpm.data_ptr(), m1.data_ptr(), n * K, 3, s),
    }
    wall = {k: [] for k in legs}
    kern = {}
    for timing in (False, True):
        for step in range(a.steps if timing else a.warmup + a.steps):
            for name, fn in legs.items():
                if name == "row_decode":
                    rw.copy_(bad)
                elif name == "report_decode":
                    pw.copy_(bad)
                elif name == "ilv_report_d4":
                    fw.copy_(f_bad)
                if timing:
                    h.timing(True)  # this call's kernels; the totals start over
                t = timed(fn)
                if not timing and step >= a.warmup:
                    wall[name].append(t)
                if timing and not name.startswith("memcpy"):
                    kern.setdefault(name, []).append(kernel_us(h))
                if a.no_verify:
                    continue
                if name == "row_decode":
                    assert torch.equal(rw, clean) and int(ok[0].sum()) == n
                elif name == "report_decode":
                    assert torch.equal(pw, clean) and int(ok[1].sum()) == n and bool((num[0] == NERR).all())
                elif name == "ilv_report_d4":
                    assert torch.equal(fw, f_clean) and int(ok[2].sum()) == n and bool((num[1] == NERR).all())
                    assert torch.equal(lst[0], lst[2]) and torch.equal(lst[1], lst[3])
                elif name.startswith("mask"):
                    assert bool((mcnt[0] == flags).all()) and not bool(mcnt[1].any())
    h.timing(False)
    kern = {leg: {k: dict(calls[0][k], us_per_call=sorted(c[k]["us_per_call"] for c in calls)[len(calls) // 2])
                  for k in calls[0]} for leg, calls in kern.items()}  # median over the steps
    line = {"workload": f"RS({W},{K}) of RS(255,223), {n} wire rows, {NERR} errors each; masks: {flags} flags per "
                        f"codeword", "steps": a.steps, "warmup": a.warmup,
            "wall_us": {k: stats(v) for k, v in wall.items()}, "kernels": kern}
    copy_us, mcopy_us = line["wall_us"]["memcpy_block"]["median"], line["wall_us"]["memcpy_mask"]["median"]
    rep = kern["report_decode"]
    line["rates"] = {
        "memcpy_block_TBps": round(2 * n * W / copy_us / 1e6, 3),
        "memcpy_mask_TBps": round(2 * n * K / mcopy_us / 1e6, 3),
        "snapshot_over_copy": round(rep["17"]["us_per_call"] / copy_us, 2),
        "report_kernel_over_copy": round(rep["18"]["us_per_call"] / copy_us, 2),
        "ilv_report_kernel_over_copy": round(kern["ilv_report_d4"]["18"]["us_per_call"] / copy_us, 2),
        "mask_d1_kernel_over_mask_copy": round(kern["mask_d1"]["19"]["us_per_call"] / mcopy_us, 2),
        "mask_d8_kernel_over_mask_copy": round(kern["mask_d8"]["19"]["us_per_call"] / mcopy_us, 2),
        "report_call_over_row_decode": round(line["wall_us"]["report_decode"]["median"]
                                             / line["wall_us"]["row_decode"]["median"], 2),
        "report_call_minus_decode_in_copies": round((line["wall_us"]["report_decode"]["median"]
                                                     - line["wall_us"]["row_decode"]["median"]) / copy_us, 2),
    }
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
