#!/usr/bin/env python3
"""Cost of the plane layout (diagnostic), resident on the device, all legs from one process and
alternating inside every step:

    workload "rs223":   2^20 codewords of RS(255,223) as 255 planes, 16 errors each (a scrub)
    workload "storage": the (14,10) shape (8-bit, 0x11D, 4 roots) at 2^24 bytes per plane, two lost
                        planes, one of them parity (a rebuild)

    plane_encode, plane_decode, plane_check     the plane calls (strided form; --offset: unaligned planes); the decode
                                                with d_dirty, plane_decode_plain without it
    row_encode, row_decode, row_check           the row calls on ready rows
    memcpy_d2d                                  hipMemcpyAsync device-to-device of the same W*count bytes
    torch_encode, torch_decode, torch_check     the caller-side route the calls replace: .t().contiguous()
                                                in, the row call, and the transpose back
    ilv8_encode, ilv8_decode, ilv8_check        rs223 only: the interleaved calls at depth 8 on the same
                                                codewords

    python tools/plane_bench.py [--steps 10] [--warmup 3] [--workloads rs223,storage] [--offset 0..15]
                                [--append FILE]

Per workload one JSON line: event time of every leg (median, min, max over the steps, us), the layout
kernels' own time from the library's events (poporon_amd_timing, ids 22 and 23, summed over the chunks
of a call) in a second pass, achieved bytes per second of the layout kernels and the copy, and whether
each plane call beat its torch route in every alternated pair.  Every decode is checked against the
clean stripe inside the loop."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import libpoporon_amd as P  # noqa: E402

WORKLOADS = {"rs223": dict(params=(8, 0x11D, 1, 1, 32), size=223, count=1 << 20, nerr=16, lost=[]),
             "storage": dict(params=(8, 0x11D, 1, 1, 4), size=10, count=1 << 24, nerr=0, lost=[3, 12])}


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
    return {"median": round(s[len(s) // 2], 1), "min": round(s[0], 1), "max": round(s[-1], 1)}


def timed(fn):
    """event time of fn's work on the current stream, us"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def run(name, steps, warmup, hip, count=None, offset=0):
    wl = WORKLOADS[name]
    size, nerr, lost = wl["size"], wl["nerr"], wl["lost"]
    n = count or wl["count"]
    nr = wl["params"][4]
    W = size + nr
    dev = torch.device("cuda", 0)
    h = P.Poporon(*wl["params"], device=0)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(0x5EED)
    clean = torch.randint(0, 256, (n, W), dtype=torch.uint8, device=dev, generator=g)  # rows
    h.encode_batch_device(clean.data_ptr(), W, clean.data_ptr() + size, W, size, n, s)
    bad = clean.clone()
    if nerr:
        pos = torch.rand((n, W), device=dev, generator=g).topk(nerr, dim=1).indices
        bad.scatter_(1, pos, bad.gather(1, pos) ^ torch.randint(1, 256, (n, nerr), dtype=torch.uint8, device=dev,
                                                                generator=g))
        del pos
    if lost:
        bad[:, lost] = 0x5A  # what a lost shard holds does not matter: zeroed before the row call, never read here
    clean_p, bad_p = clean.t().contiguous(), bad.t().contiguous()  # planes [W, n], n a multiple of 16: aligned
    zeroed = bad.clone()
    zeroed[:, lost] = 0
    # per-codeword erasure lists for the row routes, as the plane call builds them
    ls = (nr + 15) & ~15
    epos = torch.zeros((n, ls), dtype=torch.uint8, device=dev)
    ecnt = torch.full((n,), len(lost), dtype=torch.uint8, device=dev)
    if lost:
        epos[:, :len(lost)] = torch.tensor(lost, dtype=torch.uint8, device=dev)
    era = dict(d_positions=epos.data_ptr(), positions_stride=ls, d_counts=ecnt.data_ptr()) if lost else {}
    h.reserve_planes(n)
    h.reserve_interleaved(n)
    # the plane calls' stripe: planes n + 16 bytes apart, the first `offset` bytes past a 16-byte boundary
    pbuf = torch.empty((W, n + 16), dtype=torch.uint8, device=dev)
    work_p, ps = pbuf[:, offset:offset + n], n + 16
    rrows = zeroed.clone()     # ready rows
    tplanes = bad_p.clone()    # the torch route's stripe
    trows = torch.empty_like(bad)
    cp = torch.empty_like(bad)
    ok = torch.zeros((6, n), dtype=torch.uint8, device=dev)
    wp, qp, tp = pbuf.data_ptr() + offset, rrows.data_ptr(), trows.data_ptr()
    depth = 8
    fr = torch.empty((n // depth, W * depth), dtype=torch.uint8, device=dev) if name == "rs223" else None

    def torch_decode():
        if lost:
            tplanes[lost] = 0
        trows.copy_(tplanes.t())
        h.decode_batch_device(tp, W, tp + size, W, size, n, ok[1].data_ptr(), stream=s, **era)
        tplanes.copy_(trows.t())

    def torch_encode():
        trows[:, :size].copy_(tplanes[:size].t())
        h.encode_batch_device(tp, W, tp + size, W, size, n, s)
        tplanes[size:].copy_(trows[:, size:].t())

    def torch_check():
        trows.copy_(tplanes.t())
        h.check_batch_device(tp, W, tp + size, W, size, n, ok[4].data_ptr(), s)

    legs = {
        "memcpy_d2d": lambda: hip.hipMemcpyAsync(cp.data_ptr(), qp, n * W, 3, s),
        "plane_decode": lambda: h.decode_planes_strided_device(wp, ps, wp + size * ps, ps, size, n, ok[0].data_ptr(),
                                                               lost=lost, d_dirty=ok[5].data_ptr(), stream=s),
        "plane_decode_plain": lambda: h.decode_planes_strided_device(wp, ps, wp + size * ps, ps, size, n,
                                                                     ok[0].data_ptr(), lost=lost, stream=s),
        "torch_decode": torch_decode,
        "row_decode": lambda: h.decode_batch_device(qp, W, qp + size, W, size, n, ok[2].data_ptr(), stream=s, **era),
        "plane_encode": lambda: h.encode_planes_strided_device(wp, ps, wp + size * ps, ps, size, n, s),
        "torch_encode": torch_encode,
        "row_encode": lambda: h.encode_batch_device(qp, W, qp + size, W, size, n, s),
        "plane_check": lambda: h.check_planes_strided_device(wp, ps, wp + size * ps, ps, size, n, ok[3].data_ptr(), s),
        "torch_check": torch_check,
        "row_check": lambda: h.check_batch_device(qp, W, qp + size, W, size, n, ok[3].data_ptr(), s),
    }
    if fr is not None:
        fp = fr.data_ptr()
        fs = W * depth
        legs.update({
            "ilv8_decode": lambda: h.decode_interleaved_device(fp, fs, fp + size * depth, fs, size, depth, n // depth,
                                                               ok[2].data_ptr(), stream=s),
            "ilv8_encode": lambda: h.encode_interleaved_device(fp, fs, fp + size * depth, fs, size, depth, n // depth,
                                                               s),
            "ilv8_check": lambda: h.check_interleaved_device(fp, fs, fp + size * depth, fs, size, depth, n // depth,
                                                             ok[3].data_ptr(), s),
        })
        bad_f = bad.view(n // depth, depth, W).transpose(1, 2).contiguous().view(n // depth, W * depth)
    wall = {k: [] for k in legs}
    kern = {22: {}, 23: {}}
    for timing in (False, True):
        h.timing(timing)
        for step in range(steps if timing else warmup + steps):
            for leg, fn in legs.items():
                # every leg starts from the received data, an encode from the clean message and no parity
                enc = leg.endswith("encode")
                if leg.startswith("plane"):
                    work_p.copy_(clean_p if enc else bad_p)
                    if enc:
                        work_p[size:].zero_()
                elif leg.startswith("torch"):
                    tplanes.copy_(clean_p if enc else bad_p)
                    if enc:
                        tplanes[size:].zero_()
                elif leg.startswith("row") or leg == "memcpy_d2d":
                    rrows.copy_(clean if enc else zeroed)
                else:
                    fr.copy_(bad_f)
                t = timed(fn)
                if not timing and step >= warmup:
                    wall[leg].append(t)
                if leg in ("plane_decode", "plane_decode_plain"):
                    assert torch.equal(work_p, clean_p) and int(ok[0].sum()) == n and not int(ok[5].sum())
                elif leg == "torch_decode":
                    assert torch.equal(tplanes, clean_p) and int(ok[1].sum()) == n
                elif leg == "row_decode":
                    assert torch.equal(rrows, clean) and int(ok[2].sum()) == n
                elif leg == "plane_encode":
                    assert torch.equal(work_p[size:], clean_p[size:])
                elif leg == "torch_encode":
                    assert torch.equal(tplanes[size:], clean_p[size:])
                elif leg == "ilv8_decode":
                    assert int(ok[2].sum()) == n
                if timing:
                    for k in kern:
                        ms, cnt = h.timing_read(k)
                        if leg.startswith("plane") and cnt:
                            kern[k].setdefault(leg, []).append(ms * 1e3)
                    h.timing(True)
    h.timing(False)
    med = {k: stats(v) for k, v in wall.items()}
    line = {"workload": name, "plane_offset": offset, "codewords": n, "row_bytes": W, "errors": nerr, "lost": lost,
            "tile": P.plane_tile(W), "steps": steps, "event_us": med,
            "kernel_us": {f"{P.PLANE_KERNEL_NAMES[k]} in {leg}": stats(v) for k, d in kern.items()
                          for leg, v in d.items()},
            "copy_TBps": round(2 * n * W / (med["memcpy_d2d"]["median"] * 1e-6) / 1e12, 3),
            "plane_wins_every_pair": {op: all(a < b for a, b in zip(wall[f"plane_{op}"],
                                                                    wall[f"torch_{op.split('_')[0]}"]))
                                      for op in ("encode", "decode", "decode_plain", "check")}}
    h.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="rs223,storage")
    ap.add_argument("--count", type=int, default=0, help="codewords, instead of the workload's own (a multiple of 16)")
    ap.add_argument("--offset", type=int, default=0, help="bytes of every plane past a 16-byte boundary (0..15)")
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "plane_bench needs a GPU"
    hip = hip_runtime()
    for name in a.workloads.split(","):
        line = run(name, a.steps, a.warmup, hip, a.count, a.offset)
        print(json.dumps(line), flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
