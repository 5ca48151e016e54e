#!/usr/bin/env python3
"""Cost of the convolutional-interleaver layout (diagnostic): 2^20 codewords of DVB (RS(204,188),
12 branches of cell 17, 8 errors each) and of ATSC (RS(207,187), 52 branches of cell 4, 10 errors
each), resident on the device, all legs from one process and alternating inside every step:

    interleave, deinterleave    the two layout calls (rs_conv_scatter_k, rs_conv_gather_k)
    encode_conv, decode_conv, check_conv
    row_encode, row_decode, row_check
                                the row calls on ready rows
    memcpy_d2d                  hipMemcpyAsync device-to-device of the same count*W bytes
    torch_decode, torch_encode  the caller-side equivalent the calls replace: a torch index gather
                                (scatter) over every byte with a precomputed int64 index tensor,
                                and the row call

    python tools/conv_bench.py [--steps 10] [--warmup 3] [--batch 1048576] [--append FILE]

Per standard one JSON line: event time of every leg (median, min, max over the steps, us); the
layout kernels' own time from the library's events (poporon_amd_timing, ids 20 and 21) in a second
pass; achieved bytes per second of the layout kernels and the copy (bytes read + bytes written
over the time); and whether decode_conv / encode_conv beat their torch equivalents in every
alternated pair.  Every decode is checked against the clean rows inside the loop."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import libpoporon_amd as P  # noqa: E402

STANDARDS = {"dvb": dict(params=(8, 0x11D, 0, 1, 16), size=188, branches=12, cell=17, nerr=8),
             "atsc": dict(params=(8, 0x11D, 0, 1, 20), size=187, branches=52, cell=4, nerr=10)}


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


def run(name, n, steps, warmup, hip):
    st = STANDARDS[name]
    size, I, M, nerr = st["size"], st["branches"], st["cell"], st["nerr"]
    nr = st["params"][4]
    W, phase = size + nr, 0
    dev = torch.device("cuda", 0)
    h = P.Poporon(*st["params"], device=0)
    s = torch.cuda.current_stream().cuda_stream
    span = P.conv_span(W, n, I, M)
    g = torch.Generator(device=dev).manual_seed(0x5EED)
    clean = torch.randint(0, 256, (n, W), dtype=torch.uint8, device=dev, generator=g)
    h.encode_batch_device(clean.data_ptr(), W, clean.data_ptr() + size, W, size, n, s)
    pos = torch.rand((n, W), device=dev, generator=g).topk(nerr, dim=1).indices
    bad = clean.clone()
    bad.scatter_(1, pos, bad.gather(1, pos) ^ torch.randint(1, 256, (n, nerr), dtype=torch.uint8, device=dev,
                                                            generator=g))
    del pos
    # the caller-side index tensor: offset of every byte of the batch in its span
    idx = torch.arange(n * W, dtype=torch.int64, device=dev)
    idx += ((phase + idx) % I) * (M * I)
    stream = torch.randint(0, 256, (span,), dtype=torch.uint8, device=dev, generator=g)  # holes: other codewords
    h.conv_interleave_device(bad.data_ptr(), W, bad.data_ptr() + size, W, size, n, I, M, phase, stream.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(stream[idx].view(n, W), bad), "the library's interleave is not the index formula"
    h.reserve(n)
    h.reserve_interleaved(n)
    rows, trows, rrows = torch.empty_like(bad), torch.empty_like(bad), bad.clone()
    out, tout = torch.empty_like(stream), torch.empty_like(stream)
    enc = clean.clone()  # messages with parity to overwrite
    cp = torch.empty_like(bad)
    ok = torch.zeros((4, n), dtype=torch.uint8, device=dev)
    sp, rp, tp, qp, ep = stream.data_ptr(), rows.data_ptr(), trows.data_ptr(), rrows.data_ptr(), enc.data_ptr()

    def torch_decode():
        torch.index_select(stream, 0, idx, out=trows.view(-1))
        h.decode_batch_device(tp, W, tp + size, W, size, n, ok[1].data_ptr(), stream=s)

    def torch_encode():
        h.encode_batch_device(ep, W, ep + size, W, size, n, s)
        tout.index_copy_(0, idx, enc.view(-1))

    legs = {
        "deinterleave": lambda: h.conv_deinterleave_device(sp, I, M, phase, rp, W, rp + size, W, size, n, s),
        "interleave": lambda: h.conv_interleave_device(qp, W, qp + size, W, size, n, I, M, phase, out.data_ptr(), s),
        "memcpy_d2d": lambda: hip.hipMemcpyAsync(cp.data_ptr(), qp, n * W, 3, s),
        "decode_conv": lambda: h.decode_conv_device(sp, I, M, phase, rp, W, rp + size, W, size, n, ok[0].data_ptr(),
                                                    stream=s),
        "torch_decode": torch_decode,
        "row_decode": lambda: h.decode_batch_device(qp, W, qp + size, W, size, n, ok[2].data_ptr(), stream=s),
        "encode_conv": lambda: h.encode_conv_device(ep, W, ep + size, W, size, n, I, M, phase, out.data_ptr(), s),
        "torch_encode": torch_encode,
        "row_encode": lambda: h.encode_batch_device(ep, W, ep + size, W, size, n, s),
        "check_conv": lambda: h.check_conv_device(sp, I, M, phase, size, n, ok[3].data_ptr(), s),
        "row_check": lambda: h.check_batch_device(qp, W, qp + size, W, size, n, ok[3].data_ptr(), s),
    }
    wall = {k: [] for k in legs}
    kern = {20: [], 21: []}
    for timing in (False, True):
        h.timing(timing)
        for step in range(steps if timing else warmup + steps):
            for leg, fn in legs.items():
                if leg in ("row_decode", "row_check", "interleave", "memcpy_d2d"):
                    rrows.copy_(bad)
                t = timed(fn)
                if not timing and step >= warmup:
                    wall[leg].append(t)
                if leg == "decode_conv":
                    assert torch.equal(rows, clean) and int(ok[0].sum()) == n
                elif leg == "torch_decode":
                    assert torch.equal(trows, clean) and int(ok[1].sum()) == n
                elif leg == "row_decode":
                    assert torch.equal(rrows, clean) and int(ok[2].sum()) == n
                elif leg in ("encode_conv", "torch_encode", "row_encode"):
                    assert torch.equal(enc, clean)
                if timing:
                    for k in kern:
                        ms, cnt = h.timing_read(k)
                        if leg in ("deinterleave", "interleave") and cnt:
                            kern[k].append(ms * 1e3)
                    h.timing(True)
    h.timing(False)
    # the encode legs wrote the same bytes of their spans
    assert torch.equal(out[idx], tout[idx]) and torch.equal(out[idx].view(n, W), clean)
    med = {k: stats(v) for k, v in wall.items()}
    line = {"standard": name, "codewords": n, "row_bytes": W, "branches": I, "cell": M, "errors": nerr,
            "tile": P.conv_tile(W, I, M), "steps": steps, "event_us": med,
            "kernel_us": {P.CONV_KERNEL_NAMES[k]: stats(v) for k, v in kern.items() if v},
            "TBps": {k: round(2 * n * W / (med[k]["median"] * 1e-6) / 1e12, 3)
                     for k in ("deinterleave", "interleave", "memcpy_d2d")},
            "layout_over_copy": {k: round(med[k]["median"] / med["memcpy_d2d"]["median"], 2)
                                 for k in ("deinterleave", "interleave")},
            "decode_conv_wins_every_pair": all(a < b for a, b in zip(wall["decode_conv"], wall["torch_decode"])),
            "encode_conv_wins_every_pair": all(a < b for a, b in zip(wall["encode_conv"], wall["torch_encode"]))}
    h.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "conv_bench needs a GPU"
    hip = hip_runtime()
    for name in STANDARDS:
        line = run(name, a.batch, a.steps, a.warmup, hip)
        print(json.dumps(line), flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
