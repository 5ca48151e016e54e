#!/usr/bin/env python3
"""Cost of the product-code calls (diagnostic), resident on the device, all legs from one process and
alternating inside every step:

    workload: 5,041 DVD RS-PC blocks (208 x 182; rows RS(182,172), columns RS(208,192); 2^20 row
              codewords, one chunk), 16 overwritten rows plus 2 errors in every other row of every block;
              schedule row, column, row with couple = 1

    product_decode   (a) poporon_decode_product_device, tight blocks (the row code in place)
    product_staged       the same on a block stride that is no multiple of the pitch (rows staged too)
    memcpy_d2d       (c) hipMemcpyAsync device-to-device of the same count*208*182 bytes
    caller_decode    (d) the caller-side route the call replaces: row call in place and its check,
                         .transpose copy, lists built by torch ops from the flags, column call and its
                         check, transpose back, lists again, row call.  It does LESS than (a): no flags
                         of the last pass, no final column check, no block-ok
    product_encode, caller_encode  (e) the encode, and transpose / column encode / transpose back /
                         row encode

(b) is the layout and list kernels' own time from the library's events (poporon_amd_timing, ids 24 to
26 on both axis handles) in a second pass.

    python tools/product_bench.py [--steps 10] [--warmup 3] [--blocks 5041] [--append FILE]

One JSON line: event time of every leg (median, min, max over the steps, us), the kernels' own time,
bytes per second of the copy, and whether the product call beat the caller route in every alternated
pair.  Every decode is checked inside the loop: the caller route's bytes equal the product call's, and
every block the call reports ok equals the clean block."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import libpoporon_amd as P  # noqa: E402

ROW, COL = (8, 0x11D, 0, 1, 10), (8, 0x11D, 0, 1, 16)
K1, K2, N1, N2 = 172, 192, 182, 208


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


def lists_from_flags(flags, roots, ncw):
    """the threshold rule by torch ops: flags u8[count, n] -> (positions u8[count*ncw, 16 or roots rounded up],
    counts u8[count*ncw])"""
    count, n = flags.shape
    ls = (roots + 15) & ~15
    num = flags.ne(0).sum(1)
    use = (num > roots // 2) & (num <= roots)
    order = torch.argsort(flags.eq(0).to(torch.uint8), dim=1, stable=True)[:, :ls]  # the flagged indices first
    keep = (torch.arange(ls, device=flags.device)[None, :] < num[:, None]) & use[:, None]
    pos = torch.where(keep, order, torch.zeros_like(order)).to(torch.uint8)
    cnt = torch.where(use, num, torch.zeros_like(num)).to(torch.uint8)
    return pos[:, None, :].expand(count, ncw, ls).contiguous(), cnt[:, None].expand(count, ncw).contiguous(), ls


def run(steps, warmup, count, hip):
    dev = torch.device("cuda", 0)
    p = P.Product(ROW, COL, device=0)
    hr, hc = P.Poporon(*ROW, device=0), P.Poporon(*COL, device=0)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(0x5EED)
    clean = torch.zeros((count, N2, N1), dtype=torch.uint8, device=dev)
    clean[:, :K2, :K1] = torch.randint(0, 256, (count, K2, K1), dtype=torch.uint8, device=dev, generator=g)
    p.reserve(K1, K2, count)
    p.encode_device(clean.data_ptr(), N1, N1 * N2, K1, K2, count, s)
    bad = clean.clone()
    first = torch.randint(0, N1, (count, N2, 1), device=dev, generator=g)
    pos = torch.cat([first, (first + 1 + torch.randint(0, N1 - 1, (count, N2, 1), device=dev, generator=g)) % N1], 2)
    bad.scatter_(2, pos, bad.gather(2, pos) ^ torch.randint(1, 256, (count, N2, 2), dtype=torch.uint8, device=dev,
                                                            generator=g))
    rows = torch.rand((count, N2), device=dev, generator=g).topk(16, dim=1).indices
    bad[torch.arange(count, device=dev)[:, None], rows] = torch.randint(0, 256, (count, 16, N1), dtype=torch.uint8,
                                                                        device=dev, generator=g)
    del first, pos, rows
    nbytes = count * N1 * N2
    pitch_s, stride_s = N1 + 3, N2 * (N1 + 3) + 7  # the staged placement
    sbuf = torch.empty(count * stride_s, dtype=torch.uint8, device=dev)
    swork = torch.as_strided(sbuf, (count, N2, N1), (stride_s, pitch_s, 1))
    work, twork = torch.empty_like(bad), torch.empty_like(bad)
    cols = torch.empty((count, N1, N2), dtype=torch.uint8, device=dev)
    cp = torch.empty_like(bad)
    rd = torch.zeros((2, count, N2), dtype=torch.uint8, device=dev)
    cd = torch.zeros((2, count, N1), dtype=torch.uint8, device=dev)
    okb = torch.zeros((2, count), dtype=torch.uint8, device=dev)
    okc = torch.zeros(count * N2, dtype=torch.uint8, device=dev)
    wp, tp, cpx = work.data_ptr(), twork.data_ptr(), cols.data_ptr()

    def caller_decode():
        hr.decode_batch_device(tp, N1, tp + K1, N1, K1, count * N2, okc.data_ptr(), stream=s)
        hr.check_batch_device(tp, N1, tp + K1, N1, K1, count * N2, rd[1].data_ptr(), s)
        cols.copy_(twork.transpose(1, 2))
        epos, ecnt, ls = lists_from_flags(rd[1], 16, N1)
        hc.decode_batch_device(cpx, N2, cpx + K2, N2, K2, count * N1, okc.data_ptr(), stream=s,
                               d_positions=epos.data_ptr(), positions_stride=ls, d_counts=ecnt.data_ptr())
        hc.check_batch_device(cpx, N2, cpx + K2, N2, K2, count * N1, cd[1].data_ptr(), s)
        twork.copy_(cols.transpose(1, 2))
        epos, ecnt, ls = lists_from_flags(cd[1], 10, N2)
        hr.decode_batch_device(tp, N1, tp + K1, N1, K1, count * N2, okc.data_ptr(), stream=s,
                               d_positions=epos.data_ptr(), positions_stride=ls, d_counts=ecnt.data_ptr())

    def caller_encode():
        cols[:, :K1, :K2].copy_(twork[:, :K2, :K1].transpose(1, 2))
        hc.encode_batch_device(cpx, N2, cpx + K2, N2, K2, count * N1, s)  # (all n1 rows of cols: one strided batch)
        twork[:, K2:, :K1].copy_(cols[:, :K1, K2:].transpose(1, 2))
        hr.encode_batch_device(tp, N1, tp + K1, N1, K1, count * N2, s)

    legs = {
        "memcpy_d2d": lambda: hip.hipMemcpyAsync(cp.data_ptr(), wp, nbytes, 3, s),
        "product_decode": lambda: p.decode_device(wp, N1, N1 * N2, K1, K2, count, 0, 3, 1, rd[0].data_ptr(),
                                                  cd[0].data_ptr(), okb[0].data_ptr(), stream=s),
        "caller_decode": caller_decode,
        "product_staged": lambda: p.decode_device(sbuf.data_ptr(), pitch_s, stride_s, K1, K2, count, 0, 3, 1,
                                                  rd[0].data_ptr(), cd[0].data_ptr(), okb[1].data_ptr(), stream=s),
        "product_encode": lambda: p.encode_device(wp, N1, N1 * N2, K1, K2, count, s),
        "caller_encode": caller_encode,
    }
    wall = {k: [] for k in legs}
    ids = (P.KERNEL_PROD_GATHER, P.KERNEL_PROD_SCATTER, P.KERNEL_PROD_LISTS)
    kern = {}
    axes = (p.handle(0), p.handle(1))
    repaired = None
    for timing in (False, True):
        for h in axes:
            h.timing(timing)
        for step in range(steps if timing else warmup + steps):
            for leg, fn in legs.items():
                enc = leg.endswith("encode")
                dst = swork if leg == "product_staged" else twork if leg.startswith("caller") else work
                dst.copy_(clean if enc else bad)
                if enc:
                    dst[:, K2:, :].zero_()
                    dst[:, :, K1:].zero_()
                t = timed(fn)
                if not timing and step >= warmup:
                    wall[leg].append(t)
                if leg == "product_decode":
                    good = okb[0].bool()
                    assert torch.equal(work[good], clean[good]) and not rd[0][good].any() and not cd[0][good].any()
                    repaired = int(good.sum())
                elif leg == "caller_decode":
                    assert torch.equal(twork, work)
                elif leg == "product_staged":
                    assert torch.equal(swork, work) and torch.equal(okb[1], okb[0])
                elif enc:
                    assert torch.equal(dst, clean)
                if timing:
                    for a, h in enumerate(axes):
                        for k in ids:
                            ms, cnt = h.timing_read(k)
                            if cnt:
                                kern.setdefault(f"{leg}: axis {a} {P.PROD_KERNEL_NAMES[k]} x{cnt}", []).append(ms * 1e3)
                        h.timing(True)
    for h in axes:
        h.timing(False)
    med = {k: stats(v) for k, v in wall.items()}
    line = {"workload": "dvd", "blocks": count, "bytes": nbytes, "schedule": "row, column, row; couple 1",
            "blocks_repaired": repaired, "steps": steps, "event_us": med,
            "kernel_us": {k: stats(v) for k, v in kern.items()},
            "copy_TBps": round(2 * nbytes / (med["memcpy_d2d"]["median"] * 1e-6) / 1e12, 3),
            "product_wins_every_pair": {op: all(a < b for a, b in zip(wall[f"product_{op}"], wall[f"caller_{op}"]))
                                        for op in ("decode", "encode")}}
    p.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5041)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "product_bench needs a GPU"
    line = run(a.steps, a.warmup, a.blocks, hip_runtime())
    print(json.dumps(line), flush=True)
    if a.append:
        with open(a.append, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
