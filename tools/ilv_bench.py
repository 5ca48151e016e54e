#!/usr/bin/env python3
"""Cost of the interleaved layout (diagnostic): bench.py's workload -- 2^20
codewords of RS(255,223), 16 errors each, resident on the device -- as CCSDS
wire blocks of depth 1, 4, 5 and 8 through poporon_*_interleaved_device, next
to the same codewords as rows through poporon_*_batch_device and to a
hipMemcpyAsync device-to-device copy of the same byte count, all from one
process with the legs alternating inside every step.

    python tools/ilv_bench.py [--steps 10] [--warmup 3] [--batch 1048576] [--wire-form] [--append FILE]

--wire-form adds two legs per depth, alternating with the others: the same
frames in CCSDS wire form (dual-basis symbols, randomized) decoded by a handle
with poporon_amd_set_wire_form_ccsds set ("wire_decode"), and the caller-side
equivalent the wire form replaces ("caller_decode"): torch XOR with the
sequence and a table gather over the block, the plain interleaved decode, and
a table gather back.  --append FILE appends the per-depth lines to FILE.

Per depth one JSON line: wall time of call + synchronise (median, min, max
over the steps, us); per-kernel time per call from the library's events
(poporon_amd_timing, ids 15 = gather, 16 = scatter, and the codec ids) in a
second pass; the layout kernels' achieved bytes per second (bytes read +
bytes written over the kernel time) and the copy's (2 x bytes over its wall
time)."""
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

K, N, NR, NERR = 223, 255, 32, 16


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


def kernel_ms(h, calls):
    names = {**P.KERNEL_NAMES, **P.ILV_KERNEL_NAMES}
    out = {}
    for k in names:
        ms, n = h.timing_read(k)
        if n:
            out[str(k)] = {"name": names[k], "us_per_call": round(ms * 1e3 / calls, 1), "launches_per_call": n / calls}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--wire-form", action="store_true")
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip = hip_runtime()
    hi, hr = P.Poporon.default(device=0), P.Poporon.default(device=0)  # interleaved calls, row calls
    s = torch.cuda.current_stream().cuda_stream
    n0 = a.batch
    clean = torch.zeros((n0, N), dtype=torch.uint8, device=dev)
    clean[:, :K] = devdata.synth_bytes(bench.SEED, 0, n0, K, dev)
    hr.encode_batch_device(clean.data_ptr(), N, clean.data_ptr() + K, N, K, n0, s)
    pos, mag = devdata.synth_errors(bench.SEED + 1, 0, n0, NERR, N, dev)
    bad = clean.clone()
    devdata.channel(pos, mag, NERR, bad.data_ptr(), N, n0, s)
    torch.cuda.synchronize()
    hi.reserve_interleaved(n0)
    hr.reserve(n0)
    if a.wire_form:
        hw = P.Poporon.default(device=0)  # interleaved calls with the CCSDS wire form
        hw.set_wire_form_ccsds(True, True)
        hw.reserve_interleaved(n0)
        to_code, to_wire = (torch.from_numpy(t).to(dev) for t in P.ccsds_dual_basis())
        rand = torch.from_numpy(P.ccsds_randomizer()).to(dev)
    result = {"workload": f"RS(255,223), {n0} codewords, {NERR} errors each", "steps": a.steps, "depths": {}}
    for depth in (1, 4, 5, 8):
        frames = n0 // depth
        n = frames * depth
        fb = N * depth  # wire block: message region, then parity region
        to_frames = lambda rows: rows[:n].view(frames, depth, N).transpose(1, 2).contiguous()  # noqa: E731
        f_clean, f_bad = to_frames(clean), to_frames(bad)
        fw, rw = f_bad.clone(), bad[:n].clone()
        cp = torch.empty_like(fw)
        ok = torch.zeros((4, n), dtype=torch.uint8, device=dev)
        fp, rp = fw.data_ptr(), rw.data_ptr()
        legs = {
            "ilv_decode": lambda: hi.decode_interleaved_device(fp, fb, fp + K * depth, fb, K, depth, frames,
                                                               ok[0].data_ptr(), stream=s),
            "row_decode": lambda: hr.decode_batch_device(rp, N, rp + K, N, K, n, ok[1].data_ptr(), stream=s),
            "ilv_encode": lambda: hi.encode_interleaved_device(fp, fb, fp + K * depth, fb, K, depth, frames, stream=s),
            "row_encode": lambda: hr.encode_batch_device(rp, N, rp + K, N, K, n, s),
            "memcpy_d2d": lambda: hip.hipMemcpyAsync(cp.data_ptr(), fp, n * N, 3, s),
        }
        owner = {k: hi if k.startswith("ilv") else hr for k in legs}  # whose kernel timers a leg's call fills
        if a.wire_form:
            # the sequence as it falls on one block (a frame tensor is [frames, symbol, codeword])
            seq = rand[torch.arange(fb, device=dev) % rand.numel()].view(N, depth)
            w_bad, w_clean = to_wire[f_bad.int()] ^ seq, to_wire[f_clean.int()]  # received; decoded, derandomized
            ww, cw = w_bad.clone(), w_bad.clone()
            wp, cwp = ww.data_ptr(), cw.data_ptr()

            def caller_decode():
                torch.bitwise_xor(cw, seq, out=cw)
                cw.copy_(to_code[cw.int()])
                hi.decode_interleaved_device(cwp, fb, cwp + K * depth, fb, K, depth, frames, ok[3].data_ptr(),
                                             stream=s)
                cw.copy_(to_wire[cw.int()])

            legs["wire_decode"] = lambda: hw.decode_interleaved_device(wp, fb, wp + K * depth, fb, K, depth, frames,
                                                                       ok[2].data_ptr(), stream=s)
            legs["caller_decode"] = caller_decode
            owner.update(wire_decode=hw, caller_decode=hi)
        wall = {k: [] for k in legs}
        kern = {}
        for timing in (False, True):
            for h in set(owner.values()):
                h.timing(timing)
            for step in range(a.warmup + a.steps if not timing else a.steps):
                for name, fn in legs.items():
                    if name == "ilv_decode":
                        fw.copy_(f_bad)
                    elif name == "row_decode":
                        rw.copy_(bad[:n])
                    elif name == "wire_decode":
                        ww.copy_(w_bad)
                    elif name == "caller_decode":
                        cw.copy_(w_bad)
                    t = timed(fn)
                    if not timing and step >= a.warmup:
                        wall[name].append(t)
                    if name == "ilv_decode":
                        assert torch.equal(fw, f_clean) and int(ok[0].sum()) == n
                    elif name == "row_decode":
                        assert torch.equal(rw, clean[:n]) and int(ok[1].sum()) == n
                    elif name == "ilv_encode":
                        assert torch.equal(fw, f_clean)
                    elif name == "wire_decode":
                        assert torch.equal(ww, w_clean) and int(ok[2].sum()) == n
                    elif name == "caller_decode":
                        assert torch.equal(cw, w_clean) and int(ok[3].sum()) == n
                    if timing and name != "memcpy_d2d":  # this call's kernels; the totals start over
                        h = owner[name]
                        kern.setdefault(name, []).append(kernel_ms(h, 1))
                        h.timing(True)
        for h in set(owner.values()):
            h.timing(False)
        kern = {leg: {k: dict(calls[0][k], us_per_call=sorted(c[k]["us_per_call"] for c in calls)[len(calls) // 2])
                      for k in calls[0]} for leg, calls in kern.items()}  # median over the steps
        line = {"depth": depth, "codewords": n, "wall_us": {k: stats(v) for k, v in wall.items()}, "kernels": kern}
        copy_s = line["wall_us"]["memcpy_d2d"]["median"] * 1e-6
        rates = {"memcpy_d2d_TBps": round(2 * n * N / copy_s / 1e12, 3)}
        # bytes read + written per codeword: decode moves both regions each way, encode the
        # message in and the parity out (row side in dwords: the message's 223 bytes as 224)
        moved = {("ilv_decode", "15"): 2 * N, ("ilv_decode", "16"): 2 * N, ("ilv_encode", "15"): K + K + 1,
                 ("ilv_encode", "16"): 2 * NR, ("wire_decode", "15"): 2 * N, ("wire_decode", "16"): 2 * N}
        for (leg, kid), b in moved.items():
            if kid in kern.get(leg, {}):
                rates[f"{leg}_id{kid}_TBps"] = round(n * b / (kern[leg][kid]["us_per_call"] * 1e-6) / 1e12, 3)
        line["rates"] = rates
        result["depths"][depth] = line
        print(json.dumps(line), flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(json.dumps(line) + "\n")
        del f_clean, f_bad, fw, rw, cp, ok, legs
        if a.wire_form:
            del w_bad, w_clean, ww, cw, seq
    print(json.dumps(result))


if __name__ == "__main__":
    main()
