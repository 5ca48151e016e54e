#!/usr/bin/env python3
"""Throughput and error counts of the K = 7 Viterbi decode over block and overlap (diagnostic), resident on
the device, all legs from one process:

    one frame of 2^27 info bits of the DVB code (171/133) at rate 1/2 and at rate 7/8, BPSK over AWGN at
    --ebn0 dB per rate (default 3.0 and 5.5), LLR = rint(32 y) clipped to +-127, fixed seed

    decode        poporon_cc_decode_device between device events, block in {256, 512, 1024, 2048} x overlap in
                  {32, 64, 96, 128}, and overlap = 1024 at every block as the yardstick of the error counts
    copy          a device-to-device copy of the frame's LLR bytes: what moving the input alone costs
    encode        poporon_cc_encode_device of the frame

    python tools/cc_bench.py [--steps 5] [--warmup 2] [--log2-bits 27] [--ebn0 3.0,5.5] [--seed 3271]
                             [--blocks 256,512,1024,2048] [--overlaps 32,64,96,128] [--append FILE]

Other seeds give the run-to-run spread of the error counts, which is what the choice of the library's default
block and overlap is held against.

One JSON line per leg: the event times (median, min, max over the steps, us), info Mbit/s at the median, and
for a decode the bit errors against the transmitted bits and the bits that differ from overlap = 1024 at the
same block."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import libpoporon_amd as P  # noqa: E402

SCALE = 32.0
BLOCKS = (256, 512, 1024, 2048)
OVERLAPS = (32, 64, 96, 128)
REFERENCE_OVERLAP = 1024
RATES = (("1/2", P.CC_PUNCTURE_NONE, 0.5), ("7/8", P.CC_PUNCTURE_DVB_7_8, 7.0 / 8.0))
PIECE = 1 << 24  # symbols per piece of the LLR generation


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


def run_timed(fn, steps, warmup):
    return stats([timed(fn) for _ in range(warmup + steps)][warmup:])


def make_llr(sym, nsym, sigma, g):
    """packed symbols (MSB first) -> int8 LLRs, piece by piece"""
    llr = torch.empty(nsym, dtype=torch.int8, device=sym.device)
    shifts = torch.arange(7, -1, -1, device=sym.device, dtype=torch.uint8)
    for a in range(0, nsym, PIECE):
        b = min(nsym, a + PIECE)
        bits = ((sym[a // 8:(b + 7) // 8, None] >> shifts) & 1).reshape(-1)[:b - a]
        y = (1.0 - 2.0 * bits.float()) + sigma * torch.randn(b - a, device=sym.device, generator=g)
        llr[a:b] = torch.clamp(torch.round(SCALE * y), -127, 127).to(torch.int8)
    return llr


def bit_count(x, table):
    """set bits of a uint8 tensor"""
    total = 0
    for a in range(0, x.numel(), PIECE):
        total += int(table[x[a:a + PIECE].long()].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2-bits", type=int, default=27)
    ap.add_argument("--ebn0", default="3.0,5.5")
    ap.add_argument("--seed", type=int, default=0xCC7)
    ap.add_argument("--blocks", default=",".join(map(str, BLOCKS)))
    ap.add_argument("--overlaps", default=",".join(map(str, OVERLAPS)))
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    blocks, overlaps = [int(x) for x in a.blocks.split(",")], tuple(int(x) for x in a.overlaps.split(",") if x)
    assert torch.cuda.is_available(), "cc_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nbits = 1 << a.log2_bits
    ebn0 = [float(x) for x in a.ebn0.split(",")]
    table = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    msg = torch.randint(0, 256, (nbits // 8,), dtype=torch.uint8, device=dev, generator=g)
    s = torch.cuda.current_stream().cuda_stream

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(json.dumps(line) + "\n")

    for (name, punct, rate), db in zip(RATES, ebn0):
        enc = P.Cc(P.CC_CODE_DVB, punct, 512, 64)
        nsym = enc.symbols(nbits)
        sym = torch.zeros((nsym + 7) // 8, dtype=torch.uint8, device=dev)
        head = {"code": "171/133", "rate": name, "info_bits": nbits, "symbols": nsym, "ebn0_db": db,
                "llr": "rint(32 y) clipped to +-127", "seed": a.seed, "steps": a.steps}
        t = run_timed(lambda: enc.encode(msg, msg.numel(), nbits, 1, sym, sym.numel(), 0, stream=s), a.steps, a.warmup)
        emit(dict(head, leg="encode", event_us=t, mbit_s=round(nbits / t["median"], 1)))
        sigma = math.sqrt(1.0 / (2.0 * rate * 10.0 ** (db / 10.0)))
        llr = make_llr(sym, nsym, sigma, g)
        other = torch.empty_like(llr)
        t = run_timed(lambda: other.copy_(llr), a.steps, a.warmup)
        emit(dict(head, leg="copy", bytes=nsym, event_us=t, gb_s=round(nsym / t["median"] / 1e3, 1)))
        del other
        out = torch.empty_like(msg)
        ref = torch.empty_like(msg)
        for block in blocks:
            for overlap in (REFERENCE_OVERLAP,) + overlaps:
                cc = P.Cc(P.CC_CODE_DVB, punct, block, overlap)
                dst = ref if overlap == REFERENCE_OVERLAP else out
                t = run_timed(lambda: cc.decode(llr, nsym, nbits, 1, dst, msg.numel(), 0, -1, stream=s), a.steps,
                              a.warmup)
                emit(dict(head, leg="decode", block=block, overlap=overlap, event_us=t,
                          mbit_s=round(nbits / t["median"], 1), bit_errors=bit_count(dst ^ msg, table),
                          differs_from_overlap_1024=bit_count(dst ^ ref, table)))
                cc.close()
        enc.close()
        del llr, sym, out, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
