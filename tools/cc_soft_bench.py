#!/usr/bin/env python3
"""Throughput of the K = 7 soft-output decode beside the hard decode of the same tree, and the failed codewords
of the concatenated chain with and without soft outputs (diagnostic), resident on the device, all legs from one
process:

    one frame of 2^27 info bits of the DVB code (171/133) at rate 1/2 and at rate 7/8, BPSK over AWGN at
    --ebn0 dB per rate (default 3.0 and 5.5), LLR = rint(32 y) clipped to +-127, fixed seed: the workload of
    tools/cc_bench.py

    copy          a device-to-device copy of the frame's LLR bytes
    decode        poporon_cc_decode_device between device events, at every block / overlap of --settings
    decode_soft   poporon_cc_decode_siso_device (shift 0) at the same settings; `ratio_to_hard` is its median
                  over the hard decode's, and `sign_differs_from_hard` counts the non-zero outputs whose sign is
                  not the hard decode's bit (the contract says none)

    chain         --codewords RS(255,223) codewords (default 2^14), one per frame of 2040 info bits of the CCSDS
                  code at rate 1/2 from state 0, at each --chain-ebn0 (dB per info bit of the whole chain):
                  hard Viterbi -> poporon_decode_batch_device against soft decode -> poporon_decode_soft_batch_device
                  at --flips; a codeword fails if its row does not come back as sent

    python tools/cc_soft_bench.py [--steps 5] [--warmup 2] [--log2-bits 27] [--ebn0 3.0,5.5] [--seed 3271]
                                  [--settings 512/96,512/64,1024/96] [--codewords 16384]
                                  [--chain-ebn0 2.4,2.8] [--flips 4] [--append FILE]

One JSON line per leg: the event times (median, min, max over the steps, us) and info Mbit/s at the median."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import libpoporon_amd as P  # noqa: E402
from cc_bench import RATES, bit_count, make_llr, run_timed  # noqa: E402

RS223 = (8, 0x11D, 1, 1, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2-bits", type=int, default=27)
    ap.add_argument("--ebn0", default="3.0,5.5")
    ap.add_argument("--seed", type=int, default=0xCC7)
    ap.add_argument("--settings", default="512/96,512/64,1024/96")
    ap.add_argument("--codewords", type=int, default=1 << 14)
    ap.add_argument("--chain-ebn0", default="2.4,2.8")
    ap.add_argument("--flips", type=int, default=4)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    settings = [tuple(int(v) for v in x.split("/")) for x in a.settings.split(",") if x]
    assert torch.cuda.is_available(), "cc_soft_bench needs a GPU"
    dev = torch.device("cuda", 0)
    nbits = 1 << a.log2_bits
    ebn0 = [float(x) for x in a.ebn0.split(",")]
    table = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int32, device=dev)
    shifts = torch.arange(7, -1, -1, device=dev, dtype=torch.uint8)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    msg = torch.randint(0, 256, (nbits // 8,), dtype=torch.uint8, device=dev, generator=g)
    s = torch.cuda.current_stream().cuda_stream

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(json.dumps(line) + "\n")

    for (name, punct, rate), db in zip(RATES, ebn0):
        if not settings:
            break
        enc = P.Cc(P.CC_CODE_DVB, punct, 512, 64)
        nsym = enc.symbols(nbits)
        sym = torch.zeros((nsym + 7) // 8, dtype=torch.uint8, device=dev)
        head = {"code": "171/133", "rate": name, "info_bits": nbits, "symbols": nsym, "ebn0_db": db,
                "llr": "rint(32 y) clipped to +-127", "seed": a.seed, "steps": a.steps}
        enc.encode(msg, msg.numel(), nbits, 1, sym, sym.numel(), 0, stream=s)
        sigma = math.sqrt(1.0 / (2.0 * rate * 10.0 ** (db / 10.0)))
        llr = make_llr(sym, nsym, sigma, g)
        del sym
        other = torch.empty_like(llr)
        t = run_timed(lambda: other.copy_(llr), a.steps, a.warmup)
        emit(dict(head, leg="copy", bytes=nsym, event_us=t, gb_s=round(nsym / t["median"] / 1e3, 1)))
        del other
        out = torch.empty_like(msg)
        soft = torch.empty(nbits, dtype=torch.int8, device=dev)
        for block, overlap in settings:
            cc = P.Cc(P.CC_CODE_DVB, punct, block, overlap)
            th = run_timed(lambda: cc.decode(llr, nsym, nbits, 1, out, msg.numel(), 0, -1, stream=s), a.steps, a.warmup)
            emit(dict(head, leg="decode", block=block, overlap=overlap, event_us=th,
                      mbit_s=round(nbits / th["median"], 1), bit_errors=bit_count(out ^ msg, table)))
            ts = run_timed(lambda: cc.decode_soft(llr, nsym, nbits, 1, soft, nbits, 0, -1, 0, stream=s), a.steps,
                           a.warmup)
            differs = zeros = sat = errors = 0
            for lo in range(0, nbits, 1 << 24):  # piece by piece: the bits of `out` beside the signs of `soft`
                piece = soft[lo:lo + (1 << 24)]
                hard = ((out[lo // 8:(lo + (1 << 24)) // 8, None] >> shifts) & 1).reshape(-1)
                sent = ((msg[lo // 8:(lo + (1 << 24)) // 8, None] >> shifts) & 1).reshape(-1)
                differs += int(((piece < 0) != (hard == 1))[piece != 0].sum())
                errors += int(((piece < 0) != (sent == 1)).sum())
                zeros += int((piece == 0).sum())
                sat += int((piece.abs() == 127).sum())
            emit(dict(head, leg="decode_soft", block=block, overlap=overlap, shift=0, event_us=ts,
                      mbit_s=round(nbits / ts["median"], 1), ratio_to_hard=round(ts["median"] / th["median"], 3),
                      sign_differs_from_hard=differs, sign_errors=errors, zeros=zeros, saturated=sat))
            cc.close()
        enc.close()
        del llr, out, soft
        torch.cuda.empty_cache()

    # ---- the chain: failed codewords with and without soft outputs -------------------------------
    count, size, W = a.codewords, 223, 255
    if count:
        h = P.Poporon(*RS223)
        cc = P.Cc(P.CC_CODE_CCSDS, P.CC_PUNCTURE_NONE, P.CC_DEFAULT_BLOCK, P.CC_DEFAULT_OVERLAP)
        fbits = W * 8
        nsym = cc.symbols(fbits)
        cw = torch.randint(0, 256, (count, W), dtype=torch.uint8, device=dev, generator=g)
        h.encode_batch_device(cw.data_ptr(), W, cw.data_ptr() + size, W, size, count)
        sym = torch.zeros((count, nsym // 8), dtype=torch.uint8, device=dev)
        cc.encode(cw, W, fbits, count, sym, nsym // 8, 0)
        rate = 0.5 * size / W
        for db in (float(x) for x in a.chain_ebn0.split(",") if x):
            sigma = math.sqrt(1.0 / (2.0 * rate * 10.0 ** (db / 10.0)))
            llr = make_llr(sym.reshape(-1), count * nsym, sigma, g).reshape(count, nsym)
            rows = torch.zeros((count, W), dtype=torch.uint8, device=dev)
            ok = torch.zeros(count, dtype=torch.uint8, device=dev)
            cc.decode(llr, nsym, fbits, count, rows, W, 0, -1)
            inner = int((rows != cw).any(1).sum())
            h.decode_batch_device(rows.data_ptr(), W, rows.data_ptr() + size, W, size, count, ok.data_ptr())
            torch.cuda.synchronize()
            hard_failed = int(((ok == 0) | (rows != cw).any(1)).sum())
            soft = torch.zeros((count, fbits), dtype=torch.int8, device=dev)
            cc.decode_soft(llr, nsym, fbits, count, soft, fbits, 0, -1, 0)
            rows.zero_()
            ok.zero_()
            h.decode_soft_batch_device(soft.data_ptr(), fbits, rows.data_ptr(), W, rows.data_ptr() + size, W, size,
                                       count, a.flips, ok.data_ptr())
            torch.cuda.synchronize()
            soft_failed = int(((ok == 0) | (rows != cw).any(1)).sum())
            emit({"leg": "chain", "outer": "RS(255,223)", "inner": "CCSDS 171/133 rate 1/2, block 512 overlap 96",
                  "codewords": count, "ebn0_db": db, "seed": a.seed, "flips": a.flips,
                  "codewords_wrong_after_viterbi": inner, "failed_hard_chain": hard_failed,
                  "failed_soft_chain": soft_failed})
            del llr, soft
        cc.close()
        h.close()


if __name__ == "__main__":
    main()
