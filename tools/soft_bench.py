#!/usr/bin/env python3
"""Cost and gain of the soft-decision decode (diagnostic), resident on the device, all legs from one process:

    2^16 codewords of RS(255,223), BPSK over AWGN at --ebn0 dB (default 5.6), LLR = rint(32 y) clipped to
    +-127, fixed seed; flips = 0, 2, 4 and 6

    soft          poporon_decode_soft_batch_device: event time of the call, and in a second pass the
                  library's own kernel times per id (27 = rs_soft_expand_k, 28 = rs_soft_select_k, the
                  decode of the candidates under its own ids)
    hard          poporon_decode_batch_device on the 2^16 hard rows
    floor         poporon_decode_batch_device on the 2^16 << flips candidate rows, ready in memory: what the
                  decodes alone cost
    torch         the caller-side route the call replaces: torch builds the candidates (top-k of the keys,
                  XOR into copies of the hard rows), the row decode runs on them, torch scores them (per bit
                  plane, |llr| summed where the decoded row differs from the hard row), takes the minimum of
                  score * 64 + p over the ok candidates and gathers the winners

    python tools/soft_bench.py [--steps 5] [--warmup 2] [--count 65536] [--ebn0 5.6] [--flips 0,2,4,6]
                               [--append FILE]

One JSON line per flips: the event times (median, min, max over the steps, us), the kernel times, how many
codewords came back as the transmitted ones, how many of those flips = 0 does not recover, how many were
accepted wrongly, and whether the call and the torch route agree in every output (they must)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import libpoporon_amd as P  # noqa: E402

PARAMS, SIZE, NR, M = (8, 0x11D, 1, 1, 32), 223, 32, 8
W = SIZE + NR
SCALE = 32.0


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


def make_llr(h, n, ebn0, dev, s):
    g = torch.Generator(device=dev).manual_seed(0x50F7)
    cw = torch.randint(0, 256, (n, W), dtype=torch.uint8, device=dev, generator=g)
    h.encode_batch_device(cw.data_ptr(), W, cw.data_ptr() + SIZE, W, SIZE, n, s)
    shifts = torch.arange(M - 1, -1, -1, device=dev, dtype=torch.uint8)
    bits = ((cw[:, :, None] >> shifts) & 1).reshape(n, W * M)
    sigma = math.sqrt(1.0 / (2.0 * (SIZE / W) * 10.0 ** (ebn0 / 10.0)))
    y = (1.0 - 2.0 * bits.float()) + sigma * torch.randn((n, W * M), device=dev, generator=g)
    return cw, torch.clamp(torch.round(SCALE * y), -127, 127).to(torch.int8)


def hard_rows(llr):
    n = llr.shape[0]
    w = (1 << torch.arange(M - 1, -1, -1, device=llr.device)).to(torch.uint8)
    return ((llr.view(n, W, M) < 0).to(torch.uint8) * w).sum(2, dtype=torch.uint8)


def torch_candidates(llr, hard, flips, cand):
    """cand[n, P, W] <- the hard rows with the picked bits flipped"""
    n, np_ = llr.shape[0], 1 << flips
    cand.copy_(hard[:, None, :].expand(n, np_, W))
    if not flips:
        return
    key = llr.to(torch.int32).abs() * 4096 + torch.arange(W * M, device=llr.device, dtype=torch.int32)
    pick = key.topk(flips, dim=1, largest=False, sorted=True).indices
    rows = torch.arange(n, device=llr.device)[:, None]
    ps = torch.arange(np_, device=llr.device)
    for k in range(flips):
        sym = (pick[:, k] // M)[:, None].expand(n, np_)
        val = (1 << (M - 1 - pick[:, k] % M)).to(torch.uint8)[:, None] * ((ps >> k) & 1).to(torch.uint8)[None, :]
        cand[rows, ps[None, :], sym] ^= val


def torch_select(llr, hard, cand, cok):
    """(ok, rows, pattern, score) from the decoded candidates"""
    n, np_ = cand.shape[0], cand.shape[1]
    mag = llr.to(torch.int16).abs().view(n, W, M)
    diff = cand ^ hard[:, None, :]
    score = torch.zeros((n, np_), dtype=torch.int32, device=llr.device)
    for j in range(M):
        bit = ((diff >> (M - 1 - j)) & 1).to(torch.int16)
        score += (bit * mag[:, None, :, j]).sum(2, dtype=torch.int32)
    key = torch.where(cok.view(n, np_) != 0, score * 64 + torch.arange(np_, device=llr.device, dtype=torch.int32),
                      torch.full_like(score, 0x7FFFFFFF))
    best = key.min(1).values
    ok = best != 0x7FFFFFFF
    p = torch.where(ok, best & 63, torch.zeros_like(best))
    rows = torch.where(ok[:, None], cand[torch.arange(n, device=llr.device), p.long()], hard)
    return ok.to(torch.uint8), rows, p.to(torch.uint8), torch.where(ok, best >> 6, torch.zeros_like(best))


def run(h, cw, llr, flips, steps, warmup, base_ok):
    dev, n, np_ = llr.device, llr.shape[0], 1 << flips
    s = torch.cuda.current_stream().cuda_stream
    hard = hard_rows(llr)
    rows = torch.empty((n, W), dtype=torch.uint8, device=dev)
    out = torch.zeros((3, n), dtype=torch.uint8, device=dev)
    score = torch.zeros((n,), dtype=torch.int32, device=dev)
    work = torch.empty_like(hard)
    hok = torch.zeros((n,), dtype=torch.uint8, device=dev)
    cand = torch.empty((n, np_, W), dtype=torch.uint8, device=dev)
    cok = torch.zeros((n * np_,), dtype=torch.uint8, device=dev)
    ready = torch.empty_like(cand)
    torch_candidates(llr, hard, flips, ready)
    h.reserve_soft(flips, n)
    h.reserve_interleaved(n * np_)  # the row decodes' workspace for the floor and the torch route

    def soft():
        h.decode_soft_batch_device(llr.data_ptr(), W * M, rows.data_ptr(), W, rows.data_ptr() + SIZE, W, SIZE, n,
                                   flips, out[0].data_ptr(), changed_ptr=out[1].data_ptr(),
                                   pattern_ptr=out[2].data_ptr(), score_ptr=score.data_ptr(), stream=s)

    def plain(buf, count, okbuf):
        h.decode_batch_device(buf.data_ptr(), W, buf.data_ptr() + SIZE, W, SIZE, count, okbuf.data_ptr(), stream=s)

    res = {}

    def torch_route():
        torch_candidates(llr, hard, flips, cand)
        plain(cand, n * np_, cok)
        res["torch"] = torch_select(llr, hard, cand, cok)

    wall = {"soft": [], "hard": [], "floor": [], "torch": []}
    for step in range(warmup + steps):
        t = {"soft": timed(soft)}
        work.copy_(hard)
        t["hard"] = timed(lambda: plain(work, n, hok))
        cand.copy_(ready)
        t["floor"] = timed(lambda: plain(cand, n * np_, cok))
        t["torch"] = timed(torch_route)
        if step >= warmup:
            for k, v in t.items():
                wall[k].append(v)
    tok, trows, tp, tscore = res["torch"]
    agree = bool(torch.equal(tok, out[0]) and torch.equal(trows, rows) and torch.equal(tp, out[2]) and
                 torch.equal(tscore, score))
    kern = {}
    h.timing(True)
    for _ in range(steps):
        soft()
        torch.cuda.synchronize()
        for k in range(29):
            ms, cnt = h.timing_read(k)
            if cnt:
                kern.setdefault(k, []).append(ms * 1e3)
        h.timing(True)
    fkern = {}
    for _ in range(steps):
        cand.copy_(ready)
        h.timing(True)
        plain(cand, n * np_, cok)
        torch.cuda.synchronize()
        for k in range(29):
            ms, cnt = h.timing_read(k)
            if cnt:
                fkern.setdefault(k, []).append(ms * 1e3)
    h.timing(False)
    ok = out[0] != 0
    exact = ok & (rows == cw).all(1)
    line = {"flips": flips, "codewords": n, "candidate_rows": n * np_, "steps": steps,
            "event_us": {k: stats(v) for k, v in wall.items()},
            "kernel_us": {str(k): stats(v) for k, v in sorted(kern.items())},
            "floor_kernel_us": {str(k): stats(v) for k, v in sorted(fkern.items())},
            "recovered": int(exact.sum()), "accepted_wrong": int((ok & ~exact).sum()), "failed": int((~ok).sum()),
            "recovered_beyond_flips_0": None if base_ok is None else int((exact & ~base_ok).sum()),
            "call_equals_torch_route": agree,
            "soft_over_floor": round(stats(wall["soft"])["median"] / stats(wall["floor"])["median"], 3),
            "torch_over_soft": round(stats(wall["torch"])["median"] / stats(wall["soft"])["median"], 3)}
    return line, exact


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--count", type=int, default=1 << 16)
    ap.add_argument("--ebn0", type=float, default=5.6)
    ap.add_argument("--flips", default="0,2,4,6")
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "soft_bench needs a GPU"
    dev = torch.device("cuda", 0)
    h = P.Poporon(*PARAMS, device=0)
    cw, llr = make_llr(h, a.count, a.ebn0, dev, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    base = None
    for flips in [int(f) for f in a.flips.split(",")]:
        line, exact = run(h, cw, llr, flips, a.steps, a.warmup, base)
        if flips == 0:
            base = exact
        line = dict({"code": "RS(255,223)", "ebn0_db": a.ebn0, "llr": "rint(32 y) clipped to +-127"}, **line)
        print(json.dumps(line), flush=True)
        if a.append:
            with open(a.append, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()
    h.close()


if __name__ == "__main__":
    main()
