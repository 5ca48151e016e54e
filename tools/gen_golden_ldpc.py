#!/usr/bin/env python3
"""Generate tests/golden/ldpc_golden.npz by running the REAL reference's LDPC codec.

``oracle/_ref/libpoporon_ref.so`` (compiled from the reference's sources by
oracle/Makefile) is driven through poporon_ldpc_config_create / poporon_create /
poporon_encode / poporon_decode (tests/ldpc_ref.py: RefLdpc).  Inputs come from
seeded numpy Generators (tests/ldpc_ref.py) and are recorded as SHA-256 only;
the reference's outputs are recorded in full or as an XOR against a row the
test can rebuild (so that correct decodes compress to nothing):

  getters           (block, rate, parity_bytes, info_bytes) for 3 blocks x 6 rates
  <X>_row_ptr ...   the graph of codes A-F, M (G: SHA-256 of each array)
  <X>_enc_*         257 encoded rows: parity, and the data where an interleaver rewrites it
  <X>_chk_dirty     poporon_ldpc_check on those rows with one bit flipped
  <X>_hard_*        384 received rows (0/1/2/4/8/16 flips x 64): ok, corrected_num (sentinel
                    777 in), iterations_used, data' ^ message, codeword buffer ^ clean codeword
  <X>_soft_*        A, C, F: 3 sigmas x 64 rows + 16 uniform rows: ok, iterations, data', buffer
  A_it0_* / A_it1_* max_iterations 0 (= 50) and 1 on A's 8- and 16-flip rows
  G_*               2 rows of the largest code, 3 iterations at most, as SHA-256

Run where the reference's sources are present:  python tools/gen_golden_ldpc.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ldpc_ref as R  # noqa: E402


def record_graph(out, name, ref, hashed=False):
    g = ref.graph()
    out[name + "_dims"] = np.array([ref.parity_bytes, ref.info_bytes, g["num_checks"], g["num_bits"], g["num_edges"]],
                                   np.uint32)
    for k in ("row_ptr", "col_idx", "inner_forward", "outer_forward"):
        if g[k] is not None:
            out[f"{name}_{k}"] = np.array(R.sha(g[k].astype(np.uint32))) if hashed else g[k].astype(np.uint32)
    return g


def encode_rows(ref, data):
    dd, pp = np.zeros_like(data), np.zeros((data.shape[0], ref.parity_bytes), np.uint8)
    for i in range(data.shape[0]):
        dd[i], pp[i] = ref.encode(data[i])
    return dd, pp


def decode_rows(ref, data, parity, llr=None):
    n = data.shape[0]
    ok, cor, it = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    dout, hard = np.zeros_like(data), np.zeros((n, ref.codeword_bytes), np.uint8)
    for i in range(n):
        if llr is not None:
            ref.set_llr(llr[i])
        ok[i], cor[i], it[i], dout[i], hard[i] = ref.decode(data[i], parity[i])
    return ok, cor, it, dout, hard


def record_hard(out, pre, ref, g, msgs, enc_d, enc_p, src, din, pin):
    ok, cor, it, dout, hard = decode_rows(ref, din, pin)
    clean = R.deinterleave(np.concatenate([enc_d, enc_p], axis=1), g["inner_forward"], ref.codeword_bits)
    out[pre + "in_sha"] = np.array(R.sha(np.concatenate([din, pin], axis=1)))
    out[pre + "ok"], out[pre + "cor"], out[pre + "iter"] = ok, cor, it
    out[pre + "data_x"] = dout ^ msgs[src]
    out[pre + "hard_x"] = hard ^ clean[src]
    return ok, it


def main():
    if not R.reference_available():
        sys.exit("oracle/_ref/libpoporon_ref.so missing: run `make -C oracle` where the reference's sources are")
    out = {}
    get = []
    for block in (32, 36, 8192):
        for rate in range(6):
            ref = R.RefLdpc(dict(R.CODES["A"], block=block, rate=rate))
            get.append((block, rate) + ref.getters())
            ref.close()
    out["getters"] = np.array(get, np.uint32)

    for name in R.SMALL + "M":
        code = R.CODES[name]
        ref = R.RefLdpc(code)
        g = record_graph(out, name, ref)
        rows = R.ENC_ROWS if name != "M" else 8
        msgs = R.enc_inputs(name, rows)
        enc_d, enc_p = encode_rows(ref, msgs)
        out[name + "_enc_in_sha"] = np.array(R.sha(msgs))
        out[name + "_enc_parity"] = enc_p
        if code["inner"] or code["outer"]:
            out[name + "_enc_data"] = enc_d
        else:
            assert (enc_d == msgs).all()
        # one flipped bit per row
        bits = np.random.default_rng([ord(name), 20]).integers(0, 8 * ref.codeword_bytes, rows)
        dirty = np.zeros(rows, np.uint8)
        for i in range(rows):
            assert not ref.dirty(enc_d[i], enc_p[i])
            d, p = R.apply_flips(enc_d[i], enc_p[i], [int(bits[i])])
            dirty[i] = ref.dirty(d, p)
        out[name + "_chk_dirty"] = dirty
        # hard path
        if name == "M":
            src, din, pin, nf = R.flip_rows(enc_d, enc_p, flips=(0, 4, 40, 400), per=2)
        else:
            src, din, pin, nf = R.flip_rows(enc_d, enc_p)
        ok, it = record_hard(out, name + "_hard_", ref, g, msgs, enc_d, enc_p, src, din, pin)
        summary = f"{name}: {int(g['num_edges'])} edges; hard ok by flips " + ", ".join(
            f"{f}:{int(ok[nf == f].sum())}" for f in sorted(set(nf.tolist()))) + f"; iterations {sorted(set(it.tolist()))}"
        if name != "M":
            # the row set the GPU tests rely on
            assert (ok == 0).any() and (it[ok == 1] == 0).any() and (it[ok == 1] == 1).any() and \
                (it[ok == 1] >= 3).any(), summary
        ref.close()
        if name == "A":
            sel = nf >= 8
            for mi in (0, 1):
                r2 = R.RefLdpc(code, max_iterations=mi)
                ok2, it2 = record_hard(out, f"A_it{mi}_", r2, g, msgs, enc_d, enc_p, src[sel], din[sel], pin[sel])
                assert (ok2 == 0).any() and set(it2[ok2 == 0].tolist()) == {50 if mi == 0 else 1}
                r2.close()
        if name in R.SOFT:
            rs = R.RefLdpc(code, soft=True)
            llr, jd, jp = R.soft_rows(name, enc_d, enc_p, rs.codeword_bits)
            ok, cor, it, dout, hard = decode_rows(rs, jd, jp, llr)
            out[name + "_soft_in_sha"] = np.array(R.sha(llr) + R.sha(jd) + R.sha(jp))
            out[name + "_soft_ok"], out[name + "_soft_cor"], out[name + "_soft_iter"] = ok, cor, it
            out[name + "_soft_data"], out[name + "_soft_hard"] = dout, hard
            summary += "; soft ok " + "/".join(str(int(ok[i * 64:(i + 1) * 64].sum())) for i in range(3)) + \
                f" + {int(ok[192:].sum())}/16"
            rs.close()
        print(summary, flush=True)

    # G: the largest code, 2 rows, at most 3 iterations
    ref = R.RefLdpc(R.CODES["G"], max_iterations=3)
    g = record_graph(out, "G", ref, hashed=True)
    msgs, flips = R.g_inputs()
    enc_d, enc_p = encode_rows(ref, msgs)
    out["G_enc_in_sha"] = np.array(R.sha(msgs))
    out["G_enc_parity_sha"] = np.array(R.sha(enc_p))
    rx = [R.apply_flips(enc_d[i], enc_p[i], flips[i]) for i in range(2)]
    din, pin = np.stack([r[0] for r in rx]), np.stack([r[1] for r in rx])
    out["G_chk_dirty"] = np.array([ref.dirty(din[i], pin[i]) for i in range(2)], np.uint8)
    ok, cor, it, dout, hard = decode_rows(ref, din, pin)
    out["G_hard_ok"], out["G_hard_cor"], out["G_hard_iter"] = ok, cor, it
    out["G_hard_data_sha"] = np.array([R.sha(dout[i]) for i in range(2)])
    out["G_hard_hard_sha"] = np.array([R.sha(hard[i]) for i in range(2)])
    print(f"G: {g['num_edges']} edges; ok {ok.tolist()} iterations {it.tolist()}", flush=True)
    ref.close()

    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
