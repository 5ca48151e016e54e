#!/usr/bin/env python3
"""Generate tests/golden/ldpc_sweep_golden.npz by running the REAL reference's LDPC
codec on the sweep codes (tests/ldpc_ref.py: SWEEP), the way tools/gen_golden_ldpc.py
does for codes A-M; tests/golden/ldpc_golden.npz is not touched.

Per code <X>, from seeded inputs that tests/ldpc_ref.py rebuilds:

  <X>_dims        parity_bytes, info_bytes, num_checks, num_bits, num_edges
  <X>_graph_sha   SHA-256 of row_ptr, col_idx, inner_forward, outer_forward (uint32; "" when off)
  <X>_in_sha      SHA-256 of the messages, the one-flip rows, the hard rows, the LLRs and the
                  junk data / parity of the soft rows
  <X>_enc_sha     SHA-256 of data' and parity of the encoded messages
  <X>_chk_dirty   poporon_ldpc_check on the encoded rows with one bit flipped
  <X>_hard_*      ok, corrected_num (sentinel 777 in), iterations_used in full;
                  <X>_hard_sha: SHA-256 of data' and of the decoder's codeword buffer
  <X>_soft_*      the same for the 22 soft rows
  <X>_edge_*      where the code has a check row with a single edge: the same for LLR rows that
                  balance that edge's bit against the row's message (<X>_edge_sha: LLRs, data', buffer)

and asserts, from the reference alone, what the tests rely on: every sweep code is
served (its inner table is a permutation), every hard row set holds a failed row and
rows leaving at iteration 0, 1 and >= 3, every soft row set holds both outcomes, the
refused variant of W340 is no permutation, and one sweep code has a check row with a
single edge.

Run where the reference's sources are present:  python tools/gen_golden_ldpc_sweep.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ldpc_ref as R  # noqa: E402
from gen_golden_ldpc import decode_rows, encode_rows  # noqa: E402


def graph_sha(g):
    return np.array([R.sha(g[k].astype(np.uint32)) if g[k] is not None else ""
                     for k in ("row_ptr", "col_idx", "inner_forward", "outer_forward")])


def is_permutation(table):
    return table is None or np.unique(table).size == table.size


def main():
    if not R.reference_available():
        sys.exit("oracle/_ref/libpoporon_ref.so missing: run `make -C oracle` where the reference's sources are")
    out = {}
    single_edge = []
    for name, code in R.SWEEP.items():
        ref = R.RefLdpc(code)
        g = ref.graph()
        assert is_permutation(g["inner_forward"]), f"{name}: the inner table is no permutation, the code is not served"
        out[name + "_dims"] = np.array([ref.parity_bytes, ref.info_bytes, g["num_checks"], g["num_bits"],
                                        g["num_edges"]], np.uint32)
        out[name + "_graph_sha"] = graph_sha(g)
        degree = np.diff(g["row_ptr"].astype(np.int64))
        if (degree == 1).any():
            single_edge.append(name)
        msgs = R.sweep_enc_inputs(name)
        enc_d, enc_p = encode_rows(ref, msgs)
        out[name + "_enc_sha"] = np.array([R.sha(enc_d), R.sha(enc_p)])
        fd, fp = R.sweep_flip_one(name, enc_d, enc_p, ref.codeword_bits)
        assert not any(ref.dirty(enc_d[i], enc_p[i]) for i in range(len(msgs)))
        out[name + "_chk_dirty"] = np.array([ref.dirty(fd[i], fp[i]) for i in range(len(fd))], np.uint8)
        src, din, pin, nf = R.sweep_hard_rows(name, enc_d, enc_p)
        ok, cor, it, dout, hard = decode_rows(ref, din, pin)
        out[name + "_hard_ok"], out[name + "_hard_cor"], out[name + "_hard_iter"] = ok, cor, it
        out[name + "_hard_sha"] = np.array([R.sha(dout), R.sha(hard)])
        won = it[ok == 1]
        summary = f"{name}: {int(g['num_bits'])} bits, {int(g['num_edges'])} edges, row degree {degree.min()}.." \
            f"{degree.max()}; hard ok by flips " + ", ".join(
                f"{f}:{int(ok[nf == f].sum())}" for f in sorted(set(nf.tolist()))) + f"; iterations {sorted(set(won.tolist()))}"
        assert (ok == 0).any() and (won == 0).any() and (won == 1).any() and (won >= 3).any(), summary
        assert (cor[ok == 0] == R.SENT).all() and (it[ok == 0] == R.MAX_ITER).all() and (cor[ok == 1] == won).all()
        ref.close()
        rs = R.RefLdpc(code, soft=True)
        llr, jd, jp = R.sweep_soft_rows(name, enc_d, enc_p, rs.codeword_bits)
        ok, cor, it, dout, hard = decode_rows(rs, jd, jp, llr)
        out[name + "_soft_ok"], out[name + "_soft_cor"], out[name + "_soft_iter"] = ok, cor, it
        out[name + "_soft_sha"] = np.array([R.sha(dout), R.sha(hard)])
        assert (ok == 0).any() and (ok == 1).any(), summary
        # all 0 and all 127 decode to the zero codeword at iteration 1, all -128 fails
        assert (ok[16], it[16], ok[17], ok[18], it[18]) == (1, 1, 0, 1, 1), summary
        summary += f"; soft ok {int(ok.sum())}/{len(ok)}"
        if (degree == 1).any():
            # the bit on a single-edge check row balanced against the +30000 that row sends it
            el = R.sweep_single_edge_rows(g)
            ed, ep = np.full((len(el), ref.info_bytes), 0x5A, np.uint8), np.full((len(el), ref.parity_bytes), 0xC3, np.uint8)
            ok, cor, it, dout, hard = decode_rows(rs, ed, ep, el)
            out[name + "_edge_ok"], out[name + "_edge_cor"], out[name + "_edge_iter"] = ok, cor, it
            out[name + "_edge_sha"] = np.array([R.sha(el), R.sha(dout), R.sha(hard)])
            assert (ok == 0).any() and (it[ok == 1] == 1).any() and (it[ok == 1] > 1).any(), (ok, it)
            summary += f"; single-edge rows ok {ok.tolist()} iterations {it.tolist()}"
        rs.close()
        out[name + "_in_sha"] = np.array([R.sha(msgs), R.sha(np.concatenate([fd, fp], axis=1)),
                                          R.sha(np.concatenate([din, pin], axis=1)), R.sha(llr), R.sha(jd), R.sha(jp)])
        print(summary, flush=True)
    assert single_edge, "no sweep code has a check row with a single edge: pick a seed of W848 that gives one"
    print("check rows with a single edge:", ", ".join(single_edge))
    ref = R.RefLdpc(R.SWEEP_REFUSED)
    g = ref.graph()
    assert not is_permutation(g["inner_forward"]), "W340 with the automatic depth was meant to be refused"
    out["refused_dims"] = np.array([ref.parity_bytes, ref.info_bytes, g["num_checks"], g["num_bits"], g["num_edges"]],
                                   np.uint32)
    out["refused_graph_sha"] = graph_sha(g)
    ref.close()
    np.savez_compressed(R.SWEEP_GOLDEN, **out)
    print(R.SWEEP_GOLDEN, os.path.getsize(R.SWEEP_GOLDEN), "bytes")


if __name__ == "__main__":
    main()
