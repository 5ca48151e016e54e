"""The refusal table of the RS layout forms (interleaved, report, conv, planes, strided planes, product,
the reserve calls, the mask lists and the wire-form handle check).

Every form checks its arguments before it touches the GPU and says what is wrong through
poporon_amd_last_error().  The texts, and which text wins when two arguments are wrong at once, are part
of the interface: tests/golden/form_refusals.json holds, per case, the entry point, the kind of handle,
the argument tuple, the return value and the text.  It was recorded by this module's __main__ block at
commit 2cc3cac ("Add RS product-code blocks: encode, scheduled decode and check"), before the forms'
host code was folded into one driver, and never from the code under test.  The test replays the table
against the built library and compares byte for byte.

An argument tuple follows the C signature behind the handle: integers as they are; a pointer as 0 (NULL)
or 1 (a non-NULL address that no refusal dereferences); a plane table as {"planes": W, "null": [...]}
and a lost list as {"lost": [...]}, the two host arrays the plane checks do read.

Per entry point there is one case per refusal of its argument checks (ilv_args, rep_args,
decode_row_args, conv_args, plane_args, plane_strided, prod_args), the count-0 return, and a handful with
two arguments wrong at once.  Left out, since they are reached only after gpu_init and so need a device:
  * whatever a call with valid arguments and count > 0 answers (HIP failures, "no HIP device available");
  * the reserve calls behind their handle checks (poporon_amd_reserve_interleaved / _report / _planes,
    poporon_amd_product_reserve behind its shape check);
  * "RS parameters not served by the GPU kernels" (gpu_init_steps).
No case may pass the argument checks with count > 0: on a machine with a device the dummy pointers
would then be read.  The recorder and the test both refuse a table with a text from behind gpu_init.
"""
import ctypes as C
import json
import os

import pytest

import libpoporon_amd as P

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "form_refusals.json")
X = 0x1000  # a non-NULL pointer that is never dereferenced
INTS = (C.c_size_t, C.c_int, C.c_bool)
RS15 = (4, 0x13, 1, 1, 4)

# ---- the entry points: parameter names behind the handle, and a base tuple that would pass ----------------

ILV = dict(data=1, ds=892, par=1, ps=128, size=223, depth=4, count=3)
ERA = dict(pos=0, pstride=0, cnt=0)
REP = dict(num=1, epos=1, eval=1, rstride=32)
ROW = dict(data=1, ds=255, par=1, ps=255, size=223, count=3)
CONV = dict(branches=3, cell=2, phase=1)
PLN = dict(planes={"planes": 14, "null": []}, size=10, count=4)
LOST = dict(lost={"lost": []}, nlost=0)
STR = dict(data=1, ds=64, par=1, ps=64, size=10, count=4)
PROD = dict(blocks=1, pitch=15, bstride=225, k1=11, k2=11, count=2)
SCHED = dict(first_axis=0, passes=3, couple=1)
FLAGS = dict(rd=1, cd=1, bok=1)

ENTRY = {  # name: (handle kind of the base case, ordered parameters)
    "poporon_encode_interleaved_device": ("rs255", {**ILV, "stream": 0}),
    "poporon_decode_interleaved_device": ("rs255", {**ILV, **ERA, "ok": 1, "cor": 0, "stream": 0}),
    "poporon_check_interleaved_device": ("rs255", {**ILV, "dirty": 1, "stream": 0}),
    "poporon_encode_interleaved": ("rs255", {**ILV}),
    "poporon_decode_interleaved": ("rs255", {**ILV, **ERA, "ok": 1, "cor": 0}),
    "poporon_decode_interleaved_report_device": ("rs255", {**ILV, **ERA, "ok": 1, "cor": 0, **REP, "stream": 0}),
    "poporon_decode_batch_report_device": ("rs255", {**ROW, **ERA, "ok": 1, "cor": 0, **REP, "stream": 0}),
    "poporon_decode_batch_report": ("rs255", {**ROW, **ERA, "ok": 1, "cor": 0, **REP}),
    "poporon_amd_erasures_from_mask_device": ("rs255", dict(mask=1, mstride=892, size=223, depth=4, count=3, pos=1,
                                                            pstride=32, cnt=1, over=0, stream=0)),
    "poporon_amd_conv_interleave_device": ("rs255", {**ROW, **CONV, "cstream": 1, "stream": 0}),
    "poporon_amd_conv_deinterleave_device": ("rs255", {"cstream": 1, **CONV, **ROW, "stream": 0}),
    "poporon_encode_conv_device": ("rs255", {**ROW, **CONV, "cstream": 1, "stream": 0}),
    "poporon_decode_conv_device": ("rs255", {"cstream": 1, **CONV, **ROW, **ERA, "ok": 1, "cor": 0, "stream": 0}),
    "poporon_decode_conv_report_device": ("rs255", {"cstream": 1, **CONV, **ROW, **ERA, "ok": 1, "cor": 0, **REP,
                                                    "stream": 0}),
    "poporon_check_conv_device": ("rs255", {"cstream": 1, **CONV, "size": 223, "count": 3, "dirty": 1, "stream": 0}),
    "poporon_encode_planes_device": ("rs14", {**PLN, "stream": 0}),
    "poporon_decode_planes_device": ("rs14", {**PLN, **LOST, "ok": 1, "cor": 0, "dirty": 0, "stream": 0}),
    "poporon_decode_planes_report_device": ("rs14", {**PLN, **LOST, "ok": 1, "cor": 0, "dirty": 0, **REP,
                                                     "rstride": 4, "stream": 0}),
    "poporon_check_planes_device": ("rs14", {**PLN, "dirty": 1, "stream": 0}),
    "poporon_encode_planes_strided_device": ("rs14", {**STR, "stream": 0}),
    "poporon_decode_planes_strided_device": ("rs14", {**STR, **LOST, "ok": 1, "cor": 0, "dirty": 0, "stream": 0}),
    "poporon_check_planes_strided_device": ("rs14", {**STR, "dirty": 1, "stream": 0}),
    "poporon_encode_product_device": ("prod", {**PROD, "stream": 0}),
    "poporon_decode_product_device": ("prod", {**PROD, **SCHED, **FLAGS, "stream": 0}),
    "poporon_check_product_device": ("prod", {**PROD, **FLAGS, "stream": 0}),
    "poporon_encode_product": ("prod", {**PROD}),
    "poporon_decode_product": ("prod", {**PROD, **SCHED, **FLAGS}),
    "poporon_amd_product_reserve": ("prod", dict(k1=11, k2=11, max_blocks=4)),
    "poporon_amd_reserve_interleaved": ("rs255", dict(max_codewords=10)),
    "poporon_amd_reserve_report": ("rs255", dict(max_codewords=10)),
    "poporon_amd_reserve_planes": ("rs255", dict(max_codewords=10)),
    "poporon_amd_set_wire_form_ccsds": ("rs255", dict(dual=1, rand=1)),
    "poporon_amd_get_wire_form": ("rs255", dict(to_code=0, to_wire=0, seq=0, cap=0, n=0)),
}

BIG = (1 << 64) - 1

# refusals by the parameters a call has: (parameters it needs, the overrides); a handle kind under "h"
MUTATIONS = [
    ((), dict(h="null")),
    ((), dict(h="bch")),
    ((), dict(h="ldpc")),
    # ---- rows, frames and their strides
    (("data",), dict(data=0)),
    (("par",), dict(par=0)),
    (("ok",), dict(ok=0)),
    (("dirty", "size"), dict(dirty=0)),
    (("depth",), dict(depth=0)),
    (("depth",), dict(depth=65)),
    (("size",), dict(size=0)),
    (("size",), dict(size=252)),
    (("size",), dict(size=252, count=0)),
    (("depth", "ds"), dict(ds=891)),
    (("depth", "ps"), dict(ps=127)),
    (("mstride",), dict(mstride=891)),
    (("mask",), dict(mask=0)),
    (("mask",), dict(pstride=31)),
    (("cnt",), dict(pos=1, pstride=32, cnt=0)),
    (("cnt", "ok"), dict(pos=1, pstride=3, cnt=1)),
    (("count",), dict(count=0)),
    (("count", "data"), dict(count=0, data=0, par=0)),
    # ---- report arrays
    (("num",), dict(num=0)),
    (("num",), dict(eval=0)),
    (("num",), dict(rstride=3)),
    (("num",), dict(num=0, count=0)),
    (("num",), dict(rstride=3, count=0)),
    # ---- convolutional streams
    (("cstream",), dict(cstream=0)),
    (("cstream",), dict(branches=0)),
    (("cstream",), dict(branches=129, phase=0)),
    (("cstream",), dict(cell=0)),
    (("cstream",), dict(cell=256)),
    (("cstream",), dict(phase=3)),
    (("cstream", "ds"), dict(ds=222)),
    (("cstream", "ps"), dict(ps=31)),
    (("cstream",), dict(count=1 << 62)),
    (("cstream",), dict(h="rs255_tile", branches=64, cell=64)),
    # ---- planes
    (("planes",), dict(planes=0)),
    (("planes",), dict(planes={"planes": 14, "null": [3]})),
    (("planes",), dict(planes={"planes": 14, "null": [12]})),
    (("planes",), dict(planes={"planes": 14, "null": [10, 11, 12, 13]})),
    (("lost",), dict(lost={"lost": [5, 2]}, nlost=2)),
    (("lost",), dict(lost={"lost": [2, 2]}, nlost=2)),
    (("lost",), dict(lost={"lost": [3, 14]}, nlost=2)),
    (("lost",), dict(lost={"lost": [0, 1, 2, 3, 4]}, nlost=5)),
    (("lost",), dict(lost=0, nlost=2)),
    (("lost",), dict(lost={"lost": [5, 2]}, nlost=2, count=0)),
    (("lost", "planes"), dict(planes={"planes": 14, "null": [3]}, lost={"lost": [4]}, nlost=1)),
    # ---- product blocks
    (("k1",), dict(k1=0)),
    (("k1",), dict(k1=12)),
    (("k2",), dict(k2=0)),
    (("k2",), dict(k2=12)),
    (("pitch",), dict(pitch=14)),
    (("pitch",), dict(bstride=224)),
    (("pitch",), dict(pitch=BIG // 8)),
    (("first_axis",), dict(first_axis=2)),
    (("first_axis",), dict(passes=0)),
    (("first_axis",), dict(passes=17)),
    (("rd",), dict(rd=0, cd=0, bok=0)),
    (("blocks",), dict(blocks=0)),
    (("blocks",), dict(bstride=BIG // 4, count=8)),
    (("blocks",), dict(count=0, blocks=0)),
    # ---- the wire form's handle
    (("dual",), dict(h="rs15")),
    (("to_code",), dict(h="rs15")),
    (("to_code",), dict()),  # no wire form is set
    # ---- two arguments wrong at once: which text wins
    (("depth",), dict(depth=0, size=0)),
    (("depth",), dict(data=0, depth=0)),
    (("depth",), dict(ds=891, ps=127)),
    (("depth",), dict(size=0, ds=0)),
    (("depth",), dict(h="null", depth=0, size=0)),
    (("depth", "num"), dict(size=0, num=0)),
    (("depth", "num"), dict(depth=0, rstride=3)),
    (("num", "ok"), dict(ok=0, num=0)),
    (("num", "size"), dict(size=0, rstride=3)),
    (("cstream",), dict(branches=0, phase=0, cell=0)),
    (("cstream",), dict(phase=5, size=0)),
    (("cstream", "ok"), dict(ok=0, size=0)),
    (("cstream", "ok"), dict(ok=0, cstream=0)),
    (("cstream", "dirty"), dict(dirty=0, phase=3)),
    (("cstream", "num"), dict(num=0, ok=0)),
    (("planes", "size"), dict(size=0, planes=0)),
    (("lost", "planes"), dict(lost={"lost": [5, 2]}, nlost=2, planes=0)),
    (("lost", "ok"), dict(ok=0, lost={"lost": [3, 14]}, nlost=2)),
    (("planes", "num"), dict(size=0, num=0)),
    (("planes", "num"), dict(planes=0, rstride=3)),
    (("planes", "num"), dict(h="bch", num=0)),
    (("lost", "data"), dict(data=0, lost={"lost": [5, 2]}, nlost=2)),
    (("lost", "data"), dict(size=0, data=0)),
    (("k1",), dict(k1=0, k2=0)),
    (("pitch",), dict(pitch=14, bstride=0)),
    (("first_axis",), dict(first_axis=2, passes=0, rd=0, cd=0, bok=0)),
    (("rd",), dict(rd=0, cd=0, bok=0, blocks=0)),
    (("blocks",), dict(h="prod_null", k1=0)),
]


# optional arguments: these overrides pass the checks and go on to the GPU, so they are not cases
OPTIONAL = [("poporon_amd_conv_interleave_device", dict(par=0)), ("poporon_amd_conv_deinterleave_device", dict(par=0)),
            ("poporon_encode_planes_device", dict(planes={"planes": 14, "null": [12]})),
            ("poporon_decode_planes_device", dict(dirty=0)), ("poporon_decode_planes_report_device", dict(dirty=0)),
            ("poporon_decode_planes_strided_device", dict(dirty=0))]


def cases():
    """[(entry point, handle kind, argument list)] of every mutation an entry point has the parameters for"""
    out = []
    for fn, (kind, base) in ENTRY.items():
        for need, over in MUTATIONS:
            if (fn, over) in OPTIONAL:
                continue
            over = dict(over)
            h = over.pop("h", kind)
            if not all(k in base for k in need) or not all(k in base for k in over):
                continue
            if kind == "prod":
                if h in ("bch", "ldpc", "rs15", "rs255_tile"):
                    continue
                h = {"null": "prod_null"}.get(h, h)
            elif h == "prod_null":
                continue
            if not over and h == kind and fn != "poporon_amd_get_wire_form":
                continue
            args = [{**base, **over}[k] for k in base]
            if (fn, h, args) not in out:
                out.append((fn, h, args))
    return out


def _handles(env_set, env_del):
    """kind -> (object kept alive, the pointer passed)"""
    hs = {"null": (None, None), "prod_null": (None, None)}
    for kind, make in (("rs255", P.Poporon.default), ("rs14", lambda: P.Poporon(8, 0x11D, 1, 1, 4)),
                       ("rs15", lambda: P.Poporon(*RS15)), ("bch", P.Bch.default),
                       ("ldpc", lambda: P.Ldpc(32, P.LDPC_RATE_1_2)), ("prod", lambda: P.Product(RS15, RS15))):
        o = make()
        hs[kind] = (o, o.h)
    env_set("POPORON_AMD_CONV_PATH", "tile")  # read at poporon_create
    try:
        o = P.Poporon.default()
    finally:
        env_del("POPORON_AMD_CONV_PATH")
    hs["rs255_tile"] = (o, o.h)
    return hs


def call(hs, fn, kind, args):
    """(return value, last_error() after a false return or None)"""
    keep, cargs = [], []
    types = P._SIGS[fn][1][1:]
    assert len(types) == len(args), fn
    for t, a in zip(types, args):
        if t in INTS:
            cargs.append(a)
        elif isinstance(a, dict) and "planes" in a:
            keep.append((C.c_void_p * a["planes"])(*[None if j in a["null"] else X + 0x100 * j
                                                     for j in range(a["planes"])]))
            cargs.append(keep[-1])
        elif isinstance(a, dict):
            keep.append((C.c_uint8 * max(1, len(a["lost"])))(*a["lost"]))
            cargs.append(keep[-1])
        else:
            assert a in (0, 1), (fn, a)
            cargs.append(C.cast(X, t) if a and t is not C.c_void_p else (X if a else None))
    ret = bool(getattr(P.load_library(), fn)(hs[kind][1], *cargs))
    return ret, (None if ret else P.last_error())


def _behind_gpu_init(text):
    return text is not None and ("HIP" in text or "GPU kernels" in text)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_table_covers_every_case(recorded):
    have = [(c["fn"], c["handle"], c["args"]) for c in recorded["cases"]]
    assert have == cases()
    assert {c["fn"] for c in recorded["cases"]} == set(ENTRY)
    assert not [c for c in recorded["cases"] if _behind_gpu_init(c["error"])]
    # nothing recorded passes the checks with work to do: a true return is a count-0 call
    for c in recorded["cases"]:
        if c["ret"]:
            names = list(ENTRY[c["fn"]][1])
            assert c["args"][names.index("count")] == 0, c


def test_refusals_replay(recorded, monkeypatch):
    hs = _handles(monkeypatch.setenv, monkeypatch.delenv)
    wrong = []
    for c in recorded["cases"]:
        got = call(hs, c["fn"], c["handle"], c["args"])
        if got != (c["ret"], c["error"]):
            wrong.append((c["fn"], c["handle"], c["args"], got, (c["ret"], c["error"])))
    assert not wrong, f"(entry point, handle, arguments, answered, recorded): {wrong[:8]} ({len(wrong)} in all)"


if __name__ == "__main__":
    # recorder, run from the repository root at the commit whose texts are the record:
    #   PYTHONPATH=.:tests python tests/test_form_refusals_cpu.py COMMIT [OUT]
    import sys

    hs_ = _handles(os.environ.__setitem__, os.environ.pop)
    rows = []
    for fn_, kind_, args_ in cases():
        ret_, err_ = call(hs_, fn_, kind_, args_)
        assert not _behind_gpu_init(err_), (fn_, kind_, args_, err_)
        assert not ret_ or args_[list(ENTRY[fn_][1]).index("count")] == 0, (fn_, kind_, args_)
        rows.append({"fn": fn_, "handle": kind_, "args": args_, "ret": ret_, "error": err_})
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        f.write('{\n "recorded_at_commit": %s,\n "cases": [\n' % json.dumps(sys.argv[1]))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]\n}\n")
    print(len(rows), "cases")
