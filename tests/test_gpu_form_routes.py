"""The launch table of the RS layout forms.

The interleaved, report, convolutional, plane and product calls are host code around the row kernels:
per chunk a gather, the codec launches, a snapshot and a report where asked, a scatter.  Which launches a
call makes, and how many chunks it makes them for, shows in the launch counts that timing_read returns
per timing id.  Every case here runs one call with timing on, checks that it returned true and that the
bytes, ok and flags are the ones the construction of the input fixes (at most t errors, or erasures in
ascending order, per codeword: the rows come back clean), and compares the tuple of launch counts over
every RS timing id with the one recorded in tests/golden/form_routes.json.  The table was recorded on
the MI355X by this module's __main__ block at commit 2cc3cac ("Add RS product-code blocks: encode,
scheduled decode and check"), before the forms' chunk loops were folded into one driver; never from the
code under test.

Two codes, RS(255,223) and RS(15,11) (symbol size 4, 0x13, 4 roots), with POPORON_AMD_ILV_CHUNK=96 and
POPORON_AMD_REPORT_CHUNK=96 in force at poporon_create, and counts 1, 96, 97 and 250: one short chunk,
exactly one, one and a remainder of one, two and a remainder.  Interleaved frames run at depth 1 (in
place), depth 5 x 100 frames (chunks of 19 frames) and depth 64 x 3 frames (a frame is the chunk), plain,
with erasure arrays and with report arrays; RS(255,223) also under the CCSDS wire form at depth 1 and 5
(a wire form maps bytes).  Product blocks are RS(15,11) x RS(15,11), 5 blocks, packed (the in-place row
route) and pitched, with both handles' counts side by side.
"""
import json
import os

import numpy as np
import pytest

import libpoporon_amd as P

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "form_routes.json")
ENV = {"POPORON_AMD_ILV_CHUNK": "96", "POPORON_AMD_REPORT_CHUNK": "96"}
CODES = {"rs255_223": (8, 0x11D, 1, 1, 32), "rs15_11": (4, 0x13, 1, 1, 4)}
COUNTS = (1, 96, 97, 250)
FRAMES = tuple((1, c) for c in COUNTS) + ((5, 100), (64, 3))  # (depth, frames)
NMAX = 500
# every RS timing id (KERNEL_NAMES leaves the check's out)
NAMES = {**P.KERNEL_NAMES, P.KERNEL_CHECK: "check", **P.ILV_KERNEL_NAMES, **P.REPORT_KERNEL_NAMES,
         **P.CONV_KERNEL_NAMES, **P.PLANE_KERNEL_NAMES, **P.PROD_KERNEL_NAMES}
KERNEL_IDS = sorted(NAMES)
GROUPS = [(c, g) for c in CODES for g in ("ilv", "report", "planes", "conv")] + [("rs255_223", "wire"),
                                                                                 ("rs15_11", "product")]


def _create(make):
    """a handle made with the chunk sizes in the environment (they are read at poporon_create)"""
    prev = {k: os.environ.get(k) for k in ENV}
    os.environ.update(ENV)
    try:
        return make()
    finally:
        for k, v in prev.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


_inputs = {}


def _code_inputs(code):
    """host rows, made once per code and never written: clean codewords; the same with nr/2 errors in
    the dirty rows; with nr/2 erasures in ascending message positions, their slots and counts"""
    if code in _inputs:
        return _inputs[code]
    m, _, _, _, nr = CODES[code]
    h = P.Poporon(*CODES[code])
    rng = np.random.default_rng(len(code) * 1000 + 23)
    size, q = (1 << m) - 1 - nr, 1 << m
    w = size + nr
    data = rng.integers(0, q, (NMAX, size), dtype=np.uint8)
    clean = np.concatenate([data, h.encode_batch(data)], 1)
    h.close()
    mask = np.zeros(NMAX, np.uint8)
    mask[::7] = 1
    mask[[95, 96, 249, 499]] = 1
    err, era = clean.copy(), clean.copy()
    st = (nr + 15) // 16 * 16  # slot rows 16-byte aligned
    slots, cnt = np.zeros((NMAX, st), np.uint8), np.zeros(NMAX, np.uint8)
    for c in np.nonzero(mask)[0]:
        pos = rng.permutation(w)[: nr // 2]
        err[c, pos] ^= rng.integers(1, q, pos.size, dtype=np.uint8)
        pos = np.sort(rng.permutation(size)[: nr // 2])
        era[c, pos] ^= rng.integers(1, q, pos.size, dtype=np.uint8)
        slots[c, : pos.size] = pos
        cnt[c] = pos.size
    inp = dict(size=size, nr=nr, w=w, q=q, clean=clean, err=err, era=era, slots=slots, cnt=cnt, mask=mask, st=st)
    _inputs[code] = inp
    return inp


def _timed(torch, handles, call):
    """launch counts over KERNEL_IDS, handle after handle, of one call"""
    for h in handles:
        h.timing(True)
    call()
    torch.cuda.synchronize()
    launches = [int(h.timing_read(k)[1]) for h in handles for k in KERNEL_IDS]
    for h in handles:
        h.timing(False)
    return launches


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _zeros(torch, *shape):
    return torch.zeros(shape, dtype=torch.uint8, device="cuda")


def _same(t, a):
    return bool((t.cpu().numpy() == a).all())


class _Report:
    """report arrays of n codewords, and what they must hold after a decode of `bad` into `clean`"""

    def __init__(self, torch, n, nr):
        self.num, self.pos, self.val, self.nr = _zeros(torch, n), _zeros(torch, n, nr), _zeros(torch, n, nr), nr

    def args(self):
        return self.num.data_ptr(), self.pos.data_ptr(), self.val.data_ptr(), self.nr

    def holds(self, bad, clean):
        return _same(self.num, (bad != clean).sum(1))


# ---- interleaved frames, plain and under the CCSDS wire form ------------------------------------------

def run_ilv(torch, code, wire=False):
    import interleave_ref as R
    import wire_ref as W
    inp = _code_inputs(code)
    size, nr, st = inp["size"], inp["nr"], inp["st"]
    h = _create(lambda: P.Poporon(*CODES[code]))
    tc = tw = seq = None
    if wire:
        h.set_wire_form_ccsds(True, True)
        (tc, tw), seq = P.ccsds_dual_basis(), P.ccsds_randomizer()
    s = torch.cuda.current_stream().cuda_stream
    routes = {}
    for depth, frames in FRAMES if not wire else FRAMES[:5]:
        n = depth * frames

        def regions(rows):
            return R.rows_to_frames(rows[:n, :size], depth), R.rows_to_frames(rows[:n, size:], depth)

        cd, cp = regions(inp["clean"])
        want_d, want_p = (cd, cp) if not wire else W.to_wire_frames(cd, cp, depth, tw, None)
        for var in ("enc", "dec", "chk", "dec_era", "dec_rep"):
            if wire and var == "dec_era":
                continue
            bad = inp["era"] if var == "dec_era" else inp["clean"] if var == "enc" else inp["err"]
            d, p = regions(bad)
            if wire:  # an encode reads the message through the map and uses no sequence
                d, p = W.to_wire_frames(d, p, depth, tw, None if var == "enc" else seq)
            d, p = _dev(torch, d), _dev(torch, p if var != "enc" else np.zeros_like(p))
            geo = (d.data_ptr(), size * depth, p.data_ptr(), nr * depth, size, depth, frames)
            ok, cor, dirty, rep = _zeros(torch, n), _zeros(torch, n), _zeros(torch, n), _Report(torch, n, nr)
            sl, cn = _dev(torch, inp["slots"][:n]), _dev(torch, inp["cnt"][:n])
            call = {
                "enc": lambda: h.encode_interleaved_device(*geo, s),
                "dec": lambda: h.decode_interleaved_device(*geo, ok.data_ptr(), cor.data_ptr(), stream=s),
                "chk": lambda: h.check_interleaved_device(*geo, dirty.data_ptr(), s),
                "dec_era": lambda: h.decode_interleaved_device(*geo, ok.data_ptr(), cor.data_ptr(), sl.data_ptr(), st,
                                                               cn.data_ptr(), s),
                "dec_rep": lambda: h.decode_interleaved_report_device(*geo, ok.data_ptr(), *rep.args(),
                                                                      d_corrected=cor.data_ptr(), stream=s),
            }[var]
            key = f"{var}|{depth}x{frames}"
            routes[key] = _timed(torch, [h], call)
            if var == "chk":
                assert _same(dirty, inp["mask"][:n]), (code, key, "dirty")
                continue
            assert _same(p, want_p), (code, key, "parity")
            if var == "enc":
                continue
            assert _same(d, want_d), (code, key, "data")
            assert int(ok.sum()) == n, (code, key, "ok")
            if var == "dec_rep" and not wire:
                assert rep.holds(bad[:n], inp["clean"][:n]), (code, key, "err_num")
    h.close()
    return routes


# ---- the row report: wire rows (one device copy) and split data / parity (the snapshot kernel) -----------

def run_report(torch, code):
    inp = _code_inputs(code)
    size, nr, w, st = inp["size"], inp["nr"], inp["w"], inp["st"]
    h = _create(lambda: P.Poporon(*CODES[code]))
    s = torch.cuda.current_stream().cuda_stream
    routes = {}
    for n in COUNTS:
        for era in (False, True):
            for split in (False, True):
                bad = inp["era" if era else "err"][:n]
                if split:
                    d, p = _dev(torch, bad[:, :size]), _dev(torch, bad[:, size:])
                    geo = (d.data_ptr(), size, p.data_ptr(), nr, size, n)
                else:
                    d = p = _dev(torch, bad)
                    geo = (d.data_ptr(), w, d.data_ptr() + size, w, size, n)
                ok, cor, rep = _zeros(torch, n), _zeros(torch, n), _Report(torch, n, nr)
                sl, cn = _dev(torch, inp["slots"][:n]), _dev(torch, inp["cnt"][:n])
                kw = dict(d_positions=sl.data_ptr(), positions_stride=st, d_counts=cn.data_ptr()) if era else {}
                key = f"{n}|{'era' if era else 'err'}|{'split' if split else 'rows'}"
                routes[key] = _timed(torch, [h], lambda: h.decode_batch_report_device(
                    *geo, ok.data_ptr(), *rep.args(), d_corrected=cor.data_ptr(), stream=s, **kw))
                got = torch.cat([d, p], 1) if split else d
                assert _same(got, inp["clean"][:n]), (code, key, "rows")
                assert int(ok.sum()) == n and rep.holds(bad, inp["clean"][:n]), (code, key, "ok / err_num")
    h.close()
    return routes


# ---- planes ------------------------------------------------------------------------------------------------

def run_planes(torch, code):
    inp = _code_inputs(code)
    size, nr, w = inp["size"], inp["nr"], inp["w"]
    h = _create(lambda: P.Poporon(*CODES[code]))
    s = torch.cuda.current_stream().cuda_stream
    pitch = 256
    lost = [1, size + 1]
    routes = {}

    def stripe(rows, n, off):
        """the rows as planes `pitch` bytes apart, `off` bytes past a 16-byte boundary: (buffer, view, table)"""
        buf = _zeros(torch, w * pitch + 16)
        assert buf.data_ptr() % 16 == 0
        view = buf[off: off + w * pitch].view(w, pitch)
        view[:, :n] = _dev(torch, rows[:n].T)
        return buf, view, [buf.data_ptr() + off + j * pitch for j in range(w)]

    def one(key, var, n, off, strided=False):
        clean = inp["clean"][:n]
        bad = inp["err"][:n].copy() if var in ("chk", "dec", "dec_dirty", "dec_rep") else clean.copy()
        if var == "enc":
            bad[:, size:] = 0
        if var == "dec_lost":
            bad[:, lost] ^= 0x05
        buf, view, tab = stripe(bad, n, off)
        ok, cor, dirty, rep = _zeros(torch, n), _zeros(torch, n), _zeros(torch, n) + 2, _Report(torch, n, nr)
        sg = (tab[0], pitch, tab[size], pitch, size, n)
        call = {
            ("enc", False): lambda: h.encode_planes_device(tab, size, n, s),
            ("chk", False): lambda: h.check_planes_device(tab, size, n, dirty.data_ptr(), s),
            ("dec", False): lambda: h.decode_planes_device(tab, size, n, ok.data_ptr(), None, cor.data_ptr(), None, s),
            ("dec_lost", False): lambda: h.decode_planes_device(tab, size, n, ok.data_ptr(), lost, cor.data_ptr(),
                                                                None, s),
            ("dec_dirty", False): lambda: h.decode_planes_device(tab, size, n, ok.data_ptr(), None, cor.data_ptr(),
                                                                 dirty.data_ptr(), s),
            ("dec_rep", False): lambda: h.decode_planes_report_device(tab, size, n, ok.data_ptr(), *rep.args(),
                                                                      d_corrected=cor.data_ptr(), stream=s),
            ("enc", True): lambda: h.encode_planes_strided_device(*sg, s),
            ("chk", True): lambda: h.check_planes_strided_device(*sg, dirty.data_ptr(), s),
            ("dec", True): lambda: h.decode_planes_strided_device(*sg, ok.data_ptr(), None, cor.data_ptr(), None, s),
        }[(var, strided)]
        routes[key] = _timed(torch, [h], call)
        if var == "chk":
            assert _same(dirty, inp["mask"][:n]), (code, key, "dirty")
            return
        assert _same(view[:, :n], clean.T), (code, key, "planes")
        if var != "enc":
            assert int(ok.sum()) == n, (code, key, "ok")
        if var == "dec_dirty":
            assert int(dirty.sum()) == 0, (code, key, "dirty")
        if var == "dec_rep":
            assert rep.holds(bad, clean), (code, key, "err_num")

    for n in COUNTS:
        for off in (0, 1):
            for var in ("enc", "chk", "dec", "dec_lost", "dec_dirty", "dec_rep"):
                one(f"{var}|{n}|+{off}", var, n, off)
    for var in ("enc", "chk", "dec"):
        one(f"{var}|97|strided", var, 97, 0, strided=True)
    h.close()
    return routes


# ---- convolutional streams -----------------------------------------------------------------------------

def run_conv(torch, code):
    import conv_ref as CR
    inp = _code_inputs(code)
    size, nr = inp["size"], inp["nr"]
    h = _create(lambda: P.Poporon(*CODES[code]))
    s = torch.cuda.current_stream().cuda_stream
    I, M, ph = 3, 2, 1
    routes = {}
    n = 250
    stream = _dev(torch, CR.rows_to_stream(inp["err"][:n], I, M, ph, 0))
    dirty = _zeros(torch, n) + 2
    routes["chk|250"] = _timed(torch, [h], lambda: h.check_conv_device(stream.data_ptr(), I, M, ph, size, n,
                                                                       dirty.data_ptr(), s))
    assert _same(dirty, inp["mask"][:n]), (code, "conv check")
    n = 97
    stream = _dev(torch, CR.rows_to_stream(inp["err"][:n], I, M, ph, 0))
    d, p, ok, cor, rep = _zeros(torch, n, size), _zeros(torch, n, nr), _zeros(torch, n), _zeros(torch, n), \
        _Report(torch, n, nr)
    routes["dec_rep|97"] = _timed(torch, [h], lambda: h.decode_conv_report_device(
        stream.data_ptr(), I, M, ph, d.data_ptr(), size, p.data_ptr(), nr, size, n, ok.data_ptr(), *rep.args(),
        d_corrected=cor.data_ptr(), stream=s))
    assert _same(torch.cat([d, p], 1), inp["clean"][:n]) and int(ok.sum()) == n, (code, "conv decode")
    assert rep.holds(inp["err"][:n], inp["clean"][:n]), (code, "conv err_num")
    h.close()
    return routes


# ---- product blocks: RS(15,11) x RS(15,11) ----------------------------------------------------------------

def run_product(torch, code):
    par = CODES[code]
    m, nr = par[0], par[4]
    k, n1, nb = (1 << m) - 1 - nr, (1 << m) - 1, 5
    rng = np.random.default_rng(77)
    h = P.Poporon(*par)
    msg = rng.integers(0, 1 << m, (nb, k, k), dtype=np.uint8)
    rows = np.concatenate([msg, h.encode_batch(msg.reshape(nb * k, k)).reshape(nb, k, nr)], 2)  # [nb, k, n1]
    cols = np.ascontiguousarray(rows.transpose(0, 2, 1)).reshape(nb * n1, k)
    cpar = h.encode_batch(cols).reshape(nb, n1, nr).transpose(0, 2, 1)                            # [nb, nr, n1]
    clean = np.concatenate([rows, cpar], 1)                                                         # [nb, n1, n1]
    h.close()
    bad = clean.copy()
    bad[:, 3, 2] ^= 1
    bad[:, 3, 9] ^= 5
    bad[:, 7, 12] ^= 3
    only_msg = np.zeros_like(clean)
    only_msg[:, :k, :k] = msg
    pr = _create(lambda: P.Product(par, par))
    hs = [pr.handle(0), pr.handle(1)]
    s = torch.cuda.current_stream().cuda_stream
    routes = {}
    for name, pitch, bstride in (("packed", n1, n1 * n1), ("pitched", n1 + 4, (n1 + 4) * n1 + 5)):
        def place(blocks):
            buf = _zeros(torch, nb * bstride)
            view = buf.as_strided((nb, n1, n1), (bstride, pitch, 1))
            view.copy_(_dev(torch, blocks))
            return buf, view

        geo = (pitch, bstride, k, k, nb)
        for var in ("enc", "dec_a0", "dec_a1", "chk"):
            buf, view = place(only_msg if var == "enc" else bad)
            rd, cd, bok = _zeros(torch, nb, n1), _zeros(torch, nb, n1), _zeros(torch, nb) + 2
            fl = dict(d_row_dirty=rd.data_ptr(), d_col_dirty=cd.data_ptr(), d_block_ok=bok.data_ptr(), stream=s)
            call = {"enc": lambda: pr.encode_device(buf.data_ptr(), *geo, s),
                    "dec_a0": lambda: pr.decode_device(buf.data_ptr(), *geo, 0, 3, 1, **fl),
                    "dec_a1": lambda: pr.decode_device(buf.data_ptr(), *geo, 1, 3, 1, **fl),
                    "chk": lambda: pr.check_device(buf.data_ptr(), *geo, **fl)}[var]
            key = f"{var}|{name}"
            routes[key] = _timed(torch, hs, call)
            if var == "chk":
                want = np.zeros((nb, n1), np.uint8)
                want[:, [3, 7]] = 1
                assert _same(rd, want) and int(bok.sum()) == 0, (key, "flags")
                continue
            assert _same(view, clean), (key, "blocks")
            if var != "enc":
                assert int(bok.sum()) == nb and int(rd.sum()) == 0 and int(cd.sum()) == 0, (key, "flags")
    pr.close()
    return routes


RUN = {"ilv": run_ilv, "wire": lambda torch, code: run_ilv(torch, code, wire=True), "report": run_report,
       "planes": run_planes, "conv": run_conv, "product": run_product}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("code,group", GROUPS)
def test_form_route_table(recorded, code, group):
    import torch
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    assert recorded["kernel_ids"] == KERNEL_IDS
    got = RUN[group](torch, code)
    want = recorded["routes"][code][group]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, f"{code} {group}: (launched, recorded) per case over ids {KERNEL_IDS}: {wrong}"


if __name__ == "__main__":
    # recorder, run from the repository root at the commit whose launches are the record:
    #   PYTHONPATH=.:tests python tests/test_gpu_form_routes.py COMMIT [OUT]
    import sys

    import torch

    table = {}
    for code_, group_ in GROUPS:
        table.setdefault(code_, {})[group_] = RUN[group_](torch, code_)
        print(code_, group_, len(table[code_][group_]), "cases", flush=True)
    with open(sys.argv[2] if len(sys.argv) > 2 else FIXTURE, "w") as f:
        f.write("{\n")
        f.write(f' "recorded_at_commit": {json.dumps(sys.argv[1])},\n')
        f.write(f' "kernel_ids": {json.dumps(KERNEL_IDS)},\n')
        f.write(f' "kernel_names": {json.dumps([NAMES[k] for k in KERNEL_IDS])},\n')
        f.write(' "routes": {\n')
        for i, (code_, groups) in enumerate(table.items()):
            f.write(f'  {json.dumps(code_)}: {{\n')
            for j, (group_, r) in enumerate(groups.items()):
                f.write(f'   {json.dumps(group_)}: {{\n')
                f.write(",\n".join(f'    {json.dumps(k)}: {json.dumps(v)}' for k, v in r.items()))
                f.write(f'\n   }}{"," if j + 1 < len(groups) else ""}\n')
            f.write(f'  }}{"," if i + 1 < len(table) else ""}\n')
        f.write(" }\n}\n")
