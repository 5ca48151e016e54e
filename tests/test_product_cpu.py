"""RS x RS product-code blocks without a GPU (poporon_*_product*, include/poporon_amd.h): the encode
property on the oracle (every row and column of an encoded block is clean, whichever axis goes first),
count-0 erasure lists, the model of tests/product_ref.py against the compiled reference driven codeword
by codeword, the index arithmetic of the layout kernels restated in numpy (every rectangle byte moved
exactly once, no LDS index past the image, nothing outside a rectangle or the tile's staging rows), the
repair patterns of the GPU tests on the model, every argument check of every entry point (none reaches
the GPU), and the new names and ids."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libpoporon_amd as P
import product_ref as R

# (row params, column params, row_size, col_size)
PAIRS = {
    "dvd": (R.DVD_ROW, R.DVD_COL, 172, 192),
    "gf16": ((4, 0x13, 1, 1, 4), (4, 0x13, 1, 1, 6), 11, 9),            # RS(15,11) x RS(15,9)
    "full": ((8, 0x11D, 1, 1, 32), (8, 0x11D, 1, 1, 16), 223, 239),     # RS(255,223) x RS(255,239)
    "roots100": ((8, 0x11D, 1, 1, 4), (8, 0x11D, 1, 1, 100), 16, 20),   # rows RS(20,16), columns RS(120,20)
    "dvd_row1": (R.DVD_ROW, R.DVD_COL, 1, 192),
    "dvd_col1": (R.DVD_ROW, R.DVD_COL, 172, 1),
}
X = 0x1000  # a non-NULL pointer that is never dereferenced
SEED = 20


# ---- the encode property, on the oracle -----------------------------------------------------

@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_encoded_block_is_a_codeword_on_every_row_and_column(pair):
    row, col, k1, k2 = PAIRS[pair]
    m = R.Model(row, col)
    rng = np.random.default_rng([SEED, k1, k2])
    msg = rng.integers(0, 1 << row[0], (3, k2, k1), dtype=np.uint8)
    blocks = m.encode(msg)
    n1, n2 = m.shape(k1, k2)
    assert blocks.shape == (3, n2, n1) and (blocks[:, :k2, :k1] == msg).all()
    rd, cd, ok = m.check(blocks, k1, k2)
    assert rd.shape == (3, n2) and cd.shape == (3, n1)
    assert not rd.any() and not cd.any() and ok.all()  # parity rows and parity columns included
    assert (m.encode(msg, rows_first=True) == blocks).all()
    blocks[1, n2 - 1, n1 - 1] ^= 1  # the checks-on-checks corner is covered by both axes
    rd, cd, ok = m.check(blocks, k1, k2)
    assert rd.sum() == 1 and rd[1, n2 - 1] and cd.sum() == 1 and cd[1, n1 - 1] and ok.tolist() == [1, 0, 1]


# ---- count-0 lists and the errors-only decode ------------------------------------------------

@pytest.mark.parametrize("params,size", [(R.DVD_ROW, 172), ((4, 0x13, 1, 1, 4), 11)])
def test_count_zero_list_against_the_errors_only_decode(params, size):
    from oracle import Oracle
    o = Oracle(*params)
    nr, mask = params[4], (1 << params[0]) - 1
    rng = np.random.default_rng([SEED, size])
    data = rng.integers(0, mask + 1, (64, size), dtype=np.uint8)
    rows = np.concatenate([data, o.encode_batch(data)], 1)
    for c in range(64):  # 0 .. nr errors: inside t, at t and past it
        pos = rng.choice(size + nr, c % (nr + 1), replace=False)
        rows[c, pos] ^= rng.integers(1, mask + 1, len(pos), dtype=np.uint8)
    nerr = np.arange(64) % (nr + 1)
    plain = o.decode_batch(rows[:, :size], rows[:, size:])
    assert plain[0][nerr <= nr // 2].all() and not plain[0][nerr > nr // 2].all()
    listed = o.decode_batch(rows[:, :size], rows[:, size:], np.zeros((64, nr), np.uint32), np.zeros(64, np.uint32))
    # It is NOT the errors-only decode.  ok and corrected_num agree, and so does every byte of
    # a clean codeword and of a failed one.  A codeword with 1 .. t errors differs: in erasure mode the reference
    # XORs magnitude i into list slot i, read past the count (quirk Q2), so with the zero fill every magnitude
    # lands on symbol 0, the result is ok = 1 with wrong bytes, and the check flags it.
    assert (plain[0] == listed[0]).all() and (plain[1] == listed[1]).all()
    same = (plain[2] == listed[2]).all(1) & (plain[3] == listed[3]).all(1)
    fixed = (plain[0] == 1) & (nerr > 0)
    assert same[~fixed].all() and not same[fixed].all()
    dirty = o.syndrome_batch(listed[2], listed[3])[0]
    assert dirty[fixed & ~same].all() and not o.syndrome_batch(plain[2], plain[3])[0][fixed].any()
    want = rows.copy()  # every magnitude of the errors-only decode, XORed into symbol 0
    want[fixed, 0] ^= np.bitwise_xor.reduce(np.concatenate([plain[2], plain[3]], 1) ^ rows, axis=1)[fixed]
    assert (np.concatenate([listed[2], listed[3]], 1) == np.where(fixed[:, None], want, rows)).all()


# ---- the model against the compiled reference ------------------------------------------------

def _reference_schedule(blocks, first_axis, passes, couple):
    """Model.decode on one DVD block with the reference library itself, one poporon_decode per codeword"""
    from oracle import Reference
    m = R.Model(R.DVD_ROW, R.DVD_COL)
    k, r = (R.DVD_K1, R.DVD_K2), (10, 16)
    b = blocks.copy()
    flag = [None, None]
    a = first_axis
    for p in range(passes):
        rows = R.codewords(b, a)
        lists = couple and p > 0
        ref = Reference(*(R.DVD_ROW, R.DVD_COL)[a], erasure=bool(lists))
        if lists:
            e = np.nonzero(flag[a ^ 1][0])[0]
            ref.set_erasures(e if r[a] // 2 < len(e) <= r[a] else [])
        # wire rows, parity right behind the data, as every row call here has them: in erasure mode the reference
        # indexes data[] with the list's positions, and a parity row's position lies past the message
        rows = np.ascontiguousarray(rows)
        n = C.c_size_t(0)
        for row in rows:
            at = row.ctypes.data
            ref.lib.poporon_decode(ref.h, C.cast(at, C.POINTER(C.c_uint8)), k[a],
                                   C.cast(at + k[a], C.POINTER(C.c_uint8)), C.byref(n))
        ref.close()
        b = R.from_codewords(rows, a, 1)
        flag[a] = m.flags(b, a, k[a])
        a ^= 1
    flag[a] = m.flags(b, a, k[a])
    return b, flag[0], flag[1]


@pytest.mark.parametrize("name", ["rows16", "rows16_nocouple", "burst", "planted", "cols10"])
def test_model_equals_the_compiled_reference_on_dvd_passes(name):
    from oracle import reference_available
    if not reference_available():
        pytest.skip("oracle/_ref not built")
    m = R.Model(R.DVD_ROW, R.DVD_COL)
    clean = R.dvd_blocks(m, 1, SEED)
    bad, first, passes, couple, _ = R.dvd_pattern(name, clean, SEED)
    want = m.decode(bad, R.DVD_K1, R.DVD_K2, first, passes, couple)
    got = _reference_schedule(bad, first, passes, couple)
    for a, b in zip(want[:3], got):
        assert (a == b).all()


# ---- the repair patterns of the GPU tests, on the model --------------------------------------

@pytest.mark.parametrize("name", R.DVD_PATTERNS)
def test_patterns_on_the_model(name):
    m = R.Model(R.DVD_ROW, R.DVD_COL)
    clean = R.dvd_blocks(m, 2, SEED)
    bad, first, passes, couple, repaired = R.dvd_pattern(name, clean, SEED)
    out, rd, cd, ok = m.decode(bad, R.DVD_K1, R.DVD_K2, first, passes, couple)
    assert (name == "clean") == (bad == clean).all()
    if repaired is True:
        assert (out == clean).all() and ok.all() and not rd.any() and not cd.any()
    elif repaired is False:
        assert not ok.any() and (out != clean).any()
    # d_block_ok is truthful about the returned bytes, Q2 results included
    crd, ccd, cok = m.check(out, R.DVD_K1, R.DVD_K2)
    assert (crd == rd).all() and (ccd == cd).all() and (cok == ok).all()


def test_what_the_schedules_need():
    """the table's claims beyond 'repaired': one row pass leaves rows16 dirty, rows9 takes lists and rows8
    does not, the burst is not repaired by a row pass alone"""
    m = R.Model(R.DVD_ROW, R.DVD_COL)
    clean = R.dvd_blocks(m, 1, SEED)
    k = (R.DVD_K1, R.DVD_K2)
    for name, nflag in (("rows8", 8), ("rows9", 9), ("rows16", 16), ("rows17", 17)):
        bad = R.dvd_pattern(name, clean, SEED)[0]
        out, rd, cd, ok = m.decode(bad, *k, 0, 1, 1)
        assert rd.sum() == nflag and not ok.any()
        pos, cnt = R.coupling_lists(rd, 16, 182)
        assert (cnt == (nflag if 8 < nflag <= 16 else 0)).all()
        if cnt.any():
            assert (pos[:, :nflag] == np.nonzero(rd[0])[0][None, :]).all() and not pos[:, nflag:].any()
    bad = R.dvd_pattern("burst", clean, SEED)[0]
    assert not m.decode(bad, *k, 0, 1, 1)[3].any() and m.decode(bad, *k, 0, 2, 1)[3].all()
    for first in (0, 1):
        for passes in (1, 2, 3, 4, 16):
            out = m.decode(bad, *k, first, passes, 1)
            if first == 0:
                assert bool(out[3].all()) == (passes >= 2), passes
            else:  # column first: every column fails, and the count-0 row pass that follows does not repair (Q2)
                assert not out[3].any()


# ---- the tile rule and the index model -------------------------------------------------------

def test_tile_rule():
    for w in range(1, 256):
        for cw in (1, 2, 15, 16, 17, 100, 128, 129, 182, 208, 254, 255):
            g, u, tpb = R.tile_rule(w, cw)
            assert P.product_tile(w, cw) == (g, u)
            assert g >= 1 and 1 <= u and tpb >= 1
            if tpb == 1:
                assert u == cw and g * cw * w <= (R.LDS_PACK if g > 1 else R.LDS_BYTES)
                assert g == 1 or (g + 1) * cw * w > R.LDS_PACK
            else:
                assert g == 1 and u % 16 == 0 and u * w <= R.LDS_BYTES and (tpb - 1) * u < cw <= tpb * u
    assert P.product_tile(208, 182) == (1, 96) and P.product_tile(182, 208) == (1, 112)
    assert P.product_tile(15, 15) == (72, 15) and P.product_tile(255, 255) == (1, 128)
    for bad in ((0, 5), (5, 0), (256, 5), (5, 256), (1 << 40, 1), (-1, 5)):
        assert P.product_tile(*bad) is None
    assert "poporon_amd_product_tile" in P.last_error()


def _sweep_case(axis, n1, n2, m0, m1, cw, pitch, bstride, base, count):
    """every workgroup of a pass: the rectangle's bytes that move are touched exactly once and nothing else is; the
    image bytes of a tile are touched exactly once; the row side covers the staging rows exactly once"""
    w = n2 if axis else n1
    mem, rows = [], []
    for t in range(R.tiles(w, cw, count)):
        tile = R.tile_model(axis, w, cw, m0, m1, pitch, bstride, base, count, t)
        assert tile is not None  # the grid has no idle workgroup
        mem.append(tile["mem"])
        rows.append(tile["rows"])
        img = np.sort(tile["img"])
        assert (img == R.expected_image(axis, w, cw, m0, m1, tile)).all()
    assert R.tile_model(axis, w, cw, m0, m1, pitch, bstride, base, count, R.tiles(w, cw, count)) is None
    assert (np.sort(np.concatenate(mem)) == R.expected_mem(axis, w, cw, m0, m1, pitch, bstride, base, count)).all()
    assert (np.sort(np.concatenate(rows)) == np.arange(count * cw * w)).all()


@pytest.mark.parametrize("n1", [15, 16, 182, 255])
@pytest.mark.parametrize("n2", [15, 208, 255])
def test_index_model(n1, n2):
    for axis in (0, 1):
        w, cw = (n2, n1) if axis else (n1, n2)
        g, u, tpb = R.tile_rule(w, cw)
        for pitch in (n1, n1 + 1, n1 + 13):
            for bstride in (n2 * pitch, (n2 - 1) * pitch + n1 + (5 if pitch > n1 else 0)):
                for count in sorted({max(1, g - 1), g, g + 1}):
                    for align in range(16):
                        _sweep_case(axis, n1, n2, 0, w, cw, pitch, bstride, 0x70000 + align, count)
        # the passes of an encode: the message in, the parity out; fewer codewords on the column pass
        k = w - min(w - 1, 10)
        kc = cw - min(cw - 1, 6) if axis else cw
        for align in (0, 1, 15):
            _sweep_case(axis, n1, n2, 0, k, kc, n1 + 3, n2 * (n1 + 3) + 7, 0x70000 + align, g + 1)
            _sweep_case(axis, n1, n2, k, w, kc, n1 + 3, n2 * (n1 + 3) + 7, 0x70000 + align, g + 1)


# ---- argument checks: all of them fail before the GPU is touched -------------------------

def _product(pair="dvd"):
    row, col, k1, k2 = PAIRS[pair]
    return P.Product(row, col)


def _calls(h, k1=172, k2=192, pitch=182, stride=182 * 208, count=2, first=0, passes=2, buf=X, out=(X, X, X)):
    lib = P.load_library()
    return [
        ("poporon_encode_product_device",
         lambda: lib.poporon_encode_product_device(h, buf, pitch, stride, k1, k2, count, None)),
        ("poporon_decode_product_device",
         lambda: lib.poporon_decode_product_device(h, buf, pitch, stride, k1, k2, count, first, passes, 1, *out, None)),
        ("poporon_check_product_device",
         lambda: lib.poporon_check_product_device(h, buf, pitch, stride, k1, k2, count, *out, None)),
        ("poporon_encode_product", lambda: lib.poporon_encode_product(h, buf, pitch, stride, k1, k2, count)),
        ("poporon_decode_product",
         lambda: lib.poporon_decode_product(h, buf, pitch, stride, k1, k2, count, first, passes, 1, *out)),
    ]


ENCODES = ("poporon_encode_product_device", "poporon_encode_product")
DECODES = ("poporon_decode_product_device", "poporon_decode_product")
CHECKS = ("poporon_check_product_device",)


def _all_fail(calls, word, only=None):
    n = 0
    for name, f in calls:
        if only is not None and name not in only:
            continue
        assert f() is False, name
        msg = P.last_error()
        assert name in msg and word in msg, (name, msg)
        n += 1
    assert n == (5 if only is None else len(only))


def test_null_handle():
    _all_fail(_calls(None), "NULL handle")
    lib = P.load_library()
    assert lib.poporon_amd_product_handle(None, 0) is None
    assert lib.poporon_amd_product_shape(None, 1, 1, None, None) is False and "NULL handle" in P.last_error()
    assert lib.poporon_amd_product_reserve(None, 172, 192, 1) is False and "NULL handle" in P.last_error()
    lib.poporon_amd_product_destroy(None)


def test_create_needs_one_field_and_served_codes():
    lib = P.load_library()

    def create(row, col):
        cfgs = [lib.poporon_rs_config_create(*p, None, None) if p else None for p in (row, col)]
        h = lib.poporon_amd_product_create(*cfgs)
        for c in cfgs:
            if c:
                lib.poporon_config_destroy(c)
        if h:
            lib.poporon_amd_product_destroy(h)
        return bool(h)

    assert create(R.DVD_ROW, R.DVD_COL)
    assert create((8, 0x11D, 0, 1, 10), (8, 0x11D, 112, 11, 32))  # fcr, prim and num_roots may differ
    assert not create((8, 0x11D, 0, 1, 10), (8, 0x187, 0, 1, 16)) and "one field" in P.last_error()
    assert not create((8, 0x11D, 0, 1, 10), (4, 0x13, 1, 1, 4)) and "one field" in P.last_error()
    assert not create(None, R.DVD_COL) and "NULL config" in P.last_error()
    assert not create(R.DVD_ROW, None) and "NULL config" in P.last_error()
    bch = lib.poporon_bch_config_create(4, 0x13, 3)
    rs = lib.poporon_rs_config_create(*R.DVD_ROW, None, None)
    assert not lib.poporon_amd_product_create(rs, bch) and "RS configs" in P.last_error()
    assert not lib.poporon_amd_product_create(bch, rs) and "RS configs" in P.last_error()
    lib.poporon_config_destroy(bch)
    lib.poporon_config_destroy(rs)


def test_handles_and_shape():
    p = _product()
    assert p.shape(172, 192) == (182, 208) and p.shape(1, 1) == (11, 17) and p.shape(245, 239) == (255, 255)
    for k1, k2, word in ((0, 192, "row_size"), (246, 192, "row_size"), (172, 0, "col_size"), (172, 240, "col_size")):
        with pytest.raises(P.PoporonError, match=word):
            p.shape(k1, k2)
    assert p.handle(0).h != p.handle(1).h and p.handle(0).supported and p.handle(1).supported
    assert (p.handle(0).parity_size, p.handle(1).parity_size) == (10, 16)
    with pytest.raises(P.PoporonError):
        p.handle(2)
    lib = P.load_library()
    assert lib.poporon_amd_product_shape(p.h, 172, 192, None, None) is True  # either output may be NULL
    assert lib.poporon_amd_product_reserve(p.h, 0, 192, 1) is False and "row_size" in P.last_error()


def test_sizes_pitch_and_stride():
    p = _product()
    _all_fail(_calls(p.h, k1=0), "row_size")
    _all_fail(_calls(p.h, k1=246), "row_size")
    _all_fail(_calls(p.h, k2=0), "col_size")
    _all_fail(_calls(p.h, k2=240), "col_size")
    _all_fail(_calls(p.h, k2=240, count=0), "col_size")  # the limits hold at count 0 too
    _all_fail(_calls(p.h, pitch=181), "row_pitch")
    _all_fail(_calls(p.h, stride=207 * 182 + 181), "block_stride")
    _all_fail(_calls(p.h, pitch=190, stride=207 * 190 + 181), "block_stride")
    _all_fail(_calls(p.h, pitch=1 << 62, stride=1 << 63), "block_stride")
    _all_fail(_calls(p.h, stride=1 << 62, count=8), "passes size_t")


def test_schedule_arguments_and_nulls():
    p = _product()
    _all_fail(_calls(p.h, first=2), "first_axis", DECODES)
    _all_fail(_calls(p.h, first=-1), "first_axis", DECODES)
    _all_fail(_calls(p.h, passes=0), "passes", DECODES)
    _all_fail(_calls(p.h, passes=17), "passes", DECODES)
    _all_fail(_calls(p.h, out=(None, None, None)), "NULL argument", DECODES + CHECKS)
    _all_fail(_calls(p.h, out=(None, None, None), count=0), "NULL argument", DECODES + CHECKS)
    _all_fail(_calls(p.h, buf=None), "NULL argument")


def test_count_zero_succeeds_without_a_gpu_call():
    p = _product()
    for name, f in _calls(p.h, count=0, buf=None):
        assert f() is True, (name, P.last_error())
    for name, f in _calls(p.h, count=0, buf=None, out=(None, X, None)):  # any one output is enough
        assert f() is True, (name, P.last_error())


# ---- names and ids ------------------------------------------------------------------------

def test_kernel_ids_and_names():
    text = open(os.path.join(P.INCLUDE_DIR, "poporon_amd.h")).read()
    ids = dict(re.findall(r"POPORON_AMD_KERNEL_(PROD_\w+) = (\d+)", text))
    assert ids == {"PROD_GATHER": "24", "PROD_SCATTER": "25", "PROD_LISTS": "26"}
    assert not re.search(r"#define POPORON_AMD_KERNEL_PROD", text)  # enumerators: the macro ids stay 22
    assert (P.KERNEL_PROD_GATHER, P.KERNEL_PROD_SCATTER, P.KERNEL_PROD_LISTS) == (24, 25, 26)
    assert sorted(P.PROD_KERNEL_NAMES) == [24, 25, 26]
    assert not set(P.PROD_KERNEL_NAMES) & (set(P.KERNEL_NAMES) | set(P.CONV_KERNEL_NAMES) | set(P.PLANE_KERNEL_NAMES))
    lib = P.load_library()
    h = P.Poporon(*R.DVD_ROW)
    assert lib.poporon_amd_timing_read(h.h, 27, None, None) is False


def test_every_new_symbol_is_bound():
    names = [n for n in P.header_symbols() if "product" in n]
    assert sorted(names) == sorted(["poporon_amd_product_create", "poporon_amd_product_destroy",
                                    "poporon_amd_product_handle", "poporon_amd_product_shape",
                                    "poporon_amd_product_tile", "poporon_amd_product_reserve",
                                    "poporon_encode_product_device", "poporon_decode_product_device",
                                    "poporon_check_product_device", "poporon_encode_product",
                                    "poporon_decode_product"])
    lib = P.load_library()
    assert all(hasattr(lib, n) and n in P._SIGS for n in names)
