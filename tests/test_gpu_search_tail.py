"""rs_search_apply_k, the split decode's tail as one kernel (root search, Forney, apply:
POPORON_AMD_DECODE_TAIL=search, and the default for batches of more than one 1024-row batch per
compute unit), on the rows of tests/rs_syndrome_rows.py.

Each wave of the kernel carries a software pipeline over its batches: the root list of batch
b + 1 is searched while the second half of block b is in flight, and the corrections of b
are applied on either side of that search.  So besides what the two-kernel tails are tested
on, the things that can go wrong here are a state carried into the wrong batch, a wave that
leaves the loop with half a block pending, and the two byte windows a quarter block is
staged in.  Every row of every test is compared with the oracle on ok, corrected_num and all
its bytes; where the fused and split tails run on the same input, the three outputs are
identical, guard bytes included.
"""
import numpy as np
import pytest

import libpoporon_amd as P
import rs_syndrome_rows as R
import test_gpu_rs_chosen_syndromes as C

pytestmark = pytest.mark.gpu

DEFAULT = C.DEFAULT
# DECODE_PATH=split: the split kernels at every count
TAILS = {tail: {"POPORON_AMD_DECODE_PATH": "split", "POPORON_AMD_DECODE_TAIL": tail}
         for tail in ("search", "fused", "split")}
GUARD = 64  # guard rows on either side of a batch


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _handle(code, tail, monkeypatch):
    """The environment is read at poporon_create: set it, then create."""
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    for name in ("POPORON_AMD_GENERIC", "POPORON_AMD_DECODE_PATH", "POPORON_AMD_DECODE_TAIL",
                 "POPORON_AMD_FORCE_VERIFY"):
        monkeypatch.delenv(name, raising=False)
    for name, value in TAILS[tail].items():
        monkeypatch.setenv(name, value)
    h = P.Poporon(*code)
    assert h.supported
    return h


def _launches(h, fn):
    h.timing(True)
    fn()
    t = {k: h.timing_read(k)[1] for k in (P.KERNEL_BM, P.KERNEL_CHIEN, P.KERNEL_FORNEY, P.KERNEL_APPLY)}
    h.timing(False)
    return t


def _decode(torch, h, pc, order, tail, count=None, layout="wire", guard=0, null_corrected=False, what="",
            split_kernels=True):
    """decode_batch_device of pool rows `order` in one of the layouts
      wire       rows size + nr bytes apart, 16-byte aligned base
      off1       the same, the base one byte past a 16-byte boundary
      stride256  rows size + nr + 1 apart
      separate   data rows and parity rows in buffers of their own
    with `guard` rows of a fixed pattern before and after the batch in the same allocation.
    The first `count` rows are decoded.  Compares ok, corrected_num and every byte of every
    buffer with the oracle's rows and the bytes that were there; returns all of it.
    split_kernels: whether the call reaches them (the timers say which kernels ran)."""
    data, parity, want = C._take(pc, order)
    n, size = data.shape
    nr = parity.shape[1]
    count = n if count is None else count

    def patterned(length):
        return ((np.arange(length, dtype=np.uint32) * 37 + 11) % 251).astype(np.uint8)

    def carve(bufs):
        """the (n, size) data rows and (n, nr) parity rows inside the buffers"""
        if layout == "separate":
            return [bufs[0][starts[0]:starts[0] + n * size].reshape(n, size),
                    bufs[1][starts[1]:starts[1] + n * nr].reshape(n, nr)]
        rows = bufs[0][starts[0]:starts[0] + n * w].reshape(n, w)
        return [rows[:, :size], rows[:, size:size + nr]]

    if layout == "separate":
        ds, ps = size, nr
        bufs = [patterned((n + 2 * guard) * size + 16), patterned((n + 2 * guard) * nr + 16)]
        starts = [guard * size, guard * nr]
    else:
        w = size + nr + (1 if layout == "stride256" else 0)
        ds = ps = w
        starts = [(1 if layout == "off1" else 0) + guard * w]
        bufs = [patterned(starts[0] + (n + guard) * w + 16)]
    views = carve(bufs)
    views[0][:], views[1][:] = data, parity
    dev = [torch.from_numpy(b).cuda() for b in bufs]
    dptr = dev[0].data_ptr() + starts[0]
    pptr = dev[1].data_ptr() + starts[1] if layout == "separate" else dptr + size
    if layout in ("wire", "off1") and w == 255:
        assert dptr % 16 == (1 if layout == "off1" else 0)
    okd = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    cord = torch.full((n + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    t = _launches(h, lambda: h.decode_batch_device(dptr, ds, pptr, ps, size, count, okd.data_ptr(),
                                                   None if null_corrected else cord.data_ptr(),
                                                   stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    # the route: the split kernels, and the tail asked for
    if split_kernels:
        assert t[P.KERNEL_BM] == 1 and t[P.KERNEL_APPLY] == 1, (what, tail, t)
        assert t[P.KERNEL_CHIEN] == (0 if tail == "search" else 1), (what, tail, t)
        assert t[P.KERNEL_FORNEY] == (1 if tail == "split" else 0), (what, tail, t)
    else:
        assert not any(t.values()), (what, tail, t)
    ok, cor = okd.cpu().numpy(), cord.cpu().numpy()
    got = [d.cpu().numpy() for d in dev]
    what = f"{what}, tail {tail}, layout {layout}, count {count}"
    assert (ok[count:] == 0xEE).all() and (cor[count:] == 0xEE).all(), f"{what}: flags written past the count"
    if null_corrected:
        assert (cor == 0xEE).all(), f"{what}: corrected_num written with no array given"
    gviews = carve(got)
    # without a corrected_num array, the oracle's own column stands in for it
    C._same(what, pc, (ok[:count], want[1][:count] if null_corrected else cor[:count], gviews[0][:count],
                       gviews[1][:count]), tuple(a[:count] for a in want), order)
    # everything else: guard rows, the rows past the count, the bytes between rows
    views[0][:count], views[1][:count] = want[2][:count], want[3][:count]
    for g, b in zip(got, bufs):
        bad = np.nonzero(g != b)[0]
        assert bad.size == 0, f"{what}: byte {bad[0]} outside the decoded rows changed ({bad.size} bytes differ)"
    return ok, cor, got


def _three(torch, monkeypatch, pc, order, **kw):
    """the same input through the three tails: each equal to the oracle, all three identical"""
    res = {}
    for tail in TAILS:
        h = _handle(pc.code, tail, monkeypatch)
        res[tail] = _decode(torch, h, pc, order, tail, **kw)
        h.close()
    for tail in ("fused", "split"):
        for a, b in zip(res["search"][:2], res[tail][:2]):
            assert (a == b).all(), (tail, kw)
        assert all((a == b).all() for a, b in zip(res["search"][2], res[tail][2])), (tail, kw)


def _mixed(pc):
    """The pool shuffled, every family and every error count 0 .. t + 1 within the first 2112 rows"""
    order = R.shuffled(pc.pool)
    head = order[:2048 + 64]
    fam = set(pc.pool.families()[head])
    need = {"ordinary", "late_discrepancy", "sparse", "zero_run", "positions"}
    need |= {"padding_roots"} if pc.size < C._k(pc.code) else set()
    assert need <= fam, need - fam
    assert {pc.pool.tags[r].e for r in head if pc.pool.tags[r].family == "ordinary"} == set(range(pc.t + 2))
    assert np.isin(R.list_rows(pc.pool, pc.t), head).any()  # deg != L / L > t: the list
    return order


def _rejected(pc):
    """Rows of t + 1 errors that fail: Berlekamp-Massey ends with deg = L = t and the root
    search finds fewer than t roots (a locator of t + 1 errors' syndromes seldom splits)"""
    rows = pc.pool.where(lambda g: g.family == "ordinary" and g.e == pc.t + 1)
    rows = rows[pc.want[0][rows] == 0]
    assert rows.size >= 64
    return rows


# ---------------------------------------------------------------------------
# 1. count edges
# ---------------------------------------------------------------------------
NR16 = (8, 0x11D, 1, 1, 16)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 127, 1024, 1024 + 63, 2048 + 64])
def test_count_edges(torch_cuda, monkeypatch, count):
    """The partial wave, one block, a block and a partial wave, a whole workgroup and its
    edge, at full length (the wire layout: the block path) and shortened to 101 bytes (roots in
    the padding; rows back to back are no wire rows: byte by byte).  A single codeword of a
    32-root code goes to the one-workgroup decoder on every path (api.cpp decode_route), so the
    16-root code, whose single calls take the split kernels, runs the same counts."""
    for code, size in ((DEFAULT, C._k(DEFAULT)), (DEFAULT, C._short(DEFAULT)), (NR16, C._k(NR16))):
        pc = C._pool(code, size)
        order = _mixed(pc)
        start = (2048 + 64 - count) // 2  # not always the same first rows
        _three(torch_cuda, monkeypatch, pc, order[start:start + count], what=f"{C._id(code)}, size {size}",
               split_kernels=code != DEFAULT or count > 1)


# ---------------------------------------------------------------------------
# 2 / 3. several batches per wave: what is carried from one to the next
# ---------------------------------------------------------------------------
def _device_pool(torch, pc, rows):
    """pool rows as device tensors: the received rows and the oracle's (ok, corrected, rows)"""
    cat = lambda a, b: torch.from_numpy(np.ascontiguousarray(np.concatenate([a[rows], b[rows]], 1))).cuda()  # noqa: E731
    return (cat(pc.pool.data, pc.pool.parity), torch.from_numpy(pc.want[0][rows].astype(np.uint8)).cuda(),
            torch.from_numpy(pc.want[1][rows].astype(np.uint8)).cuda(), cat(pc.want[2], pc.want[3]))


def _decode_tiled(torch, h, pc, rows, idx, what, chien=0):
    """Batch row i = pool row rows[idx[i]] (idx: a device index tensor), built, decoded in the wire
    layout and compared with the tiled oracle results on the device.  chien: launches of rs_chien_k
    (none where rs_search_apply_k is the tail)."""
    recv, wok, wcor, wrows = _device_pool(torch, pc, rows)
    n = idx.numel()
    batch = recv.index_select(0, idx)
    assert batch.data_ptr() % 16 == 0 and batch.is_contiguous() and batch.shape[1] == 255
    ok = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    cor = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    size = pc.size
    t = _launches(h, lambda: h.decode_batch_device(batch.data_ptr(), 255, batch.data_ptr() + size, 255, size, n,
                                                   ok.data_ptr(), cor.data_ptr(),
                                                   stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert t == {P.KERNEL_BM: 1, P.KERNEL_CHIEN: chien, P.KERNEL_FORNEY: 0, P.KERNEL_APPLY: 1}, (what, t)
    for name, g, w in (("ok", ok, wok.index_select(0, idx)), ("corrected_num", cor, wcor.index_select(0, idx)),
                       ("bytes", batch, wrows.index_select(0, idx))):
        bad = (g != w) if g.dim() == 1 else (g != w).any(1)
        if bool(bad.any()):
            c = int(torch.nonzero(bad)[0])
            r = int(rows[int(idx[c])])
            pytest.fail(f"{what}: {name} differs at batch row {c} (batch {c // 1024}, wave {c % 1024 // 64}): "
                        f"{C._describe(pc, r)} ({int(bad.sum())} rows differ)")


def test_carry_across_batches(torch_cuda, monkeypatch):
    """3 C 1024 + 64 + 37 rows (C compute units): every workgroup runs 3 or 4 batches and the
    batch ends in a partial wave.  Row i is row i mod 8191 of 8191 pool rows, all error counts
    and families mixed: the period is a prime, so a lane's consecutive batches never hold the
    same row, and a stale root list or corrections applied to the wrong batch show."""
    torch = torch_cuda
    pc = C._pool(DEFAULT, C._k(DEFAULT))
    rows = _mixed(pc)[:8191]
    assert rows.size == 8191
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus * 1024 + 64 + 37
    idx = torch.arange(n, device="cuda") % 8191
    h = _handle(DEFAULT, "search", monkeypatch)
    _decode_tiled(torch, h, pc, rows, idx, "prime period")
    h.close()


def test_default_tail_by_count(torch_cuda, monkeypatch):
    """With nothing set the tail goes by the count (api.cpp split_tail): up to one 1024-row batch for
    each of the C workgroups rs_chien_k and rs_forney_apply_k, the launches recorded for such batches in
    tests/golden/decode_routes.json; from C 1024 + 1 rows on rs_search_apply_k alone."""
    torch = torch_cuda
    pc = C._pool(DEFAULT, C._k(DEFAULT))
    rows = _mixed(pc)[:8191]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if P.device_count() == 0:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box")
    for name in ("POPORON_AMD_GENERIC", "POPORON_AMD_DECODE_PATH", "POPORON_AMD_DECODE_TAIL",
                 "POPORON_AMD_FORCE_VERIFY"):
        monkeypatch.delenv(name, raising=False)
    h = P.Poporon(*DEFAULT)
    for n, chien in ((cus * 1024, 1), (cus * 1024 + 1, 0)):
        assert n >= R.SPLIT_MIN_COUNT
        _decode_tiled(torch, h, pc, rows, torch.arange(n, device="cuda") % 8191, f"default tail, {n} rows", chien=chien)
    h.close()


def _kinds(pc):
    """whole-wave kinds -> 64 pool rows each (a few variants of each kind)"""
    t = pc.t
    e = lambda lo, hi: pc.pool.where(lambda g: g.family == "ordinary" and lo <= g.e <= hi)  # noqa: E731
    lst, rej = R.list_rows(pc.pool, t), _rejected(pc)
    assert lst.size >= 30
    kinds = {"clean": e(0, 0), "deg1": e(1, 1), "full": e(t, t), "fast": e(1, t), "listed": lst, "rejected": rej}
    waves = {k: [np.resize(np.roll(v, -64 * j), 64) for j in range(3)] for k, v in kinds.items()}
    for base in ("clean", "listed", "rejected"):  # exactly one fast row, at lane 0, 37 or 63
        waves["one_in_" + base] = []
        for j, lane in enumerate((0, 37, 63)):
            w = waves[base][j].copy()
            w[lane] = kinds["fast"][7 * j + 3]
            waves["one_in_" + base].append(w)
    return waves


# the kinds of one wave's three consecutive batches
TRIPLES = [("clean", "one_in_clean", "clean"), ("listed", "one_in_listed", "listed"),
           ("rejected", "one_in_rejected", "rejected"), ("clean", "one_in_rejected", "listed"),
           ("one_in_clean", "clean", "one_in_listed"), ("full", "clean", "full"), ("clean", "full", "clean"),
           ("deg1", "full", "deg1"), ("full", "deg1", "listed"), ("rejected", "full", "rejected"),
           ("listed", "deg1", "clean"), ("fast", "rejected", "fast"), ("deg1", "deg1", "deg1")]


def test_waves_alike_across_batches(torch_cuda, monkeypatch):
    """3 C batches, so every wave of every workgroup runs three of them, C batches apart: whole
    waves of one kind (clean, on the list, rejected by the search, degree 1, degree t) in the
    orders of TRIPLES, among them a wave with exactly one fast row between two with none: the
    "no fast row" exits with a half block pending before and after."""
    torch = torch_cuda
    pc = C._pool(DEFAULT, C._k(DEFAULT))
    waves = _kinds(pc)
    names = sorted(waves)
    rows = np.concatenate([w for k in names for w in waves[k]])  # 64 rows per (kind, variant)
    slot = {(k, j): 64 * (3 * names.index(k) + j) for k in names for j in range(3)}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    wpb = 16  # waves per batch
    # the workgroup that starts at batch nb - 1 - g takes nb - 1 - g - C and nb - 1 - g - 2 C next: a wave's
    # three batches are the same wave of sections 2, 1, 0 (C batches each)
    starts = np.empty((3, cus * wpb), np.int64)
    for j in range(cus * wpb):
        tr = TRIPLES[j % len(TRIPLES)]
        for s in range(3):
            starts[2 - s, j] = slot[(tr[s], (j // len(TRIPLES)) % 3)]
    idx = (starts.reshape(-1, 1) + np.arange(64)).reshape(-1)
    assert idx.size == 3 * cus * 1024
    h = _handle(DEFAULT, "search", monkeypatch)
    _decode_tiled(torch, h, pc, rows, torch.from_numpy(idx).cuda(), "waves alike")
    h.close()


def test_waves_alike_one_batch(torch_cuda, monkeypatch):
    """The same kinds of waves where every workgroup has one batch, and the layouts of
    rs_syndrome_rows (uniform_blocks, lone_lane), through the three tails."""
    pc = C._pool(DEFAULT, C._k(DEFAULT))
    waves = _kinds(pc)
    order = np.concatenate([waves[k][0] for tr in TRIPLES for k in tr] +
                           [R.uniform_blocks(pc.pool, pc.t), R.lone_lane(pc.pool, pc.t)])
    _three(torch_cuda, monkeypatch, pc, order, what="waves alike")


# ---------------------------------------------------------------------------
# 4. layouts that fall back to bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["stride256", "off1", "separate", "short101"])
def test_layouts_that_fall_back(torch_cuda, monkeypatch, layout):
    """Row stride 256, a base one byte past a 16-byte boundary, parity in a buffer of its own,
    and size 101 (rows 133 bytes apart, roots in the padding): corrected byte by byte."""
    size = C._short(DEFAULT) if layout == "short101" else C._k(DEFAULT)
    assert size == (101 if layout == "short101" else 223)
    pc = C._pool(DEFAULT, size)
    order = _mixed(pc)[:1024 + 63]
    if layout == "short101":  # rows back to back, at an aligned base: size + nr != 255 alone keeps them off the blocks
        _three(torch_cuda, monkeypatch, pc, order, layout="wire", guard=16, what=layout)
    else:
        _three(torch_cuda, monkeypatch, pc, order, layout=layout, guard=16, what=layout)


# ---------------------------------------------------------------------------
# 5. the other codes the kernel serves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", [64 + 37, 16384])
@pytest.mark.parametrize("code", [NR16, (8, 0x11D, 5, 7, 32), (8, 0x11D, 0, 1, 32)], ids=C._id)
def test_other_codes(torch_cuda, monkeypatch, code, count):
    """16 roots in the wire layout (positions below size + 16, rs_bm_k<true> in front), and the
    general-exponent Forney (P11 = false) of fcr 0.  fcr 5, prim 7 would take it too, but its
    verification exponents pass 2^15 and no route gives it to the split kernels (api.cpp
    split_ok): the rows decode on the general kernel, whatever tail is asked for."""
    pc = C._pool(code, C._k(code))
    order = np.resize(_mixed(pc), count)
    reaches = C._takes_split(code, "split")
    assert reaches == (code != (8, 0x11D, 5, 7, 32))
    _three(torch_cuda, monkeypatch, pc, order, what=C._id(code), split_kernels=reaches)


# ---------------------------------------------------------------------------
# 6. neighbours
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", [64, 65, 1024 + 63])
def test_neighbours(torch_cuda, monkeypatch, count):
    """64 guard rows of a fixed pattern before and after the batch in the same allocation come
    back unchanged (the block path writes whole 16-byte chunks of whole waves only); once more
    with no corrected_num array."""
    pc = C._pool(DEFAULT, C._k(DEFAULT))
    order = _mixed(pc)[100:100 + count]
    _three(torch_cuda, monkeypatch, pc, order, guard=GUARD, what="guard rows")
    h = _handle(DEFAULT, "search", monkeypatch)
    _decode(torch_cuda, h, pc, order, "search", guard=GUARD, null_corrected=True, what="null corrected")
    h.close()
