"""Device-side harness shared by the LDPC GPU tests (not a test module): rows at odd
offsets and padded strides in buffers full of canary bytes, and the three device
batch calls on them."""
import contextlib
import os

import numpy as np
import pytest

CANARY = 0xA5


@contextlib.contextmanager
def _env(**kw):
    prev = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Rows:
    """count rows of w bytes at an odd offset, a padded stride apart, in a device buffer
    full of canary bytes; canaries() tells whether every byte between the rows survived."""

    def __init__(self, torch, rows, off=3, pad=5):
        rows = np.ascontiguousarray(rows).view(np.uint8)
        self.n, self.w = rows.shape
        self.off, self.stride = off, self.w + pad
        host = np.full(off + self.n * self.stride + 9, CANARY, np.uint8)
        host[off:off + self.n * self.stride].reshape(self.n, self.stride)[:, :self.w] = rows
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + off

    def _host(self):
        return self.dev.cpu().numpy()

    def rows(self):
        return self._host()[self.off:self.off + self.n * self.stride].reshape(self.n, self.stride)[:, :self.w].copy()

    def canaries(self):
        h = self._host()
        body = h[self.off:self.off + self.n * self.stride].reshape(self.n, self.stride)
        return (h[:self.off] == CANARY).all() and (h[self.off + self.n * self.stride:] == CANARY).all() and \
            (body[:, self.w:] == CANARY).all()


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dev_decode(torch, h, din, pin, llr=None, want_iter=True, want_hard=True, off=3, pad=5):
    """poporon_ldpc_decode_batch_device on separate, oddly placed data / parity / llr / hard
    buffers.  Returns (ok, iterations or None, data', hard or None); asserts the canaries and
    that parity was not written."""
    n = din.shape[0]
    d, p = Rows(torch, din, off, pad), Rows(torch, pin, off + 2, pad + 2)
    l = Rows(torch, llr, off + 4, pad + 6) if llr is not None else None
    hd = Rows(torch, np.full((n, h.codeword_bytes), CANARY, np.uint8), off + 6, pad + 4) if want_hard else None
    ok = torch.full((n + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    it = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    h.decode_batch_device(d.ptr, d.stride, p.ptr, p.stride, n, ok.data_ptr(), it.data_ptr() if want_iter else None,
                          hd.ptr if hd else None, hd.stride if hd else 0, l.ptr if l else None,
                          l.stride if l else 0, _stream(torch))
    torch.cuda.synchronize()
    assert d.canaries() and p.canaries() and (hd is None or hd.canaries()) and (l is None or l.canaries())
    assert (p.rows() == pin).all(), "decode wrote parity bytes"
    if l is not None:
        assert (l.rows() == np.ascontiguousarray(llr).view(np.uint8)).all()
    okh, ith = ok.cpu().numpy(), it.cpu().numpy().view(np.uint32)
    assert okh[n] == 0xEE and ith[n] == 0xFFFFFFFF
    if not want_iter:
        assert (ith == 0xFFFFFFFF).all()
    return okh[:n], ith[:n] if want_iter else None, d.rows(), hd.rows() if hd else None


def _dev_encode(torch, h, msgs, off=1, pad=3):
    d = Rows(torch, msgs, off, pad)
    p = Rows(torch, np.full((msgs.shape[0], h.parity_bytes), CANARY, np.uint8), off + 2, pad + 4)
    h.encode_batch_device(d.ptr, d.stride, p.ptr, p.stride, msgs.shape[0], _stream(torch))
    torch.cuda.synchronize()
    assert d.canaries() and p.canaries()
    return d.rows(), p.rows()


def _dev_check(torch, h, dd, pp, off=5, pad=1):
    d, p = Rows(torch, dd, off, pad), Rows(torch, pp, off + 1, pad + 2)
    dirty = torch.full((dd.shape[0] + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    h.check_batch_device(d.ptr, d.stride, p.ptr, p.stride, dd.shape[0], dirty.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    out = dirty.cpu().numpy()
    assert out[-1] == 0xEE and d.canaries() and p.canaries()
    assert (d.rows() == dd).all() and (p.rows() == pp).all()
    return out[:-1]


def _same(what, name, got, want):
    for label, g, w in zip(("ok", "iterations", "data", "hard"), got, want):
        if g is None:
            continue
        bad = (g != w) if g.ndim == 1 else (g != w).any(1)
        if bad.any():
            c = int(np.nonzero(bad)[0][0])
            pytest.fail(f"{what}: {label} differs on code {name}, row {c}: got {g[c]}, reference {w[c]} "
                        f"({int(bad.sum())} of {len(bad)} rows differ)")
