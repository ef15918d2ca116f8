"""Helpers of the tests that call the C entry points directly (test_gpu_hbm_kernels.py,
test_gpu_train_kernels.py): device pointers, outputs inside pattern-filled buffers, inputs inside
NaN margins, and bitwise comparison."""
import numpy as np
import torch

PATTERN = 0xA5
PAD = 256


def P(t):
    from expecto_amd import _lib
    return None if t is None else _lib.dptr(t)


def ST():
    from expecto_amd import _lib
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_offset(a, nbytes):
    """``a`` on the device at an address ``nbytes`` past an allocation's (512-byte aligned) start."""
    a = np.ascontiguousarray(a)
    assert nbytes % a.itemsize == 0
    k = nbytes // a.itemsize
    buf = torch.empty(a.size + k, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[k:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 512 == nbytes % 512
    return view


class Guarded:
    """An output of ``shape`` / ``dtype`` (numpy) inside a pattern-filled device buffer, at least
    PAD bytes from both ends; ``offset`` bytes move it off the buffer's 256-byte alignment."""

    def __init__(self, shape, dtype, offset=0):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.lo = PAD + offset
        self.buf = torch.full((self.lo + self.nbytes + PAD + (-self.nbytes) % 16,), PATTERN, dtype=torch.uint8,
                              device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + self.lo

    def put(self, a):
        """Set the region (an output that is also read, such as a model's weights) to ``a``."""
        a = np.ascontiguousarray(a, self.dtype)
        assert a.shape == self.shape
        self.buf[self.lo:self.lo + self.nbytes] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).cuda()
        return self

    def result(self):
        """The region as a host array, after checking that the bytes around it kept the pattern."""
        raw = self.buf.cpu().numpy()
        before, after = raw[:self.lo], raw[self.lo + self.nbytes:]
        assert before.size >= PAD and after.size >= PAD
        bad = np.nonzero(before != PATTERN)[0]
        assert bad.size == 0, f"{bad.size} bytes written before the output, nearest at -{self.lo - bad[-1]}"
        bad = np.nonzero(after != PATTERN)[0]
        assert bad.size == 0, f"{bad.size} bytes written after the output, nearest at +{bad[0]}"
        return raw[self.lo:self.lo + self.nbytes].copy().view(self.dtype).reshape(self.shape)

    def untouched(self):
        return bool((self.result().view(np.uint8) == PATTERN).all())


class Margined:
    """A float32 input ``a`` ([rows, n]: columns of a matrix, or the labels / row weights of a batch)
    laid out with ``stride`` floats per row (0: one shared row) inside one device allocation that
    holds ``margin`` (+ ``shift``) floats of NaN before the first row and ``margin`` after the
    last; the ``stride - n`` floats after every row are NaN too.  A load that should have been
    dropped, or an index off by one, lands in memory the test owns and poisons a sum."""

    def __init__(self, a, stride, margin, shift=0):
        a = np.atleast_2d(np.asarray(a, np.float32))
        rows, n = a.shape
        assert (stride >= n) if stride else rows == 1
        step = stride if stride else n
        host = np.full(margin + shift + rows * step + margin, np.nan, np.float32)
        body = host[margin + shift:margin + shift + rows * step].reshape(rows, step)
        body[:, :n] = a
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + 4 * (margin + shift)
        self.stride = stride


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    iv = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    same = got.view(iv) == want.view(iv)
    if got.dtype.kind == "f":
        same |= np.isnan(got) & np.isnan(want)
    bad = np.argwhere(~same)
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}: "
                           f"got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")
