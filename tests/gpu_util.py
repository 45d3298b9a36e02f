"""Helpers for the `-m gpu` parity tests: every call goes through the C-ABI (libmi355diff.so)."""
import numpy as np
import torch

from cudavideostream_amd import CUDACore as _CUDACore

DEV = "cuda:0"

_DEVICE_CALLS = {"diff_stream_batch", "diff_pairs_batch", "diff_stream_wire_batch", "apply_batch",
                 "apply_wire_batch", "merge_parts", "int_diff", "gray_avg", "gray_weighted", "binarize_chain",
                 "heat_map", "red_dense", "red_overlap", "red_stream_batch", "conv3x3", "median5x5", "filter_batch"}


class CUDACore(_CUDACore):
    """The product class with one test-side addition: a core runs on a non-blocking stream of its own, which is NOT
    ordered against torch's streams (include/mi355diff.h, "Streams"), so buffers the tests fill with torch (uploads,
    torch.full on torch's stream) must be complete before a device-resident entry point is enqueued.  Every such entry
    point is wrapped: torch's streams are drained when the method is CALLED -- not when it is looked up (round 3's
    harness did that, and a method bound before the last torch.full raced with the fill: 1 failure in 12 runs)."""


def _synced(name):
    inner = getattr(_CUDACore, name)

    def call(self, *args, **kwargs):
        torch.cuda.synchronize()
        # (temporaries handed in -- core.conv3x3(to_dev(a), out) -- are kept alive by the product class itself until
        # synchronize(): cudavideostream_amd/core.py, _hold)
        return inner(self, *args, **kwargs)

    call.__name__ = name
    call.__doc__ = inner.__doc__
    return call


for _name in _DEVICE_CALLS:
    setattr(CUDACore, _name, _synced(_name))


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


GUARD = 0x5C
PAD = 256            # guard elements before and behind every guarded buffer
_FILL = {torch.uint8: GUARD, torch.int32: -7, torch.int64: -3}


class Guarded:
    """`count` elements of `dtype` with PAD guard elements before and behind them, the first of them `skew` elements behind
    an aligned address.  Everything starts as the guard value of its type; get() asserts that the guards still hold it.
    Hand `ptr` to the library (the view `t` is empty for count == 0)."""

    def __init__(self, count, dtype=torch.uint8, skew=0, data=None):
        self.count, self.lo, self.fill = int(count), PAD + skew, _FILL[dtype]
        self.buf = torch.full((self.lo + self.count + PAD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[self.lo:self.lo + self.count]
        self.ptr = self.buf.data_ptr() + self.lo * self.buf.element_size()
        if data is not None and self.count:
            self.t.copy_(to_dev(data))

    def get(self, written=None):
        """The count elements (numpy); only the first `written` of them may have been written."""
        h = self.buf.cpu().numpy()
        assert (h[:self.lo] == self.fill).all(), "written before the buffer"
        assert (h[self.lo + self.count:] == self.fill).all(), "written behind the buffer"
        body = h[self.lo:self.lo + self.count]
        if written is not None:
            assert (body[written:] == self.fill).all(), "written behind the part that was to be written"
        return body


class Region:
    """S frames of n bytes, `stride` apart, in a guarded device buffer, the first `skew` bytes behind an aligned address.
    Every byte outside the S frames -- before, behind, and in the stride gaps -- holds GUARD; get() asserts that it still
    does."""

    def __init__(self, S, n, stride=None, skew=0):
        self.S, self.n, self.stride, self.skew = S, n, n if stride is None else stride, skew
        self.lo = PAD + skew
        self.buf = torch.full((self.lo + max(S, 1) * self.stride + PAD,), GUARD, dtype=torch.uint8, device=DEV)
        self.t = self.buf[self.lo:]
        self.ptr = self.t.data_ptr()
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == skew % 16

    def _frames(self, h):
        """The [S, stride] view of a host copy of the buffer: columns [:n] are the frames, [n:] the stride gaps."""
        return h[self.lo:self.lo + self.S * self.stride].reshape(self.S, self.stride)

    def put(self, rows):
        """rows: up to S rows of n bytes (one [S, n] array is copied in one piece, whatever S is)."""
        h = np.full(self.buf.numel(), GUARD, np.uint8)
        if isinstance(rows, np.ndarray) and rows.shape == (self.S, self.n):
            self._frames(h)[:, :self.n] = rows
        else:
            for s, row in enumerate(rows):
                h[self.lo + s * self.stride:self.lo + s * self.stride + self.n] = row
        self.buf.copy_(to_dev(h))
        return self

    def get(self):
        """(rows as numpy [S, n]); asserts the guard bytes."""
        h = self.buf.cpu().numpy()
        body = self._frames(h)
        assert (h[:self.lo] == GUARD).all(), "bytes in front of the frames were written"
        assert (h[self.lo + self.S * self.stride:] == GUARD).all(), "bytes behind the frames were written"
        assert (body[:, self.n:] == GUARD).all(), "bytes in the stride gaps were written"
        return body[:, :self.n].copy()

    def clone(self):
        r = Region(self.S, self.n, self.stride, self.skew)
        r.buf.copy_(self.buf)
        return r


class FarRegion:
    """Region's interface for strides of many MiB or GiB: S windows of n bytes, `stride` apart, in ONE device allocation of
    PAD + skew + (S - 1) * stride + n + PAD bytes that never crosses to the host.  The allocation is filled with GUARD on the
    device; put() uploads the S x n rows and scatters them there; get() gathers the S windows there, downloads those, and
    asserts on the device, in pieces of at most 1 GiB, that every other byte -- the front pad, every stride gap in full, the
    tail pad -- still holds GUARD.  (S * n bytes cross the bus each way, whatever the stride.)"""

    PIECE = 1 << 30

    def __init__(self, S, n, stride, skew=0, device=DEV):
        assert S >= 1 and stride >= n
        self.S, self.n, self.stride, self.skew, self.lo = S, n, stride, skew, PAD + skew
        self.buf = torch.full((self.bytes_needed(S, n, stride, skew),), GUARD, dtype=torch.uint8, device=device)
        self.ptr = self.buf.data_ptr() + self.lo
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == skew % 16

    @staticmethod
    def bytes_needed(S, n, stride, skew=0):
        return PAD + skew + (S - 1) * stride + n + PAD

    def window(self, s):
        """The view of window s (a slice of the allocation: its offset is 64-bit host arithmetic)."""
        at = self.lo + s * self.stride
        return self.buf[at:at + self.n]

    def put(self, rows):
        """rows: S rows of n bytes (an [S, n] array or a list of rows)."""
        rows = np.ascontiguousarray(np.stack([np.asarray(r, np.uint8) for r in rows]) if not isinstance(rows, np.ndarray) else rows)
        assert rows.shape == (self.S, self.n) and rows.dtype == np.uint8
        d = torch.from_numpy(rows).to(self.buf.device)
        for s in range(self.S):
            self.window(s).copy_(d[s])
        return self

    def gaps(self):
        """[(first byte, end, name)] of everything outside the windows, in address order."""
        out = [(0, self.lo, "the front pad")]
        for s in range(self.S - 1):
            out.append((self.lo + s * self.stride + self.n, self.lo + (s + 1) * self.stride, f"the gap behind window {s}"))
        end = self.lo + (self.S - 1) * self.stride + self.n
        out.append((end, self.buf.numel(), "the tail pad"))
        return [g for g in out if g[1] > g[0]]

    def get(self):
        """(rows as numpy [S, n]); asserts every guard byte, on the device."""
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        rows = torch.stack([self.window(s) for s in range(self.S)]).cpu().numpy()
        pieces = [(a, min(a + self.PIECE, hi), name) for lo, hi, name in self.gaps() for a in range(lo, hi, self.PIECE)]
        bad = torch.stack([(self.buf[a:b] != GUARD).any() for a, b, _ in pieces]).cpu().numpy()
        for (a, b, name), hit in zip(pieces, bad):
            if hit:
                first = a + int(torch.argmax((self.buf[a:b] != GUARD).to(torch.uint8)))   # (the first of the maxima)
                where = first - self.lo
                raise AssertionError(f"byte {first} of the allocation (window base {where:+d}, that is {where // self.stride} "
                                     f"strides and {where % self.stride} bytes) was written: it lies in {name}")
        return rows

    def free(self):
        self.buf = None


def run_stream(core, frames, capacity=None, stride=None, pair_prev=None):
    """frames: (T, N) uint8 numpy or cuda tensor.  Returns (offsets, xs, diff) as numpy, with xs/diff
    cut to min(total, capacity)."""
    d_frames = frames if torch.is_tensor(frames) else to_dev(frames)
    T = d_frames.shape[0]
    n = core.total
    cap = T * n if capacity is None else capacity
    d_off = torch.full((T + 1,), 0xFFFFFFFF, dtype=torch.int64, device=DEV).to(torch.int32)
    d_xs = torch.full((max(cap, 1),), -7, dtype=torch.int32, device=DEV)
    d_df = torch.full((max(cap, 1),), 0xA5, dtype=torch.uint8, device=DEV)
    if pair_prev is None:
        core.diff_stream_batch(d_frames, T, d_off, d_xs, d_df, cap, stride=stride)
    else:
        d_prev = pair_prev if torch.is_tensor(pair_prev) else to_dev(pair_prev)
        core.diff_pairs_batch(d_frames, d_prev, T, d_off, d_xs, d_df, cap, stride=stride)
    core.synchronize()
    off = d_off.cpu().numpy().view(np.uint32)
    tot = min(int(off[-1]), cap)
    return off, d_xs[:tot].cpu().numpy(), d_df[:tot].cpu().numpy(), (d_xs, d_df)


def oracle_pairs(po, cur, prev, thr=20):
    offs, xs, df = [0], [], []
    for t in range(cur.shape[0]):
        c, x, d, _ = po.diff_pack(cur[t], prev[t], thr)
        offs.append(offs[-1] + c); xs.append(x); df.append(d)
    return (np.array(offs, np.uint32), np.concatenate(xs) if xs else np.empty(0, np.int32),
            np.concatenate(df) if df else np.empty(0, np.uint8))


class BigGuarded:
    """Guarded's interface for outputs of many GiB that never cross to the host: `count` elements of `dtype` with PAD guard
    elements before and behind them, everything filled with the guard value of its type on the device.  check() asserts on the
    device, in pieces of at most PIECE bytes, that both pads -- and the body from element `written` on -- still hold it."""

    PIECE = 1 << 30

    def __init__(self, count, dtype=torch.uint8, device=DEV):
        self.count, self.fill = int(count), _FILL[dtype]
        self.buf = torch.full((self.bytes_needed(count, dtype) // torch.empty(0, dtype=dtype).element_size(),), self.fill,
                              dtype=dtype, device=device)
        self.t = self.buf[PAD:PAD + self.count]
        self.ptr = self.buf.data_ptr() + PAD * self.buf.element_size()

    @staticmethod
    def bytes_needed(count, dtype=torch.uint8):
        return (PAD + int(count) + PAD) * torch.empty(0, dtype=dtype).element_size()

    def check(self, written=None):
        step = self.PIECE // self.buf.element_size()
        spans = [(0, PAD, "before the buffer"), (PAD + self.count, self.buf.numel(), "behind the buffer")]
        if written is not None:
            spans.insert(1, (PAD + int(written), PAD + self.count, "behind the part that was to be written"))
        for lo, hi, name in spans:
            for a in range(lo, hi, step):
                piece = self.buf[a:min(a + step, hi)]
                if bool((piece != self.fill).any()):
                    first = a + int(torch.argmax((piece != self.fill).to(torch.uint8))) - PAD
                    raise AssertionError(f"element {first} of the buffer's {self.count} was written: it lies {name}")

    def free(self):
        self.buf = self.t = None


def assert_same_on_device(got, want, what, piece=1 << 30):
    """Two device tensors of one shape and type, compared where they lie in slices of at most `piece` bytes; the message names
    the first element that differs and both values."""
    assert got.shape == want.shape and got.dtype == want.dtype and got.dim() == 1, (what, got.shape, want.shape)
    step = max(1, piece // got.element_size())
    for a in range(0, got.numel(), step):
        g, w = got[a:a + step], want[a:a + step]
        if not torch.equal(g, w):
            first = a + int(torch.argmax((g != w).to(torch.uint8)))
            raise AssertionError(f"{what}: element {first} is {got[first].item()}, the reference's {want[first].item()}")
