"""Host-side mirror of the reference's operator for the hot path: ``diff::cuda::CUDACore``
(server/include/kernels.cuh:13-43, server/src/kernels.cu:377-536), over the C-ABI of
libmi355diff.so.  Same method names and argument meaning as the C++ class, plus the
device-resident batch entry points used by the benchmark and the parity tests.

PyTorch is used only as plumbing for device buffers / streams (``tensor.data_ptr()``); every
computation happens in the HIP library.
"""
import ctypes as C

import numpy as np

from . import lib as _l

CHARS_STR = "0123456789BFPSWbkps :/"  # server/include/common.h:13
LR_THRESHOLDS = 20                     # server/include/common.h:14


def _ptr(x):
    """Device/host address of a torch tensor, numpy array, int or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()


def _headers(counts, escapes, n):
    """The headers (n, e) of n records as a client read them: two contiguous uint32 arrays of at least n elements.  The caller
    keeps them referenced until the C call has returned."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    escapes = np.ascontiguousarray(escapes, dtype=np.uint32)
    assert counts.size >= n and escapes.size >= n
    return counts, escapes


def _table(x, per, n, dtype):
    """A host table of `per` members for each of n streams (rectangles, placements, budgets), contiguous."""
    x = np.ascontiguousarray(x, dtype=dtype)
    assert x.size >= per * n
    return x


class PinnedArray:
    """numpy view over hipHostMalloc'ed memory (CUDACore::alloc_arrays, kernels.cu:531-536)."""

    def __init__(self, nbytes, dtype=np.uint8):
        self._lib = _l.load()
        p = C.c_void_p()
        _l.check(self._lib.mi355_host_alloc(C.byref(p), nbytes))
        self.ptr = p.value
        buf = (C.c_uint8 * nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=np.uint8).view(dtype)

    def free(self):
        if self.ptr:
            self.array = None
            _l.check(self._lib.mi355_host_free(self.ptr))
            self.ptr = None


class CUDACore:
    """MI355X drop-in for the reference's CUDACore.

    Reference constructor (kernels.cu:377): CUDACore(charsPx, charsSz, k, total, sampleMatData,
    frameSz).  Here: the same data by keyword; `total` is implied by the frame size.
    """

    def __init__(self, width, height, k=None, sample_mat_data=None, chars_px=None, chars_sz=None,
                 charset=CHARS_STR, threshold=LR_THRESHOLDS, max_batch=1, device=-1,
                 noise_filter=False, visualizer=_l.VIS_NONE, flags=0):
        self._lib = _l.load()
        self.width, self.height = int(width), int(height)
        self.total = 3 * self.width * self.height
        self.max_batch = int(max_batch)
        cfg = _l.Config(self.width, self.height, int(threshold), self.max_batch, int(device),
                        int(bool(noise_filter)), int(visualizer), int(flags))   # flags: lib.FLAG_*
        h = C.c_void_p()
        _l.check(self._lib.mi355_create(C.byref(cfg), C.byref(h)))
        self._h = h
        # The device-resident entry points are asynchronous on the core's OWN stream, which PyTorch's caching allocator
        # knows nothing about: a tensor the caller drops right after the call (a temporary, a slice) could be handed to
        # another torch kernel while the library still reads or writes it.  Every such call therefore keeps its
        # arguments referenced here until synchronize() (include/mi355diff.h, "Lifetime of the caller's buffers").
        self._held = []
        self._own_stream = True
        if k is not None:  # cudaMemcpyToSymbol(dev_k, ...) kernels.cu:394
            k = np.ascontiguousarray(k, dtype=np.float32).reshape(-1)
            assert k.size == 9
            _l.check(self._lib.mi355_set_conv_kernel(self._h, k.ctypes.data))
        if chars_px is not None:  # kernels.cu:379-382
            gh, gw = chars_sz
            chars_px = np.ascontiguousarray(chars_px, dtype=np.uint8).reshape(-1)
            assert chars_px.size == len(charset) * 3 * gh * gw
            _l.check(self._lib.mi355_set_glyphs(self._h, chars_px.ctypes.data, len(charset), gh, gw,
                                                charset.encode()))
        if sample_mat_data is not None:  # kernels.cu:406
            self.set_state(sample_mat_data)

    # -- life cycle -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.mi355_destroy(self._h)   # completes the core's streams first
            self._h = None
        self._held = []

    def _hold(self, *objs):
        """Keeps the arguments of an asynchronous call alive until the next synchronize()."""
        if not self._own_stream:
            return   # a caller's (torch) stream: the allocator orders reuse on that very stream
        if len(self._held) > 4096:   # a caller that never synchronises: bound the list
            self.synchronize()
        self._held.append([o for o in objs if o is not None and not isinstance(o, (int, np.ndarray))])

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def workspace_bytes(self):
        return self._lib.mi355_workspace_bytes(self._h)

    def prepare(self, what=_l.PREPARE_ALL):
        """mi355_prepare: make now what the entry points would otherwise make on first use (lib.PREPARE_*), so that no
        asynchronous call allocates."""
        _l.check(self._lib.mi355_prepare(self._h, int(what)))

    def alloc_outputs(self, capacity):
        """mi355_alloc_outputs: (d_xs, d_diff, draws) -- device addresses (ints) of an index array and a value array of
        `capacity` entries whose placement lets the dense expansion run at its fast speed; free with dev_free()."""
        xs, df, draws = C.c_void_p(), C.c_void_p(), C.c_int(0)
        _l.check(self._lib.mi355_alloc_outputs(self._h, int(capacity), C.byref(xs), C.byref(df), C.byref(draws)))
        return int(xs.value), int(df.value), draws.value

    def dev_free(self, d_ptr):
        _l.check(self._lib.mi355_dev_free(self._h, C.c_void_p(int(d_ptr))))

    def use_torch_stream(self):
        """Enqueue on PyTorch's current stream (0 = the default stream), so torch ops, events and
        collectives issued on it are ordered with the core's kernels."""
        import torch
        _l.check(self._lib.mi355_set_stream(self._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))   # waits for the old stream
        self._own_stream = False
        self._held = []

    def use_own_stream(self):
        _l.check(self._lib.mi355_use_own_stream(self._h))
        self._own_stream = True

    def synchronize(self):
        _l.check(self._lib.mi355_synchronize(self._h))
        self._held = []

    def set_option(self, option, value):
        """lib.OPT_*: OPT_PIPELINE switches the own-stream pipelining; OPT_MEDIAN_ROWS and OPT_SCAN_EPOCH_LEFT are seams
        for the tests (include/mi355diff.h, "Options").  None of them changes a result."""
        _l.check(self._lib.mi355_set_option(self._h, int(option), int(value)))
        self._held = []   # (the call completed what was queued)

    def get_option(self, option):
        v = C.c_int(0)
        _l.check(self._lib.mi355_get_option(self._h, int(option), C.byref(v)))
        return v.value

    # -- reference surface ------------------------------------------------------------------------
    @staticmethod
    def alloc_arrays(r, c):
        """kernels.cu:531-536: three pinned 3rc(+slack) frames and one pinned 3rc int array."""
        n = 3 * r * c
        slack = CUDACore.chunkt_size()
        h_frame = PinnedArray(n + slack)
        n_frame = PinnedArray(n + slack)
        o_frame = PinnedArray(n + slack)
        h_xs = PinnedArray(n * 4 + slack, np.int32)
        return h_frame, n_frame, o_frame, h_xs

    @staticmethod
    def chunkt_size():
        """kernels.cu:527-529 returns sizeof(long4)=32, the reference's access granule; the slack a
        caller must leave behind its buffers.  This implementation never touches bytes past N, the
        value is kept for callers that size their buffers with it."""
        return 32

    def exec_core(self, frame_data, show_ready_n_data, text, h_xs):
        """kernels.cu:430-525.  frame_data (uint8[>=N], in: frame, out: diff[0..h_pos)),
        show_ready_n_data (uint8[>=N] or None), text (str), h_xs (int32[>=N]).  Returns h_pos."""
        pos = C.c_uint32(0)
        t = text.encode() if text else None
        _l.check(self._lib.mi355_exec(self._h, _ptr(frame_data), _ptr(show_ready_n_data), t,
                                      C.addressof(pos), _ptr(h_xs)))
        return pos.value

    # -- exec_core, pipelined (threads.cpp's ring moved below the boundary) ----------------------------
    def pipe_open(self, depth=3):
        _l.check(self._lib.mi355_pipe_open(self._h, int(depth)))

    def pipe_close(self):
        _l.check(self._lib.mi355_pipe_close(self._h))

    def exec_submit(self, frame_data, show_ready_n_data, text, h_xs):
        """Arguments of exec_core (pinned buffers); returns a ticket for exec_wait."""
        ticket = C.c_int64(-1)
        t = text.encode() if text else None
        _l.check(self._lib.mi355_pipe_submit(self._h, _ptr(frame_data), _ptr(show_ready_n_data), t, _ptr(h_xs),
                                             C.byref(ticket)))
        return ticket.value

    def exec_wait(self, ticket):
        """Blocks until the frame's outputs are in its buffers; returns h_pos."""
        pos = C.c_uint32(0)
        _l.check(self._lib.mi355_pipe_wait(self._h, ticket, C.byref(pos)))
        return pos.value

    # -- exec_core into ONE compact record per frame (include/mi355diff.h) -------------------------------
    @staticmethod
    def alloc_record(r, c):
        """A pinned buffer for one frame's compact record: cwire_bytes_max(3rc, 1) bytes, the capacity the compact calls ask for."""
        return PinnedArray(cwire_bytes_max(3 * r * c, 1))

    @staticmethod
    def _record_capacity(h_record, capacity):
        return int(capacity) if capacity is not None else int(h_record.nbytes)

    def exec_core_compact(self, frame_data, show_ready_n_data, text, h_record, capacity=None):
        """exec_core with the frame's changes as one compact record in h_record (uint8, 4-byte aligned, capacity -- by
        default its size -- at least cwire_bytes_max(N, 1)); frame_data is only read.  Returns (h_pos, escapes, bytes): the
        record is h_record[:bytes]."""
        n, e, b = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        t = text.encode() if text else None
        _l.check(self._lib.mi355_exec_cwire(self._h, _ptr(frame_data), _ptr(show_ready_n_data), t, _ptr(h_record),
                                            self._record_capacity(h_record, capacity), C.byref(n), C.byref(e), C.byref(b)))
        return n.value, e.value, b.value

    def exec_submit_compact(self, frame_data, show_ready_n_data, text, h_record, capacity=None):
        """Arguments of exec_core_compact (pinned buffers); returns a ticket for exec_wait_compact (or exec_wait)."""
        ticket = C.c_int64(-1)
        t = text.encode() if text else None
        _l.check(self._lib.mi355_pipe_submit_cwire(self._h, _ptr(frame_data), _ptr(show_ready_n_data), t, _ptr(h_record),
                                                   self._record_capacity(h_record, capacity), C.byref(ticket)))
        return ticket.value

    def exec_wait_compact(self, ticket):
        """Blocks until the frame's record is in its buffer; returns (h_pos, escapes, bytes)."""
        n, e, b = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        _l.check(self._lib.mi355_pipe_wait_cwire(self._h, ticket, C.byref(n), C.byref(e), C.byref(b)))
        return n.value, e.value, b.value

    # -- state ------------------------------------------------------------------------------------
    def set_state(self, frame):
        frame = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
        assert frame.size == self.total
        _l.check(self._lib.mi355_set_state(self._h, frame.ctypes.data))

    def get_state(self):
        out = np.empty(self.total, np.uint8)
        _l.check(self._lib.mi355_get_state(self._h, out.ctypes.data))
        return out

    def state_ptr(self):
        return self._lib.mi355_state_device_ptr(self._h)

    # -- device-resident hot path -----------------------------------------------------------------
    def diff_stream_batch(self, d_frames, nframes, d_offsets, d_xs, d_diff, capacity, stride=None):
        self._hold(d_frames, d_offsets, d_xs, d_diff)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_stream_batch(self._h, _ptr(d_frames), stride, nframes,
                                                   _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), capacity))

    def diff_pairs_batch(self, d_cur, d_prev, nframes, d_offsets, d_xs, d_diff, capacity, stride=None):
        self._hold(d_cur, d_prev, d_offsets, d_xs, d_diff)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_pairs_batch(self._h, _ptr(d_cur), _ptr(d_prev), stride, nframes,
                                                  _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), capacity))

    def diff_consecutive_batch(self, d_first_prev, d_frames, nframes, d_offsets, d_xs, d_diff, capacity, stride=None):
        """Frame 0 against the one frame at d_first_prev, frame t against frame t - 1 of d_frames; no feedback, every frame
        read once.  The core's state is not involved (include/mi355diff.h)."""
        self._hold(d_first_prev, d_frames, d_offsets, d_xs, d_diff)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_consecutive_batch(self._h, _ptr(d_first_prev), _ptr(d_frames), stride, nframes,
                                                        _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), capacity))

    # -- the stream either side of the path (wire format, client, row-band merge) -------------------
    def diff_stream_wire_batch(self, d_frames, nframes, d_offsets, d_wire, capacity_bytes, stride=None):
        """threads.cpp:227-229 byte stream of the batch: {u32 n, i32 xs[n], u8 diff[n]} per frame."""
        self._hold(d_frames, d_offsets, d_wire)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_stream_wire_batch(self._h, _ptr(d_frames), stride, nframes,
                                                        _ptr(d_offsets), _ptr(d_wire), capacity_bytes))

    def diff_stream_cwire_batch(self, d_frames, nframes, d_offsets, d_frame_pos, d_cwire, capacity_bytes, stride=None):
        """diff_stream_batch straight into compact records (include/mi355diff.h): d_frame_pos uint64[nframes + 1] record
        positions; a frame whose record ends past capacity_bytes is skipped whole."""
        self._hold(d_frames, d_offsets, d_frame_pos, d_cwire)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_stream_cwire_batch(self._h, _ptr(d_frames), stride, int(nframes), _ptr(d_offsets),
                                                         _ptr(d_frame_pos), _ptr(d_cwire), int(capacity_bytes)))

    # -- many streams, one frame each: the states live in the caller's memory (include/mi355diff.h) --------------------
    def diff_multi_batch(self, d_frames, d_states, nstreams, d_offsets, d_xs, d_diff, capacity, stride=None):
        """One tick of nstreams streams: stream s diffs d_frames[s] against d_states[s], which takes the negative feedback;
        segment s of (d_offsets, d_xs, d_diff) is that stream's packed frame.  The core's own state is not involved."""
        self._hold(d_frames, d_states, d_offsets, d_xs, d_diff)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_multi_batch(self._h, _ptr(d_frames), _ptr(d_states), int(stride), int(nstreams),
                                                  _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), int(capacity)))

    def diff_multi_wire_batch(self, d_frames, d_states, nstreams, d_offsets, d_wire, capacity_bytes, stride=None):
        """diff_multi_batch into the sender's byte stream: {u32 n, i32 xs[n], u8 diff[n]} per stream."""
        self._hold(d_frames, d_states, d_offsets, d_wire)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_multi_wire_batch(self._h, _ptr(d_frames), _ptr(d_states), int(stride), int(nstreams),
                                                       _ptr(d_offsets), _ptr(d_wire), int(capacity_bytes)))

    def diff_multi_cwire_batch(self, d_frames, d_states, nstreams, d_offsets, d_frame_pos, d_cwire, capacity_bytes,
                               stride=None):
        """diff_multi_batch into compact records: stream s's record at d_frame_pos[s] (uint64[nstreams + 1])."""
        self._hold(d_frames, d_states, d_offsets, d_frame_pos, d_cwire)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_multi_cwire_batch(self._h, _ptr(d_frames), _ptr(d_states), int(stride), int(nstreams),
                                                        _ptr(d_offsets), _ptr(d_frame_pos), _ptr(d_cwire),
                                                        int(capacity_bytes)))

    # -- many streams, many frames each: frame t of stream s at d_frames[s * nframes + t], batch index s * nframes + t ---------
    def diff_multi_stream_batch(self, d_frames, d_states, nstreams, nframes, d_offsets, d_xs, d_diff, capacity, stride=None):
        """nframes frames of each of nstreams streams: what diff_stream_batch(nframes) does on a core whose state is
        d_states[s], for every s; segments s * nframes .. (s + 1) * nframes - 1 of (d_offsets, d_xs, d_diff) are stream s's
        packed frames.  The core's own state is not involved."""
        self._hold(d_frames, d_states, d_offsets, d_xs, d_diff)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_multi_stream_batch(self._h, _ptr(d_frames), _ptr(d_states), int(stride), int(nstreams),
                                                         int(nframes), _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff),
                                                         int(capacity)))

    def diff_multi_stream_wire_batch(self, d_frames, d_states, nstreams, nframes, d_offsets, d_wire, capacity_bytes,
                                     stride=None):
        """diff_multi_stream_batch into the sender's byte stream: {u32 n, i32 xs[n], u8 diff[n]} per batch index."""
        self._hold(d_frames, d_states, d_offsets, d_wire)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_multi_stream_wire_batch(self._h, _ptr(d_frames), _ptr(d_states), int(stride),
                                                              int(nstreams), int(nframes), _ptr(d_offsets), _ptr(d_wire),
                                                              int(capacity_bytes)))

    def diff_multi_stream_cwire_batch(self, d_frames, d_states, nstreams, nframes, d_offsets, d_frame_pos, d_cwire,
                                      capacity_bytes, stride=None):
        """diff_multi_stream_batch into compact records: batch index b's record at d_frame_pos[b]
        (uint64[nstreams * nframes + 1])."""
        self._hold(d_frames, d_states, d_offsets, d_frame_pos, d_cwire)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_diff_multi_stream_cwire_batch(self._h, _ptr(d_frames), _ptr(d_states), int(stride),
                                                               int(nstreams), int(nframes), _ptr(d_offsets),
                                                               _ptr(d_frame_pos), _ptr(d_cwire), int(capacity_bytes)))

    # ... and their receiving end: segment / record s onto d_states[s], the frame to show
    def apply_multi_batch(self, d_offsets, d_xs, d_diff, nstreams, d_states, stride=None):
        """client/opencv.cpp:64-66 for one tick of nstreams streams: segment s of (d_offsets, d_xs, d_diff) is added to
        d_states[s].  The core's own state is not involved."""
        self._hold(d_offsets, d_xs, d_diff, d_states)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_apply_multi_batch(self._h, _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), int(nstreams),
                                                   _ptr(d_states), int(stride)))

    def apply_multi_wire_batch(self, d_wire, counts, nstreams, d_states, stride=None):
        """apply_multi_batch from the wire bytes; counts: the streams' headers as read from the sockets."""
        self._hold(d_wire, d_states)
        stride = self.total if stride is None else stride
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert counts.size >= nstreams
        _l.check(self._lib.mi355_apply_multi_wire_batch(self._h, _ptr(d_wire), counts.ctypes.data, int(nstreams),
                                                        _ptr(d_states), int(stride)))

    def apply_multi_cwire_batch(self, d_cwire, counts, escapes, nstreams, d_states, stride=None):
        """apply_multi_batch straight from compact records, one per stream, back to back where the headers (counts,
        escapes) put them; only the tiles of a state that its record touches are read and written."""
        self._hold(d_cwire, d_states)
        stride = self.total if stride is None else stride
        counts, escapes = _headers(counts, escapes, nstreams)
        _l.check(self._lib.mi355_apply_multi_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                         int(nstreams), _ptr(d_states), int(stride)))

    # ... and of a burst: segments / records s * nframes + t, t in order, onto d_states[s]; the frames in between on request
    def apply_multi_stream_batch(self, d_offsets, d_xs, d_diff, nstreams, nframes, d_states, stride=None, d_frames_out=None,
                                 out_stride=None):
        """client/opencv.cpp:64-66 for nframes ticks of nstreams streams, stream-major as diff_multi_stream_batch makes them:
        segments s * nframes .. (s + 1) * nframes - 1 are added to d_states[s] in order.  d_frames_out: the frame of stream s
        after segment t is also written at (s * nframes + t) * out_stride.  The core's own state is not involved."""
        self._hold(d_offsets, d_xs, d_diff, d_states, d_frames_out)
        stride = self.total if stride is None else stride
        out_stride = self.total if out_stride is None else out_stride
        _l.check(self._lib.mi355_apply_multi_stream_batch(self._h, _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), int(nstreams),
                                                          int(nframes), _ptr(d_states), int(stride), _ptr(d_frames_out),
                                                          int(out_stride)))

    def apply_multi_stream_wire_batch(self, d_wire, counts, nstreams, nframes, d_states, stride=None, d_frames_out=None,
                                      out_stride=None):
        """apply_multi_stream_batch from the wire bytes; counts[s * nframes + t]: the headers as read from the sockets."""
        self._hold(d_wire, d_states, d_frames_out)
        stride = self.total if stride is None else stride
        out_stride = self.total if out_stride is None else out_stride
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert counts.size >= nstreams * nframes
        _l.check(self._lib.mi355_apply_multi_stream_wire_batch(self._h, _ptr(d_wire), counts.ctypes.data, int(nstreams),
                                                               int(nframes), _ptr(d_states), int(stride), _ptr(d_frames_out),
                                                               int(out_stride)))

    def apply_multi_stream_cwire_batch(self, d_cwire, counts, escapes, nstreams, nframes, d_states, stride=None,
                                       d_frames_out=None, out_stride=None):
        """apply_multi_stream_batch straight from compact records, back to back in s * nframes + t order where the headers
        (counts, escapes) put them; a tile of a state is loaded and stored once per call, and only if a record touches it."""
        self._hold(d_cwire, d_states, d_frames_out)
        stride = self.total if stride is None else stride
        out_stride = self.total if out_stride is None else out_stride
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        _l.check(self._lib.mi355_apply_multi_stream_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                                int(nstreams), int(nframes), _ptr(d_states), int(stride),
                                                                _ptr(d_frames_out), int(out_stride)))

    # ... and a relay between the two: a burst of records per stream -> one record per stream, no state involved
    def cwire_coalesce_batch(self, d_cwire, counts, escapes, nstreams, nframes, d_offsets, d_xs, d_diff, capacity):
        """nframes compact records of each of nstreams streams (s * nframes + t order, headers counts / escapes) -> segment s
        of (d_offsets, d_xs, d_diff): the sums (mod 256) of the stream's differences per byte index that are not 0, ascending.
        Applying segment s equals applying the stream's records in order."""
        self._hold(d_cwire, d_offsets, d_xs, d_diff)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        _l.check(self._lib.mi355_cwire_coalesce_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                      int(nstreams), int(nframes), _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff),
                                                      int(capacity)))

    def cwire_coalesce_cwire_batch(self, d_cwire, counts, escapes, nstreams, nframes, d_offsets, d_frame_pos, d_cwire_out,
                                   capacity_bytes):
        """cwire_coalesce_batch into compact records: stream s's ONE record at d_frame_pos[s] (uint64[nstreams + 1]), the
        canonical encoding of its segment."""
        self._hold(d_cwire, d_offsets, d_frame_pos, d_cwire_out)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        _l.check(self._lib.mi355_cwire_coalesce_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                            int(nstreams), int(nframes), _ptr(d_offsets), _ptr(d_frame_pos),
                                                            _ptr(d_cwire_out), int(capacity_bytes)))

    # ... and a relay for a viewer that zooms into a camera: the coalesced records cut to a rectangle per stream
    def cwire_crop_batch(self, d_cwire, counts, escapes, nstreams, nframes, rects, d_offsets, d_xs, d_diff, capacity, flags=0):
        """cwire_coalesce_batch with stream s's sums cut to rects[s] = (x0, y0, w, h) in pixels and written with the byte index
        of the rectangle's own w x h frame (flags = lib.CROP_KEEP_INDEX: with the full frame's index).  Applying segment s to
        the crop of a state equals the crop of applying the stream's records to the state."""
        self._hold(d_cwire, d_offsets, d_xs, d_diff)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        rects = _table(rects, 4, nstreams, np.int32)
        _l.check(self._lib.mi355_cwire_crop_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data, int(nstreams),
                                                  int(nframes), rects.ctypes.data, int(flags), _ptr(d_offsets), _ptr(d_xs),
                                                  _ptr(d_diff), int(capacity)))

    def cwire_crop_cwire_batch(self, d_cwire, counts, escapes, nstreams, nframes, rects, d_offsets, d_frame_pos, d_cwire_out,
                               capacity_bytes, flags=0):
        """cwire_crop_batch into compact records: stream s's ONE record at d_frame_pos[s] (uint64[nstreams + 1]), the
        canonical encoding of its segment."""
        self._hold(d_cwire, d_offsets, d_frame_pos, d_cwire_out)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        rects = _table(rects, 4, nstreams, np.int32)
        _l.check(self._lib.mi355_cwire_crop_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                        int(nstreams), int(nframes), rects.ctypes.data, int(flags),
                                                        _ptr(d_offsets), _ptr(d_frame_pos), _ptr(d_cwire_out),
                                                        int(capacity_bytes)))

    # ... and a multiview relay: the coalesced records of many cameras placed on one canvas, ONE record out
    def cwire_mosaic_batch(self, d_cwire, counts, escapes, nstreams, nframes, place, canvas_w, canvas_h, d_offsets, d_xs, d_diff,
                           capacity):
        """cwire_coalesce_batch of all the streams into ONE segment of a canvas_w x canvas_h BGR24 canvas: place[s] = (sx, sy, w,
        h, dx, dy) in pixels puts that rectangle of camera s at (dx, dy); overlapping destinations add.  d_offsets: uint32[2].
        Applying the segment to a canvas state equals placing what the streams' records make of the cameras' states."""
        self._hold(d_cwire, d_offsets, d_xs, d_diff)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        place = _table(place, 6, nstreams, np.int32)
        _l.check(self._lib.mi355_cwire_mosaic_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data, int(nstreams),
                                                    int(nframes), place.ctypes.data, int(canvas_w), int(canvas_h), _ptr(d_offsets),
                                                    _ptr(d_xs), _ptr(d_diff), int(capacity)))

    def cwire_mosaic_cwire_batch(self, d_cwire, counts, escapes, nstreams, nframes, place, canvas_w, canvas_h, d_offsets,
                                 d_frame_pos, d_cwire_out, capacity_bytes):
        """cwire_mosaic_batch into ONE compact record at d_cwire_out, the canonical encoding of the segment; d_frame_pos
        (uint64[2]) = {0, record bytes}."""
        self._hold(d_cwire, d_offsets, d_frame_pos, d_cwire_out)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        place = _table(place, 6, nstreams, np.int32)
        _l.check(self._lib.mi355_cwire_mosaic_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                          int(nstreams), int(nframes), place.ctypes.data, int(canvas_w),
                                                          int(canvas_h), _ptr(d_offsets), _ptr(d_frame_pos), _ptr(d_cwire_out),
                                                          int(capacity_bytes)))

    # ... and the sender's rate control: the records of one tick held to an entry budget each
    def cwire_budget_cwire_batch(self, d_cwire, counts, escapes, d_states, nstreams, budgets, d_thresholds, d_offsets,
                                 d_frame_pos, d_cwire_out, capacity_bytes, stride=None):
        """The records diff_multi_cwire_batch just made (headers counts / escapes), thinned: stream s keeps at most budgets[s]
        entries (0xFFFFFFFF: no limit) -- those above the least threshold T_s >= the core's that allows it, written to
        d_thresholds[s] (uint32[nstreams]).  The thinned record s goes to d_cwire_out + d_frame_pos[s], and d_states[s] takes the
        previous value at every dropped entry: records and states are those of a tick diffed at T_s."""
        self._hold(d_cwire, d_states, d_thresholds, d_offsets, d_frame_pos, d_cwire_out)
        stride = self.total if stride is None else stride
        counts, escapes = _headers(counts, escapes, nstreams)
        budgets = _table(budgets, 1, nstreams, np.uint32)
        _l.check(self._lib.mi355_cwire_budget_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                          _ptr(d_states), int(stride), int(nstreams), budgets.ctypes.data,
                                                          _ptr(d_thresholds), _ptr(d_offsets), _ptr(d_frame_pos),
                                                          _ptr(d_cwire_out), int(capacity_bytes)))

    # ... and its second lever: the records of one tick without their isolated changes
    def cwire_despeckle_cwire_batch(self, d_cwire, counts, escapes, d_states, nstreams, need, d_dropped, d_offsets, d_frame_pos,
                                    d_cwire_out, capacity_bytes, stride=None):
        """The records diff_multi_cwire_batch just made (headers counts / escapes), despeckled: an entry of stream s stays when
        at least need[s] (0 .. 8; 0: the stream passes through) of the 8 pixels around its pixel changed too.  The kept entries
        go to d_cwire_out + d_frame_pos[s], the entries dropped per stream to d_dropped (uint32[nstreams]), and d_states[s] takes
        the previous value at every dropped entry: records and states are those of a tick on frames without the speckle."""
        self._hold(d_cwire, d_states, d_dropped, d_offsets, d_frame_pos, d_cwire_out)
        stride = self.total if stride is None else stride
        counts, escapes = _headers(counts, escapes, nstreams)
        need = _table(need, 1, nstreams, np.uint32)
        _l.check(self._lib.mi355_cwire_despeckle_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                             _ptr(d_states), int(stride), int(nstreams), need.ctypes.data,
                                                             _ptr(d_dropped), _ptr(d_offsets), _ptr(d_frame_pos),
                                                             _ptr(d_cwire_out), int(capacity_bytes)))

    # ... and what any of these nodes can ask about a camera: is it moving, and where
    def activity_batch(self, d_offsets, d_xs, nstreams, nframes, cell_w, cell_h, d_cells, d_summary, min_count=1,
                       accumulate=False):
        """The segments diff_multi_batch / diff_multi_stream_batch wrote (s * nframes + t order) -> per stream a grid of
        changed bytes per cell of cell_w x cell_h pixels (d_cells, uint32[nstreams][activity_cells(...)[0]]) and
        d_summary, uint32[nstreams][8]: entries, box x0, y0, x1, y1, cells of at least min_count, peak, peak cell.
        accumulate: add onto what the two buffers hold instead of clearing them first."""
        self._hold(d_offsets, d_xs, d_cells, d_summary)
        _l.check(self._lib.mi355_activity_batch(self._h, _ptr(d_offsets), _ptr(d_xs), int(nstreams), int(nframes), int(cell_w),
                                                int(cell_h), int(min_count), int(bool(accumulate)), _ptr(d_cells),
                                                _ptr(d_summary)))

    def cwire_activity_batch(self, d_cwire, counts, escapes, nstreams, nframes, cell_w, cell_h, d_cells, d_summary,
                             min_count=1, accumulate=False):
        """activity_batch straight from compact records (headers counts / escapes, s * nframes + t order)."""
        self._hold(d_cwire, d_cells, d_summary)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        _l.check(self._lib.mi355_cwire_activity_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                      int(nstreams), int(nframes), int(cell_w), int(cell_h), int(min_count),
                                                      int(bool(accumulate)), _ptr(d_cells), _ptr(d_summary)))

    # ... and, before any of them trusts what arrived: is every record well-formed and canonical
    def cwire_check_batch(self, d_cwire, counts, escapes, nrecords, d_verdicts):
        """One verdict per compact record (headers counts / escapes, back to back) into d_verdicts, uint32[nrecords][4]:
        {lib.CWIRE_BAD_* flags (0: well-formed and canonical), 255 codes, first entry at or past the frame's end (n: none),
        1 + the last decoded index, saturated}.  No state is read or written; cwire_check_host is the same on the host."""
        self._hold(d_cwire, d_verdicts)
        counts, escapes = _headers(counts, escapes, nrecords)
        _l.check(self._lib.mi355_cwire_check_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                   int(nrecords), _ptr(d_verdicts)))

    # ... and a sender on a datagram socket: every record cut into pieces that are records themselves
    def cwire_split_cwire_batch(self, d_cwire, counts, escapes, nrecords, max_bytes, d_piece_first, d_piece_pos, piece_capacity,
                                d_cwire_out, capacity_bytes):
        """Every compact record (headers counts / escapes, back to back) cut into pieces of at most max_bytes bytes (a multiple of
        4 in [64, 65536]), each a record of the same frame: piece p at d_cwire_out + d_piece_pos[p] (uint64[piece_capacity + 1]),
        record r's pieces are d_piece_first[r] .. d_piece_first[r + 1] (uint32[nrecords + 1]).  cwire_split_host is the same on
        the host and the definition; cwire_split_pieces_max / cwire_split_bytes_max give sufficient capacities."""
        self._hold(d_cwire, d_piece_first, d_piece_pos, d_cwire_out)
        counts, escapes = _headers(counts, escapes, nrecords)
        _l.check(self._lib.mi355_cwire_split_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                         int(nrecords), int(max_bytes), _ptr(d_piece_first), _ptr(d_piece_pos),
                                                         int(piece_capacity), _ptr(d_cwire_out), int(capacity_bytes)))

    # ... and either end of a stream socket: records run-coded where that makes them smaller, and back
    def cwire_runs_encode_batch(self, d_cwire, counts, escapes, nrecords, policy, d_forms, d_pos, d_out, capacity_bytes):
        """Every compact record (headers counts / escapes, back to back) for the link: in the run form where `policy`
        (lib.RUNS_WHERE_SMALLER, lib.RUNS_ALWAYS) says so, copied otherwise.  d_forms, uint32[nrecords][4] = {form
        (lib.RUNS_FORM_*), n, e, r} per record: what the receiver hands to cwire_runs_decode_batch; record b at d_out + d_pos[b]
        (uint64[nrecords + 1], always exact), written only if it fits.  cwire_runs_encode_host is the same on the host and the
        definition; cwire_runs_bytes_max gives a sufficient capacity."""
        self._hold(d_cwire, d_forms, d_pos, d_out)
        counts, escapes = _headers(counts, escapes, nrecords)
        _l.check(self._lib.mi355_cwire_runs_encode_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                         int(nrecords), int(policy), _ptr(d_forms), _ptr(d_pos), _ptr(d_out),
                                                         int(capacity_bytes)))

    def cwire_runs_decode_batch(self, d_in, forms, nrecords, d_frame_pos, d_cwire_out, capacity_bytes):
        """What cwire_runs_encode_batch wrote, back into compact records: `forms` is the sender's table (host, uint32[nrecords][4]),
        record b goes to d_cwire_out + d_frame_pos[b] (uint64[nrecords + 1], always exact), written only if it fits.
        cwire_runs_decode_host is the same on the host and the definition."""
        self._hold(d_in, d_frame_pos, d_cwire_out)
        forms = _table(forms, 4, nrecords, np.uint32)
        _l.check(self._lib.mi355_cwire_runs_decode_batch(self._h, _ptr(d_in), forms.ctypes.data, int(nrecords), _ptr(d_frame_pos),
                                                         _ptr(d_cwire_out), int(capacity_bytes)))

    # ... with parity datagrams behind the pieces, so that a receiver rebuilds what the link lost
    def cwire_fec_batch(self, d_pieces, pieces_bytes, d_piece_first, d_piece_pos, piece_capacity, nrecords, group, nparity, pitch,
                        d_fec_first, d_fec_len, group_capacity, d_out, capacity_bytes):
        """nparity (1: P, 2: P and Q) parity blocks per group of `group` (1 .. 255) pieces of what cwire_split_cwire_batch wrote,
        on the same stream behind it: block q of group g at d_out + (g*nparity + q)*pitch, d_fec_len[g] (uint32[group_capacity])
        bytes long; record r's groups are d_fec_first[r] .. d_fec_first[r + 1] (uint32[nrecords + 1]).  cwire_fec_host is the same
        on the host and the definition; cwire_fec_groups_max gives a sufficient group_capacity."""
        self._hold(d_pieces, d_piece_first, d_piece_pos, d_fec_first, d_fec_len, d_out)
        _l.check(self._lib.mi355_cwire_fec_batch(self._h, _ptr(d_pieces), int(pieces_bytes), _ptr(d_piece_first), _ptr(d_piece_pos),
                                                 int(piece_capacity), int(nrecords), int(group), int(nparity), int(pitch),
                                                 _ptr(d_fec_first), _ptr(d_fec_len), int(group_capacity), _ptr(d_out),
                                                 int(capacity_bytes)))

    def cwire_fec_repair_batch(self, d_rx, rx_bytes, njobs, job_first, slot_off, slot_len, parity_off, fec_len, d_out, pitch,
                               d_verdict):
        """The lost pieces of njobs groups rebuilt from what arrived in d_rx: job j has the slots job_first[j] .. job_first[j + 1]
        of slot_off (byte offsets into d_rx, lib.FEC_ABSENT: lost) / slot_len, its parity blocks at parity_off[j] = (P, Q)
        (lib.FEC_ABSENT: not there) and fec_len[j]; rebuilt block k to d_out + (2j + k)*pitch, its verdict (lib.FEC_BAD_*) to
        d_verdict, uint32[njobs][2].  cwire_fec_repair_host is the same for one group on the host and the definition."""
        self._hold(d_rx, d_out, d_verdict)
        job_first = np.ascontiguousarray(job_first, dtype=np.uint32)
        slot_off = np.ascontiguousarray(slot_off, dtype=np.uint64)
        slot_len = np.ascontiguousarray(slot_len, dtype=np.uint32)
        parity_off = np.ascontiguousarray(parity_off, dtype=np.uint64)
        fec_len = np.ascontiguousarray(fec_len, dtype=np.uint32)
        assert job_first.size >= njobs + 1 and parity_off.size >= 2 * njobs and fec_len.size >= njobs
        assert slot_off.size >= int(job_first[njobs]) <= slot_len.size
        _l.check(self._lib.mi355_cwire_fec_repair_batch(self._h, _ptr(d_rx), int(rx_bytes), int(njobs), job_first.ctypes.data,
                                                        slot_off.ctypes.data, slot_len.ctypes.data, parity_off.ctypes.data,
                                                        fec_len.ctypes.data, _ptr(d_out), int(pitch), _ptr(d_verdict)))

    # ... and when a record was refused or lost after all: the receiver's digests, the sender's refresh, the receiver's clear
    def state_digest_batch(self, d_states, nstreams, d_digests, stride=None):
        """Two words per tile of 4096 bytes of each of nstreams states (stream s at d_states + s*stride, any alignment) into
        d_digests, uint32[nstreams][state_tiles(N)][2]; state_digest_host is the same on the host and the definition."""
        self._hold(d_states, d_digests)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_state_digest_batch(self._h, _ptr(d_states), int(stride), int(nstreams), _ptr(d_digests)))

    def refresh_cwire_batch(self, d_states, nstreams, d_peer_digests, d_tile_mask, d_offsets, d_frame_pos, d_cwire_out,
                            capacity_bytes, stride=None):
        """The sender's answer to a receiver's digests (None: every tile, a key frame): d_tile_mask,
        uint32[nstreams][ceil(tiles / 32)], has the bits of the tiles whose digest differs from the sender's, and stream s's ONE
        record at d_frame_pos[s] holds (x, state[s][x]) for the nonzero bytes of those tiles -- an ordinary compact record that
        makes a state with those tiles cleared (state_clear_tiles_batch) equal to the sender's there.  Offsets, frame positions
        and capacity as for cwire_coalesce_cwire_batch; the states are only read."""
        self._hold(d_states, d_peer_digests, d_tile_mask, d_offsets, d_frame_pos, d_cwire_out)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_refresh_cwire_batch(self._h, _ptr(d_states), int(stride), int(nstreams), _ptr(d_peer_digests),
                                                     _ptr(d_tile_mask), _ptr(d_offsets), _ptr(d_frame_pos), _ptr(d_cwire_out),
                                                     int(capacity_bytes)))

    def state_clear_tiles_batch(self, d_states, nstreams, d_tile_mask, stride=None):
        """Zeroes the tiles of each state whose bit of d_tile_mask (refresh_cwire_batch's) is set, inside the state's N bytes
        only; apply_multi_cwire_batch of the refresh records follows on the same stream."""
        self._hold(d_states, d_tile_mask)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_state_clear_tiles_batch(self._h, _ptr(d_states), int(stride), int(nstreams), _ptr(d_tile_mask)))

    # ... and the wall that shows its cameras: thumbnails of the states in one frame, repainted where records landed
    def wall_compose_batch(self, d_states, nstreams, place, d_wall, wall_w, wall_h, wall_pitch=None, d_tile_mask=None, stride=None):
        """Box-downscaled thumbnails of nstreams states (stream s at d_states + s*stride, any alignment) into the BGR24 wall of
        wall_w x wall_h pixels at d_wall (pixel (X, Y) at Y*wall_pitch + 3*X).  place is int32[nstreams][3] = {x, y, k}: the
        thumbnail at scale k (1 .. 16; wall_thumb_size) goes to (x, y), k == 0 hides the stream.  d_tile_mask
        (refresh_cwire_batch's or cwire_touched_tiles_batch's) limits the repaint to where a selected tile lands; None: all."""
        self._hold(d_states, d_tile_mask, d_wall)
        stride = self.total if stride is None else stride
        wall_pitch = 3 * int(wall_w) if wall_pitch is None else wall_pitch
        place = _table(place, 3, nstreams, np.int32)
        _l.check(self._lib.mi355_wall_compose_batch(self._h, _ptr(d_states), int(stride), int(nstreams), place.ctypes.data,
                                                    _ptr(d_tile_mask), _ptr(d_wall), int(wall_w), int(wall_h), int(wall_pitch)))

    def cwire_touched_tiles_batch(self, d_cwire, counts, escapes, nstreams, nframes, d_tile_mask, accumulate=False):
        """The tiles of 4096 bytes that the compact records of each stream (headers counts / escapes, s * nframes + t order) have
        an entry in, as the tile mask of refresh_cwire_batch: uint32[nstreams][ceil(tiles / 32)], overwritten or, with
        accumulate, ORed onto."""
        self._hold(d_cwire, d_tile_mask)
        counts, escapes = _headers(counts, escapes, nstreams * nframes)
        _l.check(self._lib.mi355_cwire_touched_tiles_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                           int(nstreams), int(nframes), int(bool(accumulate)), _ptr(d_tile_mask)))

    # ... and the low-resolution viewer behind it: records of the thumbnails, made where the tick's mask says something changed
    def thumb_cwire_batch(self, d_states, nstreams, k, threshold, d_thumbs, d_offsets, d_frame_pos, d_cwire_out, capacity_bytes,
                          d_tile_mask=None, stride=None, thumb_stride=None):
        """ONE compact record per stream of the tw x th thumbnail (scale k in 1 .. 16; wall_thumb_size) of the state at
        d_states + s*stride against the held thumbnail at d_thumbs + s*thumb_stride (3*tw*th bytes, any alignment): an entry
        where |new - held| > threshold, and the held byte becomes the new one there.  d_tile_mask (cwire_touched_tiles_batch's
        or refresh_cwire_batch's, over the full-size state) limits the work to where a selected tile lands; None: everywhere.
        Offsets, frame positions and capacity as for refresh_cwire_batch; a stream whose record does not fit keeps its held
        thumbnail.  thumb_cwire_host is the same on the host and the definition."""
        self._hold(d_states, d_tile_mask, d_thumbs, d_offsets, d_frame_pos, d_cwire_out)
        stride = self.total if stride is None else stride
        if thumb_stride is None:
            thumb_stride = 3 * wall_thumb_size(self.width, self.height, k)[0]
        _l.check(self._lib.mi355_thumb_cwire_batch(self._h, _ptr(d_states), int(stride), int(nstreams), int(k), int(threshold),
                                                   _ptr(d_tile_mask), _ptr(d_thumbs), int(thumb_stride), _ptr(d_offsets),
                                                   _ptr(d_frame_pos), _ptr(d_cwire_out), int(capacity_bytes)))

    def wire_bytes(self, nframes, entries):
        return self._lib.mi355_wire_bytes(nframes, entries)

    def apply_batch(self, d_offsets, d_xs, d_diff, nframes, d_frames_out=None, stride=None):
        """client/opencv.cpp:64-66 on this core's state, frame by frame."""
        self._hold(d_offsets, d_xs, d_diff, d_frames_out)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_apply_batch(self._h, _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), nframes,
                                             _ptr(d_frames_out), stride))

    def apply_wire_batch(self, d_wire, counts, nframes, d_frames_out=None, stride=None):
        self._hold(d_wire, d_frames_out)
        stride = self.total if stride is None else stride
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert counts.size >= nframes
        _l.check(self._lib.mi355_apply_wire_batch(self._h, _ptr(d_wire), counts.ctypes.data, nframes,
                                                  _ptr(d_frames_out), stride))

    def merge_parts(self, d_part_offsets, part_base, xs_bias, d_xs_all, d_diff_all, nframes, d_offsets, d_xs,
                    d_diff, capacity):
        """Row-band streams of one video stream -> the stream of the whole frame."""
        self._hold(d_part_offsets, d_xs_all, d_diff_all, d_offsets, d_xs, d_diff)
        part_base = np.ascontiguousarray(part_base, dtype=np.uint32)
        xs_bias = np.ascontiguousarray(xs_bias, dtype=np.int32)
        assert part_base.size == xs_bias.size
        _l.check(self._lib.mi355_merge_parts(self._h, part_base.size, nframes, _ptr(d_part_offsets),
                                             part_base.ctypes.data, xs_bias.ctypes.data, _ptr(d_xs_all),
                                             _ptr(d_diff_all), _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff),
                                             capacity))

    # -- compact wire format (include/mi355diff.h): gap-coded indices, about 2/5 of the wire form's bytes ------------------
    def cwire_encode_batch(self, d_offsets, d_xs, d_diff, entries_capacity, nframes, d_frame_pos, d_cwire, capacity_bytes):
        """Packed stream (offsets, xs, diff) of nframes frames -> compact records in d_cwire; d_frame_pos: uint64[nframes + 1]
        record positions (frame_pos[nframes] = the batch's bytes, or 2^64 - 1 if offsets[nframes] > entries_capacity)."""
        self._hold(d_offsets, d_xs, d_diff, d_frame_pos, d_cwire)
        _l.check(self._lib.mi355_cwire_encode_batch(self._h, _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), int(entries_capacity),
                                                    int(nframes), _ptr(d_frame_pos), _ptr(d_cwire), int(capacity_bytes)))

    def cwire_decode_batch(self, d_cwire, counts, escapes, nframes, d_offsets, d_xs, d_diff, capacity):
        """Compact records -> packed stream; counts / escapes: the frames' headers (n, e) as the client read them."""
        self._hold(d_cwire, d_offsets, d_xs, d_diff)
        counts, escapes = _headers(counts, escapes, nframes)
        _l.check(self._lib.mi355_cwire_decode_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                    int(nframes), _ptr(d_offsets), _ptr(d_xs), _ptr(d_diff), int(capacity)))

    def apply_cwire_batch(self, d_cwire, counts, escapes, nframes, d_frames_out=None, stride=None):
        """client/opencv.cpp:50-66 straight from compact records on this core's state, in one call; counts / escapes: the
        frames' headers (n, e) as the client read them.  d_frames_out: frame t is also written at t * stride."""
        self._hold(d_cwire, d_frames_out)
        stride = self.total if stride is None else stride
        counts, escapes = _headers(counts, escapes, nframes)
        _l.check(self._lib.mi355_apply_cwire_batch(self._h, _ptr(d_cwire), counts.ctypes.data, escapes.ctypes.data,
                                                   int(nframes), _ptr(d_frames_out), int(stride)))

    def int_diff(self, d_cur, d_prev, d_out, n):
        self._hold(d_cur, d_prev, d_out)
        _l.check(self._lib.mi355_int_diff(self._h, _ptr(d_cur), _ptr(d_prev), _ptr(d_out), n))

    # -- filters ----------------------------------------------------------------------------------
    def gray_avg(self, d_in, d_out):
        self._hold(d_in, d_out)
        _l.check(self._lib.mi355_gray_avg(self._h, _ptr(d_in), _ptr(d_out)))

    def gray_weighted(self, d_in, d_out):
        self._hold(d_in, d_out)
        _l.check(self._lib.mi355_gray_weighted(self._h, _ptr(d_in), _ptr(d_out)))

    def binarize_chain(self, d_gray, d_out, d_hist=None, d_thr=None):
        self._hold(d_gray, d_out, d_hist, d_thr)
        _l.check(self._lib.mi355_binarize_chain(self._h, _ptr(d_gray), _ptr(d_out), _ptr(d_hist),
                                                _ptr(d_thr)))

    def conv_kxk(self, d_in, d_out, k):
        """The K x K filter of the reference's filter study (noise_filter_benchmark/v2.cu:36-80); k: K*K floats."""
        self._hold(d_in, d_out)
        k = np.ascontiguousarray(k, dtype=np.float32).reshape(-1)
        K = int(round(k.size ** 0.5))
        assert K * K == k.size
        _l.check(self._lib.mi355_conv_kxk(self._h, _ptr(d_in), _ptr(d_out), k.ctypes.data, K))

    def heat_map(self, d_cur, d_prev, d_out):
        self._hold(d_cur, d_prev, d_out)
        _l.check(self._lib.mi355_heat_map(self._h, _ptr(d_cur), _ptr(d_prev), _ptr(d_out)))

    def red_dense(self, d_cur, d_prev, d_out):
        self._hold(d_cur, d_prev, d_out)
        _l.check(self._lib.mi355_red_dense(self._h, _ptr(d_cur), _ptr(d_prev), _ptr(d_out)))

    def red_overlap(self, d_img, d_xs, d_count=None, count=0):
        self._hold(d_img, d_xs, d_count)
        _l.check(self._lib.mi355_red_overlap(self._h, _ptr(d_img), _ptr(d_xs), _ptr(d_count), count))

    def red_stream_batch(self, d_offsets, d_xs, nframes, d_frames, clear=True, stride=None):
        """Red motion maps of a batch from its packed stream (kernels.cu:513-518 per frame)."""
        self._hold(d_offsets, d_xs, d_frames)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_red_stream_batch(self._h, _ptr(d_offsets), _ptr(d_xs), nframes, _ptr(d_frames),
                                                  stride, int(bool(clear))))

    def conv3x3(self, d_in, d_out):
        self._hold(d_in, d_out)
        _l.check(self._lib.mi355_conv3x3(self._h, _ptr(d_in), _ptr(d_out)))

    def median5x5(self, d_in, d_out):
        self._hold(d_in, d_out)
        _l.check(self._lib.mi355_median5x5(self._h, _ptr(d_in), _ptr(d_out)))

    def filter_batch(self, op, d_in, d_out, nframes, d_in2=None, stride=None):
        """Batched per-frame filter (lib.OP_*): one launch per kernel for nframes frames."""
        self._hold(d_in, d_out, d_in2)
        stride = self.total if stride is None else stride
        _l.check(self._lib.mi355_filter_batch(self._h, int(op), _ptr(d_in), _ptr(d_in2), _ptr(d_out), stride,
                                              nframes))

    # -- measurement ------------------------------------------------------------------------------
    def set_timing(self, on):
        _l.check(self._lib.mi355_set_timing(self._h, int(bool(on))))

    def reset_timing(self):
        _l.check(self._lib.mi355_reset_timing(self._h))

    def get_kernel_timing(self):
        """(ms in k_diff_pack, ms in k_scan_groups, ms in k_expand, launches) since reset."""
        a, b, d, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int(0)
        _l.check(self._lib.mi355_get_kernel_timing(self._h, C.byref(a), C.byref(b), C.byref(d), C.byref(n)))
        return a.value, b.value, d.value, n.value

    def probe_clock(self, milliseconds=200):
        """Shader clock (MHz) the device holds under an integer-VALU load (csrc/diag.hip)."""
        mhz = C.c_double(0)
        _l.check(self._lib.mi355_probe_clock(self._h, int(milliseconds), C.byref(mhz)))
        return mhz.value

    def probe_hbm_read(self, megabytes=2048):
        """GB/s of a plain streaming read on this board (csrc/diag.hip)."""
        v = C.c_double(0)
        _l.check(self._lib.mi355_probe_hbm_read(self._h, int(megabytes), C.byref(v)))
        return v.value

    def probe_hbm_write(self, megabytes=2048, narrow=False):
        """GB/s of plain streaming writes on this board: 16 bytes per lane, or (narrow) the dense expansion's
        4-byte index + 1-byte value per lane (csrc/diag.hip)."""
        v = C.c_double(0)
        _l.check(self._lib.mi355_probe_hbm_write(self._h, int(megabytes), 1 if narrow else 0, C.byref(v)))
        return v.value

    def get_timing(self):
        """(ms in the diff/threshold/pack kernel, ms in pack+scan+gather, launches) since reset."""
        a, b, n = C.c_double(0), C.c_double(0), C.c_int(0)
        _l.check(self._lib.mi355_get_timing(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value


# -- compact wire format, host side ---------------------------------------------------------------------------------------
def cwire_frame_bytes(n, e):
    """Bytes of one compact record: 8 + 2 * pad4(n) + 4 * e."""
    return _l.load().mi355_cwire_frame_bytes(int(n), int(e))


def cwire_bytes_max(frame_bytes, nframes):
    """Largest compact stream of nframes frames of frame_bytes bytes: nframes * (8 + 2 * pad4(frame_bytes))."""
    return _l.load().mi355_cwire_bytes_max(int(frame_bytes), int(nframes))


def cwire_budget_entries(frame_bytes, record_bytes):
    """The most entries a record of a frame of frame_bytes bytes may hold so that it fits record_bytes whatever its escapes:
    a sender's per-socket byte budget as a budget of cwire_budget_cwire_batch."""
    return _l.load().mi355_cwire_budget_entries(int(frame_bytes), int(record_bytes))


def activity_cells(width, height, cell_w, cell_h):
    """(cells, grid_w, grid_h) of the motion grid of activity_batch / cwire_activity_batch: ceil(width / cell_w) columns,
    ceil(height / cell_h) rows; all 0 for an argument below 1."""
    gw, gh = C.c_int(0), C.c_int(0)
    cells = _l.load().mi355_activity_cells(int(width), int(height), int(cell_w), int(cell_h), C.byref(gw), C.byref(gh))
    return cells, gw.value, gh.value


def wall_thumb_size(width, height, k):
    """(pixels, tw, th) of the thumbnail of a width x height state at scale k of wall_compose_batch: ceil(width / k) by
    ceil(height / k); all 0 for a width or height below 1 or a k outside 1 .. 16."""
    tw, th = C.c_int(0), C.c_int(0)
    pixels = _l.load().mi355_wall_thumb_size(int(width), int(height), int(k), C.byref(tw), C.byref(th))
    return pixels, tw.value, th.value


def thumb_cwire_host(state, width, height, k, threshold, thumb, tile_mask=None, capacity_bytes=None):
    """thumb_cwire_batch for one stream computed on the host (no GPU, no core) and its definition: (record bytes, n, e) of the
    thumbnail at scale k of the uint8 `state` (3*width*height bytes) against the held thumbnail `thumb` (uint8 numpy array of
    3*tw*th bytes, updated in place), processing exactly the pixels that tile_mask (uint32 words over the state's tiles; None:
    every tile) requires.  The record is b"" and thumb stays as it is when it does not fit capacity_bytes (default: always
    enough); n and e are exact either way."""
    L = _l.load()
    state = np.ascontiguousarray(np.frombuffer(state, np.uint8) if isinstance(state, (bytes, bytearray)) else state, dtype=np.uint8)
    assert isinstance(thumb, np.ndarray) and thumb.dtype == np.uint8 and thumb.flags.c_contiguous
    assert state.size == 3 * int(width) * int(height) and thumb.size == 3 * wall_thumb_size(width, height, k)[0]
    mask = None if tile_mask is None else np.ascontiguousarray(tile_mask, dtype=np.uint32)
    if capacity_bytes is None:
        capacity_bytes = L.mi355_cwire_bytes_max(thumb.size, 1)
    out = np.zeros(max(int(capacity_bytes), 1), np.uint8)
    n, e, nbytes = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    _l.check(L.mi355_thumb_cwire_host(state.ctypes.data, int(width), int(height), int(k), int(threshold),
                                      None if mask is None else mask.ctypes.data, thumb.ctypes.data, out.ctypes.data,
                                      int(capacity_bytes), C.byref(n), C.byref(e), C.byref(nbytes)))
    fits = nbytes.value <= int(capacity_bytes)
    return (out[:nbytes.value].tobytes() if fits else b""), n.value, e.value


def cwire_apply_host(state, buf, nframes):
    """The client on the host (no GPU): applies nframes compact records of `buf` to `state` (uint8 numpy array, changed in
    place) and returns the bytes consumed.  Malformed input raises lib.Mi355Error; its `consumed` attribute holds the bytes
    of the frames before the bad one, which stay applied."""
    L = _l.load()
    assert isinstance(state, np.ndarray) and state.dtype == np.uint8 and state.flags.c_contiguous
    buf = np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else buf, dtype=np.uint8)
    consumed = C.c_size_t(0)
    rc = L.mi355_cwire_apply_host(state.ctypes.data, state.size, buf.ctypes.data, buf.size, int(nframes), C.byref(consumed))
    if rc != _l.OK:
        err = _l.Mi355Error(rc, L.mi355_last_error().decode(errors="replace"))
        err.consumed = consumed.value
        raise err
    return consumed.value


def cwire_check_host(buf, counts, escapes, frame_bytes):
    """The verdicts of cwire_check_batch computed on the host (no GPU, no core): uint32[nrecords, 4] for the records of `buf`
    that the headers counts / escapes describe, on a frame of frame_bytes bytes.  Headers that cannot be followed (more escapes
    than entries, more entries than frame bytes, records past the end of buf) raise lib.Mi355Error."""
    L = _l.load()
    buf = np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else buf, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    escapes = np.ascontiguousarray(escapes, dtype=np.uint32)
    assert counts.size == escapes.size
    verdicts = np.zeros((counts.size, 4), np.uint32)
    _l.check(L.mi355_cwire_check_host(int(frame_bytes), buf.ctypes.data, buf.size, counts.ctypes.data, escapes.ctypes.data,
                                      counts.size, verdicts.ctypes.data))
    return verdicts


def cwire_despeckle_host(width, height, buf, counts, escapes, states, need, stride=None, capacity_bytes=None):
    """cwire_despeckle_cwire_batch computed on the host (no GPU, no core) and its definition: (dropped uint32[nstreams], offsets
    uint32[nstreams + 1], frame_pos uint64[nstreams + 1], out uint8[capacity_bytes]) for the records of `buf` that the headers
    counts / escapes describe.  `states` (uint8, nstreams states `stride` bytes apart) is reverted in place at the dropped
    entries.  The capacity defaults to cwire_bytes_max, which always suffices."""
    L = _l.load()
    buf = _as_bytes(buf)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    escapes = np.ascontiguousarray(escapes, dtype=np.uint32)
    need = np.ascontiguousarray(need, dtype=np.uint32)
    nstreams = counts.size
    assert escapes.size == nstreams and need.size == nstreams
    assert isinstance(states, np.ndarray) and states.dtype == np.uint8 and states.flags.c_contiguous
    n = 3 * int(width) * int(height)
    stride = n if stride is None else int(stride)
    assert nstreams == 0 or stride < n or states.size >= (nstreams - 1) * stride + n
    if capacity_bytes is None:
        capacity_bytes = L.mi355_cwire_bytes_max(n, nstreams)
    dropped = np.zeros(nstreams, np.uint32)
    offsets = np.zeros(nstreams + 1, np.uint32)
    frame_pos = np.zeros(nstreams + 1, np.uint64)
    out = np.zeros(max(int(capacity_bytes), 1), np.uint8)
    _l.check(L.mi355_cwire_despeckle_host(int(width), int(height), buf.ctypes.data, buf.size, counts.ctypes.data, escapes.ctypes.data,
                                          states.ctypes.data, stride, nstreams, need.ctypes.data, dropped.ctypes.data,
                                          offsets.ctypes.data, frame_pos.ctypes.data, out.ctypes.data, int(capacity_bytes)))
    return dropped, offsets, frame_pos, out[:int(capacity_bytes)]


def cwire_split_pieces_max(n, e, max_bytes):
    """A sufficient piece count for a record of n entries and e escapes split at max_bytes (0 for a max_bytes outside
    [64, 65536])."""
    return _l.load().mi355_cwire_split_pieces_max(int(n), int(e), int(max_bytes))


def cwire_split_bytes_max(n, e, max_bytes):
    """A sufficient byte count for the pieces of a record of n entries and e escapes split at max_bytes."""
    return _l.load().mi355_cwire_split_bytes_max(int(n), int(e), int(max_bytes))


def cwire_split_host(buf, counts, escapes, frame_bytes, max_bytes, piece_capacity=None, capacity_bytes=None):
    """cwire_split_cwire_batch computed on the host (no GPU, no core) and its definition: (piece_first uint32[nrecords + 1],
    piece_pos uint64[piece_capacity + 1], out uint8[capacity_bytes]) for the records of `buf` that the headers counts / escapes
    describe.  The capacities default to the helpers' sums, which always suffice."""
    L = _l.load()
    buf = np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else buf, dtype=np.uint8)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    escapes = np.ascontiguousarray(escapes, dtype=np.uint32)
    assert counts.size == escapes.size
    if piece_capacity is None:
        piece_capacity = sum(L.mi355_cwire_split_pieces_max(int(n), int(e), int(max_bytes)) for n, e in zip(counts, escapes))
    if capacity_bytes is None:
        capacity_bytes = sum(L.mi355_cwire_split_bytes_max(int(n), int(e), int(max_bytes)) for n, e in zip(counts, escapes))
    piece_first = np.zeros(counts.size + 1, np.uint32)
    piece_pos = np.zeros(int(piece_capacity) + 1, np.uint64)
    out = np.zeros(max(int(capacity_bytes), 1), np.uint8)
    _l.check(L.mi355_cwire_split_host(int(frame_bytes), buf.ctypes.data, buf.size, counts.ctypes.data, escapes.ctypes.data,
                                      counts.size, int(max_bytes), piece_first.ctypes.data, piece_pos.ctypes.data,
                                      int(piece_capacity), out.ctypes.data, int(capacity_bytes)))
    return piece_first, piece_pos, out[:int(capacity_bytes)]


def cwire_runs_frame_bytes(n, e, r):
    """Bytes of a record of n entries, e escapes and r runs in the run form."""
    return _l.load().mi355_cwire_runs_frame_bytes(int(n), int(e), int(r))


def cwire_runs_bytes_max(frame_bytes, nrecords, policy):
    """A sufficient output size for cwire_runs_encode_* of nrecords records of frames of frame_bytes bytes under `policy` (0 for
    an unknown policy)."""
    return _l.load().mi355_cwire_runs_bytes_max(int(frame_bytes), int(nrecords), int(policy))


def _as_bytes(buf):
    return np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else buf, dtype=np.uint8)


def cwire_runs_encode_host(buf, counts, escapes, frame_bytes, policy, capacity_bytes=None):
    """cwire_runs_encode_batch computed on the host (no GPU, no core) and its definition: (forms uint32[nrecords, 4], pos
    uint64[nrecords + 1], out uint8[capacity_bytes]) for the records of `buf` that the headers counts / escapes describe.  The
    capacity defaults to cwire_runs_bytes_max."""
    L = _l.load()
    buf = _as_bytes(buf)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    escapes = np.ascontiguousarray(escapes, dtype=np.uint32)
    assert counts.size == escapes.size
    if capacity_bytes is None:
        capacity_bytes = L.mi355_cwire_runs_bytes_max(int(frame_bytes), counts.size, int(policy))
    forms = np.zeros((counts.size, 4), np.uint32)
    pos = np.zeros(counts.size + 1, np.uint64)
    out = np.zeros(max(int(capacity_bytes), 1), np.uint8)
    _l.check(L.mi355_cwire_runs_encode_host(int(frame_bytes), buf.ctypes.data, buf.size, counts.ctypes.data, escapes.ctypes.data,
                                            counts.size, int(policy), forms.ctypes.data, pos.ctypes.data, out.ctypes.data,
                                            int(capacity_bytes)))
    return forms, pos, out[:int(capacity_bytes)]


def cwire_runs_decode_host(buf, forms, frame_bytes, capacity_bytes=None, out=None):
    """cwire_runs_decode_batch computed on the host and its definition: (frame_pos uint64[nrecords + 1], cwire uint8[capacity_bytes])
    from the link bytes `buf` and the sender's table `forms`.  The capacity defaults to the records' size.  `out`: an array to
    decode into (what a refused call had written before it stopped stays there)."""
    L = _l.load()
    buf = _as_bytes(buf)
    forms = np.ascontiguousarray(forms, dtype=np.uint32).reshape(-1, 4)
    if capacity_bytes is None:
        capacity_bytes = sum(L.mi355_cwire_frame_bytes(int(f[1]), int(f[2])) for f in forms) if out is None else out.size
    frame_pos = np.zeros(forms.shape[0] + 1, np.uint64)
    if out is None:
        out = np.zeros(max(int(capacity_bytes), 1), np.uint8)
    _l.check(L.mi355_cwire_runs_decode_host(int(frame_bytes), buf.ctypes.data, buf.size, forms.ctypes.data, forms.shape[0],
                                            frame_pos.ctypes.data, out.ctypes.data, int(capacity_bytes)))
    return frame_pos, out[:int(capacity_bytes)]


def cwire_fec_groups_max(piece_capacity, nrecords, group):
    """A sufficient group count for piece_capacity pieces in nrecords records at `group` pieces per group (0 for a group outside
    1 .. 255)."""
    return _l.load().mi355_cwire_fec_groups_max(int(piece_capacity), int(nrecords), int(group))


def cwire_fec_host(pieces, pieces_bytes, piece_first, piece_pos, piece_capacity, group, nparity, pitch, group_capacity=None,
                   capacity_bytes=None, fill=0):
    """cwire_fec_batch computed on the host (no GPU, no core) and its definition: (fec_first uint32[nrecords + 1], fec_len
    uint32[group_capacity], out uint8[capacity_bytes]) for the pieces of cwire_split_host / _cwire_batch.  The capacities default
    to what always suffices; what the call does not write keeps `fill` (fec_len: fill in every byte)."""
    L = _l.load()
    pieces = np.ascontiguousarray(pieces, dtype=np.uint8)
    piece_first = np.ascontiguousarray(piece_first, dtype=np.uint32)
    piece_pos = np.ascontiguousarray(piece_pos, dtype=np.uint64)
    nrecords = piece_first.size - 1
    assert pieces.size >= pieces_bytes and piece_pos.size >= piece_capacity + 1
    if group_capacity is None:
        group_capacity = L.mi355_cwire_fec_groups_max(int(piece_capacity), nrecords, int(group))
    if capacity_bytes is None:
        capacity_bytes = int(group_capacity) * int(nparity) * int(pitch)
    fec_first = np.zeros(nrecords + 1, np.uint32)
    fec_len = np.full(max(int(group_capacity), 1), fill * 0x01010101, np.uint32)
    out = np.full(max(int(capacity_bytes), 1), fill, np.uint8)
    _l.check(L.mi355_cwire_fec_host(pieces.ctypes.data, int(pieces_bytes), piece_first.ctypes.data, piece_pos.ctypes.data,
                                    int(piece_capacity), nrecords, int(group), int(nparity), int(pitch), fec_first.ctypes.data,
                                    fec_len.ctypes.data, int(group_capacity), out.ctypes.data, int(capacity_bytes)))
    return fec_first, fec_len[:int(group_capacity)], out[:int(capacity_bytes)]


def cwire_fec_repair_host(slots, p, q, fec_len):
    """One group repaired on the host (no GPU, no core), the definition of cwire_fec_repair_batch: slots is the group's members
    in slot order, uint8 arrays or None for a lost one; p, q its parity blocks or None.  Returns (rebuilt blocks, one uint8 array
    of fec_len bytes per lost slot, and their verdicts, lib.FEC_BAD_* flags)."""
    L = _l.load()
    keep = [None if s is None else np.ascontiguousarray(s, dtype=np.uint8) for s in slots]
    p = None if p is None else np.ascontiguousarray(p, dtype=np.uint8)
    q = None if q is None else np.ascontiguousarray(q, dtype=np.uint8)
    assert all(x is None or x.size >= fec_len for x in (p, q))
    ptrs = (C.c_void_p * max(len(keep), 1))(*[None if s is None else s.ctypes.data for s in keep])
    lens = np.array([0 if s is None else s.size for s in keep] + [0], np.uint32)
    lost = sum(s is None for s in keep)
    outs = [np.zeros(int(fec_len), np.uint8) for _ in range(2)]
    verdict = np.zeros(2, np.uint32)
    _l.check(L.mi355_cwire_fec_repair_host(len(keep), C.addressof(ptrs), lens.ctypes.data, _ptr(p), _ptr(q), int(fec_len),
                                           outs[0].ctypes.data, outs[1].ctypes.data, verdict.ctypes.data))
    return outs[:lost], verdict[:lost]


def state_tiles(frame_bytes):
    """Tiles of 4096 bytes of a state of frame_bytes bytes (the last may be ragged): the rows of a digest array."""
    return _l.load().mi355_state_tiles(int(frame_bytes))


def state_digest_host(state):
    """The digests of state_digest_batch computed on the host (no GPU, no core) and their definition: uint32[tiles, 2] for the
    uint8 array `state` -- per tile of 4096 bytes, zero-extended, the sum of its little-endian words and the sum of their
    position-keyed mixes, both mod 2^32."""
    L = _l.load()
    state = np.ascontiguousarray(np.frombuffer(state, np.uint8) if isinstance(state, (bytes, bytearray)) else state, dtype=np.uint8)
    digests = np.zeros((L.mi355_state_tiles(state.size), 2), np.uint32)
    _l.check(L.mi355_state_digest_host(state.ctypes.data, state.size, digests.ctypes.data))
    return digests
