"""A caller's stream that is provably still busy when the library's entries return: the tool of test_gpu_caller_streams.py and of
the caller's-stream tests of test_gpu_acquisition.py.  A helper module like the *_model.py ones: no tests in here.

What a test does with it: hold() puts a delay on a non-blocking stream of the test's own and records the event `gate` directly behind
it; the test then enqueues its producer (an asynchronous H2D from pinned memory into a device buffer that holds 0x5A until then), the
library's `_dev` entries and its consumer (an asynchronous D2H into pinned memory) behind the gate, calls assert_held() once its last
library call has returned, and only then waits, for THAT stream alone (hipStreamSynchronize; never hipDeviceSynchronize, which would
hide work stranded on another stream).  assert_held() is hipEventQuery(gate) == hipErrorNotReady: while it holds, nothing the test
enqueued behind the gate can have run, so everything the library enqueued ran later than its host call returned, and a kernel, fill or
copy of the library's that went to another stream ran against the filler, not the samples.  A test whose delay had already drained
would prove nothing, so it fails there, with "stall too short".

THE DELAY.  Two candidates were measured on an MI355X (ROCm 7.2, the gate queried right after the enqueueing host call returned and
then waited for; three repeats each, the first discarded):
  - a pageable hipMemcpyAsync of a large block in front (what test_gpu_acquisition.py used to do): the host call itself takes 1.2 ms
    (64 MiB), 1.8 ms (96 MiB), 4.8 ms (256 MiB), and the gate is ready 0.015 ms after it returns.  The copy is over, all of it, before
    the host gets control back: it holds NOTHING open, and a test built on it is vacuous.
  - torch.cuda._sleep(cycles) on torch.cuda.ExternalStream(stream), a kernel that spins on the shader clock: the host call takes
    0.012 - 0.034 ms, and the gate becomes ready 0.42 ms (10^6 cycles), 4.157 ms (10^7) and 41.50 ms (10^8) after it returned, to
    three digits the same in every repeat: 2.41 cycles per nanosecond.
So the delay is torch.cuda._sleep with HOLD_CYCLES = 4.8 * 10^8 cycles: measured busy for 200.2 ms after a host call of 0.02 - 0.03 ms
(three repeats: 200.233, 200.217, 200.227 ms).  The clock does not run faster than this; where it runs slower the hold is longer.
Behind it, hold() returning to assert_held() passing, the 100 holds of the two test files measured a median of 0.05 ms; the device-
resident chains (three stages, a search and a decision, the copies) 0.13 - 0.20 ms; and the LONGEST, test D of the (5120, 5119)
resampler, 7.4 ms (7.0 and 7.5 ms in two other sessions, and once 58 ms before every new stream was given a first piece of work to
finish at creation: the runtime sets up something of a stream's on first use, on the host).  200.2 / 7.4: the hold is 27 times the
longest enqueue sequence, 1000 times the usual one, against the 10 that host jitter on a shared machine asks for.  spans and
longest_enqueue_ms() hold the figures of the running session.

torch is imported here, at import time, because it brings its own HIP runtime, which must be the first one the process loads (see
test_gpu_mixed_grid.py); the ctypes handle below then names that same runtime, and so does the product library."""
import ctypes as C
import time

import numpy as np
import torch   # before the HIP library, see above

HOLD_CYCLES = 480_000_000
HOLD_MS_MEASURED = 200.2
ENQUEUE_MS_MEASURED = 7.4      # the longest hold() -> assert_held() span of any test; the median is 0.05
FILL = 0x5A
H2D, D2H = 1, 2
NOT_READY = 600                # hipErrorNotReady

_longest = [0.0, ""]
spans = []                     # (milliseconds, tag) of every assert_held() that passed
# Pinned memory is handed out as numpy views, and a view must never outlive its memory (a failing test's report prints the arrays it
# holds): blocks go back to this pool when their stream closes and are reused, never freed before the process ends.
_pool, _pinned_at = {}, set()


def longest_enqueue_ms():
    """(milliseconds, tag) of the longest hold() -> assert_held() span of this process so far"""
    return tuple(_longest)


def _hip():
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipHostFree.argtypes = [C.c_void_p]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    hip.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    hip.hipEventCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventQuery.argtypes = [C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


class HeldStream:
    """One non-blocking stream of the caller's, its gate, and the pinned and device buffers of one test.  `stream` is the integer the
    library's `stream=` arguments and set_stream take.  Use as a context manager, or close() it: that waits for the stream first."""

    def __init__(self):
        self.hip = _hip()
        s, g, e = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0          # hipStreamNonBlocking, like the library's own
        assert self.hip.hipEventCreateWithFlags(C.byref(g), 2) == 0           # hipEventDisableTiming
        assert self.hip.hipEventCreateWithFlags(C.byref(e), 2) == 0
        self._s, self._gate, self._order = s, g, e
        self.stream = s.value
        self._torch_stream = torch.cuda.ExternalStream(self.stream)
        with torch.cuda.stream(self._torch_stream):     # the stream's first work, waited for: what the runtime sets up on a stream's first
            torch.cuda._sleep(1)                         # use has cost up to 58 ms of host time when it fell behind a hold
        assert self.hip.hipStreamSynchronize(s) == 0
        self._pinned, self._device = [], []
        self._held_at, self.tag = None, ""
        self._owned = []

    def own(self, handle):
        """a library handle that works on this stream: close() closes it (its own close() may be called earlier) BEFORE the stream goes,
        also when the test fails half-way, so that no handle outlives the stream its last call ran on"""
        self._owned.append(handle)
        return handle

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- the hold
    def hold(self, tag=""):
        """the delay, and the gate directly behind it"""
        with torch.cuda.stream(self._torch_stream):
            torch.cuda._sleep(HOLD_CYCLES)
        assert self.hip.hipEventRecord(self._gate, self._s) == 0
        self._held_at, self.tag = time.perf_counter(), tag

    def assert_held(self):
        """after the test's last library call has returned, before it waits for anything: the delay is still running, so nothing
        behind the gate has run yet"""
        assert self._held_at is not None, "assert_held() without a hold()"
        q = self.hip.hipEventQuery(self._gate)
        self.hip.hipGetLastError()                    # (a not-ready answer is no error of anybody's: leave none behind for the library's own checks)
        span = (time.perf_counter() - self._held_at) * 1e3
        assert q == NOT_READY, "stall too short: the gate answered %d, %.3f ms after the hold was enqueued (%s)" % (q, span, self.tag)
        spans.append((span, self.tag))
        if span > _longest[0]:
            _longest[:] = [span, self.tag]
        return span

    def sync(self):
        """waits for THIS stream only"""
        assert self.hip.hipStreamSynchronize(self._s) == 0

    # ---- ordering against another stream by the caller's own event
    def record(self):
        """an event behind everything enqueued on this stream so far (one per stream: the last record() counts)"""
        assert self.hip.hipEventRecord(self._order, self._s) == 0
        return self._order

    def wait_for(self, other):
        """everything enqueued on this stream from now on runs behind what `other` (a HeldStream) has enqueued so far; no host wait"""
        assert self.hip.hipStreamWaitEvent(self._s, other.record(), 0) == 0

    # ---- buffers
    def device(self, nbytes, fill=FILL):
        """device memory filled with `fill`, the fill finished before this returns"""
        p = C.c_void_p()
        nbytes = max(int(nbytes), 1)
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        assert self.hip.hipMemset(p, fill, nbytes) == 0
        assert self.hip.hipDeviceSynchronize() == 0   # (before anything is held: the fill is ordered on the NULL stream only)
        self._device.append(p)
        return p.value

    def pinned(self, nbytes, fill=0xEE):
        """pinned host memory as a uint8 array (from the module's pool: valid, though reused, after close())"""
        nbytes = max(int(nbytes), 1)
        size = 4096
        while size < nbytes:
            size *= 2
        free = _pool.setdefault(size, [])
        if free:
            p = free.pop()
        else:
            p = C.c_void_p()
            assert self.hip.hipHostMalloc(C.byref(p), size, 0) == 0
            _pinned_at.add(p.value)
        self._pinned.append((size, p))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (size,))[:nbytes]
        a[:] = fill
        return a

    def stage(self, arr):
        """the bytes of arr in pinned memory (a uint8 array), for an h2d() that must not stop to allocate"""
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        out = self.pinned(raw.size)
        out[:raw.size] = raw
        return out[:raw.size]

    def h2d(self, d_ptr, staged):
        """asynchronous copy of a stage()d array to d_ptr, on this stream"""
        assert staged.ctypes.data in _pinned_at, "h2d() takes what stage() returned"
        if staged.size:
            assert self.hip.hipMemcpyAsync(d_ptr, staged.ctypes.data, staged.size, H2D, self._s) == 0

    def d2h(self, d_ptr, nbytes, out=None):
        """asynchronous copy of nbytes at d_ptr to pinned memory (out: an array of pinned(), else a new one), on this stream -> the
        uint8 array they land in, valid once sync() has returned"""
        out = out if out is not None else self.pinned(nbytes)
        assert out.ctypes.data in _pinned_at and out.size >= nbytes
        assert self.hip.hipMemcpyAsync(out.ctypes.data, d_ptr, int(nbytes), D2H, self._s) == 0
        return out

    def memset(self, d_ptr, value, nbytes):
        """asynchronous fill on this stream"""
        assert self.hip.hipMemsetAsync(d_ptr, value, int(nbytes), self._s) == 0

    def put(self, d_ptr, arr):
        """blocking copy to the device (the synchronous reference runs; nothing may be held)"""
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        if raw.size:
            assert self.hip.hipMemcpy(d_ptr, raw.ctypes.data, raw.size, H2D) == 0

    def get(self, d_ptr, nbytes):
        """blocking copy from the device of what has been WAITED for (the handle's synchronize(), or sync()); this does not wait for
        any stream the library created"""
        out = np.zeros(max(int(nbytes), 1), np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data, d_ptr, int(nbytes), D2H) == 0
        return out[:int(nbytes)]

    def close(self):
        if self._s is None:
            return
        self.hip.hipStreamSynchronize(self._s)
        for h in reversed(self._owned):
            h.close()
        self._owned = []
        for p in self._device:
            self.hip.hipFree(p)
        for size, p in self._pinned:
            _pool[size].append(p)
        self._device, self._pinned = [], []
        self.hip.hipEventDestroy(self._gate)
        self.hip.hipEventDestroy(self._order)
        self.hip.hipStreamDestroy(self._s)
        self._s = None
