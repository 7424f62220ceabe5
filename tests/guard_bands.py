"""Poisoned guard bands around a device entry's buffers.  A helper module like stage_instantiations.py, not a test and not a conftest.

The GPU files cut their blocks out of one contiguous buffer (the bytes in front of a block are the stream's true past, the bytes behind
it its true future) and keep everything else in zero-filled allocations of its own, so a kernel that reads outside what it was handed
finds the right words, or zeros.  Here a payload sits in the middle of ONE allocation

    [ guard | pad | payload | guard ]          every byte outside the payload = fill

whose last payload byte is directly followed by guard and whose first byte is aligned to `align` and, below 16, to nothing larger (an
element-only aligned input starts on an odd element).  The same call runs once per fill of FILLS; a word that depends on a byte outside
the payload differs between two of the runs (same_words), whatever the model's bar would forgive.  As float32 0xFF is a NaN and 0x7F is
3.39e38; as int8 they are -1 and 127.  A value that is loaded and never used cannot be seen this way.

The guards are 64 KiB a side: a condition, not a measurement.  That is more than any tile, halo or prefetch in csrc/, so a stray read
stays inside the allocation and the result is a wrong word, never a fault.  No payload is placed at the end of an allocation or a page.

tests/test_guard_bands_host.py holds the arithmetic and shows on a numpy stand-in that the check can fail."""
import numpy as np

GUARD = 65536
FILLS = (0x00, 0xFF, 0x7F)


def layout(base, nbytes, align, guard=GUARD):
    """the allocation at address `base` that carries nbytes of payload -> (pad, total): the payload starts at base + guard + pad and
    ends where the back guard begins.  Its address is a multiple of align; for align < 16 it is an ODD multiple, so it is aligned to no
    larger power of two."""
    assert align >= 1 and align & (align - 1) == 0 and align <= 256 and guard >= GUARD and nbytes >= 0
    start = base + guard
    pad = -start % align
    if align < 16 and (start + pad) % (2 * align) == 0:
        pad += align
    return pad, guard + pad + nbytes + guard


class Carved(int):
    """the payload's address (an int: pass it on, add to it), with what guards_intact needs"""

    def __new__(cls, base, pad, payload, fill, guard):
        self = super().__new__(cls, base + guard + pad)
        self.base, self.pad, self.payload, self.fill, self.guard = base, pad, payload, fill, guard
        self.nbytes = payload.size
        self.total = guard + pad + payload.size + guard
        return self

    @property
    def end(self):
        return int(self) + self.nbytes


def _bytes(payload):
    """payload: an array (its bytes), or a byte count -> (bytes or None, count)"""
    if isinstance(payload, (int, np.integer)):
        return None, int(payload)
    b = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    return b, b.size


def carve(hipbuf, payload_bytes, fill, *, align, guard=GUARD):
    """one allocation of guard + pad + payload + guard bytes, all `fill`, the payload copied into its middle -> its address (a Carved).
    payload_bytes: an array, or a byte count for an output buffer, which then keeps the fill and is remembered as such."""
    data, n = _bytes(payload_bytes)
    # hipMalloc's addresses are multiples of 256, so the pad is known before the address is (and checked once it is)
    pad, total = layout(0, n, align, guard)
    base = hipbuf.alloc(total, fill=fill)
    assert base % 256 == 0 and layout(base, n, align, guard) == (pad, total)
    if data is None:
        data = np.full(n, fill, np.uint8)
    c = Carved(base, pad, data.copy(), fill, guard)
    if n:
        assert hipbuf.hip.hipMemcpy(int(c), c.payload.ctypes.data, n, 1) == 0
    assert int(c) % align == 0 and (align >= 16 or int(c) % (2 * align) == align) and c.end + guard == base + total
    return c


def guards_intact(hipbuf, c, payload=True):
    """both guards (the pad with the front one) still hold the fill, and, with payload=True, the payload is what was put there"""
    front = hipbuf.download(c.base, c.guard + c.pad, np.uint8)
    back = hipbuf.download(c.end, c.guard, np.uint8)
    ok = bool((front == c.fill).all() and (back == c.fill).all())
    if payload and c.nbytes:
        ok = ok and bool((hipbuf.download(int(c), c.nbytes, np.uint8) == c.payload).all())
    return ok


def read_back(hipbuf, c, dtype):
    """the payload as it is now"""
    return hipbuf.download(int(c), c.nbytes, np.uint8).view(dtype)


def overlap(a, na, b, nb):
    """the byte ranges [a, a + na) and [b, b + nb) share a byte: what the entries that refuse aliasing look at"""
    return na > 0 and nb > 0 and a < b + nb and b < a + na


def disjoint(*carved):
    """no two carved allocations share a byte, so neither do their payloads, and no payload lies in another's guard"""
    spans = sorted((c.base, c.base + c.total) for c in carved)
    return all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:]))


def _flat(out):
    if isinstance(out, dict):
        return [(k, out[k]) for k in sorted(out)]
    if isinstance(out, (list, tuple)):
        return list(enumerate(out))
    return [(0, out)]


def _name(fill):
    return "0x%02X" % fill if isinstance(fill, int) else str(fill)


def same_words(runs):
    """runs: {fill (or any name of a run): outputs} with outputs an array, a sequence of arrays or a dict of arrays (numbers count as arrays).  Every output has
    the same shape, type and BITS under every fill (a NaN equals itself, -0.0 is not 0.0)."""
    fills = list(runs)
    assert len(fills) >= 2, "one run shows nothing"
    first = _flat(runs[fills[0]])
    for f in fills[1:]:
        other = _flat(runs[f])
        assert [k for k, _ in other] == [k for k, _ in first], (fills[0], f)
        for (k, a), (_, b) in zip(first, other):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype, (k, _name(fills[0]), _name(f), a.shape, b.shape)
            diff = a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)
            assert not diff.any(), "output %r: runs %s and %s differ, first at byte %d of %d" % (
                k, _name(fills[0]), _name(f), int(np.flatnonzero(diff)[0]), diff.size)


# ---- the same layout in host memory, for the test that shows the check can fail ------------------------------------------------------
def carve_host(payload, fill, *, align, guard=GUARD, base=0x7F0000001000):
    """the allocation as a numpy byte array, laid out as if it stood at address `base` -> (bytes, offset of the payload)"""
    data, n = _bytes(payload)
    pad, total = layout(base, n, align, guard)
    buf = np.full(total, fill, np.uint8)
    buf[guard + pad:guard + pad + n] = data
    return buf, guard + pad


class Scattered:
    """A stage handle whose input does not lie where the caller of process_dev thinks.  The owning files' _feed functions walk ONE
    device buffer: call i gets d_x + done.  Wrapped in this, a _feed that makes one call of the whole stream from the made-up address
    `d_x` instead makes the calls `cuts`, call i reading pieces[i], a carved buffer of its own: no call has the stream's past in front
    of its pointer or the stream's future behind its last sample.  Outputs go behind each other where _feed put them, captured
    blocks too, so _feed's own filler checks and its return value stay what they are.

    signature: the names of process_dev's positional arguments behind d_in, one of SIGNATURES, so that every argument this touches is
    found by name: `n_in` (the call's length), `d_out` (moves on by the outputs delivered, 8 bytes each) and, where the stage has one,
    `out_cap` (the room left at d_out, which shrinks by them); `fmt` and `out_stride` pass through.  blocks: (R bytes, w bytes) of a
    captured block for the stages that capture."""
    FAKE = 0x10000                      # an address nothing is read from
    SIGNATURES = dict(stream=("fmt", "n_in", "d_out", "out_cap"),                 # gm_resampler, gm_excisor, gm_nuller, gm_stap
                      ddc=("n_in", "d_out", "out_cap"),
                      planes=("fmt", "n_in", "d_out", "out_stride"),              # gm_beamformer, gm_lcmv
                      channelizer=("fmt", "n_in", "d_out", "out_stride", "out_cap"))

    def __init__(self, handle, pieces, lengths, bytes_per_sample, signature="stream", blocks=None):
        assert len(pieces) == len(lengths)
        self._h, self._pieces, self._lengths, self._bps = handle, pieces, lengths, bytes_per_sample
        self._names, self._blocks = self.SIGNATURES[signature], blocks
        self._capture = None
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self._h, name)

    def capture(self, d_R=None, d_w=None, cap_blocks=0):
        self._capture = (d_R, d_w, cap_blocks) if d_R else None
        self._h.capture(d_R, d_w, cap_blocks)

    def process_dev(self, d_in, *args):
        assert len(args) == len(self._names), (args, self._names)
        a = dict(zip(self._names, args))
        assert d_in == self.FAKE and a["n_in"] == sum(self._lengths), "one call of the whole stream"
        d_out, room, got = a["d_out"], a.get("out_cap"), 0
        for piece, k in zip(self._pieces, self._lengths):
            assert piece.nbytes == k * self._bps
            a["n_in"], a["d_out"] = k, d_out + got * 8
            if room is not None:
                a["out_cap"] = room - got
            if self._capture:
                d_R, d_w, cap = self._capture
                nb = got // self._h.block
                self._h.capture(d_R + nb * self._blocks[0], d_w + nb * self._blocks[1], cap - nb)
            got += self._h.process_dev(piece, *[a[name] for name in self._names])
            self.calls += 1
        return got
