"""The caller's-stream contract of every streaming `_dev` entry (include/gnss_mi355x.h: "asynchronous on `stream` (NULL: the handle's
own)"): gm_frontend, gm_resampler, gm_excisor, gm_ddc, gm_channelizer and gm_nuller, driven the way a receiver that keeps its
conditioning chain on the GPU drives them, on a stream of the CALLER's that is provably still held back when each entry returns
(stream_stall.py: a spinning kernel in front, the event `gate` behind it, assert_held() after the last library call and before any
wait).  Nothing here is about arithmetic: every expected word comes from fresh handles of the same configuration run synchronously,
the handle's own stream, synchronize() after every call, the same cuts, and has to be met BIT FOR BIT (outputs, captures, stats(),
gains, PSD words, front-end state, whole buffers with their 0x5A filler).  The other test files tie those synchronous words to the
float64 models.  What a miss means is ordering: a kernel, fill or copy that the host layer (csrc/gm_api.hip: stage_*, *_launch, chain_*)
enqueued somewhere else than on the caller's stream reads the filler or an old history, and a join that does not wait lets the next
call or query overtake the held one.

Per handle: A one held call between its producer (H2D) and consumer (D2H); B consecutive held calls cut inside the history, no host
wait between them; C every documented join issued while a call is still held (synchronize() then the handle's own stream, stats(),
reset(), the host-buffer process(), a write_ring chain, and for the excisor set_gains / gains / psd / block_stats); D two streams of
the caller's ordered by the caller's event alone; E the excisor's adapt_dev -> process_dev chain; F the nuller's mode switch between
two held calls.  Then three device-resident chains on ONE held stream with an AcquisitionEngine behind them (set_stream), no host wait
between the first H2D and the last D2H.

Deliberately NOT tested:
  - destroying a handle with work in flight: hipFree waits for the device, so a test could not tell, and a failure would be a fault
    rather than a wrong word;
  - set_gains followed at once by a `_dev` call on another stream (the gains_ev wait): the window is a 1-16 KB copy on the handle's
    private stream and cannot be held open from outside;
  - a front-end query after a call on a caller's stream without synchronising that stream: the header documents that
    gm_frontend_synchronize waits for the handle's own stream only.
gm_frontend_process_dev_batch waits on the host for `stream` while it hands its descriptors over (the header says so), so a hold
cannot outlive that call: its test asserts the hold directly BEFORE the call instead."""
import numpy as np
import pytest

import stream_stall as SS            # (imports torch before the HIP library)
import fe_model as FM
from test_gpu_channelizer import _stream as _channelizer_stream
from test_gpu_ddc import _stream as _ddc_stream
from test_gpu_excise import _stream as _excise_stream
from test_gpu_nuller import _stream as _nuller_stream
from test_gpu_resample import _stream as _resample_stream

pytestmark = pytest.mark.gpu
GAP = 8                              # filler words behind every output (and between a channelizer's planes)


def _fmt(name):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if name == "i8" else _lib.FMT_C32


# ------------------------------------------------------------------------------------------------ one run's buffers
class Bufs:
    """the device buffers of one run (0x5A until something is written), the pinned arrays their words are copied to, and which of
    their bytes the calls were entitled to write"""

    def __init__(self, S):
        self.S, self.dev, self.host, self.used = S, {}, {}, {}
        self.got = 0                 # outputs so far (per plane)
        self.blocks = 0              # captured blocks so far

    def add(self, name, nbytes):
        self.dev[name] = (self.S.device(nbytes), nbytes)
        self.host[name] = self.S.pinned(nbytes)
        self.used[name] = []
        return self.dev[name][0]

    def ptr(self, name):
        return self.dev[name][0]

    def fetch_async(self):
        for name, (p, nbytes) in self.dev.items():
            self.S.d2h(p, nbytes, self.host[name])

    def fetch_now(self):
        for name, (p, nbytes) in self.dev.items():
            self.host[name][:] = self.S.get(p, nbytes)

    def words(self, prefix=""):
        return {prefix + k: v.copy() for k, v in self.host.items()}

    def check_filler(self, tag):
        for name, arr in self.host.items():
            free = np.ones(arr.size, bool)
            for lo, hi in self.used[name]:
                free[lo:hi] = False
            assert (arr[free] == SS.FILL).all(), (tag, name, "a word outside the call's outputs was written")
            assert not free.all() or name != "y", (tag, "no output at all")


class Mode:
    """the two ways every scenario is run: held (the caller's stream, nothing waited for until finish()) and synchronous (the
    handle's own stream, synchronize() after every call)"""

    def __init__(self, S, held, tag):
        self.S, self.held, self.tag = S, held, tag
        self.stream = S.stream if held else None

    def begin(self):
        if self.held:
            self.S.hold(self.tag)

    def load(self, d_ptr, staged):
        if self.held:
            self.S.h2d(d_ptr, staged)
        else:
            self.S.put(d_ptr, staged)

    def called(self, *handles):
        if not self.held:
            for h in handles:
                h.synchronize()

    def finish(self, *bufs):
        """the consumer, the proof that the stream was still held, then the wait for that stream alone"""
        if self.held:
            for b in bufs:
                b.fetch_async()
            self.S.assert_held()
            self.S.sync()
        else:
            for b in bufs:
                b.fetch_now()


def _same(tag, got, want):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for k in sorted(got):
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert g.shape == w.shape and g.dtype == w.dtype, (tag, k, g.shape, w.shape)
            bad = np.nonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[0]
            assert bad.size == 0, (tag, k, "%d bytes differ from the synchronous run, the first at byte %d" % (bad.size, bad[0]))
        else:
            assert g == w, (tag, k, g, w)


def _both(tag, scenario):
    """scenario(S, mode) -> dict of words and values: held against synchronous, bit for bit"""
    with SS.HeldStream() as S:
        want = scenario(S, Mode(S, False, tag))
    with SS.HeldStream() as S:
        got = scenario(S, Mode(S, True, tag))
    _same(tag, got, want)
    return got


# ------------------------------------------------------------------------------------------------ the stage handles
class Kind:
    """one configuration of one stage handle: how to make it, its input stream, its output buffers and one process_dev call"""
    fmt = "c32"
    write_ring = None

    def bps(self):
        return 2 if self.fmt == "i8" else 8

    def raw(self, x):
        return np.ascontiguousarray(x)

    def layout(self, S, x):
        b = Bufs(S)
        b.x = S.stage(self.raw(x))
        b.d_x = S.device(b.x.size)
        b.cap = self.cap(len(x))
        b.add("y", (b.cap + GAP) * 8)
        return b

    def cuts(self, n):
        """consecutive calls cut at the positions of self.at"""
        edges = [0] + [a for a in self.at if a < n] + [n]
        return list(zip(edges[:-1], edges[1:]))

    def extra(self, h):
        return {"stats": h.stats()}


class ResamplerKind(Kind):
    n = 6007

    def __init__(self, up, down, fmt):
        self.up, self.down, self.fmt = up, down, fmt
        self.name = "resampler_%d_%d_%s" % (up, down, fmt)
        from gnss_sdr_rs_amd import resample
        self.T = resample.plan(up, down)["taps"]
        self.at = (self.T - 1, 1000)

    def new(self):
        from gnss_sdr_rs_amd import resample
        return resample.Resampler(self.up, self.down)

    def x(self, n, seed):
        return _resample_stream(self.fmt, n, seed)

    def cap(self, n):
        return n * self.up // self.down + 4

    def call(self, h, b, lo, hi, stream):
        got = h.process_dev(b.d_x + lo * self.bps(), _fmt(self.fmt), hi - lo, b.ptr("y") + b.got * 8, b.cap - b.got, stream)
        b.got += got
        b.used["y"] = [(0, b.got * 8)]

    def write_ring(self, h, ring, x):
        """the rest of the stream through a front-end into the ring, this handle behind it"""
        return self.fe.write_ring(ring, x, resampler=h)


class ExcisorKind(Kind):
    def __init__(self, B, fmt, block_adapt):
        self.B, self.fmt, self.block_adapt = B, fmt, block_adapt
        self.name = "excisor_%d_%s%s" % (B, fmt, "_block" if block_adapt else "")
        self.n = 5 * B + 7
        self.at = (B // 2 - 1, 1000)
        self.thr = 150.0 if fmt == "i8" else 6.5

    def new(self):
        from gnss_sdr_rs_amd import excise
        ex = excise.Excisor(self.B, blank_threshold=self.thr)
        if self.block_adapt:
            ex.set_block_adapt(4.0, 1)
        return ex

    def x(self, n, seed):
        x = _excise_stream(self.fmt, n, seed)
        t = np.arange(n)
        tone = np.exp(2j * np.pi * 0.2 * t)                                    # something for the block-adapt mask to find
        if self.fmt == "i8":
            x = x.copy()
            keep = (x == -128)
            y = np.clip(x // 2 + np.stack([np.rint(50 * tone.real), np.rint(50 * tone.imag)], axis=1), -128, 127).astype(np.int8)
            y[keep] = -128
            return y
        return (x + 4.0 * tone).astype(np.complex64)

    def cap(self, n):
        return n + self.B

    def layout(self, S, x):
        b = Kind.layout(self, S, x)
        if self.block_adapt:
            b.cap_blocks = len(x) // (self.B // 2) + 8
            b.add("power", b.cap_blocks * self.B * 4)
            b.add("mask", b.cap_blocks * self.B)
        return b

    def call(self, h, b, lo, hi, stream):
        if self.block_adapt:
            h.block_capture(b.ptr("power") + b.blocks * self.B * 4, b.ptr("mask") + b.blocks * self.B, b.cap_blocks - b.blocks)
        got = h.process_dev(b.d_x + lo * self.bps(), _fmt(self.fmt), hi - lo, b.ptr("y") + b.got * 8, b.cap - b.got, stream)
        b.got += got
        b.used["y"] = [(0, b.got * 8)]
        if self.block_adapt and got >= self.B // 2:
            b.blocks += got // (self.B // 2) + 1
            b.used["power"], b.used["mask"] = [(0, b.blocks * self.B * 4)], [(0, b.blocks * self.B)]

    def extra(self, h):
        return {"stats": h.stats(), "block_stats": h.block_stats(), "gains": h.gains()}

    def write_ring(self, h, ring, x):
        return self.fe.write_ring(ring, x, excisor=h)


class DdcKind(Kind):
    n = 6007
    fmt = "real"

    def __init__(self, up, down):
        self.up, self.down = up, down
        self.name = "ddc_%d_%d" % (up, down)
        from gnss_sdr_rs_amd import ddc
        self.T = ddc.plan(0.2501, up, down)["taps"]
        self.at = (self.T - 1, 1000)

    def bps(self):
        return 1

    def new(self):
        from gnss_sdr_rs_amd import ddc
        return ddc.Ddc(0.2501, self.up, self.down, blank_threshold=100.0)

    def x(self, n, seed):
        return _ddc_stream(n, seed)

    def cap(self, n):
        return n * self.up // self.down + 4

    def call(self, h, b, lo, hi, stream):
        got = h.process_dev(b.d_x + lo, hi - lo, b.ptr("y") + b.got * 8, b.cap - b.got, stream)
        b.got += got
        b.used["y"] = [(0, b.got * 8)]

    def write_ring(self, h, ring, x):
        return h.write_ring(ring, x)


class ChannelizerKind(Kind):
    n = 6007

    def __init__(self, M, D, P, channels, fmt):
        self.M, self.D, self.P, self.channels, self.fmt = M, D, P, channels, fmt
        self.planes = len(channels) if channels is not None else M
        self.name = "channelizer_%d_%d_%d_%s" % (M, D, P, fmt)
        self.at = (M * P - 1, 1000)

    def new(self):
        from gnss_sdr_rs_amd import channelizer
        return channelizer.Channelizer(self.M, self.D, channels=self.channels, taps_per_branch=self.P, blank_threshold=90.0 if self.fmt == "i8" else 4.0)

    def x(self, n, seed):
        return _channelizer_stream(self.fmt, n, seed, self.M)

    def cap(self, n):
        return n // self.D + 2

    def layout(self, S, x):
        b = Bufs(S)
        b.x = S.stage(self.raw(x))
        b.d_x = S.device(b.x.size)
        b.cap = self.cap(len(x))
        b.stride = b.cap + GAP                                               # out_stride > count: the gap is checked
        b.add("y", self.planes * b.stride * 8)
        return b

    def call(self, h, b, lo, hi, stream):
        got = h.process_dev(b.d_x + lo * self.bps(), _fmt(self.fmt), hi - lo, b.ptr("y") + b.got * 8, b.stride, b.cap - b.got, stream)
        b.got += got
        b.used["y"] = [(i * b.stride * 8, (i * b.stride + b.got) * 8) for i in range(self.planes)]


class NullerKind(Kind):
    def __init__(self, A, B, fmt):
        self.A, self.B, self.fmt = A, B, fmt
        self.name = "nuller_%d_%d_%s" % (A, B, fmt)
        self.n = (B - 1) + (B + 1) + (3 * B + 7)
        self.at = (B - 1, 2 * B)         # the first call finishes no block: the state kernel alone carries the history forward

    def bps(self):
        return self.A * (2 if self.fmt == "i8" else 8)

    def new(self):
        from gnss_sdr_rs_amd import nuller
        return nuller.Nuller(self.A, self.B)

    def x(self, n, seed):
        return _nuller_stream(self.fmt, n, self.A, seed)

    def cap(self, n):
        return n + self.B

    def layout(self, S, x):
        b = Kind.layout(self, S, x)
        b.cap_blocks = b.cap // self.B + 1
        b.add("R", b.cap_blocks * self.A * self.A * 8)
        b.add("w", b.cap_blocks * self.A * 8)
        b.static_from = None
        return b

    def call(self, h, b, lo, hi, stream, static=False):
        A, nb = self.A, b.got // self.B
        h.capture(b.ptr("R") + nb * A * A * 8, b.ptr("w") + nb * A * 8, b.cap_blocks - nb)
        got = h.process_dev(b.d_x + lo * self.bps(), _fmt(self.fmt), hi - lo, b.ptr("y") + b.got * 8, b.cap - b.got, stream)
        b.got += got
        b.used["y"] = [(0, b.got * 8)]
        b.used["w"] = [(0, b.got // self.B * A * 8)]
        if not static:
            b.used["R"] = [(0, b.got // self.B * A * A * 8)]


def _kinds():
    return [ResamplerKind(2, 3, "i8"), ResamplerKind(5120, 5119, "c32"),
            ExcisorKind(256, "i8", True), ExcisorKind(1024, "c32", False),
            DdcKind(1, 2), DdcKind(20460, 40919),
            ChannelizerKind(8, 4, 16, None, "i8"), ChannelizerKind(32, 9, 16, list(range(31, -1, -1)), "c32"),
            NullerKind(4, 256, "c32"), NullerKind(3, 256, "i8")]


KIND_IDS = ["resampler_2_3_i8", "resampler_5120_5119_c32", "excisor_256_i8_block", "excisor_1024_c32", "ddc_1_2", "ddc_20460_40919",
            "channelizer_8_4_16_i8", "channelizer_32_9_16_c32", "nuller_4_256_c32", "nuller_3_256_i8"]
KINDS = pytest.mark.parametrize("kind_index", range(len(KIND_IDS)), ids=KIND_IDS)
RING_KINDS = pytest.mark.parametrize("kind_index", range(6), ids=KIND_IDS[:6])


def _kind(gpu, index):
    k = _kinds()[index]
    assert k.name == KIND_IDS[index]
    return k


def _feed(kind, mode, S, x, cuts, h=None):
    """the calls `cuts` of the stream x through process_dev behind one producer, nothing waited for in held mode -> (handle, buffers)"""
    h = h if h is not None else S.own(kind.new())
    b = kind.layout(S, x)
    mode.begin()
    mode.load(b.d_x, b.x)
    for lo, hi in cuts:
        kind.call(h, b, lo, hi, mode.stream)
        mode.called(h)
    return h, b


# ------------------------------------------------------------------------------------------------ A, B
@KINDS
def test_a_producer_stage_consumer_on_one_held_stream(gpu, kind_index):
    """A: the delay, the input H2D, ONE process_dev of the whole stream with stream= the caller's, the D2H of outputs and captures;
    assert_held(), then a wait for that stream only.  Until the H2D runs the input buffer holds 0x5A."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 100 + kind_index)

    def scenario(S, mode):
        h, b = _feed(kind, mode, S, x, [(0, kind.n)])
        mode.finish(b)
        b.check_filler(kind.name)
        out = dict(b.words(), got=b.got, **kind.extra(h))
        h.close()
        return out
    got = _both("A " + kind.name, scenario)
    assert got["got"] > 0


@KINDS
def test_b_consecutive_calls_on_the_held_stream(gpu, kind_index):
    """B: the same stream in three calls cut inside the history (T - 1, H - 1, L - 1, B - 1) and at 1000, all three on the held stream
    with no host wait between them: the second call reads the history the first one writes, from the buffer that changed roles when
    the first was enqueued."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 200 + kind_index)
    cuts = kind.cuts(kind.n)
    assert len(cuts) == 3

    def scenario(S, mode):
        h, b = _feed(kind, mode, S, x, cuts)
        mode.finish(b)
        b.check_filler(kind.name)
        out = dict(b.words(), got=b.got, **kind.extra(h))
        h.close()
        return out
    _both("B " + kind.name, scenario)


# ------------------------------------------------------------------------------------------------ C: the joins
def _held_then(kind, tag, x, cuts, then, prepare=None):
    """every call of `cuts` but the last on the held stream; assert_held(); then(h, b, mode, S, rest) is the join under test and what
    follows it; rest = prepare(S): whatever that needs allocated, made BEFORE the hold (an allocation's fill waits for the device and
    would do the join's work for it).  The held calls' own outputs are part of the result."""
    def scenario(S, mode):
        h = S.own(kind.new())
        rest = prepare(S) if prepare else None
        h, b = _feed(kind, mode, S, x, cuts[:-1], h)
        if mode.held:
            S.assert_held()
        out = then(h, b, mode, S, rest)
        if mode.held:
            S.sync()                 # (the join has waited for it already: this returns at once, and a D2H behind it is safe)
        b.fetch_now()
        out.update(b.words())
        out.update(kind.extra(h))
        h.close()
        return out
    return _both(tag, scenario)


@KINDS
def test_c_synchronize_then_the_handles_own_stream(gpu, kind_index):
    """C: synchronize() with a call held on the caller's stream waits for THAT call too; the next call, on the handle's own stream, then
    continues the stream from the history the held call wrote."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 300 + kind_index)
    cuts = kind.cuts(kind.n)

    def then(h, b, mode, S, rest):
        h.synchronize()
        kind.call(h, b, cuts[-1][0], cuts[-1][1], None)
        h.synchronize()
        return {"got": b.got}
    _held_then(kind, "C synchronize " + kind.name, x, cuts, then)


@KINDS
def test_c_stats_with_a_call_held(gpu, kind_index):
    """C: stats() joins the held call: the blanked counter it reads is the one that call's kernel has added to."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 400 + kind_index)
    cuts = kind.cuts(kind.n)

    def then(h, b, mode, S, rest):
        return {"stats_at_join": h.stats()}
    got = _held_then(kind, "C stats " + kind.name, x, cuts, then)
    assert got["stats_at_join"]["inputs"] == cuts[-1][0]
    if "blanked" in got["stats_at_join"] and not isinstance(kind, ResamplerKind):
        assert got["stats_at_join"]["blanked"] > 0, "the stream blanks nothing: the check is blind"


@KINDS
def test_c_reset_with_a_call_held(gpu, kind_index):
    """C: reset(index) joins the held call before it zeroes the history (a held call that ran later would write its own over the
    zeros); the stream that follows, on the handle's own stream, is a new handle's at that index."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 500 + kind_index)
    cuts = kind.cuts(kind.n)
    x2 = kind.x(kind.n, 550 + kind_index)

    def prepare(S):
        b2 = kind.layout(S, x2)
        S.put(b2.d_x, b2.x)
        return b2

    def then(h, b, mode, S, b2):
        h.reset(12345)
        kind.call(h, b2, 0, kind.n, None)
        h.synchronize()
        b2.fetch_now()
        return dict(b2.words("after_reset_"), stats_after_reset=h.stats())

    got = _held_then(kind, "C reset " + kind.name, x, cuts, then, prepare)
    # ... and a handle that never saw the first stream gives the same words
    with SS.HeldStream() as S:
        h = S.own(kind.new())
        h.reset(12345)
        b2 = kind.layout(S, x2)
        S.put(b2.d_x, b2.x)
        kind.call(h, b2, 0, kind.n, None)
        h.synchronize()
        b2.fetch_now()
        _same("C reset, new handle " + kind.name, {k: v for k, v in got.items() if k.startswith("after_reset_")}, b2.words("after_reset_"))
        assert got["stats_after_reset"] == h.stats()
        h.close()


@KINDS
def test_c_host_buffer_process_with_a_call_held(gpu, kind_index):
    """C: the host-buffer process() continues the stream behind a held call: it joins before its own H2D and kernel go out on the
    handle's stream."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 600 + kind_index)
    cuts = kind.cuts(kind.n)

    def then(h, b, mode, S, rest):
        y = h.process(x[cuts[-1][0]:])
        assert y.size
        return {"host_y": np.ascontiguousarray(y)}
    _held_then(kind, "C process " + kind.name, x, cuts, then)


@RING_KINDS
def test_c_write_ring_with_a_call_held(gpu, kind_index):
    """C: a write_ring chain continues the stream into a 2^12 ring behind a held call: write_ring(..., resampler=) and
    write_ring(..., excisor=) of a front-end, and Ddc.write_ring; the chain joins every stage's last call before its first block."""
    from gnss_sdr_rs_amd import frontend, tracking
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 700 + kind_index)
    cuts = kind.cuts(kind.n)
    tail = x[cuts[-1][0]:cuts[-1][0] + 4000]

    def prepare(S):
        kind.fe = S.own(frontend.DigitalFrontend(1.25e6, 8.0e6, 8.0e6))
        return S.own(tracking.MulticastRingBuffer(1 << 12))

    def then(h, b, mode, S, ring):
        total = kind.write_ring(h, ring, tail)
        ring.flush()
        assert total > 0 and ring.get_head() == total
        words = np.ascontiguousarray(ring.copy_to_slice(0, total)).view(np.uint8).copy()
        kind.fe.close()
        ring.close()
        return {"ring": words, "total": total}
    _held_then(kind, "C write_ring " + kind.name, x, cuts, then, prepare)


EXCISOR_IDS = [2, 3]
EXCISORS = pytest.mark.parametrize("kind_index", EXCISOR_IDS, ids=[KIND_IDS[i] for i in EXCISOR_IDS])


def _new_gains(B):
    g = np.random.default_rng(B).random(B).astype(np.float32)
    g[::17] = 0.0
    return g


@EXCISORS
def test_c_excisor_set_gains_with_a_call_held(gpu, kind_index):
    """C: set_gains(new) while a process_dev is held: the held call used the OLD gains (set_gains joins before its copy goes out on the
    handle's stream), the next call the new ones."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 800 + kind_index)
    cuts = kind.cuts(kind.n)
    new = _new_gains(kind.B)

    def then(h, b, mode, S, rest):
        h.set_gains(new)
        kind.call(h, b, cuts[-1][0], cuts[-1][1], None)
        h.synchronize()
        return {"got": b.got}
    got = _held_then(kind, "C set_gains " + kind.name, x, cuts, then)
    assert (got["gains"] == new).all()


@EXCISORS
def test_c_excisor_queries_after_a_held_adapt(gpu, kind_index):
    """C: gains(), psd() and block_stats() each join a held adapt_dev (and a held process_dev in front of it): the words they return are
    the ones that adapt wrote."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 900 + kind_index)
    for query in ("gains", "psd", "block_stats"):
        def scenario(S, mode):
            h = S.own(kind.new())
            b = kind.layout(S, x)
            mode.begin()
            mode.load(b.d_x, b.x)
            kind.call(h, b, 0, 1000, mode.stream)
            mode.called(h)
            h.adapt_dev(b.d_x, _fmt(kind.fmt), kind.n, mode.stream)
            mode.called(h)
            if mode.held:
                S.assert_held()
            r = getattr(h, query)()
            out = {"psd_" + k: v for k, v in r.items()} if query == "psd" else {query: r}
            out.update(kind.extra(h))
            out["psd_all"] = h.psd()["P"]
            h.close()
            return out
        got = _both("C %s %s" % (query, kind.name), scenario)
        assert (got["gains"] == 0.0).any() and (got["gains"] == 1.0).any(), "the adapt flagged nothing: the check is blind"


# ------------------------------------------------------------------------------------------------ D: two streams, the caller's event
@KINDS
def test_d_two_caller_streams_ordered_by_the_callers_event(gpu, kind_index):
    """D: call 1 on the held stream s1, hipEventRecord(s1), hipStreamWaitEvent(s2), call 2 on s2.  The caller has ordered the two; the
    library needs no host wait for it: s1 is still held when both calls have returned."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 1000 + kind_index)
    cuts = kind.cuts(kind.n)
    cuts = [cuts[0], (cuts[1][0], kind.n)]

    def scenario(S, mode):
        S2 = S.own(SS.HeldStream())          # (owned first, so closed last: behind the handle whose last call ran on it)
        h, b = _feed(kind, mode, S, x, cuts[:1])
        if mode.held:
            S2.wait_for(S)
            kind.call(h, b, cuts[1][0], cuts[1][1], S2.stream)
            for name, (p, nbytes) in b.dev.items():
                S2.d2h(p, nbytes, b.host[name])
            S.assert_held()
            S2.sync()
            S.sync()
        else:
            kind.call(h, b, cuts[1][0], cuts[1][1], None)
            h.synchronize()
            b.fetch_now()
        b.check_filler(kind.name)
        out = dict(b.words(), got=b.got, **kind.extra(h))
        h.close()
        return out
    _both("D " + kind.name, scenario)


# ------------------------------------------------------------------------------------------------ E: the excisor's adapt chain
@EXCISORS
def test_e_excisor_adapt_then_process_on_the_held_stream(gpu, kind_index):
    """E: adapt_dev on the held stream, process_dev behind it on the same stream: the outputs are filtered with the ADAPTED gains (the
    reference ran adapt, synchronised, then process)."""
    kind = _kind(gpu, kind_index)
    x = kind.x(kind.n, 1100 + kind_index)

    def scenario(S, mode):
        h = S.own(kind.new())
        b = kind.layout(S, x)
        mode.begin()
        mode.load(b.d_x, b.x)
        h.adapt_dev(b.d_x, _fmt(kind.fmt), kind.n, mode.stream)
        mode.called(h)
        kind.call(h, b, 0, kind.n, mode.stream)
        mode.called(h)
        mode.finish(b)
        b.check_filler(kind.name)
        out = dict(b.words(), got=b.got, psd=h.psd()["P"], **kind.extra(h))
        h.close()
        return out
    got = _both("E " + kind.name, scenario)
    assert (got["gains"] == 0.0).any(), "the adapt flagged nothing: the check is blind"
    # ... and they are not the words of the unit gains (in block-adapt mode they are: each block's own mask has zeroed the tone already)
    with SS.HeldStream() as S:
        h, b = _feed(kind, Mode(S, False, ""), S, x, [(0, kind.n)])
        b.fetch_now()
        assert (b.host["y"] != got["y"]).any() or kind.block_adapt
        h.close()


# ------------------------------------------------------------------------------------------------ F: the nuller's mode switch
@pytest.mark.parametrize("kind_index", [8, 9], ids=KIND_IDS[8:])
def test_f_nuller_mode_switch_between_two_held_calls(gpu, kind_index):
    """F: an adaptive call held, set_weights(w), a second call on the same stream: the first call's blocks are adaptive (the capture
    holds R and w), the second's static (w only: their R words keep the filler)."""
    kind = _kind(gpu, kind_index)
    A, B = kind.A, kind.B
    x = kind.x(kind.n, 1200 + kind_index)
    cut = 2 * B + 5
    w = (np.arange(1, A + 1) * (0.25 - 0.5j)).astype(np.complex64)

    def scenario(S, mode):
        h = S.own(kind.new())
        b = kind.layout(S, x)
        mode.begin()
        mode.load(b.d_x, b.x)
        kind.call(h, b, 0, cut, mode.stream)
        mode.called(h)
        h.set_weights(w)
        kind.call(h, b, cut, kind.n, mode.stream, static=True)
        mode.called(h)
        mode.finish(b)
        b.check_filler(kind.name)
        out = dict(b.words(), got=b.got, **kind.extra(h))
        h.close()
        return out
    got = _both("F " + kind.name, scenario)
    nb = got["got"] // B
    wq = got["w"].view(np.complex64).reshape(-1, A)
    assert nb == 5 and not (wq[:2] == w).all(axis=1).any() and (wq[2:nb] == w).all()
    assert (got["R"][2 * A * A * 8:] == SS.FILL).all() and (got["R"][:2 * A * A * 8] != SS.FILL).any()


# ------------------------------------------------------------------------------------------------ the front-end
FE_FORMS = [("sequential", FM.NO_TABLE, FM.SEQ, False, (2 * 2048 + 8 * 3 + 5, 2048 + 8)),
            ("fast", FM.A_SETTINGS[0], FM.TAB, True, (2 * 2048 + 8 * 3 + 5, 2048 + 8)),
            ("speculative", FM.A_SETTINGS[1], FM.SPEC, True, (FM.SPEC_MIN + 8 * 37 + 5, FM.SPEC_MIN))]


def _fe_state(fe):
    ph, br, bi = fe.state()
    return {"phase": np.array([ph], np.float32), "bias_re": br, "bias_im": bi}


@pytest.mark.parametrize("name,key,form,i8,sizes", FE_FORMS, ids=[f[0] for f in FE_FORMS])
def test_frontend_forms_on_the_held_stream(gpu, name, key, form, i8, sizes):
    """The front-end's sequential, fast (table) and speculative kernels, selected by settings and length and confirmed with
    gm_frontend_debug_forms as test_gpu_frontend_forms.py does: two consecutive out-of-place process_dev calls on the held stream, the
    second starting from the state the first leaves.  The speculative form's FIRST use on the handle is the held call: that is where its
    scratch is allocated and zeroed, by a fill that has to go out on the caller's stream too (a 1000-sample call in front, waited for,
    has put the handle on its table)."""
    from gnss_sdr_rs_amd import frontend as F
    ins = [FM.noise_dc(31 + k, n, i8)[0] for k, n in enumerate(sizes)]
    warm = FM.noise_dc(30, 1000, i8)[0]
    fmt = _fmt("i8" if i8 else "c32")

    def scenario(S, mode):
        fe = S.own(F.DigitalFrontend(key[0], key[1], key[1]))
        b = Bufs(S)
        staged = [S.stage(np.ascontiguousarray(r)) for r in ins]
        d_in = [S.device(s.size) for s in staged]
        for k, n in enumerate(sizes):
            b.add("y%d" % k, (n + GAP) * 8)
            b.used["y%d" % k] = [(0, n * 8)]
        if form == FM.SPEC:
            d_w, d_wo = S.device(warm.nbytes), S.device(1000 * 8)
            S.put(d_w, warm)
            fe.process_dev(d_w, fmt, d_wo, 1000)
            fe.synchronize()
        before = fe.debug_forms()
        mode.begin()
        for k, n in enumerate(sizes):
            mode.load(d_in[k], staged[k])
            fe.process_dev(d_in[k], fmt, b.ptr("y%d" % k), n, mode.stream)
            mode.called(fe)
        mode.finish(b)
        b.check_filler(name)
        delta = tuple(int(a) - int(c) for a, c in zip(fe.debug_forms(), before))
        assert delta == tuple(2 if i == form else 0 for i in range(3)), (name, delta)
        out = dict(b.words(), **_fe_state(fe))
        if form == FM.SPEC:
            out["repairs"] = fe.debug_repairs()
        fe.close()
        return out
    _both("front-end " + name, scenario)


def test_frontend_batch_of_three_behind_a_held_producer(gpu):
    """gm_frontend_process_dev_batch with three front-ends whose inputs arrive by an H2D behind the hold.  The entry waits on the host for
    `stream` while its descriptors travel (documented), so the hold is asserted directly BEFORE the call: the inputs were not there yet
    when it was made, the kernel ran behind them on the caller's stream, and two batches follow each other on that stream."""
    from gnss_sdr_rs_amd import frontend as F
    n = 2048 + 8 * 3 + 5
    keys = [FM.A_SETTINGS[0], FM.A_SETTINGS[1], FM.NO_TABLE]
    ins = [[FM.noise_dc(60 + 3 * r + k, n, True)[0] for k in range(3)] for r in range(2)]

    def scenario(S, mode):
        fes = [S.own(F.DigitalFrontend(k[0], k[1], k[1])) for k in keys]
        b = Bufs(S)
        staged = [[S.stage(np.ascontiguousarray(a)) for a in row] for row in ins]
        d_in = [[S.device(s.size) for s in row] for row in staged]
        for r in range(2):
            for k in range(3):
                b.add("y%d%d" % (r, k), (n + GAP) * 8)
                b.used["y%d%d" % (r, k)] = [(0, n * 8)]
        mode.begin()
        for r in range(2):
            for k in range(3):
                mode.load(d_in[r][k], staged[r][k])
        if mode.held:
            S.assert_held()
        for r in range(2):
            F.process_dev_batch(fes, d_in[r], _fmt("i8"), [b.ptr("y%d%d" % (r, k)) for k in range(3)], n, mode.stream)
            mode.called(fes[0])
        if mode.held:
            b.fetch_async()
            S.sync()
        else:
            b.fetch_now()
        b.check_filler("batch")
        out = b.words()
        for k, fe in enumerate(fes):
            out.update({"fe%d_%s" % (k, name): v for name, v in _fe_state(fe).items()})
            fe.close()
        return out
    _both("front-end batch", scenario)


# ------------------------------------------------------------------------------------------------ device-resident chains
def _engine(fft_size, prns):
    from gnss_sdr_rs_amd import acquisition as A
    dop = np.arange(-1000.0, 1001.0, 500.0, dtype=np.float32)
    return A.AcquisitionEngine(fft_size * 1000.0, 0.0, fft_size, doppler_hz=dop, prn_ids=prns, n_integrations=2,
                               decision_mode=A.DECIDE_BEST_BIN), 3 * len(prns) * dop.size


def _key(r):
    return r and (r["prn"], r["code_phase_samples"], r["doppler_bin"], r["mag_relative"])


def test_chain_nuller_excisor_resampler_search(gpu):
    """int8 4-antenna stream -> Nuller(4, 1024) -> Excisor(1024) -> Resampler(2, 3) -> search_dev + decide_dev at fft_size 2048, two
    integrations, on ONE held stream: each stage's output buffer is the next one's input pointer, the engine has been given the stream
    (set_stream), and nothing is waited for between the first H2D and the last D2H.  7168 time samples: 7 nuller blocks, 6656 excisor
    outputs, 4416 resampler outputs, of which the dwell takes 4096."""
    from gnss_sdr_rs_amd import _lib, excise, nuller, resample
    n, prns = 7 * 1024, [3, 7, 12, 25]
    x = _nuller_stream("i8", n, 4, 77)
    assert (x == -128).any()

    def scenario(S, mode):
        nl, ex, rs = S.own(nuller.Nuller(4, 1024)), S.own(excise.Excisor(1024, blank_threshold=150.0)), S.own(resample.Resampler(2, 3))
        eng, words = _engine(2048, prns)
        S.own(eng)
        b = Bufs(S)
        xs = S.stage(x)
        d_x = S.device(xs.size)
        d1, d2, d3, d_met = b.add("nulled", (n + GAP) * 8), b.add("excised", (n + GAP) * 8), b.add("resampled", (n + GAP) * 8), b.add("metrics", words * 4)
        b.used["metrics"] = [(0, words * 4)]
        if mode.held:
            eng.set_stream(S.stream)
        mode.begin()
        mode.load(d_x, xs)
        g1 = nl.process_dev(d_x, _lib.FMT_I8_IQ, n, d1, n, mode.stream)
        mode.called(nl)
        g2 = ex.process_dev(d1, _lib.FMT_C32, g1, d2, n, mode.stream)
        mode.called(ex)
        g3 = rs.process_dev(d2, _lib.FMT_C32, g2, d3, n, mode.stream)
        mode.called(rs)
        assert (g1, g2, g3) == (7168, 6656, 4416)
        b.used["nulled"], b.used["excised"], b.used["resampled"] = [(0, g1 * 8)], [(0, g2 * 8)], [(0, g3 * 8)]
        eng.search_dev(d3, _lib.FMT_C32, d_met)
        eng.decide_dev(d_met)
        mode.called(eng)
        mode.finish(b)
        b.check_filler("chain 1")
        out = dict(b.words(), decisions=[_key(r) for r in eng.fetch_results(len(prns))],
                   nuller=nl.stats(), excisor=ex.stats(), resampler=rs.stats())
        for h in (eng, nl, ex, rs):
            h.close()
        return out
    got = _both("chain nuller-excisor-resampler-search", scenario)
    assert got["resampler"]["outputs"] == 4416


def test_chain_ddc_channelizer_search_per_plane(gpu):
    """real int8 -> Ddc(1, 2) -> Channelizer(8, 4, 16) -> search_dev on two plane pointers (d_out + i * out_stride * 8) at fft_size
    256, two integrations, on ONE held stream; no host wait between the first H2D and the last D2H.  4256 input
    bytes: 2112 down-converted samples, 512 outputs per plane: one dwell."""
    from gnss_sdr_rs_amd import _lib, channelizer, ddc
    n, stride = 4256, 512 + GAP
    x = _ddc_stream(n, 78)
    assert (x == -128).any()

    def scenario(S, mode):
        dd, ch = S.own(ddc.Ddc(0.2501, 1, 2, blank_threshold=100.0)), S.own(channelizer.Channelizer(8, 4, taps_per_branch=16))
        engs = [_engine(256, [1]) for _ in range(2)]
        for e in engs:
            S.own(e[0])
        words = engs[0][1]
        b = Bufs(S)
        xs = S.stage(x)
        d_x = S.device(xs.size)
        d1, d2 = b.add("baseband", (2112 + GAP) * 8), b.add("planes", 8 * stride * 8)
        d_met = [b.add("metrics%d" % i, words * 4) for i in range(2)]
        for i in range(2):
            b.used["metrics%d" % i] = [(0, words * 4)]
            if mode.held:
                engs[i][0].set_stream(S.stream)
        mode.begin()
        mode.load(d_x, xs)
        g1 = dd.process_dev(d_x, n, d1, 2112, mode.stream)
        mode.called(dd)
        g2 = ch.process_dev(d1, _lib.FMT_C32, g1, d2, stride, 512, mode.stream)
        mode.called(ch)
        assert (g1, g2) == (2112, 512)
        b.used["baseband"] = [(0, g1 * 8)]
        b.used["planes"] = [(i * stride * 8, (i * stride + g2) * 8) for i in range(8)]
        for i, plane in enumerate((1, 6)):
            engs[i][0].search_dev(d2 + plane * stride * 8, _lib.FMT_C32, d_met[i])      # a plane pointer goes straight into the search
            engs[i][0].decide_dev(d_met[i])
            mode.called(engs[i][0])
        mode.finish(b)
        b.check_filler("chain 2")
        out = dict(b.words(), ddc=dd.stats(), channelizer=ch.stats())
        for i in range(2):
            out["decisions%d" % i] = [_key(r) for r in engs[i][0].fetch_results(1)]
            engs[i][0].close()
        dd.close(); ch.close()
        return out
    got = _both("chain ddc-channelizer-search", scenario)
    assert got["ddc"]["blanked"] > 0


def test_chain_frontend_excisor_resampler_twice(gpu):
    """DigitalFrontend.process_dev -> Excisor(256) -> Resampler(5120, 5119), two passes in a row on ONE held stream: the second pass
    starts from the front-end state and from both histories that the first leaves, none of which has been written yet when it is
    enqueued."""
    from gnss_sdr_rs_amd import _lib, excise, frontend, resample
    n = 4096
    xs_np = [_resample_stream("i8", n, 79 + k) for k in range(2)]

    def scenario(S, mode):
        fe = S.own(frontend.DigitalFrontend(1.25e6, 8.0e6, 8.0e6))
        ex, rs = S.own(excise.Excisor(256, blank_threshold=150.0)), S.own(resample.Resampler(5120, 5119))
        b = Bufs(S)
        staged = [S.stage(a) for a in xs_np]
        d_x = [S.device(s.size) for s in staged]
        names = [("fe%d" % k, "ex%d" % k, "rs%d" % k) for k in range(2)]
        for trio in names:
            for name in trio:
                b.add(name, (n + 256 + GAP) * 8)
        mode.begin()
        counts = []
        for k in range(2):
            mode.load(d_x[k], staged[k])
            fe.process_dev(d_x[k], _lib.FMT_I8_IQ, b.ptr(names[k][0]), n, mode.stream)
            mode.called(fe)
            g2 = ex.process_dev(b.ptr(names[k][0]), _lib.FMT_C32, n, b.ptr(names[k][1]), n + 256, mode.stream)
            mode.called(ex)
            g3 = rs.process_dev(b.ptr(names[k][1]), _lib.FMT_C32, g2, b.ptr(names[k][2]), n + 256, mode.stream)
            mode.called(rs)
            counts.append((g2, g3))
            b.used[names[k][0]], b.used[names[k][1]], b.used[names[k][2]] = [(0, n * 8)], [(0, g2 * 8)], [(0, g3 * 8)]
        assert [c[0] for c in counts] == [3968, 4096] and counts[1][1] > 0
        mode.finish(b)
        b.check_filler("chain 3")
        out = dict(b.words(), counts=counts, excisor=ex.stats(), resampler=rs.stats(), **_fe_state(fe))
        for h in (fe, ex, rs):
            h.close()
        return out
    got = _both("chain frontend-excisor-resampler x2", scenario)
    assert got["excisor"]["blanked"] > 0
