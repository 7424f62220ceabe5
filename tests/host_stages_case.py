"""What the two tests of tests/cpp/host_stages.cpp share (test_cpp_host_stages_host.py, test_gpu_cpp_host_stages.py): the one build of
the driver, the case file's writer, the result file's reader, the child process, and the steps.  A step is a pair (the bytes the driver
reads, a function that runs the same call through the Python layer and returns the records the driver must write): one definition
serves both sides, so that the two cannot drift apart."""
import os
import struct
import subprocess
import time

import numpy as np

from conftest import ROOT

PROCESS, PROCESS_DEV, RESET, STATS, TAPS, SYNC, WRITE_RING, RING_READ = 1, 2, 3, 4, 5, 6, 7, 8
SET_GAINS, GAINS, ADAPT_DEV, PSD, SET_BLOCK_ADAPT, CLEAR_BLOCK_ADAPT, BLOCK_STATS, BLOCK_CAPTURE = 10, 11, 12, 13, 14, 15, 16, 17
SET_WEIGHTS, SET_STEERING, SET_CONSTRAINTS, CAPTURE, STATS_PLAIN = 20, 21, 22, 23, 24
REFUSE = 0x8000
C32, I8_IQ, I8_REAL = 0, 1, 2
INVALID = -1
FATAL = (134, 139, 124, 137, -6, -11, -9)       # abort, segmentation fault, time limits: nothing more runs on the GPU in that test
GUARD_FILL = 0x5A
_BUILT = {}


def build(gm):
    """the one g++ compile of the driver, the way tests/test_cpp_host_api.py builds its program -> (path, seconds)"""
    if "exe" not in _BUILT:
        exe = os.path.join(ROOT, "gnss-sdr-rs_amd", "build", "host_stages")
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        libdir = os.path.dirname(gm.library_path())
        cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "gnss-sdr-rs_amd", "host"),
               "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "cpp", "host_stages.cpp"), "-o", exe,
               "-L", libdir, "-lgnss_mi355x", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        _BUILT["exe"], _BUILT["seconds"] = exe, time.perf_counter() - t0
        print("host_stages: the one g++ compile took %.2f s" % _BUILT["seconds"])
    return _BUILT["exe"], _BUILT["seconds"]


def pk(fmt, *v):
    return struct.pack("<" + fmt, *v)


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def words(kind, a):
    """uint32 count + the array's bytes: a vector argument"""
    a = np.ascontiguousarray(a, kind).reshape(-1)
    return pk("I", a.size) + a.tobytes()


def case(head, steps):
    """the case file's bytes and the function that gives the Python layer's records for an object made by the caller"""
    body = head + pk("I", len(steps)) + b"".join(s[0] for s in steps)

    def run(obj, hb=None):
        out = []
        for _, f in steps:
            out += f(obj, hb)
        return out
    return body, run


def rec(tag, a, kind=None):
    return tag, (np.ascontiguousarray(a, kind) if kind is not None else np.ascontiguousarray(a)).tobytes()


def u64(tag, *v):
    return tag, np.array(v, np.uint64).tobytes()


def u32(tag, v):
    return tag, np.array([v], np.uint32).tobytes()


def run_driver(exe, op, body, tmp_path, cpu_only=False, want=0):
    """one fresh child, at most 60 s -> the records [(tag, bytes)]; a fatal status or the time limit fails the test here"""
    tmp_path = str(tmp_path)
    n = len(os.listdir(tmp_path))
    cf, rf = os.path.join(tmp_path, "%s_%d.case" % (op, n)), os.path.join(tmp_path, "%s_%d.result" % (op, n))
    with open(cf, "wb") as f:
        f.write(body)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([exe] + (["--cpu-only"] if cpu_only else []) + [op, cf, rf], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
    except subprocess.TimeoutExpired:
        raise AssertionError("host_stages fatal: %s ran into the 60 s limit" % op)
    print("host_stages %s: %.2f s, status %d" % (op, time.perf_counter() - t0, r.returncode))
    assert r.returncode not in FATAL, "host_stages fatal: %s ended with status %d\n%s" % (op, r.returncode, r.stdout)
    with open(rf, "rb") as f:
        b = f.read()
    assert r.returncode == want, (op, r.returncode, r.stdout, b[-300:])         # (an unexpected Panic's text ends the result file)
    out, at = [], 0
    while at < len(b):
        tl, = struct.unpack_from("<I", b, at)
        tag = b[at + 4:at + 4 + tl].decode()
        nb, = struct.unpack_from("<Q", b, at + 4 + tl)
        at += 12 + tl
        out.append((tag, b[at:at + nb]))
        at += nb
    assert at == len(b)
    return out


def same(cpp, py, what=""):
    """every record of the C++ run against the Python run's: the same tags in the same order, the same bytes"""
    assert cpp and cpp[-1][0] == "end", (what, [t for t, _ in cpp][-3:])
    cpp = cpp[:-1]
    assert [t for t, _ in cpp] == [t for t, _ in py], (what, [t for t, _ in cpp], [t for t, _ in py])
    for i, ((tag, a), (_, b)) in enumerate(zip(cpp, py)):
        if a != b:
            n = min(len(a), len(b))
            first = next((k for k in range(n) if a[k] != b[k]), n)
            raise AssertionError("%s: record %d (%s): C++ %d bytes, Python %d bytes, first difference at byte %d"
                                 % (what, i, tag, len(a), len(b), first))


def get(records, tag, kind, nth=None):
    """the records of a tag as arrays (nth None: all of them)"""
    v = [np.frombuffer(b, kind) for t, b in records if t == tag]
    return v if nth is None else v[nth]


# ---------------------------------------------------------------------------------------------------------------- device buffers
def _dev_in(hb, x):
    return hb.upload(x) if x.nbytes else hb.alloc(8)


def dev_out(hb, nbytes, call):
    """what the driver's DevBuf does: nbytes of 0x5A, call(pointer) -> (the buffer's image afterwards)"""
    p = hb.alloc(max(nbytes, 8), fill=GUARD_FILL)
    v = call(p)
    return v, hb.download(p, max(nbytes, 8), np.uint8)[:nbytes]


def refused(step):
    """the step with the refusal bit: the driver records the Panic's status, the Python layer must refuse with the same one (a ValueError
    of the Python wrapper's own size check stands for the header's own GM_ERR_INVALID_ARG)"""
    from gnss_sdr_rs_amd import _lib
    body, f = step
    code, = struct.unpack_from("<I", body, 0)

    def g(o, hb):
        try:
            f(o, hb)
        except _lib.GmError as e:
            st = e.status
        except ValueError:
            st = INVALID
        else:
            raise AssertionError("the Python layer took what it was to refuse")
        return [("refused", np.array([st], np.int32).tobytes())]
    return pk("I", code | REFUSE) + body[4:], g


# ---------------------------------------------------------------------------------------------------------------- steps
def _n(fmt, x, A=1):
    return x.size // (2 * A) if fmt == I8_IQ else x.size // A


def s_reset(at):
    return pk("IQ", RESET, at), lambda o, hb: (o.reset(at), [])[1]


def s_stats(keys=("inputs", "outputs", "blanked")):
    return pk("I", STATS), lambda o, hb: [u64("stats", *[o.stats()[k] for k in keys])]


def s_process(fmt, x):
    """Resampler, Excisor: process / process_i8"""
    return pk("IIQ", PROCESS, fmt, _n(fmt, x)) + raw(x), lambda o, hb: [rec("y", o.process(x))]


def s_process_dev(fmt, x, cap):
    n = _n(fmt, x)

    def f(o, hb):
        d_in = _dev_in(hb, x)
        got, img = dev_out(hb, cap * 8, lambda p: o.process_dev(d_in, fmt, n, p, cap))
        return [u64("got", got), rec("dev", img), u32("dev.guards", 1), u32("in.guards", 1)]
    return pk("IIQQ", PROCESS_DEV, fmt, n, cap) + raw(x), f


def s_taps(n_words=None):
    """n_words: what the caller of Resampler::taps sizes its table with; Channelizer::taps sizes its own"""
    return pk("I", TAPS) + (pk("Q", n_words) if n_words is not None else b""), lambda o, hb: [rec("taps", o.taps())]


# ---- Excisor
def s_set_gains(g):
    return pk("I", SET_GAINS) + words(np.float32, g), lambda o, hb: (o.set_gains(g), [])[1]


def s_gains():
    return pk("I", GAINS), lambda o, hb: [rec("gains", o.gains())]


def s_adapt_dev(fmt, x):
    n = _n(fmt, x)

    def f(o, hb):
        o.adapt_dev(_dev_in(hb, x), fmt, n)
        o.synchronize()
        return [u32("in.guards", 1)]
    return pk("IIQ", ADAPT_DEV, fmt, n) + raw(x), f


def s_psd():
    def f(o, hb):
        p = o.psd()
        return [rec("psd", p["P"]), rec("median", np.float32(p["median"])), u32("n_flagged", p["n_flagged"]), u32("n_zeroed", p["n_zeroed"]),
                rec("psd.alone", p["P"])]
    return pk("I", PSD), f


def s_set_block_adapt(factor, guard):
    return pk("IfI", SET_BLOCK_ADAPT, factor, guard), lambda o, hb: (o.set_block_adapt(factor, guard), [])[1]


def s_clear_block_adapt():
    return pk("I", CLEAR_BLOCK_ADAPT), lambda o, hb: (o.set_block_adapt(None), [])[1]


def s_block_stats():
    def f(o, hb):
        s = o.block_stats()
        return [u64("block_stats", s["blocks"], s["blocks_flagged"], s["bins_flagged"], s["bins_zeroed"]), u64("bins_flagged.alone", s["bins_flagged"])]
    return pk("I", BLOCK_STATS), f


class _Held:
    """device buffers a capture step armed, until the step that disarms it"""
    bufs = None


def s_block_capture(cap_blocks, held):
    def f(o, hb):
        if cap_blocks:
            sizes = (cap_blocks * o.block * 4, cap_blocks * o.block)
            held.bufs = [(hb.alloc(n, fill=GUARD_FILL), n) for n in sizes]
            o.block_capture(held.bufs[0][0], held.bufs[1][0], cap_blocks)
            return []
        o.block_capture(None, None, 0)
        o.synchronize()
        (p, n), (m, k) = held.bufs
        return [rec("power", hb.download(p, n, np.uint8)), u32("power.guards", 1), rec("mask", hb.download(m, k, np.uint8)), u32("mask.guards", 1)]
    return pk("IQ", BLOCK_CAPTURE, cap_blocks), f


# ---- Ddc
def s_ddc_process(x):
    return pk("IQ", PROCESS, x.size) + raw(x), lambda o, hb: [rec("y", o.process(x))]


def s_ddc_process_dev(x, cap, offset):
    def f(o, hb):
        d_in = _dev_in(hb, np.concatenate([np.zeros(offset, np.int8), x]))
        got, img = dev_out(hb, cap * 8, lambda p: o.process_dev(d_in + offset, x.size, p, cap))
        return [u64("got", got), rec("dev", img), u32("dev.guards", 1), u32("in.guards", 1)]
    return pk("IQQI", PROCESS_DEV, x.size, cap, offset) + raw(x), f


def s_ddc_tables(n_words):
    def f(o, hb):
        t, whi, wlo = o.tables()
        return [rec("taps", t), rec("whi", whi), rec("wlo", wlo), rec("taps.alone", t), rec("whi.alone", whi)]
    from gnss_sdr_rs_amd import ddc
    return pk("IQQ", TAPS, n_words, ddc.TABLE_WORDS), f


# ---- Channelizer
def s_ch_process(fmt, x):
    def f(o, hb):
        y = o.process(x)
        return [rec("y", y), u64("n_out", y.shape[1])]
    return pk("IIQ", PROCESS, fmt, _n(fmt, x)) + raw(x), f


def s_ch_process_dev(fmt, x, stride, cap):
    n = _n(fmt, x)

    def f(o, hb):
        d_in = _dev_in(hb, x)
        got, img = dev_out(hb, len(o.channels) * stride * 8, lambda p: o.process_dev(d_in, fmt, n, p, stride, cap))
        return [u64("got", got), rec("dev", img), u32("dev.guards", 1), u32("in.guards", 1)]
    return pk("IIQQQ", PROCESS_DEV, fmt, n, stride, cap) + raw(x), f


# ---- the array stages: x is [n, A] complex64 or [n, A, 2] int8
def _afmt(x):
    return I8_IQ if x.dtype == np.int8 else C32


def s_array_process(x, want, planes=False):
    """want: 1 R, 2 w, 4 (Beamformer, Lcmv) n_out; the Python layer gives R and w together or not at all"""
    def f(o, hb):
        if want & 3:
            y, R, w = o.process(x, want_blocks=True)
        else:
            y = o.process(x)
        out = [rec("y", y)]
        if want & 4:
            out.append(u64("n_out", y.shape[-1]))
        return out + ([rec("R", R)] if want & 1 else []) + ([rec("w", w)] if want & 2 else [])
    return pk("IIQI", PROCESS, _afmt(x), x.shape[0], want) + raw(x), f


def s_array_process_dev(x, cap):
    def f(o, hb):
        d_in = _dev_in(hb, x)
        got, img = dev_out(hb, cap * 8, lambda p: o.process_dev(d_in, _afmt(x), x.shape[0], p, cap))
        return [u64("got", got), rec("dev", img), u32("dev.guards", 1), u32("in.guards", 1)]
    return pk("IIQQ", PROCESS_DEV, _afmt(x), x.shape[0], cap) + raw(x), f


def s_beams_process_dev(x, stride):
    def f(o, hb):
        d_in = _dev_in(hb, x)
        got, img = dev_out(hb, o.n_beams * stride * 8, lambda p: o.process_dev(d_in, _afmt(x), x.shape[0], p, stride))
        return [u64("got", got), rec("dev", img), u32("dev.guards", 1), u32("in.guards", 1)]
    return pk("IIQQ", PROCESS_DEV, _afmt(x), x.shape[0], stride) + raw(x), f


def s_set_weights(w):
    """w None: the empty vector, back to the adaptive rule"""
    return pk("I", SET_WEIGHTS) + words(np.complex64, [] if w is None else w), lambda o, hb: (o.set_weights(w), [])[1]


def s_set_steering(beam, row):
    return pk("II", SET_STEERING, beam) + words(np.complex64, row), lambda o, hb: (o.set_steering(beam, row), [])[1]


def s_set_constraints(beam, rows, f):
    return (pk("II", SET_CONSTRAINTS, beam) + words(np.complex64, rows) + words(np.complex64, f),
            lambda o, hb: (o.set_constraints(beam, rows, f), [])[1])


def s_capture(cap_blocks, held):
    """arms the capture on buffers of the step's own, or (0) disarms it and gives what they hold"""
    def f(o, hb):
        if cap_blocks:
            P = o._P or 1
            sizes = (cap_blocks * o._M * o._M * 8, cap_blocks * P * o._M * 8)
            held.bufs = [(hb.alloc(n, fill=GUARD_FILL), n) for n in sizes]
            o.capture(held.bufs[0][0], held.bufs[1][0], cap_blocks)
            return []
        o.capture(None, None, 0)
        o.synchronize()
        (p, n), (m, k) = held.bufs
        return [rec("cap.R", hb.download(p, n, np.uint8)), u32("cap.R.guards", 1), rec("cap.w", hb.download(m, k, np.uint8)), u32("cap.w.guards", 1)]
    return pk("IQ", CAPTURE, cap_blocks), f


def s_stap_stats(plain=False):
    keys = ("inputs", "outputs", "blocks") + (() if plain else ("fallback_blocks",))
    return pk("I", STATS_PLAIN if plain else STATS), lambda o, hb: [u64("stats", *[o.stats()[k] for k in keys])]


def s_beams_stats(plain=False):
    def f(o, hb):
        s = o.stats()
        out = [u64("stats", s["inputs"], s["outputs"], s["blocks"])]
        return out if plain else out + [rec("fallbacks", np.array(s["fallbacks"], np.uint64))]
    return pk("I", STATS_PLAIN if plain else STATS), f


# ---- the ring writers: obj is (ring, source, excisor, resampler)
def s_write_ring(fmt, x):
    n = x.size if fmt != I8_IQ else x.size // 2

    def f(o, hb):
        ring, src, ex, rs = o
        total = src.write_ring(ring, x, excisor=ex, resampler=rs)
        return [u64("total", total), u64("enqueued", ring.get_enqueued_head())]
    return pk("IIQ", WRITE_RING, fmt, n) + raw(x), f


def s_ring_read(start, n):
    def f(o, hb):
        ring = o[0]
        ring.flush()
        return [u64("head", ring.get_head()), rec("ring", ring.copy_to_slice(start, n))]
    return pk("IQQ", RING_READ, start, n), f


def s_ring_stats(with_ddc):
    def f(o, hb):
        ring, src, ex, rs = o
        v = []
        for h in (src if with_ddc else None, ex, rs):
            s = h.stats() if h is not None else dict(inputs=0, outputs=0, blanked=0)
            v += [s["inputs"], s["outputs"], s["blanked"]]
        return [u64("stats", *v)]
    return pk("I", STATS), f
