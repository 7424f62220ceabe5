"""Rate conversion and pulse blanking on the GPU (gm_resampler, csrc/resample_kernels.hip) against the float64 model of
resample_model.py, which is handed the library's own table words (gm_resampler_taps).

1. Words.  Per output and component |device - model| <= (T + 4) 2^-24 sum_j |c_j| |x_j|: the bound of a float32 dot product of T
   fused multiply-adds in ANY order (Higham, gamma_T), plus the two roundings inside c_j (the difference of the rows and the blend) and
   the model's own float64 blend.  Derived, not measured; the largest error over bound seen is printed.  Every ratio and tap count of
   CONFIGS, both sample formats (the int8 stream holds -128), and block lengths where the tile, halo and history logic can go wrong.
2. Splitting: one call against the same stream in blocks of 1, 7, T - 1, 1000 and 3001, bit for bit; after reset; at absolute indices
   2^32 - 3 and 2^40 + 12345.
3. Blanking: spikes inside a tile, on a tile edge, in a halo and in the history across a call boundary; exactly at the threshold.
4. The ring path against process_dev(front-end) -> process_dev(resampler), word for word, over two wraps of a 2^12 ring.
5. Every refusal, with the state untouched.
6. The chain: the host test's scene at 50 dB-Hz through Resampler, then a plain search_dev."""
import ctypes as C

import numpy as np
import pytest

import resample_model as RM
import stage_instantiations as SI

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5

# (up, down, taps, n_phases): the ratios 1/1, 3/2, 2/3, 4/25 (224 taps by default), 5120/5119, 40920/40919; taps 8, 32, 256; phases 16,
# 256; and 1/8 and 1/16 at 256 taps, whose tiles are 256 and 240 outputs (a lane owns one output; 4/25: two; the others: four); and the two
# of stage_instantiations.py that blend with a lane owning two outputs (3/16, T = 192) and one (3/40 at 256 taps): with them every
# <FMT, BLEND, OPL> runs
CONFIGS = [(1, 1, 8, 16), (1, 1, 32, 256), (3, 2, 32, 256), (3, 2, 256, 16), (2, 3, 0, 0), (2, 3, 8, 16), (4, 25, 0, 0), (4, 25, 256, 16),
           (5120, 5119, 0, 0), (5120, 5119, 8, 16), (40920, 40919, 32, 256), (40920, 40919, 256, 256), (1, 8, 256, 256), (1, 16, 256, 16)] + SI.RESAMPLE_ADDED


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stream(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "i8":
        x = rng.integers(-128, 128, (n, 2)).astype(np.int8)
        if n:
            x[n // 3] = (-128, 127)
            x[n // 2] = (-128, -128)
        return x
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _bps(fmt):
    return 2 if fmt == "i8" else 8


def _fmt(fmt):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_C32


def _feed(hipbuf, rs, d_x, fmt, n, blocks=None, cap=None):
    """the n samples at d_x through rs.process_dev in blocks (None: one call) -> complex64 outputs, all of them behind each other in
    one device buffer whose tail must stay as it was filled"""
    cap = cap if cap is not None else n * rs.up // rs.down + 2
    d_y = hipbuf.alloc(cap * 8 + 64, fill=0x5A)
    done = got = 0
    step = blocks or max(n, 1)
    while True:
        k = min(step, n - done)
        got += rs.process_dev(d_x + done * _bps(fmt), _fmt(fmt), k, d_y + got * 8, cap - got)
        done += k
        if done >= n:
            break
    rs.synchronize()
    raw = hipbuf.download(d_y, cap * 8 + 64, np.complex64)
    assert (raw[got:].view(np.uint8) == 0x5A).all()                     # nothing behind the last output
    return raw[:got].copy()


def _check(tag, got, want, weight, T):
    assert got.size == want.size, (tag, got.size, want.size)
    if not got.size:
        return 0.0
    bound = (T + 4) * 2.0 ** -24 * weight
    err = np.stack([np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag)], axis=1)
    assert np.isfinite(got.view(np.float32)).all(), tag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (tag, worst)
    return worst


def _lengths(p):
    """block lengths of a fresh stream: nothing, no output yet, the first outputs, a block shorter than the history, one tile of
    outputs give or take an input, and about 20000 with a ragged tail"""
    T, tile = p["T"], RM.tile_outputs(p)
    n_tile = next(n for n in range(T // 2, 1 << 20) if RM.total_out(p, n) >= tile)
    assert RM.total_out(p, n_tile - 1) < tile <= RM.total_out(p, n_tile)
    return [0, T // 2 - 1, T // 2 + 1, T - 1, n_tile - 1, n_tile, n_tile + 1, 20011]


@pytest.mark.parametrize("config", CONFIGS)
def test_words_against_the_model(gpu, hipbuf, config):
    from gnss_sdr_rs_amd import resample
    up, down, taps, phases = config
    rs = resample.Resampler(up, down, taps=taps, n_phases=phases)
    p = RM.resolve(up, down, taps, phases)
    assert (rs.up, rs.down, rs.n_taps, rs.n_phases) == (p["up"], p["down"], p["T"], p["PHI"])
    g = rs.taps()
    lengths = _lengths(p)
    assert RM.total_out(p, lengths[1]) == 0 and RM.total_out(p, lengths[2]) >= 1
    worst = 0.0
    for fmt in ("i8", "c32"):
        x = _stream(fmt, lengths[-1], 17 + up)
        d_x = hipbuf.upload(x)
        for n in lengths:
            rs.reset(0)
            got = _feed(hipbuf, rs, d_x, fmt, n)
            want, weight, m = RM.run(p, g, x[:n])
            worst = max(worst, _check((config, fmt, n), got, want, weight, p["T"]))
            assert rs.stats() == dict(inputs=n, outputs=RM.total_out(p, n), blanked=0)
            assert (hipbuf.download(d_x, x.nbytes, x.dtype).reshape(x.shape) == x).all()       # the input is only read
    print("%s: tile %d outputs, largest error / bound %.3f" % (config, RM.tile_outputs(p), worst))
    rs.close()


SPLITS = (1, 7, None, 1000, 3001)          # None: T - 1


@pytest.mark.parametrize("config,fmt", [((2, 3, 0, 0), "i8"), ((5120, 5119, 0, 0), "c32"), ((4, 25, 0, 0), "i8"), ((3, 2, 32, 256), "c32"),
                                        (SI.RESAMPLE_BLEND_2, "i8")])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, config, fmt):
    from gnss_sdr_rs_amd import resample
    up, down, taps, phases = config
    rs = resample.Resampler(up, down, taps=taps, n_phases=phases)
    p = RM.resolve(up, down, taps, phases)
    g = rs.taps()
    n = 6007
    x = _stream(fmt, n, 5)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, rs, d_x, fmt, n)
    want, weight, _ = RM.run(p, g, x)
    _check((config, "whole"), whole, want, weight, p["T"])
    for blocks in SPLITS:
        rs.reset(0)
        got = _feed(hipbuf, rs, d_x, fmt, n, blocks or p["T"] - 1)
        assert (_words(got) == _words(whole)).all(), (config, blocks)
    rs.reset(0)
    assert (_words(_feed(hipbuf, rs, d_x, fmt, n)) == _words(whole)).all()                      # again after reset: the same words
    # absolute indices above 2^32: the model at those indices, and the cuts still do not matter
    for index in ((1 << 40) + 12345, (1 << 32) - 3):
        rs.reset(index)
        far = _feed(hipbuf, rs, d_x, fmt, n)
        want, weight, m = RM.run(p, g, x, input_index=index)
        assert far.size == m.outputs == RM.plan(p, index, n)
        _check((config, index), far, want, weight, p["T"])
        rs.reset(index)
        assert (_words(_feed(hipbuf, rs, d_x, fmt, n, 1000)) == _words(far)).all()
        assert rs.stats() == dict(inputs=n, outputs=far.size, blanked=0)
    rs.close()


def _spiky(fmt, p, n):
    """a quiet stream (|re|, |im| <= 20) with spikes inside the first tile, around the input the second tile starts at (both tiles'
    halos), around the cuts of the 1000-sample split, and the pair that sits exactly at / just above the threshold 100"""
    rng = np.random.default_rng(9)
    x = rng.integers(-20, 21, (n, 2)).astype(np.int8)
    edge = RM.tile_outputs(p) * p["down"] // p["up"]               # i0 of the second tile's first output
    half = p["T"] // 2
    spikes = [700, edge - half, edge - 1, edge, edge + 1, edge + half, 999, 1000, 1001, 1999, 2000, 2000 + half, 2999, n - 1]
    for s in spikes:
        x[s] = (127, -128)
    x[300] = (60, 80)                                              # 3600 + 6400 = 10000 = thr^2: kept
    x[301] = (60, 81)                                              # blanked
    x[302] = (-100, 0)                                             # kept
    x[303] = (0, 101)                                              # blanked
    n_blank = len(set(spikes)) + 2
    if fmt == "c32":
        return (x[:, 0].astype(np.float32) + 1j * x[:, 1].astype(np.float32)).astype(np.complex64), n_blank
    return x, n_blank


@pytest.mark.parametrize("fmt", ["i8", "c32"])
def test_blanking(gpu, hipbuf, fmt):
    from gnss_sdr_rs_amd import resample
    rs = resample.Resampler(2, 3, blank_threshold=100.0)
    p = RM.resolve(2, 3, blank_threshold=100.0)
    assert RM.tile_outputs(p) == 1024 and p["T"] == 64
    g = rs.taps()
    n = 5003
    x, n_blank = _spiky(fmt, p, n)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, rs, d_x, fmt, n)
    want, weight, m = RM.run(p, g, x)
    assert m.blanked == n_blank
    _check((fmt, "whole"), whole, want, weight, p["T"])
    assert rs.stats() == dict(inputs=n, outputs=whole.size, blanked=n_blank)
    for blocks in SPLITS:
        rs.reset(0)
        got = _feed(hipbuf, rs, d_x, fmt, n, blocks or p["T"] - 1)
        assert (_words(got) == _words(whole)).all(), blocks
        assert rs.stats() == dict(inputs=n, outputs=whole.size, blanked=n_blank), blocks       # each input once, whatever the cuts
    # the blanked samples matter: the model without blanking is somewhere else
    plain_p = RM.resolve(2, 3)
    want_plain, weight_plain, _ = RM.run(plain_p, g, x)
    assert np.abs(want_plain - want).max() > 10.0
    # threshold 0 is a handle without blanking
    off, zero = resample.Resampler(2, 3), resample.Resampler(2, 3, blank_threshold=0.0)
    a, b = _feed(hipbuf, off, d_x, fmt, n), _feed(hipbuf, zero, d_x, fmt, n)
    assert (_words(a) == _words(b)).all() and zero.stats()["blanked"] == 0
    _check((fmt, "off"), a, want_plain, weight_plain, p["T"])
    for h in (rs, off, zero):
        h.close()


def test_the_ring_path(gpu, hipbuf):
    """write_ring with a resampler into a 2^12 ring, call after call over two wraps, against process_dev(front-end) ->
    process_dev(resampler) with the same block cuts (a call longer than the ring's 4096-sample staging slot is two blocks)"""
    from gnss_sdr_rs_amd import _lib, frontend, resample, tracking
    F_IF, FS = 1.25e6, 8.0e6
    ring = tracking.MulticastRingBuffer(1 << 12)
    fe, fe_ref = frontend.DigitalFrontend(F_IF, FS, FS * 2 / 3), frontend.DigitalFrontend(F_IF, FS, FS * 2 / 3)
    rs, rs_ref = resample.Resampler(2, 3, blank_threshold=150.0), resample.Resampler(2, 3, blank_threshold=150.0)
    p = RM.resolve(2, 3, blank_threshold=150.0)
    calls = [20, 3000, 6000, 4096, 17, 4091, 1234]                 # 20 < T/2 + 1: no output yet; 6000: blocks of 4096 and 1904
    x = _stream("i8", sum(calls), 23)
    d_x = hipbuf.upload(x)
    d_mid = hipbuf.alloc(4096 * 8)
    done = head = 0
    for n in calls:
        total = fe.write_ring(ring, x[done:done + n], resampler=rs)
        want_n = RM.plan(p, done, n)
        assert total == want_n and ring.get_enqueued_head() == head + want_n
        ring.flush()
        assert ring.get_head() == head + want_n
        ref = []
        for s in range(0, n, 4096):
            k = min(4096, n - s)
            fe_ref.process_dev(d_x + (done + s) * 2, _lib.FMT_I8_IQ, d_mid, k)
            fe_ref.synchronize()
            d_y = hipbuf.alloc(4096 * 8)
            got = rs_ref.process_dev(d_mid, _lib.FMT_C32, k, d_y, 4096)
            rs_ref.synchronize()
            ref.append(hipbuf.download(d_y, 4096 * 8, np.complex64)[:got])
        ref = np.concatenate(ref)
        assert ref.size == want_n
        if n == 20:
            assert want_n == 0 and ring.get_head() == 0              # too short to yield output: the head stays
        assert (_words(ring.copy_to_slice(head, want_n)) == _words(ref)).all(), n
        head += want_n
        done += n
    assert head > 2 * (1 << 12)                                      # the ring wrapped twice
    assert rs.stats() == rs_ref.stats() and rs.stats()["inputs"] == sum(calls) and rs.stats()["outputs"] == head
    assert rs.stats()["blanked"] > 0
    # more outputs than the ring holds: refused, nothing moved
    with pytest.raises(_lib.GmError) as e:
        fe.write_ring(ring, x[:6200], resampler=rs)
    assert e.value.status == OUT_OF_RANGE and ring.get_enqueued_head() == head and rs.stats()["inputs"] == sum(calls)
    st = gpu.lib().gm_frontend_write_ring_resampled(fe._h, rs._h, ring._h, x.ctypes.data_as(C.c_void_p), 64, _lib.FMT_I8_REAL, None)
    assert st == INVALID and ring.get_enqueued_head() == head
    # a plain write_ring on another ring gives the front-end's own words, as before
    ring2 = tracking.MulticastRingBuffer(1 << 12)
    fe2, fe3 = frontend.DigitalFrontend(F_IF, FS, FS), frontend.DigitalFrontend(F_IF, FS, FS)
    assert fe2.write_ring(ring2, x[:4096]) is None
    ring2.flush()
    fe3.process_dev(d_x, _lib.FMT_I8_IQ, d_mid, 4096)
    fe3.synchronize()
    assert ring2.get_head() == 4096
    assert (_words(ring2.copy_to_slice(0, 4096)) == _words(hipbuf.download(d_mid, 4096 * 8, np.complex64))).all()
    for h in (fe, fe_ref, fe2, fe3, rs, rs_ref, ring, ring2):
        h.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, resample
    import test_resample_host as TH
    L = gpu.lib()
    for cfg in TH.REFUSED:
        with pytest.raises(_lib.GmError) as e:
            resample.Resampler(**cfg)
        assert e.value.status == INVALID, cfg
    h = C.c_void_p()
    assert L.gm_resampler_create(None, C.byref(h)) == INVALID and L.gm_resampler_create(C.byref(_lib.ResamplerCfg(1, 1)), None) == INVALID
    rs = resample.Resampler(3, 2, blank_threshold=3.0)
    p = RM.resolve(3, 2, blank_threshold=3.0)
    g = rs.taps()
    n = 2500
    x = _stream("c32", n, 31)
    room = np.zeros(n + 2 * n, np.complex64)                        # the stream with room for its output right behind it
    room[:n] = x
    d_x = hipbuf.upload(room)
    d_y = hipbuf.alloc(2 * n * 8, fill=0x5A)
    first = 1000
    n1 = rs.process_dev(d_x, _lib.FMT_C32, first, d_y, 2 * n)
    state = rs.stats()
    assert state["inputs"] == first and state["outputs"] == n1 == RM.plan(p, 0, first) and state["blanked"] > 0
    rest = n - first
    n2 = RM.plan(p, first, rest)
    got = C.c_size_t(77)
    call = lambda d_in, fmt, n_in, d_out, cap: L.gm_resampler_process_dev(rs._h, d_in, fmt, n_in, d_out, cap, C.byref(got), None)
    src = d_x + first * 8
    assert call(src, _lib.FMT_I8_REAL, rest, d_y + n1 * 8, 2 * n) == INVALID
    assert call(src, 7, rest, d_y + n1 * 8, 2 * n) == INVALID
    assert call(None, _lib.FMT_C32, rest, d_y + n1 * 8, 2 * n) == INVALID
    assert call(src, _lib.FMT_C32, rest, None, 2 * n) == INVALID
    assert call(src, _lib.FMT_C32, rest, d_y + n1 * 8, n2 - 1) == OUT_OF_RANGE
    assert call(src, _lib.FMT_C32, rest, d_y + n1 * 8, 0) == OUT_OF_RANGE
    for d_out in (src, src + 8, src - 8 * (n2 - 1), src + rest * 8 - 8):          # d_out overlapping d_in
        assert call(src, _lib.FMT_C32, rest, d_out, n2) == INVALID, d_out - src
    assert got.value == 77 and rs.stats() == state
    assert L.gm_resampler_reset(rs._h, (1 << 62) + 1) == INVALID and rs.stats() == state
    assert (hipbuf.download(d_y + n1 * 8, 64, np.uint8) == 0x5A).all()            # nothing was written
    assert call(None, _lib.FMT_C32, 0, None, 0) == 0 and got.value == 0 and rs.stats() == state       # n_in = 0
    # d_out right behind d_in is no overlap; the next good call continues the stream as if nothing had been refused
    assert call(src, _lib.FMT_C32, rest, d_x + n * 8, 2 * n) == 0 and got.value == n2
    rs.synchronize()
    y = np.concatenate([hipbuf.download(d_y, n1 * 8, np.complex64), hipbuf.download(d_x + n * 8, n2 * 8, np.complex64)])
    want, weight, m = RM.run(p, g, x)
    _check("after the refusals", y, want, weight, p["T"])
    assert rs.stats() == dict(inputs=n, outputs=y.size, blanked=m.blanked)
    # the host-buffer form: the same words, the same refusals
    rs.reset(0)
    assert (_words(rs.process(x)) == _words(y)).all()
    out = np.zeros(4, np.complex64)
    st = L.gm_resampler_process(rs._h, x.ctypes.data_as(C.c_void_p), _lib.FMT_C32, 100, out.ctypes.data_as(C.c_void_p), 4, None)
    assert st == OUT_OF_RANGE and rs.stats()["inputs"] == n and not out.any()
    assert L.gm_resampler_process(rs._h, x.ctypes.data_as(C.c_void_p), _lib.FMT_I8_REAL, 100, out.ctypes.data_as(C.c_void_p), 4, None) == INVALID
    rs.close()


def test_a_resampled_dwell_needs_no_drift_compensation(gpu, hipbuf):
    """The host test's scene at 50 dB-Hz (code period 2047.6 samples): Resampler 5120/5119, then search_dev at N = 2048 WITHOUT the
    code-drift compensation finds the model's code phase +-1 on the true worker, with a peak-to-mean of at least 0.8 of the
    drift-compensated search of the original on the same GPU — the condition the model meets on the CPU (test_resample_host.py)."""
    from gnss_sdr_rs_amd import _lib, acquisition as A, resample
    import test_resample_host as TH
    r = TH.scene_run(50.0)
    print("model: plain %s, drift starts %s, resampled %s" % (r["plain"], r["drift"], r["resampled"]))
    assert r["resampled"][2] >= 0.8 * r["drift"][2] and r["plain"][2] < r["resampled"][2]
    rs = resample.Resampler.from_rates(2047600, 2048000)
    assert (rs.up, rs.down, rs.n_taps) == (RM.UP, RM.DOWN, 32)
    y = rs.process(r["x"])
    dwell = RM.PERIODS * RM.N
    assert y.size == RM.total_out(r["p"], RM.N_IN) >= dwell
    assert np.abs(y[:dwell] - r["y"]).max() <= 1e-4 * np.abs(r["y"]).max()
    eng = A.AcquisitionEngine(RM.FS, 0.0, RM.N, doppler_hz=RM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=RM.PERIODS,
                              codes=r["chips"], code_rate=1.023e6)
    assert eng.dwell_samples == dwell
    w = RM.SAT["worker"]
    d_y, d_x = hipbuf.upload(y[:dwell]), hipbuf.upload(r["x"])
    eng.search_dev(d_y, _lib.FMT_C32)
    resampled = RM.best_cell(*eng.metrics(), w)
    eng.search_dev(d_x, _lib.FMT_C32)
    plain = RM.best_cell(*eng.metrics(), w)
    eng.set_code_drift(np.full(3, RM.T_TRUE))
    assert eng.dwell_samples <= RM.N_IN
    eng.search_dev(d_x, _lib.FMT_C32)
    drift = RM.best_cell(*eng.metrics(), w)
    print("GPU: plain %s, drift compensation %s, resampled %s" % (plain, drift, resampled))
    assert resampled[0] == r["resampled"][0] and abs(resampled[1] - r["resampled"][1]) <= 1
    assert resampled[2] >= 0.8 * drift[2]
    assert plain[2] < resampled[2]
    other = RM.best_cell(*eng.metrics(), 1 - w)
    assert other[2] < 0.5 * drift[2]                                # the code that is not in the scene finds nothing
    eng.close()
    rs.close()
