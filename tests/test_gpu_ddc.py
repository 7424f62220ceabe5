"""Real-IF down-conversion on the GPU (gm_ddc, csrc/ddc_kernels.hip) against the model of ddc_model.py, which is handed the library's own
filter and phasor words (gm_ddc_tables) and forms the phasors and the products bit for bit as defined.

1. Words.  Per output and component |device - model| <= (T + 4) 2^-24 sum_j |c_j| |p_j|: tests/test_gpu_resample.py's dot-product bound
   with p in x's place (p is the same float32 word on both sides).  Derived, not measured; the largest error over bound is printed.
   Every ratio and tap count of CONFIGS, the mix values MIXES, the call lengths of _lengths and input pointers 0, 1, 3 and 15 bytes off
   an aligned allocation; the streams hold -128 and +127.
2. Splitting: one call against the same stream in blocks of 1, 7, T - 1, 1000 and 3001, bit for bit; after reset at absolute indices
   2^32 - 3 and 2^40 + 12345, where the words also go against the model (a 32-bit phase product shows there); two handles agree.
3. Blanking: spikes on a tile edge, in a halo, in the history and across a call boundary; exactly at the threshold.
4. Every refusal, with the state untouched.
5. gm_ddc_write_ring over two wraps of a 2^12 ring, for the four (excisor, resampler) combinations, against the host-buffer entries of
   fresh handles on the same blocks, word for word.
6. The chain: the host test's scene at 50 dB-Hz through Ddc.from_rates, then a plain search_dev at fft_size = 8184."""
import ctypes as C

import numpy as np
import pytest

import ddc_model as DM
import resample_model as RM
import stage_instantiations as SI

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5

# (up, down, taps, n_phases): 1/1 with 8 taps (the mix alone), 1/2 (up divides the phase count: no blend), 20460/40919 (blend), 3/8,
# 1/16 at 256 taps (a tile of 240 outputs, a lane owns one), 2/1, and 16 phases in place of 256 with and without the blend; and the three
# of stage_instantiations.py: the blend with a lane owning two outputs (3/16) and one (3/40 at 256 taps), and 4/25 (no blend, two
# outputs): with them every <BLEND, OPL> runs
CONFIGS = [(1, 1, 8, 0), (1, 2, 0, 0), (20460, 40919, 0, 0), (3, 8, 0, 0), (1, 16, 256, 0), (2, 1, 0, 0), (1, 2, 0, 16),
           (20460, 40919, 32, 16)] + SI.DDC_ADDED
MIXES = [0.0, 0.25, DM.MIX, -0.37, 1e-9]
OFFSETS = [0, 1, 3, 15]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stream(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-128, 128, n).astype(np.int8)
    if n > 2:
        x[n // 3], x[n // 2] = -128, 127
    return x


def _upload(hipbuf, x, offset):
    """x at `offset` bytes behind an aligned allocation -> the device address of x[0]"""
    buf = np.zeros(offset + x.size + 16, np.int8)
    buf[offset:offset + x.size] = x
    base = hipbuf.upload(buf)
    assert base % 256 == 0
    return base + offset


def _feed(hipbuf, d, d_x, n, blocks=None, cap=None):
    """the n bytes at d_x through d.process_dev in blocks (None: one call) -> complex64 outputs, all of them behind each other in one
    device buffer whose tail must stay as it was filled"""
    cap = cap if cap is not None else n * d.up // d.down + 2
    d_y = hipbuf.alloc(cap * 8 + 64, fill=0x5A)
    done = got = 0
    step = blocks or max(n, 1)
    while True:
        k = min(step, n - done)
        got += d.process_dev(d_x + done, k, d_y + got * 8, cap - got)
        done += k
        if done >= n:
            break
    d.synchronize()
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


def _lengths(T):
    return [1, T // 2 - 1, T // 2, T // 2 + 1, T - 1, 4095, 4113, 40000]


def _make(mix, config, **cfg):
    from gnss_sdr_rs_amd import ddc
    up, down, taps, phases = config
    d = ddc.Ddc(mix, up, down, taps=taps, n_phases=phases, **cfg)
    p = DM.resolve(mix, up, down, taps=taps, n_phases=phases, **cfg)
    assert (d.up, d.down, d.n_taps, d.n_phases, d.phase_inc) == (p["up"], p["down"], p["T"], p["PHI"], p["inc"])
    return d, p


@pytest.mark.parametrize("config", CONFIGS)
def test_words_against_the_model(gpu, hipbuf, config):
    from gnss_sdr_rs_amd import resample
    ci = CONFIGS.index(config)
    handles = [_make(mix, config) for mix in MIXES]
    p0 = handles[0][1]
    T = p0["T"]
    g, whi, wlo = handles[0][0].tables()
    assert (g == resample.design(config[0], config[1], taps=config[2], n_phases=config[3])).all()      # gm_resampler_design's words
    mine = DM.phasor_tables()
    assert np.abs(whi - mine[0]).max() <= 2.0 ** -23 and np.abs(wlo - mine[1]).max() <= 2.0 ** -23
    lengths = _lengths(T)
    x = _stream(lengths[-1], 17 + ci)
    d_xs = [_upload(hipbuf, x, off) for off in OFFSETS]
    worst = 0.0
    for i, n in enumerate(lengths):
        for j, off in enumerate(OFFSETS):
            d, p = handles[(i + j + ci) % len(MIXES)]
            d.reset(0)
            got = _feed(hipbuf, d, d_xs[j], n)
            want, weight, m = DM.run(p, g, whi, wlo, x[:n])
            worst = max(worst, _check((config, p["mix"], n, off), got, want, weight, T))
            assert d.stats() == dict(inputs=n, outputs=RM.total_out(p, n), blanked=0)
    for j, off in enumerate(OFFSETS):                                   # the input is only read
        assert (hipbuf.download(d_xs[j] - off, off + x.size, np.int8)[off:] == x).all()
    print("%s: tile %d outputs, largest error / bound %.3f" % (config, RM.tile_outputs(p0), worst))
    assert RM.total_out(p0, lengths[1]) == 0 and RM.total_out(p0, lengths[3]) >= 1
    for d, _ in handles:
        d.close()


SPLITS = (1, 7, None, 1000, 3001)          # None: T - 1


@pytest.mark.parametrize("config,mix", [((1, 2, 0, 0), DM.MIX), ((20460, 40919, 0, 0), -0.37), ((3, 8, 0, 0), 0.25),
                                        (SI.RESAMPLE_BLEND_1, DM.MIX)])
def test_the_words_do_not_depend_on_the_cuts(gpu, hipbuf, config, mix):
    d, p = _make(mix, config)
    twin, _ = _make(mix, config)
    g, whi, wlo = d.tables()
    n = 6007
    x = _stream(n, 5)
    d_x = _upload(hipbuf, x, 1)
    whole = _feed(hipbuf, d, d_x, n)
    want, weight, _ = DM.run(p, g, whi, wlo, x)
    _check((config, "whole"), whole, want, weight, p["T"])
    assert (_words(_feed(hipbuf, twin, d_x, n, 1000)) == _words(whole)).all()                   # two handles, the same words
    for blocks in SPLITS:
        d.reset(0)
        got = _feed(hipbuf, d, d_x, n, blocks or p["T"] - 1)
        assert (_words(got) == _words(whole)).all(), (config, blocks)
    # absolute indices at and above 2^32: the model at those indices, and the cuts still do not matter
    for index in ((1 << 32) - 3, (1 << 40) + 12345):
        d.reset(index)
        far = _feed(hipbuf, d, d_x, n)
        want, weight, m = DM.run(p, g, whi, wlo, x, input_index=index)
        assert far.size == m.outputs == RM.plan(p, index, n)
        _check((config, index), far, want, weight, p["T"])
        assert not (far.size == whole.size and (_words(far) == _words(whole)).all())            # the phase is the absolute index's
        for blocks in SPLITS:
            d.reset(index)
            assert (_words(_feed(hipbuf, d, d_x, n, blocks or p["T"] - 1)) == _words(far)).all(), (index, blocks)
        twin.reset(index)
        assert (_words(_feed(hipbuf, twin, d_x, n, 3001)) == _words(far)).all()
        assert d.stats() == dict(inputs=n, outputs=far.size, blanked=0)
    d.close()
    twin.close()


def _spiky(p, n):
    """a quiet stream (|x| <= 20) with spikes inside the first tile, around the input the second tile starts at (both tiles' halos),
    around the cuts of the 1000-sample split, and the values exactly at / just above the threshold 100"""
    rng = np.random.default_rng(9)
    x = rng.integers(-20, 21, n).astype(np.int8)
    edge = RM.tile_outputs(p) * p["down"] // p["up"]               # i0 of the second tile's first output
    half = p["T"] // 2
    spikes = [700, edge - half, edge - 1, edge, edge + 1, edge + half, 999, 1000, 1001, 1999, 2000, 2000 + half, 2999, n - 1]
    for i, s in enumerate(spikes):
        x[s] = 127 if i % 2 else -128
    x[300], x[301], x[302], x[303] = 100, 101, -100, -101           # 100^2 = thr^2: kept; 101: blanked
    return x, len(set(spikes)) + 2


def test_blanking(gpu, hipbuf):
    config = (1, 2, 0, 0)
    d, p = _make(DM.MIX, config, blank_threshold=100.0)
    assert RM.tile_outputs(p) == 1024 and p["T"] == 64
    g, whi, wlo = d.tables()
    n = 5003
    x, n_blank = _spiky(p, n)
    d_x = _upload(hipbuf, x, 3)
    whole = _feed(hipbuf, d, d_x, n)
    want, weight, m = DM.run(p, g, whi, wlo, x)
    assert m.blanked == n_blank
    _check("whole", whole, want, weight, p["T"])
    assert d.stats() == dict(inputs=n, outputs=whole.size, blanked=n_blank)
    for blocks in SPLITS:
        d.reset(0)
        got = _feed(hipbuf, d, d_x, n, blocks or p["T"] - 1)
        assert (_words(got) == _words(whole)).all(), blocks
        assert d.stats() == dict(inputs=n, outputs=whole.size, blanked=n_blank), blocks        # each input once, whatever the cuts
    # the blanked samples matter: the model without blanking is somewhere else
    plain_p = DM.resolve(DM.MIX, 1, 2)
    want_plain, weight_plain, _ = DM.run(plain_p, g, whi, wlo, x)
    assert np.abs(want_plain - want).max() > 1.0
    off, _ = _make(DM.MIX, config)
    a = _feed(hipbuf, off, d_x, n)
    assert off.stats()["blanked"] == 0
    _check("off", a, want_plain, weight_plain, p["T"])
    d.close()
    off.close()


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, ddc
    import test_resample_host as TH
    L = gpu.lib()
    for cfg in TH.REFUSED:
        with pytest.raises(_lib.GmError) as e:
            ddc.Ddc(DM.MIX, **cfg)
        assert e.value.status == INVALID, cfg
    for mix in (float("nan"), float("inf")):
        with pytest.raises(_lib.GmError) as e:
            ddc.Ddc(mix, 1, 2)
        assert e.value.status == INVALID
    h = C.c_void_p()
    assert L.gm_ddc_create(None, C.byref(h)) == INVALID and L.gm_ddc_create(C.byref(_lib.DdcCfg(0.25, 1, 1)), None) == INVALID
    d, p = _make(DM.MIX, (3, 8, 0, 0), blank_threshold=100.0)
    g, whi, wlo = d.tables()
    n = 2504
    x = _stream(n, 31)
    room = np.zeros(n + 8 * n, np.int8)                             # the stream with room for its output right behind it
    room[:n] = x
    d_x = hipbuf.upload(room)
    d_y = hipbuf.alloc(n * 8, fill=0x5A)
    first = 1000
    n1 = d.process_dev(d_x, first, d_y, n)
    state = d.stats()
    assert state["inputs"] == first and state["outputs"] == n1 == RM.plan(p, 0, first) and state["blanked"] > 0
    rest = n - first
    n2 = RM.plan(p, first, rest)
    got = C.c_size_t(77)
    call = lambda d_in, n_in, d_out, cap: L.gm_ddc_process_dev(d._h, d_in, n_in, d_out, cap, C.byref(got), None)
    src = d_x + first
    assert call(None, rest, d_y + n1 * 8, n) == INVALID
    assert call(src, rest, None, n) == INVALID
    assert call(src, rest, d_y + n1 * 8, n2 - 1) == OUT_OF_RANGE
    assert call(src, rest, d_y + n1 * 8, 0) == OUT_OF_RANGE
    assert call(src, (1 << 31) + 1, d_y + n1 * 8, n) == INVALID
    for d_out in (src, src + 1, src - 8 * n2 + 1, src + rest - 1):                # d_out overlapping d_in
        assert call(src, rest, d_out, n2) == INVALID, d_out - src
    assert got.value == 77 and d.stats() == state
    assert L.gm_ddc_reset(d._h, (1 << 62) + 1) == INVALID and d.stats() == state
    assert (hipbuf.download(d_y + n1 * 8, 64, np.uint8) == 0x5A).all()            # nothing was written
    assert call(None, 0, None, 0) == 0 and got.value == 0 and d.stats() == state  # n_in = 0
    # d_out right behind d_in is no overlap; the next good call continues the stream as if nothing had been refused
    assert call(src, rest, d_x + n, n2) == 0 and got.value == n2
    d.synchronize()
    y = np.concatenate([hipbuf.download(d_y, n1 * 8, np.complex64), hipbuf.download(d_x + n, n2 * 8, np.complex64)])
    want, weight, m = DM.run(p, g, whi, wlo, x)
    _check("after the refusals", y, want, weight, p["T"])
    assert d.stats() == dict(inputs=n, outputs=y.size, blanked=m.blanked)
    # the host-buffer form: the same words, the same refusals
    d.reset(0)
    assert (_words(d.process(x)) == _words(y)).all()
    out = np.zeros(4, np.complex64)
    st = L.gm_ddc_process(d._h, x.ctypes.data_as(C.c_void_p), 100, out.ctypes.data_as(C.c_void_p), 4, None)
    assert st == OUT_OF_RANGE and d.stats()["inputs"] == n and not out.any()
    assert L.gm_ddc_process(d._h, None, 100, out.ctypes.data_as(C.c_void_p), 4, None) == INVALID
    d.close()


@pytest.mark.parametrize("with_excisor,with_resampler", [(False, False), (True, False), (False, True), (True, True)])
def test_the_ring_path(gpu, with_excisor, with_resampler):
    """write_ring into a 2^12 ring, call after call over two wraps, against Ddc.process -> Excisor.process -> Resampler.process of
    fresh handles with the same block cuts (a call longer than the ring's 4096-sample staging slot is two blocks)"""
    from gnss_sdr_rs_amd import _lib, ddc, excise, resample, tracking
    ring = tracking.MulticastRingBuffer(1 << 12)
    mk = lambda: (ddc.Ddc(DM.MIX, 1, 2, blank_threshold=120.0), excise.Excisor(256) if with_excisor else None,
                  resample.Resampler(2, 3) if with_resampler else None)
    d, ex, rs = mk()
    d_ref, ex_ref, rs_ref = mk()
    if with_excisor:
        gains = np.ones(256, np.float32)
        gains[40:44] = 0.0                                           # a notch: the excisor is not the identity
        ex.set_gains(gains)
        ex_ref.set_gains(gains)
    calls = [20, 3000, 6000, 4096, 17, 4091, 1234, 8000, 8192, 5000, 7000]
    x = _stream(sum(calls), 23)
    done = head = 0
    for n in calls:
        block = x[done:done + n]
        total = d.write_ring(ring, block, excisor=ex, resampler=rs)
        ref = []
        for s in range(0, n, 4096):
            y = d_ref.process(block[s:s + 4096])
            if with_excisor and y.size:
                y = ex_ref.process(y)
            if with_resampler and y.size:
                y = rs_ref.process(y)
            ref.append(y)
        ref = np.concatenate(ref)
        assert total == ref.size and ring.get_enqueued_head() == head + ref.size
        ring.flush()
        assert ring.get_head() == head + ref.size
        if n == 20:
            assert ref.size == 0 and ring.get_head() == 0             # too short to yield output: the head stays
        assert (_words(ring.copy_to_slice(head, ref.size)) == _words(ref)).all(), n
        head += ref.size
        done += n
    assert head > 2 * (1 << 12)                                      # the ring wrapped twice
    assert d.stats() == d_ref.stats() and d.stats()["inputs"] == sum(calls) and d.stats()["blanked"] > 0
    for a, b in ((ex, ex_ref), (rs, rs_ref)):
        if a is not None:
            assert a.stats() == b.stats() and a.stats()["inputs"] > 0
    last = rs if with_resampler else ex if with_excisor else d
    assert last.stats()["outputs"] == head
    # more outputs than the ring holds: refused, nothing moved
    before = d.stats()
    with pytest.raises(_lib.GmError) as e:
        d.write_ring(ring, np.zeros(14000, np.int8), excisor=ex, resampler=rs)
    assert e.value.status == OUT_OF_RANGE and ring.get_enqueued_head() == head and d.stats() == before
    assert gpu.lib().gm_ddc_write_ring(d._h, None, None, ring._h, None, 64, None) == INVALID and d.stats() == before
    for h in (d, d_ref, ex, ex_ref, rs, rs_ref, ring):
        if h is not None:
            h.close()


def test_a_down_converted_capture_is_searched_at_half_the_size(gpu, hipbuf):
    """The host test's scene at 50 dB-Hz (int8 real at 16.3676 Msps, IF 4.1304 MHz, code period 16367.6 samples): Ddc.from_rates to
    8.184 Msps, then a plain search_dev at fft_size = 8184 finds the +1 kHz bin and the model's code phase +-1.  Printed for
    comparison: the same int8 real dwell searched directly at 16368 with the code-drift compensation."""
    from gnss_sdr_rs_amd import _lib, acquisition as A, ddc
    import test_ddc_host as TH
    r = TH.scene_run(50.0)
    print("model: down-converted %s" % (r["ddc"],))
    assert r["ddc"][0] == DM.TRUE_BIN and abs(r["ddc"][1] - DM.EXPECTED_PHASE) <= 1
    d = ddc.Ddc.from_rates(16367600, 8184000, 4130400)
    assert (d.up, d.down, d.n_taps, d.phase_inc) == (DM.UP, DM.DOWN, 64, DM.phase_inc(DM.MIX))
    y = d.process(r["x"])
    dwell = DM.M * DM.N
    assert y.size == RM.total_out(r["p"], DM.N_IN) >= dwell
    assert np.abs(y[:dwell] - r["y"]).max() <= 1e-4 * np.abs(r["y"]).max()
    eng = A.AcquisitionEngine(DM.FS_OUT, 0.0, DM.N, doppler_hz=DM.DOP.astype(np.float32), prn_ids=[1], n_integrations=DM.M,
                              codes=r["chips"], code_rate=1.023e6)
    assert eng.dwell_samples == dwell
    eng.search_dev(hipbuf.upload(y[:dwell]), _lib.FMT_C32)
    found = DM.best_cell(*eng.metrics())
    eng.close()
    direct = A.AcquisitionEngine(DM.FS_IN, DM.F_MIX, 16368, doppler_hz=DM.DOP.astype(np.float32), prn_ids=[1], n_integrations=DM.M,
                                 codes=r["chips"], code_rate=1.023e6)
    direct.set_code_drift(np.full(DM.DOP.size, DM.T_TRUE))
    assert direct.dwell_samples <= DM.N_IN
    direct.search_dev(hipbuf.upload(r["x"]), _lib.FMT_I8_REAL)
    real = DM.best_cell(*direct.metrics(), n=16368)
    direct.close()
    print("GPU: down-converted, N = 8184 %s; int8 real with drift compensation, N = 16368 %s" % (found, real))
    assert found[0] == DM.TRUE_BIN and abs(found[1] - DM.EXPECTED_PHASE) <= 1
    assert found[0] == r["ddc"][0] and abs(found[1] - r["ddc"][1]) <= 1
    d.close()
