"""GPU: the classes of the C++ host mirror (gnss-sdr-rs_amd/host/gnss_sdr.hpp) that tests/cpp/test_host_api.cpp does not run, through
tests/cpp/host_stages.cpp: one fresh child process per case, at most 60 s each, one at a time.

(a) Word for word.  The same inputs and the same sequence of calls go through gnss_sdr_rs_amd's own class in this process, on the same
    library; every output word, count, flag and statistic of the C++ run must equal the Python run's byte for byte (tests/
    host_stages_case.py builds both sides of a step from one definition).  Buffers handed to a _dev method lie between two 64-byte
    guards of 0x5A and start as 0x5A themselves; their whole image is compared, so a word written past the delivered count, between two
    planes or into a guard fails the test.  No stage had to fall back to (b) alone: every stage was bit-stable between the two runs.
(b) One model check per class: the C++ words of one case against the float64 model in tests/*_model.py at the bar of that class's
    own GPU test, imported from it (test_gpu_resample._check, test_gpu_excise._check, test_gpu_ddc._check, test_gpu_channelizer._check,
    test_gpu_nuller._check, test_gpu_stap._check for Stap and for every beam of a Beamformer, test_gpu_lcmv._check, fft_model's bound and
    Bluestein's L2 bars of test_gpu_fft_paths).  The ring writers and the re-steering entries have no float64 model of their
    own stream: the Python ring path they equal word for word is held to the process() chains of fresh handles by the ring tests of
    test_gpu_ddc, test_gpu_excise and test_gpu_resample, and test_resteer holds the solved rows to tests/array_probe_model.py.

Call lengths of the streaming stages, on one handle, in this order: 0, 1, B - 1, 1, B, B + 1, 3B - 1 (B: the smallest block the plan
accepts, 256; the excisor's segment H = 128; T / 2 for the resampler and the down-converter, so that calls of T/2 - 1 and T/2 + 1 inputs
are there), in both sample formats, then after a reset to 2^32 - 3 calls of B - 1 and 1, where the call of one sample delivers a whole
block.

method -> operation of the driver -> test
  Resampler(cfg), Resampler(up, down, blank), process, process_i8, process_dev, reset, stats, taps, synchronize -> resampler -> test_resampler
  Excisor(cfg), Excisor(block, guard, blank), block, process, process_i8, process_dev, adapt_dev, set_gains, gains, psd (all three outputs
    and none), set_block_adapt, clear_block_adapt, block_stats, block_capture, reset, stats, synchronize -> excisor -> test_excisor
  Ddc(cfg), Ddc(mix, up, down, blank), process, process_dev, reset, stats, tables, synchronize -> ddc -> test_ddc
  Ddc::plan -> plans -> test_cpp_host_stages_host.test_the_plans
  Ddc::write_ring (alone, with an Excisor, with a Resampler, with both) -> ring -> test_the_ring_writers
  Channelizer(cfg), Channelizer(M, D, channels, blank), planes, glonass_channels, process, process_dev, reset, stats, taps, synchronize
    -> channelizer -> test_channelizer;  glonass_code, glonass_channels -> glonass -> test_cpp_host_stages_host
  Nuller, block, antennas, process (R, w, both, neither), process_dev, set_weights (and empty), capture, reset, stats, synchronize
    -> nuller -> test_nuller
  Stap, block, antennas, taps, weights, process, process_dev, set_weights, capture, reset, stats (with and without fallback_blocks),
    synchronize -> stap -> test_stap
  Beamformer, block, weights, beams, process (n_out, R, w), process_dev, set_steering, set_weights, capture, reset, stats (with and
    without the fallbacks vector), synchronize -> beamformer -> test_beamformer
  Lcmv, Lcmv::Beam, block, weights, beams, process, process_dev, set_constraints (a Q that changes), set_weights, capture, reset, stats,
    synchronize -> lcmv -> test_lcmv
  DigitalFrontend::write_ring / write_ring_i8 with a Resampler, with an Excisor, with both -> ring -> test_the_ring_writers
  FFT::execute (one item and a batch of 3), FFT::power_spectrum, RealFFT::execute -> fft -> test_fft
  solve_row, solve_plan, TrackingManager::bank_plan, ::array_plan -> solve_row, plans -> test_cpp_host_stages_host
  every refused construction -> refuse -> test_cpp_host_stages_host; every wrong-size vector the header checks itself and one refused
    call per handle, each followed by one more block -> the classes' own operations above
  solve_plan, solve_rows_dev (R empty and R captured from a Stap), Beamformer::set_steering_dev (every default; with the flags; with
    d_info and a min_ratio that rejects one row), Stap::capture into device buffers -> resteer -> test_resteer

  AcquisitionEngine from caller-built tables, search_i8 against search, refine_doppler (one worker not found; none found),
    local_search and cancel (snapshot and device dwell, both formats; no candidate), array_prompts (no candidate and three), solve_row and
    solve_rows_dev on array_prompts' words as they came out -> acquisition -> test_acquisition_from_caller_built_tables
  AcquisitionEngine with coherent_periods = 2: set_edge_search, set_code_drift, dwell_samples after each, edge_offset_periods,
    refine_doppler, local_search -> acquisition -> test_acquisition_coherent_edges_and_drift
  TrackingManager::bank, ::array_prompts (own channels; a record vector with a skipped record; with and without done and offsets),
    ::array_prompts_dev, TrackingChannel::start -> tracking -> test_tracking_bank_and_array_prompts

Left out, and why: nothing of the list.  Two choices differ from it.  The acquisition cases run at fft_size 2048, not at the 256 of the
refine, local-search and cancel tests: those use custom code tables, which neither C++ constructor takes, and 2048 is the smallest size
at which the suite runs these entries on the C/A code (test_gpu_array_probe, the i8 cells of the refine and local-search tests).  The scene
carries no secondary code, so the row (1, -1) is set and its dwell read, and the search itself runs under the row (1, 1).  test_resteer
keeps synthetic prompt vectors for the gate's sake (a row that a min_ratio rejects); that array_prompts' [cands][R_u][taps][n_antennas]
words are what solve_row and solve_rows_dev take is checked in the acquisition case, which hands them over as they came out.

Two defects turned up and are fixed in the header.  Excisor::set_gains threw std::invalid_argument for a vector of the wrong size where
every other size check of the header throws gnss::Panic(GM_ERR_INVALID_ARG); test_excisor's refused set_gains step ended the child with an
unhandled exception before the fix.  AcquisitionEngine::array_prompts and ::local_search handed the library the null data() of an empty
candidate vector (and local_search that of an empty result vector), which it refuses before it looks at the count: no candidates threw
a Panic where the ABI and the Python layer return nothing.  Both now hand over a spare entry.

Proof that these tests can fail, on copies of the header that were not kept: Beamformer::process copying from p * got fails
test_beamformer[2-8-3], [8-4-16] and [8-1-3] at the first call that delivers a block (record y, first difference at plane 1; the one-beam
case cannot see it); Nuller::process handing w where R belongs (and R where w belongs, both vectors sized for R so that nothing is written
out of bounds) fails test_nuller[2] and [8] at the first R; Channelizer::process with cap = n / decim_ fails both test_channelizer cases
with a Panic from the first call that delivers n / D + 1 outputs.

Wall time on an MI355X, from pytest's own report of this file alone: 42 cases in 19.40 s, of which the one g++ compile of the driver
(the module fixture; its cost is g++'s) took 1.45 s, so about 18 s for the 42 cases.  (In that run the first acquisition case still
held a finer_doppler step, which the library refuses at this size in both layers; it ended there after 0.29 s, and runs to its end in
about the same time since.)  The slowest calls are the first imports of the existing GPU tests the bars come from (test_nuller[2] 1.75 s,
test_resampler[16-1-0] 1.06 s); every other case takes 0.22 .. 0.56 s, most of it the child's start and its first use of the device.
That is six times tests/test_gpu_grid_geometry.py's 3.4 s for 42 child processes, and below 30 s in all.
"""
import numpy as np
import pytest

import host_stages_case as H
from host_stages_case import C32, I8_IQ

pytestmark = pytest.mark.gpu
B = 256
AT = (1 << 32) - 3


@pytest.fixture(scope="module")
def exe(gm):
    return H.build(gm)[0]


def _lengths(b):
    return [0, 1, b - 1, 1, b, b + 1, 3 * b - 1]


def _cuts(x, lengths):
    at, out = 0, []
    for n in lengths:
        out.append(x[at:at + n])
        at += n
    return out, at


def _both(exe, tmp_path, hipbuf, op, head, steps, make, first=lambda o: []):
    """the case through the driver in a child, then through the Python layer's object here -> the C++ records"""
    body, run = H.case(head, steps)
    cpp = H.run_driver(exe, op, body, tmp_path)
    obj = make()
    try:
        py = list(first(obj)) + run(obj, hipbuf)
    finally:
        for h in (obj if isinstance(obj, tuple) else (obj,)):
            if h is not None:
                h.close()
    H.same(cpp, py, op)
    for tag, b in cpp:
        if tag.endswith("guards"):
            assert np.frombuffer(b, np.uint32)[0] == 1, tag
    return cpp


def _stream(fmt, n, seed):
    from test_gpu_resample import _stream as s
    return s("i8" if fmt == I8_IQ else "c32", n, seed)


def _ys(cpp, first, count):
    return np.concatenate(H.get(cpp, "y", np.complex64)[first:first + count])


# ---------------------------------------------------------------------------------------------------------------- Resampler
@pytest.mark.parametrize("up,down,short_form", [(16, 1, 0), (1, 16, 0), (6, 4, 1)])
def test_resampler(gpu, hipbuf, exe, tmp_path, up, down, short_form):
    import resample_model as RM
    import test_gpu_resample as TR
    from gnss_sdr_rs_amd import resample
    pl = resample.plan(up, down)
    T, lengths = pl["taps"], _lengths(pl["taps"] // 2)
    steps, xs = [], {}
    for fmt in (C32, I8_IQ):
        x = _stream(fmt, sum(lengths) + 4 * T, 5 + up)
        cuts, at = _cuts(x, lengths)
        xs[fmt] = x[:at]
        steps += [H.s_reset(0)] + [H.s_process(fmt, c) for c in cuts] + [H.s_stats()]
        n = 2 * T + 3
        steps += [H.s_process_dev(fmt, x[at:at + n], n * pl["up"] // pl["down"] + 2 + 5), H.s_stats()]
        steps += [H.s_reset(AT), H.s_process(fmt, x[:T - 1]), H.s_process(fmt, x[T - 1:T]), H.s_process(fmt, x[T:2 * T + 1]), H.s_stats()]
        # a refused call (no room for the outputs), then one more block: the handle is as it was
        steps += [H.refused(H.s_process_dev(fmt, x[:2 * T], 0)), H.s_process(fmt, x[2 * T + 1:3 * T]), H.s_stats()]
    steps.append(H.s_taps((pl["n_phases"] + 1) * T))
    head = H.pk("IIIIfffI", up, down, 0, 0, 0.0, 0.0, 0.0, short_form)
    cpp = _both(exe, tmp_path, hipbuf, "resampler", head, steps, lambda: resample.Resampler(up, down))
    p, g = RM.resolve(up, down), H.get(cpp, "taps", np.float32, 0).reshape(pl["n_phases"] + 1, T)
    per = len(H.get(cpp, "y", np.complex64)) // 2
    for k, fmt in enumerate((C32, I8_IQ)):
        want, weight, _ = RM.run(p, g, xs[fmt])
        got = _ys(cpp, k * per, len(lengths))
        assert got.size == RM.total_out(p, xs[fmt].shape[0])
        print("resampler %d/%d fmt %d: largest error / bound %.3f" % (up, down, fmt, TR._check((up, down, fmt), got, want, weight, T)))


# ---------------------------------------------------------------------------------------------------------------- Excisor
@pytest.mark.parametrize("short_form", [0, 1])
def test_excisor(gpu, hipbuf, exe, tmp_path, short_form):
    import excise_model as EM
    import test_gpu_excise as TE
    from gnss_sdr_rs_amd import excise
    H2 = B // 2
    lengths = _lengths(H2)
    gains = TE._gain_sets(B, 3)[1][1]
    steps, xs, held = [H.s_set_gains(gains), H.s_gains()], {}, H._Held()
    for fmt in (C32, I8_IQ):
        x = _stream(fmt, sum(lengths) + 8 * B, 9 + fmt)
        cuts, at = _cuts(x, lengths)
        xs[fmt] = x[:at]
        steps += [H.s_reset(0)] + [H.s_process(fmt, c) for c in cuts] + [H.s_stats()]
        steps += [H.s_process_dev(fmt, x[at:at + 2 * B + 3], 2 * B + 3 + B + 5), H.s_stats()]
        steps += [H.s_reset(AT), H.s_process(fmt, x[:H2 - 1]), H.s_process(fmt, x[H2 - 1:H2]), H.s_process(fmt, x[H2:B + 1]), H.s_stats()]
        # the adaptive step, its words with all three optional outputs and with none, and the gains it left
        steps += [H.s_adapt_dev(fmt, x[:6 * B]), H.s_psd(), H.s_gains(), H.s_process(fmt, x[B + 1:3 * B])]
        # block-adapt mode with a capture on device buffers, its counters, and off again
        steps += [H.s_set_block_adapt(0.0, 2), H.s_block_capture(8, held), H.s_process_dev(fmt, x[3 * B:3 * B + 5 * H2], 6 * H2 + 5),
                  H.s_block_capture(0, held), H.s_block_stats(), H.s_clear_block_adapt(), H.s_set_gains(gains)]
        # the wrong-size set_gains throws; then one more block
        steps += [H.refused(H.s_set_gains(gains[:-1])), H.refused(H.s_process_dev(fmt, x[:B], 0)), H.s_process(fmt, x[6 * B:7 * B]), H.s_gains(),
                  H.s_stats()]
    head = H.pk("IIffI", B, 0, 0.0, 0.0, short_form)
    cpp = _both(exe, tmp_path, hipbuf, "excisor", head, steps, lambda: excise.Excisor(B), lambda o: [H.u32("block", o.block)])
    p = EM.resolve(B)
    wa, ws = excise.windows(B)
    per = len(H.get(cpp, "y", np.complex64)) // 2
    for k, fmt in enumerate((C32, I8_IQ)):
        want, scale, _ = EM.run(p, xs[fmt], wa, ws, gains)
        got = _ys(cpp, k * per, len(lengths))
        assert got.size == EM.total_out(B, xs[fmt].shape[0])
        print("excisor fmt %d: largest error / bound %.3f" % (fmt, TE._check((B, fmt), got, want, scale)))


# ---------------------------------------------------------------------------------------------------------------- Ddc
@pytest.mark.parametrize("up,down,short_form", [(16, 1, 1), (1, 16, 0), (6, 4, 0)])
def test_ddc(gpu, hipbuf, exe, tmp_path, up, down, short_form):
    import ddc_model as DM
    import test_gpu_ddc as TD
    from gnss_sdr_rs_amd import ddc
    mix = DM.MIX
    pl = ddc.plan(mix, up, down)
    T, lengths = pl["taps"], _lengths(pl["taps"] // 2)
    x = TD._stream(sum(lengths) + 4 * T, 21 + up)
    cuts, at = _cuts(x, lengths)
    steps = [H.s_ddc_process(c) for c in cuts] + [H.s_stats()]
    n = 2 * T + 3
    for offset in (0, 3):
        steps += [H.s_ddc_process_dev(x[at:at + n], n * pl["up"] // pl["down"] + 2 + 5, offset), H.s_stats()]
    steps += [H.s_reset(AT), H.s_ddc_process(x[:T - 1]), H.s_ddc_process(x[T - 1:T]), H.s_ddc_process(x[T:2 * T + 1]), H.s_stats()]
    steps += [H.refused(H.s_ddc_process_dev(x[:2 * T], 0, 0)), H.s_ddc_process(x[2 * T + 1:3 * T]), H.s_stats(),
              H.s_ddc_tables((pl["n_phases"] + 1) * T)]
    head = H.pk("dIIIIfffI", mix, up, down, 0, 0, 0.0, 0.0, 0.0, short_form)
    cpp = _both(exe, tmp_path, hipbuf, "ddc", head, steps, lambda: ddc.Ddc(mix, up, down))
    p, g = DM.resolve(mix, up, down), H.get(cpp, "taps", np.float32, 0).reshape(pl["n_phases"] + 1, T)
    whi, wlo = H.get(cpp, "whi", np.complex64, 0), H.get(cpp, "wlo", np.complex64, 0)
    want, weight, _ = DM.run(p, g, whi, wlo, x[:at])
    print("ddc %d/%d: largest error / bound %.3f" % (up, down, TD._check((up, down), _ys(cpp, 0, len(lengths)), want, weight, T)))


# ---------------------------------------------------------------------------------------------------------------- Channelizer
@pytest.mark.parametrize("M,D,channels,short_form", [(4, 3, [2, 0, 3], 1), (64, 64, "glonass", 0)])
def test_channelizer(gpu, hipbuf, exe, tmp_path, M, D, channels, short_form):
    import channelizer_model as CM
    import test_gpu_channelizer as TC
    from gnss_sdr_rs_amd import channelizer
    glonass = channels == "glonass"
    listed = channelizer.glonass_channels(M) if glonass else channels
    pl = channelizer.plan(M, D, channels=listed)
    L = pl["n_taps"]
    # nothing, no output yet, the first outputs, then calls around multiples of D
    lengths = [0, 1, L // 2 - 1, 1, 5 * D, 5 * D + 1, 5 * D - 1, 1, 3 * L - 1]
    steps, xs = [], {}
    for fmt in (C32, I8_IQ):
        x = TC._stream("i8" if fmt == I8_IQ else "c32", sum(lengths) + 4 * L, 31 + M, M)
        cuts, at = _cuts(x, lengths)
        xs[fmt] = x[:at]
        steps += [H.s_reset(0)] + [H.s_ch_process(fmt, c) for c in cuts] + [H.s_stats()]
        n = L + 7 * D + 1
        cap = n // D + 2
        steps += [H.s_ch_process_dev(fmt, x[at:at + n], cap + 5, cap), H.s_stats()]
        steps += [H.s_reset(AT), H.s_ch_process(fmt, x[:L - 1]), H.s_ch_process(fmt, x[L - 1:L]), H.s_stats()]
        steps += [H.refused(H.s_ch_process_dev(fmt, x[:2 * L], 2 * L, 0)), H.s_ch_process(fmt, x[L:2 * L + D]), H.s_stats()]
    steps.append(H.s_taps())
    head = H.pk("IIIfffII", M, D, 0, 0.0, 0.0, 0.0, short_form, int(glonass)) + H.words(np.uint32, [] if glonass else listed)
    cpp = _both(exe, tmp_path, hipbuf, "channelizer", head, steps, lambda: channelizer.Channelizer(M, D, channels=listed),
                lambda o: [H.u32("planes", len(o.channels))])
    p, g = CM.resolve(M, D, channels=listed), H.get(cpp, "taps", np.float32, 0)
    ys, outs = H.get(cpp, "y", np.complex64), H.get(cpp, "n_out", np.uint64)
    per = len(ys) // 2
    for k, fmt in enumerate((C32, I8_IQ)):
        planes = [ys[i].reshape(len(listed), int(outs[i][0])) for i in range(k * per, k * per + len(lengths))]
        want, weight, _ = CM.run(p, g, xs[fmt])
        print("channelizer M %d D %d fmt %d: largest |C++ - model| / sum |g||x| = %.3g (bar %.0e)"
              % (M, D, fmt, TC._check((M, D, fmt), np.concatenate(planes, axis=1), want, weight), TC.BAR))


# ---------------------------------------------------------------------------------------------------------------- the array stages
def _array_stream(fmt, n, A, seed):
    import test_gpu_stap as TS
    return TS._stream("i8" if fmt == I8_IQ else "c32", n, A, seed)


def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _array_steps(A, words_w, wrong_w, process, process_dev, stats, extra, held):
    """the sequence every array class runs, per format: the call lengths with R and w asked for, a call with neither and with one of
    them, process_dev with a capture into device buffers, static weights and back, `extra` (the class's own setters), a reset far out
    where a call of one sample delivers a block, the refusals and one more block -> (steps, the inputs of the first calls per format)"""
    lengths = _lengths(B)
    steps, xs = [], {}
    for fmt in (C32, I8_IQ):
        x = _array_stream(fmt, sum(lengths) + 9 * B, A, 50 + A + fmt)
        cuts, at = _cuts(x, lengths)
        xs[fmt] = x[:at]
        steps += [H.s_reset(0)] + [process(c, 3) for c in cuts] + [stats(False)]
        steps += [process(x[at:at + B - 1], 0), process(x[at + B - 1:at + 2 * B + 3], 1), process(x[at + 2 * B + 3:at + 3 * B], 2), stats(True)]
        n = 2 * B + 3
        steps += [H.s_capture(4, held), process_dev(x[:n], n), H.s_capture(0, held), stats(False)]
        steps += [H.s_set_weights(words_w), process(x[n:n + B + 5], 3), H.s_set_weights(None), process(x[n + B + 5:n + 2 * B + 9], 3)]
        steps += extra(x[n + 2 * B + 9:n + 4 * B])
        steps += [H.s_reset(AT), process(x[:B - 1], 3), process(x[B - 1:B], 3), stats(False)]
        steps += [H.refused(H.s_set_weights(wrong_w)), H.refused(H.s_reset(1 << 63)), process(x[B:2 * B + 1], 3), stats(False)]
    return steps, xs, lengths


def _first_calls(cpp, k, count, M, P=None):
    """y, R [nb, M, M] and w [nb, M] or [nb, P, M] of format k's first `count` calls behind each other, as the models take them"""
    ys, Rs, ws = ([r for r in H.get(cpp, t, np.complex64)] for t in ("y", "R", "w"))
    ys, Rs, ws = (v[k * (len(v) // 2):k * (len(v) // 2) + count] for v in (ys, Rs, ws))
    R = np.concatenate(Rs).reshape(-1, M, M)
    w = np.concatenate(ws).reshape((-1, M) if P is None else (-1, P, M))
    if P is None:
        return np.concatenate(ys), R, w
    return np.concatenate([y.reshape(P, -1) for y in ys], axis=1), R, w


@pytest.mark.parametrize("A", [2, 8])
def test_nuller(gpu, hipbuf, exe, tmp_path, A):
    import nuller_model as NM
    import test_gpu_nuller as TN
    from gnss_sdr_rs_amd import nuller
    s = None if A == 2 else _rand(A, 3)
    held = H._Held()
    steps, xs, lengths = _array_steps(A, _rand(A, 4), _rand(A + 1, 5), lambda c, want: H.s_array_process(c, want),
                                      lambda c, n: H.s_array_process_dev(c, n + B + 5), lambda plain: H.s_stats(("inputs", "outputs", "blocks")),
                                      lambda x: [], held)
    head = H.pk("IIf", A, B, 1e-2) + H.words(np.complex64, [] if s is None else s)
    cpp = _both(exe, tmp_path, hipbuf, "nuller", head, steps, lambda: nuller.Nuller(A, B, 1e-2, s),
                lambda o: [H.u32("block", o.block), H.u32("antennas", o.n_antennas)])
    p = NM.resolve(A, B, 1e-2, s)
    for k, fmt in enumerate((C32, I8_IQ)):
        TN._check(("nuller", A, fmt), p, xs[fmt], *_first_calls(cpp, k, len(lengths), A))


def _taps_for(A):
    return (1, min(8, 32 // A))                 # taps are 1 .. 8 with A L <= 32


@pytest.mark.parametrize("A,L", [(2, 1), (2, 8), (8, 1), (8, 4)])
def test_stap(gpu, hipbuf, exe, tmp_path, A, L):
    import stap_model as SM
    import test_gpu_stap as TS
    from gnss_sdr_rs_amd import stap
    assert L in _taps_for(A)
    M = A * L
    s = None if L == 1 else _rand(M, 3)
    held = H._Held()
    steps, xs, lengths = _array_steps(A, _rand(M, 4), _rand(M + 1, 5), lambda c, want: H.s_array_process(c, want),
                                      lambda c, n: H.s_array_process_dev(c, n + B + 5), lambda plain: H.s_stap_stats(plain), lambda x: [], held)
    head = H.pk("IIIf", A, L, B, 1e-2) + H.words(np.complex64, [] if s is None else s)
    cpp = _both(exe, tmp_path, hipbuf, "stap", head, steps, lambda: stap.Stap(A, L, B, 1e-2, s),
                lambda o: [H.u32("block", o.block), H.u32("weights", o.n_weights), H.u32("antennas", o.n_antennas), H.u32("taps", o.taps)])
    p = SM.resolve(A, L, B, 1e-2, s)
    for k, fmt in enumerate((C32, I8_IQ)):
        TS._check(("stap", A, L, fmt), p, xs[fmt], *_first_calls(cpp, k, len(lengths), M))


@pytest.mark.parametrize("A,L,P", [(2, 1, 1), (2, 8, 3), (8, 4, 16), (8, 1, 3)])
def test_beamformer(gpu, hipbuf, exe, tmp_path, A, L, P):
    import beam_model as BM
    import test_gpu_beam as TB
    import test_gpu_stap as TS
    from gnss_sdr_rs_amd import beamformer
    M = A * L
    rows = TB._rows(P, M, 7 * M + P)
    held = H._Held()
    new_row = _rand(M, 8)
    extra = lambda x: [H.s_set_steering(P - 1, new_row), H.s_array_process(x, 7), H.refused(H.s_set_steering(0, new_row[:-1])),
                       H.refused(H.s_set_steering(P, new_row)), H.s_set_steering(P - 1, rows[P - 1])]
    steps, xs, lengths = _array_steps(A, _rand(P * M, 4), _rand(P * M + 1, 5), lambda c, want: H.s_array_process(c, want | 4 if want else 0),
                                      lambda c, n: H.s_beams_process_dev(c, n + B + 5), lambda plain: H.s_beams_stats(plain), extra, held)
    head = H.pk("IIIf", A, L, B, 1e-2) + H.words(np.complex64, rows)
    cpp = _both(exe, tmp_path, hipbuf, "beamformer", head, steps, lambda: beamformer.Beamformer(A, L, rows, B, 1e-2),
                lambda o: [H.u32("block", o.block), H.u32("weights", o.n_weights), H.u32("beams", o.n_beams)])
    p = BM.resolve(A, L, rows, B, 1e-2)
    for k, fmt in enumerate((C32, I8_IQ)):
        y, R, w = _first_calls(cpp, k, len(lengths), M, P)
        for beam in range(P):
            TS._check(("beamformer", A, L, P, fmt, beam), p["beams"][beam], xs[fmt], y[beam], R, w[:, beam])


def _constraints(M, qs, seed):
    out = []
    for k, Q in enumerate(qs):
        f = _rand(Q, seed + 100 + k)
        f[0] = 1.0
        out.append((_rand((Q, M), seed + k), f))
    return out


@pytest.mark.parametrize("A,L,qs", [(2, 1, [1]), (8, 4, [1, 2, 8]), (8, 1, [1] * 16), (2, 8, [8, 2, 1])])
def test_lcmv(gpu, hipbuf, exe, tmp_path, A, L, qs):
    import lcmv_model as LM
    import test_gpu_lcmv as TL
    from gnss_sdr_rs_amd import lcmv
    M, P = A * L, len(qs)
    cs = _constraints(M, qs, 11 * M + P)
    held = H._Held()
    q_new = 2 if qs[0] == 1 and sum(qs) < 16 and M >= 2 else 1          # beam 0's count changes where the 16 rows allow it
    rows_new, f_new = _constraints(M, [q_new], 77)[0]
    extra = lambda x: [H.s_set_constraints(0, rows_new, f_new), H.s_array_process(x, 7),
                       H.refused(H.s_set_constraints(0, rows_new.reshape(-1)[:-1], f_new)), H.refused(H.s_set_constraints(P, rows_new, f_new)),
                       H.s_set_constraints(0, *cs[0])]
    steps, xs, lengths = _array_steps(A, _rand(P * M, 4), _rand(P * M + 1, 5), lambda c, want: H.s_array_process(c, want | 4 if want else 0),
                                      lambda c, n: H.s_beams_process_dev(c, n + B + 5), lambda plain: H.s_beams_stats(plain), extra, held)
    head = H.pk("IIIfI", A, L, B, 1e-2, P) + b"".join(H.words(np.complex64, r) + H.words(np.complex64, f) for r, f in cs)
    cpp = _both(exe, tmp_path, hipbuf, "lcmv", head, steps, lambda: lcmv.Lcmv(A, L, cs, block=B, loading=1e-2),
                lambda o: [H.u32("block", o.block), H.u32("weights", o.n_weights), H.u32("beams", o.n_beams)])
    p = LM.resolve(A, L, cs, B, 1e-2)
    for k, fmt in enumerate((C32, I8_IQ)):
        y, R, w = _first_calls(cpp, k, len(lengths), M, P)
        TL._check(("lcmv", A, L, qs, fmt), p, xs[fmt], y, R, w)


# ---------------------------------------------------------------------------------------------------------------- the ring writers
@pytest.mark.parametrize("source,fmt,with_excisor,with_resampler",
                         [("ddc", H.I8_REAL, False, False), ("ddc", H.I8_REAL, True, True), ("ddc", H.I8_REAL, True, False), ("ddc", H.I8_REAL, False, True),
                          ("frontend", C32, False, True), ("frontend", I8_IQ, False, True), ("frontend", C32, True, False),
                          ("frontend", I8_IQ, True, True), ("frontend", C32, True, True), ("frontend", I8_IQ, True, False)])
def test_the_ring_writers(gpu, hipbuf, exe, tmp_path, source, fmt, with_excisor, with_resampler):
    """Ddc::write_ring and the resampled and conditioned DigitalFrontend::write_ring / write_ring_i8 over one wrap of a 2^12 ring: the
    returned totals, the enqueued and published heads, the ring's words and the stages' counters"""
    import ddc_model as DM
    import test_gpu_ddc as TD
    from gnss_sdr_rs_amd import ddc, excise, frontend, resample, tracking
    ring_size = 1 << 12
    calls = [20, 3000, 6000, 4096, 17, 4091, 1234] if source == "ddc" else [20, 1500, 3000, 2048, 17, 2043]
    if source == "ddc":
        x = TD._stream(sum(calls), 23)
    else:
        x = _stream(fmt, sum(calls), 29)
    gains = np.ones(B, np.float32)
    gains[40:44] = 0.0
    steps, at = [], 0
    for n in calls:
        steps += [H.s_write_ring(fmt, x[at:at + n])]
        at += n
    # the words are read back from what the Python ring says it holds: the last ring_size words at the most
    head = H.pk("QI", ring_size, 0 if source == "ddc" else 1)
    head += H.pk("dIIf", DM.MIX, 1, 2, 120.0) if source == "ddc" else H.pk("fff", 4.092e6, 16.368e6, 16.368e6)
    head += (H.pk("I", B) + H.raw(gains)) if with_excisor else H.pk("I", 0)
    head += H.pk("II", 2, 3) if with_resampler else H.pk("II", 0, 0)

    def make():
        ex = excise.Excisor(B) if with_excisor else None
        if ex is not None:
            ex.set_gains(gains)
        src = ddc.Ddc(DM.MIX, 1, 2, blank_threshold=120.0) if source == "ddc" else frontend.DigitalFrontend(4.092e6, 16.368e6, 16.368e6)
        return tracking.MulticastRingBuffer(ring_size), src, ex, resample.Resampler(2, 3) if with_resampler else None

    # how many outputs the calls enqueue is what the stages say; the read step asks for the last words the ring still holds
    probe = make()
    try:
        total = sum(probe[1].write_ring(probe[0], x[a:a + n], excisor=probe[2], resampler=probe[3]) or 0
                    for a, n in zip(np.cumsum([0] + calls[:-1]), calls))
    finally:
        for h in probe:
            if h is not None:
                h.close()
    assert total > ring_size                                               # the ring wrapped
    steps += [H.s_ring_read(total - ring_size + 7, ring_size - 7), H.s_ring_stats(source == "ddc")]
    _both(exe, tmp_path, hipbuf, "ring", head, steps, make)


# ---------------------------------------------------------------------------------------------------------------- FFT, RealFFT
@pytest.mark.parametrize("n", [8, 1024, 127])
def test_fft(gpu, exe, tmp_path, n):
    """FFT::execute on a batch of 3 (returned copy and the words left in place), power_spectrum and RealFFT::execute at an in-LDS length
    and two Bluestein lengths of tests/fft_model.py"""
    import fft_model as FM
    from gnss_sdr_rs_amd import fft
    x, one = FM.noise(n, 41, 3), FM.mixture(n, 42)
    real = np.random.default_rng([43, n]).standard_normal(n).astype(np.float32)
    cpp = H.run_driver(exe, "fft", H.pk("QI", n, 3) + H.raw(x) + H.raw(one[0]) + H.raw(real), tmp_path)
    words = fft.FFT(n).execute(x.copy().reshape(-1))
    buf = one[0].copy()
    H.same(cpp, [H.rec("execute", words), H.rec("execute.in_place", words), H.rec("power_spectrum", fft.FFT(n).power_spectrum(buf)),
                 H.rec("rfft", fft.RealFFT(n).execute(real))], "fft")
    got = H.get(cpp, "execute", np.complex64, 0).reshape(3, n)
    ref = FM.reference(x)
    l2 = FM.l2_rel(got, ref).max()
    if FM.path(n) == "bluestein":
        assert FM.bluestein_L(n) in FM.POW2_PLANS and l2 < 3e-6, (n, l2)          # test_bluestein_length_classes' bar
    else:
        eob = FM.err_over_bound(got, ref, FM.B(n), x).max()
        assert eob <= 1.0 and l2 < 1e-6, (n, eob, l2)                              # test_every_lds_plan_per_bin's bars
    print("fft %d (%s): relative L2 error %.3e" % (n, FM.path(n), l2))


# ---------------------------------------------------------------------------------------------------------------- re-steering on the device
def test_resteer(gpu, hipbuf, exe, tmp_path):
    """solve_plan, solve_rows_dev with R empty and with R captured from a Stap of the same run, Beamformer::set_steering_dev with every
    default, with the flags, and with d_info under a min_ratio that rejects one row; the beams' words behind each install.  The rows are
    held to tests/array_probe_model.py at test_array_probe_host.py's ROW_BAR."""
    import array_probe_model as PM
    import test_gpu_array_resteer as TR
    import test_gpu_beam as TB
    import test_gpu_stap as TS
    from test_array_probe_host import ROW_BAR
    from gnss_sdr_rs_amd import acquisition as AQ, beamformer, stap
    A, L, P, n, loading = 4, 2, 3, 12, 1e-3
    M, n_time = A * L, 4 * B + 2
    half = n_time // 2
    steering = TB._rows(P, M, 5)
    z, _ = TR._inputs(M, n, 0, P, 9)
    z[1] = (0.15 * z[1] + _rand((n, M), 10)).astype(np.complex64)          # a poorer estimate: the row the gate rejects
    x = TS._stream("c32", n_time, A, 77)
    ratios = sorted(i["lambda1"] / i["lambda2"] for i in (AQ.solve_row(z[p], None, loading)[1] for p in range(P)))
    assert ratios[1] > 2.0 * ratios[0]
    min_ratio = float(np.sqrt(ratios[0] * ratios[1]))
    body = H.pk("IIIIff", A, L, B, n, loading, min_ratio) + H.words(np.complex64, steering) + H.pk("Q", z.size) + H.raw(z) + H.pk("Q", x.size) + H.raw(x)
    cpp = H.run_driver(exe, "resteer", body, tmp_path)

    img = lambda p, nbytes: H.rec("", hipbuf.download(p, nbytes, np.uint8))[1]
    fill = lambda nbytes: hipbuf.alloc(nbytes, fill=H.GUARD_FILL)
    py = []
    d_x, d_z = hipbuf.upload(x), hipbuf.upload(z)
    d_R, d_w, d_y = fill(2 * M * M * 8), fill(2 * M * 8), fill((n_time + B) * 8)
    st = stap.Stap(A, L, B)
    st.capture(d_R, d_w, 2)
    py.append(H.u64("stap.got", st.process_dev(d_x, C32, half, d_y, half + B)))
    st.synchronize()
    st.capture(None, None, 0)
    st.close()
    py += [("R", img(d_R, 2 * M * M * 8)), H.u32("R.guards", 1)]
    rows0, info0, rows1, info1 = fill(P * M * 8), fill(P * 24), fill(P * M * 8), fill(P * 24)
    e, e2 = AQ.solve_plan(M, n, P, 0, loading=loading), AQ.solve_plan(M, n, P, 2, loading=loading)
    AQ.solve_rows_dev(M, n, P, d_z, rows0, info0, loading=loading)
    py.append(H.u64("extents", *[d[k] for d in (e, e2) for k in ("z_words", "R_words", "row_words")]))
    AQ.solve_rows_dev(M, n, P, d_z, rows1, info1, d_R=d_R, n_blocks=2, loading=loading)
    for tag, p, nbytes in (("rows0", rows0, P * M * 8), ("info0", info0, P * 24), ("rows1", rows1, P * M * 8), ("info1", info1, P * 24)):
        py += [(tag, img(p, nbytes)), H.u32(tag + ".guards", 1)]
    bf = beamformer.Beamformer(A, L, steering, B)

    def run(tag):
        y, R, w = bf.process(x[half:], want_blocks=True)
        bf.reset(0)
        return [H.rec(tag + ".y", y), H.u64(tag + ".n_out", y.shape[1]), H.rec(tag + ".w", w)]
    py += run("before")
    installed, gated = fill(P), fill(P)
    bf.set_steering_dev(0, P, rows1)
    py += run("plain")
    bf.set_steering_dev(0, P, rows1, None, 0.0, installed)
    bf.synchronize()
    py += [("installed", img(installed, P)), H.u32("installed.guards", 1)]
    bf.set_steering_dev(0, P, rows0, info0, min_ratio, gated)
    bf.synchronize()
    py += [("gated", img(gated, P)), H.u32("gated.guards", 1)]
    py += run("gated") + [H.u32("in.guards", 1)]
    bf.close()
    H.same(cpp, py, "resteer")
    # what the C++ run itself says: every row installed without the gate, one rejected under it, and the beams changed each time
    assert H.get(cpp, "installed", np.uint8, 0).tolist() == [1] * P and sorted(H.get(cpp, "gated", np.uint8, 0).tolist()) == [0] + [1] * (P - 1)
    ys = [H.get(cpp, t + ".y", np.complex64, 0) for t in ("before", "plain", "gated")]
    assert ys[0].size == P * 2 * B and (ys[0] != ys[1]).any() and (ys[1] != ys[2]).any()
    R = H.get(cpp, "R", np.complex64, 0).reshape(2, M, M)
    rows, info = H.get(cpp, "rows1", np.complex64, 0).reshape(P, M), H.get(cpp, "info1", np.uint8, 0).view(TR.INFO)
    held = 0
    for p in range(P):
        assert info["status"][p] == 0
        want, winfo = PM.solve_row(z[p], R, loading, ref_index=int(info["ref_index"][p]))
        if winfo["lambda1"] < 2.0 * winfo["lambda2"]:                      # the bar is stated for a separated eigenvalue (test_array_probe_host)
            continue
        held += 1
        err = float(np.abs(rows[p].astype(np.complex128) - want).max())
        print("resteer row %d: largest word difference %.2e (bar %.0e)" % (p, err, ROW_BAR))
        assert err <= ROW_BAR, (p, err)
    assert held >= 2


# ---------------------------------------------------------------------------------------------------------------- AcquisitionEngine
FS, N = 2.048e6, 2048            # the smallest fft_size the C++ constructors reach at the C/A code (they take no custom code table;
DOP = np.array([-500.0, 0.0, 500.0], np.float32)      # test_gpu_array_probe and the i8 cells of the refine tests run at it too)
PRNS = [5, 6]                    # PRN 5 is in the scene, PRN 6 is not: its optional stays empty


def _acq_head(M, K, from_tables):
    return H.pk("ffI", FS, 0.0, N) + H.words(np.float32, DOP) + H.words(np.uint8, PRNS) + H.pk("IfII", M, 7.0, K, from_tables)


def _acq_scene(oracle, n, config_id):
    from gnss_sdr_rs_amd import synth
    sats = [dict(prn_row=4, cn0_dbhz=52.0, doppler_hz=40.0, code_start=777)]
    return synth.make_scene(oracle.ca_code_table(), FS, 0.0, n, sats, config_id=config_id)


def _res_words(results):
    out = b""
    for r in results:
        out += H.pk("QQffffQiI", r["prn"], r["code_phase_samples"], r["code_phase_chips"], r["carrier_freq"], r["fs"], r["mag_relative"],
                    r["sample_global_index"], r["doppler_bin"], 1) if r else bytes(48)
    return "results", out


def a_search(x):
    fmt = I8_IQ if x.dtype == np.int8 else C32

    def f(o, hb):
        o.last = o.search(x)
        return [_res_words(o.last)]
    return H.pk("IIQQQ", 1, fmt, x.shape[0], 0, 2 ** 64 - 1) + H.raw(x), f


def a_refine(drop=0xFFFFFFFF, span=0, n_freq=0, half_span=0.0):
    from gnss_sdr_rs_amd import _lib

    def f(o, hb):
        r = [None if i == drop else v for i, v in enumerate(o.last)]
        got = o.refine_doppler(r, span, n_freq, half_span)
        return [H.rec("refine.found", [g is not None for g in got], np.uint8), ("refine", b"".join(bytes(_lib.AcqRefineOut(**g)) for g in got if g))]
    return H.pk("IIIfI", 3, span, n_freq, half_span, drop), f


def _cands(cands):
    return H.pk("I", len(cands)) + b"".join(H.pk("IiII", c["worker"], c["doppler_bin"], c["code_phase_samples"], c.get("offset_periods", 0)) for c in cands)


def _dwell(x, fmt, on_device):
    return H.pk("IIQ", int(on_device), fmt, x.shape[0] if on_device else 0) + (H.raw(x) if on_device else b"")


def a_local(cands, x=None, lag_half_window=2):
    from gnss_sdr_rs_amd import _lib
    fmt = C32 if x is None or x.dtype != np.int8 else I8_IQ

    def f(o, hb):
        got = o.local_search(cands, hb.upload(x) if x is not None else None, lag_half_window, fmt=fmt)
        return [("local", b"".join(bytes(_lib.AcqLocalOut(**g))[:84] for g in got)), H.u32("in.guards", 1)]
    return H.pk("I", 4) + _cands(cands) + H.pk("IIIf", lag_half_window, 0, 0, 0.0) + _dwell(x if x is not None else np.zeros(0), fmt, x is not None), f


def a_array(cands, xa, L):
    """xa: [dwell, A] complex64 or [dwell, A, 2] int8 on the device"""
    fmt = I8_IQ if xa.dtype == np.int8 else C32

    def f(o, hb):
        o.z = o.array_prompts(cands, hb.upload(xa), xa.shape[1], L, fmt)
        return [H.rec("z", o.z), H.u32("periods", o.K * o.M), H.u32("in.guards", 1)]
    return H.pk("I", 5) + _cands(cands) + H.pk("II", xa.shape[1], L) + _dwell(xa, fmt, True), f


def a_cancel(cands, dwell, x=None):
    from gnss_sdr_rs_amd import _lib
    fmt = C32 if x is None or x.dtype != np.int8 else I8_IQ

    def f(o, hb):
        assert o.dwell_samples == dwell
        d_out = hb.alloc(dwell * 8, fill=H.GUARD_FILL)
        got = o.cancel(cands, d_out, hb.upload(x) if x is not None else None, fmt)
        return [("cancel", b"".join(bytes(_lib.AcqCancelOut(**g))[:28] for g in got)), H.rec("cancel.out", hb.download(d_out, dwell * 8, np.uint8)),
                H.u32("cancel.out.guards", 1), H.u32("in.guards", 1)]
    body = H.pk("II", 6, len(cands)) + b"".join(H.pk("IIddd", c["worker"], 0, c["carrier_hz"], c["code_phase"], c.get("period_samples", 0.0)) for c in cands)
    return body + _dwell(x if x is not None else np.zeros(0), fmt, x is not None), f


def a_set_edge(offsets, secondary=None):
    return (H.pk("I", 7) + H.words(np.uint32, offsets) + H.words(np.int8, [] if secondary is None else secondary),
            lambda o, hb: (o.set_edge_search(offsets, secondary), [])[1])


def a_set_drift(periods):
    return H.pk("I", 8) + H.words(np.float64, periods), lambda o, hb: (o.set_code_drift(periods if len(periods) else None), [])[1]


def a_dwell():
    return H.pk("I", 9), lambda o, hb: [H.u64("dwell_samples", o.dwell_samples)]


def a_edge_offsets():
    return H.pk("I", 10), lambda o, hb: [H.rec("edge_offset_periods", [r["edge_offset_periods"] if r else 0 for r in o.last], np.uint32)]


def a_solve(loading):
    """the last array_prompts words, as they came out, through solve_row per candidate and through solve_rows_dev"""
    from gnss_sdr_rs_amd import acquisition as AQ

    def f(o, hb):
        out = []
        n_c, R_u, L, A = o.z.shape
        for c in range(n_c):
            row, info = AQ.solve_row(o.z[c], None, loading)
            out += [H.rec("row", row), H.rec("lambda", np.array([info["lambda1"], info["lambda2"]])), H.u32("ref_index", info["ref_index"])]
        rows, info = hb.alloc(n_c * L * A * 8, fill=H.GUARD_FILL), hb.alloc(n_c * 24, fill=H.GUARD_FILL)
        AQ.solve_rows_dev(L * A, R_u, n_c, hb.upload(o.z), rows, info, loading=loading)
        return out + [H.rec("rows", hb.download(rows, n_c * L * A * 8, np.uint8)), H.u32("rows.guards", 1),
                      H.rec("info", hb.download(info, n_c * 24, np.uint8)), H.u32("info.guards", 1), H.u32("in.guards", 1)]
    return H.pk("If", 11, loading), f


def _array_of(x, A, fmt, seed):
    """the scene on A antennas: a steering phase per antenna, and a little noise of each antenna's own"""
    rng = np.random.default_rng(seed)
    xa = x[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :] + 2.0 * (rng.standard_normal((x.size, A)) + 1j * rng.standard_normal((x.size, A)))
    if fmt == C32:
        return xa.astype(np.complex64)
    return np.stack([np.clip(np.rint(xa.real), -128, 127), np.clip(np.rint(xa.imag), -128, 127)], axis=-1).astype(np.int8)


def test_acquisition_from_caller_built_tables(gpu, oracle, hipbuf, exe, tmp_path):
    """the caller-built-tables constructor with everything but search alone: search_i8 against search, refine_doppler
    with one worker not found and with none found, local_search and cancel on the snapshot and on a device dwell, array_prompts with
    no candidate and with three, and the rows solved from its words.  The search's words go against the oracle's workers at smoke()'s bar."""
    from gnss_sdr_rs_amd import acquisition as AQ, synth
    M, A, L = 2, 4, 2
    xc = _acq_scene(oracle, M * N, 99)
    x, xi = synth.to_c32(xc), synth.to_i8_iq(xc)
    tables = lambda: [AQ.DopplerShiftTable(0.0, float(d), FS, N) for d in DOP]
    probe = AQ.AcquisitionEngine(FS, 0.0, N, prn_ids=PRNS, n_integrations=M, tables=tables(), any_length=True)
    found = probe.search(x)
    assert found[0] is not None and found[1] is None and probe.dwell_samples == M * N
    cand = dict(worker=0, doppler_bin=found[0]["doppler_bin"], code_phase_samples=found[0]["code_phase_samples"], offset_periods=0)
    three = [cand, dict(cand, worker=1), dict(cand, doppler_bin=0, code_phase_samples=5)]
    loc = probe.local_search([cand], lag_half_window=2)
    kill = probe.cancel_cands_from_local(loc, [0])
    probe.close()
    steps = [a_search(xi), a_search(x), a_refine(), a_refine(drop=0), a_refine(n_freq=33, half_span=200.0), a_local([cand]), a_local(three, x),
             a_local([]), a_local(three, xi), a_cancel(kill, M * N), a_cancel(kill, M * N, x), a_cancel(kill, M * N, xi), a_dwell()]
    for fmt in (C32, I8_IQ):
        xa = _array_of(xc, A, fmt, 5)
        steps += [a_array([], xa, L), a_array(three, xa, L), a_solve(1e-3)]
    cpp = _both(exe, tmp_path, hipbuf, "acquisition", _acq_head(M, 1, 1), steps,
                lambda: AQ.AcquisitionEngine(FS, 0.0, N, prn_ids=PRNS, n_integrations=M, tables=tables(), any_length=True))
    res = [np.frombuffer(b, np.uint8) for t, b in cpp if t == "results"]
    assert (res[0] == res[1]).all()                                        # search_i8 against search: the scene's words are integers
    tabs = [oracle.DopplerShiftTable(0.0, float(d), FS, N) for d in DOP]
    exp = [oracle.AcquisitionWorker(p, N, FS).search_satellite(x, tabs, 0, M) for p in PRNS]
    prn, cps, _, _, _, mag, _, dbin, ok = __import__("struct").unpack("<QQffffQiI", res[1][:48].tobytes())
    assert exp[1] is None and not res[1][48:].any() and ok == 1
    assert (prn, cps, dbin) == (exp[0]["prn"], exp[0]["code_phase_samples"], exp[0]["doppler_bin"])
    assert abs(mag - exp[0]["mag_relative"]) <= 1e-5 * exp[0]["mag_relative"]
    zs = H.get(cpp, "z", np.complex64)
    assert zs[0].size == 0 and zs[1].size == 3 * M * L * A


def test_acquisition_coherent_edges_and_drift(gpu, oracle, hipbuf, exe, tmp_path):
    """coherent_periods = 2 with set_edge_search({0, 1}, secondary) and set_code_drift per bin: dwell_samples() after each, then a search,
    edge_offset_periods, refine_doppler and local_search on that handle, and the setters switched off again"""
    from gnss_sdr_rs_amd import acquisition as AQ, synth
    M, K = 2, 2
    drift = [N + 0.004 * k for k in range(len(DOP))]
    make = lambda: AQ.AcquisitionEngine(FS, 0.0, N, doppler_hz=DOP, prn_ids=PRNS, n_integrations=M, any_length=True, coherent_periods=K)
    probe = make()
    probe.set_edge_search([0, 1], [1, 1])
    probe.set_code_drift(drift)
    dwell = probe.dwell_samples
    assert dwell > (K * M + 1) * N - 8
    x = synth.to_c32(_acq_scene(oracle, dwell, 98))
    found = probe.search(x)
    probe.close()
    assert found[0] is not None and found[1] is None
    cand = dict(worker=0, doppler_bin=found[0]["doppler_bin"], code_phase_samples=found[0]["code_phase_samples"],
                offset_periods=found[0]["edge_offset_periods"])
    # (the scene carries no secondary code: the row (1, -1) is set and its dwell read, the search runs under (1, 1))
    steps = [a_dwell(), a_set_edge([0, 1], [1, -1]), a_dwell(), a_set_edge([0, 1], [1, 1]), a_set_drift(drift), a_dwell(), a_search(x), a_edge_offsets(),
             a_refine(), a_refine(drop=0), a_local([cand]), a_local([cand], x), H.refused(a_set_edge([1, 0])), a_dwell(), a_set_drift([]), a_dwell(),
             a_set_edge([]), a_dwell()]
    cpp = _both(exe, tmp_path, hipbuf, "acquisition", _acq_head(M, K, 0), steps, make)
    dw = [int(v[0]) for v in H.get(cpp, "dwell_samples", np.uint64)]
    assert dw[0] == K * M * N and dw[1] == (K * M + 1) * N and dw[2] == dwell and dw[3] == dwell and dw[4] == dw[1] and dw[5] == dw[0]


# ---------------------------------------------------------------------------------------------------------------- TrackingManager
def t_start(ch, r):
    return (H.pk("IIQQffffQiI", 1, ch, r["prn"], r["code_phase_samples"], r["code_phase_chips"], r["carrier_freq"], r["fs"], r["mag_relative"],
                 r["sample_global_index"], r["doppler_bin"], 1), lambda o, hb: (o[0].channels[ch].start(r), [])[1])


def _recs(recs):
    return H.pk("II", int(recs is not None), len(recs or [])) + b"".join(bytes(r) for r in recs or [])


def t_bank(taps, offs, recs, want_done):
    def f(o, hb):
        out, done = o[0].bank(o[1], taps, offs if len(offs) else None, states=recs)
        return [H.rec("bank", out)] + ([H.rec("done", done)] if want_done else [])
    return H.pk("I", 2) + H.words(np.float32, taps) + H.words(np.float32, offs) + _recs(recs) + H.pk("I", int(want_done)), f


def t_array(xd, fmt, first, n_time, L, tau, recs, want_done, dev=False):
    A = xd.shape[1]

    def f(o, hb):
        d_x = hb.upload(xd)
        if dev:
            d_z, d_done = hb.alloc(len(recs) * L * A * 8, fill=H.GUARD_FILL), hb.alloc(len(recs), fill=H.GUARD_FILL)
            o[0].array_prompts_dev(d_x, n_time, A, recs, d_z, d_done, L, first, tau, fmt)
            o[0].synchronize()
            return [H.rec("z.dev", hb.download(d_z, len(recs) * L * A * 8, np.uint8)), H.u32("z.dev.guards", 1),
                    H.rec("done.dev", hb.download(d_done, len(recs), np.uint8)), H.u32("done.dev.guards", 1), H.u32("in.guards", 1)]
        z, done = o[0].array_prompts(d_x, n_time, A, L, recs, first, tau, fmt)
        return [H.rec("z", z)] + ([H.rec("done", done)] if want_done else []) + [H.u32("in.guards", 1)]
    return H.pk("IQQIf", 4 if dev else 3, first, n_time, L, tau) + _recs(recs) + H.pk("I", int(want_done)), f


@pytest.mark.parametrize("fmt", [C32, I8_IQ])
def test_tracking_bank_and_array_prompts(gpu, oracle, hipbuf, exe, tmp_path, fmt):
    """TrackingManager::bank and ::array_prompts on the handle's own channels (one started, one idle: its flag is 0 and its words are
    zeros) and on a record vector holding one skipped record, with and without the done vector and the offsets; array_prompts_dev into
    guarded device buffers.  The words of the records that run go against trk_bank_model and trk_array_model at the existing tests' bars."""
    import ctypes
    import stap_model as SM
    import test_gpu_stap as TS
    import test_gpu_trk_array as TA
    import test_gpu_trk_bank as TBk
    import trk_array_model as AM
    from gnss_sdr_rs_amd import _lib, synth, tracking as T
    assert ctypes.sizeof(_lib.TrkState) == 64
    n, A, L, mode = N, 4, 2, T.CODE_INDEX_FIXED
    table = oracle.ca_code_table()
    prns = [3, 9, 17, 25]
    sc = synth.tracking_scene(table, FS, 0.0, prns, 4, config_id=71, cn0=50.0, code_rows=[p - 1 for p in prns])
    x = synth.to_c32(sc["x"])
    recs = [TBk._record(T, s["prn"], s["code_start"], n, s["doppler_hz"] + 7.0 * k, code_phase=0.125 * (k % 3)) for k, s in enumerate(sc["sats"])]
    rows = [table[p - 1] for p in prns]
    idle = TBk._record(T, 7, recs[0].next_sample_index, n, 0.0, active=0)
    with_idle = recs[:2] + [idle] + recs[2:]
    taps, offs = TBk.TAP_SETS[3], TBk.OFF_SETS[3]
    n_time = 2 * n + 777
    xd = TS._stream("i8" if fmt == I8_IQ else "c32", n_time, A, 100 * A + L)
    arecs = TA._records(T, n, L, n_time, 6, n + A + L)
    a_idle = TA._record(T, 7, 5, 0.0, active=0)
    a_with_idle = arecs[:3] + [a_idle] + arecs[3:]
    s0 = sc["sats"][0]
    r0 = dict(prn=s0["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=float(s0["doppler_hz"]), fs=FS, mag_relative=1.0,
              sample_global_index=int(s0["code_start"]), doppler_bin=0)
    steps = [t_start(0, r0), t_bank(taps, offs, None, True), t_bank(taps, [], None, False), t_bank(taps, offs, with_idle, True),
             t_bank(taps, [], with_idle, False), t_bank(taps, offs, recs, True),
             t_array(xd, fmt, 0, n_time, L, 0.0, None, True), t_array(xd, fmt, 0, n_time, L, 0.0, a_with_idle, True),
             t_array(xd, fmt, 0, n_time, L, 0.5, a_with_idle, False), t_array(xd, fmt, 0, n_time, L, 0.0, arecs, True),
             t_array(xd, fmt, 0, n_time, L, 0.0, a_with_idle, False, dev=True)]
    head = H.pk("fIIQQ", FS, 2, mode, 1 << 16, x.size) + H.raw(x) + H.pk("IQI", fmt, n_time, A) + H.raw(xd)

    def make():
        ring = T.MulticastRingBuffer(1 << 16)
        ring.write_samples(x)
        return T.TrackingManager(FS, n_channels=2, code_index_mode=mode), ring
    cpp = _both(exe, tmp_path, hipbuf, "tracking", head, steps, make)
    banks, dones, zs = H.get(cpp, "bank", np.complex64), H.get(cpp, "done", np.uint8), H.get(cpp, "z", np.complex64)
    assert dones[0].tolist() == [1, 0] and not banks[0].reshape(2, -1)[1].any()                   # the idle channel
    assert dones[1].tolist() == [1, 1, 0, 1, 1] and not banks[2].reshape(5, -1)[2].any()          # the skipped record
    assert not banks[3].reshape(5, -1)[2].any() and banks[3].size == 5 * len(taps)
    print("bank: largest fraction of the envelope %.2e (bar %.0e)"
          % (TBk._worst(banks[4].reshape(4, len(offs), len(taps)), dones[2], recs, x, FS, rows, taps, offs, mode), TBk.REL))
    assert dones[4].tolist() == [1, 1, 1, 0, 1, 1, 1] and not zs[1].reshape(7, -1)[3].any() and not zs[2].reshape(7, -1)[3].any()
    worst = TA._worst(zs[3].reshape(6, L, A), dones[5], arecs, SM.as_c128(xd), FS, TA._rows(table, arecs, AM.FIXED), L, 0.0, AM.FIXED)
    print("array_prompts: largest |z - model| / envelope %.2e (bar %.0e)" % (worst, TA.REL))
    assert worst <= TA.REL
    zdev = H.get(cpp, "z.dev", np.complex64, 0)
    assert (zdev.view(np.uint32) == zs[1].view(np.uint32)).all() and H.get(cpp, "done.dev", np.uint8, 0).tolist() == dones[4].tolist()
