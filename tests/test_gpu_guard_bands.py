"""Every device entry held to its buffers: the inputs of the _dev entries carved out of poisoned guard bands (tests/guard_bands.py).

The other GPU files cut a stream's calls out of ONE device buffer, so the bytes in front of a call's pointer are the stream's true past
and the bytes behind its last sample its true future, and keep every other array in a zero-filled allocation of its own.  A kernel that
took a history word from in[-1] instead of the handle's history buffer, a halo sample from behind n_in, or a 16-byte load that starts an
element early would find the right words there, or zeros.  Here every input sits in an allocation of its own between two 64 KiB guards,
its last byte directly followed by guard, its first on an odd element (aligned to the element and to nothing larger), and every case runs
under the three fills 0x00, 0xFF (float32: NaN, int8: -1) and 0x7F (float32: 3.39e38, int8: 127).  Per case:

  * the outputs pass the owning file's own check against its float64 model (or the oracle) at that file's bar: _check and the models
    are imported, no bar is restated here;
  * the output words are the same bits under the three fills (guard_bands.same_words);
  * both guards of every input still hold the fill and the input is what was put there; behind the outputs the owning file's _feed
    finds its 0x5A filler.

Streaming and array stages (gm_resampler, gm_ddc, gm_excisor with adapt_dev and the block-adapt mode, gm_channelizer, gm_nuller, gm_stap,
gm_beamformer, gm_lcmv, all through process_dev): one configuration per kernel form of tests/stage_instantiations.py, both formats.  A
stream of about three tiles goes through a fresh handle in THREE calls whose inputs are three separately carved buffers
(guard_bands.Scattered under the owning file's _feed), so no call has the stream's past in front of it or its future behind it:

    call 1  ends one element behind a tile (block, segment) boundary;
    call 2  is shorter than the history (a few samples: it produces nothing by itself but history);
    call 3  takes the stream to one element in front of a tile boundary.

The concatenated outputs go to the model check and equal, bit for bit, the words of the owning file's _feed from one buffer in one call
on another fresh handle.  The array stages run L = 2 (a wave carries one lag) and L = 5 (two) at every A: the smallest L with a halo
(L = 1 has no history a call could take from in front of its pointer).

gm_frontend_process_dev: a plain block (table form) and the smallest block of the speculative form, carved, bit-exact with the oracle.

Acquisition (gm_acq_search_dev, gm_acq_prepare_dev + gm_acq_search_prepared_dev): a dwell of exactly dwell_samples() elements, carved, in
c32, int8 IQ and int8 real, at the smallest fft_size of each form gm_acq_plan_info reports (acq_model.CASES: 256 in LDS, 18000 composite,
6144 long, 2040 padded to 4096), {max, argmax, sum} of every cell against the float64 model of acq_model.py at its REL as
tests/test_gpu_stage_f_variants.py holds it; coherent K = 2, an edge search with two offsets and code drift at 256 and 6144; and a
handle that has searched a dwell of 0x7F bytes before.  tests/test_guard_bands_host.py holds these scenes to acq_model.GAP on the CPU.

Known cells: gm_acq_local_search, gm_acq_array_prompts, gm_acq_cancel (d_out carved at both of its alignments) and
gm_trk_array_prompts / _dev take the dwell as fresh d_samples, candidates and records reaching the buffer's last sample;
gm_array_rows_solve_dev and gm_plane_ring_write_dev run with strides above the minimum, the gaps holding the fill byte.

Rings: gm_acq_search_ring, gm_trk_update_all (persistent, strict_libm, serial), gm_trk_bank and gm_trk_update_planes on rings that held one
full lap of NaN before the scene, `head` inside a code period, against the same run on a lap of zeros and against the oracle or model."""
import numpy as np
import pytest

import guard_bands as GB
import stage_instantiations as SI

pytestmark = pytest.mark.gpu
FAKE = GB.Scattered.FAKE


def _align(fmt):
    """the element: an int8 IQ pair or a complex64 word (an antenna's sample in the array stages' rows)"""
    return 2 if fmt == "i8" else 8


def _scatter(hipbuf, x, cuts, align, bps, make, feed, **proxy):
    """the stream x in the calls `cuts`, each from a carved buffer of its own, on a fresh handle per fill -> the outputs (the same bits
    under every fill, and those of feed(handle, one buffer holding x) on another fresh handle) and the handle's counters"""
    assert sum(cuts) == len(x) and min(cuts) > 0
    bounds = np.cumsum([0] + list(cuts))
    runs, stats = {}, {}
    for fill in GB.FILLS:
        h = make()
        pieces = [GB.carve(hipbuf, x[lo:hi], fill, align=align) for lo, hi in zip(bounds, bounds[1:])]
        assert GB.disjoint(*pieces)
        s = GB.Scattered(h, pieces, list(cuts), bps, **proxy)
        runs[fill] = feed(s, FAKE)
        assert s.calls == len(cuts)
        stats[fill] = h.stats()
        assert all(GB.guards_intact(hipbuf, c) for c in pieces), hex(fill)          # guards and inputs are only read
        h.close()
    GB.same_words(runs)
    assert stats[0x00] == stats[0xFF] == stats[0x7F]
    h = make()
    GB.same_words({"carved": runs[0x00], "one buffer": feed(h, hipbuf.upload(x))})
    assert h.stats() == stats[0x00]
    h.close()
    return runs[0x00], stats[0x00]


# ---- gm_resampler, gm_ddc ---------------------------------------------------------------------------------------------------------------
def _rate_cuts(p, RM):
    """(first, short, rest): one input more than gives the first tile's last output; T / 2 - 1 inputs, less than the T - 1 of history;
    up to one input less than gives the third tile's last output"""
    T, tile = p["T"], RM.tile_outputs(p)
    n_of = lambda outputs: next(n for n in range(T // 2, 1 << 22) if RM.total_out(p, n) >= outputs)
    first, short, n = n_of(tile) + 1, T // 2 - 1, n_of(3 * tile) - 1
    assert RM.total_out(p, first - 1) >= tile > RM.total_out(p, first - 2) and RM.total_out(p, n) < 3 * tile <= RM.total_out(p, n + 1)
    assert 0 < short < T - 1 and n - first - short > tile
    return (first, short, n - first - short)


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("form", sorted(SI.RESAMPLE_CHOSEN))
def test_resampler(gpu, hipbuf, form, fmt):
    import resample_model as RM
    import test_gpu_resample as TR
    from gnss_sdr_rs_amd import resample
    config = SI.RESAMPLE_CHOSEN[form]
    assert SI.resample_form(fmt, config) == (fmt,) + form
    up, down, taps, phases = config
    p = RM.resolve(up, down, taps, phases)
    cuts = _rate_cuts(p, RM)
    n = sum(cuts)
    x = TR._stream(fmt, n, 40 + up)
    make = lambda: resample.Resampler(up, down, taps=taps, n_phases=phases)
    got, stats = _scatter(hipbuf, x, cuts, _align(fmt), TR._bps(fmt), make, lambda h, d_x: TR._feed(hipbuf, h, d_x, fmt, n))
    h = make()
    want, weight, _ = RM.run(p, h.taps(), x)
    h.close()
    worst = TR._check((config, fmt), got, want, weight, p["T"])
    assert stats == dict(inputs=n, outputs=RM.total_out(p, n), blanked=0) and got.size > 2 * RM.tile_outputs(p)
    print("guard bands, resampler %s %s: calls %s, %.3f of the bar" % (config, fmt, cuts, worst))


@pytest.mark.parametrize("form", sorted(SI.DDC_CHOSEN))
def test_ddc(gpu, hipbuf, form):
    """real int8 at any byte address: the carved buffers start on odd bytes"""
    import ddc_model as DM
    import resample_model as RM
    import test_gpu_ddc as TD
    config = SI.DDC_CHOSEN[form]
    assert SI.ddc_form(config) == form
    d0, p = TD._make(DM.MIX, config)
    g, whi, wlo = d0.tables()
    d0.close()
    cuts = _rate_cuts(p, RM)
    n = sum(cuts)
    x = TD._stream(n, 50 + config[0])
    got, stats = _scatter(hipbuf, x, cuts, 1, 1, lambda: TD._make(DM.MIX, config)[0], lambda h, d_x: TD._feed(hipbuf, h, d_x, n), signature="ddc")
    want, weight, _ = DM.run(p, g, whi, wlo, x)
    worst = TD._check((config,), got, want, weight, p["T"])
    assert stats == dict(inputs=n, outputs=RM.total_out(p, n), blanked=0) and got.size > 2 * RM.tile_outputs(p)
    print("guard bands, ddc %s: calls %s, %.3f of the bar" % (config, cuts, worst))


# ---- gm_excisor -------------------------------------------------------------------------------------------------------------------------
def _excise_cuts(B):
    """a segment is H = B / 2 inputs and the history B - H: one input behind the first segment's end, seven inputs, then up to one input
    in front of the seventh segment's end"""
    H = B // 2
    return (H + 1, 7, 6 * H - 9)


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("block", SI.BLOCKS)
def test_excisor_process(gpu, hipbuf, block, fmt):
    """excise_kernel<Plan, FMT, false>: random static gains"""
    import excise_model as EM
    import test_gpu_excise as TE
    from gnss_sdr_rs_amd import excise
    B, cuts = block, _excise_cuts(block)
    n = sum(cuts)
    assert n == 7 * (B // 2) - 1 and SI.excise_form(B, fmt, False) in SI.EXCISE_FORMS
    g = TE._gain_sets(B, 7)[1][1]
    x = TE._stream(fmt, n, 60 + B)

    def make():
        ex = excise.Excisor(B)
        ex.set_gains(g)
        return ex
    got, stats = _scatter(hipbuf, x, cuts, _align(fmt), TE._bps(fmt), make, lambda h, d_x: TE._feed(hipbuf, h, d_x, fmt, n))
    wa, ws = excise.windows(B)
    want, scale, _ = EM.run(EM.resolve(B), x, wa, ws, g)
    worst = TE._check((B, fmt), got, want, scale)
    assert stats == dict(inputs=n, outputs=EM.total_out(B, n), blanked=0) and got.size == 5 * (B // 2)
    print("guard bands, excisor B = %d %s: calls %s, %.3f of the bar" % (B, fmt, cuts, worst))


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("block", SI.BLOCKS)
def test_excisor_block_adapt(gpu, hipbuf, block, fmt):
    """excise_kernel<Plan, FMT, true> on test_gpu_excise_block.py's moving CW.  The masks the model needs are the device's own: they are
    captured by the one-call run of _one_case (which holds that run to the model), and the carved runs' words, equal to that run's
    bit for bit, go against the model handed those masks."""
    import excise_block_model as BM
    import excise_model as EM
    import test_gpu_excise_block as TX
    from gnss_sdr_rs_amd import excise
    B, cuts = block, _excise_cuts(block)
    n = sum(cuts)
    assert SI.excise_form(B, fmt, True) in SI.EXCISE_FORMS
    x = TX._moving(fmt, n, B, 3 + B)
    make = lambda: excise.Excisor(B).set_block_adapt(16.0, 2)
    got, stats = _scatter(hipbuf, x, cuts, _align(fmt), TX._bps(fmt), make, lambda h, d_x: TX._feed(hipbuf, h, d_x, fmt, n))
    ex = make()
    wa, ws = ex.windows()
    p = EM.resolve(B)
    perr, yerr, M = TX._one_case(ex, p, x, 16.0, 2, wa, ws, None, (B, fmt))
    ex.close()
    want, scale, _, _, _ = BM.run(p, x, 16.0, 2, masks=M, wa=wa, ws=ws)
    worst = TX._check((B, fmt, "carved"), got, want, scale)
    assert ((M == 0).sum(axis=1) >= 1).all()                             # every block has bins to zero
    assert stats == dict(inputs=n, outputs=EM.total_out(B, n), blanked=0)
    print("guard bands, excisor block-adapt B = %d %s: calls %s, %.3f of the bar" % (B, fmt, cuts, worst))


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("block", SI.BLOCKS)
def test_excisor_adapt(gpu, hipbuf, block, fmt):
    """excise_psd_kernel<Plan, FMT>: test_gpu_excise.py's CW input of 31 blocks and three samples that belong to no block (int8: its
    noise stream of 32 segments), carved"""
    import excise_model as EM
    import test_gpu_excise as TE
    from gnss_sdr_rs_amd import excise
    B, J = block, 31
    assert SI.excise_psd_form(B, fmt) in SI.EXCISE_PSD_FORMS
    blank = 150.0 if fmt == "i8" else 0.0
    x = TE._stream("i8", (J + 1) * (B // 2), J) if fmt == "i8" else TE._adapt_input(B, J, "cw", J)
    p = EM.resolve(B, 0, 0.0, blank)
    runs, worst = {}, 0.0
    for fill in GB.FILLS:
        ex = excise.Excisor(B, guard_bins=0, blank_threshold=blank)
        c = GB.carve(hipbuf, x, fill, align=_align(fmt))
        ex.adapt_dev(c, TE._fmt(fmt), len(x))
        err, r = TE._check_adapt(ex, p, x, ex.windows()[0], (B, fmt, hex(fill)))
        worst = max(worst, err)
        runs[fill] = dict(r, gains=ex.gains())
        assert GB.guards_intact(hipbuf, c) and ex.stats() == dict(inputs=0, outputs=0, blanked=0)
        ex.close()
    GB.same_words(runs)
    print("guard bands, excisor adapt B = %d %s: %.3f of the bar" % (B, fmt, worst))


# ---- gm_channelizer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,fmt", SI.CHANNELIZER_CHOSEN)
def test_channelizer(gpu, hipbuf, shape, fmt):
    import channelizer_model as CM
    import test_gpu_channelizer as TC
    from gnss_sdr_rs_amd import channelizer
    M, D, P = shape
    p = CM.resolve(M, D, taps_per_branch=P)
    L, tile = p["L"], CM.tile_outputs(p)
    n_of = lambda outputs: L // 2 + (outputs - 1) * D + 1                # the inputs that give that many outputs
    first, short, n = n_of(tile) + 1, L // 2 - 1, n_of(3 * tile) - 1
    cuts = (first, short, n - first - short)
    assert CM.total_out(p, first - 1) == tile and CM.total_out(p, n) == 3 * tile - 1 and 0 < short < L - 1
    x = TC._stream(fmt, n, 70 + M + D, M)
    make = lambda: channelizer.Channelizer(M, D, taps_per_branch=P)
    got, stats = _scatter(hipbuf, x, cuts, _align(fmt), TC._bps(fmt), make, lambda h, d_x: TC._feed(hipbuf, h, d_x, fmt, n),
                         signature="channelizer")
    h = make()
    want, weight, _ = CM.run(p, h.taps(), x)
    h.close()
    worst = TC._check((shape, fmt), got, want, weight)
    assert stats == dict(inputs=n, outputs=3 * tile - 1, blanked=0)
    print("guard bands, channelizer %s %s: calls %s, %.3g of the bar" % (shape, fmt, cuts, worst / TC.BAR))


# ---- gm_nuller, gm_stap, gm_beamformer, gm_lcmv --------------------------------------------------------------------------------------------
B = SI.SWEEP_BLOCK
ARRAY_N = 4 * B - 1                       # three blocks and a pending tail that ends one time sample in front of the fourth block's end
ARRAY_PAIRS = [(A, 2) for A in range(SI.A_MIN, SI.A_MAX + 1)] + [(A, 5) for A in range(SI.A_MIN, 7)]
assert sorted(SI.array_form(A, L) for A, L in ARRAY_PAIRS) == sorted(SI.ARRAY_FORMS)


def _array_cuts(L):
    """one time sample behind the first block's end, fewer than the L - 1 of history (one where there is none to undercut), the rest"""
    short = max(1, L - 2)
    return (B + 1, short, ARRAY_N - B - 1 - short)


@pytest.mark.parametrize("shape,fmt", SI.NULLER_CHOSEN)
def test_nuller(gpu, hipbuf, shape, fmt):
    import nuller_model as NM
    import test_gpu_nuller as TN
    from gnss_sdr_rs_amd import nuller
    A, block = shape
    assert block == B
    s = (np.random.default_rng(A).standard_normal(A) + 1j * np.random.default_rng(B).standard_normal(A)).astype(np.complex64)
    cuts, n = _array_cuts(1), ARRAY_N
    x = TN._stream(fmt, n, A, 80 + A)
    (y, R, w), stats = _scatter(hipbuf, x, cuts, _align(fmt), TN._bps(fmt, A), lambda: nuller.Nuller(A, B, 1e-4, s),
                                lambda h, d_x: TN._feed(hipbuf, h, d_x, fmt, n), blocks=(A * A * 8, A * 8))
    TN._check(("guard bands, nuller", shape, fmt), NM.resolve(A, B, 1e-4, s), x, y, R, w)
    assert stats == dict(inputs=n, outputs=3 * B, blocks=3)


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("A,L", ARRAY_PAIRS)
def test_stap(gpu, hipbuf, A, L, fmt):
    import stap_model as SM
    import test_gpu_stap as TS
    from gnss_sdr_rs_amd import stap
    M = A * L
    s = (np.random.default_rng(M).standard_normal(M) + 1j * np.random.default_rng(B + L).standard_normal(M)).astype(np.complex64)
    cuts, n = _array_cuts(L), ARRAY_N
    x = TS._stream(fmt, n, A, SI.sweep_seed(A, L))
    (y, R, w), stats = _scatter(hipbuf, x, cuts, _align(fmt), TS._bps(fmt, A), lambda: stap.Stap(A, L, B, SI.SWEEP_LOADING, s),
                                lambda h, d_x: TS._feed(hipbuf, h, d_x, fmt, n), blocks=(M * M * 8, M * 8))
    TS._check(("guard bands, stap", A, L, fmt), SM.resolve(A, L, B, SI.SWEEP_LOADING, s), x, y, R, w)
    assert stats == dict(inputs=n, outputs=3 * B, blocks=3, fallback_blocks=0)


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("A,L", ARRAY_PAIRS)
def test_beamformer(gpu, hipbuf, A, L, fmt):
    """five rows: a full group of four beams and a partial one"""
    import beam_model as BM
    import test_gpu_beam as TB
    import test_gpu_stap as TS
    from gnss_sdr_rs_amd import beamformer
    M, P = A * L, SI.BEAM_ROWS
    rows = TB._rows(P, M, 7 * M + P, e0_last=True)
    cuts, n = _array_cuts(L), ARRAY_N
    x = TS._stream(fmt, n, A, SI.sweep_seed(A, L))
    (y, R, w), stats = _scatter(hipbuf, x, cuts, _align(fmt), TS._bps(fmt, A), lambda: beamformer.Beamformer(A, L, rows, B, SI.SWEEP_LOADING),
                                lambda h, d_x: TB._feed(hipbuf, h, d_x, fmt, n), signature="planes", blocks=(M * M * 8, P * M * 8))
    p = BM.resolve(A, L, rows, B, SI.SWEEP_LOADING)
    for k in range(P):
        TS._check(("guard bands, beamformer", A, L, fmt, k), p["beams"][k], x, y[k], R, w[:, k])
    assert stats == dict(inputs=n, outputs=3 * B, blocks=3, fallbacks=[0] * P)


@pytest.mark.parametrize("fmt", SI.FORMATS)
@pytest.mark.parametrize("A,L", ARRAY_PAIRS)
def test_lcmv(gpu, hipbuf, A, L, fmt):
    import lcmv_model as LM
    import test_gpu_beam as TB
    import test_gpu_lcmv as TL
    import test_gpu_stap as TS
    from gnss_sdr_rs_amd import lcmv
    case = SI.lcmv_case(A, L)
    M, P = A * L, len(case[3])
    cs, redraws = LM.drawn(case)
    assert redraws == 0
    cuts, n = _array_cuts(L), ARRAY_N
    x = TS._stream(fmt, n, A, LM.case_seed(case))
    got, stats = _scatter(hipbuf, x, cuts, _align(fmt), TS._bps(fmt, A), lambda: lcmv.Lcmv(A, L, cs, block=B, loading=SI.SWEEP_LOADING),
                          lambda h, d_x: TB._feed(hipbuf, h, d_x, fmt, n), signature="planes", blocks=(M * M * 8, P * M * 8))
    worst = TL._check(("guard bands, lcmv", A, L, fmt), LM.resolve(A, L, cs, B, SI.SWEEP_LOADING), x, *got)
    assert stats == dict(inputs=n, outputs=3 * B, blocks=3, fallbacks=[0] * P)
    print("guard bands, lcmv (%d, %d) %s: R %.3g of its bar, w %.3g, C^H w = f %.3g, y %.3g" % ((A, L, fmt) + tuple(worst)))


# ---- gm_frontend ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i8", [False, True], ids=["c32", "i8"])
def test_frontend(gpu, oracle, hipbuf, i8):
    """after a 1000-sample block from a plain buffer (the state the forms need): a block of 2048 + 8 * 3 + 5 samples on the table form
    and the smallest block of the speculative form (48 pipeline segments), input and output carved, bit-exact with the oracle"""
    import fe_model as FM
    import test_gpu_frontend_forms as TF
    fmt, runs = TF._fmt(i8), {}
    blocks = ((2048 + 8 * 3 + 5, FM.TAB), (FM.SPEC_MIN, FM.SPEC))
    assert FM.nseg_of(FM.SPEC_MIN) >= 48
    for fill in GB.FILLS:
        fe, ofe = TF._pair(oracle, FM.C_BOUNDARY_SETTING)
        raw, f32 = FM.noise_dc(3, 1000, i8)
        TF._block(fe, ofe, hipbuf, raw, f32, i8, "first")
        outs = []
        for n, form in blocks:
            before = fe.debug_forms()
            raw, f32 = FM.noise_dc(n % 1000 + 17 * i8, n, i8)
            c_in = GB.carve(hipbuf, raw, fill, align=2 if i8 else 8)
            c_out = GB.carve(hipbuf, n * 8, 0x5A, align=8)
            assert c_in.nbytes == n * (2 if i8 else 8) and GB.disjoint(c_in, c_out)
            fe.process_dev(c_in, fmt, c_out, n)
            fe.synchronize()
            got = GB.read_back(hipbuf, c_out, np.float32)
            want = ofe.process_block(f32.copy())
            assert (TF._bits(got) == TF._bits(want)).all(), (n, hex(fill))
            TF._same_state(fe, ofe)
            assert TF._delta(fe, before) == TF._only(form), (n, hex(fill))
            assert GB.guards_intact(hipbuf, c_in) and GB.guards_intact(hipbuf, c_out, payload=False)
            outs.append(got)
        runs[fill] = outs + list(fe.state())
        fe.close()
    GB.same_words(runs)


# ---- acquisition: gm_acq_search_dev, gm_acq_prepare_dev + gm_acq_search_prepared_dev --------------------------------------------------------
ACQ_ELEMENT = {"i8": 2, "real": 1, "c32": 8}                    # int8 IQ pairs, int8 real samples, complex64 words
ACQ_FORMS = ("lds", "composite", "long", "long_padded")
# coherent K = 2; an edge search with two offsets; code drift, where the dwell is max_d s[d][R - 1] + N by the plan's rule, so the last
# period of the bin with the longest code period (bin 2) ends exactly on the dwell's last sample
ACQ_MODES = (("coherent", 2, 2, None, None, None, 0),
             ("edge", 2, 2, (0, 2), (1, -1), None, 1),
             ("drift", 2, 2, None, None, (-0.4, 0.3), 2))


def _acq_row(form):
    """the row of acq_model.CASES with the smallest fft_size of a form"""
    import acq_model as AM
    return min((n, i) for i, (n, f, _) in enumerate(AM.CASES) if f == form)[1]


def _acq_fmt(A, fmt):
    return dict(i8=A.FMT_I8_IQ, real=A.FMT_I8_REAL, c32=A.FMT_C32)[fmt]


def _acq_engine(c, form, K, M):
    import test_gpu_stage_f_variants as TV
    from gnss_sdr_rs_amd import acquisition as A
    eng = TV._engine(A, c, form, K, M, False)
    if c["offsets"]:
        eng.set_edge_search(c["offsets"], c["sec"])
    if c["T"] is not None:
        eng.set_code_drift(c["T"])
        assert (eng.code_drift_starts() == c["starts"]).all()
    return eng


def _acq_words(hipbuf, eng, d_x, fmt, prepared=False):
    """one search of the dwell at d_x into a carved metrics block -> dict of the block's words [3][P][D] and, with an edge search, the
    per-hypothesis block and the choice"""
    import acq_model as AM
    from gnss_sdr_rs_amd import acquisition as A
    n = 3 * AM.P * AM.D
    d_met = GB.carve(hipbuf, n * 4, 0x5A, align=4)
    if prepared:
        eng.search_prepared_dev(eng.prepare_dev(d_x, _acq_fmt(A, fmt)), d_met)
    else:
        eng.search_dev(d_x, _acq_fmt(A, fmt), d_met)
    eng.synchronize()
    assert GB.guards_intact(hipbuf, d_met, payload=False)
    out = dict(metrics=GB.read_back(hipbuf, d_met, np.uint32).reshape(3, AM.P, AM.D))
    return out


def acq_window(c):
    """[P][H][D] bool: the cells whose arg-max must lie where the scene puts the code phase.  Every cell, but for the coherent fold at
    K = 2 without a secondary row: a satellite 430 or 470 Hz off a bin (one code period is 1 ms) folds to |1 + e^(j 2 pi 0.43)| / 2 =
    0.22 or 0.09 of its power there, and the cell's peak need not be the satellite's; there the fold must keep half the amplitude.
    tests/test_guard_bands_host.py holds every scene of this file to this window and to acq_model.GAP on the CPU."""
    import acq_model as AM
    w = np.ones(c["expect"].shape[:3], bool)
    if c["name"] == "coherent":
        off = np.asarray(AM.SAT_DOPPLER, np.float64)[:, None] - AM.DOP.astype(np.float64)[None, :]
        w[:] = (np.abs(1.0 + np.exp(2j * np.pi * off * 1e-3)) / 2.0 >= 0.5)[:, None, :]
    return w


def _acq_check(tag, c, eng, x, K, M, words):
    """every cell against the float64 model of acq_model.py as tests/test_gpu_stage_f_variants.py holds it: the arg-max equal and, in
    the cells of acq_window, where the scene puts the code phase; max and sum within REL; with offsets the per-hypothesis block against
    the model and the reduced block against numpy's reduction of it"""
    import acq_model as AM
    import test_gpu_stage_f_variants as TV
    met = words["metrics"]
    mx, am, sm = met[0].view(np.float32), met[1], met[2].view(np.float32)
    if c["offsets"]:
        fmx, fam, fsm = words["edge_max"], words["edge_argmax"], words["edge_sum"]
        rmx, ram, rsm, ch = AM.reduce_block(fmx, fam, fsm)
        assert (TV._words(mx) == TV._words(rmx)).all() and (am == ram).all() and (TV._words(sm) == TV._words(rsm)).all(), tag
        assert (words["edge_choice"] == ch).all(), tag
    else:
        fmx, fam, fsm = mx[:, None, :], am[:, None, :], sm[:, None, :]
    starts = None if c["T"] is None and not c["offsets"] and K * M * c["N"] == len(x) else c["starts"]
    emx, eam, esm = AM.search_model(x, eng.tables(), c["codes"], c["N"], K, M, AM.DOP, c["fs"], starts, c["offsets"], c["sec"])
    rel = lambda got, want: float(np.max(np.abs(got.astype(np.float64) / want - 1.0)))
    assert (fam == eam).all(), (tag, fam, eam)
    assert (((eam >= c["expect"][..., 0]) & (eam <= c["expect"][..., 1])) | ~acq_window(c)).all(), (tag, eam)
    assert np.allclose(fmx, emx, rtol=AM.REL, atol=0.0), (tag, fmx, emx)
    assert np.allclose(fsm, esm, rtol=AM.REL, atol=0.0), (tag, fsm, esm)
    return max(rel(fmx, emx), rel(fsm, esm)) / AM.REL


def _acq_case(hipbuf, c, form, K, M, x, prepared_too):
    """the dwell x, carved, through a fresh handle per fill -> the largest fraction of REL"""
    fmt = c["fmt"]
    runs, worst = {}, 0.0
    for fill in GB.FILLS:
        eng = _acq_engine(c, form, K, M)
        assert eng.dwell_samples == len(x)
        d_x = GB.carve(hipbuf, x, fill, align=ACQ_ELEMENT[fmt])
        assert d_x.nbytes == len(x) * ACQ_ELEMENT[fmt]
        words = _acq_words(hipbuf, eng, d_x, fmt)
        if c["offsets"]:
            fmx, fam, fsm = eng.edge_metrics()
            words.update(edge_max=fmx, edge_argmax=fam, edge_sum=fsm, edge_choice=eng.edge_choice())
        worst = max(worst, _acq_check((c["N"], form, c["name"], fmt, hex(fill)), c, eng, x, K, M, words))
        if prepared_too:
            GB.same_words({"search_dev": words, "prepared": _acq_words(hipbuf, eng, d_x, fmt, prepared=True)})
        assert GB.guards_intact(hipbuf, d_x), hex(fill)
        runs[fill] = words
        eng.close()
    GB.same_words(runs)
    return worst


@pytest.mark.parametrize("fmt_index", range(3), ids=["i8", "real", "c32"])
@pytest.mark.parametrize("form", ACQ_FORMS)
def test_acquisition_plain(gpu, oracle, hipbuf, form, fmt_index):
    """K = 1, M = 2 on the first two periods of the coherent scene of the form's smallest size (256, 18000, 6144, 2040), a dwell of
    exactly dwell_samples() elements, through search_dev and through prepare_dev + search_prepared_dev.  On the padded form (N = 2040
    in transforms of 4096) the reads between N, 2 N and the transform length are the point."""
    import acq_model as AM
    row = _acq_row(form)
    N = AM.CASES[row][0]
    assert N == {"lds": 256, "composite": 18000, "long": 6144, "long_padded": 2040}[form]
    c = AM.build_case(oracle.ca_code_table(), N, 0, fmt_index)            # (the row index only chooses the format)
    assert c["fmt"] == AM.FORMATS[fmt_index] and c["T"] is None and c["offsets"] is None
    c = dict(c, name="plain")
    x = c["x"][:2 * N]
    worst = _acq_case(hipbuf, c, form, 1, 2, x, prepared_too=True)
    print("guard bands, acquisition plain N = %d (%s) %s: %.3g of the bar" % (N, form, c["fmt"], worst))


@pytest.mark.parametrize("mode", range(len(ACQ_MODES)), ids=[m[0] for m in ACQ_MODES])
@pytest.mark.parametrize("form", ["lds", "long"])
def test_acquisition_modes(gpu, oracle, hipbuf, form, mode):
    """coherent K = 2, an edge search with the offsets [0, 2] and the row [1, -1], and code drift (T_d = N - 0.4 + 0.3 d), at N = 256
    and N = 6144; the formats rotate over the modes"""
    import acq_model as AM
    N = AM.CASES[_acq_row(form)][0]
    c = AM.build_case(oracle.ca_code_table(), N, ACQ_MODES[mode], 0)
    if c["T"] is not None:                                                # the drift plan admits the flush end: it is the dwell's definition
        assert c["dwell"] == int(c["starts"][:, -1].max()) + N == int(c["starts"][AM.D - 1, -1]) + N
    worst = _acq_case(hipbuf, c, form, c["K"], c["M"], c["x"], prepared_too=False)
    print("guard bands, acquisition %s N = %d (%s) %s: %.3g of the bar" % (c["name"], N, form, c["fmt"], worst))


@pytest.mark.parametrize("form", ["composite", "long", "long_padded"])
def test_acquisition_scratch_of_the_search_before(gpu, oracle, hipbuf, form):
    """a handle that has searched a dwell of 0x7F bytes (float32: 3.39e38 in every word, int8: 127) gives the words of a fresh handle on
    the real dwell: nothing of the reused scratch (the long path's zero-padded transforms, partials, planes) decides a word"""
    import acq_model as AM
    N = AM.CASES[_acq_row(form)][0]
    c = AM.build_case(oracle.ca_code_table(), N, 0, 2)
    assert c["fmt"] == "c32"
    x = c["x"][:2 * N]
    runs = {}
    for name in ("fresh", "after 0x7F"):
        eng = _acq_engine(c, form, 1, 2)
        if name != "fresh":
            _acq_words(hipbuf, eng, GB.carve(hipbuf, np.full(x.nbytes, 0x7F, np.uint8), 0x7F, align=8), "c32")
        d_x = GB.carve(hipbuf, x, 0xFF, align=8)
        runs[name] = _acq_words(hipbuf, eng, d_x, "c32")
        assert GB.guards_intact(hipbuf, d_x)
        eng.close()
    GB.same_words(runs)
    eng = _acq_engine(c, form, 1, 2)
    _acq_check((N, form, "after 0x7F"), dict(c, name="plain"), eng, x, 1, 2, runs["after 0x7F"])
    eng.close()


# ---- known cells: gm_acq_local_search on fresh samples --------------------------------------------------------------------------------------
def test_local_search(gpu, oracle, hipbuf):
    """test_gpu_local_search.py's smallest case (N = 256, coherent, c32: below one tile), every (worker, bin) cell a candidate centred
    on the search's arg-max, lag_half_window = 64, the dwell handed over as d_samples in a carved buffer.  Worker 0's code starts at
    N - 91, so its 129 lags reach across the period's end in every period, the dwell's last one included."""
    import acq_model as AM
    import test_gpu_local_search as TL
    L = 64
    eng, c, am, off = TL._searched(oracle, 256, "lds", 0, 2)
    assert c["fmt"] == "c32" and int(am[0].max()) > c["N"] - 100
    tab, tf = eng.tables(), eng.table_freq
    cands = [TL._cand(w, d, am[w, d], off[w, d]) for w in range(AM.P) for d in range(AM.D)]
    want = [TL._model(c, tab, tf, cand, L) for cand in cands]
    runs, worst = {}, np.zeros(3)
    for fill in GB.FILLS:
        d_x = GB.carve(hipbuf, c["x"], fill, align=8)
        got = eng.local_search(cands, samples=d_x, lag_half_window=L, want_prompts=True, want_surface=True, fmt=TL._fmt(c))
        for i, (cand, g, m) in enumerate(zip(cands, got, want)):
            worst = np.maximum(worst, TL._check_against_model(("guard bands", hex(fill), i), c, g, m, cand, L)[:3])
        assert GB.guards_intact(hipbuf, d_x), hex(fill)
        runs[fill] = {"%d.%s" % (i, k): v for i, g in enumerate(got) for k, v in g.items()}
    eng.close()
    GB.same_words(runs)
    print("guard bands, local search: prompts %.3g of the bar, surface %.3g, fine code phase %.2e sample" %
          (worst[0] / TL.REL, worst[1] / (3 * TL.REL), worst[2]))



def test_local_search_reads_the_whole_last_period(gpu, oracle, hipbuf):
    """what test_local_search rests on: every candidate's prompts take the dwell's first and its very last sample (a lag is a rotation
    inside a period, so each of the 129 lags reads all N samples of every period, the last one up to the byte in front of the guard)"""
    import acq_model as AM
    import test_gpu_local_search as TL
    eng, c, am, off = TL._searched(oracle, 256, "lds", 0, 2)
    cands = [TL._cand(w, d, am[w, d], off[w, d]) for w in range(AM.P) for d in range(AM.D)]
    x = c["x"].copy()
    run = lambda v: eng.local_search(cands, samples=GB.carve(hipbuf, v, 0xFF, align=8), lag_half_window=64, want_prompts=True, fmt=TL._fmt(c))
    ref = run(x)
    for index in (0, len(x) - 1):
        y = x.copy()
        y[index] += np.complex64(40 + 40j)
        for g, r in zip(run(y), ref):
            assert (g["prompts"].view(np.uint32) != r["prompts"].view(np.uint32)).any(axis=1).all(), index      # every lag's prompts moved
    eng.close()


# ---- known cells on an antenna array: gm_acq_array_prompts, gm_trk_array_prompts(_dev) ------------------------------------------------------
@pytest.mark.parametrize("fmt", SI.FORMATS)
def test_acq_array_prompts(gpu, hipbuf, fmt):
    """tests/test_gpu_array_probe.py's N = 2048 handle (K = 1, M = 3), A = 4 antennas at the largest tap count L = 8, its 40 candidates
    (code phases 0, 1 and N - 1 among them: with eight taps their last period ends on the carved dwell's last time sample)"""
    import stap_model as SM
    import test_gpu_array_probe as TP
    A, L = 4, 8
    s = TP._setup(2048)
    xd = TP._stream(fmt, s["dwell"], A, 100 * A + L)
    cands = TP._cands(2048, s["o_max"])
    assert {c["code_phase_samples"] for c in cands[:12]} == {0, 1, 2047}
    runs = {}
    for fill in GB.FILLS:
        d_x = GB.carve(hipbuf, xd, fill, align=_align(fmt))
        runs[fill] = s["eng"].array_prompts(cands, d_x, A, L, TP._fmt(fmt))
        assert GB.guards_intact(hipbuf, d_x), hex(fill)
    worst = TP._fraction(s, SM.as_c128(xd), cands, runs[0x00], A, L)
    assert worst <= TP.REL
    GB.same_words(runs)
    print("guard bands, acq array prompts %s: %.3g of the bar" % (fmt, worst / TP.REL))


@pytest.mark.parametrize("fmt", SI.FORMATS)
def test_trk_array_prompts(gpu, hipbuf, oracle, fmt):
    """tests/test_gpu_trk_array.py's smallest size (n = 2048, A = 4) at the largest tap count L = 8: 40 records, among them s = 0, 1, L - 1
    (the zero halo) and the two that end on and one before the carved buffer's last time sample; the host-output entry and the _dev
    entry, whose z and done buffers are carved too"""
    import stap_model as SM
    import test_gpu_trk_array as TA
    import trk_array_model as M
    from gnss_sdr_rs_amd import tracking as T
    n, A, L = 2048, 4, 8
    fs, n_time = 1000.0 * n, 2 * n + 777
    xd = TA._stream(fmt, n_time, A, 100 * A + L)
    table = oracle.ca_code_table()
    mgr = T.TrackingManager(fs, n_channels=2, code_index_mode=T.CODE_INDEX_FIXED)
    recs = TA._records(T, n, L, n_time, 40, n + A + L)
    assert [st.next_sample_index for st in recs[:6]] == [0, 1, L - 1, 3, n_time - n, n_time - n - 1]
    rows = TA._rows(table, recs, M.FIXED)
    runs = {}
    for fill in GB.FILLS:
        d_x = GB.carve(hipbuf, xd, fill, align=_align(fmt))
        z, done = mgr.array_prompts(d_x, n_time, A, L, states=recs, fmt=TA._fmt(fmt))
        d_z, d_done = GB.carve(hipbuf, 40 * L * A * 8, 0x5A, align=8), GB.carve(hipbuf, 40, 0x5A, align=1)
        mgr.array_prompts_dev(d_x, n_time, A, recs, d_z, d_done, taps=L, fmt=TA._fmt(fmt))
        mgr.synchronize()
        z_dev, done_dev = GB.read_back(hipbuf, d_z, np.complex64).reshape(40, L, A), GB.read_back(hipbuf, d_done, np.uint8)
        GB.same_words({"host outputs": (z, done), "_dev": (z_dev, done_dev)})
        assert GB.guards_intact(hipbuf, d_x) and GB.guards_intact(hipbuf, d_z, payload=False) and GB.guards_intact(hipbuf, d_done, payload=False)
        runs[fill] = (z, done)
    worst = TA._worst(runs[0x00][0], runs[0x00][1], recs, SM.as_c128(xd), fs, rows, L, 0.0, M.FIXED)
    assert worst <= TA.REL
    GB.same_words(runs)
    mgr.close()
    print("guard bands, trk array prompts %s: %.3g of the bar" % (fmt, worst / TA.REL))


# ---- gm_acq_cancel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i8", "real", "c32"])
def test_cancel(gpu, oracle, hipbuf, fmt):
    """tests/test_gpu_cancel.py's drift scene (12286 samples: no multiple of 8) and its five candidates, the dwell carved, d_out carved
    at both of its alignments (8 bytes and no more: stores of one sample; 16 bytes)"""
    import test_gpu_cancel as TC
    c = TC._scene(oracle, fmt, True)
    D = c["dwell"]
    eng = TC._engine(c, TC.M_PARITY, True)
    cands = TC._candidate_sets(D)["five"]
    runs, worst = {}, None
    for fill in GB.FILLS:
        d_x = GB.carve(hipbuf, c["x"], fill, align={"i8": 2, "real": 1, "c32": 8}[fmt])
        for out_align in (8, 16):
            d_out = GB.carve(hipbuf, D * 8, 0x5A, align=out_align)
            assert GB.disjoint(d_x, d_out)
            got = eng.cancel(cands, d_out, samples=d_x, fmt=TC._fmt(fmt), want_amps=True)
            y = GB.read_back(hipbuf, d_out, np.complex64)
            assert GB.guards_intact(hipbuf, d_out, payload=False) and GB.guards_intact(hipbuf, d_x), (hex(fill), out_align)
            if worst is None:
                worst = TC._check((fmt, "guard bands"), c, cands, got, y)
            runs[(fill, out_align)] = dict({"%d.%s" % (i, k): v for i, g in enumerate(got) for k, v in g.items()}, y=y)
    eng.close()
    GB.same_words(runs)
    print("guard bands, cancel %s: output %.3g of the bar, amplitudes %.3g" % (fmt, worst[0] / TC.REL, worst[1] / TC.REL))


# ---- gm_array_rows_solve_dev, gm_plane_ring_write_dev: strides above the minimum ---------------------------------------------------------------
def _strided(blocks, stride, fill):
    """the equal-sized blocks `stride` complex64 words apart, the gaps between them holding the fill byte, nothing behind the last"""
    k = blocks.shape[1]
    buf = np.full(((len(blocks) - 1) * stride + k) * 8, fill, np.uint8).view(np.complex64)
    for i, b in enumerate(blocks):
        buf[i * stride:i * stride + k] = b
    return buf


@pytest.mark.parametrize("m,n,n_blocks,n_rows,loading", [(8, 9, 1, 5, 1e-2), (3, 9, 20, 16, 1e-2)])
def test_rows_solve_dev_with_gaps(gpu, hipbuf, m, n, n_blocks, n_rows, loading):
    """vec_stride = m + 3 and row_stride = n vec_stride + 5, both above the minimum: the gaps between the vectors and between the rows
    hold the fill byte (part of the carved payload, so guards_intact shows them unchanged) and the last vector of the last row ends at
    the guard; R carved as well.  Against gm_array_row_solve on the host at tests/test_gpu_array_resteer.py's bars."""
    import test_gpu_array_resteer as TR
    z, R = TR._inputs(m, n, n_blocks, n_rows, 1000 * m + n + n_blocks + n_rows)
    want, infos = TR._host(z, R, loading, n == 1)
    vs = m + 3
    rs = n * vs + 5
    runs = {}
    for fill in GB.FILLS:
        rows = np.stack([_strided(z[p], vs, fill) for p in range(n_rows)])
        flat = _strided(rows, rs, fill)
        assert flat.size == (n_rows - 1) * rs + (n - 1) * vs + m and (flat[rs + (n - 1) * vs:rs + (n - 1) * vs + m] == z[1, n - 1]).all()
        d_z, d_R = GB.carve(hipbuf, flat, fill, align=8), GB.carve(hipbuf, R, fill, align=8)
        got, info = TR._device(hipbuf, None, R, m, n, n_rows, loading, row_stride=rs, vec_stride=vs, d_z=d_z, d_R=d_R)
        assert GB.guards_intact(hipbuf, d_z) and GB.guards_intact(hipbuf, d_R), hex(fill)          # the gap words included
        runs[fill] = (got, info.view(np.uint8))
    got, info = runs[0x00][0], runs[0x00][1].view(TR.INFO)
    assert not info["status"].any()
    assert float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))) <= TR.ROW_BAR
    l1 = np.array([i["lambda1"] for i in infos]); l2 = np.array([i["lambda2"] for i in infos])
    assert (np.abs(info["lambda1"] - l1) <= 1e-9 * l1).all() and (np.abs(info["lambda2"] - l2) <= 1e-9 * l2 + 1e-12 * l1).all()
    assert list(info["ref_index"]) == [i["ref_index"] for i in infos]
    GB.same_words(runs)


@pytest.mark.parametrize("n,in_stride,align", [(1001, 1004, 8), (1000, 1006, 16)])
def test_plane_ring_write_dev_with_gaps(gpu, hipbuf, n, in_stride, align):
    """three planes in_stride > n words apart, the gaps holding the fill byte and the last plane ending at the guard, written twice into
    a ring of 2^11 samples a plane so that the second write wraps; odd n from an 8-byte address (8-byte accesses) and even n, even stride
    from a 16-byte one (16-byte accesses).  Every plane of the ring holds its words and nothing else."""
    from gnss_sdr_rs_amd import tracking as T
    P, size = 3, 1 << 11
    rng = np.random.default_rng(n)
    calls = [(rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))).astype(np.complex64) for _ in range(3)]
    runs = {}
    for fill in GB.FILLS:
        pr = T.PlaneRing(P, size)
        for planes in calls:
            d = GB.carve(hipbuf, _strided(planes, in_stride, fill), fill, align=align)
            pr.write_dev(d, in_stride, n)
            pr.synchronize()
            assert GB.guards_intact(hipbuf, d), hex(fill)
        assert pr.get_head() == 3 * n > size
        runs[fill] = np.stack([pr.copy_to_slice(p, 3 * n - size, size) for p in range(P)])
        pr.close()
    assert (runs[0x00].view(np.uint32) == np.concatenate(calls, axis=1)[:, 3 * n - size:].view(np.uint32)).all()
    GB.same_words(runs)


# ---- rings: nothing beyond `head` decides a word ------------------------------------------------------------------------------------------
def _lap(nan, shape):
    """one full lap of a ring: NaN in every word, or zeros (what a ring holds beyond `head` in every other test)"""
    return np.full(shape, complex(np.nan, np.nan) if nan else 0.0, np.complex64)


def test_search_ring_behind_a_lap_of_nan(gpu, oracle):
    """gm_acq_search_ring on a ring of 2^13 samples that has held one lap of NaN: three periods of N = 2048 follow, so `head` is 6144
    into the second lap, the dwell is the 4096 samples in front of it and every position beyond `head` is NaN.  The results and the
    metric words are those of a ring whose lap was zeros, and go against the oracle as in tests/test_gpu_any_length.py."""
    import test_gpu_any_length as TA
    from gnss_sdr_rs_amd import acquisition as A, synth, tracking as T
    N, M, size, rate = 2048, 2, 1 << 13, 1.023e6
    fs = float(N) * 1000.0
    dop = np.array([-500.0, 0.0, 500.0], np.float32)
    prns = [5, 12, 20]
    sats = [dict(prn_row=4, cn0_dbhz=50.0, doppler_hz=120.0, code_start=1500), dict(prn_row=11, cn0_dbhz=50.0, doppler_hz=-310.0, code_start=55)]
    x = synth.to_c32(synth.make_scene(oracle.ca_code_table(), fs, 0.0, 3 * N, sats, config_id=340))
    runs = {}
    for name in ("zeros", "nan"):
        eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prns, n_integrations=M)
        ring = T.MulticastRingBuffer(size)
        ring.write_samples(_lap(name == "nan", size))
        ring.write_samples(x)
        res, tail = eng.search_ring(ring)
        assert tail == size + N and ring.get_head() == size + 3 * N
        eng.last_results = res
        mx, am, sm = TA._check_against_oracle(oracle, eng, x[N:], fs, N, M, dop, prns, None, rate)
        assert res[0]["code_phase_samples"] == 1500 and res[1]["code_phase_samples"] == 55
        runs[name] = dict(mx=mx, am=am, sm=sm, found=np.array([r is not None for r in res]),
                          mag=np.array([r["mag_relative"] if r else 0.0 for r in res], np.float64),
                          index=np.array([r["sample_global_index"] if r else 0 for r in res], np.int64))
        ring.close(); eng.close()
    GB.same_words(runs)


TRK_FORMS = [dict(), dict(strict_libm=True), dict(strict_libm=True, strict_sum_order=True)]


@pytest.mark.parametrize("kw", TRK_FORMS, ids=["persistent", "strict_libm", "serial"])
def test_update_all_behind_a_lap_of_nan(gpu, oracle, kw):
    """gm_trk_update_all (the persistent default, strict_libm, and strict_libm + strict_sum_order: the serial path) on
    tests/test_gpu_tracking.py's six-channel scene, on a ring of 2^16 samples that has held one lap of NaN: 13 ms follow, every channel's
    next period begins inside the written part and ends beyond `head`, so the give-up gate and the kernel's prefetch both meet the lap.
    Outputs, flags and every state word equal the run on a ring whose lap was zeros, and the outputs go against the oracle's update() at
    that file's bar."""
    import test_gpu_tracking as TT
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, n, mode, size = 4_096_000.0, 4096, 1, 1 << 16
    sc = synth.tracking_scene(oracle.ca_code_table(), fs, 0.0, [3, 8, 13, 21, 27, 31], 14, config_id=23, cn0=50.0)
    x = synth.to_c32(sc["x"])
    runs = {}
    for name in ("zeros", "nan"):
        ring, oring = T.MulticastRingBuffer(size), oracle.MulticastRingBuffer(size)
        mgr = T.TrackingManager(fs, n_channels=8, code_index_mode=mode, **kw)
        ocs = []
        for i, s in enumerate(sc["sats"]):
            r = TT._acq_result(s["prn"], s["doppler_hz"] + 30.0, 0.0, fs, idx=size + s["code_start"])
            mgr.channels[i].start(r)
            ocs.append(oracle.TrackingChannel(i, fs, code_index_mode=mode))
            ocs[-1].start(r)
        for rg in (ring, oring):
            rg.write_samples(_lap(name == "nan", size))
            rg.write_samples(x[:13 * n])
        assert (ring.get_head() - size) % n == 0 and all(s["code_start"] % n for s in sc["sats"])      # `head` is inside every period
        outs, proc, lost, done = mgr.update_all(ring, 16)
        ran = proc.astype(bool)
        assert done == 12 and not lost.any() and np.isfinite(outs[ran]).all()
        for i, oc in enumerate(ocs):
            for ep in range(16):
                rc, exp, msg = oc.update(oring)
                assert (rc != 0) == bool(proc[ep, i]), (i, ep)
                if rc:
                    assert np.max(np.abs(outs[ep, i] - exp)) <= 2.5 * TT.REL * float(np.hypot(exp[0], exp[1])), (name, i, ep)
            assert mgr.channels[i].state.next_sample_index == oc.c.next_sample_index
        state = np.concatenate([np.frombuffer(bytes(mgr.channels[i].state), np.uint8) for i in range(8)])
        runs[name] = dict(state=state, outs=outs[ran], proc=proc, lost=lost)
        mgr.close(); ring.close()
    GB.same_words(runs)


def test_bank_behind_a_lap_of_nan(gpu, oracle):
    """gm_trk_bank on tests/test_gpu_trk_bank.py's scene (n = 2048, four satellites, 4 ms) behind one lap of NaN on a ring of 2^16: the
    fifth record's period is the last whole one in front of `head`; 3 x 3 and 32 x 8 words"""
    import test_gpu_trk_bank as TB
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, rate, n, mode, size = 2.048e6, 1.023e6, 2048, 1, 1 << 16
    table = oracle.ca_code_table()
    prns = [3, 9, 17, 25]
    sc = synth.tracking_scene(table, fs, 0.0, prns, 4, config_id=71, cn0=50.0, code_rows=[p - 1 for p in prns])
    x = synth.to_c32(sc["x"])
    recs, rows = [], []
    for k, s in enumerate(sc["sats"] + sc["sats"][:1]):
        nxt = size + s["code_start"] + (2 * n if k == 4 else 0)
        recs.append(TB._record(T, s["prn"], nxt, n, s["doppler_hz"] + 7.0 * k, code_phase=0.125 * (k % 3), code_rate=rate))
        rows.append(table[prns[k % 4] - 1])
    head = size + len(x)
    assert head - 2 * n < recs[4].next_sample_index + n <= head and sc["sats"][0]["code_start"] % n
    xx = np.concatenate([np.zeros(size, np.complex64), x])
    runs = {}
    for name in ("zeros", "nan"):
        ring = T.MulticastRingBuffer(size)
        ring.write_samples(_lap(name == "nan", size))
        ring.write_samples(x)
        mgr = T.TrackingManager(fs, n_channels=2, code_index_mode=mode)
        out = {}
        for nt, nf in ((3, 3), (32, 8)):
            taps, offs = TB.TAP_SETS[nt], TB.OFF_SETS[nf]
            o, done = mgr.bank(ring, taps, offs, states=recs)
            TB._worst(o, done, recs, xx, fs, rows, taps, offs, mode)
            out["%dx%d" % (nt, nf)], out["done%d" % nt] = o, done
        runs[name] = out
        mgr.close(); ring.close()
    GB.same_words(runs)


def test_update_planes_behind_a_lap_of_nan(gpu, oracle):
    """gm_trk_update_planes on tests/test_gpu_trk_planes.py's three planes and five channels (n = 2048), every plane of a gm_plane_ring
    of 2^16 samples having held one lap of NaN: 13 periods follow and 16 passes are asked for, so every channel gives up with its next
    period reaching beyond `head`.  The oracle twins of that file at its bars; every output and state word equals the run on a lap of
    zeros."""
    import test_gpu_trk_planes as TP
    from gnss_sdr_rs_amd import tracking as T
    n, mode, E, size = 2048, 1, 12, 1 << 16
    x, by_prn = TP._plane_scenes(oracle, n * 1000.0, mode, E + 2, 300 + (n % 100) * 3 + mode * 40)
    x = x[:, :(E + 1) * n]
    runs = {}
    for name in ("zeros", "nan"):
        pr, orings = TP._rings(oracle, _lap(name == "nan", (3, size)), size)
        pr.write(x)
        for p, o in enumerate(orings):
            o.write_samples(x[p])
        mgr = T.TrackingManager(TP.FS, n_channels=6, code_index_mode=mode)
        mgr.set_channel_planes(TP.MAP + [1])
        starts = [dict(r, sample_global_index=r["sample_global_index"] + size) for r in TP._starts(by_prn, TP.FS)]
        tw = TP.Twin(mgr, orings, TP.MAP + [1], starts + [None], lambda i: oracle.TrackingChannel(i, TP.FS, code_index_mode=mode), 3)
        result = mgr.update_planes(pr, 16)
        assert tw.step(result) == E and tw.ran == [E] * 5 + [0]
        TP._fractions("guard bands, update_planes behind a lap of %s" % name, tw.check_states())
        state = np.concatenate([np.frombuffer(bytes(mgr.channels[i].state), np.uint8) for i in range(6)])
        runs[name] = dict(outs=result[0], proc=result[1], lost=result[2], state=state)
        mgr.close(); pr.close()
    GB.same_words(runs)
