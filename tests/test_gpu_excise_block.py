"""The excisor's block-adapt mode on the GPU (gm_excisor_set_block_adapt, csrc/excise_kernels.hip) against excise_block_model.py.

The streams are 6007 to 12301 samples of noise plus a CW that moves five bins a block, so that every block gets a mask of its own.
1. Masks.  The captured power words within 1e-5 max_k p[k] of the float64 model per block; the captured masks EQUAL, byte for byte, to
   the model's float32 rule applied to the device's own power words; block_stats equal to the counts from those masks under the
   once-per-block rule.  B = 256, 512, 1024, 2048, 4096 (every plan: at 512 one wave holds every bin and every lane holds bins, at 2048
   two of the four waves hold bins), both formats, factor 16 and 6, guard 0, 2 and 16 (4096: factor 16, guard 2).
2. Outputs within the 1e-5 max|xb| bound of the float64 stream model, which is handed the library's windows, the static gains and the
   device's masks; one run with random static gains, so that both gains multiply.
3. Independence: one call against blocks of 1, 7, H - 1, 1000 and 3001 bit for bit, counters included; after a reset to 2^32 - 3; twice.
4. Off is off; a factor so large that nothing is flagged gives the static handle's words.
5. Blanking: the mask is taken on the blanked block.
6. Every refusal leaves gains, mode, state and counters alone.
7. The ring paths pick the mode up through the handle.
8. The chain: the swept scene at J/N 30 dB through the mode and a plain search_dev."""
import ctypes as C
import math

import numpy as np
import pytest

import excise_block_model as BM
import excise_model as EM
import stage_instantiations as SI

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_RANGE = -1, -5
REL = 1e-5


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _moving(fmt, n, B, seed, bins_per_block=5.0):
    """noise plus a CW 20 dB above each noise component that starts at bin 0.11 B and moves bins_per_block bins every B samples"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    cycles = 0.11 * t + 0.5 * (bins_per_block / (B * B)) * t * t
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n) + 10.0 * np.exp(2j * np.pi * (cycles - np.floor(cycles)))
    if fmt == "i8":
        v = np.clip(np.round(8.0 * np.stack([z.real, z.imag], axis=1)), -128, 127).astype(np.int8)
        return v
    return z.astype(np.complex64)


def _bps(fmt):
    return 2 if fmt == "i8" else 8


def _fmt(fmt):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if fmt == "i8" else _lib.FMT_C32


def _feed(hipbuf, ex, d_x, fmt, n, blocks=None):
    """the n samples at d_x through ex.process_dev in blocks (None: one call) -> complex64 outputs"""
    cap = n + 4096
    d_y = hipbuf.alloc(cap * 8 + 64, fill=0x5A)
    done = got = 0
    step = blocks or max(n, 1)
    while done < n:
        k = min(step, n - done)
        got += ex.process_dev(d_x + done * _bps(fmt), _fmt(fmt), k, d_y + got * 8, cap - got)
        done += k
    ex.synchronize()
    raw = hipbuf.download(d_y, cap * 8 + 64, np.complex64)
    assert (raw[got:].view(np.uint8) == 0x5A).all()
    return raw[:got].copy()


def _check(tag, got, want, scale):
    assert got.size == want.size and got.size, (tag, got.size, want.size)
    assert np.isfinite(got.view(np.float32)).all(), tag
    err = np.abs(got.astype(np.complex128) - want)
    bound = REL * scale
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (tag, worst)
    return worst


def _one_case(ex, p, x, factor, guard, wa, ws, gains, tag):
    """one call with the capture -> (worst power error / bound, worst output error / bound, masks)"""
    ex.reset(0)
    y, P, M = ex.process(x, want_blocks=True)
    want, scale, P64, _, _ = BM.run(p, x, factor, guard, masks=M, wa=wa, ws=ws, gains=gains)
    assert P.shape == M.shape == P64.shape == (y.size // (p["B"] // 2) + 1, p["B"]), tag
    perr = float((np.abs(P.astype(np.float64) - P64).max(axis=1) / (REL * P64.max(axis=1))).max())
    assert perr <= 1.0, (tag, perr)
    _, flag, mask = BM.decide(P, factor, guard)
    assert (mask == M).all(), (tag, int((mask != M).sum()))
    assert ex.block_stats() == BM.count([flag], [mask]), tag
    return perr, _check(tag, y, want, scale), M


N_OF = {256: 6007, 512: 6007, 1024: 9001, 2048: 9001}


@pytest.mark.parametrize("block,n", [(B, N_OF[B]) for B in SI.BLOCK_ADAPT_SWEPT])
def test_masks_and_outputs_against_the_model(gpu, block, n):
    from gnss_sdr_rs_amd import excise
    B = block
    ex = excise.Excisor(B)
    p = EM.resolve(B)
    wa, ws = ex.windows()
    worst_p = worst_y = 0.0
    for fmt in ("i8", "c32"):
        x = _moving(fmt, n, B, 3 + B)
        for factor in (16.0, 6.0):
            for guard in (0, 2, 16):
                ex.set_block_adapt(factor, guard)
                perr, yerr, M = _one_case(ex, p, x, factor, guard, wa, ws, None, (B, fmt, factor, guard))
                worst_p, worst_y = max(worst_p, perr), max(worst_y, yerr)
                zeroed = (M == 0).sum(axis=1)
                assert (zeroed >= 1).all()                                                # the CW is in every block
                first = np.array([np.flatnonzero(r == 0)[0] for r in M[2:-1]])
                assert len(set(first.tolist())) >= min(len(first), 4)                     # and it moves: the masks differ
    # both gains multiply: random static gains under the masks
    rng = np.random.default_rng(B)
    g = rng.random(B).astype(np.float32)
    g[::17] = 0.0
    ex.set_gains(g)
    ex.set_block_adapt(0.0, 2)
    x = _moving("c32", n, B, 5)
    perr, yerr, M = _one_case(ex, p, x, 16.0, 2, wa, ws, g, (B, "static gains"))
    ones, _, _, _, _ = BM.run(p, x, 16.0, 2, masks=M, wa=wa, ws=ws)
    both, _, _, _, _ = BM.run(p, x, 16.0, 2, masks=M, wa=wa, ws=ws, gains=g)
    assert np.abs(ones - both).max() > 1.0                                                # the static gains matter
    print("B = %d: largest p error / bound %.3f, largest output error / bound %.3f" % (B, max(worst_p, perr), max(worst_y, yerr)))
    ex.close()


def test_masks_and_outputs_at_4096(gpu):
    _at_the_largest_block(4096, "i8")


@pytest.mark.parametrize("block,fmt", SI.BLOCK_ADAPT_TOP)
def test_masks_and_outputs_at_the_largest_block(gpu, block, fmt):
    """both formats (the case above is the int8 one under its earlier name)"""
    _at_the_largest_block(block, fmt)


def _at_the_largest_block(B, fmt):
    from gnss_sdr_rs_amd import excise
    ex = excise.Excisor(B).set_block_adapt(guard_bins=2)
    wa, ws = ex.windows()
    x = _moving(fmt, 12301, B, 11)
    perr, yerr, M = _one_case(ex, EM.resolve(B), x, 16.0, 2, wa, ws, None, (B, fmt))
    assert ((M == 0).sum(axis=1) >= 1).all()
    print("B = %d, %s: p error / bound %.3f, output error / bound %.3f" % (B, fmt, perr, yerr))
    ex.close()


SPLITS = (1, 7, None, 1000, 3001)          # None: H - 1


@pytest.mark.parametrize("block,fmt,n", [(1024, "i8", 6007), (256, "c32", 6007), (4096, "i8", 12301), (512, "i8", 6007),
                                         (2048, "c32", 9001)])
def test_the_words_and_counters_do_not_depend_on_the_cuts(gpu, hipbuf, block, fmt, n):
    from gnss_sdr_rs_amd import excise
    B, H = block, block // 2
    ex = excise.Excisor(B).set_block_adapt(6.0, 2)
    x = _moving(fmt, n, B, 7)
    d_x = hipbuf.upload(x)
    whole = _feed(hipbuf, ex, d_x, fmt, n)
    stats = ex.block_stats()
    assert stats["blocks"] == whole.size // H and stats["blocks_flagged"] >= stats["blocks"] - 2 and stats["bins_zeroed"] > stats["bins_flagged"] > 0
    for blocks in SPLITS:
        ex.reset(0)
        assert ex.block_stats() == dict.fromkeys(BM.COUNTERS, 0)                              # reset zeroes the counters
        got = _feed(hipbuf, ex, d_x, fmt, n, blocks or H - 1)
        assert (_words(got) == _words(whole)).all(), (B, blocks)
        assert ex.block_stats() == stats, (B, blocks)
    ex.reset(0)
    assert (_words(_feed(hipbuf, ex, d_x, fmt, n)) == _words(whole)).all() and ex.block_stats() == stats      # again: the same words
    ex.reset((1 << 32) - 3)
    far = _feed(hipbuf, ex, d_x, fmt, n)
    far_stats = ex.block_stats()
    assert far.size == EM.plan(B, (1 << 32) - 3, n) and far_stats["blocks"] == far.size // H
    ex.reset((1 << 32) - 3)
    assert (_words(_feed(hipbuf, ex, d_x, fmt, n, 1000)) == _words(far)).all() and ex.block_stats() == far_stats
    ex.close()


def test_off_is_off(gpu, hipbuf):
    from gnss_sdr_rs_amd import excise
    B, n = 1024, 6007
    rng = np.random.default_rng(2)
    g = rng.random(B).astype(np.float32)
    x = _moving("c32", n, B, 9)
    d_x = hipbuf.upload(x)
    fresh = excise.Excisor(B)
    fresh.set_gains(g)
    want = _feed(hipbuf, fresh, d_x, "c32", n)
    assert fresh.block_stats() == dict.fromkeys(BM.COUNTERS, 0)
    ex = excise.Excisor(B)
    ex.set_gains(g)
    ex.set_block_adapt(6.0, 2)
    on = _feed(hipbuf, ex, d_x, "c32", n)
    assert not (_words(on) == _words(want)).all()
    counted = ex.block_stats()
    ex.set_block_adapt(None)
    ex.reset(0)
    assert (_words(_feed(hipbuf, ex, d_x, "c32", n)) == _words(want)).all()
    assert ex.block_stats() == dict.fromkeys(BM.COUNTERS, 0) and counted["bins_zeroed"] > 0
    # in the mode, nothing flagged: the static handle's words, and the blocks are still counted
    for factor in (math.inf, 1e30):
        ex.set_block_adapt(factor, 16)
        ex.reset(0)
        assert (_words(_feed(hipbuf, ex, d_x, "c32", n)) == _words(want)).all(), factor
        assert ex.block_stats() == dict(blocks=want.size // (B // 2), blocks_flagged=0, bins_flagged=0, bins_zeroed=0)
    ex.close(); fresh.close()


def test_the_mask_is_taken_on_the_blanked_block(gpu):
    from gnss_sdr_rs_amd import excise
    B, n = 1024, 6007
    x = _moving("c32", n, B, 13)
    for s in (700, 1536, 2047, 2048, 4000):
        x[s] = 3000.0 + 0j
    ex = excise.Excisor(B, blank_threshold=100.0).set_block_adapt(guard_bins=2)
    p = EM.resolve(B, blank_threshold=100.0)
    wa, ws = ex.windows()
    perr, yerr, M = _one_case(ex, p, x, 16.0, 2, wa, ws, None, "blanked")
    assert ex.stats()["blanked"] == 5
    # without the blanking a spike lifts every bin of its blocks: the model's masks there are elsewhere
    _, _, P_plain, M_plain, _ = BM.run(EM.resolve(B), x, 16.0, 2, wa=wa, ws=ws)
    assert (M_plain != M).any(axis=1).sum() >= 4
    print("blanked: p error / bound %.3f, output error / bound %.3f" % (perr, yerr))
    ex.close()


BAD_CFGS = [(1.0, 0), (0.5, 0), (-16.0, 0), (math.nan, 0), (16.0, 17)]


def test_every_refusal_leaves_the_state_alone(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, excise
    L = gpu.lib()
    B, H, n = 1024, 512, 6007
    g = np.random.default_rng(4).random(B).astype(np.float32)
    x = _moving("c32", n, B, 15)
    d_x = hipbuf.upload(x)
    ex, twin = excise.Excisor(B), excise.Excisor(B)
    for h in (ex, twin):
        h.set_gains(g)
        h.set_block_adapt(6.0, 2)
    d_y = hipbuf.alloc(2 * n * 8, fill=0x5A)
    first = 2500
    n1 = ex.process_dev(d_x, _lib.FMT_C32, first, d_y, 2 * n)
    state = (ex.stats(), ex.block_stats())
    assert state[1]["blocks"] == n1 // H and state[1]["bins_zeroed"] > 0
    for factor, guard in BAD_CFGS:
        assert BM.resolve(factor, guard) is None
        with pytest.raises(_lib.GmError) as e:
            ex.set_block_adapt(factor, guard)
        assert e.value.status == INVALID, (factor, guard)
    bad = _lib.ExcisorBlockCfg(16.0, 2, (C.c_uint32 * 6)(0, 0, 0, 0, 1, 0))
    assert L.gm_excisor_set_block_adapt(ex._h, C.byref(bad)) == INVALID
    assert L.gm_excisor_set_block_adapt(None, None) == INVALID and L.gm_excisor_block_stats(None, None, None, None, None) == INVALID
    assert L.gm_excisor_block_capture(None, None, None, 0) == INVALID
    # a capture that cannot hold the call's blocks: refused before anything runs
    rest = n - first
    n2 = EM.plan(B, first, rest)
    d_p, d_m = hipbuf.alloc((n2 // H + 1) * B * 4, fill=0x5A), hipbuf.alloc((n2 // H + 1) * B, fill=0x5A)
    ex.block_capture(d_p, d_m, n2 // H)
    got = C.c_size_t(77)
    src = d_x + first * 8
    assert L.gm_excisor_process_dev(ex._h, src, _lib.FMT_C32, rest, d_y + n1 * 8, 2 * n, C.byref(got), None) == OUT_OF_RANGE
    assert got.value == 77 and (ex.stats(), ex.block_stats()) == state
    assert (hipbuf.download(d_y + n1 * 8, 64, np.uint8) == 0x5A).all() and (hipbuf.download(d_p, 64, np.uint8) == 0x5A).all()
    ex.block_capture(None, None, 0)
    # a capture armed with the mode off
    off = excise.Excisor(B)
    with pytest.raises(_lib.GmError) as e:
        off.block_capture(d_p, d_m, 100)
    assert e.value.status == INVALID
    off.block_capture(None, None, 0)                                                         # disarming is always allowed
    off.close()
    assert (_words(ex.gains()) == _words(g)).all() and (ex.stats(), ex.block_stats()) == state
    # the stream goes on as if nothing had been refused: the twin never saw a refusal
    twin.process_dev(d_x, _lib.FMT_C32, first, d_y, 2 * n)
    d_a, d_b = hipbuf.alloc(n2 * 8), hipbuf.alloc(n2 * 8)
    assert ex.process_dev(src, _lib.FMT_C32, rest, d_a, n2) == n2 and twin.process_dev(src, _lib.FMT_C32, rest, d_b, n2) == n2
    ex.synchronize(); twin.synchronize()
    assert (hipbuf.download(d_a, n2 * 8, np.uint32) == hipbuf.download(d_b, n2 * 8, np.uint32)).all()
    assert ex.block_stats() == twin.block_stats() and ex.block_stats()["blocks"] == (n1 + n2) // H
    ex.close(); twin.close()


def test_the_front_end_ring_path_picks_the_mode_up(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, excise, frontend, tracking
    F_IF, FS = 1.25e6, 8.0e6
    B, H = 256, 128
    ring = tracking.MulticastRingBuffer(1 << 13)
    fe, fe_ref = frontend.DigitalFrontend(F_IF, FS, FS), frontend.DigitalFrontend(F_IF, FS, FS)
    ex, ex_ref = excise.Excisor(B).set_block_adapt(6.0, 2), excise.Excisor(B).set_block_adapt(6.0, 2)
    calls = [3052, 2000]
    x = _moving("i8", sum(calls), B, 21)
    d_x = hipbuf.upload(x)
    d_mid, d_e = hipbuf.alloc(4096 * 8), hipbuf.alloc(4352 * 8)
    done = head = 0
    for n in calls:
        total = fe.write_ring(ring, x[done:done + n], excisor=ex)
        fe_ref.process_dev(d_x + done * 2, _lib.FMT_I8_IQ, d_mid, n)
        fe_ref.synchronize()
        got = ex_ref.process_dev(d_mid, _lib.FMT_C32, n, d_e, 4352)
        ex_ref.synchronize()
        ref = hipbuf.download(d_e, 4352 * 8, np.complex64)[:got]
        ring.flush()
        assert total == got and (_words(ring.copy_to_slice(head, got)) == _words(ref)).all(), n
        head += got
        done += n
    assert ex.block_stats() == ex_ref.block_stats() and ex.block_stats()["bins_zeroed"] > 0 and ex.block_stats()["blocks"] == head // H
    for h in (fe, fe_ref, ex, ex_ref, ring):
        h.close()


def test_the_ddc_ring_path_picks_the_mode_up(gpu):
    import ddc_model as DM
    from gnss_sdr_rs_amd import ddc, excise, tracking
    B, H = 256, 128
    ring = tracking.MulticastRingBuffer(1 << 13)
    d, d_ref = ddc.Ddc(DM.MIX, 1, 2), ddc.Ddc(DM.MIX, 1, 2)
    ex, ex_ref = excise.Excisor(B).set_block_adapt(6.0, 2), excise.Excisor(B).set_block_adapt(6.0, 2)
    calls = [4000, 3000]
    rng = np.random.default_rng(5)
    t = np.arange(sum(calls), dtype=np.float64)
    cycles = (DM.MIX + 0.02) * t + 0.5 * (1.0 / (B * B)) * t * t                                # 0.02 cycles a sample above the mix, moving
    x = np.clip(np.round(6.0 * rng.standard_normal(t.size) + 90.0 * np.cos(2 * np.pi * cycles)), -128, 127).astype(np.int8)
    done = head = 0
    for n in calls:
        total = d.write_ring(ring, x[done:done + n], excisor=ex)
        ref = ex_ref.process(d_ref.process(x[done:done + n]))
        ring.flush()
        assert total == ref.size and (_words(ring.copy_to_slice(head, ref.size)) == _words(ref)).all(), n
        head += ref.size
        done += n
    assert ex.block_stats() == ex_ref.block_stats() and ex.block_stats()["bins_zeroed"] > 0 and ex.block_stats()["blocks"] == head // H
    for h in (d, d_ref, ex, ex_ref, ring):
        h.close()


def test_a_swept_dwell_is_found_again(gpu, hipbuf):
    """The host test's swept scene (a CW 30 dB above the noise sweeping -800 .. +800 kHz over the dwell) through
    Excisor(1024).set_block_adapt(guard_bins=2), process and a plain search_dev: the true worker's best cell is (bin 2, 700); the same
    search of the jammed dwell misses."""
    from gnss_sdr_rs_amd import _lib, acquisition as A, excise
    x = BM.sweep_scene(2, 30.0)
    ex = excise.Excisor(1024).set_block_adapt(guard_bins=2)
    y = ex.process(x)
    st = ex.block_stats()
    print("per block: %s" % st)
    assert y.size >= EM.DWELL and st["blocks_flagged"] == st["blocks"] and 20 * st["blocks"] <= st["bins_zeroed"] <= 160 * st["blocks"]
    eng = A.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                              codes=EM.scene_codes(), code_rate=1.023e6)
    w = EM.SAT["worker"]
    d_y, d_x = hipbuf.upload(y[:EM.DWELL]), hipbuf.upload(x[:EM.DWELL])
    eng.search_dev(d_y, _lib.FMT_C32)
    excised = EM.best_cell(*eng.metrics(), w)
    eng.search_dev(d_x, _lib.FMT_C32)
    jammed = EM.best_cell(*eng.metrics(), w)
    print("GPU: jammed %s, excised %s" % (jammed, excised))
    assert EM.found(excised) and excised[2] >= 6.0
    assert not EM.found(jammed)
    eng.close()
    ex.close()
