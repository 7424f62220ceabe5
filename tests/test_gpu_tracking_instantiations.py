"""Every instantiation of the persistent tracking kernel against the oracle, at small shapes.

launch_trk_persistent compiles the sample code per key (arms 3 / 5) x (code index FAITHFUL / FIXED) x (plain / BOC(1,1)), each in a
default and a strict_libm form, plus the FAIR3 form of the three-arm keys.  Each key has its own chip tables — the padded float row
whose guard entries serve floor(phase) = -1, = len and = len + 1, and for BOC the half-chip table in front of it — its own block
width, prefetch scheme and exchange width.  tests/test_gpu_tracking_shapes.py runs three of the eight keys at BASELINE's shapes; this
file runs all of them, with the same comparisons (_compare: teacher-forced and free-running) and the same bars, unchanged:

  REL = 1e-5 of the prompt envelope, F64_REL = 5e-7 against the f64 accumulation, FREE_REL = 2.5e-5, final state words at 0 ulps.

At n <= 20 460 samples per sum the reference's sequential f32 summation noise (~eps/2 * sqrt(n/3) = 5e-6 at the largest n, 2e-6 at
n = 4096) is below REL, so no case needs a wider bar.

Custom +-1 codes are used for every key (they index row prn - 1 in both modes, so the mode changes the negative-phase rule only);
every code row has chips[0] != chips[len - 1], which is where FAITHFUL (floor = -1 reads chip 0) and FIXED (reads the last chip)
differ, and every case proves FROM THE ORACLE'S STATES ALONE that its late arms reach floor = -1 and its early arms floor = len.
"""
import numpy as np
import pytest

from test_gpu_tracking_shapes import (F64_REL, FREE_REL, REL, STRICT_F64_REL, STRICT_FREE_REL, _acq_result,
                                      _assert_bit_identical_free_running, _boc_scene, _compare)

pytestmark = pytest.mark.gpu

KEYS = [(arms, mode, boc) for arms in (3, 5) for mode in (0, 1) for boc in (False, True)]      # mode 0: FAITHFUL, 1: FIXED


def _key_id(k):
    return "%darms-%s-%s" % (k[0], "fixed" if k[1] else "faithful", "boc" if k[2] else "plain")


def _codes(n_rows, L, seed, second_differs=False):
    """random +-1 rows with chips[0] != chips[L - 1]; second_differs: chips[1] differs from chips[0] AND from chips[L - 1] instead,
    so that neither a read of chip 0 nor one of the last chip (the two values the front guard entry can hold) passes for chip 1"""
    c = np.where(np.random.default_rng(seed).integers(0, 2, (n_rows, L)) > 0, 1, -1).astype(np.int8)
    c[:, 0], c[:, L - 1] = 1, -1
    if second_differs:
        c[:, 1], c[:, L - 1] = -1, 1
    return c


def _recording(oracle, log):
    """oracle.TrackingChannel that notes (code_phase, code_rate, n) as it stands at the start of every teacher-forced epoch"""
    class Rec(oracle.TrackingChannel):
        def update_forced(self, ring, forced):
            log.append((np.float32(self.c.code_phase), np.float32(self.c.code_rate), int(self.c.num_samples_per_code)))
            return super().update_forced(ring, forced)
    return Rec


def _assert_guards_reached(log, fs, L, arms, el, vel):
    """early_late_correlation's chip phases (do_tracking.rs:252-255) restated in numpy f32 from the oracle's epoch-start states:
    over the run every late arm must see floor(phase) = -1 and every early arm floor(phase) = len at least once."""
    spaces = {"e/l": np.float32(el)}
    if arms == 5:
        spaces["ve/vl"] = np.float32(vel)
    below = dict.fromkeys(spaces, 0)
    above = dict.fromkeys(spaces, 0)
    assert log
    for cp, rate, n in log:
        step = np.float32(rate) / np.float32(fs)
        t = np.float32(cp) + np.arange(n, dtype=np.float32) * step
        chip = np.fmod(t, np.float32(L))
        assert chip.dtype == np.float32
        for k, s in spaces.items():
            below[k] += int((np.floor(chip - s) == -1).sum())
            above[k] += int((np.floor(chip + s) == L).sum())
    assert all(below.values()) and all(above.values()), (below, above)


def _custom_case(oracle, key, L, fs, rate, C, el, vel, E, seed, strict_libm=False, amp=0.6):
    """-> (mgr, ring, oring, starts, make_oracle, log): n_sats = min(C, 8) code rows in the air, channel i on row i % 8 from its
    own carrier offset (no two channels hold the same state)"""
    from gnss_sdr_rs_amd import tracking as T
    arms, mode, boc = key
    n = int(round(fs / (rate / L)))
    S = min(C, 8)
    codes = _codes(S, L, seed)
    assert (codes[:, 0] != codes[:, L - 1]).all()
    rng = np.random.default_rng(seed + 1)
    dopp = rng.uniform(-2000, 2000, S)
    cstart = rng.integers(0, 5000, S)
    x = _boc_scene(codes, fs, rate, L, (E + 1) * n + 5000, dopp, cstart, amp=amp, seed=seed + 2, boc=boc)
    ring, oring = T.MulticastRingBuffer(1 << 19), oracle.MulticastRingBuffer(1 << 19)
    assert x.size <= 1 << 19
    ring.write_samples(x)
    oring.write_samples(x)
    mgr = T.TrackingManager(fs, n_channels=C, n_arms=arms, code_index_mode=mode, early_late_space=el, very_early_late_space=vel,
                            boc11=boc, codes=codes, nominal_code_rate=rate, strict_libm=strict_libm)
    starts = [_acq_result(1 + i % S, float(dopp[i % S]) + 10.0 - 0.17 * (i // S), fs, int(cstart[i % S])) for i in range(C)]
    log = []
    Rec = _recording(oracle, log)

    def mk(i):
        return Rec(i, fs, code_index_mode=mode, n_arms=arms, el_space=el, vel_space=vel, boc11=boc, codes=codes, code_rate=rate)
    return mgr, ring, oring, starts, mk, log


# (name, L, fs, C, el, vel): n = 4096 and 16384 (multiples of the 512-lane workgroup), n = 5000 (not one); 3 channels (32 or 16
# workgroups per channel, most of them without a sample at n = 4096) and 40 (12 per channel); narrow arms and the defaults
SHAPES = [("L1023-n4096-C3", 1023, 4.096e6, 3, 0.25, 0.6),
          ("L1023-n5000-C40", 1023, 5.0e6, 40, 0.25, 0.6),
          ("L1023-n4096-C40-default-arms", 1023, 4.096e6, 40, 0.5, 1.0)]
SWEEP = [(k, s) for k in KEYS for s in SHAPES]
SWEEP += [((3, 1, True), ("L4092-n16384-C3", 4092, 4.096e6, 3, 0.25, 0.6)), ((5, 0, True), ("L4092-n16384-C3", 4092, 4.096e6, 3, 0.25, 0.6))]


@pytest.mark.parametrize("key,shape", SWEEP, ids=[_key_id(k) + "-" + s[0] for k, s in SWEEP])
def test_key_sweep_custom_codes(gpu, oracle, key, shape):
    """A1: all eight keys through _compare at the project's own bars, 8 epochs."""
    name, L, fs, C, el, vel = shape
    E = 8
    mgr, ring, oring, starts, mk, log = _custom_case(oracle, key, L, fs, 1.023e6, C, el, vel, E, seed=1000 + 100 * KEYS.index(key) + C + L)
    w = _compare(mgr, ring, oring, starts, mk, key[0], E, E)
    print("key sweep", _key_id(key), name, w)
    assert len(log) == C * E
    _assert_guards_reached(log, fs, L, key[0], el, vel)
    mgr.close(); ring.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_key_sweep_builtin_ca_table(gpu, oracle, mode):
    """A1: the two plain three-arm keys on the built-in C/A table at n = 4096 (FAITHFUL reads row `prn`, FIXED row prn - 1), with
    PRNs whose row starts and ends on different chips."""
    from gnss_sdr_rs_amd import tracking as T, synth
    fs, n, E = 4.096e6, 4096, 8
    t = oracle.ca_code_table()
    row_of = (lambda p: p) if mode == 0 else (lambda p: p - 1)
    prns = [p for p in range(1, 32) if t[row_of(p)][0] != t[row_of(p)][1022]][:3]
    assert len(prns) == 3
    sc = synth.tracking_scene(t, fs, 0.0, prns, E + 2, config_id=81, cn0=50.0, code_rows=[row_of(p) for p in prns])
    x = synth.to_c32(sc["x"])
    ring, oring = T.MulticastRingBuffer(1 << 16), oracle.MulticastRingBuffer(1 << 16)
    ring.write_samples(x[:(E + 2) * n])
    oring.write_samples(x[:(E + 2) * n])
    mgr = T.TrackingManager(fs, n_channels=3, code_index_mode=mode)
    starts = [_acq_result(s["prn"], s["doppler_hz"] + 10.0, fs, s["code_start"]) for s in sc["sats"]]
    log = []
    Rec = _recording(oracle, log)
    w = _compare(mgr, ring, oring, starts, lambda i: Rec(i, fs, code_index_mode=mode), 3, E, E)
    print("key sweep C/A mode", mode, w)
    _assert_guards_reached(log, fs, 1023, 3, 0.5, 1.0)
    mgr.close(); ring.close()


@pytest.mark.parametrize("key", KEYS, ids=[_key_id(k) for k in KEYS])
def test_strict_libm_forms(gpu, oracle, key):
    """A2: the <.., STRICT = 1> instantiation of every key (n = 5000, 3 channels), teacher-forced: identical per-sample products, so
    the sums sit within the tree sum's own error of their f64 accumulation (STRICT_F64_REL)."""
    L, fs, el, vel, E = 1023, 5.0e6, 0.25, 0.6, 8
    mgr, ring, oring, starts, mk, log = _custom_case(oracle, key, L, fs, 1.023e6, 3, el, vel, E, seed=2000 + KEYS.index(key), strict_libm=True)
    w = _compare(mgr, ring, oring, starts, mk, key[0], E, E, rel=REL, free_rel=STRICT_FREE_REL)
    print("strict_libm", _key_id(key), w)
    assert w["f64"] <= STRICT_F64_REL, w
    _assert_guards_reached(log, fs, L, key[0], el, vel)
    mgr.close(); ring.close()


@pytest.mark.parametrize("key", KEYS, ids=[_key_id(k) for k in KEYS])
def test_strict_libm_and_sum_order_bit_identical(gpu, oracle, key):
    """A2: strict_libm + strict_sum_order (launch_trk_epoch's serial path, run-time flags) for every (arms, mode, boc): 6 epochs
    free-running, 3 channels, every sum and every state word equal to the oracle's bit for bit."""
    from gnss_sdr_rs_amd import tracking as T
    arms, mode, boc = key
    L, fs, rate, el, vel, E, C = 1023, 5.0e6, 1.023e6, 0.25, 0.6, 6, 3
    n = 5000
    codes = _codes(C, L, 3000 + KEYS.index(key))
    rng = np.random.default_rng(3100 + KEYS.index(key))
    dopp = rng.uniform(-2000, 2000, C)
    cstart = rng.integers(0, 5000, C)
    x = _boc_scene(codes, fs, rate, L, (E + 1) * n + 5000, dopp, cstart, seed=3200, boc=boc)
    ring, oring = T.MulticastRingBuffer(1 << 16), oracle.MulticastRingBuffer(1 << 16)
    ring.write_samples(x)
    oring.write_samples(x)
    mgr = T.TrackingManager(fs, n_channels=C, n_arms=arms, code_index_mode=mode, early_late_space=el, very_early_late_space=vel,
                            boc11=boc, codes=codes, nominal_code_rate=rate, strict_libm=True, strict_sum_order=True)
    starts = [_acq_result(c + 1, float(dopp[c]) + 10.0, fs, int(cstart[c])) for c in range(C)]
    _assert_bit_identical_free_running(
        mgr, ring, oring, starts,
        lambda i: oracle.TrackingChannel(i, fs, code_index_mode=mode, n_arms=arms, el_space=el, vel_space=vel, boc11=boc, codes=codes,
                                         code_rate=rate), arms, E)
    mgr.close(); ring.close()


def test_fair3_form_three_arm_boc(gpu, oracle):
    """A3: 257 channels x 8 Msps leave one workgroup per channel and 15 rows of samples per lane, the geometry at which the launcher
    takes the FAIR3 instantiation (test_channel_count_sweep_covers_every_G reaches it for the plain FIXED key): here for the
    three-arm FIXED BOC key."""
    key, L, fs, C, el, vel, E = (3, 1, True), 1023, 8.0e6, 257, 0.25, 0.6, 6
    mgr, ring, oring, starts, mk, log = _custom_case(oracle, key, L, fs, 1.023e6, C, el, vel, E, seed=4000)
    w = _compare(mgr, ring, oring, starts, mk, 3, E, E)
    print("FAIR3 3 arms BOC", w)
    _assert_guards_reached(log, fs, L, 3, el, vel)
    mgr.close(); ring.close()


@pytest.mark.parametrize("arms", [3, 5])
def test_l5_length_code(gpu, oracle, arms):
    """A5: 10 230 chips at 10.23 Mcps and 20.46 Msps (n = 20 460), the L5 / E5a geometry: a 40 KB padded row in dynamic LDS."""
    key, L, fs, rate, C, el, vel, E = (arms, 1, False), 10230, 20.46e6, 10.23e6, 3, 0.5, 1.0, 4
    mgr, ring, oring, starts, mk, log = _custom_case(oracle, key, L, fs, rate, C, el, vel, E, seed=5000 + arms)
    assert int(round(fs / (rate / L))) == 20460
    w = _compare(mgr, ring, oring, starts, mk, arms, E, E)
    print("L = 10230,", arms, "arms", w)
    _assert_guards_reached(log, fs, L, arms, el, vel)
    mgr.close(); ring.close()


# ------------------------------------------------------------------------------------------ A4: a power-of-two code length
# chip_idx < len and a spacing of 1.0 do NOT keep floor(chip_idx + 1.0) at len or below in f32 when len = 2^k: with
# chip_idx = nextbelow(len) the sum's exact value len + 1 - ulp/2 lies halfway between two floats of the next binade and rounds (to
# even) to len + 1.  The reference's `% len` then reads chip 1.
POW2_CASES = [(5, 0, False), (5, 0, True), (5, 1, False), (5, 1, True), (3, 0, False), (3, 0, True), (3, 1, False), (3, 1, True)]


def _pow2_case(oracle, key):
    """L = 1024 at 2.048 Msps and 1.024 Mcps (n = 2048, half a chip per sample).  One satellite per channel whose code runs a quarter
    chip behind the replica started at code_phase = nextbelow(1024), so that every sample's prompt chip is the one in the air; the
    ring sample under replica sample 0 — the only one whose outermost early arm has floor(phase) = 1025 — is 60 + 60j.
    ONE epoch: at exactly half a chip per sample every sample sits on a half-chip edge, so from the second epoch on an oracle that
    runs free of the device (a code rate one ulp apart) reads other chips on half of the samples — the geometry's own property, not
    the kernel's; the epoch that holds the case is the first, which both comparisons enter with the same state."""
    arms, mode, boc = key
    L, fs, rate, C, E = 1024, 2.048e6, 1.024e6, 3, 1
    n = 2048
    el, vel = (0.5, 1.0) if arms == 5 else (1.0, 1.0)
    cp0 = np.nextafter(np.float32(1024), np.float32(0))
    assert np.floor(cp0 + np.float32(1.0)) == 1025            # the rounding this case is about
    codes = _codes(C, L, 6000 + POW2_CASES.index(key), second_differs=True)
    assert (codes[:, 0] != codes[:, 1]).all() and (codes[:, L - 1] != codes[:, 1]).all()
    rng = np.random.default_rng(6100 + POW2_CASES.index(key))
    dopp = rng.uniform(-2000, 2000, C)
    cstart = rng.integers(100, 3000, C)
    while len(set(int(c) for c in cstart)) < C:
        cstart = rng.integers(100, 3000, C)
    x = _boc_scene(codes, fs, rate, L, (E + 1) * n + 3000, dopp, cstart + 0.5, seed=6200, boc=boc)
    for c in cstart:
        x[int(c)] = 60.0 + 60.0j
    starts = [_acq_result(c + 1, float(dopp[c]) + 10.0, fs, int(cstart[c])) for c in range(C)]
    kw = dict(n_arms=arms, code_index_mode=mode, early_late_space=el, very_early_late_space=vel, boc11=boc, codes=codes,
              nominal_code_rate=rate)

    class Orc(oracle.TrackingChannel):
        def start(self, r):
            super().start(r)
            self.c.code_phase = float(cp0)

    def mk(i):
        return Orc(i, fs, code_index_mode=mode, n_arms=arms, el_space=el, vel_space=vel, boc11=boc, codes=codes, code_rate=rate)

    # the test cannot miss a wrong chip there: sample 0 alone (a one-hot period) through the oracle, with chip 1 as it is and flipped
    outer = 6 if arms == 5 else 2                                  # very-early (five arms) / early (three arms, spacing 1.0) sums
    flipped = codes.copy()
    flipped[:, 1] = -flipped[:, 1]
    for c in range(C):
        seg = np.zeros(n, np.complex64)
        seg[0] = x[int(cstart[c])]
        sums = []
        for tab in (codes, flipped):
            oc = oracle.TrackingChannel(c, fs, code_index_mode=mode, n_arms=arms, el_space=el, vel_space=vel, boc11=boc, codes=tab, code_rate=rate)
            oc.start(starts[c])
            oc.c.code_phase = float(cp0)
            sums.append(oc.early_late_correlation_ex(seg)[0])
        full = mk(c)
        full.start(starts[c])
        ref = full.early_late_correlation_ex(x[int(cstart[c]):int(cstart[c]) + n])[0]
        env = float(np.hypot(ref[0], ref[1]))
        assert env > 100.0
        moved = float(np.max(np.abs(sums[0][outer:outer + 2] - sums[1][outer:outer + 2])))
        assert moved > 100.0 * REL * env, (c, moved, env)
        others = [k for k in range(2 * arms) if k not in (outer, outer + 1)]
        assert np.array_equal(sums[0][others], sums[1][others])     # and no other arm reads chip 1 at that sample
    return dict(L=L, fs=fs, n=n, C=C, E=E, arms=arms, kw=kw, starts=starts, mk=mk, x=x, cp0=cp0, cstart=cstart)


class _StartAt:
    """a manager whose channels are put at a code phase right after start() (what _compare calls)"""
    class _Ch:
        def __init__(self, ch, cp):
            self._ch, self._cp = ch, cp

        def start(self, r):
            self._ch.start(r)
            self._ch.set_state(code_phase=float(self._cp))

        @property
        def state(self):
            return self._ch.state

    def __init__(self, mgr, cp):
        self._m = mgr
        self.channels = [self._Ch(c, cp) for c in mgr.channels]

    def update_all(self, ring, epochs):
        return self._m.update_all(ring, epochs)


@pytest.mark.parametrize("form", ["update_all", "strict_libm"])
@pytest.mark.parametrize("key", POW2_CASES, ids=[_key_id(k) for k in POW2_CASES])
def test_power_of_two_code_length_persistent(gpu, oracle, key, form):
    """A4: the persistent kernel's fast form (correlate_block_fast, through the padded tables) and its strict_libm form
    (correlate_sample<FAST = true>, through chip_index_arm) at floor(phase) = len + 1.  Both at REL and at F64_REL (inside
    _compare).  STRICT_F64_REL is not applied to the strict form here: it was measured on configs[2]'s 47 dB-Hz scene, and this one
    is 2048 samples of sigma-8 noise with three 85-unit samples in it under an envelope of ~1000, where a tree sum of the identical
    products sits up to 3.0e-7 from their f64 accumulation (5arms-faithful-plain; the default form of the same case 1.2e-7)."""
    from gnss_sdr_rs_amd import tracking as T
    p = _pow2_case(oracle, key)
    ring, oring = T.MulticastRingBuffer(1 << 14), oracle.MulticastRingBuffer(1 << 14)
    ring.write_samples(p["x"])
    oring.write_samples(p["x"])
    strict = form == "strict_libm"
    mgr = T.TrackingManager(p["fs"], n_channels=p["C"], strict_libm=strict, **p["kw"])
    w = _compare(_StartAt(mgr, p["cp0"]), ring, oring, p["starts"], p["mk"], p["arms"], p["E"], p["E"],
                 rel=REL, free_rel=STRICT_FREE_REL if strict else FREE_REL)
    print("2^k chips", form, _key_id(key), w)
    mgr.close(); ring.close()


@pytest.mark.parametrize("key", POW2_CASES, ids=[_key_id(k) for k in POW2_CASES])
def test_power_of_two_code_length_unit_entry(gpu, oracle, key):
    """A4: early_late_correlation on the same samples (trk_correlate_kernel, whose fast form indexes through chip_index_arm)."""
    from gnss_sdr_rs_amd import tracking as T
    p = _pow2_case(oracle, key)
    mgr = T.TrackingManager(p["fs"], n_channels=p["C"], **p["kw"])
    nv = 2 * p["arms"]
    for c in range(p["C"]):
        ch, oc = mgr.channels[c], p["mk"](c)
        ch.start(p["starts"][c])
        ch.set_state(code_phase=float(p["cp0"]))
        oc.start(p["starts"][c])
        seg = p["x"][int(p["cstart"][c]):int(p["cstart"][c]) + p["n"]]
        got = np.array(ch.early_late_correlation(seg), np.float32)
        want, want64 = oc.early_late_correlation_ex(seg)
        env = float(np.hypot(want[0], want[1]))
        e1 = float(np.max(np.abs(got - want[:nv]))) / env
        e64 = float(np.max(np.abs(got - want64[:nv]))) / env
        print("2^k chips unit entry", _key_id(key), c, e1, e64)
        assert env > 100.0 and e1 <= REL, (c, e1, got, want[:nv])
        assert e64 <= F64_REL, (c, e64)
        assert ch.state.code_phase == oc.c.code_phase and ch.state.carrier_phase == oc.c.carrier_phase
    mgr.close()


# ------------------------------------------------------------------------------------------ D: codes the kernel cannot hold
def test_create_refuses_a_code_beyond_the_lds_limit(gpu):
    """gm_trk_create reads the persistent kernel's static LDS and the device's per-workgroup limit and refuses a code whose padded
    tables do not fit beside it (GM_ERR_OUT_OF_RANGE, the limit in the message) — at create, nothing is launched.  The L5 / E5a
    length is accepted."""
    from gnss_sdr_rs_amd import tracking as T, _lib
    for L, boc in ((100000, False), (60000, True)):              # 400 KB / 720 KB of tables: beyond any CU's 160 KB
        with pytest.raises(_lib.GmError) as ei:
            T.TrackingManager(4.0e6, n_channels=1, code_index_mode=1, codes=np.ones((1, L), np.int8), boc11=boc, n_arms=5)
        assert ei.value.status == -5 and "LDS" in str(ei.value) and "bytes" in str(ei.value), ei.value
    for arms in (3, 5):
        T.TrackingManager(20.46e6, n_channels=3, n_arms=arms, code_index_mode=1, codes=np.ones((3, 10230), np.int8), nominal_code_rate=10.23e6).close()
