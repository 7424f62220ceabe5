"""The ring, the channel table and the coverage rules of the off-signal tracking tests (tests/test_gpu_tracking_off_signal.py on the
device, tests/test_tracking_off_signal_host.py on the oracle alone).

One ring of 2^19 samples, L = 1023, fs = 4.096 Msps (n = 4096 at the nominal rate), 40 channels, 12 epochs:

  [NOISE_AT, +16 n)   unit-variance complex noise.  25 channels run here from staggered starts; the power of a prompt sum is ~4096,
                      far above LOCK_THRESHOLD = 15, so an epoch is "locked" on nothing (all but 0.4 % of them: P(power < 15) = 15 / 4096): atan sees a uniformly distributed angle,
                      the DLL random envelopes, and both loops integrate garbage.  13 of them (a third of the 40) start with
                      code_rate a few ulps from a rate at which round(fs / (rate / len)) changes, so the epoch length changes
                      during the run and both the spc_rate_bounds shortcut and the definition are taken.
  [WEAK_AT, +21 n)    noise at sigma = 1e-3 (power ~4e-3: never locked), longer than MAX_LOST_EPOCHS periods.  4 channels run here;
                      12 epochs cannot count to 20 from zero, so they start with lost_counter 10, 12, 14, 16 (set_state) and give up
                      in epochs 9, 7, 5, 3 — inside a multi-epoch launch, next to channels that carry on.
  [CRAFT_AT, +33 n)   one-hot epochs: window w holds one sample a + jb at its first index and zeros elsewhere.  11 channels start at
                      windows 0, 2, .., 20 with carrier_freq = 0: in a channel's first TWO epochs the carrier phase at the window's
                      first sample is exactly 0 (cos = 1, sin = 0 in every sincos form), so the prompt sums are +-a, +-b exactly and
                      q / i is b / a: window 2c carries class c with q / i > 0, window 2c + 1 the same class with q / i < 0.  Classes:
                      |q/i| = 2^-30 (below 2^-29), one ulp below and exactly at each of 7/16, 11/16, 19/16, 39/16, 2^26 (above
                      2^25), and i = 0 exactly (q / i = +-inf, atan = +-pi/2).  |a|, |b| lie in [2^-30, 2^30] (a = 0 for the last class)
                      and a^2 + b^2 > 15, so every window is locked.  With one non-zero sample the early and late envelopes are equal,
                      the DLL error is exactly 0 and the epoch length stays 4096, so the windows stay aligned.  From its third epoch on
                      a channel meets the later windows under its own carrier phase: large and tiny values at arbitrary angles.

0/0 is left out: a locked epoch has power > 15, so q / i = 0 / 0 cannot occur in a locked epoch, and no NaN state is constructed.
"""
import numpy as np

import device_math_sets as S

F32 = np.float32
L, FS, RATE, N0, C, E = 1023, 4.096e6, 1.023e6, 4096, 40, 12
RING = 1 << 19
LOCK_THRESHOLD, MAX_LOST_EPOCHS = 15.0, 20
NOISE_AT, WEAK_AT, CRAFT_AT = 0, 16 * N0, 37 * N0
N_WINDOWS = 33
TOTAL = CRAFT_AT + (N_WINDOWS + 1) * N0
PLAIN, BOUNDARY, WEAK, CRAFT = range(0, 12), range(12, 25), range(25, 29), range(29, 40)
THRESHOLDS = [7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16]
CRAFT_CLASSES = ["below 2^-29"] + [s % t for t in ("7/16", "11/16", "19/16", "39/16") for s in ("just below %s", "at %s")] + \
                ["above 2^25", "i = 0"]
FEW_ULPS = 4


def _below(v):
    return float(np.nextafter(F32(v), F32(0)))


def crafted_values():
    """(a, b) of the 11 classes, q / i = b / a > 0; the divisions are by powers of two, hence exact"""
    v = [(2.0 ** 10, 2.0 ** -20)]
    for k, t in enumerate(THRESHOLDS):
        scale = 2.0 ** (4 + 6 * k)                       # a = 16, 2^10, 2^16, 2^22: b / a is exact at every scale
        v += [(scale, _below(t) * scale), (scale, t * scale)]
    v += [(2.0 ** -10, 2.0 ** 16), (0.0, 2.0 ** 30)]
    return v


def ring_samples(seed=20260):
    rng = np.random.default_rng(seed)
    x = np.zeros(TOTAL, np.complex64)
    k = WEAK_AT - NOISE_AT
    x[NOISE_AT:WEAK_AT] = ((rng.standard_normal(k) + 1j * rng.standard_normal(k)) * np.sqrt(0.5)).astype(np.complex64)
    k = CRAFT_AT - WEAK_AT
    x[WEAK_AT:CRAFT_AT] = ((rng.standard_normal(k) + 1j * rng.standard_normal(k)) * (1.0e-3 * np.sqrt(0.5))).astype(np.complex64)
    vals = crafted_values()
    for w in range(N_WINDOWS):
        if w < 2 * len(vals):
            a, b = vals[w // 2]
            b = -b if w % 2 else b
        else:                                            # behind the classes: magnitudes over the whole admitted range
            a, b = rng.choice([-1.0, 1.0], 2) * 2.0 ** rng.uniform(-30, 30, 2)
            if a * a + b * b <= 2 * LOCK_THRESHOLD:
                a = 8.0
        assert a * a + b * b > LOCK_THRESHOLD and all(v == 0 or 2.0 ** -30 <= abs(v) <= 2.0 ** 30 for v in (a, b))
        x[CRAFT_AT + w * N0] = a + 1j * b
    assert x.size <= RING
    return x


def boundary_rates():
    """13 code rates within a few ulps of the rates at which the epoch length steps 4097 -> 4096 and 4096 -> 4095"""
    out = []
    for n_hi in (4097.0, 4096.0):
        lo, hi = int(S.bits(F32(RATE - 400.0))[0]), int(S.bits(F32(RATE + 400.0))[0])
        while hi - lo > 1:                               # largest rate (as a bit pattern) that still gives n_hi
            mid = (lo + hi) // 2
            if S.spc_definition_np(FS, S.from_bits(np.array([mid], np.uint32)), L)[0] >= n_hi:
                lo = mid
            else:
                hi = mid
        assert S.spc_definition_np(FS, S.from_bits(np.array([lo, hi], np.uint32)), L).tolist() == [n_hi, n_hi - 1]
        out.append(lo)
    rates = []
    for j in range(len(BOUNDARY)):
        rates.append(float(S.from_bits(np.array([out[j % 2] + (j // 2) - 3], np.uint32))[0]))
    return rates


def channel_table(n_prn):
    """-> per channel dict(prn, start (acquisition hand-over), code_rate or None, lost_counter or None); n_prn: code rows in use"""
    rng = np.random.default_rng(977)
    rates = boundary_rates()
    lost0 = [10, 12, 14, 16]
    tab = []
    for i in range(C):
        d = dict(prn=1 + i % n_prn, code_rate=None, lost_counter=None)
        if i in PLAIN or i in BOUNDARY:
            d["idx"], d["freq"] = NOISE_AT + 113 * i, float(rng.uniform(-2000, 2000))
            if i in BOUNDARY:
                d["code_rate"] = rates[i - BOUNDARY[0]]
        elif i in WEAK:
            d["idx"], d["freq"], d["lost_counter"] = WEAK_AT + 101 * (i - WEAK[0]), float(rng.uniform(-2000, 2000)), lost0[i - WEAK[0]]
        else:
            d["idx"], d["freq"] = CRAFT_AT + 2 * (i - CRAFT[0]) * N0, 0.0
        tab.append(d)
    return tab


def acq_result(d):
    return dict(prn=d["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=d["freq"], fs=FS, mag_relative=10.0,
                sample_global_index=d["idx"], doppler_bin=0)


def spc(rate):
    return int(S.spc_definition_np(FS, [rate], L)[0])


def start_oracle(oc, d):
    oc.start(acq_result(d))
    if d["code_rate"] is not None:
        oc.c.code_rate = d["code_rate"]
        oc.c.num_samples_per_code = spc(d["code_rate"])
    if d["lost_counter"] is not None:
        oc.c.lost_counter = d["lost_counter"]


def start_device(ch, d):
    ch.start(acq_result(d))
    kw = {}
    if d["code_rate"] is not None:
        kw.update(code_rate=d["code_rate"], num_samples_per_code=spc(d["code_rate"]))
    if d["lost_counter"] is not None:
        kw.update(lost_counter=d["lost_counter"])
    if kw:
        ch.set_state(**kw)


# ------------------------------------------------------------------------------------------------ the oracle's record and its coverage
def before(oc):
    return dict(lost=int(oc.c.lost_counter), n=int(oc.c.num_samples_per_code), rate=F32(oc.c.code_rate))


def coverage(records):
    """records: per channel a list of dict(before = before(oc), rc, sums (the six sums the loops consumed), lost (bool)) of the epochs
    the oracle processed.  Everything below is restated from those in numpy f32, in the epilogue's order of operations."""
    atan = np.zeros(8, np.int64)
    crafted = {(k, s): 0 for k in CRAFT_CLASSES for s in "+-"}
    dll = {"+": 0, "-": 0, "0": 0}
    n_changes = resets_from_19 = locked = unlocked = 0
    for rec in records:
        ns = [r["before"]["n"] for r in rec]
        n_changes += sum(1 for p, q in zip(ns, ns[1:]) if p != q)
        for r in rec:
            ip, qp, ie, qe, il, ql = [F32(v) for v in r["sums"]]
            if not (ip * ip + qp * qp > F32(LOCK_THRESHOLD)):
                unlocked += 1
                if r["before"]["lost"] == MAX_LOST_EPOCHS - 1:
                    assert r["lost"], "lost_counter 19 and an unlocked epoch, but no reset"
                    resets_from_19 += 1
                continue
            locked += 1
            with np.errstate(divide="ignore"):
                ratio = qp / ip
            assert not np.isnan(ratio)
            atan[int(S.atan_class(np.array([ratio], F32))[0])] += 1
            sign = "-" if np.signbit(ratio) else "+"
            ab = np.abs(ratio)
            if 0 < ab < F32(2.0 ** -29):
                crafted[("below 2^-29", sign)] += 1
            if np.isinf(ab):
                assert ip == 0
                crafted[("i = 0", sign)] += 1
            elif ab >= F32(2.0 ** 25):
                crafted[("above 2^25", sign)] += 1
            for t, name in zip(THRESHOLDS, ("7/16", "11/16", "19/16", "39/16")):
                d = int(S.bits(ab)[0]) - int(S.bits(F32(t))[0])
                if -FEW_ULPS <= d < 0:
                    crafted[("just below " + name, sign)] += 1
                elif 0 <= d <= FEW_ULPS:
                    crafted[("at " + name, sign)] += 1
            pe, pl = np.sqrt(ie * ie + qe * qe), np.sqrt(il * il + ql * ql)
            dll["+" if pe > pl else ("-" if pe < pl else "0")] += 1
    return dict(atan=dict(zip(S.ATAN_CLASSES, atan.tolist())), crafted=crafted, dll=dll, n_changes=n_changes, resets_from_19=resets_from_19,
                locked=locked, unlocked=unlocked)


def assert_coverage(cov):
    for k in S.ATAN_CLASSES[1:6]:                                      # atan's five finite-interval classes
        assert cov["atan"][k] >= 20, cov["atan"]
    missing = [k for k, v in cov["crafted"].items() if v < 1]
    assert not missing, missing
    assert cov["n_changes"] >= 3, cov["n_changes"]
    assert cov["dll"]["+"] >= 1 and cov["dll"]["-"] >= 1, cov["dll"]
    assert cov["resets_from_19"] >= 1, cov


def summary(cov):
    return "atan %s; crafted classes reached %d of %d; epoch length changed %d times; dll_err +%d / -%d / 0: %d; resets from 19: %d; " \
           "locked %d, unlocked %d" % (cov["atan"], sum(1 for v in cov["crafted"].values() if v), len(cov["crafted"]), cov["n_changes"],
                                      cov["dll"]["+"], cov["dll"]["-"], cov["dll"]["0"], cov["resets_from_19"], cov["locked"], cov["unlocked"])


# ------------------------------------------------------------------------------------------------ the arrangements under test
def codes_for(key):
    """eight random +-1 rows with chips[0] != chips[L - 1] (where FAITHFUL and FIXED differ), as in test_gpu_tracking_instantiations.py"""
    arms, mode, boc = key
    c = np.where(np.random.default_rng(8800 + 10 * arms + 2 * mode + int(boc)).integers(0, 2, (8, L)) > 0, 1, -1).astype(np.int8)
    c[:, 0], c[:, L - 1] = 1, -1
    return c


KEY_A, KEY_B = (3, 1, False), (5, 0, True)           # (arms, mode, boc): (3, FIXED, plain) and (5, FAITHFUL, BOC)
EL, VEL = 0.25, 0.6


def make_oracle(oracle, key):
    """-> (factory(i), n_prn): key None is the built-in C/A table, three arms, FIXED (the do_work form)"""
    if key is None:
        return (lambda i: oracle.TrackingChannel(i, FS, code_index_mode=1)), 31
    arms, mode, boc = key
    codes = codes_for(key)
    return (lambda i: oracle.TrackingChannel(i, FS, code_index_mode=mode, n_arms=arms, el_space=EL, vel_space=VEL, boc11=boc, codes=codes,
                                             code_rate=RATE)), 8
