"""The run-time choice between the exact fast forms and the general forms of the tracked-state kernels, as data: the two predicates of
csrc/trk_kernels.hip restated in numpy float32, every (kernel, instantiation, class) that can be launched, and the records that reach
each of them.

A helper module like array_prompt_classes.py and stage_instantiations.py, not a test.  Shared by tests/test_trk_form_classes_host.py
(CPU: the literals against the source, every case in the class it is named for, every row with a case, what the older records reach,
the triggers the entries refuse) and by the GPU files test_gpu_trk_bank.py, test_gpu_array_prompt_classes.py and
test_gpu_trk_planes.py, which build their records from TRIGGERS.

The predicates, restated without reading the file (every operation rounded to f32 where the device rounds it):

  fast_code_ok   n < 2^24 and 0 <= code_phase < len and 0 <= step and fl(fl(n) step) < fl(1.99 len), step = fl(code_rate / fs), and both
                 arm spacings of the HANDLE in (0, 1]
  fast_car_ok    the significand of fs is not all ones and 1 < fs < 1e12 and (w = 0 or 1e-12 < |w| < 1e12) and
                 fl(|carrier_phase| + fl(|w| fl(fl(n) fl(1 / fs)))) < 1e5, w = fl(fl(2 pi) f), f = carrier_freq or fl(carrier_freq + df)

  gm_trk_bank            trk_bank_kernel<TG> takes trk_bank_body<TG, FASTC = fast_code_ok>; per carrier offset the division is the exact
                         fast form where FASTC and fast_car_ok hold.  TG = 1, 4, 8, 16 for T <= 1, 4, 8, more.
  gm_trk_array_prompts   trk_array_kernel<FMT, A, LC> takes ta_ref_image<FASTC>, the same two tests; a launch class is a
                         (format, A, L, pointer form) of array_prompt_classes.launches().
  gm_trk_update_planes   trk_planes_kernel<ARMS> takes correlate_sample<ARMS, FAST>, FAST = both tests at once (fast_code_range).
With the code test false the carrier takes the general division whatever its own test says; a class is still the pair of tests."""
import numpy as np

import array_prompt_classes as AC

F32 = np.float32
FAST, GENERAL = "fast", "general"
FORMS = [(c, k) for c in (FAST, GENERAL) for k in (FAST, GENERAL)]       # (code, carrier)

# ---- the literals of the two predicates, in the order the source writes them ----------------------------------------------------------------
N_EXACT = 1 << 24                    # sample indices are exact as floats below it
SPAN = F32(1.99)                     # n step < 1.99 len: one conditional subtraction suffices
SPACE_MIN, SPACE_MAX = F32(0.0), F32(1.0)      # an arm spacing in (0, 1]
MANTISSA = 0x7fffff                  # fs with all of these set: the reciprocal form is not the rounded quotient
FS_MIN, FS_MAX = F32(1.0), F32(1.0e12)
W_MIN, W_MAX = F32(1.0e-12), F32(1.0e12)
PHASE_MAX = F32(1.0e5)               # the fast sin / cos admits |phase| below it
LITERALS = {
    "fast_code_ok": [float(N_EXACT), 0.0, 0.0, float(SPAN), float(SPACE_MIN), float(SPACE_MAX), float(SPACE_MIN), float(SPACE_MAX)],
    "fast_car_ok": [float(MANTISSA), float(MANTISSA), float(FS_MIN), float(FS_MAX), 0.0, float(W_MIN), float(W_MAX), float(PHASE_MAX)],
}

LEN, RATE = 1023, 1.023e6


def handle(fs, code_len=LEN, early_late_space=0.5, very_early_late_space=1.0, **_):
    """what gm_trk_create makes of a configuration: a spacing of 0 takes its default"""
    return dict(fs=F32(fs), lenf=F32(code_len), el=F32(early_late_space if early_late_space > 0 else 0.5),
                vel=F32(very_early_late_space if very_early_late_space > 0 else 1.0))


def samples_per_code(fs, code_rate=RATE, code_len=LEN):
    """round(fs / (code_rate / code_len)) in f32 (trk_bank_model.samples_per_code on a count that exists)"""
    return int(np.floor(float(F32(fs) / (F32(code_rate) / F32(code_len))) + 0.5))


def fast_code_ok(h, code_phase, code_rate, n):
    cp, step = F32(code_phase), F32(code_rate) / h["fs"]
    code_ok = bool(n < N_EXACT and cp >= F32(0.0) and cp < h["lenf"] and step >= F32(0.0) and F32(n) * step < SPAN * h["lenf"])
    arms_ok = bool(h["el"] > SPACE_MIN and h["el"] <= SPACE_MAX and h["vel"] > SPACE_MIN and h["vel"] <= SPACE_MAX)
    return code_ok and arms_ok


def two_pi_f(carrier_freq, df=None):
    f = F32(carrier_freq) if df is None else F32(carrier_freq) + F32(df)
    return (F32(2.0) * F32(np.pi)) * f


def fast_car_ok(h, carrier_phase, w, n):
    fs = h["fs"]
    inv_fs = F32(1.0) / fs
    ones = (int(np.array(fs, F32).view(np.uint32)) & MANTISSA) == MANTISSA
    w_ok = bool(w == F32(0.0) or (abs(w) > W_MIN and abs(w) < W_MAX))
    return bool(not ones and fs > FS_MIN and fs < FS_MAX and w_ok and abs(F32(carrier_phase)) + abs(w) * (F32(n) * inv_fs) < PHASE_MAX)


def classify(h, st, n, df=None):
    """-> (code, carrier) of one record (a dict or a gm_trk_state) on handle h over n samples, at carrier offset df"""
    g = st.get if isinstance(st, dict) else lambda k: getattr(st, k)
    code = FAST if fast_code_ok(h, g("code_phase"), g("code_rate"), n) else GENERAL
    car = FAST if fast_car_ok(h, g("carrier_phase"), two_pi_f(g("carrier_freq"), df), n) else GENERAL
    return code, car


# ---- every (kernel, instantiation, class) that can be launched --------------------------------------------------------------------------------
BANK_TG = {1: 1, 3: 4, 7: 8, 17: 16}             # the T the GPU cases use -> the tap group it launches


def tap_group(T):
    return 1 if T <= 1 else 4 if T <= 4 else 8 if T <= 8 else 16


ROWS = ([("bank", tg, form) for tg in (1, 4, 8, 16) for form in FORMS] +
        [("array", launch, form) for launch in AC.launches() for form in FORMS] +
        [("planes", arms, form) for arms in (3, 5) for form in (FAST, GENERAL)])
assert len(ROWS) == 16 + 4 * 172 + 4

# the smallest (A, L) of each tap class of trk_array_kernel: LC = 1, 2, 4, 8, 6 (A = 5) and 5 (A = 6)
ARRAY_SMALLEST = [(2, 1), (2, 2), (2, 3), (2, 5), (5, 5), (6, 5)]

# ---- the handles and the triggers -------------------------------------------------------------------------------------------------------------
HANDLES = {
    "base": dict(fs=2.048e6),                                              # n = 2048
    "el15": dict(fs=2.048e6, early_late_space=1.5),                        # the bank's and the array entry's taps do not depend on it
    "vel15": dict(fs=2.048e6, n_arms=5, very_early_late_space=1.5),
    "fs50": dict(fs=50.0e6),                                               # n = 50 000, the persistent kernel's own 20 MHz case
    "fs16": dict(fs=16777215.0),                                           # 2^24 - 1: the significand is all ones; n = 16 777
}
STATE = dict(carrier_freq=1830.0, carrier_phase=0.3, code_phase=0.25, code_rate=RATE)
MIXED_OFFSETS = (0.0, 2.0e4, -250.0)       # beside carrier_phase = 9.99e4: 0 and -250 Hz stay below 1e5 rad, 20 kHz adds 126 rad and does not
TINY_OFFSETS = (1.0e-13, 0.0, 500.0)       # beside carrier_freq = 0: |2 pi f| = 6.3e-13, 0 and 3.1e3
OFFSETS = (0.0, 500.0, -250.0)             # test_gpu_trk_bank.OFF_SETS[3]

# id, handle, the state's words that differ from STATE, the class it is named for, and which kernels take it ("bank" alone: the entry's
# own n or carrier offsets are needed).  `n`: the linear bank's sample count where it is not the handle's; `offsets`: the bank's
TRIGGERS = [
    dict(id="eligible", handle="base", state={}, form=(FAST, FAST)),
    dict(id="code-phase-negative", handle="base", state=dict(code_phase=-0.75), form=(GENERAL, FAST)),
    dict(id="code-phase-past-len", handle="base", state=dict(code_phase=LEN + 0.5), form=(GENERAL, FAST)),
    # fmodf keeps the sign: c[i] stays below -len + 2 for the first samples, and a tap of -2 chips and less takes the phase below -len —
    # the second wrap of chip_index, which no arm of the tracker needs (so not a planes case) and code_phase = -0.75 does not reach
    dict(id="code-phase-minus-1022", handle="base", state=dict(code_phase=-(LEN - 1.0)), form=(GENERAL, FAST), only=("bank", "array")),
    dict(id="early-late-1.5", handle="el15", state={}, form=(GENERAL, FAST)),
    dict(id="very-early-late-1.5-five-arms", handle="vel15", state={}, form=(GENERAL, FAST)),
    dict(id="two-code-periods", handle="base", state={}, n=4096, form=(GENERAL, FAST), only=("bank",)),
    dict(id="carrier-phase-1.2e5", handle="base", state=dict(carrier_phase=1.2e5), form=(FAST, GENERAL)),
    dict(id="if-20MHz-at-50Msps", handle="fs50", state=dict(carrier_freq=20.0e6), form=(FAST, GENERAL)),
    dict(id="fs-significand-all-ones", handle="fs16", state={}, form=(FAST, GENERAL)),
    dict(id="two-pi-f-6e-13", handle="base", state=dict(carrier_freq=1.0e-13), form=(FAST, GENERAL), only=("array", "planes")),
    dict(id="two-pi-f-6e-13-by-offset", handle="base", state=dict(carrier_freq=0.0), offsets=TINY_OFFSETS,
         forms=[(FAST, GENERAL), (FAST, FAST), (FAST, FAST)], only=("bank",)),
    dict(id="both-general", handle="base", state=dict(code_phase=-0.75, carrier_phase=1.2e5), form=(GENERAL, GENERAL)),
    dict(id="offsets-on-both-sides", handle="base", state=dict(carrier_phase=9.99e4), offsets=MIXED_OFFSETS,
         forms=[(FAST, FAST), (FAST, GENERAL), (FAST, FAST)], only=("bank",)),
]
BY_ID = {t["id"]: t for t in TRIGGERS}
# what the every-launch sweep of the array entry runs on each (format, A, L, pointer form): one record a class
SWEEP = ["eligible", "code-phase-negative", "carrier-phase-1.2e5", "both-general"]


def triggers(kernel, handle_name=None, arms=3):
    """the triggers `kernel` takes (on one handle); the planes kernel of three arms has no very-early / very-late spacing to widen"""
    out = []
    for t in TRIGGERS:
        if kernel not in t.get("only", ("bank", "array", "planes")) or (handle_name is not None and t["handle"] != handle_name):
            continue
        if kernel == "planes" and arms == 3 and t["handle"] == "vel15":
            continue
        out.append(t)
    return out


def state_of(t):
    return dict(STATE, **t["state"])


def samples_of(t):
    return t.get("n", samples_per_code(HANDLES[t["handle"]]["fs"]))


def forms_of(t):
    """-> the (code, carrier) classes a trigger is named for: one, or one per carrier offset of the bank"""
    return list(t["forms"]) if "forms" in t else [t["form"]]


def classes_of(t):
    """-> what the restated predicates make of the trigger, in the order of forms_of"""
    h, st, n = handle(**HANDLES[t["handle"]]), state_of(t), samples_of(t)
    return [classify(h, st, n, df) for df in t["offsets"]] if "offsets" in t else [classify(h, st, n)]


# ---- triggers the entries refuse, or cannot be given: (what, the rule) — none of them is a row ------------------------------------------------
REFUSED = [
    ("code_rate < 0 (step < 0)", "n = round(fs / (code_rate / len)) is not positive: the ring entries and gm_trk_update_planes skip the record "
     "(done 0, processed 0); gm_trk_bank_samples runs it only where the caller's n equals num_samples_per_code, and then the sign of step "
     "is the only test that fails — not a case here: no receiver tracks a code backwards"),
    ("an arm spacing of 0", "gm_trk_create takes 0 as `default` (0.5 and 1.0)"),
    ("an arm spacing below 0 or of code_len and more", "gm_trk_create refuses it (GM_ERR_INVALID_ARG): the general index wraps once each way"),
    ("n >= 2^24", "no case: the issue keeps n at 50 000 and below"),
    ("n step >= 1.99 len on the ring entries, the array entry and the planes", "they take n from code_rate, n = round(fs len / code_rate), so n "
     "step is len to a rounding; only gm_trk_bank_samples takes n from the record"),
    ("fs <= 1 or fs >= 1e12, |2 pi f| >= 1e12", "no receiver samples there; the carrier offsets are bounded by fs / 2"),
]


# ---- the signal under a record ----------------------------------------------------------------------------------------------------------------
def replica(row, fs, n, carrier_freq, code_phase, code_rate=RATE, boc=False, amp=0.6):
    """what a satellite at this state puts under n samples, in float64: the code at code_phase + i code_rate / fs (wrapped into the row),
    BOC(1,1)'s sub-carrier, the carrier at carrier_freq from phase 0 (the record's own carrier_phase turns the prompt, not its size)"""
    i = np.arange(n, dtype=np.float64)
    row = np.asarray(row, np.float64)
    cp = (float(code_phase) + i * (float(code_rate) / float(fs))) % row.size
    sub = np.where((cp - np.floor(cp)) < 0.5, 1.0, -1.0) if boc else 1.0
    return amp * row[np.floor(cp).astype(np.int64)] * sub * np.exp(2j * np.pi * float(carrier_freq) * i / float(fs))


def noise(n, seed, sigma=8.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * sigma
