"""A plain model of the front-end's DISPATCH (gm_api.hip frontend_launch / gm_frontend_process_dev_batch / gm_frontend_set_state and
fe_kernels.hip fs_run_bounds / fs_guess), numpy only.  The ARITHMETIC reference stays the oracle (oracle.DigitalFrontend); what this
file answers is which of the three kernel forms a call takes, where on the tabulated phase orbit a handle stands, how the speculative
form cuts a block into runs, and which of its guessed runs are expected to stand.  It also holds the case tables and the inputs of
tests/test_gpu_frontend_forms.py, so that tests/test_fe_model_host.py can check on a CPU what each GPU case claims to cover."""
import math
from array import array

import numpy as np

F32 = np.float32
LUT = 2048
SEG = 3840                       # FE_FAST_SEG: samples per pipeline segment (480 chain steps)
SPEC_MIN = 48 * SEG              # FE_SPEC_MIN
SPEC_K, SPEC_K_MAX = 32, 64      # runs per block: default, most
SPEC_WARM = 18                   # FS_WARM_SEGS
GUESS_STEPS = 16384              # FS_GUESS_STEPS
ORBIT_CAP = (1 << 24) + (1 << 16)
SEQ, TAB, SPEC = 0, 1, 2         # indices of gm_frontend_debug_forms
ALPHA = F32(0.001)
CON = F32(1.0) - ALPHA


def phase_step(f_if, fs):
    """(f_if / fs_in) * 2048 in f32 (nco_lut.rs:34)"""
    return (F32(f_if) / F32(fs)) * F32(2048.0)


def has_table(step):
    """the settings frontend_build_table covers (the orbit's length is checked by orbit())"""
    a = abs(float(step))
    return a < 2048.0 and (a == 0.0 or a > 1.0e-20)           # false for NaN


def _f32_round(t):
    """a double t in [0, 2) rounded to f32, to nearest even: adding 2^(e + 28) leaves a double 24 significant bits of t"""
    if t == 0.0:
        return 0.0
    c = math.ldexp(1.0, math.frexp(t)[1] + 28)
    return (t + c) - c


def orbit_values(s, n, r=0.0):
    """n values of r -> fract(fl(r + s)) from r, f32 throughout (fe_orbit_step), and the value that follows them.  r and s are f32 in
    [0, 1) and s >= 2^-28, so r + s is exact in a double and one rounding to f32 is what the f32 addition does."""
    assert 2.0 ** -28 <= s < 1.0 or s == 0.0
    out = array("d")
    add = out.append
    c1, c0, cm1, cm2 = 2.0 ** 29, 2.0 ** 28, 2.0 ** 27, 2.0 ** 26
    for _ in range(n):
        add(r)
        t = r + s
        if t >= 1.0:
            r = ((t + c1) - c1) - 1.0
        elif t >= 0.5:
            r = (t + c0) - c0
        elif t >= 0.25:
            r = (t + cm1) - cm1
        elif t >= 0.125:
            r = (t + cm2) - cm2
        else:
            r = _f32_round(t)
    return np.frombuffer(out, np.float64).astype(F32), r


_orbits = {}


def orbit(f_if, fs):
    """(step, mu, lam, lam') of the NCO phase orbit from 0, or None where the library builds no table.  mu: the transient, lam: the
    period, lam': lam repeated until it is >= SEG (the table holds mu + lam' entries)."""
    o = orbit_table(f_if, fs)
    return None if o is None else o[:4]


def orbit_table(f_if, fs):
    """orbit() and the table itself: (step, mu, lam, lam', r[0 .. mu + lam'))"""
    key = (float(f_if), float(fs))
    if key in _orbits:
        return _orbits[key]
    step = phase_step(f_if, fs)
    res = None
    if has_table(step):
        s = float(F32(abs(step)) * F32(1.0 / 2048.0))
        vals, r, n = np.zeros(0, F32), 0.0, 8192
        while vals.size <= 2 * ORBIT_CAP:
            more, r = orbit_values(s, n - vals.size, r)
            vals = np.concatenate([vals, more])
            bits = vals.view(np.uint32)
            seen = np.nonzero(bits[:-1] == bits[-1])[0]
            if seen.size:                                   # the last value was seen before: it is on the cycle, lam steps after its last visit
                lam = vals.size - 1 - int(seen[-1])
                mu = int(np.nonzero(bits[:-lam] == bits[lam:])[0][0])     # the first value that comes back after lam steps
                lam2 = lam * ((SEG + lam - 1) // lam)
                if lam <= ORBIT_CAP and mu <= ORBIT_CAP and mu + lam2 <= ORBIT_CAP:
                    tab = np.concatenate([vals[:mu], np.tile(vals[mu:mu + lam], lam2 // lam)])
                    res = (step, mu, lam, lam2, tab)
                break
            n += n // 4
    _orbits[key] = res
    return res


def fold(o, p):
    """frontend_fold: table index of stream position p"""
    _, mu, _, lam2 = o[:4]
    return p if p < mu + lam2 else mu + (p - mu) % lam2


def table_phase(o, pos):
    """the phase_accumulator the table kernels write for table index pos: r * (+-2048), -0.0 for a negative chain on 0"""
    return F32(o[4][pos]) * (F32(-2048.0) if o[0] < 0 else F32(2048.0))


def set_state_pos(f_if, fs, phase):
    """gm_frontend_set_state's orbit lookup: the table index the handle stands on after the phase is set, None when it is off the orbit
    (or there is no table): the sequential kernel from there on"""
    phase = F32(phase)
    if phase == 0 and not np.signbit(phase):
        return 0
    o = orbit_table(f_if, fs)
    if o is None:
        return None
    neg = bool(o[0] < 0)
    sign_ok = (not phase > 0) if neg else (not phase < 0)
    if not (sign_ok and abs(phase) < F32(2048.0)):
        return None
    r = abs(phase) * F32(1.0 / 2048.0)
    hits = np.nonzero(o[4] == r)[0]             # (a zero of either sign is entry 0: the table starts there)
    return int(hits[0]) if hits.size else None


def expected_form(n, in_place, table, on_orbit, batch=None, spec=True):
    """the form a call of n samples takes.  table: the handle's setting has a phase table; on_orbit: its phase stands on it;
    batch: None for a single-stream call, else the (table, on_orbit) pairs of ALL members (one launch, one form for every member)."""
    if batch is not None:
        return TAB if all(t and o for t, o in batch) else SEQ
    if not (table and on_orbit):
        return SEQ
    return SPEC if spec and n >= SPEC_MIN and not in_place else TAB


def run_bounds(nseg, K):
    """fs_run_bounds for every run s < K: (first, last) pipeline segment, empty where first >= last"""
    per = (nseg + K - 1) // K
    out = []
    for s in range(K):
        first = min(s * per, nseg)
        out.append((first, min(first + per, nseg)))
    return out


def nseg_of(n):
    return ((n & ~7) + SEG - 1) // SEG


def guessed_runs(nseg, K, w=SPEC_WARM):
    """the runs that start from a guess: the non-empty ones whose warm-up does not reach back to the block's first segment"""
    w = w if w > 0 else SPEC_WARM
    return [s for s, (f, l) in enumerate(run_bounds(nseg, K)) if f < l and f > w]


def clamp_k(k):
    return min(max(k, 2), SPEC_K_MAX)


def _chain_inputs(raw):
    """x * alpha rounded to f32 for the sixteen chains, [step][chain]: chain j < 8 is re of SIMD lane j, 8 + j its im"""
    x = np.asarray(raw).astype(F32).reshape(-1, 2)
    x = x[:x.shape[0] & ~7].reshape(-1, 8, 2)
    return np.concatenate([x[:, :, 0], x[:, :, 1]], axis=1) * ALPHA


def predict_standing(raw, b_init, K, w=SPEC_WARM):
    """For one block (raw: interleaved I/Q, int8 or f32) entered with the sixteen biases b_init (re lanes, then im lanes): for every guessed
    run, whether all sixteen f32 chains started from the guess w segments earlier are bit-equal to the true chain at the run's first step.
    The guess is the recurrence in f64 over the <= 16 384 steps before that point from b_init, rounded to f32 (here as its closed form,
    one dot product; the GPU sums 128 partial windows: the two can differ in the last bit of the guess).  Returns (standing, b_end):
    one bool per guessed run, and the true biases after the block."""
    w = w if w > 0 else SPEC_WARM
    xa = _chain_inputs(raw)
    steps, sps = xa.shape[0], SEG // 8
    nseg = (steps + sps - 1) // sps
    b = np.asarray(b_init, F32).copy()
    at_seg = np.zeros((nseg + 1, 16), F32)
    for k in range(steps):                                      # the true chains: bias = fl(fl(bias * con) + xa)
        if k % sps == 0:
            at_seg[k // sps] = b
        b = b * CON + xa[k]
    at_seg[nseg] = b
    runs = guessed_runs(nseg, K, w)
    if not runs:
        return [], b
    firsts = np.array([run_bounds(nseg, K)[s][0] for s in runs])
    c = float(CON)
    g = np.zeros((len(runs), 16), F32)
    for i, f in enumerate(firsts):
        p = (int(f) - w) * sps
        nw = min(p, GUESS_STEPS)
        wts = c ** np.arange(nw - 1, -1, -1, dtype=np.float64)
        g[i] = (np.asarray(b_init, np.float64) * c ** nw + wts @ xa[p - nw:p].astype(np.float64)).astype(F32)
    start = (firsts - w) * sps
    for t in range(w * sps):                                    # the warm-up: every guessed run's chains at once
        g = g * CON + xa[start + t]
    want = at_seg[firsts]
    return [bool((g[i].view(np.uint32) == want[i].view(np.uint32)).all()) for i in range(len(runs))], b


# ---------------------------------------------------------------------------------------------- inputs
def noise_dc(seed, n, fmt_i8, sigma=30.0, dc=(5.0, -3.0)):
    """noise plus a DC offset, n samples: (what the GPU is given, the same values as interleaved f32 for the oracle)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 2)) * sigma + np.array(dc)
    if fmt_i8:
        raw = np.clip(np.rint(x), -127, 127).astype(np.int8).reshape(-1)
        return raw, raw.astype(F32)
    f = x.astype(F32).reshape(-1)
    return f, f.copy()


def wander_i8(seed, n):
    """clipped int8 noise (sigma 18) around a DC offset that wanders and jumps: what makes a guessed bias converge late"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    dc = 20.0 * np.sin(t * 3.0e-5) + np.where((t // 300000) % 2 == 0, 25.0, -15.0)
    return np.clip(np.rint(rng.normal(0.0, 18.0, (n, 2)) + dc[:, None] * np.array([1.0, -0.6])), -127, 127).astype(np.int8).reshape(-1)


# ---------------------------------------------------------------------------------------------- the cases of test_gpu_frontend_forms.py
N_RAGGED = 48 * SEG + 8 * 37 + 5          # 49 segments: the last one of 37 steps, and a 5-sample unprocessed tail
NO_TABLE = (37.5e6, 25.0e6)               # step 3072

# A: set state.  (name, phase or None = "what a twin handle holds after 1000 samples"), the lengths of the three blocks that follow
A_SETTINGS = [(1.0e6, 8.0e6), (-1.25e6, 8.0e6)]
A_BLOCKS = (8, 2048 + 8, 2 * 2048 + 8 * 3 + 5)
A_PHASES = [("on_orbit", None), ("off_orbit", "1000.5 with the step's sign"), ("neg_zero", -0.0), ("pos_zero", 0.0), ("wrong_sign", "100 against the step"),
            ("below_2048", 2047.9999), ("5e9", 5.0e9), ("3e19", 3.0e19), ("minus_5", -5.0), ("nan", float("nan"))]


def a_phase(name, value, f_if, fs):
    """the f32 phase of a case of A for one setting"""
    neg = f_if < 0
    if name == "on_orbit":
        o = orbit_table(f_if, fs)
        return table_phase(o, fold(o, 1000))
    if name == "off_orbit":
        return F32(-1000.5 if neg else 1000.5)
    if name == "wrong_sign":
        return F32(100.0 if neg else -100.0)
    return F32(value)


# B: one launch of five members; the last is set off its orbit
B_SETTINGS = [(1.0e6, 8.0e6), (-1.25e6, 8.0e6), (0.0, 8.0e6), NO_TABLE, (2.0e6, 8.0e6)]
B_OFF_ORBIT_PHASE = 77.25                 # (2e6, 8e6) visits 0, 512, 1024, 1536 only
B_N, B_ALONE_N = 2 * 2048 + 8 * 3 + 5, 5000

C_SETTINGS = [(0.0, 8.0e6), (1.0001e6, 6.5536e6), (3.999e6, 8.0e6), (-0.4e6, 8.0e6)]
C_BOUNDARY_SETTING = (1.0001e6, 6.5536e6)  # SPEC_MIN - 1 samples out of place: table form; SPEC_MIN: speculative

# D: (fmt_i8, setting, lengths of the consecutive blocks).  Every format, setting and length appears; c32 appears with a negative IF.
D_LEN = {"48": (48 * SEG,), "ragged": (N_RAGGED,), "65": (65 * SEG,), "137_then_48": (137 * SEG, 48 * SEG)}
D_CASES = [(True, (4.1304e6, 16.3676e6), "137_then_48"), (False, (-1.25e6, 8.0e6), "48"), (False, (1.0001e6, 6.5536e6), "ragged"),
           (True, (3.999e6, 8.0e6), "65"), (False, (4.1304e6, 16.3676e6), "65"), (True, (-1.25e6, 8.0e6), "ragged"),
           (True, (1.0001e6, 6.5536e6), "48"), (False, (3.999e6, 8.0e6), "137_then_48")]

# E: the walk.  (GM_FE_SPEC_K or None, GM_FE_SPEC_WARM or None, segments of the block: 48 means the ragged block N_RAGGED)
E_SETTING = (4.1304e6, 16.3676e6)
E_SEED, E_W_MIX = 2024, 12
E_N137 = 137 * SEG
E_SWEEP = [(2, None, 48), (2, None, 137), (64, None, 48), (64, None, 137), (None, 1, 48)]
