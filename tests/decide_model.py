"""The acquisition decision on metric words, as the reference writes it (do_acquisition.rs:195-238), in numpy float32 with one
operation per rounding — and a catalogue of the word rows on which a 64-lane prefix scan and this sequential scan can part company.

The decision is a pure function of a code's D metric triples {max, first argmax, sum} (`decide_body` in csrc/acq_kernels.hip on the
device, gm_acq_decide_host and the oracle's orc_decide_from_metrics on the host):

    best = (max 0.0, sum 0.0, phase 0, bin -1)
    for d in 0 .. D-1:
        if mx[d] > best.max: best = (mx[d], sm[d], am[d], d)            # first STRICT maximum
        [reference mode: after every bin; best-bin mode: once, after the last bin]
        avg = f32(f32(best.sum - best.max) / f32(N - 1))
        if f32(best.max / avg) > threshold: found, stop

A found record carries code_phase_chips = f32(f32(f32(phase) * code_rate) / fs) and sample_global_index = local_tail + phase in 64
bits; a code that is not found — or is masked out — carries AcquisitionResult::new: the code's prn, doppler_bin -1, zeros elsewhere.

`cases(N, D)` is the catalogue: named rows (name, mx, am, sm), deterministic for a given fft_size N and bin count D.  A name is
"family/variant@bin"; `families(D)` lists the families a D has room for.  Every family is placed at the bins that matter to a scan in
trips of 64 lanes with a carry: 0, 1, 62, 63, 64, 65, 127, 128 and D - 1, where they exist (`positions`).

Tie rows come in two variants.  In "fail" the earlier of the two equal maxima fails the ratio test and the later would pass: a scan
that takes the later bin finds a satellite where there is none, in either mode.  In "pass" the earlier one passes: the reference mode
stops there before it ever sees the later bin, so a wrong tie rule shows in best-bin mode only (the later bin's phase, sum and
frequency would be reported); in reference mode the row still pins that the exit lane reports ITS OWN running best.

Denormal words are deliberately NOT in the catalogue: the metric words are sums of squared correlations and never get there, and what
the device does with them (flushed or kept) is not settled here.  Every word is zero, normal, infinite or NaN.
"""
import functools

import numpy as np

f32 = np.float32
CA_RATE = 1.023e6
LOCAL_TAILS = (0, 2 ** 32 - 1, 2 ** 40)
THRESHOLDS = (7.0, 2.5)
FIELDS = ("found", "prn", "code_phase_samples", "code_phase_chips", "carrier_freq", "fs", "mag_relative", "sample_global_index",
          "doppler_bin")
# gm_acq_result as the C ABI lays it out (48 bytes, the padding left out), floats as their words
RESULT_DTYPE = np.dtype({"names": ["prn", "code_phase_samples", "code_phase_chips", "carrier_freq", "fs", "mag_relative",
                                   "sample_global_index", "doppler_bin"],
                         "formats": ["u1", "<u8", "<u4", "<u4", "<u4", "<u4", "<u8", "<i4"],
                         "offsets": [0, 8, 16, 20, 24, 28, 32, 40], "itemsize": 48})


def bits(x):
    return int(np.asarray(x, f32).view(np.uint32))


def table_freq(D):
    """D distinct frequencies, none of them the not-found record's 0.0, so that the bin a result was taken from shows in carrier_freq"""
    return (f32(-4001.0) + f32(62.5) * np.arange(D, dtype=f32)).astype(f32)


def not_found(prn):
    return dict(found=0, prn=int(prn), code_phase_samples=0, code_phase_chips=f32(0), carrier_freq=f32(0), fs=f32(0),
                mag_relative=f32(0), sample_global_index=0, doppler_bin=-1)


def scan(mx, am, sm, fft_size, threshold=7.0, best_bin=False, later_on_tie=False):
    """-> (found, max, phase, bin) of one code's row.  later_on_tie: the deliberately WRONG tie rule (tests only)."""
    mx, sm = np.asarray(mx, f32), np.asarray(sm, f32)
    best, bsum, phase, bin_ = f32(0), f32(0), 0, -1
    nm1, thr, D = f32(fft_size - 1), f32(threshold), len(mx)
    with np.errstate(all="ignore"):
        for d in range(D):
            if mx[d] > best or (later_on_tie and bin_ >= 0 and mx[d] == best):
                best, bsum, phase, bin_ = mx[d], sm[d], int(am[d]), d
            if best_bin and d + 1 < D:
                continue
            avg = f32(f32(bsum - best) / nm1)
            if f32(best / avg) > thr:
                return 1, best, phase, bin_
    return 0, f32(0), 0, -1


def ratio(mx_d, sm_d, fft_size):
    """the tested quantity of a bin that is the running best"""
    with np.errstate(all="ignore"):
        return f32(f32(mx_d) / f32(f32(f32(sm_d) - f32(mx_d)) / f32(fft_size - 1)))


def record(hit, tf, prn, fs, local_tail=0, code_rate=CA_RATE):
    found, best, phase, bin_ = hit
    if not found:
        return not_found(prn)
    return dict(found=1, prn=int(prn), code_phase_samples=phase,
                code_phase_chips=f32(f32(f32(phase) * f32(code_rate)) / f32(fs)), carrier_freq=f32(tf[bin_]), fs=f32(fs),
                mag_relative=f32(best), sample_global_index=(int(local_tail) + phase) & (2 ** 64 - 1), doppler_bin=bin_)


def decide(mx, am, sm, tf, fft_size, prn, fs, local_tail=0, code_rate=CA_RATE, threshold=7.0, best_bin=False, searched=True,
           later_on_tie=False):
    """The full gm_acq_result fields plus the found byte of one code."""
    if not searched:
        return not_found(prn)
    return record(scan(mx, am, sm, fft_size, threshold, best_bin, later_on_tie), tf, prn, fs, local_tail, code_rate)


def words(rec):
    """a record as integers, floats by their bit patterns: what the tests compare"""
    return (rec["found"], rec["prn"], rec["code_phase_samples"], bits(rec["code_phase_chips"]), bits(rec["carrier_freq"]),
            bits(rec["fs"]), bits(rec["mag_relative"]), rec["sample_global_index"], rec["doppler_bin"])


def unpack(raw, found, n):
    """n gm_acq_result records (raw bytes) and found bytes -> the tuples of `words`"""
    r = np.frombuffer(bytes(raw), RESULT_DTYPE, n)
    return [(int(found[i]), int(r["prn"][i]), int(r["code_phase_samples"][i]), int(r["code_phase_chips"][i]),
             int(r["carrier_freq"][i]), int(r["fs"][i]), int(r["mag_relative"][i]), int(r["sample_global_index"][i]),
             int(r["doppler_bin"][i])) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ the catalogue
def positions(D):
    return [b for b in (0, 1, 62, 63, 64, 65, 127, 128) if b < D - 1] + [D - 1]


def families(D):
    """the families cases(N, D) holds for this D"""
    fam = ["first_pass", "mid_pass", "no_pass", "mono_inc", "mono_dec", "nonpos", "nonpos_then_pass", "nan_between", "inf_inf",
           "neg_inf", "sm_eq", "sm_lt", "sm_nan", "sm_inf", "edge_eq", "edge_above", "argmax"]
    if D >= 2:
        fam.append("tie_trip")
    if D >= 65:
        fam += ["tie_63_64", "tie_carry"]
    return fam


QUIET = (1.2, 2.0)       # ratios that fail both thresholds
PASS = (9.0, 20.0)       # ... pass both
MID = 4.0                # ... passes 2.5, fails 7.0
EDGE_K = 16384.0         # the threshold edge: mx = 7 k, sm = mx + (N - 1) k


def _sum_for(mx, r, N):
    """the plane sum at which max / ((sum - max) / (N - 1)) is about r"""
    return (np.asarray(mx, np.float64) * (1.0 + (N - 1) / np.asarray(r, np.float64))).astype(f32)


class _Rows:
    def __init__(self, N, D):
        self.N, self.D, self.rng, self.out = N, D, np.random.default_rng(1000 * N + D), []

    def quiet(self, lo=1000.0, hi=2000.0):
        """random positive maxima in [lo, hi), every bin failing both thresholds"""
        mx = self.rng.uniform(lo, hi, self.D).astype(f32)
        sm = _sum_for(mx, self.rng.uniform(*QUIET, self.D), self.N)
        am = self.rng.integers(0, self.N, self.D).astype(np.uint32)
        return mx, am, sm

    def put(self, row, b, value, r):
        mx, am, sm = row
        mx[b] = f32(value)
        sm[b] = _sum_for(mx[b], r, self.N)

    def passing(self):
        return self.rng.uniform(*PASS)

    def failing(self):
        return self.rng.uniform(*QUIET)

    def add(self, name, row):
        mx, am, sm = row
        self.out.append((name, np.ascontiguousarray(mx, f32), np.ascontiguousarray(am, np.uint32), np.ascontiguousarray(sm, f32)))

    def tie(self, name, e, l):
        """the same maximum at bins e < l, nothing larger anywhere; argmax and sum differ"""
        for variant in ("pass", "fail"):
            row = self.quiet()
            v = 3.0e5 + self.rng.integers(0, 1000)
            self.put(row, e, v, self.passing() if variant == "pass" else self.failing())
            self.put(row, l, v, self.passing())
            row[1][l] = (row[1][e] + 1 + self.rng.integers(0, self.N - 1)) % self.N
            assert row[0][e] == row[0][l] and row[1][e] != row[1][l] and row[2][e] != row[2][l]
            self.add("%s/%s@%d_%d" % (name, variant, e, l), row)


@functools.lru_cache(maxsize=None)
def cases(N, D):
    """-> tuple of (name, mx, am, sm): float32 / uint32 / float32 arrays of D words each.  Treat them as read-only."""
    R = _Rows(N, D)
    rng, pos = R.rng, positions(D)
    nan, inf = f32(np.nan), f32(np.inf)
    for b in pos:
        # the first passing bin is b: earlier bins fail, later bins hold stronger peaks that must not be reported
        row = R.quiet()
        R.put(row, b, 3.0e5, R.passing())
        for d in range(b + 1, D):
            R.put(row, d, rng.uniform(5.0e5, 9.0e5), R.passing())
        R.add("first_pass/@%d" % b, row)
        # ... and with the strongest peak of all, in the last bin, failing: found at b in reference mode, not found in best-bin mode
        if b < D - 1:
            row = (row[0].copy(), row[1].copy(), row[2].copy())
            R.put(row, D - 1, 9.5e5, R.failing())
            R.add("first_pass/strongest_fails@%d" % b, row)
        # the same with a bin in front (where there is one) that passes 2.5 only
        row = R.quiet()
        if b > 0:
            R.put(row, b - 1 if b < 3 else b - 2, 2.0e5, MID)
            R.put(row, b, 3.0e5, R.passing())
        else:
            R.put(row, 0, 2.0e5, MID)
        R.add("mid_pass/@%d" % b, row)
        # nothing positive in front of b (zeros, negatives, NaN, -inf: the running best is still (0, bin -1) at b, across the carry)
        row = R.quiet()
        for d in range(b):
            row[0][d] = (f32(0), f32(-0.0), f32(-rng.uniform(1, 1e6)), nan, -inf)[int(rng.integers(0, 5))]
        R.put(row, b, 3.0e5, R.passing())
        R.add("nonpos_then_pass/@%d" % b, row)
        # a NaN maximum at b between a smaller maximum and a larger one: it neither replaces the best nor blocks the next
        row = R.quiet()
        row[0][b] = nan
        row[2][b] = f32(1.0)
        if b + 1 < D:
            R.put(row, b + 1, 5.0e5, R.passing())
        R.add("nan_between/@%d" % b, row)
        # +inf as the best at b and another +inf behind it: inf / (anything) never passes, and nothing replaces it
        row = R.quiet()
        row[0][b] = inf
        row[0][D - 1 if b < D - 1 else 0] = inf
        if b + 1 < D - 1:
            R.put(row, b + 1, 5.0e5, R.passing())
        R.add("inf_inf/@%d" % b, row)
        # -inf at b never replaces anything; the peak next to it (cyclically) is found
        row = R.quiet()
        R.put(row, (b + 1) % D, 5.0e5, R.passing())
        row[0][b] = -inf
        R.add("neg_inf/@%d" % b, row)
        # awkward sums on the best bin b
        for fam, s in (("sm_eq", None), ("sm_lt", f32(1.5e5)), ("sm_nan", nan), ("sm_inf", inf)):
            row = R.quiet()
            R.put(row, b, 3.0e5, R.passing())
            row[2][b] = row[0][b] if s is None else s
            R.add("%s/@%d" % (fam, b), row)
        # the threshold edge on the best bin b: ratio exactly 7.0 (fails 7.0), and one ulp of the maximum above it (passes)
        for fam, up in (("edge_eq", False), ("edge_above", True)):
            row = R.quiet()
            k = f32(EDGE_K)
            m = f32(7.0) * k
            row[2][b] = m + f32(N - 1) * k
            row[0][b] = np.nextafter(m, inf) if up else m
            r = ratio(row[0][b], row[2][b], N)
            assert (r > f32(7.0) and r < f32(7.00001)) if up else r == f32(7.0), (fam, N, float(r))
            R.add("%s/@%d" % (fam, b), row)
    # rows with no passing bin
    R.add("no_pass/quiet", R.quiet())
    R.add("no_pass/wide", R.quiet(1.0, 1.0e9))
    row = R.quiet()
    row[0][:] = row[0][0]                                        # one value in every bin: bin 0 stays the best
    R.add("no_pass/flat", row)
    # monotone maxima: increasing (every lane replaces), decreasing (only lane 0 does)
    inc = np.sort(rng.uniform(1000.0, 2000.0, D).astype(f32))
    inc += np.arange(D, dtype=f32)                               # strictly
    assert D == 1 or (np.diff(inc) > 0).all()
    row = R.quiet(); row[0][:] = inc; row[2][:] = _sum_for(inc, rng.uniform(*QUIET, D), N)
    R.add("mono_inc/none", row)
    row = (row[0].copy(), row[1].copy(), row[2].copy())
    R.put(row, D - 1, row[0][D - 1], R.passing())
    R.add("mono_inc/pass_last", row)
    row = R.quiet(); row[0][:] = inc[::-1]
    row[2][:] = _sum_for(row[0], rng.uniform(*PASS, D), N)       # every later bin would pass if it were taken
    row[2][0] = _sum_for(row[0][0], R.failing(), N)
    R.add("mono_dec/none", row)
    row = (row[0].copy(), row[1].copy(), row[2].copy())
    row[2][0] = _sum_for(row[0][0], R.passing(), N)
    R.add("mono_dec/pass_first", row)
    # no positive maximum at all: the best stays (0, 0), 0 / 0 is NaN and fails
    for name, vals in (("zero", (f32(0),)), ("negative", (f32(-1.0), f32(-3.0e5))), ("nan", (nan,)),
                       ("mixed", (f32(0), f32(-0.0), f32(-2.5), nan, -inf))):
        row = R.quiet()
        row[0][:] = [vals[int(i)] for i in rng.integers(0, len(vals), D)]
        R.add("nonpos/" + name, row)
    row = R.quiet()
    row[0][:] = 0; row[2][:] = 0; row[1][:] = 0
    R.add("nonpos/all_words_zero", row)
    # argmax words
    for a in (0, N - 1, 2 ** 24 + 1, 0xFFFFFFFF):
        row = R.quiet()
        b = min(1, D - 1)
        R.put(row, b, 3.0e5, R.passing())
        row[1][b] = a
        R.add("argmax/%d" % a, row)
    # ties
    for d0 in range(0, D, 64):
        n = min(64, D - d0)
        if n >= 2:
            R.tie("tie_trip", d0 + (1 if n > 2 else 0), d0 + n - 1)
    if D >= 65:
        R.tie("tie_63_64", 63, 64)
        for l in [b for b in pos if b >= 64]:
            R.tie("tie_carry", 7, l)
    names = [c[0] for c in R.out]
    assert len(set(names)) == len(names)
    for _, mx, am, sm in R.out:
        for a in (mx, am, sm):
            a.setflags(write=False)
        fin = np.isfinite(mx) & (mx != 0)
        assert (np.abs(mx[fin]) >= np.finfo(f32).tiny).all()     # no denormals (module docstring)
        fin = np.isfinite(sm) & (sm != 0)
        assert (np.abs(sm[fin]) >= np.finfo(f32).tiny).all()
    return tuple(R.out)


def family_of(name):
    return name.split("/")[0]


def stack(rows):
    """rows of cases() -> the [P][D] planes mx, am, sm"""
    return (np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]))


def scans(rows, fft_size, threshold=7.0, best_bin=False):
    """the scan of every row: what `expected` needs of the words themselves (local_tail, code_rate, fs and the mask come after it)"""
    return [scan(mx, am, sm, fft_size, threshold, best_bin) for _, mx, am, sm in rows]


def expected(hits, tf, prns, fs, local_tail=0, code_rate=CA_RATE, mask=None):
    """the `words` of every code from its scan; mask: bit p switches code p < 64 on (codes from 64 on are always searched), None: all on"""
    on = lambda p: mask is None or p >= 64 or bool((mask >> p) & 1)
    return [words(record(h, tf, prns[p], fs, local_tail, code_rate) if on(p) else not_found(prns[p])) for p, h in enumerate(hits)]


def limit_rows(N, D):
    """three rows for a single call at a large D (the n_bins limit of the device entry): the first pass in the last bin, a tie between
    bin 7 and the last bin whose earlier bin fails, and nothing"""
    R = _Rows(N, D)
    row = R.quiet()
    R.put(row, D - 1, 3.0e5, R.passing())
    R.add("limit/pass_last", row)
    R.tie("limit_tie", 7, D - 1)
    R.add("limit/quiet", R.quiet())
    return tuple(r for r in R.out if "/pass@" not in r[0])
