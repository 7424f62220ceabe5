"""The lag sweep: scenes that put the correlation peak on every code phase of every search plan, and their expected words.

A helper module like acq_model.py, not a test.  Shared by tests/test_acq_sweep_host.py (CPU: the coverage guard against the planner,
the model's peak gap, the shift identity, the schedules) and tests/test_gpu_lag_sweep.py (GPU: every search of every case).

A search reports max, argmax and sum of a power plane that never leaves the device, and max and sum do not change when lags are
permuted: a correlation kernel that writes a class of lags to the wrong place passes every test whose peak is not on such a lag.
Here every lag of every plan is the strict peak of at least one cell.

The construction.  A handle with custom codes, code_len = N and code_rate = fs = 2^20: the resampling index
floorf(float(i) * rate / fs) is i itself, a chip is a sample.  b is a seeded random +-1 sequence of N values; worker p's code row is
roll(b, r_p); the caller-built mix table of bin d is roll(b, s_d) as complex words (+-1, 0), table_freq all zero.  The dwell is
M periods of the constant sample (A, 0), A = 8 on most sizes (below), so the carrier mix hands stage F A * roll(b, s_d) exactly (an
integer times +-1).  Circular correlation commutes with circular shifts: in exact arithmetic the plane of cell (p, d) is the plane of the unshifted cell
rotated by s_d - r_p, so
    argmax[p][d] = (s_d - r_p) mod N
and max and sum are the same two numbers in every cell of every search.  They come from ONE evaluation of acq_model.search_model
on the unshifted cell: float64, the oracle's scaling (transforms without 1/N), and on the long forms still the plain length-N
circular correlation, which the library's long_scale exists to equal.  tests/test_acq_sweep_host.py asserts the peak gap of that
plane, and the shift identity on small sizes, instead of assuming them.

The schedule.  Search j of a case with P workers and D bins puts the P D lags j P D + d P + p on its cells:
    r_p = (c_j - p) mod N,  s_d = (c_j + j P D + d P) mod N,
c_j a seeded offset that moves both shifts from search to search; ceil(N / (P D)) searches cover 0 .. N - 1 (the last one wraps).

The amplitude.  A = 8 except on the sizes of AMPLITUDE.  Every value of the exact plane is (A N c)^2 with c an even integer, one peak
holds half the sum, and strict_sum_order adds the plane in the reference's order: eight sequential float32 sums of N / 8 values.  A
lane that has taken the peak rounds every later value to the peak's ulp, and those values are multiples of one large power of two:
they fall on a few residues of the ulp, ties among them, and the roundings do not average out.  reference_order_sum applied to the
model's own plane (no kernel involved) is up to 3.1e-5 from the float64 sum at N = 16384 and 2.3e-5 at 32768 with A = 8: there the
reference's order itself misses REL, and a test of the sum could not tell a right kernel from a wrong one.  So the scene of a size
must keep half the bound free: reference_order_error(N, A) <= REL / 2, which test_acq_sweep_host.py asserts for every size that
runs with strict_sum_order.  Where A = 8 does not meet that, AMPLITUDE holds an odd amplitude that does (the residues spread)."""
import functools

import numpy as np

import acq_model as AM

FS = float(1 << 20)          # code_rate = fs: exactly one sample a chip up to 2^18 samples
AMP = 8                      # the dwell's constant sample (AMP, 0) ...
AMPLITUDE = {16368: 7, 16384: 11, 20000: 7, 24576: 7, 32736: 7, 32768: 7}      # ... but for these sizes ("The amplitude" above)


def amplitude(N):
    return AMPLITUDE.get(N, AMP)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# 1. every in-LDS size: what gm_fft_supported_sizes returns and gm_acq_create accepts
LDS = [256, 512, 1024, 2000, 2048, 4000, 4096, 5000, 6000, 8000, 8184, 8192, 10000, 12000, 15000, 16000, 16368, 16384]
# 2. (fft_size, base, Q): every composite pair gm_acq_plan_info(n, 0) can return.  The walk of test_acq_sweep_host.py finds these 29;
# acq_composite.hip instantiates one more, 2 x 8184, which only the diagnostic switch GM_COMP_BASE reaches (16368 has an in-LDS plan)
COMPOSITE = [
    (32768, 16384, 2), (49152, 16384, 3), (65536, 16384, 4), (81920, 16384, 5), (98304, 16384, 6), (131072, 16384, 8),
    (32736, 16368, 2), (49104, 16368, 3), (65472, 16368, 4), (81840, 16368, 5), (98208, 16368, 6), (130944, 16368, 8),
    (32000, 16000, 2), (48000, 16000, 3), (64000, 16000, 4), (80000, 16000, 5), (96000, 16000, 6), (128000, 16000, 8),
    (24000, 8000, 3), (40000, 8000, 5), (24576, 8192, 3), (40960, 8192, 5), (24552, 8184, 3), (40920, 8184, 5),
    (18000, 6000, 3), (30000, 6000, 5), (36000, 6000, 6), (20000, 5000, 4), (25000, 5000, 5),
]
COMPOSITE_STRICT = [32768, 32736, 32000, 24000, 24576, 24552, 18000, 20000]      # strict_sum_order too: the smallest Q of each base
# 3. (fft_size, base, Q): per base of the long path the smallest and the largest Q gm_acq_plan_info(n, 1) reports as long up to 2^18,
# and an odd Q between them (the run-time Q of acq_long.hip; bases 2048, 4096, 8000 and 8192 are reached with odd Q only)
LONG = [
    (6144, 2048, 3), (34816, 2048, 17), (63488, 2048, 31),
    (12288, 4096, 3), (69632, 4096, 17), (126976, 4096, 31),
    (56000, 8000, 7), (152000, 8000, 19), (248000, 8000, 31),
    (57344, 8192, 7), (155648, 8192, 19), (253952, 8192, 31),
    (50000, 10000, 5), (150000, 10000, 15), (260000, 10000, 26),
    (112000, 16000, 7), (176000, 16000, 11), (256000, 16000, 16),
    (114688, 16384, 7), (180224, 16384, 11), (262144, 16384, 16),
]
# 4. the long-padded rows of acq_model.CASES: (fft_size, base)
LONG_PADDED = [(n, base) for n, form, base in AM.CASES if form == "long_padded"]


class Case:
    """One parametrised case: a size on its plan, the grid of one search, the handle's options and the dwell's sample format"""

    def __init__(self, group, N, form, base, M, P, D, strict=False, ref=False, index=0):
        self.group, self.N, self.form, self.base, self.M, self.P, self.D = group, N, form, base, M, P, D
        self.strict, self.ref = strict, ref
        self.fmt = AM.FORMATS[index % 3]
        self.id = "%s-%d-%dx%d-M%d%s%s-%s" % (form, N, P, D, M, "-strict" if strict else "", "-refmul" if ref else "", self.fmt)

    @property
    def any_length(self):
        return self.form.startswith("long")

    @property
    def searches(self):
        return -(-self.N // (self.P * self.D))


def _side(N):
    """P = D of a full grid: 64, below 4096 lags the largest power of two with P D <= N"""
    s = 64
    while s * s > N:
        s //= 2
    return s


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, index=len(out), **k))
    for N in LDS:               # group 1: M = 1 on the full grid, under the three option sets that have a kernel or a reduction each
        for opt in ({}, dict(ref=True), dict(strict=True)):
            add("lds", N, "lds", N, 1, _side(N), _side(N), **opt)
    for N in LDS:               # group 2: M = 2 on 8 x 32 items, a grid corr() (acq_kernels.hip) cuts every item of: 32 items per
        add("lds_cut", N, "lds", N, 2, 8, 32)   # XCD are at most the 32 * WG_PER_CU resident slots, whatever WG_PER_CU the plan has
    for N, base, q in COMPOSITE:  # group 3: the code-side table is P Q N 8 bytes (twice while it is built): 32 workers from Q = 6 on
        add("composite", N, "composite", base, 1, 64 if q <= 5 else 32, 64)
        if N in COMPOSITE_STRICT:                 # the plane-storing variants keep P D N 4 bytes of planes
            add("composite", N, "composite", base, 1, 32, 32, strict=True)
    for N, base, q in LONG:     # group 4
        add("long", N, "long", base, 1, _side(N), _side(N))
    for N, base in LONG_PADDED:
        add("long", N, "long_padded", base, 1, _side(N), _side(N))
    return out


CASES = _cases()


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
class Table:
    """what AcquisitionEngine(tables=...) takes: a caller-built mix table and its frequency"""

    def __init__(self, table):
        self.table, self.doppler_freq_hz = table, 0.0


@functools.lru_cache(maxsize=None)
def base_sequence(N):
    """b: N seeded random +-1 values (int8), read only"""
    b = (2 * np.random.default_rng(77000 + N).integers(0, 2, N) - 1).astype(np.int8)
    b.setflags(write=False)
    return b


def schedule(N, P, D):
    """[(r [P], s [D])] per search, int64 in 0 .. N - 1: cell (p, d) of search j peaks at (s_d - r_p) mod N = (j P D + d P + p) mod N"""
    rng = np.random.default_rng(78000 + N)
    out = []
    for j in range(-(-N // (P * D))):
        c = int(rng.integers(0, N))
        out.append(((c - np.arange(P, dtype=np.int64)) % N, (c + j * P * D + np.arange(D, dtype=np.int64) * P) % N))
    return out


def expected_lags(N, r, s):
    """[P][D] uint32: (s_d - r_p) mod N"""
    return ((np.asarray(s, np.int64)[None, :] - np.asarray(r, np.int64)[:, None]) % N).astype(np.uint32)


def rolled(b, shifts, dtype):
    """[len(shifts)][N]: row i is roll(b, shifts[i]) as `dtype`, cut from one doubled copy of b"""
    N = b.size
    bb = np.concatenate([b, b]).astype(dtype)
    out = np.empty((len(shifts), N), dtype)
    for i, sh in enumerate(shifts):
        k = int(sh) % N
        out[i] = bb[N - k:2 * N - k]
    return out


def code_rows(N, r):
    """[P][N] int8: the handle's codes, code_len = N"""
    return rolled(base_sequence(N), r, np.int8)


def mix_tables(N, s):
    """[D][N] complex64: the handle's tables, words (+-1, 0)"""
    return rolled(base_sequence(N), s, np.complex64)


def dwell(N, M, fmt):
    """M periods of the constant sample (amplitude(N), 0) in the sample format `fmt`"""
    return AM.convert(np.full(M * N, amplitude(N) + 0j, np.complex128), fmt)


def exact_plane(N, amp=None):
    """[N] float64: the one-period power plane of the unshifted cell in exact arithmetic, (amp N c[lag])^2 with c the integer
    circular autocorrelation of b (amp N c is exact in float64; its square is rounded once, 1e-16 relative)"""
    b = base_sequence(N).astype(np.float64)
    c = np.round(np.fft.ifft(np.abs(np.fft.fft(b)) ** 2).real)
    assert c[0] == N
    return (float(amplitude(N) if amp is None else amp) * N * c) ** 2


def reference_order_sum(plane32):
    """The plane sum in the reference's order, which strict_sum_order keeps: eight running float32 sums, lane l adding
    power[8 c + l] for c = 0, 1, ..., then an ordered add of the eight lanes starting from -0.0"""
    lanes = np.cumsum(np.asarray(plane32, np.float32).reshape(-1, 8), axis=0, dtype=np.float32)[-1]      # (cumsum adds in sequence)
    s = np.float32(-0.0)
    for v in lanes:
        s = np.float32(s + v)
    return s


def reference_order_error(N, amp=None, rotations=512):
    """The largest relative distance of reference_order_sum from the float64 sum over rotations of the exact plane rounded to
    float32: the eight rotations 0 .. 7 (the peak in each lane) and about `rotations` more, evenly spread"""
    pl = exact_plane(N, amp)
    total = float(pl.sum())
    p2 = np.concatenate([pl, pl]).astype(np.float32)
    lags = list(range(8)) + list(range(8, N, max(1, N // rotations)))
    return max(abs(float(reference_order_sum(p2[N - k:2 * N - k])) / total - 1.0) for k in lags)


@functools.lru_cache(maxsize=None)
def expected(N, M):
    """(max, sum, gap) of every cell: acq_model.search_model on the unshifted cell (r = s = 0), whose peak is lag 0"""
    mx, am, sm, gap = AM.search_model(dwell(N, M, "c32"), mix_tables(N, [0]), code_rows(N, [0]), N, 1, M, np.zeros(1, np.float32), FS,
                                      with_gap=True)
    assert am.shape == (1, 1, 1) and int(am[0, 0, 0]) == 0
    return float(mx[0, 0, 0]), float(sm[0, 0, 0]), float(gap[0, 0, 0])
