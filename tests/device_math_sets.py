"""Argument sets, classes and comparisons shared by tests/test_device_math_host.py (CPU) and tests/test_gpu_device_math.py (GPU).

The sets follow tests/cpu/test_libm.cpp, thinned so that a case takes a second or two: every 1021st f32 bit pattern (all exponents,
both signs, denormals, inf, NaN), a dense sweep of 2^22 points over the operating range, and +-2000 ulps around every branch boundary.
The classifiers restate the thresholds of gnss-sdr-rs_amd/csrc/gm_libm.h as they stand there (on the bit pattern where the header
tests the bit pattern), so that a case can assert that every branch is entered >= MIN_PER_CLASS times before it compares anything.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

F32, U32 = np.float32, np.uint32
MIN_PER_CLASS = 1000
ULP1 = 2.0 ** -24                          # ulp of results in [0.5, 1): the unit of test_libm.cpp's sincos_cw bar
SINCOS_BAR = 1.6 * ULP1

DIV_DIVISORS = [2.0e6, 2.046e6, 2.048e6, 4.0e6, 4.092e6, 4.096e6, 5.0e6, 5.456e6, 6.0e6, 8.0e6, 8.184e6, 8.192e6, 1.0e7, 1.2e7, 1.5e7,
                1.6e7, 1.6368e7, 1.63676e7, 2.5e7, 3.8192e7, 5.0e7, 1023.0, 2046.0, 4092.0, 10230.0, 511.0, 6.28318530717958647692]
FMOD_DIVISORS = [6.28318530717958647692, 1023.0, 2046.0, 4092.0, 10230.0, 511.0]
SPC_FSS = [2.048e6, 4.0e6, 4.096e6, 5.0e6, 8.0e6, 1.0e7, 1.6368e7, 1.63676e7, 2.5e7, 3.8192e7, 5.0e7]
SPC_CODES = [(1023.0, 1.023e6), (2046.0, 2.046e6), (4092.0, 1.023e6), (10230.0, 1.023e7)]
CHIP_LENS = [511, 1023, 1024, 4092, 10230]


# ------------------------------------------------------------------------------------------------ the host helper
_host = None


def host_lib(include_dir=None):
    """tests/cpu/libm_host.cpp built with the g++ line of test_abi_and_host.py (+ -fPIC -shared) into a temp directory.
    include_dir: where gm_libm.h is taken from (the mutation check points it at an altered copy); default: the product's csrc."""
    global _host
    if include_dir is None and _host is not None:
        return _host
    so = os.path.join(tempfile.mkdtemp(prefix="gm_libm_host_"), "libm_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                    include_dir or os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpu", "libm_host.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    lib.gm_host_math.restype = C.c_int
    lib.gm_host_math.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 4
    if include_dir is None:
        _host = lib
    return lib


def host_math(op, x, p0=0.0, p1=0.0, lib=None):
    """-> (h0, h1, r0, r1) uint32 words: the header's host evaluation and the platform's functions"""
    x = np.ascontiguousarray(x, F32)
    out = [np.zeros(x.size, U32) for _ in range(4)]
    rc = (lib or host_lib()).gm_host_math(op, x.ctypes.data, x.size, float(p0), float(p1), 0.0, *[o.ctypes.data for o in out])
    assert rc == 0, (op, rc)
    return out


# ------------------------------------------------------------------------------------------------ building blocks
def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def from_bits(u):
    return np.ascontiguousarray(u, U32).view(F32)


_patterns = None


def bit_patterns():
    """every 1021st f32 bit pattern (a prime stride: all exponents, both signs, denormals, inf, NaN), 4.2e6 values"""
    global _patterns
    if _patterns is None:
        _patterns = from_bits(np.arange(0, 1 << 32, 1021, dtype=np.uint64).astype(U32))
        _patterns.setflags(write=False)
    return _patterns


def dense(lo, hi, n=1 << 22):
    return np.linspace(lo, hi, n + 1, dtype=np.float64).astype(F32)


def around(edges, k=2000, both_signs=True):
    """the k floats below and above each (positive) edge, and the edge; with their negatives"""
    e = bits(np.asarray(edges, F32)).astype(np.int64)
    u = (e[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).ravel()
    u = u[(u >= 0) & (u <= 0x7f800000)]
    v = from_bits(u.astype(U32))
    return np.concatenate([v, -v]) if both_signs else v


def same_words(a, b):
    """words equal, or both NaN"""
    fa, fb = from_bits(a), from_bits(b)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


def same_or_both_zero(a, b):
    """test_libm.cpp's allowance for div_const against IEEE division: only a zero's sign may differ (both NaN counts as equal)"""
    fa, fb = from_bits(a), from_bits(b)
    return same_words(a, b) | ((fa == 0) & (fb == 0))


def report_mismatches(name, x, ok, got, want, limit=5):
    bad = np.flatnonzero(~ok)
    return "%s: %d of %d arguments differ; first: %s" % (
        name, bad.size, x.size, [(float(x[i]).hex(), hex(int(got[i])), hex(int(want[i]))) for i in bad[:limit]])


def assert_classes(name, counts, minimum=MIN_PER_CLASS):
    short = {k: v for k, v in counts.items() if v < minimum}
    assert not short, "%s: argument classes with fewer than %d members: %s (all: %s)" % (name, minimum, short, counts)


# ------------------------------------------------------------------------------------------------ op 0: atanf_glibc
ATAN_EDGES = [2.0 ** -29, 7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16, 2.0 ** 25]
ATAN_CLASSES = ["below 2^-29", "2^-29..7/16", "7/16..11/16", "11/16..19/16", "19/16..39/16", "39/16..2^25", "2^25 and above", "NaN"]


def atan_args():
    return np.concatenate([bit_patterns(), dense(-4.0, 4.0), around(ATAN_EDGES)])


def atan_class(x):
    """index into ATAN_CLASSES by the header's own tests on ix = bits & 0x7fffffff"""
    ix = bits(x) & U32(0x7fffffff)
    c = np.searchsorted(np.array([0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000], np.uint64), ix.astype(np.uint64),
                        side="right")
    return np.where(ix > 0x7f800000, 7, c)


def atan_counts(x):
    return dict(zip(ATAN_CLASSES, np.bincount(atan_class(x), minlength=8).tolist()))


# ------------------------------------------------------------------------------------------------ ops 1-3: the sine / cosine forms
# sincosf_glibc branches on abstop12 = (bits >> 20) & 0x7ff: 0x398 is 2^-12; 0x3f4 is abstop12(pi/4), so the branch is taken at 0.75,
# the first float with those top bits, not at pi/4 itself (both are in the edge list); 0x42f is 120; 0x7f8 is inf / NaN
SINCOS_EDGES_GLIBC = [2.0 ** -12, 0.78539816339744830962, 0.75, 120.0, 2.0 ** -126, 2.0 ** 23, 2.0 ** 31]
SINCOS_EDGES_CW = [2.0 ** -12, 0.78539816339744830962, 0.75, 120.0, 2.0 ** -126, 1.0e5, 131072.0]
SINCOSF_CLASSES = ["below 2^-12", "polynomial on x", "reduce_fast", "reduce_large", "inf / NaN"]


def sincosf_args():
    return np.concatenate([bit_patterns(), dense(-2.7e5, 2.7e5), around(SINCOS_EDGES_GLIBC)])


def sincosf_class(x):
    top = (bits(x) >> U32(20)) & U32(0x7ff)
    return np.searchsorted(np.array([0x398, 0x3f4, 0x42f, 0x7f8]), top, side="right")


def sincosf_counts(x):
    return dict(zip(SINCOSF_CLASSES, np.bincount(sincosf_class(x), minlength=5).tolist()))


def sincos_cw_args():
    """sincos_cw converts k = rint(x * 2/pi) to int: defined for |x| <= 2^30, so the bit patterns are cut there (beyond, the host's
    and the device's conversions may differ by the language's rules, and the function is only used below 1e5)"""
    p = bit_patterns()
    return np.concatenate([p[np.abs(p) <= F32(2.0 ** 30)], dense(-2.7e5, 2.7e5), around(SINCOS_EDGES_CW)])


def sincos_via_f64_args():
    """|x| <= 2^31 (the function's comment admits |kd| < 2^31): the bit patterns cut there, the operating range, a dense sweep of the
    whole range, and the edges"""
    v = np.concatenate([bit_patterns(), dense(-2.7e5, 2.7e5), dense(-2.0 ** 31, 2.0 ** 31), around(SINCOS_EDGES_CW),
                        around([2.0 ** 23, 2.0 ** 31])])
    return v[np.abs(v) <= F32(2.0 ** 31)]


def sincos_f64_error(x, s_words, c_words):
    """max |error| of the f32 results against float64 sin / cos of the same f32 argument"""
    xd = np.asarray(x, np.float64)
    es = np.abs(from_bits(s_words).astype(np.float64) - np.sin(xd))
    ec = np.abs(from_bits(c_words).astype(np.float64) - np.cos(xd))
    return float(max(es.max(), ec.max()))


# ------------------------------------------------------------------------------------------------ ops 4-5: division and fmod
def div_args(y, seed, n=150000):
    """test_libm.cpp's four kinds of dividend (sample counts, code rates, 1..1e7 over every exponent, angles), plus multiples of y +- a
    few ulps"""
    rng = np.random.default_rng(seed)
    q = n // 4
    counts = rng.integers(0, 300001, q).astype(F32)
    rates = (F32(1.0e6) + rng.integers(0, 100000, q).astype(F32) * F32(0.5)).astype(F32)
    expo = from_bits((0x3f800000 + rng.integers(0, 0x0c000000, q)).astype(U32))
    angles = (F32(-3.2) + rng.integers(0, 6400001, q).astype(F32) * F32(1.0e-6)).astype(F32)
    mult = (rng.integers(-4000, 4001, 2000).astype(F32) * F32(y)).astype(F32)
    near = from_bits((bits(mult).astype(np.int64) + rng.integers(-3, 4, mult.size)).astype(U32))
    return np.concatenate([counts, rates, expo, angles, near])


FMOD_CLASSES = ["|x| < y", "y <= |x| < 4096 y", "beyond 4096 y", "non-finite"]


def fmod_args(y, seed, n=260000):
    """test_libm.cpp's kinds (the admitted range and a little beyond, a few periods, around multiples of y, any bit pattern), plus
    multiples of y +- a few ulps and +-2000 ulps around the 4096 y edge where the library's fmodf takes over"""
    rng = np.random.default_rng(seed)
    yf = F32(y)
    wide = ((rng.random(n).astype(F32) * F32(2.0) - F32(1.0)) * F32(4200.0) * yf).astype(F32)
    few = ((rng.random(n).astype(F32) * F32(2.0) - F32(1.0)) * F32(3.0) * yf).astype(F32)
    m = rng.integers(-4000, 4001, n).astype(F32)
    close = (m * yf + (rng.random(n).astype(F32) - F32(0.5)) * F32(1.0e-3) * yf).astype(F32)
    mult = (rng.integers(-4100, 4101, 4000).astype(F32) * yf).astype(F32)
    near = from_bits((bits(mult).astype(np.int64) + rng.integers(-3, 4, mult.size)).astype(U32))
    return np.concatenate([wide, few, close, near, around([F32(4096.0) * yf, yf]), bit_patterns()])


def fmod_class(x, y):
    ax = np.abs(np.asarray(x, F32))
    yf = F32(y)
    with np.errstate(invalid="ignore"):
        c = np.where(ax < yf, 0, np.where(ax < F32(4096.0) * yf, 1, 2))
    return np.where(np.isfinite(ax), c, 3)


def fmod_counts(x, y):
    return dict(zip(FMOD_CLASSES, np.bincount(fmod_class(x, y), minlength=4).tolist()))


# ------------------------------------------------------------------------------------------------ op 6: sqrt
def sqrt_args():
    """every 1021st bit pattern (negative arguments and NaN give NaN on both sides), the power sums' range, and the floats around the
    denormal boundary, an odd and an even exponent, and the largest finite value"""
    return np.concatenate([bit_patterns(), dense(0.0, 2.0 ** 26), around([2.0 ** -126, 2.0 ** -125, 1.0, 2.0, 3.4028234e38], both_signs=False)])


# ------------------------------------------------------------------------------------------------ ops 7-8: the epoch length
def spc_definition_np(fs, rate, length):
    """round(fs / (rate / len)) in numpy f32: two correctly rounded divisions, round half away from zero (f32::round)"""
    rate = np.asarray(rate, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (F32(fs) / (rate / F32(length))).astype(F32)
    v64 = v.astype(np.float64)
    r = np.where(v64 >= 0, np.floor(v64 + 0.5), np.ceil(v64 - 0.5))       # exact in f64 for every f32 v
    return r


def spc_ns(fs, length, rate0):
    """n0 - 40 .. n0 + 40 of test_libm.cpp, where n0 is the nominal epoch length (2 <= n < 2^23)"""
    n0 = float(spc_definition_np(fs, [rate0], length)[0])
    ns = n0 + np.arange(-40, 41, dtype=np.float64)
    return ns[(ns >= 2.0) & (ns < 8388608.0)].astype(F32)


def spc_rates(lo, hi, seed, k=64, n_random=200):
    """rates within +-k ulps of every interval end (inside and outside the interval), and random rates inside"""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    d = np.arange(-k, k + 1, dtype=np.int64)
    ends = np.concatenate([(bits(lo).astype(np.int64)[:, None] + d).ravel(), (bits(hi).astype(np.int64)[:, None] + d).ravel()])
    rng = np.random.default_rng(seed)
    inside = (lo[:, None] + (hi - lo)[:, None] * rng.random((lo.size, n_random)).astype(F32)).astype(F32).ravel()
    return np.concatenate([from_bits(ends.astype(U32)), inside])


# ------------------------------------------------------------------------------------------------ op 9: fmod_code
def fmod_code_args(length):
    """t in (-len, 3 len), the precondition stated above fmod_code in trk_kernels.hip: a dense sweep and the floats around 0, len,
    2 len and both ends"""
    L = F32(length)
    v = np.concatenate([dense(-float(length), 3.0 * length, 1 << 18), around([0.0, length, 2.0 * length, 3.0 * length])])
    return v[(v > -L) & (v < F32(3.0) * L)]


# ------------------------------------------------------------------------------------------------ op 10: chip_index
def chip_index_args(length):
    """phases in [-len - 2, 2 len + 2] at quarter-chip steps, plus +-8 ulps around -1, 0, len and len + 1"""
    q = (np.arange(-4 * (length + 2), 4 * (2 * length + 2) + 1, dtype=np.float64) * 0.25).astype(F32)
    e = around([1.0, 0.0, float(length), float(length + 1)], k=8)
    return np.concatenate([q, e[(e >= F32(-length - 2)) & (e <= F32(2 * length + 2))]])


def chip_index_reference(phase, length):
    """get_ca_chip's index (do_tracking.rs:275): FAITHFUL `(phase.floor() as usize) % len` with Rust's saturating cast (a negative
    value and NaN give 0); FIXED the wrapped form, floor(phase) mod len with the sign of len"""
    f = np.floor(np.asarray(phase, F32)).astype(np.float64)
    faithful = np.where(f > 0, f, 0.0).astype(np.int64) % length
    fixed = np.mod(f.astype(np.int64), length)
    return faithful.astype(U32), fixed.astype(U32)
