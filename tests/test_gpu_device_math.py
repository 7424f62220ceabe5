"""The tracking loop's scalar device math ON THE DEVICE, branch by branch.

Tracking's bit-for-bit claim rests on csrc/gm_libm.h and the scalar helpers of csrc/trk_kernels.hip.  tests/cpu/test_libm.cpp holds
the header to glibc with g++; through tracking in lock the device reaches one argument class of most of these functions.  Here
gm_debug_math evaluates each function on the device — by a kernel compiled with the tracking kernels, one argument per lane — over
argument sets that are first classified by the header's own thresholds (>= 1000 arguments in every class, or the case fails before
it compares anything; tests/test_device_math_host.py proves the same sets adequate without a GPU).  What runs on the device and not
under g++: __fdiv_rn, the correctly rounded sqrt lowering, f32 denormal handling, __builtin_rintf, the f64 fused multiply-adds and
conversions of sincosf_glibc, the 64-bit products of reduce_large, ocml's fmodf behind fmod_bounded's fallback and readfirstlane,
and that -ffp-contract=off holds in that translation unit.

Bars:
  * device against the host evaluation of the same header (ops 0-2, 4-6, 8): words equal, or both NaN.  Nothing else.
  * device against the platform's functions (ops 0, 1, 4, 5, 6): the allowances of tests/cpu/test_libm.cpp and no more (both NaN
    counts as equal; for div_const only a zero's sign may differ).
  * ops 2 and 3 against float64 sin / cos: max |error| <= 1.6 * 2^-24 (test_libm.cpp's bar for sincos_cw, there on |x| <= 131072;
    op 3 over |x| <= 2^31).  The worst value is printed.
  * op 7: the two forms of samples_per_code agree with each other and with round(fs / (rate / len)) in numpy f32.
  * op 8: every rate inside the device's [lo, hi] gives n by op 7.
  * op 9: fmod_code<true> == fmod_code<false> == np.fmod on (-len, 3 len), the precondition in its comment.
  * op 10: integers equal to `floor(phase) as usize % len` (saturating cast, FAITHFUL) and to the wrapped form (FIXED).
"""
import numpy as np
import pytest

import device_math_sets as S

pytestmark = pytest.mark.gpu


def _dev(op, x, p0=0.0, p1=0.0):
    from gnss_sdr_rs_amd import tracking as T
    return T.debug_math(op, x, p0, p1)


def _equal(name, x, got, want, ok=None):
    ok = S.same_words(got, want) if ok is None else ok
    assert ok.all(), S.report_mismatches(name, x, ok, got, want)


def test_atanf_glibc(gpu):
    x = S.atan_args()
    counts = S.atan_counts(x)
    S.assert_classes("atan", counts)
    d0, _ = _dev(0, x)
    h0, _, r0, _ = S.host_math(0, x)
    print("op 0 atanf_glibc: %d arguments, %d mismatches against the header on the host, %d against atanf; classes %s"
          % (x.size, int((~S.same_words(d0, h0)).sum()), int((~S.same_words(d0, r0)).sum()), counts))
    _equal("device atanf_glibc vs host atanf_glibc", x, d0, h0)
    _equal("device atanf_glibc vs atanf", x, d0, r0)


def test_sincosf_glibc(gpu):
    x = S.sincosf_args()
    counts = S.sincosf_counts(x)
    S.assert_classes("sincosf", counts)
    d0, d1 = _dev(1, x)
    h0, h1, r0, r1 = S.host_math(1, x)
    bad_h = int((~(S.same_words(d0, h0) & S.same_words(d1, h1))).sum())
    bad_r = int((~(S.same_words(d0, r0) & S.same_words(d1, r1))).sum())
    print("op 1 sincosf_glibc: %d arguments, %d mismatches against the header on the host, %d against sinf / cosf; classes %s"
          % (x.size, bad_h, bad_r, counts))
    _equal("device sincosf_glibc sin vs host", x, d0, h0)
    _equal("device sincosf_glibc cos vs host", x, d1, h1)
    _equal("device sincosf_glibc sin vs sinf", x, d0, r0)
    _equal("device sincosf_glibc cos vs cosf", x, d1, r1)


def test_sincos_cw(gpu):
    x = S.sincos_cw_args()
    assert (np.abs(x) < 2.0 ** -126).sum() >= S.MIN_PER_CLASS and (np.abs(x) > 1.0e5).sum() >= S.MIN_PER_CLASS
    d0, d1 = _dev(2, x)
    h0, h1, _, _ = S.host_math(2, x)
    m = np.abs(x) <= 131072.0
    worst = S.sincos_f64_error(x[m], d0[m], d1[m])
    print("op 2 sincos_cw: %d arguments, %d mismatches against the header on the host; max |error| on |x| <= 131072 (%d arguments) = "
          "%.3f * 2^-24" % (x.size, int((~(S.same_words(d0, h0) & S.same_words(d1, h1))).sum()), int(m.sum()), worst / S.ULP1))
    _equal("device sincos_cw sin vs host", x, d0, h0)
    _equal("device sincos_cw cos vs host", x, d1, h1)
    assert worst <= S.SINCOS_BAR, worst / S.ULP1


def test_sincos_f32_via_f64(gpu):
    x = S.sincos_via_f64_args()
    assert (np.abs(x) < 2.0 ** -126).sum() >= S.MIN_PER_CLASS and (np.abs(x) > 2.0 ** 30).sum() >= S.MIN_PER_CLASS
    d0, d1 = _dev(3, x)
    worst = S.sincos_f64_error(x, d0, d1)
    small = np.abs(x) <= 131072.0
    print("op 3 sincos_f32_via_f64: %d arguments in |x| <= 2^31, max |error| = %.3f * 2^-24 (on |x| <= 131072: %.3f * 2^-24)"
          % (x.size, worst / S.ULP1, S.sincos_f64_error(x[small], d0[small], d1[small]) / S.ULP1))
    assert worst <= S.SINCOS_BAR, worst / S.ULP1


def test_div_const_and_div_rn(gpu):
    n = 0
    for i, y in enumerate(S.DIV_DIVISORS):
        x = S.div_args(y, 400 + i)
        m = np.ones(x.size, bool)                          # where div_const's contract against x / y holds: test_libm.cpp's dividends
        if i == len(S.DIV_DIVISORS) - 1:                   # 2 pi: also every 1021st bit pattern as the dividend (denormal, inf, NaN)
            x = np.concatenate([x, S.bit_patterns()])
            m = np.arange(x.size) < m.size
        d0, d1 = _dev(4, x, y)
        h0, h1, r0, _ = S.host_math(4, x, y)
        _equal("device div_const vs host, y = %r" % y, x, d0, h0)
        _equal("device div_rn vs host, y = %r" % y, x, d1, h1)
        _equal("device div_rn vs x / y, y = %r" % y, x, d1, r0)
        _equal("device div_const vs x / y, y = %r" % y, x[m], d0[m], r0[m], S.same_or_both_zero(d0[m], r0[m]))
        n += x.size
    print("op 4 div_const, div_rn: %d operands over %d divisors, 0 mismatches" % (n, len(S.DIV_DIVISORS)))


@pytest.mark.parametrize("k", range(len(S.FMOD_DIVISORS)), ids=["y=%g" % y for y in S.FMOD_DIVISORS])
def test_fmod_bounded(gpu, k):
    y = S.FMOD_DIVISORS[k]
    x = S.fmod_args(y, 500 + k)
    counts = S.fmod_counts(x, y)
    S.assert_classes("fmod", counts)
    d0, _ = _dev(5, x, y)
    h0, _, r0, _ = S.host_math(5, x, y)
    print("op 5 fmod_bounded y = %r: %d operands, %d mismatches against the header on the host, %d against fmodf; classes %s"
          % (y, x.size, int((~S.same_words(d0, h0)).sum()), int((~S.same_words(d0, r0)).sum()), counts))
    _equal("device fmod_bounded vs host", x, d0, h0)
    _equal("device fmod_bounded vs fmodf", x, d0, r0)


def test_sqrt_rn(gpu):
    x = S.sqrt_args()
    assert ((x > 0) & (x < 2.0 ** -126)).sum() >= S.MIN_PER_CLASS
    d0, _ = _dev(6, x)
    h0, _, r0, _ = S.host_math(6, x)
    print("op 6 sqrt_rn: %d arguments, %d mismatches against the header on the host, %d against sqrtf"
          % (x.size, int((~S.same_words(d0, h0)).sum()), int((~S.same_words(d0, r0)).sum())))
    _equal("device sqrt_rn vs host", x, d0, h0)
    _equal("device sqrt_rn vs sqrtf", x, d0, r0)


def test_epoch_length_forms_and_rate_bounds(gpu):
    n_rates = n_inside = n_shortcut_off = 0
    for k, fs in enumerate(S.SPC_FSS):
        for j, (length, rate0) in enumerate(S.SPC_CODES):
            ns = S.spc_ns(fs, length, rate0)
            dlo, dhi = _dev(8, ns, fs, length)
            hlo, hhi, _, _ = S.host_math(8, ns, fs, length)
            _equal("device spc_rate_bounds lo vs host, fs = %r len = %r" % (fs, length), ns, dlo, hlo)
            _equal("device spc_rate_bounds hi vs host, fs = %r len = %r" % (fs, length), ns, dhi, hhi)
            lo, hi = S.from_bits(dlo), S.from_bits(dhi)
            keep = lo <= hi
            assert keep.sum() >= 41
            r = S.spc_rates(lo[keep], hi[keep], 700 + 10 * k + j)
            r = r[np.isfinite(r) & (r > 0)]
            a, b = _dev(7, r, fs, length)
            want = S.spc_definition_np(fs, r, length)
            assert (a == b).all(), S.report_mismatches("samples_per_code forms, fs = %r len = %r" % (fs, length), r, a == b, a, b)
            ok = a.astype(np.float64) == want
            assert ok.all(), S.report_mismatches("samples_per_code vs numpy, fs = %r len = %r" % (fs, length), r, ok, a, want.astype(np.uint32))
            inside = (r[None, :] >= lo[keep][:, None]) & (r[None, :] <= hi[keep][:, None])
            rows, cols = np.nonzero(inside)
            assert rows.size > 100 * int(keep.sum())
            assert (a[cols].astype(np.float64) == ns[keep][rows].astype(np.float64)).all(), (fs, length)
            n_rates, n_inside = n_rates + r.size, n_inside + rows.size
            n_shortcut_off += int((~inside.any(axis=0)).sum())
    assert n_shortcut_off >= S.MIN_PER_CLASS                 # rates in no interval: where the caller evaluates the definition
    print("ops 7-8: %d rates, two forms and numpy agree on all; %d rates inside a device interval, 0 with another n; %d in none"
          % (n_rates, n_inside, n_shortcut_off))


@pytest.mark.parametrize("length", S.CHIP_LENS)
def test_fmod_code(gpu, length):
    t = S.fmod_code_args(length)
    a, b = _dev(9, t, length)
    want = S.bits(np.fmod(t, np.float32(length)))
    print("op 9 fmod_code len = %d: %d arguments, %d mismatches (fast), %d (fmodf)" % (length, t.size, int((a != want).sum()), int((b != want).sum())))
    _equal("fmod_code<true> vs np.fmod", t, a, want, a == want)
    _equal("fmod_code<false> vs np.fmod", t, b, want, b == want)


@pytest.mark.parametrize("length", S.CHIP_LENS)
def test_chip_index(gpu, length):
    p = S.chip_index_args(length)
    a, b = _dev(10, p, length)
    fa, fi = S.chip_index_reference(p, length)
    print("op 10 chip_index len = %d: %d phases, %d mismatches (FAITHFUL), %d (FIXED)" % (length, p.size, int((a != fa).sum()), int((b != fi).sum())))
    _equal("chip_index FAITHFUL", p, a, fa, a == fa)
    _equal("chip_index FIXED", p, b, fi, b == fi)
