"""CPU: the argument sets of tests/test_gpu_device_math.py enter every branch of csrc/gm_libm.h, and the host helper that the GPU test
compares the device with (tests/cpu/libm_host.cpp) agrees with the platform's functions on those same sets.

With this the sets are proven adequate without a GPU: each is classified by the header's own thresholds and must hold at least 1000
arguments per class; and the helper's evaluation of the header — the thing the device has to reproduce word for word — is held to
atanf, sinf / cosf, x / y, fmodf, sqrtf and the definition of the epoch length under the allowances of tests/cpu/test_libm.cpp and
no others (both NaN counts as equal; for div_const only a zero's sign may differ; sincos_cw within 1.6 * 2^-24 of float64).
"""
import numpy as np
import pytest

import device_math_sets as S


def test_argument_sets_enter_every_class():
    a = S.atan_counts(S.atan_args())
    print("atan classes", a)
    S.assert_classes("atan", a)
    c = S.sincosf_counts(S.sincosf_args())
    print("sincosf classes", c)
    S.assert_classes("sincosf", c)
    for i, y in enumerate(S.FMOD_DIVISORS):
        f = S.fmod_counts(S.fmod_args(y, 500 + i), y)
        print("fmod classes y = %r" % y, f)
        S.assert_classes("fmod y = %r" % y, f)
    # the two sincos forms of the correlators: every argument inside the range their int conversion is defined on, none NaN
    for v, lim in ((S.sincos_cw_args(), 2.0 ** 30), (S.sincos_via_f64_args(), 2.0 ** 31)):
        assert np.isfinite(v).all() and np.abs(v).max() <= lim and (np.abs(v) < 2.0 ** -126).sum() >= S.MIN_PER_CLASS
    # ops 7-8: every pair of the table yields intervals; op 10: phases on both sides of every rule
    for fs in S.SPC_FSS:
        for length, rate in S.SPC_CODES:
            assert S.spc_ns(fs, length, rate).size >= 41
    for L in S.CHIP_LENS:
        p = S.chip_index_args(L)
        f = np.floor(p)
        assert p.min() == -L - 2 and p.max() == 2 * L + 2
        for lo, hi in ((-L - 2, -1), (-1, 0), (0, L), (L, L + 1), (L + 1, 2 * L), (2 * L, 2 * L + 3)):
            assert ((f >= lo) & (f < hi)).sum() >= 4, (L, lo, hi)
        assert ((p < 0) & (p > -1e-30)).sum() >= 8            # negative denormals: floor = -1


def test_header_on_host_equals_the_platform_functions():
    x = S.atan_args()
    h0, _, r0, _ = S.host_math(0, x)
    ok = S.same_words(h0, r0)
    print("atanf_glibc (host): %d arguments, %d mismatches" % (x.size, int((~ok).sum())))
    assert ok.all(), S.report_mismatches("atanf_glibc vs atanf", x, ok, h0, r0)

    x = S.sincosf_args()
    h0, h1, r0, r1 = S.host_math(1, x)
    ok = S.same_words(h0, r0) & S.same_words(h1, r1)
    print("sincosf_glibc (host): %d arguments, %d mismatches" % (x.size, int((~ok).sum())))
    assert ok.all(), S.report_mismatches("sincosf_glibc vs sinf", x, ok, h0, r0)

    x = S.sincos_cw_args()
    x = x[np.abs(x) <= 131072.0]
    h0, h1, _, _ = S.host_math(2, x)
    worst = S.sincos_f64_error(x, h0, h1)
    print("sincos_cw (host): %d arguments, max |error| = %.3f * 2^-24" % (x.size, worst / S.ULP1))
    assert worst <= S.SINCOS_BAR

    n = bad = 0
    for i, y in enumerate(S.DIV_DIVISORS):
        x = S.div_args(y, 400 + i)
        h0, h1, r0, _ = S.host_math(4, x, y)
        ok = S.same_or_both_zero(h0, r0) & S.same_words(h1, r0)
        n, bad = n + x.size, bad + int((~ok).sum())
        assert ok.all(), S.report_mismatches("div_const / div_rn vs x / y, y = %r" % y, x, ok, h0, r0)
    print("div_const, div_rn (host): %d operands, %d mismatches" % (n, bad))

    n = 0
    for i, y in enumerate(S.FMOD_DIVISORS):
        x = S.fmod_args(y, 500 + i)
        h0, _, r0, _ = S.host_math(5, x, y)
        ok = S.same_words(h0, r0)
        n += x.size
        assert ok.all(), S.report_mismatches("fmod_bounded vs fmodf, y = %r" % y, x, ok, h0, r0)
    print("fmod_bounded (host): %d operands, 0 mismatches" % n)

    x = S.sqrt_args()
    h0, _, r0, _ = S.host_math(6, x)
    ok = S.same_words(h0, r0)
    assert ok.all(), S.report_mismatches("sqrt_rn vs sqrtf", x, ok, h0, r0)
    with np.errstate(invalid="ignore"):
        assert S.same_words(h0, S.bits(np.sqrt(x))).all()
    print("sqrt_rn (host): %d arguments, 0 mismatches" % x.size)


def test_rate_bounds_on_host_keep_the_definition():
    """spc_rate_bounds as the helper evaluates it: every rate inside [lo, hi] gives n by the definition, in the helper's C++ and in
    the numpy restatement the GPU test holds op 7 to (which therefore agree)."""
    total = 0
    for k, fs in enumerate(S.SPC_FSS):
        for j, (length, rate0) in enumerate(S.SPC_CODES):
            ns = S.spc_ns(fs, length, rate0)
            lo, hi, _, _ = S.host_math(8, ns, fs, length)
            lo, hi = S.from_bits(lo), S.from_bits(hi)
            keep = lo <= hi
            assert keep.sum() >= 41
            r = S.spc_rates(lo[keep], hi[keep], 700 + 10 * k + j)
            r = r[np.isfinite(r) & (r > 0)]
            d, _, _, _ = S.host_math(7, r, fs, length)
            want = S.spc_definition_np(fs, r, length)
            assert (d.astype(np.float64) == want).all()
            nn = ns[keep]
            inside = (r[None, :] >= lo[keep][:, None]) & (r[None, :] <= hi[keep][:, None])
            rows, cols = np.nonzero(inside)
            assert rows.size > 100 * nn.size
            assert (want[cols] == nn[rows]).all(), (fs, length)
            total += rows.size
    print("spc_rate_bounds (host): %d rates inside their intervals, 0 mismatches" % total)


def test_comparison_reports_an_altered_threshold(tmp_path):
    """The comparison can fail: a copy of gm_libm.h whose 11/16 threshold of atanf_glibc is moved to 12/16, built into a second
    helper, differs from the platform's atanf — and only for arguments of the two classes that meet at that threshold."""
    import os
    src = open(os.path.join(S.ROOT, "gnss-sdr-rs_amd", "csrc", "gm_libm.h")).read()
    assert src.count("0x3f300000u") == 1
    (tmp_path / "gm_libm.h").write_text(src.replace("0x3f300000u", "0x3f400000u"))
    alt = S.host_lib(include_dir=str(tmp_path))
    x = S.atan_args()
    h0, _, r0, _ = S.host_math(0, x, lib=alt)
    bad = ~S.same_words(h0, r0)
    cls = S.atan_class(x)
    print("altered threshold: %d mismatches in classes %s" % (int(bad.sum()), sorted(set(cls[bad].tolist()))))
    assert bad.sum() >= 100 and set(cls[bad].tolist()) == {3}            # 11/16 <= |x| < 12/16 lies in class "11/16..19/16"
    assert (np.abs(x[bad]) >= 0.6875).all() and (np.abs(x[bad]) < 0.75).all()
