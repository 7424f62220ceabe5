"""gm_acq_plan_info (host only): which path gm_acq_create takes for every fft_size, with gm_acq_cfg.any_length clear and set.

With the flag clear the accepted set is exactly today's: the in-LDS plan sizes plus the composites Q x base of acq_composite.hip
(restated here from that file's rule, not read back from the entry).  With the flag set every multiple of 8 in [1024, 2^18] is
accepted; the sizes served before keep their path, the rest run on the long path (acq_long.hip), natively (L = N) where a base
divides N with Q <= 32, else padded (2N <= L)."""
import ctypes as C

import numpy as np

LDS, COMPOSITE, LONG, LONG_PADDED = 0, 1, 2, 3
OK, INVALID_ARG, UNSUPPORTED_N, ALIGNMENT = 0, -1, -2, -6
# acq_composite.hip: bases in find_comp's order (largest first, 16368 before 16000, 8000 before 8192), Q in {2, 3, 4, 5, 6, 8}
COMP_BASES = (16384, 16368, 16000, 8000, 8192, 8184, 6000, 5000, 4000)
COMP_Q = (2, 3, 4, 5, 6, 8)
NMAX = 1 << 18


def _lds_sizes(lib):
    n = lib.gm_fft_supported_sizes(None, 0)
    buf = (C.c_uint32 * n)()
    assert lib.gm_fft_supported_sizes(C.cast(buf, C.c_void_p), n) == n
    return set(int(v) for v in buf)


def _expected_today(n, lds):
    """(status, form, base, q) gm_acq_create gives an fft_size with any_length = 0, from the rule of acq_composite.hip."""
    if n == 0:
        return INVALID_ARG, None, None, None
    if n % 8:
        return ALIGNMENT, None, None, None
    if n in lds:
        return OK, LDS, n, 1
    for b in COMP_BASES:
        for q in COMP_Q:
            if b * q == n:
                return OK, COMPOSITE, b, q
    return UNSUPPORTED_N, None, None, None


def _walk(lib, any_length, sizes):
    from gnss_sdr_rs_amd._lib import AcqPlan
    o = AcqPlan()
    out = {}
    for n in sizes:
        o.form, o.base, o.q, o.transform_len = -1, 0, 0, 0
        st = lib.gm_acq_plan_info(n, any_length, C.byref(o))
        out[n] = (st, int(o.form), int(o.base), int(o.q), int(o.transform_len))
    return out


def test_plan_info_flag_clear_is_todays_set(gm):
    lib = gm.lib()
    lds = _lds_sizes(lib)
    got = _walk(lib, 0, range(8, NMAX + 8 + 1, 8))
    accepted = []
    for n, (st, form, base, q, tl) in got.items():
        est, eform, ebase, eq = _expected_today(n, lds)
        assert st == est, (n, st, est)
        if st == OK:
            accepted.append(n)
            assert (form, base, q, tl) == (eform, ebase, eq, n), (n, form, base, q, tl)
    # 18 in-LDS sizes (two of them below 1024) and 29 composites: 45 between 1024 and 2^18
    assert len([n for n in accepted if 1024 <= n <= NMAX]) == 45
    for n in (34000, 90000, 7 * 16368, 9 * 8000, 7 * 8184, 50000, 200000, 38400):
        assert got[n][0] == UNSUPPORTED_N, n
    for n in (0, 2046, 1001):
        assert _walk(lib, 0, [n])[n][0] == _expected_today(n, lds)[0]


def test_plan_info_any_length(gm):
    lib = gm.lib()
    lds = _lds_sizes(lib)
    got = _walk(lib, 1, range(8, NMAX + 1, 8))
    today = _walk(lib, 0, range(8, NMAX + 1, 8))
    forms = {LDS: 0, COMPOSITE: 0, LONG: 0, LONG_PADDED: 0}
    for n, (st, form, base, q, tl) in got.items():
        if today[n][0] == OK:
            assert got[n] == today[n], (n, got[n], today[n])      # served before: same form, base and Q
        if n < 1024:
            assert st == today[n][0], n
            continue
        assert st == OK, (n, st)
        forms[form] += 1
        assert base in lds and 1 <= q <= 32 and tl == q * base, (n, form, base, q, tl)
        if form in (LDS, COMPOSITE, LONG):
            assert tl == n, (n, form, tl)
        else:
            assert tl >= 2 * n, (n, tl)
            if n >= 2048:
                assert tl <= 3 * n, (n, tl)
    assert forms[LONG] > 0 and forms[LONG_PADDED] > 0
    for n, nb, q in ((50000, 10000, 5), (200000, 10000, 20), (61440, 4096, 15), (100000, 10000, 10)):
        assert got[n] == (OK, LONG, nb, q, n), (n, got[n])
    assert got[262136][1] == LONG_PADDED and got[262136][4] <= 32 * 16384
    assert _walk(lib, 1, [2046])[2046][0] == ALIGNMENT
    assert _walk(lib, 1, [262152])[262152][0] == UNSUPPORTED_N
    assert _walk(lib, 1, [0])[0][0] == INVALID_ARG


def test_plan_info_python_helper(gm):
    from gnss_sdr_rs_amd import acquisition as A
    assert A.plan_info(50000, any_length=False) == (UNSUPPORTED_N, None)
    st, info = A.plan_info(50000, any_length=True)
    assert st == OK and info == dict(form="long", base=10000, q=5, transform_len=50000)
    st, info = A.plan_info(38400, any_length=True)
    assert st == OK and info["form"] == "long_padded" and info["transform_len"] >= 2 * 38400
    assert A.plan_info(16368, any_length=True) == (OK, dict(form="lds", base=16368, q=1, transform_len=16368))
    assert A.plan_info(32000, any_length=True) == (OK, dict(form="composite", base=16000, q=2, transform_len=32000))
