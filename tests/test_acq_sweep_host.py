"""The lag sweep of tests/acq_sweep_model.py on the CPU: its case list against the planner, and what tests/test_gpu_lag_sweep.py takes
for granted about its scenes.

(a) the coverage guard: gm_acq_plan_info walked over every multiple of 8 up to 2^18, any_length clear and set, reaches exactly the
in-LDS sizes and the composite (base, Q) pairs of the helper's lists, and its long rows are what the walk reports for their sizes:
the smallest and the largest Q of every long base and an odd one between.  A plan or pair added later fails here until the sweep
searches it.  (b) the model at every size: the second-largest lag of the unshifted plane is at least GAP below the peak (so the GPU
test's exact arg-max cannot fail on a tie), and the largest power is finite in float32.  (c) the shift identity at three small sizes:
the model on shifted tables and codes finds (s - r) mod N with the unshifted max and sum.  (d) every case's schedule leaves no lag
out.  (e) the reference's sum order, which strict_sum_order keeps, applied to the exact plane of every size that runs strict: within
REL / 2 of the float64 sum, so that half the bound is the kernels' (acq_sweep_model.py, "The amplitude")."""
import numpy as np
import pytest

import acq_model as AM
import acq_sweep_model as SW


# ---- (a) the case list against the planner --------------------------------------------------------------------------------------------
def test_the_sweep_lists_every_plan_the_planner_can_return(gm):
    from gnss_sdr_rs_amd import acquisition as A, fft as F
    lds, comp, long_q = set(), set(), {}
    for any_length in (False, True):
        for n in range(8, (1 << 18) + 1, 8):
            st, info = A.plan_info(n, any_length)
            if st:
                continue
            if info["form"] == "lds":
                lds.add(n)
            elif info["form"] == "composite":
                assert info["base"] * info["q"] == n
                comp.add((n, info["base"], info["q"]))
            elif info["form"] == "long":
                assert info["base"] * info["q"] == n and any_length
                long_q.setdefault(info["base"], set()).add(info["q"])
    assert len(set(SW.LDS)) == len(SW.LDS) and lds == set(SW.LDS), (sorted(lds - set(SW.LDS)), sorted(set(SW.LDS) - lds))
    assert lds == set(n for n in F.supported_sizes() if A.plan_info(n, False)[0] == 0)
    assert len(set(SW.COMPOSITE)) == len(SW.COMPOSITE)
    assert comp == set(SW.COMPOSITE), (sorted(comp - set(SW.COMPOSITE)), sorted(set(SW.COMPOSITE) - comp))
    assert max(n for n, _, _ in comp) <= 131072
    # one strict row per composite base, on its smallest Q
    least = {}
    for n, base, q in SW.COMPOSITE:
        least[base] = min(least.get(base, n), n)
    assert sorted(SW.COMPOSITE_STRICT) == sorted(least.values())
    # the long rows: per base the smallest and the largest Q the walk reports, and an odd Q strictly between where there is one
    rows = {}
    for n, base, q in SW.LONG:
        st, info = A.plan_info(n, True)
        assert st == 0 and (info["form"], info["base"], info["q"]) == ("long", base, q) and n == base * q, (n, base, q, info)
        rows.setdefault(base, []).append(q)
    assert set(rows) == set(long_q), (sorted(rows), sorted(long_q))
    for base, qs in rows.items():
        lo, hi = min(long_q[base]), max(long_q[base])
        between = [q for q in long_q[base] if lo < q < hi and q % 2]
        assert len(set(qs)) == len(qs) and lo in qs and hi in qs, (base, qs, lo, hi)
        mid = [q for q in qs if q not in (lo, hi)]
        assert (len(mid) == 1 and mid[0] in between) if between else not mid, (base, qs, between)
    # the long-padded rows are acq_model's, and they are what they say
    assert SW.LONG_PADDED and len(SW.LONG_PADDED) == sum(1 for _, form, _ in AM.CASES if form == "long_padded")
    for n, base in SW.LONG_PADDED:
        st, info = A.plan_info(n, True)
        assert st == 0 and (info["form"], info["base"]) == ("long_padded", base), (n, base, info)


def test_every_listed_plan_has_its_cases():
    """The parametrised cases are the lists: every in-LDS size under the three option sets and on the cut grid, every composite pair,
    every long row; the three sample formats all occur in every group; no handle's larger tables pass about 1 GB."""
    key = lambda c: (c.group, c.N, c.M, c.strict, c.ref)
    keys = [key(c) for c in SW.CASES]
    assert len(set(keys)) == len(keys) and len(set(c.id for c in SW.CASES)) == len(SW.CASES)
    for N in SW.LDS:
        for strict, ref in ((False, False), (False, True), (True, False)):
            assert ("lds", N, 1, strict, ref) in keys
        assert ("lds_cut", N, 2, False, False) in keys
    for N, base, q in SW.COMPOSITE:
        assert ("composite", N, 1, False, False) in keys
        assert (("composite", N, 1, True, False) in keys) == (N in SW.COMPOSITE_STRICT)
    for N in [n for n, _, _ in SW.LONG] + [n for n, _ in SW.LONG_PADDED]:
        assert ("long", N, 1, False, False) in keys
    for group in ("lds", "lds_cut", "composite", "long"):
        assert set(c.fmt for c in SW.CASES if c.group == group) == set(AM.FORMATS), group
    q_of = {n: q for n, _, q in SW.COMPOSITE}
    for c in SW.CASES:
        assert c.P * c.D <= c.N and c.N <= 1 << 18, c.id       # (up to 2^18 samples float(i) * rate / fs is i exactly)
        if c.group == "lds_cut":
            assert (c.P, c.D, c.M) == (8, 32, 2), c.id             # 8 x 32 items: every XCD's share is within its resident slots
        L = 2 * c.N if c.form == "long_padded" else c.N
        sizes = [c.P * L * 8, c.D * c.M * L * 8, c.D * c.N * 8]
        if c.form == "composite":
            sizes += [2 * c.P * q_of[c.N] * c.N * 8]
        if c.strict and c.form != "lds":
            sizes += [c.P * c.D * c.N * 4]
        assert sum(sizes) < 1 << 30, (c.id, sizes)


# ---- (b) the model at every size --------------------------------------------------------------------------------------------------------
SIZES = sorted(set((c.N, c.M) for c in SW.CASES))


@pytest.mark.parametrize("N,M", SIZES, ids=["%d-M%d" % s for s in SIZES])
def test_the_unshifted_plane_has_a_clean_peak(N, M):
    mx, sm, gap = SW.expected(N, M)
    print("N=%d M=%d: max %.6e, sum %.6e, gap %.6f" % (N, M, mx, sm, gap))
    assert gap >= AM.GAP, (N, M, gap)
    # the peak is A N^2 in every period: the model's max is that number, and it is finite in float32 (and so is the sum)
    peak = (float(SW.amplitude(N)) * N * N) ** 2 * M
    assert abs(mx / peak - 1.0) < 1e-12, (mx, peak)
    assert peak < float(np.finfo(np.float32).max) and np.isfinite(np.float32(mx)) and np.isfinite(np.float32(sm)) and sm > mx


def test_chips_are_samples():
    """code_len = N and code_rate = fs = 2^20: the float32 resampling index is the sample index up to 2^18"""
    i = np.arange(1 << 18, dtype=np.float32)
    assert (np.floor((i * np.float32(SW.FS)) / np.float32(SW.FS)).astype(np.int64) == np.arange(1 << 18)).all()
    b = SW.base_sequence(2000)
    assert (AM.sample_codes(b[None, :], SW.FS, SW.FS, 2000)[0] == b).all() and set(np.unique(b)) == {-1, 1}


# ---- (c) the shift identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,fmt", [(256, 1, "i8"), (2000, 2, "real"), (16368, 1, "c32")])
def test_shifted_cells_are_the_unshifted_plane_rotated(N, M, fmt):
    rng = np.random.default_rng(N)
    r, s = rng.integers(0, N, 3), rng.integers(0, N, 4)
    r[0], s[0] = N - 1, 0                                   # the wrap: lag (0 - (N - 1)) mod N = 1
    mx, am, sm = AM.search_model(SW.dwell(N, M, fmt), SW.mix_tables(N, s), SW.code_rows(N, r), N, 1, M, np.zeros(4, np.float32), SW.FS)
    emx, esm, _ = SW.expected(N, M)
    assert (am[:, 0, :] == SW.expected_lags(N, r, s)).all() and am[0, 0, 0] == 1, (am[:, 0, :], r, s)
    assert np.max(np.abs(mx / emx - 1.0)) <= 1e-12 and np.max(np.abs(sm / esm - 1.0)) <= 1e-12, (mx / emx - 1.0, sm / esm - 1.0)
    # the rows are rolls of b
    b = SW.base_sequence(N)
    assert (SW.code_rows(N, r)[1] == np.roll(b, r[1])).all()
    assert (SW.mix_tables(N, s)[2] == np.roll(b, s[2]).astype(np.complex64)).all()


# ---- (d) the schedules ------------------------------------------------------------------------------------------------------------------
def test_every_schedule_puts_the_peak_on_every_lag():
    for N, P, D in sorted(set((c.N, c.P, c.D) for c in SW.CASES)):
        seen = np.zeros(N, bool)
        sched = SW.schedule(N, P, D)
        assert len(sched) == -(-N // (P * D))
        for r, s in sched:
            assert r.shape == (P,) and s.shape == (D,) and r.min() >= 0 and s.min() >= 0 and r.max() < N and s.max() < N
            lags = SW.expected_lags(N, r, s)
            assert len(np.unique(lags)) == P * D, (N, P, D)      # a search's cells all peak on different lags
            seen[lags.reshape(-1)] = True
        assert seen.all(), (N, P, D, np.flatnonzero(~seen)[:16])


# ---- (e) the reference's sum order on the scenes that run strict ------------------------------------------------------------------------
STRICT_SIZES = sorted(set(c.N for c in SW.CASES if c.strict))


def test_the_exact_plane_is_the_models():
    N = 2000
    _, _, sm, _ = AM.search_model(SW.dwell(N, 1, "c32"), SW.mix_tables(N, [0]), SW.code_rows(N, [0]), N, 1, 1, np.zeros(1, np.float32),
                                  SW.FS, with_gap=True)
    pl = SW.exact_plane(N)
    assert pl[0] == (SW.amplitude(N) * N * N) ** 2 and abs(pl.sum() / sm[0, 0, 0] - 1.0) < 1e-12
    # the order: lane l adds power[8 c + l], then the lanes are added in turn
    v = np.arange(1, 25, dtype=np.float32)
    assert SW.reference_order_sum(v) == np.float32(300.0)
    big = np.zeros(16, np.float32)
    big[0], big[8] = 2.0 ** 24, 1.0       # lane 0: 2^24 + 1 rounds to 2^24 in float32
    assert SW.reference_order_sum(big) == np.float32(2.0 ** 24)


@pytest.mark.parametrize("N", STRICT_SIZES)
def test_the_reference_sum_order_leaves_half_the_bound(N):
    err = SW.reference_order_error(N)
    print("N=%d A=%d: the reference's sum order is %.2e from the float64 sum" % (N, SW.amplitude(N), err))
    assert err <= AM.REL / 2, (N, SW.amplitude(N), err)
    if N in SW.AMPLITUDE:               # an exception is there because the usual amplitude does not meet this, for nothing else
        assert SW.AMPLITUDE[N] % 2 == 1 and 0 < SW.AMPLITUDE[N] <= 127
        assert SW.reference_order_error(N, SW.AMP) > AM.REL / 2, N


def test_every_amplitude_exception_is_a_strict_size():
    assert set(SW.AMPLITUDE) <= set(STRICT_SIZES)
