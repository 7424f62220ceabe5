"""The correlation peak on every code phase of every search plan (tests/acq_sweep_model.py holds the construction and the cases;
tests/test_acq_sweep_host.py holds the case list to the planner and the scenes to the float64 model).

A search reports max, argmax and sum per (worker, bin) cell, and max and sum do not change when lags are permuted: a stage-C kernel
that writes a residue class of lags to the wrong place, or carries the wrong index through its lane, wave or LDS reduction, passes
every test whose peak is not on an affected lag.  Here worker p's code is roll(b, r_p), bin d's mix table is roll(b, s_d) and the
dwell is constant, so cell (p, d) peaks at (s_d - r_p) mod N, and the shifts of a case's searches walk that lag through 0 .. N - 1.

Every search of a case: argmax equal to the expected lag in every cell; max and sum within REL = 1e-5 of the float64 model's pair,
which is the same in every cell; every worker found, at the lag of the bin it chose.  Wrong lags are printed as (expected, got)
pairs: the residue pattern names the index map at fault.

1. in-LDS sizes, M = 1, a full P x D grid: default options, reference_products and strict_sum_order, which each have a kernel
   instantiation or a reduction of their own (N = 16368: acq_corr_ws31_kernel<CP, false> and <CP, true>).
2. in-LDS sizes, M = 2, 8 workers x 32 bins.  corr() (acq_kernels.hip) cuts every item of a grid whose share per XCD is within the
   resident slots, so every lag's peak goes through the ticket merge and the slab's register order.  Which items were cut is
   asserted: gm_acq_debug_corr_grid reports the grid the launcher decided, and every search of the group requires "every item cut
   into M parts" of it (the classes of that decision have a test of their own, tests/test_gpu_grid_geometry.py).
3. every composite (base, Q) pair, M = 1; strict_sum_order on the smallest Q of each base, which runs the plane-storing variants
   and plane_strict_sum_kernel.
4. the long rows (the smallest, an odd and the largest run-time Q of each base) and the long-padded rows, any_length set, M = 1.

A handle's codes and tables are fixed when it is created, so every search has a handle of its own; the dwell is constant and is
uploaded once per case.  A case's cost is its host side: N / (P D) handles of (P + 8 D) N bytes each, N^2 / 28 bytes at 64 x 64, which
is why the five long rows next to 2^18 samples take seven to eight seconds and every other case at most four.

With strict_sum_order the sum is the reference's eight sequential float32 sums, whose own distance from the float64 sum is not
negligible beside REL; acq_sweep_model.py ("The amplitude") chooses the dwell's amplitude per size so that it stays below REL / 2
on the exact plane, and tests/test_acq_sweep_host.py asserts that.

Measured on an MI355X, worst case of each group (max rel, sum rel): in-LDS default 2.0e-6, 1.3e-6; reference_products 2.0e-6,
1.3e-6; strict 2.0e-6, 3.8e-6; cut items 2.0e-6, 1.3e-6; composite 2.5e-6, 2.1e-6; composite strict 2.3e-6, 7.0e-6 (3 x 8184);
long 1.9e-6, 1.1e-6; long-padded 1.8e-6, 9.7e-7.  No lag came back wrong in the 5.35 million cells of the 137 cases' 2174 searches."""
import numpy as np
import pytest

import acq_model as AM
import acq_sweep_model as SW

pytestmark = pytest.mark.gpu
REL = AM.REL
SHOWN = 48          # wrong lags printed per case


def _sweep(A, _lib, hipbuf, c, all_cut=False):
    N, M, P, D = c.N, c.M, c.P, c.D
    emx, esm, gap = SW.expected(N, M)
    assert gap >= AM.GAP
    fmt = {"c32": _lib.FMT_C32, "i8": _lib.FMT_I8_IQ, "real": _lib.FMT_I8_REAL}[c.fmt]
    d_x = hipbuf.upload(SW.dwell(N, M, c.fmt))
    ids = np.arange(1, P + 1, dtype=np.uint8)
    wrong, n_wrong, lost, worst_mx, worst_sm = [], 0, 0, 0.0, 0.0
    sched = SW.schedule(N, P, D)
    for j, (r, s) in enumerate(sched):
        tabs = SW.mix_tables(N, s)
        eng = A.AcquisitionEngine(SW.FS, 0.0, N, tables=[SW.Table(t) for t in tabs], prn_ids=ids, n_integrations=M,
                                  codes=SW.code_rows(N, r), code_rate=SW.FS, any_length=c.any_length, strict_sum_order=c.strict,
                                  reference_products=c.ref)
        try:
            info = eng.plan_info()
            assert (info["form"], info["base"]) == (c.form, c.base), (c.id, info)
            assert eng.dwell_samples == M * N and (eng.table_freq == 0.0).all()
            eng.search_dev(d_x, fmt)
            if all_cut:     # the launcher's own record of this launch: every item of every XCD cut into one part per integration
                g = eng.debug_corr_grid()
                assert (g["cut"], g["split_from"], g["split_k"], g["split_items"], g["grid"]) == (1, 0, M, g["share"], 8 * M * g["share"]), (c.id, g)
                assert g["share"] <= g["slots"] and (g["n_workers"], g["n_bins"], g["n_int"]) == (P, D, M), (c.id, g)
            eng.decide_dev()
            res = eng.fetch_results()
            mx, am, sm = eng.metrics()
        finally:
            eng.close()
        want = SW.expected_lags(N, r, s)
        bad = np.argwhere(am != want)
        n_wrong += len(bad)
        wrong += [(int(want[p, d]), int(am[p, d])) for p, d in bad[:SHOWN - len(wrong)]]
        worst_mx = max(worst_mx, float(np.max(np.abs(mx.astype(np.float64) / emx - 1.0))))
        worst_sm = max(worst_sm, float(np.max(np.abs(sm.astype(np.float64) / esm - 1.0))))
        for p, got in enumerate(res):       # found, and at the lag of the bin the decision chose
            if got is None or int(got["code_phase_samples"]) != int(am[p, int(got["doppler_bin"])]):
                lost += 1
    print("%s: %d searches of %d x %d cells, worst max rel %.2e, worst sum rel %.2e, model gap %.4f"
          % (c.id, len(sched), P, D, worst_mx, worst_sm, gap))
    if n_wrong:
        print("%s: %d wrong lags, (expected, got): %s" % (c.id, n_wrong, wrong))
    assert n_wrong == 0, (c.id, n_wrong, wrong)
    assert worst_mx <= REL, (c.id, worst_mx)
    assert worst_sm <= REL, (c.id, worst_sm)
    assert lost == 0, (c.id, lost)


def _cases(group):
    cs = [c for c in SW.CASES if c.group == group]
    return pytest.mark.parametrize("c", cs, ids=[c.id for c in cs])


@_cases("lds")
def test_in_lds_plans_on_every_lag(gpu, hipbuf, c):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _sweep(A, _lib, hipbuf, c)


@_cases("lds_cut")
def test_in_lds_plans_on_every_lag_through_the_cut_items(gpu, hipbuf, c):
    """M = 2 on 8 x 32 items: 32 items per XCD are within the 32 * WG_PER_CU resident slots of every plan, and corr() cuts every item
    of such a grid into one part per integration, merged through the tickets and the register-order slab.  Asserted for every
    search through gm_acq_debug_corr_grid (cut kind "all", M parts, no uncut slot); no diagnostic variable is set."""
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _sweep(A, _lib, hipbuf, c, all_cut=True)


@_cases("composite")
def test_composite_pairs_on_every_lag(gpu, hipbuf, c):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _sweep(A, _lib, hipbuf, c)


@_cases("long")
def test_long_paths_on_every_lag(gpu, hipbuf, c):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _sweep(A, _lib, hipbuf, c)
