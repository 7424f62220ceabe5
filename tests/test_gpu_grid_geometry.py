"""Every grid geometry of stage C held to a cell-by-cell lag check (tests/acq_grid_model.py holds the shape table, the classes and the
scene; tests/test_acq_corr_grid_host.py holds the table to the census of the launcher's plan).

Stage C deals its workgroups onto (worker, Doppler bin, integration) items by a tile map and a grid-tail cut that Launch<PL>::corr
chooses (csrc/acq_corr_grid.h) and four device copies of a decode undo.  Here every class of that choice runs on the device, on
every kernel copy, in a scene where every cell of a search peaks on a lag no other cell has: a workgroup that computes the wrong
cell, a cell twice and another never, or merges parts of two items is a wrong lag, a wrong max or a word that was never written.

Per case, one handle: the caller's metric buffer pre-filled with 0x5A bytes; a search; gm_acq_debug_corr_grid — the class the table
declares for the shape, and every number equal to what the plan functions give on the host (the CPU binary's --shapes), so which
items were cut is asserted, not assumed; argmax exact in every searched cell; max and sum within acq_model.REL of the float64 model;
the cells of masked workers still 0x5A, byte for byte; a second search on the same handle equal bit for bit (the tickets restart
from zero in every launch).

The in-LDS shapes with a cut run a second pass with the lowest worker dropped, then all but the last: the class changes (tail to
all, one map to another) and the cells common to both runs are equal bit for bit — a cell does not depend on whether its item was cut.
One edge search at H = 3 per in-LDS kernel (3 D bins against a scratch sized for P D), one prepared search on an all-cut shape (its
tickets are cleared by corr()'s memset, not by stage F), and the diagnostic tiled walk (map_mode >= 16) in a child process per
in-LDS kernel copy.

Measured on an MI355X (every case prints its own line): worst max rel 1.8e-6 (12000, 3 x 86, M = 1), worst sum rel 1.7e-6 (12000,
3 x 86, M = 2, strict_sum_order); no wrong lag and no written sentinel in the 99 cases, which take 3.4 s together."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import acq_grid_model as GM
import acq_model as AM
import acq_sweep_model as SW
from conftest import ROOT

pytestmark = pytest.mark.gpu
REL = AM.REL
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def host_plans():
    """{(shape id, n_workers): (class, numbers)} by the plan functions on the host, for every launch this module makes"""
    from gnss_sdr_rs_amd import acquisition as A
    L = {k: A.plan_info(v["N"], v["form"].startswith("long"))[1]["transform_len"] for k, v in GM.KERNELS.items()}
    keys, lines = [], []
    for s in GM.SHAPES + GM.EDGE_SHAPES + [GM.PREPARED_SHAPE]:
        keys.append((s.id, s.n_workers)); lines.append(s.line(L=L[s.kernel]))
    for s in GM.CUT_SHAPES:
        for nw in (s.P - 1, 1):
            keys.append((s.id, nw)); lines.append(s.line(n_workers=nw))
    for s in GM.TILED_SHAPES:
        keys.append((s.id, s.n_workers)); lines.append(s.line(cb_env=4))
    return dict(zip(keys, GM.classify(lines)))


class Run:
    """One handle of a shape in the scene of acq_grid_model.py, its dwell on the device, and the checks of one search"""

    def __init__(self, A, _lib, hipbuf, s, index=0):
        self.s, self.hipbuf = s, hipbuf
        k = GM.KERNELS[s.kernel]
        N, P, D, M = s.N, s.P, s.D, s.M
        r, sh = GM.shifts(N, P, D)
        self.want = GM.expected_lags(N, P, D)
        fmt = "c32" if s.H else AM.FORMATS[index % 3]
        self.fmt = {"c32": _lib.FMT_C32, "i8": _lib.FMT_I8_IQ, "real": _lib.FMT_I8_REAL}[fmt]
        self.eng = A.AcquisitionEngine(SW.FS, 0.0, N, tables=[SW.Table(t) for t in SW.mix_tables(N, sh)], prn_ids=np.arange(1, P + 1, dtype=np.uint8),
                                       n_integrations=M, codes=SW.code_rows(N, r), code_rate=SW.FS, any_length=k["form"].startswith("long"),
                                       strict_sum_order=s.strict, coherent_periods=s.K)
        info = self.eng.plan_info()
        assert (info["form"], info["base"]) == (k["form"], k["base"]), (s.id, info)
        if s.H:
            self.eng.set_edge_search(list(range(s.H)))
        n = self.eng.dwell_samples
        assert n == (s.K * M + max(s.H - 1, 0)) * N
        self.d_x = hipbuf.upload(AM.convert(np.full(n, SW.amplitude(N) + 0j, np.complex128), fmt))
        emx, esm, gap = SW.expected(N, M)
        assert gap >= AM.GAP
        # two coherent periods of the constant dwell fold to twice the sample: four times the power, exactly
        self.emx, self.esm = emx * s.K * s.K, esm * s.K * s.K
        self.worst = [0.0, 0.0]

    def close(self):
        self.eng.close()

    def search(self, workers, host, prepared=False):
        """one search into a caller's buffer of 0x5A bytes -> the [3][P][D] words; the export and every cell checked"""
        s, eng, P, D = self.s, self.eng, self.s.P, self.s.D
        d_met = self.hipbuf.upload(np.full(3 * P * D, SENTINEL, np.uint32))
        eng.set_prn_mask(sum(1 << p for p in workers))
        if prepared:
            eng.search_prepared_dev(eng.prepare_dev(self.d_x, self.fmt), d_met)
        else:
            eng.search_dev(self.d_x, self.fmt, d_met)
        eng.synchronize()
        words = self.hipbuf.download(d_met, 3 * P * D * 4, np.uint32).reshape(3, P, D)
        # (c) the launcher's record: the path, the launch, the class and every number the host plan gives
        info = eng.debug_corr_grid()
        k = GM.KERNELS[s.kernel]
        assert info["path"] == k["path"] and info["wg_per_cu"] == k["wg"], (s.id, info)
        assert (info["n_workers"], info["n_bins"], info["n_int"]) == (len(workers), D * max(s.H, 1), s.M), (s.id, info)
        cls, nums = host
        assert GM.info_class(info) == cls, (s.id, len(workers), GM.info_class(info), cls, info)
        assert GM.info_numbers(info) == nums, (s.id, len(workers), info, nums)
        # (d), (e) the searched cells; (f) the others
        mx, am, sm = words[0].view(np.float32), words[1], words[2].view(np.float32)
        on = np.zeros(P, bool)
        on[list(workers)] = True
        bad = np.argwhere(am[on] != self.want[on])
        assert len(bad) == 0, (s.id, len(workers), len(bad), [(int(self.want[on][p, d]), int(am[on][p, d])) for p, d in bad[:32]])
        wmx = float(np.max(np.abs(mx[on].astype(np.float64) / self.emx - 1.0)))
        wsm = float(np.max(np.abs(sm[on].astype(np.float64) / self.esm - 1.0)))
        self.worst = [max(self.worst[0], wmx), max(self.worst[1], wsm)]
        assert wmx <= REL and wsm <= REL, (s.id, len(workers), wmx, wsm)
        assert (words[:, ~on, :] == SENTINEL).all(), (s.id, "a cell of a masked worker was written")
        return words, info

    def report(self, n_searches):
        print("%s [%s]: %d searches of %d x %d cells, worst max rel %.2e, worst sum rel %.2e"
              % (self.s.id, self.s.cls, n_searches, self.s.P, self.s.D, self.worst[0], self.worst[1]))


def _ids(shapes):
    return pytest.mark.parametrize("s", shapes, ids=[s.id for s in shapes])


@_ids(GM.SHAPES)
def test_every_class_of_the_grid_on_every_kernel_copy(gpu, hipbuf, host_plans, s):
    from gnss_sdr_rs_amd import _lib, acquisition as A
    run = Run(A, _lib, hipbuf, s, GM.SHAPES.index(s))
    try:
        assert s.cls == host_plans[(s.id, s.n_workers)][0]
        first, _ = run.search(s.workers, host_plans[(s.id, s.n_workers)])
        again, _ = run.search(s.workers, host_plans[(s.id, s.n_workers)])        # (g)
        assert (first == again).all(), (s.id, int((first != again).sum()))
    finally:
        run.close()
    run.report(2)


@_ids(GM.CUT_SHAPES)
def test_a_cell_does_not_depend_on_whether_its_item_was_cut(gpu, hipbuf, host_plans, s):
    """the full list, the lowest worker dropped, all but the last dropped: the classes the host plan names, and equal words"""
    from gnss_sdr_rs_amd import _lib, acquisition as A
    run = Run(A, _lib, hipbuf, s)
    try:
        full, i0 = run.search(range(s.P), host_plans[(s.id, s.P)])
        less, i1 = run.search(range(1, s.P), host_plans[(s.id, s.P - 1)])
        one, i2 = run.search([s.P - 1], host_plans[(s.id, 1)])
        assert (less[:, 1:, :] == full[:, 1:, :]).all() and (one[:, s.P - 1, :] == full[:, s.P - 1, :]).all(), s.id
        print("%s: classes %s | %s | %s" % (s.id, GM.info_class(i0), GM.info_class(i1), GM.info_class(i2)))
    finally:
        run.close()
    run.report(3)


@_ids(GM.EDGE_SHAPES)
def test_edge_search_bins_against_a_scratch_sized_for_the_handle(gpu, hipbuf, host_plans, s):
    """H = 3 hypotheses of a two-period coherent handle on the constant dwell: stage C runs 3 D bins, every hypothesis plane of a cell
    peaks at the cell's lag, the reduction keeps hypothesis 0 (the lowest on ties)"""
    from gnss_sdr_rs_amd import _lib, acquisition as A
    run = Run(A, _lib, hipbuf, s)
    try:
        first, info = run.search(s.workers, host_plans[(s.id, s.n_workers)])
        mx, am, sm = run.eng.edge_metrics()
        assert (am == run.want[:, None, :]).all(), (s.id, int((am != run.want[:, None, :]).sum()))
        assert float(np.max(np.abs(mx.astype(np.float64) / run.emx - 1.0))) <= REL and float(np.max(np.abs(sm.astype(np.float64) / run.esm - 1.0))) <= REL
        assert (mx[:, 0, :].view(np.uint32) == first[0]).all() and (run.eng.edge_choice() == 0).all()
        again, _ = run.search(s.workers, host_plans[(s.id, s.n_workers)])
        assert (first == again).all()
    finally:
        run.close()
    run.report(2)


def test_prepared_search_on_an_all_cut_grid(gpu, hipbuf, host_plans):
    """gm_acq_prepare_dev + gm_acq_search_prepared_dev: stage F ran ahead on another stream, so the merge tickets are cleared by corr()'s
    own memset; twice on one handle, between two ordinary searches"""
    from gnss_sdr_rs_amd import _lib, acquisition as A
    s = GM.PREPARED_SHAPE
    run = Run(A, _lib, hipbuf, s)
    try:
        host = host_plans[(s.id, s.n_workers)]
        a, info = run.search(s.workers, host)
        assert info["cut"] == GM.CUT["all"]
        b, _ = run.search(s.workers, host, prepared=True)
        c, _ = run.search(s.workers, host, prepared=True)
        d, _ = run.search(s.workers, host)
        assert (a == b).all() and (a == c).all() and (a == d).all()
    finally:
        run.close()
    run.report(4)


def _child(index):
    """the body of the tiled-walk child process: one search of TILED_SHAPES[index], its record and its wrong cells as a JSON line"""
    from conftest import HipBuffers
    from gnss_sdr_rs_amd import _lib, acquisition as A
    _lib.init(0)
    s = GM.TILED_SHAPES[index]
    hipbuf = HipBuffers()
    run = Run(A, _lib, hipbuf, s)
    try:
        P, D = s.P, s.D
        d_met = hipbuf.upload(np.full(3 * P * D, SENTINEL, np.uint32))
        run.eng.search_dev(run.d_x, run.fmt, d_met)
        run.eng.synchronize()
        w = hipbuf.download(d_met, 3 * P * D * 4, np.uint32).reshape(3, P, D)
        info = run.eng.debug_corr_grid()
        out = dict(info=info, cls=GM.info_class(info), wrong=int((w[1] != run.want).sum()),
                   max_rel=float(np.max(np.abs(w[0].view(np.float32).astype(np.float64) / run.emx - 1.0))),
                   sum_rel=float(np.max(np.abs(w[2].view(np.float32).astype(np.float64) / run.esm - 1.0))))
    finally:
        run.close()
        hipbuf.close()
    print(json.dumps(out))


@pytest.mark.parametrize("index", range(len(GM.TILED_SHAPES)), ids=[s.id for s in GM.TILED_SHAPES])
def test_diagnostic_tiled_walk_in_a_child_process(gpu, host_plans, index):
    """map_mode >= 16 is reached through GM_DIAGNOSTICS=1 GM_CORR_CB=4 only, read once per process: a child of its own per kernel copy"""
    s = GM.TILED_SHAPES[index]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GM_")}
    env.update(GM_DIAGNOSTICS="1", GM_CORR_CB="4")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_grid_geometry as T; T._child(%d)" % (ROOT, os.path.join(ROOT, "tests"), index)
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    cls, nums = host_plans[(s.id, s.n_workers)]
    print("%s: %s, %d wrong lags, max rel %.2e, sum rel %.2e" % (s.id, out["cls"], out["wrong"], out["max_rel"], out["sum_rel"]))
    assert out["cls"] == cls == s.cls and GM.info_numbers(out["info"]) == nums and out["info"]["map_mode"] >> 4 == 4, (out, cls, nums)
    assert out["info"]["path"] == GM.KERNELS[s.kernel]["path"]
    assert out["wrong"] == 0 and out["max_rel"] <= REL and out["sum_rel"] <= REL, out
