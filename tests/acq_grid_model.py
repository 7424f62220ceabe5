"""Stage C's grid geometry: the shape table of tests/test_gpu_grid_geometry.py, the class each shape declares, and the scene.

A helper module like acq_sweep_model.py, not a test.  Shared by tests/test_acq_corr_grid_host.py (CPU: every class of the census of
tests/cpu/test_acq_corr_grid.cpp has a shape here, and every shape's declared class is what the plan functions of
csrc/acq_corr_grid.h give) and tests/test_gpu_grid_geometry.py (GPU: every shape run, the class confirmed by gm_acq_debug_corr_grid).

A class is what the launcher decides for a grid: (path, workgroups per CU of the plan, tile map, which items are cut and — where none
is — the first rule that forbade it, one resident round or several).  The shapes are the smallest (P x D, then M) of each class found
by enumerating P <= 64, D <= 128 through the CPU binary; where the binary and this table disagree the host test fails, and a class
added to the launcher fails there until a shape runs it.

The scene is acq_sweep_model.py's: worker p's code is roll(b, r_p), bin d's mix table roll(b, s_d), the dwell constant, so cell (p, d)
peaks at (s_d - r_p) mod N.  Here ONE search puts every cell on a lag of its own, (d P + p) * floor(N / (P D)): a workgroup that
computes another item's cell, a cell twice and another never, or merges parts of two items shows as a wrong lag, a wrong max or a
word that still holds the sentinel."""
import os
import subprocess
import tempfile

import numpy as np

import acq_sweep_model as SW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gm_acq_corr_grid_info.path / .cut / .why (include/gnss_mi355x.h)
PATH_LDS, PATH_LDS_WS31, PATH_COMP, PATH_COMP_WS, PATH_LONG = 1, 2, 3, 4, 5
CUT = {"none": 0, "all": 1, "tail": 2}
WHY = {"cut": 0, "m1": 1, "strict": 2, "off": 3, "share": 4, "max_k": 5, "scratch": 6, "one_wg_rounds": 7, "clamped": 8}

# the smallest size that reaches each kernel copy: fft_size, what plan_info says of it, the export's path, WG_PER_CU of the plan
KERNELS = {
    "lds2": dict(N=1024, form="lds", base=1024, path=PATH_LDS, wg=2),               # acq_corr_kernel, two workgroups per CU
    "lds1": dict(N=12000, form="lds", base=12000, path=PATH_LDS, wg=1),             # acq_corr_kernel, one workgroup per CU
    "ws31": dict(N=16368, form="lds", base=16368, path=PATH_LDS_WS31, wg=1),        # acq_corr_ws31_kernel
    "comp": dict(N=18000, form="composite", base=6000, path=PATH_COMP, wg=0),       # comp_corr_kernel, 3 x 6000
    "comp_ws": dict(N=32000, form="composite", base=16000, path=PATH_COMP_WS, wg=0),  # comp_corr_ws_kernel, 2 x 16000
    "long": dict(N=6144, form="long", base=2048, path=PATH_LONG, wg=0),             # launch_long_corr, 3 x 2048
}


class Shape:
    """One handle: `kernel` of KERNELS, P codes x D bins x M integrations; `drop`: worker indices masked off before the search
    (gm_acq_set_prn_mask); H > 0: an edge search of H hypotheses on a handle of two coherent periods (stage C sees H * D bins against a
    scratch sized for P * D); cls: the class the shape declares for that launch."""

    def __init__(self, kernel, P, D, M, strict, cls, drop=(), H=0):
        self.kernel, self.P, self.D, self.M, self.strict, self.drop, self.H = kernel, P, D, M, bool(strict), tuple(drop), H
        k = KERNELS[kernel]
        self.N, self.wg = k["N"], k["wg"]
        self.cls = ("lds wg=%d %s" % (self.wg, cls)) if k["form"] == "lds" else cls
        self.id = "%s-%dx%d-M%d%s%s%s" % (kernel, P, D, M, "-strict" if strict else "", "-drop%d" % len(drop) if drop else "", "-H%d" % H if H else "")
        assert P * D <= self.N and P <= 64

    @property
    def n_workers(self):
        return self.P - len(self.drop)

    @property
    def workers(self):
        return [p for p in range(self.P) if p not in self.drop]

    @property
    def mask(self):
        return sum(1 << p for p in self.workers)

    @property
    def K(self):
        return 2 if self.H else 1

    def line(self, n_workers=None, L=None, cb_env=-1):
        """the shape as tests/cpu/test_acq_corr_grid.cpp --shapes reads it"""
        nw = self.n_workers if n_workers is None else n_workers
        form = KERNELS[self.kernel]["form"]
        if form == "lds":
            return "lds %d %d %d %d %d %d %d %d" % (self.P, self.D, self.M, nw, max(self.H, 1), self.wg, int(self.strict), cb_env)
        if form == "composite":
            return "comp %d %d %d" % (nw, self.D * max(self.H, 1), cb_env)
        return "long %d %d %d %d %d %d" % (self.P, self.D, self.M, self.N if L is None else L, nw, max(self.H, 1))


# (kernel, P, D, M, strict, class): one shape per in-LDS class of the census, on the generic kernel of each WG_PER_CU
_LDS = [
    ("lds1", 33, 1, 2, 0, "map=0 cut=all why=cut rounds=one"),
    ("lds1", 33, 1, 1, 0, "map=0 cut=none why=m1 rounds=one"),
    ("lds1", 33, 9, 1, 0, "map=0 cut=none why=m1 rounds=several"),
    ("lds1", 33, 1, 17, 0, "map=0 cut=none why=max_k rounds=one"),
    ("lds1", 33, 9, 17, 0, "map=0 cut=none why=max_k rounds=several"),
    ("lds1", 33, 9, 2, 0, "map=0 cut=none why=one_wg_rounds rounds=several"),
    ("lds1", 18, 9, 16, 0, "map=0 cut=none why=scratch rounds=one"),
    ("lds1", 33, 1, 2, 1, "map=0 cut=none why=strict rounds=one"),
    ("lds1", 33, 9, 2, 1, "map=0 cut=none why=strict rounds=several"),
    ("lds1", 1, 1, 2, 0, "map=1 cut=all why=cut rounds=one"),
    ("lds1", 1, 1, 1, 0, "map=1 cut=none why=m1 rounds=one"),
    ("lds1", 3, 86, 1, 0, "map=1 cut=none why=m1 rounds=several"),
    ("lds1", 7, 23, 17, 0, "map=1 cut=none why=max_k rounds=one"),
    ("lds1", 3, 86, 17, 0, "map=1 cut=none why=max_k rounds=several"),
    ("lds1", 3, 86, 2, 0, "map=1 cut=none why=one_wg_rounds rounds=several"),
    ("lds1", 7, 23, 16, 0, "map=1 cut=none why=scratch rounds=one"),
    ("lds1", 1, 1, 2, 1, "map=1 cut=none why=strict rounds=one"),
    ("lds1", 3, 86, 2, 1, "map=1 cut=none why=strict rounds=several"),
    ("lds1", 2, 1, 2, 0, "map=2 cut=all why=cut rounds=one"),
    ("lds1", 2, 1, 1, 0, "map=2 cut=none why=m1 rounds=one"),
    ("lds1", 6, 43, 1, 0, "map=2 cut=none why=m1 rounds=several"),
    ("lds1", 23, 7, 17, 0, "map=2 cut=none why=max_k rounds=one"),
    ("lds1", 6, 43, 17, 0, "map=2 cut=none why=max_k rounds=several"),
    ("lds1", 6, 43, 2, 0, "map=2 cut=none why=one_wg_rounds rounds=several"),
    ("lds1", 23, 7, 16, 0, "map=2 cut=none why=scratch rounds=one"),
    ("lds1", 2, 1, 2, 1, "map=2 cut=none why=strict rounds=one"),
    ("lds1", 6, 43, 2, 1, "map=2 cut=none why=strict rounds=several"),
    ("lds2", 33, 9, 2, 0, "map=0 cut=all why=cut rounds=one"),
    ("lds2", 33, 9, 1, 0, "map=0 cut=none why=m1 rounds=one"),
    ("lds2", 43, 17, 1, 0, "map=0 cut=none why=m1 rounds=several"),
    ("lds2", 33, 9, 17, 0, "map=0 cut=none why=max_k rounds=one"),
    ("lds2", 43, 17, 17, 0, "map=0 cut=none why=max_k rounds=several"),
    ("lds2", 33, 9, 16, 0, "map=0 cut=none why=scratch rounds=one"),
    ("lds2", 33, 9, 2, 1, "map=0 cut=none why=strict rounds=one"),
    ("lds2", 43, 17, 2, 1, "map=0 cut=none why=strict rounds=several"),
    ("lds2", 43, 17, 2, 0, "map=0 cut=tail why=cut rounds=several"),
    ("lds2", 1, 1, 2, 0, "map=1 cut=all why=cut rounds=one"),
    ("lds2", 1, 1, 1, 0, "map=1 cut=none why=m1 rounds=one"),
    ("lds2", 5, 103, 1, 0, "map=1 cut=none why=m1 rounds=several"),
    ("lds2", 7, 23, 17, 0, "map=1 cut=none why=max_k rounds=one"),
    ("lds2", 5, 103, 17, 0, "map=1 cut=none why=max_k rounds=several"),
    ("lds2", 7, 23, 16, 0, "map=1 cut=none why=scratch rounds=one"),
    ("lds2", 1, 1, 2, 1, "map=1 cut=none why=strict rounds=one"),
    ("lds2", 5, 103, 2, 1, "map=1 cut=none why=strict rounds=several"),
    ("lds2", 5, 103, 2, 0, "map=1 cut=tail why=cut rounds=several"),
    ("lds2", 2, 1, 2, 0, "map=2 cut=all why=cut rounds=one"),
    ("lds2", 2, 1, 1, 0, "map=2 cut=none why=m1 rounds=one"),
    ("lds2", 9, 57, 1, 0, "map=2 cut=none why=m1 rounds=several"),
    ("lds2", 23, 7, 17, 0, "map=2 cut=none why=max_k rounds=one"),
    ("lds2", 9, 57, 17, 0, "map=2 cut=none why=max_k rounds=several"),
    ("lds2", 23, 7, 16, 0, "map=2 cut=none why=scratch rounds=one"),
    ("lds2", 2, 1, 2, 1, "map=2 cut=none why=strict rounds=one"),
    ("lds2", 9, 57, 2, 1, "map=2 cut=none why=strict rounds=several"),
    ("lds2", 9, 57, 2, 0, "map=2 cut=tail why=cut rounds=several"),
    # an odd part count, on the tail and on every item
    ("lds2", 43, 17, 3, 0, "map=0 cut=tail why=cut rounds=several"),
    ("lds2", 33, 9, 3, 0, "map=0 cut=all why=cut rounds=one"),
    # acq_corr_ws31_kernel holds its own copy of the decode: the three maps on several rounds (never cut), and every item cut
    ("ws31", 33, 9, 2, 0, "map=0 cut=none why=one_wg_rounds rounds=several"),
    ("ws31", 3, 86, 2, 0, "map=1 cut=none why=one_wg_rounds rounds=several"),
    ("ws31", 6, 43, 2, 0, "map=2 cut=none why=one_wg_rounds rounds=several"),
    ("ws31", 33, 1, 2, 0, "map=0 cut=all why=cut rounds=one"),
    ("ws31", 2, 1, 3, 0, "map=2 cut=all why=cut rounds=one"),
    ("ws31", 7, 23, 16, 0, "map=1 cut=none why=scratch rounds=one"),
]
# composite: n_workers 1 and 4 walk the list in order (cb = 0), 5, 6, 7 and 36 in blocks of cb = 4 workers, ragged against it, over 1, 9
# and 41 bins; 7 workers are 8 codes with the lowest masked off.  One strict_sum_order case per kernel: the plane-storing instantiation.
_COMP = [
    (1, 9, 1, 0, "comp cb=0 rounds=one", ()), (4, 41, 2, 0, "comp cb=0 rounds=one", ()), (4, 70, 1, 0, "comp cb=0 rounds=several", ()),
    (5, 1, 1, 0, "comp cb=4 rounds=one", ()), (6, 9, 2, 0, "comp cb=4 rounds=one", ()), (8, 41, 1, 0, "comp cb=4 rounds=several", (0,)),
    (36, 9, 2, 0, "comp cb=4 rounds=several", ()), (5, 9, 1, 1, "comp cb=4 rounds=one", ()),
]
# long, N = 6144 = 3 x 2048 (slabs of 2730 items at M = 1, 1365 at M = 2): one slab; two slabs with a ragged last one and the boundary
# inside a bin (2730 = 248 * 11 + 2; 1365 = 124 * 11 + 1); two whole slabs
_LONG = [
    (8, 8, 1, "long slabs=one"), (11, 250, 1, "long slabs=several_ragged"), (11, 130, 2, "long slabs=several_ragged"),
    (13, 210, 2, "long slabs=several"),
]

SHAPES = ([Shape(*row) for row in _LDS] +
          [Shape(k, P, D, M, s, cls, drop) for k in ("comp", "comp_ws") for P, D, M, s, cls, drop in _COMP] +
          [Shape("long", P, D, M, 0, cls) for P, D, M, cls in _LONG])
# the second pass of every in-LDS shape with a cut: the lowest worker dropped, then all but the last one
CUT_SHAPES = [s for s in SHAPES if KERNELS[s.kernel]["form"] == "lds" and "why=cut" in s.cls and s.P > 1]
# an edge search at H = 3 per in-LDS kernel: 3 D bins against a scratch sized for P x D
EDGE_SHAPES = [Shape("lds2", 8, 32, 2, 0, "map=1 cut=tail why=cut rounds=several", H=3),
               Shape("lds1", 8, 32, 2, 0, "map=1 cut=none why=one_wg_rounds rounds=several", H=3),
               Shape("ws31", 9, 19, 2, 0, "map=2 cut=none why=one_wg_rounds rounds=several", H=3)]
# gm_acq_prepare_dev + gm_acq_search_prepared_dev on an all-cut shape: the tickets are cleared by corr()'s memset, not by stage F
PREPARED_SHAPE = Shape("lds2", 33, 9, 2, 0, "map=0 cut=all why=cut rounds=one")
# the diagnostic tiled walk (GM_DIAGNOSTICS=1 GM_CORR_CB=4), one child process per in-LDS kernel copy
TILED_SHAPES = [Shape("lds2", 8, 8, 2, 0, "map=16 cut=all why=cut rounds=one"), Shape("ws31", 8, 8, 2, 0, "map=16 cut=all why=cut rounds=one")]


# ---- the CPU binary ----------------------------------------------------------------------------------------------------------------------
_EXE = None


def binary():
    """tests/cpu/test_acq_corr_grid.cpp compiled with g++ (once per process)"""
    global _EXE
    if _EXE is None:
        exe = os.path.join(tempfile.mkdtemp(prefix="gm_corrgrid_"), "test_acq_corr_grid")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I", os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpu", "test_acq_corr_grid.cpp"), "-o", exe], check=True)
        _EXE = exe
    return _EXE


def classify(lines):
    """[(class, [numbers])] per shape line, by the plan functions of csrc/acq_corr_grid.h (the binary's --shapes).  Numbers: lds
    map_mode share slots split_from split_k split_items grid cut why split_planes; comp cb rows_max slots; long long_slab long_slabs."""
    r = subprocess.run([binary(), "--shapes"], input="".join(l + "\n" for l in lines), stdout=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:]
    out = []
    for l in r.stdout.splitlines():
        head, nums = l.split(" | ")
        out.append((head.split(" -> ")[1], [int(v) for v in nums.split()]))
    assert len(out) == len(lines)
    return out


LDS_FIELDS = ("map_mode", "share", "slots", "split_from", "split_k", "split_items", "grid", "cut", "why", "split_planes")
COMP_FIELDS = ("cb", "rows_max", "slots")
LONG_FIELDS = ("long_slab", "long_slabs")


def info_class(info):
    """the class string of a gm_acq_corr_grid_info dict, built from the export's own fields as the binary builds it from the plan"""
    cut = {v: k for k, v in CUT.items()}
    why = {v: k for k, v in WHY.items()}
    if info["path"] in (PATH_LDS, PATH_LDS_WS31):
        return "lds wg=%d map=%d cut=%s why=%s rounds=%s" % (info["wg_per_cu"], min(info["map_mode"], 16), cut[info["cut"]], why[info["why"]],
                                                             "one" if info["share"] <= info["slots"] else "several")
    if info["path"] in (PATH_COMP, PATH_COMP_WS):
        return "comp cb=%d rounds=%s" % (info["cb"], "one" if info["slots"] <= 32 else "several")
    assert info["path"] == PATH_LONG, info
    items = info["n_workers"] * info["n_bins"]
    return "long slabs=" + ("one" if info["long_slabs"] <= 1 else "several_ragged" if items % info["long_slab"] else "several")


def info_numbers(info):
    f = LDS_FIELDS if info["path"] in (PATH_LDS, PATH_LDS_WS31) else COMP_FIELDS if info["path"] in (PATH_COMP, PATH_COMP_WS) else LONG_FIELDS
    return [info[k] for k in f]


# ---- the scene -----------------------------------------------------------------------------------------------------------------------------
def shifts(N, P, D):
    """(r [P], s [D]): cell (p, d) peaks at (s_d - r_p) mod N = (d P + p) * floor(N / (P D)), a lag no other cell of the search has"""
    assert P * D <= N
    g = N // (P * D)
    c = int(np.random.default_rng(79000 + N + 7 * P + D).integers(0, N))
    return (c - g * np.arange(P, dtype=np.int64)) % N, (c + g * P * np.arange(D, dtype=np.int64)) % N


def expected_lags(N, P, D):
    r, s = shifts(N, P, D)
    want = SW.expected_lags(N, r, s)
    assert len(np.unique(want)) == P * D
    return want
