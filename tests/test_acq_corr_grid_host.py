"""CPU: tests/cpu/test_acq_corr_grid.cpp — how stage C's workgroups are dealt onto (worker, bin, integration) items
(csrc/acq_corr_grid.h): the launcher's plan held to the host mirrors of the device decodes over n_workers 1..70 x n_bins 1..512, that
the check fails for a wrong decode, and that every class the sweep reaches has a shape in the GPU test's table (acq_grid_model.py)."""
import re
import subprocess

import pytest

import acq_grid_model as GM
import acq_sweep_model as SW


def _run(*args):
    r = subprocess.run([GM.binary(), *args], stdout=subprocess.PIPE, text=True, timeout=600)
    return r.returncode, r.stdout


@pytest.fixture(scope="module")
def output():
    return _run()


def test_grid_program_passes(output):
    """Anchors, the sweep (n_workers 1..70 x n_bins 1..512, H in {1, 3}, n_int in {1, 2, 3, 5, 15, 16, 17}, WG_PER_CU in {1, 2},
    split_planes of every P >= n_workers up to 70), the composite walk with cb 0 and 4, the tiled walk of the in-LDS kernels and the long
    slabs: the program exits non-zero on any failure."""
    rc, text = output
    assert rc == 0, text[-3000:]
    assert "acq_corr_grid: 0 failed" in text
    m = re.search(r"sweep: (\d+) plans, (\d+) uncut walks, (\d+) whole grids block by block", text)
    assert m and int(m.group(1)) > 1_000_000 and int(m.group(2)) >= 70 * 512 and int(m.group(3)) > 300_000, text[-2000:]
    assert len(re.findall(r"^anchor ", text, re.M)) == 6


@pytest.mark.parametrize("wrong", ["each_floor", "swap_hk"])
def test_a_wrong_decode_fails_the_program(wrong):
    """The check has teeth: with the leftover share of map 2 rounded down instead of up (items never visited), or h / split_k
    exchanged with h % split_k (parts of one item handed to another), the same program fails."""
    rc, text = _run("--wrong=" + wrong)
    assert rc == 1, text[-2000:]
    m = re.search(r"acq_corr_grid: (\d+) failed", text)
    assert m and int(m.group(1)) > 0 and "FAIL" in text


def test_clamps_on_split_items_are_unreachable(output):
    """while a launch's n_int is the handle's M, neither the GM_CORR_SPLIT_MAX_ITEMS clamp nor the split_planes clamp on
    split_items changes a plan of the sweep, and the classes `share`, `clamped` and `off` are never reached."""
    rc, text = output
    assert "clamps on split_items that would have bitten: MAX_ITEMS 0, split_planes 0" in text
    census = set(re.findall(r"^class (.*)$", text, re.M))
    assert not [c for c in census if "why=share" in c or "why=clamped" in c or "why=off" in c]


def test_every_class_of_the_census_has_a_shape_in_the_gpu_table(output):
    """A class the launcher can reach and no GPU shape runs fails here: add a shape to acq_grid_model.py."""
    rc, text = output
    census = set(re.findall(r"^class (.*)$", text, re.M))
    assert len(census) >= 61, sorted(census)
    declared = {s.cls for s in GM.SHAPES}
    assert census <= declared, sorted(census - declared)
    # both kernel copies of every path that has two
    for k in GM.KERNELS:
        assert any(s.kernel == k for s in GM.SHAPES), k


def test_every_shape_is_in_the_class_it_declares():
    """The table's declarations against the plan functions: the main table, the masked second passes, the edge searches, the
    prepared search and the tiled walk."""
    from gnss_sdr_rs_amd import acquisition as A
    L = {}
    for k, v in GM.KERNELS.items():
        st, info = A.plan_info(v["N"], v["form"].startswith("long"))
        assert st == 0 and (info["form"], info["base"]) == (v["form"], v["base"]), (k, info)
        L[k] = info["transform_len"]
    shapes = GM.SHAPES + GM.EDGE_SHAPES + [GM.PREPARED_SHAPE]
    got = GM.classify([s.line(L=L[s.kernel]) for s in shapes])
    for s, (cls, nums) in zip(shapes, got):
        assert cls == s.cls, (s.id, cls, s.cls)
    for s, (cls, nums) in zip(GM.TILED_SHAPES, GM.classify([s.line(cb_env=4) for s in GM.TILED_SHAPES])):
        assert cls == s.cls and nums[0] >> 4 == 4, (s.id, cls, nums)
    # dropping workers moves a cut shape into another class (what the second pass of the GPU test is for) at least once per cut kind
    moved = set()
    for s in GM.CUT_SHAPES:
        a, b = GM.classify([s.line(n_workers=s.P - 1), s.line(n_workers=1)])
        moved |= {(s.cls.split()[3], a[0].split()[3]), (s.cls.split()[3], b[0].split()[3])}
    assert ("cut=tail", "cut=all") in moved, moved
    assert {s.kernel for s in GM.CUT_SHAPES} == {"lds1", "lds2", "ws31"} and {s.cls.split()[3] for s in GM.CUT_SHAPES} == {"cut=all", "cut=tail"}
    ids = [s.id for s in GM.SHAPES + GM.EDGE_SHAPES]
    assert len(set(ids)) == len(ids)


def test_the_scene_gives_every_cell_a_lag_of_its_own():
    for s in GM.SHAPES + GM.EDGE_SHAPES + GM.TILED_SHAPES:
        want = GM.expected_lags(s.N, s.P, s.D)
        assert want.shape == (s.P, s.D) and int(want.max()) < s.N
        r, sh = GM.shifts(s.N, s.P, s.D)
        assert (SW.expected_lags(s.N, r, sh) == want).all() and r.shape == (s.P,) and sh.shape == (s.D,)
