"""CPU: tests/cpu/test_trk_persist_plan.cpp — the persistent tracking kernel's launch layout (csrc/trk_persist_plan.h), decided by one
pure host function: what layout a configuration gets, and that every layout it can give keeps its grid resident."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def output():
    """The program built with the g++ line of test_abi_and_host.py: the header includes no HIP header"""
    exe = os.path.join(tempfile.mkdtemp(prefix="gm_trkplan_"), "test_trk_persist_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "test_trk_persist_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=60)
    return r.returncode, r.stdout


def test_plan_program_passes(output):
    """Anchors, the invariant sweep (channels 1..129, 256, 512, 1024 x arms x four sample rates x share_device x 64 / 256 CUs x 1 / 2
    workgroups per CU), the residency rule where FAIR3 is possible, the diagnostic overrides and stamps_fit: the program exits
    non-zero on any failure."""
    rc, text = output
    assert rc == 0, text[-3000:]
    assert "trk_persist_plan: 0 failed" in text
    assert "invariants: %d points" % (132 * 2 * 4 * 2 * 2 * 2) in text


def test_anchor_layouts_are_the_documented_ones(output):
    """The layouts the README and DESIGN.md quote, read back from the program's own listing: 36 channels of five arms on a 4092-chip
    code at 25 Msps take 14 workgroups each, packed, 504 of the 512 places; with share_device 3 each, 120 places."""
    rc, text = output
    rows = {}
    for m in re.finditer(r"^anchor C=(\d+) arms=(\d) fs=(\S+) len=(\d+) share=(\d) -> G=(\d+) packed=(\d+) grid=(\d+) per=(\d+) fair_share=(\d+) fair3=(\d)", text, re.M):
        c, arms, fs, ln, share, g, packed, grid, per, fair, fair3 = m.groups()
        rows[(int(c), int(arms), float(fs), int(ln), int(share))] = (int(g), int(packed), int(grid), int(per), int(fair), int(fair3))
    assert len(rows) == 11
    assert rows[(36, 5, 25e6, 4092, 0)] == (14, 63, 504, 7168, 32, 0)
    assert rows[(36, 3, 25e6, 4092, 0)] == (14, 63, 504, 7168, 32, 1)
    assert rows[(36, 5, 25e6, 4092, 1)] == (3, 0, 120, 33472, 32, 0)
    assert rows[(32, 3, 25e6, 1023, 0)] == (16, 0, 512, 1600, 0, 0)
