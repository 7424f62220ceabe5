"""CPU: tests/cpu/test_fused_twiddles.cpp — the constant twiddles folded into the radix-25 / radix-16 butterflies (csrc/fft_core.h
BflyTw) against the plain Bfly + ConstTw path, butterfly by butterfly, and the whole Hybrid8000 inverse against the plain header's."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def outputs():
    """The program built twice with the g++ line of test_abi_and_host.py: as shipped, and with -DGM_NO_FUSED_TW (the plain form everywhere)"""
    tmp = tempfile.mkdtemp(prefix="gm_fusedtw_")
    out = {}
    for name, extra in (("fused", []), ("plain", ["-DGM_NO_FUSED_TW"])):
        exe = os.path.join(tmp, "test_fused_twiddles_" + name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpu", "test_fused_twiddles.cpp"), "-o", exe], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=600)
        out[name] = (r.returncode, r.stdout)
    return out


def test_every_twiddle_row_fused_against_plain(outputs):
    """Both directions, (R, M, K) = (25, 125, 0..4) and (16, 64, 0..3), 2000 random butterflies each: every output finite, the fused
    path's largest relative error at most 1.5 x the plain path's on the same inputs (the program exits non-zero otherwise)."""
    rc, text = outputs["fused"]
    assert rc == 0, text[-3000:]
    rows = re.findall(r"^row R=\s*(\d+) M=\s*(\d+) K=(\d) (inv|fwd)\s+fused_max=(\S+) plain_max=(\S+) ratio=(\S+) (\S+)", text, re.M)
    assert sorted((int(r), int(m), int(k), d) for r, m, k, d, *_ in rows) == sorted(
        [(25, 125, k, d) for k in range(5) for d in ("inv", "fwd")] + [(16, 64, k, d) for k in range(4) for d in ("inv", "fwd")])
    for r, m, k, d, f, p, ratio, verdict in rows:
        print(r, m, k, d, f, p, ratio)
        assert verdict == "ok" and float(f) <= 1.5 * float(p) and 0.0 < float(p) < 1e-5, (r, m, k, d, f, p)
    r20 = re.findall(r"^row20 .* (inv|fwd)\s+fused_max=(\S+) plain_max=(\S+) ratio=(\S+) (\S+)", text, re.M)
    assert sorted(d for d, *_ in r20) == ["fwd", "inv"]            # pass 0's radix 20 with the multiply-free radix 5 as its second layer
    for d, f, p, ratio, verdict in r20:
        print(20, d, f, p, ratio)
        assert verdict == "ok" and float(f) <= 1.5 * float(p) and 0.0 < float(p) < 1e-5, (d, f, p)
    assert "rows: 0 failed" in text


def test_whole_hybrid8000_inverse_fused_against_plain(outputs):
    """The Hybrid8000 inverse (the transform of acq_corr_kernel at N = 8000) as the product's CorrPlan8000 runs it stays within 1.25 x the relative L2
    error of the same program compiled with -DGM_NO_FUSED_TW."""
    (rc_f, fused), (rc_p, plain) = outputs["fused"], outputs["plain"]
    assert rc_f == 0 and rc_p == 0
    assert "fused=1" in fused and "fused=0" in plain          # the product's plan runs the fused form; the macro turns it off
    err = lambda t: float(re.search(r"Hybrid8000 inv rel_l2_err=(\S+)", t).group(1))
    print("Hybrid8000 inv: fused %.4e plain %.4e ratio %.3f" % (err(fused), err(plain), err(fused) / err(plain)))
    assert 0.0 < err(plain) < 7e-7
    assert err(fused) <= 1.25 * err(plain), (err(fused), err(plain))
