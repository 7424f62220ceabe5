"""CPU: tests/fft_model.py against the sources it restates, and evidence that its bound separates right from subtly wrong.

No device code runs here.  The table of radices is parsed out of csrc/fft_plans.h; `split` and `bluestein_L` are held to the facts
read from gm_api.hip (pow2_split, bluestein_len); on every in-LDS size the float64 transform with ONE twiddle index off by one is
outside B's bound on the impulse batch by a factor of ten or more, and the float64 transform rounded to float32 is inside it."""
import os
import re

import numpy as np
import pytest

import fft_model as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc")


def test_radix_table_equals_the_header(gm):
    text = open(os.path.join(CSRC, "fft_plans.h")).read()
    text = re.sub(r"\\\n", " ", text)                                   # macro bodies on continued lines
    found = {}
    for n, t, rs in re.findall(r"\bPlan<\s*(\d+)\s*,\s*(\d+)\s*((?:,\s*\d+\s*)+)>", text):
        plan = (int(t), tuple(int(r) for r in re.findall(r"\d+", rs)))
        assert found.setdefault(int(n), plan) == plan, n                # one definition per length
    assert len(re.findall(r"#define GM_PLAN_\d+ Plan<", text)) == 3     # the three macro bodies are among them
    assert found == M.RADICES
    listed = re.search(r"#define GM_FOR_EACH_PLAN\(X\)(.*?)#endif", text, re.S).group(1)
    assert sorted(int(n) for n in re.findall(r"X\(gm::Plan(\d+)\)", listed)) == sorted(M.RADICES)
    from gnss_sdr_rs_amd import fft
    assert sorted(fft.supported_sizes()) == sorted(M.RADICES) and len(M.RADICES) == 18
    for n, (t, rs) in M.RADICES.items():
        assert int(np.prod(rs)) == n and all(r in M.K for r in rs)
    assert M.POW2_PLANS == (256, 512, 1024, 2048, 4096, 8192, 16384)


def test_bound_is_not_below_the_first_order_count():
    """B was raised above the (r + 8)-per-pass count where the code rounds more often (the twiddle power tree): never below it"""
    for n in M.RADICES:
        assert M.B(n) >= M.first_order_count(n), n
    for p in M.POW2_PLANS:
        assert M.B(p, 256) >= M.first_order_count(p, 256) and M.B(256, p) == M.B(p, 256)
    assert abs(M.B(16384) - 104.51) < 0.01 and abs(M.B(16368) - 184.82) < 0.01 and abs(M.B(256) - 54.61) < 0.01


def test_split_pairs():
    facts = {32768: None, 1 << 16: (256, 256), 1 << 17: (512, 256), 1 << 18: (1024, 256), 1 << 22: (16384, 256),
             1 << 23: (16384, 512), 1 << 24: (16384, 1024), 1 << 28: (16384, 16384)}
    for n, pair in facts.items():
        assert M.split(n) == pair, n
    for lg in range(16, 29):
        n1, n2 = M.split(1 << lg)
        assert n1 * n2 == 1 << lg and n1 >= n2 and n2 == max(256, (1 << lg) // 16384)      # the smallest N2 that works
    for n in (0, 1, 255, 256, 16384, 65535, 65537, 3 << 15, 1 << 29, (1 << 32) + 256):
        assert M.split(n) is None, n
    assert M.path(256) == "lds" and M.path(1 << 16) == "four_step" and M.path(32768) == "bluestein" and M.path((1 << 23) + 1) is None


def test_bluestein_length():
    facts = {8191: 16384, 8193: 65536, 40000: 1 << 17, 65537: 1 << 18}
    for n, L in facts.items():
        assert M.bluestein_L(n) == L, n
    assert [M.bluestein_L(n) for n in (1, 2, 3, 127, 128, 129)] == [256, 256, 256, 256, 256, 512]
    assert M.bluestein_L(16383) == 65536 and M.bluestein_L(100003) == 1 << 18 and M.bluestein_L(32768) == 65536
    assert M.bluestein_L(1 << 23) == 1 << 24 and M.bluestein_L((1 << 23) + 1) is None and M.bluestein_L((1 << 32) + 256) is None
    for n in (5, 1000, 8200, 32736, 70001):
        L = M.bluestein_L(n)
        assert L >= 2 * n - 1 and L & (L - 1) == 0 and (L in M.POW2_PLANS or M.split(L))
        assert L == 256 or L // 2 < 2 * n - 1 or not (L // 2 in M.POW2_PLANS or M.split(L // 2))


@pytest.mark.parametrize("n", sorted(M.RADICES))
def test_bound_separates_right_from_subtly_wrong(n):
    x = M.impulses(n, 11)
    assert x.shape == (64, n) and sorted(M.impulse_positions(n, 11, 64)[:7]) == sorted({0, 1, 2, n - 1, n - 2, n // 2, n // 3})
    for inv in (False, True):
        ref = M.reference(x, inv)
        wrong = M.err_over_bound(M.wrong_reference(ref, n), ref, M.B(n), x)
        assert wrong.min() >= 10.0, (n, inv, wrong.min())               # every impulse of the batch shows it
        right = M.err_over_bound(ref.astype(np.complex64), ref, M.B(n), x)
        assert right.max() <= 1.0 / M.B(n) + 1e-9, (n, inv, right.max())     # one rounding of |X| <= |x|_1 against B of them


def test_inputs_are_what_they_say():
    n = 4000
    t = M.tones(n, 5)
    assert t.shape == (16, n) and t.dtype == np.complex64 and {n // 2, 1, n - 1, 0} <= set(M.tone_bins(n, 5, 16)[:5])
    X = M.reference(t)
    for b, k in enumerate(M.tone_bins(n, 5, 16)):
        assert abs(X[b, k] - n) < 1e-3 * n and np.abs(np.delete(X[b], k)).max() < 1e-3
    m = M.mixture(n, 5)
    a = np.sort(np.abs(m[0]))
    assert a[-1] > 0.98 and abs(a[-2] - 2.0 ** -6) < 1e-6 and M.noise(n, 5).shape == (1, n)
    assert M.impulses(3, 1).shape == (3, 3) and M.impulses(1, 1).shape == (1, 1) and M.tones(2, 1).shape == (2, 2)
    assert M.impulse_positions(1 << 16, 3, 2) == [(1 << 16) - 1, (1 << 16) // 3] and M.impulses(1 << 16, 3, 1)[0, -1] == np.complex64(1 + 0.5j)
    e = M.bound(2.0, np.ones((1, 8), np.complex64))
    assert e[0] == 16 * M.U
    pb = M.power_bound(2.0, np.ones((1, 8), np.complex64), np.full((1, 8), 3.0 + 4.0j))
    assert np.allclose(pb, 2 * 5 * e[0] + e[0] ** 2 + 3 * M.U * (5 + e[0]) ** 2)
