"""gm_acq_cfg.coherent_periods on the CPU: the ABI, the argument check gm_acq_create makes before any device call, and
acquisition.detection_threshold against the Gamma(M) law of a noise cell."""
import math
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_9_and_the_trailing_field(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert _lib.AcqCfg._fields_[-1][0] == "coherent_periods"
    assert "gm_acq_coherent_phasors" in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "rust", "src", "mi355x.rs")).read()
    body = re.sub(r"//[^\n]*", "", re.search(r"pub struct GmAcqCfg\s*\{([^}]*)\}", src, re.S).group(1))
    assert re.findall(r"pub\s+(\w+)\s*:", body)[-1] == "coherent_periods"
    assert "pub fn gm_acq_coherent_phasors(" in src


def test_create_checks_coherent_periods_before_any_device_call(gm):
    """33 is GM_ERR_INVALID_ARG without a device; 10 passes the argument checks and meets GM_ERR_NO_DEVICE."""
    code = ("import sys; sys.path.insert(0, %r); import numpy as np, ctypes as C; import gnss_sdr_rs_amd as g;"
            "from gnss_sdr_rs_amd._lib import AcqCfg; L = g.lib(); n = C.c_int(0); L.gm_device_count(C.byref(n));"
            "dop = np.zeros(3, np.float32); ids = np.array([1, 2], np.uint8); out = []\n"
            "for k in (33, 10):\n"
            "    c = AcqCfg(); c.fs, c.fft_size, c.n_integrations, c.n_bins = 8.0e6, 8000, 2, 3\n"
            "    c.doppler_hz, c.n_prn, c.prn_ids, c.coherent_periods = dop.ctypes.data, 2, ids.ctypes.data, k\n"
            "    h = C.c_void_p(); out.append(L.gm_acq_create(C.byref(c), C.byref(h)))\n"
            "print(n.value, *out)") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    ndev, rc33, rc10 = out.stdout.split()[-3:]
    assert int(rc33) == -1, out.stdout + out.stderr
    if int(ndev) == 0:
        assert int(rc10) == -3, out.stdout + out.stderr


def _q(M, x):
    return math.exp(-x) * sum(x ** i / math.factorial(i) for i in range(M))


def test_detection_threshold_closed_form():
    from gnss_sdr_rs_amd import acquisition as A
    assert abs(A.detection_threshold(1, 8000, 1e-3) - math.log(8000 / 1e-3)) < 1e-6
    for M, cells, pfa in ((1, 8000, 1e-3), (2, 8000 * 41, 1e-6), (5, 1e5, 1e-2), (20, 8000 * 81, 1e-3)):
        t = A.detection_threshold(M, cells, pfa)
        assert cells * _q(M, t * M) <= pfa * (1 + 1e-9)
        assert cells * _q(M, t * M * (1 - 1e-6)) > pfa
    assert 14.5 < A.detection_threshold(2, 8000 * 41, 1e-6) < 15.5


def test_detection_threshold_monte_carlo():
    """Per-cell probability 1e-3 (n_cells = 1): the fraction of Gamma(M) / M draws above t is 1e-3 within its sampling error."""
    from gnss_sdr_rs_amd import acquisition as A
    rng = np.random.default_rng(1234)
    n = 2_000_000
    for M in (1, 2, 4):
        t = A.detection_threshold(M, 1, 1e-3)
        frac = float(np.mean(rng.gamma(M, 1.0, n) / M > t))
        assert abs(frac - 1e-3) < 5 * math.sqrt(1e-3 / n), (M, t, frac)
