"""gm_beamformer's definition (include/gnss_mi355x.h) in float64 numpy, built on stap_model.py: beam p of a handle with rows s_0 ..
s_{P-1} is stap_model.run with steering = s_p, nothing else.  And the scenes that motivate the entry: stap_model.scene's construction
with a second satellite from another direction, searched behind the power-inversion row e_0 and behind a row that points at each
satellite.  Run as a script it prints the README's table.

x is always [n, A] complex128 (stap_model.as_c128 converts the device formats)."""
import numpy as np

import excise_model as EM
import nuller_model as NM
import stap_model as SM

P_MIN, P_MAX = 1, 16
INDEX_MAX = SM.INDEX_MAX


def resolve(n_antennas, taps, steering, block=0, loading=0.0, reserved32=0, reserved=0):
    """the argument rules and defaults -> dict(A, L, M, B, loading, P, s [P, M] complex128, beams: stap_model.resolve's dict per row), or
    None where refused.  steering: [P][L][A] (any shape of P M words), required"""
    if reserved32 or steering is None:
        return None
    if not SM.L_MIN <= taps <= SM.L_MAX or not SM.A_MIN <= n_antennas <= SM.A_MAX or n_antennas * taps > SM.M_MAX:
        return None
    M = n_antennas * taps
    s = np.asarray(steering).reshape(-1)
    if s.size == 0 or s.size % M or not P_MIN <= s.size // M <= P_MAX:
        return None
    beams = [SM.resolve(n_antennas, taps, block, loading, row, reserved) for row in s.reshape(-1, M)]
    if any(b is None for b in beams):
        return None
    b0 = beams[0]
    return dict(A=b0["A"], L=b0["L"], M=M, B=b0["B"], loading=b0["loading"], P=len(beams), s=np.stack([b["s"] for b in beams]), beams=beams)


def total_out(p, T):
    return T // p["B"] * p["B"]


def plan(p, inputs_so_far, n_in):
    """outputs PER BEAM that n_in more time samples deliver, or None where the indices are refused"""
    return SM.plan(p["beams"][0], inputs_so_far, n_in)


def run(p, x, input_index=0):
    """the whole definition -> stap_model.run's dict per beam"""
    return [SM.run(b, x, input_index=input_index) for b in p["beams"]]


# ---- the scenes: stap_model.scene's construction, two satellites -----------------------------------------------------------------------
N, FS, DWELL, N_IN = SM.N, SM.FS, SM.DWELL, SM.N_IN
DETECT = SM.DETECT
CW_HZ = SM.CW_HZ
# name -> (A, white jammers' azimuths, CWs' (azimuth, Hz))
SCENES = {
    "clean": (4, (), ()),
    "T1": (4, (-0.9,), ((0.8, CW_HZ),)),
    "T2": (8, (-0.9, 0.9, -0.3), ((0.8, CW_HZ),)),
}
TAPS = {"clean": 1, "T1": 2, "T2": 1}
SAT0 = dict(EM.SAT, az=NM.SAT_AZ)
SAT1 = dict(worker=1, code_phase=1300, doppler=500.0, phase=2.1, cn0=45.0, bin=1, az=-0.55)
SATS = (SAT0, SAT1)


def scene(name, seed, jn_db=40.0):
    """[N_IN, A] complex128: nuller_model.scene(seed, A) (satellite 0 and the noise) widened to complex128, then stap_model.scene's
    interferers drawn from numpy.random.default_rng(1000 + seed) in list order (the white jammers, then the CWs), then satellite 1,
    noise-free, with satellite 0's amplitude and chip formulas"""
    A, whites, cws = SCENES[name]
    x = NM.scene(seed, A).astype(np.complex128)
    rng = np.random.default_rng(1000 + seed)
    n = x.shape[0]
    t = np.arange(n, dtype=np.float64)
    for az in whites:
        jam = np.sqrt(10.0 ** (jn_db / 10.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x = x + jam[:, None] * NM.steer(az, A)[None, :]
    for az, f in cws:
        cw = np.sqrt(2.0 * 10.0 ** (jn_db / 10.0)) * np.exp(2j * np.pi * f * t / FS)
        x = x + cw[:, None] * NM.steer(az, A)[None, :]
    chips = EM.scene_codes()
    u = (t - SAT1["code_phase"]) / N
    chip = chips[SAT1["worker"]][np.minimum(1022, np.floor((u - np.floor(u)) * 1023.0).astype(np.int64))].astype(np.float64)
    amp = np.sqrt(2.0 * 10.0 ** (SAT1["cn0"] / 10.0) / FS)
    cyc = SAT1["doppler"] * t / FS
    sig = amp * chip * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 1j * SAT1["phase"])
    return x + sig[:, None] * NM.steer(SAT1["az"], A)[None, :]


def rows(A, L):
    """[3, L A] complex64: e_0, then a row that points at each satellite at tap 0 (zeros on the later taps)"""
    s = np.zeros((3, L, A), np.complex64)
    s[0, 0, 0] = 1.0
    s[1, 0] = NM.steer(SAT0["az"], A)
    s[2, 0] = NM.steer(SAT1["az"], A)
    return s.reshape(3, L * A)


def beams(x, taps, steering, block=1024, loading=1e-4):
    """the scene through the model -> complex64 [P, DWELL]"""
    p = resolve(np.asarray(x).shape[1], taps, steering, block, loading)
    return np.stack([r["y"] for r in run(p, x)]).astype(np.complex64)


def search(y, worker):
    """the plain search of a dwell -> (bin, code phase, peak-to-mean) of `worker`'s best cell"""
    import acq_model as AM
    tabs, tf = EM.scene_tables()
    y = np.asarray(y).astype(np.complex64)
    return EM.best_cell(*AM.search_model(y[:DWELL], tabs, EM.sampled_codes(EM.scene_codes()), N, 1, EM.PERIODS, tf, FS), worker)


def found(cell, worker):
    return cell[0] == SATS[worker]["bin"] and cell[1] == SATS[worker]["code_phase"]


_CELLS = {}


def cells(name, seed):
    """the scene of `seed` through the three rows at the scene's taps -> {(worker, "e0" | "beam"): cell}; computed once and shared"""
    if (name, seed) not in _CELLS:
        x = scene(name, seed)
        y = beams(x, TAPS[name], rows(x.shape[1], TAPS[name]))
        _CELLS[(name, seed)] = {(0, "e0"): search(y[0], 0), (0, "beam"): search(y[1], 0), (1, "e0"): search(y[0], 1), (1, "beam"): search(y[2], 1)}
    return _CELLS[(name, seed)]


def table(seeds=(1, 2, 3), out=print):
    """the README's table: per scene each satellite's best cell (peak-to-mean) behind e_0 and behind its own beam"""
    for name in ("clean", "T1", "T2"):
        c = [cells(name, seed) for seed in seeds]
        out("%s (A = %d, L = %d)" % (name, SCENES[name][0], TAPS[name]))
        for w in (0, 1):
            for k in ("e0", "beam"):
                out("  sat %d behind %-5s %s" % (w, k, " / ".join("%.1f at (%d, %d)" % (v[(w, k)][2], v[(w, k)][0], v[(w, k)][1]) for v in c)))


if __name__ == "__main__":
    table()
