"""gm_nuller's definition (include/gnss_mi355x.h) in float64 numpy: the counts, the block covariance R, the weights w by
numpy.linalg.solve, the output y and the static mode.  Every function accepts the device's own R or w words in place of its own, so a
test can hold each step to its own bar.  And the scene that motivates the entry: the excision scene's signal (excise_model.py) on a
uniform line array of A antennas at half a wavelength, with a white noise jammer from another direction.

x is always [n, A] complex128 (as_c128 converts [n, A] complex64 and [n, A, 2] int8, -128 becoming -128.0)."""
import numpy as np

import excise_model as EM

INDEX_MAX = 1 << 62
A_MIN, A_MAX = 2, 8
BLOCKS = (256, 512, 1024, 2048, 4096, 8192, 16384)
F32_1E_6 = float(np.float32(1e-6))


def resolve(n_antennas, block=0, loading=0.0, steering=None, reserved=0):
    """the argument rules and defaults -> dict(A, B, loading (the float32 word, widened), s [A] complex128), or None where refused"""
    if reserved or not A_MIN <= n_antennas <= A_MAX:
        return None
    B = block or 1024
    if B not in BLOCKS:
        return None
    ld = float(np.float32(loading))
    if not np.isfinite(ld) or (ld != 0.0 and not F32_1E_6 <= ld <= 1.0):
        return None
    if ld == 0.0:
        ld = float(np.float32(1e-4))
    s = np.zeros(n_antennas, np.complex128)
    s[0] = 1.0
    if steering is not None:
        s = np.asarray(steering).astype(np.complex64).astype(np.complex128)
        if s.shape != (n_antennas,) or not np.isfinite(s.view(np.float64)).all() or not s.any():
            return None
    return dict(A=n_antennas, B=B, loading=ld, s=s)


def total_out(p, T):
    return T // p["B"] * p["B"]


def plan(p, inputs_so_far, n_in):
    """outputs that n_in more time samples deliver, or None where the indices are refused"""
    if inputs_so_far > INDEX_MAX or n_in > INDEX_MAX or inputs_so_far + n_in > INDEX_MAX:
        return None
    return total_out(p, inputs_so_far + n_in) - total_out(p, inputs_so_far)


def as_c128(x):
    x = np.asarray(x)
    if x.dtype == np.int8:
        return x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)
    return x.astype(np.complex128)


def blocks_of(p, x, input_index=0):
    """the finished blocks of a stream that continues after input_index zero time samples -> [blocks, B, A] complex128"""
    x = as_c128(x)
    lead = input_index % p["B"]
    full = np.concatenate([np.zeros((lead, p["A"]), np.complex128), x])
    nb = full.shape[0] // p["B"]
    return full[:nb * p["B"]].reshape(nb, p["B"], p["A"])


def covariance(xb):
    """[blocks, B, A] -> (R [blocks, A, A] with R[i][j] = sum_t x_i conj(x_j), weight [blocks, A, A] = sum_t |x_i| |x_j|)"""
    R = np.einsum("bti,btj->bij", xb, xb.conj())
    W = np.einsum("bti,btj->bij", np.abs(xb), np.abs(xb))
    return R, W


def weights(p, R):
    """[blocks, A, A] (the model's R, or the device's float32 words) -> w [blocks, A] complex128, before the rounding to float32"""
    A, s = p["A"], p["s"]
    R = np.asarray(R).astype(np.complex128)
    w = np.zeros((R.shape[0], A), np.complex128)
    for b in range(R.shape[0]):
        tr = float(np.trace(R[b]).real)
        if tr == 0.0:
            w[b] = s / np.vdot(s, s).real
            continue
        u = np.linalg.solve(R[b] + p["loading"] * (tr / A) * np.eye(A), s)
        w[b] = u / np.vdot(s, u)
    return w


def to_f32(w):
    return np.asarray(w).astype(np.complex64)


def combine(xb, w):
    """[blocks, B, A] and w [blocks, A] (one row: the same for every block) -> (y [blocks * B], weight = sum_a |w[a]| |x_a|)"""
    w = np.asarray(w).astype(np.complex128)
    if w.ndim == 1:
        w = np.broadcast_to(w, (xb.shape[0], w.shape[0]))
    y = np.einsum("ba,bta->bt", w.conj(), xb)
    wt = np.einsum("ba,bta->bt", np.abs(w), np.abs(xb))
    return y.reshape(-1), wt.reshape(-1)


def run(p, x, input_index=0, R=None, w=None, static_w=None):
    """the whole definition -> dict(xb, R, R_weight, w (float64), w32 (the float32 words used), y, y_weight); R / w: the device's words in
    place of the model's; static_w: the static mode (R and w are not computed)"""
    xb = blocks_of(p, x, input_index)
    out = dict(xb=xb)
    if static_w is not None:
        w32 = to_f32(static_w)
        out.update(R=None, w=None, w32=w32)
        y, wt = combine(xb, w32)
    else:
        Rm, Rw = covariance(xb)
        wm = weights(p, Rm if R is None else R)
        w32 = to_f32(wm) if w is None else np.asarray(w)
        out.update(R=Rm, R_weight=Rw, w=wm, w32=w32)
        y, wt = combine(xb, w32)
    out.update(y=y, y_weight=wt)
    return out


# ---- the scene: the excision scene's signal on a line array, a white jammer from another direction -------------------------------------
N, FS, PERIODS, DWELL = EM.N, EM.FS, EM.PERIODS, EM.DWELL
N_IN = DWELL                               # 20 blocks of 1024: the stage has no delay
SAT_AZ, JAM_AZ = 0.3, -0.9
DETECT = 7.0


def steer(az, A):
    """a uniform line array at half a wavelength"""
    return np.exp(1j * np.pi * np.arange(A) * np.sin(az))


def scene(seed, A=4, jn_db=None, int8=False):
    """[N_IN, A] complex64 (or [N_IN, A, 2] int8): the excision scene's satellite (code phase 700, Doppler 1 kHz, 45 dB-Hz) from azimuth
    0.3 rad, unit-variance-per-component noise independent per antenna, and a white Gaussian jammer jn_db above the noise power from
    azimuth -0.9 rad (None: none).  int8: scaled so that the noise is 1.5 LSB per component, rounded, clipped at -128 .. 127."""
    chips = EM.scene_codes()
    rng = np.random.default_rng(seed)
    n = np.arange(N_IN, dtype=np.float64)
    u = (n - EM.SAT["code_phase"]) / N
    chip = chips[EM.SAT["worker"]][np.minimum(1022, np.floor((u - np.floor(u)) * 1023.0).astype(np.int64))].astype(np.float64)
    amp = np.sqrt(2.0 * 10.0 ** (EM.SAT["cn0"] / 10.0) / FS)
    cyc = EM.SAT["doppler"] * n / FS
    sig = amp * chip * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 1j * EM.SAT["phase"])
    x = sig[:, None] * steer(SAT_AZ, A)[None, :]
    x = x + rng.standard_normal((N_IN, A)) + 1j * rng.standard_normal((N_IN, A))
    if jn_db is not None:
        jam = np.sqrt(10.0 ** (jn_db / 10.0)) * (rng.standard_normal(N_IN) + 1j * rng.standard_normal(N_IN))
        x = x + jam[:, None] * steer(JAM_AZ, A)[None, :]
    if int8:
        v = 1.5 * x
        return np.stack([np.clip(np.rint(v.real), -128, 127), np.clip(np.rint(v.imag), -128, 127)], axis=-1).astype(np.int8)
    return x.astype(np.complex64)


SCENES = (("clean, c32", None, False), ("J/N 40 dB, c32", 40.0, False), ("J/N 50 dB, c32", 50.0, False), ("J/N 30 dB, int8", 30.0, True))


def nulled(x, block=1024, loading=1e-4, steering=None):
    """the scene through the model -> complex64 [DWELL]"""
    A = np.asarray(x).shape[1]
    r = run(resolve(A, block, loading, steering), x)
    return r["y"].astype(np.complex64)


def search(y):
    """the plain search of a dwell -> (bin, code phase, peak-to-mean) of the true worker's best cell"""
    return EM.search(np.asarray(y).astype(np.complex64))


def found(cell):
    return EM.found(cell)
