"""gm_stap's definition (include/gnss_mi355x.h) in float64 numpy: the counts, the stacked samples z[t][l A + a] = x_a[t - l], the exact
Gram matrix R of each block, the weights w by numpy.linalg.solve with the fallback rule, the output y and the static mode.  Every
function accepts the device's own R or w words in place of its own, so a test can hold each step to its own bar.  And the scenes that
motivate the entry: the nuller's scene (nuller_model.py) with as many interferers as antennas, one of them a plain CW.

x is always [n, A] complex128 (as_c128 converts [n, A] complex64 and [n, A, 2] int8, -128 becoming -128.0)."""
import numpy as np

import nuller_model as NM

INDEX_MAX = NM.INDEX_MAX
A_MIN, A_MAX, L_MIN, L_MAX, M_MAX = 2, 8, 1, 8, 32
BLOCKS = NM.BLOCKS
as_c128 = NM.as_c128
to_f32 = NM.to_f32


# ---- what the GPU tests draw and hold (tests/test_gpu_stap.py and the files that share its stream) -----------------------------------
BAR_R, BAR_W, BAR_Y = 1e-5, 2.0 ** -22, 1e-5          # the three bars of test_gpu_stap.py's docstring


def stream(fmt, n, A, seed):
    """[n, A] complex64 or [n, A, 2] int8: unit noise (int8: 1.2 LSB), a rank-one white jammer 30 dB above it and a CW 30 dB above it
    from another direction"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))
    jam = 10.0 ** 1.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x + jam[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]
    cw = np.sqrt(2.0) * 10.0 ** 1.5 * np.exp(2j * np.pi * (0.0617 * np.arange(n) + rng.random()))
    x = x + cw[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]
    if fmt == "i8":
        v = 1.2 * x
        q = np.stack([np.clip(np.rint(v.real), -128, 127), np.clip(np.rint(v.imag), -128, 127)], axis=-1).astype(np.int8)
        if n > 2:
            q[n // 3, A - 1] = (-128, 127)
            q[n // 2, 0] = (-128, -128)
        return q
    return x.astype(np.complex64)


def derived_R(B, L):
    """the derived bound on R's error, as a fraction of sum_t |z_p| |z_q|"""
    return np.sqrt(2.0) * (min(B, 1024) / 32 + 6 + B / 1024 + 2 * (L - 1)) * 2.0 ** -24


def resolve(n_antennas, taps, block=0, loading=0.0, steering=None, reserved=0):
    """the argument rules and defaults -> dict(A, L, M, B, loading (the float32 word, widened), s [M] complex128 laid out [L][A]), or
    None where refused"""
    if not L_MIN <= taps <= L_MAX or not A_MIN <= n_antennas <= A_MAX or n_antennas * taps > M_MAX:
        return None
    M = n_antennas * taps
    if steering is not None:
        steering = np.asarray(steering).reshape(-1)
        if steering.shape != (M,):
            return None
    p = NM.resolve(n_antennas, block, loading, None, reserved)          # the nuller's rules for B, loading and reserved
    if p is None:
        return None
    s = np.zeros(M, np.complex128)
    s[0] = 1.0
    if steering is not None:
        s = steering.astype(np.complex64).astype(np.complex128)
        if not np.isfinite(s.view(np.float64)).all() or not s.any():
            return None
    return dict(A=n_antennas, L=taps, M=M, B=p["B"], loading=p["loading"], s=s)


def total_out(p, T):
    return T // p["B"] * p["B"]


def plan(p, inputs_so_far, n_in):
    """outputs that n_in more time samples deliver, or None where the indices are refused"""
    if inputs_so_far > INDEX_MAX or n_in > INDEX_MAX or inputs_so_far + n_in > INDEX_MAX:
        return None
    return total_out(p, inputs_so_far + n_in) - total_out(p, inputs_so_far)


def blocks_of(p, x, input_index=0):
    """the stacked samples of the finished blocks of a stream that continues after input_index zero time samples
    -> [blocks, B, M] complex128; samples before the stream's start are zeros"""
    x = as_c128(x)
    A, L, B = p["A"], p["L"], p["B"]
    lead = input_index % B
    full = np.concatenate([np.zeros((lead + L - 1, A), np.complex128), x])
    n = full.shape[0] - (L - 1)
    nb = n // B
    z = np.concatenate([full[L - 1 - l:L - 1 - l + nb * B] for l in range(L)], axis=1)      # column l A + a = x_a[t - l]
    return z.reshape(nb, B, A * L)


def covariance(zb):
    """[blocks, B, M] -> (R [blocks, M, M] with R[p][q] = sum_t z_p conj(z_q), weight [blocks, M, M] = sum_t |z_p| |z_q|)"""
    return NM.covariance(zb)


def weights(p, R, want_fallback=False):
    """[blocks, M, M] (the model's R, or the device's float32 words) -> w [blocks, M] complex128, before the rounding to float32 (and the
    blocks that took the fallback w = s / (s^H s): tr = 0, or a Cholesky pivot not greater than 0 or not finite)"""
    M, s = p["M"], p["s"]
    R = np.asarray(R).astype(np.complex128)
    w = np.zeros((R.shape[0], M), np.complex128)
    fb = np.zeros(R.shape[0], bool)
    for b in range(R.shape[0]):
        tr = float(np.trace(R[b]).real)
        Rl = R[b] + p["loading"] * (tr / M) * np.eye(M)
        ok = tr != 0.0 and np.isfinite(Rl.view(np.float64)).all()
        if ok:
            try:
                c = np.linalg.cholesky(Rl)
                ok = bool(np.isfinite(c.view(np.float64)).all() and (np.diagonal(c).real > 0.0).all())
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            fb[b] = True
            w[b] = s / np.vdot(s, s).real
            continue
        u = np.linalg.solve(Rl, s)
        w[b] = u / np.vdot(s, u)
    return (w, fb) if want_fallback else w


def combine(zb, w):
    """[blocks, B, M] and w [blocks, M] (one row: the same for every block) -> (y [blocks * B], weight = sum |w| |z|)"""
    return NM.combine(zb, w)


def run(p, x, input_index=0, R=None, w=None, static_w=None):
    """the whole definition -> dict(zb, R, R_weight, w (float64), w32 (the float32 words used), fallback, y, y_weight); R / w: the
    device's words in place of the model's; static_w: the static mode (R and w are not computed)"""
    zb = blocks_of(p, x, input_index)
    out = dict(zb=zb)
    if static_w is not None:
        w32 = to_f32(np.asarray(static_w).reshape(-1))
        out.update(R=None, w=None, w32=w32)
    else:
        Rm, Rw = covariance(zb)
        wm, fb = weights(p, Rm if R is None else R, want_fallback=True)
        w32 = to_f32(wm) if w is None else np.asarray(w)
        out.update(R=Rm, R_weight=Rw, w=wm, w32=w32, fallback=fb)
    y, wt = combine(zb, w32)
    out.update(y=y, y_weight=wt)
    return out


# ---- the scenes: the nuller's scene with as many interferers as antennas ---------------------------------------------------------------
N, FS, DWELL, N_IN = NM.N, NM.FS, NM.DWELL, NM.N_IN
DETECT = NM.DETECT
CW_HZ = 123456.7
# name -> (A, white jammers' azimuths, CWs' (azimuth, Hz))
SCENES = {
    "S1": (2, (-0.9,), ((0.8, CW_HZ),)),
    "S2": (4, (-0.9, 0.9, -0.3), ((0.6, CW_HZ),)),
    "S3": (8, (-0.9, 0.9, -0.3, 0.0, -0.6, 0.6, 1.2), ((-1.2, CW_HZ),)),
    "clean": (4, (), ()),
}


def scene(name, seed, jn_db=40.0, int8=False):
    """[N_IN, A] complex128 (or [N_IN, A, 2] int8): nuller_model.scene(seed, A) (the satellite and the noise) widened to complex128, then
    the interferers drawn from numpy.random.default_rng(1000 + seed) in list order: the white jammers first, each
    sqrt(10^(JN/10)) (standard_normal(n) + 1j standard_normal(n)) times steer(az, A), then the CWs, each
    sqrt(2 10^(JN/10)) exp(2j pi f t / FS) times steer(az, A).  int8: scaled so that the noise is 1.5 LSB per component, rounded,
    clipped at -128 .. 127."""
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
    if int8:
        v = 1.5 * x
        return np.stack([np.clip(np.rint(v.real), -128, 127), np.clip(np.rint(v.imag), -128, 127)], axis=-1).astype(np.int8)
    return x


def nulled(x, taps, block=1024, loading=1e-4, steering=None):
    """the scene through the model -> complex64 [DWELL]"""
    A = np.asarray(x).shape[1]
    r = run(resolve(A, taps, block, loading, steering), x)
    return r["y"].astype(np.complex64)


search = NM.search
found = NM.found


def table(seeds=(1, 2, 3), out=print):
    """the README's table: per scene the true worker's best cell (peak-to-mean, code phase) of antenna 0 alone and behind L = 1, 2, 4, 8"""
    rows = [("S1", 40.0, False, (1, 2, 4, 8)), ("S2", 40.0, False, (1, 2, 4, 8)), ("S3", 40.0, False, (1, 2, 4)),
            ("S1", 50.0, False, (1, 2, 4, 8)), ("S1", 30.0, True, (1, 2, 4, 8)), ("clean", None, False, (1, 2, 4))]
    for name, jn, int8, taps in rows:
        cells = {}
        for seed in seeds:
            x = scene(name, seed, jn if jn is not None else 40.0, int8)
            cells.setdefault("antenna 0", []).append(search(as_c128(x)[:, 0]))
            for L in taps:
                cells.setdefault("L = %d" % L, []).append(search(nulled(x, L)))
        out("%s%s%s" % (name, "" if jn is None else " at %g dB" % jn, ", int8" if int8 else ""))
        for k, v in cells.items():
            out("  %-10s %s" % (k, " / ".join("%.1f at (%d, %d)" % (c[2], c[0], c[1]) for c in v)))
    s = np.zeros(5 * 2, np.complex64)
    s[2 * 2] = 1.0                                                 # the reference on tap 2 of 5: the peak comes back two samples late
    v = [search(nulled(scene("S1", seed), 5, steering=s)) for seed in seeds]
    out("S1 at 40 dB, L = 5, the reference on tap 2\n  %-10s %s" % ("", " / ".join("%.1f at (%d, %d)" % (c[2], c[0], c[1]) for c in v)))


if __name__ == "__main__":
    table()
