"""gm_acq_array_prompts' and gm_array_row_solve's definitions (include/gnss_mi355x.h, "Beam rows from the array's own correlations")
in float64 numpy, written from the header alone, and the scenes that motivate them: beam_model.scene's, unchanged, with each
satellite's constraint row ESTIMATED from the array's prompts and the beamformer's own Gram matrix in place of nuller_model.steer().

A helper module like beam_model.py (which it imports, with stap_model.py, and does not edit), not a test.  Shared by
tests/test_array_probe_host.py (CPU) and tests/test_gpu_array_probe.py (GPU).  Run as a script it prints the README's table.

x is always [n, A] complex128 (stap_model.as_c128 converts the device formats)."""
import numpy as np

import beam_model as BM
import excise_model as EM
import nuller_model as NM
import stap_model as SM

A_MIN, A_MAX, L_MIN, L_MAX, M_MAX = SM.A_MIN, SM.A_MAX, SM.L_MIN, SM.L_MAX, SM.M_MAX
K_MAX, CANDS_MAX = 32, 1024
LOADING_DEFAULT, LOADING_MIN, LOADING_MAX = 1e-4, 1e-6, 1.0


# ---- the argument rules (gm_acq_array_plan) ----------------------------------------------------------------------------------------
def plan(K, M, A, L):
    """dict(periods = R_u, words_per_cand = R_u L A), or None where the rules say GM_ERR_INVALID_ARG"""
    K = max(1, int(K))
    if K > K_MAX or M < 1 or not A_MIN <= A <= A_MAX or not L_MIN <= L <= L_MAX or A * L > M_MAX or K * M * A * L >= 1 << 32:
        return None
    return dict(periods=K * M, words_per_cand=K * M * L * A)


# ---- the prompts -------------------------------------------------------------------------------------------------------------------
def reference(table_d, code_w, N, cp):
    """ref[n] = tab[d][n] c_w[(n - cp) mod N], complex128 [N]"""
    return np.asarray(table_d).astype(np.complex128)[:N] * np.roll(np.asarray(code_w, np.float64)[:N], int(cp))


def delayed(x, s, l, N):
    """x[s - l .. s - l + N) of [n, A], a time index below 0 reading as zero"""
    lo = int(s) - int(l)
    if lo >= 0:
        return x[lo:lo + N]
    return np.concatenate([np.zeros((-lo, x.shape[1]), x.dtype), x[:lo + N]])


def prompts(x, table_d, code_w, N, starts_d, o, R_u, cp, L, want_envelope=False):
    """z[i][l][a] = sum_{n<N} x_a[s[o + i] + n - l] ref[n] -> complex128 [R_u, L, A]; with want_envelope also sum_n |x_a[s + n - l]|
    (|ref| = 1), what the GPU test's bar is a fraction of"""
    x = SM.as_c128(x)
    ref = reference(table_d, code_w, N, cp)
    z = np.zeros((R_u, L, x.shape[1]), np.complex128)
    env = np.zeros((R_u, L, x.shape[1]), np.float64)
    for i in range(R_u):
        for l in range(L):
            seg = delayed(x, starts_d[o + i], l, N)
            z[i, l] = ref @ seg
            env[i, l] = np.abs(seg).sum(axis=0)
    return (z, env) if want_envelope else z


# ---- the row -----------------------------------------------------------------------------------------------------------------------
def solve_row(z, R_blocks=None, loading=0.0, ref_index=None):
    """the nine steps -> (row complex128 [m] BEFORE the rounding to float32, dict(lambda1, lambda2, ref_index)), or None where the
    rules refuse.  z: [n, m] (any shape [n, ...]); R_blocks: [n_blocks, m, m] (or [m, m]) as the capture writes them, None: the
    identity.  ref_index: rotate at this word instead of the largest one (numpy's eigenvector against the library's choice)."""
    z = np.asarray(z)
    if z.ndim < 2 or z.shape[0] == 0:
        return None
    z = z.reshape(z.shape[0], -1).astype(np.complex128)
    m = z.shape[1]
    load = LOADING_DEFAULT if loading == 0.0 else float(np.float32(loading))
    if not 2 <= m <= M_MAX or not LOADING_MIN <= load <= LOADING_MAX or not np.isfinite(z.view(np.float64)).all():
        return None
    if R_blocks is None:
        Rs = np.eye(m, dtype=np.complex128)
    else:
        Rb = np.asarray(R_blocks).astype(np.complex128).reshape(-1, m, m)
        up = np.triu(Rb.sum(axis=0))                                   # only the upper triangle is read
        if Rb.shape[0] == 0 or not np.isfinite(up.view(np.float64)).all():
            return None
        Rs = up + np.triu(up, 1).conj().T
        Rs[np.arange(m), np.arange(m)] = Rs.diagonal().real
    tr = float(Rs.diagonal().real.sum())
    if not tr > 0.0:
        return None
    Rl = Rs + load * (tr / m) * np.eye(m)
    try:
        Cf = np.linalg.cholesky(Rl)
    except np.linalg.LinAlgError:
        return None
    zt = np.linalg.solve(Cf, z.T)                                      # [m, n]: column i is C^-1 z_i
    Q = zt @ zt.conj().T
    lam, vec = np.linalg.eigh(Q)
    lambda1, lambda2 = float(lam[-1]), max(float(lam[-2]), 0.0)
    if not lambda1 > 0.0:
        return None
    s = Cf @ vec[:, -1]
    k = int(np.argmax(np.abs(s))) if ref_index is None else int(ref_index)
    s = s * np.exp(-1j * np.angle(s[k]))
    s = s * np.sqrt(m / np.vdot(s, s).real)
    return s, dict(lambda1=lambda1, lambda2=lambda2, ref_index=k)


# ---- the scenes: beam_model.scene's, the rows estimated ------------------------------------------------------------------------------
N, FS, DWELL, PERIODS = BM.N, BM.FS, BM.DWELL, EM.PERIODS
DETECT = BM.DETECT
BLOCK, LOADING = 1024, 1e-4
SEEDS = (1, 2, 3)
CONFIGS = tuple((name, L) for name in ("clean", "T1", "T2") for L in sorted({1, BM.TAPS[name]}))


def scene_prompts(x, worker, L, cell=None):
    """the R_u = PERIODS prompt vectors of satellite `worker` at its cell (bin, code phase; None: the true one) on the scene x"""
    tabs, _ = EM.scene_tables()
    codes = EM.sampled_codes(EM.scene_codes())
    d, cp = cell if cell is not None else (BM.SATS[worker]["bin"], BM.SATS[worker]["code_phase"])
    return prompts(x, tabs[d], codes[worker], N, np.arange(PERIODS) * N, 0, PERIODS, cp, L)


def gram(x, L):
    """the Gram matrices a Beamformer(A, L, .., BLOCK) captures on x: [blocks, M, M] complex128"""
    p = SM.resolve(x.shape[1], L, BLOCK, LOADING)
    return SM.covariance(SM.blocks_of(p, x))[0]


def beams(x, L, rows, R=None):
    """x through the model's beams with these rows -> complex64 [P, DWELL]: beam_model.beams' steps with the Gram matrix formed once"""
    A = x.shape[1]
    p0 = SM.resolve(A, L, BLOCK, LOADING)
    zb = SM.blocks_of(p0, x)
    R = SM.covariance(zb)[0] if R is None else R
    out = []
    for s in np.asarray(rows).reshape(-1, A * L):
        p = SM.resolve(A, L, BLOCK, LOADING, s)
        out.append(SM.combine(zb, NM.to_f32(SM.weights(p, R)))[0])
    return np.stack(out).astype(np.complex64)


def estimated_rows(x, L, R="gram", loading=LOADING):
    """[2, L A] complex64 and the two infos: each satellite's row from its prompts at the true cell and R ("gram": the beamformer's
    own blocks; None: the identity)"""
    Rb = gram(x, L) if isinstance(R, str) else R
    got = [solve_row(scene_prompts(x, w, L), Rb, loading) for w in (0, 1)]
    return np.stack([g[0] for g in got]).astype(np.complex64), [g[1] for g in got]


def spatial_rows(x, L):
    """the first negative control: the row estimated from the A tap-0 words and the A x A Gram matrix, placed in tap 0 of L taps"""
    A = x.shape[1]
    s1, _ = estimated_rows(x, 1)
    s = np.zeros((2, L, A), np.complex64)
    s[:, 0] = s1
    return s.reshape(2, L * A)


_CELLS = {}


def cells(name, seed, L):
    """the scene through [e_0, steer(sat 0), steer(sat 1), estimated 0, estimated 1] at L taps -> {(worker, "e0" | "true" | "est"):
    (bin, code phase, peak-to-mean), (worker, "quality"): lambda1 / lambda2}; computed once and shared"""
    key = (name, seed, L)
    if key not in _CELLS:
        x = BM.scene(name, seed)
        R = gram(x, L)
        est, infos = estimated_rows(x, L, R)
        y = beams(x, L, np.concatenate([BM.rows(x.shape[1], L), est]), R)
        out = {}
        for w in (0, 1):
            out[(w, "e0")], out[(w, "true")], out[(w, "est")] = BM.search(y[0], w), BM.search(y[1 + w], w), BM.search(y[3 + w], w)
            out[(w, "quality")] = infos[w]["lambda1"] / infos[w]["lambda2"] if infos[w]["lambda2"] > 0.0 else float("inf")
        _CELLS[key] = out
    return _CELLS[key]


def ratios(name, L, seeds=SEEDS):
    """over the seeds and both satellites: (smallest est / true, smallest est / e0, smallest lambda1 / lambda2)"""
    c = [cells(name, seed, L) for seed in seeds]
    return (min(v[(w, "est")][2] / v[(w, "true")][2] for v in c for w in (0, 1)),
            min(v[(w, "est")][2] / v[(w, "e0")][2] for v in c for w in (0, 1)),
            min(v[(w, "quality")] for v in c for w in (0, 1)))


def controls(seeds=SEEDS):
    """the two negative controls -> {("spatial", seed, worker): (peak-to-mean behind the spatial-only row, behind e_0)} on T1 at
    L = 2, {("unwhitened", seed, worker): (behind the R = NULL row, behind the true row)} on T2 at L = 1"""
    out = {}
    for seed in seeds:
        x = BM.scene("T1", seed)
        y = beams(x, 2, spatial_rows(x, 2))
        for w in (0, 1):
            out[("spatial", seed, w)] = (BM.search(y[w], w)[2], cells("T1", seed, 2)[(w, "e0")][2])
        x = BM.scene("T2", seed)
        y = beams(x, 1, estimated_rows(x, 1, R=None)[0])
        for w in (0, 1):
            out[("unwhitened", seed, w)] = (BM.search(y[w], w)[2], cells("T2", seed, 1)[(w, "true")][2])
    return out


def table(seeds=SEEDS, out=print):
    """the README's table: per scene, L and satellite the peak-to-mean behind e_0, behind the true steer() row and behind the estimated
    row, lambda1 / lambda2; then the smallest ratios (the host test's bars are 0.9 of them) and the negative controls"""
    for name, L in CONFIGS:
        out("%s (A = %d), L = %d" % (name, BM.SCENES[name][0], L))
        c = [cells(name, seed, L) for seed in seeds]
        for w in (0, 1):
            for k in ("e0", "true", "est"):
                out("  sat %d behind %-5s %s" % (w, k, " / ".join("%.1f at (%d, %d)" % (v[(w, k)][2], v[(w, k)][0], v[(w, k)][1]) for v in c)))
            out("  sat %d lambda1 / lambda2  %s" % (w, " / ".join("%.1f" % v[(w, "quality")] for v in c)))
        r = ratios(name, L, seeds)
        out("  smallest est / true %.3f, est / e0 %.3f, lambda1 / lambda2 %.1f" % r)
    for k, v in sorted(controls(seeds).items()):
        out("  control %-10s seed %d sat %d: %.1f against %.1f (%.2f)" % (k[0], k[1], k[2], v[0], v[1], v[0] / v[1]))


if __name__ == "__main__":
    table()
