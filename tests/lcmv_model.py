"""gm_lcmv's definition (include/gnss_mi355x.h) in float64 numpy, built on stap_model.py: beam p carries Q_p constraint rows c_q and Q_p
responses f_q, and per block w_p = Rl^-1 C (C^H Rl^-1 C)^-1 f through the header's eight steps, with both fallbacks.  And the two scenes
that motivate the entry: a second signal with the satellite's own code from another direction, below the noise, that one constraint
leaves standing and a second row with the response 0 removes; and a space-time beam whose single constraint skews the correlation
triangle, which one constraint per tap straightens.  Run as a script it prints the README's tables.

x is always [n, A] complex128 (stap_model.as_c128 converts the device formats).  A beam is a pair (rows [Q][M], f [Q])."""
import numpy as np

import excise_model as EM
import nuller_model as NM
import stap_model as SM

P_MIN, P_MAX, Q_MIN, Q_MAX, Q_SUM = 1, 16, 1, 8, 16
DEPENDENT = 1e-10
INDEX_MAX = SM.INDEX_MAX
F32_MAX = float(np.finfo(np.float32).max)


def gram_factor(C):
    """C [M, Q] -> the lower Cholesky factor of C^H C, columns ascending, or None where a pivot is not greater than DEPENDENT times that
    row's squared norm (the rows are linearly dependent)"""
    G = C.conj().T @ C
    Q = G.shape[0]
    Lg = np.zeros((Q, Q), np.complex128)
    for j in range(Q):
        norm = G[j, j].real
        pj = norm - float(np.sum(np.abs(Lg[j, :j]) ** 2))
        if not pj > DEPENDENT * norm or not np.isfinite(pj):
            return None
        Lg[j, j] = np.sqrt(pj)
        for i in range(j + 1, Q):
            Lg[i, j] = (G[i, j] - np.sum(Lg[i, :j] * Lg[j, :j].conj())) / Lg[j, j]
    return Lg


def quiescent(C, f):
    """w0 = C (C^H C)^-1 f, complex128 [M], before the rounding to float32; None where the rows are dependent"""
    Lg = gram_factor(C)
    if Lg is None:
        return None
    y = np.linalg.solve(Lg, f)
    return C @ np.linalg.solve(Lg.conj().T, y)


def resolve(n_antennas, taps, constraints, block=0, loading=0.0, reserved32=0, reserved=0):
    """the argument rules and defaults -> dict(A, L, M, B, loading, P, Q [P], C: per beam [M, Q] complex128 (column q = row c_q), f: per
    beam [Q] complex128, w0: per beam [M] complex128, st: stap_model.resolve's dict), or None where refused.  constraints: a list of
    (rows, f) per beam, required"""
    if reserved32 or constraints is None:
        return None
    st = SM.resolve(n_antennas, taps, block, loading, None, reserved)
    if st is None:
        return None
    M = st["M"]
    if not P_MIN <= len(constraints) <= P_MAX:
        return None
    Cs, fs, w0s = [], [], []
    for rows, f in constraints:
        f = np.asarray(f).reshape(-1).astype(np.complex64).astype(np.complex128)
        rows = np.asarray(rows).astype(np.complex64).astype(np.complex128)
        Q = f.size
        if not Q_MIN <= Q <= Q_MAX or Q > M or rows.size != Q * M:
            return None
        rows = rows.reshape(Q, M)
        if not np.isfinite(rows.view(np.float64)).all() or not np.isfinite(f.view(np.float64)).all() or not rows.any(axis=1).all():
            return None
        Cs.append(rows.T.copy())
        fs.append(f)
    if sum(f.size for f in fs) > Q_SUM:
        return None
    for C, f in zip(Cs, fs):
        w0 = quiescent(C, f)
        if w0 is None or not np.isfinite(w0.view(np.float64)).all() or np.abs(w0.view(np.float64)).max() > F32_MAX:
            return None
        w0s.append(w0)
    return dict(A=st["A"], L=st["L"], M=M, B=st["B"], loading=st["loading"], P=len(fs), Q=[f.size for f in fs], C=Cs, f=fs, w0=w0s, st=st)


def total_out(p, T):
    return T // p["B"] * p["B"]


def plan(p, inputs_so_far, n_in):
    """outputs PER BEAM that n_in more time samples deliver, or None where the indices are refused"""
    return SM.plan(p["st"], inputs_so_far, n_in)


def weights(p, R, want_fallback=False):
    """[blocks, M, M] (the model's R, or the device's float32 words) -> w [blocks, P, M] complex128, before the rounding to float32 (and
    fallback [blocks, P]: the blocks whose beam took w0: tr = 0 or a bad pivot of Lc for all beams, a bad pivot of Lg or a u that is
    not finite for the beam alone)"""
    M, P = p["M"], p["P"]
    R = np.asarray(R).astype(np.complex128)
    w = np.zeros((R.shape[0], P, M), np.complex128)
    fb = np.zeros((R.shape[0], P), bool)

    def factor(G):
        if not np.isfinite(G.view(np.float64)).all():
            return None
        try:
            c = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            return None
        return c if np.isfinite(c.view(np.float64)).all() and (np.diagonal(c).real > 0.0).all() else None

    for b in range(R.shape[0]):
        tr = float(np.trace(R[b]).real)
        Rl = R[b] + p["loading"] * (tr / M) * np.eye(M)
        Lc = factor(Rl) if tr != 0.0 else None
        for k in range(P):
            u = None
            if Lc is not None:
                Z = np.linalg.solve(Lc, p["C"][k])                 # z_q = Lc^-1 c_q
                Lg = factor(Z.conj().T @ Z)
                if Lg is not None:
                    v = np.linalg.solve(Lg.conj().T, np.linalg.solve(Lg, p["f"][k]))
                    u = np.linalg.solve(Lc.conj().T, Z @ v)
                    with np.errstate(over="ignore"):
                        if not np.isfinite(u.astype(np.complex64).view(np.float32)).all():    # as the float32 words it rounds to
                            u = None
            fb[b, k] = u is None
            w[b, k] = p["w0"][k] if u is None else u
    return (w, fb) if want_fallback else w


def run(p, x, input_index=0, R=None, w=None, static_w=None):
    """the whole definition -> dict(zb, R, R_weight, w [blocks, P, M] (float64), w32 (the float32 words used), fallback [blocks, P],
    y [P, n], y_weight [P, n]); R / w: the device's words in place of the model's; static_w [P, M]: the static mode"""
    zb = SM.blocks_of(p["st"], x, input_index)
    out = dict(zb=zb)
    if static_w is not None:
        w32 = np.broadcast_to(SM.to_f32(np.asarray(static_w).reshape(p["P"], p["M"])), (zb.shape[0], p["P"], p["M"]))
        out.update(R=None, w=None, w32=w32)
    else:
        Rm, Rw = SM.covariance(zb)
        wm, fb = weights(p, Rm if R is None else R, want_fallback=True)
        w32 = SM.to_f32(wm) if w is None else np.asarray(w)
        out.update(R=Rm, R_weight=Rw, w=wm, w32=w32, fallback=fb)
    ys = [SM.combine(zb, np.asarray(w32)[:, k]) for k in range(p["P"])]
    out.update(y=np.stack([y for y, _ in ys]), y_weight=np.stack([wt for _, wt in ys]))
    return out


# ---- what the tests draw ---------------------------------------------------------------------------------------------------------------
COND_MAX = 100.0


def draw(rng, M, qs):
    """constraints for beams of qs[p] rows each: standard normal rows and responses, a beam redrawn while cond(C^H C) > COND_MAX
    -> (the list of (rows complex64 [Q, M], f complex64 [Q]), the number of redraws)"""
    out, redraws = [], 0
    for Q in qs:
        while True:
            rows = (rng.standard_normal((Q, M)) + 1j * rng.standard_normal((Q, M))).astype(np.complex64)
            f = (rng.standard_normal(Q) + 1j * rng.standard_normal(Q)).astype(np.complex64)
            c = rows.astype(np.complex128)
            if np.linalg.cond(c.conj() @ c.T) <= COND_MAX:
                break
            redraws += 1
        out.append((rows, f))
    return out, redraws


# the shapes of the GPU tests (A, L, B, the Q list): Q = 1; Q = M; two beams; P = 3, a partial group of four in pass 2; sum Q = 16 at
# NL = 2; five beams of three; M = 32 at NL = 2; sixteen beams, two substitution rounds; blocks of two and of four chunks (the other
# staging path)
CASES = [(2, 1, 256, [1]), (2, 1, 256, [2]), (4, 1, 256, [2, 1]), (4, 2, 256, [2, 2, 1]), (2, 8, 256, [8, 8]), (3, 5, 256, [3, 3, 3, 3, 3]),
         (4, 8, 256, [4, 4, 4, 4]), (8, 4, 256, [1] * 16), (4, 4, 512, [2, 2]), (4, 4, 1024, [2, 2])]
# further draws of the GPU tests: (seed, M, the Q list)
DRAWS = [(21, 12, [3, 1, 2, 8, 2]), (31, 8, [2, 2, 1]), (32, 8, [3]), (33, 8, [1]), (41, 8, [2, 1, 3]), (5, 8, [2, 3])]
FALLBACK_CASE = (4, 3, 256, [3, 1, 2, 2, 1, 1, 1, 1, 2, 2])        # ten beams: two rounds


def case_seed(case):
    A, L, B, qs = case
    return 1000 * A + 100 * L + 10 * len(qs) + sum(qs) + B % 97


def drawn(case):
    """-> (the case's constraints, the redraws they took)"""
    A, L, B, qs = case
    return draw(np.random.default_rng(case_seed(case)), A * L, qs)


def interfered(rng, n, A, jn_db=30.0):
    """[n, A] complex128: unit noise, a rank-one white jammer jn_db up and a CW jn_db up from another direction"""
    x = rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))
    jam = 10.0 ** (jn_db / 20.0) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = x + jam[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]
    cw = np.sqrt(2.0) * 10.0 ** (jn_db / 20.0) * np.exp(2j * np.pi * 0.0617 * np.arange(n))
    return x + cw[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
N, FS, DWELL, N_IN = SM.N, SM.FS, SM.DWELL, SM.N_IN
DETECT = SM.DETECT
SAT = dict(EM.SAT, az=NM.SAT_AZ)
SPOOF = dict(worker=0, code_phase=1200, doppler=EM.SAT["doppler"], phase=1.9, cn0=51.0, bin=EM.SAT["bin"], az=-0.5)
CW_AZ = 0.6


def spoofer_scene(seed, jn_db=40.0):
    """[N_IN, 4] complex128: nuller_model.scene(seed, 4, jn_db) (the satellite at code phase 700 from azimuth 0.3, the noise and a white
    jammer) and, noise-free, the same code again at code phase 1200, 51 dB-Hz, phase 1.9 rad, from azimuth -0.5, with the satellite's
    amplitude and chip formulas"""
    x = NM.scene(seed, 4, jn_db).astype(np.complex128)
    t = np.arange(x.shape[0], dtype=np.float64)
    chips = EM.scene_codes()
    u = (t - SPOOF["code_phase"]) / N
    chip = chips[SPOOF["worker"]][np.minimum(1022, np.floor((u - np.floor(u)) * 1023.0).astype(np.int64))].astype(np.float64)
    amp = np.sqrt(2.0 * 10.0 ** (SPOOF["cn0"] / 10.0) / FS)
    cyc = SPOOF["doppler"] * t / FS
    sig = amp * chip * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 1j * SPOOF["phase"])
    return x + sig[:, None] * NM.steer(SPOOF["az"], 4)[None, :]


def triangle_scene(seed, jn_db=40.0):
    """[N_IN, 4] complex128: nuller_model.scene(seed, 4, jn_db) and a CW jn_db above the noise at stap_model.CW_HZ from azimuth 0.6"""
    x = NM.scene(seed, 4, jn_db).astype(np.complex128)
    t = np.arange(x.shape[0], dtype=np.float64)
    cw = np.sqrt(2.0 * 10.0 ** (jn_db / 10.0)) * np.exp(2j * np.pi * SM.CW_HZ * t / FS)
    return x + cw[:, None] * NM.steer(CW_AZ, 4)[None, :]


def on_tap(az, A, L, l):
    """the row that points at azimuth az on tap l (zeros on the other taps), [L A] complex64"""
    s = np.zeros((L, A), np.complex64)
    s[l] = NM.steer(az, A)
    return s.reshape(-1)


def spoofer_beams(A, L):
    """three beams: the satellite's row alone; the satellite's row answering 1 with the other signal's answering 0; the swapped pair"""
    a, b = on_tap(SAT["az"], A, L, 0), on_tap(SPOOF["az"], A, L, 0)
    return [([a], [1.0]), ([a, b], [1.0, 0.0]), ([a, b], [0.0, 1.0])]


def triangle_beams(A, L):
    """two beams: the satellite's row on tap 0 alone; one constraint per tap, tap 0 answering 1 and taps 1 .. L - 1 answering 0"""
    a = on_tap(SAT["az"], A, L, 0)
    return [([a], [1.0]), ([on_tap(SAT["az"], A, L, l) for l in range(L)], [1.0] + [0.0] * (L - 1))]


def beams(x, taps, constraints, block=1024, loading=1e-4):
    """the scene through the model -> complex64 [P, DWELL]"""
    p = resolve(np.asarray(x).shape[1], taps, constraints, block, loading)
    return run(p, x)["y"].astype(np.complex64)


def planes(y, worker=0):
    """the plain search of a dwell at every bin -> float64 [D, N]: the worker's power over the code phases, summed over the periods"""
    import acq_model as AM
    tabs, tf = EM.scene_tables()
    code = EM.sampled_codes(EM.scene_codes())[worker]
    conj_code = np.conj(np.fft.fft(np.asarray(code, np.float64)))
    y = AM.as_c128(np.asarray(y).astype(np.complex64))[:DWELL]
    out = np.zeros((tabs.shape[0], N), np.float64)
    for d in range(tabs.shape[0]):
        for m in range(EM.PERIODS):
            c = np.fft.ifft(np.fft.fft(y[m * N:(m + 1) * N] * tabs[d]) * conj_code) * np.float64(N)
            out[d] += c.real * c.real + c.imag * c.imag
    return out


def ratios(plane):
    """a bin's plane -> every code phase's power over the plane's mean without its peak, as the detector forms it"""
    return plane / ((plane.sum() - plane.max()) / (plane.size - 1))


def best(pl):
    """[D, N] planes -> (bin, code phase, ratio) of the best cell"""
    r = np.stack([ratios(row) for row in pl])
    d, n = np.unravel_index(int(np.argmax(r)), r.shape)
    return int(d), int(n), float(r[d, n])


_SPOOF, _TRI = {}, {}


def spoofer_cells(seed, L):
    """-> per beam of spoofer_beams dict(best=(bin, code phase, ratio), sat=ratio at (bin 2, 700), other=ratio at (bin 2, 1200));
    computed once and shared"""
    if (seed, L) not in _SPOOF:
        x = spoofer_scene(seed)
        out = []
        for y in beams(x, L, spoofer_beams(4, L)):
            pl = planes(y)
            r = ratios(pl[SAT["bin"]])
            out.append(dict(best=best(pl), sat=float(r[SAT["code_phase"]]), other=float(r[SPOOF["code_phase"]])))
        _SPOOF[(seed, L)] = out
    return _SPOOF[(seed, L)]


def triangle_cells(seed, L):
    """-> per beam of triangle_beams dict(peak=the code phase of bin 2's peak, ratio=its ratio, early=P[699] / P[700],
    late=P[701] / P[700]); computed once and shared"""
    if (seed, L) not in _TRI:
        x = triangle_scene(seed)
        out = []
        for y in beams(x, L, triangle_beams(4, L)):
            row = planes(y)[SAT["bin"]]
            cp = SAT["code_phase"]
            out.append(dict(peak=int(np.argmax(row)), ratio=float(ratios(row)[cp]), early=float(row[cp - 1] / row[cp]), late=float(row[cp + 1] / row[cp])))
        _TRI[(seed, L)] = out
    return _TRI[(seed, L)]


def table(seeds=(1, 2, 3), out=print):
    """the README's tables"""
    out("a second signal with the satellite's code (A = 4, J/N 40 dB): ratio at lag 700 / at lag 1200, seeds %s" % " / ".join(map(str, seeds)))
    for L in (1, 2):
        c = [spoofer_cells(seed, L) for seed in seeds]
        for k, name in enumerate(("one row", "rows (1, 0)", "rows (0, 1)")):
            out("  L = %d, %-12s %s" % (L, name, " / ".join("%.1f, %.1f" % (v[k]["sat"], v[k]["other"]) for v in c)))
    out("the correlation triangle (A = 4, jammer and CW at 40 dB): P[699] / P[700], P[701] / P[700], ratio at 700")
    for L in (2, 4):
        c = [triangle_cells(seed, L) for seed in seeds]
        for k, name in enumerate(("one row", "a row a tap")):
            out("  L = %d, %-12s %s" % (L, name, " / ".join("%.3f, %.3f, %.1f" % (v[k]["early"], v[k]["late"], v[k]["ratio"]) for v in c)))


if __name__ == "__main__":
    table()
