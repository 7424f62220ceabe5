"""Beam rows from the array's own correlations on the CPU: the additive entries in every layer (this test fails without the feature), the
ABI number and gm_acq_cand left alone, gm_acq_array_plan and gm_array_row_solve (host only, no device) against the float64 model of
array_probe_model.py, and the scenes that motivate the entries: beam_model.scene's two satellites behind rows ESTIMATED from the
prompts and the beamformer's own Gram matrix.

The solver's bar.  A row's words have modulus at most sqrt(32), so the one rounding to float32 moves a word by at most
sqrt(32) 2^-24 = 3.4e-7; the float64 part (a Cholesky factor, a Jacobi against LAPACK's eigh) is negligible where lambda1 >= 2 lambda2,
which every input here is asserted to have.  Word for word within 1e-6, numpy's vector rotated at the library's ref_index.

The scenes' bars come from the model's own table (python tests/array_probe_model.py), 0.9 times the smallest value it prints over seeds
1, 2, 3 and both satellites, per scene and L (stricter than per L alone):
    scene, L      est / true   bar      est / e0   bar      lambda1 / lambda2 (smallest)
    clean, 1      1.001        0.901    3.521      3.169    43.9
    T1, 1         0.982        0.884    1.288      1.159    6.7
    T1, 2         0.873        0.786    1.206      1.085    8.2
    T2, 1         0.964        0.868    4.993      4.494    7.4
The negative controls as the model prints them (peak-to-mean behind the control row against the yardstick, seeds 1 / 2 / 3):
    spatial-only row in tap 0 of L = 2 on T1, against e_0:   sat 0  22.6 / 17.3 / 8.1 against 53.5 / 51.5 / 50.5
                                                             sat 1  9.6 / 9.1 / 8.3 against 41.4 / 45.4 / 42.5      (all six below e_0)
    R = NULL on T2 (L = 1), against the true row:            sat 0  3.6 / 3.5 / 6.7 against 175.3 / 167.9 / 170.9   (0.02 to 0.04)
                                                             sat 1  2.6 / 83.0 / 105.4 against 169.3 / 171.2 / 177.3 (0.02, 0.48, 0.59)
A FINDING: without the whitening satellite 0 is lost on every seed, but satellite 1 keeps 0.48 and 0.59 of the true-row beam on seeds 2
and 3: the principal vector of the un-whitened prompts is a jammer mixture, and what the beam constrained to it passes is chance.  The
estimator is judged as the scenes test judges it, by EVERY beam of a scene: the control asserts that on every seed the estimator fails
that criterion at 0.5 (its worst beam is below 0.5 of the true-row beam), not that each single beam is below 0.5."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import acq_local_model as LM
import array_probe_model as PM
import beam_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gm_acq_array_prompts", "gm_acq_array_plan", "gm_array_row_solve"]
INVALID = -1
ROW_BAR = 1e-6
# (scene, L) -> (bar on est / true, bar on est / e0): 0.9 times the model's own smallest values (the docstring's table)
BARS = {("clean", 1): (0.9 * 1.001, 0.9 * 3.521), ("T1", 1): (0.9 * 0.982, 0.9 * 1.288), ("T1", 2): (0.9 * 0.873, 0.9 * 1.206),
        ("T2", 1): (0.9 * 0.964, 0.9 * 4.993)}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- layers and rules ------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_in_every_layer(gm):
    from gnss_sdr_rs_amd import _lib, acquisition
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    rust_acq = _read("rust", "src", "mi355x", "do_acquisition.rs")
    L = gm.lib()
    pattern = re.search(r"global:\s*([^;]+);", _read("gnss-sdr-rs_amd", "csrc", "exports.map")).group(1).strip()
    with open(_lib.library_path(), "rb") as f:      # the dynamic symbols of the built library, read from its file
        blob = f.read()
    hpp = _read("gnss-sdr-rs_amd", "host", "gnss_sdr.hpp")
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "pub fn %s(" % name in rust, name
        assert re.fullmatch(pattern.replace("*", ".*"), name), (pattern, name)
        assert getattr(L, name) is not None
        assert name.encode() + b"\0" in blob, name
        assert name in hpp and name in rust_acq, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in _read(doc), (doc, name)
    assert "array_prompts(" in hpp and "solve_row(" in hpp
    assert "pub fn array_prompts(" in rust_acq and "pub fn solve_row(" in rust_acq and "pub struct GmArrayRowInfo" in rust
    build = _read("gnss-sdr-rs_amd", "build.py")
    assert "acq_array.hip" in build
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_array" in internal and "ArrayArgs" in internal
    for fn in ("array_plan", "solve_row", "solve_rows"):
        assert callable(getattr(acquisition, fn)), fn
    assert hasattr(acquisition.AcquisitionEngine, "array_prompts")
    for words in ("gm_array_row_info", "A time index below 0 reads as ZERO", "THE ORDER, f32", "THE LIBRARY DECIDES NOTHING",
                  "first L - 1 time samples of period 0 only", "Not built: per-antenna prompts from the tracker"):
        assert words in header, words
    assert "4.2h" in _read("DESIGN.md") and "acq_array.hip" in _read("README.md")
    stats = _read("profiles", "array_probe_kernel_stats.txt")
    assert "acq_array_prompts_kernel" in stats and "scratch" in stats
    # the ctypes struct has the header's layout
    Info = _lib.ArrayRowInfo
    assert C.sizeof(Info) == 24 and Info.lambda2.offset == 8 and Info.ref_index.offset == 16 and Info.reserved.offset == 20
    body = re.search(r"pub struct GmArrayRowInfo\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in Info._fields_]


def test_the_abi_number_and_the_candidate_stay(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    Cand = _lib.AcqCand
    assert C.sizeof(Cand) == 16
    assert [(f[0], getattr(Cand, f[0]).offset) for f in Cand._fields_] == [("worker", 0), ("doppler_bin", 4), ("code_phase_samples", 8),
                                                                          ("offset_periods", 12)]
    assert "typedef struct { uint32_t worker; int32_t doppler_bin; uint32_t code_phase_samples; uint32_t offset_periods; } gm_acq_cand;" \
        in _read("include", "gnss_mi355x.h")


def test_array_plan_holds_every_rule(gm):
    from gnss_sdr_rs_amd import acquisition
    L_ = gm.lib()
    pairs = 0
    for A in range(0, 11):
        for L in range(0, 11):
            for K, M in ((0, 1), (1, 10), (3, 2), (32, 7), (33, 1), (1, 0), (2, 0)):
                want = PM.plan(K, M, A, L)
                r, w = C.c_uint32(77), C.c_uint32(78)
                rc = L_.gm_acq_array_plan(K, M, A, L, C.byref(r), C.byref(w))
                if want is None:
                    assert rc == INVALID and (r.value, w.value) == (77, 78), (A, L, K, M)
                    with pytest.raises(gm.GmError):
                        acquisition.array_plan(K, M, A, L)
                else:
                    assert rc == 0 and (r.value, w.value) == (want["periods"], want["words_per_cand"]), (A, L, K, M)
                    assert acquisition.array_plan(K, M, A, L) == want
                    pairs += (K, M) == (1, 10)
    assert pairs == 43                                               # gm_stap's (A, L) pairs, all of them
    assert acquisition.array_plan(0, 10, 4) == dict(periods=10, words_per_cand=40)           # taps defaults to 1, K = 0 is K = 1
    assert L_.gm_acq_array_plan(2, 5, 8, 4, None, None) == 0                                  # either output may be NULL
    assert L_.gm_acq_array_plan(32, 1 << 27, 8, 4, None, None) == INVALID                     # R_u L A = 2^37 does not fit
    assert PM.plan(32, 1 << 27, 8, 4) is None


# ---- gm_array_row_solve ------------------------------------------------------------------------------------------------------------------
def _raw_solve(gm, m, n, z, R, nb, loading, row=True, info=True):
    """the C entry with sentinel-filled outputs -> (status, row words, info bytes)"""
    from gnss_sdr_rs_amd import _lib
    rw = np.full(64, 0x5A5A5A5A, np.uint32)
    inf = (C.c_uint8 * 24)(*([0x5A] * 24))
    rc = gm.lib().gm_array_row_solve(m, n, z.ctypes.data if z is not None else None, R.ctypes.data if R is not None else None, nb,
                                     C.c_float(loading), rw.ctypes.data if row else None,
                                     C.cast(inf, C.POINTER(_lib.ArrayRowInfo)) if info else None)
    return rc, rw, bytes(inf)


def _good(m, n, seed=5):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    z = (10.0 * s[None, :] * np.exp(2j * np.pi * rng.random(n))[:, None] + rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m)))
    B = rng.standard_normal((3, 40, m)) + 1j * rng.standard_normal((3, 40, m))
    R = np.einsum("btp,btq->bpq", B, B.conj())
    return np.ascontiguousarray(z, np.complex64), np.ascontiguousarray(R, np.complex64)


def test_row_solve_refuses_and_leaves_row_and_info_alone(gm):
    z, R = _good(6, 9)
    untouched = lambda r: r[0] == INVALID and (r[1] == 0x5A5A5A5A).all() and r[2] == b"\x5A" * 24
    assert _raw_solve(gm, 6, 9, z, R, 3, 0.0)[0] == 0
    for m in (0, 1, 33, 1000):
        assert untouched(_raw_solve(gm, m, 9, z, None, 0, 0.0)), m
    assert untouched(_raw_solve(gm, 6, 0, z, R, 3, 0.0))
    assert untouched(_raw_solve(gm, 6, 9, None, R, 3, 0.0))
    assert _raw_solve(gm, 6, 9, z, R, 3, 0.0, row=False)[0] == INVALID
    assert _raw_solve(gm, 6, 9, z, R, 3, 0.0, info=False)[0] == INVALID
    assert untouched(_raw_solve(gm, 6, 9, z, R, 0, 0.0))              # R without blocks
    for bad in (np.nan, np.inf, -np.inf):
        zz = z.copy(); zz[8, 5] = complex(0.0, bad)
        assert untouched(_raw_solve(gm, 6, 9, zz, R, 3, 0.0)), bad
        RR = R.copy(); RR[2, 1, 4] = complex(bad, 0.0)                 # an upper-triangle word of the last block
        assert untouched(_raw_solve(gm, 6, 9, z, RR, 3, 0.0)), bad
        RR = R.copy(); RR[2, 4, 1] = complex(bad, 0.0)                 # the lower triangle is not read
        assert _raw_solve(gm, 6, 9, z, RR, 3, 0.0)[0] == 0, bad
    for loading in (-1e-4, 0.9e-6, 1.0001, np.nan, np.inf):
        assert untouched(_raw_solve(gm, 6, 9, z, R, 3, loading)), loading
        assert PM.solve_row(z, R, loading) is None
    for loading in (1e-6, 1.0):
        assert _raw_solve(gm, 6, 9, z, R, 3, loading)[0] == 0
    assert untouched(_raw_solve(gm, 6, 9, z, np.zeros_like(R), 3, 0.0))                       # tr = 0
    assert untouched(_raw_solve(gm, 6, 9, z, np.ascontiguousarray(-R), 3, 0.0))               # tr < 0
    ind = np.zeros((1, 6, 6), np.complex64)
    ind[0] = np.eye(6); ind[0, 0, 1] = 5.0                            # tr > 0, the second pivot 1 - 25 < 0
    assert untouched(_raw_solve(gm, 6, 9, z, ind, 1, 0.0))
    assert PM.solve_row(z, ind) is None and PM.solve_row(z, np.zeros_like(R)) is None
    assert untouched(_raw_solve(gm, 6, 9, np.zeros_like(z), R, 3, 0.0))                       # lambda1 = 0
    assert PM.solve_row(np.zeros_like(z), R) is None


def _against_numpy(tag, z, R, loading=0.0):
    from gnss_sdr_rs_amd import acquisition
    z = np.ascontiguousarray(z, np.complex64)
    z = z.reshape(z.shape[0], -1)
    R = None if R is None else np.ascontiguousarray(R, np.complex64)
    row, info = acquisition.solve_row(z, R, loading)
    own, _ = PM.solve_row(z, R, loading)
    want, winfo = PM.solve_row(z, R, loading, ref_index=info["ref_index"])
    m = z.shape[1]
    assert winfo["lambda1"] >= 2.0 * winfo["lambda2"], (tag, winfo)
    assert row.dtype == np.complex64 and row.shape == (m,)
    err = float(np.max(np.abs(row.astype(np.complex128) - want)))
    print("%s: m = %d, n = %d, lambda1 / lambda2 = %.3g, largest word difference %.2e (bar %.0e)"
          % (tag, m, z.shape[0], winfo["lambda1"] / max(winfo["lambda2"], 1e-300), err, ROW_BAR))
    assert err <= ROW_BAR, (tag, err)
    assert info["lambda1"] == pytest.approx(winfo["lambda1"], rel=1e-9), tag
    assert info["lambda2"] == pytest.approx(winfo["lambda2"], rel=1e-9, abs=1e-12 * winfo["lambda1"]), tag
    # the word at ref_index is the largest (to the rounding), real and positive; s^H s = m
    assert abs(abs(own[info["ref_index"]]) - np.abs(own).max()) <= 1e-12 * np.abs(own).max(), tag
    assert row[info["ref_index"]].imag == 0.0 and row[info["ref_index"]].real > 0.0, tag
    assert float(np.vdot(row, row).real) == pytest.approx(m, rel=1e-6), tag
    return row, info


@pytest.mark.parametrize("name,L", [("T1", 1), ("T1", 2), ("T2", 1), ("T1", 4), ("T2", 4)], ids=["m4", "m8-T1", "m8-T2", "m16", "m32"])
def test_row_solve_against_numpy_on_the_scenes(gm, name, L):
    x = BM.scene(name, 1)
    R = PM.gram(x, L)
    for w in (0, 1):
        _against_numpy("%s L = %d sat %d" % (name, L, w), PM.scene_prompts(x, w, L), R, PM.LOADING)


def test_row_solve_special_inputs(gm):
    from gnss_sdr_rs_amd import acquisition
    x = BM.scene("T1", 1)
    z, R = PM.scene_prompts(x, 0, 2), PM.gram(x, 2).astype(np.complex64)
    assert R.shape == (20, 8, 8)
    _, info = _against_numpy("n = 1", z[:1], R)
    assert info["lambda2"] <= 1e-12 * info["lambda1"]                 # rank one
    zc = PM.scene_prompts(BM.scene("clean", 1), 0, 1)
    _against_numpy("R = NULL, clean", zc, None)
    one, _ = _against_numpy("one block", z, R[:1])
    twenty, _ = _against_numpy("twenty blocks", z, R)
    assert np.abs(one - twenty).max() > 1e-4                          # (the blocks differ: the sum is not one block scaled)
    _against_numpy("default loading", z, R, 0.0)
    _against_numpy("loading 1", z, R, 1.0)
    # only the upper triangle is read
    G = R.copy()
    G[:, np.tril_indices(8, -1)[0], np.tril_indices(8, -1)[1]] = 1e30
    a, b = acquisition.solve_row(z, R, 1e-4), acquisition.solve_row(z, G, 1e-4)
    assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and a[1] == b[1]
    # solve_rows: array_prompts' [n_cands, R_u, L, A] and the capture's [blocks, M, M] go in as they come out
    zz = np.stack([PM.scene_prompts(x, w, 2) for w in (0, 1)]).astype(np.complex64)
    assert zz.shape == (2, 10, 2, 4)
    rows, infos = acquisition.solve_rows(zz, R, 1e-4)
    assert rows.shape == (2, 2, 4) and rows.dtype == np.complex64 and len(infos) == 2
    for w in (0, 1):
        row, info = acquisition.solve_row(zz[w], R, 1e-4)
        assert (rows[w].reshape(-1).view(np.uint32) == row.view(np.uint32)).all() and infos[w] == info
    with pytest.raises(ValueError):
        acquisition.solve_rows(zz[0], R)
    with pytest.raises(ValueError):
        acquisition.solve_row(zz[0], R[:, :4, :4])


# ---- the model's own facts -----------------------------------------------------------------------------------------------------------------
def test_the_models_prompts_are_local_searchs_per_antenna_and_the_halo_is_zero():
    rng = np.random.default_rng(3)
    N, A, L, R_u = 64, 3, 3, 2
    n = (R_u + 1) * N + 5                                               # the last period read starts at 2 N + 3
    x = (rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))).astype(np.complex64).astype(np.complex128)
    tab = np.exp(-2j * np.pi * 0.01 * np.arange(N))
    code = np.where(rng.integers(0, 2, N) > 0, 1.0, -1.0)
    starts = np.array([0, N + 1, 2 * N + 3])
    for o in (0, 1):
        z, env = PM.prompts(x, tab, code, N, starts, o, R_u, 7, L, want_envelope=True)
        assert z.shape == env.shape == (R_u, L, A)
        for a in range(A):
            for l in range(L):
                shifted = np.concatenate([np.zeros(l), x[:, a]])[:x.shape[0]]        # x_a[t - l], zero in front of the stream
                want = LM.prompts(shifted, tab, code, N, starts, o, R_u, 7, 0)[0]
                assert np.abs(z[:, l, a] - want).max() <= 1e-12 * env[:, l, a].max(), (o, a, l)
    # tap l of period 0 at s = 0 misses its first l terms: adding a sample in front changes nothing
    z0 = PM.prompts(x, tab, code, N, starts, 0, 1, 7, L)
    ref = PM.reference(tab, code, N, 7)
    for l in range(L):
        assert np.allclose(z0[0, l], ref[l:] @ x[:N - l], rtol=0, atol=1e-12 * N)


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", PM.CONFIGS, ids=["%s-L%d" % c for c in PM.CONFIGS])
def test_every_estimated_row_finds_its_satellite(name, L):
    bar_true, bar_e0 = BARS[(name, L)]
    for seed in PM.SEEDS:
        c = PM.cells(name, seed, L)
        for w in (0, 1):
            e0, true, est = c[(w, "e0")], c[(w, "true")], c[(w, "est")]
            print("%s L = %d seed %d sat %d: e0 %.1f, true row %.1f, estimated row %.1f (%.3f of true, bar %.3f; %.3f of e0, bar %.3f), "
                  "lambda1 / lambda2 %.1f" % (name, L, seed, w, e0[2], true[2], est[2], est[2] / true[2], bar_true, est[2] / e0[2], bar_e0,
                                              c[(w, "quality")]))
            assert BM.found(est, w) and est[2] > PM.DETECT, (seed, w, est)
            assert est[2] / true[2] >= bar_true, (seed, w, est[2] / true[2])
            assert est[2] / e0[2] >= bar_e0, (seed, w, est[2] / e0[2])
            assert c[(w, "quality")] >= 2.0, (seed, w)


def test_the_two_negative_controls():
    got = PM.controls()
    for seed in PM.SEEDS:
        for w in (0, 1):
            s, e0 = got[("spatial", seed, w)]
            print("T1, L = 2, seed %d sat %d: the spatial-only row in tap 0 gives %.1f, e_0 %.1f" % (seed, w, s, e0))
            assert s < e0, (seed, w, s, e0)
        fr = [got[("unwhitened", seed, w)][0] / got[("unwhitened", seed, w)][1] for w in (0, 1)]
        print("T2, L = 1, seed %d: R = NULL reaches %.2f and %.2f of the true-row beams" % (seed, fr[0], fr[1]))
        assert min(fr) < 0.5, (seed, fr)              # the estimator fails the scenes test's criterion (every beam) at 0.5
