"""Re-steering on the device (include/gnss_mi355x.h, "Re-steering on the device"): gm_trk_array_prompts_dev, gm_array_rows_solve_dev
(csrc/array_solve.hip) and gm_beamformer_set_steering_dev on the GPU.

THE BARS are test_array_probe_host's, and the yardstick is always the HOST entry gm_array_row_solve, never the device solver itself:
ROW_BAR = 1e-6 per row word (two f32 roundings of words of modulus at most sqrt(32) come to 6.8e-7; the f64 part is negligible),
relative 1e-9 on the eigenvalues, lambda2 with abs = 1e-12 lambda1 beside it, ref_index equal.  The inputs are synthetic: z_i = a_i s +
unit noise with |a_i| = 10, one word of s made 1.5 times the largest of the others; R from 4 m jammed snapshots a block (a rank-one
jammer 30 dB up).  Asserted on the host entry's result before the device is asked: lambda1 >= 2 lambda2 (but at n = 1, rank one) and
the two largest moduli of the row at least 1e-3 apart relative, so ref_index cannot flip.

1. The solver against the host over m in {2 (one pair), 3 (odd: the idle slot), 8, 12, 32}, n in {1, 9, 300 (several batches)},
   n_blocks in {0, 1, 20}, n_rows in {1, 5, 16}, loading 0 and 1e-2, both layouts: CASES visits every value of each and every m with
   n_blocks > 0.
2. Independence: row 3 of a 16-row call, the same row alone and a second call give the same bytes; NaNs in the lower triangle of every
   block of R change nothing.
3. Statuses 1 to 5 from data (6 needs a row that comes out zero from a positive lambda1 and has no input of its own); each against the
   words the host entry refuses the same input with; a status row is zeros and the other rows keep their bytes.  By the header's rule
   (the first that applies, the host's order) R = -I has a negative trace and gives 3, as the host entry says; status 4 comes from a
   matrix with a positive trace and a negative pivot, diag(-1, 3, 3, ...).
4. gm_trk_array_prompts_dev bit for bit against the synchronous entry at n = 4097, (A, L) = (2, 1), (4, 2), (8, 4), c32 and int8 IQ;
   with skipped records of each kind; every refusal leaves the filler; on a held stream the entry returns with the gate held and d_z
   still the filler; a synchronous call right behind a _dev call on another stream returns its own right words.
5. gm_beamformer_set_steering_dev on one held stream between two process_dev calls: call 1 is the twin's with the old rows, call 2 the
   twin's that got the rows through the synchronous set_steering, outputs and captured w bit for bit; the gate; every refusal.
6. The chain with no host wait, T1 of seed 1, L = 2 (test_gpu_trk_array's records): Beamformer([e_0, e_0, e_0]) with capture and
   process_dev, array_prompts_dev of the nine records per satellite, solve_rows_dev with the captured R, set_steering_dev on beams 1
   and 2, process_dev again, all behind one held gate; each re-steered plane's peak-to-mean at the true cell is at least 0.9 of the
   yardstick's (the same records through array_prompts, solve_rows and set_steering on a twin), the device rows within ROW_BAR of
   the host's.

Measured on an MI355X (one run): in test 1 the largest row-word difference is 0 on all sixteen shapes (the f64 differences of the two
rotation orders vanish in the rounding to f32), lambda1 within 9.3e-15 relative and lambda2 within 7.9e-15 relative where it is not the
rank-one zero; the chain's rows equal the host's, and its beams give 93.91 and 54.05 at the true cells, 1.000 of the twin's.  On a side
build with s = v in place of s = C v the eleven cases of test 1 with n_blocks > 0 fail and the five with the identity pass; with the
install launched on the handle's own stream the ordering test of 5 fails."""
import ctypes as C

import numpy as np
import pytest

import stream_stall as SS            # (imports torch before the HIP library)
import test_gpu_stap as TS
import test_gpu_local_search as TL
import test_gpu_trk_array as TA
import beam_model as BM
import excise_model as EM
from test_array_probe_host import ROW_BAR

pytestmark = pytest.mark.gpu
INVALID, RANGE = -1, -5
QUALITY_BAR = 0.9                     # the margin test_array_probe_host.BARS gives an estimated row
INFO = np.dtype([("lambda1", "<f8"), ("lambda2", "<f8"), ("ref_index", "<u4"), ("status", "<u4")])
_words, _stream, _fmt = TS._words, TS._stream, TS._fmt


# ---- inputs and the host yardstick ---------------------------------------------------------------------------------------------------
def _inputs(m, n, n_blocks, n_rows, seed):
    """-> (z complex64 [n_rows, n, m], R complex64 [n_blocks, m, m] or None)"""
    rng = np.random.default_rng(seed)
    z = np.zeros((n_rows, n, m), np.complex64)
    for p in range(n_rows):
        s = rng.uniform(0.5, 1.0, m) * np.exp(2j * np.pi * rng.random(m))
        s[(3 * p + 1) % m] *= 1.5 / np.abs(s[(3 * p + 1) % m])
        a = 10.0 * np.exp(2j * np.pi * rng.random(n))
        z[p] = a[:, None] * s[None, :] + rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))
    if not n_blocks:
        return z, None
    T = 4 * m
    snap = rng.standard_normal((n_blocks, T, m)) + 1j * rng.standard_normal((n_blocks, T, m))
    jam = 10.0 ** 1.5 * (rng.standard_normal((n_blocks, T)) + 1j * rng.standard_normal((n_blocks, T)))
    snap = snap + jam[:, :, None] * np.exp(2j * np.pi * rng.random(m))[None, None, :]
    return z, np.ascontiguousarray(np.einsum("btp,btq->bpq", snap, snap.conj()), np.complex64)


def _host(z, R, loading, rank_one):
    """gm_array_row_solve per row, with the conditions on the inputs asserted -> (rows [n_rows, m], infos)"""
    from gnss_sdr_rs_amd import acquisition as AQ
    rows, infos = [], []
    for p in range(z.shape[0]):
        row, info = AQ.solve_row(z[p], R, loading)
        if not rank_one:
            assert info["lambda1"] >= 2.0 * info["lambda2"], (p, info)
        mod = np.sort(np.abs(row.astype(np.complex128)))
        assert mod[-1] - mod[-2] >= 1e-3 * mod[-1], (p, mod[-2:])
        rows.append(row); infos.append(info)
    return np.array(rows), infos


def _device(hipbuf, z_layout, R, m, n, n_rows, loading, row_stride=0, vec_stride=0, d_z=None, d_R=None):
    """solve_rows_dev on uploaded inputs, outputs pre-filled with 0x5A -> (rows complex64 [n_rows, m], info records)"""
    from gnss_sdr_rs_amd import acquisition as AQ
    d_z = hipbuf.upload(z_layout) if d_z is None else d_z
    nb = 0 if R is None else R.shape[0]
    if R is not None and d_R is None:
        d_R = hipbuf.upload(R)
    d_rows, d_info = hipbuf.alloc(n_rows * m * 8, fill=0x5A), hipbuf.alloc(n_rows * 24, fill=0x5A)
    plan = AQ.solve_plan(m, n, n_rows, nb, row_stride, vec_stride, loading)
    assert plan["row_words"] == n_rows * m and plan["R_words"] == nb * m * m
    AQ.solve_rows_dev(m, n, n_rows, d_z, d_rows, d_info, d_R=d_R, n_blocks=nb, row_stride=row_stride, vec_stride=vec_stride, loading=loading)
    return hipbuf.download(d_rows, n_rows * m * 8, np.complex64).reshape(n_rows, m), hipbuf.download(d_info, n_rows * 24, np.uint8).view(INFO)


# ---- 1. the solver against the host --------------------------------------------------------------------------------------------------
CASES = [(2, 1, 0, 1, 0.0, "acq"), (2, 9, 1, 5, 1e-2, "trk"), (2, 300, 20, 16, 0.0, "acq"),
         (3, 1, 1, 5, 0.0, "trk"), (3, 9, 20, 16, 1e-2, "acq"), (3, 300, 0, 1, 0.0, "trk"),
         (8, 1, 20, 16, 0.0, "acq"), (8, 9, 0, 5, 1e-2, "trk"), (8, 300, 1, 1, 0.0, "acq"),
         (12, 1, 1, 1, 1e-2, "trk"), (12, 9, 20, 5, 0.0, "acq"), (12, 300, 0, 16, 0.0, "trk"),
         (32, 1, 20, 5, 0.0, "trk"), (32, 9, 1, 16, 1e-2, "acq"), (32, 300, 20, 1, 0.0, "trk"), (32, 9, 0, 16, 0.0, "acq")]


# a guard on the table itself, not a test: every value of every axis is visited, and every m with n_blocks > 0
for _k, _values in enumerate(([2, 3, 8, 12, 32], [1, 9, 300], [0, 1, 20], [1, 5, 16], [0.0, 1e-2], ["acq", "trk"])):
    assert sorted({c[_k] for c in CASES}, key=str) == sorted(_values, key=str), _k
assert {c[0] for c in CASES if c[2] > 0} == {2, 3, 8, 12, 32}


@pytest.mark.parametrize("m,n,n_blocks,n_rows,loading,layout", CASES, ids=["m%d-n%d-b%d-r%d-l%g-%s" % c for c in CASES])
def test_the_solver_against_the_host_entry(gpu, hipbuf, m, n, n_blocks, n_rows, loading, layout):
    z, R = _inputs(m, n, n_blocks, n_rows, 1000 * m + n + n_blocks + n_rows)
    want, infos = _host(z, R, loading, n == 1)
    if layout == "acq":
        got, info = _device(hipbuf, z, R, m, n, n_rows, loading)
    else:                                        # a history [n][P][m]: one tracker call an epoch
        got, info = _device(hipbuf, np.ascontiguousarray(z.transpose(1, 0, 2)), R, m, n, n_rows, loading, row_stride=m, vec_stride=n_rows * m)
    assert not info["status"].any(), info["status"]
    dw = float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128))))
    l1 = np.array([i["lambda1"] for i in infos]); l2 = np.array([i["lambda2"] for i in infos])
    d1 = float(np.max(np.abs(info["lambda1"] - l1) / l1))
    d2 = float(np.max(np.abs(info["lambda2"] - l2) / np.maximum(l2, 1e-300) * (l2 > 0)))
    print("m %d, n %d, %d blocks, %d rows, loading %g, %s: largest word difference %.2e (bar %.0e), lambda1 %.2e relative, lambda2 %.2e"
          % (m, n, n_blocks, n_rows, loading, layout, dw, ROW_BAR, d1, d2))
    assert dw <= ROW_BAR
    assert (np.abs(info["lambda1"] - l1) <= 1e-9 * l1).all()
    assert (np.abs(info["lambda2"] - l2) <= 1e-9 * l2 + 1e-12 * l1).all()
    assert list(info["ref_index"]) == [i["ref_index"] for i in infos]
    assert (got[np.arange(n_rows), info["ref_index"]].imag == 0).all()


# ---- 2. independence -------------------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_its_own_inputs_alone(gpu, hipbuf):
    m, n, nb, P = 8, 9, 3, 16
    z, R = _inputs(m, n, nb, P, 77)
    d_z, d_R = hipbuf.upload(z), hipbuf.upload(R)
    rows, info = _device(hipbuf, z, R, m, n, P, 0.0, d_z=d_z, d_R=d_R)
    assert not info["status"].any()
    again, info2 = _device(hipbuf, z, R, m, n, P, 0.0, d_z=d_z, d_R=d_R)
    assert (_words(rows) == _words(again)).all() and info.tobytes() == info2.tobytes()
    alone, info3 = _device(hipbuf, z, R, m, n, 1, 0.0, d_z=d_z + 3 * n * m * 8, d_R=d_R)
    assert (_words(alone[0]) == _words(rows[3])).all() and info3[0].tobytes() == info[3].tobytes()
    assert not (_words(rows[3]) == _words(rows[4])).all()
    # the history layout reads the same vectors: the same bytes
    hist, info4 = _device(hipbuf, np.ascontiguousarray(z.transpose(1, 0, 2)), R, m, n, P, 0.0, row_stride=m, vec_stride=P * m, d_R=d_R)
    assert (_words(hist) == _words(rows)).all() and info4.tobytes() == info.tobytes()
    # only the upper triangles are read
    Rn = R.copy()
    Rn[:, np.tril_indices(m, -1)[0], np.tril_indices(m, -1)[1]] = np.nan
    lower, info5 = _device(hipbuf, z, Rn, m, n, P, 0.0, d_z=d_z)
    assert (_words(lower) == _words(rows)).all() and info5.tobytes() == info.tobytes()


# ---- 3. statuses ---------------------------------------------------------------------------------------------------------------------------
def _host_refusal(gm, z, R, loading):
    from gnss_sdr_rs_amd import acquisition as AQ
    with pytest.raises(gm.GmError) as e:
        AQ.solve_row(z, R, loading)
    return str(e.value)


def test_data_conditions_are_statuses_not_faults(gpu, hipbuf):
    gm = gpu
    m, n, nb, P = 6, 9, 3, 5
    z, R = _inputs(m, n, nb, P, 31)
    base, binfo = _device(hipbuf, z, R, m, n, P, 0.0)
    assert not binfo["status"].any()

    def zeroed(rows, info, p):
        return not _words(rows[p]).any() and info[p]["lambda1"] == 0 and info[p]["lambda2"] == 0 and info[p]["ref_index"] == 0

    # 1: a NaN in one vector of one row
    zb = z.copy()
    zb[2, 4, 1] = complex(1.0, np.nan)
    rows, info = _device(hipbuf, zb, R, m, n, P, 0.0)
    assert list(info["status"]) == [0, 0, 1, 0, 0] and zeroed(rows, info, 2)
    keep = [0, 1, 3, 4]
    assert (_words(rows[keep]) == _words(base[keep])).all() and info[keep].tobytes() == binfo[keep].tobytes()
    assert "prompt word" in _host_refusal(gm, zb[2], R, 0.0)
    # 2: an Inf in an upper-triangle word of one block, for every row
    Rb = R.copy()
    Rb[1, 2, 4] = complex(np.inf, 0.0)
    rows, info = _device(hipbuf, z, Rb, m, n, P, 0.0)
    assert list(info["status"]) == [2] * P and all(zeroed(rows, info, p) for p in range(P))
    assert "word of R" in _host_refusal(gm, z[0], Rb, 0.0)
    # 1 comes before 2
    rows, info = _device(hipbuf, zb, Rb, m, n, P, 0.0)
    assert list(info["status"]) == [2, 2, 1, 2, 2]
    # 3: a zero trace; and R = -I, whose trace is negative (the host's words for both)
    for Rz in (np.zeros((1, m, m), np.complex64), -np.eye(m, dtype=np.complex64)[None]):
        rows, info = _device(hipbuf, z, Rz, m, n, P, 1e-2)
        assert list(info["status"]) == [3] * P and all(zeroed(rows, info, p) for p in range(P))
        assert "trace" in _host_refusal(gm, z[0], Rz, 1e-2)
    # 4: a positive trace and a negative pivot
    Rp = np.diag([-1.0] + [3.0] * (m - 1)).astype(np.complex64)[None]
    rows, info = _device(hipbuf, z, Rp, m, n, P, 1e-2)
    assert list(info["status"]) == [4] * P and all(zeroed(rows, info, p) for p in range(P))
    assert "Cholesky pivot" in _host_refusal(gm, z[0], Rp, 1e-2)
    # 5: all-zero vectors in one row
    zz = z.copy()
    zz[4] = 0
    rows, info = _device(hipbuf, zz, R, m, n, P, 0.0)
    assert list(info["status"]) == [0, 0, 0, 0, 5] and zeroed(rows, info, 4)
    assert (_words(rows[:4]) == _words(base[:4])).all() and info[:4].tobytes() == binfo[:4].tobytes()
    assert "lambda1" in _host_refusal(gm, zz[4], R, 0.0)


# ---- 4. gm_trk_array_prompts_dev -------------------------------------------------------------------------------------------------------
def _dev_prompts(hipbuf, mgr, d_x, n_time, A, L, recs, fmt, first_index=0, tap_chips=0.0):
    R = len(recs)
    d_z, d_done = hipbuf.alloc(R * L * A * 8, fill=0x5A), hipbuf.alloc(R, fill=0x5A)
    mgr.array_prompts_dev(d_x, n_time, A, recs, d_z, d_done, taps=L, first_index=first_index, tap_chips=tap_chips, fmt=fmt)
    mgr.synchronize()
    return hipbuf.download(d_z, R * L * A * 8, np.complex64).reshape(R, L, A), hipbuf.download(d_done, R, np.uint8)


@pytest.mark.parametrize("fmt", ["c32", "i8"])
@pytest.mark.parametrize("A,L", [(2, 1), (4, 2), (8, 4)])
def test_the_device_form_is_the_synchronous_entry_bit_for_bit(gpu, hipbuf, A, L, fmt):
    from gnss_sdr_rs_amd import tracking as T
    n = 4097
    fs, n_time = 1000.0 * n, 2 * n + 777
    d_x = hipbuf.upload(_stream(fmt, n_time, A, 100 * A + L))
    mgr = T.TrackingManager(fs, n_channels=2, code_index_mode=T.CODE_INDEX_FIXED)
    recs = TA._records(T, n, L, n_time, 40, n + A + L)
    for sub, tau in ((recs, 0.0), (recs[:5], 0.5), ([recs[17]], -2.25)):
        z, done = mgr.array_prompts(d_x, n_time, A, L, states=sub, tap_chips=tau, fmt=_fmt(fmt))
        zd, dd = _dev_prompts(hipbuf, mgr, d_x, n_time, A, L, sub, _fmt(fmt), tap_chips=tau)
        assert done.all() and (dd == done).all() and (_words(zd) == _words(z)).all(), (len(sub), tau)
        assert np.abs(z).max() > 0
    mgr.close()


def test_skipped_records_of_each_kind_on_the_device_form(gpu, hipbuf):
    from gnss_sdr_rs_amd import tracking as T
    n, A, L = 2048, 4, 4
    fs, n_time, f0 = 1000.0 * n, 3 * n, 1000
    d_x = hipbuf.upload(_stream("c32", n_time, A, 12))
    mgr = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    r = TA._record
    group = [r(T, 3, f0 + 2000, 0.0, active=0), r(T, 3, f0 + L - 1, 1500.0), r(T, 33, f0 + 2000, 0.0), r(T, 0, f0 + 2000, 0.0),
             r(T, 3, f0 + n_time - n + 1, 0.0), r(T, 9, f0 + n_time - n, -700.0, code_phase=3.5), r(T, 3, f0 + L - 2, 0.0),
             r(T, 3, f0 - 1, 0.0), r(T, 3, 5, 0.0), r(T, 3, f0 + 2000, 0.0, code_rate=0.0), r(T, 3, f0 + 2000, 0.0, code_rate=0.5),
             r(T, 3, (1 << 63) + 5, 0.0), r(T, 17, f0 + 2500, 40.0)]
    z, done = mgr.array_prompts(d_x, n_time, A, L, states=group, first_index=f0)
    assert list(done) == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1]
    zd, dd = _dev_prompts(hipbuf, mgr, d_x, n_time, A, L, group, 0, first_index=f0)
    assert (dd == done).all() and (_words(zd) == _words(z)).all() and not _words(zd[done == 0]).any()
    zd, dd = _dev_prompts(hipbuf, mgr, d_x, n_time, A, L, [group[0], group[4]], 0, first_index=f0)       # nothing runs: zeros, a success
    assert not dd.any() and not _words(zd).any()
    mgr.close()


def test_every_refusal_of_the_device_form_leaves_the_filler(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, tracking as T
    Lib = _lib.lib()
    n, A, L = 2048, 4, 2
    fs, n_time = 1000.0 * n, 3 * n
    d_x = hipbuf.upload(_stream("c32", n_time, A, 3))
    mgr = T.TrackingManager(fs, n_channels=1, code_index_mode=T.CODE_INDEX_FIXED)
    one = [TA._record(T, 3, 100, 250.0)]
    d_z, d_done = hipbuf.alloc(4096, fill=0x5A), hipbuf.alloc(64, fill=0x5A)

    def raw(null=None, fmt=0, A=A, L=L, tau=0.0, first_index=0, n_time=n_time, n_states=1, z=None, reserved=None):
        cfg = _lib.TrkArrayCfg()
        cfg.n_antennas, cfg.taps, cfg.tap_chips = A, L, tau
        if reserved is not None:
            cfg.reserved[reserved] = 1
        arr = (T.TrkState * 1)(*one)
        p = lambda name, v: None if null == name else C.c_void_p(v)
        return Lib.gm_trk_array_prompts_dev(None if null == "handle" else mgr._h, p("samples", d_x), fmt, first_index, n_time,
                                            None if null == "states" else C.cast(arr, C.c_void_p), n_states,
                                            None if null == "cfg" else C.byref(cfg), p("z", d_z if z is None else z), p("done", d_done), None)

    cases = [(dict(null=k), INVALID) for k in ("handle", "samples", "states", "cfg", "z", "done")] + \
            [(dict(fmt=_lib.FMT_I8_REAL), INVALID), (dict(fmt=3), INVALID), (dict(A=1), RANGE), (dict(A=9), RANGE), (dict(L=0), RANGE),
             (dict(A=8, L=5), RANGE), (dict(tau=float("nan")), INVALID), (dict(tau=64.5), RANGE), (dict(first_index=1 << 62), RANGE),
             (dict(n_time=1 << 62), RANGE), (dict(n_states=0), RANGE), (dict(n_states=1025), RANGE), (dict(reserved=2), INVALID),
             (dict(z=d_x), INVALID), (dict(z=d_x + n_time * A * 8 - 8), INVALID), (dict(z=d_x - 8), INVALID)]      # d_z over the samples
    for kw, status in cases:
        assert raw(**kw) == status, kw
    mgr.synchronize()
    assert (hipbuf.download(d_z, 4096, np.uint8) == 0x5A).all() and (hipbuf.download(d_done, 64, np.uint8) == 0x5A).all()
    assert (hipbuf.download(d_x, 64, np.uint8) == _stream("c32", n_time, A, 3).view(np.uint8).reshape(-1)[:64]).all()
    assert raw() == 0                                                                                         # the same call, nothing refused
    mgr.synchronize()
    assert not (hipbuf.download(d_z, L * A * 8, np.uint8) == 0x5A).all() and hipbuf.download(d_done, 1, np.uint8)[0] == 1
    mgr.close()


def _warm(hipbuf):
    """the first launch of the solver's and the install's kernels, before anything is held (the runtime loads a code object at its first
    launch, on the host)"""
    from gnss_sdr_rs_amd import beamformer
    z, _ = _inputs(8, 2, 0, 3, 1)
    rows, _ = _device(hipbuf, z, None, 8, 2, 3, 0.0)
    bf = beamformer.Beamformer(4, 2, BM.rows(4, 2)[:1].repeat(3, axis=0), 1024, 1e-4)
    bf.set_steering_dev(0, 3, hipbuf.upload(rows))
    bf.synchronize()
    bf.close()


def test_the_device_form_on_a_held_stream_and_beside_the_synchronous_entry(gpu):
    from gnss_sdr_rs_amd import tracking as T
    n, A, L = 4097, 4, 2
    fs, n_time = 1000.0 * n, 2 * n + 777
    xd = _stream("c32", n_time, A, 100 * A + L)
    with SS.HeldStream() as S:
        d_x = S.device(xd.nbytes)
        S.put(d_x, xd)
        mgr = S.own(T.TrackingManager(fs, n_channels=2, code_index_mode=T.CODE_INDEX_FIXED))
        recs = TA._records(T, n, L, n_time, 12, 5)
        ra, rb = recs[:7], recs[7:]
        za, da = mgr.array_prompts(d_x, n_time, A, L, states=ra)          # (also grows the block to this call's size)
        zb, db = mgr.array_prompts(d_x, n_time, A, L, states=rb)
        d_z, d_done = S.device(len(ra) * L * A * 8), S.device(len(ra))
        mgr.array_prompts_dev(d_x, n_time, A, ra, d_z, d_done, taps=L, stream=S.stream)      # the stream's first call: its pinned block
        S.sync()
        assert (_words(S.get(d_z, za.nbytes).view(np.complex64)) == _words(za).reshape(-1)).all()
        S.memset(d_z, SS.FILL, za.nbytes); S.memset(d_done, SS.FILL, len(ra))
        S.sync()
        S.hold("array_prompts_dev")
        before_z, before_done = S.d2h(d_z, za.nbytes), S.d2h(d_done, len(ra))      # behind the gate, in front of the call, in stream order
        mgr.array_prompts_dev(d_x, n_time, A, ra, d_z, d_done, taps=L, stream=S.stream)
        S.assert_held()                                                            # the entry has returned; nothing behind the gate has run
        S.sync()
        # 200 ms after the entry returned the outputs still held the filler: nothing of the call ran on another stream
        assert (before_z == SS.FILL).all() and (before_done == SS.FILL).all()
        assert (_words(S.get(d_z, za.nbytes).view(np.complex64)) == _words(za).reshape(-1)).all()
        assert (S.get(d_done, len(ra)) == da).all()
        # a synchronous call right behind a _dev call on another stream: the shared block is not overwritten under the first
        S.memset(d_z, SS.FILL, za.nbytes)
        mgr.array_prompts_dev(d_x, n_time, A, ra, d_z, d_done, taps=L, stream=S.stream)
        zb2, db2 = mgr.array_prompts(d_x, n_time, A, L, states=rb)
        S.sync()
        assert (_words(zb2) == _words(zb)).all() and (db2 == db).all()
        assert (_words(S.get(d_z, za.nbytes).view(np.complex64)) == _words(za).reshape(-1)).all()
        # and the other way round
        mgr.array_prompts_dev(d_x, n_time, A, ra, d_z, d_done, taps=L, stream=S.stream)
        S.sync()
        assert (_words(S.get(d_z, za.nbytes).view(np.complex64)) == _words(za).reshape(-1)).all()


# ---- 5. gm_beamformer_set_steering_dev ---------------------------------------------------------------------------------------------------
def _beam_rows(P, M, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.standard_normal((P, M)) + 1j * rng.standard_normal((P, M)), np.complex64)


def _twin(hipbuf, A, L, rows, d_x, n_call, install):
    """two process_dev calls of n_call time samples on a handle of its own, `install(bf)` between them -> (y [2, P, n_call], w [2, ...])"""
    from gnss_sdr_rs_amd import _lib, beamformer
    P, M, nb = rows.shape[0], rows.shape[1], n_call // 1024
    bf = beamformer.Beamformer(A, L, rows, 1024, 1e-4)
    d_y, d_R, d_w = hipbuf.alloc(2 * P * n_call * 8, fill=0x5A), hipbuf.alloc(2 * nb * M * M * 8), hipbuf.alloc(2 * nb * P * M * 8, fill=0x5A)
    for k in (0, 1):
        bf.capture(d_R + k * nb * M * M * 8, d_w + k * nb * P * M * 8, nb)
        assert bf.process_dev(d_x + k * n_call * A * 8, _lib.FMT_C32, n_call, d_y + k * P * n_call * 8, n_call) == n_call
        bf.synchronize()
        if k == 0:
            install(bf)
    y, w = hipbuf.download(d_y, 2 * P * n_call * 8, np.complex64), hipbuf.download(d_w, 2 * nb * P * M * 8, np.complex64)
    bf.close()
    return y.reshape(2, P, n_call), w.reshape(2, nb, P, M)


def test_the_install_is_ordered_like_a_process_call(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, beamformer
    A, L, P, n_call = 4, 2, 3, 2048
    M, nb = A * L, n_call // 1024
    x = _stream("c32", 2 * n_call, A, 9)
    old, new = _beam_rows(P, M, 1), _beam_rows(2, M, 2)
    hx = hipbuf.upload(x)
    y_old, w_old = _twin(hipbuf, A, L, old, hx, n_call, lambda bf: None)
    y_new, w_new = _twin(hipbuf, A, L, old, hx, n_call, lambda bf: (bf.set_steering(1, new[0]), bf.set_steering(2, new[1])))
    assert (_words(y_old[0]) == _words(y_new[0])).all() and not (_words(y_old[1, 1]) == _words(y_new[1, 1])).all()
    _warm(hipbuf)
    with SS.HeldStream() as S:
        d_x, d_rows, d_inst = S.device(x.nbytes), S.device(new.nbytes), S.device(2)
        S.put(d_x, x); S.put(d_rows, new)
        d_y, d_R, d_w = S.device(2 * P * n_call * 8), S.device(2 * nb * M * M * 8), S.device(2 * nb * P * M * 8)
        bf = S.own(beamformer.Beamformer(A, L, old, 1024, 1e-4))
        S.hold("set_steering_dev between two calls")
        bf.capture(d_R, d_w, nb)
        assert bf.process_dev(d_x, _lib.FMT_C32, n_call, d_y, n_call, stream=S.stream) == n_call
        bf.set_steering_dev(1, 2, d_rows, None, 0.0, d_inst, stream=S.stream)
        bf.capture(d_R + nb * M * M * 8, d_w + nb * P * M * 8, nb)
        assert bf.process_dev(d_x + n_call * A * 8, _lib.FMT_C32, n_call, d_y + P * n_call * 8, n_call, stream=S.stream) == n_call
        S.assert_held()
        S.sync()
        y = S.get(d_y, 2 * P * n_call * 8).view(np.complex64).reshape(2, P, n_call)
        w = S.get(d_w, 2 * nb * P * M * 8).view(np.complex64).reshape(2, nb, P, M)
        assert list(S.get(d_inst, 2)) == [1, 1]
        assert (_words(y[0]) == _words(y_old[0])).all() and (_words(w[0]) == _words(w_old[0])).all()          # call 1: the old rows
        assert (_words(y[1]) == _words(y_new[1])).all() and (_words(w[1]) == _words(w_new[1])).all()          # call 2: the new ones, beam 0 untouched


def test_the_gate_and_the_refusals_of_the_install(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, beamformer
    gm = gpu
    A, L, P, n_call = 4, 2, 5, 1024
    M = A * L
    x = _stream("c32", 2 * n_call, A, 10)
    hx = hipbuf.upload(x)
    old, new = _beam_rows(P, M, 3), _beam_rows(P, M, 4)
    new[2] = 0
    new[3, 5] = complex(np.nan, 1.0)
    info = np.zeros(P, INFO)
    info["lambda1"], info["lambda2"] = [3.0, 9.0, 9.0, 9.0, 4.0], [2.0, 1.0, 1.0, 1.0, 2.0]      # row 0 fails 2.0, row 4 meets it exactly
    info["status"][1] = 4
    d_rows, d_info = hipbuf.upload(new), hipbuf.upload(info)
    for use_info, ratio, want in ((True, 2.0, [0, 0, 0, 0, 1]), (True, 0.0, [1, 0, 0, 0, 1]), (False, 0.0, [1, 1, 0, 0, 1])):
        y_want, w_want = _twin(hipbuf, A, L, old, hx, n_call, lambda bf: [bf.set_steering(p, new[p]) for p in range(P) if want[p]])
        d_inst = hipbuf.alloc(P, fill=0x5A)
        y_got, w_got = _twin(hipbuf, A, L, old, hx, n_call,
                             lambda bf: bf.set_steering_dev(0, P, d_rows, d_info if use_info else None, ratio, d_inst))
        assert list(hipbuf.download(d_inst, P, np.uint8)) == want, (use_info, ratio)
        assert (_words(y_got) == _words(y_want)).all() and (_words(w_got) == _words(w_want)).all(), (use_info, ratio)
    # a part of the beams; d_installed may be NULL
    y_want, _ = _twin(hipbuf, A, L, old, hx, n_call, lambda bf: bf.set_steering(4, new[1]))
    y_got, _ = _twin(hipbuf, A, L, old, hx, n_call, lambda bf: bf.set_steering_dev(4, 1, d_rows + M * 8))
    assert (_words(y_got) == _words(y_want)).all()
    # every refusal: nothing enqueued, the rows stay
    bf = beamformer.Beamformer(A, L, old, 1024, 1e-4)
    Lib = _lib.lib()
    f = C.c_float
    assert Lib.gm_beamformer_set_steering_dev(None, 0, 1, C.c_void_p(d_rows), None, f(0.0), None, None) == INVALID
    for args in ((0, 1, None, None, 0.0), (0, 0, d_rows, None, 0.0), (0, P + 1, d_rows, None, 0.0), (P, 1, d_rows, None, 0.0),
                 (P - 1, 2, d_rows, None, 0.0), (0xFFFFFFFF, 2, d_rows, None, 0.0), (0, 1, d_rows, None, -1.0), (0, 1, d_rows, None, float("nan")),
                 (0, 1, d_rows, d_info, float("inf"))):
        with pytest.raises(gm.GmError):
            bf.set_steering_dev(*args)
    d_y, d_R, d_w = hipbuf.alloc(P * n_call * 8), hipbuf.alloc(M * M * 8), hipbuf.alloc(P * M * 8)
    bf.capture(d_R, d_w, 1)
    bf.process_dev(hx, _lib.FMT_C32, n_call, d_y, n_call)
    bf.synchronize()
    y_old, _ = _twin(hipbuf, A, L, old, hx, n_call, lambda bf: None)
    assert (_words(hipbuf.download(d_y, P * n_call * 8, np.complex64)) == _words(y_old[0]).reshape(-1)).all()
    bf.close()


# ---- 6. the chain, no host wait ---------------------------------------------------------------------------------------------------------
def test_the_whole_update_sits_behind_one_held_gate(gpu, hipbuf):
    from gnss_sdr_rs_amd import _lib, acquisition as AQ, beamformer, tracking as T
    eng = AQ.AcquisitionEngine(EM.FS, 0.0, EM.N, doppler_hz=EM.DOP.astype(np.float32), prn_ids=[1, 2], n_integrations=EM.PERIODS,
                               codes=EM.scene_codes(), code_rate=1.023e6)
    x = BM.scene("T1", 1).astype(np.complex64)
    A, L, Mw, N = x.shape[1], 2, 8, BM.N
    assert (A, BM.TAPS["T1"], x.shape[0]) == (4, L, BM.DWELL)
    nb = BM.DWELL // 1024
    e3 = np.ascontiguousarray(BM.rows(A, L)[:1].repeat(3, axis=0))
    hx = hipbuf.upload(x)

    def figures(d_planes):
        out = []
        for w in (0, 1):
            eng.search_dev(d_planes + (1 + w) * BM.DWELL * 8, _lib.FMT_C32)
            out.append(EM.best_cell(*eng.metrics(), w))
        return out

    # the two cells behind the e_0 beam, and the yardstick: the same records through array_prompts, solve_rows and set_steering on a twin
    twin = beamformer.Beamformer(A, L, e3, 1024, 1e-4)
    d_y, d_R, d_w = hipbuf.alloc(3 * BM.DWELL * 8), hipbuf.alloc(nb * Mw * Mw * 8), hipbuf.alloc(nb * 3 * Mw * 8)
    twin.capture(d_R, d_w, nb)
    assert twin.process_dev(hx, _lib.FMT_C32, BM.DWELL, d_y, BM.DWELL) == BM.DWELL
    twin.synchronize()
    R = hipbuf.download(d_R, nb * Mw * Mw * 8, np.complex64).reshape(nb, Mw, Mw)
    eng.search_dev(d_y, _lib.FMT_C32)
    first = [EM.best_cell(*eng.metrics(), w) for w in (0, 1)]
    assert all(BM.found(first[w], w) and first[w][2] > BM.DETECT for w in (0, 1)), first
    codes = EM.scene_codes()
    recs = [TA._record(T, w + 1, int(first[w][1]) + p * N, float(EM.DOP[first[w][0]]), carrier_phase=0.0) for w in (0, 1) for p in range(9)]
    _warm(hipbuf)
    with SS.HeldStream() as S:
        mgr = S.own(T.TrackingManager(EM.FS, n_channels=2, code_index_mode=T.CODE_INDEX_FIXED, codes=codes, nominal_code_rate=1.023e6))
        z, done = mgr.array_prompts(hx, BM.DWELL, A, L, states=recs)
        assert done.all()
        rows_host, infos = AQ.solve_rows(z.reshape(2, 9, L, A), R, 1e-4)
        assert all(i["lambda1"] >= 2.0 * i["lambda2"] for i in infos), infos
        twin.capture(None, None, 0)
        twin.set_steering(1, rows_host[0]); twin.set_steering(2, rows_host[1])
        assert twin.process_dev(hx, _lib.FMT_C32, BM.DWELL, d_y, BM.DWELL) == BM.DWELL
        twin.synchronize()
        want = figures(d_y)
        twin.close()
        # the chain: everything below is enqueued on S behind the gate
        d_x = S.device(x.nbytes)
        S.put(d_x, x)
        d_y1, d_y2 = S.device(3 * BM.DWELL * 8), S.device(3 * BM.DWELL * 8)
        d_R1, d_w1, d_w2 = S.device(nb * Mw * Mw * 8), S.device(nb * 3 * Mw * 8), S.device(nb * 3 * Mw * 8)
        d_R2 = S.device(nb * Mw * Mw * 8)
        d_z, d_done, d_rows, d_info, d_inst = S.device(18 * Mw * 8), S.device(18), S.device(2 * Mw * 8), S.device(2 * 24), S.device(2)
        mgr.array_prompts_dev(d_x, BM.DWELL, A, recs, d_z, d_done, taps=L, stream=S.stream)   # the stream's first call: its pinned block
        S.sync()
        S.memset(d_z, SS.FILL, 18 * Mw * 8)
        S.sync()
        bf = S.own(beamformer.Beamformer(A, L, e3, 1024, 1e-4))
        S.hold("the chain")
        bf.capture(d_R1, d_w1, nb)
        assert bf.process_dev(d_x, _lib.FMT_C32, BM.DWELL, d_y1, BM.DWELL, stream=S.stream) == BM.DWELL
        mgr.array_prompts_dev(d_x, BM.DWELL, A, recs, d_z, d_done, taps=L, stream=S.stream)
        AQ.solve_rows_dev(Mw, 9, 2, d_z, d_rows, d_info, d_R=d_R1, n_blocks=nb, loading=1e-4, stream=S.stream)
        bf.set_steering_dev(1, 2, d_rows, d_info, 0.0, d_inst, stream=S.stream)
        bf.capture(d_R2, d_w2, nb)
        assert bf.process_dev(d_x, _lib.FMT_C32, BM.DWELL, d_y2, BM.DWELL, stream=S.stream) == BM.DWELL
        S.assert_held()
        S.sync()
        assert list(S.get(d_inst, 2)) == [1, 1] and (S.get(d_done, 18) == 1).all()
        assert (_words(S.get(d_z, 18 * Mw * 8).view(np.complex64)) == _words(z).reshape(-1)).all()
        R1 = S.get(d_R1, nb * Mw * Mw * 8).view(np.complex64).reshape(nb, Mw, Mw)
        rows_dev = S.get(d_rows, 2 * Mw * 8).view(np.complex64).reshape(2, Mw)
        info = S.get(d_info, 48).view(INFO)
        rows_ref, infos_ref = AQ.solve_rows(z.reshape(2, 9, L, A), R1, 1e-4)
        dw = float(np.max(np.abs(rows_dev.astype(np.complex128) - rows_ref.reshape(2, Mw).astype(np.complex128))))
        print("the chain: device rows within %.2e of the host rows (bar %.0e), lambda1 / lambda2 %s" %
              (dw, ROW_BAR, [float(i["lambda1"] / i["lambda2"]) for i in info]))
        assert not info["status"].any() and dw <= ROW_BAR
        assert [int(i) for i in info["ref_index"]] == [i["ref_index"] for i in infos_ref]
        # pass 1 ran with e_0 on every beam; pass 2's beams 1 and 2 with the new rows
        w2 = S.get(d_w2, nb * 3 * Mw * 8).view(np.complex64).reshape(nb, 3, Mw)
        w1 = S.get(d_w1, nb * 3 * Mw * 8).view(np.complex64).reshape(nb, 3, Mw)
        # (block 0 of pass 2 has pass 1's last samples in its halo, so only the blocks behind it repeat pass 1's Gram matrices)
        assert (_words(w1[:, 1]) == _words(w1[:, 0])).all() and (_words(w2[1:, 0]) == _words(w1[1:, 0])).all()
        assert not (_words(w2[1:, 1]) == _words(w1[1:, 1])).all() and not (_words(w2[1:, 2]) == _words(w2[1:, 1])).all()
        got = figures(d_y2)
        for w in (0, 1):
            print("T1 seed 1, satellite %d: behind the device row %s, behind the host row on the twin %s (%.3f of it, bar %.1f)"
                  % (w, got[w], want[w], got[w][2] / want[w][2], QUALITY_BAR))
            assert BM.found(got[w], w) and got[w][2] > BM.DETECT
            assert got[w][2] >= QUALITY_BAR * want[w][2]
    eng.close()
