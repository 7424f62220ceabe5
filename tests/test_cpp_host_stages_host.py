"""The host-only part of the C++ mirror's classes (gnss-sdr-rs_amd/host/gnss_sdr.hpp) through tests/cpp/host_stages.cpp --cpu-only, no
GPU: Ddc::plan, TrackingManager::bank_plan and ::array_plan and solve_plan against the Python layer's plans word for word; solve_row
against the Python layer bit for bit and against tests/array_probe_model.py at test_array_probe_host.py's ROW_BAR; glonass_code() and
glonass_channels(M); one refused construction per class, whose gnss::Panic must carry the status of the Python layer's GmError.

Of the four plans only Ddc::plan takes a stream position: it runs at inputs_so_far = 0, T - 1, 2^32 - 3 and 2^40 + 12345.  The other
three have no such argument; they run over the shapes instead (taps x offsets x states, antennas x taps, m x n x rows x blocks and the
two strides)."""
import numpy as np
import pytest

import array_probe_model as PM
import host_stages_case as H
from test_array_probe_host import ROW_BAR


@pytest.fixture(scope="module")
def exe(gm):
    return H.build(gm)[0]


DDC = [(0.25, 16, 1, 0), (0.1234, 1, 16, 0), (-0.37, 6, 4, 0), (4.092e6 / 16.368e6, 20460, 40919, 32)]


def test_the_plans(gm, exe, tmp_path):
    from gnss_sdr_rs_amd import acquisition, ddc, tracking
    steps = []
    for mix, up, down, taps in DDC:
        T = ddc.plan(mix, up, down, taps=taps)["taps"]
        for so_far in (0, T - 1, (1 << 32) - 3, (1 << 40) + 12345):
            for n_in in (0, 1, T // 2 + 1, 4097):
                def f(o, hb, a=(mix, up, down, so_far, n_in, taps)):
                    p = ddc.plan(a[0], a[1], a[2], a[3], a[4], taps=a[5])
                    return [H.u64("n_out", p["n_out"]), H.u64("phase_inc", p["phase_inc"]), H.u64("n_out.alone", p["n_out"])]
                steps.append((H.pk("IdIIIIfffQQ", 1, mix, up, down, taps, 0, 0.0, 0.0, 0.0, so_far, n_in), f))
    for fs, rate, code_len, taps, offs, ns in ((4.092e6, 0.0, 0, [-0.5, 0.0, 0.5], [], 1), (16.368e6, 0.0, 0, np.linspace(-1, 1, 41), [-250.0, 0.0, 250.0], 15),
                                               (2.048e6, 0.511e6, 511, [0.0], [10.0], 3), (16.368e6, 10.23e6, 10230, np.linspace(-2, 2, 9), [], 64)):
        def f(o, hb, a=(fs, taps, offs, ns, rate, code_len)):
            p = tracking.bank_plan(a[0], a[1], a[2] if len(a[2]) else None, a[3], a[4], a[5])
            return [H.u64("bank_plan", *[p[k] for k in ("n_taps", "n_offsets", "out_words", "samples", "slices", "tap_groups")])]
        steps.append((H.pk("IffI", 2, fs, rate, code_len) + H.words(np.float32, taps) + H.words(np.float32, offs) + H.pk("I", ns), f))
    for fs, rate, code_len, A, L, chips, ns in ((4.092e6, 0.0, 0, 2, 1, 0.0, 1), (16.368e6, 0.0, 0, 8, 4, 0.5, 15), (2.048e6, 0.511e6, 511, 4, 8, 0.25, 3),
                                                (16.368e6, 0.0, 0, 3, 5, 1.0, 64)):
        def f(o, hb, a=(fs, A, L, chips, ns, rate, code_len)):
            p = tracking.array_plan(*a)
            return [H.u64("array_plan", *[p[k] for k in ("words_per_record", "out_words", "samples", "slices")])]
        steps.append((H.pk("IffIIIfI", 3, fs, rate, code_len, A, L, chips, ns), f))
    for m, n, rows, blocks, rs, vs, ld in ((2, 1, 1, 0, 0, 0, 0.0), (32, 4096, 1024, 1 << 20, 0, 0, 1e-4), (8, 20, 3, 5, 8 * 20 + 7, 9, 1e-2),
                                           (16, 10, 16, 0, 16, 16 * 16, 0.0)):
        def f(o, hb, a=(m, n, rows, blocks, rs, vs, ld)):
            p = acquisition.solve_plan(*a)
            return [H.u64("solve_plan", p["z_words"], p["R_words"], p["row_words"])]
        steps.append((H.pk("IIIIIQQf", 4, m, n, rows, blocks, rs, vs, ld), f))
    # the refusals of the four, in the same list: the status is the Python layer's
    bad = [(H.pk("IdIIIIfffQQ", 1, 0.25, 17, 1, 0, 0, 0.0, 0.0, 0.0, 0, 0), lambda o, hb: ddc.plan(0.25, 17, 1)),
           (H.pk("IffI", 2, 4.092e6, 0.0, 0) + H.words(np.float32, np.zeros(65)) + H.words(np.float32, []) + H.pk("I", 1), lambda o, hb: tracking.bank_plan(4.092e6, np.zeros(65), None)),
           (H.pk("IffIIIfI", 3, 4.092e6, 0.0, 0, 1, 1, 0.0, 1), lambda o, hb: tracking.array_plan(4.092e6, 1)),
           (H.pk("IIIIIQQf", 4, 33, 4, 1, 0, 0, 0, 0.0), lambda o, hb: acquisition.solve_plan(33, 4, 1))]
    steps += [H.refused(s) for s in bad]
    body, run = H.case(b"", steps)
    H.same(H.run_driver(exe, "plans", body, tmp_path, cpu_only=True), run(None), "plans")


def _cell(m, n, blocks, seed):
    """n prompt vectors along one direction plus noise, and `blocks` Gram blocks of a jammed array"""
    rng = np.random.default_rng(seed)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    z = (c(n, 1) * np.exp(2j * np.pi * rng.random(m))[None, :] * 40.0 + c(n, m)).astype(np.complex64)
    if not blocks:
        return z, None
    x = c(blocks, 256, m) + 30.0 * c(blocks, 256, 1) * np.exp(2j * np.pi * rng.random(m))[None, None, :]
    return z, np.einsum("bti,btj->bij", x, x.conj()).astype(np.complex64)


def test_solve_row(gm, exe, tmp_path):
    from gnss_sdr_rs_amd import acquisition
    cells = [(2, 1, 0, 0.0, 1), (4, 10, 0, 0.0, 1), (8, 20, 3, 1e-4, 1), (32, 10, 1, 1e-2, 1), (16, 7, 2, 0.0, 0)]
    steps = []
    for k, (m, n, blocks, loading, with_info) in enumerate(cells):
        z, R = _cell(m, n, blocks, 40 + k)

        def f(o, hb, a=(z, R, loading, with_info)):
            row, info = acquisition.solve_row(a[0], a[1], a[2])
            out = [H.rec("row", row)]
            return out + ([H.rec("lambda", np.array([info["lambda1"], info["lambda2"]])), H.u32("ref_index", info["ref_index"])] if a[3] else [])
        steps.append((H.pk("II", 1, m) + H.pk("Q", z.size) + H.raw(z) + H.pk("Q", 0 if R is None else R.size) + (b"" if R is None else H.raw(R))
                      + H.pk("fI", loading, with_info), f))
    bad = (H.pk("II", 1, 4) + H.pk("Q", 8) + H.raw(np.zeros(8, np.complex64)) + H.pk("Q", 0) + H.pk("fI", 0.0, 1),
           lambda o, hb: acquisition.solve_row(np.zeros((2, 4), np.complex64)))
    steps.append(H.refused(bad))
    body, run = H.case(b"", steps)
    got = H.run_driver(exe, "solve_row", body, tmp_path, cpu_only=True)
    H.same(got, run(None), "solve_row")
    # the C++ words of every cell against the float64 model, rotated at the library's ref_index: test_array_probe_host.py's bar
    rows, refs, k = H.get(got, "row", np.complex64), H.get(got, "ref_index", np.uint32), 0
    for i, (m, n, blocks, loading, with_info) in enumerate(cells):
        if not with_info:
            continue
        z, R = _cell(m, n, blocks, 40 + i)
        want, winfo = PM.solve_row(z, R, loading, ref_index=int(refs[k][0]))
        k += 1
        err = float(np.abs(rows[i].astype(np.complex128) - want).max())
        print("solve_row m = %d, n = %d: lambda1 / lambda2 = %.3g, largest word difference %.2e (bar %.0e)"
              % (m, n, winfo["lambda1"] / max(winfo["lambda2"], 1e-300), err, ROW_BAR))
        assert winfo["lambda1"] >= 2.0 * winfo["lambda2"] and err <= ROW_BAR, (m, n, err)


def test_the_glonass_code_and_channels(gm, exe, tmp_path):
    from gnss_sdr_rs_amd import channelizer
    Ms = (16, 32, 64)
    got = H.run_driver(exe, "glonass", H.pk("I", len(Ms)) + b"".join(H.pk("I", M) for M in Ms), tmp_path, cpu_only=True)
    want = [H.rec("code", channelizer.glonass_code())] + [H.rec("channels", channelizer.glonass_channels(M), np.uint32) for M in Ms]
    H.same(got, want, "glonass")
    chips = np.frombuffer(got[0][1], np.int8)
    assert chips.size == 511 and set(chips.tolist()) == {-1, 1}


# (class number of the driver's `refuse`, a, b, c, d, words) and the Python layer's call with the same arguments
def _refusals():
    from gnss_sdr_rs_amd import beamformer, channelizer, ddc, excise, lcmv, nuller, resample, stap
    e = lambda n: np.eye(1, n, dtype=np.complex64).reshape(-1)
    return [("resampler up/down > 16", 0, 17, 1, 0, 0, [], lambda: resample.plan(17, 1)),
            ("excisor block 100", 1, 100, 0, 0, 0, [], lambda: excise.plan(100)),
            ("ddc up/down < 1/16", 2, 1, 17, 0, 0, [], lambda: ddc.plan(0.25, 1, 17)),
            ("channelizer D > M", 3, 4, 5, 0, 0, [], lambda: channelizer.plan(4, 5)),
            ("nuller of one antenna", 4, 1, 256, 0, 0, [], lambda: nuller.plan(1, 256)),
            ("nuller steering of the wrong size", 4, 4, 256, 0, 0, e(3), lambda: nuller.plan(4, 256, steering=e(3))),
            ("stap taps * n_antennas > 32", 5, 8, 5, 256, 0, [], lambda: stap.plan(8, 5, 256)),
            ("stap steering of the wrong size", 5, 4, 2, 256, 0, e(7), lambda: stap.plan(4, 2, 256, steering=e(7))),
            ("beamformer of 17 beams", 6, 2, 1, 256, 0, np.tile(e(2), 17), lambda: beamformer.plan(2, 1, np.tile(e(2), 17), 256)),
            ("beamformer steering no whole row", 6, 2, 2, 256, 0, e(6), lambda: beamformer.plan(2, 2, e(6), 256)),
            ("lcmv with no beams", 7, 2, 1, 256, 0, e(2), lambda: lcmv.plan(2, 1, [], block=256)),
            ("lcmv of 17 rows", 7, 2, 1, 256, 3, np.tile(e(2), 6), lambda: lcmv.plan(2, 1, [(np.tile(e(2), 6).reshape(6, 2), np.ones(6))] * 3, block=256))]


@pytest.mark.parametrize("k", range(12))
def test_a_refused_construction_throws_the_python_layers_status(gm, exe, tmp_path, k):
    from gnss_sdr_rs_amd import _lib
    name, cls, a, b, c, d, w, py = _refusals()[k]
    try:
        py()
    except _lib.GmError as e:
        status = e.status
    except ValueError:
        status = H.INVALID                      # the Python wrapper's own size check stands for the header's
    else:
        raise AssertionError(name + ": the Python layer took it")
    got = H.run_driver(exe, "refuse", H.pk("IIIII", cls, a, b, c, d) + H.words(np.complex64, w), tmp_path, cpu_only=True, want=3)
    assert [t for t, _ in got] == ["panic", "panic.text"], (name, got)
    assert np.frombuffer(got[0][1], np.int32)[0] == status, (name, got, status)
    assert got[1][1], name
