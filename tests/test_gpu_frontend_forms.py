"""Digital front-end: every kernel form (fe_kernels.hip: sequential, table, speculative; c32 and int8) at its state, sign and run edges.
Every output float and all 17 state words are compared BIT-EXACT with the oracle run on the same stream with the same cuts, and every
case asserts through gm_frontend_debug_forms which form ran, so a dispatch change cannot quietly move a case onto another kernel.
tests/fe_model.py holds the case tables, the inputs and the model of the dispatch; tests/test_fe_model_host.py checks them on a CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_model as M

pytestmark = pytest.mark.gpu

FMTS = pytest.mark.parametrize("i8", [False, True], ids=["c32", "i8"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_state(fe, ofe):
    ph, br, bi = fe.state()
    want = np.float32(ofe.s.phase_accumulator)
    if np.isnan(want):
        assert np.isnan(ph)
    else:
        assert _bits(np.float32(ph)) == _bits(want), (ph, want)
    assert (_bits(br) == _bits(np.array(ofe.s.bias_re[:], np.float32))).all()
    assert (_bits(bi) == _bits(np.array(ofe.s.bias_im[:], np.float32))).all()


def _pair(oracle, key):
    from gnss_sdr_rs_amd import frontend as F
    return F.DigitalFrontend(key[0], key[1], key[1]), oracle.DigitalFrontend(key[0], key[1], key[1])


def _fmt(i8):
    from gnss_sdr_rs_amd import _lib
    return _lib.FMT_I8_IQ if i8 else _lib.FMT_C32


def _set_both(fe, ofe, phase, br, bi):
    fe.set_state(float(phase), br, bi)
    ofe.s.phase_accumulator = float(phase)
    ofe.s.bias_re[:] = [float(v) for v in br]
    ofe.s.bias_im[:] = [float(v) for v in bi]


def _biases(rng):
    """sixteen biases, none zero, both signs"""
    b = (rng.uniform(0.5, 20.0, 16) * np.where(np.arange(16) % 3 == 1, -1.0, 1.0)).astype(np.float32)
    return b[:8], b[8:]


def _block(fe, ofe, hipbuf, raw, f32, i8, tag=None):
    """one out-of-place process_dev call against the oracle's process_block on the same samples: outputs and state"""
    n = f32.size // 2
    d_in, d_out = hipbuf.upload(raw), hipbuf.alloc(n * 8)
    fe.process_dev(d_in, _fmt(i8), d_out, n)
    fe.synchronize()
    got = hipbuf.download(d_out, n * 8, np.float32)
    want = ofe.process_block(f32.copy())
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (tag, n, bad.size, bad[:4] // 2)
    _same_state(fe, ofe)


def _delta(fe, before):
    return tuple(int(a) - int(b) for a, b in zip(fe.debug_forms(), before))


def _only(form, count=1):
    return tuple(count if i == form else 0 for i in range(3))


# ------------------------------------------------------------------------------------------------ A: set state
@FMTS
@pytest.mark.parametrize("name,value", M.A_PHASES, ids=[p[0] for p in M.A_PHASES])
@pytest.mark.parametrize("key", M.A_SETTINGS, ids=["pos_if", "neg_if"])
def test_set_state_then_three_blocks(gpu, oracle, hipbuf, key, name, value, i8):
    """gm_frontend_set_state, then blocks of 8, 2048 + 8 and 2 * 2048 + 8 * 3 + 5 samples.  A phase on the tabulated orbit (what a twin
    handle holds after 1000 samples, and a zero of either sign: entry 0) stays on the TABLE form; every other phase sends the handle down
    the SEQUENTIAL kernel: +-1000.5 with the step's sign and 2047.9999 / -5 where the sign agrees through nco_segment_fast, the wrong sign
    through the fmodf loop for one segment and the fast chain after it, 5e9 / 3e19 / -5 into the upper, saturating and zero branches of the
    LUT index on the first sample, NaN with index 0 for ever."""
    rng = np.random.default_rng(100 + len(name) + 7 * i8)
    fe, ofe = _pair(oracle, key)
    if name == "on_orbit":
        twin, otwin = _pair(oracle, key)
        raw, f32 = M.noise_dc(1, 1000, i8)
        _block(twin, otwin, hipbuf, raw, f32, i8)
        phase = np.float32(twin.state()[0])
        twin.close()
        assert _bits(phase) == _bits(M.a_phase(name, value, *key))
    else:
        phase = M.a_phase(name, value, *key)
    br, bi = _biases(rng)
    _set_both(fe, ofe, phase, br, bi)
    _same_state(fe, ofe)
    want = M.TAB if name in ("on_orbit", "neg_zero", "pos_zero") else M.SEQ
    for n in M.A_BLOCKS:
        before = fe.debug_forms()
        raw, f32 = M.noise_dc(int(rng.integers(1 << 30)), n, i8)
        _block(fe, ofe, hipbuf, raw, f32, i8, (name, n))
        assert _delta(fe, before) == _only(want), (name, n)
    fe.close()


@FMTS
@pytest.mark.parametrize("phase", [0.0, -0.0], ids=["pos_zero", "neg_zero"])
@pytest.mark.parametrize("key", M.A_SETTINGS, ids=["pos_if", "neg_if"])
def test_zero_phase_through_the_sequential_kernel(gpu, oracle, hipbuf, key, phase, i8):
    """A zero phase stands on the table, so alone it never meets the sequential kernel's sign rules.  Beside a member that has no table
    it does: the same three blocks in batches of two, -0.0 with a positive step and +0.0 with a negative one through nco_segment_fast."""
    from gnss_sdr_rs_amd import frontend as F
    rng = np.random.default_rng(41)
    fe, ofe = _pair(oracle, key)
    other, oother = _pair(oracle, M.NO_TABLE)
    br, bi = _biases(rng)
    _set_both(fe, ofe, np.float32(phase), br, bi)
    for n in M.A_BLOCKS:
        before = fe.debug_forms(), other.debug_forms()
        ins = [M.noise_dc(int(rng.integers(1 << 30)), n, i8) for _ in range(2)]
        d_in, d_out = [hipbuf.upload(r) for r, _ in ins], [hipbuf.alloc(n * 8) for _ in ins]
        F.process_dev_batch([fe, other], d_in, _fmt(i8), d_out, n)
        fe.synchronize()
        for h, o, (_, f32), d in zip((fe, other), (ofe, oother), ins, d_out):
            assert (_bits(hipbuf.download(d, n * 8, np.float32)) == _bits(o.process_block(f32.copy()))).all(), n
            _same_state(h, o)
        assert _delta(fe, before[0]) == _only(M.SEQ) and _delta(other, before[1]) == _only(M.SEQ)
    fe.close(); other.close()


@FMTS
@pytest.mark.parametrize("phase", [None, 0.0, -0.0], ids=["fresh", "pos_zero", "neg_zero"])
@pytest.mark.parametrize("key", M.A_SETTINGS + [(0.0, 8.0e6)], ids=["pos_if", "neg_if", "zero_if"])
def test_block_without_a_whole_chunk_leaves_the_phase_alone(gpu, oracle, hipbuf, key, phase, i8):
    """Fewer than 8 samples: nothing is processed and the accumulator keeps its bits — +0.0 on a fresh handle with a negative step (the
    table's entry 0 times -2048 would be -0.0), -0.0 where that was set before a positive step — on the table form; then 8 samples."""
    rng = np.random.default_rng(5)
    fe, ofe = _pair(oracle, key)
    if phase is not None:
        br, bi = _biases(rng)
        _set_both(fe, ofe, np.float32(phase), br, bi)
    for n in (5, 8, 7):
        before = fe.debug_forms()
        raw, f32 = M.noise_dc(n, n, i8)
        _block(fe, ofe, hipbuf, raw, f32, i8, n)
        assert _delta(fe, before) == _only(M.TAB), n
    fe.close()


# ------------------------------------------------------------------------------------------------ B: mixed batch
@FMTS
def test_mixed_batch_hands_over_to_the_table_form(gpu, oracle, hipbuf, i8):
    """One launch of three handles on their tables, one without a table and one set off its orbit: the sequential kernel runs the chains
    of all five while the host advances the table positions of the first three; two calls, then every handle alone — the three
    are back on the table form, at the position the batch left them, and everything is exact throughout."""
    from gnss_sdr_rs_amd import frontend as F
    rng = np.random.default_rng(12 + i8)
    pairs = [_pair(oracle, k) for k in M.B_SETTINGS]
    fes, ofes = [p[0] for p in pairs], [p[1] for p in pairs]
    br, bi = _biases(rng)
    _set_both(fes[4], ofes[4], np.float32(M.B_OFF_ORBIT_PHASE), br, bi)
    n = M.B_N
    for call in range(2):
        before = [f.debug_forms() for f in fes]
        ins = [M.noise_dc(int(rng.integers(1 << 30)), n, i8) for _ in fes]
        d_in, d_out = [hipbuf.upload(r) for r, _ in ins], [hipbuf.alloc(n * 8) for _ in fes]
        F.process_dev_batch(fes, d_in, _fmt(i8), d_out, n)
        fes[0].synchronize()
        for i in range(len(fes)):
            want = ofes[i].process_block(ins[i][1].copy())
            assert (_bits(hipbuf.download(d_out[i], n * 8, np.float32)) == _bits(want)).all(), (call, i)
            _same_state(fes[i], ofes[i])
            assert _delta(fes[i], before[i]) == _only(M.SEQ), (call, i)
    for i, want in enumerate([M.TAB, M.TAB, M.TAB, M.SEQ, M.SEQ]):
        before = fes[i].debug_forms()
        raw, f32 = M.noise_dc(int(rng.integers(1 << 30)), M.B_ALONE_N, i8)
        _block(fes[i], ofes[i], hipbuf, raw, f32, i8, ("alone", i))
        assert _delta(fes[i], before) == _only(want), i
    for f in fes:
        f.close()


# ------------------------------------------------------------------------------------------------ C: table form, long
@pytest.mark.parametrize("key", M.C_SETTINGS, ids=["zero_if", "period_65536", "transient_4002", "neg_period_8388599"])
def test_table_form_over_49_segments_in_place(gpu, oracle, key):
    """process_block (in place, so never speculative) on 48 * 3840 + 8 * 37 + 5 samples after a 1000-sample call: 49 pipeline segments, the
    last of 37 steps (two groups of sixteen, one quad, one step), a 5-sample tail; tab_pos is off the segment grid and the period folds."""
    fe, ofe = _pair(oracle, key)
    for n in (1000, M.N_RAGGED):
        _, f32 = M.noise_dc(n + int(abs(key[0])) % 97, n, False)
        before = fe.debug_forms()
        got = fe.process_block(f32.copy())
        want = ofe.process_block(f32.copy())
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert bad.size == 0, (n, bad.size, bad[:4] // 2)
        _same_state(fe, ofe)
        assert _delta(fe, before) == _only(M.TAB), n
    fe.close()


@FMTS
def test_speculative_threshold(gpu, oracle, hipbuf, i8):
    """out of place: FE_SPEC_MIN - 1 samples on the table form, FE_SPEC_MIN on the speculative one"""
    fe, ofe = _pair(oracle, M.C_BOUNDARY_SETTING)
    for n, want in ((M.SPEC_MIN - 1, M.TAB), (M.SPEC_MIN, M.SPEC)):
        before = fe.debug_forms()
        raw, f32 = M.noise_dc(n, n, i8)
        _block(fe, ofe, hipbuf, raw, f32, i8, n)
        assert _delta(fe, before) == _only(want), n
    fe.close()


# ------------------------------------------------------------------------------------------------ D: speculative form, shapes
@pytest.mark.parametrize("i8,key,lens", M.D_CASES, ids=["%s-%g-%s" % ("i8" if c[0] else "c32", c[1][0], c[2]) for c in M.D_CASES])
def test_speculative_shapes(gpu, oracle, hipbuf, i8, key, lens):
    """The speculative form as shipped (K = 32, 18 warm-up segments), after a 1000-sample block: 48 segments (24 runs of 2, 8 empty), 49 with
    a ragged last one, 65 (22 runs, the last of 2), and 137 followed by 48 on the same handle (the records of runs 24 .. 27 are stale
    then); positive and negative IF, a table that folds inside the block, a table with a transient."""
    fe, ofe = _pair(oracle, key)
    raw, f32 = M.noise_dc(3, 1000, i8)
    _block(fe, ofe, hipbuf, raw, f32, i8, "first")
    guessed = 0
    for n in M.D_LEN[lens]:
        before = fe.debug_forms()
        raw, f32 = M.noise_dc(n % 1000 + 17 * i8, n, i8)
        _block(fe, ofe, hipbuf, raw, f32, i8, n)
        assert _delta(fe, before) == _only(M.SPEC), n
        guessed += len(M.guessed_runs(M.nseg_of(n), M.SPEC_K))
        assert fe.debug_repairs() <= guessed, (n, fe.debug_repairs(), guessed)
    fe.close()


# ------------------------------------------------------------------------------------------------ E: speculative form, the walk
def _child_block(fe, ofe, hipbuf, raw_i8, i8, env):
    """one block under the GM_FE_* values of env (read at every launch): exact, speculative; returns the runs it repaired"""
    for k in ("GM_FE_SPEC", "GM_FE_SPEC_K", "GM_FE_SPEC_WARM"):
        os.environ.pop(k, None)
    os.environ.update(env)
    forms, repairs = fe.debug_forms(), fe.debug_repairs()
    raw = raw_i8 if i8 else raw_i8.astype(np.float32)
    _block(fe, ofe, hipbuf, raw, raw_i8.astype(np.float32), i8, env)
    assert _delta(fe, forms) == _only(M.SPEC), env
    return fe.debug_repairs() - repairs


def child_main(mode):
    """runs in a process started with GM_DIAGNOSTICS=1 (the parent test asserts its return code and the counts it prints)"""
    from conftest import HipBuffers
    from oracle import oracle
    from gnss_sdr_rs_amd import _lib
    _lib.init(0)
    hipbuf = HipBuffers()
    out = []
    for i8 in (False, True):
        fe, ofe = _pair(oracle, M.E_SETTING)
        if mode == "sweep":
            raw = M.wander_i8(77, 1000 + M.N_RAGGED + M.E_N137)
            cut = {48: raw[2000:2000 + 2 * M.N_RAGGED], 137: raw[2000 + 2 * M.N_RAGGED:]}
            _block(fe, ofe, hipbuf, raw[:2000] if i8 else raw[:2000].astype(np.float32), raw[:2000].astype(np.float32), i8, "first")
            for k, w, segs in M.E_SWEEP:
                env = {} if k is None else {"GM_FE_SPEC_K": str(k)}
                if w is not None:
                    env["GM_FE_SPEC_WARM"] = str(w)
                plain = _child_block(fe, ofe, hipbuf, cut[segs], i8, env)
                spoiled = _child_block(fe, ofe, hipbuf, cut[segs], i8, dict(env, GM_FE_SPEC="2"))
                out.append([i8, k, w, segs, plain, spoiled])
        else:
            raw = M.wander_i8(M.E_SEED, 1000 + 2 * M.N_RAGGED)
            _block(fe, ofe, hipbuf, raw[:2000] if i8 else raw[:2000].astype(np.float32), raw[:2000].astype(np.float32), i8, "first")
            env = {"GM_FE_SPEC_WARM": str(M.E_W_MIX)}
            first = _child_block(fe, ofe, hipbuf, raw[2000:2000 + 2 * M.N_RAGGED], i8, env)
            second = _child_block(fe, ofe, hipbuf, raw[2000 + 2 * M.N_RAGGED:], i8, env)
            spoiled = _child_block(fe, ofe, hipbuf, raw[2000:2000 + 2 * M.N_RAGGED], i8, dict(env, GM_FE_SPEC="2"))
            out.append([i8, first, second, spoiled])
        fe.close()
    hipbuf.close()
    print("RESULT " + json.dumps(out), flush=True)


def _run_child(mode):
    from conftest import ROOT
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_frontend_forms as T; T.child_main(%r)" % (ROOT, os.path.join(ROOT, "tests"), mode)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GM_DIAGNOSTICS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    print(line)
    return json.loads(line[7:])


def test_walk_at_k_2_and_64_and_a_warm_up_of_one_segment(gpu, oracle):
    """GM_FE_SPEC_K = 2 and 64 at 49 and 137 segments, and GM_FE_SPEC_WARM = 1 at the shipped K, c32 and int8, each block once as it is and
    once with every guess spoiled (GM_FE_SPEC=2): exact (asserted in the child), and the spoiled block repairs exactly the runs that the
    setting makes guessed ones — 1 of 2, 30 or 39 of 64, 24 with a one-segment warm-up — which is how the counters show that the setting took
    effect.  With a one-segment warm-up no guess has converged in the model (0 of 24 standing): more runs are repaired than the shipped
    warm-up has guessed runs (15).  Measured on the MI355X: 24 of 24 repaired, c32 and int8."""
    res = _run_child("sweep")
    assert len(res) == 2 * len(M.E_SWEEP)
    for i8, k, w, segs, plain, spoiled in res:
        guessed = len(M.guessed_runs(49 if segs == 48 else 137, M.clamp_k(k or M.SPEC_K), w or M.SPEC_WARM))
        assert guessed == {(2, 48): 1, (2, 137): 1, (64, 48): 30, (64, 137): 39, (None, 48): 24}[(k, segs)]
        assert spoiled == guessed, (i8, k, w, segs, spoiled)
        assert 0 <= plain <= guessed, (i8, k, w, segs, plain)
        if w == 1:
            assert plain > len(M.guessed_runs(49, M.SPEC_K)), plain


def test_walk_with_some_runs_standing_and_some_repaired(gpu, oracle):
    """The mixed walk: GM_FE_SPEC_WARM = 12 on two consecutive 49-segment blocks of clipped int8 noise around a wandering DC offset (the
    same values as c32).  The model (fe_model.predict_standing, checked in test_fe_model_host.py) predicts 6 and 10 of the 18 guessed runs
    standing; the GPU sums its guess in 128 parts, so its count may differ by a run or two: 0 < repairs < 18 in each block, and 18 once
    every guess is spoiled.  Exactness is asserted in the child for every block.
    Measured on the MI355X: 12 and 8 runs repaired (6 and 10 standing), c32 and int8 alike."""
    res = _run_child("mixed")
    assert len(res) == 2
    for i8, first, second, spoiled in res:
        assert 0 < first < 18 and 0 < second < 18, (i8, first, second)
        assert spoiled == 18, (i8, spoiled)


# ------------------------------------------------------------------------------------------------ F: across the ring's wrap
@FMTS
def test_speculative_block_across_the_ring_wrap(gpu, oracle, i8):
    """A ring of 2^18: 1000 samples, then 2^18 in one staging slot — one speculative block that wraps after 261 144 samples — then 2^18
    again; after each write the mirror's last 2^18 samples are the oracle's."""
    from gnss_sdr_rs_amd import tracking as T
    size = 1 << 18
    fe, ofe = _pair(oracle, (2.5e6, 10.0e6))
    ring = T.MulticastRingBuffer(size)
    total, outs = 0, []
    for n, want in ((1000, M.TAB), (size, M.SPEC), (size, M.SPEC)):
        raw, f32 = M.noise_dc(n + total % 1000, n, i8)
        before = fe.debug_forms()
        fe.write_ring(ring, raw if i8 else raw.view(np.complex64))
        ring.flush()
        total += n
        assert ring.get_head() == total and _delta(fe, before) == _only(want), n
        outs.append(ofe.process_block(f32.copy()).view(np.complex64))
        k = min(total, size)
        got = ring.copy_to_slice(total - k, k)
        assert (got.view(np.uint32) == np.concatenate(outs)[-k:].view(np.uint32)).all(), n
        _same_state(fe, ofe)
    fe.close(); ring.close()
