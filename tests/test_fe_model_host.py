"""CPU: tests/fe_model.py (the model of the front-end's dispatch) against the oracle, and the inputs and claims of
tests/test_gpu_frontend_forms.py against the model: every GPU case takes the kernel form it says it covers, and the mixed walk's
input meets its condition."""
import numpy as np
import pytest

import fe_model as M

SETTINGS = sorted(set(M.A_SETTINGS + M.B_SETTINGS + M.C_SETTINGS + [c[1] for c in M.D_CASES] + [M.E_SETTING, (1.0e6, 3.0e6)]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_orbits():
    """(mu, lam, lam') of the settings the GPU cases use.  ((-0.4e6, 8e6): the first lap of 20 steps adds 0.05 to values below 1/2, which
    keep finer bits than any value that has been through a sum above 1; they are never visited again: a transient of 20.)"""
    want = {(0.0, 8.0e6): (0, 1, 3840), (2.0e6, 8.0e6): (0, 4, 3840), (-1.25e6, 8.0e6): (0, 32, 3840), (1.0e6, 3.0e6): (0, 3, 3840),
            (1.0e6, 8.0e6): (0, 8, 3840), (3.999e6, 8.0e6): (4002, 1048076, 1048076), (-0.4e6, 8.0e6): (20, 8388599, 8388599),
            (1.0001e6, 6.5536e6): (0, 65536, 65536), (4.1304e6, 16.3676e6): (3, 6313323, 6313323)}
    for key in SETTINGS:
        o = M.orbit(*key)
        if key == M.NO_TABLE:
            assert o is None and float(M.phase_step(*key)) == 3072.0
        else:
            assert o[1:] == want[key], (key, o)
            assert o[3] >= M.SEG and o[3] % o[2] == 0 and o[3] - o[2] < M.SEG
    assert M.orbit(10.0, 50.0e6) is not None                      # a small step, not a denormal one
    assert not M.has_table(np.float32(1.0e-30)) and not M.has_table(np.float32("nan")) and not M.has_table(np.float32(-2048.0))


@pytest.mark.parametrize("f_if,fs", [s for s in SETTINGS if s != M.NO_TABLE])
def test_table_phases_are_the_oracles_chain(oracle, f_if, fs):
    """2048 * r_k (signed) is the oracle's phase_accumulator, bit for bit, over mu + lam' + 5000 steps.  The oracle shows its
    accumulator between chunks of 8 samples: it is read after every chunk over the first 65 536 steps and after every 481 chunks from
    there on (the chain is a function of the accumulator alone: equal at a cut, it cannot have differed before it and met again
    other than by two different values stepping onto the same one); chains entered at every other offset, over the first 5 000 steps."""
    o = M.orbit_table(f_if, fs)
    step, mu, lam, lam2, tab = o
    ofe = oracle.DigitalFrontend(f_if, fs, fs)
    assert _bits(np.float32(ofe.s.phase_step)) == _bits(step)
    total = (mu + lam2 + 5000 + 7) & ~7
    buf = np.zeros(2 * 3848, np.float32)
    p = 0
    assert _bits(np.float32(ofe.s.phase_accumulator)) == _bits(np.float32(0.0))
    while p < total:
        n = 8 if p < 65536 else min(3848, total - p)
        ofe.process_block(buf[:2 * n])
        p += n
        assert _bits(np.float32(ofe.s.phase_accumulator)) == _bits(M.table_phase(o, M.fold(o, p))), p
    for off in range(1, 8):
        for p in range(off, 5000, 8):
            ofe.s.phase_accumulator = float(M.table_phase(o, M.fold(o, p))) if p else 0.0
            ofe.process_block(buf[:16])
            assert _bits(np.float32(ofe.s.phase_accumulator)) == _bits(M.table_phase(o, M.fold(o, p + 8))), (off, p)


def _form(key, n, in_place, pos, batch=None):
    return M.expected_form(n, in_place, M.orbit(*key) is not None, pos is not None, batch)


def test_set_state_cases_take_the_form_they_claim():
    """A: the on-orbit phase and the zeros of either sign stand on the table (a zero is its entry 0) and stay on the table form; every
    other phase is off the orbit: the sequential kernel for all three blocks.  Which chain of that kernel a phase takes first
    (nco_segment_fast's guard) is stated beside it."""
    for key in M.A_SETTINGS:
        o = M.orbit_table(*key)
        neg = key[0] < 0
        for name, value in M.A_PHASES:
            ph = M.a_phase(name, value, *key)
            pos = M.set_state_pos(key[0], key[1], ph)
            want = M.TAB if name in ("on_orbit", "neg_zero", "pos_zero") else M.SEQ
            for n in M.A_BLOCKS:
                assert _form(key, n, False, pos) == want, (key, name, n)
                if pos is not None:
                    pos = M.fold(o, pos + (n & ~7))
            same_sign = not (ph > 0) if neg else not (ph < 0)
            fast_first = bool(abs(ph) < 2048.0) and bool(same_sign)
            assert fast_first == (name in ("on_orbit", "off_orbit", "neg_zero", "pos_zero") or (name, neg) in (("below_2048", False), ("minus_5", True))), (key, name)
        # the on-orbit phase: entry 1000 folded; for the negative step it is no zero (the walk to it is a real lookup)
        assert M.set_state_pos(key[0], key[1], M.a_phase("on_orbit", None, *key)) == (1000 % o[2])
    assert float(M.a_phase("on_orbit", None, -1.25e6, 8.0e6)) == -512.0
    assert float(np.float32(2047.9999)) < 2048.0 and float(np.float32(3.0e19)) >= 2.0 ** 64 and 4.0e9 < float(np.float32(5.0e9)) < 2.0 ** 64


def test_batch_cases_take_the_form_they_claim():
    """B: one member without a table, one off its orbit: the sequential kernel for all five, twice; alone again, the three that
    stand on their tables are back on the table form (their positions advanced through the batch calls)."""
    pos = [0, 0, 0, None, M.set_state_pos(*M.B_SETTINGS[4], M.B_OFF_ORBIT_PHASE)]
    assert pos[4] is None and M.orbit(*M.B_SETTINGS[3]) is None
    members = [(M.orbit(*k) is not None, p is not None) for k, p in zip(M.B_SETTINGS, pos)]
    for k, p in zip(M.B_SETTINGS, pos):
        assert _form(k, M.B_N, False, p, members) == M.SEQ
    assert [_form(k, M.B_ALONE_N, False, p) for k, p in zip(M.B_SETTINGS, pos)] == [M.TAB, M.TAB, M.TAB, M.SEQ, M.SEQ]
    assert M.expected_form(M.B_N, False, True, True, members[:3]) == M.TAB


def test_long_block_cases_take_the_form_they_claim():
    """C, D, E, F: in place stays on the table form whatever the length; out of place the speculative form starts at SPEC_MIN."""
    for key in M.C_SETTINGS:
        assert _form(key, 1000, True, 0) == M.TAB and _form(key, M.N_RAGGED, True, 0) == M.TAB
    assert M.N_RAGGED > M.SPEC_MIN and M.nseg_of(M.N_RAGGED) == 49 and ((M.N_RAGGED & ~7) - 48 * M.SEG) // 8 == 37 == 2 * 16 + 4 + 1
    assert _form(M.C_BOUNDARY_SETTING, M.SPEC_MIN - 1, False, 0) == M.TAB and _form(M.C_BOUNDARY_SETTING, M.SPEC_MIN, False, 0) == M.SPEC
    for _, key, lens in M.D_CASES:
        assert _form(key, 1000, False, 0) == M.TAB
        assert all(_form(key, n, False, 0) == M.SPEC for n in M.D_LEN[lens])
    assert {c[0] for c in M.D_CASES} == {True, False} and {c[1] for c in M.D_CASES} == set([c[1] for c in M.D_CASES][:4]) and {c[2] for c in M.D_CASES} == set(M.D_LEN)
    assert any(not i8 and key[0] < 0 for i8, key, _ in M.D_CASES)
    assert _form(M.E_SETTING, M.N_RAGGED, False, 0) == M.SPEC and _form(M.E_SETTING, M.E_N137, False, 0) == M.SPEC
    # F: a ring of 2^18 takes 2^18 samples in one staging slot, one block: speculative, written from ring position 1000 on
    assert _form((2.5e6, 10.0e6), 1 << 18, False, 0) == M.SPEC and _form((2.5e6, 10.0e6), 1000, False, 0) == M.TAB
    assert (1 << 18) - 1000 == 261144


def test_run_bounds():
    """the shapes the cases name: empty runs, a shorter last run, K = 2 and 64"""
    b = M.run_bounds(48, 32)
    assert b[:24] == [(2 * s, 2 * s + 2) for s in range(24)] and all(f >= l for f, l in b[24:])
    assert len(M.guessed_runs(48, 32)) == 14                                        # runs 10 .. 23
    b = M.run_bounds(49, 32)
    assert b[24] == (48, 49) and b[25] == (49, 49) and len(M.guessed_runs(49, 32)) == 15
    b = M.run_bounds(65, 32)
    assert b[21] == (63, 65) and b[22] == (65, 65) and sum(f < l for f, l in b) == 22
    assert [l - f for f, l in M.run_bounds(137, 32)][:28] == [5] * 27 + [2] and len(M.guessed_runs(137, 32)) == 24
    assert M.run_bounds(49, 2) == [(0, 25), (25, 49)] and M.guessed_runs(49, 2) == [1] and M.guessed_runs(137, 2) == [1]
    assert len(M.guessed_runs(49, 64)) == 30 and len(M.guessed_runs(137, 64)) == 39
    assert len(M.guessed_runs(49, 32, 1)) == 24 and len(M.guessed_runs(49, 32, M.E_W_MIX)) == 18
    for nseg in (48, 49, 65, 137):
        for K in (2, 32, 64):
            b = M.run_bounds(nseg, K)
            cover = [s for f, l in b for s in range(f, l)]
            assert cover == list(range(nseg)), (nseg, K)


def test_chain_model_is_the_oracles_dc_remover(oracle):
    """predict_standing's true chain ends on the oracle's sixteen biases (the model's arithmetic is the reference's)"""
    raw = M.wander_i8(5, 30000)
    ofe = oracle.DigitalFrontend(*M.E_SETTING, M.E_SETTING[1])
    ofe.process_block(raw.astype(np.float32))
    standing, b = M.predict_standing(raw, np.zeros(16, np.float32), 32)
    assert standing == []
    assert (_bits(b[:8]) == _bits(np.array(ofe.s.bias_re[:], np.float32))).all() and (_bits(b[8:]) == _bits(np.array(ofe.s.bias_im[:], np.float32))).all()


def test_mixed_walk_input_meets_its_condition():
    """E: with GM_FE_SPEC_WARM = E_W_MIX the model predicts between a quarter and three quarters of the guessed runs standing in each
    of the two consecutive blocks (6 and 10 of 18); none with a warm-up of 1 or 4, all with the shipped 18."""
    raw = M.wander_i8(M.E_SEED, 1000 + 2 * M.N_RAGGED)
    _, b0 = M.predict_standing(raw[:2000], np.zeros(16, np.float32), M.SPEC_K)
    counts = {}
    for w in (1, 4, M.E_W_MIX, M.SPEC_WARM):
        b, counts[w] = b0, []
        for blk in range(2):
            standing, b = M.predict_standing(raw[2000 + 2 * blk * M.N_RAGGED:2000 + 2 * (blk + 1) * M.N_RAGGED], b, M.SPEC_K, w)
            counts[w].append((sum(standing), len(standing)))
    for stand, guessed in counts[M.E_W_MIX]:
        assert guessed == 18 and guessed / 4 <= stand <= 3 * guessed / 4, counts
    assert counts[M.E_W_MIX] == [(6, 18), (10, 18)]
    assert counts[1] == [(0, 24)] * 2 and counts[4] == [(0, 22)] * 2 and counts[M.SPEC_WARM] == [(15, 15)] * 2
