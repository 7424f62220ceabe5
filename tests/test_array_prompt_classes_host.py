"""The case list of tests/test_gpu_array_prompt_classes.py against the library's own rules (CPU; both plan entries are host only).

1. PAIRS is exactly what gm_acq_array_plan and gm_trk_array_plan accept over (A, L) in 0 .. 10 squared: if a limit moves, the GPU sweep
   has to follow it instead of silently covering less.
2. PAIRS x {c32, i8} x {aligned, one element off} launches every kernel class the two files build (26 a format, the table below) and
   every load form (22, the table below), and every class with LC >= 4 both at an L below LC and at L = LC (A = 6's class 5 holds L = 5 alone: there is no L below it to run).
3. The sweep's integer cases are exact on the worst case, not on a seed: N (128 + 128) terms' worth stays below 2^24 / 1.5."""
import pytest

import array_prompt_classes as AC

# the tap classes of every antenna count (csrc/acq_array.hip, csrc/trk_array.hip: LC = 1, 2, 4 and the most taps A allows)
CLASSES = {2: (1, 2, 4, 8), 3: (1, 2, 4, 8), 4: (1, 2, 4, 8), 5: (1, 2, 4, 6), 6: (1, 2, 4, 5), 7: (1, 2, 4), 8: (1, 2, 4)}
# the load of one time sample where the period's first byte allows the wide form; each even A has the element form beside it
WIDE = {("c32", 2): "wide16", ("c32", 4): "wide16", ("c32", 6): "wide16", ("c32", 8): "wide16",
        ("i8", 2): "wide4x1", ("i8", 4): "wide8", ("i8", 6): "wide4x3", ("i8", 8): "wide16"}


def _accepted(call):
    from gnss_sdr_rs_amd import _lib
    got = []
    for A in range(0, 11):
        for L in range(0, 11):
            try:
                call(A, L)
                got.append((A, L))
            except _lib.GmError:
                pass
    return got


def test_pairs_are_what_both_plan_entries_accept(gm):
    from gnss_sdr_rs_amd import acquisition, tracking
    assert len(AC.PAIRS) == len(set(AC.PAIRS)) == 43 == 8 + 8 + 8 + 6 + 5 + 4 + 4
    assert _accepted(lambda A, L: acquisition.array_plan(1, 1, A, L)) == AC.PAIRS
    assert _accepted(lambda A, L: tracking.array_plan(4097.0e3, A, L)) == AC.PAIRS
    # the words a pair gives, so that an accepted pair is also the pair that was asked for
    for A, L in AC.PAIRS:
        assert acquisition.array_plan(1, 3, A, L) == dict(periods=3, words_per_cand=3 * A * L)
        assert tracking.array_plan(4097.0e3, A, L) == dict(words_per_record=A * L, out_words=A * L, samples=4097, slices=2)


def test_the_sweep_launches_every_class_and_every_load_form():
    assert sum(len(v) for v in CLASSES.values()) == 26
    for A, classes in CLASSES.items():
        assert classes[-1] == max(c for c in (1, 2, 4, min(8, 32 // A)))
        assert max(L for a, L in AC.PAIRS if a == A) == classes[-1]           # the widest class is the most taps A allows
    want_classes = {(fmt, A, LC) for fmt in AC.FORMATS for A, cs in CLASSES.items() for LC in cs}
    want_forms = {(fmt, A, "element") for fmt in AC.FORMATS for A in CLASSES} | {(fmt, A, form) for (fmt, A), form in WIDE.items()}
    assert len(want_classes) == 52 and len(want_forms) == 22
    runs = AC.launches()
    assert len(runs) == 43 * 4
    assert {(fmt, A, AC.tap_class(A, L)) for fmt, A, L, _ in runs} == want_classes
    assert {(fmt, A, AC.load_form(fmt, A, al)) for fmt, A, L, al in runs} == want_forms
    # every class runs on both of its load forms, and every (A, L) does
    for fmt, A, LC in want_classes:
        forms = {AC.load_form(fmt, A, al) for f, a, L, al in runs if (f, a) == (fmt, A) and AC.tap_class(a, L) == LC}
        assert forms == {form for f, a, form in want_forms if (f, a) == (fmt, A)}, (fmt, A, LC)
    # a pointer one element off is no multiple of V exactly where a wide form exists
    for fmt in AC.FORMATS:
        for A in CLASSES:
            assert AC.one_element_off_is_narrow(fmt, A) == ((fmt, A) in WIDE) == (AC.load_form(fmt, A, True) != "element")
    # the tap loop's uniform test: L below its class and L = the class itself
    for A, classes in CLASSES.items():
        for LC in classes:
            Ls = [L for a, L in AC.PAIRS if a == A and AC.tap_class(a, L) == LC]
            assert LC in Ls and max(Ls) == LC, (A, LC)
            if LC >= 4 and (A, LC) != (6, 5):                                 # A = 6: L = 5 is the whole class, 4 belongs to class 4
                assert min(Ls) < LC, (A, LC)
    assert [L for a, L in AC.PAIRS if a == 5 and AC.tap_class(a, L) == 6] == [5, 6]
    assert [L for a, L in AC.PAIRS if a == 6 and AC.tap_class(a, L) == 5] == [5]      # (A = 6 allows no L between 4 and its class)


def test_tap_class_and_load_form_at_known_points():
    assert [AC.tap_class(2, L) for L in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    assert [AC.tap_class(5, L) for L in range(1, 7)] == [1, 2, 4, 4, 6, 6] and AC.tap_class(6, 5) == 5 and AC.tap_class(8, 4) == 4
    with pytest.raises(AssertionError):
        AC.tap_class(8, 5)
    assert [AC.widest(t) for t in (4, 6, 8, 12, 16, 24, 40, 48, 56, 64)] == [4, 2, 8, 4, 16, 8, 8, 16, 8, 16]
    assert AC.load_form("c32", 6, True) == "wide16" and AC.load_form("c32", 6, False) == "element" and AC.load_form("c32", 5, True) == "element"
    assert AC.load_form("i8", 6, True) == "wide4x3" and AC.load_form("i8", 7, True) == "element" and AC.load_form("i8", 4, False) == "element"


def test_integer_sums_are_exact_on_the_worst_case():
    """every term of a sum has |re| and |im| of at most 128 + 128 (an int8 IQ sample times +-1, or times 1 + 0j), so every partial sum of
    N of them, in any order, is an integer below 2^24 and exact in float32"""
    assert AC.TERM_MAX == 256 and AC.EXACT_BOUND == 2.0 ** 24 / 1.5
    assert AC.EXACT_TERMS["acq"] * AC.TERM_MAX == 524288 and AC.EXACT_TERMS["trk"] * AC.TERM_MAX == 1048832
    for n in AC.EXACT_TERMS.values():
        assert n * AC.TERM_MAX < AC.EXACT_BOUND < 2.0 ** 24
