"""The decision model of tests/decide_model.py against the two sequential versions the project has — the oracle's
orc_decide_from_metrics (the reference's loop in C) and gm_acq_decide_host — on every catalogue row, and the catalogue against what
it claims to hold.  No GPU: tests/test_gpu_decide_words.py holds the device forms to the same model."""
import ctypes as C

import numpy as np
import pytest

import decide_model as DM

f32 = np.float32
SIZES = (2048, 2049)
BINS = (1, 2, 41, 63, 64, 65, 127, 128, 129, 151)
FS = 2.048e6


def _dict_words(d):
    return None if d is None else DM.words(dict(d, found=1))


def _model_words(rec):
    return DM.words(rec) if rec["found"] else None


@pytest.mark.parametrize("D", BINS)
def test_model_oracle_and_decide_host_agree_on_every_row(gm, oracle, D):
    from gnss_sdr_rs_amd import distributed as Dm
    for N in SIZES:
        rows = DM.cases(N, D)
        tf = DM.table_freq(D)
        prns = [1 + p % 200 for p in range(len(rows))]
        for thr in DM.THRESHOLDS:
            for tail in DM.LOCAL_TAILS:
                host = Dm.decide_host(Dm.pack_metrics(*DM.stack(rows)), prns, tf, N, FS, local_tail=tail, threshold=thr)
                for p, (name, mx, am, sm) in enumerate(rows):
                    want = _model_words(DM.decide(mx, am, sm, tf, N, prns[p], FS, tail, DM.CA_RATE, thr))
                    orc = oracle.decide_from_metrics(mx, am, sm, tf, N, prns[p], FS, tail, thr)
                    assert _dict_words(orc) == want, (name, N, thr, tail, orc)
                    assert _dict_words(host[p]) == want, (name, N, thr, tail, host[p])


def test_decide_host_not_found_record_and_code_rate(gm):
    """What distributed.decide_host's Option hides: the not-found record is AcquisitionResult::new with doppler_bin -1, every field
    of a found one is the model's word for word at a code rate that is not the C/A one, and the zero values mean 7.0 and the C/A rate."""
    from gnss_sdr_rs_amd._lib import AcqResult, lib
    assert C.sizeof(AcqResult) == DM.RESULT_DTYPE.itemsize
    N, D = 2049, 65
    rows = DM.cases(N, D)
    P, tf = len(rows), DM.table_freq(D)
    mx, am, sm = DM.stack(rows)
    ids = np.arange(3, 3 + P, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for rate, thr, want_rate, want_thr in ((2.046e6, 2.5, 2.046e6, 2.5), (0.0, 0.0, DM.CA_RATE, 7.0), (-1.0, 7.0, DM.CA_RATE, 7.0)):
        raw = np.full(P * 48, 0xA5, np.uint8)
        found = np.full(P, 0xA5, np.uint8)
        assert lib().gm_acq_decide_host(p(mx), p(am), p(sm), p(tf), P, D, p(ids), N, FS, rate, thr, 2 ** 40, p(raw), p(found)) == 0
        assert DM.unpack(raw, found, P) == DM.expected(DM.scans(rows, N, want_thr), tf, ids, FS, 2 ** 40, want_rate)


@pytest.mark.parametrize("D", BINS)
def test_catalogue_is_what_it_claims(D):
    for N in SIZES:
        rows = DM.cases(N, D)
        assert DM.cases(N, D) is rows                                   # computed once, shared
        assert [r[0] for r in rows] == [r[0] for r in DM.cases.__wrapped__(N, D)]
        assert all((a[1].view(np.uint32) == b[1].view(np.uint32)).all() and (a[2] == b[2]).all() and (a[3].view(np.uint32) == b[3].view(np.uint32)).all()
                   for a, b in zip(rows, DM.cases.__wrapped__(N, D)))   # deterministic
        assert {DM.family_of(r[0]) for r in rows} == set(DM.families(D))
        pos = DM.positions(D)
        assert pos == sorted({b for b in (0, 1, 62, 63, 64, 65, 127, 128, D - 1) if 0 <= b < D})
        for fam in ("first_pass", "nonpos_then_pass", "nan_between", "inf_inf", "neg_inf", "sm_eq", "sm_lt", "sm_nan", "sm_inf",
                    "edge_eq", "edge_above", "mid_pass"):
            assert {int(r[0].split("@")[1]) for r in rows if DM.family_of(r[0]) == fam} == set(pos), fam
        hits = {r[0]: DM.scan(r[1], r[2], r[3], N) for r in rows}
        n_found = sum(h[0] for h in hits.values())
        assert 3 * n_found >= len(rows) and 3 * (len(rows) - n_found) >= len(rows), (n_found, len(rows))
        assert {h[3] // 64 for h in hits.values() if h[0]} == set(range((D + 63) // 64))
        for name, mx, am, sm in rows:
            fam, h = DM.family_of(name), hits[name]
            assert mx.shape == am.shape == sm.shape == (D,) and mx.dtype == f32 and am.dtype == np.uint32 and sm.dtype == f32
            b = int(name.split("@")[1].split("_")[0]) if "@" in name else None
            if fam == "first_pass":
                assert h[0] and h[3] == b and (mx[:b] < mx[b]).all() and (mx[b + 1:] > mx[b]).all(), name
                assert not any(DM.ratio(mx[d], sm[d], N) > 2.5 for d in range(b)), name
                best = DM.scan(mx, am, sm, N, best_bin=True)
                assert (best[0] == 0) if "strongest_fails" in name else (best[0] == 1 and best[3] == int(np.argmax(mx))), name
                assert best[0] == 0 or b == D - 1 or best[3] > b, name
            elif fam == "mid_pass":
                low = DM.scan(mx, am, sm, N, 2.5)
                assert low[0] and (h[3] != low[3] if b > 0 else not h[0]), name
            elif fam in ("nonpos_then_pass", "sm_eq", "edge_above"):
                assert h[0] and h[3] == b, name
            elif fam in ("sm_lt", "sm_nan", "sm_inf", "edge_eq", "inf_inf", "nonpos", "no_pass"):
                assert not h[0], name
            elif fam == "nan_between":
                assert np.isnan(mx[b]) and (h[3] == b + 1 if b + 1 < D else not h[0]), name
            elif fam == "neg_inf":
                assert mx[b] == -np.inf and (h[3] == (b + 1) % D if D > 1 else not h[0]), name
            elif fam == "argmax":
                assert h[0] and h[2] == int(name.split("/")[1]), name
            if fam == "nonpos":
                assert not (mx > 0).any(), name
            if fam == "sm_eq":
                assert sm[b] == mx[b] and DM.ratio(mx[b], sm[b], N) == np.inf
            if fam == "edge_eq":
                assert DM.ratio(mx[b], sm[b], N) == f32(7.0) and DM.scan(mx, am, sm, N, 2.5)[0]
            if fam == "edge_above":
                assert DM.ratio(mx[b], sm[b], N) > f32(7.0) and DM.ratio(np.nextafter(mx[b], f32(0)), sm[b], N) == f32(7.0)
        assert (np.diff(dict((r[0], r[1]) for r in rows)["mono_inc/none"]) > 0).all()
        assert (np.diff(dict((r[0], r[1]) for r in rows)["mono_dec/none"]) < 0).all()
        assert not hits["mono_inc/none"][0] and hits["mono_inc/pass_last"][3] == D - 1
        assert not hits["mono_dec/none"][0] and hits["mono_dec/pass_first"][3] == 0
        assert {r[0].split("/")[1] for r in rows if DM.family_of(r[0]) == "argmax"} == {"0", str(N - 1), str(2 ** 24 + 1), str(0xFFFFFFFF)}


@pytest.mark.parametrize("D", [d for d in BINS if d >= 2])
def test_a_scan_that_takes_the_later_bin_of_a_tie_is_caught(D):
    """Each tie row has two equal maxima that differ in argmax, sum and table frequency, and the deliberately wrong variant of the
    model (later_on_tie: a tie replaces the running best) decides differently on it: on the "fail" rows in both modes, on the "pass"
    rows in best-bin mode (in reference mode the sequential scan has left before it sees the later bin)."""
    N = 2048
    tf = DM.table_freq(D)
    ties = [r for r in DM.cases(N, D) if DM.family_of(r[0]).startswith("tie_")]
    kinds = {DM.family_of(r[0]) for r in ties}
    assert kinds == {f for f in DM.families(D) if f.startswith("tie_")} and len(ties) >= 2
    trips = set()
    for name, mx, am, sm in ties:
        e, l = (int(v) for v in name.split("@")[1].split("_"))
        assert e < l and mx[e] == mx[l] and (np.delete(mx, [e, l]) < mx[e]).all(), name
        assert am[e] != am[l] and sm[e] != sm[l] and tf[e] != tf[l], name
        if name.startswith("tie_trip"):
            assert e // 64 == l // 64
            trips.add(e // 64)
        if name.startswith("tie_carry"):
            assert e < 64 <= l
        for best_bin in (False, True):
            right = DM.words(DM.decide(mx, am, sm, tf, N, 9, FS, 0, DM.CA_RATE, 7.0, best_bin))
            wrong = DM.words(DM.decide(mx, am, sm, tf, N, 9, FS, 0, DM.CA_RATE, 7.0, best_bin, later_on_tie=True))
            if "/fail@" in name:
                assert right[0] == 0 and wrong[0] == 1 and wrong[8] == l, (name, best_bin)
            elif best_bin:
                assert right[0] == 1 and right[8] == e and wrong[8] == l and right[2] != wrong[2] and right[4] != wrong[4], name
            else:
                assert right[0] == 1 and right[8] == e and wrong == right, name
    assert trips == {t for t in range((D + 63) // 64) if D - 64 * t >= 2}
    if D >= 65:
        assert {tuple(int(v) for v in r[0].split("@")[1].split("_")) for r in ties if r[0].startswith("tie_63_64")} == {(63, 64)}
        assert {int(r[0].split("_")[-1]) for r in ties if r[0].startswith("tie_carry")} == {b for b in DM.positions(D) if b >= 64}


def test_best_bin_mode_on_three_hand_computed_rows():
    """Best-bin mode has no reference: the strongest bin (first strict maximum) of the whole row, tested once.  N = 2048, so a sum of
    max + 2047 a makes the average a; phase 1000 at 1.023 Mchip/s and fs = 2.046 MHz is 500 chips exactly."""
    N, fs = 2048, 2.046e6
    tf = np.array([-500.0, 0.0, 500.0], f32)
    am = np.array([1000, 7, 9], np.uint32)
    found = lambda bin_, mag, phase, tail: dict(found=1, prn=4, code_phase_samples=phase, code_phase_chips=f32(phase * 0.5),
                                                carrier_freq=tf[bin_], fs=f32(fs), mag_relative=f32(mag),
                                                sample_global_index=tail + phase, doppler_bin=bin_)
    # 1. bin 0 passes (8 / 1), the strongest bin 1 does not (16 / 4): the reference mode leaves at bin 0, best-bin finds nothing at 7.0
    mx, sm = np.array([8, 16, 4], f32), np.array([8 + 2047, 16 + 4 * 2047, 4 + 2047], f32)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 5, threshold=7.0) == found(0, 8, 1000, 5)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 5, threshold=7.0, best_bin=True) == DM.not_found(4)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 5, threshold=2.5, best_bin=True) == found(1, 16, 7, 5)
    # 2. both pass: the reference mode reports the first, best-bin the strongest
    sm = np.array([8 + 2047, 16 + 2 * 2047, 4 + 2047], f32)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 2 ** 40) == found(0, 8, 1000, 2 ** 40)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 2 ** 40, best_bin=True) == found(1, 16, 7, 2 ** 40)
    # 3. a tie for the strongest: the first of the two, whatever the later one's sum; a last bin that would pass alone changes nothing
    mx, sm = np.array([16, 16, 2], f32), np.array([16 + 2 * 2047, 16 + 8 * 2047, 2 + 2047 / 8], f32)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 0, best_bin=True) == found(0, 16, 1000, 0)
    sm = np.array([16 + 8 * 2047, 16 + 2 * 2047, 2 + 2047 / 8], f32)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 0, best_bin=True) == DM.not_found(4)
    assert DM.decide(mx, am, sm, tf, N, 4, fs, 0, best_bin=True, searched=False) == DM.not_found(4)
