"""CPU: the ring of tests/test_gpu_tracking_off_signal.py reaches what it is built to reach, on the oracle alone.

The oracle runs FREE over the ring of tests/trk_off_signal.py — in each of the three arrangements the GPU test uses — and its record
must show every argument class of atan, the crafted classes in both signs, epoch lengths that change, both signs of the DLL error, and
a lost counter that reaches MAX_LOST_EPOCHS - 1 and is followed by the reset.  Seeds and boundary starts are thereby fixed before
anything runs on a GPU.
"""
import numpy as np
import pytest

import trk_off_signal as O


def test_crafted_values_and_boundary_rates_are_what_they_claim():
    import device_math_sets as S
    vals = O.crafted_values()
    assert len(vals) == len(O.CRAFT) == len(O.CRAFT_CLASSES)
    with np.errstate(divide="ignore"):
        r = np.array([np.float32(b) / np.float32(a) for a, b in vals], np.float32)
    cls = S.atan_class(r)
    # below 2^-29 | just below / at 7/16, 11/16, 19/16, 39/16: the class changes exactly there | above 2^25 (finite and inf)
    assert cls.tolist() == [0, 1, 2, 2, 3, 3, 4, 4, 5, 6, 6], cls
    for rate in O.boundary_rates():
        near = S.from_bits((S.bits(np.float32(rate)).astype(np.int64) + np.arange(-8, 9)).astype(np.uint32))
        assert len(set(S.spc_definition_np(O.FS, near, O.L).tolist())) == 2          # a step of the epoch length within 8 ulps


@pytest.mark.parametrize("key", [O.KEY_A, O.KEY_B, None], ids=["3arms-fixed-plain", "5arms-faithful-boc", "ca-table"])
def test_oracle_alone_reaches_every_class(oracle, key):
    x = O.ring_samples()
    oring = oracle.MulticastRingBuffer(O.RING)
    oring.write_samples(x)
    mk, n_prn = O.make_oracle(oracle, key)
    records = []
    for i, d in enumerate(O.channel_table(n_prn)):
        oc = mk(i)
        O.start_oracle(oc, d)
        rec = []
        for ep in range(O.E):
            b = O.before(oc)
            rc, out, msg = oc.update_ex(oring)
            if rc:
                rec.append(dict(before=b, rc=rc, sums=np.asarray(out, np.float32)[:6].copy(), lost=msg is not None))
        assert len(rec) == O.E or i in O.WEAK, (i, len(rec))
        power = [float(r["sums"][0]) ** 2 + float(r["sums"][1]) ** 2 for r in rec]
        if i in O.CRAFT:                                                              # every epoch on a hot sample is locked
            assert min(power) > 2 * O.LOCK_THRESHOLD, (i, power)
        elif i in O.WEAK:
            assert max(power) < 0.5 * O.LOCK_THRESHOLD, (i, power)
        else:                                                                         # noise: power ~ chi^2 around 4096, P(< 15) = 0.4 %
            assert sum(p > O.LOCK_THRESHOLD for p in power) >= O.E - 1, (i, power)
        records.append(rec)
    cov = O.coverage(records)
    assert cov["unlocked"] <= 4 + sum(20 - d["lost_counter"] for d in O.channel_table(n_prn) if d["lost_counter"] is not None)
    print("off-signal ring, oracle alone:", O.summary(cov))
    O.assert_coverage(cov)
    assert cov["n_changes"] >= 12 and cov["resets_from_19"] == len(O.WEAK)            # with room for a device whose sums differ in a last bit
