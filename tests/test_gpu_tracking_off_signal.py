"""The tracking epilogue where no signal holds it still: teacher-forced against the oracle, every state word after every epoch.

Through tracking in lock the epilogue's device math sees one corner of its domain: |q / i| far below 7/16, epoch lengths that never
change, a lost counter that stays at zero.  Here 40 channels run 12 epochs over the ring of tests/trk_off_signal.py (its docstring
has the layout): unit-variance noise that LOCK_THRESHOLD = 15 takes for a signal, so that atan sees a uniformly distributed angle and
both loops integrate garbage; code rates started a few ulps from a step of round(fs / (rate / len)); noise too weak to lock, where the
lost counter runs up to the give-up reset inside a launch; and one-hot epochs whose prompt sums put q / i below 2^-29, one ulp below
and exactly at 7/16, 11/16, 19/16 and 39/16, above 2^25 and at i = 0 exactly, in both signs.  (0 / 0 is left out: a locked epoch has
power > 15, so it cannot occur in one, and no NaN state is constructed on the device.)

THE STATE is the subject.  The oracle advances with the DEVICE's sums (orc_trk_update_forced), so both sides enter every epoch with
the same state, and after every launch every state word must be equal bit for bit — prn, active, lost_counter, next_sample_index,
num_samples_per_code and the ten floats as bit patterns — as must the `processed` and `lost` flags of every epoch.  Each case runs
once as one multi-epoch launch and once as one epoch per launch (states compared after every epoch), to localise a difference.

THE SUMS are random here, so they are not held to the prompt envelope (the tight bars stay where signals are) but to a worst-case bound
against the oracle's f64 accumulation of its own f32 products, relative to A = sum over the epoch of |Re x| + |Im x|:

    |S_device - S_f64| <= (gamma_n + tau) * A,    gamma_n = n u / (1 - n u),  u = 2^-24,  tau = 6.6 u.

gamma_n bounds the rounding of ANY order of n - 1 f32 additions of the device's products, whose magnitudes sum to at most A (a
product is |x_r c -+ x_i s| <= |x_r| + |x_i| up to roundings that the slack of tau covers).  tau bounds the difference between a
device product and the oracle's product of the same sample and the same f32 phase: the two cosines (and sines) differ by at most
1.6 u (the device's forms, measured against float64 in tests/test_gpu_device_math.py) + 1.0 u (glibc's, < 1 ulp) = 2.6 u, which
moves the product by 2.6 u (|x_r| + |x_i|); and each side rounds two products and one difference, 2 u (|x_r| + |x_i|) per side.
At n = 4097 the bound is 2.4e-4 A.  The worst fraction of it is printed.  On the serial strict_libm + strict_sum_order path the sums
must be the oracle's own bits, which makes the teacher-forced run a free-running one.

Coverage is asserted from the oracle's record alone (trk_off_signal.coverage), as tests/test_tracking_off_signal_host.py asserts it
for the oracle running free.
"""
import numpy as np
import pytest

import trk_off_signal as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TAU = 6.6 * U
FLOATS = ("carrier_freq", "carrier_phase", "carrier_error", "carrier_nco", "code_phase", "code_error", "code_nco", "code_rate",
          "i_prompt", "q_prompt")


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _assert_states_equal(states, ocs, where):
    for i, (s, oc) in enumerate(zip(states, ocs)):
        o = oc.c
        assert (s.prn, bool(s.active), s.lost_counter, s.next_sample_index, s.num_samples_per_code) == \
               (o.prn, oc.is_active(), o.lost_counter, o.next_sample_index, o.num_samples_per_code), (where, i)
        for k in FLOATS:
            assert _bits(getattr(s, k)) == _bits(getattr(o, k)), (where, i, k, float(getattr(s, k)).hex(), float(getattr(o, k)).hex())


class _Case:
    def __init__(self, oracle, key):
        from gnss_sdr_rs_amd import tracking as T
        self.x = O.ring_samples()
        self.cum = np.concatenate([[0.0], np.cumsum(np.abs(self.x.real.astype(np.float64)) + np.abs(self.x.imag.astype(np.float64)))])
        self.ring, self.oring = T.MulticastRingBuffer(O.RING), oracle.MulticastRingBuffer(O.RING)
        self.ring.write_samples(self.x)
        self.oring.write_samples(self.x)
        mk, n_prn = O.make_oracle(oracle, key)
        self.table = O.channel_table(n_prn)
        self.ocs = [mk(i) for i in range(O.C)]
        self.records = [[] for _ in range(O.C)]
        self.worst = 0.0
        self.nv = 6 if key is None else 2 * key[0]

    def start(self, mgr):
        for i, d in enumerate(self.table):
            O.start_device(mgr.channels[i], d)
            O.start_oracle(self.ocs[i], d)
        _assert_states_equal(mgr.get_states(), self.ocs, "start")

    def replay(self, i, ep, sums, processed, lost, bit_equal_sums=False):
        """one epoch of channel i through the oracle, forced with the device's sums; the flags and the sum bound"""
        oc = self.ocs[i]
        b = O.before(oc)
        start = int(oc.c.next_sample_index)
        rc, comp, comp64, msg = oc.update_forced(self.oring, sums)
        assert (rc != 0) == bool(processed), ("processed", i, ep, rc)
        assert bool(lost) == (msg is not None), ("lost", i, ep, msg)
        if not rc:
            return
        n = b["n"]
        A = self.cum[start + n] - self.cum[start]
        gamma = n * U / (1.0 - n * U)
        frac = float(np.max(np.abs(np.asarray(sums[:self.nv], np.float64) - comp64[:self.nv]))) / ((gamma + TAU) * A)
        self.worst = max(self.worst, frac)
        assert frac <= 1.0, ("sum bound", i, ep, frac)
        if bit_equal_sums:
            got, want = np.ascontiguousarray(sums[:self.nv], np.float32), np.ascontiguousarray(comp[:self.nv], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("sums", i, ep, got, want)
        self.records[i].append(dict(before=b, rc=rc, sums=np.asarray(sums, np.float32)[:6].copy(), lost=msg is not None))

    def finish(self, name):
        cov = O.coverage(self.records)
        print("off-signal %s: worst fraction of the sum bound %.3g; %s" % (name, self.worst, O.summary(cov)))
        O.assert_coverage(cov)
        self.ring.close()


def _run_update_all(oracle, key, form, strict_libm=False, strict_sum_order=False):
    from gnss_sdr_rs_amd import tracking as T
    arms, mode, boc = key
    case = _Case(oracle, key)
    mgr = T.TrackingManager(O.FS, n_channels=O.C, n_arms=arms, code_index_mode=mode, early_late_space=O.EL, very_early_late_space=O.VEL,
                            boc11=boc, codes=O.codes_for(key), nominal_code_rate=O.RATE, strict_libm=strict_libm,
                            strict_sum_order=strict_sum_order)
    case.start(mgr)
    launches = [O.E] if form == "one-launch" else [1] * O.E
    ep0 = 0
    for epochs in launches:
        outs, proc, lost, done = mgr.update_all(case.ring, epochs)
        assert done == epochs
        for ep in range(epochs):
            for i in range(O.C):
                case.replay(i, ep0 + ep, outs[ep, i], proc[ep, i], lost[ep, i], bit_equal_sums=strict_sum_order)
        ep0 += epochs
        _assert_states_equal(mgr.get_states(), case.ocs, "after epoch %d" % (ep0 - 1))
    case.finish("%s %s%s%s" % (key, form, " strict_libm" if strict_libm else "", " strict_sum_order" if strict_sum_order else ""))
    mgr.close()


KEYS = [O.KEY_A, O.KEY_B]
KEY_IDS = ["3arms-fixed-plain", "5arms-faithful-boc"]
FORMS = ["one-launch", "epoch-per-launch"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_persistent_default(gpu, oracle, key, form):
    _run_update_all(oracle, key, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_persistent_strict_libm(gpu, oracle, key, form):
    _run_update_all(oracle, key, form, strict_libm=True)


@pytest.mark.parametrize("form", FORMS)
def test_serial_strict_libm_and_sum_order(gpu, oracle, form):
    """launch_trk_epoch's serial path: every sum is the oracle's own bits as well, so the run is a free-running one."""
    _run_update_all(oracle, O.KEY_A, form, strict_libm=True, strict_sum_order=True)


def test_do_work_on_host_samples(gpu, oracle):
    """trk_update_kernel through the unit entry: the caller hands over each epoch's samples (three arms, the built-in C/A table, FIXED);
    the epoch length the next call needs is the one this call's epilogue stored."""
    from gnss_sdr_rs_amd import tracking as T
    case = _Case(oracle, None)
    mgr = T.TrackingManager(O.FS, n_channels=O.C, code_index_mode=1)
    case.start(mgr)
    for ep in range(O.E):
        states = mgr.get_states()
        for i in range(O.C):
            oc = case.ocs[i]
            if not states[i].active:
                assert not oc.is_active()
                continue
            at, n = int(states[i].next_sample_index), int(states[i].num_samples_per_code)
            sums, msg = mgr.channels[i].do_work(case.x[at:at + n])
            case.replay(i, ep, np.asarray(sums, np.float32), 1, msg is not None)
        _assert_states_equal(mgr.get_states(), case.ocs, "after epoch %d" % ep)
    case.finish("do_work on host samples")
    mgr.close()
