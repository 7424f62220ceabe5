"""GPU: the plane ring (gm_plane_ring) and tracking on planes (gm_trk_update_planes), channel c on plane planes[c].

YARDSTICK.  The oracle's tracking channel, used exactly as test_gpu_tracking_shapes._compare uses it, with ONE ORACLE RING PER PLANE:
update_forced is the teacher-forced form (the oracle forms each epoch's sums from its own state, they are compared, and it then advances
with the DEVICE's sums, so both sides enter every epoch with the same state), update_ex the free-running one.  The bars are that file's
own, imported from it: REL = 1e-5 of the prompt envelope, F64_REL = 5e-7 against the f64 accumulation of the same f32 products,
FREE_REL = 2.5e-5 free-running, every word of the final state at 0 ulps after teacher forcing; env > 100 wherever a ratio is taken.

SCENES.  Each plane gets a scene of its own from synth.tracking_scene with its own config_id, and each PRN is present in one plane only:
a channel that reads the wrong plane correlates against noise and misses env > 100 and the bar.  (The 4092-chip BOC(1,1) case has no
generator in synth: test_gpu_tracking_shapes._boc_scene with a seed per plane and a code row per plane.  The epochs of 2047 and 2049
samples are scenes generated at 2.047 and 2.049 Msps, read by a handle at fs = 2.048 MHz whose code_rate is 1.0235e6 / 1.0225e6: the
same chips per sample to 3e-7, so that the replica stays on the code.)

Not tested: a ring on another device (one device here), and what the header says the library does not order.  Every case prints the
largest fraction of each bar it saw."""
import ctypes as C

import numpy as np
import pytest

import stream_stall as SS            # (imports torch before the HIP library)
import trk_form_classes as FC
from test_gpu_tracking_shapes import F64_REL, FREE_REL, REL, _acq_result, _boc_scene, _ulps

pytestmark = pytest.mark.gpu

FS = 2.048e6
MAP = [2, 0, 2, 1, 0]                # P = 3 planes, C = 5 channels: two pairs share a plane, no channel sits at identity
PLANE_PRNS = [[5, 13], [9], [2, 22]]  # the PRNs of plane p
CH_PRN = [2, 5, 22, 9, 13]           # channel c tracks CH_PRN[c], which is in plane MAP[c] and nowhere else
STATE_WORDS = ("carrier_freq", "carrier_phase", "carrier_error", "carrier_nco", "code_phase", "code_error", "code_nco", "code_rate")
_cache = {}


def _plane_scenes(oracle, fs_scene, mode, n_ms, base_id, rows_custom=False):
    """-> (x complex64 [3, n_ms * N], {prn: sat}) : plane p = synth.tracking_scene(config_id = base_id + p) of PLANE_PRNS[p]"""
    key = (fs_scene, mode, n_ms, base_id, rows_custom)
    if key not in _cache:
        from gnss_sdr_rs_amd import synth
        t = oracle.ca_code_table()
        xs, by_prn = [], {}
        for p, prns in enumerate(PLANE_PRNS):
            # FAITHFUL indexes GPS_CA_CODE_32_PRN[prn] (do_tracking.rs:276): the air then carries row prn; a custom table is read at prn - 1
            rows = [q if (mode == 0 and not rows_custom) else q - 1 for q in prns]
            sc = synth.tracking_scene(t, fs_scene, 0.0, prns, n_ms, config_id=base_id + p, cn0=50.0, code_rows=rows)
            xs.append(synth.to_c32(sc["x"]))
            for s in sc["sats"]:
                by_prn[s["prn"]] = s
        _cache[key] = (np.ascontiguousarray(np.stack(xs)), by_prn)
    return _cache[key]


def _starts(by_prn, fs, scale=1.0, prns=CH_PRN):
    return [_acq_result(q, by_prn[q]["doppler_hz"] * scale + 20.0 - 3.0 * i, fs, by_prn[q]["code_start"]) for i, q in enumerate(prns)]


class Twin:
    """The channels of a handle and their two oracle twins (teacher-forced, free-running), one oracle ring per plane."""

    def __init__(self, mgr, orings, plane_of, starts, make_oracle, arms, rel=REL, free_rel=FREE_REL):
        self.mgr, self.orings, self.plane_of, self.arms, self.rel, self.free_rel = mgr, orings, plane_of, arms, rel, free_rel
        self.forced, self.free = [], []
        for i, r in enumerate(starts):
            if r is not None:                       # None: the channel is never started (inactive)
                mgr.channels[i].start(r)
            for lst in (self.forced, self.free):
                oc = make_oracle(i)
                if r is not None:
                    oc.start(r)
                lst.append(oc)
        self.worst = dict(forced=0.0, free=0.0, f64=0.0, ulps=0, ref=0.0)      # ref: the oracle's f32 sums against its own f64 accumulation
        self.ran = [0] * len(starts)

    def step(self, result):
        """replay the passes of one update_planes call; -> the oracle's epochs_done"""
        outs, proc, lost, done = result
        nv, want_done = 2 * self.arms, 0
        for i in range(len(self.forced)):
            oring = self.orings[self.plane_of[i]]
            for ep in range(outs.shape[0]):
                rc_f, comp, comp64, _ = self.forced[i].update_forced(oring, outs[ep, i])
                rc_r, exp, _ = self.free[i].update_ex(oring)
                assert (rc_f != 0) == bool(proc[ep, i]) == (rc_r != 0), (i, ep, rc_f, proc[ep, i], rc_r)
                assert not lost[ep, i], (i, ep)
                if not rc_f:
                    assert not outs[ep, i].any(), (i, ep)      # an unprocessed pass is zeros
                    continue
                want_done = max(want_done, ep + 1)
                self.ran[i] += 1
                env = float(np.hypot(comp[0], comp[1]))
                assert env > 100.0, (i, ep, env)                      # a signal is under the correlator
                e1 = float(np.max(np.abs(outs[ep, i] - comp[:nv]))) / env
                env_r = float(np.hypot(exp[0], exp[1]))
                assert env_r > 100.0, (i, ep, env_r)
                e2 = float(np.max(np.abs(outs[ep, i] - exp[:nv]))) / env_r
                e64 = float(np.max(np.abs(outs[ep, i] - comp64[:nv]))) / env
                w = self.worst
                w["forced"], w["free"], w["f64"] = max(w["forced"], e1), max(w["free"], e2), max(w["f64"], e64)
                w["ref"] = max(w["ref"], float(np.max(np.abs(comp[:nv] - comp64[:nv]))) / env)
                assert e1 <= self.rel, ("teacher-forced", i, ep, e1)
                assert e64 <= F64_REL, ("teacher-forced vs f64 accumulation", i, ep, e64)
                assert e2 <= self.free_rel, ("free-running", i, ep, e2)
        assert done == want_done, (done, want_done)
        return want_done

    def check_states(self):
        for i in range(len(self.forced)):
            s, o = self.mgr.channels[i].state, self.forced[i].c
            assert s.next_sample_index == o.next_sample_index == self.free[i].c.next_sample_index, i
            assert s.num_samples_per_code == o.num_samples_per_code, i
            assert s.lost_counter == o.lost_counter == 0 and s.prn == o.prn and bool(s.active) == self.forced[i].is_active(), i
            assert s.i_prompt == o.i_prompt and s.q_prompt == o.q_prompt, i
            for k in STATE_WORDS:
                u = _ulps(getattr(s, k), getattr(o, k))
                self.worst["ulps"] = max(self.worst["ulps"], u)
                assert u == 0, (i, k, getattr(s, k), getattr(o, k))
        return self.worst


def _fractions(tag, w):
    print("%s: largest fraction of each bar: teacher-forced %.3f (%.2e / %.0e), f64 %.3f (%.2e / %.0e), free-running %.3f (%.2e / %.1e), "
          "state %d ulps; reference's own f32-against-f64 %.2e" % (tag, w["forced"] / REL, w["forced"], REL, w["f64"] / F64_REL, w["f64"], F64_REL,
                                                                    w["free"] / FREE_REL, w["free"], FREE_REL, w["ulps"], w["ref"]))


def _rings(oracle, x, plane_size):
    """a PlaneRing holding x [P, n] and one oracle ring per plane holding the same words"""
    from gnss_sdr_rs_amd import tracking as T
    pr = T.PlaneRing(x.shape[0], plane_size)
    pr.write(x)
    orings = []
    for p in range(x.shape[0]):
        o = oracle.MulticastRingBuffer(plane_size)
        o.write_samples(x[p])
        orings.append(o)
    return pr, orings


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    dict(id="n2048-fixed", n=2048, mode=1), dict(id="n2048-faithful", n=2048, mode=0), dict(id="n2048-fixed-strict-libm", n=2048, mode=1, strict=True),
    dict(id="n2047-code-rate", n=2047, mode=1, rate=1.0235e6), dict(id="n2049-code-rate-faithful", n=2049, mode=0, rate=1.0225e6),
    dict(id="n5000", n=5000, mode=1, fs=5.0e6), dict(id="n5000-faithful-strict-libm", n=5000, mode=0, fs=5.0e6, strict=True),
]


@pytest.mark.parametrize("case", SHAPES, ids=[c["id"] for c in SHAPES])
def test_shapes_on_three_planes(gpu, oracle, case):
    """P = 3 planes, C = 5 channels behind the map [2, 0, 2, 1, 0], a sixth channel inactive, 12 epochs in one call"""
    from gnss_sdr_rs_amd import tracking as T
    n, mode, E = case["n"], case["mode"], 12
    fs = case.get("fs", FS)
    rate = case.get("rate")
    fs_scene = n * 1000.0                             # the scene's samples per code period are the handle's n
    x, by_prn = _plane_scenes(oracle, fs_scene, mode, E + 2, 300 + (n % 100) * 3 + mode * 40, rows_custom=rate is not None)
    x = x[:, :(E + 1) * n]
    pr, orings = _rings(oracle, x, 1 << 17)
    kw, okw = {}, {}
    if rate is not None:                              # a custom table (the C/A rows) so that handle and oracle take the code rate
        codes = oracle.ca_code_table().astype(np.int8)
        kw, okw = dict(codes=codes, nominal_code_rate=rate), dict(codes=codes, code_rate=rate)
    mgr = T.TrackingManager(fs, n_channels=6, code_index_mode=mode, strict_libm=bool(case.get("strict")), **kw)
    mgr.set_channel_planes(MAP + [1])
    assert mgr.channel_planes() == MAP + [1]
    tw = Twin(mgr, orings, MAP + [1], _starts(by_prn, fs, fs / fs_scene) + [None], lambda i: oracle.TrackingChannel(i, fs, code_index_mode=mode, **okw), 3)
    idle = bytes(mgr.channels[5].state)
    assert tw.step(mgr.update_planes(pr, E)) == E
    w = tw.check_states()
    assert tw.ran == [E] * 5 + [0] and bytes(mgr.channels[5].state) == idle
    assert int(mgr.channels[0].state.num_samples_per_code) == n
    _fractions(case["id"], w)
    mgr.close(); pr.close()


@pytest.mark.parametrize("mode", [1, 0])
def test_boc_4092_chips_five_arms(gpu, oracle, mode):
    """a custom 4092-chip code, BOC(1,1), five arms, n = 16368: every plane its own noise and its own code rows.
    The scene's seed.  At n = 16368 the yardstick's own error is no longer small beside REL: the oracle's sequential f32 sums, held against
    its own f64 accumulation of the same products on the CPU (no device involved), miss it by up to 0.9e-5 .. 2.4e-5 of the envelope for
    most seeds of this recipe (seeds 91 .. 111; the additions of near-equal terms round the same way for long runs, so the error has a
    long tail: rms 1.2e-6).  Seed 112 is one whose oracle-alone figure is 4.7e-6 in both modes, so that REL = 1e-5 measures the kernel
    and not the yardstick; the figure the run itself sees is printed as "reference's own"."""
    from gnss_sdr_rs_amd import tracking as T
    fs, L, rate, E = 4.092e6, 4092, 1.023e6, 12
    n = int(round(fs / (rate / L)))
    assert n == 16368
    rng = np.random.default_rng(112)
    codes = np.where(rng.integers(0, 2, (5, L)) > 0, 1, -1).astype(np.int8)      # row c is channel c's code (prn c + 1)
    dopp, cstart = rng.uniform(-2000, 2000, 5), rng.integers(0, 4000, 5)
    planes = []
    for p in range(3):
        mine = [c for c in range(5) if MAP[c] == p]
        planes.append(_boc_scene(codes[mine], fs, rate, L, (E + 1) * n, dopp[mine], cstart[mine], seed=113 + p))
    x = np.ascontiguousarray(np.stack(planes))
    pr, orings = _rings(oracle, x, 1 << 18)
    kw = dict(n_arms=5, early_late_space=0.25, very_early_late_space=0.6, boc11=True, codes=codes)
    mgr = T.TrackingManager(fs, n_channels=6, code_index_mode=mode, nominal_code_rate=rate, **kw)
    mgr.set_channel_planes(MAP + [0])
    starts = [_acq_result(c + 1, float(dopp[c]) + 10.0, fs, int(cstart[c])) for c in range(5)] + [None]

    def mk(i):
        return oracle.TrackingChannel(i, fs, code_index_mode=mode, n_arms=5, el_space=0.25, vel_space=0.6, boc11=True, codes=codes, code_rate=rate)
    tw = Twin(mgr, orings, MAP + [0], starts, mk, 5)
    assert tw.step(mgr.update_planes(pr, E)) == E
    _fractions("boc-4092-five-arms mode %d" % mode, tw.check_states())
    assert tw.ran == [E] * 5 + [0]
    mgr.close(); pr.close()


# ---- the ring's edges -------------------------------------------------------------------------------------------------------------------
def test_ring_edges_chunked_device_writes_and_epochs_across_the_wrap(gpu, oracle, hipbuf):
    """plane_size 2^14, 20 periods in chunks of 4096 and 3001 from device buffers whose in_stride exceeds n: the chunk from 14194 (even, the
    16-byte form) and the chunk from 32484 (odd count, the 8-byte form) straddle the wrap.  After every chunk the new words are read back
    with copy_to_slice, the tracker runs what the head allows, and the oracle (rings of the same size, the same chunks) replays it."""
    from gnss_sdr_rs_amd import tracking as T
    n, size, total = 2048, 1 << 14, 20 * 2048
    x, by_prn = _plane_scenes(oracle, FS, 1, 22, 400)
    x = x[:, :total]
    pr, host_pr = T.PlaneRing(3, size), T.PlaneRing(3, size)
    orings = [oracle.MulticastRingBuffer(size) for _ in range(3)]
    mgr = T.TrackingManager(FS, n_channels=5, code_index_mode=1)
    mgr.set_channel_planes(MAP)
    tw = Twin(mgr, orings, MAP, _starts(by_prn, FS), lambda i: oracle.TrackingChannel(i, FS, code_index_mode=1), 3)
    pos, k, straddled, passes = 0, 0, [], 0
    while pos < total:
        cnt = min(4096 if k % 2 == 0 else 3001, total - pos)
        stride = cnt + 8 + (1 if k % 4 == 2 else 0)                  # in_stride > n, odd and even (even where the 16-byte form is due)
        block = np.full((3, stride), 7 + 7j, np.complex64)
        block[:, :cnt] = x[:, pos:pos + cnt]
        pr.write_dev(hipbuf.upload(block), stride, cnt)
        host_pr.write(x[:, pos:pos + cnt])
        for p in range(3):
            orings[p].write_samples(x[p, pos:pos + cnt])
            assert np.array_equal(pr.copy_to_slice(p, pos, cnt).view(np.uint32), x[p, pos:pos + cnt].view(np.uint32)), (k, p)
        if (pos % size) + cnt > size:
            straddled.append((pos, cnt))
        pos += cnt
        k += 1
        assert pr.get_head() == host_pr.get_head() == pos
        passes += tw.step(mgr.update_planes(pr, 3))
    assert [c % 2 for _, c in straddled] == [0, 1], straddled          # both copy forms crossed the wrap
    for p in range(3):                                                 # the host write leaves the same ring words, and the last 2^14 samples are there
        a, b = pr.copy_to_slice(p, 0, size), host_pr.copy_to_slice(p, 0, size)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), p
        assert np.array_equal(pr.copy_to_slice(p, total - size, size).view(np.uint32), x[p, total - size:].view(np.uint32)), p
    w = tw.check_states()
    assert min(tw.ran) >= 18 and passes >= 18, tw.ran                  # the epochs that straddle 16384 and 32768 are among them
    for i in range(5):
        s0 = tw.forced[i].c.next_sample_index - tw.ran[i] * n
        assert any(s0 + e * n < size < s0 + (e + 1) * n for e in range(tw.ran[i])), i
    _fractions("ring edges", w)
    mgr.close(); pr.close(); host_pr.close()


# ---- independence -----------------------------------------------------------------------------------------------------------------------
def _run(mgr, pr, starts, E, cuts=None):
    """start the channels, run E passes (in calls of `cuts`), -> (outs [E, C, nv] as words, the states as bytes)"""
    for i, r in enumerate(starts):
        if r is not None:
            mgr.channels[i].start(r)
    outs = []
    for e in (cuts or [E]):
        o, proc, lost, done = mgr.update_planes(pr, e)
        assert proc[:, [i for i, r in enumerate(starts) if r is not None]].all() and not lost.any() and done == e
        outs.append(o)
    return np.concatenate(outs).view(np.uint32), [bytes(s) for s in mgr.get_states()]


def test_a_channels_words_depend_on_its_state_and_plane_alone(gpu, oracle):
    from gnss_sdr_rs_amd import tracking as T
    n, E = 2048, 8
    x, by_prn = _plane_scenes(oracle, FS, 1, 14, 300 + 48 * 3 + 40)
    x = x[:, :(E + 1) * n]
    starts = _starts(by_prn, FS)
    pr = T.PlaneRing(3, 1 << 15)
    pr.write(x)

    def fresh(n_channels=5, planes=MAP):
        m = T.TrackingManager(FS, n_channels=n_channels, code_index_mode=1)
        m.set_channel_planes(planes)
        return m
    mgr = fresh()
    start_states = None
    want_o, want_s = _run(mgr, pr, starts, E)
    # (1) E epochs in one call = E calls of one epoch = a cut 3 + 5; (2) a second run from set_states of the start
    for cuts in ([1] * E, [3, 5]):
        m = fresh()
        o, s = _run(m, pr, starts, E, cuts)
        assert np.array_equal(o, want_o) and s == want_s, cuts
        m.close()
    m = fresh()
    for i, r in enumerate(starts):
        m.channels[i].start(r)
    start_states = m.get_states()
    first = m.update_planes(pr, E)[0].view(np.uint32)
    m.set_states(start_states)
    again = m.update_planes(pr, E)[0].view(np.uint32)
    assert np.array_equal(first, want_o) and np.array_equal(again, want_o)
    assert [bytes(s) for s in m.get_states()] == want_s
    m.close()
    # (3) a channel alone = the same channel among four others
    for c in range(5):
        m = fresh(1, [MAP[c]])
        o, s = _run(m, pr, [starts[c]], E)
        assert np.array_equal(o[:, 0], want_o[:, c]) and s[0] == want_s[c], c
        m.close()
    # (4) the same scenes behind a permuted map, in a ring of 5 planes (planes 1 and 3 hold other words), channels in another order
    perm = [4, 2, 0]                                   # scene plane p lives in ring plane perm[p]
    x5 = np.zeros((5, x.shape[1]), np.complex64)
    x5[1], x5[3] = x[0][::-1], x[2][::-1]
    for p in range(3):
        x5[perm[p]] = x[p]
    pr5 = T.PlaneRing(5, 1 << 16)                      # another plane size: the epochs lie elsewhere in the ring
    lead = 4096                                        # ... and at other ring positions: 4096 samples in front, the starts moved with them
    pr5.write(np.zeros((5, lead), np.complex64))
    pr5.write(x5)
    order = [3, 0, 4, 1, 2]
    m = fresh(5, [perm[MAP[c]] for c in order])
    moved = [dict(starts[c], sample_global_index=starts[c]["sample_global_index"] + lead) for c in order]
    o, s = _run(m, pr5, moved, E)
    for j, c in enumerate(order):
        assert np.array_equal(o[:, j], want_o[:, c]), (j, c)
        a, b = m.channels[j].state, mgr.channels[c].state
        assert a.next_sample_index == b.next_sample_index + lead
        for k in STATE_WORDS + ("i_prompt", "q_prompt"):
            assert _ulps(getattr(a, k), getattr(b, k)) == 0, (j, c, k)
    m.close(); mgr.close(); pr.close(); pr5.close()


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def test_the_gate_is_on_the_enqueued_head(gpu, oracle):
    from gnss_sdr_rs_amd import tracking as T
    n = 2048
    x, by_prn = _plane_scenes(oracle, FS, 1, 14, 300 + 48 * 3 + 40)
    starts = _starts(by_prn, FS)
    late = int(np.argmax([r["sample_global_index"] for r in starts]))
    head = starts[late]["sample_global_index"] + n - 1            # one sample short of the latest channel's first period
    assert all(r["sample_global_index"] + n <= head for i, r in enumerate(starts) if i != late)
    size = 1 << 15
    pr = T.PlaneRing(3, size)
    orings = [oracle.MulticastRingBuffer(size) for _ in range(3)]
    mgr = T.TrackingManager(FS, n_channels=5, code_index_mode=1)
    mgr.set_channel_planes(MAP)
    tw = Twin(mgr, orings, MAP, starts, lambda i: oracle.TrackingChannel(i, FS, code_index_mode=1), 3)
    before = bytes(mgr.channels[late].state)

    def feed(a, b):
        pr.write(x[:, a:b])
        for p in range(3):
            orings[p].write_samples(x[p, a:b])
    feed(0, head)
    res = mgr.update_planes(pr, 2)
    assert tw.step(res) == 1                                       # the others run their first period, nobody a second one
    assert not res[1][:, late].any() and res[1][0].sum() == 4 and bytes(mgr.channels[late].state) == before
    feed(head, 6 * n + 100)                                        # then max_epochs beyond the data: the oracle's count and flags
    done = tw.step(mgr.update_planes(pr, 10))
    assert tw.ran == [(6 * n + 100 - r["sample_global_index"]) // n for r in starts]
    assert done == max(c - (i != late) for i, c in enumerate(tw.ran)) and done >= 4
    assert tw.step(mgr.update_planes(pr, 3)) == 0                  # nothing new: every pass unprocessed, zeros
    _fractions("gate", tw.check_states())
    mgr.close(); pr.close()


# ---- loss of lock inside a call ---------------------------------------------------------------------------------------------------------
def test_loss_of_lock_inside_update_planes(gpu, oracle):
    """channel 1 is mapped to a plane that holds faint noise only (prompt power far below LOCK_THRESHOLD = 15): 20 unlocked passes, reset +
    SatelliteLost inside the call, later passes unprocessed — against the free-running oracle as test_loss_of_lock_inside_update_all
    checks it; channel 0 keeps tracking its satellite beside it."""
    from gnss_sdr_rs_amd import tracking as T
    n, E = 2048, 26
    x, by_prn = _plane_scenes(oracle, FS, 1, 30, 430)
    rng = np.random.default_rng(12)
    noise = (0.01 * (rng.standard_normal((E + 2) * n) + 1j * rng.standard_normal((E + 2) * n))).astype(np.complex64)
    planes = np.ascontiguousarray(np.stack([x[2, :(E + 2) * n], noise]))
    pr, orings = _rings(oracle, planes, 1 << 16)
    s = by_prn[2]
    starts = [_acq_result(2, s["doppler_hz"] + 8.0, FS, s["code_start"]), _acq_result(22, s["doppler_hz"], FS, s["code_start"])]
    mgr = T.TrackingManager(FS, n_channels=2, code_index_mode=1)
    mgr.set_channel_planes([0, 1])
    ocs = []
    for i, r in enumerate(starts):
        mgr.channels[i].start(r)
        oc = oracle.TrackingChannel(i, FS, code_index_mode=1)
        oc.start(r)
        ocs.append(oc)
    outs, proc, lost, done = mgr.update_planes(pr, E)
    lost_at = {}
    for i, oc in enumerate(ocs):
        for ep in range(E):
            rc, exp, msg = oc.update_ex(orings[i])
            assert (rc != 0) == bool(proc[ep, i]), (i, ep, rc)
            if rc:
                assert float(np.max(np.abs(outs[ep, i, :6] - exp[:6]))) <= FREE_REL * max(float(np.hypot(exp[0], exp[1])), 1.0e4), (i, ep)
            else:
                assert not outs[ep, i].any()
            assert bool(lost[ep, i]) == (msg is not None), (i, ep, msg)
            if msg is not None:
                lost_at[i] = ep
        st = mgr.channels[i].state
        assert mgr.channels[i].is_active() == oc.is_active() and st.prn == oc.c.prn and st.lost_counter == oc.c.lost_counter
        assert st.next_sample_index == oc.c.next_sample_index and st.num_samples_per_code == oc.c.num_samples_per_code
    assert lost_at == {1: 19} and done == E                        # 20 unlocked passes: reset + SatelliteLost in pass 19 (0-based)
    assert not proc[20:, 1].any() and proc[:, 0].all()
    st = mgr.channels[1].state
    assert not st.active and st.prn == 0 and st.next_sample_index == 0
    for k in STATE_WORDS + ("i_prompt", "q_prompt"):
        assert getattr(st, k) == 0.0 == getattr(ocs[1].c, k), k
    mgr.close(); pr.close()


# ---- nothing existing moves -------------------------------------------------------------------------------------------------------------
def test_update_all_ignores_the_map(gpu, oracle):
    from gnss_sdr_rs_amd import tracking as T
    n, E = 2048, 6
    x, by_prn = _plane_scenes(oracle, FS, 1, 14, 300 + 48 * 3 + 40)
    ring = T.MulticastRingBuffer(1 << 15)
    ring.write_samples(x[0, :(E + 1) * n])
    starts = _starts(by_prn, FS, prns=[5, 13, 5])
    got = []
    for planes in (None, [2, 0, 1]):
        m = T.TrackingManager(FS, n_channels=3, code_index_mode=1)
        if planes:
            m.set_channel_planes(planes)
        for i, r in enumerate(starts):
            m.channels[i].start(r)
        outs, proc, lost, done = m.update_all(ring, E)
        assert proc.all() and done == E
        got.append((outs.view(np.uint32), [bytes(s) for s in m.get_states()]))
        m.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    ring.close()


# ---- device-side ordering ---------------------------------------------------------------------------------------------------------------
def test_a_held_writer_stream_orders_the_tracking_launch_on_the_device(gpu, oracle):
    """write_dev goes to a caller's stream that is provably still held back; update_planes_dev is enqueued before the release, gated on
    the ENQUEUED head.  After the release the state words equal the synchronous run's."""
    from gnss_sdr_rs_amd import tracking as T
    n, E = 2048, 6
    x, by_prn = _plane_scenes(oracle, FS, 1, 14, 300 + 48 * 3 + 40)
    x = np.ascontiguousarray(x[:, :(E + 1) * n])
    starts = _starts(by_prn, FS)

    def fresh():
        m = T.TrackingManager(FS, n_channels=5, code_index_mode=1)
        m.set_channel_planes(MAP)
        for i, r in enumerate(starts):
            m.channels[i].start(r)
        return m
    ref_pr = T.PlaneRing(3, 1 << 15)
    ref_pr.write(x)
    ref = fresh()
    ref.update_planes_dev(ref_pr, E)
    ref.synchronize()
    want = [bytes(s) for s in ref.get_states()]
    assert ref.channels[0].state.next_sample_index == starts[0]["sample_global_index"] + E * n
    ref.close(); ref_pr.close()

    with SS.HeldStream() as S:
        pr, idle = S.own(T.PlaneRing(3, 1 << 15)), S.own(T.PlaneRing(3, 16))
        mgr = S.own(fresh())
        mgr.update_planes_dev(idle, E)                              # the handle's blocks exist before anything is held (an empty ring: no pass runs)
        mgr.synchronize()
        d_x = S.device(x.nbytes)
        staged = S.stage(x)
        S.hold("plane ring writer")
        S.h2d(d_x, staged)
        pr.write_dev(d_x, x.shape[1], x.shape[1], stream=S.stream)
        assert pr.get_head() == x.shape[1]                          # enqueued, not landed
        mgr.update_planes_dev(pr, E)
        S.assert_held()
        S.sync()
        mgr.synchronize()
        assert [bytes(s) for s in mgr.get_states()] == want
        for p in range(3):
            assert np.array_equal(pr.copy_to_slice(p, 0, x.shape[1]).view(np.uint32), x[p].view(np.uint32)), p


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_outputs_states_and_head_untouched(gpu, oracle, hipbuf):
    from gnss_sdr_rs_amd import _lib, tracking as T
    L = gpu.lib()
    n, E = 2048, 2
    x, by_prn = _plane_scenes(oracle, FS, 1, 14, 300 + 48 * 3 + 40)
    pr = T.PlaneRing(3, 1 << 14)
    pr.write(x[:, :3 * n])
    ring_words = [pr.copy_to_slice(p, 0, 1 << 14) for p in range(3)]
    mgr = T.TrackingManager(FS, n_channels=5, code_index_mode=1)
    mgr.set_channel_planes(MAP)
    for i, r in enumerate(_starts(by_prn, FS)):
        mgr.channels[i].start(r)
    states = [bytes(s) for s in mgr.get_states()]
    outs = (_lib.TrkOut * (4096 * 5))()
    C.memset(outs, 0x5A, C.sizeof(outs))
    proc, lost, done = np.full(4096 * 5, 0x5A, np.uint8), np.full(4096 * 5, 0x5A, np.uint8), C.c_uint32(77)

    def call(h, r, e):
        return L.gm_trk_update_planes(h, r, e, C.cast(outs, C.c_void_p), proc.ctypes.data_as(C.c_void_p), lost.ctypes.data_as(C.c_void_p), C.byref(done))

    def untouched(m=mgr, want=states):
        assert bytes(outs) == b"\x5a" * C.sizeof(outs) and (proc == 0x5A).all() and (lost == 0x5A).all() and done.value == 77
        assert [bytes(s) for s in m.get_states()] == want and pr.get_head() == 3 * n
    for h, r, e, status in ((None, pr._h, E, -1), (mgr._h, None, E, -1), (mgr._h, pr._h, 0, -1), (mgr._h, pr._h, 4096, -5)):
        assert call(h, r, e) == status and L.gm_trk_update_planes_dev(h, r, e) == status, (h, r, e)
        untouched()
    mgr.set_channel_planes([2, 0, 3, 1, 0])                            # plane 3 of a ring of 3
    assert call(mgr._h, pr._h, E) == -5 and b"channel 2" in L.gm_last_error()
    assert L.gm_trk_update_planes_dev(mgr._h, pr._h, E) == -5
    untouched()
    with pytest.raises(_lib.GmError) as err:
        mgr.set_channel_planes([0, 0, 64, 0, 0])
    assert err.value.status == -5 and mgr.channel_planes() == [2, 0, 3, 1, 0]
    mgr.set_channel_planes(MAP)
    strict = T.TrackingManager(FS, n_channels=5, code_index_mode=1, strict_libm=True, strict_sum_order=True)
    # (the persistent kernel keeps the row as floats: gm_trk_create itself refuses such a code where the device's LDS per workgroup does
    #  not hold 64 KB of it, and then no handle exists to refuse; gm_trk_planes_plan's rule is held on the CPU either way)
    try:
        long_code = [(T.TrackingManager(FS, n_channels=5, code_index_mode=1, codes=np.ones((1, 16385), np.int8), nominal_code_rate=1.023e6), -5, b"16384")]
    except _lib.GmError as e:
        assert e.status == -5
        long_code = []
    print("a handle of 16385 chips %s on this device" % ("exists" if long_code else "is refused at create"))
    for m, status, word in [(strict, -1, b"strict_sum_order")] + long_code:
        m.channels[0].start(_acq_result(1, 0.0, FS, 0))
        want = [bytes(s) for s in m.get_states()]
        assert call(m._h, pr._h, E) == status and word in L.gm_last_error()
        assert L.gm_trk_update_planes_dev(m._h, pr._h, E) == status
        untouched(m, want)
        m.close()
    # the writer's refusals: the head and every ring word stay
    src = hipbuf.alloc(3 * 40000 * 8)
    base = pr.info()["d_base"]
    assert pr.info() == dict(n_planes=3, plane_size=1 << 14, bytes=3 * 8 << 14, d_base=base) and base
    for args, status in (((None, 100, 100), -1), ((src, (1 << 14) + 1, (1 << 14) + 1), -5), ((src, 99, 100), -5),
                         ((base, 1 << 14, 16), -5), ((base + 8 * (3 << 14) - 8, 16, 16), -5), ((base - 8 * (2 * 100 + 16) + 8, 100, 16), -5)):
        assert L.gm_plane_ring_write_dev(pr._h, args[0], args[1], args[2], None) == status, args
    host = np.zeros((3, 20000), np.complex64)
    assert L.gm_plane_ring_write(pr._h, None, 100, 100) == -1
    assert L.gm_plane_ring_write(pr._h, host.ctypes.data_as(C.c_void_p), 20000, (1 << 14) + 1) == -5
    assert L.gm_plane_ring_write(pr._h, host.ctypes.data_as(C.c_void_p), 99, 100) == -5
    assert L.gm_plane_ring_write_dev(pr._h, src, 40000, 0, None) == 0      # n = 0: nothing happens
    one = np.zeros(4, np.complex64)
    assert L.gm_plane_ring_copy_to_slice(pr._h, 3, 0, one.ctypes.data_as(C.c_void_p), 4) == -5
    assert L.gm_plane_ring_copy_to_slice(pr._h, 0, 0, None, 4) == -1
    assert L.gm_plane_ring_copy_to_slice(pr._h, 0, 0, one.ctypes.data_as(C.c_void_p), (1 << 14) + 1) == -5
    untouched()
    for p in range(3):
        assert np.array_equal(pr.copy_to_slice(p, 0, 1 << 14).view(np.uint32), ring_words[p].view(np.uint32)), p
    # and the accepted call still runs
    o, pc, ls, dn = mgr.update_planes(pr, E)
    assert dn == E and pc.all()
    mgr.close(); pr.close()


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
def test_beams_into_the_plane_ring_into_the_tracker(gpu, oracle, hipbuf):
    """a 4-antenna interleaved scene, a Beamformer in static-weights mode with P = 2 beams: process_dev -> PlaneRing.write_dev per block of
    samples (both on one stream of the caller's) -> update_planes.  Both channels stay locked for 10 epochs and meet the teacher-forced
    bars against the oracle run on the planes read back with copy_to_slice."""
    from gnss_sdr_rs_amd import _lib, tracking as T, synth
    from gnss_sdr_rs_amd.beamformer import Beamformer
    n, A, E, size = 2048, 4, 10, 1 << 15
    t = oracle.ca_code_table()
    sc = [synth.tracking_scene(t, FS, 0.0, [q], E + 3, config_id=460 + k, cn0=50.0, code_rows=[q - 1]) for k, q in enumerate((7, 19))]
    steer = np.exp(1j * np.pi * np.outer([0.31, -0.62], np.arange(A))).astype(np.complex64)      # the two array responses [2][A]
    total = (E + 2) * n
    xa = sum(np.outer(synth.to_c32(sc[k]["x"])[:total], steer[k]) for k in range(2)).astype(np.complex64)      # [time][A] interleaved
    # static weights: beam p passes satellite p with gain 1 and nulls the other one (the 2 x 2 system on the two responses)
    G = steer.conj() @ steer.T
    w = (np.linalg.solve(G, np.eye(2)).T @ steer).astype(np.complex64)                             # w_p^H a_q = delta_pq
    bf = Beamformer(A, 1, steer, block=1024)
    bf.set_weights(w)
    pr = T.PlaneRing(2, size)
    mgr = T.TrackingManager(FS, n_channels=2, code_index_mode=1)
    mgr.set_channel_planes([0, 1])
    starts = [_acq_result(q, sc[k]["sats"][0]["doppler_hz"] + 15.0, FS, sc[k]["sats"][0]["code_start"]) for k, q in enumerate((7, 19))]
    orings = [oracle.MulticastRingBuffer(size) for _ in range(2)]
    tw = Twin(mgr, orings, [0, 1], starts, lambda i: oracle.TrackingChannel(i, FS, code_index_mode=1), 3)
    with SS.HeldStream() as S:                                        # (a plain stream of the caller's: nothing is held here)
        blk, stride = 4096, 4096 + 64
        d_out = S.device(2 * stride * 8)
        fed = 0
        for a in range(0, total, blk):
            d_in = hipbuf.upload(xa[a:a + blk])
            got = bf.process_dev(d_in, _lib.FMT_C32, min(blk, total - a), d_out, stride, stream=S.stream)
            pr.write_dev(d_out, stride, got, stream=S.stream)
            head = pr.get_head()
            assert head == fed + got
            for p in range(2):                                        # the oracle runs on the planes as they were read back
                orings[p].write_samples(pr.copy_to_slice(p, fed, got))
            fed = head
            tw.step(mgr.update_planes(pr, 3))
        S.sync()
    w_ = tw.check_states()
    assert min(tw.ran) >= E and all(mgr.channels[i].is_active() for i in range(2)), tw.ran
    _fractions("beams -> plane ring -> tracker", w_)
    bf.close(); mgr.close(); pr.close()


# ---- the general sample loop: correlate_sample<ARMS, false> (trk_form_classes.py) ------------------------------------------------------------
FORM_E = 2
# the noise seed of each trigger's plane (1 where none is named).  At n = 50 000 and 16 777 the yardstick's own error is not small beside
# REL: the oracle's sequential f32 sums, held against its own f64 accumulation of the same products on the CPU (no device involved), miss
# it by 2.2e-6 .. 9.1e-6 (n = 50 000) and 1.6e-6 .. 5.1e-6 (n = 16 777) of the envelope over the seeds 1 .. 12 of this recipe, the largest
# of both epochs, both arm counts and both code-index modes (test_boc_4092_chips_five_arms has the reason for the tail).  The seeds below
# are the ones with the smallest figure, 2.2e-6 and 1.6e-6: under half of REL, so that REL measures the kernel and not the yardstick.  At
# n = 2048 the figure is 0.8e-6 .. 1.4e-6 for every trigger at seeds 1 and 2.  The figure a run itself sees is printed as "reference's own".
FORM_SEEDS = {"if-20MHz-at-50Msps": 2, "fs-significand-all-ones": 6}


def _form_planes(oracle, arms, mode, name):
    """the triggers of handle `name`, each on a plane of its own: a signal at the trigger's state from sample 0, FORM_E + 1 periods of it
    -> (triggers, x complex64 [P, (FORM_E + 1) n], handle kwargs, oracle kwargs, prns)"""
    trig = [t for t in FC.triggers("planes", name, arms) if t["id"] != "eligible"]
    hkw = dict(FC.HANDLES[name], n_arms=arms)
    fs = hkw["fs"]
    n = FC.samples_per_code(fs)
    table = oracle.ca_code_table()
    prns = [4 + 3 * k for k in range(len(trig))]
    xs = []
    for t, prn in zip(trig, prns):
        st = FC.state_of(t)
        row = table[prn if mode == 0 else prn - 1]          # FAITHFUL indexes row `prn`: that code is in the air
        total = (FORM_E + 1) * n
        xs.append((FC.replica(row, fs, total, st["carrier_freq"], st["code_phase"]) + FC.noise(total, FORM_SEEDS.get(t["id"], 1))).astype(np.complex64))
    okw = dict(n_arms=arms, el_space=hkw.get("early_late_space", 0.5), vel_space=hkw.get("very_early_late_space", 1.0))
    return trig, np.ascontiguousarray(np.stack(xs)), hkw, okw, prns


def _form_state(c, st):
    """the trigger's state words into a channel record (the oracle's or the handle's: the same f32 words)"""
    c.carrier_freq, c.carrier_phase, c.code_phase = st["carrier_freq"], st["carrier_phase"], st["code_phase"]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("arms", [3, 5])
def test_general_forms_two_epochs(gpu, oracle, arms, mode):
    """Every planes trigger of trk_form_classes: the channel is started, its state is set to the trigger's on the handle and on both oracle
    twins, and FORM_E = 2 epochs run in one call against the oracle, teacher-forced from the same state (and free-running), with the bars
    and the helpers of every other case here.  The first epoch is in the class the trigger is named for (test_trk_form_classes_host.py);
    the epilogue wraps both phases, so the second epoch is general only where the handle makes it so (spacing, fs)."""
    from gnss_sdr_rs_amd import tracking as T
    for name in FC.HANDLES:
        if not FC.triggers("planes", name, arms):           # (three arms: no very-early / very-late spacing)
            continue
        trig, x, hkw, okw, prns = _form_planes(oracle, arms, mode, name)
        fs = hkw["fs"]
        n = FC.samples_per_code(fs)
        size = 1 << int(np.ceil(np.log2(x.shape[1])))
        pr, orings = _rings(oracle, x, size)
        mgr = T.TrackingManager(n_channels=len(trig), code_index_mode=mode, **hkw)
        mgr.set_channel_planes(list(range(len(trig))))
        starts = [_acq_result(prn, FC.state_of(t)["carrier_freq"], fs, 0) for t, prn in zip(trig, prns)]
        tw = Twin(mgr, orings, list(range(len(trig))), starts, lambda i: oracle.TrackingChannel(i, fs, code_index_mode=mode, **okw), arms)
        for i, t in enumerate(trig):
            st = FC.state_of(t)
            mgr.channels[i].set_state(carrier_freq=st["carrier_freq"], carrier_phase=st["carrier_phase"], code_phase=st["code_phase"])
            _form_state(tw.forced[i].c, st)
            _form_state(tw.free[i].c, st)
            got = mgr.channels[i].state
            assert FC.classify(FC.handle(**hkw), got, n) == t["form"], t["id"]      # the record as the device holds it is in its class
        assert tw.step(mgr.update_planes(pr, FORM_E)) == FORM_E
        w = tw.check_states()
        assert tw.ran == [FORM_E] * len(trig)
        _fractions("general forms, arms %d mode %d, %s [%s]" % (arms, mode, name, ", ".join(t["id"] for t in trig)), w)
        mgr.close(); pr.close()
