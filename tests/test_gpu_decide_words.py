"""Every device form of the acquisition decision, and gm_grid_assemble_dev in front of it, on hand-written words.

`decide_body` (csrc/acq_kernels.hip) replays the reference's sequential scan as a 64-lane prefix scan of (value, bin) with a carry
between trips of 64 bins and a ballot for the exit.  It is a pure function of a few hundred 32-bit words, so every result here is
compared word for word — floats by their bit patterns, every field of every gm_acq_result, every found byte — with the sequential
model of tests/decide_model.py, whose catalogue holds the inputs on which the two scans can part company (ties, ties across lanes
63 / 64 and against the carry, D = 64, 65, 128, a first pass in the last lane of a trip, no positive maximum, NaN and inf words,
sum == max, a ratio equal to the threshold, argmax words above 2^24, a local_tail above 2^32, more than 64 codes).
tests/test_decide_model_host.py holds that model to the oracle and to gm_acq_decide_host.  No number in this file is a tolerance.

The three C entries that reach the device code:
  (a) gm_acq_decide_planes_dev (no handle)                      test_planes_dev_*
  (b) gm_acq_decide_dev, launched at once (decide_kernel)        test_decide_dev_*
  (c) the ride behind gm_acq_set_deferred_decision               test_deferred_decision_*
      (wave 0 of the trailing workgroups of acq_mix_fft_kernel<Plan>, fences instead of a barrier)
  (d) (a) against gm_acq_decide_host on the same words           test_planes_dev_equals_decide_host
and gm_grid_assemble_dev, the other word-only kernel, on words that encode their own place (test_grid_assemble_*).

`regroup_metrics_kernel` needs a communicator of more than one rank and stays untested here: tests/test_distributed_gloo.py runs the
exchange it belongs to on the CPU backend, and the single-rank RCCL test cannot reach a regroup that moves anything.

Measured on an MI355X: the 30 cases of this file run in 1.2 s (pytest's own wall time), the slowest in 0.07 s.
"""
import ctypes as C

import numpy as np
import pytest

import decide_model as DM

pytestmark = pytest.mark.gpu
f32 = np.float32
CANARY = 0xA5
REC = DM.RESULT_DTYPE.itemsize
GUARD = 2                       # canary records / 16-byte found blocks on either side
OK, INVALID_ARG, OUT_OF_RANGE = 0, -1, -5
ALL_ON = 2 ** 64 - 1
RATES = (DM.CA_RATE, 2.046e6, 10.23e6)        # one per local_tail of DM.LOCAL_TAILS
MAX_BINS = 5461                               # GM_ACQ_DECIDE_MAX_BINS


def _fs(N):
    return N * 1000.0


def _ids(P):
    return ((np.arange(P) % 250) + 1).astype(np.uint8)


@pytest.fixture
def stream(hipbuf):
    """a non-blocking stream of the caller's, through the HIP runtime handle hipbuf holds"""
    s = C.c_void_p()
    assert hipbuf.hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0      # hipStreamNonBlocking
    yield s.value
    assert hipbuf.hip.hipStreamSynchronize(s) == 0
    assert hipbuf.hip.hipStreamDestroy(s) == 0


class _Out:
    """device result and found arrays of n codes with canary-filled slots on both sides"""

    def __init__(self, hipbuf, n):
        self.hb, self.n = hipbuf, n
        self.rbytes, self.fbytes = (n + 2 * GUARD) * REC, n + 2 * GUARD * 16
        self.d_res, self.d_found = hipbuf.alloc(self.rbytes, fill=CANARY), hipbuf.alloc(self.fbytes, fill=CANARY)
        self.res, self.found = self.d_res + GUARD * REC, self.d_found + GUARD * 16

    def reset(self):
        assert self.hb.hip.hipMemset(C.c_void_p(self.d_res), CANARY, self.rbytes) == 0
        assert self.hb.hip.hipMemset(C.c_void_p(self.d_found), CANARY, self.fbytes) == 0
        assert self.hb.hip.hipDeviceSynchronize() == 0

    def raw(self):
        return self.hb.download(self.d_res, self.rbytes, np.uint8), self.hb.download(self.d_found, self.fbytes, np.uint8)

    def untouched(self):
        r, f = self.raw()
        return bool((r == CANARY).all() and (f == CANARY).all())

    def read(self):
        r, f = self.raw()
        g, h = GUARD * REC, GUARD * 16
        assert (r[:g] == CANARY).all() and (r[-g:] == CANARY).all(), "a result was written outside [0, n_prn)"
        assert (f[:h] == CANARY).all() and (f[-h:] == CANARY).all(), "a found byte was written outside [0, n_prn)"
        return DM.unpack(r[g:g + self.n * REC], f[h:h + self.n], self.n)


class _Planes:
    """the words of `rows` on the device, and gm_acq_decide_planes_dev on them"""

    def __init__(self, hipbuf, rows, tf):
        from gnss_sdr_rs_amd._lib import lib
        self.L, self.hb = lib(), hipbuf
        self.P, self.D = len(rows), len(tf)
        mx, am, sm = DM.stack(rows)
        self.ids = _ids(self.P)
        self.d = [hipbuf.upload(a) for a in (mx, am, sm, self.ids, np.ascontiguousarray(tf, f32))]
        self.out = _Out(hipbuf, self.P)

    def call(self, N, fs, rate, thr, mode, tail, stream=0, n_bins=None):
        d_mx, d_am, d_sm, d_ids, d_tf = self.d
        return self.L.gm_acq_decide_planes_dev(d_mx, d_am, d_sm, self.P, self.D if n_bins is None else n_bins, d_ids, d_tf, N, fs, rate,
                                               thr, mode, tail, self.out.res, self.out.found, stream)

    def run(self, N, fs, rate, thr, mode, tail, stream=0):
        self.out.reset()
        assert self.call(N, fs, rate, thr, mode, tail, stream) == OK
        if stream:
            assert self.hb.hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
        return self.out.read()


def _diff(got, want, rows):
    """the rows that differ, by name: what a failing case prints"""
    return [(rows[p][0], dict(zip(DM.FIELDS, got[p])), dict(zip(DM.FIELDS, want[p]))) for p in range(len(want)) if got[p] != want[p]][:6]


# ------------------------------------------------------------------------------------------------------------ (a) no handle
@pytest.mark.parametrize("D", (1, 2, 63, 64, 65, 127, 128, 129, 151))
def test_planes_dev_every_catalogue_row(gpu, hipbuf, stream, D):
    """The catalogue rows of one D as the codes of one call: both decision modes, thresholds 7.0 and 2.5, fft_size 2048 and 2049, the
    three local_tail values (each with a code rate of its own, two of them not the C/A rate), on the NULL stream and on a non-blocking
    stream of the caller's."""
    tf = DM.table_freq(D)
    for N in (2048, 2049):
        rows = DM.cases(N, D)
        pl = _Planes(hipbuf, rows, tf)
        for mode in (0, 1):
            for thr in DM.THRESHOLDS:
                hits = DM.scans(rows, N, thr, bool(mode))
                for tail, rate in zip(DM.LOCAL_TAILS, RATES):
                    want = DM.expected(hits, tf, pl.ids, _fs(N), tail, rate)
                    for st in (0, stream):
                        got = pl.run(N, _fs(N), rate, thr, mode, tail, st)
                        assert got == want, (N, mode, thr, tail, bool(st), _diff(got, want, rows))


@pytest.mark.parametrize("D", (2, 65))
def test_planes_dev_seventy_codes(gpu, hipbuf, D):
    """More than 64 codes in one call: every one of them is decided, codes 64 to 69 included (searched = p >= 64 || mask bit)."""
    N, P = 2048, 70
    cat, tf = DM.cases(N, D), DM.table_freq(D)
    rows = [cat[(5 * i) % len(cat)] for i in range(P)]
    assert sum(h[0] for h in DM.scans(rows[64:], N)) >= 2
    pl = _Planes(hipbuf, rows, tf)
    for mode in (0, 1):
        want = DM.expected(DM.scans(rows, N, 7.0, bool(mode)), tf, pl.ids, _fs(N), 2 ** 40, RATES[1])
        got = pl.run(N, _fs(N), RATES[1], 7.0, mode, 2 ** 40)
        assert got == want, (mode, _diff(got, want, rows))


def test_planes_dev_zero_values_mean_the_defaults(gpu, hipbuf):
    """threshold == 0 is 7.0 and code_rate <= 0 the C/A rate, as in gm_acq_cfg and gm_acq_decide_host (include/gnss_mi355x.h)."""
    N, D = 2049, 65
    rows, tf = DM.cases(N, D), DM.table_freq(D)
    pl = _Planes(hipbuf, rows, tf)
    want = DM.expected(DM.scans(rows, N, 7.0), tf, pl.ids, _fs(N), 77, DM.CA_RATE)
    assert sum(w[0] for w in want) >= len(rows) // 3 and any(w[0] and w[2] for w in want)
    for thr, rate in ((0.0, 0.0), (7.0, -1.0), (0.0, DM.CA_RATE), (-0.0, float("nan"))):
        got = pl.run(N, _fs(N), rate, thr, 0, 77)
        assert got == want, (thr, rate, _diff(got, want, rows))
    assert pl.run(N, _fs(N), DM.CA_RATE, 2.5, 0, 77) != want


def test_planes_dev_n_bins_limit(gpu, hipbuf):
    """n_bins above GM_ACQ_DECIDE_MAX_BINS (what decide_kernel can stage: 64 KB of dynamic LDS over 12 bytes per bin) is refused on
    the host with GM_ERR_OUT_OF_RANGE and the limit in the message, nothing written; one call AT the limit decides like the model; a
    valid call after the refusal works."""
    from gnss_sdr_rs_amd._lib import lib
    N = 2048
    rows, tf = DM.limit_rows(N, MAX_BINS), DM.table_freq(MAX_BINS)
    assert [r[0].split("@")[0] for r in rows] == ["limit/pass_last", "limit_tie/fail", "limit/quiet"]
    pl = _Planes(hipbuf, rows, tf)
    pl.out.reset()
    assert pl.call(N, _fs(N), DM.CA_RATE, 7.0, 0, 0, n_bins=MAX_BINS + 1) == OUT_OF_RANGE
    assert str(MAX_BINS) in lib().gm_last_error().decode()
    assert pl.out.untouched()
    for mode in (0, 1):
        want = DM.expected(DM.scans(rows, N, 7.0, bool(mode)), tf, pl.ids, _fs(N), 5, DM.CA_RATE)
        assert [w[0] for w in want] == [1, 0, 0] and want[0][8] == MAX_BINS - 1
        got = pl.run(N, _fs(N), DM.CA_RATE, 7.0, mode, 5)
        assert got == want, (mode, _diff(got, want, rows))
    small = _Planes(hipbuf, DM.cases(N, 2), DM.table_freq(2))
    assert small.call(N, _fs(N), DM.CA_RATE, 7.0, 0, 0, n_bins=MAX_BINS + 1) == OUT_OF_RANGE
    assert small.run(N, _fs(N), DM.CA_RATE, 7.0, 0, 0) == DM.expected(DM.scans(DM.cases(N, 2), N), DM.table_freq(2), small.ids, _fs(N))


# ------------------------------------------------------------------------------------------------------------ (d) device against host
@pytest.mark.parametrize("D", (41, 128, 151))
def test_planes_dev_equals_decide_host(gpu, hipbuf, D):
    """One D per trip count (one, two, three trips of 64 lanes): the device result equals gm_acq_decide_host on the same words,
    the zero values of threshold and code_rate included."""
    from gnss_sdr_rs_amd._lib import lib
    N = 2049
    rows, tf = DM.cases(N, D), DM.table_freq(D)
    P = len(rows)
    mx, am, sm = DM.stack(rows)
    pl = _Planes(hipbuf, rows, tf)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n_found = set()
    for thr, rate, tail in ((7.0, DM.CA_RATE, 0), (2.5, 2.046e6, 2 ** 32 - 1), (0.0, 0.0, 2 ** 40)):
        raw, found = np.full(P * REC, CANARY, np.uint8), np.full(P, CANARY, np.uint8)
        assert lib().gm_acq_decide_host(p(mx), p(am), p(sm), p(tf), P, D, p(pl.ids), N, _fs(N), rate, thr, tail, p(raw), p(found)) == OK
        host = DM.unpack(raw, found, P)
        got = pl.run(N, _fs(N), rate, thr, 0, tail)
        assert got == host, (thr, rate, tail, _diff(got, host, rows))
        n_found.add(sum(h[0] for h in host))
    assert len(n_found) == 2 and min(n_found) >= P // 3


# ------------------------------------------------------------------------------------------------------------ (b) a handle, at once
def _fetch(eng, n):
    """gm_acq_fetch_results into host arrays with canaries on both sides -> DM.words tuples"""
    from gnss_sdr_rs_amd._lib import lib
    raw, found = np.full((n + 2 * GUARD) * REC, CANARY, np.uint8), np.full(n + 2 * GUARD * 16, CANARY, np.uint8)
    g, h = GUARD * REC, GUARD * 16
    assert lib().gm_acq_fetch_results(eng._h, n, C.c_void_p(raw.ctypes.data + g), C.c_void_p(found.ctypes.data + h)) == OK
    assert (raw[:g] == CANARY).all() and (raw[-g:] == CANARY).all() and (found[:h] == CANARY).all() and (found[-h:] == CANARY).all()
    return DM.unpack(raw[g:g + n * REC], found[h:h + n], n)


def _put(hipbuf, d_ptr, block):
    b = np.ascontiguousarray(block)
    assert hipbuf.hip.hipMemcpy(C.c_void_p(d_ptr), b.ctypes.data, b.nbytes, 1) == 0


@pytest.mark.parametrize("D", (41, 65))
def test_decide_dev_at_once(gpu, hipbuf, D):
    """gm_acq_decide_dev on a small handle (N = 2048, M = 1, three C/A codes), its D set by the Doppler grid.  The caller's block of
    P rows under masks that switch single codes off (a masked code gives the not-found record even where its row passes); n_prn = 7
    and 70 with explicit prn_ids, where every code is searched whatever the handle's mask; the threshold and the mode are the
    handle's: 7.0 in reference mode, and a second handle with 2.5 in best-bin mode."""
    from gnss_sdr_rs_amd import acquisition as A, distributed as Dm
    N, fs, prns = 2048, 2.048e6, [3, 7, 12]
    P = len(prns)
    dop = (np.linspace(-5000.0, 5000.0, D) + 12.5).astype(f32)         # (no bin at 0.0, the not-found record's carrier_freq)
    cat = DM.cases(N, D)
    d_met = hipbuf.alloc(3 * P * D * 4)
    for thr, mode in ((7.0, 0), (2.5, 1)):
        eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=prns, n_integrations=1, threshold=thr, decision_mode=mode)
        try:
            tf = eng.table_freq.copy()
            assert len(set(tf.tolist())) == D and (tf != 0).all()
            hits = DM.scans(cat, N, thr, bool(mode))
            masked_hits = 0
            for c in range(0, len(cat), P):
                idx = [(c + i) % len(cat) for i in range(P)]
                mask = (0b111, 0b110, 0b101, 0b011)[(c // P) % 4]
                tail = DM.LOCAL_TAILS[(c // P) % 3]
                _put(hipbuf, d_met, Dm.pack_metrics(*DM.stack([cat[i] for i in idx])))
                eng.set_prn_mask(mask)
                eng.decide_dev(d_met, local_tail=tail)
                got = _fetch(eng, P)
                want = DM.expected([hits[i] for i in idx], tf, prns, fs, tail, DM.CA_RATE, mask)
                assert got == want, (thr, mode, mask, _diff(got, want, [cat[i] for i in idx]))
                masked_hits += sum(hits[i][0] for k, i in enumerate(idx) if not (mask >> k) & 1)
            assert masked_hits >= 3
            eng.set_prn_mask(0b010)
            for n in (7, 70):
                idx = [(3 * i) % len(cat) for i in range(n)]
                ids = _ids(n)
                d_blk = hipbuf.upload(Dm.pack_metrics(*DM.stack([cat[i] for i in idx])))
                eng.decide_dev(d_blk, n_prn=n, prn_ids=ids, local_tail=2 ** 40)
                got = _fetch(eng, n)
                want = DM.expected([hits[i] for i in idx], tf, ids, fs, 2 ** 40, DM.CA_RATE)
                assert got == want, (thr, mode, n, _diff(got, want, [cat[i] for i in idx]))
                assert sum(w[0] for w in want[:3]) + sum(w[0] for w in want[64:]) >= 2
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------------------ (c) the deferred form
# The two transform sizes: 8000 is the smallest fused in-LDS size whose correlation plan stores its spectrum permuted
# (CorrMode<CorrPlan8000>::PERMUTED: a HybridPlan; the other permuted ones are 8184, 16000 and 16368), 256 the smallest whose plan
# does not (Plan256, plain radices [16, 16]: its stage-F workgroup is the single wave that also decides).  Two instantiations of
# acq_mix_fft_kernel therefore carry the decision: one with the staging image of the permuted store, one without.
DEFERRED = [(256, D, 7.0, 0) for D in (1, 41, 64, 65)] + [(8000, D, 7.0, 0) for D in (1, 41, 64, 65)] + [(8000, 64, 2.5, 1)]


@pytest.mark.parametrize("N,D,thr,mode", DEFERRED)
def test_deferred_decision_on_words(gpu, hipbuf, N, D, thr, mode):
    """The call order of test_deferred_decision_rides_with_the_next_search (b) on catalogue words: search_dev into d_met, synchronize,
    d_met overwritten with the words by a plain hipMemcpy, set_deferred_decision(True), decide_dev(d_met), search_dev of the same
    samples into another block, fetch_results.  Whether the decision rode inside stage F or was flushed cannot be observed from
    outside; the call order is what selects the ride (the search's stage-F launch in gm_api.hip hands `dec_args` to the kernel while
    `dec_deferred` is set, i.e. when nothing between decide_dev and that search flushed it).  D = 64 is the largest D the ride accepts — every lane is live; with D = 65
    the same calls decide at once, and the results are the same.  The handle has one code per catalogue row (more than 64 of them at
    D >= 64), so the mask decides too: a mask changed after decide_dev and before the carrying search does not change the decision."""
    from gnss_sdr_rs_amd import acquisition as A, distributed as Dm
    rows = DM.cases(N, D)
    P, fs = len(rows), _fs(N)
    rng = np.random.default_rng(N + D)
    ids = _ids(P)
    codes = (2 * rng.integers(0, 2, (P, 1023)) - 1).astype(np.int8)
    dop = (np.linspace(-4000.0, 4000.0, D) + 12.5).astype(f32) if D > 1 else np.array([250.0], f32)
    d_x = hipbuf.upload(rng.standard_normal(2 * N).astype(f32))
    block = Dm.pack_metrics(*DM.stack(rows))
    d_met, d_other = hipbuf.alloc(block.nbytes), hipbuf.alloc(block.nbytes)
    hits = DM.scans(rows, N, thr, bool(mode))
    found_low = [p for p in range(min(P, 64)) if hits[p][0]]
    part = ALL_ON ^ (1 << found_low[0]) ^ (1 << found_low[-1]) ^ (1 << [p for p in range(min(P, 64)) if not hits[p][0]][0])
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=ids, n_integrations=1, codes=codes, threshold=thr, decision_mode=mode)
    try:
        assert eng.plan_info()["form"] == "lds" and eng.plan_info()["base"] == N       # the fused in-LDS path
        tf = eng.table_freq.copy()
        for at_decide, after, tail in ((ALL_ON, None, 0), (part, ALL_ON, 2 ** 32 - 1), (ALL_ON, part, 2 ** 40)):
            eng.set_prn_mask(at_decide)
            eng.search_dev(d_x, A.FMT_C32, d_met)
            eng.synchronize()
            _put(hipbuf, d_met, block)
            eng.set_deferred_decision(True)
            eng.decide_dev(d_met, local_tail=tail)
            if after is not None:
                eng.set_prn_mask(after)
            eng.search_dev(d_x, A.FMT_C32, d_other)
            got = _fetch(eng, P)
            want = DM.expected(hits, tf, ids, fs, tail, DM.CA_RATE, at_decide)
            assert got == want, (at_decide == ALL_ON, tail, _diff(got, want, rows))
            assert (hipbuf.download(d_met, block.nbytes, np.int32) == block).all()      # the words are still what was decided
        # the same words decided at once by the same handle
        eng.set_deferred_decision(False)
        eng.set_prn_mask(ALL_ON)
        eng.decide_dev(d_met, local_tail=9)
        got, want = _fetch(eng, P), DM.expected(hits, tf, ids, fs, 9, DM.CA_RATE)
        assert got == want, _diff(got, want, rows)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ gm_grid_assemble_dev
def _grid_words(nranks, pmax, D):
    """[nranks][3][pmax][D]: the word at [r][q][k][e] encodes (r, q, k, e)"""
    r, q, k, e = np.meshgrid(np.arange(nranks), np.arange(3), np.arange(pmax), np.arange(D), indexing="ij")
    return (((r * 3 + q) * 8 + k) * 128 + e).astype(np.uint32)


def _row_maps(nranks, pmax, rng):
    total = nranks * pmax
    full = (nranks + 1) // 2            # uneven shards: the first `full` ranks hold pmax rows, the others one fewer (padded)
    return {"identity": np.arange(total), "reversed": np.arange(total)[::-1],
            "skips_padding": np.array([r * pmax + k for r in range(nranks) for k in range(pmax if r < full else pmax - 1)]),
            "fewer_rows": rng.permutation(total)[:max(1, total // 2)]}


@pytest.mark.parametrize("nranks", (1, 3, 8))
def test_grid_assemble_on_words_that_encode_their_place(gpu, hipbuf, stream, nranks):
    """gathered [nranks][3][p_max][D] -> [3][n_rows][D], row i from block row_map[i] = rank * p_max + row: distributed.grid_assemble's
    indexing restated in numpy, for the identity, a reversed map, a map that skips the padded rows of uneven shards and one with
    n_rows < nranks * p_max; words past 3 * n_rows * D keep their canary; the refusals write nothing."""
    from gnss_sdr_rs_amd._lib import lib
    L, rng, TAIL = lib(), np.random.default_rng(nranks), 16
    k = 0
    for pmax in (1, 5):
        for D in (1, 41, 65):
            g = _grid_words(nranks, pmax, D)
            d_g = hipbuf.upload(g)
            for name, m in _row_maps(nranks, pmax, rng).items():
                m = np.ascontiguousarray(m, np.uint32)
                n_rows = len(m)
                want = g[m // pmax, :, m % pmax, :].transpose(1, 0, 2)          # [3][n_rows][D]
                assert want.shape == (3, n_rows, D) and want[1, n_rows - 1, D - 1] == g[m[-1] // pmax, 1, m[-1] % pmax, D - 1]
                d_out = hipbuf.alloc((want.size + TAIL) * 4, fill=CANARY)
                st = (0, stream)[k % 2]
                k += 1
                assert L.gm_grid_assemble_dev(d_g, nranks, pmax, D, hipbuf.upload(m), n_rows, d_out, st) == OK
                if st:
                    assert hipbuf.hip.hipStreamSynchronize(C.c_void_p(st)) == 0
                got = hipbuf.download(d_out, (want.size + TAIL) * 4, np.uint32)
                assert (got[:want.size] == want.ravel()).all(), (pmax, D, name)
                assert (got[want.size:] == 0xA5A5A5A5).all(), (pmax, D, name)
    # the refusals: a zero dimension, more rows than the gathered blocks hold
    pmax, D = 5, 41
    d_g, d_map = hipbuf.upload(_grid_words(nranks, pmax, D)), hipbuf.upload(np.arange(nranks * pmax + 1, dtype=np.uint32) % (nranks * pmax))
    d_out = hipbuf.alloc(3 * (nranks * pmax + 1) * D * 4, fill=CANARY)
    for args, status in (((0, pmax, D, nranks * pmax), INVALID_ARG), ((nranks, 0, D, nranks * pmax), INVALID_ARG),
                         ((nranks, pmax, 0, nranks * pmax), INVALID_ARG), ((nranks, pmax, D, 0), INVALID_ARG),
                         ((nranks, pmax, D, nranks * pmax + 1), OUT_OF_RANGE)):
        assert L.gm_grid_assemble_dev(d_g, args[0], args[1], args[2], d_map, args[3], d_out, 0) == status, args
    assert (hipbuf.download(d_out, 3 * (nranks * pmax + 1) * D * 4, np.uint8) == CANARY).all()
