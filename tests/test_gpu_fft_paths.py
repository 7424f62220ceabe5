"""GPU: FFT<T> / RealFFT<T> (gm_fft_c2c_f32, gm_fft_power_spectrum_f32, gm_rfft_f32) held to the float64 model of tests/fft_model.py
on every path a length can take: each of the 18 in-LDS plans, each of the 28 four-step kernels (through gm_debug_fft_four_step,
which names the factor pair: the public entry reaches a row plan above 512 only at 2^25 points and more), the public route onto
them, Bluestein's classes of L, the power spectrum, the real transform, and the refusals.

Yardsticks.  Per bin: |device - float64| <= B u |x|_1 with B derived from csrc/fft_core.h in fft_model.py's docstring (a worst-case
bound; it is tight enough on impulses, tones and their mixture to catch a wrong twiddle, a wrong sign or a leaked bin).  On noise
additionally the relative L2 bars the suite already had: 1e-6 in LDS, 4e-6 four-step, 3e-6 / 4e-6 Bluestein (which has no useful
per-bin bound).  The reference is np.fft of the exact float32 input words in complex128.

Not tested: public four-step lengths 2^24 .. 2^28 (256 MB .. 2 GB per buffer).  Their kernels all run in the pair matrix below, but
above L = 2^24 the twiddle argument float(n2 k1 mod L) is no longer exact, and that precision effect is covered by no test.

Measured on an MI355X — a record, not a threshold (largest per-bin error over its bound | largest relative L2 error, worst case of the group):
  in-LDS plans       noise 0.016 | 4.4e-7    impulses 0.228 (256, inverse) | 7.4e-7    tones 0.080 | 8.3e-7 (16000)    mixture 0.070 | 6.4e-7
  round trip         0.049 of twice the bound (256, impulses);  batch of 257 at N = 256: 0.024 | 2.4e-7
  four-step pairs    noise 0.0014 | 3.7e-7    impulses 0.216 (256 x 256, inverse) | 5.9e-7    tone 0.052 | 5.3e-7
  public 2^23        0.0001 | 3.3e-7 (16384 x 512, noise), and the words of every public length equal the named pair's
  Bluestein          L2 only: 0 (n = 1), 1.3e-7 (2), 1.2e-7 (3), 5.5e-7 (127), 6.8e-7 (8191), 5.5e-7 (8193), 6.3e-7 (16383), 6.8e-7 (40000),
                     7.9e-7 (100003, a tone) against bars of 3e-6 / 4e-6
  power spectrum     0.037 of its bound (256, mixture);  RealFFT 0.013 (256), Bluestein lengths 5.3e-7 L2 (1000)
So the worst-case bound is within five times of the observed error on impulses, where every value has modulus |x|_1 at every pass, and
60 to 1000 times above it on noise.
Three arithmetic-only mutants, tried on side builds (nothing of them is kept): (a) without `if (INV) sn = -sn` in big_cols_kernel all 13
inverse cases of test_every_four_step_kernel fail and all 13 forward ones pass; (b) with the four-step twiddle's phase scaled by 1 + 2^-16
all 26 fail: impulses are 10 to 14 times outside the bound, and the noise L2 (3.2e-5) misses its 4e-6 bar by 8 times as well, so the L2
bar alone would have caught this one too (either yardstick loses such a scale error near 2^-19); (c) with `% n` for `% (2 * n)` in Bluestein's chirp
every length above 2 fails (3, 127, 8191, 8193, 16383, 100003 and the even 40000; n = 1 and 2 have the same chirp either way), and so do
test_power_spectrum[1023] and test_real_fft at 3, 255 and 1000.
"""
import ctypes as C

import numpy as np
import pytest

import fft_model as M

pytestmark = pytest.mark.gpu
SEED = 20
PAIRS = [(p, 256) for p in M.POW2_PLANS] + [(256, p) for p in M.POW2_PLANS if p != 256]
WORST = {}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _note(group, case, eob=0.0, l2=0.0):
    """print a case's largest error over bound and largest L2 error; keep the worst of the group"""
    w = WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], float(eob)), max(w[1], float(l2))
    print(f"[fft_paths] {group} {case}: err/bound {float(eob):.4f}  L2 {float(l2):.3e}   (group worst {w[0]:.4f}  {w[1]:.3e})")


def _held(group, case, run, x, b, inv, l2_bar=None, fails=None):
    """run(x copy) against the float64 transform of x: every bin of every batch item within B's bound, and the L2 bar if one is given.
    With `fails` a list, a miss is appended to it and the caller asserts once every input kind has been measured and printed."""
    ref = M.reference(x, inv)
    got = run(x.copy())
    eob, l2 = M.err_over_bound(got, ref, b, x).max(), M.l2_rel(got, ref).max()
    _note(group, case, eob, l2)
    missed = [(group, case, what, v) for what, v, ok in (("err/bound", eob, eob <= 1.0), ("L2", l2, l2_bar is None or l2 < l2_bar)) if not ok]
    if fails is None:
        assert not missed, missed
    else:
        fails += missed
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. every in-LDS plan
@pytest.mark.parametrize("inv", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("n", sorted(M.RADICES))
def test_every_lds_plan_per_bin(gpu, n, inv):
    from gnss_sdr_rs_amd import fft
    run = lambda x: fft.FFT(n).execute(x.reshape(-1), inverse=inv)
    fails = []
    _held("lds", f"{n} inv={int(inv)} noise", run, M.noise(n, SEED, 3), M.B(n), inv, l2_bar=1e-6, fails=fails)
    _held("lds", f"{n} inv={int(inv)} impulses", run, M.impulses(n, SEED, 64), M.B(n), inv, fails=fails)
    _held("lds", f"{n} inv={int(inv)} tones", run, M.tones(n, SEED, 16), M.B(n), inv, fails=fails)
    _held("lds", f"{n} inv={int(inv)} mixture", run, M.mixture(n, SEED), M.B(n), inv, fails=fails)
    assert not fails, fails


@pytest.mark.parametrize("n", sorted(M.RADICES))
def test_every_lds_plan_round_trip(gpu, n):
    """inverse(forward(x)) against n x within twice the bound of an input of 1-norm n |x|_1 (fft_model.py, "Round trip")"""
    from gnss_sdr_rs_amd import fft
    for kind, x in (("noise", M.noise(n, SEED + 1, 3)), ("impulses", M.impulses(n, SEED + 1, 64)), ("mixture", M.mixture(n, SEED + 1))):
        y = fft.FFT(n).execute(fft.FFT(n).execute(x.copy().reshape(-1)), inverse=True).reshape(x.shape)
        want = n * x.astype(np.complex128)
        eob = (np.abs(y - want).max(axis=-1) / (2.0 * n * M.bound(M.B(n), x))).max()
        _note("lds round trip", f"{n} {kind}", eob)
        assert eob <= 1.0, (n, kind, eob)


@pytest.mark.parametrize("batch", [1, 257])
def test_lds_batch_items_each_against_their_own_reference(gpu, batch):
    """N = 256: every value of blockIdx.x of a batch of 257 (and a batch of one) against a reference of its own"""
    from gnss_sdr_rs_amd import fft
    for inv in (False, True):
        x = M.noise(256, SEED + batch, batch)
        got = _held("lds batch", f"256 x {batch} inv={int(inv)}", lambda v: fft.FFT(256).execute(v.reshape(-1), inverse=inv), x, M.B(256),
                    inv, l2_bar=1e-6)
        ref = M.reference(x, inv)
        assert (M.l2_rel(got, ref) < 1e-6).all() and (M.err_over_bound(got, ref, M.B(256), x) <= 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. every four-step kernel
@pytest.mark.parametrize("inv", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("n1,n2", PAIRS)
def test_every_four_step_kernel(gpu, n1, n2, inv):
    """big_cols_kernel<n1> then big_rows_kernel<n2>, named: 7 + 7 plans x 2 directions = all 28 instantiations at 2^16 .. 2^22 points"""
    from gnss_sdr_rs_amd import fft
    n, b = n1 * n2, M.B(n1, n2)
    run = lambda x: fft.four_step(n1, n2, x.reshape(-1), inverse=inv)
    count = min(64, (1 << 22) // n) if n < 1 << 20 else 2          # (at 2^22 points: four float64 reference transforms in all)
    fails = []
    _held("four-step", f"{n1}x{n2} inv={int(inv)} noise", run, M.noise(n, SEED), b, inv, l2_bar=4e-6, fails=fails)
    _held("four-step", f"{n1}x{n2} inv={int(inv)} impulses", run, M.impulses(n, SEED, count), b, inv, fails=fails)
    _held("four-step", f"{n1}x{n2} inv={int(inv)} tone", run, M.tones(n, SEED, 1), b, inv, fails=fails)
    assert not fails, fails


def test_four_step_refusals_leave_the_buffer_untouched(gpu):
    L = gpu.lib()
    one = np.full(1, 7 - 7j, np.complex64)
    for n1, n2 in ((128, 256), (256, 128), (8000, 256), (256, 16368), (4000, 4000), (384, 256), (256, 257), (32768, 16384),
                   (1 << 20, 1 << 10), (0, 256), (256, 0)):
        for d in (0, 1):
            assert L.gm_debug_fft_four_step(n1, n2, d, _vp(one), 1) == -2, (n1, n2)
    assert L.gm_debug_fft_four_step(256, 256, 0, None, 1) == -1 and L.gm_debug_fft_four_step(256, 256, 0, _vp(one), 0) == -1
    assert one[0] == np.complex64(7 - 7j)


# ---------------------------------------------------------------------------------------------------------------- 3. the public route is that code
@pytest.mark.parametrize("lg", [17, 19, 22, 23])
def test_public_route_runs_the_pair_split_names(gpu, lg):
    """FFT(n).execute gives the words of four_step(*split(n)), bit for bit; 2^23 = 16384 x 512 is the only affordable row plan above
    256 on the public route and the largest length in this file: its noise input is held to the bound as well"""
    from gnss_sdr_rs_amd import fft
    n = 1 << lg
    n1, n2 = M.split(n)
    x = M.noise(n, SEED + lg)
    for inv in ((False, True) if lg < 23 else (False,)):
        pub = fft.FFT(n).execute(x.copy().reshape(-1), inverse=inv)
        named = fft.four_step(n1, n2, x.copy().reshape(-1), inverse=inv)
        assert (pub.view(np.uint32) == named.view(np.uint32)).all(), (n, inv)
        if lg == 23:
            ref = M.reference(x, inv)
            eob, l2 = M.err_over_bound(pub, ref, M.B(n1, n2), x).max(), M.l2_rel(pub, ref).max()
            _note("public 2^23", f"{n1}x{n2} noise", eob, l2)
            assert eob <= 1.0 and l2 < 4e-6


# ---------------------------------------------------------------------------------------------------------------- 4. Bluestein's classes of L
@pytest.mark.parametrize("n", [1, 2, 3, 127, 8191, 8193, 16383, 40000, 100003])
def test_bluestein_length_classes(gpu, n):
    """L in LDS (1, 2, 3, 127, 8191), the 32768 -> 65536 skip (8193, 16383), 2^17 = 512 x 256 (40000), 2^18 (100003); the L2 bars the
    suite had (3e-6 where L is in LDS, 4e-6 where it is a four-step pair) on every input kind — there is no useful per-bin bound"""
    from gnss_sdr_rs_amd import fft
    assert M.path(n) == "bluestein" and n not in fft.supported_sizes()
    bar = 3e-6 if M.bluestein_L(n) in M.POW2_PLANS else 4e-6
    worst = 0.0
    for inv in (False, True):
        for kind, x in (("noise", M.noise(n, SEED, 3)), ("impulses", M.impulses(n, SEED, 3)), ("tones", M.tones(n, SEED, 3))):
            got = fft.FFT(n).execute(x.copy().reshape(-1), inverse=inv)
            l2 = M.l2_rel(got, M.reference(x, inv)).max()
            worst = max(worst, l2)
            _note("bluestein", f"{n} L={M.bluestein_L(n)} inv={int(inv)} {kind}", 0.0, l2)
            assert l2 < bar, (n, inv, kind, l2)
    print(f"[fft_paths] bluestein {n}: worst L2 {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 5. power_spectrum
@pytest.mark.parametrize("n", [256, 8000, 16368, 16384, 1 << 16, 1 << 17, 1 << 20, 1023])
def test_power_spectrum(gpu, n):
    """in LDS, four-step (2^20 > 256 * 2048: power_kernel's grid-stride loop runs more than once) and Bluestein (1023)"""
    from gnss_sdr_rs_amd import fft
    for kind, x in (("noise", M.noise(n, SEED + 2)), ("mixture", M.mixture(n, SEED + 2))):
        ref = M.reference(x)[0]
        buf = x[0].copy()
        p = fft.FFT(n).power_spectrum(buf)
        words = fft.FFT(n).execute(x[0].copy())
        assert (buf.view(np.uint32) == words.view(np.uint32)).all(), (n, kind)       # the returned inout words are execute's
        want = np.abs(ref) ** 2
        if M.path(n) == "bluestein":
            assert np.allclose(p, want, rtol=2e-4, atol=1e-2), (n, kind)
            continue
        eob = (np.abs(p.astype(np.float64) - want) / M.power_bound(M.coeff(n), x, ref[None, :])[0]).max()
        _note("power", f"{n} {kind}", eob)
        assert eob <= 1.0, (n, kind, eob)


# ---------------------------------------------------------------------------------------------------------------- 6. RealFFT
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 1000, 8000, 16368, 65536])
def test_real_fft(gpu, n):
    from gnss_sdr_rs_amd import fft
    r = np.random.default_rng([SEED, n, 6]).standard_normal(n).astype(np.float32)
    m = n // 2 + 1
    out = np.full(2 * (m + 1), np.frombuffer(b"\x5a" * 4, np.float32)[0], np.float32)       # one guard word behind the last output
    assert gpu.lib().gm_rfft_f32(n, _vp(r), _vp(out)) == 0
    assert (out[2 * m:].view(np.uint8) == 0x5A).all()
    got = out[:2 * m].view(np.complex64)
    full = fft.FFT(n).execute(r.astype(np.complex64))
    assert (got.view(np.uint32) == full[:m].view(np.uint32)).all()
    assert (fft.RealFFT(n).execute(r).view(np.uint32) == got.view(np.uint32)).all()
    if M.path(n) == "bluestein":                     # no per-bin bound: the full transform, whose words these are, to Bluestein's L2 bar
        assert M.bluestein_L(n) in M.POW2_PLANS
        l2 = M.l2_rel(full, M.reference(r.astype(np.complex64)[None, :])).max()
        _note("rfft", f"{n} (Bluestein)", 0.0, l2)
        assert l2 < 3e-6, (n, l2)
    else:
        ref = np.fft.rfft(r.astype(np.float64))
        eob = np.abs(got - ref).max() / M.bound(M.coeff(n), r[None, :])[0]
        _note("rfft", f"{n}", eob)
        assert eob <= 1.0, (n, eob)


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(gpu):
    """empty and null arguments, the first length beyond Bluestein, and lengths whose low 32 bits alone name a plan ((1 << 32) + 256,
    + 8000: once truncated to 256 / 8000 by int(n)) — refused by all three entries before anything is allocated or read, so a one-word
    buffer is enough"""
    L = gpu.lib()
    one, pw, rl = np.full(1, 7 - 7j, np.complex64), np.full(1, 7.0, np.float32), np.full(1, 7.0, np.float32)
    assert L.gm_fft_c2c_f32(0, 0, _vp(one), 1) == -1 and L.gm_fft_c2c_f32(256, 0, _vp(one), 0) == -1 and L.gm_fft_c2c_f32(256, 0, None, 1) == -1
    assert L.gm_fft_power_spectrum_f32(0, _vp(one), _vp(pw)) == -1 and L.gm_fft_power_spectrum_f32(256, None, _vp(pw)) == -1
    assert L.gm_fft_power_spectrum_f32(256, _vp(one), None) == -1
    assert L.gm_rfft_f32(0, _vp(rl), _vp(one)) == -1 and L.gm_rfft_f32(256, None, _vp(one)) == -1 and L.gm_rfft_f32(256, _vp(rl), None) == -1
    for n in ((1 << 23) + 1, (1 << 32) + 256, (1 << 32) + 8000, (1 << 63) + 100):
        assert M.path(n) is None
        for d in (0, 1):
            assert L.gm_fft_c2c_f32(n, d, _vp(one), 1) == -2, n
        assert L.gm_fft_power_spectrum_f32(n, _vp(one), _vp(pw)) == -2, n
        assert L.gm_rfft_f32(n, _vp(rl), _vp(one)) == -2, n
    assert one[0] == np.complex64(7 - 7j) and pw[0] == 7.0 and rl[0] == 7.0
