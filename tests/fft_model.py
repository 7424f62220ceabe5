"""A float64 model of FFT<T> / RealFFT<T> (gm_fft_c2c_f32, gm_fft_power_spectrum_f32, gm_rfft_f32): which path a length takes, a
worst-case rounding bound per bin derived from csrc/fft_core.h, and the inputs the path tests feed.  numpy only, no GPU.

Which path.  RADICES restates csrc/fft_plans.h (tests/test_fft_model_host.py parses the header against it).  `split` restates
gm_api.hip pow2_split: the SMALLEST N2 in 256, 512, ... with N1 = n / N2 >= N2 and N1 an in-LDS power-of-two plan (<= 16384).
`bluestein_L` restates fft_bluestein's choice: the smallest power of two >= max(256, 2n - 1) that is a plan or has a split
(32768 = 256 x 128 has neither: 65536 then), at most 2^24.

The bound.  u = 2^-24 (unit roundoff of float32, round to nearest; FMA rounds once).  Claim, to first order in u, for every bin k
of a transform the library runs in LDS or as a four-step pair:

        | device[k] - float64[k] |  <=  B * u * sum_n |x_n|          (modulus, hence also each component)

Everything below is in the MODULUS of complex values: E(z) is a bound on |computed z - exact z| in units of u.  Rules:
  (R1) componentwise operations with real constants (add, subtract, fma(c, t, p) with |c| <= 1, times +-1, +-j, -0.5): the rounding of
       each component is <= u |component|, so as a vector <= u |z|:   E(z) <= E(x) + E(y) + 1 * |z|.  A rounded real constant errs by
       <= u relatively: one more |c t| <= |t|.  (No factor sqrt(2) arises: the two components' roundings are the two components of ONE
       vector of modulus <= u |z|.)
  (R2) cf_mul(a, b) = (fma(ax, bx, -(ay by)), fma(ax, by, ay bx)): the two inner products err by <= u |ay| |b| as a vector, the two
       fmas by <= u |a b|:   E(a b) <= E(a) |b| + |a| E(b) + 2 |a b|.
  (R3) a constant float(cos), float(sin) of a double: each component within 2^-25, so E <= 1 / sqrt(2) (< 1).

Induction over the passes.  After pass s every value v depends on a set S(v) of P(s+1) inputs and |v| <= m(v) := sum of |x_n| over
S(v); a butterfly's r inputs have DISJOINT sets whose union is S(output); every coefficient on the way has modulus <= 1, and every
intermediate z of a butterfly is bounded by the m of the inputs it depends on.  Errors already present reach an output through the
exact linear map with weights of modulus 1: they add (their product with a rounding is second order).  So if a butterfly computes
every output with E <= K m(output) from exact inputs, then E(v) <= C_s m(v) with C_s = C_{s-1} + K(r_s) (+ the twiddle term below).

K(r) of the register butterflies, read from fft_core.h by R1 - R3.  Operands with disjoint input sets cost max(K_x, K_y) + 1; operands
that depend on the SAME inputs (the "even" and "odd" halves of the radix-3, radix-5 and prime butterflies) cost K_x + K_y + 1:
  Dft<2> 1.   Dft<4> 2: t0 = u0 + u2, t2 = u1 + u3 (1 each, disjoint), t0 +- t2 (2).
  Dft<3> 6: m = fma(-0.5, u1 + u2, u0): 2;  js = s3 * (u1 - u2): the difference, the product, s3 itself: 3;  m +- js share u1, u2: 2 + 3 + 1.
  Dft<5> 9: t_j 1;  a = fma(c, t2, fma(c, t1, u0)): inner fma max(1 + 1 for c1, 0) + 1 = 3, outer max(1 + 1 for c2, 3) + 1 = 4;
        b = fma(s, t4, s * t3): s * t3 is 1 + 1 + 1 = 3, the fma max(3, 1 + 1) + 1 = 4;  a +- jb share u1 .. u4: 4 + 4 + 1.
  DftPrime<R> (R = 11, 31; H = (R-1)/2) 2H + 5: a_j, b_j 1;  ca: a chain of H fmas over disjoint pairs, the first max(0, 1 + 1) + 1 = 3
        and one more each: H + 2;  sb likewise H + 2;  ca +- j sb share every input: 2 (H + 2) + 1.
  DftCT<A, B> (8 = 2 x 4, 16 = 4 x 4, 25 = 5 x 5, 32 = 4 x 8): K(A) + 3 + K(B); the inner twiddle is cf_mul by a rounded constant (R2, R3: 3).
  DftPFA<A, B> (10 = 2 x 5, 20 = 4 x 5, 24 = 3 x 8, 33 = 3 x 11): K(A) + K(B), no inner twiddle.
  => K: 2:1 3:6 4:2 5:9 8:6 10:10 11:15 16:7 20:11 24:12 25:21 31:35 32:11 33:21.   (Bfly<R>, the two-stage form the passes call, runs
  the same sub-butterflies and the same inner twiddles; the fused-twiddle forms are not what these entries instantiate.)

Twiddles between passes (every pass but the first), Fft::gather_stage1 with TwPow<R>: input r is multiplied by w^r, and w^r is built
from ONE table value w^1 by products w^a w^b (baby steps, giant steps, then G[g] * Bp[b]).  With e(r) = E(w^r): e(1) = 1/sqrt(2) (R3),
e(a + b) = e(a) + e(b) + 2 (R2), so e(r) = (2 + 1/sqrt(2)) r - 2 whatever the tree's shape — the rounding of w^1 is multiplied by r,
which is what makes this term larger than the butterflies'.  Applying it is one more product (2):
        T(R) = e(R - 1) + 2 = (2 + 1/sqrt(2)) (R - 1)        per pass s >= 1, relative to |input| (and sum |inputs| <= m).

        B(plan) = sum_s K(r_s)  +  sum_{s >= 1} T(r_s).

This is MORE than a count of (r_s + 8) roundings per pass (e.g. 16384 = [16, 8, 8, 16]: 104.5 against 80; 16368 = [33, 16, 31]:
184.8 against 104; test_fft_model_host.py asserts B >= that count for every plan): the butterflies are shallower than r, but the
power tree of the twiddles multiplies the table value's rounding by up to r - 1, which a count of "one twiddle product" misses, and
the prime butterflies' two halves share their inputs.  B is derived from the code as above, never from observed errors.

Four-step pair (big_cols_kernel of p1, big_rows_kernel of p2): the same induction across both transforms, plus the twiddle
W_L^{n2 k1} between them.  t = n2 k1 mod L is an integer; float(t) is exact for L <= 2^24, inv_l = 2 / L is a power of two, so the
argument of sincospif is exact.  sincospif within 2 ulp per component (<= 2 sqrt(2) in modulus) and one product (R2: 2): < 5.
        B(p1, p2) = B(p1) + B(p2) + 8          (8: a round figure that covers the 4.83 derived here)
Above L = 2^24 float(t) rounds (t has up to 28 bits) and the twiddle's phase carries that rounding: not covered by B, and not tested
(the public lengths 2^25 .. 2^28 are too large for a test; their kernels run in the pair matrix at 2^16 .. 2^22 points).

Inverse transforms: the same expressions with conjugated constants, the same B.  Round trip inverse(forward(x)) against n x: the forward
error (<= B u |x|_1 per bin) is summed over n bins with unit weights, and the inverse's own rounding is B u |X^|_1 <= B u n |x|_1:
together 2 B u n |x|_1 — "twice the bound" of an input of 1-norm n |x|_1.

Not in the model: terms of second order in u (below B u ~ 2e-5 of the bound), the float64 reference's own error (~1e-16 log n relative),
underflow (the inputs here stay far from it).

Power spectrum: with e the bound above on |X^ - X|, | |X^|^2 - |X|^2 | <= 2 |X| e + e^2, and v.x v.x + v.y v.y in float32 errs by at
most 3 u |X^|^2 whether or not the compiler contracts it:   |P^ - P| <= 2 |X| e + e^2 + 3 u (|X| + e)^2.

Bluestein has no useful bound of this form: the chirp convolution works on a sequence whose 1-norm is about 2n times the input's.
"""
import math

import numpy as np

U = 2.0 ** -24

# csrc/fft_plans.h: N -> (lanes T, radices)
RADICES = {
    8000: (512, (25, 20, 16)), 16368: (768, (33, 16, 31)), 8184: (768, (11, 31, 8, 3)), 4096: (256, (16, 16, 16)),
    2048: (256, (8, 16, 16)), 1024: (128, (8, 8, 16)), 4000: (256, (25, 16, 10)), 10000: (1024, (10, 10, 10, 10)),
    12000: (768, (20, 25, 24)), 16000: (1024, (25, 20, 32)), 2000: (128, (25, 10, 8)), 5000: (256, (25, 20, 10)),
    6000: (256, (25, 24, 10)), 8192: (512, (16, 8, 8, 8)), 15000: (768, (25, 25, 24)), 16384: (1024, (16, 8, 8, 16)),
    512: (64, (8, 8, 8)), 256: (64, (16, 16)),
}
POW2_PLANS = tuple(sorted(n for n in RADICES if n & (n - 1) == 0))          # 256 .. 16384: the factors of a four-step pair
K = {2: 1, 3: 6, 4: 2, 5: 9, 8: 6, 10: 10, 11: 15, 16: 7, 20: 11, 24: 12, 25: 21, 31: 35, 32: 11, 33: 21}
FOUR_STEP_TWIDDLE = 8.0


def _k(r):
    """K(r) from the factorisation fft_core.h uses (Fac<R> / Dft<R>), so that the table above is checked, not trusted"""
    leaf = {2: 1, 3: 6, 4: 2, 5: 9}
    if r in leaf:
        return leaf[r]
    if r in (11, 31):
        return 2 * ((r - 1) // 2) + 5
    ct = {8: (2, 4), 16: (4, 4), 25: (5, 5), 32: (4, 8)}
    pfa = {10: (2, 5), 20: (4, 5), 24: (3, 8), 33: (3, 11)}
    if r in ct:
        return _k(ct[r][0]) + 3 + _k(ct[r][1])
    return _k(pfa[r][0]) + _k(pfa[r][1])


assert all(_k(r) == k for r, k in K.items())


def twiddle_term(r):
    return (2.0 + 1.0 / math.sqrt(2.0)) * (r - 1)


def B(*plans):
    """the bound coefficient of one in-LDS plan B(n), or of a four-step pair B(n1, n2)"""
    assert len(plans) in (1, 2)
    b = FOUR_STEP_TWIDDLE if len(plans) == 2 else 0.0
    for n in plans:
        rs = RADICES[n][1]
        b += sum(K[r] for r in rs) + sum(twiddle_term(r) for r in rs[1:])
    return b


def first_order_count(*plans):
    """the first-order count the bound started from: (r + 8) per pass, + 8 for the four-step twiddle (B must not be below it)"""
    return sum(r + 8 for n in plans for r in RADICES[n][1]) + (8 if len(plans) == 2 else 0)


def split(n):
    """gm_api.hip pow2_split: (N1, N2) or None"""
    if n < 2 or n & (n - 1) or n > 1 << 28:
        return None
    n2 = 256
    while n2 * n2 <= n or n2 <= 16384:
        if n % n2 == 0:
            n1 = n // n2
            if n1 < n2:
                break
            if n1 in POW2_PLANS and n2 in POW2_PLANS:
                return n1, n2
        n2 *= 2
    return None


def bluestein_L(n):
    """gm_api.hip bluestein_len: Bluestein's transform length for n, or None above 2^23"""
    if n > 1 << 23:
        return None
    L = 256
    while L < 2 * n - 1:
        L *= 2
    while L <= 1 << 24 and L not in POW2_PLANS and split(L) is None:
        L *= 2
    return L if L <= 1 << 24 else None


def path(n):
    """'lds', 'four_step', 'bluestein' or None — the order gm_fft_c2c_f32 decides in"""
    if n in RADICES:
        return "lds"
    if split(n):
        return "four_step"
    return "bluestein" if n >= 1 and bluestein_L(n) else None


def coeff(n):
    """B of the public route of length n (in-LDS or four-step)"""
    return B(n) if n in RADICES else B(*split(n))


# ---------------------------------------------------------------------------------------------------------------- inputs
def noise(n, seed, batch=1):
    rng = np.random.default_rng([seed, n, 1])
    return (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))).astype(np.complex64)


def impulse_positions(n, seed, count):
    # the first ones must be informative alone: n - 1 has the largest index in both factors of a four-step pair (the largest twiddle
    # phases n2 k1 / L), n // 3 a generic one
    fixed = [n - 1, n // 3, 1, 0, 2, n - 2, n // 2]
    rng = np.random.default_rng([seed, n, 2])
    pos = []
    for p in fixed + [int(v) for v in rng.integers(0, n, max(count, 1) * 2 + 8)]:
        p %= n
        if p not in pos:
            pos.append(p)
    return pos[:min(count, n)]


def impulses(n, seed, count=64):
    """one unit impulse per batch item (height 1 + 0.5j so that both components are exercised)"""
    pos = impulse_positions(n, seed, count)
    x = np.zeros((len(pos), n), np.complex64)
    x[np.arange(len(pos)), pos] = 1.0 + 0.5j
    return x


def tone_bins(n, seed, count):
    rng = np.random.default_rng([seed, n, 3])
    rand = [int(v) for v in rng.integers(0, n, max(count, 1) * 2 + 8)]
    bins = []
    for k in rand[:1] + [n // 2, 1, n - 1, 0] + rand[1:]:        # a random bin first: a batch of one is a generic tone
        k %= n
        if k not in bins:
            bins.append(k)
    return bins[:min(count, n)]


def tones(n, seed, count=16):
    """unit tones exp(+2 pi j k m / n) at integer bins k, rounded to float32 from a float64 phase reduced in integers"""
    bins = tone_bins(n, seed, count)
    m = np.arange(n, dtype=np.int64)
    return np.stack([np.exp(2j * np.pi * ((k * m) % n) / n) for k in bins]).astype(np.complex64)


def mixture(n, seed):
    """one impulse plus one tone at 2^-6 of its height"""
    rng = np.random.default_rng([seed, n, 4])
    p, k = int(rng.integers(0, n)), int(rng.integers(0, n))
    m = np.arange(n, dtype=np.int64)
    x = (2.0 ** -6) * np.exp(2j * np.pi * ((k * m) % n) / n)
    x[p] += 1.0
    return x.astype(np.complex64)[None, :]


# ---------------------------------------------------------------------------------------------------------------- reference and checks
def reference(x, inverse=False):
    """np.fft of the exact float32 words in complex128 (the inverse not normalised, like the library's)"""
    xd = np.asarray(x).astype(np.complex128)
    return np.fft.ifft(xd, axis=-1) * xd.shape[-1] if inverse else np.fft.fft(xd, axis=-1)


def l1(x):
    return np.abs(np.asarray(x).astype(np.complex128)).sum(axis=-1)


def bound(b, x):
    """per batch item: B u |x|_1"""
    return b * U * l1(x)


def err_over_bound(got, ref, b, x, factor=1.0):
    """the largest |got - ref| (modulus) over the bins of each batch item, over that item's bound; <= 1 passes"""
    d = np.abs(np.asarray(got).astype(np.complex128).reshape(ref.shape) - ref).max(axis=-1)
    return d / (factor * bound(b, x))


def l2_rel(got, ref):
    """relative L2 error per batch item"""
    g = np.asarray(got).astype(np.complex128).reshape(ref.shape)
    return np.linalg.norm(g - ref, axis=-1) / np.linalg.norm(ref, axis=-1)


def power_bound(b, x, ref):
    """per bin: 2 |X| e + e^2 + 3 u (|X| + e)^2 with e = B u |x|_1"""
    e = bound(b, x)[..., None]
    a = np.abs(ref)
    return 2 * a * e + e * e + 3 * U * (a + e) ** 2


def wrong_reference(ref, n):
    """the float64 transform with one twiddle index off by one in the last pass: output bin k times exp(2 pi j / n) for k in one residue
    class of the last radix (in-LDS sizes)"""
    out = np.array(ref, np.complex128)
    rl = RADICES[n][1][-1]
    out[..., 1::rl] *= np.exp(2j * np.pi / n)
    return out
