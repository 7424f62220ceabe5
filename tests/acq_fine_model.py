"""gm_acq_finer_doppler restated in float64 (numpy only), the scenes its tests run on and the error bound they hold it to.

The entry strips the code from (periods - 1) N samples of the last search's snapshot from the code phase on, removes the snapshot's
mean, zero-pads to n = 8 next_pow2((periods - 1) N) and reports the first index of the maximum of |FFT_n|.  The model does the same
with the mean, the products and the transform in float64 (np.fft.fft on complex128); only the chip index keeps the float32
arithmetic of the kernel and the oracle (acq_model.sample_codes), and the frequency keeps the header's float32 rule.

Scenes are defined by bin index, not by Hz: a satellite is a code row, a code phase and a bin `idx` of the long transform, so that
the peak's row k1 = idx % N1 and column k2 = idx // N1 of the N1 x N2 four-step transform are chosen, not met by chance.
"""
import numpy as np

# (N, periods): the smallest geometry reaching each long-transform size 2^16 .. 2^24 with an in-LDS N ...
GEOMETRIES = [(2048, 4), (2048, 6), (2048, 10), (4096, 10), (8192, 10), (16384, 10), (16384, 18), (16384, 34), (16384, 66)]
# ... and the two where (periods - 1) N is itself a power of two: 2^13 (so 2^16) and 2^21 (so 2^24, the largest accepted)
BOUNDARY = [(2048, 5), (16384, 129)]
FORMATS = ("c32", "i8", "real")

# the power-of-two in-LDS plans (fft_plans.h): N -> (lanes, radices)
POW2_PLANS = {256: (64, (16, 16)), 512: (64, (8, 8, 8)), 1024: (128, (8, 8, 16)), 2048: (256, (8, 16, 16)),
              4096: (256, (16, 16, 16)), 8192: (512, (16, 8, 8, 8)), 16384: (1024, (16, 8, 8, 16))}
# fft_size -> (N1 of the columns, N2 of the rows, row tile of the rows plan): what the host's factor rule reaches
FACTOR_TABLE = {1 << 16: (256, 256, 4), 1 << 17: (512, 256, 4), 1 << 18: (512, 512, 8), 1 << 19: (1024, 512, 8),
                1 << 20: (1024, 1024, 8), 1 << 21: (2048, 1024, 8), 1 << 22: (2048, 2048, 8), 1 << 23: (4096, 2048, 8),
                1 << 24: (4096, 4096, 4)}


def geometries():
    """The eleven (N, periods): one per reachable factor pair, then the two boundary ones"""
    return GEOMETRIES + BOUNDARY


def fft_size_of(N, periods):
    size_use = (periods - 1) * N
    p2 = 1
    while p2 < size_use:
        p2 <<= 1
    return 8 * p2


def factor_pair(n, sizes):
    """gm_api.hip's rule: n = N1 x N2 with both factors power-of-two in-LDS plans, as square as possible, N1 >= N2 >= 256; None where
    no pair exists"""
    lg = n.bit_length() - 1
    if n != 1 << lg:
        return None
    l2 = lg // 2
    while l2 >= 8:
        if (1 << (lg - l2)) in sizes and (1 << l2) in sizes:
            return 1 << (lg - l2), 1 << l2
        l2 -= 1
    return None


def row_tile(N2):
    """FineRows<PL>::RT (acq_kernels.hip) from the plan's lanes and first radix"""
    T, radices = POW2_PLANS[N2]
    per = -(-(N2 // radices[0]) // T) * radices[0]
    if T >= 1024:
        return 1
    return 8 if per <= 8 else 4 if per <= 16 else 2 if per <= 32 else 1


def chip_index(m, code_rate, fs, code_len):
    """floor((f32(m) * f32(code_rate)) / f32(fs)) % code_len: every step rounded to float32, as the kernel and the oracle form it"""
    m = np.asarray(m, np.float32)
    return np.floor((m * np.float32(code_rate)) / np.float32(fs)).astype(np.int64) % int(code_len)


def freq_rule(idx, n, fs):
    """The header's frequency of a peak index, in float32: one_side = ceil((f32(n) + 1) / 2) — at n = 2^24 the sum rounds back to
    2^24 and one_side is 2^23, not 2^23 + 1 —; indices above it are negative frequencies"""
    f = np.float32
    one_side = int(np.ceil((f(n) + f(1.0)) / f(2.0)))
    if idx > one_side:
        return f(-((f(n - idx) * f(fs)) / f(n)))
    return f((f(idx) * f(fs)) / f(n))


def as_complex(x):
    """A snapshot in any of the three formats as complex128 (the real format: imaginary part 0)"""
    x = np.asarray(x)
    if x.dtype == np.int8 and x.ndim == 2:
        return x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    if x.dtype == np.int8:
        return x.astype(np.float64) + 0j
    return x.astype(np.complex128)


def fine_model(x, code_phase, chips, code_rate, fs, periods, N):
    """x: the snapshot as complex128 (at least periods * N samples; the entry reads the first periods * N of them).
    -> dict(mag: |X| float64 [n], peak_index: first index of the maximum, gap: (largest - second largest) / largest, freq_hz: the
    header's rule for peak_index (float32), fft_size: n, size_use, sum_abs: sum |x_n| of the transform's input, mean_abs: the mean
    of |Re s| + |Im s| over the snapshot)"""
    x = np.asarray(x, np.complex128)[:periods * N]
    assert x.size == periods * N
    mean = x.mean()
    size_use = (periods - 1) * N
    n = fft_size_of(N, periods)
    chips = np.asarray(chips, np.float64)
    c = chips[chip_index(np.arange(size_use), code_rate, fs, chips.size)]
    v = np.zeros(n, np.complex128)
    v[:size_use] = (x[code_phase:code_phase + size_use] - mean) * c
    sum_abs = float(np.abs(v[:size_use]).sum())
    mag = np.abs(np.fft.fft(v))
    del v
    k = int(np.argmax(mag))
    top = float(mag[k])
    mag[k] = -1.0
    second = float(mag.max())
    mag[k] = top
    return dict(mag=mag, peak_index=k, gap=(top - second) / top, freq_hz=freq_rule(k, n, fs), fft_size=n, size_use=size_use,
                sum_abs=sum_abs, mean_abs=float((np.abs(x.real) + np.abs(x.imag)).mean()))


def real_gap(mag, k):
    """For the real format |X[k]| = |X[n - k]|: the distance from the maximum to the next value that belongs to neither image"""
    n = mag.size
    keep = [(i, mag[i]) for i in (k, (n - k) % n)]
    top = max(v for _, v in keep)
    for i, _ in keep:
        mag[i] = -1.0
    second = float(mag.max())
    for i, v in keep:
        mag[i] = v
    return (top - second) / top


# ---- scenes -----------------------------------------------------------------------------------------------------------------
AMP, SIGMA = 24.0, 4.0      # three satellites and four sigma of noise stay below 3 * 24 + 16 = 88 < 127: int8 does not clip


def make_scene(n_samples, N, n, sats, codes, code_rate, fs, seed):
    """s[cp + m] = AMP chip(m) exp(2j pi idx m / n) summed over the satellites, plus white noise, over n_samples; m < 0 (before the
    code phase) continues the code one period earlier.  A satellite is dict(row, cp, idx) with an optional `flips`: code periods
    (counted from cp) at whose start the sign turns over — a data-bit edge.  -> complex128"""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples, dtype=np.int64)
    s = SIGMA * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    for sat in sats:
        m = t - sat["cp"]
        chip = np.asarray(codes[sat["row"]], np.float64)[chip_index(np.where(m < 0, m + N, m), code_rate, fs, len(codes[sat["row"]]))]
        sign = np.ones(n_samples)
        for f in sat.get("flips", ()):
            sign[m >= f * N] *= -1.0
        s += AMP * sign * chip * np.exp(2j * np.pi * ((sat["idx"] * m) % n) / n)
    return s


def convert(s, fmt):
    """The complex128 scene in a format the search takes: complex64, int8 [n][2] or int8 [n] (the real part)"""
    if fmt == "c32":
        return s.astype(np.complex64)
    q = lambda a: np.clip(np.rint(a), -127, 127).astype(np.int8)
    if fmt == "i8":
        return np.ascontiguousarray(np.stack([q(s.real), q(s.imag)], axis=1))
    return q(s.real)


def placements(N, periods, fmt):
    """The satellites of one geometry, placed by k1 = idx % N1 and k2 = idx // N1:
    (a) k1 = N1 - 1: the last rows workgroup and the last row of its tile; k2 = 3; code phase 0
    (b) k1 = N1 / 2 + RT, the first row of a tile away from both ends; k2 = N2 - 5, so idx > one_side: a negative frequency;
        code phase N - 1
    (c) k1 = 1 and k2 = 0 (idx below N1); code phase N / 3.  In the real format a cosine one bin from DC and its image share a
        main lobe whose maximum is bin 0, so (c) moves one column on there: k2 = 2.
    At 2^23 and 2^24 only (a) and (b), which keeps the float64 model to a few seconds."""
    n = fft_size_of(N, periods)
    N1, N2, RT = FACTOR_TABLE[n]
    sats = [dict(row=0, cp=0, idx=3 * N1 + N1 - 1), dict(row=1, cp=N - 1, idx=(N2 - 5) * N1 + N1 // 2 + RT)]
    if n < 1 << 23:
        sats.append(dict(row=2, cp=N // 3, idx=(2 * N1 if fmt == "real" else 0) + 1))
    return sats


# seeds of the noise where the first one tried left a satellite's peak less than GAP clear (test_acq_fine_host.py checks every one)
GAP = 1e-3
SEEDS = {}


def case(g, fmt=None):
    """Geometry g of geometries(): (N, periods, fmt, fs, sats, seed).  Without `fmt` the three formats rotate over the geometries, so
    each occurs at a small, a middle and a large size: that is the case the GPU test runs."""
    N, periods = geometries()[g]
    fmt = fmt or FORMATS[g % 3]
    return N, periods, fmt, 1000.0 * N, placements(N, periods, fmt), SEEDS.get((g, fmt), 1000 + g)


def case_scene(g, codes, fmt=None, code_rate=1.023e6):
    N, periods, fmt, fs, sats, seed = case(g, fmt)
    return convert(make_scene(periods * N, N, fft_size_of(N, periods), sats, codes, code_rate, fs, seed), fmt)


# ---- the two special scenes of tests/test_gpu_fine_doppler.py ------------------------------------------------------------------
def custom_case():
    """Another code at the 2^18 geometry: 2046 chips at 2.046 Mchip/s, 2048 samples a period, so a chip is 1.001 samples long and the
    float32 chip index decides nearly every sample.  -> (N, periods, fmt, fs, code_rate, codes [3][2046], sats, seed)"""
    N, periods, code_len, code_rate = 2048, 10, 2046, 2.046e6
    rng = np.random.default_rng(2046)
    codes = np.where(rng.integers(0, 2, (3, code_len)) > 0, 1, -1).astype(np.int8)
    return N, periods, "i8", 1000.0 * N, code_rate, codes, placements(N, periods, "i8"), 1100


def custom_scene():
    N, periods, fmt, fs, code_rate, codes, sats, seed = custom_case()
    return convert(make_scene(periods * N, N, fft_size_of(N, periods), sats, codes, code_rate, fs, seed), fmt)


def edge_case():
    """A coherent handle (K = 3, M = 2: the 2^17 geometry) with the edge search over the offsets 0, 1, 2, so a dwell is 8 periods.
    Satellite A turns its sign over at its period 6: only offset 0 has two clean groups (periods 0-2, 3-5).  B and C turn over at
    their periods 1 and 7: only offset 1 has (periods 1-3, 4-6).  Noise-free, a clean group folds to 3 and one with a turn-over to 1:
    the right offset's power is 9 + 9 against 9 + 1.  The code phases are a few samples, so a turn-over sits at a period's start.
    The one Doppler bin is bin 2660 of the long transform; the satellites are 3, 2 and 4 bins from it (at most 0.19 cycles over a
    coherent group).  -> dict"""
    N, K, M, offsets = 2048, 3, 2, [0, 1, 2]
    n, fs = fft_size_of(N, K * M), 1000.0 * N
    sats = [dict(row=0, cp=5, idx=2657, flips=(6,)), dict(row=1, cp=40, idx=2662, flips=(1, 7)),
            dict(row=2, cp=17, idx=2664, flips=(1, 7))]
    return dict(N=N, K=K, M=M, offsets=offsets, n=n, fs=fs, fmt="i8", sats=sats, seed=1200, doppler_hz=2660 * fs / n,
                chosen=[0, 1, 1])


def edge_scene(codes, code_rate=1.023e6):
    e = edge_case()
    n_samples = (e["K"] * e["M"] + e["offsets"][-1]) * e["N"]
    return convert(make_scene(n_samples, e["N"], e["n"], e["sats"], codes, code_rate, e["fs"], e["seed"]), e["fmt"])


def edge_cell_powers(x, e, sat, chips, code_rate=1.023e6):
    """[H] float64: per offset the non-coherent sum over the M groups of |coherent sum of K periods|^2 at the satellite's own code
    phase and the handle's Doppler bin — the cell of the search whose largest hypothesis the handle reports"""
    N, K, M = e["N"], e["K"], e["M"]
    x = as_complex(x)
    t = np.arange(x.size)
    m = t - sat["cp"]
    c = np.asarray(chips, np.float64)[chip_index(np.where(m < 0, m + N, m), code_rate, e["fs"], len(chips))]
    z = (x * c * np.exp(-2j * np.pi * e["doppler_hz"] / e["fs"] * t)).reshape(-1, N).sum(axis=1)     # one prompt a period
    return np.array([sum(abs(z[o + g * K:o + (g + 1) * K].sum()) ** 2 for g in range(M)) for o in e["offsets"]])


# ---- the error bound of tests/test_gpu_fine_doppler.py (derived in that module's docstring) -----------------------------------
def _tw_weight(R):
    """Roundings, in units of 2^-24, behind the twiddle W^r (r < R) of a pass after the first: the base is a float32 word of a
    float64 cosine / sine (2^-24 in modulus), taken to the power r <= R - 1, through `depth` complex products of the power tree
    (fft_core.h TwPow) of two roundings each"""
    depth = 5 if R > 9 else 4
    return (R - 1) + 2 * depth


def bound_constant(n):
    """c of |device - model| <= c 2^-24 sum |x_n| for one output of the N1 x N2 transform"""
    N1, N2, _ = FACTOR_TABLE[n]
    c = 1                                       # (s - mean) in float32; the product with +-1 is exact
    c += 3 * (n.bit_length() - 1)               # a radix-r butterfly as log2 r radix-2 stages: a sum (1) and a complex product (2)
    for N in (N1, N2):
        c += sum(_tw_weight(R) for R in POW2_PLANS[N][1][1:])
    c += 2 + 2                                  # sincospif (2^-23) and its complex product
    c += 1 + 2                                  # fmaf(x, x, y * y): 2 roundings of the power, 1 of the magnitude; sqrtf
    return c


def mean_depth(n_samples):
    """Float32 roundings of fine_mean_kernel's sum on one result's path: a lane's sequential sum, six shuffle levels, the first lane's
    fifteen sequential additions, the division"""
    return -(-n_samples // 1024) - 1 + 6 + 15 + 1


def bound(model, periods, N):
    """c 2^-24 sum |x_n| + size_use |mean_dev - mean_model|, the second term with the tree sum's own bound per component"""
    u = 2.0 ** -24
    return bound_constant(model["fft_size"]) * u * model["sum_abs"] + model["size_use"] * mean_depth(periods * N) * u * model["mean_abs"]
