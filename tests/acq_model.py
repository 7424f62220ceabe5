"""A float64 numpy model of the acquisition search, the float32 host fold, and the cases of tests/test_gpu_stage_f_variants.py.

A helper module like rs_api.py, not a test.  Shared by tests/test_acq_model_host.py (CPU: the model against the oracle, the plan-coverage
guard, the scenes' peak gaps) and tests/test_gpu_stage_f_variants.py (GPU: every stage-F copy against the model and, word for word,
against the plain search of the host's fold).

search_model restates the operation, not the kernels: per Doppler bin d, hypothesis h (period offset o) and group m the K periods read
from the starts s[d][o + m K + k] are summed with sec[k] * exp(-j 2 pi f_d (s[d][o + m K + k] - s[d][o + m K]) / fs), multiplied by the
bin's mix table and correlated with every replica by numpy.fft at length N; the M power planes are added.  Scaling and the `sum`
convention are the oracle's (oracle/gnss_oracle.c, orc_search_satellite and orc_is_good_satellite): forward and inverse transforms
without 1/N, power = re^2 + im^2, argmax = the first strict maximum, sum = all N lags of the accumulated plane, the maximum included
(N is a multiple of 8, so chunks_exact(8) drops nothing).  Everything is float64; the only device words it takes are the mix tables."""
import numpy as np

REL = 1e-5          # the project's bound on max and sum for anything that passed through an FFT
GAP = 1e-3          # least relative gap between the largest and the second-largest lag of a scene cell: 100 x REL
FORMATS = ("i8", "real", "c32")


# ---- samples ---------------------------------------------------------------------------------------------------------------------
def as_parts(x):
    """(re, im) float32 arrays of int8 IQ [n][2], int8 real [n] or complex64 [n] samples: what load_sample (acq_device.h) forms"""
    x = np.asarray(x)
    if x.dtype == np.int8 and x.ndim == 2:
        return x[:, 0].astype(np.float32), x[:, 1].astype(np.float32)
    if x.dtype == np.int8:
        return x.astype(np.float32), np.zeros(x.size, np.float32)
    x = x.astype(np.complex64)
    return x.real.astype(np.float32), x.imag.astype(np.float32)


def as_c128(x):
    re, im = as_parts(x)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def convert(x, fmt):
    """a complex128 scene of integers in the sample format `fmt` (the real format keeps the I arm)"""
    if fmt == "i8":
        out = np.empty((x.size, 2), np.int8)
        out[:, 0], out[:, 1] = x.real.astype(np.int8), x.imag.astype(np.int8)
        return out
    if fmt == "real":
        return x.real.astype(np.int8)
    return x.astype(np.complex64)


# ---- period starts and phasors ---------------------------------------------------------------------------------------------------
def plain_starts(D, R, N):
    """[D][R]: period p starts at p N in every bin"""
    return np.broadcast_to(np.arange(R, dtype=np.uint64) * np.uint64(N), (D, R)).copy()


def drift_starts(T, R):
    """[D][R]: s[d][p] = floor(p T_d + 0.5) in float64 (gm_acq_set_code_drift's rule)"""
    t = np.asarray(T, np.float64).reshape(-1)
    return np.floor(np.arange(R, dtype=np.float64)[None, :] * t[:, None] + 0.5).astype(np.uint64)


def phasors_f64(table_freq, fs, starts, K, M, offset=0):
    """[D][M][K] complex128: exp(-j 2 pi f_d (s[d][o + m K + k] - s[d][o + m K]) / fs), the cycles reduced before the angle"""
    s = np.asarray(starts)[:, offset:offset + K * M].astype(np.int64).reshape(-1, M, K)
    delta = (s - s[:, :, :1]).astype(np.float64)
    cyc = np.asarray(table_freq, np.float64)[:, None, None] * delta / np.float64(fs)
    ang = 2.0 * np.pi * (cyc - np.floor(cyc))
    return np.cos(ang) - 1j * np.sin(ang)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def search_model(x, tables, codes, N, K, M, table_freq, fs, starts=None, offsets=None, sec=None, with_gap=False):
    """-> (max, argmax, sum), float64 / int64 / float64 arrays [P][H][D]; with_gap also (max - second-largest lag) / max.
    x: the dwell's samples; tables: [D][N] mix tables; codes: [P][N] replicas as sampled chips; table_freq: [D] IF + Doppler of the
    tables; starts: [D][R] period starts (None: p N); offsets: [H] period offsets of the hypotheses (None: [0]); sec: [K] signs."""
    X = as_c128(x)
    tab = np.asarray(tables).astype(np.complex128)
    D, P = tab.shape[0], len(codes)
    offsets = [0] if offsets is None else [int(o) for o in offsets]
    H = len(offsets)
    if starts is None:
        starts = plain_starts(D, K * M + offsets[-1], N)
    s = np.ones(K, np.float64) if sec is None else np.asarray(sec, np.float64)
    conj_code = np.conj(np.fft.fft(np.asarray(codes, np.float64), axis=1))
    mx, sm, gap = (np.zeros((P, H, D), np.float64) for _ in range(3))
    am = np.zeros((P, H, D), np.int64)
    for h, o in enumerate(offsets):
        rho = phasors_f64(table_freq, fs, starts, K, M, o)
        for d in range(D):
            acc = np.zeros((P, N), np.float64)
            for m in range(M):
                y = np.zeros(N, np.complex128)
                for k in range(K):
                    st = int(starts[d][o + m * K + k])
                    y = y + (s[k] * rho[d, m, k]) * X[st:st + N]
                spec = np.fft.fft(y * tab[d])
                c = np.fft.ifft(spec[None, :] * conj_code, axis=1) * np.float64(N)      # the inverse without 1/N
                acc += c.real * c.real + c.imag * c.imag
            am[:, h, d] = np.argmax(acc, axis=1)
            mx[:, h, d] = acc[np.arange(P), am[:, h, d]]
            sm[:, h, d] = acc.sum(axis=1)
            if with_gap:
                second = np.partition(acc, N - 2, axis=1)[:, N - 2]
                gap[:, h, d] = (mx[:, h, d] - second) / mx[:, h, d]
    return (mx, am, sm, gap) if with_gap else (mx, am, sm)


# ---- the host's float32 fold -------------------------------------------------------------------------------------------------------
def fold(x, N, K, M, rho_dm, starts_d, offset=0, sec=None):
    """[M][N] complex64 folded groups of one bin: period k of group m is the N samples from starts_d[offset + m K + k] on, with
    sec[k] * rho_dm[m][k] as the phasor words — float32 with fold_sample's arithmetic (acq_device.h: separate real arrays, k ascending,
    every product and sum rounded on its own, no fused operations; the multiplication by +-1 is exact).  rho_dm: [M][K], or [K] for
    phasors that do not depend on the group.  test_gpu_code_drift.py's _fold with that one generalisation."""
    xr, xi = as_parts(x)
    rho_dm = np.asarray(rho_dm, np.complex64)
    if rho_dm.ndim == 1:
        rho_dm = np.broadcast_to(rho_dm, (M, K))
    s = np.ones(K, np.float32) if sec is None else np.asarray(sec, np.float32)
    y = np.empty((M, N), np.complex64)
    for m in range(M):
        st = [int(v) for v in starts_d[offset + m * K:offset + (m + 1) * K]]
        rr, ri = s * rho_dm[m].real.astype(np.float32), s * rho_dm[m].imag.astype(np.float32)
        gr, gi = xr[st[0]:st[0] + N], xi[st[0]:st[0] + N]
        are = rr[0] * gr - ri[0] * gi
        aim = rr[0] * gi + ri[0] * gr
        for k in range(1, K):
            gr, gi = xr[st[k]:st[k] + N], xi[st[k]:st[k] + N]
            are = are + (rr[k] * gr - ri[k] * gi)
            aim = aim + (rr[k] * gi + ri[k] * gr)
        y[m].real, y[m].imag = are, aim
    return y


def reduce_block(fmx, fam, fsm):
    """numpy's reduction of a [P][H][D] block: per cell the largest max, the lowest h on ties (np.argmax returns the first)"""
    ch = np.argmax(fmx, axis=1).astype(np.uint32)
    pick = lambda a: np.take_along_axis(a, ch[:, None, :].astype(np.int64), axis=1)[:, 0, :]
    return pick(fmx), pick(fam), pick(fsm), ch


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (fft_size, form, base): one row per (form, base) pair gm_acq_plan_info can return over every multiple of 8 up to 2^18, any_length
# clear and set (confirmed by the walk of test_acq_model_host.py, which fails when a plan is added without a row here).  lds: the
# size is its own base.  composite: the smallest Q x base of each base find_comp can reach (base 4000 is shadowed: 2 x 4000 = 8000
# is an in-LDS size, 3 x 4000 = 12000 too, 4 x 4000 = 2 x 8000, 5 x 4000 = 4 x 5000, 6 x 4000 = 3 x 8000, 8 x 4000 = 2 x 16000).
# long: the smallest native size of each base.  long_padded: 2048 x 3 and q = 1 on every other base.
CASES = [
    (256, "lds", 256), (512, "lds", 512), (1024, "lds", 1024), (2000, "lds", 2000), (2048, "lds", 2048), (4000, "lds", 4000),
    (4096, "lds", 4096), (5000, "lds", 5000), (6000, "lds", 6000), (8000, "lds", 8000), (8184, "lds", 8184), (8192, "lds", 8192),
    (10000, "lds", 10000), (12000, "lds", 12000), (15000, "lds", 15000), (16000, "lds", 16000), (16368, "lds", 16368),
    (16384, "lds", 16384),
    (32768, "composite", 16384), (32736, "composite", 16368), (32000, "composite", 16000), (24000, "composite", 8000),
    (24576, "composite", 8192), (24552, "composite", 8184), (18000, "composite", 6000), (20000, "composite", 5000),
    (6144, "long", 2048), (12288, "long", 4096), (56000, "long", 8000), (57344, "long", 8192), (50000, "long", 10000),
    (112000, "long", 16000), (114688, "long", 16384),
    (3064, "long_padded", 2048), (2040, "long_padded", 4096), (3992, "long_padded", 8000), (4088, "long_padded", 8192),
    (4992, "long_padded", 10000), (7992, "long_padded", 16000), (8176, "long_padded", 16384),
]
STRICT_ROWS = (2048, 18000, 6144, 4088)      # one row per form also runs the identity with strict_sum_order

P, D = 2, 3
PRN_IDS = (5, 6)                             # rows 4 and 5 of the C/A table: both are in every scene
DOP = np.array([-300.0, 0.0, 300.0], np.float32)
SAT_DOPPLER = (130.0, -170.0)                # between the bins
ROW = (1, -1, -1)
# the four variants: (name, K, M, offsets, secondary row, (T_0 - N, T_{d+1} - T_d) or None, index of the first row's sample format)
VARIANTS = (("coherent", 3, 2, None, None, None, 0),
            ("edge", 3, 2, (0, 2), ROW, None, 1),
            ("drift_fold_edge", 3, 2, (0, 2), ROW, (-0.4, 0.3), 2),
            ("drift_k1", 1, 3, None, None, (-3.7, 1.3), 0))


def sample_codes(chips, code_rate, fs, N):
    """[P][N] replicas as sampled chips: chip floor((i as f32 * code_rate) / fs) mod the code length, in float32 as the library and
    the oracle resample a chip sequence"""
    chips = np.asarray(chips, np.int8)
    idx = np.floor((np.arange(N, dtype=np.float32) * np.float32(code_rate)) / np.float32(fs)).astype(np.int64)
    return chips[:, idx % chips.shape[1]]


def case_chips(code_table, N):
    """The handle's two codes: the C/A codes of PRN_IDS; below 1024 samples a period their first N / 2 chips, so that the replica
    still has two samples a chip (at 256 samples a 1023-chip code has four chips a sample: a period read a fraction of a sample off
    correlates with nothing, and no drift scene has a peak)"""
    L = 1023 if N >= 1024 else N // 2
    return np.ascontiguousarray(np.asarray(code_table, np.int8)[[p - 1 for p in PRN_IDS], :L])


# (C/N0 of both satellites in dB-Hz, scene seed) where the rule of scene_choice does not pass the scene check
SCENE_CHOICE = {16000: (60.0, 0), 32000: (60.0, 0), 24576: (60.0, 0), 32768: (68.0, 0), 57344: (76.0, 0), 50000: (58.0, 1),
                112000: (60.0, 2), 114688: (68.0, 3)}


def scene_choice(N):
    """(C/N0 of both satellites, scene seed), chosen per size so that every cell of every variant passes the scene check of
    test_acq_model_host.py: a peak at the simulated code phase at least GAP above the cell's second lag.  One code period is 1 ms
    at every size (fs = 1000 N), so a period's correlation SNR is C/N0 - 30 dB whatever N is, while the amplitude in the int8 samples
    (sigma = 16) falls with N: 56 dB-Hz below 2048 samples, 60 below 4096 and 64 above keep both satellites clear of clipping.
    With many samples a chip a cell whose bin reads the periods a fraction of a sample apart has a flat-topped peak, and what
    separates its two best lags is as much the noise as the code's shape: on the sizes of SCENE_CHOICE the rule's scene leaves some
    cell's gap below 1.5 GAP, and another level or another noise realisation (the first of a fixed list that passes) does not."""
    return SCENE_CHOICE.get(N, (56.0 if N < 2048 else 60.0 if N < 4096 else 64.0, 0))


def build_case(code_table, N, variant, row_index):
    """One variant's scene and arguments on one CASES row, as both test files use it -> dict.
    x: the dwell in its sample format; chips, code_rate: the handle's codes (the replica runs at the scene's chip rate); expect:
    [P][H][D][2] the inclusive window of lags the simulated code phase allows.  variant: an index into VARIANTS, or a tuple of that
    form (its scene then has no entry in the scene check of test_acq_model_host.py)."""
    name, K, M, offsets, sec, drift, f0 = variant if isinstance(variant, tuple) else VARIANTS[variant]
    variant = variant if isinstance(variant, int) else len(VARIANTS) + K
    fs = N * 1000.0
    fmt = FORMATS[(f0 + row_index) % 3]
    offs = [0] if offsets is None else list(offsets)
    R = K * M + offs[-1]
    code_starts = (N - 91, (3 * N) // 7)
    chips = case_chips(code_table, N)
    if drift is None:
        T, starts, t_scene = None, plain_starts(D, R, N), float(N)
    else:
        T = N + drift[0] + drift[1] * np.arange(D)
        starts = drift_starts(T, R)
        t_scene = float(T[1])                                   # the scene's code period is bin 1's
    rate = fs * chips.shape[1] / t_scene
    dwell = int(starts[:, -1].max()) + N
    cn0, seed = scene_choice(N)
    sats = [dict(prn_row=w, cn0_dbhz=cn0, doppler_hz=SAT_DOPPLER[w], code_start=code_starts[w], phase=0.4 + w) for w in range(P)]
    from gnss_sdr_rs_amd import synth
    x = synth.make_scene(chips, fs, 0.0, dwell, sats, config_id=900 + variant + 10 * seed, code_rate=rate)
    # where the code starts inside period p as bin d reads it: e = code_start + p T_scene - s[d][p].  The samples before it belong to
    # the code period before, which began at e - T_scene and which the length-N circular correlation sees at e + (N - T_scene).  A
    # cell's peak lies within one sample of the hull of both over its periods; without the compensation that is the code start itself
    expect = np.zeros((P, len(offs), D, 2), np.int64)
    slack = 0 if drift is None else 1
    for w in range(P):
        for h, o in enumerate(offs):
            for d in range(D):
                p = np.arange(o, o + K * M, dtype=np.float64)
                e = code_starts[w] + p * t_scene - starts[d][o:o + K * M].astype(np.float64)
                expect[w, h, d] = int(np.ceil(e.min() - 1e-9)) - slack, int(np.floor(e.max() + (N - t_scene) + 1e-9)) + slack
    return dict(name=name, N=N, K=K, M=M, fs=fs, fmt=fmt, x=convert(x, fmt), offsets=None if offsets is None else offs,
                sec=None if sec is None else np.asarray(sec, np.int8), T=T, starts=starts, dwell=dwell, expect=expect,
                chips=chips, code_rate=rate, codes=sample_codes(chips, rate, fs, N))
