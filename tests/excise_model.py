"""A float64 numpy restatement of the FFT-domain narrowband interference excision (gm_excisor, include/gnss_mi355x.h), and its scene.

A helper module like resample_model.py, not a test.  Shared by tests/test_excise_host.py (CPU: gm_excisor_plan and gm_excisor_windows
against it, the model's own properties, the scenes that motivate the entry) and tests/test_gpu_excise.py (GPU: the device's words
against it).

The model restates the definition, not the kernel.  B the block length, H = B / 2:
    windows        wa[i] = sin(pi i / B), ws[i] = sin(pi i / B) / B
    total_out(A) = H max(0, A div H - 1)                                    outputs that exist after A inputs
    block b        covers absolute inputs [(b - 1) H, (b + 1) H): u_b = B ifft(g fft(wa xb))   (numpy's ifft divides by B)
    output n       s = n div H, i = n mod H:  y[n] = ws[i + H] u_s[i + H] + ws[i] u_{s+1}[i]
    xb = the input after blanking (float32: re*re + im*im > thr*thr, each product and the sum rounded on its own), zero before the
    stream's first sample.
    psd            block j covers [j H, j H + B), J = (n - B) div H + 1:  P[k] = sum_j |fft(wa block_j)[k]|^2
    detect         med = the element of rank (B - 1) div 2; flag = P > factor med; g = 0 within guard bins (circular) of a flag
Indices are Python integers; everything else is float64 (detect keeps the dtype it is given: float32 words give the device's own
product and comparison).  Model.process takes the windows and gains as given: a GPU test hands it the library's own words."""
import numpy as np

BLOCKS = (256, 512, 1024, 2048, 4096)
DEFAULT_BLOCK, DEFAULT_FACTOR = 1024, 4.0
INDEX_MAX = 1 << 62


# ---- the settings ------------------------------------------------------------------------------------------------------------------
def resolve(block=0, guard_bins=0, threshold_factor=0.0, blank_threshold=0.0, reserved=(0, 0, 0, 0)):
    """gm_excisor_plan's argument rules and defaults -> dict, or None where they say GM_ERR_INVALID_ARG"""
    if any(reserved) or (block and block not in BLOCKS) or not (0 <= guard_bins <= 16):
        return None
    if not (threshold_factor == 0.0 or threshold_factor > 1.0) or not (blank_threshold >= 0.0):
        return None
    return dict(B=block or DEFAULT_BLOCK, guard=guard_bins, factor=float(np.float32(threshold_factor)) or DEFAULT_FACTOR,
                thr=np.float32(blank_threshold))


def windows(B):
    """(wa, ws) float64 [B] each (the library rounds each word once to float32)"""
    s = np.sin(np.pi * np.arange(B, dtype=np.float64) / B)
    return s, s / B


def total_out(B, A):
    H = B // 2
    return H * max(0, A // H - 1)


def plan(B, inputs_so_far, n_in):
    """the number of outputs n_in more inputs deliver, or None where the sum exceeds 2^62"""
    if inputs_so_far > INDEX_MAX or n_in > INDEX_MAX or inputs_so_far + n_in > INDEX_MAX:
        return None
    return total_out(B, inputs_so_far + n_in) - total_out(B, inputs_so_far)


# ---- the stream --------------------------------------------------------------------------------------------------------------------
def as_c128(x):
    """complex samples, or int8 interleaved I/Q ([n][2] or flat), as complex128 — what the device's conversion to float32 holds"""
    x = np.asarray(x)
    if x.dtype == np.int8:
        v = x.reshape(-1, 2).astype(np.float64)
        return v[:, 0] + 1j * v[:, 1]
    return x.astype(np.complex64).astype(np.complex128)


def blank(x, thr):
    """-> (xb, how many were blanked): float32 arithmetic, strictly greater"""
    thr = np.float32(thr)
    if not thr > 0:
        return x, 0
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    hit = (re * re + im * im) > thr * thr
    return np.where(hit, 0.0, x), int(hit.sum())


class Model:
    def __init__(self, p, wa=None, ws=None, gains=None, input_index=0):
        self.p, self.B = p, p["B"]
        w = windows(self.B)
        self.wa = np.asarray(w[0] if wa is None else wa, np.float64)
        self.ws = np.asarray(w[1] if ws is None else ws, np.float64)
        self.g = np.ones(self.B) if gains is None else np.asarray(gains, np.float64)
        self.reset(input_index)

    def reset(self, input_index=0):
        self.base, self.inputs, self.outputs, self.blanked = int(input_index), 0, 0, 0
        self.hist = np.zeros(3 * (self.B // 2), np.complex128)

    def process(self, x):
        """one call -> (y complex128 [n_out], scale float64 [n_out]): scale = max |xb| over the two blocks an output comes from, what
        the bound of the device's float32 transforms is stated in"""
        B, H = self.B, self.B // 2
        xb, nb = blank(as_c128(x), self.p["thr"])
        A = self.base + self.inputs
        m0, m1 = total_out(B, A), total_out(B, A + xb.size)
        ext = np.concatenate([self.hist, xb])                    # ext[0] is absolute input A - 3H
        self.hist = ext[-3 * H:].copy()
        self.inputs += xb.size; self.outputs += m1 - m0; self.blanked += nb
        if m1 == m0:
            return np.zeros(0, np.complex128), np.zeros(0)
        s0, s1 = m0 // H, m1 // H
        off = A - 3 * H
        first = (s0 - 1) * H - off
        assert first >= 0 and (s1 + 1) * H - off <= ext.size
        blocks = np.stack([ext[first + k * H:first + k * H + B] for k in range(s1 - s0 + 1)])       # blocks s0 .. s1
        u = np.fft.ifft(self.g[None, :] * np.fft.fft(self.wa[None, :] * blocks, axis=1), axis=1) * B
        y = self.ws[None, H:] * u[:-1, H:] + self.ws[None, :H] * u[1:, :H]
        mag = np.abs(ext[first:first + (s1 - s0 + 2) * H]).reshape(-1, H).max(axis=1)                # per half block
        scale = np.maximum(np.maximum(mag[:-2], mag[1:-1]), mag[2:])
        return y.reshape(-1), np.repeat(scale, H)


def run(p, x, wa=None, ws=None, gains=None, blocks=None, input_index=0):
    """the whole stream x through a fresh Model, in one call or cut into `blocks` (a block length, repeated) -> (y, scale, model)"""
    m = Model(p, wa, ws, gains, input_index)
    x = as_c128(x)
    step = x.size if not blocks else blocks
    ys, ss = [], []
    for s in range(0, max(x.size, 1), max(step, 1)):
        y, sc = m.process(x[s:s + step])
        ys.append(y); ss.append(sc)
    return np.concatenate(ys), np.concatenate(ss), m


def process(p, x, gains=None):
    """y alone, the model's own windows"""
    return run(p, x, gains=gains)[0]


def psd(p, x, wa=None):
    """[B] float64 Welch periodogram of the samples given (blanked by the same rule), or None where n < B"""
    B, H = p["B"], p["B"] // 2
    xb, _ = blank(as_c128(x), p["thr"])
    if xb.size < B:
        return None
    wa = windows(B)[0] if wa is None else np.asarray(wa, np.float64)
    J = (xb.size - B) // H + 1
    P = np.zeros(B)
    for j in range(J):
        X = np.fft.fft(wa * xb[j * H:j * H + B])
        P += X.real * X.real + X.imag * X.imag
    return P


def detect(P, factor, guard):
    """-> (med, flag bool [B], gains [B] of P's dtype): arithmetic in P's own dtype"""
    P = np.asarray(P)
    B = P.size
    med = np.sort(P)[(B - 1) // 2]
    level = P.dtype.type(factor) * med
    flag = P > level
    zero = np.zeros(B, bool)
    for d in range(-guard, guard + 1):
        zero |= np.roll(flag, d)
    return med, flag, np.where(zero, 0, 1).astype(P.dtype)


# ---- the scene: a CW carrier (and pulses) on top of a C/A-like signal in noise ---------------------------------------------------------
N, FS = 2048, 2.048e6
PERIODS = 10
DOP = np.array([0.0, 500.0, 1000.0, 1500.0, 2000.0])
SAT = dict(worker=0, code_phase=700, doppler=1000.0, phase=0.7, cn0=45.0, bin=2)
CW_HZ = 123456.7
N_IN = (PERIODS + 1) * N            # one more period: the excisor's outputs lag its inputs by up to B
DWELL = PERIODS * N


def scene_codes(seed=7):
    """[2][1023] random +-1 chips: worker 0 is in the scene, worker 1 is not"""
    return np.where(np.random.default_rng(seed).integers(0, 2, (2, 1023)) > 0, 1, -1).astype(np.int8)


def scene(seed, jn_db=None, pulses=False):
    """complex64 [N_IN] at baseband: worker 0's code from code_phase on at Doppler 1 kHz and 45 dB-Hz, unit-variance-per-component noise,
    a CW at CW_HZ of jn_db above the noise power (None: no CW) and, with pulses, 40 samples of amplitude 300 every 5000 samples"""
    chips = scene_codes()
    rng = np.random.default_rng(seed)
    n = np.arange(N_IN, dtype=np.float64)
    u = (n - SAT["code_phase"]) / N
    chip = chips[SAT["worker"]][np.minimum(1022, np.floor((u - np.floor(u)) * 1023.0).astype(np.int64))].astype(np.float64)
    amp = np.sqrt(2.0 * 10.0 ** (SAT["cn0"] / 10.0) / FS)
    cyc = SAT["doppler"] * n / FS
    x = amp * chip * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 1j * SAT["phase"])
    x = x + rng.standard_normal(N_IN) + 1j * rng.standard_normal(N_IN)
    if jn_db is not None:
        cyc = CW_HZ * n / FS
        x = x + np.sqrt(2.0 * 10.0 ** (jn_db / 10.0)) * np.exp(2j * np.pi * (cyc - np.floor(cyc)) + 0.3j)
    if pulses:
        for s in range(1234, N_IN - 40, 5000):
            x[s:s + 40] += 300.0 * np.exp(1j * 0.9)
    return x.astype(np.complex64)


def scene_tables(fs=FS):
    """[5][N] complex128 mix tables exp(-j 2 pi f n / fs) of the bins DOP (f_if = 0), and their frequencies"""
    n = np.arange(N, dtype=np.float64)
    return np.exp(-2j * np.pi * DOP[:, None] * n[None, :] / fs), DOP.astype(np.float32)


def sampled_codes(chips):
    import acq_model as AM
    return AM.sample_codes(chips, 1023.0 * FS / N, FS, N)


def best_cell(mx, am, sm, w):
    """(bin, arg-max, peak-to-mean) of worker w's best cell of [P][1][D] (or [P][D]) blocks"""
    mx, am, sm = (np.asarray(a).reshape(2, -1) for a in (mx, am, sm))
    ratio = mx[w].astype(np.float64) * N / sm[w].astype(np.float64)
    d = int(np.argmax(ratio))
    return d, int(am[w][d]), float(ratio[d])


def search(x):
    """the plain search of the first DWELL samples -> best_cell of the true worker"""
    import acq_model as AM
    tabs, tf = scene_tables()
    return best_cell(*AM.search_model(np.asarray(x)[:DWELL], tabs, sampled_codes(scene_codes()), N, 1, PERIODS, tf, FS), SAT["worker"])


def found(cell):
    return cell[0] == SAT["bin"] and cell[1] == SAT["code_phase"]


def excise(x, block=1024, factor=4.0, guard=2, blank_threshold=0.0):
    """adapt on the whole of x, then process: -> (the first DWELL outputs complex64, bins zeroed)"""
    p = resolve(block, guard, factor, blank_threshold)
    _, _, g = detect(psd(p, x), p["factor"], p["guard"])
    y = process(p, x, g)
    assert y.size >= DWELL
    return y[:DWELL].astype(np.complex64), int((g == 0).sum())
