"""tests/guard_bands.py without a GPU: the carve arithmetic, and that the check it serves can fail.

1. Alignment classes: for align 1, 2, 4, 8 the payload's address is an odd multiple of align (an int8 IQ stream starts on an odd
   sample, a complex64 one on an odd word), for 16 ... 256 a multiple; at every base hipMalloc can return (multiples of 256).
2. The payload's last byte is directly followed by guard, its first directly preceded by guard or pad, both at least 64 KiB of fill;
   a smaller guard is refused.
3. The overlap rule of the entries that refuse aliasing (d_out inside, across either end of, or equal to d_in; right behind it is no
   overlap: tests/test_gpu_resample.py's refusal cases), and that separately carved buffers never overlap.
4. A numpy stand-in of a symmetric FIR stage with a history buffer, run over a carved host array under the three fills: the correct
   one gives the same words under all of them; one that takes a sample at index n, one that takes its newest history sample from
   index -1 of the input instead of from the history buffer, and one that multiplies the word at index n by a zero weight each differ
   from their fill-0x00 words under a non-zero fill.  The zero weight shows why 0xFF is among the fills: 0 * 3.39e38 = 0, 0 * NaN is not.
5. same_words itself: bits, not values (NaN = NaN, -0.0 != 0.0), shapes and types.
6. The acquisition scenes of tests/test_gpu_guard_bands.py that tests/test_acq_model_host.py does not hold (K = 1 on two periods of the
   coherent scene; coherent K = 2, edge and drift at K = 2): in the float64 model every cell's peak is at least acq_model.GAP above its
   second lag, so the arg-max the GPU test compares cannot turn on float32 rounding, and it lies in the scene's window in every cell of
   test_gpu_guard_bands.acq_window."""
import numpy as np
import pytest

import guard_bands as GB

T = 9                                    # taps of the stand-in: y[i] = sum_j c[j] s[i - j], s = history (T - 1 samples) then the input
C = np.array([1, -2, 3, -4, 5, -4, 3, -2, 1], np.float32) / 8


def test_alignment_classes_and_flush_ends():
    for base in (0, 256, 0x7F0000001000, 0x7F0000001100, 0x7FFFFFF00):
        for align in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            for n in (0, 1, 7, 8, 4096, 4097):
                pad, total = GB.layout(base, n, align)
                addr = base + GB.GUARD + pad
                assert addr % align == 0 and pad < 2 * align and total == 2 * GB.GUARD + pad + n
                if align < 16:
                    assert addr % (2 * align) == align                   # aligned to align and to nothing larger
                    assert addr // align % 2 == 1                        # "an odd element"
                payload = np.arange(n, dtype=np.uint8) | 1
                for fill in GB.FILLS:
                    buf, off = GB.carve_host(payload, fill, align=align, base=base)
                    assert buf.size == total and off == GB.GUARD + pad
                    assert (buf[off:off + n] == payload).all()
                    assert (buf[:off] == fill).all() and off >= GB.GUARD                     # 64 KiB and the pad in front
                    assert (buf[off + n:] == fill).all() and buf.size - (off + n) == GB.GUARD  # the guard starts at the byte behind
    with pytest.raises(AssertionError):
        GB.layout(0, 16, 8, guard=4096)                                  # the guards do not shrink
    with pytest.raises(AssertionError):
        GB.layout(0, 16, 3)


def test_the_overlap_rule_and_separate_allocations():
    src, rest, n2 = 0x7F0000010008, 1500, 2250                          # an input of 1500 words, an output of 2250
    for d_out in (src, src + 8, src - 8 * (n2 - 1), src + rest * 8 - 8):
        assert GB.overlap(src, rest * 8, d_out, n2 * 8), d_out - src
    for d_out in (src + rest * 8, src - 8 * n2):                         # right behind, right in front
        assert not GB.overlap(src, rest * 8, d_out, n2 * 8)
    assert not GB.overlap(src, 0, src, 8) and not GB.overlap(src, 8, src, 0)
    # carved buffers as an allocator hands them out: behind each other, each with its guards
    base, carved = 0x7F0000000000, []
    for n, align in ((100, 1), (4096, 8), (0, 2), (33, 16)):
        pad, total = GB.layout(base, n, align)
        carved.append(GB.Carved(base, pad, np.zeros(n, np.uint8), 0xFF, GB.GUARD))
        base += -(-total // 256) * 256
    assert GB.disjoint(*carved)
    for i, a in enumerate(carved):
        for b in carved[i + 1:]:
            assert not GB.overlap(a.base, a.total, int(b), b.nbytes) and not GB.overlap(int(a), a.nbytes, int(b), b.nbytes)
            assert abs(int(a) - int(b)) >= GB.GUARD                    # a read of less than a guard past one never meets another
    assert not GB.disjoint(carved[0], carved[0])


def _stage(buf, off, n, hist, variant):
    """the stand-in over the float32 words at byte `off` of buf: n inputs, the T - 1 samples before them in `hist` -> n outputs"""
    assert off % 4 == 0 and buf.size % 4 == 0
    mem, first = buf.view(np.float32), off // 4
    x = lambda i: mem[first + i]                                         # no bounds: the guard is there to be read
    y = np.zeros(n, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            acc = np.float32(0)
            for j in range(T):
                k = i - j
                if k >= 0:
                    s = x(k)
                elif variant == "history from in[-1]" and k == -1:
                    s = x(-1)                                            # right in one cut buffer, where in[-1] is the stream's past
                else:
                    s = hist[T - 1 + k]
                acc += C[j] * s
            if variant == "sample n" and i == n - 1:
                acc += C[0] * x(n)                                       # a halo one sample too long
            if variant == "zero weight" and i == n - 1:
                acc += np.float32(0) * x(n)
            y[i] = acc
    return y


VARIANTS = ("correct", "sample n", "history from in[-1]", "zero weight")


def _runs(variant, align=4):
    rng = np.random.default_rng(3)
    n = 40
    x, hist = rng.standard_normal(n).astype(np.float32), rng.standard_normal(T - 1).astype(np.float32)
    runs = {}
    for fill in GB.FILLS:
        buf, off = GB.carve_host(x, fill, align=align)
        runs[fill] = _stage(buf, off, n, hist, variant)
        assert (buf[:off] == fill).all() and (buf[off + 4 * n:] == fill).all()
    return runs


def _fails(runs):
    try:
        GB.same_words(runs)
    except AssertionError:
        return True
    return False


def test_the_check_can_fail():
    ok = _runs("correct")
    GB.same_words(ok)
    want = ok[0x00]
    for variant in VARIANTS[1:]:
        runs = _runs(variant)
        # under the zero fill two of the three are the correct words: what the suite's zero-filled allocations let through
        caught = [f for f in GB.FILLS[1:] if _fails({0x00: runs[0x00], f: runs[f]})]
        assert caught, variant
        assert _fails(runs), variant
        print("%-22s zero fill gives the correct words: %s; caught under %s" % (
            variant, bool((runs[0x00].view(np.uint32) == want.view(np.uint32)).all()), [hex(f) for f in caught]))
    assert [f for f in GB.FILLS[1:] if _fails({0: _runs("zero weight")[0], f: _runs("zero weight")[f]})] == [0xFF]
    for align in (8, 16):
        GB.same_words(_runs("correct", align))
        assert _fails(_runs("sample n", align))


def test_same_words_compares_bits_shapes_and_types():
    nan = np.array([np.nan, 1.0], np.float32)
    GB.same_words({0: nan, 255: nan.copy(), 127: nan.copy()})
    GB.same_words({0: (nan, np.int32(3)), 255: (nan.copy(), np.int32(3))})
    GB.same_words({0: dict(a=nan, b=7), 255: dict(b=7, a=nan.copy())})
    assert _fails({0: np.float32([0.0]), 255: np.float32([-0.0])})
    assert _fails({0: np.zeros(4, np.float32), 255: np.zeros(4, np.int32)})
    assert _fails({0: np.zeros(4, np.float32), 255: np.zeros(3, np.float32)})
    assert _fails({0: dict(a=nan), 255: dict(b=nan)})
    assert _fails({0: (nan, 3), 255: (nan, 4)})
    assert _fails({0: nan})


def _scene_check(oracle, c, N, K, M, x):
    import acq_model as AM
    import test_acq_model_host as TH
    import test_gpu_guard_bands as TG
    tables = TH._tables(oracle, N * 1000.0, N)
    tf = np.array([t.doppler_freq_hz for t in tables], np.float32)
    assert (tf == AM.DOP).all()
    starts = None if c["T"] is None and not c["offsets"] and K * M * N == len(x) else c["starts"]
    mx, am, sm, gap = AM.search_model(x, np.stack([t.table for t in tables]), c["codes"], N, K, M, tf, c["fs"], starts, c["offsets"],
                                      c["sec"], with_gap=True)
    inside = (am >= c["expect"][..., 0]) & (am <= c["expect"][..., 1])
    assert (inside | ~TG.acq_window(c)).all(), (N, c["name"], am)
    assert (gap >= AM.GAP).all(), (N, c["name"], gap)
    return TG.acq_window(c)


def test_the_acquisition_scenes_of_the_gpu_file_have_clean_peaks(oracle):
    import acq_model as AM
    import test_gpu_guard_bands as TG
    for form in TG.ACQ_FORMS:
        N = AM.CASES[TG._acq_row(form)][0]
        for f in range(3):
            c = dict(AM.build_case(oracle.ca_code_table(), N, 0, f), name="plain")
            assert _scene_check(oracle, c, N, 1, 2, c["x"][:2 * N]).all()
    for form in ("lds", "long"):
        N = AM.CASES[TG._acq_row(form)][0]
        for mode in TG.ACQ_MODES:
            c = AM.build_case(oracle.ca_code_table(), N, mode, 0)
            w = _scene_check(oracle, c, N, c["K"], c["M"], c["x"])
            assert w.all() == (c["name"] != "coherent") and w.mean() >= 0.5        # the coherent fold keeps half of its cells
