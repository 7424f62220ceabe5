"""The kernel classes of the two array-prompt entries as data: every (A, L) they accept, the tap class a pair launches and the load form
a (format, A, pointer) takes.

A helper module like acq_sweep_model.py, not a test.  Shared by tests/test_array_prompt_classes_host.py (CPU: the pairs against both plan
entries, the coverage of classes and load forms, the exactness premise) and tests/test_gpu_array_prompt_classes.py (GPU: every pair on
both formats and both pointer forms, for gm_acq_array_prompts and gm_trk_array_prompts).

csrc/acq_array.hip and csrc/trk_array.hip build <FMT, A, LC> for 2 formats x the tap classes of every antenna count, and launch by two
rules that are restated here without reading either file:

  tap class   LC = 1, 2 or 4 for L <= 1, 2, 4; above 4 the most taps A allows, min(8, 32 // A).  The tap loop runs to LC behind a uniform
              test against L, so an L below its class is a path of its own.
  load form   a time sample is TS = A * 8 (c32) or A * 2 (int8 IQ) bytes, V the widest power of two <= 16 that divides TS.  Where the
              first byte of a period (a record) is a multiple of V a time sample is TS / V loads of V bytes, else A element loads.  TS is
              a multiple of V, so which of the two runs depends on the stream's base pointer alone."""

A_MIN, A_MAX, L_MAX, M_MAX = 2, 8, 8, 32
FORMATS = ("c32", "i8")
ELEM = {"c32": 8, "i8": 2}                       # bytes of one antenna's element

# every (A, L) with 2 <= A <= 8, 1 <= L <= 8, A L <= 32: 8 + 8 + 8 + 6 + 5 + 4 + 4
PAIRS = [(A, L) for A in range(A_MIN, A_MAX + 1) for L in range(1, L_MAX + 1) if A * L <= M_MAX]
assert len(PAIRS) == 43


def tap_class(A, L):
    """LC of the kernel that (A, L) launches"""
    assert (A, L) in PAIRS
    return 1 if L <= 1 else 2 if L <= 2 else 4 if L <= 4 else min(L_MAX, M_MAX // A)


def widest(ts):
    """V: the widest power of two <= 16 that divides ts"""
    return 16 if ts % 16 == 0 else 8 if ts % 8 == 0 else 4 if ts % 4 == 0 else 2


def load_form(fmt, A, base_aligned):
    """the loads of one time sample: "wide16" (c32: A / 2 float4; int8: one 16-byte load), "wide8" (int8, one 8-byte load),
    "wide4x{TS/4}" (int8, TS / 4 words) or "element" (A element loads).  base_aligned: the stream's first byte is a multiple of V"""
    ts = A * ELEM[fmt]
    v = widest(ts)
    if v <= ELEM[fmt] or not base_aligned:       # V is the element itself (A odd), or the narrow fallback
        return "element"
    return "wide4x%d" % (ts // 4) if v == 4 else "wide%d" % v


def one_element_off_is_narrow(fmt, A):
    """a base pointer one element behind a 16-byte boundary is no multiple of V wherever V is wider than the element"""
    return ELEM[fmt] % widest(A * ELEM[fmt]) != 0


def launches():
    """what the GPU sweep launches: (fmt, A, L, base_aligned) for every pair, format and pointer form (aligned, one element off)"""
    return [(fmt, A, L, aligned) for A, L in PAIRS for fmt in FORMATS for aligned in (True, False)]


# the exactness premise of the sweep's integer cases: int8 IQ samples against a +-1 reference, N = 2048 (acquisition) and n = 4097
# (tracking) terms a sum, each term's |re| + |im| at most 128 + 128
EXACT_TERMS = {"acq": 2048, "trk": 4097}
TERM_MAX = 128 + 128
EXACT_BOUND = 2.0 ** 24 / 1.5                    # the bound the two existing exact tests hold their envelopes to
