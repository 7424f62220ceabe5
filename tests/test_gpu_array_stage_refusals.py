"""The refusals that gm_nuller, gm_stap and gm_beamformer make in one shared host layer (ArrayStage, csrc/gm_api.hip): each one's status
AND the exact gm_last_error text, which the per-handle test_every_refusal_leaves_the_state_alone tests do not read.  The texts are
written out here; they are part of the behaviour, and a change to the shared layer must not move them.

Shape: A = 2, B = 256; taps = 2 for stap and the beamformer, P = 2 beams.  One good process_dev of B + 40 time samples leaves a history
of 40; the refused call would take 2 B more and finish two blocks.  Every case is refused before the device is touched; after the walk
stats() is what it was and the next good call delivers the model's count.  The gm_*_plan refusals need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import beam_model as BM
import nuller_model as NM
import stap_model as SM

INVALID, OUT_OF_RANGE = -1, -5
A, L, B, P = 2, 2, 256, 2
STAGES = ("nuller", "stap", "beamformer")
ROWS = np.array([[1, 0, 0, 0], [0, 1j, 0, 0]], np.complex64)       # the beamformer's [P][L * A] constraint rows


def _last(lib):
    return (lib.gm_last_error() or b"").decode()


def _refused(lib, status, want_status, want_text, what):
    assert (status, _last(lib)) == (want_status, want_text), what


def _open(name):
    """-> (the handle's wrapper, weight words per block, planes, the float64 model's count function)"""
    from gnss_sdr_rs_amd import beamformer, nuller, stap
    if name == "nuller":
        p = NM.resolve(A, B)
        return nuller.Nuller(A, B), A, 1, lambda so_far, n_in: NM.plan(p, so_far, n_in)
    if name == "stap":
        p = SM.resolve(A, L, B)
        return stap.Stap(A, L, B), A * L, 1, lambda so_far, n_in: SM.plan(p, so_far, n_in)
    p = BM.resolve(A, L, ROWS, B)
    return beamformer.Beamformer(A, L, ROWS, B), P * A * L, P, lambda so_far, n_in: BM.plan(p, so_far, n_in)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STAGES)
def test_every_shared_refusal_says_what_it_said(gpu, hipbuf, name):
    from gnss_sdr_rs_amd import _lib
    lib = gpu.lib()
    entry = lambda e: getattr(lib, "gm_%s_%s" % (name, e))
    h, w_words, planes, count = _open(name)
    r_words = A * A if name == "nuller" else (A * L) ** 2
    first, rest = B + 40, 2 * B
    n = first + rest
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((n, A)) + 1j * rng.standard_normal((n, A))).astype(np.complex64)
    stride = n + B
    d_x = hipbuf.upload(x)
    d_y = hipbuf.alloc(planes * stride * 8)
    d_R, d_w = hipbuf.alloc(8 * r_words * 8), hipbuf.alloc(8 * w_words * 8)
    assert h.process_dev(d_x, _lib.FMT_C32, first, d_y, stride) == count(0, first) == B
    state = h.stats()
    assert (state["inputs"], state["outputs"], state["blocks"]) == (first, B, 1)
    cnt = count(first, rest)
    assert cnt == 2 * B
    got = C.c_size_t(77)
    src, out = d_x + first * A * 8, d_y + B * 8
    dev = lambda d_in, fmt, n_in, d_out, cap: entry("process_dev")(h._h, d_in, fmt, n_in, d_out, cap, C.byref(got), None)
    plan_entry = "gm_%s_plan" % name

    _refused(lib, dev(src, 7, rest, out, stride), INVALID, "%s input is interleaved c32 or int8 IQ" % name, "a bad format")
    _refused(lib, dev(src, _lib.FMT_I8_REAL, rest, out, stride), INVALID, "%s input is interleaved c32 or int8 IQ" % name, "real int8")
    _refused(lib, dev(None, _lib.FMT_C32, rest, out, stride), INVALID, "null input", "null input")
    _refused(lib, dev(src, _lib.FMT_C32, rest, None, stride), INVALID, "null output", "null output")
    _refused(lib, dev(src, _lib.FMT_C32, rest, out, cnt - 1), OUT_OF_RANGE,
             "out_cap below the call's output count (%s gives it)" % plan_entry, "out_cap (the beamformer: the stride) one below the count")
    _refused(lib, dev(src, _lib.FMT_C32, (1 << 31) + 1, out, stride), INVALID, "at most 2^31 samples a call, 2^62 a stream", "2^31 + 1")
    h.capture(d_R, d_w, 1)                                          # armed, one block short of the call's two
    _refused(lib, dev(src, _lib.FMT_C32, rest, out, stride), OUT_OF_RANGE, "the capture is smaller than the call's blocks", "capture")
    h.capture(d_R, d_w, 8)
    _refused(lib, dev(src, _lib.FMT_C32, rest, src, stride), INVALID, "d_out overlaps d_in", "d_out at d_in")
    _refused(lib, dev(src, _lib.FMT_C32, rest, src + rest * A * 8 - 8, stride), INVALID, "d_out overlaps d_in", "d_out at the last input word")
    _refused(lib, dev(src, _lib.FMT_C32, rest, src - 8 * ((planes - 1) * stride + cnt - 1), stride), INVALID, "d_out overlaps d_in",
             "the last output word at the first input word")
    for d_r, d_wt in ((d_R, None), (None, d_w)):
        _refused(lib, entry("capture")(h._h, d_r, d_wt, 8), INVALID, "d_R and d_w: both or neither", "capture with one pointer null")
    _refused(lib, entry("capture")(h._h, d_R, d_w, 0), INVALID, "cap_blocks: 0 exactly where the pointers are null", "cap_blocks = 0")
    _refused(lib, entry("capture")(h._h, None, None, 8), INVALID, "cap_blocks: 0 exactly where the pointers are null", "blocks of nothing")
    bad = np.zeros(w_words, np.complex64)
    bad[0] = 1
    for word in (math.nan, complex(0, math.inf)):
        bad[w_words - 1] = word
        _refused(lib, entry("set_weights")(h._h, bad.ctypes.data_as(C.c_void_p)), INVALID, "weights must be finite", word)
    _refused(lib, entry("reset")(h._h, (1 << 62) + 1), INVALID, "input_index above 2^62", "reset above 2^62")
    # the host-buffer entry: its own rule on the rooms for R and w, behind the same checks
    y = np.zeros((planes, stride), np.complex64)
    R, w = np.zeros(r_words, np.complex64), np.zeros(w_words, np.complex64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    host = lambda fmt, n_in, cap, blocks: entry("process")(h._h, vp(x[first:]), fmt, n_in, vp(y), cap, C.byref(got), vp(R), vp(w), blocks)
    _refused(lib, host(_lib.FMT_C32, rest, stride, 1), OUT_OF_RANGE, "cap_blocks below the call's blocks", "cap_blocks below the blocks")
    _refused(lib, host(7, rest, stride, 2), INVALID, "%s input is interleaved c32 or int8 IQ" % name, "a bad format, host form")
    _refused(lib, host(_lib.FMT_C32, rest, cnt - 1, 2), OUT_OF_RANGE, "out_cap below the call's output count (%s gives it)" % plan_entry,
             "out_cap, host form")
    _refused(lib, entry("process_dev")(None, src, _lib.FMT_C32, rest, out, stride, C.byref(got), None), INVALID, "null handle", "null handle")

    assert got.value == 77 and h.stats() == state and not y.any() and not R.any() and not w.any()
    h.capture(None, None, 0)
    assert h.process_dev(src, _lib.FMT_C32, rest, out, stride) == cnt
    h.synchronize()
    h.close()


def _cfg(name, block=B, loading=0.0, steering="default", reserved=0):
    """-> (the ctypes cfg, what it points at)"""
    from gnss_sdr_rs_amd import _lib
    if name == "nuller":
        s = None if isinstance(steering, str) else np.ascontiguousarray(steering, np.complex64)
        return _lib.NullerCfg(A, block, loading, reserved, s.ctypes.data if s is not None else None), s
    if name == "stap":
        s = None if isinstance(steering, str) else np.ascontiguousarray(steering, np.complex64)
        return _lib.StapCfg(A, L, block, loading, s.ctypes.data if s is not None else None, reserved), s
    s = ROWS if isinstance(steering, str) else np.ascontiguousarray(steering, np.complex64)
    return _lib.BeamformerCfg(A, L, block, loading, P, 0, s.ctypes.data, reserved), s


@pytest.mark.parametrize("name", STAGES)
def test_every_plan_refusal_says_what_it_said(gm, name):
    lib = gm.lib()
    n = C.c_uint64(77)
    plan = lambda cfg, so_far=0, n_in=10: getattr(lib, "gm_%s_plan" % name)(cfg, so_far, n_in, None, None, C.byref(n))
    words = A if name == "nuller" else A * L
    zero = np.zeros(words if name != "beamformer" else (P, words), np.complex64)
    if name == "beamformer":
        zero[0, 0] = 1                                              # one good row, one all-zero row
    reserved = "gm_beamformer_cfg.reserved32 and reserved must be 0" if name == "beamformer" else "gm_%s_cfg.reserved must be 0" % name
    _refused(lib, plan(None), INVALID, "null cfg", "null cfg")
    cases = [(dict(reserved=1), reserved),
             (dict(block=1000), "block: a power of two in 256 .. 16384, 0 for the default"),
             (dict(block=128), "block: a power of two in 256 .. 16384, 0 for the default"),
             (dict(loading=math.nan), "loading must be finite"), (dict(loading=math.inf), "loading must be finite"),
             (dict(loading=9e-7), "loading: [1e-6, 1], 0 for the default"),
             (dict(steering=zero), "a steering row is all zero" if name == "beamformer" else "steering is all zero")]
    nan = zero.copy()
    nan.reshape(-1)[0], nan.reshape(-1)[-1] = 1, math.nan
    cases.append((dict(steering=nan), "steering must be finite"))
    for kw, text in cases:
        cfg, keep = _cfg(name, **kw)
        _refused(lib, plan(C.byref(cfg)), INVALID, text, kw)
    ok, keep = _cfg(name)
    for so_far, n_in in (((1 << 62) + 1, 0), (0, (1 << 62) + 1), (1 << 62, 1), ((1 << 64) - 1, 2)):
        _refused(lib, plan(C.byref(ok), so_far, n_in), INVALID, "inputs_so_far + n_in above 2^62", (so_far, n_in))
    assert n.value == 77                                            # nothing written
    assert plan(C.byref(ok), B + 40, 2 * B) == 0 and n.value == 2 * B
