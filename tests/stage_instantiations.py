"""The template instantiations of the eight stage kernels as data: every form the library builds, the rule that takes a shape to the form
it launches, and one chosen shape per form.

A helper module like array_prompt_classes.py, not a test.  Shared by tests/test_stage_instantiations_host.py (CPU: the chosen shapes
cover every form, the plan entries accept exactly what is listed, the parametrisations of the GPU files reach every form, the
premises of the GPU sweep) and by the GPU files: tests/test_gpu_stage_instantiations.py takes the pairs and the sweep's settings from
here, test_gpu_resample.py and test_gpu_ddc.py their added configs, test_gpu_excise.py and test_gpu_excise_block.py the block sizes of
the cases that sweep B.  The channelizer's and the nuller's GPU files keep their own SHAPES; the host test reads them as text.

The launch rules are restated here without reading the kernels' files:

  resample_kernel<FMT, BLEND, OPL>    a lane owns OPL = 4, 2 or 1 outputs for a tile above 512, above 256, or at most 256 outputs (the tile
  ddc_kernel<BLEND, OPL>              is resample_model.tile_outputs); BLEND = PHI % up != 0 (with up dividing PHI the blend weight is 0)
  excise_kernel<PL, FMT, ADAPT>       PL = the plan of the block size B; ADAPT = the handle is in block-adapt mode
  excise_psd_kernel<PL, FMT>          (gm_excisor_adapt_dev)
  channelizer_kernel<M, FMT>          M = the channel count
  nuller_kernel<A, FMT>               A = the antenna count
  stap_kernel<A, NL>, beam_kernel<A, NL>, lcmv_kernel<A, NL>    NL = the lags a wave carries: 1 for L <= 4, else 2 (a wave carries the
                                      lags `wave` and `wave + 4` that are below L, so L = 5, 6, 7 leave 3, 2, 1 waves with one lag)"""
import ddc_model as DM
import resample_model as RM

FORMATS = ("c32", "i8")


# ---- gm_resampler and gm_ddc: (up, down, taps, n_phases) ----------------------------------------------------------------------------------
def opl(tile):
    """the outputs a lane owns in a tile of `tile` outputs"""
    return 4 if tile > 512 else 2 if tile > 256 else 1


def blend(p):
    return p["PHI"] % p["up"] != 0


RESAMPLE_FORMS = [(fmt, b, o) for fmt in FORMATS for b in (False, True) for o in (4, 2, 1)]
DDC_FORMS = [(b, o) for b in (False, True) for o in (4, 2, 1)]


def resample_form(fmt, config):
    p = RM.resolve(*config)
    return (fmt, blend(p), opl(RM.tile_outputs(p)))


def ddc_form(config):
    up, down, taps, phases = config
    p = DM.resolve(DM.MIX, up, down, taps=taps, n_phases=phases)
    return (blend(p), opl(RM.tile_outputs(p)))


# tiles of 1024, 620 -> 512 and 480 -> 256 outputs without the blend; 1024, 732 -> 512 (T = 192) and 288 -> 256 with it
RESAMPLE_BLEND_2, RESAMPLE_BLEND_1 = (3, 16, 0, 0), (3, 40, 256, 256)
RESAMPLE_CHOSEN = {(False, 4): (1, 1, 8, 16), (False, 2): (4, 25, 0, 0), (False, 1): (1, 8, 256, 256),
                   (True, 4): (3, 2, 32, 256), (True, 2): RESAMPLE_BLEND_2, (True, 1): RESAMPLE_BLEND_1}
# tiles of 1024, 620 -> 512 (4/25 at its default 224 taps: 4 divides 256) and 240 outputs without the blend; 1024, 512 and 256 with it
DDC_PLAIN_2 = (4, 25, 0, 0)
DDC_CHOSEN = {(False, 4): (1, 2, 0, 0), (False, 2): DDC_PLAIN_2, (False, 1): (1, 16, 256, 0),
              (True, 4): (20460, 40919, 0, 0), (True, 2): RESAMPLE_BLEND_2, (True, 1): RESAMPLE_BLEND_1}
# what the GPU files add to their CONFIGS: the forms their lists did not hold
RESAMPLE_ADDED = [RESAMPLE_BLEND_2, RESAMPLE_BLEND_1]
DDC_ADDED = [RESAMPLE_BLEND_2, RESAMPLE_BLEND_1, DDC_PLAIN_2]


# ---- gm_excisor: the block size B ------------------------------------------------------------------------------------------------------
BLOCKS = (256, 512, 1024, 2048, 4096)
EXCISE_FORMS = [("Plan%d" % B, fmt, adapt) for B in BLOCKS for fmt in FORMATS for adapt in (False, True)]
EXCISE_PSD_FORMS = [("Plan%d" % B, fmt) for B in BLOCKS for fmt in FORMATS]


def excise_plan(B):
    assert B in BLOCKS
    return "Plan%d" % B


def excise_form(B, fmt, block_adapt):
    """the kernel of a process call on a handle of block size B, in block-adapt mode or not"""
    return (excise_plan(B), fmt, bool(block_adapt))


def excise_psd_form(B, fmt):
    """the kernel of an adapt call"""
    return (excise_plan(B), fmt)


# a shape is (B, format, mode) itself; what runs them is the GPU files' parametrisations, which the host test reads: every case of
# test_gpu_excise.py's words and adapt tests and of test_gpu_excise_block.py's masks tests runs both formats
BLOCK_ADAPT_SWEPT = (256, 512, 1024, 2048)   # the masks test's block sizes (factor 16 and 6, guard 0, 2, 16)
BLOCK_ADAPT_TOP = ((4096, "i8"), (4096, "c32"))    # the largest block's own cases (factor 16, guard 2)


# ---- gm_channelizer: (M, decim, taps per branch); gm_nuller: (A, B) -------------------------------------------------------------------
CHANNEL_COUNTS = (4, 8, 16, 32, 64)
CHANNELIZER_FORMS = [(M, fmt) for M in CHANNEL_COUNTS for fmt in FORMATS]
CHANNELIZER_CHOSEN = [((4, 3, 4), fmt) for fmt in FORMATS] + [((8, 4, 16), fmt) for fmt in FORMATS] + \
                     [((16, 5, 32), fmt) for fmt in FORMATS] + [((32, 9, 16), fmt) for fmt in FORMATS] + [((64, 18, 16), fmt) for fmt in FORMATS]


def channelizer_form(shape, fmt):
    return (shape[0], fmt)


A_MIN, A_MAX, L_MAX, M_MAX = 2, 8, 8, 32
NULLER_FORMS = [(A, fmt) for A in range(A_MIN, A_MAX + 1) for fmt in FORMATS]
NULLER_CHOSEN = [((A, 256), fmt) for A in range(A_MIN, A_MAX + 1) for fmt in FORMATS]


def nuller_form(shape, fmt):
    return (shape[0], fmt)


# ---- gm_stap, gm_beamformer, gm_lcmv: (A, L) ------------------------------------------------------------------------------------------------
# every (A, L) with 2 <= A <= 8, 1 <= L <= 8, A L <= 32: 8 + 8 + 8 + 6 + 5 + 4 + 4
PAIRS = [(A, L) for A in range(A_MIN, A_MAX + 1) for L in range(1, L_MAX + 1) if A * L <= M_MAX]
assert len(PAIRS) == 43


def lags_per_wave(L):
    """NL"""
    return 1 if L <= 4 else 2


def array_form(A, L):
    assert (A, L) in PAIRS
    return (A, lags_per_wave(L))


# more than four taps only at A <= 6: 7 + 5 forms, the same for the three stages
ARRAY_FORMS = [(A, 1) for A in range(A_MIN, A_MAX + 1)] + [(A, 2) for A in range(A_MIN, 7)]
STAP_FORMS = BEAM_FORMS = LCMV_FORMS = ARRAY_FORMS
# L = 3 (three waves with a lag, one without); L = 7 where A allows it (wave 3 has one lag, the others two), else the most taps of A
ARRAY_CHOSEN = [(A, 3) for A in range(A_MIN, A_MAX + 1)] + [(2, 7), (3, 7), (4, 7), (5, 6), (6, 5)]

SWEEP_BLOCK = 256                     # the smallest block: one chunk of 256 time samples
SWEEP_N = 3 * SWEEP_BLOCK + 7         # three blocks, then a pending tail
SWEEP_STEP = 300                      # the second run's call length: calls that end at 300, 600 and 775, so blocks 1 and 2 are each begun
                                      # by one call (44 and 88 pending samples, with their halos) and finished by the next
SWEEP_LOADING = 1e-4
BEAM_ROWS = 5                         # a full group of four beams and a partial one


def sweep_seed(A, L):
    """the seed of the stap's and the beamformer's stream of a pair (test_gpu_stap.py's recipe at B = 256)"""
    return 100 * A + L + SWEEP_BLOCK % 97


def lcmv_qs(M):
    """the constraint counts of the sweep's three beams, each <= min(8, M) and all different wherever M allows it: the most that
    leaves the beam half of its freedoms, two (three where that is the first count), and one.  M = 3: half of the freedoms is one row,
    so the last beam takes all three (a fully constrained beam).  M = 2 admits the counts 1 and 2 only: [1, 2, 1], the one pair with two
    different counts."""
    big = max(1, min(8, M // 2))
    return [big, 3 if big == 2 else 2, 3 if M == 3 else 1]


def lcmv_case(A, L):
    """the sweep's case of a pair in lcmv_model.CASES' form: lcmv_model.drawn(case) gives its constraints"""
    return (A, L, SWEEP_BLOCK, lcmv_qs(A * L))
