"""The stage kernels' instantiations on the CPU: the chosen shapes of stage_instantiations.py reach every form of every list, the lists
are the whole products, the host-only plan entries accept exactly the shapes the lists are built from, the parametrisations of the
stages' GPU files (read as syntax trees, not imported) reach every form, and the premises of the GPU sweep
(tests/test_gpu_stage_instantiations.py) hold: its bounds sit below the bars, its second run cuts blocks, its streams take no fallback
block, its constraint draws are well conditioned."""
import ast
import ctypes as C
import itertools
import os
import re

import numpy as np

import lcmv_model as LM
import resample_model as RM
import stage_instantiations as SI
import stap_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _covers(forms, reached, count):
    """every form once in the list, and each of them reached by exactly one chosen shape: none missing, none twice"""
    assert len(forms) == len(set(forms)) == count, (len(forms), count)
    assert sorted(reached) == sorted(forms), (sorted(set(forms) - set(reached)), sorted(set(reached) - set(forms)))


def test_the_chosen_shapes_reach_every_instantiation_once():
    plans = ["Plan%d" % B for B in (256, 512, 1024, 2048, 4096)]
    # the lists are the whole products, written out again
    assert sorted(SI.RESAMPLE_FORMS) == sorted(itertools.product(("c32", "i8"), (False, True), (1, 2, 4)))
    assert sorted(SI.DDC_FORMS) == sorted(itertools.product((False, True), (1, 2, 4)))
    assert sorted(SI.EXCISE_FORMS) == sorted(itertools.product(plans, ("c32", "i8"), (False, True)))
    assert sorted(SI.EXCISE_PSD_FORMS) == sorted(itertools.product(plans, ("c32", "i8")))
    assert sorted(SI.CHANNELIZER_FORMS) == sorted(itertools.product((4, 8, 16, 32, 64), ("c32", "i8")))
    assert sorted(SI.NULLER_FORMS) == sorted(itertools.product(range(2, 9), ("c32", "i8")))
    assert sorted(SI.ARRAY_FORMS) == sorted({(A, 1 if L <= 4 else 2) for A in range(2, 9) for L in range(1, 9) if A * L <= 32})
    _covers(SI.RESAMPLE_FORMS, [SI.resample_form(fmt, c) for fmt in SI.FORMATS for c in SI.RESAMPLE_CHOSEN.values()], 12)
    _covers(SI.DDC_FORMS, [SI.ddc_form(c) for c in SI.DDC_CHOSEN.values()], 6)
    assert len(SI.EXCISE_FORMS) == len(set(SI.EXCISE_FORMS)) == 20 and len(SI.EXCISE_PSD_FORMS) == len(set(SI.EXCISE_PSD_FORMS)) == 10
    _covers(SI.CHANNELIZER_FORMS, [SI.channelizer_form(*s) for s in SI.CHANNELIZER_CHOSEN], 10)
    _covers(SI.NULLER_FORMS, [SI.nuller_form(*s) for s in SI.NULLER_CHOSEN], 14)
    for forms in (SI.STAP_FORMS, SI.BEAM_FORMS, SI.LCMV_FORMS):
        _covers(forms, [SI.array_form(A, L) for A, L in SI.ARRAY_CHOSEN], 12)
    # each chosen config stands under the form it is chosen for
    for (b, o), c in SI.RESAMPLE_CHOSEN.items():
        assert all(SI.resample_form(fmt, c) == (fmt, b, o) for fmt in SI.FORMATS), c
    for form, c in SI.DDC_CHOSEN.items():
        assert SI.ddc_form(c) == form, c
    # and the whole sweep of pairs reaches the same twelve forms, L = 7 and L = 3 among them
    assert {SI.array_form(A, L) for A, L in SI.PAIRS} == set(SI.ARRAY_FORMS)
    assert {(A, 7) for A in (2, 3, 4)} <= set(SI.ARRAY_CHOSEN) <= set(SI.PAIRS) and {A for A, L in SI.PAIRS if L == 7} == {2, 3, 4}


def _gpu_file(name):
    """a GPU file's syntax tree: the files are read as text, since importing one imports torch and the HIP library"""
    with open(os.path.join(ROOT, "tests", name)) as f:
        return ast.parse(f.read())


def _value(node):
    import ddc_model as DM
    return eval(compile(ast.Expression(node), "<gpu file>", "eval"), {"SI": SI, "DM": DM})


def _assigned(tree, name):
    """the value of a module-level `name = ...` (an expression of literals and of stage_instantiations' names)"""
    node, = [n for n in tree.body if isinstance(n, ast.Assign) and [getattr(t, "id", None) for t in n.targets] == [name]]
    return _value(node.value)


def _cases(tree, test, names=None):
    """the cases of `test`'s pytest.mark.parametrize -> a list of values (tuples where it names several arguments); [()] without one"""
    names = names or {}
    fn, = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == test]
    marks = [d for d in fn.decorator_list if isinstance(d, ast.Call) and ast.unparse(d.func) == "pytest.mark.parametrize"]
    if not marks:
        return [()]
    mark, = marks
    return list(eval(compile(ast.Expression(mark.args[1]), "<gpu file>", "eval"), dict(names, SI=SI)))


def _loops_both_formats(tree, test):
    fn, = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == test]
    return any(isinstance(n, ast.For) and sorted(_value(n.iter)) == ["c32", "i8"] for n in ast.walk(fn) if isinstance(n, ast.For)
               and isinstance(n.iter, ast.Tuple) and all(isinstance(e, ast.Constant) for e in n.iter.elts))


def test_the_gpu_files_reach_every_instantiation():
    """the parametrisations of the five stages' own GPU files, read as text, against the lists: dropping a config, a block size, a
    channel count or an antenna count from a GPU file fails here"""
    # gm_resampler, gm_ddc: CONFIGS; the words test of the resampler runs both formats on each
    rs, dd = _gpu_file("test_gpu_resample.py"), _gpu_file("test_gpu_ddc.py")
    rs_configs, dd_configs = [tuple(c) for c in _assigned(rs, "CONFIGS")], [tuple(c) for c in _assigned(dd, "CONFIGS")]
    assert set(SI.RESAMPLE_CHOSEN.values()) <= set(rs_configs) and set(SI.DDC_CHOSEN.values()) <= set(dd_configs)
    assert len(rs_configs) == len(set(rs_configs)) and len(dd_configs) == len(set(dd_configs))
    assert [tuple(c) for c in _cases(rs, "test_words_against_the_model", dict(CONFIGS=rs_configs))] == rs_configs
    assert [tuple(c) for c in _cases(dd, "test_words_against_the_model", dict(CONFIGS=dd_configs))] == dd_configs
    assert _loops_both_formats(rs, "test_words_against_the_model")
    assert {SI.resample_form(fmt, c) for fmt in SI.FORMATS for c in rs_configs} == set(SI.RESAMPLE_FORMS)
    assert {SI.ddc_form(c) for c in dd_configs} == set(SI.DDC_FORMS)
    # gm_excisor: the words test (process, static), the adapt test (PSD), the masks tests (process, block-adapt)
    ex, eb = _gpu_file("test_gpu_excise.py"), _gpu_file("test_gpu_excise_block.py")
    reached = []
    assert _loops_both_formats(ex, "test_words_against_the_model") and _loops_both_formats(eb, "test_masks_and_outputs_against_the_model")
    reached += [SI.excise_form(B, fmt, False) for B in _cases(ex, "test_words_against_the_model") for fmt in SI.FORMATS]
    n_of = _assigned(eb, "N_OF")
    reached += [SI.excise_form(B, fmt, True) for B, n in _cases(eb, "test_masks_and_outputs_against_the_model", dict(N_OF=n_of))
                for fmt in SI.FORMATS]
    reached += [SI.excise_form(B, fmt, True) for B, fmt in _cases(eb, "test_masks_and_outputs_at_the_largest_block")]
    _covers(SI.EXCISE_FORMS, reached, 20)
    psd = [n for n in ast.walk([n for n in ex.body if isinstance(n, ast.FunctionDef) and n.name == "test_adapt"][0])
           if isinstance(n, ast.Constant) and n.value in SI.FORMATS]
    assert {n.value for n in psd} == set(SI.FORMATS)                # test_adapt's list of cases names both formats at every B
    _covers(SI.EXCISE_PSD_FORMS, [SI.excise_psd_form(B, fmt) for B in _cases(ex, "test_adapt") for fmt in SI.FORMATS], 10)
    # gm_channelizer, gm_nuller: their own SHAPES, both formats in the words test
    ch, nl = _gpu_file("test_gpu_channelizer.py"), _gpu_file("test_gpu_nuller.py")
    assert _loops_both_formats(ch, "test_words_against_the_model") and _loops_both_formats(nl, "test_words_against_the_model")
    ch_shapes, nl_shapes = _assigned(ch, "SHAPES"), _assigned(nl, "SHAPES")
    assert {SI.channelizer_form(s, fmt) for s in ch_shapes for fmt in SI.FORMATS} == set(SI.CHANNELIZER_FORMS)
    assert {SI.nuller_form(s, fmt) for s in nl_shapes for fmt in SI.FORMATS} == set(SI.NULLER_FORMS)
    assert {s for s, fmt in SI.CHANNELIZER_CHOSEN} <= set(ch_shapes) and {s for s, fmt in SI.NULLER_CHOSEN} <= set(nl_shapes)


def test_the_tile_rule_is_the_kernels(gm):
    """resample_model.tile_outputs against resample_tile_out of csrc/gm_internal.h for every chosen config.  The rule is RESTATED here
    from the header's text (the span constant and the expression are read out of the file and evaluated in Python integers), not read
    from the library: gm_resampler_plan and gm_ddc_plan do not report the tile."""
    with open(os.path.join(ROOT, "gnss-sdr-rs_amd", "csrc", "gm_internal.h")) as f:
        text = f.read()
    span = int(re.search(r"constexpr int RS_SPAN_MAX = (\d+);", text).group(1))
    body = re.search(r"inline uint32_t resample_tile_out\(uint32_t T, uint32_t up, uint32_t down\) \{(.*?)\n\}", text, re.S).group(1)
    assert "uint64_t(RS_SPAN_MAX - int(T) - 1) * up / down + 1" in body
    assert "n >= 1024 ? 1024u : n >= 512 ? 512u : n >= 256 ? 256u : uint32_t(n)" in body

    def tile_out(T, up, down):
        n = (span - T - 1) * up // down + 1
        return 1024 if n >= 1024 else 512 if n >= 512 else 256 if n >= 256 else n

    from gnss_sdr_rs_amd import ddc, resample
    import ddc_model as DM
    for config in set(SI.RESAMPLE_CHOSEN.values()) | set(SI.DDC_CHOSEN.values()):
        up, down, taps, phases = config
        for p in (RM.resolve(*config), DM.resolve(DM.MIX, up, down, taps=taps, n_phases=phases)):
            assert RM.tile_outputs(p) == tile_out(p["T"], p["up"], p["down"]), config
        # T, up, down and PHI are the library's: the plan entries resolve the defaults as the models do
        p = RM.resolve(*config)
        got = resample.plan(up, down, taps=taps, n_phases=phases)
        assert (got["up"], got["down"], got["taps"], got["n_phases"]) == (p["up"], p["down"], p["T"], p["PHI"]), config
        got = ddc.plan(DM.MIX, up, down, taps=taps, n_phases=phases)
        assert (got["up"], got["down"], got["taps"], got["n_phases"]) == (p["up"], p["down"], p["T"], p["PHI"]), config
    assert RM.tile_outputs(RM.resolve(*SI.RESAMPLE_BLEND_2)) == 512 and RM.resolve(*SI.RESAMPLE_BLEND_2)["T"] == 192
    assert RM.tile_outputs(RM.resolve(*SI.RESAMPLE_BLEND_1)) == 256 and RM.tile_outputs(RM.resolve(*SI.DDC_PLAIN_2)) == 512


def test_the_pairs_are_what_the_three_plan_entries_accept(gm):
    from gnss_sdr_rs_amd import _lib
    L_ = gm.lib()
    e0 = np.zeros(128, np.complex64)
    e0[0] = 1.0
    one = np.ones(1, np.complex64)
    q = np.ones(1, np.uint32)
    accepted = {"stap": [], "beamformer": [], "lcmv": []}
    for A in range(0, 11):
        for L in range(0, 11):
            cfgs = dict(stap=_lib.StapCfg(A, L, 0, 0.0, None, 0), beamformer=_lib.BeamformerCfg(A, L, 0, 0.0, 1, 0, e0.ctypes.data, 0),
                        lcmv=_lib.LcmvCfg(A, L, 0, 0.0, 1, 0, q.ctypes.data, e0.ctypes.data, one.ctypes.data, 0))
            for name, cfg in cfgs.items():
                st = getattr(L_, "gm_%s_plan" % name)(C.byref(cfg), 0, 1000, None, None, None)
                assert st in (0, -1), (name, A, L, st)
                if st == 0:
                    accepted[name].append((A, L))
    for name, pairs in accepted.items():
        assert pairs == SI.PAIRS, name


def test_the_block_sizes_and_channel_counts_are_what_the_plan_entries_accept(gm):
    from gnss_sdr_rs_amd import _lib, channelizer, excise
    blocks = []
    for B in [2 ** k for k in range(5, 15)] + [384, 768, 3072]:
        try:
            assert excise.plan(B)["block"] == B
            blocks.append(B)
        except _lib.GmError as e:
            assert e.status == -1, B
    assert tuple(sorted(blocks)) == SI.BLOCKS
    counts = []
    for M in range(1, 130):
        try:
            channelizer.plan(M, 1)
            counts.append(M)
        except _lib.GmError as e:
            assert e.status == -1, M
    assert tuple(counts) == SI.CHANNEL_COUNTS
    for shape, fmt in SI.CHANNELIZER_CHOSEN:                         # the chosen shapes are accepted as they stand
        assert channelizer.plan(shape[0], shape[1], taps_per_branch=shape[2])["taps_per_branch"] == shape[2]


def test_the_derived_bounds_stay_below_the_bars_for_every_pair():
    for A, L in SI.PAIRS:
        assert SM.derived_R(SI.SWEEP_BLOCK, L) < SM.BAR_R and (A * L + 2) * 2.0 ** -24 < SM.BAR_Y, (A, L)


def test_the_second_run_cuts_blocks():
    """the calls of the sweep's second run end inside blocks 1 and 2, so both are begun by one call and finished by the next"""
    B, n, step = SI.SWEEP_BLOCK, SI.SWEEP_N, SI.SWEEP_STEP
    ends = list(range(step, n, step)) + [n]
    assert len(ends) >= 3 and n // B == 3 and n % B
    cut = {e // B for e in ends[:-1] if e % B}
    assert {1, 2} <= cut, ends


def test_the_sweeps_streams_take_no_fallback_block():
    """for every pair and both formats, the model on the sweep's own stream reports no fallback block, with e_0 and with the
    beamformer's and the constraint rows' solves conditioned as the draws say: the sweep's fallback_blocks == 0 is the model's too"""
    B, n = SI.SWEEP_BLOCK, SI.SWEEP_N
    for A, L in SI.PAIRS:
        for fmt in SI.FORMATS:
            x = SM.stream(fmt, n, A, SI.sweep_seed(A, L))
            if fmt == "i8":
                assert (x == -128).any()
            m = SM.run(SM.resolve(A, L, B, SI.SWEEP_LOADING), x)
            assert m["zb"].shape[0] == 3 and not np.asarray(m["fallback"]).any(), (A, L, fmt)


def test_the_constraint_draws_need_no_redraw():
    """lcmv_model.draw redraws a beam while cond(C^H C) > COND_MAX; the bars of test_gpu_lcmv.py's _check rest on that conditioning.  None
    of the sweep's 43 draws needs a redraw, so each beam is the seed's first draw, and each stands at or below COND_MAX"""
    for A, L in SI.PAIRS:
        case = SI.lcmv_case(A, L)
        M, qs = A * L, case[3]
        assert len(qs) == 3 and all(1 <= Q <= min(8, M) for Q in qs) and sum(qs) <= 16, case
        assert len(set(qs)) == (3 if M >= 3 else 2), case           # M = 2 admits the counts 1 and 2 only
        cs, redraws = LM.drawn(case)
        assert redraws == 0, case
        for rows, f in cs:
            c = rows.astype(np.complex128)
            assert np.linalg.cond(c.conj() @ c.T) <= LM.COND_MAX, case
        for fmt in SI.FORMATS:                                         # and no beam of the sweep's stream falls back
            m = LM.run(LM.resolve(A, L, cs, SI.SWEEP_BLOCK, SI.SWEEP_LOADING), SM.stream(fmt, SI.SWEEP_N, A, LM.case_seed(case)))
            assert m["zb"].shape[0] == 3 and not m["fallback"].any(), (case, fmt)
