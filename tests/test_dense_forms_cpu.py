"""CPU: the premises of tests/test_gpu_dense_forms.py, none of which needs a device.

  * completeness - every instantiation the macros compile (tests/dense_forms.py: 34 wave forms, 8 runs forms, D = 1..6
    generic) is selected by at least one case as the smoother and one as the score form, and no case selects a form
    that is not compiled;
  * dispatch - the transcription of the host's dispatch in tests/dense_forms.py against the library's host-only size
    queries eks_smooth_workspace_bytes / eks_nll_workspace_bytes, under each case's knobs and under the two knobs that
    remove an organisation (EKS_DENSE_TREE_SCAN, EKS_DENSE_LEGACY): the query equals the transcribed layout of the
    transcribed path, and changes exactly where the path does;
  * reference - on every case's inputs the oracle's covariance-form smoother and its information-form smoother agree
    to 1e-8 in the suite's relative measure (and so does the C oracle where the GPU test uses it, K > 1000): three
    decades below the kernels' 1e-5 bar, which makes that bar a statement about the kernel."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import eks_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_forms as df  # noqa: E402
from dense_forms import CASES, SCORE, SMOOTH  # noqa: E402

REFERENCE_BAR = 1e-8


def test_every_compiled_form_is_selected_by_a_case_in_both_modes():
    hit = {SMOOTH: set(), SCORE: set()}
    for c in CASES:
        for mode, form in c.forms().items():
            if form is None:
                assert mode == SCORE and c.T < 2, c
                continue
            assert df.compiled(form), (c, mode, form)
            hit[mode].add(form)
    for mode in (SMOOTH, SCORE):
        wave = {f for f in hit[mode] if f[0] == 'wave'}
        runs = {f[1:3] for f in hit[mode] if f[0] == 'runs'}
        gen = {f[1] for f in hit[mode] if f[0] == 'generic'}
        print(f'mode {mode}: {len(wave)} wave forms, {len(runs)} runs forms, generic D {sorted(gen)}')
        assert wave == set(df.WAVE_FORMS) and len(wave) == 34, set(df.WAVE_FORMS) ^ wave
        assert runs == set(df.RUNS_FORMS) and len(runs) == 8, set(df.RUNS_FORMS) ^ runs
        assert gen == set(df.GENERIC_D), gen
    # the run-time chunk length of the runs kernels: one to eight checkpoints per lane, and two lengths in between
    assert {f[3] for f in hit[SMOOTH] if f[0] == 'runs'} == {4, 12, 16, 28, 32}


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_case_selects_the_form_it_is_meant_for(case):
    forms = case.forms()
    assert forms[SMOOTH] == case.form
    assert forms[SCORE] == (case.form if case.T >= 2 else None)


def test_the_shapes_have_the_edges_they_are_there_for():
    by = {}
    for c in CASES:
        by.setdefault(c.group, []).append(c)
    for c in by['wave1']:      # two units per keypoint, the second with its last (or only) chunk ragged
        B = c.form[4]
        assert df.dw_units(c.T, c.K, B) == 2 * c.K and c.T % B != 0 and -(-c.T // B) in (65, 66)
    for c in by['wave2']:      # an odd number of units (a spare pair), or two units per keypoint
        units = df.dw_units(c.T, c.K, 8)
        assert 256 < units <= 1024 and (units % 2 == 1 or units == 2 * c.K)
    for c in by['wave1many'] + by['waveknob']:
        assert df.dw_units(c.T, c.K, 8) == 257
    for c in by['waveknob']:   # the forced chunk alone would need more units than one-pair workgroups take
        assert df.dw_units(c.T, c.K, int(c.knobs['EKS_DW_CHUNK'])) > df.DW_UNITS_PAIR
    for c in by['runs'] + by['genericmany']:
        assert df.dw_units(c.T, c.K, 8) > df.DW_UNITS_MAX
    assert any(c.T % c.form[3] % 4 != 0 for c in by['runs'])                 # a ragged group of a checkpointed lane
    assert {c.T for c in by['runs']} >= {1, 3}


def _query(lib, c, n_cand=None):
    from eks_amd import _lib
    d = _lib.EksDims(c.K, c.T, c.D, c.O, 0)
    if n_cand is None:
        return int(lib.eks_smooth_workspace_bytes(ctypes.byref(d)))
    return int(lib.eks_nll_workspace_bytes(ctypes.byref(d), n_cand))


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_transcribed_dispatch_is_the_librarys(case, set_knob):
    from eks_amd import _lib
    lib = _lib.load()
    c = case
    for name, value in c.knobs.items():
        set_knob(name, value)
    base = _query(lib, c)
    assert base == df.smooth_workspace_bytes(c.T, c.K, c.D, c.O, c.knobs) > 0
    if c.form[0] == 'wave' and c.O <= 8:   # the layout of the chunk length that is launched, not of one the knob asked for
        assert base == df.dw_layout_bytes(c.T, c.K, c.D, c.form[4])
    elif c.form[0] == 'wave':  # five / six cameras keep 8 frames inside a workspace sized without looking at O
        assert base == df.dw_layout_bytes(c.T, c.K, c.D, df.dw_chunk_frames(c.T, c.K, 0, c.knobs)) \
            >= df.dw_layout_bytes(c.T, c.K, c.D, 8)
    # the score form shares the smoother's workspace; eks_nll asks for the larger of that and the dual-number tree's
    score = _query(lib, c, 1)
    set_knob('EKS_DENSE_DUAL_GRAD', '1')
    dual = _query(lib, c, 1)
    set_knob('EKS_DENSE_DUAL_GRAD', None)
    assert score == (max(dual, base) if c.T >= 2 else dual)
    path = c.form[0]
    for knob, moves in (('EKS_DENSE_TREE_SCAN', path == 'runs'), ('EKS_DENSE_LEGACY', path in ('wave', 'runs'))):
        set_knob(knob, '1')
        kn = dict(c.knobs, **{knob: '1'})
        got = _query(lib, c)
        set_knob(knob, None)
        assert got == df.smooth_workspace_bytes(c.T, c.K, c.D, c.O, kn)
        assert df.dense_path(c.T, c.K, c.D, c.O, kn) == ('generic' if moves else path)
        assert (got != base) == moves, (knob, got, base)


def test_forced_short_chunk_holds_only_where_its_kernels_exist(set_knob):
    """EKS_DW_CHUNK = 2 / 4 with more units than the one-pair workgroups take: the call runs 8 frames per lane, and the
    size query follows the launch (it used to follow the knob while the 8-frame kernels were launched)."""
    from eks_amd import _lib
    lib = _lib.load()
    size = lambda T, K: int(lib.eks_smooth_workspace_bytes(ctypes.byref(_lib.EksDims(K, T, 3, 4, 0))))    # noqa: E731
    for forced in ('2', '4'):
        set_knob('EKS_DW_CHUNK', forced)
        B = int(forced)
        assert size(9, 257) == df.dw_layout_bytes(9, 257, 3, 8) != df.dw_layout_bytes(9, 257, 3, B)
        assert size(64 * B * 2, 128) == df.dw_layout_bytes(64 * B * 2, 128, 3, B)           # 256 units: the knob holds
        assert size(64 * B * 2 + 1, 128) == df.dw_layout_bytes(64 * B * 2 + 1, 128, 3, 8)   # 384 units at B: 8 frames


_REF_MEMO = {}


def reference(case):
    """(ms_o, Vs_o) of orc.kalman_smoother on the case's inputs, computed once per case."""
    if case.id not in _REF_MEMO:
        arrs, _, _, s = case.problem()
        Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
        _REF_MEMO[case.id] = orc.kalman_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                                                 arrs['Qs'], s, Rd)[:2]
    return _REF_MEMO[case.id]


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_reference_forms_agree_on_the_cases_inputs(case):
    arrs, _, _, s = case.problem()
    Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
    args = (arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s)
    ms_o, Vs_o = reference(case)
    ms_i, Vs_i = orc.info_form_smoother(arrs['ys'], *args, Rd)[:2]
    e_m, e_V = df.rel(ms_i, ms_o, axis_scale=(1, 2)), df.rel(Vs_i, Vs_o, axis_scale=(1, 2, 3))
    line = f'FIGURES {case.id}: information form against covariance form ms {e_m:.2e} Vs {e_V:.2e}'
    if case.K > 1000:          # the reference the GPU test uses at this width
        from oracle import c_oracle
        ms_c, Vs_c, _ = c_oracle.smooth(arrs['ys'], Rd, *args)
        e_mc, e_Vc = df.rel(ms_c, ms_o, axis_scale=(1, 2)), df.rel(Vs_c, Vs_o, axis_scale=(1, 2, 3))
        line += f'; C oracle ms {e_mc:.2e} Vs {e_Vc:.2e}'
        e_m, e_V = max(e_m, e_mc), max(e_V, e_Vc)
    print(line)
    assert e_m < REFERENCE_BAR and e_V < REFERENCE_BAR, line


@pytest.mark.parametrize('D,O', df.WIDE_PAIRS)
def test_float64_reference_forms_agree_at_the_wide_pairs(D, O):
    """tests/test_gpu_smooth_tv.py, _robust, _jumps and _innovations set their float64 bar from the disagreement of a
    sequential and a joint reference form (100 x, capped at 1e-8).  On the inputs those tests use at the wide pairs -
    same models, sessions and lengths - the forms agree to 1e-11: three decades under the cap."""
    pytest.importorskip('torch')                               # (the GPU test modules import it)
    import innovations_ref as iref
    import smooth_tv_ref as tref
    import test_gpu_innovations as ti
    import test_gpu_jumps as tj
    import test_gpu_robust as tr
    from test_gpu_increments import PARAMS, dense_session, stable
    from test_increments_cpu import dense_case
    from test_smooth_tv_cpu import random_w
    K = 3
    M = stable(dense_case(K, D, O, False, seed=df.general_seed(D, O, K)))
    par = tuple(M[k] for k in PARAMS)

    def apart(a, b, unit_scale=False):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        if unit_scale:
            return float(np.abs(a - b).max())
        scale = np.abs(a).transpose(1, 0, *range(2, a.ndim)).reshape(K, -1).max(axis=1)
        return float((np.abs(a - b) / scale.reshape((1, K) + (1,) * (a.ndim - 2))).max())

    worst = dict(tv=0.0, innovations=0.0, robust=0.0, jumps=0.0)
    for i, T in enumerate((1, 2, 16, 17, 33, 100)):
        y, var = dense_session(M, T, O, seed=T)
        w = random_w(np.random.default_rng(T + K), (T, K) if i % 2 else (T,))
        seq, joint = tref.dense_smooth_tv(y, var, *par, w), tref.dense_smooth_tv_joint(y, var, *par, w)
        worst['tv'] = max(worst['tv'], apart(seq[0], joint[0]), apart(seq[1], joint[1]))
        seq, joint = iref.dense_innovations_sequential(y, var, *par), iref.dense_innovations_joint(y, var, *par)
        scales = ti.dense_scales(seq, y, T, O)
        worst['innovations'] = max([worst['innovations']]
                                   + [float(np.max(np.abs(seq[n] - joint[n]) / scales[n])) for n in seq])
    for T in (1, 2, 17, 33, 100):
        for name, mod, session in (('robust', tr, tr.dense_displaced), ('jumps', tj, tj.dense_jumpy)):
            y, var = session(M, T, O, seed=T)
            seq, joint = mod.dense_refs(M, y, var, 4.0, (1, 3))
            for n in (1, 3):
                third = (1.0 / np.asarray(seq[n][2], np.float64), 1.0 / np.asarray(joint[n][2], np.float64)) \
                    if name == 'jumps' else (seq[n][2], joint[n][2])
                worst[name] = max(worst[name], apart(seq[n][0], joint[n][0]), apart(seq[n][1], joint[n][1]),
                                  apart(*third, unit_scale=True), apart(seq[n][3], joint[n][3], unit_scale=True))
    print(f'FIGURES D={D} O={O}: sequential against joint form ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert max(worst.values()) < 1e-11, worst
