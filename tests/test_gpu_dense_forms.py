"""GPU: the general-model kernels, one compiled form per case (tests/dense_forms.py has the dispatch, the list of
instantiations and the case table; tests/test_dense_forms_cpu.py shows that the table reaches every instantiation in
both modes and that the references used here agree among themselves to 1e-8).

Per case, with the case's knobs set:
  smoother - hip_ops.smooth with full Vs and with vs_diag against orc.kalman_smoother (the C oracle where K > 1000), at
             the project's bar: 1e-5 of the keypoint's largest magnitude on ms and on Vs, every keypoint, frame and entry;
  score    - (T >= 2) hip_ops.nll(per_keypoint, want_grad, EKS_FLAG_Q_PD) against orc.filter_nll's value and forward-mode
             gradient at 1e-8 relative / 1e-7 of max |g|, and against the dual-number kernels (flags = 0) at 1e-10 / 1e-7;
  form     - one profiled call: the wave kernels report summarize and replay scopes and no scan, the runs and generic
             kernels all three; the workspace the call is given is exactly the queried size, which equals the
             transcribed layout of the transcribed path (guards around it stay intact);
  bits     - a second call gives the same bits, and so does a call whose workspace held 0xFF bytes.
Each case prints its worst figures before it asserts."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import eks_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_guard as bg  # noqa: E402
import dense_forms as df  # noqa: E402
from dense_forms import CASES, SCORE, SMOOTH  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

BAR = 1e-5                                         # BASELINE.json: smoothed means / covariances, relative
NLL_BAR, GRAD_BAR = 1e-8, 1e-7                     # against the oracle (test_nll_dense_score_gradient_...)
NLL_DUAL_BAR, GRAD_DUAL_BAR = 1e-10, 1e-7          # against the dual-number kernels


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _params_dev(arrs):
    return [_dev(arrs[k], torch.float64) for k in ('m0s', 'S0s', 'As', 'Cs', 'Qs')]


def profiled(lib, fn):
    """(scope names of the call, its result)."""
    lib.eks_profile_drain(None, 0, None, 0)
    lib.eks_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.eks_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    ms = (ctypes.c_float * 4096)()
    n = lib.eks_profile_drain(buf, len(buf), ms, 4096)
    return [nm.decode() for nm in buf.raw.split(b'\0')[:n]], out


def expected_scopes(form, mode):
    stem = 'dense_score_' if mode == SCORE else 'dense_'
    phases = ('summarize', 'replay') if form[0] == 'wave' else ('summarize', 'scan', 'replay')
    return [stem + p for p in phases]


def set_knobs(case, set_knob):
    for name in ('EKS_DW_CHUNK', 'EKS_DENSE_CHUNK', 'EKS_DENSE_LEGACY', 'EKS_DENSE_TREE_SCAN', 'EKS_DENSE_DUAL_GRAD'):
        assert os.environ.get(name) is None, f'{name} is set outside the test'
    for name, value in case.knobs.items():
        set_knob(name, value)


def smoother_reference(case, arrs, s):
    Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
    args = (arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s)
    if case.K > 1000:
        from oracle import c_oracle
        return c_oracle.smooth(arrs['ys'], Rd, *args)[:2]
    return orc.kalman_smoother(arrs['ys'], *args, Rd)[:2]


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_smoother_of_every_form_matches_oracle(case, set_knob, monkeypatch):
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    set_knobs(case, set_knob)
    form = case.forms()[SMOOTH]
    assert form == case.form and df.compiled(form)
    arrs, y, var, s = case.problem()
    ms_o, Vs_o = smoother_reference(case, arrs, s)
    args = (_dev(y), _dev(var), *_params_dev(arrs), _dev(s))
    ms_a, Vs_a = hip_ops.smooth(*args, flags=0)
    ms_b, Vs_b = hip_ops.smooth(*args, flags=0)
    ms_d, Vd_d = hip_ops.smooth(*args, flags=0, vs_diag=True)
    # exactly the queried bytes, 0xFF in every one of them, guards around them; profiled
    gw = bg.guarded_workspaces(monkeypatch, 0xFF)
    scopes, (ms_c, Vs_c) = profiled(lib, lambda: hip_ops.smooth(*args, flags=0))
    gw.assert_intact()
    need = df.smooth_workspace_bytes(case.T, case.K, case.D, case.O, case.knobs)

    to64 = lambda t, perm: np.transpose(t.cpu().numpy().astype(np.float64), perm)      # noqa: E731
    e_m = df.rel(to64(ms_a, (1, 0, 2)), ms_o, axis_scale=(1, 2))
    e_V = df.rel(to64(Vs_a, (1, 0, 2, 3)), Vs_o, axis_scale=(1, 2, 3))
    Vd_o = np.diagonal(Vs_o, axis1=2, axis2=3)
    e_md = df.rel(to64(ms_d, (1, 0, 2)), ms_o, axis_scale=(1, 2))
    e_Vd = df.rel(to64(Vd_d, (1, 0, 2)), Vd_o, axis_scale=(1, 2))
    again = bg.same_bits(ms_a, ms_b) and bg.same_bits(Vs_a, Vs_b)
    stale = bg.same_bits(ms_a, ms_c) and bg.same_bits(Vs_a, Vs_c)
    line = (f'FIGURES {case.id} {form}: ms {e_m:.2e} Vs {e_V:.2e} | vs_diag ms {e_md:.2e} Vs {e_Vd:.2e} | '
            f'workspace {gw.buffers[-1].nbody} B (transcribed {need}) scopes {scopes} | second call same bits {again}, '
            f'0xFF workspace same bits {stale}')
    print(line)
    assert tuple(ms_a.shape) == (case.T, case.K, case.D) and tuple(Vs_a.shape) == (case.T, case.K, case.D, case.D)
    assert all(bool(torch.isfinite(t).all()) for t in (ms_a, Vs_a, ms_d, Vd_d)), line
    assert max(e_m, e_V, e_md, e_Vd) < BAR, line
    assert scopes == expected_scopes(form, SMOOTH), line
    assert len(gw.buffers) == 1 and gw.buffers[0].nbody == need, line
    assert again and stale, line


SCORE_CASES = [c for c in CASES if c.T >= 2]       # a single frame has no transition: eks_nll keeps its dual-number kernels


def test_single_frame_cases_have_no_score_form():
    assert all(c.forms()[SCORE] is None for c in CASES if c.T < 2)
    assert all(c.forms()[SCORE] == c.form for c in SCORE_CASES)


@pytest.mark.parametrize('case', SCORE_CASES, ids=repr)
def test_score_of_every_form_matches_oracle_and_dual_numbers(case, set_knob, monkeypatch):
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    set_knobs(case, set_knob)
    form = case.forms()[SCORE]
    assert form == case.form and df.compiled(form)
    arrs, y, var, s = case.problem()
    # Q is positive definite with a margin; the general path whatever else the model is (D = O = 1 is also a diagonal model)
    assert hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs']) & _lib.FLAG_Q_PD
    flags = _lib.FLAG_Q_PD
    rconst = hip_ops.const_r(_dev(var), 1e-4)
    args = (_dev(y), rconst, *_params_dev(arrs), _dev(s[:, None]))
    call = lambda fl: hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=fl)      # noqa: E731
    n_a, g_a = call(flags)
    n_b, g_b = call(flags)
    scopes0, (n_0, g_0) = profiled(lib, lambda: call(0))
    gw = bg.guarded_workspaces(monkeypatch, 0xFF)
    scopes, (n_c, g_c) = profiled(lib, lambda: call(flags))
    gw.assert_intact()
    need = df.smooth_workspace_bytes(case.T, case.K, case.D, case.O, case.knobs)

    ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s,
                               rconst.cpu().numpy(), want_grad=True)
    host = lambda t: t.cpu().numpy()[:, 0]      # noqa: E731
    gmax = np.abs(gref).max()
    e_n = (np.abs(host(n_a) - ref) / np.abs(ref)).max()
    e_g = (np.abs(host(g_a) - gref) / gmax).max()
    e_n0 = (np.abs(host(n_a) - host(n_0)) / np.abs(ref)).max()
    e_g0 = (np.abs(host(g_a) - host(g_0)) / gmax).max()
    again = bg.same_bits(n_a, n_b) and bg.same_bits(g_a, g_b)
    stale = bg.same_bits(n_a, n_c) and bg.same_bits(g_a, g_c)
    line = (f'FIGURES {case.id} {form}: against the oracle nll {e_n:.2e} grad {e_g:.2e} | against dual numbers '
            f'nll {e_n0:.2e} grad {e_g0:.2e} | workspace {gw.buffers[-1].nbody} B (score form {need}) scopes {scopes}, '
            f'flags 0: {scopes0} | second call same bits {again}, 0xFF workspace same bits {stale}')
    print(line)
    assert tuple(n_a.shape) == tuple(g_a.shape) == (case.K, 1)
    assert np.all(np.isfinite(host(n_a))) and np.all(np.isfinite(host(g_a))) and gmax > 0, line
    assert e_n < NLL_BAR and e_g < GRAD_BAR, line
    assert e_n0 < NLL_DUAL_BAR and e_g0 < GRAD_DUAL_BAR, line
    assert scopes == expected_scopes(form, SCORE) and scopes0 == ['dense_nll'], line
    # eks_nll's workspace: the larger of the score form's (the smoother's layout) and the dual-number tree's
    d = _lib.EksDims(case.K, case.T, case.D, case.O, flags)
    assert len(gw.buffers) == 1 and gw.buffers[0].nbody == lib.eks_nll_workspace_bytes(ctypes.byref(d), 1) >= need, line
    assert again and stale, line
