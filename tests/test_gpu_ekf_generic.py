"""GPU: the extended smoother for user-supplied differentiable emission functions - eks_ekf_affine_sweep driven to
its fixed point through the C ABI, and run_kalman_smoother / optimize_smooth_param with an
eks_amd.emission.DifferentiableEmission - against the sequential extended Kalman filter / smoother of
oracle/ekf_oracle.py (reference eks/core.py:159-302 with h_fn).  Models: synth.emission_problem (the calibrated
projection restated in torch, a D = 2 map, a D = 6 constant-velocity rig, a D = 1 map).
Tolerances: those of tests/test_gpu_ekf.py (outputs 1e-5 relative to magnitude, s by Adam 1e-4)."""
import logging

import numpy as np
import pytest

from eks_amd import calibration as cal
from eks_amd import synth
from oracle import ekf_oracle as ek
from oracle import eks_oracle as orc

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a), device='cuda')
    return t if dtype is None else t.to(dtype)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _abi_fixed_point(prob, y, var, rconst, m0, S0, A, Q, s, Kd, vs_diag=False, tol=1e-10, cap=32):
    """tabulate (vmapped jacfwd) + hip_ops.ekf_affine_sweep until no point moves by more than tol, then the
    smoothing sweep (var given) on the last tables."""
    import torch
    from eks_amd import hip_ops
    from eks_amd.emission import DifferentiableEmission
    h = DifferentiableEmission(prob['fn'])
    K, D = m0.shape
    T = y.shape[0]
    xlin = m0[:, None, :].expand(K, T, D).contiguous()
    for n in range(1, cap + 1):
        X = xlin.transpose(0, 1).reshape(-1, D)
        hx, J = h.values_and_jacobians(X)
        off = (hx - (J @ X[:, :, None])[..., 0]).reshape(T, K, -1).contiguous()
        jac = J.reshape(T, K, -1, D).contiguous()
        _, _, nll, ch = hip_ops.ekf_affine_sweep(y, var, rconst, m0, S0, A, Q, s, jac, off, xlin)
        if ch.item() <= tol:
            break
    ms = Vs = None
    if var is not None:
        ms, Vs, nll, _ = hip_ops.ekf_affine_sweep(y, var, rconst, m0, S0, A, Q, s, jac, off, xlin, want_smoother=True,
                                                  vs_diag=vs_diag)
    return n, ch.item(), nll, ms, Vs, xlin


@pytest.mark.parametrize('model,T,K,V', [('pinhole', 1500, 3, 3), ('quad', 37, 2, 2), ('pinhole', 4100, 2, 4),
                                         ('exp1', 1, 2, 2), ('cv6', 500, 3, 3), ('cv6', 37, 2, 2),
                                         ('exp1', 1500, 3, 2)])
def test_abi_sweeps_reach_the_sequential_extended_smoother(model, T, K, V):
    import torch
    prob = synth.emission_problem(model, max(T, 12), K, seed=11, V=V)
    y, var = prob['y_tko'][:T], prob['var_tko'][:T]
    s = np.exp(np.linspace(-4, 5, K))
    m0 = _dev(prob['m0s'])
    n, ch, nll, ms, Vs, xlin = _abi_fixed_point(prob, _dev(y, torch.float32), _dev(var, torch.float32), None, m0,
                                                _dev(prob['S0s']), _dev(prob['As']), _dev(prob['Qs']), _dev(s), K)
    assert ch <= 1e-10 and n <= 16, (n, ch)
    ms, Vs, nll, xl = ms.cpu().numpy(), Vs.cpu().numpy(), nll.cpu().numpy(), xlin.cpu().numpy()
    for k in range(K):
        args = (_f32(y[:, k]), np.maximum(_f32(var[:, k]), 1e-12), prob['m0s'][k], prob['S0s'][k], prob['As'][k],
                prob['Qs'][k], s[k], prob['h_np'])
        mo, Vo, ll = ek.eks_smoother(*args)
        mp = ek.ekf_filter(*args)[3]
        assert np.abs(xl[k] - mp).max() < 1e-7 * max(1.0, np.abs(mp).max())
        assert np.abs(ms[:, k] - mo).max() < 1e-5 * np.abs(mo).max()
        assert np.abs(Vs[:, k] - Vo).max() < 1e-5 * np.abs(Vo).max()
        assert abs(nll[k] + ll) < 1e-9 * abs(ll)


def test_abi_constant_r_over_replicated_chains_and_vs_diag():
    import torch
    T, Kd, n_rep = 400, 2, 3
    prob = synth.emission_problem('quad', T, Kd, seed=5)
    rconst = np.maximum(np.median(_f32(prob['var_tko']), axis=0), 1e-4)
    s = np.exp(np.linspace(-3, 3, n_rep * Kd))                       # chain c -> keypoint c % Kd
    rep = lambda a: _dev(np.tile(a, (n_rep,) + (1,) * (a.ndim - 1)))   # noqa: E731
    y = _dev(prob['y_tko'], torch.float32)
    _, ch, nll, ms, _, _ = _abi_fixed_point(prob, y, None, _dev(rconst), rep(prob['m0s']), rep(prob['S0s']),
                                            rep(prob['As']), rep(prob['Qs']), _dev(s), Kd)
    assert ms is None and ch <= 1e-10
    nll = nll.cpu().numpy()
    for c in range(n_rep * Kd):
        k = c % Kd
        ref = ek.ekf_nll(_f32(prob['y_tko'][:, k]), rconst[k], prob['m0s'][k], prob['S0s'][k], prob['As'][k],
                         prob['Qs'][k], s[c], prob['h_np'])
        assert abs(nll[c] - ref) < 1e-9 * abs(ref)
    args = (prob, y, _dev(prob['var_tko'], torch.float32), None, _dev(prob['m0s']), _dev(prob['S0s']),
            _dev(prob['As']), _dev(prob['Qs']), _dev(s[:Kd]), Kd)
    full = _abi_fixed_point(*args)
    diag = _abi_fixed_point(*args, vs_diag=True)
    assert torch.equal(full[3], diag[3])
    assert torch.equal(torch.diagonal(full[4], dim1=2, dim2=3), diag[4])


def test_abi_rejects_bad_arguments():
    import ctypes
    import torch
    from eks_amd import _lib, hip_ops
    T, K, D, O = 64, 2, 3, 4
    f64 = dict(dtype=torch.float64, device='cuda')
    base = dict(y=torch.zeros((T, K, O), dtype=torch.float32, device='cuda'),
                var=torch.ones((T, K, O), dtype=torch.float32, device='cuda'), rconst=None,
                m0=torch.zeros((K, D), **f64), S0=torch.eye(D, **f64).repeat(K, 1, 1),
                A=torch.eye(D, **f64).repeat(K, 1, 1), Q=torch.eye(D, **f64).repeat(K, 1, 1),
                s=torch.ones(K, **f64), jac=torch.zeros((T, K, O, D), **f64), off=torch.zeros((T, K, O), **f64),
                xlin=torch.zeros((K, T, D), **f64))
    hip_ops.ekf_affine_sweep(**base)                                    # the well-formed call runs
    with pytest.raises(_lib.EksHipError, match='status -3'):             # D = 7
        D7 = 7
        hip_ops.ekf_affine_sweep(**{**base, 'm0': torch.zeros((K, D7), **f64),
                                    'S0': torch.eye(D7, **f64).repeat(K, 1, 1), 'A': torch.eye(D7, **f64).repeat(K, 1, 1),
                                    'Q': torch.eye(D7, **f64).repeat(K, 1, 1), 'jac': torch.zeros((T, K, O, D7), **f64),
                                    'xlin': torch.zeros((K, T, D7), **f64)})
    with pytest.raises(_lib.EksHipError, match='status -3'):             # O = 65
        O65 = 65
        hip_ops.ekf_affine_sweep(**{**base, 'y': torch.zeros((T, K, O65), dtype=torch.float32, device='cuda'),
                                    'var': torch.ones((T, K, O65), dtype=torch.float32, device='cuda'),
                                    'jac': torch.zeros((T, K, O65, D), **f64), 'off': torch.zeros((T, K, O65), **f64)})
    for missing in ('jac', 'off'):
        with pytest.raises(_lib.EksHipError, match=f'status {_status(lib_name="EKS_ERR_SHAPE")}'):
            hip_ops.ekf_affine_sweep(**{**base, missing: None})
    lib = _lib.load()
    d = _lib.EksDims(K, T, D, O, 0)
    small = lib.eks_ekf_affine_workspace_bytes(ctypes.byref(d), 0)
    assert lib.eks_ekf_affine_workspace_bytes(ctypes.byref(d), 1) > small > 0
    with pytest.raises(_lib.EksHipError, match=f'status {_status(lib_name="EKS_ERR_WORKSPACE")}'):
        hip_ops.ekf_affine_sweep(**base, ws=torch.empty(small - 8, dtype=torch.uint8, device='cuda'))
    with pytest.raises(_lib.EksHipError, match=f'status {_status(lib_name="EKS_ERR_WORKSPACE")}'):   # smoother's
        hip_ops.ekf_affine_sweep(**base, want_smoother=True, ws=torch.empty(small, dtype=torch.uint8, device='cuda'))


def _status(lib_name):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, 'include', 'eks_hip.h')).read()
    return int(re.search(rf'#define {lib_name}\s+\(?(-?\d+)', txt).group(1))


# ---- the torch restatement of the calibrated projection against the native pinhole path ------------------
def test_torch_pinhole_emission_matches_the_pinhole_path():
    from eks_amd.core import run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    T, K, V = 300, 2, 2
    prob = synth.calibrated_multicam(T, K, V, seed=13)
    ys = np.swapaxes(prob['y_tko'], 0, 1)
    args = (ys, prob['m0s'], prob['S0s'], prob['As'], None, prob['Qs'], prob['var_tko'])
    pin = cal.PinholeProjection(prob['cams_packed'])
    gen = DifferentiableEmission(synth.torch_pinhole(prob['cams_packed']))
    for sp in (4.0, None):
        s_p, ms_p, Vs_p = run_kalman_smoother(*args, smooth_param=sp, h_fn=pin)
        s_g, ms_g, Vs_g, info = run_kalman_smoother(*args, smooth_param=sp, h_fn=gen, return_info=True)
        assert info['change'] <= 1e-10
        assert np.abs(s_g / s_p - 1.0).max() < 1e-6
        if sp is None:        # outputs at the SAME s
            s_g, ms_g, Vs_g = run_kalman_smoother(*args, smooth_param=list(s_p), h_fn=gen)
        assert np.abs(ms_g - ms_p).max() < 1e-6 * np.abs(ms_p).max()
        assert np.abs(Vs_g - Vs_p).max() < 1e-6 * np.abs(Vs_p).max()


# ---- the reference-shaped operator with non-pinhole models ------------------------------------------------
def _operator_args(prob):
    ys = np.swapaxes(prob['y_tko'], 0, 1)
    return ys, (ys, prob['m0s'], prob['S0s'], prob['As'], None, prob['Qs'], prob['var_tko'])


@pytest.mark.parametrize('model,T,smooth_param', [('quad', 600, 4.0), ('cv6', 500, [0.5, 30.0, 2.0]),
                                                  ('exp1', 600, [0.3, 2.0, 9.0])])
def test_run_kalman_smoother_with_emission_fixed_s(model, T, smooth_param, caplog):
    from eks_amd.core import run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    prob = synth.emission_problem(model, T, 3, seed=11)
    ys, args = _operator_args(prob)
    D = prob['m0s'].shape[1]
    with caplog.at_level(logging.WARNING, logger='eks_amd.core'):
        s, ms, Vs = run_kalman_smoother(*args, smooth_param=smooth_param, h_fn=DifferentiableEmission(prob['fn']))
    assert not [r for r in caplog.records if 'linearisation' in r.getMessage()]
    assert ms.shape == (3, T, D) and Vs.shape == (3, T, D, D) and ms.dtype == np.float32
    so, mo, Vo, _ = ek.run_kalman_smoother_nonlinear(_f32(ys), prob['m0s'], prob['S0s'], prob['As'], prob['Qs'],
                                                     _f32(prob['var_tko']), prob['h_np'], smooth_param=smooth_param)
    np.testing.assert_array_equal(s, so)
    assert np.abs(ms - mo).max() < 1e-5 * np.abs(mo).max()
    assert np.abs(Vs - Vo).max() < 1e-5 * np.abs(Vo).max()


@pytest.mark.parametrize('blocks,s_frames', [(None, None), ([[0, 1]], [(30, 270)])])
def test_run_kalman_smoother_with_emission_optimises_s(blocks, s_frames, caplog):
    from eks_amd.core import run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    prob = synth.emission_problem('quad', 300, 2, seed=13)
    ys, args = _operator_args(prob)
    with caplog.at_level(logging.WARNING, logger='eks_amd.core'):
        s, ms, Vs, info = run_kalman_smoother(*args, h_fn=DifferentiableEmission(prob['fn']), blocks=blocks,
                                              s_frames=s_frames, return_info=True)
    assert not [r for r in caplog.records if 'linearisation' in r.getMessage()]
    assert info['mode'] == 'adam' and info['search_change'] <= 1e-10 and info['search_sweeps'] >= info['launches']
    so, _, _, _ = ek.run_kalman_smoother_nonlinear(_f32(ys), prob['m0s'], prob['S0s'], prob['As'], prob['Qs'],
                                                   _f32(prob['var_tko']), prob['h_np'], blocks=blocks,
                                                   s_frames=s_frames)
    assert np.abs(s / so - 1.0).max() < 1e-4
    if blocks:
        assert s[0] == s[1]
    _, mo, Vo, _ = ek.run_kalman_smoother_nonlinear(_f32(ys), prob['m0s'], prob['S0s'], prob['As'], prob['Qs'],
                                                    _f32(prob['var_tko']), prob['h_np'], smooth_param=list(s))
    assert np.abs(ms - mo).max() < 1e-5 * np.abs(mo).max()
    assert np.abs(Vs - Vo).max() < 1e-5 * np.abs(Vo).max()


def test_grid_mode_with_emission_picks_the_oracle_argmin():
    from eks_amd.core import run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    prob = synth.emission_problem('exp1', 400, 2, seed=17)
    ys, args = _operator_args(prob)
    s, _, _, info = run_kalman_smoother(*args, h_fn=DifferentiableEmission(prob['fn']), s_mode='grid', n_grid=9,
                                        return_info=True)
    assert info['mode'] == 'grid' and tuple(info['nll'].shape) == (2, 9)
    cand = np.exp(np.linspace(-8, 8, 9))
    ev = np.swapaxes(_f32(prob['var_tko']), 0, 1)
    for k in range(2):
        rc = orc.constant_R_from_timevarying(np.maximum(ev[k], 1e-12), 1e-4)
        nll = [ek.ekf_nll(_f32(ys[k]), rc, prob['m0s'][k], prob['S0s'][k], prob['As'][k], prob['Qs'][k], c,
                          prob['h_np']) for c in cand]
        assert s[k] == cand[int(np.argmin(nll))]


def test_optimize_smooth_param_with_emission_writes_s_in_place_and_device_outputs():
    import torch
    from eks_amd.core import optimize_smooth_param, run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    T, K = 300, 2
    prob = synth.emission_problem('quad', T, K, seed=13)
    ys, args = _operator_args(prob)
    h = DifferentiableEmission(prob['fn'])
    Rs = np.stack([[np.diag(r) for r in np.maximum(prob['var_tko'][:, k], 1e-12)] for k in range(K)])
    guesses = [orc.compute_initial_guess(prob['var_tko'][:, k, :]) for k in range(K)]
    s_finals = np.zeros(K)
    optimize_smooth_param(ys, prob['m0s'], prob['S0s'], prob['As'], None, prob['Qs'], Rs, None, s_finals, None,
                          guesses, tol=1e-2, h_fn_combined=h)
    s_ref, _, _ = run_kalman_smoother(*args, h_fn=h)
    np.testing.assert_allclose(s_finals, s_ref, rtol=1e-12)
    # device outputs, the diagonal of Vs and a first guess of the points
    s_dev, ms, Vs, info = run_kalman_smoother(*args, smooth_param=list(s_ref), h_fn=h, return_device=True,
                                              return_info=True, vs_diag=True, x_init=np.swapaxes(prob['latent'], 0, 1))
    assert isinstance(s_dev, np.ndarray) and s_dev.dtype == np.float64
    assert isinstance(ms, torch.Tensor) and ms.is_cuda and tuple(ms.shape) == (K, T, 2) and ms.dtype == torch.float32
    assert isinstance(Vs, torch.Tensor) and tuple(Vs.shape) == (K, T, 2)
    assert isinstance(info['sweeps'], int) and info['sweeps'] >= 1 and info['change'] <= 1e-10


def test_capped_sweeps_warn_and_report_their_last_change(caplog):
    from eks_amd.core import run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    prob = synth.emission_problem('cv6', 500, 2, seed=11)
    _, args = _operator_args(prob)
    with caplog.at_level(logging.WARNING, logger='eks_amd.core'):
        _, ms, _, info = run_kalman_smoother(*args, smooth_param=1.0, return_info=True,
                                             h_fn=DifferentiableEmission(prob['fn'], max_sweeps=2))
    assert info['change'] > 1e-10 and info['sweeps'] == 3
    assert [r for r in caplog.records if 'linearisation points still moving' in r.getMessage()]
    assert np.isfinite(ms).all()
