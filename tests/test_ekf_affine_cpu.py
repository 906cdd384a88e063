"""CPU: the extended smoother for user-supplied emission functions (eks_amd.emission.DifferentiableEmission).

* one sweep of eks_ekf_affine_sweep (AffineObs tables, eks_amd/csrc/eks_dense_lane.hpp), run from plain loops over
  the SAME lane header (tests/host_sim/ekf_affine_sim.cpp), iterated from Python with the tables rebuilt between
  sweeps, reaches the sequential extended filter / smoother of oracle/ekf_oracle.py;
* constant tables are the linear filter and stop changing after one sweep;
* Jacobians: vmapped jacfwd, a supplied jacobian and the oracle's complex step agree;
* host-side validation of the wrapper runs before any device call.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from eks_amd import calibration as cal
from eks_amd import synth
from oracle import ekf_oracle as ek
from oracle import eks_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'ekf_affine_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libekf_affine_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    so = ctypes.CDLL(lib)
    so.sim_affine_sweep.restype = ctypes.c_double
    return so


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _jac_cs(h_np, X, step=1e-30):
    """dh/dx at every row of X (..., D) by complex step -> (..., O, D)."""
    cols = []
    for i in range(X.shape[-1]):
        Xc = X.astype(np.complex128)
        Xc[..., i] += 1j * step
        cols.append(np.imag(h_np(Xc)) / step)
    return np.stack(cols, axis=-1)


def _tables(h_np, xlin):
    """(jac [T][K][O][D], off [T][K][O]) at the points xlin (K, T, D), the kernels' layout."""
    X = np.ascontiguousarray(np.swapaxes(xlin, 0, 1))
    J = _jac_cs(h_np, X)
    off = h_np(X) - np.einsum('tkod,tkd->tko', J, X)
    return np.ascontiguousarray(J), np.ascontiguousarray(off)


def _fixed_point(sim, y, var, rconst, m0, S0, A, Q, s, tab, xlin, Kd, B=16, tol=1e-10, cap=40, smooth=True):
    """tabulate + sweep until no point moves by more than tol, then the smoothing sweep on the last tables
    (what eks_amd/core.py does).  Returns (sweeps, last change, nll, ms, Vs)."""
    K, T, D = xlin.shape
    O = y.shape[2]
    nll = np.zeros(K)
    ms = np.zeros((T, K, D), np.float32) if smooth else None
    Vs = np.zeros((T, K, D, D), np.float32) if smooth else None
    for n in range(1, cap + 1):
        jac, off = tab(xlin)
        ch = sim.sim_affine_sweep(T, K, Kd, D, O, B, _p(y), _p(var), _p(rconst), _p(m0), _p(S0), _p(A), _p(Q),
                                  _p(s), _p(jac), _p(off), _p(xlin), None, None, _p(nll))
        if ch <= tol:
            break
    if smooth:
        sim.sim_affine_sweep(T, K, Kd, D, O, B, _p(y), _p(var), _p(rconst), _p(m0), _p(S0), _p(A), _p(Q), _p(s),
                             _p(jac), _p(off), _p(xlin), _p(ms), _p(Vs), _p(nll))
    return n, ch, nll, ms, Vs


# sweeps to 1e-10 ("Extended smoother for user-supplied emission functions")
_MAX_SWEEPS = {'pinhole': 8, 'quad': 12, 'cv6': 11, 'exp1': 15}


@pytest.mark.parametrize('model,T,init', [('pinhole', 700, 'prior'), ('pinhole', 700, 'triangulated'),
                                          ('quad', 600, 'prior'), ('cv6', 500, 'prior'), ('exp1', 600, 'prior')])
def test_host_sim_sweeps_reach_the_sequential_extended_smoother(sim, model, T, init):
    K = 3
    prob = synth.emission_problem(model, T, K, seed=11)
    y = prob['y_tko'].astype(np.float32)
    var = prob['var_tko'].astype(np.float32)
    s = np.array([2.0, 0.01, 300.0])
    m0, S0, A, Q = prob['m0s'], prob['S0s'], prob['As'], prob['Qs']
    D = m0.shape[1]
    if init == 'prior':
        xlin = np.repeat(m0[:, None, :], T, axis=1).copy()
    else:
        p = synth.calibrated_multicam(T, K, 3, seed=11)
        xy = np.transpose(p['y_tko'].reshape(T, K, 3, 2), (2, 1, 0, 3)).reshape(3, K * T, 2)
        xlin = cal.triangulate(p['cams_packed'], xy).reshape(K, T, 3).copy()
    h = prob['h_np']
    n, ch, nll, ms, Vs = _fixed_point(sim, y, var, None, m0, S0, A, Q, s, lambda x: _tables(h, x), xlin, K)
    assert ch <= 1e-10 and n <= _MAX_SWEEPS[model], (n, ch)
    for k in range(K):
        args = (y[:, k].astype(np.float64), np.maximum(var[:, k].astype(np.float64), 1e-12), m0[k], S0[k], A[k],
                Q[k], s[k], h)
        mo, Vo, ll = ek.eks_smoother(*args)
        mp = ek.ekf_filter(*args)[3]
        assert np.abs(xlin[k] - mp).max() < 1e-7 * max(1.0, np.abs(mp).max())     # points = predicted means
        assert np.abs(ms[:, k] - mo).max() < 1e-5 * np.abs(mo).max()
        assert np.abs(Vs[:, k] - Vo).max() < 1e-5 * np.abs(Vo).max()
        assert abs(nll[k] + ll) < 1e-10 * abs(ll)


def test_host_sim_constant_r_over_replicated_chains(sim):
    T, Kd, rep = 400, 2, 3
    prob = synth.emission_problem('quad', T, Kd, seed=5)
    y = prob['y_tko'].astype(np.float32)
    rconst = np.median(prob['var_tko'], axis=0)
    s = np.exp(np.linspace(-3, 3, rep * Kd))                       # chain c -> keypoint c % Kd
    tile = lambda a: np.ascontiguousarray(np.tile(a, (rep,) + (1,) * (a.ndim - 1)))   # noqa: E731
    m0, S0, A, Q = (tile(prob[n]) for n in ('m0s', 'S0s', 'As', 'Qs'))
    xlin = np.repeat(m0[:, None, :], T, axis=1).copy()
    h = prob['h_np']
    n, ch, nll, _, _ = _fixed_point(sim, y, None, rconst, m0, S0, A, Q, s, lambda x: _tables(h, x), xlin, Kd,
                                    smooth=False)
    assert ch <= 1e-10
    for c in range(rep * Kd):
        k = c % Kd
        ref = ek.ekf_nll(y[:, k].astype(np.float64), rconst[k], m0[c], S0[c], A[c], Q[c], s[c], h)
        assert abs(nll[c] - ref) < 1e-10 * abs(ref)


@pytest.mark.parametrize('B', [16, 32])
def test_constant_tables_are_the_linear_filter_and_stop_after_one_sweep(sim, B):
    rng = np.random.default_rng(0)
    T, K, D, O = 300, 2, 3, 4
    C = rng.normal(size=(K, O, D))
    off = rng.normal(size=(K, O)) * 10
    y = (rng.normal(size=(T, K, O)).cumsum(axis=0)).astype(np.float32)
    var = (0.5 + rng.random((T, K, O))).astype(np.float32)
    m0, S0 = rng.normal(size=(K, D)), np.tile(np.eye(D) * 4.0, (K, 1, 1))
    A = np.tile(np.eye(D), (K, 1, 1)) + 0.05 * rng.normal(size=(K, D, D))
    Q = np.tile(np.diag([1.0, 2.0, 0.5]), (K, 1, 1))
    s = np.array([0.7, 3.0])
    jac = np.ascontiguousarray(np.broadcast_to(C[None], (T, K, O, D)))
    offt = np.ascontiguousarray(np.broadcast_to(off[None], (T, K, O)))
    xlin = rng.normal(size=(K, T, D)) * 50
    n, ch, nll, ms, Vs = _fixed_point(sim, y, var, None, m0, S0, A, Q, s, lambda x: (jac, offt), xlin, K, B=B)
    assert n == 2 and ch == 0.0                   # the second sweep reproduces the first bit for bit
    yo = np.swapaxes(y.astype(np.float64), 0, 1) - off[:, None, :]
    mo, Vo, nllo = orc.kalman_smoother(yo, m0, S0, A, C, Q, s, np.swapaxes(var.astype(np.float64), 0, 1))
    assert np.abs(np.swapaxes(ms, 0, 1) - mo).max() < 1e-5 * np.abs(mo).max()
    assert np.abs(np.swapaxes(Vs, 0, 1) - Vo).max() < 1e-5 * np.abs(Vo).max()
    np.testing.assert_allclose(nll, nllo, rtol=1e-10)


@pytest.mark.parametrize('model', ['exp1', 'quad', 'cv6'])
def test_autodiff_supplied_and_complex_step_jacobians_agree(model):
    import torch
    from eks_amd.emission import DifferentiableEmission
    prob = synth.emission_problem(model, 50, 2, seed=3)
    X = prob['latent'].reshape(-1, prob['latent'].shape[-1])[:64]
    Xt = torch.as_tensor(X)
    ref = _jac_cs(prob['h_np'], X)
    scale = np.abs(ref).max()
    h_auto, J_auto = DifferentiableEmission(prob['fn']).values_and_jacobians(Xt)
    jac = prob['jac'] if prob['jac'] is not None else (lambda x: torch.func.jacrev(prob['fn'])(x))
    h_given, J_given = DifferentiableEmission(prob['fn'], jacobian=jac).values_and_jacobians(Xt)
    batched = DifferentiableEmission(torch.func.vmap(prob['fn']), batched=True)
    h_b, J_b = batched.values_and_jacobians(Xt)
    for h, J in ((h_auto, J_auto), (h_given, J_given), (h_b, J_b)):
        assert J.dtype == torch.float64 and tuple(J.shape) == ref.shape
        assert np.abs(J.numpy() - ref).max() < 1e-9 * scale
        assert np.abs(h.numpy() - prob['h_np'](X)).max() < 1e-12 * np.abs(h.numpy()).max()
    # the oracle's own complex step, point by point
    for x, J in zip(X[:4], J_auto.numpy()[:4]):
        assert np.abs(ek.jacobian_cs(prob['h_np'], x) - J).max() < 1e-9 * scale


# ---- host-side validation: before any device call, so it runs on a CPU-only box --------------------------
def _call(fn, D=2, O=3, K=2, T=6, **kw):
    from eks_amd.core import run_kalman_smoother
    from eks_amd.emission import DifferentiableEmission
    z = np.zeros
    h = fn if not callable(fn) or hasattr(fn, 'values') else DifferentiableEmission(fn, **kw)
    return run_kalman_smoother(z((K, T, O)), z((K, D)), np.tile(np.eye(D), (K, 1, 1)), np.tile(np.eye(D), (K, 1, 1)),
                               None, np.tile(np.eye(D), (K, 1, 1)), np.ones((T, K, O)), smooth_param=1.0, h_fn=h)


def test_validation_rejects_bad_emissions_before_any_device_call():
    import torch
    quad = lambda x: torch.stack([x[0], x[1] ** 2, x[0] * x[1]])                     # noqa: E731
    with pytest.raises(ValueError, match='fn at m0s must return'):
        _call(quad, O=4)                                                            # ys says O = 4, fn gives 3
    with pytest.raises(ValueError, match='1..6'):
        _call(lambda x: x[:3], D=7, O=3)
    with pytest.raises(ValueError, match='1..64'):
        _call(lambda x: torch.cat([x] * 33)[:65], D=2, O=65)
    with pytest.raises(ValueError, match='non-finite'):
        _call(lambda x: torch.stack([x[0], 1.0 / x[1], x[0]]))                      # m0 = 0: 1 / 0
    with pytest.raises(ValueError, match='jacobian at m0s'):
        _call(quad, jacobian=lambda x: torch.zeros(3, 3, dtype=x.dtype))
    with pytest.raises(ValueError, match='x_init'):
        from eks_amd.core import run_kalman_smoother
        from eks_amd.emission import DifferentiableEmission
        run_kalman_smoother(np.zeros((2, 6, 3)), np.zeros((2, 2)), np.tile(np.eye(2), (2, 1, 1)),
                            np.tile(np.eye(2), (2, 1, 1)), None, np.tile(np.eye(2), (2, 1, 1)), np.ones((6, 2, 3)),
                            smooth_param=1.0, h_fn=DifferentiableEmission(quad), x_init=np.zeros((2, 6, 3)))


def test_bare_callables_are_still_refused_and_the_message_names_the_wrapper():
    from eks_amd.core import run_kalman_smoother
    z = np.zeros
    with pytest.raises(NotImplementedError, match='DifferentiableEmission'):
        run_kalman_smoother(z((1, 4, 4)), z((1, 3)), z((1, 3, 3)), z((1, 3, 3)), z((1, 4, 3)),
                            z((1, 3, 3)), z((4, 1, 4)), smooth_param=1.0, h_fn=lambda x: x)


def test_wrapper_is_exported_lazily():
    import eks_amd
    from eks_amd.emission import DifferentiableEmission
    assert eks_amd.DifferentiableEmission is DifferentiableEmission
    with pytest.raises(TypeError):
        DifferentiableEmission(3.0)
