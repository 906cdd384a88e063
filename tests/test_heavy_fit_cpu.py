"""No GPU: the references of eks_smooth_heavy_fit (tests/heavy_fit_ref.py) checked against themselves - the bound
under the M-step for s (monotone over 40 passes, and its direct evaluation from the joint posterior across a step), the
fixed point, the Gaussian limit against tests/em_ref.py's EM loop, and what the fit buys on the feature's session - the
float64 statistic and step of eks_amd/csrc/eks_smooth_heavy_fit_lane.hpp run from plain loops by the stand-alone
tests/host_sim/heavy_fit_sim.cpp (plain and under -fsanitize=address,undefined; never loaded into this process), the C
ABI's refusals (returned before anything touches a device) and the Python argument checks.

The quality bars come from the reference alone, measured when the feature was written (seeds 0, 1, 2):
Gaussian EM fixed point s q = 67 .. 102 at a truth of 0.05; the 40-pass fit from s q = 1 gives 0.042 .. 0.052; RMSE
0.355 .. 0.363 px against 3.8 .. 6.2 px for the robust smoother at the Gaussian s."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref as eref  # noqa: E402
import heavy_fit_ref as fref  # noqa: E402
import heavy_ref as href  # noqa: E402
from test_increments_cpu import dense_case  # noqa: E402

INF = math.inf
PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')


# ---- the bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('sq', [0.005, 0.05, 0.5])
def test_bound_never_drops_over_40_passes_with_the_step(seed, sq):
    """heavy_session (jumps and displaced frames), both nu = 4, from three starts; tests/test_heavy_cpu.py's tolerance
    for the same check without the step."""
    s = href.heavy_session(seed)
    m0, S0, a, c, _ = s['args']
    hist = []
    out = fref.scalar_fit(s['y'], s['var'], m0, S0, a, c, np.ones(2), sq, 4.0, 4.0, 40, D=2, history=hist)
    path = fref.elbo_path(hist, 4.0, 4.0, 2)
    steps = np.diff(path, axis=0)
    print(f'seed {seed} from s q = {sq}: s q = {out[4][0]:.4g} after 40 passes, RMSE {fref.rmse(out[0], s["x"]):.3g}; '
          f'smallest step of the bound {steps.min():+.3g}')
    assert np.all(steps >= -1e-9 * np.abs(path[1:]))
    assert len({float(h[5][0]) for h in hist}) == 40             # s moved in every pass


@pytest.mark.parametrize('nus', [(3.0, 5.0)])
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3)])
def test_direct_evaluation_of_the_bound_rises_across_a_step(D, O, nus):
    """T = 6, general model: the bound after pass i + 1 (under s_{i+1}, with the q(lam), q(u) of pass i) evaluated term
    by term from the joint posterior (heavy_ref.elbo_direct) is the compact form, and it is not below the bound after
    pass i - the chain q(lam), q(u) -> s -> q(x) is coordinate ascent."""
    T, K = 6, 2
    M = dense_case(K, D, O, False, seed=D + 11)
    par = tuple(M[k] for k in PARAMS)
    rng = np.random.default_rng(D)
    y = rng.normal(size=(T, K, O)) * 2
    y[3:] += 9.0
    y[2, :, 0] -= 14.0
    var = np.exp(rng.normal(0.0, 0.6, (T, K, O)))
    hist = []
    fref.dense_fit(y, var, *par, nus[0], nus[1], 5, history=hist, bounds=(-20.0, 20.0))
    path = fref.elbo_path(hist, nus[0], nus[1], D)
    direct = np.empty_like(path)
    for i in range(1, len(hist)):
        for k in range(K):
            direct[i - 1, k] = href.elbo_direct(y[:, k], var[:, k], *(p[k] for p in par[:5]), hist[i][5][k], nus[0],
                                                nus[1], hist[i - 1][2][:, k], hist[i - 1][3][:, k])
    assert np.all(np.abs(direct - path) <= 1e-9 * np.abs(direct))
    assert np.all(np.diff(direct, axis=0) >= -1e-9 * np.abs(direct[1:]))
    moved = np.abs(np.log(hist[2][5] / hist[1][5]))
    assert moved.min() > 1e-3, 'the step did not move s: nothing was tested'
    # the step alone, q(x), q(lam), q(u) held: E_q log p as a function of s is -n/2 log s - S s_old / (2 s) + const,
    # largest at s_new = s_old S / n
    lam, w, dobs, dproc, ll, s_old = hist[1]
    u_new = np.clip((nus[1] + D) / (nus[1] + dproc[1:]), 1e-30, (nus[1] + D) / nus[1])
    S, n = (u_new * dproc[1:]).sum(axis=0), D * (T - 1)
    f = lambda s: -0.5 * n * np.log(s) - 0.5 * S * s_old / s  # noqa: E731
    s_new = s_old * S / n
    assert np.all(f(s_new) >= f(s_new * 1.01)) and np.all(f(s_new) >= f(s_new * 0.99)) and np.all(f(s_new) >= f(s_old))


def test_fixed_point_has_statistic_over_n_equal_to_one():
    """The step multiplies s by S / n, so row 2 of change is |log(S / n)|: it falls towards 0, and at the s the
    iteration converges to the statistic recomputed from the planes is n."""
    s = fref.outlier_session(0, T=200, n_bad=5)
    hist = []
    out = fref.scalar_fit(s['y'], s['var'], *s['args'], 1.0, 4.0, INF, 400, D=2, history=hist)
    lam, w, dobs, dproc, ll, s_last = hist[-1]
    ratio = fref.statistic(w, dproc)[0] / (2 * 199)
    print(f'after 400 passes: s q = {out[4][0]:.6g}, S / n = {ratio:.9f}, last |delta log s| = {out[5][2][0]:.3g}')
    assert abs(ratio - 1.0) < 1e-6 and out[5][2][0] < 1e-6
    assert np.array_equal(out[3], np.ones_like(out[3])) and not out[5][1].any()      # the Gaussian side


def test_both_sides_gaussian_is_the_em_loop_of_em_ref():
    T, K, D = 150, 3, 2
    rng = np.random.default_rng(4)
    q = rng.uniform(0.5, 2.0, K * D)
    a, c = 0.98, 1.3
    x = np.zeros((T, K * D))
    for t in range(1, T):
        x[t] = a * x[t - 1] + rng.normal(size=K * D) * np.sqrt(0.3 * q)
    var = rng.uniform(0.5, 2.0, (T, K * D))
    y = c * x + rng.normal(size=(T, K * D)) * np.sqrt(var)
    m0, S0 = np.zeros(K * D), np.full(K * D, 4.0)
    s0 = np.array([0.01, 0.3, 20.0])
    n_iters = 12
    hist = []
    out = fref.scalar_fit(y, var, m0, S0, a, c, q, s0, INF, INF, n_iters + 1, D=D, history=hist, bounds=(-3.0, 3.0))
    trace = eref.scalar_trace_fn(y, var, m0, S0, np.full(K * D, a), np.full(K * D, c), q, D)
    path, deltas, _ = eref.em_scale_loop(trace, D * (T - 1), np.log(s0), [[k] for k in range(K)], -3.0, 3.0, 0.0,
                                         1000, n_iters)
    mine = np.log(np.array([h[5] for h in hist]))
    assert mine.shape == path.shape
    assert np.abs(mine - path).max() < 1e-9, np.abs(mine - path).max()
    assert np.abs(out[5][2] - deltas[-1]).max() < 1e-9
    assert np.array_equal(out[2], np.ones_like(out[2])) and np.array_equal(out[3], np.ones_like(out[3]))


# ---- what the fit buys -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def table():
    rows = []
    for seed in (0, 1, 2):
        s = fref.outlier_session(seed)
        gauss = fref.scalar_fit(s['y'], s['var'], *s['args'], 1.0, INF, INF, 80, D=2)
        robust = fref.scalar_fit(s['y'], s['var'], *s['args'], gauss[4], 4.0, INF, 12, D=2, fit=False)
        fit = fref.scalar_fit(s['y'], s['var'], *s['args'], 1.0, 4.0, INF, 40, D=2)
        stuck = fref.scalar_fit(s['y'], s['var'], *s['args'], gauss[4], 4.0, INF, 40, D=2)
        rows.append(dict(s=s, gauss=gauss, robust=robust, fit=fit, stuck=stuck))
    return rows


def test_the_three_seed_table(table):
    """T = 600, one keypoint, two unit chains, true s q = 0.05, fourteen frames displaced by 20 .. 60 px."""
    truth = 0.05
    for seed, row in enumerate(table):
        x = row['s']['x']
        g, r, f = (fref.rmse(row[k][0], x) for k in ('gauss', 'robust', 'fit'))
        sg, sf = float(row['gauss'][4][0]), float(row['fit'][4][0])
        print(f'seed {seed}: Gaussian EM fixed point s q = {sg:.4g} (RMSE {g:.3g}); robust at that s RMSE {r:.3g}; '
              f'fitted s q = {sf:.4g} (RMSE {f:.3g}); from the Gaussian s: s q = {float(row["stuck"][4][0]):.4g} '
              f'(RMSE {fref.rmse(row["stuck"][0], x):.3g})')
        assert sg > 100 * truth
        assert truth / 2.5 <= sf <= truth * 2.5
        assert f < 0.25 * r


# ---- the lanes from plain loops ------------------------------------------------------------------------------------------
def _build_sim(path, extra):
    subprocess.run(['g++', '-std=c++17', *extra, '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'heavy_fit_sim.cpp'), '-o', path], check=True)
    return path


@pytest.mark.parametrize('which', ['plain', 'san'])
def test_host_simulator_self_check(which, tmp_path):
    """Slab edges, the long-double sum, subset bits, a poisoned keypoint and the bounds: the checks live in the program."""
    extra = ['-O2'] if which == 'plain' else ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    sim = _build_sim(str(tmp_path / f'heavy_fit_sim_{which}'), extra)
    r = subprocess.run([sim], capture_output=True, text=True)
    assert r.returncode == 0 and 'heavy_fit_sim: ok' in r.stdout, r.stdout + r.stderr


def test_reference_step_conventions():
    s, dl = fref.step(np.array([1.0, 1.0, 1.0, 0.0, 2.0]), np.array([np.nan, np.inf, 0.0, 5.0, 30.0]), 10.0, (-8.0, 8.0))
    assert s[0] == 1.0 and s[1] == 1.0 and s[3] == 0.0 and dl[0] == dl[1] == dl[3] == 0.0
    assert s[2] == math.exp(-8.0) and dl[2] == 8.0
    assert s[4] == 6.0 and abs(dl[4] - math.log(3.0)) < 1e-15


# ---- the C ABI's refusals (returned before anything touches a device) ------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_entry_points_declared_bound_and_exported(lib):
    from eks_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_smooth_heavy_fit', 'eks_smooth_heavy_fit_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name) is not None


def test_c_abi_refusals(lib):
    """On host buffers: the fit's own refusals, then eks_smooth_heavy's status for every defect it shares."""
    from eks_amd import _lib
    import test_api_refusals_cpu as api
    buf = ctypes.create_string_buffer(64)
    one, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    dref = lambda dims: None if dims is None else ctypes.byref(_lib.EksDims(*dims))  # noqa: E731
    names = api.MODEL + ['s_out', 'ms', 'Vs']

    def fit(dims, nu=(4.0, 4.0), n_iters=8, bounds=(-8.0, 8.0), planes_in=0, weights=null, scales=null, ws=one,
            ws_bytes=1 << 40, **nulls):
        p = [null if nulls.get(n) else one for n in names]
        return int(lib.eks_smooth_heavy_fit(dref(dims), *p[:8], nu[0], nu[1], n_iters, bounds[0], bounds[1], weights,
                                            scales, planes_in, null, *p[8:], ws, ws_bytes, None))

    def heavy(dims, nu=(4.0, 4.0), n_iters=8, planes_in=0, weights=null, scales=null, ws=one, ws_bytes=1 << 40, **nulls):
        p = [null if nulls.get(n) else one for n in api.MODEL + ['ms', 'Vs']]
        return int(lib.eks_smooth_heavy(dref(dims), *p[:8], nu[0], nu[1], n_iters, weights, scales, planes_in, null,
                                        *p[8:], ws, ws_bytes, None))

    qf = lambda dims: int(lib.eks_smooth_heavy_fit_workspace_bytes(dref(dims)))  # noqa: E731
    qh = lambda dims: int(lib.eks_smooth_heavy_workspace_bytes(dref(dims)))  # noqa: E731
    nan = float('nan')
    for dims in (api.CHAINS, api.GENERAL, api.CHAINS[:4] + (api.DIAG | api.UNIT,)):
        one_frame = dims[:1] + (1,) + dims[2:]
        assert fit(one_frame) == -2 and qf(one_frame) == 0 and qh(one_frame) > 0
        assert fit(one_frame, y=True) == -2                                  # shapes come before the pointers
        for nu in ((0.0, 4.0), (4.0, -1.0), (nan, 4.0), (4.0, nan), (-INF, 4.0)):
            assert fit(dims, nu=nu) == -2 and fit(dims, nu=nu, y=True) == -2
        for bounds in ((1.0, 0.0), (-INF, 0.0), (0.0, INF), (nan, 0.0), (0.0, nan)):
            assert fit(dims, bounds=bounds) == -2 and fit(dims, bounds=bounds, ms=True) == -2
        assert fit(dims, bounds=(0.0, 0.0), ws=null) == -4                   # lo == hi is allowed
        assert fit(dims, n_iters=0) == -2 and fit(dims, n_iters=0, Vs=True) == -2
        # a Gaussian side takes no input plane
        assert fit(dims, nu=(4.0, INF), planes_in=2, scales=one) == -2
        assert fit(dims, nu=(4.0, INF), planes_in=1, weights=one, ws=null) == -4
        diag = bool(dims[4] & api.DIAG)
        assert fit(dims, nu=(INF, 4.0), planes_in=1, weights=one) == -2
        assert fit(dims, nu=(INF, 4.0), ws=null) == (-4 if diag else -3)     # general models: nu_obs = +inf unsupported
        assert fit(dims, nu=(INF, INF), ws=null) == (-4 if diag else -3)
        assert fit(dims, nu=(INF, 4.0), y=True) == (-1 if diag else -3)
        # every defect eks_smooth_heavy shares, in its order
        for a in api.MODEL + ['ms', 'Vs']:
            assert fit(dims, **{a: True}) == heavy(dims, **{a: True}) == -1
        assert fit(dims, s_out=True) == -1 and fit(dims, s_out=True, ws=null) == -1
        assert fit(dims, ws=null) == heavy(dims, ws=null) == -4
        assert fit(dims, y=True, ws=null) == -1
        assert fit(dims, ws_bytes=qf(dims) - 1) == -4 and fit(dims, ws_bytes=qh(dims)) == -4
        for bits, kw in ((1, dict(scales=one)), (2, dict(weights=one)), (3, dict())):
            assert fit(dims, planes_in=bits, **kw) == heavy(dims, planes_in=bits, **kw) == -1
            assert fit(dims, planes_in=bits, nu=(0.0, 4.0), **kw) == -2
        assert fit(dims, planes_in=3, weights=one, scales=one, ws=null) == -4
        # the size: eks_smooth_heavy's plus [ceil((T - 1) / R)][K] doubles and one ticket per keypoint tile, each on 256 bytes
        assert qf(dims) == qh(dims) + 256 + 256
    for dims in list(api.BAD_DIMS.values()) + list(api.UNSUPPORTED_DIMS.values()):
        assert fit(dims) == heavy(dims) != 0 and qf(dims) == 0
    big = (65, 3 * fref.R + 2, 2, 2, api.DIAG | api.VSD)
    assert qf(big) == qh(big) + (4 * 65 * 8 + 255) // 256 * 256 + 256


def test_python_argument_checks():
    from eks_amd import heavy_tails
    K, T = 2, 10
    eye = np.tile(np.eye(2), (K, 1, 1))
    args = (np.zeros((K, T, 2)), np.zeros((K, 2)), eye, eye, eye, eye, np.ones((T, K, 2)), 1.0)
    for kw in (dict(nu_obs=0.0), dict(nu_proc=-1.0), dict(nu_obs=float('nan')), dict(n_iters=0), dict(n_iters=2.5),
               dict(log_s_bounds=(1.0, 0.5)), dict(log_s_bounds=(0.0, INF)), dict(log_s_bounds=(float('nan'), 1.0))):
        with pytest.raises(ValueError):
            heavy_tails.fit_heavy_tailed(*args, **kw)
    with pytest.raises(ValueError):
        heavy_tails.fit_heavy_tailed(np.zeros((K, 1, 2)), *args[1:6], np.ones((1, K, 2)), 1.0)
    with pytest.raises(NotImplementedError):
        heavy_tails.fit_heavy_tailed(*args, h_fn=lambda x: x)
    import eks_amd
    assert eks_amd.fit_heavy_tailed is heavy_tails.fit_heavy_tailed
    assert eks_amd.fit_singlecam_heavy_tailed is heavy_tails.fit_singlecam_heavy_tailed
