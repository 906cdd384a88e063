"""CPU: eks_smooth_robust without a GPU - the variational bound of tests/robust_ref.py against its term-by-term
evaluation from the joint Gaussian posterior, its monotonicity over 32 passes, the Gaussian limit, what the method buys
on sessions with displaced frames, the dense reference against the scalar one, the float32 lane arithmetic of
eks_amd/csrc/eks_smooth_student_lane.hpp run from plain loops by the stand-alone tests/host_sim/robust_sim.cpp (plain and
under -fsanitize=address,undefined; never loaded into this process), the C ABI's refusals and the Python argument
checks.

Float32 bar (robust_ref.bars), the project's rule: error / scale <= max(1e-5, 4 x the float32 NumPy transcription's
own worst error / scale on the same inputs); ms over the chain's max |y|, Vs over its own value, weights and change
over 1.  The transcription is the yardstick, never the simulator.

Pass counts: a call of n passes updates the weights n - 1 times, and a continued call's first pass smooths again under
the weights it was given, so n1 passes followed by n2 passes are one call of n1 + n2 - 1 passes (3 then 6 = 8).

Recorded (float64): bound against its direct evaluation 1.4e-16 (D, O = 1, 1), 2.8e-16 (2, 3) relative; smallest step
of the bound over 32 passes, seeds 0..4, +3.9e-10; nu = 1e12 against the Gaussian smoother 8.4e-10; robust RMSE over
Gaussian RMSE 0.155 - 0.182; displaced frames' weights <= 0.022, clean frames' >= 0.185; dense against scalar
reference 2.2e-15.  Host simulator, worst error / scale over all cases (transcription's worst on that case): UNIT ms
1.9e-7 (1.0e-7), Vs 2.2e-5 (2.0e-5), weights 3.4e-5 (2.4e-5), change 1.3e-5 (9.7e-6); a = 0.98, c = 1.3: ms 8.0e-7
(8.0e-7), Vs 8.7e-5 (4.4e-5), weights 6.0e-5 (4.5e-5), change 5.0e-5 (2.4e-5)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import innovations_ref as nref  # noqa: E402
import robust_ref as rref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')
SEEDS = (0, 1, 2, 3, 4)


@pytest.fixture(scope='module')
def sessions():
    """The feature's five sessions as the five chains of one problem, and their Gaussian / robust (nu = 4, 8 passes)
    results."""
    S = [rref.outlier_session(seed) for seed in SEEDS]
    y, var, x = (np.concatenate([s[k] for s in S], axis=1) for k in ('y', 'var', 'x'))
    bad = np.stack([s['bad'] for s in S], axis=1)
    N = len(S)
    args = (np.zeros(N), np.full(N, 100.0), 1.0, 1.0, np.full(N, 2.0))
    gauss = rref.scalar_robust(y, var, *args, 4.0, 1)
    robust = rref.scalar_robust(y, var, *args, 4.0, 8)
    return dict(y=y, var=var, x=x, bad=bad, args=args, gauss=gauss, robust=robust)


# ---- the bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3)])
def test_bound_formula_against_its_terms_from_the_joint_posterior(D, O):
    T, K, nu = 6, 2, 4.0
    M = dense_case(K, D, O, False, seed=D + 3)
    rng = np.random.default_rng(D)
    y = rng.normal(size=(T, K, O)) * 2
    y[3, :, 0] += 15.0
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    par = tuple(M[k] for k in PARAMS)
    hist = []
    rref.dense_robust(y, var, *par, nu, 4, history=hist)
    worst = 0.0
    for i in (1, 3):
        lam, _ = hist[i]
        delta_prev = hist[i - 1][1]
        assert np.allclose(lam, (nu + 1) / (nu + delta_prev), rtol=1e-14)
        ll = nref.dense_innovations_sequential(y, rref._clip(var) / lam, *par)['loglik']
        got = rref.elbo(ll, delta_prev, nu)
        for k in range(K):
            want = rref.elbo_direct(y[:, k], var[:, k], *(p[k] for p in par), nu, delta_prev[:, k])
            worst = max(worst, abs(got[k] - want) / abs(want))
    print(f'D={D} O={O}: bound against its direct evaluation {worst:.3g}')
    assert worst < 1e-9


def test_bound_never_drops_over_32_passes(sessions):
    path = rref.scalar_elbo_path(sessions['y'], sessions['var'], *sessions['args'], 4.0, 32)
    steps = np.diff(path, axis=0)
    print(f'smallest step of the bound over 32 passes, seeds {SEEDS}: {steps.min():+.3g}')
    assert np.all(steps >= -1e-9 * np.maximum(1.0, np.abs(path[1:])))


def test_large_nu_is_the_gaussian_smoother(sessions):
    y, var, args = sessions['y'], sessions['var'], sessions['args']
    ms, Vs, lam, _ = rref.scalar_robust(y, var, *args, 1e12, 8)
    gm, gV = sessions['gauss'][:2]
    worst = max(np.abs(ms - gm).max() / np.abs(y).max(), (np.abs(Vs - gV) / gV).max(), np.abs(lam - 1).max())
    print(f'nu = 1e12, 8 passes, against the Gaussian smoother: {worst:.3g}')
    assert worst < 1e-9


def test_robust_smoother_recovers_the_truth_and_flags_the_displaced_frames(sessions):
    x, bad = sessions['x'], sessions['bad']
    rmse = lambda ms: np.sqrt(((ms - x) ** 2).mean(axis=0))
    rg, rr = rmse(sessions['gauss'][0]), rmse(sessions['robust'][0])
    lam = sessions['robust'][2]
    print(f'RMSE Gaussian {rg.round(2)}, robust {rr.round(2)}, ratio {(rr / rg).round(3)}; '
          f'displaced weights <= {lam[bad].max():.3g}, clean weights >= {lam[~bad].min():.3g}')
    assert np.all(rr <= 0.5 * rg)
    assert lam[bad].max() < 0.1 < lam[~bad].min()
    assert np.all(lam > 0) and np.all(lam <= 5.0 / 4.0)


def test_dense_reference_on_a_diagonal_model_is_the_scalar_one():
    pb = make_session(150, 3, 2, 2.0, False, seed=5, centre=3.0)
    T, K, D = pb['T'], pb['K'], pb['D']
    pb['y'][::37] += 30.0
    sc = rref.scalar_robust(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], 4.0, 8)
    worst = 0.0
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        dn = rref.dense_robust(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS), 4.0,
                               8, form=form)
        worst = max(worst, np.abs(dn[0].reshape(T, -1) - sc[0]).max() / np.abs(pb['y']).max(),
                    np.abs(np.diagonal(dn[1], axis1=2, axis2=3).reshape(T, -1) / sc[1] - 1).max(),
                    np.abs(dn[2].reshape(T, -1) - sc[2]).max(), np.abs(dn[3] - sc[3].reshape(K, D).max(axis=1)).max())
    print(f'dense against scalar reference: {worst:.3g}')
    assert worst < 1e-12


def test_continuation_pass_count_in_the_reference():
    """n1 passes then n2 passes from the returned weights are one call of n1 + n2 - 1 passes."""
    s = rref.outlier_session(7, T=300)
    whole = rref.scalar_robust(s['y'], s['var'], *s['args'], 4.0, 8)
    first = rref.scalar_robust(s['y'], s['var'], *s['args'], 4.0, 3)
    cont = rref.scalar_robust(s['y'], s['var'], *s['args'], 4.0, 6, lam0=first[2])
    for a, b in zip(whole, cont):
        assert np.array_equal(a, b)


# ---- the lane header from plain loops: a stand-alone program -----------------------------------------------------------
def _build_sim(path, extra):
    subprocess.run(['g++', '-std=c++17', *extra, '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'robust_sim.cpp'), '-o', path], check=True)
    return path


@pytest.fixture(scope='module')
def sims(tmp_path_factory):
    d = tmp_path_factory.mktemp('robust_sim')
    return dict(dir=d, plain=_build_sim(str(d / 'robust_sim'), ['-O2']),
                san=_build_sim(str(d / 'robust_sim_san'),
                               ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


@pytest.mark.parametrize('which', ['plain', 'san'])
def test_simulator_self_check(sims, which):
    """n_iters = 1 is bit for bit the smooth_tv bodies at w = 1 (elements, the scan's planes, outputs), weights 1 and
    change 0; 2 and 8 passes finite and in range; 3 then 6 passes are the bits of 8 - on workspaces of exactly the
    reported size, plain and under AddressSanitizer + UBSan."""
    r = subprocess.run([sims[which]], capture_output=True, text=True)
    assert r.returncode == 0 and 'robust_sim: ok' in r.stdout, r.stdout + r.stderr


def run_sim(sims, which, pb, B, nu, n_iters, lam0=None):
    T, N, D, K = pb['T'], pb['N'], pb['D'], pb['K']
    fin, fout = str(sims['dir'] / 'in.bin'), str(sims['dir'] / 'out.bin')
    par = pb['par']
    with open(fin, 'wb') as f:
        f.write(np.array([T, N, D, B, int(pb['unit']), n_iters, int(lam0 is not None)], np.int32).tobytes())
        f.write(np.array([nu], np.float64).tobytes())
        for a in (pb['y'], pb['var']) + (() if lam0 is None else (lam0,)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        for k in PARAMS:
            f.write(np.ascontiguousarray(par[k], np.float64).tobytes())
    r = subprocess.run([sims[which], fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, np.float32)
    assert out.size == 3 * T * N + K
    planes = out[:3 * T * N].reshape(3, T, N)
    return planes[0], planes[1], planes[2], out[3 * T * N:]


def displace(pb, seed):
    """About 2 % of the frames moved by 20 .. 60 px."""
    rng = np.random.default_rng(seed)
    hit = rng.random(pb['y'].shape) < 0.02
    pb['y'] = (pb['y'] + hit * rng.choice([-1.0, 1.0], hit.shape) * rng.uniform(20, 60, hit.shape)).astype(np.float32)
    return pb


@pytest.mark.parametrize('unit', [True, False])
def test_host_simulator_meets_the_float32_bar(sims, unit):
    worst = {}
    cases = [(T, B) for T in (1, 2, 5, 31, 32, 33, 129, 1000) for B in (4, 8, 16, 32)]
    for i, (T, B) in enumerate(cases):
        K, D = 3, 2
        pb = displace(make_session(T, K, D, 2.0, unit, seed=i), i)
        nu = (1.0, 4.0, 30.0)[i % 3]
        args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu)
        for n_iters in (2, 8):
            ref = list(rref.scalar_robust(*args, n_iters))
            r32 = list(rref.scalar_robust_f32(*args, n_iters, unit=unit))
            got = list(run_sim(sims, 'san' if i % 8 == 0 else 'plain', pb, B, nu, n_iters))
            ref[3], r32[3] = (c.reshape(K, D).max(axis=1) for c in (ref[3], r32[3]))
            bars = rref.bars(r32, ref, pb['y'])
            err, et = rref.errors(got, ref, pb['y']), rref.errors(r32, ref, pb['y'])
            for k in err:
                e = float(np.max(err[k]))
                if e > worst.get(k, (0.0, 0.0))[0]:
                    worst[k] = (e, float(np.max(et[k])))
                assert e <= bars[k], f'{k}: {e:.3g} over the bar {bars[k]:.3g} at T={T} B={B} nu={nu} n_iters={n_iters}'
            assert np.all(got[2] > 0) and np.all(got[2] <= np.float32((nu + 1) / nu))
    print(f'unit={unit}: host simulator worst error / scale (transcription on that case): '
          + ', '.join(f'{k} {v[0]:.2g} ({v[1]:.2g})' for k, v in worst.items()))


def test_simulator_single_pass_under_given_weights_is_the_smoother_on_var_over_weights(sims):
    pb = displace(make_session(200, 3, 2, 2.0, True, seed=3), 3)
    lam = np.random.default_rng(0).uniform(0.05, 1.25, pb['y'].shape).astype(np.float32)
    ms, Vs, out_lam, change = run_sim(sims, 'plain', pb, 32, 4.0, 1, lam0=lam)
    assert np.array_equal(out_lam, lam) and not change.any()
    args = (pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], np.ones(200))
    var_eff = pb['var'].astype(np.float64) / lam
    rms, rVs = tref.scalar_smooth_tv(pb['y'], var_eff, *args)
    bars = tref.f32_bars(*tref.scalar_smooth_tv_f32(pb['y'], (pb['var'] * (np.float32(1) / lam)), *args, unit=True), rms,
                         rVs, pb['y'])
    err = tref.f32_errors(ms, Vs, rms, rVs, pb['y'])
    assert float(err['ms'].max()) <= bars['ms'] and float(err['Vs'].max()) <= bars['Vs']


# ---- the C ABI's refusals (returned before anything touches a device) ------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_c_abi_refusals_need_no_device(lib):
    from eks_amd import _lib
    d = lambda K, T, D, O, fl: _lib.EksDims(K, T, D, O, fl)
    DIAG, VSD, UNIT = _lib.FLAG_DIAG_MODEL, _lib.FLAG_VS_DIAG, _lib.FLAG_UNIT_AC
    wsb = lambda dims: lib.eks_smooth_robust_workspace_bytes(ctypes.byref(dims))
    tvb = lambda dims: lib.eks_smooth_tv_workspace_bytes(ctypes.byref(dims))
    good = d(3, 100, 2, 2, DIAG | UNIT)
    plane = lambda n: (n * 4 + 255) // 256 * 256
    assert wsb(good) == tvb(good) + plane(100 * 6) + plane(100) > 0                 # .. the plane and the ones
    assert wsb(d(3, 100, 3, 4, 0)) == tvb(d(3, 100, 3, 4, 0)) + plane(100 * 12) > 0
    assert wsb(d(3, 100, 7, 7, 0)) == 0 and wsb(d(3, 100, 2, 65, 0)) == 0           # D > 6, O > 64: unsupported
    assert wsb(d(0, 100, 2, 2, DIAG)) == 0 and wsb(d(3, 100, 2, 3, DIAG)) == 0
    assert wsb(d(3, 100, 9, 9, DIAG)) == 0 and wsb(d(3, 100, 9, 9, DIAG | VSD)) > 0  # full Vs rows: D <= 8
    one = ctypes.c_void_p(16)                                                        # non-NULL, never dereferenced
    null = ctypes.c_void_p(0)

    def call(dims, null_at=None, nu=4.0, n_iters=8, weights=one, weights_in=0, change=one, ws=one, ws_bytes=1 << 40):
        ptrs = [one] * 8                                                             # y, var, m0 .. s
        out = [one, one]                                                             # ms, Vs
        if null_at is not None:
            if null_at < 8:
                ptrs[null_at] = null
            else:
                out[null_at - 8] = null
        return lib.eks_smooth_robust(ctypes.byref(dims), *ptrs, nu, n_iters, weights, weights_in, change, *out, ws,
                                     ws_bytes, None)

    assert lib.eks_smooth_robust(None, *[one] * 8, 4.0, 8, one, 0, one, one, one, one, 1, None) == -1
    for i in range(10):
        assert call(good, null_at=i) == -1, i
    assert call(good, weights=null, weights_in=1) == -1                              # weights_in needs weights
    for nu in (0.0, -1.0, float('nan'), float('inf')):
        assert call(good, nu=nu) == -2, nu
    assert call(good, n_iters=0) == -2 and call(good, n_iters=-3) == -2
    assert call(d(3, 0, 2, 2, DIAG)) == -2 and call(d(3, 100, 2, 3, DIAG)) == -2
    assert call(d(3, 100, 2, 2, UNIT)) == -3                                         # UNIT_AC without DIAG_MODEL
    assert call(d(3, 100, 7, 7, 0)) == -3 and call(d(3, 100, 2, 65, 0)) == -3 and call(d(3, 100, 9, 9, DIAG)) == -3
    assert call(good, ws=null) == -4 and call(good, ws_bytes=wsb(good) - 1) == -4
    assert call(good, ws_bytes=tvb(good)) == -4                                      # eks_smooth_tv's size is too small
    assert call(d(3, 100, 3, 4, 0), ws_bytes=wsb(d(3, 100, 3, 4, 0)) - 1) == -4


# ---- the Python surface's argument checks (raised before a device is asked for) --------------------------------------
def test_python_argument_checks():
    import eks_amd
    from eks_amd import robust
    assert eks_amd.smooth_robust is robust.smooth_robust
    assert eks_amd.smooth_singlecam_robust is robust.smooth_singlecam_robust
    K, T, D = 2, 6, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    args = (np.zeros((K, T, D)), np.zeros((K, D)), eye, eye, eye, eye, np.ones((T, K, D)), 1.0)
    for kw in (dict(nu=0.0), dict(nu=-2.0), dict(nu=np.nan), dict(nu=np.inf), dict(n_iters=0), dict(n_iters=2.5),
               dict(tol=0.0), dict(tol=np.nan), dict(tol=1e-3, max_iters=4), dict(tol=1e-3, max_iters=9.5),
               dict(tol=1e-3, n_iters=1)):
        with pytest.raises(ValueError):
            robust.smooth_robust(*args, **kw)
    with pytest.raises(ValueError):
        robust.smooth_robust(args[0], args[1], eye, eye, eye, eye, np.ones((T + 1, K, D)), 1.0)
    with pytest.raises(NotImplementedError):
        robust.smooth_robust(*args, h_fn=lambda x: x)
    from eks_amd.marker_array import MarkerArray
    ma = MarkerArray(np.zeros((2, 1, T, K, 3)), data_fields=['x', 'y', 'likelihood'])
    with pytest.raises(ValueError):
        robust.smooth_singlecam_robust(ma, ['a'], 1.0)
    with pytest.raises(ValueError):
        robust.smooth_singlecam_robust(ma, ['a', 'b'], 1.0, nu=0.0)
    with pytest.raises(ValueError):
        robust.smooth_singlecam_robust(MarkerArray(np.zeros((2, 2, T, K, 3)), data_fields=['x', 'y', 'likelihood']),
                                       ['a', 'b'], 1.0)
