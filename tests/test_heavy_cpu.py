"""CPU: eks_smooth_heavy without a GPU - the variational bound of tests/heavy_ref.py against its term-by-term
evaluation from the joint posterior, its monotonicity over 32 passes, the two single-sided limits against
tests/robust_ref.py and tests/jumps_ref.py, the dense references against the scalar one, what the model buys on the
feature's session (six true jumps AND twelve displaced frames), the float32 lane arithmetic of
eks_amd/csrc/eks_smooth_student_lane.hpp run from plain loops by the stand-alone tests/host_sim/heavy_sim.cpp (plain and
under -fsanitize=address,undefined; never loaded into this process), the C ABI's refusals against eks_smooth_jumps' and
the Python argument checks.

Float32 bar (heavy_ref.bars), the project's rule: error / scale <= max(1e-5, 4 x the float32 NumPy transcription's own
worst error / scale on the same inputs); ms over the chain's max |y|, Vs over its own value, weights, u = 1 / scales
and change over 1.  The transcription is the yardstick, never the simulator.

Pass counts: a call of n passes updates the planes n - 1 times, and a continued call's first pass smooths again under
the planes it was given, so n1 passes followed by n2 passes are one call of n1 + n2 - 1 passes (3 then 6 = 8).

The session, measured on the float64 reference (seeds 0 .. 7, 12 passes, nu 4 / 4): RMSE 0.350 .. 0.390 px against
3.58 .. 3.97 for the Gaussian smoother (this iteration with the scale update off: 5.09 .. 8.76; with the weight
update off: 6.03 .. 6.72); scales at the six jumps >= 2 919, on a displaced frame and the frame after it <= 1.16,
elsewhere <= 1.70; weights on displaced frames <= 0.033, on clean frames >= 0.240; smallest step of the bound
+0.0102."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heavy_ref as href  # noqa: E402
import jumps_ref as jref  # noqa: E402
import robust_ref as rref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')
SEEDS = tuple(range(8))
FORMS = (tref.dense_smooth_tv, tref.dense_smooth_tv_joint)


# ---- the bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3)])
def test_bound_equals_its_direct_evaluation(D, O):
    T, K = 6, 2
    M = dense_case(K, D, O, False, seed=D + 11)
    par = tuple(M[k] for k in PARAMS)
    rng = np.random.default_rng(D)
    y = rng.normal(size=(T, K, O)) * 2
    y[3:] += 9.0
    y[2, :, 0] -= 14.0
    var = np.exp(rng.normal(0.0, 0.6, (T, K, O)))
    for form in FORMS:
        hist = []
        href.dense_heavy(y, var, *par, 3.0, 5.0, 4, form=form, history=hist)
        path = href.elbo_path(hist, 3.0, 5.0, D)
        for i in range(1, len(hist)):
            for k in range(K):
                want = href.elbo_direct(y[:, k], var[:, k], *(p[k] for p in par), 3.0, 5.0, hist[i - 1][2][:, k],
                                        hist[i - 1][3][:, k])
                rel = abs(path[i - 1][k] - want) / abs(want)
                assert rel < 1e-9, (form.__name__, i, k, path[i - 1][k], want)


@pytest.fixture(scope='module')
def sessions():
    out = []
    for seed in SEEDS:
        s = href.heavy_session(seed)
        gauss = href.scalar_heavy(s['y'], s['var'], *s['args'], 4.0, 4.0, 1, D=2)
        heavy = href.scalar_heavy(s['y'], s['var'], *s['args'], 4.0, 4.0, 12, D=2)
        out.append(dict(s=s, gauss=gauss, heavy=heavy))
    return out


def test_bound_never_drops_over_32_passes():
    s = href.heavy_session(0)
    hist = []
    href.scalar_heavy(s['y'], s['var'], *s['args'], 4.0, 4.0, 32, D=2, history=hist)
    path = href.elbo_path(hist, 4.0, 4.0, 2)
    steps = np.diff(path, axis=0)
    print(f'smallest step of the bound over 32 passes: {steps.min():+.3g}')
    assert np.all(steps >= -1e-9 * np.abs(path[1:]))


# ---- the single-sided limits and the dense forms ----------------------------------------------------------------------
def test_large_nu_proc_is_the_robust_reference(sessions):
    s = sessions[0]['s']
    y, var = s['y'], s['var']
    ms, Vs, lam, w, ch = href.scalar_heavy(y, var, *s['args'], 4.0, 1e12, 8, D=2)
    rm, rV, rl, rc = rref.scalar_robust(y, var, *s['args'], 4.0, 8)
    worst = max(np.abs(ms - rm).max() / np.abs(y).max(), (np.abs(Vs - rV) / rV).max(), np.abs(lam - rl).max(),
                np.abs(w - 1).max(), abs(ch[0, 0] - rc.max()))
    print(f'nu_proc = 1e12 against robust_ref: {worst:.3g}')
    assert worst < 1e-8


def test_large_nu_obs_is_the_jumps_reference(sessions):
    s = sessions[0]['s']
    y, var = s['y'], s['var']
    ms, Vs, lam, w, ch = href.scalar_heavy(y, var, *s['args'], 1e12, 4.0, 8, D=2)
    jm, jV, jw, jc = jref.scalar_jumps(y, var, *s['args'], 4.0, 8, D=2)
    worst = max(np.abs(ms - jm).max() / np.abs(y).max(), (np.abs(Vs - jV) / jV).max(), np.abs(lam - 1).max(),
                np.abs(1 / w - 1 / jw).max(), np.abs(ch[1] - jc).max())
    print(f'nu_obs = 1e12 against jumps_ref: {worst:.3g}')
    assert worst < 1e-8


def heavy_problem(T, K, D, unit, seed, sval=0.05, centre=50.0):
    """make_session with true jumps (jumps_ref.add_jumps) and displaced single frames (observations only), never
    adjacent to each other."""
    pb = make_session(T, K, D, sval, unit, seed=seed, centre=centre)
    jumps = [(t, k) for t, k in jref.random_jumps(T, K, seed)]
    pb = jref.add_jumps(pb, jumps, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    y = pb['y'].astype(np.float64)
    near = {(t + dt, k) for t, k in jumps for dt in (-1, 0, 1)}
    for t, k in jref.random_jumps(T, K, seed + 500, rate=0.02):
        if (t, k) in near or T < 3:
            continue
        near |= {(t - 1, k), (t, k), (t + 1, k)}
        sl = slice(k * D, (k + 1) * D)
        y[t, sl] += pb['c'][sl] * rng.choice([-1.0, 1.0], D) * rng.uniform(20.0, 60.0, D)
    pb['y'] = np.ascontiguousarray(y, np.float32)
    return pb


def test_dense_references_on_a_diagonal_model_are_the_scalar_one():
    pb = heavy_problem(150, 3, 2, False, seed=5, centre=3.0)
    T, K, D = pb['T'], pb['K'], pb['D']
    sc = href.scalar_heavy(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], 3.0, 5.0, 8, D=D)
    worst = 0.0
    for form in FORMS:
        dn = href.dense_heavy(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS), 3.0,
                              5.0, 8, form=form)
        worst = max(worst, np.abs(dn[0].reshape(T, -1) - sc[0]).max() / np.abs(pb['y']).max(),
                    np.abs(np.diagonal(dn[1], axis1=2, axis2=3).reshape(T, -1) / sc[1] - 1).max(),
                    np.abs(dn[2].reshape(T, -1) - sc[2]).max(), np.abs(1 / dn[3] - 1 / sc[3]).max(),
                    np.abs(dn[4] - sc[4]).max())
    print(f'dense against scalar reference: {worst:.3g}')
    assert worst < 1e-10


def test_continuation_pass_count_in_the_reference():
    s = href.heavy_session(7)
    whole = href.scalar_heavy(s['y'], s['var'], *s['args'], 4.0, 4.0, 8, D=2)
    first = href.scalar_heavy(s['y'], s['var'], *s['args'], 4.0, 4.0, 3, D=2)
    cont = href.scalar_heavy(s['y'], s['var'], *s['args'], 4.0, 4.0, 6, D=2, lam0=first[2], w0=first[3])
    for a, b in zip(whole, cont):
        assert np.array_equal(a, b)


# ---- the feature's session ---------------------------------------------------------------------------------------------
def test_session_with_jumps_and_displaced_frames(sessions):
    for S in sessions:
        s = S['s']
        ms, _, lam, w, _ = S['heavy']
        w = w[:, 0]
        T = len(w)
        rmse = lambda m: float(np.sqrt(((m - s['x']) ** 2).mean()))
        rg, rh = rmse(S['gauss'][0]), rmse(ms)
        bad, jumps = s['bad'], s['jumps']
        after = np.unique(np.concatenate([bad, bad + 1]))
        other = np.setdiff1d(np.arange(1, T), np.concatenate([jumps, after]))
        clean = np.setdiff1d(np.arange(T), bad)
        print(f'RMSE Gaussian {rg:.3g}, heavy {rh:.3g}; scales at the jumps >= {w[jumps].min():.4g}, on displaced frames '
              f'and the next <= {w[after].max():.3g}, elsewhere <= {w[other].max():.3g}; weights on displaced frames <= '
              f'{lam[bad].max():.3g}, on clean frames >= {lam[clean].min():.3g}')
        assert len(bad) == 14 and len(jumps) == 6
        assert np.all(w[jumps] >= 100.0)
        assert np.all(w[after] <= 3.0)
        assert np.all(w[other] <= 3.0)
        assert np.all(lam[bad] <= 0.1)
        assert np.all(lam[clean] >= 0.1)
        assert rh <= rg / 4.0
        assert w[0] == 1.0


# ---- the lane header from plain loops: a stand-alone program -----------------------------------------------------------
def _build_sim(path, extra):
    subprocess.run(['g++', '-std=c++17', *extra, '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'heavy_sim.cpp'), '-o', path], check=True)
    return path


@pytest.fixture(scope='module')
def sims(tmp_path_factory):
    d = tmp_path_factory.mktemp('heavy_sim')
    return dict(dir=d, plain=_build_sim(str(d / 'heavy_sim'), ['-O2']),
                san=_build_sim(str(d / 'heavy_sim_san'),
                               ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


@pytest.mark.parametrize('which', ['plain', 'san'])
def test_simulator_self_check(sims, which):
    """Chunk lengths 4 .. 32, T = 1 .. 1000, unit chains and a = 0.98, c = 1.3: n_iters = 1 gives weights 1, scales 1,
    change 0 and the bits of the smooth_tv bodies at w = 1; a middle pass writes every contribution of rows 1 .. T-1
    of a poisoned plane; 2 and 8 passes finite and in range; 3 then 6 passes are the bits of 8 - on planes of exactly
    the stated sizes, plain and under AddressSanitizer + UBSan."""
    r = subprocess.run([sims[which]], capture_output=True, text=True)
    assert r.returncode == 0 and 'heavy_sim: ok' in r.stdout, r.stdout + r.stderr


def run_sim(sims, which, pb, B, nu_obs, nu_proc, n_iters, lam0=None, w0=None):
    T, N, D, K = pb['T'], pb['N'], pb['D'], pb['K']
    fin, fout = str(sims['dir'] / 'in.bin'), str(sims['dir'] / 'out.bin')
    par = pb['par']
    with open(fin, 'wb') as f:
        f.write(np.array([T, N, D, B, int(pb['unit']), n_iters, int(lam0 is not None) + 2 * int(w0 is not None)],
                         np.int32).tobytes())
        f.write(np.array([nu_obs, nu_proc], np.float64).tobytes())
        for a in (pb['y'], pb['var']) + (() if lam0 is None else (lam0,)) + (() if w0 is None else (w0,)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        for k in PARAMS:
            f.write(np.ascontiguousarray(par[k], np.float64).tobytes())
    r = subprocess.run([sims[which], fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, np.float32)
    assert out.size == 3 * T * N + T * K + 2 * K
    TN = T * N
    return (out[:TN].reshape(T, N), out[TN:2 * TN].reshape(T, N), out[2 * TN:3 * TN].reshape(T, N),
            out[3 * TN:3 * TN + T * K].reshape(T, K), out[3 * TN + T * K:].reshape(2, K))


@pytest.mark.parametrize('unit', [True, False])
def test_host_simulator_meets_the_float32_bar(sims, unit):
    worst = {}
    cases = [(T, B) for T in (1, 2, 5, 31, 32, 33, 129, 1000) for B in (4, 8, 16, 32)]
    for i, (T, B) in enumerate(cases):
        K, D = 3, 2
        pb = heavy_problem(T, K, D, unit, seed=i)
        nu_obs, nu_proc = ((1.0, 30.0), (4.0, 4.0), (30.0, 1.0))[i % 3]
        args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu_obs, nu_proc)
        for n_iters in (2, 8):
            ref = href.scalar_heavy(*args, n_iters, D=D)
            r32 = href.scalar_heavy_f32(*args, n_iters, D=D, unit=unit, B=B)
            got = run_sim(sims, 'san' if i % 8 == 0 else 'plain', pb, B, nu_obs, nu_proc, n_iters)
            bars = href.bars(r32, ref, pb['y'], D)
            err, et = href.errors(got, ref, pb['y'], D), href.errors(r32, ref, pb['y'], D)
            for k in err:
                e = float(np.max(err[k]))
                if e > worst.get(k, (0.0, 0.0))[0]:
                    worst[k] = (e, float(np.max(et[k])))
                assert e <= bars[k], (f'{k}: {e:.3g} over the bar {bars[k]:.3g} at T={T} B={B} nu={nu_obs}/{nu_proc} '
                                      f'n_iters={n_iters}')
            u = 1.0 / got[3].astype(np.float64)
            assert np.all(u > 0) and np.all(u <= (nu_proc + D) / nu_proc * (1 + 1e-7))
            assert np.all(got[2] > 0) and np.all(got[2] <= np.float32((nu_obs + 1) / nu_obs))
    print(f'unit={unit}: host simulator worst error / scale (transcription on that case): '
          + ', '.join(f'{k} {v[0]:.2g} ({v[1]:.2g})' for k, v in worst.items()))


# ---- the C ABI's refusals (returned before anything touches a device) ------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_entry_points_declared_bound_and_exported(lib):
    from eks_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_smooth_heavy', 'eks_smooth_heavy_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name) is not None


def test_c_abi_refusals_are_those_of_eks_smooth_jumps(lib):
    """Every defect and defect pair tests/test_api_refusals_cpu.py tries on eks_smooth_jumps, on host buffers: the
    status of eks_smooth_heavy must be eks_smooth_jumps' for the same defect - with a bad nu on either side - and the
    size queries must refuse the same shapes.  Then the planes_in cases."""
    from eks_amd import _lib
    import test_api_refusals_cpu as api
    buf = ctypes.create_string_buffer(64)
    one, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    dref = lambda dims: None if dims is None else ctypes.byref(_lib.EksDims(*dims))
    names = api.MODEL + ['ms', 'Vs']

    def jumps(dims, nu=4.0, n_iters=8, plane_in=0, plane=null, ws=one, ws_bytes=1 << 40, **nulls):
        p = [null if nulls.get(n) else one for n in names]
        return int(lib.eks_smooth_jumps(dref(dims), *p[:8], nu, n_iters, plane, plane_in, null, *p[8:], ws, ws_bytes, None))

    def heavy(dims, nu=(4.0, 4.0), n_iters=8, planes_in=0, weights=null, scales=null, ws=one, ws_bytes=1 << 40, **nulls):
        p = [null if nulls.get(n) else one for n in names]
        return int(lib.eks_smooth_heavy(dref(dims), *p[:8], nu[0], nu[1], n_iters, weights, scales, planes_in, null, *p[8:],
                                        ws, ws_bytes, None))

    qj = lambda dims: int(lib.eks_smooth_jumps_workspace_bytes(dref(dims)))
    qh = lambda dims: int(lib.eks_smooth_heavy_workspace_bytes(dref(dims)))
    chain_T = api._first_refused_T(lib, 1 << 22, 2, 2, api.DIAG | api.VSD)
    dense_T = api._first_refused_T(lib, 5000000, 3, 4, 0)
    chain_limit = (1 << 22, chain_T, 2, 2, api.DIAG | api.VSD)
    dense_limit = (5000000, dense_T, 3, 4, 0)
    n = 0

    def same(dims, **kw):
        """eks_smooth_jumps' status for the defect; eks_smooth_heavy's for it alone and with either nu bad too."""
        nonlocal n
        want = jumps(dims, **kw)
        assert want != 0
        assert heavy(dims, **kw) == want, (dims, kw)
        if 'nu' not in kw:
            for bad in (0.0, -1.0, float('inf'), float('nan')):
                wj = jumps(dims, nu=bad, **kw)
                assert heavy(dims, nu=(bad, 4.0), **kw) == wj and heavy(dims, nu=(4.0, bad), **kw) == wj, (dims, kw, bad)
        n += 1

    for name, dims in dict(chains=api.CHAINS, chains_no_vs_diag=api.CHAINS[:4] + (api.DIAG,), general=api.GENERAL,
                           **api.UNSUPPORTED_DIMS, **api.BAD_DIMS, chain_limit=chain_limit,
                           dense_limit=dense_limit).items():
        assert (qh(dims) > 0) == (qj(dims) > 0), name
    for dims in api.BAD_DIMS.values():
        same(dims)
        same(dims, y=True)
    for dims in api.UNSUPPORTED_DIMS.values():
        same(dims)
    same(chain_limit)
    same(dense_limit)
    for lim, T in ((chain_limit, chain_T), (dense_limit, dense_T)):
        assert heavy(lim[:1] + (T - 1,) + lim[2:], ws=null) == jumps(lim[:1] + (T - 1,) + lim[2:], ws=null) == -4
    for dims in (api.CHAINS, api.GENERAL):
        for a in names:
            same(dims, **{a: True})
        same(dims, ws=null)
        same(dims, y=True, ws=null)
        assert heavy(dims, ws_bytes=qh(dims) - 1) == jumps(dims, ws_bytes=qj(dims) - 1) == -4
        assert heavy(dims, ws=null, ws_bytes=qh(dims) - 1) == jumps(dims, ws=null, ws_bytes=qj(dims) - 1) == -4
        assert heavy(dims, ws_bytes=qj(dims)) == -4            # eks_smooth_jumps' size is too small
        for bad in (0.0, -1.0, float('inf'), float('nan')):
            for nu in ((bad, 4.0), (4.0, bad), (bad, bad)):
                assert heavy(dims, nu=nu) == jumps(dims, nu=bad) == -2
                assert heavy(dims, nu=nu, y=True) == jumps(dims, nu=bad, y=True) == -2
        same(dims, n_iters=0)
        same(dims, n_iters=0, Vs=True)
        # planes_in: a bit set with a NULL plane is eks_smooth_jumps' scales_in = 1 without scales
        for bits, kw in ((1, dict(scales=one)), (2, dict(weights=one)), (3, dict(weights=one)), (3, dict(scales=one)),
                         (3, dict())):
            assert heavy(dims, planes_in=bits, **kw) == jumps(dims, plane_in=1) == -1
            assert heavy(dims, planes_in=bits, s=True, **kw) == jumps(dims, plane_in=1, s=True) == -1
            assert heavy(dims, planes_in=bits, ws=null, **kw) == jumps(dims, plane_in=1, ws=null) == -1
            assert heavy(dims, planes_in=bits, nu=(0.0, 4.0), **kw) == jumps(dims, plane_in=1, nu=0.0) == -2
        # with the planes there the call gets as far as the workspace
        assert heavy(dims, planes_in=3, weights=one, scales=one, ws=null) == -4
    assert n >= 40
    # the size query holds both planes whether or not the caller passes them
    plane = lambda cnt, e=4: (cnt * e + 255) // 256 * 256
    tvb = lambda dims: int(lib.eks_smooth_tv_workspace_bytes(dref(dims)))
    g = (3, 100, 2, 2, api.DIAG | api.UNIT)
    assert qh(g) == tvb(g) + 2 * plane(100 * 6) + plane(100 * 3)
    g = (3, 100, 3, 4, 0)
    assert qh(g) == tvb(g) + plane(100 * 3 * 4) + plane(100 * 3) + plane(100 * 3, 8)


# ---- the Python surface's argument checks (raised before a device is asked for) --------------------------------------
def test_python_argument_checks():
    import eks_amd
    from eks_amd import heavy_tails, hip_ops
    assert eks_amd.smooth_heavy_tailed is heavy_tails.smooth_heavy_tailed
    assert eks_amd.smooth_singlecam_heavy_tailed is heavy_tails.smooth_singlecam_heavy_tailed
    assert callable(hip_ops.smooth_heavy)
    K, T, D = 2, 6, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    args = (np.zeros((K, T, D)), np.zeros((K, D)), eye, eye, eye, eye, np.ones((T, K, D)), 1.0)
    for kw in (dict(nu_obs=0.0), dict(nu_proc=-2.0), dict(nu_obs=np.nan), dict(nu_proc=np.inf), dict(n_iters=0),
               dict(n_iters=2.5), dict(tol=0.0), dict(tol=np.nan), dict(tol=1e-3, max_iters=4),
               dict(tol=1e-3, max_iters=9.5), dict(tol=1e-3, n_iters=1)):
        with pytest.raises(ValueError):
            heavy_tails.smooth_heavy_tailed(*args, **kw)
    with pytest.raises(ValueError):
        heavy_tails.smooth_heavy_tailed(args[0], args[1], eye, eye, eye, eye, np.ones((T + 1, K, D)), 1.0)
    with pytest.raises(NotImplementedError):
        heavy_tails.smooth_heavy_tailed(*args, h_fn=lambda x: x)
    from eks_amd.marker_array import MarkerArray
    ma = MarkerArray(np.zeros((2, 1, T, K, 3)), data_fields=['x', 'y', 'likelihood'])
    with pytest.raises(ValueError):
        heavy_tails.smooth_singlecam_heavy_tailed(ma, ['a'], 1.0)
    with pytest.raises(ValueError):
        heavy_tails.smooth_singlecam_heavy_tailed(ma, ['a', 'b'], 1.0, nu_proc=0.0)
    with pytest.raises(ValueError):
        heavy_tails.smooth_singlecam_heavy_tailed(MarkerArray(np.zeros((2, 2, T, K, 3)),
                                                              data_fields=['x', 'y', 'likelihood']), ['a', 'b'], 1.0)
