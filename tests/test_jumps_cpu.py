"""CPU: eks_smooth_jumps without a GPU - delta_t of tests/jumps_ref.py against the joint Gaussian posterior by plain
linear algebra (random scales, singular Q), the variational bound's monotonicity over 32 passes, the Gaussian limit,
what the method buys on the feature's session with six true jumps, the dense reference against the scalar one, the
continuation pass counts, the float32 lane arithmetic of eks_amd/csrc/eks_smooth_student_lane.hpp run from plain loops by
the stand-alone tests/host_sim/jumps_sim.cpp (plain and under -fsanitize=address,undefined; never loaded into this
process), the C ABI's refusals and size queries, and the Python argument checks.

Float32 bar (jumps_ref.bars), the project's rule: error / scale <= max(1e-5, 4 x the float32 NumPy transcription's own
worst error / scale on the same inputs); ms over the chain's max |y|, Vs over its own value, u = 1 / scales and change
over 1.  The transcription is the yardstick, never the simulator.

Pass counts: a call of n passes updates the scales n - 1 times, and a continued call's first pass smooths again under
the scales it was given, so n1 passes followed by n2 passes are one call of n1 + n2 - 1 passes (3 then 6 = 8)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jumps_ref as jref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')
SEEDS = (0, 1, 2)
FORMS = (tref.dense_smooth_tv, tref.dense_smooth_tv_joint)


# ---- delta against the joint posterior -----------------------------------------------------------------------------------
@pytest.mark.parametrize('D,O,singular_q', [(1, 1, False), (2, 3, False), (3, 4, False), (6, 12, False),
                                            (2, 3, True), (3, 4, True), (6, 12, True)])
def test_delta_of_both_dense_forms_against_the_joint_posterior(D, O, singular_q):
    """(A singular 1 x 1 Q is zero: the scalar s q = 0 case below.)"""
    T, K = 7, 2
    M = dense_case(K, D, O, singular_q, seed=D + 3)
    rng = np.random.default_rng(D)
    y = rng.normal(size=(T, K, O)) * 2
    y[3:] += 15.0
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    w = np.exp(rng.normal(0.0, 1.5, (T, K)))
    par = tuple(M[k] for k in PARAMS)
    worst = 0.0
    for form in FORMS:
        ms, Vs, delta, _ = jref.dense_pass(y, var, *par, w, form)
        rm, rV = form(y, var, *par, w)
        assert np.array_equal(ms, rm) and np.array_equal(Vs, rV)
        for k in range(K):
            want = jref.joint_delta(y[:, k], var[:, k], *(p[k] for p in par), w[:, k])
            worst = max(worst, np.abs(delta[1:, k] - want[1:]).max() / np.abs(want[1:]).max())
    print(f'D={D} O={O} singular={singular_q}: delta against the joint posterior {worst:.3g}')
    assert worst < 1e-9


def test_scalar_delta_against_the_joint_posterior_with_a_noiseless_chain():
    """Two chains sharing one weight; the second has s q = 0 and contributes w_t, its prior value."""
    T, D = 8, 2
    rng = np.random.default_rng(2)
    y = rng.normal(size=(T, D)) * 2
    y[4:] += 12.0
    var = np.exp(rng.normal(0.0, 0.5, (T, D)))
    w = np.exp(rng.normal(0.0, 1.0, (T, 1)))
    a, c, qs = np.array([0.95, 0.9]), np.array([1.2, 0.8]), np.array([0.7, 0.0])
    m0, S0 = np.array([0.3, -0.2]), np.array([2.0, 3.0])
    _, _, delta, _ = jref.scalar_pass(y, var, m0, S0, a, c, qs, w, D)
    want = jref.joint_delta(y, var, m0, np.diag(S0), np.diag(a), np.diag(c), np.diag(qs), 1.0, w[:, 0])
    assert np.abs(delta[1:, 0] - want[1:]).max() < 1e-10 * np.abs(want).max()
    # no data: the term is w_t, so w = 1 is the fixed point
    _, _, d0, _ = jref.scalar_pass(y, np.full((T, D), 1e30), m0, S0, a, c, qs, w, D)
    assert np.abs(d0[1:, 0] - D * w[1:, 0]).max() < 1e-9


# ---- the feature's session -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sessions():
    out = []
    for seed in SEEDS:
        s = jref.jump_session(seed)
        hist = []
        gauss = jref.scalar_jumps(s['y'], s['var'], *s['args'], 4.0, 1, D=2)
        jumps = jref.scalar_jumps(s['y'], s['var'], *s['args'], 4.0, 12, D=2, history=hist)
        out.append(dict(s=s, gauss=gauss, jumps=jumps, hist=hist))
    return out


def test_jump_session_scales_and_rmse(sessions):
    for S in sessions:
        s, w = S['s'], S['jumps'][2][:, 0]
        rmse = lambda ms: float(np.sqrt(((ms - s['x']) ** 2).mean()))
        rg, rj = rmse(S['gauss'][0]), rmse(S['jumps'][0])
        calm = np.ones(len(w), bool)
        calm[s['frames']] = False
        print(f'RMSE Gaussian {rg:.3g}, jumps {rj:.3g} (ratio {rj / rg:.3g}); scales at the jumps '
              f'{w[s["frames"]].min():.4g} .. {w[s["frames"]].max():.4g}, elsewhere <= {w[calm].max():.3g}, median '
              f'{np.median(w[calm]):.3g}; last change {S["jumps"][3][0]:.3g}')
        assert np.all(w[s['frames']] >= 100.0)
        assert np.all(w[calm] <= 3.0)
        assert rj <= rg / 3.0
        assert w[0] == 1.0


def test_bound_never_drops_over_32_passes():
    s = jref.jump_session(0, T=300)
    hist = []
    jref.scalar_jumps(s['y'], s['var'], *s['args'], 4.0, 32, D=2, history=hist)
    path = jref.elbo_path(hist, 4.0, 2)
    steps = np.diff(path, axis=0)
    print(f'smallest step of the bound over 32 passes: {steps.min():+.3g}')
    assert np.all(steps >= -1e-9 * np.maximum(1.0, np.abs(path[1:])))
    M = dense_case(2, 2, 3, False, seed=4)
    rng = np.random.default_rng(0)
    y = rng.normal(size=(40, 2, 3)) * 2
    y[17:] += 25.0
    hist = []
    jref.dense_jumps(y, np.exp(rng.normal(0, 0.5, y.shape)), *(M[k] for k in PARAMS), 4.0, 32, history=hist)
    path = jref.elbo_path(hist, 4.0, 2)
    assert np.all(np.diff(path, axis=0) >= -1e-9 * np.maximum(1.0, np.abs(path[1:])))


def test_large_nu_is_the_gaussian_smoother(sessions):
    S = sessions[0]
    s = S['s']
    ms, Vs, w, _ = jref.scalar_jumps(s['y'], s['var'], *s['args'], 1e12, 8, D=2)
    gm, gV = S['gauss'][:2]
    worst = max(np.abs(ms - gm).max() / np.abs(s['y']).max(), (np.abs(Vs - gV) / gV).max(), np.abs(w - 1).max())
    print(f'nu = 1e12, 8 passes, against the Gaussian smoother: {worst:.3g}')
    assert worst < 1e-8


def test_dense_reference_on_a_diagonal_model_is_the_scalar_one():
    pb = make_session(150, 3, 2, 0.05, False, seed=5, centre=3.0)
    pb = jref.add_jumps(pb, [(1, 0), (60, 1), (61, 1), (149, 2)], seed=5)
    T, K, D = pb['T'], pb['K'], pb['D']
    sc = jref.scalar_jumps(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], 4.0, 8, D=D)
    worst = 0.0
    for form in FORMS:
        dn = jref.dense_jumps(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS), 4.0,
                              8, form=form)
        worst = max(worst, np.abs(dn[0].reshape(T, -1) - sc[0]).max() / np.abs(pb['y']).max(),
                    np.abs(np.diagonal(dn[1], axis1=2, axis2=3).reshape(T, -1) / sc[1] - 1).max(),
                    np.abs(1 / dn[2] - 1 / sc[2]).max(), np.abs(dn[3] - sc[3]).max())
    print(f'dense against scalar reference: {worst:.3g}')
    assert worst < 1e-10


def test_continuation_pass_count_in_the_reference():
    """n1 passes then n2 passes from the returned scales are one call of n1 + n2 - 1 passes."""
    s = jref.jump_session(7, T=200)
    whole = jref.scalar_jumps(s['y'], s['var'], *s['args'], 4.0, 8, D=2)
    first = jref.scalar_jumps(s['y'], s['var'], *s['args'], 4.0, 3, D=2)
    cont = jref.scalar_jumps(s['y'], s['var'], *s['args'], 4.0, 6, D=2, w0=first[2])
    for a, b in zip(whole, cont):
        assert np.array_equal(a, b)


# ---- the lane header from plain loops: a stand-alone program -----------------------------------------------------------
def _build_sim(path, extra):
    subprocess.run(['g++', '-std=c++17', *extra, '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'jumps_sim.cpp'), '-o', path], check=True)
    return path


@pytest.fixture(scope='module')
def sims(tmp_path_factory):
    d = tmp_path_factory.mktemp('jumps_sim')
    return dict(dir=d, plain=_build_sim(str(d / 'jumps_sim'), ['-O2']),
                san=_build_sim(str(d / 'jumps_sim_san'),
                               ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


@pytest.mark.parametrize('which', ['plain', 'san'])
def test_simulator_self_check(sims, which):
    """n_iters = 1 gives scales 1, change 0 and the bits of one pass under given ones; a middle pass writes every
    contribution of rows 1 .. T-1; 2 and 8 passes finite and in range; 3 then 6 passes are the bits of 8 - on planes of
    exactly the stated sizes, plain and under AddressSanitizer + UBSan."""
    r = subprocess.run([sims[which]], capture_output=True, text=True)
    assert r.returncode == 0 and 'jumps_sim: ok' in r.stdout, r.stdout + r.stderr


def run_sim(sims, which, pb, B, nu, n_iters, w0=None):
    T, N, D, K = pb['T'], pb['N'], pb['D'], pb['K']
    fin, fout = str(sims['dir'] / 'in.bin'), str(sims['dir'] / 'out.bin')
    par = pb['par']
    with open(fin, 'wb') as f:
        f.write(np.array([T, N, D, B, int(pb['unit']), n_iters, int(w0 is not None)], np.int32).tobytes())
        f.write(np.array([nu], np.float64).tobytes())
        for a in (pb['y'], pb['var']) + (() if w0 is None else (w0,)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        for k in PARAMS:
            f.write(np.ascontiguousarray(par[k], np.float64).tobytes())
    r = subprocess.run([sims[which], fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, np.float32)
    assert out.size == 2 * T * N + T * K + K
    return (out[:T * N].reshape(T, N), out[T * N:2 * T * N].reshape(T, N), out[2 * T * N:2 * T * N + T * K].reshape(T, K),
            out[2 * T * N + T * K:])


@pytest.mark.parametrize('unit', [True, False])
def test_host_simulator_meets_the_float32_bar(sims, unit):
    worst = {}
    cases = [(T, B) for T in (1, 2, 5, 31, 32, 33, 129, 1000) for B in (4, 8, 16, 32)]
    for i, (T, B) in enumerate(cases):
        K, D = 3, 2
        pb = make_session(T, K, D, 0.05, unit, seed=i, centre=50.0)
        pb = jref.add_jumps(pb, jref.random_jumps(T, K, i), seed=i)
        nu = (1.0, 4.0, 30.0)[i % 3]
        args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu)
        for n_iters in (2, 8):
            ref = jref.scalar_jumps(*args, n_iters, D=D)
            r32 = jref.scalar_jumps_f32(*args, n_iters, D=D, unit=unit, B=B)
            got = run_sim(sims, 'san' if i % 8 == 0 else 'plain', pb, B, nu, n_iters)
            bars = jref.bars(r32, ref, pb['y'], D)
            err, et = jref.errors(got, ref, pb['y'], D), jref.errors(r32, ref, pb['y'], D)
            for k in err:
                e = float(np.max(err[k]))
                if e > worst.get(k, (0.0, 0.0))[0]:
                    worst[k] = (e, float(np.max(et[k])))
                assert e <= bars[k], f'{k}: {e:.3g} over the bar {bars[k]:.3g} at T={T} B={B} nu={nu} n_iters={n_iters}'
            u = 1.0 / got[2].astype(np.float64)
            assert np.all(u > 0) and np.all(u <= (nu + D) / nu * (1 + 1e-7))
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
    for name in ('eks_smooth_jumps', 'eks_smooth_jumps_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name) is not None


def test_c_abi_refusals_need_no_device(lib):
    from eks_amd import _lib
    d = lambda K, T, D, O, fl: _lib.EksDims(K, T, D, O, fl)
    DIAG, VSD, UNIT = _lib.FLAG_DIAG_MODEL, _lib.FLAG_VS_DIAG, _lib.FLAG_UNIT_AC
    wsb = lambda dims: lib.eks_smooth_jumps_workspace_bytes(ctypes.byref(dims))
    tvb = lambda dims: lib.eks_smooth_tv_workspace_bytes(ctypes.byref(dims))
    good = d(3, 100, 2, 2, DIAG | UNIT)
    plane = lambda n, e=4: (n * e + 255) // 256 * 256
    assert wsb(good) == tvb(good) + plane(100 * 3) + plane(100 * 6) > 0             # .. the scale and contribution planes
    assert wsb(d(3, 100, 3, 4, 0)) == tvb(d(3, 100, 3, 4, 0)) + plane(100 * 3) + plane(100 * 3, 8) > 0
    assert wsb(d(3, 100, 7, 7, 0)) == 0 and wsb(d(3, 100, 2, 65, 0)) == 0           # D > 6, O > 64: unsupported
    assert wsb(d(0, 100, 2, 2, DIAG)) == 0 and wsb(d(3, 100, 2, 3, DIAG)) == 0
    assert wsb(d(3, 100, 9, 9, DIAG)) == 0 and wsb(d(3, 100, 9, 9, DIAG | VSD)) > 0  # full Vs rows: D <= 8
    one = ctypes.c_void_p(16)                                                        # non-NULL, never dereferenced
    null = ctypes.c_void_p(0)

    def call(dims, null_at=None, nu=4.0, n_iters=8, scales=one, scales_in=0, change=one, ws=one, ws_bytes=1 << 40):
        ptrs = [one] * 8                                                             # y, var, m0 .. s
        out = [one, one]                                                             # ms, Vs
        if null_at is not None:
            if null_at < 8:
                ptrs[null_at] = null
            else:
                out[null_at - 8] = null
        return lib.eks_smooth_jumps(ctypes.byref(dims), *ptrs, nu, n_iters, scales, scales_in, change, *out, ws,
                                    ws_bytes, None)

    assert lib.eks_smooth_jumps(None, *[one] * 8, 4.0, 8, one, 0, one, one, one, one, 1, None) == -1
    for i in range(10):
        assert call(good, null_at=i) == -1, i
    assert call(good, scales=null, scales_in=1) == -1                                # scales_in needs scales
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
    from eks_amd import hip_ops, jumps
    assert eks_amd.smooth_jumps is jumps.smooth_jumps
    assert eks_amd.smooth_singlecam_jumps is jumps.smooth_singlecam_jumps
    assert callable(hip_ops.smooth_jumps)
    K, T, D = 2, 6, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    args = (np.zeros((K, T, D)), np.zeros((K, D)), eye, eye, eye, eye, np.ones((T, K, D)), 1.0)
    for kw in (dict(nu=0.0), dict(nu=-2.0), dict(nu=np.nan), dict(nu=np.inf), dict(n_iters=0), dict(n_iters=2.5),
               dict(tol=0.0), dict(tol=np.nan), dict(tol=1e-3, max_iters=4), dict(tol=1e-3, max_iters=9.5),
               dict(tol=1e-3, n_iters=1)):
        with pytest.raises(ValueError):
            jumps.smooth_jumps(*args, **kw)
    with pytest.raises(ValueError):
        jumps.smooth_jumps(args[0], args[1], eye, eye, eye, eye, np.ones((T + 1, K, D)), 1.0)
    with pytest.raises(NotImplementedError):
        jumps.smooth_jumps(*args, h_fn=lambda x: x)
    from eks_amd.marker_array import MarkerArray
    ma = MarkerArray(np.zeros((2, 1, T, K, 3)), data_fields=['x', 'y', 'likelihood'])
    with pytest.raises(ValueError):
        jumps.smooth_singlecam_jumps(ma, ['a'], 1.0)
    with pytest.raises(ValueError):
        jumps.smooth_singlecam_jumps(ma, ['a', 'b'], 1.0, nu=0.0)
    with pytest.raises(ValueError):
        jumps.smooth_singlecam_jumps(MarkerArray(np.zeros((2, 2, T, K, 3)), data_fields=['x', 'y', 'likelihood']),
                                     ['a', 'b'], 1.0)
