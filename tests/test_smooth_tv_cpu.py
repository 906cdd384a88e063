"""CPU: eks_smooth_tv without a GPU - the float64 references (tests/smooth_tv_ref.py) against the joint Gaussian
posterior by plain linear algebra, against the oracle at w = 1 and against the padded session of the gap identity;
the float32 lane arithmetic of eks_amd/csrc/eks_smooth_tv_lane.hpp run from plain loops
(tests/host_sim/smooth_tv_sim.cpp) bit for bit against the constant-q lane bodies at w = 1 and against the float64
reference at random w; the C ABI's refusals and the Python argument checks.

Float32 bar (smooth_tv_ref.f32_bars), the project's rule: per chain, error / scale <= max(1e-5, 4 x the float32 NumPy
transcription's own worst error / scale on the same inputs), with the scale of ms the chain's max |y| and of Vs its own
value.  The transcription is the yardstick, never the kernels.

Float64 bars, reasoned: (a) 1e-9 of the array's largest entry - the joint posterior solves a T O x T O system whose
condition number reaches 1e5 with variances between the 0.25 and 1e3 used here; (b) 1e-12 as the feature states it;
(c) 1e-10 as the feature states it (padding frames carry a weight of 1e-30, below float64's resolution).

Recorded (float64): both dense forms and the scalar form against the joint posterior <= 1.7e-13, worst at D = 3, O = 4;
w = 1 against the oracle <= 2.5e-14; gap identity 4.6e-16 (scalar), 7.8e-16 and 1.4e-15 (general, A = I).  Host
simulator at w = 1: no lane differs from the constant-q bodies in any bit; at random w, worst error / scale
(transcription's worst on that case): ms 3.4e-7 (2.1e-7), Vs 4.5e-7 (3.4e-7) unit and 3.2e-7 (2.5e-7), 4.9e-7
(4.9e-7) at a = 0.98, c = 1.3."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')


def random_w(rng, shape, zeros=True, big=True):
    """log-uniform in [0.05, 50] with exact zeros and one 1e4 mixed in; entry 0 is NaN (never read)."""
    w = np.exp(rng.uniform(np.log(0.05), np.log(50.0), shape))
    flat = w.reshape(shape[0], -1)
    if zeros and shape[0] > 3:
        flat[rng.random(flat.shape) < 0.05] = 0.0
    if big and shape[0] > 4:
        flat[shape[0] // 2, 0] = 1e4
    flat[0] = np.nan
    return w.astype(np.float32)


def dense_data(T, K, O, seed):
    rng = np.random.default_rng(seed)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    var[T // 2, K - 1, O - 1] = 1e3
    return rng.normal(size=(T, K, O)) * 2, var


# ---- (a) the references against the joint Gaussian posterior ----------------------------------------------------------
@pytest.mark.parametrize('singular_q', [False, True])
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3), (3, 4)])
def test_references_are_the_joint_gaussian_posterior(D, O, singular_q):
    T, K = 12, 2
    M = dense_case(K, D, O, singular_q and D > 1, seed=D + 10)
    y, var = dense_data(T, K, O, seed=3)
    rng = np.random.default_rng(D)
    w = rng.uniform(0.0, 20.0, (T, K))
    w[[3, 7], 0] = 0.0
    w[5, 1] = 0.0
    w[0] = np.nan
    par = tuple(M[k] for k in PARAMS)
    worst = 0.0
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        ms, Vs = form(y, var, *par, w)
        for k in range(K):
            jm, jV = tref.joint_posterior(y[:, k], var[:, k], *(p[k] for p in par), w[:, k])
            worst = max(worst, np.abs(ms[:, k] - jm).max() / np.abs(jm).max(), np.abs(Vs[:, k] - jV).max() / np.abs(jV).max())
    if D == 1:
        ms, Vs = tref.scalar_smooth_tv(y[:, :, 0], var[:, :, 0], M['m0'][:, 0], M['S0'][:, 0, 0], M['A'][:, 0, 0],
                                       M['C'][:, 0, 0], M['s'] * M['Q'][:, 0, 0], w)
        for k in range(K):
            jm, jV = tref.joint_posterior(y[:, k], var[:, k], *(p[k] for p in par), w[:, k])
            worst = max(worst, np.abs(ms[:, k] - jm[:, 0]).max() / np.abs(jm).max(),
                        np.abs(Vs[:, k] - jV[:, 0, 0]).max() / np.abs(jV).max())
    print(f'D={D} O={O} singular Q={singular_q}: references against the joint posterior {worst:.3g}')
    assert worst < 1e-9


def test_a_shifted_index_is_visible_in_the_joint_posterior():
    """The check above can tell w[t] from w[t + 1]: the reference run on w shifted by one frame misses the joint
    posterior of the unshifted w by far more than the bar."""
    T, K, D, O = 12, 1, 2, 3
    M = dense_case(K, D, O, False, seed=1)
    y, var = dense_data(T, K, O, seed=3)
    w = np.ones(T)
    w[6] = 20.0
    par = tuple(M[k] for k in PARAMS)
    jm, jV = tref.joint_posterior(y[:, 0], var[:, 0], *(p[0] for p in par), w)
    for shift in (-1, 1):
        _, Vs = tref.dense_smooth_tv(y, var, *par, np.roll(w, shift))
        assert np.abs(Vs[:, 0] - jV).max() / np.abs(jV).max() > 1e-3


# ---- (b) w = 1 against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3), (3, 4)])
def test_unit_scale_is_the_oracle_smoother(D, O):
    from oracle import eks_oracle as orc
    T, K = 60, 3
    M = dense_case(K, D, O, False, seed=D)
    y, var = dense_data(T, K, O, seed=1)
    par = tuple(M[k] for k in PARAMS)
    oms, oVs, _ = orc.kalman_smoother(np.swapaxes(y, 0, 1), *par, np.swapaxes(var, 0, 1))
    oms, oVs = np.swapaxes(oms, 0, 1), np.swapaxes(oVs, 0, 1)
    worst = 0.0
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        ms, Vs = form(y, var, *par, np.ones(T))
        worst = max(worst, np.abs(ms - oms).max() / np.abs(oms).max(), np.abs(Vs - oVs).max() / np.abs(oVs).max())
    print(f'D={D} O={O}: w = 1 against oracle.eks_oracle.kalman_smoother {worst:.3g}')
    assert worst < 1e-12


# ---- (c) the gap identity ------------------------------------------------------------------------------------------------
def gap_scale(rng, T):
    w = np.ones(T)
    w[rng.choice(np.arange(1, T), size=max(1, T // 8), replace=False)] = rng.integers(2, 6, size=max(1, T // 8))
    return w


def test_gap_identity_scalar_chains():
    rng = np.random.default_rng(4)
    T, N = 80, 5
    y = np.cumsum(rng.normal(size=(T, N)), axis=0)
    var = rng.uniform(0.5, 4.0, (T, N))
    w = gap_scale(rng, T)
    args = (np.zeros(N), np.full(N, 10.0), 1.0, 1.0, np.full(N, 0.7))
    ms, Vs = tref.scalar_smooth_tv(y, var, *args, w)
    yp, vp, idx = tref.pad_gaps(y, var, w)
    assert yp.shape[0] == int(w[1:].sum()) + 1 > T
    pm, pV = tref.scalar_smooth_tv(yp, vp, *args, np.ones(yp.shape[0]))
    worst = max(np.abs(ms - pm[idx]).max() / np.abs(y).max(), (np.abs(Vs - pV[idx]) / Vs).max())
    print(f'gap identity, scalar chains: {worst:.3g}')
    assert worst < 1e-10


@pytest.mark.parametrize('D,O', [(2, 3), (3, 4)])
def test_gap_identity_general_models_with_identity_dynamics(D, O):
    rng = np.random.default_rng(D)
    T, K = 50, 2
    M = dense_case(K, D, O, False, seed=D + 20)
    M['A'] = np.tile(np.eye(D), (K, 1, 1))
    y, var = dense_data(T, K, O, seed=6)
    w = gap_scale(rng, T)
    par = tuple(M[k] for k in PARAMS)
    ms, Vs = tref.dense_smooth_tv(y, var, *par, w)
    yp, vp, idx = tref.pad_gaps(y, var, w)
    pm, pV = tref.dense_smooth_tv(yp, vp, *par, np.ones(yp.shape[0]))
    worst = max(np.abs(ms - pm[idx]).max() / np.abs(ms).max(), np.abs(Vs - pV[idx]).max() / np.abs(Vs).max())
    print(f'gap identity, D={D} O={O}, A = I: {worst:.3g}')
    assert worst < 1e-10


def test_scalar_and_dense_references_agree_on_a_diagonal_model_with_per_keypoint_scale():
    pb = make_session(150, 3, 2, 2.0, False, seed=5, centre=3.0)
    T, K, D = pb['T'], pb['K'], pb['D']
    w = random_w(np.random.default_rng(0), (T, K))
    ms, Vs = tref.scalar_smooth_tv(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], w, D=D)
    dm, dV = tref.dense_smooth_tv(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS), w)
    assert np.abs(dm.reshape(T, -1) - ms).max() / np.abs(pb['y']).max() < 1e-11
    assert np.abs(np.diagonal(dV, axis1=2, axis2=3).reshape(T, -1) / Vs - 1).max() < 1e-10


# ---- the lane header from plain loops ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('smooth_tv_sim') / 'libsmooth_tv_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'smooth_tv_sim.cpp'), '-o', so], check=True)
    return ctypes.CDLL(so)


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def run_sim(sim, pb, w, B, gs=0, compare=0):
    T, N, D = pb['T'], pb['N'], pb['D']
    ms, Vs = np.full((T, N), np.nan, np.float32), np.full((T, N), np.nan, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    f, d = ctypes.c_float, ctypes.c_double
    par = pb['par']
    rc = sim.sim_smooth_tv(T, N, D, B, gs, int(pb['unit']), _p(pb['y'], f), _p(pb['var'], f), _p(w, f), int(w.ndim == 2),
                           *(_p(par[k], d) for k in PARAMS), compare, _p(ms, f), _p(Vs, f))
    return rc, ms, Vs


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('B', [4, 8, 16, 32])
def test_unit_scale_gives_the_constant_q_lane_bodies_bits(sim, B, unit):
    """With w = 1 every lane's element, carried belief, filtered pairs and outputs are bit for bit those of
    summarize_loaded / filter_loaded / smooth_rows - shared and per-keypoint w alike."""
    for T in (1, 2, 3, B - 1, B, B + 1, 5 * B + 3, 1000):
        for sval in (1e-2, 2.0, 300.0):
            pb = make_session(T, 3, 2, sval, unit, seed=T)
            for w in (np.ones(T, np.float32), np.ones((T, 3), np.float32)):
                w[0] = np.nan                                            # never read
                rc, ms, Vs = run_sim(sim, pb, w, B, compare=1)
                assert rc == 0, f'{rc} lanes differ at T={T} B={B} s={sval}'
                assert np.isfinite(ms).all() and np.isfinite(Vs).all()


@pytest.mark.parametrize('unit', [True, False])
def test_host_simulator_meets_the_float32_bar_at_random_scales(sim, unit):
    worst = dict(ms=(0.0, 0.0), Vs=(0.0, 0.0))
    cases = [(T, B) for T in (1, 2, 3, 5, 31, 32, 33, 129, 1000, 3001) for B in (4, 8, 16, 32)]
    for i, (T, B) in enumerate(cases):
        sval = (1e-2, 2.0, 300.0)[i % 3]
        K, D = 3, 2
        pb = make_session(T, K, D, sval, unit, seed=i)
        rng = np.random.default_rng(i)
        w = random_w(rng, (T, K) if i % 2 else (T,))
        args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], w)
        rms, rVs = tref.scalar_smooth_tv(*args, D=D)
        tms, tVs = tref.scalar_smooth_tv_f32(*args, D=D, unit=unit)
        bars = tref.f32_bars(tms, tVs, rms, rVs, pb['y'])
        rc, ms, Vs = run_sim(sim, pb, w, B)
        assert rc == 0
        err = tref.f32_errors(ms, Vs, rms, rVs, pb['y'])
        et = tref.f32_errors(tms, tVs, rms, rVs, pb['y'])
        for k in err:
            e = float(err[k].max())
            if e > worst[k][0]:
                worst[k] = (e, float(et[k].max()))
            assert e <= bars[k], f'{k}: {e:.3g} over the bar {bars[k]:.3g} at T={T} B={B} s={sval} unit={unit}'
    print(f'unit={unit}: host simulator worst error / scale (transcription on that case): '
          + ', '.join(f'{k} {v[0]:.2g} ({v[1]:.2g})' for k, v in worst.items()))


def test_a_spike_shifted_by_one_frame_is_far_outside_the_bar(sim):
    """The simulator at a spike w[p] = 400 matches the reference at p and misses the references at p - 1 and p + 1 by
    more than ten bars, for p on both sides of a chunk edge."""
    B, T = 8, 40
    pb = make_session(T, 2, 1, 2.0, True, seed=9, centre=3.0)
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    for p in (1, B - 1, B, B + 1, 2 * B, T - 1):
        w = np.ones(T, np.float32)
        w[p] = 400.0
        rc, ms, Vs = run_sim(sim, pb, w, B)
        rms, rVs = tref.scalar_smooth_tv(*args, w)
        bars = tref.f32_bars(*tref.scalar_smooth_tv_f32(*args, w, unit=True), rms, rVs, pb['y'])
        assert float(tref.f32_errors(ms, Vs, rms, rVs, pb['y'])['Vs'].max()) <= bars['Vs']
        for q in (p - 1, p + 1):
            if 1 <= q < T:
                w2 = np.ones(T, np.float32)
                w2[q] = 400.0
                oms, oVs = tref.scalar_smooth_tv(*args, w2)
                assert float(tref.f32_errors(ms, Vs, oms, oVs, pb['y'])['Vs'].max()) > 10 * bars['Vs']


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
    wsb = lambda dims: lib.eks_smooth_tv_workspace_bytes(ctypes.byref(dims))
    good = d(3, 100, 2, 2, DIAG | UNIT)
    assert wsb(good) == lib.eks_em_stats_workspace_bytes(ctypes.byref(d(3, 100, 2, 2, DIAG | UNIT | VSD))) > 0
    assert wsb(d(3, 100, 3, 4, 0)) > 0
    assert wsb(d(3, 100, 7, 7, 0)) == 0 and wsb(d(3, 100, 2, 65, 0)) == 0          # D > 6, O > 64: unsupported
    assert wsb(d(0, 100, 2, 2, DIAG)) == 0 and wsb(d(3, 100, 2, 3, DIAG)) == 0
    assert wsb(d(3, 100, 9, 9, DIAG)) == 0 and wsb(d(3, 100, 9, 9, DIAG | VSD)) > 0  # full Vs rows: D <= 8
    one = ctypes.c_void_p(16)                                                        # non-NULL, never dereferenced

    def call(dims, null_at=None, ws=one, ws_bytes=1 << 40):
        ptrs = [one] * 11
        if null_at is not None:
            ptrs[null_at] = ctypes.c_void_p(0)
        return lib.eks_smooth_tv(ctypes.byref(dims), ptrs[0], ptrs[1], ptrs[2], 0, *ptrs[3:], ws, ws_bytes, None)

    assert lib.eks_smooth_tv(None, *[one] * 3, 0, *[one] * 8, one, 1, None) == -1
    for i in range(11):                                                              # y, var, qscale, m0 .. s, ms, Vs
        assert call(good, null_at=i) == -1, i
    assert call(d(3, 0, 2, 2, DIAG)) == -2 and call(d(3, 100, 2, 3, DIAG)) == -2
    assert call(d(3, 100, 2, 2, UNIT)) == -3                                         # UNIT_AC without DIAG_MODEL
    assert call(d(3, 100, 7, 7, 0)) == -3 and call(d(3, 100, 2, 65, 0)) == -3 and call(d(3, 100, 9, 9, DIAG)) == -3
    assert call(good, ws=ctypes.c_void_p(0)) == -4 and call(good, ws_bytes=wsb(good) - 1) == -4
    assert call(d(3, 100, 3, 4, 0), ws_bytes=wsb(d(3, 100, 3, 4, 0)) - 1) == -4


# ---- the Python surface's argument checks (raised before a device is asked for) --------------------------------------
def test_process_noise_scale_from_times():
    import eks_amd
    f = eks_amd.process_noise_scale_from_times
    t = np.arange(100) / 60.0
    keep = np.ones(100, bool)
    keep[[10, 40, 41, 42, 43, 70]] = False                       # two single drops and one 4-frame hole
    w = f(t[keep])
    assert w.dtype == np.float32 and w.shape == (94,) and w[0] == 1.0
    assert np.allclose(w[np.flatnonzero(w > 1.5)], [2, 5, 2]) and np.allclose(np.delete(w, np.flatnonzero(w > 1.5)), 1)
    half = f(t[keep], nominal_dt=1 / 30.0)
    assert half[0] == 1.0 and np.allclose(half[1:], w[1:] / 2)
    assert f([3.0]).tolist() == [1.0]
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 2.0], [0.0, np.inf], [[0.0, 1.0]], []):
        with pytest.raises(ValueError):
            f(bad)
    with pytest.raises(ValueError):
        f([0.0, 1.0], nominal_dt=0.0)


def test_python_argument_checks():
    import eks_amd
    from eks_amd import irregular
    assert eks_amd.smooth_time_varying is irregular.smooth_time_varying
    assert eks_amd.smooth_singlecam_irregular is irregular.smooth_singlecam_irregular
    K, T, D = 2, 6, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    args = (np.zeros((K, T, D)), np.zeros((K, D)), eye, eye, eye, eye, np.ones((T, K, D)), 1.0)
    for bad in (np.ones(T + 1), np.ones((T, K)), np.full(T, -1.0), np.full(T, 2e6), np.full(T, np.nan),
                np.full(T, np.inf)):
        with pytest.raises(ValueError):
            irregular.smooth_time_varying(*args, bad)
    with pytest.raises(NotImplementedError):
        irregular.smooth_time_varying(*args, np.ones(T), h_fn=lambda x: x)
    w0 = np.ones(T)
    w0[0] = np.nan                                                # entry 0 is never read: no complaint about it
    assert irregular._check_scale(w0, K, T).tolist() == [1.0] * T
    assert irregular._check_scale(np.arange(K * T, dtype=float).reshape(K, T), K, T).shape == (T, K)
    from eks_amd.marker_array import MarkerArray
    ma = MarkerArray(np.zeros((2, 1, T, K, 3)), data_fields=['x', 'y', 'likelihood'])
    for kw in (dict(), dict(frame_times=np.arange(T), process_noise_scale=np.ones(T))):
        with pytest.raises(ValueError):
            irregular.smooth_singlecam_irregular(ma, ['a', 'b'], 1.0, **kw)
    for doc in (irregular.smooth_time_varying.__doc__, irregular.__doc__):
        doc = ' '.join(doc.lower().split())
        assert 'brownian motion' in doc and 'uniform model' in doc and 'once per frame' in doc
