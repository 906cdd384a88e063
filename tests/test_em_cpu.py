"""CPU: the EM entry points without a GPU - the float64 references (tests/em_ref.py) against the joint posterior by
plain linear algebra, their own properties (Fisher's identity, monotone likelihood, the pooled block step), the
float32 lane arithmetic of eks_amd/csrc/eks_em_lane.hpp run from plain loops (tests/host_sim/em_sim.cpp) against the
float64 reference, the C ABI's refusals and the Python argument checks.

Float32 bar (em_ref.bar_excess), the project's rule: per chain, |Sw - reference| / reference <= max(1e-5, 4 x the
float32 NumPy transcription's own worst relative error on the same inputs).  1e-5 is the project's standing bar, the
transcription is what plain sequential float32 reaches without a chunk scan, 4 x covers the scan.  Nothing is compared
with the kernels' own output.

Recorded (float64): the references against the joint posterior at T = 12 agree to 1.4e-14 (scalar) and 1.4e-13
(dense, of the keypoint's largest entry; the increments reference reached 3e-14); Fisher's identity holds to 5.1e-8 of
max(|value|, 1e-3 n) against a central difference with step 1e-4 in log s.  Host simulator over the sweep (sessions
at 400 px): worst relative error of Sw 6.8e-6 where the transcription has 3.6e-6 (s = 1e-4, unit, T = 1000, chunks of
16); the transcription itself stays within 4.0e-6 on the long-session sweep."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402


# ---- the references against the joint posterior ----------------------------------------------------------------------
@pytest.mark.parametrize('a,c,s', [(1.0, 1.0, 1e-2), (0.97, 1.3, 0.5), (-0.8, 0.7, 3.0)])
def test_scalar_reference_against_the_joint_posterior(a, c, s):
    T, N = 12, 3
    rng = np.random.default_rng(3)
    var = rng.uniform(0.5, 4.0, (T, N))
    var[5, 1] = 1e3
    y = rng.normal(size=(T, N))
    m0, S0, q = rng.normal(size=N), rng.uniform(0.5, 5.0, N), rng.uniform(0.5, 2.0, N)
    Sw = em_ref.scalar_em_stats(y, var, m0, S0, a, c, q * s)
    worst = 0.0
    for n in range(N):
        J = em_ref.joint_posterior_stats(y[:, n:n + 1], var[:, n:n + 1], m0[n:n + 1], [[S0[n]]], np.array([[a]]),
                                         np.array([[c]]), np.array([[q[n]]]), s)[0, 0]
        worst = max(worst, abs(Sw[n] / J - 1))
    print(f'scalar reference a={a} c={c} s={s}: Sw against the joint posterior {worst:.3g}')
    assert worst < 1e-11


@pytest.mark.parametrize('D,O,singular_q', [(3, 4, False), (5, 6, False), (3, 4, True), (5, 6, True),
                                           # the pairs the GPU test adds at the accepted width (tests/dense_forms.py)
                                           (1, 64, False), (6, 33, False), (3, 5, False)])
def test_dense_reference_against_the_joint_posterior(D, O, singular_q):
    T, K = 12, 2
    M = dense_case(K, D, O, singular_q, seed=D)
    if singular_q:
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    rng = np.random.default_rng(1)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    var[5, 1, 2] = 1e3
    y = rng.normal(size=(T, K, O))
    par = tuple(M[k] for k in ('m0', 'S0', 'A', 'C', 'Q', 's'))
    Sw = em_ref.dense_em_stats(y, var, *par)
    worst = 0.0
    for k in range(K):
        J = em_ref.joint_posterior_stats(y[:, k], var[:, k], *(p[k] for p in par))
        worst = max(worst, np.abs(Sw[k] - J).max() / np.abs(J).max())
    print(f'dense reference D={D} O={O} singular Q={singular_q}: Sw against the joint posterior {worst:.3g}')
    assert worst < 1e-11


def test_scalar_and_dense_references_agree_on_a_diagonal_model():
    pb = make_session(200, 3, 2, 2.0, False, seed=5, centre=3.0)
    par = pb['par']
    T, K, D = pb['T'], pb['K'], pb['D']
    Sw = em_ref.scalar_em_stats(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    Sd = em_ref.dense_em_stats(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(par[k] for k in
                                                                                      ('m0', 'S0', 'A', 'C', 'Q', 's')))
    assert np.abs(np.diagonal(Sd, axis1=1, axis2=2).ravel() / Sw - 1).max() < 1e-11
    ll_s = em_ref.scalar_loglik(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    ll_d = em_ref.dense_loglik(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(par[k] for k in
                                                                                      ('m0', 'S0', 'A', 'C', 'Q', 's')))
    assert np.abs(ll_s.reshape(K, D).sum(axis=1) / ll_d - 1).max() < 1e-12


# ---- properties of the references --------------------------------------------------------------------------------------
def long_session(a, s_true, seed, T=3000, N=4):
    rng = np.random.default_rng(seed)
    x = np.empty((T, N))
    x[0] = rng.normal(0, 1, N)
    for t in range(1, T):
        x[t] = a * x[t - 1] + rng.normal(0, np.sqrt(s_true), N)
    var = rng.uniform(0.5, 4.0, (T, N))
    var[rng.random((T, N)) < 0.02] = 1e3
    y = x + rng.normal(size=(T, N)) * np.sqrt(np.minimum(var, 50.0))
    return y, var, np.zeros(N), np.full(N, 5.0)


@pytest.mark.parametrize('a', [1.0, 0.98, -0.8])
@pytest.mark.parametrize('s_true', [1e-3, 2.0])
def test_fisher_identity_against_a_central_difference(a, s_true):
    """d loglik / d log s = (Sw / (s q) - n) / 2 with q = 1.  Bar: 1e-6 of max(|value|, 1e-3 n): a central difference
    with step eps = 1e-4 in log s has a truncation error ~ eps^2 / 6 x the third derivative (of order n: 2e-9 n) and a
    rounding error ~ 1e-16 |loglik| / eps ~ 1e-12 n x |loglik| / n; both are far below 1e-9 n = 1e-6 x 1e-3 n."""
    y, var, m0, S0 = long_session(a, s_true, seed=11)
    T, N = y.shape
    n = T - 1
    for s in (s_true, 3 * s_true):
        Sw = em_ref.scalar_em_stats(y, var, m0, S0, a, 1.0, s)
        value = 0.5 * (Sw / s - n)
        eps = 1e-4
        fd = (em_ref.scalar_loglik(y, var, m0, S0, a, 1.0, s * np.exp(eps)) -
              em_ref.scalar_loglik(y, var, m0, S0, a, 1.0, s * np.exp(-eps))) / (2 * eps)
        rel = np.abs(value - fd) / np.maximum(np.abs(value), 1e-3 * n)
        print(f'Fisher a={a} s_true={s_true} s={s}: value {value[0]:.6g}, difference {fd[0]:.6g}, worst relative {rel.max():.3g}')
        assert rel.max() < 1e-6


def test_loglik_never_decreases_over_the_scale_loop():
    for a, s_true in ((1.0, 2.0), (0.98, 1e-3), (-0.8, 2.0)):
        y, var, m0, S0 = long_session(a, s_true, seed=4, T=800)
        T, N = y.shape
        q = np.ones(N)
        fn = em_ref.scalar_trace_fn(y, var, m0, S0, a, 1.0, q, 1)
        hist, _, _ = em_ref.em_scale_loop(fn, T - 1, np.zeros(N), [[k] for k in range(N)], -8, 8, 0.0, 30, 30)
        ll = np.array([em_ref.scalar_loglik(y, var, m0, S0, a, 1.0, np.exp(h)) for h in hist])
        assert hist.shape == (31, N)
        assert (np.diff(ll, axis=0) >= -1e-12 * np.abs(ll[:-1])).all()
        assert (ll[-1] > ll[0]).all()


def test_loglik_never_decreases_over_the_full_q_loop():
    M = dense_case(2, 3, 4, False, seed=6)
    rng = np.random.default_rng(2)
    T = 300
    var = np.exp(rng.normal(0.0, 0.7, (T, 2, 4)))
    y = rng.normal(size=(T, 2, 4)) * 2
    Qs = em_ref.em_full_q_loop(y, var, M['m0'], M['S0'], M['A'], M['C'], M['Q'], 30)
    ll = np.array([em_ref.dense_loglik(y, var, M['m0'], M['S0'], M['A'], M['C'], Q, 1.0) for Q in Qs])
    assert (np.diff(ll, axis=0) >= -1e-12 * np.abs(ll[:-1])).all() and (ll[-1] > ll[0]).all()
    for Q in Qs:
        assert np.array_equal(Q, np.swapaxes(Q, 1, 2)) and np.linalg.eigvalsh(Q).min() > 0


def test_block_step_is_the_pooled_formula():
    y, var, m0, S0 = long_session(0.98, 2.0, seed=9, T=400, N=5)
    T, N = y.shape
    q = np.array([0.5, 1.0, 2.0, 1.5, 0.7])
    fn = em_ref.scalar_trace_fn(y, var, m0, S0, 0.98, 1.0, q, 1)
    blocks = [[0, 3], [1, 2, 4]]
    hist, deltas, st = em_ref.em_scale_loop(fn, T - 1, np.log([0.5, 3.0]), blocks, -8, 8, 0.0, 5, 1)
    s_k = np.empty(N)
    s_k[[0, 3]], s_k[[1, 2, 4]] = 0.5, 3.0
    Sw = em_ref.scalar_em_stats(y, var, m0, S0, 0.98, 1.0, s_k * q)
    for b, mem in enumerate(blocks):
        pooled = (Sw[mem] / q[mem]).sum() / (len(mem) * (T - 1))
        assert abs(np.exp(hist[1, b]) / pooled - 1) < 1e-14
    # and the pooled step raises the block's summed likelihood
    ll0 = em_ref.scalar_loglik(y, var, m0, S0, 0.98, 1.0, s_k * q)
    s1 = np.empty(N)
    s1[[0, 3]], s1[[1, 2, 4]] = np.exp(hist[1])
    ll1 = em_ref.scalar_loglik(y, var, m0, S0, 0.98, 1.0, s1 * q)
    for mem in blocks:
        assert ll1[mem].sum() >= ll0[mem].sum()


def test_scale_loop_stop_rule_and_bounds():
    y, var, m0, S0 = long_session(1.0, 2.0, seed=3, T=300, N=2)
    fn = em_ref.scalar_trace_fn(y, var, m0, S0, 1.0, 1.0, np.ones(2), 1)
    hist, deltas, st = em_ref.em_scale_loop(fn, 299, np.log([1.0, 1.5]), [[0], [1]], -8, 8, 1e-2, 50, 50)
    assert st['done'].all() and (st['iters'] < 50).all()
    for b in range(2):
        assert np.isnan(deltas[st['iters'][b]:, b]).all() and (hist[st['iters'][b]:, b] == hist[-1, b]).all()
    hist, _, _ = em_ref.em_scale_loop(fn, 299, np.array([9.0, -9.0]), [[0], [1]], -1.0, 0.25, 0.0, 3, 3)
    assert ((hist[1:] >= -1.0) & (hist[1:] <= 0.25)).all()


# ---- the lane code in the host simulator -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'em_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libem_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def run_sim(sim, pb, B, gs=0):
    f, d = ctypes.c_float, ctypes.c_double
    par = pb['par']
    Sw = np.full(pb['N'], np.nan)
    rc = sim.sim_em(pb['T'], pb['N'], pb['D'], B, gs, int(pb['unit']), _p(pb['y'], f), _p(pb['var'], f), _p(par['m0'], d),
                    _p(par['S0'], d), _p(par['A'], d), _p(par['C'], d), _p(par['Q'], d), _p(par['s'], d), _p(Sw, d))
    assert rc == 0
    return Sw


def scalar_refs(pb):
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    return em_ref.scalar_em_stats(*args), em_ref.scalar_em_stats_f32(*args, unit=pb['unit'])


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('sval', [1e-4, 2.0, 300.0])
@pytest.mark.parametrize('T', [2, 37, 1000, 3001])
def test_host_sim_against_the_float64_reference_for_every_chunk_length(sim, T, sval, unit):
    pb = make_session(T, 3, 2, sval, unit, seed=T + int(sval * 10))
    r64, r32 = scalar_refs(pb)
    for B, gs in ((4, 0), (8, 3), (16, 0), (32, 0), (32, 1)):
        got = run_sim(sim, pb, B, gs)
        assert np.isfinite(got).all() and (got > 0).all()
        excess, err, trans = em_ref.bar_excess(got, r64, r32)
        print(f'T={T} s={sval} unit={unit} B={B} gs={gs}: Sw {err:.3g} (transcription {trans:.3g})')
        assert excess <= 1.0


def test_host_sim_single_frame_gives_exact_zeros(sim):
    for unit in (True, False):
        pb = make_session(1, 3, 2, 2.0, unit, seed=1)
        for B in (4, 32):
            assert not run_sim(sim, pb, B).any()


def test_the_transcription_itself_on_long_sessions():
    """So that the rule (4 x the transcription) cannot hide a failure: on 3 000 frames x 16 chains, a = 1 and
    a = 0.98, s from 1e-4 to 300, the float32 transcription of Sw stays within 1e-5 of the float64 reference."""
    worst = 0.0
    for sval in (1e-4, 1e-2, 2.0, 300.0):
        for unit in (True, False):
            pb = make_session(3000, 8, 2, sval, unit, seed=17)
            r64, r32 = scalar_refs(pb)
            worst = max(worst, float(np.abs(r32 / r64 - 1).max()))
    print(f'float32 transcription of Sw over the sweep: {worst:.3g}')
    assert worst < 1e-5


def test_rts_step_em_repeats_rts_step_bit_for_bit(sim):
    rng = np.random.default_rng(2)
    out = (ctypes.c_float * 5)()
    for i in range(4000):
        unit = i % 2
        a = 1.0 if unit else float(rng.choice([0.98, 0.5, -0.8, 1.0]))
        Pf, Ps = float(np.exp(rng.normal(0, 3))), float(np.exp(rng.normal(0, 3)))
        qs = float(np.exp(rng.normal(-3, 4)))
        sim.sim_rts_em_steps(unit, ctypes.c_float(a), ctypes.c_double(1 - a), ctypes.c_double(1 - a * a),
                             ctypes.c_float(qs), ctypes.c_float(rng.normal(0, 50)), ctypes.c_float(Ps),
                             ctypes.c_float(rng.normal(0, 50)), ctypes.c_float(Pf), out)
        assert out[0] == out[2] and out[1] == out[3]
        assert out[4] >= 0.0


# ---- C ABI surface and Python argument checks --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_em_entry_points_are_declared_bound_and_exported(lib):
    from eks_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_em_stats', 'eks_em_stats_workspace_bytes', 'eks_em_scale_step', 'eks_em_scale_run'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)


def test_em_refusals_come_before_any_launch(lib):
    from eks_amd import _lib
    fl = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    one = ctypes.c_void_p(8)
    query = lambda d: lib.eks_em_stats_workspace_bytes(ctypes.byref(d))

    def stats(d, ins=None, Sw=one, ws=one, nbytes=1 << 40):
        return lib.eks_em_stats(ctypes.byref(d), *([one] * 8 if ins is None else ins), Sw, ws, nbytes, None)

    def step(d, nb=2, max_iters=5, ptrs=None):
        p = [one] * 7 if ptrs is None else ptrs       # Q, Sw, offsets, members, state, s_keypoint, n_active
        return lib.eks_em_scale_step(ctypes.byref(d), p[0], p[1], nb, p[2], p[3], -8.0, 8.0, 1e-4, max_iters, p[4], p[5],
                                     p[6], None)

    def run(d, nb=2, n_iters=3, ws=one, nbytes=1 << 40, y=one):
        return lib.eks_em_scale_run(ctypes.byref(d), y, *[one] * 6, nb, one, one, -8.0, 8.0, 1e-4, 5, n_iters, one, one,
                                    one, one, ws, nbytes, None)

    d = _lib.EksDims(256, 100000, 2, 2, fl | _lib.FLAG_VS_DIAG)
    need = query(d)
    # the increments planes plus ONE float64 plane of chunk partials: nothing of length T
    inc = lib.eks_smooth_increments_workspace_bytes(ctypes.byref(d))
    assert need == inc + 3125 * 512 * 8
    g = _lib.EksDims(4, 100, 3, 4, _lib.FLAG_Q_PD)
    assert query(g) > 0
    assert stats(d, Sw=None) == -1 and stats(d, ins=[None] + [one] * 7) == -1
    assert stats(d, ws=None, nbytes=0) == -4 and stats(d, nbytes=need - 1) == -4
    assert stats(g, nbytes=query(g) - 1) == -4
    for bad, rc in ((_lib.EksDims(256, 100000, 2, 2, fl), -3),                       # scalar chains without VS_DIAG
                    (_lib.EksDims(4, 100, 7, 7, 0), -3), (_lib.EksDims(4, 100, 3, 65, 0), -3),
                    (_lib.EksDims(0, 10, 2, 2, fl | _lib.FLAG_VS_DIAG), -2),
                    (_lib.EksDims(1 << 23, 2048, 2, 2, fl | _lib.FLAG_VS_DIAG), -2),   # launch indices beyond an int
                    (_lib.EksDims(1 << 22, 8192, 3, 4, 0), -2)):
        assert stats(bad) == rc and query(bad) == 0
        assert step(bad) == rc and run(bad) == rc
    assert query(_lib.EksDims(1 << 23, 2016, 2, 2, fl | _lib.FLAG_VS_DIAG)) > 0
    # the M-step: T < 2, no blocks, general models with diagonals only / without Q_PD
    one_frame = _lib.EksDims(4, 1, 2, 2, fl | _lib.FLAG_VS_DIAG)
    assert query(one_frame) > 0                                                        # eks_em_stats: zeros
    assert step(one_frame) == -2 and run(one_frame) == -2
    assert step(d, nb=0) == -2 and run(d, nb=0) == -2 and run(d, n_iters=-1) == -2
    assert step(d, ptrs=[one, None] + [one] * 5) == -1 and run(d, y=None) == -1
    assert run(d, ws=None, nbytes=0) == -4 and run(d, nbytes=need - 1) == -4
    assert step(_lib.EksDims(4, 100, 3, 4, _lib.FLAG_Q_PD | _lib.FLAG_VS_DIAG)) == -3
    assert run(_lib.EksDims(4, 100, 3, 4, 0)) == -3                                    # Q not asserted positive definite


def test_em_functions_validate_before_any_device_call(lib):
    import eks_amd
    from eks_amd import em
    assert eks_amd.process_noise_statistics is em.process_noise_statistics
    assert eks_amd.refine_smooth_param_em is em.refine_smooth_param_em
    assert eks_amd.fit_process_noise_em is em.fit_process_noise_em
    K, T, D = 3, 20, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    good = dict(ys=np.zeros((K, T, D)), m0s=np.zeros((K, D)), S0s=eye, As=eye, Cs=eye, Qs=eye,
                ensemble_vars=np.ones((T, K, D)))
    fns = ((em.process_noise_statistics, dict(s=np.ones(K))), (em.refine_smooth_param_em, dict(s_init=np.ones(K))),
           (em.fit_process_noise_em, {}))
    for fn, extra in fns:
        def call(**kw):
            args = {**good, **extra, **kw}
            if fn is em.fit_process_noise_em:
                args['Qs_init'] = args.pop('Qs')
            return fn(**args)
        with pytest.raises(ValueError):
            call(ys=np.zeros((K, T)))
        with pytest.raises(ValueError):
            call(ensemble_vars=np.ones((K, T, D)))
        with pytest.raises(ValueError):
            call(Qs=np.tile(np.eye(3), (K, 1, 1)))
        with pytest.raises(NotImplementedError):
            call(h_fn=lambda x: x)
        for name in extra:
            with pytest.raises(ValueError):
                call(**{name: np.ones(K + 1)})
            with pytest.raises(ValueError):
                call(**{name: -np.ones(K)})
    with pytest.raises(ValueError):
        em.refine_smooth_param_em(**good, s_init=1.0, blocks=[[0, 1]])                # does not partition 3 keypoints
    with pytest.raises(ValueError):
        em.refine_smooth_param_em(**good, s_init=1.0, s_bounds_log=(2.0, -2.0))
    with pytest.raises(ValueError):
        em.refine_smooth_param_em(**{**good, 'ys': np.zeros((K, 1, D)), 'ensemble_vars': np.ones((1, K, D))}, s_init=1.0)
    full = np.tile(np.array([[1.0, 0.5], [0.5, 1.0]]), (K, 1, 1))
    sing = np.tile(np.array([[1.0, 1.0], [1.0, 1.0]]), (K, 1, 1))
    with pytest.raises(ValueError):
        em.refine_smooth_param_em(**{**good, 'As': full, 'Qs': sing}, s_init=1.0)     # general model, singular Q
    import torch
    if not torch.cuda.is_available():
        from eks_amd import _lib
        for fn, extra in fns[:2]:
            with pytest.raises(_lib.EksHipError):          # valid arguments reach the device check: no CPU fallback
                fn(**good, **extra)
