"""CPU: eks_innovations without a GPU - the float64 references (tests/innovations_ref.py) against each other, against
em_ref's log-likelihoods and against the Gaussian log-density of the stacked observations by plain linear algebra;
whiteness of the standardised innovations on the reference alone; the float32 lane arithmetic of
eks_amd/csrc/eks_innov_lane.hpp run from plain loops (tests/host_sim/innov_sim.cpp) against the float64 reference;
the C ABI's refusals and the Python argument checks.

Float32 bar (innovations_ref.f32_rule), the project's rule: per chain, error / scale <= max(1e-5, 4 x the float32
NumPy transcription's own worst error / scale on the same inputs), with the scale of innov the chain's max |y|, of
innov_var its own value and of loglik max(|loglik|, T).  The transcription is the yardstick, never the kernels.

Recorded (float64): sequential against joint dense form 6.1e-15 (innov), 2.8e-15 (innov_var), 1.3e-14 (nis), 7.2e-15
(frame_ll), 3.4e-16 (loglik), worst at D = 6, O = 12 with a rank D-1 Q; loglik against the T.O x T.O Gaussian
log-density at T = 12: 1.7e-15.  Whiteness at T = 4 000 x 8 chains, A = C = 1, s = 2: mean z^2 0.999 and |lag-one| <=
0.020 at the true s (bar 0.079); at s / 100 lag-one >= 0.68 and mean z^2 = 6.3.  Host simulator over the sweep, worst
error / scale (transcription's worst on that case): innov 1.2e-6 (6.3e-7), innov_var 2.7e-7 (2.7e-7), loglik 9.9e-6
(9.3e-7) with chunks of 4 at T = 31 and 8.5e-6 (1.4e-6) with the kernels' chunks of 32 at T = 129 - both unit chains
at s = 1e-4 centred at 400 px, where the chunk's entry mean carries the scan's rounding through a whole chunk of
near-zero gains; elsewhere below 4e-6.  The carried belief is filter_loaded's in every lane."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref  # noqa: E402
import innovations_ref as iref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')


def dense_data(T, K, O, seed):
    rng = np.random.default_rng(seed)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    var[T // 2, K - 1, O - 1] = 1e3
    return rng.normal(size=(T, K, O)) * 2, var


def dense_disagreement(a, b, T, O):
    """{name: worst |a - b| / scale}: innov over the keypoint's max |y|-sized scale max |innov|, innov_var over its own
    value, nis and frame_ll over max(|.|, O), loglik over max(|loglik|, T O)."""
    return dict(
        innov=float((np.abs(a['innov'] - b['innov']) / np.abs(a['innov']).max(axis=(0, 2), keepdims=True)).max()),
        innov_var=float((np.abs(a['innov_var'] - b['innov_var']) / a['innov_var']).max()),
        nis=float((np.abs(a['nis'] - b['nis']) / np.maximum(np.abs(a['nis']), O)).max()),
        frame_ll=float((np.abs(a['frame_ll'] - b['frame_ll']) / np.maximum(np.abs(a['frame_ll']), O)).max()),
        loglik=float((np.abs(a['loglik'] - b['loglik']) / np.maximum(np.abs(a['loglik']), T * O)).max()))


# ---- the references against each other ---------------------------------------------------------------------------------
@pytest.mark.parametrize('D,O,singular_q', [(1, 1, False), (2, 3, False), (2, 3, True), (3, 4, False), (3, 4, True),
                                            (6, 12, False), (6, 12, True)])
def test_sequential_and_joint_dense_forms_agree(D, O, singular_q):
    T, K = 60, 3
    M = dense_case(K, D, O, singular_q, seed=D)
    y, var = dense_data(T, K, O, seed=1)
    par = tuple(M[k] for k in PARAMS)
    a, b = iref.dense_innovations_sequential(y, var, *par), iref.dense_innovations_joint(y, var, *par)
    dis = dense_disagreement(a, b, T, O)
    print(f'D={D} O={O} singular Q={singular_q}: sequential against joint ' + ', '.join(f'{k} {v:.3g}' for k, v in dis.items()))
    assert max(dis.values()) < 1e-11
    ll = em_ref.dense_loglik(y, var, *par)
    for r in (a, b):
        assert (np.abs(r['loglik'] - ll) / np.maximum(np.abs(ll), T * O)).max() < 1e-11
        assert np.abs(r['frame_ll'].sum(axis=0) - r['loglik']).max() == 0.0


def test_scalar_and_dense_references_agree_on_a_diagonal_model():
    pb = make_session(200, 3, 2, 2.0, False, seed=5, centre=3.0)
    par = pb['par']
    T, K, D = pb['T'], pb['K'], pb['D']
    v, S, ll = iref.scalar_innovations(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    d = iref.dense_innovations_sequential(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(par[k] for k in PARAMS))
    assert np.abs(d['innov'].reshape(T, -1) - v).max() / np.abs(pb['y']).max() < 1e-11
    assert np.abs(d['innov_var'].reshape(T, -1) / S - 1).max() < 1e-11
    assert np.abs(ll.reshape(K, D).sum(axis=1) / d['loglik'] - 1).max() < 1e-11
    assert np.abs((v * v / S).reshape(T, K, D).sum(axis=2) - d['nis']).max() / np.abs(d['nis']).max() < 1e-11
    ll_em = em_ref.scalar_loglik(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    assert np.abs(ll / ll_em - 1).max() < 1e-11


@pytest.mark.parametrize('singular_q', [False, True])
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3), (3, 4)])
def test_loglik_is_the_gaussian_log_density_of_the_observations(D, O, singular_q):
    T, K = 12, 2
    M = dense_case(K, D, O, singular_q and D > 1, seed=D + 3)
    y, var = dense_data(T, K, O, seed=2)
    par = tuple(M[k] for k in PARAMS)
    worst = 0.0
    for r in (iref.dense_innovations_sequential(y, var, *par), iref.dense_innovations_joint(y, var, *par)):
        for k in range(K):
            J = iref.joint_log_density(y[:, k], var[:, k], *(p[k] for p in par))
            worst = max(worst, abs(r['loglik'][k] - J) / max(abs(J), T * O))
    print(f'D={D} O={O} singular Q={singular_q}: loglik against the joint Gaussian log-density {worst:.3g}')
    assert worst < 1e-11
    if D == 1:
        v, S, ll = iref.scalar_innovations(y[:, :, 0], var[:, :, 0], M['m0'][:, 0], M['S0'][:, 0, 0], M['A'][:, 0, 0],
                                           M['C'][:, 0, 0], M['s'] * M['Q'][:, 0, 0])
        for k in range(K):
            J = iref.joint_log_density(y[:, k], var[:, k], *(p[k] for p in par))
            assert abs(ll[k] - J) / max(abs(J), T) < 1e-11


# ---- whiteness, on the reference alone ---------------------------------------------------------------------------------
def test_standardised_innovations_are_white_at_the_true_scale_only():
    """T = 4 000, 8 chains, A = C = 1, simulated at s = 2 with the model's own time-varying R.  Bars as stated with the
    feature: |lag-one| < 5 / sqrt(T) per chain at the true s (z is then exactly N(0, 1) and white: five standard
    errors); at s / 100 lag-one > 0.5 per chain and mean z^2 > 5 pooled."""
    T, N, s = 4000, 8, 2.0
    rng = np.random.default_rng(0)
    x = np.cumsum(rng.normal(0, np.sqrt(s), (T, N)), axis=0)
    var = rng.uniform(0.5, 4.0, (T, N))
    y = x + rng.normal(size=(T, N)) * np.sqrt(var)
    m0, S0 = np.zeros(N), np.full(N, 10.0)
    v, S, _ = iref.scalar_innovations(y, var, m0, S0, 1.0, 1.0, s)
    z = v / np.sqrt(S)
    r1 = iref.lag1_autocorr(z)
    print(f'true s: mean z^2 {np.mean(z * z):.3f}, |lag-one| <= {np.abs(r1).max():.3f} (bar {5 / np.sqrt(T):.3f}), '
          f'beyond 3 sigma {np.mean(np.abs(z) > 3):.4f}')
    assert (np.abs(r1) < 5 / np.sqrt(T)).all()
    assert abs(np.mean(z * z) - 1) < 0.05
    v, S, _ = iref.scalar_innovations(y, var, m0, S0, 1.0, 1.0, s / 100)
    z = v / np.sqrt(S)
    r1 = iref.lag1_autocorr(z)
    print(f's / 100: mean z^2 {np.mean(z * z):.3f}, lag-one >= {r1.min():.3f}, beyond 3 sigma {np.mean(np.abs(z) > 3):.3f}')
    assert (r1 > 0.5).all()
    assert np.mean(z * z) > 5


# ---- the lane code in the host simulator -------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'innov_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libinnov_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def run_sim(sim, pb, B, gs=0, want=('v', 'S', 'll')):
    f, d = ctypes.c_float, ctypes.c_double
    par = pb['par']
    T, N = pb['T'], pb['N']
    v = np.full((T, N), np.nan, np.float32) if 'v' in want else None
    S = np.full((T, N), np.nan, np.float32) if 'S' in want else None
    ll = np.full(N, np.nan) if 'll' in want else None
    rc = sim.sim_innov(T, N, pb['D'], B, gs, int(pb['unit']), _p(pb['y'], f), _p(pb['var'], f), _p(par['m0'], d),
                       _p(par['S0'], d), _p(par['A'], d), _p(par['C'], d), _p(par['Q'], d), _p(par['s'], d), _p(v, f),
                       _p(S, f), _p(ll, d))
    assert rc == 0, f'{rc} lanes carry a belief that is not filter_loaded\'s'
    return dict(v=v, S=S, ll=ll)


def scalar_refs(pb):
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    v, S, ll = iref.scalar_innovations(*args)
    v32, S32, ll32 = iref.scalar_innovations_f32(*args, unit=pb['unit'])
    return dict(v=v, S=S, ll=ll, y=pb['y'].astype(np.float64)), dict(v=v32, S=S32, ll=ll32)


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('T', [1, 2, 3, 31, 32, 33, 1000, 3001])
def test_host_sim_against_the_float64_reference_for_every_chunk_length(sim, T, unit):
    worst = {}
    for sval in (1e-4, 2.0, 300.0):
        for centre in (0.0, 400.0):
            pb = make_session(T, 3, 2, sval, unit, seed=T + int(sval * 10), centre=centre)
            ref, r32 = scalar_refs(pb)
            for B, gs in ((4, 0), (8, 3), (16, 0), (32, 0), (32, 1)):
                got = run_sim(sim, pb, B, gs)
                assert all(np.isfinite(got[k]).all() for k in got) and (got['S'] > 0).all()
                for name, (excess, err, trans) in iref.f32_rule(got, r32, ref).items():
                    w = worst.setdefault(name, (0.0, 0.0))
                    worst[name] = (max(w[0], err), max(w[1], trans))
                    assert excess <= 1.0, (f'T={T} s={sval} unit={unit} centre={centre} B={B} gs={gs}: {name} is '
                                           f'{excess:.3g} x its bar; {err:.3g} (transcription {trans:.3g})')
    print(f'T={T} unit={unit}: simulator (transcription) ' +
          ', '.join(f'{k} {a:.3g} ({b:.3g})' for k, (a, b) in worst.items()))


def test_host_sim_absent_outputs_change_no_bit(sim):
    pb = make_session(129, 3, 2, 2.0, False, seed=9)
    full = run_sim(sim, pb, 32)
    for want in (('v',), ('S',), ('ll',), ('v', 'll'), ('S', 'll'), ('v', 'S')):
        got = run_sim(sim, pb, 32, want=want)
        for k in ('v', 'S', 'll'):
            assert got[k] is None if k not in want else np.array_equal(got[k], full[k])


def test_the_transcription_itself_on_long_sessions():
    """So that the rule (4 x the transcription) cannot hide a failure: on 3 000 frames x 16 chains, a = 1 and
    a = 0.98, s from 1e-4 to 300, sessions at 0 and at 400 px, the float32 transcription stays within 1e-5 of the
    float64 reference on every output's own scale."""
    worst = dict(v=0.0, S=0.0, ll=0.0)
    for sval in (1e-4, 1e-2, 2.0, 300.0):
        for unit in (True, False):
            for centre in (0.0, 400.0):
                pb = make_session(3000, 8, 2, sval, unit, seed=17, centre=centre)
                ref, r32 = scalar_refs(pb)
                for k, e in iref.f32_errors(r32, ref).items():
                    worst[k] = max(worst[k], float(e.max()))
    print('float32 transcription over the sweep: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) < 1e-5


# ---- C ABI surface and Python argument checks --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_innovations_entry_points_are_declared_bound_and_exported(lib):
    from eks_amd import _build, _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_innovations', 'eks_innovations_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert 'eks_innov.hip' in _build.SOURCES and '-fno-slp-vectorize' in _build.PER_FILE_FLAGS['eks_innov.hip']


def test_innovations_refusals_come_before_any_launch(lib):
    from eks_amd import _lib
    fl = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    one = ctypes.c_void_p(8)
    query = lambda d: lib.eks_innovations_workspace_bytes(ctypes.byref(d))

    def call(d, ins=None, outs=(one, one, None, None, one), ws=one, nbytes=1 << 40):
        return lib.eks_innovations(ctypes.byref(d), *([one] * 8 if ins is None else ins), *outs, ws, nbytes, None)

    d = _lib.EksDims(256, 100000, 2, 2, fl)
    need = query(d)
    # eks_em_stats' planes and its ONE float64 plane of chunk partials: nothing of length T; VS_DIAG is ignored
    assert need == lib.eks_em_stats_workspace_bytes(ctypes.byref(_lib.EksDims(256, 100000, 2, 2, fl | _lib.FLAG_VS_DIAG)))
    assert query(_lib.EksDims(256, 100000, 2, 2, fl | _lib.FLAG_VS_DIAG)) == need
    g = _lib.EksDims(4, 100, 3, 4, 0)
    # general models: no filtered-belief stream, so less than the smoother's generic workspace
    assert 0 < query(g) < lib.eks_smooth_increments_workspace_bytes(ctypes.byref(g))
    assert query(_lib.EksDims(4, 100, 3, 4, _lib.FLAG_VS_DIAG)) == query(g)
    assert call(d, outs=(None,) * 5) == -1 and call(g, outs=(None,) * 5) == -1           # not all outputs may be NULL
    assert call(d, ins=[None] + [one] * 7) == -1 and call(d, ins=[one] * 7 + [None]) == -1
    for outs in ((one, one, one, None, one), (None, None, None, one, None), (one, one, one, one, one)):
        assert call(d, outs=outs) == -3                                                  # nis / frame_ll on scalar chains
    assert call(d, ws=None, nbytes=0) == -4 and call(d, nbytes=need - 1) == -4
    assert call(g, outs=(one,) * 5, nbytes=query(g) - 1) == -4 and call(g, outs=(one,) * 5, ws=None) == -4
    for bad, rc in ((_lib.EksDims(4, 100, 7, 7, 0), -3), (_lib.EksDims(4, 100, 3, 65, 0), -3),
                    (_lib.EksDims(0, 10, 2, 2, fl), -2), (_lib.EksDims(4, 0, 2, 2, fl), -2),
                    (_lib.EksDims(4, 10, 2, 3, fl), -2),
                    (_lib.EksDims(1 << 23, 2048, 2, 2, fl), -2),                         # launch indices beyond an int
                    (_lib.EksDims(1 << 22, 8192, 3, 4, 0), -2)):
        assert call(bad) == rc and query(bad) == 0
    assert query(_lib.EksDims(1 << 23, 2016, 2, 2, fl)) > 0
    assert query(_lib.EksDims(4, 1, 2, 2, fl)) > 0 and query(_lib.EksDims(4, 1, 3, 4, 0)) > 0   # T = 1 is valid


def test_diagnostics_validate_before_any_device_call(lib):
    import eks_amd
    from eks_amd import diagnostics as dg
    for name in ('filter_innovations', 'log_likelihood', 'innovation_summary', 'innovations_singlecam'):
        assert getattr(eks_amd, name) is getattr(dg, name)
    assert dg.FilterInnovations._fields == ('innov', 'innov_var', 'nis', 'frame_loglik', 'loglik')
    K, T, D = 3, 20, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    good = dict(ys=np.zeros((K, T, D)), m0s=np.zeros((K, D)), S0s=eye, As=eye, Cs=eye, Qs=eye,
                ensemble_vars=np.ones((T, K, D)), s_finals=np.ones(K))
    for fn in (dg.filter_innovations, dg.log_likelihood, dg.innovation_summary):
        def call(**kw):
            return fn(**{**good, **kw})
        with pytest.raises(ValueError):
            call(ys=np.zeros((K, T)))
        with pytest.raises(ValueError):
            call(ensemble_vars=np.ones((K, T, D)))
        with pytest.raises(ValueError):
            call(Qs=np.tile(np.eye(3), (K, 1, 1)))
        with pytest.raises(ValueError):
            call(s_finals=np.ones(K + 1))
        with pytest.raises(NotImplementedError):
            call(h_fn=lambda x: x)
    with pytest.raises(ValueError):
        dg.innovations_singlecam(np.zeros((2, 2, 10, 3, 3)), ['a', 'b', 'c'], 1.0)       # two views
    with pytest.raises(ValueError):
        dg.innovations_singlecam(np.zeros((2, 1, 10, 3, 3)), ['a', 'b'], 1.0)            # names do not match
    import torch
    if not torch.cuda.is_available():
        from eks_amd import _lib
        for fn in (dg.filter_innovations, dg.log_likelihood):
            with pytest.raises(_lib.EksHipError):          # valid arguments reach the device check: no CPU fallback
                fn(**good)
