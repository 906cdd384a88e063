"""CPU: eks_smooth_increments without a GPU - the float64 references (tests/increments_ref.py) against the joint
posterior covariance by plain linear algebra and against the oracle's smoother, the float32 lane arithmetic of
eks_amd/csrc/eks_increments_lane.hpp run from plain loops (tests/host_sim/increments_sim.cpp) against the float64
reference, the moments of backward-sampled trajectories, the C ABI surface and the Python argument checks.

Float32 bars (rule_excess).  Per chain, |error| <= max(1e-5 x the chain's scale, 4 x the float32 NumPy
transcription's own error on the same inputs): the scale is the chain's largest |reference| of that output over the
session (of Vs for lag1: a covariance is measured against the variances it ties together), the transcription's error
its worst |error| over the chains of the case, in the output's own units.  1e-5 is the project's bar for ms / Vs, the
transcription is what plain sequential float32 reaches without a chunk scan, 4 x covers the scan.  dV is additionally
held per entry, relative to the reference entry, under max(1e-5, 4 x the transcription's worst such figure).  The
printed figures are errors as fractions of the chain's scale.  Nothing is compared with the kernels' own output.

Worst figures of the host-simulator sweep below (T = 2 .. 3001, s = 1e-4 .. 300, unit and a = 0.98 / c = 1.3, chunk
lengths 4 .. 32) are printed by the test; DESIGN.md 9d quotes them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import increments_ref as iref  # noqa: E402
import sampling_ref as sref  # noqa: E402

NAMES = ('ms', 'Vs', 'lag1', 'dmean', 'dV')


# ---- the references against the joint posterior and the oracle ---------------------------------------------------
def joint_blocks(S, T, D):
    """lag1[t] = block (t, t+1), dV[t] = J_tt + J_t+1,t+1 - J_t,t+1 - J_t+1,t of the joint covariance, t < T-1."""
    blk = lambda i, j: S[i * D:(i + 1) * D, j * D:(j + 1) * D]
    lag = np.stack([blk(t, t + 1) for t in range(T - 1)])
    dV = np.stack([blk(t, t) + blk(t + 1, t + 1) - blk(t, t + 1) - blk(t + 1, t) for t in range(T - 1)])
    Vs = np.stack([blk(t, t) for t in range(T)])
    return Vs, lag, dV


@pytest.mark.parametrize('a,c,s', [(1.0, 1.0, 1e-4), (0.97, 1.3, 0.5), (-0.8, 0.7, 3.0)])
def test_scalar_reference_against_the_joint_posterior_and_the_oracle(a, c, s):
    from oracle import eks_oracle as orc
    T, N = 12, 3
    rng = np.random.default_rng(3)
    var = rng.uniform(0.5, 4.0, (T, N))
    var[5, 1] = 1e3
    y = rng.normal(size=(T, N))
    m0, S0, q = rng.normal(size=N), rng.uniform(0.5, 5.0, N), rng.uniform(0.5, 2.0, N)
    ms, Vs, lag1, dmean, dV = iref.scalar_increments(y, var, m0, S0, a, c, q * s)
    assert np.all(lag1[-1] == 0) and np.all(dmean[-1] == 0) and np.all(dV[-1] == 0)
    worst = dict(lag1=0.0, dV=0.0, Vs=0.0)
    for n in range(N):
        S = sref.dense_joint_posterior(var[:, n:n + 1], [[S0[n]]], np.array([[a]]), np.array([[c]]), np.array([[q[n]]]), s)
        Vj, lj, dj = (x[:, 0, 0] for x in joint_blocks(S, T, 1))
        worst['Vs'] = max(worst['Vs'], np.abs(Vs[:, n] / Vj - 1).max())
        worst['lag1'] = max(worst['lag1'], (np.abs(lag1[:-1, n] - lj) / np.abs(Vj).max()).max())
        worst['dV'] = max(worst['dV'], np.abs(dV[:-1, n] / dj - 1).max())      # per entry: J's own sum cancels at small s
    assert np.abs(dmean[:-1] - np.diff(ms, axis=0)).max() < 1e-13
    eye = np.ones((N, 1, 1))
    mo, Vo = orc.kalman_smoother(y.T[:, :, None], m0[:, None], S0[:, None, None], a * eye, c * eye, q[:, None, None],
                                 np.full(N, s), var.T[:, :, None])[:2]
    worst['ms_oracle'] = (np.abs(ms - mo[:, :, 0].T) / np.abs(ms).max(axis=0)).max()
    worst['Vs_oracle'] = np.abs(Vs / Vo[:, :, 0, 0].T - 1).max()
    print(f'scalar reference a={a} c={c} s={s}: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) < 1e-10


def dense_case(K, D, O, singular_q, seed):
    rng = np.random.default_rng(seed)
    A = np.eye(D) * 0.9 + 0.1 * rng.normal(size=(K, D, D)) / np.sqrt(D)
    C = rng.normal(size=(K, O, D))
    Lq = rng.normal(size=(K, D, D)) * 0.4 + np.eye(D)
    Q = Lq @ np.swapaxes(Lq, 1, 2)
    if singular_q:                                         # one eigen-direction projected out: rank D - 1
        u = rng.normal(size=(K, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        Pj = np.eye(D) - u[:, :, None] * u[:, None, :]
        Q = Pj @ Q @ Pj
        Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
    L0 = rng.normal(size=(K, D, D)) * 0.3 + 1.5 * np.eye(D)
    S0 = L0 @ np.swapaxes(L0, 1, 2)
    return dict(m0=rng.normal(size=(K, D)), S0=S0, A=A, C=C, Q=Q, s=rng.uniform(0.5, 2.0, K))


@pytest.mark.parametrize('D,O,singular_q', [(3, 4, False), (5, 6, False), (3, 4, True), (5, 6, True),
                                           # the pairs the GPU test adds at the accepted width (tests/dense_forms.py)
                                           # ((1, 64) is left to tests/test_em_cpu.py: with D = 1 the lag-one convention
                                           #  asserted below cannot be observed)
                                           (6, 33, False), (3, 5, False)])
def test_dense_reference_against_the_joint_posterior_and_the_oracle(D, O, singular_q):
    from oracle import eks_oracle as orc
    T, K = 12, 2
    M = dense_case(K, D, O, singular_q, seed=D)
    if singular_q:
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    rng = np.random.default_rng(1)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    var[5, 1, 2] = 1e3
    y = rng.normal(size=(T, K, O))
    par = tuple(M[k] for k in ('m0', 'S0', 'A', 'C', 'Q', 's'))
    ms, Vs, lag1, dmean, dV = iref.dense_increments(y, var, *par)
    assert not lag1[-1].any() and not dmean[-1].any() and not dV[-1].any()
    worst = dict(Vs=0.0, lag1=0.0, dV=0.0)
    for k in range(K):
        S = sref.dense_joint_posterior(var[:, k], M['S0'][k], M['A'][k], M['C'][k], M['Q'][k], M['s'][k])
        Vj, lj, dj = joint_blocks(S, T, D)
        scale = np.abs(Vj).max()
        worst['Vs'] = max(worst['Vs'], np.abs(Vs[:, k] - Vj).max() / scale)
        worst['lag1'] = max(worst['lag1'], np.abs(lag1[:-1, k] - lj).max() / scale)   # NOT its transpose: row = x_t
        worst['dV'] = max(worst['dV'], np.abs(dV[:-1, k] - dj).max() / np.abs(dj).max())
        assert np.abs(lag1[:-1, k] - np.swapaxes(lj, 1, 2)).max() / scale > 1e-3      # the convention is observable
    assert np.abs(dmean[:-1] - np.diff(ms, axis=0)).max() == 0.0
    mo, Vo = orc.kalman_smoother(y.transpose(1, 0, 2), *par, var.transpose(1, 0, 2))[:2]
    worst['ms_oracle'] = np.abs(ms - mo.transpose(1, 0, 2)).max() / np.abs(ms).max()
    worst['Vs_oracle'] = np.abs(Vs - Vo.transpose(1, 0, 2, 3)).max() / np.abs(Vs).max()
    print(f'dense reference D={D} O={O} singular Q={singular_q}: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) < 1e-10
    r32 = iref.dense_increments_f32out(y, var, *par)
    assert all(o.dtype == np.float32 for o in r32)
    assert 0 < np.abs(r32[4] - dV).max() <= 2.0 ** -24 * np.abs(dV).max()


# ---- the lane code in the host simulator ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'increments_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libincrements_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def make_session(T, K, D, sval, unit, seed, a=0.98, c=1.3, centre=400.0):
    """Positions near `centre` px, variances in [0.5, 4] with 2 % of the frames at 1e3, q = 1."""
    rng = np.random.default_rng(seed)
    N = K * D
    av, cv = (np.ones(N), np.ones(N)) if unit else (np.full(N, a), np.full(N, c))
    x = centre + np.cumsum(rng.normal(0, np.sqrt(min(sval, 4.0)), (T, N)), axis=0)
    var = rng.uniform(0.5, 4.0, (T, N))
    var[rng.random((T, N)) < 0.02] = 1e3
    y = cv * x + rng.normal(0, 1, (T, N)) * np.sqrt(np.minimum(var, 50.0))
    m0 = np.full(N, centre)
    S0d = np.full(N, 10.0)

    def diag(v):
        out = np.zeros((K, D, D))
        out[:, np.arange(D), np.arange(D)] = np.reshape(v, (K, D))
        return out
    par = dict(m0=m0.reshape(K, D).copy(), S0=diag(S0d), A=diag(av), C=diag(cv), Q=diag(np.ones(N)),
               s=np.full(K, float(sval)))
    return dict(T=T, K=K, D=D, N=N, a=av, c=cv, qs=np.full(N, float(sval)), S0d=S0d, m0f=m0, par=par, unit=unit,
                y=np.ascontiguousarray(y, np.float32), var=np.ascontiguousarray(var, np.float32))


def run_sim(sim, pb, B, gs=0, plain=False, want=NAMES):
    T, N, D = pb['T'], pb['N'], pb['D']
    out = {n: (np.full((T, N), np.nan, np.float32) if n in want else None) for n in NAMES}
    f, d = ctypes.c_float, ctypes.c_double
    par = pb['par']
    rc = sim.sim_increments(T, N, D, B, gs, int(pb['unit']), int(plain), _p(pb['y'], f), _p(pb['var'], f),
                            _p(par['m0'], d), _p(par['S0'], d), _p(par['A'], d), _p(par['C'], d), _p(par['Q'], d),
                            _p(par['s'], d), *(_p(out[n], f) for n in NAMES))
    assert rc == 0
    return out


def references(pb):
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    r64 = dict(zip(NAMES, iref.scalar_increments(*args)))
    r32 = dict(zip(NAMES, iref.scalar_increments_f32(*args, unit=pb['unit'])))
    return r64, r32


def scaled_error(x, r64, name):
    """worst |x - reference| per chain as a fraction of the chain's scale (of Vs for lag1)."""
    scale = np.abs(r64['Vs' if name == 'lag1' else name]).max(axis=0)
    return float((np.abs(x.astype(np.float64) - r64[name]).max(axis=0) / scale).max())


def rule_excess(x, r32, r64, name):
    """The bar rule as a ratio (<= 1 passes): per chain, |x - reference| over
    max(1e-5 x the chain's scale, 4 x the transcription's own error), the latter in the output's own units: the
    transcription's worst |error| over the case, whose chains share their model kind, s and data.  An absolute
    figure, because float32's error on these outputs is set by the size of the positions and variances, not by how
    large a chain's own largest increment happens to be: on a session of a few frames one chain in a hundred has
    increments (or, at one frame, a mean) a hundred times below its neighbours', and the ratio of two roundings on
    that chain bounds nothing."""
    scale = np.abs(r64['Vs' if name == 'lag1' else name]).max(axis=0)
    err = np.abs(x.astype(np.float64) - r64[name]).max(axis=0)
    trans = np.abs(r32[name].astype(np.float64) - r64[name]).max()
    return float((err / np.maximum(1e-5 * scale, 4.0 * trans)).max())


def entry_error(x, r64):
    """worst |dV - reference| / reference over the entries t < T-1 (the reference's dV is positive there)."""
    return float(np.abs(x[:-1].astype(np.float64) / r64['dV'][:-1] - 1).max())


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('sval', [1e-4, 2.0, 300.0])
@pytest.mark.parametrize('T', [2, 37, 1000, 3001])
def test_host_sim_against_the_float64_reference_for_every_chunk_length(sim, T, sval, unit):
    pb = make_session(T, 3, 2, sval, unit, seed=T + int(sval * 10))
    r64, r32 = references(pb)
    trans = {n: scaled_error(r32[n], r64, n) for n in ('lag1', 'dmean', 'dV')}
    trans_entry = entry_error(r32['dV'], r64)
    for B, gs in ((4, 0), (8, 3), (16, 0), (32, 0), (32, 1)):
        got = run_sim(sim, pb, B, gs)
        plain = run_sim(sim, pb, B, gs, plain=True, want=('ms', 'Vs'))
        assert np.array_equal(got['ms'], plain['ms']) and np.array_equal(got['Vs'], plain['Vs'])   # bit for bit
        for n in ('lag1', 'dmean', 'dV'):
            assert not got[n][-1].any()                                                           # row T-1: zeros
        err = {n: scaled_error(got[n], r64, n) for n in ('lag1', 'dmean', 'dV')}
        ent = entry_error(got['dV'], r64)
        print(f'T={T} s={sval} unit={unit} B={B} gs={gs}: ' +
              ', '.join(f'{n} {err[n]:.3g} (transcription {trans[n]:.3g})' for n in err) +
              f', dV per entry {ent:.3g} (transcription {trans_entry:.3g})')
        for n in err:
            assert rule_excess(got[n], r32, r64, n) <= 1.0
        assert ent <= max(1e-5, 4 * trans_entry)
        assert scaled_error(got['ms'], r64, 'ms') < 1e-5 and scaled_error(got['Vs'], r64, 'Vs') < 1e-5


def test_the_transcription_itself_on_the_long_session_sweep():
    """Two assertions about the float32 transcription, so that the bar rule (4 x the transcription) cannot hide a
    failure.  Inputs: the sessions the bounds were stated for - 3 000 frames x 16 chains, positions near 400 px,
    variances in [0.5, 4] with 2 % of the frames at 1e3, a = 1 and a = 0.98, s from 1e-4 to 300.  (A session of a
    few frames has no such bound on dmean: its scale is one or two increments of ~1e-3 px against a float32 spacing
    of 3e-5 px at 400 px.)
    1. The transcription stays within 1e-5 for lag1 (of the chain's largest variance) and dV (per entry) and within
       5e-3 of the chain's largest increment for dmean.
    2. Why the kernel emits dV: at s = 1e-4, Vs[t] + Vs[t+1] - 2 lag1[t] formed (in float64) from the CORRECTLY
       ROUNDED float32 reference outputs is at least 10 x worse per entry than the transcription of g^2 Ps + Pf h,
       which never leaves float32."""
    worst = dict(lag1=0.0, dmean=0.0, dV=0.0)
    naive_worst = trans_small_s = 0.0
    for sval in (1e-4, 1e-2, 2.0, 300.0):
        for unit in (True, False):
            pb = make_session(3000, 8, 2, sval, unit, seed=17)
            r64, r32 = references(pb)
            worst['lag1'] = max(worst['lag1'], scaled_error(r32['lag1'], r64, 'lag1'))
            worst['dmean'] = max(worst['dmean'], scaled_error(r32['dmean'], r64, 'dmean'))
            ent = entry_error(r32['dV'], r64)
            worst['dV'] = max(worst['dV'], ent)
            if sval == 1e-4:
                V = r64['Vs'].astype(np.float32).astype(np.float64)
                L = r64['lag1'].astype(np.float32).astype(np.float64)
                naive = V[:-1] + V[1:] - 2 * L[:-1]
                naive_worst = max(naive_worst, float(np.abs(naive / r64['dV'][:-1] - 1).max()))
                trans_small_s = max(trans_small_s, ent)
    print('float32 transcription over the sweep: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()) +
          f'; dV per entry at s = 1e-4: from rounded float32 outputs {naive_worst:.3g}, in-lane form {trans_small_s:.3g}')
    assert worst['lag1'] < 1e-5 and worst['dV'] < 1e-5 and worst['dmean'] < 5e-3
    assert naive_worst >= 10 * trans_small_s


def test_rts_step_with_increments_repeats_rts_step_bit_for_bit(sim):
    rng = np.random.default_rng(2)
    out = (ctypes.c_float * 7)()
    for i in range(4000):
        unit = i % 2
        a = 1.0 if unit else float(rng.choice([0.98, 0.5, -0.8, 1.0]))
        Pf, Ps = float(np.exp(rng.normal(0, 3))), float(np.exp(rng.normal(0, 3)))
        qs = float(np.exp(rng.normal(-3, 4)))
        sim.sim_rts_steps(unit, ctypes.c_float(a), ctypes.c_double(1 - a), ctypes.c_double(1 - a * a), ctypes.c_float(qs),
                          ctypes.c_float(rng.normal(0, 50)), ctypes.c_float(Ps), ctypes.c_float(rng.normal(0, 50)),
                          ctypes.c_float(Pf), out)
        assert out[0] == out[2] and out[1] == out[3]
        assert out[6] >= 0.0


# ---- moments of backward-sampled trajectories ----------------------------------------------------------------------
def moment_errors(e, Vs, lag1, dV):
    """e [n][T][N]: zero-mean posterior deviations.  Errors, in standard errors, of the sample variance of the
    increments, the sample lag-one covariance and the sample mean of the increments (dmean + mean of diff e)."""
    n = e.shape[0]
    de = np.diff(e, axis=1)
    var_err = np.abs(de.var(axis=0, ddof=1) - dV[:-1]) / (np.sqrt(2.0 / (n - 1)) * dV[:-1])
    lag = (e[:, :-1] * e[:, 1:]).mean(axis=0)
    lag_err = np.abs(lag - lag1[:-1]) / np.sqrt((Vs[:-1] * Vs[1:] + lag1[:-1] ** 2) / n)
    mean_err = np.abs(de.mean(axis=0)) / np.sqrt(dV[:-1] / n)
    return float(var_err.max()), float(lag_err.max()), float(mean_err.max())


def test_moments_of_backward_sampled_increments_match_the_reference():
    T, N, n = 40, 6, 4096
    rng = np.random.default_rng(8)
    a, c = np.array([1, 1, 0.97, 0.97, -0.8, 0.9]), np.array([1, 1, 1.3, 0.7, 1.0, 1.2])
    qs = rng.uniform(0.2, 2.0, N)
    var = rng.uniform(0.5, 4.0, (T, N))
    var[11, 2] = 1e3
    y = rng.normal(0, 2, (T, N))
    m0, S0 = np.zeros(N), np.full(N, 5.0)
    ms, Vs, lag1, dmean, dV = iref.scalar_increments(y, var, m0, S0, a, c, qs)
    _, Pf, ms2, Vs2, _ = sref.scalar_filter_smoother(y, var, m0, S0, a, c, qs)
    assert np.abs(ms - ms2).max() < 1e-12 and np.abs(Vs - Vs2).max() < 1e-12
    e = sref.scalar_deviations(Pf, a, qs, rng.normal(size=(n, T, N)))
    errs = moment_errors(e, Vs, lag1, dV)
    print('moments, in standard errors: increment variance %.2f, lag-one covariance %.2f, increment mean %.2f' % errs)
    assert max(errs) < 6


# ---- C ABI surface and Python argument checks ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_increments_entry_points_are_declared_bound_and_exported(lib):
    from eks_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_smooth_increments', 'eks_smooth_increments_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    fl = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    d = _lib.EksDims(256, 100000, 2, 2, fl | _lib.FLAG_VS_DIAG)
    need = lib.eks_smooth_increments_workspace_bytes(ctypes.byref(d))
    # 9 planes of [ceil(T/32)][N] floats plus the scan groups': under a third of ONE of the five output planes
    assert 9 * 3125 * 512 * 4 <= need < 100000 * 512 * 4 // 3
    g = _lib.EksDims(4, 100, 3, 4, 0)
    gneed = lib.eks_smooth_increments_workspace_bytes(ctypes.byref(g))
    assert gneed > 0
    assert lib.eks_smooth_increments_workspace_bytes(ctypes.byref(_lib.EksDims(4, 100, 3, 4, _lib.FLAG_VS_DIAG))) == gneed
    # refusals are returned before anything is enqueued (no device here, no valid pointers)
    one = ctypes.c_void_p(8)
    ins = [one] * 8

    def call(dims, ms=one, Vs=one, lag1=one, dmean=one, dV=one, ws=one, nbytes=1 << 40, inputs=ins):
        return lib.eks_smooth_increments(ctypes.byref(dims), *inputs, ms, Vs, lag1, dmean, dV, ws, nbytes, None)
    assert call(d, lag1=None, dmean=None, dV=None) == -1                  # all three new outputs NULL
    assert call(d, inputs=[None] + ins[1:]) == -1
    assert call(d, ws=None, nbytes=0) == -4
    assert call(d, nbytes=need - 1) == -4                                 # a byte short
    assert call(g, nbytes=gneed - 1) == -4
    full = _lib.EksDims(256, 100000, 2, 2, fl)                            # scalar chains without VS_DIAG
    assert call(full) == -3 and lib.eks_smooth_increments_workspace_bytes(ctypes.byref(full)) == 0
    big = _lib.EksDims(4, 100, 7, 7, 0)
    assert call(big) == -3 and lib.eks_smooth_increments_workspace_bytes(ctypes.byref(big)) == 0
    wide_o = _lib.EksDims(4, 100, 3, 65, 0)
    assert call(wide_o) == -3 and lib.eks_smooth_increments_workspace_bytes(ctypes.byref(wide_o)) == 0
    bad = _lib.EksDims(0, 10, 2, 2, fl | _lib.FLAG_VS_DIAG)
    assert call(bad) == -2 and lib.eks_smooth_increments_workspace_bytes(ctypes.byref(bad)) == 0
    # 2^24 chains x 64 chunks: a launch would index its threads beyond an int
    huge = _lib.EksDims(1 << 23, 2048, 2, 2, fl | _lib.FLAG_VS_DIAG)
    assert call(huge) == -2 and lib.eks_smooth_increments_workspace_bytes(ctypes.byref(huge)) == 0
    assert lib.eks_smooth_increments_workspace_bytes(ctypes.byref(_lib.EksDims(1 << 23, 2016, 2, 2, fl | _lib.FLAG_VS_DIAG))) > 0


def test_smooth_increments_validates_before_any_device_call(lib):
    import eks_amd
    from eks_amd import posterior
    assert eks_amd.smooth_increments is posterior.smooth_increments
    assert eks_amd.velocity_singlecam is posterior.velocity_singlecam
    assert posterior.SmoothIncrements._fields == NAMES
    K, T, D = 3, 20, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    good = dict(ys=np.zeros((K, T, D)), m0s=np.zeros((K, D)), S0s=eye, As=eye, Cs=eye, Qs=eye,
                ensemble_vars=np.ones((T, K, D)), s_finals=np.ones(K))

    def call(**kw):
        return posterior.smooth_increments(**{**good, **kw})
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
        posterior.velocity_singlecam(np.zeros((2, 2, 10, 3, 3)), ['a', 'b', 'c'], 1.0)       # two views
    with pytest.raises(ValueError):
        posterior.velocity_singlecam(np.zeros((2, 1, 10, 3, 3)), ['a', 'b'], 1.0)
    with pytest.raises(ValueError):
        posterior.velocity_singlecam(np.zeros((2, 1, 10, 3, 3)), ['a', 'b', 'c'], 1.0, fps=0.0)
    import torch
    if not torch.cuda.is_available():
        from eks_amd import _lib
        with pytest.raises(_lib.EksHipError):           # valid arguments reach the device check: no CPU fallback
            call()
