"""CPU: the general-model chunk bodies of eks_smooth_increments and eks_em_stats without a GPU - dense_increments_chunk
(eks_amd/csrc/eks_increments_lane.hpp) and dense_em_chunk (eks_em_lane.hpp), i.e. the shared forward pass and backward
walker of eks_dense_lane.hpp with their two visitors, run from plain loops over chunked sequences
(tests/host_sim/dense_walk_sim.cpp) against the float64 references of tests/increments_ref.py and tests/em_ref.py.

Bars: those of the references' GPU tests.  Increments (tests/test_gpu_increments.py: check_dense), per keypoint as a
fraction of the keypoint's largest |reference| (of Vs for lag1): ms, Vs within 1e-5, the three increment outputs
within max(1e-5, 4 x the error of the reference rounded to float32); row T-1 of the increment outputs exactly zero.
EM (tests/test_gpu_em.py: check_dense): Sw within 1.3e-12 of the keypoint's largest |Sw| entry, exact zeros at T = 1.

Shapes: 16-frame chunks; T = 1 (one frame), 2 (one transition), 16 (exactly one chunk), 17 (a one-frame last chunk),
70 (a ragged last chunk of 6); identity and general A; one case with variances below the 1e-12 clip."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref  # noqa: E402
import increments_ref as iref  # noqa: E402
import sampling_ref as sref  # noqa: E402
from test_increments_cpu import NAMES, dense_case  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')
NEW = ('lag1', 'dmean', 'dV')
K, B = 3, 16
DENSE_SW_BAR = 1.3e-12          # tests/test_gpu_em.py: min(100 x the measured 1.3e-14, 1e-8)


@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'dense_walk_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libdense_walk_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def model(D, O, identity_a, seed):
    """tests/test_gpu_increments.py: stable(dense_case(...)) - a general A scaled to spectral radius <= 0.99, or I."""
    M = dense_case(K, D, O, False, seed=seed)
    if identity_a:
        M['A'] = np.tile(np.eye(D), (K, 1, 1))
    else:
        rho = np.abs(np.linalg.eigvals(M['A'])).max(axis=1)
        M['A'] = M['A'] * np.minimum(1.0, 0.99 / rho)[:, None, None]
    return M


def session(M, T, O, seed):
    """tests/test_gpu_increments.py: dense_session - simulated from the model, 2 % of the frames occluded."""
    rng = np.random.default_rng(seed)
    D = M['m0'].shape[1]
    L0, Lq = sref.chol_psd(M['S0']), sref.chol_psd(M['s'][:, None, None] * M['Q'])
    x = M['m0'] + np.einsum('kij,kj->ki', L0, rng.normal(size=(K, D)))
    xs = np.empty((T, K, D))
    for t in range(T):
        if t:
            x = np.einsum('kij,kj->ki', M['A'], x) + np.einsum('kij,kj->ki', Lq, rng.normal(size=(K, D)))
        xs[t] = x
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    y = np.einsum('koj,tkj->tko', M['C'], xs) + np.sqrt(var) * rng.normal(size=(T, K, O))
    var[rng.random((T, K)) < 0.02] = 1000.0
    return y.astype(np.float32), var.astype(np.float32)


def run_increments(sim, M, y, var, vs_diag):
    T, _, O = y.shape
    D = M['m0'].shape[1]
    par = [np.ascontiguousarray(M[k], np.float64) for k in PARAMS]
    shape = dict(ms=(T, K, D), dmean=(T, K, D))
    out = {n: np.full(shape.get(n, (T, K, D) if vs_diag else (T, K, D, D)), np.nan, np.float32) for n in NAMES}
    rc = sim.sim_dense_increments(T, K, D, O, B, int(vs_diag), _p(y, ctypes.c_float), _p(var, ctypes.c_float),
                                  *(_p(a, ctypes.c_double) for a in par), *(_p(out[n], ctypes.c_float) for n in NAMES))
    assert rc == 0
    return out


def run_em(sim, M, y, var, diag):
    T, _, O = y.shape
    D = M['m0'].shape[1]
    par = [np.ascontiguousarray(M[k], np.float64) for k in PARAMS]
    Sw = np.full((K, D) if diag else (K, D, D), np.nan)
    rc = sim.sim_dense_em(T, K, D, O, B, int(diag), _p(y, ctypes.c_float), _p(var, ctypes.c_float),
                          *(_p(a, ctypes.c_double) for a in par), _p(Sw, ctypes.c_double))
    assert rc == 0
    return Sw


def keypoint_error(x, ref, scale_ref):
    e = np.abs(x.astype(np.float64) - ref).transpose(1, 0, *range(2, ref.ndim)).reshape(K, -1).max(axis=1)
    s = np.abs(scale_ref).transpose(1, 0, *range(2, scale_ref.ndim)).reshape(K, -1).max(axis=1)
    return float((e / s).max())


def check_increments(label, M, y, var, got, vs_diag):
    r64 = dict(zip(NAMES, iref.dense_increments(y, var, *(M[k] for k in PARAMS))))
    T = y.shape[0]
    figs = []
    for n in NAMES:
        ref, t32 = r64[n], r64[n].astype(np.float32)
        if vs_diag and n not in ('ms', 'dmean'):
            ref, t32 = (np.diagonal(a, axis1=-2, axis2=-1) for a in (ref, t32))
        assert got[n].shape == ref.shape and np.isfinite(got[n]).all(), f'{label}: {n}'
        if n in NEW:
            assert not got[n][-1].any(), f'{label}: row T-1 of {n} is not zero'
            if T == 1:
                continue
        scale_ref = r64['Vs'] if n == 'lag1' else r64[n]
        err, trans = keypoint_error(got[n], ref, scale_ref), keypoint_error(t32, ref, scale_ref)
        bar = 1e-5 if n in ('ms', 'Vs') else max(1e-5, 4 * trans)
        figs.append(f'{n} {err:.3g} ({trans:.3g})')
        print(f'{label}: {figs[-1]}')
        assert err <= bar, f'{label}: {n} {err:.3g} against the bar {bar:.3g} (transcription {trans:.3g})'


def check_em(label, M, y, var, got, diag):
    if y.shape[0] == 1:
        assert not got.any(), f'{label}: T = 1 must give exact zeros'
        return
    ref = em_ref.dense_em_stats(y, var, *(M[k] for k in PARAMS))
    scale = np.abs(ref).reshape(K, -1).max(axis=1)
    want = np.diagonal(ref, axis1=1, axis2=2) if diag else ref
    assert np.isfinite(got).all()
    err = float((np.abs(got - want).reshape(K, -1).max(axis=1) / scale).max())
    print(f'{label}: Sw {err:.3g} of the keypoint\'s largest entry')
    assert err <= DENSE_SW_BAR, f'{label}: Sw {err:.3g} against the bar {DENSE_SW_BAR:.3g}'


@pytest.mark.parametrize('identity_a', [True, False])
@pytest.mark.parametrize('T', [1, 2, 16, 17, 70])
@pytest.mark.parametrize('D,O', [(d, o) for d in (1, 2, 3) for o in (1, 4)])
def test_chunk_bodies_against_the_float64_references(sim, D, O, T, identity_a):
    M = model(D, O, identity_a, seed=10 * D + O)
    y, var = session(M, T, O, seed=T)
    for diag in (False, True):
        label = f'D={D} O={O} T={T} A={"I" if identity_a else "general"} diag={diag}'
        check_increments(label, M, y, var, run_increments(sim, M, y, var, diag), diag)
        check_em(label, M, y, var, run_em(sim, M, y, var, diag), diag)


@pytest.mark.parametrize('identity_a', [True, False])
def test_chunk_bodies_with_variances_at_the_clip(sim, identity_a):
    """Single variances below the 1e-12 floor (the lane clips them to it, as the references do): in the middle of a
    chunk, on a chunk's first frame and on a chunk's last.  One observation of a frame, not a whole frame: with all
    O > D observations of a frame at the clip the covariance-form recursion of the float64 reference is itself only
    good to 1e-2 (tests/test_host_sim.py has the measurement), so it could not hold the lane code to 1e-5."""
    D, O, T = 3, 4, 70
    M = model(D, O, identity_a, seed=7)
    y, var = session(M, T, O, seed=3)
    var[20, 1, 2] = 1e-13
    var[32, 0, 0] = 0.0
    var[47, 2, 3] = 1e-20
    for diag in (False, True):
        label = f'clip A={"I" if identity_a else "general"} diag={diag}'
        check_increments(label, M, y, var, run_increments(sim, M, y, var, diag), diag)
        check_em(label, M, y, var, run_em(sim, M, y, var, diag), diag)
