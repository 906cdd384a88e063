"""CPU: the posterior sampler without a GPU - the generator's known answers, the float32 lane arithmetic of
eks_amd/csrc/eks_sample_lane.hpp run from plain loops (tests/host_sim/sample_sim.cpp) against the float64 reference
(tests/sampling_ref.py), the exact law on short sessions, the C ABI surface and the Python argument checks.

Float32 bars: max(1e-5, 4 x the worst error of the float32 NumPy transcription on the same inputs) - 1e-5 is the
project's bar for ms / Vs, the transcription is what plain float32 reaches without a chunk scan, 4 x covers the scan.
Nothing is compared with the kernels' own output.

The deviations are read off the float32 output x = ms + e as x - ms, so they carry the output's own rounding,
2^-24 |x| whatever the algorithm does (where a variance sits at the 1e-12 floor sd is 1e-6 and that rounding is
several per cent of sd).  Two assertions follow from that: the raw error max |e - e_ref| / sd against the issue's
rule with the float32 transcription read through the same float32 output (ref.read_through_f32_output), and
`dev_error`, which allows each entry exactly its own 2^-24 |x| on top of the bar without it - the tighter of the two
wherever the output's rounding is small.  Both figures are printed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as ref  # noqa: E402

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'sample_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libsample_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


def make_chains(T, K, D, sval, unit, seed, spikes=True):
    """K keypoints x D independent chains, each with its own a, c, q, S0; variances with entries at the floor (1e-12)
    and at 1000 (the drivers' nan_replacement)."""
    rng = np.random.default_rng(seed)
    N = K * D
    a = np.ones(N) if unit else rng.uniform(0.9, 1.0, N)
    c = np.ones(N) if unit else rng.uniform(0.5, 1.5, N)
    q = rng.uniform(0.5, 2.0, N)
    S0d = rng.uniform(0.5, 20.0, N)
    m0 = rng.normal(0, 1, N)
    x = np.cumsum(rng.normal(0, np.sqrt(min(sval, 4.0)), (T, N)), axis=0)
    var = np.exp(rng.normal(0.5, 1.0, (T, N)))
    if spikes and T >= 4:
        hit = rng.random((T, N))
        var[hit < 0.02] = 1000.0
        var[hit > 0.99] = 1e-12
    y = c * x + rng.normal(0, 1, (T, N)) * np.sqrt(np.minimum(var, 50.0))

    def diag(v):
        out = np.zeros((K, D, D))
        out[:, np.arange(D), np.arange(D)] = v.reshape(K, D)
        return out
    par = dict(m0=m0.reshape(K, D).copy(), S0=diag(S0d), A=diag(a), C=diag(c), Q=diag(q), s=np.full(K, float(sval)))
    return dict(T=T, K=K, D=D, N=N, a=a, c=c, qs=q * sval, S0d=S0d, m0f=m0, par=par,
                y=np.ascontiguousarray(y, np.float32), var=np.ascontiguousarray(var, np.float32), unit=unit)


def dev_error(e, e_ref, x, sd):
    """max over entries of (|e - e_ref| - 2^-24 |x|)+ / sd: the error of the deviations beyond the rounding of the
    float32 output they were read from."""
    return float((np.maximum(np.abs(e - e_ref) - 2.0 ** -24 * np.abs(x), 0.0) / sd).max())


def run_sim(sim, pb, B, n_draws, noise=None, seed=0, gs=0, first_keypoint=0, first_draw=0):
    T, N, D = pb['T'], pb['N'], pb['D']
    ms = np.empty((T, N), np.float32)
    draws = np.empty((n_draws, T, N), np.float32)
    f, d = ctypes.c_float, ctypes.c_double
    par = pb['par']
    nz = None if noise is None else np.ascontiguousarray(noise, np.float32)
    rc = sim.sim_sample(T, N, D, B, gs, int(pb['unit']), _p(pb['y'], f), _p(pb['var'], f), _p(par['m0'], d),
                        _p(par['S0'], d), _p(par['A'], d), _p(par['C'], d), _p(par['Q'], d), _p(par['s'], d), n_draws,
                        ctypes.c_ulonglong(seed), first_keypoint, first_draw, _p(nz, f), _p(ms, f), _p(draws, f))
    assert rc == 0
    return ms, draws


def test_philox_known_answers_reference_and_lane_header(sim):
    for ctr, key, want in KAT:
        got = [int(w) for w in ref.philox4x32_10(ctr, key)]
        assert tuple(got) == want
        c = (ctypes.c_uint32 * 4)(*ctr)
        k = (ctypes.c_uint32 * 2)(*key)
        out = (ctypes.c_uint32 * 4)()
        sim.sim_philox(c, k, out)
        assert tuple(out) == want


def test_lane_generator_matches_the_reference_normals(sim):
    T, N, S = 11, 5, 3
    seed = 0x123456789abcdef
    z = np.empty((S, T, N), np.float32)
    sim.sim_sample_noise(T, N, S, ctypes.c_ulonglong(seed), 7, 2, _p(z, ctypes.c_float))
    zr = ref.scalar_noise(seed, T, N, S, first_chain=7, first_draw=2)
    # float32 log / sqrt / sin / cos on |z| <= 5.9: a few ulps of 5.9
    assert np.abs(z - zr).max() < 5e-6
    big = ref.scalar_noise(3, 4000, 8, 4)
    assert abs(big.mean()) < 6 / np.sqrt(big.size) and abs(big.var() - 1) < 6 * np.sqrt(2 / big.size)


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('sval', [0.01, 2.0, 300.0])
@pytest.mark.parametrize('T', [2, 37, 1000, 3001])
def test_host_sim_matches_float64_reference_for_every_chunk_length(sim, T, sval, unit):
    K, D, S = 3, 2, 3
    pb = make_chains(T, K, D, sval, unit, seed=T + int(sval * 10))
    z = np.random.default_rng(5).normal(size=(S, T, pb['N']))
    z32 = z.astype(np.float32)
    mf, Pf, ms64, Vs64, _ = ref.scalar_filter_smoother(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    e64 = ref.scalar_deviations(Pf, pb['a'], pb['qs'], z32)
    sd = np.sqrt(Vs64)
    e32 = ref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z32)
    trans = float(np.abs((e32 - e64) / sd).max())
    bar = max(1e-5, 4 * trans)
    trans_out = float(np.abs((ref.read_through_f32_output(ms64, e32) - e64) / sd).max())
    bar_raw = max(1e-5, 4 * trans_out)
    results = []
    for B, gs in ((4, 0), (8, 3), (16, 0), (32, 0), (32, 1)):
        ms0, d0 = run_sim(sim, pb, B, S, noise=np.zeros_like(z32), gs=gs)
        assert np.array_equal(d0, np.broadcast_to(ms0, d0.shape))          # z = 0 returns the smoothed mean
        assert (np.abs(ms0 - ms64) / np.abs(ms64).max(axis=0)).max() < 1e-5
        ms, dr = run_sim(sim, pb, B, S, noise=z32, gs=gs)
        assert np.array_equal(ms, ms0)
        err = dev_error(dr - ms[None], e64, dr, sd)
        raw = float(np.abs((dr - ms[None] - e64) / sd).max())
        print(f'T={T} s={sval} unit={unit} B={B} gs={gs}: e/sd error {err:.3g} beyond the output rounding '
              f'(transcription {trans:.3g}, bar {bar:.3g}); raw {raw:.3g} (transcription through the float32 output '
              f'{trans_out:.3g}, bar {bar_raw:.3g})')
        assert err < bar
        assert raw < bar_raw
        results.append(dr - ms[None])
    for r in results[1:]:                 # the chunk length changes float32 rounding of the scan only
        assert dev_error(r, results[0], 2 * np.abs(dr), sd) < 2 * bar


def _law_inputs(unit=False):
    pb = make_chains(12, 3, 2, 1.7, unit, seed=11, spikes=False)
    pb['var'][5, 1] = 1000.0                                               # one R spike
    return pb


def unit_noise(T, K, W):
    """draw 0: zeros; draw 1 + t W + w: the unit vector at (frame t, word w) for every keypoint."""
    z = np.zeros((T * W + 1, T, K, W), np.float32)
    for t in range(T):
        for w in range(W):
            z[1 + t * W + w, t, :, w] = 1.0
    return z


def test_exact_law_on_a_short_session_through_the_lane_code(sim):
    pb = _law_inputs()
    T, K, D, N = pb['T'], pb['K'], pb['D'], pb['N']
    z = unit_noise(T, K, D)
    ms, dr = run_sim(sim, pb, 8, z.shape[0], noise=z.reshape(-1, T, N))
    _, Pf, _, Vs64, _ = ref.scalar_filter_smoother(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    e64 = ref.scalar_deviations(Pf, pb['a'], pb['qs'], z.reshape(-1, T, N))
    e32 = ref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z.reshape(-1, T, N))
    worst = worst64 = worst32 = 0.0
    for n in range(N):
        w = n % D
        S = ref.dense_joint_posterior(pb['var'][:, n:n + 1], [[pb['S0d'][n]]], np.array([[pb['a'][n]]]),
                                      np.array([[pb['c'][n]]]), np.array([[pb['qs'][n]]]), 1.0)
        assert np.abs(np.diag(S) / Vs64[:, n] - 1).max() < 1e-12
        cols = [1 + t * D + w for t in range(T)]
        worst = max(worst, ref.law_error((dr[cols, :, n] - dr[0, :, n]).T.astype(np.float64), S))
        worst64 = max(worst64, ref.law_error(e64[cols, :, n].T, S))
        worst32 = max(worst32, ref.law_error(e32[cols, :, n].T.astype(np.float64), S))
    bar = max(1e-5, 4 * worst32)
    print(f'law: lane code {worst:.3g}, float64 recurrence {worst64:.3g}, float32 transcription {worst32:.3g}, bar {bar:.3g}')
    assert worst64 < 1e-13
    assert worst < bar


def dense_model(K, D, O, seed):
    rng = np.random.default_rng(seed)
    A = np.eye(D) * 0.95 + 0.05 * rng.normal(size=(K, D, D)) / np.sqrt(D)
    C = rng.normal(size=(K, O, D))
    Lq = rng.normal(size=(K, D, D)) * 0.4 + np.eye(D)
    Q = Lq @ np.swapaxes(Lq, 1, 2)                                   # non-diagonal, positive definite
    L0 = rng.normal(size=(K, D, D)) * 0.3 + 1.5 * np.eye(D)
    S0 = L0 @ np.swapaxes(L0, 1, 2)
    return dict(m0=rng.normal(size=(K, D)), S0=S0, A=A, C=C, Q=Q, s=rng.uniform(0.5, 2.0, K))


def drop_one_direction(M, names, seed):
    """M with one random eigen-direction per keypoint projected out of the matrices `names` (rank D - 1, exactly
    symmetric); D = 1 leaves a zero."""
    rng = np.random.default_rng(seed)
    M = dict(M)
    for nm in names:
        K, D, _ = M[nm].shape
        u = rng.normal(size=(K, D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        Pj = np.eye(D) - u[:, :, None] * u[:, None, :]
        X = Pj @ M[nm] @ Pj
        M[nm] = 0.5 * (X + np.swapaxes(X, 1, 2))
    return M


def short_dense_session(T, K, O, seed=1):
    rng = np.random.default_rng(seed)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O))).astype(np.float32)
    var[5, 1, min(2, O - 1)] = 1000.0
    return rng.normal(size=(T, K, O)).astype(np.float32), var


def dense_law_error(dev, var, M):
    """dev [1 + T W][T][K][D] from unit_noise: worst law_error over the keypoints against dense_joint_posterior."""
    T, K, D = dev.shape[1:]
    worst = 0.0
    for k in range(K):
        S = ref.dense_joint_posterior(var[:, k], M['S0'][k], M['A'][k], M['C'][k], M['Q'][k], M['s'][k])
        worst = max(worst, ref.law_error(dev[1:, :, k].reshape(-1, T * D).T.astype(np.float64), S))
    return worst


@pytest.mark.parametrize('singular', [(), ('Q',), ('S0',), ('Q', 'S0')])
@pytest.mark.parametrize('D,O', [(1, 3), (3, 4), (6, 12)])
def test_dense_durbin_koopman_reference_has_the_exact_law(D, O, singular):
    """ref.dense_durbin_koopman in float64 against the joint posterior covariance by plain linear algebra: the
    deviations of the T (D + O) unit normals are the columns of a factor of it.  Plain float64 gives 4.6e-14 at
    D, O = 1, 3, 2.8e-13 at 3, 4 and 4.8e-13 at 6, 12 (the worst over full-rank and rank D - 1 Q / S0); the bar is
    a decade above the worst of these.  At D = 1 a rank-deficient S0 is zero and leaves frame 0 without variance to
    normalise by, so that case keeps S0 and drops Q alone."""
    T, K = 12, 3
    if D == 1:
        singular = tuple(n for n in singular if n != 'S0')
    M = drop_one_direction(dense_model(K, D, O, seed=D), singular, seed=7)
    for nm in singular:
        assert np.linalg.matrix_rank(M[nm][0]) == D - 1
    y, var = short_dense_session(T, K, O)
    z = unit_noise(T, K, D + O)
    ms, Vs, dev = ref.dense_durbin_koopman(y, var, M['m0'], M['S0'], M['A'], M['C'], M['Q'], M['s'], z)
    assert dev.shape == (z.shape[0], T, K, D) and ms.shape == (T, K, D) and Vs.shape == (T, K, D, D)
    assert np.abs(dev[0]).max() == 0.0                                   # z = 0 returns the smoothed mean
    worst, bar = dense_law_error(dev, var, M), 5e-12
    print(f'law, float64 Durbin-Koopman reference D={D} O={O} singular={singular}: {worst:.3g}, bar {bar:.3g}')
    assert worst < bar
    for k in range(K):                                                   # its Vs are that covariance's diagonal blocks
        S = ref.dense_joint_posterior(var[:, k], M['S0'][k], M['A'][k], M['C'][k], M['Q'][k], M['s'][k])
        for t in range(T):
            blk = S[t * D:(t + 1) * D, t * D:(t + 1) * D]
            assert np.abs(Vs[t, k] - blk).max() < 1e-10 * np.abs(blk).max()
    # the float32-storage transcription differs by float32 rounding of O(|x+|), no more
    _, _, dev32 = ref.dense_durbin_koopman(y, var, M['m0'], M['S0'], M['A'], M['C'], M['Q'], M['s'], z,
                                           storage=np.float32)
    sd = np.sqrt(np.diagonal(Vs, axis1=-2, axis2=-1))
    assert 0.0 < np.abs((dev32 - dev) / sd).max() < 1e-5


def test_chol_psd_zero_pivot_rule():
    M = np.array([[[4.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 9.0]],          # second pivot exactly zero
                  [[0.0, 0.0, 0.0], [0.0, 2.0, 1.0], [0.0, 1.0, 5.0]]])         # first pivot zero
    L = ref.chol_psd(M)
    assert np.array_equal(L[0], [[2.0, 0, 0], [1.0, 0, 0], [0, 0, 3.0]])
    assert np.all(L[1][:, 0] == 0) and np.abs(L[1] @ L[1].T - M[1]).max() < 1e-15
    assert np.all(np.triu(L, 1) == 0)


def test_draws_do_not_depend_on_tiling_over_keypoints_or_draws(sim):
    pb = make_chains(70, 4, 2, 2.0, True, seed=3)
    _, full = run_sim(sim, pb, 16, 6, seed=99)
    sub = dict(pb, K=2, N=4, y=np.ascontiguousarray(pb['y'][:, 4:8]), var=np.ascontiguousarray(pb['var'][:, 4:8]),
               par={k: np.ascontiguousarray(v[2:4]) for k, v in pb['par'].items()})
    _, part = run_sim(sim, sub, 16, 2, seed=99, first_keypoint=2, first_draw=3)
    assert np.array_equal(part, full[3:5, :, 4:8])
    _, again = run_sim(sim, pb, 16, 6, seed=99)
    assert np.array_equal(full, again)
    _, other = run_sim(sim, pb, 16, 6, seed=100)
    assert not np.array_equal(full, other)


# ---- C ABI surface and Python argument checks ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_sampling_entry_points_are_declared_bound_and_exported(lib):
    from eks_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_sample', 'eks_sample_noise', 'eks_sample_noise_width', 'eks_sample_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and hasattr(lib, name)
    d = _lib.EksDims(256, 100000, 2, 2, _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC)
    assert lib.eks_sample_noise_width(ctypes.byref(d)) == 2
    g = _lib.EksDims(4, 100, 3, 4, 0)
    assert lib.eks_sample_noise_width(ctypes.byref(g)) == 7
    w1, w16 = (lib.eks_sample_workspace_bytes(ctypes.byref(d), n) for n in (1, 16))
    assert 0 < w1 < w16 < 16 * 100000 * 512 * 4 // 8        # scratch stays far below the draws themselves
    assert lib.eks_sample_workspace_bytes(ctypes.byref(d), 0) == 0
    assert lib.eks_sample_workspace_bytes(ctypes.byref(g), 2) > 0
    # argument errors are reported before anything is enqueued
    one = ctypes.c_void_p(8)
    args = [one] * 8
    assert lib.eks_sample(ctypes.byref(d), *args, 0, 0, 0, 0, None, None, one, one, 1 << 40, None) == -2
    assert lib.eks_sample(ctypes.byref(d), *args, 1, 0, 0, 0, None, None, None, one, 1 << 40, None) == -1
    assert lib.eks_sample(ctypes.byref(d), *args, 1, 0, 0, 0, None, None, one, None, 0, None) == -4
    assert lib.eks_sample(ctypes.byref(d), *args, 1, 0, 0, 0, None, None, one, one, 16, None) == -4
    big = _lib.EksDims(4, 100, 7, 7, 0)
    assert lib.eks_sample(ctypes.byref(big), *args, 1, 0, 0, 0, None, None, one, one, 1 << 40, None) == -3
    need = lib.eks_sample_workspace_bytes(ctypes.byref(g), 2)
    assert lib.eks_sample(ctypes.byref(g), *args, 2, 0, 0, 0, None, None, one, one, need - 1, None) == -4   # a byte short
    # (n_draws + 1) K D > 2^24 stacked chains on a general model: a shape error, and no workspace size
    wide = _lib.EksDims(1 << 20, 4, 3, 4, 0)
    assert lib.eks_sample(ctypes.byref(wide), *args, 7, 0, 0, 0, None, None, one, one, 1 << 40, None) == -2
    assert lib.eks_sample_workspace_bytes(ctypes.byref(wide), 7) == 0
    assert lib.eks_sample_workspace_bytes(ctypes.byref(wide), 4) > 0
    assert lib.eks_sample_workspace_bytes(ctypes.byref(big), 1) == 0
    assert lib.eks_sample_noise(ctypes.byref(_lib.EksDims(4, 100, 7, 64, 0)), 1, 0, 0, 0, one, None) == -2   # W = 71
    assert lib.eks_sample_noise(ctypes.byref(big), 1, 0, 0, 0, one, None) == -3
    assert lib.eks_sample_noise(ctypes.byref(d), 0, 0, 0, 0, one, None) == -2
    assert lib.eks_sample_noise(ctypes.byref(d), 1, 0, 0, 0, None, None) == -1


def test_sample_kalman_posterior_validates_before_any_device_call(lib):
    import eks_amd
    from eks_amd.posterior import sample_kalman_posterior
    assert eks_amd.sample_kalman_posterior is sample_kalman_posterior and callable(eks_amd.sample_singlecam)
    K, T, D = 3, 20, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    good = dict(ys=np.zeros((K, T, D)), m0s=np.zeros((K, D)), S0s=eye, As=eye, Cs=eye, Qs=eye,
                ensemble_vars=np.ones((T, K, D)), s_finals=np.ones(K), n_draws=4)

    def call(**kw):
        return sample_kalman_posterior(**{**good, **kw})
    with pytest.raises(ValueError):
        call(n_draws=0)
    with pytest.raises(ValueError):
        call(ys=np.zeros((K, T)))
    with pytest.raises(ValueError):
        call(ensemble_vars=np.ones((K, T, D)))
    with pytest.raises(ValueError):
        call(Qs=np.tile(np.eye(3), (K, 1, 1)))
    with pytest.raises(ValueError):
        call(s_finals=np.ones(K + 1))
    with pytest.raises(ValueError):
        call(first_draw=-1)
    with pytest.raises(NotImplementedError):
        call(h_fn=lambda x: x)
    with pytest.raises(ValueError):
        call(noise=np.zeros((4, T, K, D + D)))          # diagonal model: W = D
    dense = eye.copy()
    dense[:, 0, 1] = dense[:, 1, 0] = 0.3
    with pytest.raises(ValueError):
        call(Qs=dense, noise=np.zeros((4, T, K, D)))    # general model: W = D + O
    import torch
    if not torch.cuda.is_available():
        from eks_amd import _lib
        with pytest.raises(_lib.EksHipError):           # valid arguments reach the device check: no CPU fallback
            call()


def test_draw_groups_follow_the_memory_budget(lib):
    from eks_amd import _lib
    from eks_amd.posterior import draws_per_group
    fl = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    assert draws_per_group(64, 20000, 2, 2, fl, 16, 1 << 40) == 16
    g = draws_per_group(64, 20000, 2, 2, fl, 16, 50 << 20)
    assert 1 <= g < 16
    assert draws_per_group(64, 20000, 2, 2, fl, 16, 1) == 1


@pytest.mark.parametrize('D,O', [(1, 3), (3, 4), (6, 12)])
def test_reference_filter_by_scalar_updates_against_both_formulations_of_the_oracle(D, O):
    """ref.filter_by_scalar_updates (+ the oracle's RTS pass), the smoother inside dense_durbin_koopman, against
    oracle.eks_oracle.kalman_smoother (joint update through inv(S)) on 300 frames with variances within four decades,
    and against the oracle's information-form smoother after one variance of the first and of the last keypoint is
    set to the 1e30 clip, where inv(S) is not to be trusted.  Plain float64 gives at most 3.8e-13 (Vs, D, O = 6, 12)
    and 1.9e-14; the bar is 5e-12, a decade above the larger."""
    from oracle import eks_oracle as orc
    T, K = 300, 3
    M = dense_model(K, D, O, seed=D)
    rng = np.random.default_rng(5)
    R = np.exp(rng.normal(0, 0.7, (K, T, O)))
    R[:, ::17] = 1000.0
    y = rng.normal(size=(K, T, O))
    par = tuple(M[k] for k in ('m0', 'S0', 'A', 'C', 'Q', 's'))

    def worst(a, Va, b, Vb):
        return max(float((np.abs(a - b) / np.abs(a).max(axis=1, keepdims=True)).max()),
                   float((np.abs(Va - Vb) / np.abs(Va).max(axis=1, keepdims=True)).max()))
    figures = []
    for spread in (False, True):
        if spread:
            R[0, T // 3, 0] = R[K - 1, (2 * T) // 3, O - 1] = ref.VAR_CEIL
            a, Va = orc.info_form_smoother(y, *par, R)[:2]
        else:
            a, Va = orc.kalman_smoother(y, *par, R)[:2]
        mf, Pf = ref.filter_by_scalar_updates(y, *par, R)
        b, Vb = orc.rts_smoother(mf, Pf, M['A'], M['Q'], M['s'])
        figures.append(worst(a, Va, b, Vb))
    print(f'scalar-update filter D={D} O={O}: against kalman_smoother {figures[0]:.3g}, with a variance at 1e30 against '
          f'the information form {figures[1]:.3g}, bar 5e-12')
    assert max(figures) < 5e-12
