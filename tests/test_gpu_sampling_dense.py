"""GPU: eks_sample on general models (Durbin-Koopman, eks_amd/csrc/eks_sample_dense.hip) at the sizes where its
stacked smoothing call over (n_draws + 1) K chains takes each kernel organisation, against the float64 reference
ref.dense_durbin_koopman fed the same float32 normals.

Bars as in tests/test_gpu_sampling.py: the deviations draws - ms are compared with the float64 reference's relative
to the float64 posterior standard deviation, beyond the rounding of the float32 output they are read from
(dev_error), under max(1e-5, 4 x the worst error of the float32-storage transcription on the same inputs) - the
same float64 construction with x+, y+ and the stacked means rounded to float32, where the kernels store float32.
The raw figure is held to the same rule with the transcription read through the float32 output.  ms is held to the
suite's 1e-5.  Nothing is compared with the kernels' own output.

Which organisation a case takes is derived from dense_path / dense_chunk (eks_dense.hip), dense_wave_covers /
dw_chunk_frames (eks_dense_wave.hip) and dense_wide_covers (eks_dense_wide.hip) for (T, Kp = (n_draws + 1) K, D, O):
  wave    : D in {2, 3}, O in {2, 4, 6, 8} (or D = 3, O in {10, 12}) and Kp ceil(ceil(T / B) / 64) <= 1024, B the
            first of 2, 4 with Kp ceil(ceil(T / B) / 64) <= 160, else 8 (O > 8: always 8);
  runs    : otherwise D in {2, 3}, O in {2, 4, 6, 8}; chunks of 16 frames while Kp ceil(T / 16) <= 2^18, else 32;
  generic : everything else (and everything under EKS_DENSE_LEGACY), same chunk rule.

Every parity test prints the kernels' figure, the transcription's figure and the bar.  Measured on the MI355X, worst
deviation error relative to the posterior standard deviation beyond the output rounding, kernels / transcription
(bar), stable A and then A = I:
  wave, 8-frame chunks (T = 4001, Kp = 32)     : 1.73e-5 / 1.75e-5 (7.0e-5);  6.86e-5 / 1.06e-4 (4.2e-4)
  runs, 16-frame chunks (T = 1500, Kp = 1280)  : 1.15e-5 / 1.16e-5 (4.6e-5);  5.74e-5 / 6.15e-5 (2.5e-4)
  runs, 32-frame chunks (T = 6000, Kp = 800)   : 1.36e-5 / 1.48e-5 (5.9e-5);  2.00e-4 / 2.61e-4 (1.0e-3)
  generic, 16-frame chunks (T = 1100, stable A): 5.0e-6 / 6.7e-6 (1, 3), 4.4e-6 / 4.9e-6 (3, 5), 9.9e-6 / 1.2e-5
      (4, 8), 8.7e-6 / 9.5e-6 (5, 6), 1.20e-5 / 1.24e-5 (6, 12), 2.1e-6 / 2.4e-6 (2, 2 under EKS_DENSE_LEGACY)
  generic with A = I (the wave case under EKS_DENSE_LEGACY; the runs case under EKS_DENSE_TREE_SCAN): 6.86e-5 / 1.06e-4;
      5.74e-5 / 6.15e-5 - the figures of the specialised kernels to three digits
  wave at T = 1100: 2.1e-6 / 2.4e-6 (2, 2; 2 frames), 4.5e-6 / 5.1e-6 (2, 2; 4 frames), 1.45e-5 / 1.51e-5 (3, 10)
  golden multi-camera model (A = I, T = 2000, Kp = 68): 1.48e-4 / 1.52e-4 (6.1e-4)
  singular Q, S0, both: 1.35e-5 / 1.62e-5, 1.24e-5 / 1.26e-5, 1.49e-5 / 1.73e-5; law at T = 12: 2.8e-7 to 6.3e-7, equal
      to the transcription's
  ms against the reference's: 4.1e-8 to 5.8e-8 everywhere (bar 1e-5).
The smoother's arithmetic is float64 whatever the organisation, so the kernels never exceed the transcription: what
they show is the float32 stores of x+, y+ and the stacked means, 1e-5 of the posterior sd with a stable A and 1e-4
to 3e-4 with A = I at these lengths."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as ref  # noqa: E402
from test_sampling_cpu import (dense_law_error, dense_model, dev_error, drop_one_direction, make_chains,  # noqa: E402
                               unit_noise)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def stable_model(K, D, O, seed, unit_root=False):
    """dense_model with every A scaled to a spectral radius of at most 0.99 (dense_model's A = 0.95 I + noise exceeds
    1 for a few keypoints in a hundred, and x+ then overflows float32 over thousands of frames), or A = I."""
    M = dense_model(K, D, O, seed)
    if unit_root:
        M['A'] = np.tile(np.eye(D), (K, 1, 1))
    else:
        rho = np.abs(np.linalg.eigvals(M['A'])).max(axis=1)
        M['A'] = M['A'] * np.minimum(1.0, 0.99 / rho)[:, None, None]
    return M


def session(M, T, O, seed):
    """y [T][K][O] simulated from the model itself and variances [T][K][O] with whole frames at 1000 (the drivers'
    nan_replacement), one entry at inf and one at 1e30 (both meet the kernels' clip at 1e30)."""
    rng = np.random.default_rng(seed)
    K, D = M['m0'].shape
    L0, Lq = ref.chol_psd(M['S0']), ref.chol_psd(M['s'][:, None, None] * M['Q'])
    x = M['m0'] + np.einsum('kij,kj->ki', L0, rng.normal(size=(K, D)))
    xs = np.empty((T, K, D))
    for t in range(T):
        if t:
            x = np.einsum('kij,kj->ki', M['A'], x) + np.einsum('kij,kj->ki', Lq, rng.normal(size=(K, D)))
        xs[t] = x
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    y = np.einsum('koj,tkj->tko', M['C'], xs) + np.sqrt(var) * rng.normal(size=(T, K, O))
    var[rng.random((T, K)) < 0.02] = 1000.0
    var = var.astype(np.float32)
    var[T // 3, 0, 0] = np.inf
    var[(2 * T) // 3, K - 1, O - 1] = 1e30
    return y.astype(np.float32), var


def compared_keypoints(K, most=8, seed=0):
    """All keypoints, or - where the float64 reference over every stacked chain would take minutes - a fixed seeded
    subset that always holds the first and the last keypoint: with every draw of those keypoints compared, the first
    and the last chain of every set of the stacked problem are among the compared chains."""
    if K <= most:
        return np.arange(K)
    mid = np.random.default_rng(seed).choice(np.arange(1, K - 1), most - 2, replace=False)
    return np.sort(np.concatenate([[0, K - 1], mid]))


_REF_CACHE = {}


def reference(key, M, y, var, z, ks):
    """(ms64, sd, dev64, dev32, ms32) on keypoints ks; cached per case (the knob variants share their inputs)."""
    if key not in _REF_CACHE:
        args = (y[:, ks], var[:, ks], *(M[k][ks] for k in PARAMS), z[:, :, ks])
        ms64, Vs, dev64 = ref.dense_durbin_koopman(*args)
        ms32, _, dev32 = ref.dense_durbin_koopman(*args, storage=np.float32, round_output=False)
        sd = np.sqrt(np.diagonal(Vs, axis1=-2, axis2=-1))
        _REF_CACHE[key] = (ms64, sd, dev64, dev32, ms32)
    return _REF_CACHE[key]


def check_parity(label, key, M, y, var, dr, ms, z, ks):
    """dr (n, T, K, D), ms (T, K, D) from the kernels against the reference on keypoints ks; prints and asserts."""
    assert np.isfinite(dr).all() and np.isfinite(ms).all()
    n, T, K, D = dr.shape
    assert len(ks) == K or (n + 1) * len(ks) >= 32
    ms64, sd, dev64, dev32, ms32 = reference(key, M, y, var, z, ks)
    dr, ms = dr[:, :, ks].astype(np.float64), ms[:, ks].astype(np.float64)
    trans = float(np.abs((dev32 - dev64) / sd).max())
    bar = max(1e-5, 4 * trans)
    err = dev_error(dr - ms[None], dev64, dr, sd)
    raw = float(np.abs((dr - ms[None] - dev64) / sd).max())
    through = (ms32[None] + dev32).astype(np.float32).astype(np.float64) - ms32[None]
    trans_out = float(np.abs((through - dev64) / sd).max())
    bar_raw = max(1e-5, 4 * trans_out)
    ms_err = float((np.abs(ms - ms64) / np.abs(ms64).max(axis=0)).max())
    print(f'parity {label} ({(n + 1) * len(ks)} of {(n + 1) * K} chains): kernels {err:.3g} beyond the output '
          f'rounding, float32-storage transcription {trans:.3g}, bar {bar:.3g}; raw {raw:.3g}, transcription through '
          f'the float32 output {trans_out:.3g}, bar {bar_raw:.3g}; ms {ms_err:.3g}, bar 1e-05')
    assert err < bar
    assert raw < bar_raw
    assert ms_err < 1e-5


def gpu_sample(M, y, var, z, flags=0):
    from eks_amd import hip_ops
    dr, ms = hip_ops.sample(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), z.shape[0], flags=flags, noise=_dev(z),
                            want_mean=True)
    torch.cuda.synchronize()
    return dr.cpu().numpy(), ms.cpu().numpy()


def run_case(label, T, K, D, O, n_draws, unit_root, seed, singular=()):
    M = drop_one_direction(stable_model(K, D, O, seed, unit_root), singular, seed=seed + 1)
    y, var = session(M, T, O, seed + 2)
    z = np.random.default_rng(seed + 3).normal(size=(n_draws, T, K, D + O)).astype(np.float32)
    dr, ms = gpu_sample(M, y, var, z)
    key = (T, K, D, O, n_draws, unit_root, seed, singular)
    check_parity(f'{label} T={T} K={K} D={D} O={O} draws={n_draws} A={"I" if unit_root else "stable"}', key, M, y, var,
                 dr, ms, z, compared_keypoints(K))


# Kp = 8 x 4 = 32, D, O = 3, 4: 32 ceil(2001 / 64) = 1024 and 32 ceil(1001 / 64) = 512 exceed 160, so 8-frame chunks:
# ceil(4001 / 8) = 501 chunks = 8 blocks of 64 per chain, 32 x 8 = 256 <= 1024 units -> wave
WAVE = dict(T=4001, K=4, D=3, O=4, n_draws=7, seed=100)
# Kp = 8 x 160 = 1280: 1280 ceil(188 / 64) = 3840 > 1024 units -> not wave; 1280 ceil(1500 / 16) = 120 320 <= 2^18 ->
# 16-frame chunks (94 per chain); D, O = 3, 4 -> runs
RUNS16 = dict(T=1500, K=160, D=3, O=4, n_draws=7, seed=200)
# Kp = 8 x 100 = 800: 800 ceil(750 / 64) = 9600 > 1024 units -> not wave; 800 ceil(6000 / 16) = 300 000 > 2^18 ->
# 32-frame chunks (188 per chain); D, O = 2, 4 -> runs
RUNS32 = dict(T=6000, K=100, D=2, O=4, n_draws=7, seed=300)


@pytest.mark.parametrize('unit_root', [False, True])
def test_parity_at_size_wave_many_blocks(unit_root):
    run_case('wave B=8', unit_root=unit_root, **WAVE)


@pytest.mark.parametrize('unit_root', [False, True])
@pytest.mark.parametrize('knob', ['EKS_DENSE_LEGACY', 'EKS_DENSE_TREE_SCAN'])
def test_parity_at_size_wave_shape_under_the_generic_knobs(knob, unit_root, set_knob):
    """The inputs of the wave case again.  EKS_DENSE_LEGACY switches the wave and the keypoint-major kernels off: the
    stacked call takes the generic kernels with 16-frame chunks (251 chunks = 4 blocks of 64).  dense_wave_covers does
    not read EKS_DENSE_TREE_SCAN, so under that knob this shape stays on the wave form; the knob's effect (runs ->
    generic with the keypoint-major summarize and the tree scan) is asserted on the runs shape below."""
    set_knob(knob, '1')
    run_case(f'wave shape, {knob}=1', unit_root=unit_root, **WAVE)


@pytest.mark.parametrize('unit_root', [False, True])
def test_parity_at_size_runs_16_frame_chunks(unit_root):
    """Reference on 8 of the 160 keypoints (64 of the 1280 stacked chains, first and last of every set included):
    batched NumPy filter + RTS over all 1280 chains costs 3.8 ms per frame step here against 0.2 ms for a handful."""
    run_case('runs B=16', unit_root=unit_root, **RUNS16)


def test_parity_at_size_runs_shape_with_the_tree_scan(set_knob):
    """EKS_DENSE_TREE_SCAN on the runs shape: dense_path returns generic, the keypoint-major summarize feeding the
    tree scan over 94 sixteen-frame chunks (2 blocks of 64)."""
    set_knob('EKS_DENSE_TREE_SCAN', '1')
    run_case('runs shape, EKS_DENSE_TREE_SCAN=1', unit_root=True, **RUNS16)


@pytest.mark.parametrize('unit_root', [False, True])
def test_parity_at_size_runs_32_frame_chunks(unit_root):
    """Reference on 8 of the 100 keypoints (64 of the 800 stacked chains), as above."""
    run_case('runs B=32', unit_root=unit_root, **RUNS32)


# T = 1100 = 68 x 16 + 12: 69 sixteen-frame chunks, one past a block of 64, the last one partial.
@pytest.mark.parametrize('D,O,K,n_draws,org', [
    (1, 3, 3, 3, 'generic B=16'),        # D = 1: neither wave nor runs
    (3, 5, 3, 3, 'generic B=16'),        # O = 5: neither wave nor runs
    (4, 8, 2, 2, 'generic B=16'),        # D = 4
    (5, 6, 3, 2, 'generic B=16'),        # D = 5
    (6, 12, 3, 3, 'generic B=16'),       # D = 6
    (2, 64, 3, 2, 'generic B=16'),       # the widest observation the library accepts
    (2, 2, 3, 3, 'wave B=2'),            # Kp = 12: 12 ceil(550 / 64) = 108 <= 160 units -> wave, 2-frame chunks, 9 blocks
    (2, 2, 5, 5, 'wave B=4'),            # Kp = 30: 30 x 9 = 270 > 160, 30 ceil(275 / 64) = 150 <= 160 -> 4-frame chunks
    (3, 10, 3, 3, 'wave B=8'),           # O > 8 keeps 8 frames: 138 chunks, 12 x 3 = 36 units -> wave (five-camera form)
])
def test_parity_generic_shapes_across_a_block_of_chunks(D, O, K, n_draws, org):
    """D, O = 2, 2 cannot reach the generic kernels without a knob (few chains: wave; many: runs), so it is run on the
    wave form at the two chunk lengths the larger cases do not take."""
    run_case(org, 1100, K, D, O, n_draws, False, seed=400 + 10 * D + O)


def test_parity_generic_kernels_at_d_o_2_2_under_the_legacy_knob(set_knob):
    """The D, O = 2, 2, Kp = 12 case above under EKS_DENSE_LEGACY: the only way D = 2 meets the generic kernels
    (16-frame chunks, 69 of them: one past a block of 64, the last partial)."""
    set_knob('EKS_DENSE_LEGACY', '1')
    run_case('generic B=16, EKS_DENSE_LEGACY=1', 1100, 3, 2, 2, 3, False, seed=400 + 10 * 2 + 2)


@pytest.mark.parametrize('singular', [('Q',), ('S0',), ('Q', 'S0')])
def test_singular_q_and_s0_same_noise_parity(singular):
    """One zero eigen-direction in Q, in S0, in both (D, O = 3, 4; Kp = 16: wave, 2-frame chunks): the draws carry no
    variance the reference does not have."""
    run_case(f'singular {"+".join(singular)}', 1100, 4, 3, 4, 3, False, seed=500, singular=singular)


@pytest.mark.parametrize('singular', [('Q',), ('S0',), ('Q', 'S0')])
def test_singular_q_and_s0_exact_law_on_a_short_session(singular):
    from test_sampling_cpu import short_dense_session
    T, K, D, O = 12, 3, 3, 4
    M = drop_one_direction(dense_model(K, D, O, seed=D), singular, seed=7)
    y, var = short_dense_session(T, K, O)
    z = unit_noise(T, K, D + O)
    dr, ms = gpu_sample(M, y, var, z)
    assert np.abs(dr[0] - ms).max() <= 1e-5 * np.abs(ms).max()
    _, _, dev32 = ref.dense_durbin_koopman(y, var, *(M[k] for k in PARAMS), z, storage=np.float32)
    worst = dense_law_error(dr.astype(np.float64) - dr[:1], var, M)
    worst32 = dense_law_error(dev32, var, M)
    bar = max(1e-5, 4 * worst32)
    print(f'law, singular {singular}: kernels {worst:.3g}, float32-storage transcription {worst32:.3g}, bar {bar:.3g}')
    assert worst < bar


def test_real_multicam_model_same_noise_parity(golden_dir):
    """The multi-camera driver's model on the golden mirror-mouse markers: D = 3, O = 4, A = I, PCA loadings, T = 2000,
    K = 4, s = 10, 16 draws through eks_amd.posterior (Kp = 68: 68 ceil(250 / 64) = 272 units -> wave, 8-frame chunks)."""
    from eks_amd.posterior import sample_kalman_posterior
    from oracle import eks_oracle as orc
    a = orc.multicam_arrays(np.load(os.path.join(golden_dir, 'mirror_mouse_multicam.npz'))['markers'])
    K, T, O = a['ys'].shape
    D, n = 3, 16
    assert (T, K, O) == (2000, 4, 4) and np.array_equal(a['As'], np.tile(np.eye(D), (K, 1, 1)))
    M = dict(m0=a['m0s'], S0=a['S0s'], A=a['As'], C=a['Cs'], Q=a['Qs'], s=np.full(K, 10.0))
    var = np.ascontiguousarray(a['ensemble_vars'], np.float32)
    var[np.random.default_rng(5).random((T, K)) < 0.02] = 1000.0
    var[T // 3, 0, 0] = np.inf
    var[(2 * T) // 3, K - 1, O - 1] = 1e30
    ys = np.ascontiguousarray(a['ys'], np.float32)
    z = np.random.default_rng(6).normal(size=(n, T, K, D + O)).astype(np.float32)
    dr, ms = sample_kalman_posterior(ys, M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'], n, noise=z,
                                     return_mean=True)
    assert dr.shape == (K, n, T, D) and ms.shape == (K, T, D)
    check_parity('multicam golden T=2000 K=4 D=3 O=4 draws=16 A=I', 'multicam', M, np.swapaxes(ys, 0, 1), var,
                 np.transpose(dr, (1, 2, 0, 3)), np.swapaxes(ms, 0, 1), z, np.arange(K))


@pytest.mark.parametrize('unit', [True, False])
def test_diagonal_model_down_the_general_path(unit):
    """flags = 0 on a D = O = 2 diagonal model (Kp = 20 at T = 2000: 20 ceil(500 / 64) = 160 units -> wave, 4-frame
    chunks): ms is hip_ops.smooth's on the scalar-chain path within 1e-5; on a 12-frame session both paths have the
    law of dense_joint_posterior although their noise mappings differ (W = 4 against W = 2 normals per frame)."""
    from eks_amd import _lib, hip_ops
    diag_flags = _lib.FLAG_DIAG_MODEL | (_lib.FLAG_UNIT_AC if unit else 0)
    T, K, D = 2000, 4, 2
    pb = make_chains(T, K, D, 2.0, unit, seed=31)
    y, var = pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D)
    z = np.random.default_rng(7).normal(size=(4, T, K, 2 * D)).astype(np.float32)
    dr, ms = gpu_sample(pb['par'], y, var, z)
    assert np.isfinite(dr).all()
    ms_s, _ = hip_ops.smooth(_dev(y), _dev(var), *(_dev(pb['par'][k]) for k in PARAMS), flags=diag_flags, vs_diag=True)
    ms_s = ms_s.cpu().numpy()
    ms_err = float((np.abs(ms - ms_s) / np.abs(ms_s).max(axis=0)).max())
    print(f'diagonal model, general path against eks_smooth on scalar chains, unit={unit}: ms {ms_err:.3g}')
    assert ms_err < 1e-5
    # the exact law of both paths
    T = 12
    pb = make_chains(T, 3, D, 1.7, unit, seed=11, spikes=False)
    pb['var'][5, 1] = 1000.0
    M, K = pb['par'], 3
    y, var = pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D)
    zg, zs = unit_noise(T, K, 2 * D), unit_noise(T, K, D)
    drg, _ = gpu_sample(M, y, var, zg)
    drs, _ = gpu_sample(M, y, var, zs, flags=diag_flags)
    _, _, dev32 = ref.dense_durbin_koopman(y, var, *(M[k] for k in PARAMS), zg, storage=np.float32)
    e32s = ref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], zs.reshape(-1, T, K * D))
    eg, es = drg.astype(np.float64) - drg[:1], drs.astype(np.float64) - drs[:1]
    worst_g, worst32 = dense_law_error(eg, var, M), dense_law_error(dev32, var, M)
    worst_s, worst32s = dense_law_error(es, var, M), dense_law_error(e32s.reshape(-1, T, K, D), var, M)
    bar, bar_s = max(1e-5, 4 * worst32), max(1e-5, 4 * worst32s)
    print(f'law, diagonal model unit={unit}: general path {worst_g:.3g}, float32-storage transcription {worst32:.3g}, '
          f'bar {bar:.3g}; scalar chains {worst_s:.3g}, float32 transcription {worst32s:.3g}, bar {bar_s:.3g}')
    assert worst_g < bar and worst_s < bar_s
    # and so of each other: the implied covariances agree entry by entry
    for k in range(K):
        Lg, Ls = eg[1:, :, k].reshape(-1, T * D).T, es[1:, :, k].reshape(-1, T * D).T
        Sg, Ss = Lg @ Lg.T, Ls @ Ls.T
        sd = np.sqrt(np.diag(Ss))
        assert np.abs((Sg - Ss) / np.outer(sd, sd)).max() < bar + bar_s
