"""GPU: eks_sample through the C ABI wrappers (eks_amd.hip_ops) and through eks_amd.posterior, against the float64
reference of tests/sampling_ref.py.

Float32 bars as in tests/test_sampling_cpu.py: max(1e-5, 4 x the float32 transcription's worst error on the same
inputs), on the deviations relative to the posterior standard deviation, beyond the rounding of the float32 output
they are read from (dev_error).  Statistical bars: six standard errors, the standard error taken from the float64
reference sampler run with 32 other seeds on the same inputs; the reference with a 33rd seed has to pass first.
Nothing is compared with the kernels' own output except where two calls have to agree bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as ref  # noqa: E402
from test_sampling_cpu import dense_model, dev_error, make_chains, unit_noise  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _flags(pb):
    from eks_amd import _lib
    return _lib.FLAG_DIAG_MODEL | (_lib.FLAG_UNIT_AC if pb['unit'] else 0)


def gpu_sample(pb, n_draws, noise=None, seed=0, want_mean=True, kp=None, first_keypoint=0, first_draw=0):
    """hip_ops.sample on the chains of make_chains (keypoints kp = slice, optional).  Returns draws (S, T, N), ms (T, N)."""
    from eks_amd import hip_ops
    T, K, D = pb['T'], pb['K'], pb['D']
    sl = slice(0, K) if kp is None else kp
    par = pb['par']
    y = _dev(pb['y'].reshape(T, K, D)[:, sl])
    var = _dev(pb['var'].reshape(T, K, D)[:, sl])
    Kc = y.shape[1]
    nz = None if noise is None else _dev(np.asarray(noise, np.float32).reshape(n_draws, T, Kc, D))
    dr, ms = hip_ops.sample(y, var, *(_dev(par[k][sl]) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')), n_draws, seed=seed,
                            flags=_flags(pb), first_keypoint=first_keypoint, first_draw=first_draw, noise=nz,
                            want_mean=want_mean)
    torch.cuda.synchronize()
    return dr.cpu().numpy().reshape(n_draws, T, Kc * D), None if ms is None else ms.cpu().numpy().reshape(T, Kc * D)


def ref_chain(pb):
    mf, Pf, ms, Vs, G = ref.scalar_filter_smoother(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    return Pf, ms, Vs, G


@pytest.mark.parametrize('unit', [True, False])
def test_exact_law_on_a_short_session_scalar_chains(unit):
    from eks_amd import hip_ops
    pb = make_chains(12, 3, 2, 1.7, unit, seed=11, spikes=False)
    pb['var'][5, 1] = 1000.0
    T, K, D, N = pb['T'], pb['K'], pb['D'], pb['N']
    W = hip_ops.sample_noise_width(D, D, _flags(pb))
    assert W == D
    z = unit_noise(T, K, W)
    dr, ms = gpu_sample(pb, z.shape[0], noise=z)
    Pf, ms64, Vs64, _ = ref_chain(pb)
    assert np.array_equal(dr[0], ms)
    e32 = ref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z.reshape(-1, T, N))
    worst = worst32 = 0.0
    for n in range(N):
        S = ref.dense_joint_posterior(pb['var'][:, n:n + 1], [[pb['S0d'][n]]], np.array([[pb['a'][n]]]),
                                      np.array([[pb['c'][n]]]), np.array([[pb['qs'][n]]]), 1.0)
        cols = [1 + t * D + n % D for t in range(T)]
        worst = max(worst, ref.law_error((dr[cols, :, n] - dr[0, :, n]).T.astype(np.float64), S))
        worst32 = max(worst32, ref.law_error(e32[cols, :, n].T.astype(np.float64), S))
    bar = max(1e-5, 4 * worst32)
    print(f'law, scalar chains unit={unit}: kernels {worst:.3g}, float32 transcription {worst32:.3g}, bar {bar:.3g}')
    assert worst < bar


@pytest.mark.parametrize('D,O', [(3, 4), (5, 6)])
def test_exact_law_on_a_short_session_dense_models(D, O):
    """Durbin-Koopman path through eks_amd.posterior.  The bar is the project's 1e-5 as it stands (measured on the
    MI355X: 2.1e-7 at D = 3, O = 4 and 2.6e-7 at D = 5, O = 6); the float32-storage transcription of this path
    (ref.dense_durbin_koopman) sets the bars of tests/test_gpu_sampling_dense.py."""
    from eks_amd import hip_ops
    from eks_amd.posterior import sample_kalman_posterior
    T, K = 12, 3
    M = dense_model(K, D, O, seed=D)
    rng = np.random.default_rng(1)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O))).astype(np.float32)
    var[5, 1, 2] = 1000.0
    ys = rng.normal(size=(K, T, O)).astype(np.float32)
    W = hip_ops.sample_noise_width(D, O, 0)
    assert W == D + O
    z = unit_noise(T, K, W)
    dr, ms = sample_kalman_posterior(ys, M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'], z.shape[0], noise=z,
                                     return_mean=True)
    assert dr.shape == (K, z.shape[0], T, D) and dr.dtype == np.float32
    assert np.abs(dr[:, 0] - ms).max() <= 1e-5 * np.abs(ms).max()          # z = 0 returns the smoothed mean
    worst, bar = 0.0, 1e-5                                                # the project's bar for ms / Vs
    for k in range(K):
        S = ref.dense_joint_posterior(var[:, k], M['S0'][k], M['A'][k], M['C'][k], M['Q'][k], M['s'][k])
        Lm = (dr[k, 1:] - dr[k, :1]).reshape(T * W, T * D).T.astype(np.float64)
        worst = max(worst, ref.law_error(Lm, S))
    print(f'law, dense D={D} O={O}: kernels {worst:.3g}, bar {bar:.3g}')
    assert worst < bar


@pytest.mark.parametrize('T,K,unit,sval', [(20000, 64, True, 2.0), (20000, 8, False, 300.0), (4000, 64, False, 0.01)])
def test_same_noise_parity_with_the_float64_reference_at_size(T, K, unit, sval):
    from eks_amd import hip_ops
    S = 8
    pb = make_chains(T, K, 2, sval, unit, seed=K + T)
    z = np.random.default_rng(9).normal(size=(S, T, pb['N'])).astype(np.float32)
    dr, ms = gpu_sample(pb, S, noise=z)
    Pf, ms64, Vs64, _ = ref_chain(pb)
    sd = np.sqrt(Vs64)
    e64 = ref.scalar_deviations(Pf, pb['a'], pb['qs'], z)
    e32 = ref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z)
    trans = float(np.abs((e32 - e64) / sd).max())
    bar = max(1e-5, 4 * trans)
    err = dev_error(dr - ms[None], e64, dr, sd)
    # the raw figure, under the issue's rule with the transcription read through the same float32 output
    raw = float(np.abs((dr - ms[None] - e64) / sd).max())
    trans_out = float(np.abs((ref.read_through_f32_output(ms64, e32) - e64) / sd).max())
    bar_raw = max(1e-5, 4 * trans_out)
    print(f'parity T={T} K={K} unit={unit} s={sval}: kernels {err:.3g} beyond the output rounding, float32 '
          f'transcription {trans:.3g}, bar {bar:.3g}; raw {raw:.3g}, transcription through the float32 output '
          f'{trans_out:.3g}, bar {bar_raw:.3g}')
    assert err < bar
    assert raw < bar_raw
    # the optional ms output: the reference's means, and eks_smooth's on the same inputs, within the suite's 1e-5
    assert (np.abs(ms - ms64) / np.abs(ms64).max(axis=0)).max() < 1e-5
    par = pb['par']
    ms_s, _ = hip_ops.smooth(_dev(pb['y'].reshape(T, K, 2)), _dev(pb['var'].reshape(T, K, 2)),
                             *(_dev(par[k]) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')), flags=_flags(pb), vs_diag=True)
    ms_s = ms_s.cpu().numpy().reshape(T, -1)
    assert (np.abs(ms - ms_s) / np.abs(ms_s).max(axis=0)).max() < 1e-5


# N = K D chains against the lane mapping of chain_coords (eks_chain_plan.hpp): 2^nt_log2 = min(64, pow2ceil(N)) chains
# per wave row, so N = 1, 3, 6 put 64, 16, 8 chunks of one chain side by side in a wave (with idle lanes at N = 3, 6);
# N = 63 leaves one lane of every row idle; N = 65, 130, 195 have a ragged last tile of 1, 2, 3 chains.
EDGE_CHAINS = [(1, 1), (3, 1), (1, 3), (3, 2), (21, 3), (63, 1), (65, 1), (65, 2), (65, 3)]
# T against the 32-frame chunks and the two-level scan groups gs = ceil(sqrt(nc)): 1, 2, 3 frames; one chunk short of /
# exactly / past a chunk edge; nc = 32 -> 33 at T = 1024 -> 1025 (gs = 6, six groups, the last of two -> three chunks);
# nc = 31 = gs^2 - gs + 1 at T = 32 x 30 + 5 (the last group holds a single, partial chunk) and nc = 32 at
# T = 32 x 31 + 5 (the last group holds two chunks of six, the second partial).
EDGE_FRAMES = [1, 2, 3, 31, 32, 33, 965, 997, 1024, 1025]


@pytest.mark.parametrize('T', EDGE_FRAMES)
@pytest.mark.parametrize('K,D', EDGE_CHAINS)
def test_scalar_chain_edge_shapes_injected_noise_and_generator(K, D, T):
    """Unit and non-unit chains.  Injected normals: same-noise parity with the float64 reference under the bar rule of
    test_same_noise_parity_with_the_float64_reference_at_size.  Generator: eks_sample(seed) equals
    eks_sample(noise = eks_sample_noise(seed)) bit for bit (so the generator path shares the arithmetic held to the
    tight bar above), its normals are ref.scalar_noise's within the 1e-4 the suite allows the hardware log2 / sin / cos,
    and its draws are the reference's on ref.scalar_noise's normals within the parity bar plus what 1e-4 on every
    normal can move a deviation: e is linear in z with non-negative coefficients (G_t >= 0 for a > 0), so that is
    1e-4 e(z = 1), computed by the float64 reference.  A wrong lane, chain or counter word is an O(1) difference.
    Measured on the MI355X, worst over the 90 shapes: kernels 9.1e-7 beyond the output rounding, transcription 9.5e-7
    (bar 1e-5); ms 7.5e-7 (3.8e-7 over the shapes of 31 frames and more); generator max |dz| 3.4e-5."""
    from eks_amd import hip_ops
    S, N = 3, K * D
    for unit in (True, False):
        pb = make_chains(T, K, D, 2.0 if unit else 0.7, unit, seed=1000 * N + T)
        Pf, ms64, Vs64, _ = ref_chain(pb)
        sd = np.sqrt(Vs64)
        # scale of a chain's means: its largest |ms|, the suite's scale.  With one to three frames that can itself be a
        # cancelled value far below its operands (ms_0 = (1 - k c) m0 + k y: at K, D, T = 21, 3, 1 one chain has
        # |ms| = 1.5e-3 from operands near one), where float32 arithmetic on those operands owes no relative accuracy;
        # there, and only there, |m0| enters the scale: |k y| <= |ms_0| + |m0| bounds the operands by it.
        scale = np.abs(ms64).max(axis=0)
        if T <= 3:
            scale = np.maximum(scale, np.abs(pb['m0f']))

        def parity(dr, ms, z):
            e64 = ref.scalar_deviations(Pf, pb['a'], pb['qs'], z)
            e32 = ref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z)
            trans = float(np.abs((e32 - e64) / sd).max())
            trans_out = float(np.abs((ref.read_through_f32_output(ms64, e32) - e64) / sd).max())
            return e64, max(1e-5, 4 * trans), max(1e-5, 4 * trans_out), trans, trans_out

        # injected normals
        z = np.random.default_rng(N + T).normal(size=(S, T, N)).astype(np.float32)
        dr, ms = gpu_sample(pb, S, noise=z)
        assert dr.shape == (S, T, N) and np.isfinite(dr).all()
        e64, bar, bar_raw, trans, trans_out = parity(dr, ms, z)
        err = dev_error(dr - ms[None], e64, dr, sd)
        raw = float(np.abs((dr - ms[None] - e64) / sd).max())
        print(f'edge K={K} D={D} T={T} unit={unit} injected: kernels {err:.3g} beyond the output rounding, float32 '
              f'transcription {trans:.3g}, bar {bar:.3g}; raw {raw:.3g}, transcription through the float32 output '
              f'{trans_out:.3g}, bar {bar_raw:.3g}; ms {(np.abs(ms - ms64) / scale).max():.3g} (relative to the '
              f"chain's largest |ms| alone: {(np.abs(ms - ms64) / np.abs(ms64).max(axis=0)).max():.3g}), bar 1e-05")
        assert err < bar
        assert raw < bar_raw
        assert (np.abs(ms - ms64) / scale).max() < 1e-5
        # the generator
        seed = 0x5eed0000 + 977 * N + T
        gen, ms_g = gpu_sample(pb, S, seed=seed)
        assert np.array_equal(ms_g, ms)
        nz = hip_ops.sample_noise(T, K, D, D, S, seed=seed, flags=_flags(pb))
        torch.cuda.synchronize()
        nz = nz.cpu().numpy().reshape(S, T, N)
        inj, _ = gpu_sample(pb, S, noise=nz)
        assert np.array_equal(gen, inj)                                   # (T % 4 != 0 included)
        zr = ref.scalar_noise(seed, T, N, S)
        dz = float(np.abs(nz - zr).max())
        e64, bar, bar_raw, trans, trans_out = parity(gen, ms_g, zr)
        moved = 1e-4 * ref.scalar_deviations(Pf, pb['a'], pb['qs'], np.ones((1, T, N)))[0] / sd
        excess = np.maximum(np.abs(gen - ms_g[None] - e64) - 2.0 ** -24 * np.abs(gen), 0.0) / sd - moved[None]
        print(f'edge K={K} D={D} T={T} unit={unit} generator: max |dz| {dz:.3g} (bar 1e-04); error beyond the output '
              f'rounding and 1e-4 per normal {max(float(excess.max()), 0.0):.3g}, bar {bar:.3g}')
        assert dz < 1e-4
        assert excess.max() < bar


def test_generator_noise_tiling_over_keypoints_draws_and_memory_budget_are_bit_exact():
    from eks_amd import hip_ops
    from eks_amd.posterior import draws_per_group, sample_kalman_posterior
    T, K, D, S, seed = 3001, 64, 2, 16, 0xfeedface12345678
    pb = make_chains(T, K, D, 2.0, True, seed=4)
    full, ms = gpu_sample(pb, S, seed=seed)
    # eks_sample(seed) == eks_sample(noise = eks_sample_noise(seed))
    nz = hip_ops.sample_noise(T, K, D, D, S, seed=seed, flags=_flags(pb))
    torch.cuda.synchronize()
    nz_h = nz.cpu().numpy()
    inj, _ = gpu_sample(pb, S, noise=nz_h)
    assert np.array_equal(full, inj)
    # the normals are the reference's (hardware log2 / sin / cos are accurate in absolute terms; a wrong counter or
    # word order is an O(1) difference)
    zr = ref.scalar_noise(seed, T, K * D, S)
    print(f'generator against the float64 reference: max |dz| = {np.abs(nz_h.reshape(S, T, -1) - zr).max():.3g}')
    assert np.abs(nz_h.reshape(S, T, -1) - zr).max() < 1e-4
    # keypoints 16..31 of the 64-keypoint call == a 16-keypoint call with first_keypoint = 16
    part, _ = gpu_sample(pb, S, seed=seed, kp=slice(16, 32), first_keypoint=16)
    assert np.array_equal(part, full[:, :, 16 * D:32 * D])
    # draws 8..15 of 16 == an 8-draw call with first_draw = 8
    tail, _ = gpu_sample(pb, 8, seed=seed, first_draw=8)
    assert np.array_equal(tail, full[8:])
    assert not np.array_equal(full[:8], full[8:])
    # a call tiled by the memory budget == the untiled call (through eks_amd.posterior)
    par = pb['par']
    args = (np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'], par['Q'],
            pb['var'].reshape(T, K, D), par['s'], S)
    budget = 8 << 20
    assert draws_per_group(K, T, D, D, _flags(pb), S, budget) < S
    one = sample_kalman_posterior(*args, seed=seed)
    tiled = sample_kalman_posterior(*args, seed=seed, memory_budget=budget)
    assert one.shape == (K, S, T, D) and one.dtype == np.float32
    assert np.array_equal(one, tiled)
    assert np.array_equal(np.transpose(one, (1, 2, 0, 3)).reshape(S, T, K * D), full)
    other = sample_kalman_posterior(*args, seed=seed + 1)
    assert not np.array_equal(one, other)
    dev = sample_kalman_posterior(*args, seed=seed, return_device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), one)


def test_general_model_generator_seed_noise_and_slices():
    """The general path's own generator: eks_sample_noise against the float64 reference, eks_sample(seed) against
    eks_sample(noise = eks_sample_noise(seed)) bit for bit, and first_keypoint / first_draw slices.  The normals of a
    slice are the larger call's bit for bit; its draws go through a smoothing call over a different number of stacked
    chains, which may take another kernel organisation, so they are held to the project's 1e-5 instead."""
    from eks_amd import hip_ops
    T, K, D, O, S, seed = 50, 6, 3, 4, 5, 0x0123456789abcdef
    M = dense_model(K, D, O, seed=8)
    rng = np.random.default_rng(3)
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O))).astype(np.float32)
    y = rng.normal(size=(T, K, O)).astype(np.float32)
    W = D + O

    def run(kp=slice(0, K), n=S, noise=None, **kw):
        dr, _ = hip_ops.sample(_dev(y[:, kp]), _dev(var[:, kp]), *(_dev(M[k][kp]) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')),
                               n, seed=seed, noise=noise, **kw)
        torch.cuda.synchronize()
        return dr.cpu().numpy()
    nz = hip_ops.sample_noise(T, K, D, O, S, seed=seed)
    assert tuple(nz.shape) == (S, T, K, W)
    nz_h = nz.cpu().numpy()
    zr = ref.dense_noise(seed, T, K, W, S)
    print(f'general generator against the float64 reference: max |dz| = {np.abs(nz_h - zr).max():.3g}')
    assert np.abs(nz_h - zr).max() < 1e-4          # hardware log2 / sin / cos; a wrong counter word is O(1)
    full = run()
    assert np.array_equal(full, run(noise=nz))
    part_nz = hip_ops.sample_noise(T, 2, D, O, 2, seed=seed, first_keypoint=3, first_draw=2).cpu().numpy()
    assert np.array_equal(part_nz, nz_h[2:4, :, 3:5])
    part = run(kp=slice(3, 5), n=2, first_keypoint=3, first_draw=2)
    assert np.abs(part - full[2:4, :, 3:5]).max() <= 1e-5 * np.abs(full).max()
    assert not np.array_equal(full[0], full[1])


def pooled_moments(e, sd, G, Vs):
    """per chain, pooled over frames and draws: mean (e / sd)^2 - 1 and the lag-one sum of e_t e_{t+1} / (sd_t sd_{t+1})
    minus its expectation sum_t G_t sqrt(Vs_{t+1} / Vs_t), per frame."""
    u = e / sd
    m2 = (u * u).mean(axis=(0, 1)) - 1.0
    lag = (u[:, :-1] * u[:, 1:]).mean(axis=0).sum(axis=0) - (G[:-1] * np.sqrt(Vs[1:] / Vs[:-1])).sum(axis=0)
    return np.stack([m2, lag / (e.shape[1] - 1)])


def test_moments_at_size_with_the_generator():
    T, K, S = 6000, 64, 8
    pb = make_chains(T, K, 2, 2.0, True, seed=21, spikes=False)
    hit = np.random.default_rng(2).random(pb['var'].shape)
    pb['var'][hit < 0.02] = 1000.0
    Pf, ms64, Vs64, G = ref_chain(pb)
    sd = np.sqrt(Vs64)
    refs = np.stack([pooled_moments(ref.scalar_deviations(Pf, pb['a'], pb['qs'], ref.scalar_noise(1000 + i, T, pb['N'], S)),
                                    sd, G, Vs64) for i in range(33)])
    se = refs[:32].std(axis=0, ddof=1)
    assert np.all(np.abs(refs[32]) < 6 * se)                      # the reference with a 33rd seed passes its own bar
    dr, ms = gpu_sample(pb, S, seed=77)
    got = pooled_moments(dr.astype(np.float64) - ms[None], sd, G, Vs64)
    print(f'moments: worst |stat| / se = {np.abs(got / se).max():.2f} (reference, 33rd seed: {np.abs(refs[32] / se).max():.2f})')
    assert np.all(np.abs(got) < 6 * se)


def test_sample_singlecam_on_the_golden_markers(golden_dir):
    from eks_amd.marker_array import MarkerArray
    from eks_amd.posterior import sample_singlecam
    from eks_amd.singlecam_smoother import ensemble_kalman_smoother_singlecam
    from oracle import eks_oracle as orc
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers']
    names = [str(k) for k in g['keypoints']]
    M_, V, T, K, _ = mk.shape
    ma = MarkerArray(mk.astype(np.float64), data_fields=['x', 'y', 'likelihood'])
    df, s = ensemble_kalman_smoother_singlecam(ma, names, smooth_param=10.0)
    S = 256
    dr = sample_singlecam(ma, names, s, S, seed=5)
    assert dr.shape == (S, T, K, 2) and dr.dtype == np.float32
    assert np.array_equal(dr, sample_singlecam(ma, names, s, S, seed=5))
    assert not np.array_equal(dr, sample_singlecam(ma, names, s, S, seed=6))
    tab = df.to_numpy().reshape(T, K, 9)
    mean_col, var_col = tab[:, :, 0:2].reshape(T, K * 2), tab[:, :, 7:9].reshape(T, K * 2)
    # the same chains for the reference sampler: standard errors of the pooled statistics from 32 other seeds
    arrs = orc.singlecam_arrays(mk)
    var = arrs['ensemble_vars'].reshape(T, K * 2).astype(np.float32)
    S0d = np.diagonal(arrs['S0s'], axis1=1, axis2=2).reshape(-1)
    one = np.ones(K * 2)
    _, Pf, _, Vs64, G = ref.scalar_filter_smoother(np.zeros_like(var), var, 0 * one, S0d, one, one, 10.0 * one)
    assert np.abs(var_col / Vs64 - 1).max() < 1e-4               # the driver's posterior variances are these chains'

    def stats(e):
        u = e / np.sqrt(Vs64)
        return np.stack([u.mean(axis=(0, 1)), (u * u).mean(axis=(0, 1)) - 1.0])
    refs = np.stack([stats(ref.scalar_deviations(Pf, one, 10.0 * one, ref.scalar_noise(500 + i, T, K * 2, S)))
                     for i in range(33)])
    se = refs[:32].std(axis=0, ddof=1)
    assert np.all(np.abs(refs[32]) < 6 * se)
    got = stats(dr.reshape(S, T, K * 2).astype(np.float64) - mean_col[None])
    print(f'sample_singlecam: worst |stat| / se = {np.abs(got / se).max():.2f}')
    assert np.all(np.abs(got) < 6 * se)


def test_sample_abi_refuses_what_it_documents_without_launching():
    """Through the library, with real device buffers: every refusal below is returned by a guard that runs before the
    first launch (eks_api.hip: eks_sample, eks_sample_noise; eks_sample_dense.hip: dense_sample checks D, O, then
    (n_draws + 1) K D, then the workspace)."""
    import ctypes
    from eks_amd import _lib
    lib = _lib.load()
    f32 = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    f64 = torch.zeros(1 << 16, dtype=torch.float64, device='cuda')
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    par = [p(f64)] * 6

    def sample(d, n_draws, draws, ws_bytes):
        return lib.eks_sample(ctypes.byref(d), p(f32), p(f32), *par, n_draws, 0, 0, 0, None, None, draws, p(ws),
                              ws_bytes, None)
    diag = _lib.EksDims(4, 100, 2, 2, _lib.FLAG_DIAG_MODEL)                   # K, T, D, O, flags
    gen = _lib.EksDims(4, 100, 3, 4, 0)
    for d in (diag, gen):
        need = lib.eks_sample_workspace_bytes(ctypes.byref(d), 2)
        assert 0 < need <= ws.numel()
        rc = sample(d, 2, p(f32), need - 1)                                   # one byte short
        assert rc == -4 and b'workspace' in lib.eks_status_string(rc)
        assert sample(d, 2, None, need) == -1                                 # null draws
        assert sample(d, 0, p(f32), need) == -2                               # n_draws < 1
    d7 = _lib.EksDims(4, 100, 7, 7, 0)
    rc = sample(d7, 2, p(f32), ws.numel())
    assert rc == -3 and b'unsupported' in lib.eks_status_string(rc)           # D = 7 on a general model
    assert sample(_lib.EksDims(4, 100, 3, 65, 0), 2, p(f32), ws.numel()) == -3    # O = 65
    # (n_draws + 1) K D = 8 x 2^20 x 3 > 2^24 (K D itself passes check_dims); the workspace named is too small for any
    # launch of that shape as well
    wide = _lib.EksDims(1 << 20, 4, 3, 4, 0)
    assert lib.eks_smooth_workspace_bytes(ctypes.byref(wide)) > 0
    rc = sample(wide, 7, p(f32), 16)
    assert rc == -2 and b'shape' in lib.eks_status_string(rc)
    assert sample(wide, 0x7fffffff, p(f32), 16) == -2                         # n_draws + 1 does not wrap
    # eks_sample_workspace_bytes is 0 for what eks_sample refuses
    for d, n in ((d7, 2), (_lib.EksDims(4, 100, 3, 65, 0), 2), (wide, 7), (wide, 0x7fffffff), (gen, 0), (diag, 0),
                 (_lib.EksDims(4, 100, 2, 3, _lib.FLAG_DIAG_MODEL), 2), (_lib.EksDims(4, 0, 3, 4, 0), 2)):
        assert lib.eks_sample_workspace_bytes(ctypes.byref(d), n) == 0
    assert lib.eks_sample_workspace_bytes(ctypes.byref(wide), 4) > 0          # 5 x 2^20 x 3 <= 2^24 is accepted
    # eks_sample_noise: W = D + O > 70 is a shape error; a refused model within 70 normals stays "unsupported"
    assert lib.eks_sample_noise(ctypes.byref(_lib.EksDims(4, 100, 7, 64, 0)), 2, 0, 0, 0, p(f32), None) == -2
    assert lib.eks_sample_noise(ctypes.byref(_lib.EksDims(4, 100, 3, 68, 0)), 2, 0, 0, 0, p(f32), None) == -2
    assert lib.eks_sample_noise(ctypes.byref(d7), 2, 0, 0, 0, p(f32), None) == -3
    assert lib.eks_sample_noise(ctypes.byref(gen), 2, 0, 0, 0, None, None) == -1
    torch.cuda.synchronize()                                                  # nothing was enqueued, nothing faulted
