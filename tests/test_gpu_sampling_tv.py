"""GPU: eks_sample_tv through the C ABI wrappers (eks_amd.hip_ops) and through eks_amd.posterior, against the float64
reference of tests/sampling_tv_ref.py.

Float32 bars as in tests/test_gpu_sampling.py: max(1e-5, 4 x the float32 transcription's worst error on the same
inputs), on the deviations relative to the posterior standard deviation, beyond the rounding of the float32 output
they are read from (dev_error), and the raw figure against the transcription read through the same output.  The
transcription (tvref.scalar_deviations_f32) carries w and lam; no constant here was tuned on the device.  General
models: the float64 Durbin-Koopman transcription with float32 stores, as tests/test_gpu_sampling_dense.py.  Two float32
forms of the same means (the sampler's ms and a smoother's) are each inside the float32 bar of the float64 reference,
so they are held to twice that bar against each other.  Bit contracts compare two runs of the same kernels and are
exact.  Statistical condition of the drivers: the mean of 256 draws within 6 posterior sd / sqrt(256) of the driver's
smoothed value on every frame - the float64 reference on the generator's own normals has to satisfy it first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as ref  # noqa: E402
import sampling_tv_ref as tvref  # noqa: E402
import smooth_tv_ref as stv  # noqa: E402
from test_sampling_cpu import dense_model, dev_error, make_chains  # noqa: E402
from test_sampling_tv_cpu import make_planes, ms_error_and_bar, reference, set_ac  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _flags(pb):
    from eks_amd import _lib
    return _lib.FLAG_DIAG_MODEL | (_lib.FLAG_UNIT_AC if pb['unit'] else 0)


def gpu_sample_tv(pb, n_draws, w=None, lam=None, noise=None, seed=0, kp=None, first_keypoint=0, first_draw=0):
    """hip_ops.sample_tv on the chains of make_chains (keypoints kp = slice, optional).  w (T,) or (T, K); lam (T, K D).
    Returns draws (S, T, N), ms (T, N)."""
    from eks_amd import hip_ops
    T, K, D = pb['T'], pb['K'], pb['D']
    sl = slice(0, K) if kp is None else kp
    par = pb['par']
    y = _dev(pb['y'].reshape(T, K, D)[:, sl])
    var = _dev(pb['var'].reshape(T, K, D)[:, sl])
    Kc = y.shape[1]
    nz = None if noise is None else _dev(np.asarray(noise, np.float32).reshape(n_draws, T, Kc, D))
    wq = None if w is None else _dev(w if np.ndim(w) == 1 else w[:, sl])
    lm = None if lam is None else _dev(np.asarray(lam, np.float32).reshape(T, K, D)[:, sl])
    dr, ms = hip_ops.sample_tv(y, var, *(_dev(par[k][sl]) for k in PARAMS), n_draws, qscale=wq, weights=lm, seed=seed,
                               flags=_flags(pb), first_keypoint=first_keypoint, first_draw=first_draw, noise=nz,
                               want_mean=True)
    torch.cuda.synchronize()
    return dr.cpu().numpy().reshape(n_draws, T, Kc * D), ms.cpu().numpy().reshape(T, Kc * D)


def edge_chains(T, K, D, unit, seed):
    """make_chains with a = 0.98, c = -1.3 on the non-unit form, one frame at var = 1e30 and (N >= 3) one chain with
    s q = 0."""
    pb = make_chains(T, K, D, 2.0 if unit else 0.7, unit, seed=seed)
    if not unit:
        set_ac(pb, 0.98, -1.3)
    pb['var'][T // 2, 0] = 1e30
    if pb['N'] >= 3:
        pb['par']['Q'][K - 1, D - 1, D - 1] = 0.0
        pb['qs'][-1] = 0.0
    return pb


# T against the 32-frame chunks and the two-level scan groups gs = ceil(sqrt(nc)), as tests/test_gpu_sampling.py: 1, 2,
# 3 frames, a chunk edge, two chunks and a frame, and nc = 33 at T = 1025 (gs = 6, six groups, the last of three chunks)
EDGE_FRAMES = [1, 2, 3, 31, 32, 33, 65, 1025]
EDGE_CHAINS = [(1, 1), (3, 1), (3, 2), (21, 3), (65, 1), (65, 2)]          # N = K D = 1, 3, 6, 63, 65, 130
PLANES = [('shared', True), ('per_keypoint', False), ('per_keypoint', True), (None, True), ('shared', False)]


@pytest.mark.parametrize('T', EDGE_FRAMES)
@pytest.mark.parametrize('K,D', EDGE_CHAINS)
def test_scalar_chain_edge_shapes_planes_injected_noise_and_generator(K, D, T):
    """Measured on the MI355X: see DESIGN.md 9r."""
    from eks_amd import hip_ops
    S, N = 3, K * D
    worst = dict(err=0.0, trans=0.0, ms=0.0)
    for unit in (True, False):
        pb = edge_chains(T, K, D, unit, seed=1000 * N + T)
        z = np.random.default_rng(N + T).normal(size=(S, T, N)).astype(np.float32)
        for qform, has_w in PLANES:
            w, lam = make_planes(T, K, D, seed=N + T, per_keypoint=qform == 'per_keypoint')
            w = None if qform is None else w
            lam = lam if has_w else None
            ms64, sd, e64, bar, bar_raw, trans = reference(pb, z, w, lam)
            dr, ms = gpu_sample_tv(pb, S, w, lam, noise=z)
            assert dr.shape == (S, T, N) and np.isfinite(dr).all()
            err = dev_error(dr - ms[None], e64, dr, sd)
            raw = float(np.abs((dr - ms[None] - e64) / sd).max())
            ms_err, bar_ms = ms_error_and_bar(pb, ms, ms64, w, lam)
            print(f'edge K={K} D={D} T={T} unit={unit} qscale={qform} weights={has_w}: kernels {err:.3g} beyond the '
                  f'output rounding, float32 transcription {trans:.3g}, bar {bar:.3g}; raw {raw:.3g}, bar {bar_raw:.3g}; '
                  f'ms {ms_err:.3g}, bar {bar_ms:.3g}')
            assert err < bar
            assert raw < bar_raw
            assert ms_err < bar_ms
            worst = dict(err=max(worst['err'], err), trans=max(worst['trans'], trans), ms=max(worst['ms'], ms_err))
        # the generator under the last planes: eks_sample_tv(seed) == eks_sample_tv(noise = eks_sample_noise(seed))
        seed = 0x5eed0000 + 977 * N + T
        gen, ms_g = gpu_sample_tv(pb, S, w, lam, seed=seed)
        nz = hip_ops.sample_noise(T, K, D, D, S, seed=seed, flags=_flags(pb))
        torch.cuda.synchronize()
        inj, ms_i = gpu_sample_tv(pb, S, w, lam, noise=nz.cpu().numpy().reshape(S, T, N))
        assert np.array_equal(gen, inj) and np.array_equal(ms_g, ms_i)
    print(f'edge K={K} D={D} T={T} worst: kernels {worst["err"]:.3g}, transcription {worst["trans"]:.3g}, ms {worst["ms"]:.3g}')


def test_the_kernels_own_law_on_a_short_session():
    """T = 40 (a full chunk and a partial one), 40 one-hot draws: column t of L is draw t minus ms.  L L' against the
    float64 joint posterior covariance relative to its diagonal; the bar is the float32 transcription's own error on
    the same case times 4, floored at 1e-5."""
    T, K, D = 40, 3, 2
    worst = {}
    for unit in (True, False):
        pb = make_chains(T, K, D, 1.7, unit, seed=11, spikes=False)
        if not unit:
            set_ac(pb, 0.98, -1.3)
        pb['var'][5, 1] = 1000.0
        N = pb['N']
        w, lam = make_planes(T, K, D, seed=3, per_keypoint=True)
        z = np.broadcast_to(np.eye(T, dtype=np.float32)[:, :, None], (T, T, N)).copy()
        dr, ms = gpu_sample_tv(pb, T, w, lam, noise=z)
        e32 = tvref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z, w, lam, D)
        got = got32 = 0.0
        for n in range(N):
            S_ = tvref.joint_covariance(tvref.r_eff(pb['var'][:, n:n + 1], lam[:, n:n + 1]), pb['S0d'][n], pb['a'][n],
                                        pb['c'][n], 1.0, pb['qs'][n], np.concatenate([[1.0], w[1:, n // D]]))
            got = max(got, ref.law_error((dr[:, :, n] - ms[None, :, n]).T.astype(np.float64), S_))
            got32 = max(got32, ref.law_error(e32[:, :, n].T.astype(np.float64), S_))
        bar = max(1e-5, 4 * got32)
        print(f'law of the kernels, unit={unit}: {got:.3g}, float32 transcription {got32:.3g}, bar {bar:.3g}')
        assert got < bar
        worst[unit] = got


def test_bit_contracts_subsets_reused_workspace_nan_row_zero_and_zero_noise():
    from eks_amd import hip_ops
    T, K, D, S, seed = 200, 70, 2, 8, 0xfeedface12345678
    pb = make_chains(T, K, D, 2.0, True, seed=4)
    w, lam = make_planes(T, K, D, seed=9, per_keypoint=True)
    full, ms = gpu_sample_tv(pb, S, w, lam, seed=seed)
    # keypoints [3, 67) of 70 (N = 128: two full tiles where the full call has three, the last ragged) and draws [2, 5)
    part, ms_p = gpu_sample_tv(pb, 3, w, lam, seed=seed, kp=slice(3, 67), first_keypoint=3, first_draw=2)
    assert np.array_equal(part, full[2:5, :, 3 * D:67 * D]) and np.array_equal(ms_p, ms[:, 3 * D:67 * D])
    assert not np.array_equal(full[0], full[1])
    # a NaN in row 0 of qscale changes no bit (make_planes puts one there); neither does a 1
    w1 = w.copy()
    w1[0] = 1.0
    again, ms_a = gpu_sample_tv(pb, S, w1, lam, seed=seed)
    assert np.isnan(w[0]).all() and np.array_equal(again, full) and np.array_equal(ms_a, ms)
    # all-zero noise gives draws == ms
    zero, ms_z = gpu_sample_tv(pb, 2, w, lam, noise=np.zeros((2, T, K * D), np.float32))
    assert np.array_equal(zero, np.broadcast_to(ms_z, zero.shape)) and np.array_equal(ms_z, ms)
    # two calls on ONE workspace, the second after another shape has used it
    import ctypes
    from eks_amd import _lib
    lib = _lib.load()
    par = pb['par']
    bufs = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)), _dev(w), _dev(lam.reshape(T, K, D))] + \
        [_dev(par[k]) for k in PARAMS]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    d = _lib.EksDims(K, T, D, D, _flags(pb) | _lib.FLAG_VS_DIAG)
    small = _lib.EksDims(5, 77, D, D, _flags(pb) | _lib.FLAG_VS_DIAG)
    need = lib.eks_sample_tv_workspace_bytes(ctypes.byref(d), S)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device='cuda')
    outs = []
    for dims in (d, small, d):
        out = torch.empty((S, T, K, D), dtype=torch.float32, device='cuda')
        rc = lib.eks_sample_tv(ctypes.byref(dims), p(bufs[0]), p(bufs[1]), p(bufs[2]), 1, p(bufs[3]), *[p(b) for b in bufs[4:]],
                               S, seed, 0, 0, None, None, p(out), p(ws), need, hip_ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy().reshape(S, T, K * D))
    assert np.array_equal(outs[0], full) and np.array_equal(outs[2], full)


@pytest.mark.parametrize('unit', [True, False])
def test_without_planes_the_draws_are_eks_samples(unit):
    from eks_amd import hip_ops
    T, K, D, S = 1025, 21, 3, 4
    pb = edge_chains(T, K, D, unit, seed=77)
    z = np.random.default_rng(1).normal(size=(S, T, pb['N'])).astype(np.float32)
    ms64, sd, e64, bar, bar_raw, trans = reference(pb, z, None, None)
    dr, ms = gpu_sample_tv(pb, S, noise=z)
    par = pb['par']
    dr_s, ms_s = hip_ops.sample(_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)),
                                *(_dev(par[k]) for k in PARAMS), S, flags=_flags(pb), noise=_dev(z.reshape(S, T, K, D)),
                                want_mean=True)
    torch.cuda.synchronize()
    dr_s, ms_s = dr_s.cpu().numpy().reshape(S, T, -1), ms_s.cpu().numpy().reshape(T, -1)
    same = np.array_equal(dr, dr_s) and np.array_equal(ms, ms_s)
    gap = dev_error(dr - ms[None], (dr_s - ms_s[None]).astype(np.float64), 2 * np.abs(dr), sd)
    ms_gap, bar_ms = ms_error_and_bar(pb, ms, ms_s.astype(np.float64), None, None)
    _, bar_ms = ms_error_and_bar(pb, ms, ms64, None, None)   # each form is inside it, so the two differ by at most twice it
    print(f'eks_sample_tv(NULL, NULL) against eks_sample, unit={unit}: bit-identical {same}; deviations differ by '
          f'{gap:.3g} of sd beyond the output rounding (bar {bar:.3g}), ms by {ms_gap:.3g} (bar {2 * bar_ms:.3g})')
    assert gap < bar and ms_gap < 2 * bar_ms
    assert dev_error(dr - ms[None], e64, dr, sd) < bar


def test_ms_is_the_smoothers_under_the_same_planes():
    """ms against eks_smooth_tv under (var, qscale) and against eks_smooth_heavy's last pass under the planes it returns:
    each is inside the float32 bar of the float64 reference (smooth_tv_ref.f32_bars), so the two differ by at most twice it."""
    from eks_amd import hip_ops
    T, K, D = 1025, 21, 2
    for unit in (True, False):
        pb = edge_chains(T, K, D, unit, seed=5)
        par = pb['par']
        y3, v3 = pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D)
        model = [_dev(par[k]) for k in PARAMS]
        w, _ = make_planes(T, K, D, seed=6, per_keypoint=True)
        ms_tv, _ = hip_ops.smooth_tv(_dev(y3), _dev(v3), _dev(w), *model, flags=_flags(pb), vs_diag=True)
        ms_h, _, lam_h, w_h, _ = hip_ops.smooth_heavy(_dev(y3), _dev(v3), *model, nu_obs=4.0, nu_proc=4.0, n_iters=4,
                                                      flags=_flags(pb), vs_diag=True)
        torch.cuda.synchronize()
        lam_h, w_h = lam_h.cpu().numpy().reshape(T, K * D), w_h.cpu().numpy()
        for label, ms_ref, wq, lam in (('eks_smooth_tv', ms_tv, w, None), ('eks_smooth_heavy', ms_h, w_h, lam_h)):
            _, ms = gpu_sample_tv(pb, 1, wq, lam, noise=np.zeros((1, T, K * D), np.float32))
            ms_ref = ms_ref.cpu().numpy().reshape(T, K * D)
            r32 = tvref.r_eff(pb['var'], lam, np.float32)
            _, _, ms64, Vs64, _ = tvref.scalar_filter_smoother(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'],
                                                               pb['qs'], wq, lam, D)
            t_ms, t_Vs = stv.scalar_smooth_tv_f32(pb['y'], r32, pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'],
                                                  np.where(np.isnan(wq), 1.0, wq), D, unit)
            bar = stv.f32_bars(t_ms, t_Vs, ms64, Vs64, pb['y'])['ms']
            e_ref = float(stv.f32_errors(ms, Vs64, ms64, Vs64, pb['y'])['ms'].max())
            gap = float((np.abs(ms.astype(np.float64) - ms_ref) / np.abs(pb['y'].astype(np.float64)).max(axis=0)).max())
            print(f'ms against {label}, unit={unit}: bit-identical {np.array_equal(ms, ms_ref)}, gap {gap:.3g} (bar '
                  f'{2 * bar:.3g}); against the float64 reference {e_ref:.3g} (bar {bar:.3g})')
            assert e_ref < bar and gap < 2 * bar


# ---- general models ----------------------------------------------------------------------------------------------------
def dense_case(D, O, K, T, seed, singular_q=False, unit_root=False):
    from test_gpu_sampling_dense import session, stable_model
    from test_sampling_cpu import drop_one_direction
    M = stable_model(K, D, O, seed, unit_root=unit_root)
    if singular_q and D > 1:
        M = drop_one_direction(M, ('Q',), seed)
    y, var = session(M, T, O, seed)
    rng = np.random.default_rng(seed + 1)
    w = np.exp(rng.uniform(np.log(0.2), np.log(5.0), (T, K))).astype(np.float32)
    w[rng.random((T, K)) < 0.05] = 1e3
    w[rng.random((T, K)) < 0.05] = 1e-3
    w[0] = np.nan
    lam = rng.uniform(0.05, 1.25, (T, K, O)).astype(np.float32)
    lam[rng.random((T, K, O)) < 0.03] = 1e-30
    return M, y, var, w, lam


def check_dense(label, M, y, var, w, lam, S=3, seed=0):
    from eks_amd import hip_ops
    T, K, O = y.shape
    D = M['m0'].shape[1]
    z = np.random.default_rng(seed + 2).normal(size=(S, T, K, D + O)).astype(np.float32)
    dr, ms = hip_ops.sample_tv(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), S, qscale=_dev(w), weights=_dev(lam),
                               noise=_dev(z), want_mean=True)
    torch.cuda.synchronize()
    dr, ms = dr.cpu().numpy().astype(np.float64), ms.cpu().numpy().astype(np.float64)
    assert np.isfinite(dr).all() and np.isfinite(ms).all()
    args = (y, var, *(M[k] for k in PARAMS), z, w, lam)
    ms64, Vs, dev64 = tvref.dense_durbin_koopman(*args)
    ms32, _, dev32 = tvref.dense_durbin_koopman(*args, storage=np.float32, round_output=False)
    sd = np.sqrt(np.diagonal(Vs, axis1=-2, axis2=-1))
    trans = float(np.abs((dev32 - dev64) / sd).max())
    bar = max(1e-5, 4 * trans)
    err = dev_error(dr - ms[None], dev64, dr, sd)
    raw = float(np.abs((dr - ms[None] - dev64) / sd).max())
    through = (ms32[None] + dev32).astype(np.float32).astype(np.float64) - ms32[None]
    bar_raw = max(1e-5, 4 * float(np.abs((through - dev64) / sd).max()))
    ms_err = float((np.abs(ms - ms64) / np.abs(ms64).max(axis=0)).max())
    print(f'general {label}: kernels {err:.3g} beyond the output rounding, float32-storage transcription {trans:.3g}, bar '
          f'{bar:.3g}; raw {raw:.3g}, bar {bar_raw:.3g}; ms {ms_err:.3g}, bar 1e-05')
    assert err < bar
    assert raw < bar_raw
    assert ms_err < 1e-5


@pytest.mark.parametrize('T', [2, 17, 70])
@pytest.mark.parametrize('K', [1, 5])
@pytest.mark.parametrize('D,O', [(1, 1), (2, 4), (3, 4), (6, 8)])
def test_general_models_injected_noise_against_the_float64_reference(D, O, K, T):
    M, y, var, w, lam = dense_case(D, O, K, T, seed=10 * D + O + K + T)
    check_dense(f'D={D} O={O} K={K} T={T} per-keypoint w, weights', M, y, var, w, lam)
    if T == 17:
        check_dense(f'D={D} O={O} K={K} T={T} shared w, no weights', M, y, var, w[:, 0].copy(), None)
        check_dense(f'D={D} O={O} K={K} T={T} no w, weights', M, y, var, None, lam)


@pytest.mark.parametrize('which', ['singular_q', 'unit_root'])
def test_general_models_singular_q_and_unit_root(which):
    M, y, var, w, lam = dense_case(3, 4, 5, 70, seed=31, singular_q=which == 'singular_q', unit_root=which == 'unit_root')
    check_dense(which, M, y, var, w, lam)


def test_general_model_generator_equals_its_injected_normals():
    from eks_amd import hip_ops
    D, O, K, T, S, seed = 3, 4, 5, 33, 4, 0x0123456789abcdef
    M, y, var, w, lam = dense_case(D, O, K, T, seed=3)
    run = lambda **kw: hip_ops.sample_tv(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), S, qscale=_dev(w),  # noqa: E731
                                         weights=_dev(lam), **kw)[0].cpu().numpy()
    nz = hip_ops.sample_noise(T, K, D, O, S, seed=seed)
    assert np.array_equal(run(seed=seed), run(noise=nz))


# ---- the Python surface -------------------------------------------------------------------------------------------------
N_DRAWS = 256


def within_six_standard_errors(mean, centre, sd):
    return bool(np.all(np.abs(mean - centre) < 6.0 * sd / np.sqrt(N_DRAWS)))


def _marker_array(mk):
    from eks_amd.marker_array import MarkerArray
    return MarkerArray(mk.astype(np.float64), data_fields=['x', 'y', 'likelihood'])


def _scalar_reference_means(model, s, seed, w=None, lam=None):
    """The float64 reference sampler on the generator's own normals for a single-camera model: mean deviation, sd."""
    ys, m0s, S0s, As, Cs, Qs, evs = model
    K, T, _ = ys.shape
    N = K * 2
    diag = lambda a: np.diagonal(np.asarray(a, np.float64), axis1=1, axis2=2).reshape(-1)  # noqa: E731
    var = np.asarray(evs, np.float32).reshape(T, N)
    qs = np.repeat(np.broadcast_to(np.asarray(s, np.float64), (K,)), 2) * diag(Qs)
    _, Pf, _, Vs, _ = tvref.scalar_filter_smoother(np.zeros((T, N)), var, np.zeros(N), diag(S0s), diag(As), diag(Cs), qs,
                                                   w, lam, 2)
    e = tvref.scalar_deviations(Pf, diag(As), qs, ref.scalar_noise(seed, T, N, N_DRAWS), w, 2)
    return e.mean(axis=0), np.sqrt(Vs)


def test_sample_singlecam_irregular_on_a_synthetic_session():
    from eks_amd import sample_singlecam_irregular, smooth_singlecam_irregular
    from eks_amd._problem import singlecam_problem
    from eks_amd.irregular import process_noise_scale_from_times
    from eks_amd.synth import singlecam_markers
    T, K, seed = 300, 3, 5
    ma = _marker_array(singlecam_markers(T, K, seed=2))
    names = [f'k{i}' for i in range(K)]
    rng = np.random.default_rng(1)
    times = np.cumsum(np.where(rng.random(T) < 0.05, rng.integers(2, 30, T), 1)).astype(np.float64) / 60.0
    s = np.array([0.5, 2.0, 8.0])
    sm = smooth_singlecam_irregular(ma, names, s, frame_times=times)
    model, _, _ = singlecam_problem('test', ma, names, 'median', 'confidence_weighted_var')
    e_mean, sd = _scalar_reference_means(model, s, seed, w=process_noise_scale_from_times(times))
    assert within_six_standard_errors(e_mean, 0.0, sd)                       # the reference alone, same normals
    assert np.abs(sd.reshape(T, K, 2) ** 2 / sm['Vs'] - 1).max() < 1e-4     # the driver's variances are these chains'
    dr = sample_singlecam_irregular(ma, names, s, N_DRAWS, frame_times=times, seed=seed)
    assert dr.shape == (N_DRAWS, T, K, 2) and dr.dtype == np.float32
    assert np.array_equal(dr, sample_singlecam_irregular(ma, names, s, N_DRAWS, frame_times=times, seed=seed))
    assert within_six_standard_errors(dr.astype(np.float64).mean(axis=0), sm['ms'], np.sqrt(sm['Vs']))
    with pytest.raises(ValueError):
        sample_singlecam_irregular(ma, names, s, 4)


@pytest.mark.parametrize('nu_obs,nu_proc', [(4.0, 4.0), (4.0, float('inf')), (float('inf'), 4.0)])
def test_sample_singlecam_heavy_tailed_on_the_heavy_session_events(nu_obs, nu_proc):
    import heavy_ref
    from eks_amd import sample_singlecam_heavy_tailed
    from eks_amd._problem import singlecam_problem
    from eks_amd.synth import singlecam_markers
    T, K, seed = 300, 2, 9
    mk = singlecam_markers(T, K, seed=3)
    H = heavy_ref.heavy_session(0)                                           # its jumps and displaced frames below T
    assert (H['jumps'] < T).sum() >= 3 and (H['bad'] < T).sum() >= 3
    rng = np.random.default_rng(4)
    mk[:, 0, :, 0, :2] = 200.0 + H['y'][None, :T] + rng.normal(0.0, 0.8, (mk.shape[0], T, 2))
    ma = _marker_array(mk)
    names = [f'k{i}' for i in range(K)]
    s = np.array([0.05, 1.0])
    dr, sm = sample_singlecam_heavy_tailed(ma, names, s, N_DRAWS, nu_obs=nu_obs, nu_proc=nu_proc, seed=seed,
                                           return_smoothed=True)
    assert dr.shape == (N_DRAWS, T, K, 2) and dr.dtype == np.float32
    assert ('weights' in sm) == np.isfinite(nu_obs) and ('scales' in sm) == np.isfinite(nu_proc)
    model, _, _ = singlecam_problem('test', ma, names, 'median', 'confidence_weighted_var')
    lam = sm['weights'].reshape(T, K * 2) if 'weights' in sm else None
    e_mean, sd = _scalar_reference_means(model, s, seed, w=sm.get('scales'), lam=lam)
    assert within_six_standard_errors(e_mean, 0.0, sd)                       # the reference alone, same normals
    assert within_six_standard_errors(dr.astype(np.float64).mean(axis=0), sm['ms'], np.sqrt(sm['Vs']))


def test_sample_multicam_robust_on_a_synthetic_session():
    from eks_amd import sample_multicam_robust, smooth_multicam_robust
    from eks_amd.robust import multicam_problem, smooth_robust_grouped
    from eks_amd.synth import multicam_markers
    T, K, V, seed = 300, 2, 2, 13
    mk = multicam_markers(T, K, V=V, seed=1)
    ma = _marker_array(mk)
    names, cams = [f'k{i}' for i in range(K)], [f'c{i}' for i in range(V)]
    kw = dict(avg_mode='median', var_mode='confidence_weighted_var')
    s = 1.0
    sm = smooth_multicam_robust(ma, names, cams, s, **kw)
    pix, lat = sample_multicam_robust(ma, names, cams, s, N_DRAWS, seed=seed, return_latent=True, **kw)
    D = sm['ms'].shape[-1]
    assert pix.shape == (N_DRAWS, T, K, 2 * V) and pix.dtype == np.float32 and lat.shape == (N_DRAWS, T, K, D)
    # the float64 reference on the generator's normals under the driver's own weights
    model, mu = multicam_problem(ma, names, cams, 50.0, kw['avg_mode'], kw['var_mode'], None, D)
    ys, m0s, S0s, As, Cs, Qs, evs = model
    lam = np.repeat(sm['weights'], 2, axis=2)
    z = ref.dense_noise(seed, T, K, D + 2 * V, N_DRAWS)
    _, Vs, dev = tvref.dense_durbin_koopman(np.swapaxes(ys, 0, 1), evs, m0s, S0s, As, Cs, Qs, np.full(K, s), z, None, lam)
    sd = np.sqrt(np.diagonal(Vs, axis1=-2, axis2=-1))
    assert within_six_standard_errors(dev.mean(axis=0), 0.0, sd)             # the reference alone, same normals
    assert np.abs(sd ** 2 / sm['Vs'] - 1).max() < 1e-3                       # the driver's variances are this model's
    assert within_six_standard_errors(lat.astype(np.float64).mean(axis=0), sm['ms'], np.sqrt(sm['Vs']))
    rep = np.einsum('kod,ntkd->ntko', Cs, lat.astype(np.float64)) + mu[None, None]
    assert np.abs(pix - rep).max() <= 1e-5 * np.abs(rep).max()              # the pixels are C x + the centring means
