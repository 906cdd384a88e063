"""GPU: eks_smooth_increments (eks_amd/csrc/eks_increments.hip on scalar chains, dense_increments in eks_dense.hip on
general models) against the float64 references of tests/increments_ref.py.

Bars as in tests/test_increments_cpu.py (rule_excess): per chain, |error| <= max(1e-5 x the chain's scale, 4 x the
float32 transcription's own error on the same inputs) - scale: the chain's largest |reference| of that output over the
session, of Vs for lag1; the transcription's error: its worst |error| over the chains of the case, in the output's
units; dV of scalar chains additionally per entry, relative to the reference entry.  ms and Vs of scalar chains go by
the same rule; general models - float64 in the lane - are measured per keypoint as fractions of the keypoint's scale,
new outputs under max(1e-5, 4 x the float32-output transcription), ms and Vs under the suite's flat 1e-5.  The printed
figures are errors as fractions of scale, kernels (transcription).  Nothing is compared with the kernels' own output.

Why the transcription's error enters in the output's units and not as a fraction of each chain's scale: the edge
shapes have sessions of one to three frames, so a chain's scale is one number or two.  Float32's error on them is set
by the size of the positions (a mean of 0.0136 px formed as 3 + K (y - 3) carries the rounding of 3, 1.8e-5 of
itself), and among 130 chains one always has an increment or a mean a hundred times below its neighbours'.  Measured
on the MI355X with per-chain fractions: dmean at N = 130, T = 2, s = 300 was 3.0e-4 of that one chain's scale against
1.2e-5 for the transcription, two roundings of the same size on an accidental scale.  The edge sessions are centred
at 3 px (not 400, where the positions' spacing alone is 3e-5 px against increments of 1e-3 px at s = 1e-4, and not 0,
where every chain's scale is accidental).  The parity case at size (20 000 frames x 64 keypoints x 2) is at 400 px; its
worst values are printed and quoted in DESIGN.md 9d.

Measured on the MI355X, kernels (transcription), parity at size: s = 2: lag1 2.5e-7 (1.8e-7), dmean 4.2e-5 (1.9e-5),
dV 3.4e-7 (2.8e-7), per entry 3.9e-7 (3.3e-7); s = 1e-4: lag1 2.7e-6 (1.6e-6), dmean 4.5e-3 (1.6e-3), dV per entry
2.2e-7 (2.0e-7).  General models: every output within 5.6e-8 of scale, the rounding of the float32 store.  Moments of
4 096 eks_sample draws: 2.8, 2.6, 3.3 standard errors.  DESIGN.md 9d has the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import increments_ref as iref  # noqa: E402
import sampling_ref as sref  # noqa: E402
from test_increments_cpu import (NAMES, dense_case, entry_error, make_session, moment_errors, references,  # noqa: E402
                                 rule_excess, scaled_error)
from dense_forms import general_grid, general_seed  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')
NEW = ('lag1', 'dmean', 'dV')
T_EDGES = (1, 2, 3, 31, 32, 33, 64, 65, 128, 129, 288, 289)     # chunk edges; ceil(sqrt(nc)) changes at nc = 2, 5, 10


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def diag_flags(pb):
    from eks_amd import _lib
    return _lib.FLAG_DIAG_MODEL | (_lib.FLAG_UNIT_AC if pb['unit'] else 0)


def gpu_scalar(pb, want=NEW, want_smooth=True, flags=None, y=None):
    """hip_ops.smooth_increments on the chains of make_session -> dict of (T, N) float32 arrays."""
    from eks_amd import hip_ops
    T, K, D = pb['T'], pb['K'], pb['D']
    par = pb['par']
    out = hip_ops.smooth_increments(_dev((pb['y'] if y is None else y).reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)),
                                    *(_dev(par[k]) for k in PARAMS), flags=diag_flags(pb) if flags is None else flags,
                                    vs_diag=True, want=want, want_smooth=want_smooth)
    torch.cuda.synchronize()
    return {n: v.cpu().numpy().reshape(T, K * D) for n, v in out.items()}


def check_scalar(label, pb, got, per_entry=True):
    r64, r32 = references(pb)
    T = pb['T']
    for n in NEW:
        assert not got[n][-1].any(), f'{label}: row T-1 of {n} is not zero'
    figs = []
    for n in NAMES:
        assert np.isfinite(got[n]).all()
        if T == 1 and n in NEW:
            continue                                   # all zeros, checked above; no scale to divide by
        err, trans = scaled_error(got[n], r64, n), scaled_error(r32[n], r64, n)
        excess = rule_excess(got[n], r32, r64, n)
        figs.append(f'{n} {err:.3g} ({trans:.3g})')
        assert excess <= 1.0, f'{label}: {n} is {excess:.3g} x its bar; of scale {err:.3g} (transcription {trans:.3g})'
    if per_entry and T > 1:
        ent, tent = entry_error(got['dV'], r64), entry_error(r32['dV'], r64)
        figs.append(f'dV per entry {ent:.3g} ({tent:.3g})')
        assert ent <= max(1e-5, 4 * tent), f'{label}: dV per entry {ent:.3g}, transcription {tent:.3g}'
    return ', '.join(figs)


def edge_session(T, K, D, sval, kind, seed):
    """make_session centred at 3 px; kind: 'unit', 'decay' (a = 0.98) or 'flip' (a = -0.8), the last two with
    c = 1.3 and a q of its own per chain."""
    pb = make_session(T, K, D, sval, kind == 'unit', seed, a=0.98 if kind == 'decay' else -0.8, c=1.3, centre=3.0)
    if kind != 'unit':
        q = np.random.default_rng(seed + 1).uniform(0.5, 2.0, K * D)
        pb['par']['Q'][:, np.arange(D), np.arange(D)] = q.reshape(K, D)
        pb['qs'] = q * sval
    return pb


@pytest.mark.parametrize('kind', ['unit', 'decay', 'flip'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 1), (3, 2), (21, 3), (65, 1), (65, 2)])
def test_scalar_chain_edge_shapes(K, D, kind):
    worst = ''
    for T in T_EDGES:
        for sval in (1e-4, 2.0, 300.0):
            pb = edge_session(T, K, D, sval, kind, seed=T + K)
            got = gpu_scalar(pb)
            worst = check_scalar(f'N={K * D} D={D} T={T} s={sval} {kind}', pb, got)
            if T == 1:                                 # (ms, Vs of the single frame: held by check_scalar's rule)
                assert all(not got[n].any() for n in NEW)
    print(f'N={K * D} D={D} {kind}, last case kernels (transcription): {worst}')


def test_scalar_chains_with_extreme_variances():
    """Variances at the 1e-12 floor, at 1e30 and at inf (both meet the clip at 1e30): the per-chain-scale bar only -
    in front of an unobserved frame the reference's dV is dominated by one term and a per-entry ratio says nothing
    more, behind a floored one it is ~1e-12 of the chain's scale."""
    for unit in (True, False):
        pb = make_session(129, 3, 2, 2.0, unit, seed=4, centre=0.0)
        pb['var'][7, 0] = 1e-12
        pb['var'][40, 1] = 1e30
        pb['var'][41, 1] = np.inf
        pb['var'][64, 2] = np.inf
        pb['var'][128, 3] = 1e-12
        pb['var'][0, 4] = np.inf
        print(f'extreme variances unit={unit}: ' + check_scalar('extreme variances', pb, gpu_scalar(pb), per_entry=False))


@pytest.mark.parametrize('sval', [2.0, 1e-4])
def test_scalar_parity_at_modest_size(sval):
    """20 000 frames x 64 keypoints x D = 2 at 400 px.  Worst values over the session, kernels (transcription), are
    printed; DESIGN.md 9d records them beside the host simulator's."""
    pb = make_session(20000, 64, 2, sval, True, seed=9)
    print(f'parity at size s={sval}: ' + check_scalar(f'parity s={sval}', pb, gpu_scalar(pb)))


def test_null_output_combinations_are_bit_identical_to_the_full_call():
    from eks_amd import _lib
    for unit in (True, False):
        pb = make_session(200, 5, 2, 2.0, unit, seed=12, centre=0.0)
        full = gpu_scalar(pb)
        for want, smooth in ((('lag1',), True), (('dmean',), True), (('dV',), True), (NEW, False),
                             (('dV', 'lag1'), False)):
            part = gpu_scalar(pb, want=want, want_smooth=smooth)
            assert sorted(part) == sorted(want + (('ms', 'Vs') if smooth else ()))
            for n, v in part.items():
                assert np.array_equal(v, full[n]), f'{n} with want={want} smooth={smooth} unit={unit}'
    # general model, same property
    M = dense_case(3, 3, 4, False, seed=3)
    y, var = dense_session(M, 50, 4, seed=1)
    full = gpu_dense(M, y, var, vs_diag=False)
    for want, smooth in ((('lag1',), True), (('dmean',), False), (('dV',), False)):
        part = gpu_dense(M, y, var, vs_diag=False, want=want, want_smooth=smooth)
        for n, v in part.items():
            assert np.array_equal(v, full[n])
    # all three NULL: refused before anything is enqueued
    lib = _lib.load()
    f32 = torch.zeros(1 << 12, dtype=torch.float32, device='cuda')
    f64 = torch.zeros(1 << 12, dtype=torch.float64, device='cuda')
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda')
    d = _lib.EksDims(2, 16, 2, 2, _lib.FLAG_DIAG_MODEL | _lib.FLAG_VS_DIAG)
    p32, p64 = ctypes.c_void_p(f32.data_ptr()), ctypes.c_void_p(f64.data_ptr())
    args = [p32, p32] + [p64] * 6
    assert lib.eks_smooth_increments(ctypes.byref(d), *args, p32, p32, None, None, None, ctypes.c_void_p(ws.data_ptr()),
                                     ws.numel(), None) == -1
    torch.cuda.synchronize()


def test_a_nan_observation_stays_in_its_keypoint():
    for unit in (True, False):
        pb = make_session(150, 6, 2, 2.0, unit, seed=14, centre=0.0)
        healthy = gpu_scalar(pb)
        y = pb['y'].copy()
        y[70, 2 * 2 + 1] = np.nan                       # keypoint 2, coordinate 1
        sick = gpu_scalar(pb, y=y)
        others = [n for n in range(pb['N']) if n // 2 != 2]
        for n in NAMES:
            assert np.array_equal(sick[n][:, others], healthy[n][:, others]), n
        assert np.isnan(sick['ms'][:, 5]).any()


# ---- general models -------------------------------------------------------------------------------------------------
def dense_session(M, T, O, seed):
    rng = np.random.default_rng(seed)
    K, D = M['m0'].shape
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


def stable(M, unit_root=False):
    K, D = M['m0'].shape
    M = dict(M)
    if unit_root:
        M['A'] = np.tile(np.eye(D), (K, 1, 1))
    else:
        rho = np.abs(np.linalg.eigvals(M['A'])).max(axis=1)
        M['A'] = M['A'] * np.minimum(1.0, 0.99 / rho)[:, None, None]
    return M


def gpu_dense(M, y, var, vs_diag, want=NEW, want_smooth=True, flags=0):
    from eks_amd import hip_ops
    out = hip_ops.smooth_increments(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), flags=flags, vs_diag=vs_diag,
                                    want=want, want_smooth=want_smooth)
    torch.cuda.synchronize()
    return {n: v.cpu().numpy() for n, v in out.items()}


def keypoint_error(x, ref, scale_ref):
    """worst |x - ref| per keypoint over the keypoint's largest |scale_ref|; arrays [T][K]..."""
    K = ref.shape[1]
    e = np.abs(x.astype(np.float64) - ref).transpose(1, 0, *range(2, ref.ndim)).reshape(K, -1).max(axis=1)
    s = np.abs(scale_ref).transpose(1, 0, *range(2, scale_ref.ndim)).reshape(K, -1).max(axis=1)
    return float((e / s).max())


def check_dense(label, M, y, var, got, vs_diag):
    r64 = dict(zip(NAMES, iref.dense_increments(y, var, *(M[k] for k in PARAMS))))
    r32 = {n: v.astype(np.float32) for n, v in r64.items()}
    T = y.shape[0]
    figs = []
    for n in NAMES:
        ref, t32 = r64[n], r32[n]
        if vs_diag and n != 'ms' and n != 'dmean':
            ref, t32 = (np.diagonal(a, axis1=-2, axis2=-1) for a in (ref, t32))
        assert got[n].shape == ref.shape and np.isfinite(got[n]).all()
        if n in NEW:
            assert not got[n][-1].any(), f'{label}: row T-1 of {n} is not zero'
            if T == 1:
                continue
        scale_ref = r64['Vs'] if n == 'lag1' else r64[n]
        err, trans = keypoint_error(got[n], ref, scale_ref), keypoint_error(t32, ref, scale_ref)
        bar = 1e-5 if n in ('ms', 'Vs') else max(1e-5, 4 * trans)
        figs.append(f'{n} {err:.3g} ({trans:.3g})')
        assert err <= bar, f'{label}: {n} {err:.3g} against the bar {bar:.3g} (transcription {trans:.3g})'
    return ', '.join(figs), r64


# (and the accepted width, odd O past 32 and the smallest odd O, at K = 3: tests/dense_forms.py WIDE_PAIRS)
@pytest.mark.parametrize('D,O,K', general_grid([(1, 1), (2, 2), (3, 4), (6, 12)]))
def test_general_models_against_the_dense_reference(D, O, K, set_knob):
    M = stable(dense_case(K, D, O, False, seed=general_seed(D, O, K)))
    figs = ''
    for i, T in enumerate((1, 2, 15, 16, 17, 33, 100)):
        y, var = dense_session(M, T, O, seed=T)
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            vs_diag = bool((i + int(chunk) // 16) % 2)
            figs, _ = check_dense(f'D={D} O={O} K={K} T={T} chunk={chunk}', M, y, var, gpu_dense(M, y, var, vs_diag), vs_diag)
    print(f'general D={D} O={O} K={K}, last case kernels (transcription): {figs}')


@pytest.mark.parametrize('chunk,T', [('16', 1100), ('32', 2100)])
def test_general_model_spanning_more_than_one_scan_block(chunk, T, set_knob):
    """ceil(T / chunk) > 64 chunks: two blocks of dense_scan_kernel, boundaries through dense_scan_blocks_kernel."""
    set_knob('EKS_DENSE_CHUNK', chunk)
    assert -(-T // int(chunk)) > 64
    M = stable(dense_case(3, 3, 4, False, seed=5))
    y, var = dense_session(M, T, 4, seed=2)
    figs, _ = check_dense(f'T={T} chunk={chunk}', M, y, var, gpu_dense(M, y, var, False), False)
    print(f'general, {-(-T // int(chunk))} chunks of {chunk}: {figs}')


@pytest.mark.parametrize('variant', ['unit_root', 'singular_q'])
@pytest.mark.parametrize('vs_diag', [False, True])
def test_general_model_variants_and_the_shape_of_the_outputs(variant, vs_diag):
    K, D, O, T = 3, 3, 4, 100
    M = stable(dense_case(K, D, O, variant == 'singular_q', seed=8), unit_root=variant == 'unit_root')
    if variant == 'singular_q':
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    y, var = dense_session(M, T, O, seed=3)
    got = gpu_dense(M, y, var, vs_diag)
    figs, r64 = check_dense(f'{variant} vs_diag={vs_diag}', M, y, var, got, vs_diag)
    print(f'general {variant} vs_diag={vs_diag}: {figs}')
    if vs_diag:
        return
    # lag1 is NOT symmetric: row = coordinate of x_t, column = coordinate of x_{t+1}; the transposed convention is
    # far outside the bar
    scale = np.abs(r64['Vs']).max()
    assert np.abs(got['lag1'] - np.swapaxes(r64['lag1'], -1, -2)).max() / scale > 1e-3
    # dV symmetric and positive semi-definite to rounding
    dV = got['dV'][:-1].astype(np.float64)
    assert np.array_equal(got['dV'], np.swapaxes(got['dV'], -1, -2))
    for k in range(K):
        ev = np.linalg.eigvalsh(dV[:, k])
        assert ev.min() >= -2.0 ** -22 * np.abs(dV[:, k]).max()


def test_a_diagonal_model_down_the_general_path_agrees_with_the_scalar_path():
    pb = edge_session(100, 5, 2, 2.0, 'decay', seed=6)
    a = gpu_scalar(pb)
    b = gpu_scalar(pb, flags=0)                                   # no DIAG_MODEL flag: dense_increments, VS_DIAG
    print('scalar path: ' + check_scalar('scalar path', pb, a))
    print('general path: ' + check_scalar('general path on a diagonal model', pb, b))


# ---- against the shipped sampler, and the Python surface ------------------------------------------------------------------
def test_moments_of_eks_sample_draws_match_the_increment_outputs():
    from eks_amd import hip_ops
    T, K, D, n = 40, 3, 2, 4096
    pb = make_session(T, K, D, 2.0, False, seed=31, centre=0.0)
    par = pb['par']
    dev = [_dev(par[k]) for k in PARAMS]
    y, var = _dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))
    draws, ms = hip_ops.sample(y, var, *dev, n, seed=3, flags=diag_flags(pb), want_mean=True)
    inc = gpu_scalar(pb)
    torch.cuda.synchronize()
    x = draws.cpu().numpy().reshape(n, T, K * D).astype(np.float64)
    e = x - ms.cpu().numpy().reshape(1, T, K * D).astype(np.float64)
    Vs, lag1, dmean, dV = (inc[k].astype(np.float64) for k in ('Vs', 'lag1', 'dmean', 'dV'))
    var_err, lag_err, _ = moment_errors(e, Vs, lag1, dV)
    mean_err = float((np.abs(np.diff(x, axis=1).mean(axis=0) - dmean[:-1]) / np.sqrt(dV[:-1] / n)).max())
    print(f'eks_sample against eks_smooth_increments, in standard errors: increment variance {var_err:.2f}, '
          f'lag-one covariance {lag_err:.2f}, increment mean {mean_err:.2f}')
    assert max(var_err, lag_err, mean_err) < 6


def test_smooth_increments_and_velocity_singlecam_on_the_golden_markers(golden_dir):
    from eks_amd.marker_array import MarkerArray
    from eks_amd.posterior import smooth_increments, velocity_singlecam
    from eks_amd.singlecam_smoother import ensemble_kalman_smoother_singlecam
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers']
    names = [str(k) for k in g['keypoints']]
    M_, V, T, K, _ = mk.shape
    ma = MarkerArray(mk.astype(np.float64), data_fields=['x', 'y', 'likelihood'])
    df, s = ensemble_kalman_smoother_singlecam(ma, names, smooth_param=10.0)
    fps = 60.0
    vel = velocity_singlecam(ma, names, s, fps=fps)
    assert vel['velocity'].shape == (T - 1, K, 2) and vel['velocity_var'].shape == (T - 1, K, 2)
    assert vel['speed_rms'].shape == (T - 1, K) and all(v.dtype == np.float32 for v in vel.values())
    # the same model through smooth_increments (built as sample_singlecam builds it): diagonals, then the diagonal
    # embedding with full_cov
    from eks_amd.core import ensemble
    from eks_amd.singlecam_smoother import initialize_kalman_filter
    from eks_amd.utils import center_predictions
    ens = ensemble(ma, avg_mode='median', var_mode='confidence_weighted_var')
    _, centered, _, _ = center_predictions(ens, quantile_keep_pca=100)
    m0s, S0s, As, Qs, Cs = initialize_kalman_filter(centered)
    args = (np.swapaxes(np.asarray(centered.array)[0, 0], 0, 1), m0s, S0s, As, Cs, Qs,
            np.asarray(ens.array)[0, 0][:, :, 2:4], s)
    inc = smooth_increments(*args)
    assert inc.ms.shape == (K, T, 2) and inc.Vs.shape == (K, T, 2)
    assert inc.lag1.shape == inc.dmean.shape == inc.dV.shape == (K, T - 1, 2)
    dmean, dV = np.swapaxes(inc.dmean, 0, 1), np.swapaxes(inc.dV, 0, 1)
    assert np.allclose(vel['velocity_var'], dV * np.float32(fps * fps), rtol=1e-6, atol=0)
    assert np.allclose(vel['velocity'], dmean * np.float32(fps), rtol=1e-6, atol=1e-6 * np.abs(vel['velocity']).max())
    want2 = fps * fps * ((dmean.astype(np.float64) ** 2).sum(-1) + dV.astype(np.float64).sum(-1))
    assert np.allclose(vel['speed_rms'].astype(np.float64) ** 2, want2, rtol=1e-5)
    # the driver's columns are these chains' marginals
    tab = df.to_numpy().reshape(T, K, 9)
    assert np.abs(np.swapaxes(inc.Vs, 0, 1) / tab[:, :, 7:9] - 1).max() < 1e-4
    full = smooth_increments(*args, full_cov=True)
    assert full.Vs.shape == (K, T, 2, 2) and full.lag1.shape == full.dV.shape == (K, T - 1, 2, 2)
    for a, b in ((full.Vs, inc.Vs), (full.lag1, inc.lag1), (full.dV, inc.dV)):
        assert np.array_equal(np.diagonal(a, axis1=-2, axis2=-1), b)
        assert not a[..., 0, 1].any() and not a[..., 1, 0].any()
    assert np.array_equal(full.ms, inc.ms) and np.array_equal(full.dmean, inc.dmean)
    devt = smooth_increments(*args, return_device=True, full_cov=True)
    assert devt.dV.is_cuda and tuple(devt.dV.shape) == (K, T - 1, 2, 2)
    assert np.array_equal(devt.dV.cpu().numpy(), full.dV)
