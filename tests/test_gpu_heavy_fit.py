"""GPU: eks_smooth_heavy_fit (the drivers of eks_amd/csrc/eks_smooth_student.hip and eks_dense.hip with the M-step of
eks_amd/csrc/eks_smooth_heavy_fit.hip) and eks_amd.heavy_tails.fit_* against the references of tests/heavy_fit_ref.py,
through the C ABI.

Bars.  Scalar chains (float32 lanes), the project's rule (heavy_fit_ref.bars): error / scale <= max(1e-5, 4 x the
float32 NumPy transcription's own worst error / scale on the same inputs); scales as tests/test_gpu_heavy.py's, log s
and row 2 of change over 1.  General models: tests/test_gpu_heavy.py's bars (100 x the disagreement of the two float64
reference forms, floored at 1e-12 and capped at 1e-8, plus one float32 ulp), log s and row 2 of change over 1.  Scalar
inputs are tests/test_gpu_heavy.py's sessions, general ones dense_inputs below.  Nothing is compared with the kernels'
own output, except where the test is about bits (the identities with eks_smooth_heavy, continuation, determinism,
subsets, a poisoned keypoint, buffers) or about two kernels (both sides Gaussian against eks_em_scale_run, under the
same bar).

Measured on the MI355X: DESIGN.md 9q."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_guard as bg  # noqa: E402
import heavy_fit_ref as fref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case  # noqa: E402
from test_gpu_increments import PARAMS, _dev, diag_flags, stable  # noqa: E402
from test_gpu_em import subset  # noqa: E402
from test_gpu_jumps import dense_excess, dense_session, u_in_range  # noqa: E402
import test_gpu_heavy as gh  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B = 32
R = fref.R
INF = math.inf
T_EDGES = (2, 3, B - 1, B, B + 1, R + 1, 33 * B + 1)
N_ITERS = (2, 3, 8)
NUS = ((4.0, 4.0), (4.0, INF), (INF, 4.0), (INF, INF))
NAMES = ('ms', 'Vs', 'weights', 'scales', 's_out', 'change')


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def raw_call(dims_args, ins, nus, n_iters, bounds, weights, scales, planes_in, change, s_out, ms, Vs, ws=None,
             ws_bytes=None):
    """eks_smooth_heavy_fit itself: ins = y, var, m0 .. s.  Returns the status."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*dims_args)
    if ws is None:
        need = int(lib.eks_smooth_heavy_fit_workspace_bytes(ctypes.byref(dims)))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda')
    p = hip_ops._ptr
    rc = lib.eks_smooth_heavy_fit(ctypes.byref(dims), *[p(t) for t in ins], float(nus[0]), float(nus[1]), int(n_iters),
                                  float(bounds[0]), float(bounds[1]), p(weights), p(scales), int(planes_in), p(change),
                                  p(s_out), p(ms), p(Vs), p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                  hip_ops._stream())
    torch.cuda.synchronize()
    return rc


def _outputs(T, K, D, O, vs_diag, lam0, w0):
    nan = lambda shape, dt=torch.float32: torch.full(shape, np.nan, dtype=dt, device='cuda')  # noqa: E731
    ms, Vs = nan((T, K, D)), nan((T, K, D) if vs_diag else (T, K, D, D))
    lam = _dev(np.ascontiguousarray(lam0, np.float32).reshape(T, K, O)) if lam0 is not None else nan((T, K, O))
    sc = _dev(np.ascontiguousarray(w0, np.float32).reshape(T, K)) if w0 is not None else nan((T, K))
    return ms, Vs, lam, sc, nan((3, K)), nan((K,), torch.float64)


def gpu_scalar(pb, nus, n_iters, bounds=fref.BOUNDS, lam0=None, w0=None, s0=None, ins=None, in_place=False):
    """-> ms (T, N), Vs (T, N), weights (T, N), scales (T, K), s_out (K,) float64, change (3, K)."""
    from eks_amd import _lib
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = list(gh.scalar_ins(pb) if ins is None else ins)
    if s0 is not None:
        ins[7] = _dev(np.ascontiguousarray(s0, np.float64))
    ms, Vs, lam, sc, ch, s_out = _outputs(T, K, D, D, True, lam0, w0)
    if in_place:
        ins[7] = ins[7].clone()
        s_out = ins[7]
    rc = raw_call((K, T, D, D, diag_flags(pb) | _lib.FLAG_VS_DIAG), ins, nus, n_iters, bounds, lam, sc,
                  int(lam0 is not None) + 2 * int(w0 is not None), ch, s_out, ms, Vs)
    assert rc == 0
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return h(ms).reshape(T, K * D), h(Vs).reshape(T, K * D), h(lam).reshape(T, K * D), h(sc), h(s_out), h(ch)


def chain_q(pb):
    return np.diagonal(pb['par']['Q'], axis1=1, axis2=2).reshape(-1)


def scalar_refs(pb, nus, counts, bounds=fref.BOUNDS, lam0=None, w0=None, s0=None):
    """{n: (float64 result, float32 transcription's result, bars)} for calls of n passes."""
    D = pb['D']
    s0 = pb['par']['s'] if s0 is None else s0
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], chain_q(pb), s0, nus[0], nus[1], max(counts))
    s64, s32 = dict.fromkeys(counts), dict.fromkeys(counts)
    fref.scalar_fit(*args, D=D, bounds=bounds, lam0=lam0, w0=w0, snapshots=s64)
    fref.scalar_fit_f32(*args, D=D, bounds=bounds, lam0=lam0, w0=w0, unit=pb['unit'], B=B, snapshots=s32)
    return {n: (s64[n], s32[n], fref.bars(s32[n], s64[n], pb['y'], D)) for n in counts}


def check_scalar(label, pb, got, ref, worst=None):
    r64, r32, bars = ref
    assert all(np.isfinite(x).all() for x in got) and (got[1] > 0).all() and (got[3] > 0).all() and (got[2] > 0).all() \
        and (got[4] > 0).all(), f'{label}: non-finite output'
    err, et = fref.errors(got, r64, pb['y'], pb['D']), fref.errors(r32, r64, pb['y'], pb['D'])
    for k in err:
        e, t = float(np.max(err[k])), float(np.max(et[k]))
        print(f'{label}: {k} {e:.3g} (transcription {t:.3g}, bar {bars[k]:.3g})')
        if worst is not None:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e, t))
        assert e <= bars[k], f'{label}: {k} {e:.3g} over its bar {bars[k]:.3g} (transcription {t:.3g})'


# ---- scalar chains: parity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nus', NUS, ids=lambda v: f'nu_{v[0]}_{v[1]}')
@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 2), (21, 3), (65, 2)])
def test_scalar_chain_edge_shapes(K, D, kind, nus):
    worst = {}
    for T in T_EDGES:
        pb = gh.session(T, K, D, kind, seed=T + K)
        ins = gh.scalar_ins(pb)
        refs = scalar_refs(pb, nus, N_ITERS)
        for n in N_ITERS:
            got = gpu_scalar(pb, nus, n, ins=ins)
            label = f'N={K * D} D={D} T={T} {kind} nu={nus} n_iters={n}'
            check_scalar(label, pb, got, refs[n], worst)
            assert (got[3][0] == 1).all() and (np.log(got[4]) >= -8 - 1e-12).all() and (np.log(got[4]) <= 8 + 1e-12).all()
            if math.isfinite(nus[0]):
                assert gh.lam_in_range(got[2], nus[0]), label
            else:
                assert (got[2] == 1).all() and not got[5][0].any(), label
            if math.isfinite(nus[1]):
                assert u_in_range(got[3], nus[1], D), label
            else:
                assert (got[3] == 1).all() and not got[5][1].any(), label
    print(f'N={K * D} D={D} {kind} nu={nus}, worst kernels (transcription on that case): '
          + ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (e, t) in worst.items()))


# ---- scalar chains: bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_one_and_two_passes_are_eks_smooth_heavy(kind):
    """n_iters = 1: eks_smooth_heavy's single pass bit for bit and s_out = s; n_iters = 2, both nu finite: its 2-pass
    planes and change bit for bit (pass 1 and its updates precede the first step), under another s."""
    T, K, D = 5 * B + 7, 5, 2
    pb = gh.session(T, K, D, kind, seed=11)
    ins = gh.scalar_ins(pb)
    for n in (1, 2):
        heavy = gh.gpu_scalar(pb, (4.0, 4.0), n, ins=ins)
        fit = gpu_scalar(pb, (4.0, 4.0), n, ins=ins)
        assert np.array_equal(fit[2], heavy[2]) and np.array_equal(fit[3], heavy[3]), n
        assert np.array_equal(fit[5][:2], heavy[4]), n
        if n == 1:
            assert np.array_equal(fit[0], heavy[0]) and np.array_equal(fit[1], heavy[1])
            assert np.array_equal(fit[4], pb['par']['s']) and not fit[5].any()
        else:
            assert (fit[4] != pb['par']['s']).all() and (fit[5][2] > 0).all()
            assert not np.array_equal(fit[0], heavy[0])
    # a Gaussian side: its plane comes back as ones, and a single pass leaves s alone
    for nus in NUS[1:]:
        one = gpu_scalar(pb, nus, 1, ins=ins)
        assert (one[2] == 1).all() and (one[3] == 1).all() and np.array_equal(one[4], pb['par']['s']) and not one[5].any()


@pytest.mark.parametrize('nus', NUS, ids=lambda v: f'nu_{v[0]}_{v[1]}')
def test_continuation_through_the_planes_and_s_out(nus):
    T, K, D = R + 40, 5, 2
    pb = gh.session(T, K, D, 'general', seed=11)
    ins = gh.scalar_ins(pb)
    whole8, whole7 = gpu_scalar(pb, nus, 8, ins=ins), gpu_scalar(pb, nus, 7, ins=ins)
    first = gpu_scalar(pb, nus, 3, ins=ins)
    cont = gpu_scalar(pb, nus, 6, lam0=first[2] if math.isfinite(nus[0]) else None,
                      w0=first[3] if math.isfinite(nus[1]) else None, s0=first[4], ins=ins)
    for name, a, b in zip(NAMES, cont, whole8):
        assert np.array_equal(a, b), (nus, name)
    assert not np.array_equal(whole7[4], whole8[4])
    aliased = gpu_scalar(pb, nus, 8, ins=ins, in_place=True)            # s_out == s
    for name, a, b in zip(NAMES, aliased, whole8):
        assert np.array_equal(a, b), (nus, name, 'in place')


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_two_calls_and_a_subset_of_the_keypoints_give_the_same_bits(kind):
    """Keypoints [3, 67) of K = 70 alone (another lane mapping, other keypoint tiles and last blocks of the sum) give the full call's
    s_out bytes - and with them every other output's."""
    T, K, D = 35 * B + 1, 70, 2                                            # two slabs of the sum
    pb = gh.session(T, K, D, kind, seed=21)
    ins = gh.scalar_ins(pb)
    full, again = gpu_scalar(pb, (4.0, 4.0), 4, ins=ins), gpu_scalar(pb, (4.0, 4.0), 4, ins=ins)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    assert (full[5] > 0).all()
    for k0, k1 in ((3, 67), (5, 8), (40, 41)):                             # tiles of 16 keypoints shifted against the full call's, and of 4
        sub = gpu_scalar(subset(pb, k0, k1), (4.0, 4.0), 4)
        assert sub[4].tobytes() == full[4][k0:k1].tobytes(), (k0, k1)
        for i in (0, 1, 2):
            assert np.array_equal(sub[i], full[i][:, D * k0:D * k1]), NAMES[i]
        assert np.array_equal(sub[3], full[3][:, k0:k1]) and np.array_equal(sub[5], full[5][:, k0:k1])


# ---- scalar chains: other behaviour ----------------------------------------------------------------------------------
def test_a_start_at_either_bound_stays_clipped():
    T, K, D = 300, 3, 2
    pb = gh.session(T, K, D, 'unit', seed=3)
    for bounds, at, nus in (((-8.0, -6.0), -6.0, (4.0, 4.0)), ((3.0, 8.0), 3.0, (4.0, 4.0)), ((-8.0, 1.0), 1.0, (INF, INF))):
        s0 = np.full(K, math.exp(at))
        got = gpu_scalar(pb, nus, 6, bounds=bounds, s0=s0)
        ref = scalar_refs(pb, nus, (6,), bounds=bounds, s0=s0)[6]
        assert np.abs(np.log(ref[0][4]) - at).max() < 1e-12, 'the reference left the bound: the case tests nothing'
        assert np.abs(np.log(got[4]) - at).max() < 1e-12 and np.abs(got[5][2]).max() < 1e-6, (bounds, got[4], got[5][2])
        check_scalar(f'start at the bound {at}', pb, got, ref)


def test_a_nan_keypoint_keeps_its_s_and_leaves_the_others_alone():
    T, K, D = R + 77, 6, 2
    pb = gh.session(T, K, D, 'general', seed=5)
    healthy = gpu_scalar(pb, (4.0, 4.0), 5)
    bad = dict(pb, y=pb['y'].copy())
    bad['y'][T // 2, 2 * D] = np.nan                                        # keypoint 2
    got = gpu_scalar(bad, (4.0, 4.0), 5)
    assert got[4][2].tobytes() == pb['par']['s'][2].tobytes() and got[5][2][2] == 0
    keep = np.array([k for k in range(K) if k != 2])
    cols = np.concatenate([np.arange(k * D, (k + 1) * D) for k in keep])
    assert got[4][keep].tobytes() == healthy[4][keep].tobytes()
    for i in (0, 1, 2):
        assert np.array_equal(got[i][:, cols], healthy[i][:, cols]), NAMES[i]
    assert np.array_equal(got[3][:, keep], healthy[3][:, keep]) and np.array_equal(got[5][:, keep], healthy[5][:, keep])


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_both_sides_gaussian_against_eks_em_scale_run(kind):
    """One keypoint per block, tol = 0 (no block stops): n passes are n - 1 iterations of eks_em_scale_run.  The
    float64 reference's bar for log s holds for either kernel against the reference, and between the two."""
    from eks_amd import hip_ops
    T, K, D = R + 200, 7, 2
    pb = gh.session(T, K, D, kind, seed=8, extra=False, events=[])
    n = 6
    ins = gh.scalar_ins(pb)
    s0 = pb['par']['s'] * np.geomspace(0.2, 5.0, K)                        # starts on either side of the session's s
    got = gpu_scalar(pb, (INF, INF), n, ins=ins, s0=s0)
    ref = scalar_refs(pb, (INF, INF), (n,), s0=s0)[n]
    check_scalar(f'{kind} both Gaussian', pb, got, ref)
    state = np.zeros((K, 4))
    state[:, 0] = np.log(s0)
    loop = hip_ops.EmScaleLoop(*ins[:7], _dev(np.arange(K + 1, dtype=np.int32)), _dev(np.arange(K, dtype=np.int32)),
                               _dev(state), _dev(s0.copy()), -8.0, 8.0, 0.0, 1000, flags=diag_flags(pb))
    loop.run(n - 1)
    torch.cuda.synchronize()
    em = loop.s_keypoint.cpu().numpy()
    bar = ref[2]['log_s']
    e_em, e_fit = np.abs(np.log(em) - np.log(ref[0][4])).max(), np.abs(np.log(got[4]) - np.log(ref[0][4])).max()
    print(f'{kind}: log s against the reference: eks_em_scale_run {e_em:.3g}, eks_smooth_heavy_fit {e_fit:.3g} (bar {bar:.3g})')
    assert e_em <= bar and e_fit <= bar
    assert np.abs(np.log(em) - np.log(got[4])).max() <= bar
    assert np.abs(np.log(ref[0][4] / s0)).min() > 1e-3, 's does not move in the reference: nothing was compared'


# ---- general models ------------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, nus, n_iters, bounds=fref.BOUNDS, vs_diag=False):
    from eks_amd import _lib
    T, K, O = y.shape
    D = M['m0'].shape[1]
    ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
    ms, Vs, lam, sc, ch, s_out = _outputs(T, K, D, O, vs_diag, None, None)
    assert raw_call((K, T, D, O, _lib.FLAG_VS_DIAG if vs_diag else 0), ins, nus, n_iters, bounds, lam, sc, 0, ch, s_out,
                    ms, Vs) == 0
    h = lambda t: t.cpu().numpy()  # noqa: E731
    return h(ms), h(Vs), h(lam), h(sc), h(s_out), h(ch)


def dense_inputs(M, T, O, seed):
    """tests/test_gpu_jumps.py's dense_session with true jumps of the state, seen through C, entering frames T // 4,
    T // 2 and 3 T // 4 of the even keypoints (20 .. 60 px in the largest observed coordinate, alternating in sign - at
    T = 1 100 dense_jumpy's 2 % of the frames walk a keypoint past 400 px) and the observations of about 2 % of the
    (frame, keypoint) pairs displaced by 20 .. 60 px in every coordinate."""
    y, var = dense_session(M, T, O, seed)
    rng = np.random.default_rng(seed + 100)
    K, D = M['m0'].shape
    y = y.astype(np.float64)
    for k in range(0, K, 2):
        sign = 1.0
        for t in sorted({T // 4, T // 2, 3 * T // 4} - {0}):
            dy = M['C'][k] @ rng.normal(size=D)
            y[t:, k] += dy * (sign * rng.uniform(20.0, 60.0) / np.abs(dy).max())
            sign = -sign
    hit = rng.random((T, K)) < 0.02
    if T > 5:
        hit[T // 2 + 3, 0] = True
    for t, k in np.argwhere(hit):
        y[t, k] += rng.choice([-1.0, 1.0], O) * rng.uniform(20.0, 60.0, O)
    assert np.abs(y).max() <= 400
    return y.astype(np.float32), np.maximum(var, np.float32(0.02))


def dense_refs(M, y, var, nus, counts):
    par = tuple(M[k] for k in PARAMS)
    out = []
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        snaps = dict.fromkeys(counts)
        fref.dense_fit(y, var, *par, nus[0], nus[1], max(counts), form=form, snapshots=snaps, plane_dtype=np.float32)
        out.append(snaps)
    return out


def check_dense(label, got, seq, joint, worst):
    five = lambda r: (r[0], r[1], r[2], r[3], np.asarray(r[5])[:2])  # noqa: E731
    gh.check_dense(label, five(got), five(seq), five(joint), worst)
    for name, g, a, b in (('log_s', np.log(got[4]), np.log(seq[4]), np.log(joint[4])),
                          ('dlog_s', got[5][2], seq[5][2], joint[5][2])):
        assert np.isfinite(g).all(), f'{label}: {name} is not finite'
        excess, bar = dense_excess(g[None], a[None], b[None], unit_scale=True)
        worst[name] = max(worst.get(name, 0.0), excess)
        assert excess <= 1.0, f'{label}: {name} is {excess:.3g} x its bar {bar:.3g} (+ one float32 ulp)'


@pytest.mark.parametrize('nus', [(4.0, 4.0), (4.0, INF)], ids=lambda v: f'nu_{v[0]}_{v[1]}')
@pytest.mark.parametrize('T', [2, 17, 1100])
@pytest.mark.parametrize('D,O,K', [(D, O, K) for K in (1, 3, 65) for D, O in [(1, 1), (2, 3), (3, 4), (6, 12)]])
def test_general_models_against_the_two_float64_forms(D, O, K, T, nus):
    M = stable(dense_case(K, D, O, False, seed=10 * D + K))
    y, var = dense_inputs(M, T, O, seed=T)
    seq, joint = dense_refs(M, y, var, nus, (2, 3))
    worst = {}
    for n in (2, 3):
        got = gpu_dense(M, y, var, nus, n, vs_diag=(n == 2))
        check_dense(f'D={D} O={O} K={K} T={T} nu={nus} n_iters={n}', got, seq[n], joint[n], worst)
        assert gh.lam_in_range(got[2], nus[0]) and (got[3][0] == 1).all()
        assert u_in_range(got[3], nus[1], D) if math.isfinite(nus[1]) else ((got[3] == 1).all() and not got[5][1].any())
    print(f'general D={D} O={O} K={K} T={T} nu={nus}: worst fraction of the bar '
          + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


def test_general_model_identities_with_eks_smooth_heavy():
    M = stable(dense_case(3, 3, 4, False, seed=12))
    y, var = gh.dense_heavy_inputs(M, 150, 4, seed=4)
    for n in (1, 2):
        heavy, fit = gh.gpu_dense(M, y, var, (4.0, 4.0), n), gpu_dense(M, y, var, (4.0, 4.0), n)
        assert np.array_equal(fit[2], heavy[2]) and np.array_equal(fit[3], heavy[3]) and np.array_equal(fit[5][:2], heavy[4])
        if n == 1:
            assert np.array_equal(fit[0], heavy[0]) and np.array_equal(fit[1], heavy[1]) and np.array_equal(fit[4], M['s'])
    a, b = gpu_dense(M, y, var, (4.0, INF), 4), gpu_dense(M, y, var, (4.0, INF), 4)
    for x, z in zip(a, b):
        assert np.array_equal(x, z)


# ---- refusals and buffers ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from eks_amd import _lib
    pb = gh.session(100, 3, 2, 'unit', seed=2)
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = gh.scalar_ins(pb)
    outs = [torch.full(shape, 7.0, dtype=dt, device='cuda')
            for shape, dt in (((T, K, D), torch.float32), ((T, K), torch.float32), ((3, K), torch.float32),
                              ((K,), torch.float64), ((T, K, D), torch.float32), ((T, K, D, D), torch.float32))]
    lam, sc, ch, so, ms, Vs = outs
    diag = diag_flags(pb)
    untouched = lambda: all(bool((o == 7.0).all()) for o in outs)  # noqa: E731
    call = lambda dims, tensors=ins, nus=(4.0, 4.0), n=8, bounds=(-8.0, 8.0), l=lam, w=sc, p_in=0, c=ch, s=so, m=ms, V=Vs, **kw: \
        raw_call(dims, tensors, nus, n, bounds, l, w, p_in, c, s, m, V, **kw)  # noqa: E731,E741
    good, dense = (K, T, D, D, diag), (K, T, D, D, 0)
    nan = float('nan')
    cases = [
        (call((K, 1, D, D, diag)), -2), (call((K, 1, D, D, 0)), -2),
        (call(good, nus=(0.0, 4.0)), -2), (call(good, nus=(4.0, -1.0)), -2), (call(good, nus=(nan, 4.0)), -2),
        (call(good, nus=(4.0, nan)), -2), (call(good, n=0), -2), (call(dense, n=-1), -2),
        (call(good, bounds=(1.0, 0.0)), -2), (call(good, bounds=(-INF, 0.0)), -2), (call(good, bounds=(0.0, INF)), -2),
        (call(dense, bounds=(nan, 0.0)), -2),
        (call(good, nus=(INF, 4.0), p_in=1), -2), (call(good, nus=(4.0, INF), p_in=2), -2), (call(dense, nus=(4.0, INF), p_in=3), -2),
        (call(dense, nus=(INF, 4.0)), -3), (call(dense, nus=(INF, INF)), -3),
        (call(good, l=None, p_in=1), -1), (call(good, w=None, p_in=2), -1), (call(dense, l=None, p_in=3), -1),
        (call(good, tensors=ins[:3] + [None] + ins[4:]), -1), (call(good, tensors=ins[:7] + [None]), -1),
        (call(good, s=None), -1), (call(good, m=None), -1), (call(good, V=None), -1),
        (call((0, T, D, D, diag)), -2), (call((K, T, D, D + 1, diag)), -2), (call((K, T, D, D, _lib.FLAG_UNIT_AC)), -3),
        (call((K, T, 7, 7, 0)), -3), (call((K, T, D, 65, 0)), -3), (call(good, ws_bytes=255), -4), (call(dense, ws_bytes=255), -4),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, (i, got, want)
    assert untouched()
    hb = int(_lib.load().eks_smooth_heavy_workspace_bytes(ctypes.byref(_lib.EksDims(*good))))
    assert call(good, ws_bytes=hb) == -4 and untouched()                     # eks_smooth_heavy's size lacks the partial sums
    assert call(good) == 0
    assert not any(bool((o == 7.0).any()) for o in outs)


@pytest.mark.parametrize('case', ['diag', 'diag_gauss_obs', 'dense'])
def test_guarded_workspace_and_outputs_at_an_offset(case):
    """A workspace of exactly the queried size filled with 0xFF between guards, and every output one element off its
    allocation's alignment (s_out, float64, one double off): nothing outside their extents is touched, and the result
    is the bits of the plain call - with the caller's planes and with the workspace's."""
    from eks_amd import _lib
    nus = (INF, 4.0) if case == 'diag_gauss_obs' else (4.0, 4.0)
    if case != 'dense':
        pb = gh.session(R + 70, 5, 2, 'unit', seed=2)
        T, K, D, O = pb['T'], pb['K'], pb['D'], pb['D']
        ins, flags = gh.scalar_ins(pb), diag_flags(pb) | _lib.FLAG_VS_DIAG
        plain = gpu_scalar(pb, nus, 3, ins=ins)
    else:
        M = stable(dense_case(3, 3, 4, False, seed=5))
        T, K, D, O = R + 70, 3, 3, 4
        y, var = dense_inputs(M, T, O, seed=2)
        ins, flags = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS], _lib.FLAG_VS_DIAG
        plain = gpu_dense(M, y, var, nus, 3, vs_diag=True)
    dims = _lib.EksDims(K, T, D, O, flags)
    need = int(_lib.load().eks_smooth_heavy_fit_workspace_bytes(ctypes.byref(dims)))
    gw = bg.GuardedWorkspaces(0xFF)
    ws = gw(need, 'cuda')
    assert ws.numel() == need
    for planes_given in (True, False):
        outs = dict(ms=bg.guarded_output((T, K, D), offset=1, name='ms'), Vs=bg.guarded_output((T, K, D), offset=1, name='Vs'),
                    weights=bg.guarded_output((T, K, O), offset=1, name='weights'),
                    scales=bg.guarded_output((T, K), offset=1, name='scales'),
                    s_out=bg.guarded_output((K,), dtype=torch.float64, offset=1, name='s_out'),
                    change=bg.guarded_output((3, K), offset=1, name='change'))
        rc = raw_call((K, T, D, O, flags), ins, nus, 3, fref.BOUNDS, outs['weights'].tensor if planes_given else None,
                      outs['scales'].tensor if planes_given else None, 0, outs['change'].tensor, outs['s_out'].tensor,
                      outs['ms'].tensor, outs['Vs'].tensor, ws=ws)
        assert rc == 0
        gw.assert_intact()
        for o in outs.values():
            o.assert_intact()
        for name in (NAMES if planes_given else ('ms', 'Vs', 's_out', 'change')):
            want = plain[NAMES.index(name)]
            assert np.array_equal(outs[name].tensor.cpu().numpy().reshape(want.shape), want), (name, planes_given)


def test_stale_and_poisoned_workspaces_give_the_same_bits():
    from eks_amd import _lib
    pb, other = gh.session(R + 70, 5, 2, 'general', seed=6), gh.session(R + 70, 5, 2, 'general', seed=7)
    dims_args = (5, pb['T'], 2, 2, diag_flags(pb) | _lib.FLAG_VS_DIAG)
    need = int(_lib.load().eks_smooth_heavy_fit_workspace_bytes(ctypes.byref(_lib.EksDims(*dims_args))))
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')

    def run(p):
        ins = gh.scalar_ins(p)
        ms, Vs, lam, sc, ch, s_out = _outputs(p['T'], 5, 2, 2, True, None, None)
        assert raw_call(dims_args, ins, (4.0, 4.0), 4, fref.BOUNDS, None, None, 0, ch, s_out, ms, Vs, ws=ws) == 0
        return [t.cpu().numpy() for t in (ms, Vs, s_out, ch)]

    clean = run(pb)
    run(other)
    stale = run(pb)
    ws.fill_(0xFF)
    poisoned = run(pb)
    for other_run in (stale, poisoned):
        for x, y_ in zip(clean, other_run):
            assert np.array_equal(x, y_)


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_fit_heavy_tailed_on_the_three_seed_session():
    """fit_heavy_tailed with nu_proc = inf on heavy_fit_ref.outlier_session reproduces the reference's s_fit within
    the bar, and the reference's quality assertions (tests/test_heavy_fit_cpu.py) hold for the device's output."""
    from eks_amd import fit_heavy_tailed, smooth_robust
    truth, eye = 0.05, np.eye(2)[None]
    for seed in (0, 1, 2):
        s = fref.outlier_session(seed)
        T = s['y'].shape[0]
        m0, S0, a, c, q = s['args']
        args = (s['y'].astype(np.float32)[None], m0[None], S0[None] * eye, eye, eye, eye, s['var'].astype(np.float32)[:, None])
        ref_args = (s['y'].astype(np.float32), s['var'].astype(np.float32), m0, S0, a, c, q)
        ms, Vs, lam, w, s_fit, ch = fit_heavy_tailed(*args, 1.0, nu_obs=4.0, nu_proc=INF, n_iters=40, vs_diag=True)
        assert ms.shape == (1, T, 2) and lam.shape == (1, T, 2) and w.shape == (1, T) and s_fit.shape == (1,)
        assert ch.shape == (3, 1) and s_fit.dtype == np.float64 and (w == 1).all()
        r64 = fref.scalar_fit(*ref_args, 1.0, 4.0, INF, 40, D=2)
        r32 = fref.scalar_fit_f32(*ref_args, 1.0, 4.0, INF, 40, D=2, unit=True, B=B)
        bars = fref.bars(r32, r64, ref_args[0], 2)
        got = (ms[0], Vs[0], lam[0], w.T, s_fit, ch)
        err = fref.errors(got, r64, ref_args[0], 2)
        for k in err:
            e = float(np.max(err[k]))
            print(f'seed {seed}: {k} {e:.3g} (bar {bars[k]:.3g})')
            assert e <= bars[k], (seed, k, e, bars[k])
        gauss = fit_heavy_tailed(*args, 1.0, nu_obs=INF, nu_proc=INF, n_iters=80, vs_diag=True)
        robust = smooth_robust(*args, gauss[4], nu=4.0, n_iters=12, vs_diag=True)
        r_fit, r_rob = fref.rmse(ms[0], s['x']), fref.rmse(robust[0][0], s['x'])
        print(f'seed {seed}: Gaussian fixed point s q = {gauss[4][0]:.4g}; fitted s q = {s_fit[0]:.4g}; RMSE fitted '
              f'{r_fit:.3g}, robust at the Gaussian s {r_rob:.3g}')
        assert gauss[4][0] > 100 * truth
        assert truth / 2.5 <= s_fit[0] <= truth * 2.5
        assert r_fit < 0.25 * r_rob


def test_fit_singlecam_heavy_tailed_returns_the_drivers_dictionary_and_s_fit(golden_dir):
    from eks_amd import fit_singlecam_heavy_tailed, smooth_singlecam_heavy_tailed
    from eks_amd.marker_array import MarkerArray
    mk, moved, names, bad, s = gh.golden_case(golden_dir)
    ma = MarkerArray(moved, data_fields=['x', 'y', 'likelihood'])
    T, K = moved.shape[2], moved.shape[3]
    one = fit_singlecam_heavy_tailed(ma, names, s, n_iters=1)
    same = smooth_singlecam_heavy_tailed(ma, names, s, n_iters=1)
    assert set(one) == set(same) | {'s_fit'} and np.array_equal(one['s_fit'], np.broadcast_to(s, (K,)))
    for k in same:
        assert np.array_equal(one[k], same[k]), k
    out = fit_singlecam_heavy_tailed(ma, names, s / 100.0, n_iters=12)
    assert out['ms'].shape == (T, K, 2) and out['scales'].shape == (T, K) and out['s_fit'].shape == (K,)
    assert all(np.isfinite(v).all() for v in out.values()) and (out['s_fit'] > 0).all()
