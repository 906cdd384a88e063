"""GPU: eks_innovations (eks_amd/csrc/eks_innov.hip on scalar chains, dense_innovations in eks_dense.hip on general
models) and eks_amd.diagnostics against the float64 references of tests/innovations_ref.py.

Bars.  Scalar chains (float32 filter, float32 term, float64 sum), the project's rule (innovations_ref.f32_rule): per
chain, error / scale <= max(1e-5, 4 x the float32 NumPy transcription's own worst error / scale on the same inputs);
scale of innov: the chain's max |y|; of innov_var: its own value; of loglik: max(|loglik|, T).  General models
(float64 in the lane): 100 x the disagreement of the two independent float64 reference forms (sequential updates;
S_t as a matrix through numpy.linalg.cholesky) on the same inputs, floored at 1e-12 and capped at 1e-8
(innovations_ref.f64_bar), relative to max(|loglik|, T O) for loglik, the keypoint's max |y| for innov, its own value
for innov_var and max(|value|, O) for nis and frame_ll; the float32 outputs get one float32 ulp of the reference value
added, because they are rounded once.  Nothing is compared with the kernels' own output, except where the test is
about bits (absent outputs, determinism, subsets, NaN isolation).

Measured on the MI355X, kernels (transcription's worst on that case), error over scale.  Scalar edge shapes: innov_var
<= 3.5e-7 (2.3e-7), loglik <= 5.7e-7 (2.3e-7), innov <= 1.3e-6 (1.3e-6) up to N = 65 and 1.9e-5 (1.9e-5) at N = 130 - a
one-frame chain whose only |y| is small, the transcription's own figure; extreme variances innov 5.7e-8 (6.8e-8),
innov_var 1.1e-7 (1.1e-7), loglik 4.8e-8 (1.4e-8) unit and 8.6e-8 (1.3e-7), 1.8e-7 (2.0e-7), 5.3e-8 (2.7e-8) decaying.
General models: every float32 output at 0.5 of (bar 1e-12 + one float32 ulp) - its one rounding - and loglik within
1.4e-15 of max(|loglik|, T O), two scan blocks and the rank D-1 Q included.  Fisher's identity: gap 3.1e-7 where the two
float64 references have 3.3e-7.  Along 12 EM iterations the device loglik never dropped: smallest change +1.2e-2
(scalar unit), +3.6e-5 (decaying), +1.7e-8 (dense).  DESIGN.md 9f has the table."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref  # noqa: E402
import innovations_ref as iref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402
from test_gpu_increments import PARAMS, _dev, dense_session, diag_flags, edge_session, stable  # noqa: E402
from test_gpu_em import make_loop, subset  # noqa: E402
from dense_forms import general_grid, general_seed  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

SCALAR_OUT = ('innov', 'innov_var', 'loglik')
DENSE_OUT = ('innov', 'innov_var', 'nis', 'frame_ll', 'loglik')
T_EDGES = (1, 2, 32, 33, 129, 160, 161, 1121)   # one chunk, two chunks, the first shape with two scan groups, 6 x 6 groups


# ---- scalar chains -----------------------------------------------------------------------------------------------------
def gpu_scalar(pb, want=SCALAR_OUT, s=None, y=None):
    """hip_ops.innovations on the chains of make_session -> dict v, S (T, N) float32 and ll (N,) float64 (None if absent)."""
    from eks_amd import hip_ops
    T, K, D = pb['T'], pb['K'], pb['D']
    par = dict(pb['par'])
    if s is not None:
        par['s'] = np.asarray(s, np.float64)
    out = hip_ops.innovations(_dev((pb['y'] if y is None else y).reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)),
                              *(_dev(par[k]) for k in PARAMS), flags=diag_flags(pb), want=want)
    torch.cuda.synchronize()
    assert set(out) == set(want)
    for n in ('innov', 'innov_var'):
        assert n not in out or (out[n].dtype == torch.float32 and tuple(out[n].shape) == (T, K, D))
    assert 'loglik' not in out or (out['loglik'].dtype == torch.float64 and tuple(out['loglik'].shape) == (K, D))
    get = lambda n, shape: out[n].cpu().numpy().reshape(shape) if n in out else None
    return dict(v=get('innov', (T, K * D)), S=get('innov_var', (T, K * D)), ll=get('loglik', (K * D,)))


def scalar_refs(pb):
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    v, S, ll = iref.scalar_innovations(*args)
    v32, S32, ll32 = iref.scalar_innovations_f32(*args, unit=pb['unit'])
    return dict(v=v, S=S, ll=ll, y=pb['y'].astype(np.float64)), dict(v=v32, S=S32, ll=ll32)


def check_scalar(label, pb, got, worst=None):
    assert all(np.isfinite(got[k]).all() for k in got), f'{label}: non-finite output'
    assert (got['S'] > 0).all()
    ref, r32 = scalar_refs(pb)
    figs = iref.f32_rule(got, r32, ref)
    for name, (excess, err, trans) in figs.items():
        if worst is not None:
            w = worst.setdefault(name, (0.0, 0.0))
            worst[name] = max(w, (err, trans))
        assert excess <= 1.0, f'{label}: {name} is {excess:.3g} x its bar; {err:.3g} (transcription {trans:.3g})'
    return ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (_, e, t) in figs.items())


@pytest.mark.parametrize('kind', ['unit', 'decay'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 1), (3, 2), (21, 3), (65, 1), (65, 2)])
def test_scalar_chain_edge_shapes(K, D, kind):
    worst = {}
    for T in T_EDGES:
        for sval in (1e-4, 2.0, 300.0):
            pb = edge_session(T, K, D, sval, kind, seed=T + K)
            check_scalar(f'N={K * D} D={D} T={T} s={sval} {kind}', pb, gpu_scalar(pb), worst)
    print(f'N={K * D} D={D} {kind}, worst kernels (transcription on that case): ' +
          ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (e, t) in worst.items()))


def test_scalar_chains_with_extreme_variances():
    """Variances at the 1e-12 floor, at 1e30 and at inf (both meet the clip at 1e30): every output stays finite and
    the rule holds."""
    for unit in (True, False):
        pb = make_session(129, 3, 2, 2.0, unit, seed=4, centre=0.0)
        pb['var'][7, 0] = 1e-12
        pb['var'][40, 1] = 1e30
        pb['var'][41, 1] = np.inf
        pb['var'][64, 2] = np.inf
        pb['var'][128, 3] = 1e-12
        pb['var'][0, 4] = np.inf
        got = gpu_scalar(pb)
        assert got['S'][41, 1] == np.float32(1e30) and got['S'][0, 4] == np.float32(1e30)
        print(f'extreme variances unit={unit}: ' + check_scalar('extreme variances', pb, got))


# ---- general models ------------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, want=DENSE_OUT, flags=0, s=None):
    from eks_amd import hip_ops
    par = dict(M)
    if s is not None:
        par['s'] = np.asarray(s, np.float64)
    out = hip_ops.innovations(_dev(y), _dev(var), *(_dev(par[k]) for k in PARAMS), flags=flags, want=want)
    torch.cuda.synchronize()
    T, K, O = y.shape
    assert set(out) == set(want)
    shapes = dict(innov=(T, K, O), innov_var=(T, K, O), nis=(T, K), frame_ll=(T, K), loglik=(K,))
    for n, t in out.items():
        assert tuple(t.shape) == shapes[n] and t.dtype == (torch.float64 if n == 'loglik' else torch.float32)
    return {n: t.cpu().numpy() for n, t in out.items()}


def dense_scales(ref, y, T, O):
    return dict(innov=np.abs(y).max(axis=(0, 2))[None, :, None] * np.ones_like(ref['innov']), innov_var=ref['innov_var'],
                nis=np.maximum(np.abs(ref['nis']), O), frame_ll=np.maximum(np.abs(ref['frame_ll']), O),
                loglik=np.maximum(np.abs(ref['loglik']), T * O))


def check_dense(label, M, y, var, got, worst=None):
    T, K, O = y.shape
    par = tuple(M[k] for k in PARAMS)
    seq, joint = iref.dense_innovations_sequential(y, var, *par), iref.dense_innovations_joint(y, var, *par)
    scales = dense_scales(seq, y, T, O)
    figs = []
    for name in got:
        assert np.isfinite(got[name]).all(), f'{label}: {name} is not finite'
        bar = iref.f64_bar(seq[name], joint[name], scales[name])
        ulp = 0.0 if name == 'loglik' else np.spacing(np.abs(seq[name]).astype(np.float32)).astype(np.float64)
        err = np.abs(got[name].astype(np.float64) - seq[name])
        excess = float((err / (bar * scales[name] + ulp)).max())
        figs.append(f'{name} {excess:.2g} x (bar {bar:.2g})')
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), excess)
        assert excess <= 1.0, f'{label}: {name} is {excess:.3g} x its bar {bar:.3g} (+ one float32 ulp)'
    if 'frame_ll' in got and 'loglik' in got:   # the float32 frames sum to the float64 total, up to their roundings
        bar = iref.f64_bar(seq['loglik'], joint['loglik'], scales['loglik'])
        slack = np.spacing(np.abs(seq['frame_ll']).astype(np.float32)).astype(np.float64).sum(axis=0)
        assert (np.abs(got['frame_ll'].astype(np.float64).sum(axis=0) - got['loglik']) <=
                bar * scales['loglik'] + slack).all(), f'{label}: frame_ll does not sum to loglik'
    return ', '.join(figs)


# (and the accepted width, odd O past 32 and the smallest odd O, at K = 3: tests/dense_forms.py WIDE_PAIRS)
@pytest.mark.parametrize('D,O,K', general_grid([(1, 1), (2, 3), (3, 4), (6, 12)]))
def test_general_models_against_the_two_float64_forms(D, O, K, set_knob):
    M = stable(dense_case(K, D, O, False, seed=general_seed(D, O, K)))
    worst = {}
    for T in (1, 2, 16, 17, 33, 100):
        y, var = dense_session(M, T, O, seed=T)
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            check_dense(f'D={D} O={O} K={K} T={T} chunk={chunk}', M, y, var, gpu_dense(M, y, var), worst)
    print(f'general D={D} O={O} K={K}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('chunk,T', [('16', 1100), ('32', 2100)])
def test_general_model_spanning_more_than_one_scan_block(chunk, T, set_knob):
    """ceil(T / chunk) > 64 chunks: two blocks of dense_scan_kernel, boundaries through dense_scan_blocks_kernel."""
    set_knob('EKS_DENSE_CHUNK', chunk)
    assert -(-T // int(chunk)) > 64
    M = stable(dense_case(3, 3, 4, False, seed=5))
    y, var = dense_session(M, T, 4, seed=2)
    print(f'T={T} chunk={chunk}: ' + check_dense(f'T={T} chunk={chunk}', M, y, var, gpu_dense(M, y, var)))


@pytest.mark.parametrize('variant', ['unit_root', 'singular_q'])
@pytest.mark.parametrize('D,O', [(2, 3), (3, 4), (6, 12)])
def test_general_model_variants(D, O, variant):
    """A = I, and a rank D-1 Q: nothing is factored, so a singular Q is fine."""
    M = stable(dense_case(3, D, O, variant == 'singular_q', seed=8), unit_root=variant == 'unit_root')
    if variant == 'singular_q':
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    y, var = dense_session(M, 100, O, seed=3)
    print(f'{variant} D={D} O={O}: ' + check_dense(f'{variant} D={D} O={O}', M, y, var, gpu_dense(M, y, var)))


def test_a_diagonal_model_down_the_general_path_agrees_with_the_scalar_path():
    pb = edge_session(100, 5, 2, 2.0, 'decay', seed=6)
    T, K, D = pb['T'], pb['K'], pb['D']
    a = gpu_scalar(pb)
    print('scalar path: ' + check_scalar('scalar path', pb, a))
    y, var = pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D)
    b = gpu_dense(pb['par'], y, var)                                  # no DIAG_MODEL flag: dense_innovations
    check_dense('general path on a diagonal model', pb['par'], y, var, b)
    ref, r32 = scalar_refs(pb)
    ll = a['ll'].reshape(K, D).sum(axis=1)
    bar = max(1e-5, 4 * float(iref.f32_errors(r32, ref)['ll'].max()))
    assert (np.abs(ll - b['loglik']) <= bar * D * np.maximum(np.abs(b['loglik']), T)).all()


# ---- absent outputs, refusals --------------------------------------------------------------------------------------------
def raw_call(dims_args, tensors, outs):
    """eks_innovations itself: tensors = the 8 inputs, y .. s; outs = the 5 outputs or None.  Returns the status."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*dims_args)
    ws = torch.empty(max(int(lib.eks_innovations_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8, device='cuda')
    rc = lib.eks_innovations(ctypes.byref(dims), *[hip_ops._ptr(t) for t in tensors], *[hip_ops._ptr(t) for t in outs],
                             hip_ops._ptr(ws), ws.numel(), hip_ops._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('kind', ['unit', 'decay'])
def test_every_combination_of_absent_outputs_on_scalar_chains_gives_the_same_bits(kind):
    pb = edge_session(161, 21, 3, 2.0, kind, seed=12)
    full = gpu_scalar(pb)
    key = dict(innov='v', innov_var='S', loglik='ll')
    for r in (1, 2):
        for want in itertools.combinations(SCALAR_OUT, r):
            got = gpu_scalar(pb, want=want)
            for n in want:
                assert np.array_equal(got[key[n]], full[key[n]]), (want, n)


def test_every_combination_of_absent_outputs_on_a_general_model_gives_the_same_bits():
    M = stable(dense_case(3, 3, 4, False, seed=3))
    y, var = dense_session(M, 100, 4, seed=1)
    full = gpu_dense(M, y, var)
    for r in (1, 2, 3, 4):
        for want in itertools.combinations(DENSE_OUT, r):
            got = gpu_dense(M, y, var, want=want)
            for n in want:
                assert np.array_equal(got[n], full[n]), (want, n)


def test_refusals_leave_the_outputs_untouched():
    from eks_amd import _lib
    pb = edge_session(100, 3, 2, 2.0, 'unit', seed=2)
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
    dims = (K, T, D, D, diag_flags(pb))
    assert raw_call(dims, ins, [None] * 5) == -1                                     # all NULL
    assert raw_call((K, T, D, D, 0), ins, [None] * 5) == -1                          # and on the general path
    mk = lambda shape, dt=torch.float32: torch.full(shape, 7.0, dtype=dt, device='cuda')
    for with_nis, with_fll in ((True, False), (False, True), (True, True)):
        outs = [mk((T, K, D)), mk((T, K, D)), mk((T, K)) if with_nis else None, mk((T, K)) if with_fll else None,
                mk((K, D), torch.float64)]
        assert raw_call(dims, ins, outs) == _lib.EKS_ERR_UNSUPPORTED                 # nis / frame_ll on scalar chains
        assert all(bool((t == 7.0).all()) for t in outs if t is not None)
    outs = [mk((T, K, D)), mk((T, K, D)), None, None, mk((K, D), torch.float64)]
    assert raw_call(dims, ins, outs) == 0 and not any(bool((t == 7.0).any()) for t in outs if t is not None)


# ---- bits: two calls, a subset of the keypoints, a NaN observation -------------------------------------------------------
@pytest.mark.parametrize('kind', ['unit', 'decay'])
def test_two_calls_and_a_subset_of_the_keypoints_give_the_same_bits(kind):
    """Fixed-order reduction, no floating-point atomics; a chain's outputs depend on the session length alone, so
    keypoints [3, 67) of a K = 70 session called alone (another lane mapping) give the bits of the full call."""
    pb = edge_session(1121, 70, 2, 2.0, kind, seed=21)
    full, again = gpu_scalar(pb), gpu_scalar(pb)
    assert all(np.array_equal(full[k], again[k]) for k in full)
    k0, k1 = 3, 67
    sub = gpu_scalar(subset(pb, k0, k1))
    assert np.array_equal(sub['ll'], full['ll'][2 * k0:2 * k1])
    assert np.array_equal(sub['v'], full['v'][:, 2 * k0:2 * k1]) and np.array_equal(sub['S'], full['S'][:, 2 * k0:2 * k1])
    M = stable(dense_case(3, 3, 4, False, seed=3))
    y, var = dense_session(M, 300, 4, seed=1)
    a, b = gpu_dense(M, y, var), gpu_dense(M, y, var)
    assert all(np.array_equal(a[n], b[n]) for n in a)


def test_a_nan_observation_stays_inside_its_keypoint():
    pb = edge_session(300, 5, 2, 2.0, 'decay', seed=8)
    healthy = gpu_scalar(pb)
    y = pb['y'].copy()
    y[50, 2 * 2] = np.nan                                            # keypoint 2, first coordinate
    sick = gpu_scalar(pb, y=y)
    keep = np.array([n for n in range(10) if n // 2 != 2])
    for k in ('v', 'S', 'll'):
        assert np.array_equal(sick[k][..., keep], healthy[k][..., keep]), k
    assert np.isnan(sick['ll'].reshape(5, 2).sum(axis=1)[2])
    M = stable(dense_case(4, 3, 4, False, seed=4))
    yd, var = dense_session(M, 200, 4, seed=2)
    healthy = gpu_dense(M, yd, var)
    yd = yd.copy()
    yd[70, 1, 2] = np.nan
    sick = gpu_dense(M, yd, var)
    keep = [0, 2, 3]
    for n in DENSE_OUT:
        axis_k = 0 if n == 'loglik' else 1
        assert np.array_equal(np.take(sick[n], keep, axis=axis_k), np.take(healthy[n], keep, axis=axis_k)), n
    assert np.isnan(sick['loglik'][1])


# ---- cross-checks with the EM calls ----------------------------------------------------------------------------------------
def fisher_case():
    M = stable(dense_case(3, 3, 4, False, seed=12))
    y, var = dense_session(M, 400, 4, seed=5)
    return M, y, var


def test_fishers_identity_between_the_device_loglik_and_the_device_statistic():
    """d loglik / d log s by a central difference of eks_innovations' loglik at log s +- 1e-4 against
    (tr(Q^-1 Sw) / s - n) / 2 from eks_em_stats.  Bar: 10 x what the two float64 references give for the same
    comparison on the same inputs (the difference's own truncation and rounding)."""
    from eks_amd import _lib, hip_ops
    M, y, var = fisher_case()
    T, K, O = y.shape
    D = M['m0'].shape[1]
    n, eps, s = D * (T - 1), 1e-4, M['s']
    par = tuple(M[k] for k in ('m0', 'S0', 'A', 'C', 'Q'))
    fd_ref = (em_ref.dense_loglik(y, var, *par, s * np.exp(eps)) - em_ref.dense_loglik(y, var, *par, s * np.exp(-eps))) / (2 * eps)
    val_ref = 0.5 * (em_ref.trace_qinv(M['Q'], em_ref.dense_em_stats(y, var, *par, s)) / s - n)
    bar = 10 * np.abs(fd_ref - val_ref).max()
    up = gpu_dense(M, y, var, want=('loglik',), flags=_lib.FLAG_Q_PD, s=s * np.exp(eps))['loglik']
    dn = gpu_dense(M, y, var, want=('loglik',), flags=_lib.FLAG_Q_PD, s=s * np.exp(-eps))['loglik']
    Sw = hip_ops.em_stats(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), flags=_lib.FLAG_Q_PD).cpu().numpy()
    fd, val = (up - dn) / (2 * eps), 0.5 * (em_ref.trace_qinv(M['Q'], Sw) / s - n)
    print(f'Fisher: device difference {fd}, device statistic {val}; |gap| {np.abs(fd - val).max():.3g}, references '
          f'{np.abs(fd_ref - val_ref).max():.3g}, bar {bar:.3g}')
    assert np.abs(fd - val).max() <= bar


def em_iterates(loop, em_call, n_iters):
    """n_iters x { eks_em_stats at the loop's s -> EmScaleLoop.step() }: the s of every iterate, [n_iters + 1][K]."""
    hist = [loop.s_keypoint.cpu().numpy().copy()]
    for _ in range(n_iters):
        loop.Sw.copy_(em_call(loop.s_keypoint))
        loop.step()
        torch.cuda.synchronize()
        hist.append(loop.s_keypoint.cpu().numpy().copy())
    return hist


@pytest.mark.parametrize('kind', ['unit', 'decay'])
def test_device_loglik_never_drops_along_the_scale_loop_on_scalar_chains(kind):
    from eks_amd import hip_ops
    pb = edge_session(600, 5, 2, 2.0, kind, seed=31)
    T, K, D = pb['T'], pb['K'], pb['D']
    yv = (_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)))
    par = [_dev(pb['par'][k]) for k in ('m0', 'S0', 'A', 'C', 'Q')]
    loop = make_loop(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), pb['par'], diag_flags(pb),
                     [[k] for k in range(K)], np.zeros(K), -8.0, 8.0, 0.0, 12)
    hist = em_iterates(loop, lambda s: hip_ops.em_stats(*yv, *par, s, flags=diag_flags(pb), vs_diag=True), 12)
    ll = np.array([gpu_scalar(pb, want=('loglik',), s=s)['ll'].reshape(K, D).sum(axis=1) for s in hist])
    bar = 1e-5 * np.maximum(np.abs(ll[:-1]), T)
    print(f'scalar loop {kind}: loglik {ll[0]} -> {ll[-1]}; smallest change {np.diff(ll, axis=0).min():.3g}')
    assert (np.diff(ll, axis=0) >= -bar).all() and (ll[-1] > ll[0]).all()


def test_device_loglik_never_drops_along_the_scale_loop_on_a_general_model():
    from eks_amd import _lib, hip_ops
    M, y, var = fisher_case()
    T, K, O = y.shape
    dev = [_dev(y), _dev(var)] + [_dev(M[k]) for k in ('m0', 'S0', 'A', 'C', 'Q')]
    loop = make_loop(y, var, M, _lib.FLAG_Q_PD, [[k] for k in range(K)], np.zeros(K), -8.0, 8.0, 0.0, 12)
    hist = em_iterates(loop, lambda s: hip_ops.em_stats(*dev, s, flags=_lib.FLAG_Q_PD), 12)
    ll = np.array([gpu_dense(M, y, var, want=('loglik',), flags=_lib.FLAG_Q_PD, s=s)['loglik'] for s in hist])
    par = tuple(M[k] for k in ('m0', 'S0', 'A', 'C', 'Q'))
    s0 = np.ones(K)
    scale = np.maximum(np.abs(ll[:-1]), T * O)
    bar = iref.f64_bar(iref.dense_innovations_sequential(y, var, *par, s0)['loglik'],
                       iref.dense_innovations_joint(y, var, *par, s0)['loglik'], scale[0])
    print(f'dense loop: loglik {ll[0]} -> {ll[-1]}; smallest change {np.diff(ll, axis=0).min():.3g}; bar {bar:.3g}')
    assert (np.diff(ll, axis=0) >= -bar * scale).all() and (ll[-1] > ll[0]).all()


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def numpy_summary(fi):
    z = (fi.innov / np.sqrt(fi.innov_var)).astype(np.float64)
    out = []
    for k in range(z.shape[0]):
        out.append(dict(mean_nis_per_dim=float(fi.nis[k].astype(np.float64).mean() / z.shape[2]),
                        lag1_autocorr=iref.lag1_autocorr(z[k]), frac_beyond_3=float((np.abs(z[k]) > 3).mean())))
    return out


@pytest.mark.parametrize('model', ['scalar', 'general'])
def test_filter_innovations_log_likelihood_and_summary(model):
    from eks_amd import diagnostics as dg
    if model == 'scalar':
        pb = edge_session(500, 4, 2, 2.0, 'decay', seed=3)
        T, K, O = pb['T'], pb['K'], pb['D']
        M, y, var = pb['par'], pb['y'].reshape(T, K, O), pb['var'].reshape(T, K, O)
    else:
        M = stable(dense_case(3, 3, 4, False, seed=7))
        y, var = dense_session(M, 500, 4, seed=4)
        T, K, O = y.shape
    args = (np.swapaxes(y, 0, 1), M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'])
    fi = dg.filter_innovations(*args)
    assert fi.innov.shape == fi.innov_var.shape == (K, T, O) and fi.nis.shape == fi.frame_loglik.shape == (K, T)
    assert all(a.dtype == np.float32 for a in fi[:4]) and fi.loglik.dtype == np.float64 and fi.loglik.shape == (K,)
    ref = iref.dense_innovations_sequential(y, var, *(M[k] for k in PARAMS))
    tol = 1e-5 if model == 'scalar' else 1e-6
    assert np.abs(np.swapaxes(fi.nis, 0, 1) - ref['nis']).max() <= 10 * tol * np.abs(ref['nis']).max()
    assert np.abs(np.swapaxes(fi.frame_loglik, 0, 1) - ref['frame_ll']).max() <= 10 * tol * np.abs(ref['frame_ll']).max()
    assert (np.abs(fi.loglik - ref['loglik']) <= tol * O * np.maximum(np.abs(ref['loglik']), T)).all()
    assert np.array_equal(dg.log_likelihood(*args), fi.loglik)
    dev = dg.filter_innovations(*args, return_device=True)
    assert dev.innov.is_cuda and tuple(dev.nis.shape) == (K, T) and dev.loglik.dtype == torch.float64
    assert np.array_equal(dev.innov.cpu().numpy(), fi.innov) and np.array_equal(dev.loglik.cpu().numpy(), fi.loglik)
    assert dg.log_likelihood(*args, return_device=True).is_cuda
    got, want = dg.innovation_summary(*args), numpy_summary(fi)
    assert len(got) == K
    for g, w in zip(got, want):
        assert abs(g['mean_nis_per_dim'] - w['mean_nis_per_dim']) <= 1e-5 * w['mean_nis_per_dim']
        assert g['lag1_autocorr'].shape == (O,) and np.abs(g['lag1_autocorr'] - w['lag1_autocorr']).max() <= 1e-5
        assert abs(g['frac_beyond_3'] - w['frac_beyond_3']) <= 1.5 / (T * O)
    print(f'{model}: summary of keypoint 0 {got[0]}')


def test_innovations_singlecam_on_the_golden_markers(golden_dir):
    from eks_amd.core import ensemble
    from eks_amd.diagnostics import innovations_singlecam
    from eks_amd.marker_array import MarkerArray
    from eks_amd.singlecam_smoother import ensemble_kalman_smoother_singlecam, initialize_kalman_filter
    from eks_amd.utils import center_predictions
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers']
    names = [str(k) for k in g['keypoints']]
    M_, V, T, K, _ = mk.shape
    ma = MarkerArray(mk.astype(np.float64), data_fields=['x', 'y', 'likelihood'])
    _, s = ensemble_kalman_smoother_singlecam(ma, names, smooth_param=10.0)
    res = innovations_singlecam(ma, names, s)
    assert res['z'].shape == (T, K, 2) and res['nis'].shape == (T, K) and res['loglik'].shape == (K,)
    assert res['z'].dtype == np.float32 and res['nis'].dtype == np.float32 and res['loglik'].dtype == np.float64
    # the reference fed the same centred ensemble
    ens = ensemble(ma, avg_mode='median', var_mode='confidence_weighted_var')
    _, centered, _, _ = center_predictions(ens, quantile_keep_pca=100)
    m0s, S0s, As, Qs, Cs = initialize_kalman_filter(centered)
    cen = np.asarray(centered.array)[0, 0].astype(np.float32)                       # (T, K, 2), as the device sees it
    var = np.asarray(ens.array)[0, 0][:, :, 2:4].astype(np.float32)
    dg = lambda A: np.diagonal(np.asarray(A, np.float64), axis1=1, axis2=2).reshape(-1)
    qs = np.repeat(np.broadcast_to(np.asarray(s, np.float64), (K,)), 2) * dg(Qs)
    args = (cen.reshape(T, 2 * K), var.reshape(T, 2 * K), np.asarray(m0s, np.float64).reshape(-1), dg(S0s), dg(As),
            dg(Cs), qs)
    v, S, ll = iref.scalar_innovations(*args)
    v32, S32, ll32 = iref.scalar_innovations_f32(*args, unit=bool((dg(As) == 1).all() and (dg(Cs) == 1).all()))
    ref = dict(v=v, S=S, ll=ll, y=cen.reshape(T, 2 * K).astype(np.float64))
    et = iref.f32_errors(dict(v=v32, S=S32, ll=ll32), ref)
    bar = {k: max(1e-5, 4 * float(e.max())) for k, e in et.items()}
    z = v / np.sqrt(S)
    ymax = np.abs(ref['y']).max(axis=0)
    # z = v / sqrt(S): the bars of v and S carried through, plus the roundings of the quotient and the root
    z_bar = bar['v'] * ymax / np.sqrt(S) + np.abs(z) * (0.5 * bar['S'] + 4 * 2.0 ** -24)
    assert (np.abs(res['z'].reshape(T, 2 * K) - z) <= z_bar).all()
    nis = (z * z).reshape(T, K, 2).sum(axis=2)
    nis_bar = (2 * np.abs(z) * z_bar + z_bar ** 2).reshape(T, K, 2).sum(axis=2) + 4 * 2.0 ** -24 * nis
    assert (np.abs(res['nis'] - nis) <= nis_bar).all()
    llk = ll.reshape(K, 2).sum(axis=1)
    assert (np.abs(res['loglik'] - llk) <= bar['ll'] * np.maximum(np.abs(ll), T).reshape(K, 2).sum(axis=1)).all()
    print(f'golden single-camera markers: loglik {res["loglik"]}, mean nis / 2 {res["nis"].mean(axis=0) / 2}')
