"""GPU: eks_em_stats, eks_em_scale_step / eks_em_scale_run (eks_amd/csrc/eks_em.hip on scalar chains, dense_em in
eks_dense.hip on general models) and eks_amd.em against the float64 references of tests/em_ref.py.

Bars.  Scalar chains (float32 filter and RTS step, float64 sum): per chain, |Sw - reference| / reference <=
max(1e-5, 4 x the float32 NumPy transcription's own worst relative error on the chains of the case) - the project's
rule, em_ref.bar_excess; log s of the loop by the same rule on |log s - reference|, with the transcription run through
the same loop.  General models (float64 in the lane, float64 out): the worst |Sw - reference| as a fraction of the
keypoint's largest |Sw| entry, MEASURED on the MI355X and recorded below, bar = 100 x that and in no case looser than
1e-8 (a figure near 1e-7 means a float32 value leaked into the sum); log s of the dense loop likewise.  Nothing is
compared with the kernels' own output, except where the test is about bits (determinism, subsets, the stopped loop).

Measured on the MI355X.  Scalar chains, kernels (transcription), relative: edge shapes within the rule everywhere,
e.g. N = 1 at T = 1 121, s = 300: 5.5e-8 (1.2e-8); extreme variances 1.5e-7 (8.4e-8) unit, 7.2e-8 (7.8e-8) decaying;
log s after 12 iterations 2.1e-7 (3.9e-8) unit, 8.9e-8 (1.3e-7) decaying; blocks of 2 and 3: 3.0e-8 (8.4e-8), with a
start outside the bounds 4.6e-8 (8.3e-8).  General models: Sw within 1.3e-14 of the keypoint's largest entry (rank D-1
Q; 3.2e-15 otherwise), log s of the dense loop within 6.8e-14.  The float64 log-likelihood along 15 GPU iterations never
dropped (worst relative change +2.2e-12, a gain).  refine_smooth_param_em from the Adam result on 2 000 x 6 x 2
(simulated at s = 2): Adam's constant-R optimum 2.76 .. 3.24, EM 1.98 .. 2.10 after 22 - 23 iterations, log-likelihood
gain 28 .. 63 per keypoint, |tr(Q^-1 Sw) / (s n) - 1| <= 6.7e-5 at tol = 1e-4.  DESIGN.md 9e has the table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402
from test_gpu_increments import PARAMS, _dev, dense_session, diag_flags, edge_session, stable  # noqa: E402
from dense_forms import general_grid, general_seed  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

# General models, measured on the MI355X (worst over every case of this file): Sw within 1.3e-14 of the keypoint's
# largest |Sw| entry (the rank D-1 Q; 3.2e-15 elsewhere), log s after 12 iterations of the dense loop within 6.8e-14.
# Bars: 100 x the measured figure (the cap of 1e-8 is four decades above both).
MEASURED = dict(dense_sw=1.3e-14, dense_log_s=6.8e-14)
DENSE_SW_BAR = min(100 * MEASURED['dense_sw'], 1e-8)
DENSE_LOG_S_BAR = min(100 * MEASURED['dense_log_s'], 1e-8)

T_EDGES = (1, 2, 3, 31, 32, 33, 64, 65, 129, 289, 1121)   # chunk edges; ceil(sqrt(nc)) changes at nc = 2, 5, 10, 36


def gpu_scalar(pb, s=None, y=None):
    """hip_ops.em_stats on the chains of make_session -> (N,) float64."""
    from eks_amd import hip_ops
    T, K, D = pb['T'], pb['K'], pb['D']
    par = dict(pb['par'])
    if s is not None:
        par['s'] = np.asarray(s, np.float64)
    Sw = hip_ops.em_stats(_dev((pb['y'] if y is None else y).reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)),
                          *(_dev(par[k]) for k in PARAMS), flags=diag_flags(pb), vs_diag=True)
    torch.cuda.synchronize()
    assert Sw.dtype == torch.float64 and tuple(Sw.shape) == (K, D)
    return Sw.cpu().numpy().reshape(K * D)


def scalar_refs(pb):
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    return em_ref.scalar_em_stats(*args), em_ref.scalar_em_stats_f32(*args, unit=pb['unit'])


def check_scalar(label, pb, got):
    assert np.isfinite(got).all()
    if pb['T'] == 1:
        assert not got.any(), f'{label}: T = 1 must give exact zeros'
        return 'zeros'
    r64, r32 = scalar_refs(pb)
    excess, err, trans = em_ref.bar_excess(got, r64, r32)
    assert excess <= 1.0, f'{label}: Sw is {excess:.3g} x its bar; relative {err:.3g} (transcription {trans:.3g})'
    return f'Sw {err:.3g} ({trans:.3g})'


@pytest.mark.parametrize('kind', ['unit', 'decay', 'flip'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 1), (3, 2), (21, 3), (65, 1), (65, 2)])
def test_scalar_chain_edge_shapes(K, D, kind):
    worst, figs = 0.0, ''
    for T in T_EDGES:
        for sval in (1e-4, 2.0, 300.0):
            pb = edge_session(T, K, D, sval, kind, seed=T + K)
            figs = check_scalar(f'N={K * D} D={D} T={T} s={sval} {kind}', pb, gpu_scalar(pb))
    print(f'N={K * D} D={D} {kind}, last case kernels (transcription): {figs}')


def test_scalar_chains_with_extreme_variances():
    """Variances at the 1e-12 floor, at 1e30 and at inf (both meet the clip at 1e30): the per-chain bar only."""
    for unit in (True, False):
        pb = make_session(129, 3, 2, 2.0, unit, seed=4, centre=0.0)
        pb['var'][7, 0] = 1e-12
        pb['var'][40, 1] = 1e30
        pb['var'][41, 1] = np.inf
        pb['var'][64, 2] = np.inf
        pb['var'][128, 3] = 1e-12
        pb['var'][0, 4] = np.inf
        print(f'extreme variances unit={unit}: ' + check_scalar('extreme variances', pb, gpu_scalar(pb)))


def subset(pb, k0, k1):
    D = pb['D']
    sub = dict(pb, K=k1 - k0, N=(k1 - k0) * D)
    T = pb['T']
    for key in ('y', 'var'):
        sub[key] = np.ascontiguousarray(pb[key].reshape(T, pb['K'], D)[:, k0:k1].reshape(T, -1))
    sub['par'] = {k: np.ascontiguousarray(v[k0:k1]) for k, v in pb['par'].items()}
    return sub


@pytest.mark.parametrize('kind', ['unit', 'decay'])
def test_two_calls_and_a_subset_of_the_keypoints_give_the_same_bits(kind):
    """Fixed-order reduction, no floating-point atomics; a chain's sum depends on the session length alone, so
    keypoints [k0, k1) of a K = 70 session called alone (another lane mapping: 128 and 14 .. 60 chains) give the bits
    of the full call."""
    pb = edge_session(1121, 70, 2, 2.0, kind, seed=21)
    full = gpu_scalar(pb)
    assert np.array_equal(full, gpu_scalar(pb))
    for k0, k1 in ((0, 7), (33, 63), (69, 70), (5, 70)):
        assert np.array_equal(gpu_scalar(subset(pb, k0, k1)), full[2 * k0:2 * k1]), (k0, k1)
    M = stable(dense_case(3, 3, 4, False, seed=3))
    y, var = dense_session(M, 300, 4, seed=1)
    assert np.array_equal(gpu_dense(M, y, var, False), gpu_dense(M, y, var, False))


# ---- general models -------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, vs_diag, flags=0):
    from eks_amd import hip_ops
    Sw = hip_ops.em_stats(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), flags=flags, vs_diag=vs_diag)
    torch.cuda.synchronize()
    K, D = M['m0'].shape
    assert Sw.dtype == torch.float64 and tuple(Sw.shape) == ((K, D) if vs_diag else (K, D, D))
    return Sw.cpu().numpy()


def check_dense(label, M, y, var, got, vs_diag):
    ref = em_ref.dense_em_stats(y, var, *(M[k] for k in PARAMS))
    if y.shape[0] == 1:
        assert not got.any(), f'{label}: T = 1 must give exact zeros'
        return 0.0
    K = ref.shape[0]
    scale = np.abs(ref).reshape(K, -1).max(axis=1)
    want = np.diagonal(ref, axis1=1, axis2=2) if vs_diag else ref
    assert np.isfinite(got).all()
    err = float((np.abs(got - want).reshape(K, -1).max(axis=1) / scale).max())
    print(f'{label}: Sw {err:.3g} of the keypoint\'s largest entry')
    assert err <= DENSE_SW_BAR, f'{label}: Sw {err:.3g} against the bar {DENSE_SW_BAR:.3g}'
    return err


# (and the accepted width, odd O past 32 and the smallest odd O, at K = 3: tests/dense_forms.py WIDE_PAIRS)
@pytest.mark.parametrize('D,O,K', general_grid([(1, 1), (3, 4), (6, 12)]))
def test_general_models_against_the_dense_reference(D, O, K, set_knob):
    M = stable(dense_case(K, D, O, False, seed=general_seed(D, O, K)))
    worst = 0.0
    for i, T in enumerate((1, 2, 15, 16, 17, 33, 100)):
        y, var = dense_session(M, T, O, seed=T)
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            vs_diag = bool((i + int(chunk) // 16) % 2)
            worst = max(worst, check_dense(f'D={D} O={O} K={K} T={T} chunk={chunk} vs_diag={vs_diag}', M, y, var,
                                           gpu_dense(M, y, var, vs_diag), vs_diag))
    print(f'general D={D} O={O} K={K}: worst {worst:.3g}')


@pytest.mark.parametrize('chunk,T', [('16', 1100), ('32', 2100)])
def test_general_model_spanning_more_than_one_scan_block(chunk, T, set_knob):
    """ceil(T / chunk) > 64 chunks: two blocks of dense_scan_kernel, boundaries through dense_scan_blocks_kernel."""
    set_knob('EKS_DENSE_CHUNK', chunk)
    assert -(-T // int(chunk)) > 64
    M = stable(dense_case(3, 3, 4, False, seed=5))
    y, var = dense_session(M, T, 4, seed=2)
    check_dense(f'T={T} chunk={chunk}', M, y, var, gpu_dense(M, y, var, False), False)


@pytest.mark.parametrize('variant', ['unit_root', 'singular_q'])
@pytest.mark.parametrize('vs_diag', [False, True])
def test_general_model_variants(variant, vs_diag):
    K, D, O, T = 3, 3, 4, 100
    M = stable(dense_case(K, D, O, variant == 'singular_q', seed=8), unit_root=variant == 'unit_root')
    if variant == 'singular_q':
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    y, var = dense_session(M, T, O, seed=3)
    got = gpu_dense(M, y, var, vs_diag)
    check_dense(f'{variant} vs_diag={vs_diag}', M, y, var, got, vs_diag)
    if not vs_diag:
        assert np.abs(got - np.swapaxes(got, 1, 2)).max() <= 1e-12 * np.abs(got).max()


def test_a_diagonal_model_down_the_general_path_agrees_with_the_scalar_path():
    pb = edge_session(100, 5, 2, 2.0, 'decay', seed=6)
    T, K, D = pb['T'], pb['K'], pb['D']
    a = gpu_scalar(pb)
    M = pb['par']
    y, var = pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D)
    b = gpu_dense(M, y, var, True)                                # no DIAG_MODEL flag: dense_em, diagonals
    print('scalar path: ' + check_scalar('scalar path', pb, a))
    check_dense('general path on a diagonal model', M, y, var, b, True)
    full = gpu_dense(M, y, var, False)
    assert np.array_equal(np.diagonal(full, axis1=1, axis2=2), b)
    # (the full statistic of independent chains is NOT diagonal: E[w_a w_b | y] = E w_a E w_b; the scalar path leaves
    #  those sums out because a diagonal Q's M-step never reads them)
    check_dense('general path on a diagonal model, full', M, y, var, full, False)
    r64, r32 = scalar_refs(pb)
    assert np.abs(a / b.reshape(-1) - 1).max() <= max(1e-5, 4 * float(np.abs(r32 / r64 - 1).max()))


# ---- the loop -----------------------------------------------------------------------------------------------------------
def make_loop(y, var, M, flags, blocks, log_s0, lo, hi, tol, max_iters):
    """hip_ops.EmScaleLoop on frame-major (T, K, O) arrays; blocks: lists of keypoints."""
    from eks_amd import hip_ops
    K = M['m0'].shape[0]
    offs = np.zeros(len(blocks) + 1, np.int32)
    offs[1:] = np.cumsum([len(b) for b in blocks])
    members = np.concatenate([np.asarray(b, np.int32) for b in blocks])
    state = np.zeros((len(blocks), 4))
    state[:, 0] = log_s0
    s_k = np.empty(K)
    for b, mem in enumerate(blocks):
        s_k[list(mem)] = np.exp(log_s0[b])
    return hip_ops.EmScaleLoop(_dev(y), _dev(var), *(_dev(M[k]) for k in ('m0', 'S0', 'A', 'C', 'Q')), _dev(offs),
                               _dev(members), _dev(state), _dev(s_k), lo, hi, tol, max_iters, flags=flags)


def scalar_loop_problem(T, K, kind, seed, sval=2.0):
    pb = edge_session(T, K, 2, sval, kind, seed)
    q = np.diagonal(pb['par']['Q'], axis1=1, axis2=2).reshape(-1).copy()
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], q, 2)
    return pb, q, args


def run_scalar_loop(pb, blocks, log_s0, lo, hi, tol, max_iters, n_iters):
    T, K, D = pb['T'], pb['K'], pb['D']
    loop = make_loop(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), pb['par'], diag_flags(pb), blocks, log_s0, lo,
                     hi, tol, max_iters)
    loop.run(n_iters)
    torch.cuda.synchronize()
    return loop


@pytest.mark.parametrize('kind', ['unit', 'decay'])
def test_scalar_loop_after_exactly_twelve_iterations(kind):
    pb, q, args = scalar_loop_problem(600, 5, kind, seed=31)
    blocks = [[k] for k in range(5)]
    n = 2 * 599
    h64, _, _ = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args), n, np.zeros(5), blocks, -8, 8, 0.0, 12, 12)
    h32, _, _ = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args, stats=em_ref.scalar_em_stats_f32, unit=pb['unit']), n,
                                     np.zeros(5), blocks, -8, 8, 0.0, 12, 12)
    loop = run_scalar_loop(pb, blocks, np.zeros(5), -8.0, 8.0, 0.0, 12, 12)
    st = loop.state.cpu().numpy()
    err, trans = np.abs(st[:, 0] - h64[-1]).max(), np.abs(h32[-1] - h64[-1]).max()
    print(f'scalar loop {kind}: log s after 12 iterations {err:.3g} (transcription loop {trans:.3g})')
    assert err <= max(1e-5, 4 * trans)
    assert (st[:, 2] == 12).all() and not st[:, 3].any() and int(loop.n_active.item()) == 0   # all at max_iters
    assert np.array_equal(loop.s_keypoint.cpu().numpy(), np.exp(st[:, 0]))
    assert np.abs(st[:, 1] - np.abs(h64[-1] - h64[-2])).max() <= max(1e-5, 4 * trans)


def test_dense_loop_after_exactly_twelve_iterations():
    from eks_amd import _lib
    M = stable(dense_case(3, 3, 4, False, seed=12))
    y, var = dense_session(M, 400, 4, seed=5)
    blocks = [[k] for k in range(3)]
    h64, _, _ = em_ref.em_scale_loop(em_ref.dense_trace_fn(y, var, *(M[k] for k in ('m0', 'S0', 'A', 'C', 'Q'))), 3 * 399,
                                     np.zeros(3), blocks, -8, 8, 0.0, 12, 12)
    loop = make_loop(y, var, M, _lib.FLAG_Q_PD, blocks, np.zeros(3), -8.0, 8.0, 0.0, 12)
    loop.run(12)
    torch.cuda.synchronize()
    st = loop.state.cpu().numpy()
    err = np.abs(st[:, 0] - h64[-1]).max()
    print(f'dense loop: log s after 12 iterations {err:.3g}; log s {st[:, 0]}')
    assert err <= DENSE_LOG_S_BAR
    assert (st[:, 2] == 12).all() and tuple(loop.Sw.shape) == (3, 3, 3)


def test_stop_rule_same_iteration_as_the_reference_and_nothing_moves_afterwards():
    """Seed chosen on the CPU: the float64 |delta log s| sequences of the three blocks cross tol = 1e-3 with no value
    within 10 % of it (asserted here from the reference alone), so float32's 1e-6 cannot move a stopping iteration."""
    pb, q, args = scalar_loop_problem(600, 3, 'unit', seed=117)
    blocks = [[k] for k in range(3)]
    tol = 1e-3
    _, deltas, ref = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args), 2 * 599, np.zeros(3), blocks, -8, 8, tol, 60, 60)
    d = deltas[~np.isnan(deltas)]
    assert ref['done'].all() and np.abs(d / tol - 1).min() > 0.10 and len(set(ref['iters'])) > 1
    loop = run_scalar_loop(pb, blocks, np.zeros(3), -8.0, 8.0, tol, 60, int(ref['iters'].max()) - 1)
    assert int(loop.n_active.item()) > 0                       # the slowest block is still running
    loop.run(1)
    torch.cuda.synchronize()
    st = loop.state.cpu().numpy()
    assert np.array_equal(st[:, 2].astype(int), ref['iters']) and (st[:, 3] == 1).all()
    assert int(loop.n_active.item()) == 0
    s_before, st_before = loop.s_keypoint.cpu().numpy(), st.copy()
    loop.run(5)
    torch.cuda.synchronize()
    assert np.array_equal(loop.s_keypoint.cpu().numpy(), s_before)          # bit for bit
    assert np.array_equal(loop.state.cpu().numpy(), st_before) and int(loop.n_active.item()) == 0


def test_blocks_of_two_and_three_keypoints_and_a_start_outside_the_bounds():
    pb, q, args = scalar_loop_problem(600, 5, 'decay', seed=33)
    blocks = [[0, 3], [1, 2, 4]]
    n = 2 * 599
    for log_s0, lo, hi, iters in ((np.log([0.5, 3.0]), -8.0, 8.0, 6), (np.array([2.0, -3.0]), -1.0, 0.5, 4)):
        h64, _, _ = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args), n, log_s0, blocks, lo, hi, 0.0, iters, iters)
        h32, _, _ = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args, stats=em_ref.scalar_em_stats_f32, unit=False), n,
                                         log_s0, blocks, lo, hi, 0.0, iters, iters)
        loop = run_scalar_loop(pb, blocks, log_s0, lo, hi, 0.0, iters, iters)
        st = loop.state.cpu().numpy()
        err, trans = np.abs(st[:, 0] - h64[-1]).max(), np.abs(h32[-1] - h64[-1]).max()
        print(f'blocks {blocks} bounds ({lo}, {hi}): log s {st[:, 0]} error {err:.3g} (transcription loop {trans:.3g})')
        assert err <= max(1e-5, 4 * trans)
        assert (st[:, 0] >= lo).all() and (st[:, 0] <= hi).all()
        s_k = loop.s_keypoint.cpu().numpy()
        for b, mem in enumerate(blocks):
            assert (s_k[mem] == np.exp(st[b, 0])).all()


def test_loglik_of_the_reference_never_decreases_along_the_gpu_iterates():
    pb, q, args = scalar_loop_problem(600, 5, 'decay', seed=35)
    blocks = [[k] for k in range(5)]
    loop = run_scalar_loop(pb, blocks, np.zeros(5), -8.0, 8.0, 0.0, 15, 0)

    def loglik(s_k):
        ll = em_ref.scalar_loglik(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], np.repeat(s_k, 2) * q)
        return ll.reshape(5, 2).sum(axis=1)
    lls = [loglik(loop.s_keypoint.cpu().numpy())]
    for _ in range(15):
        loop.run(1)                                             # one call per iteration
        torch.cuda.synchronize()
        lls.append(loglik(loop.s_keypoint.cpu().numpy()))
    lls = np.array(lls)
    drop = (lls[:-1] - lls[1:]) / np.abs(lls[:-1])
    print(f'log-likelihood along 15 GPU iterations: total gain {lls[-1] - lls[0]}, worst relative drop {drop.max():.3g}')
    assert (drop <= 1e-6).all() and (lls[-1] > lls[0]).all()


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_refine_smooth_param_em_from_the_adam_result():
    from eks_amd import em
    from eks_amd.core import run_kalman_smoother
    T, K, D = 2000, 6, 2
    pb = make_session(T, K, D, 2.0, True, seed=41, centre=3.0)
    par = pb['par']
    ys = np.ascontiguousarray(np.swapaxes(pb['y'].reshape(T, K, D), 0, 1))
    ev = pb['var'].reshape(T, K, D)
    args = (ys, par['m0'], par['S0'], par['A'], par['C'], par['Q'], ev)
    s_adam = run_kalman_smoother(*args)[0]
    tol = 1e-4
    s_em, info = em.refine_smooth_param_em(*args, s_adam, tol=tol, return_info=True)
    assert s_em.shape == (K,) and s_em.dtype == np.float64 and info['done'].all() and (info['iterations'] <= 100).all()

    def loglik(s_k):
        ll = em_ref.scalar_loglik(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], np.repeat(s_k, D))
        return ll.reshape(K, D).sum(axis=1)
    l0, l1 = loglik(s_adam), loglik(s_em)
    print(f'Adam s {s_adam}\nEM s {s_em} after {info["iterations"]} iterations\nlog-likelihood gain {l1 - l0}')
    assert (l1 >= l0).all()
    Sw, n = em.process_noise_statistics(*args, s_em)
    assert Sw.shape == (K, D, D) and Sw.dtype == np.float64 and n == D * (T - 1)
    ratio = np.trace(np.linalg.solve(par['Q'], Sw), axis1=1, axis2=2) / (s_em * n)
    print(f'tr(Q^-1 Sw) / (s n) - 1: {ratio - 1}')
    assert (np.abs(ratio - 1) < tol).all()
    Sd, _ = em.process_noise_statistics(*args, s_em, return_device=True)
    assert Sd.is_cuda and np.array_equal(Sd.cpu().numpy(), Sw)
    with pytest.raises(NotImplementedError):
        em.refine_smooth_param_em(*args, s_adam, h_fn=lambda x: x)


def test_fit_process_noise_em_on_a_general_model():
    from eks_amd import em
    K, D, O, T = 3, 3, 4, 400
    M = stable(dense_case(K, D, O, False, seed=14))
    M['s'] = np.ones(K)
    y, var = dense_session(M, T, O, seed=7)                       # simulated with the known Q at s = 1
    ys = np.ascontiguousarray(np.swapaxes(y, 0, 1))
    base = (ys, M['m0'], M['S0'], M['A'], M['C'])

    def loglik(Q):
        return em_ref.dense_loglik(y, var, M['m0'], M['S0'], M['A'], M['C'], Q, 1.0)
    Q = np.tile(np.eye(D), (K, 1, 1)) * 3.0
    lls = [loglik(Q)]
    for _ in range(8):
        Q = em.fit_process_noise_em(*base, Q, var, max_iters=1, tol=0.0)
        assert Q.shape == (K, D, D) and np.array_equal(Q, np.swapaxes(Q, 1, 2)) and np.linalg.eigvalsh(Q).min() > 0
        lls.append(loglik(Q))
    lls = np.array(lls)
    assert (np.diff(lls, axis=0) >= -1e-9 * np.abs(lls[:-1])).all() and (lls[-1] > lls[0]).all()
    Qf = em.fit_process_noise_em(*base, np.tile(np.eye(D), (K, 1, 1)) * 3.0, var)
    assert np.array_equal(Qf, np.swapaxes(Qf, 1, 2)) and np.linalg.eigvalsh(Qf).min() > 0
    assert (loglik(Qf) >= lls[-1] - 1e-9 * np.abs(lls[-1])).all()
    print(f'full-Q EM: log-likelihood {lls[0]} -> {lls[-1]} -> {loglik(Qf)}; Q[0] diagonal {np.diag(Qf[0])} '
          f'(simulated with {np.diag(M["Q"][0])})')
    # scalar chains keep Q diagonal
    pb = make_session(300, 2, 2, 2.0, False, seed=43, centre=3.0)
    par = pb['par']
    Qd = em.fit_process_noise_em(np.ascontiguousarray(np.swapaxes(pb['y'].reshape(300, 2, 2), 0, 1)), par['m0'], par['S0'],
                                 par['A'], par['C'], par['Q'], pb['var'].reshape(300, 2, 2), max_iters=5)
    assert not (Qd * (1 - np.eye(2))).any() and (np.diagonal(Qd, axis1=1, axis2=2) > 0).all()
