"""GPU: every kernel form of the pupil loss and optimiser (eks_ar1_nll, eks_pupil_adam_step, eks_pupil_adam_run) at
the sizes that select it, against float64 references that never touch the kernels.

Which kernel runs depends on the shape (eks_dense_wave.hip dense_wave_run, eks_loss_kernels.hpp loss_launch):
  wave  (EKS_FLAG_Q_PD, D = 3, O = 8, at most 1024 (chain, 64-chunk) units): dw_summarize / dw_replay MODE 2 with
        2, 4 or 8 frames per lane, four-wave workgroups above 256 units, then dw_ar1_finish_kernel or, inside
        eks_pupil_adam_run with at most 64 chains, dw_ar1_finish_step_kernel;
  dual  (everything else): dual-number elements through loss_chunks_kernel and up to two loss_reduce_kernel levels.
Every case asserts the form it is about - profile scopes for wave / dual, EKS_DW_CHUNK or a mirror of the host's
choice for the chunk length and the unit count - so that a moved threshold cannot turn it into a duplicate.

References: the pupil shape from orc.pupil_nll_and_grad(use_c=True) per chain (complex-step C filter); general
(D, O) and arbitrary tangents from ar1_basis() + combine() below (the derivative is linear in (da, dq): the 2 D
basis directions once per chain); the optimiser from pupil_trajectory(), a restatement of
orc.pupil_optimize_smooth's loop that records every iteration.  tests/test_pupil_cpu.py checks these helpers.

Bars (tests/test_gpu_pupil.py): |nll - L| < 1e-9 max(|L|, 1); gradients rtol 1e-8, atol 1e-9 max|g|; iteration
counts and done flags exact; u after a run rtol 1e-9.  Every check prints its worst figures before it asserts."""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import c_oracle
from oracle import eks_oracle as orc

pytestmark = pytest.mark.gpu

US = [(4.6, 3.9), (0.5, -1.0), (-2.0, 6.0)]
EKS_ERR_UNSUPPORTED = -3


# ---------------------------------------------------------------------------------------------
# references (float64, CPU)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain(T, seed, floor=True):
    """One synthetic pupil chain (ys, ev, m0, S0, lv), float32-rounded observations, S0's diagonal and the latent
    variances floored at 0.3 (the optimiser's chains: as drawn); shared between cases, read-only."""
    from eks_amd import synth
    ys, ev, m0, S0, lv = synth.pupil_observations(T, seed)
    if floor:
        S0 = S0.copy()
        S0[np.diag_indices(3)] = np.maximum(np.diag(S0), 0.3)
        lv = np.maximum(lv, 0.3)
    out = (ys, ev, m0, S0, lv)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pupil_ref(T, seed, u):
    ys, ev, m0, S0, lv = chain(T, seed)
    L, g = orc.pupil_nll_and_grad(np.asarray(u, np.float64), ys, m0, S0, orc.PUPIL_C, ev, lv, use_c=True)
    return float(L), np.asarray(g)


def pupil_params(u, lv):
    """a, q (3,) and the two tangents da, dq (2, 3) of the pupil's parametrisation at u."""
    s, ds = orc.pupil_to_stable_s(np.asarray(u, np.float64))
    a = np.array([s[0], s[1], s[1]])
    q = lv * (1 - a * a)
    da = np.array([[ds[0], 0, 0], [0, ds[1], ds[1]]])
    dq = np.array([[-2 * s[0] * ds[0] * lv[0], 0, 0], [0, -2 * s[1] * ds[1] * lv[1], -2 * s[1] * ds[1] * lv[2]]])
    return a, q, da, dq


def ar1_basis(y, var, m0, S0, C, a, q, use_c=None):
    """One chain of the AR(1) model A = diag(a), Q = diag(q), R_t = diag(max(var, 1e-12)): (nll, d nll / d a (D,),
    d nll / d q (D,)).  The C oracle's complex-step filter for O <= 16 (its limit), the NumPy oracle's forward
    sensitivities (the 2 D directions as one batch) above."""
    D, O = len(a), C.shape[0]
    A, Q = np.diag(a), np.diag(q)
    Rd = np.maximum(np.asarray(var, np.float64), 1e-12)
    dA, dQ = np.zeros((2 * D, D, D)), np.zeros((2 * D, D, D))
    for i in range(D):
        dA[i, i, i] = 1.0
        dQ[D + i, i, i] = 1.0
    if use_c is None:
        use_c = O <= 16
    if use_c:
        L, g = c_oracle.nll_directional(y, Rd, m0, S0, A, C, Q, dA, dQ)
    else:
        rep = lambda x: np.broadcast_to(x, (2 * D,) + x.shape)      # noqa: E731
        f = orc.kalman_filter(rep(np.asarray(y, np.float64)), rep(m0), rep(S0), rep(A), rep(C), rep(Q), 1.0, rep(Rd),
                              tangent=(dA, dQ))
        L, g = -f['ll'][0], -f['dll']
    return float(L), np.array(g[:D]), np.array(g[D:])


def combine(ga, gq, da, dq):
    """Directional derivatives along the tangents (da, dq) (n_tan, D) from the basis derivatives."""
    return np.asarray(da) @ ga + np.asarray(dq) @ gq


@functools.lru_cache(maxsize=None)
def pupil_basis(T, seed, u):
    ys, ev, m0, S0, lv = chain(T, seed)
    a, q, _, _ = pupil_params(u, lv)
    return ar1_basis(ys, ev, m0, S0, orc.PUPIL_C, a, q)


def pupil_trajectory(ys, m0, S0, C, ev, lv, lr, tol, cap):
    """The loop of orc.pupil_optimize_smooth with every iteration recorded: dict(u (n, 2) after each iteration,
    L, prev, thr (n,) of each stop test, stopped: whether the rule ended it)."""
    s0 = np.array([0.99, 0.98], dtype=np.float32).astype(np.float64)
    u = np.log(s0 / (1.0 - s0))
    mom, vel, prev = np.zeros(2), np.zeros(2), np.inf
    rec = dict(u=[], L=[], prev=[], thr=[], stopped=False)
    while len(rec['L']) < cap and not rec['stopped']:
        L, g = orc.pupil_nll_and_grad(u, ys, m0, S0, C, ev, lv, use_c=True)
        n = len(rec['L']) + 1
        mom = 0.9 * mom + (1 - 0.9) * g
        vel = 0.999 * vel + (1 - 0.999) * g * g
        u = u - lr * (mom / (1 - 0.9 ** n)) / (np.sqrt(vel / (1 - 0.999 ** n)) + 1e-8)
        thr = tol * abs(np.log(max(prev, 1e-12))) + 1e-6 if np.isfinite(prev) else np.nan
        rec['stopped'] = bool(np.isfinite(prev) and abs(L - prev) < thr)
        for key, v in (('u', u), ('L', L), ('prev', prev), ('thr', thr)):
            rec[key].append(v)
        prev = L
    return {k: (np.array(v) if k != 'stopped' else v) for k, v in rec.items()}


def trajectory_at(rec, cap):
    """(iters, done, u, last loss) of the recorded run had it been capped at `cap` iterations."""
    n = len(rec['L'])
    it = min(n, cap)
    return it, bool(rec['stopped'] and n <= cap), rec['u'][it - 1], float(rec['L'][it - 1])


# ---------------------------------------------------------------------------------------------
# mirrors of the host's choices (asserted as the cases' premises)
# ---------------------------------------------------------------------------------------------
def dw_units(T, K, B):
    """eks_dense_wave.hip dw_units: (chain, 64-chunk) units of dense_wave_run at B frames per lane."""
    return K * -(-(-(-T // B)) // 64)


def dw_chunk_frames(T, K):
    """eks_dense_wave.hip dw_chunk_frames without EKS_DW_CHUNK (dense_wave_run: more than 256 units take four-wave
    workgroups, dense_wave_covers: more than 1024 are not served)."""
    return 2 if dw_units(T, K, 2) <= 160 else 4 if dw_units(T, K, 4) <= 160 else 8


def loss_tree(T, streams):
    """eks_loss_kernels.hpp loss_chunk / loss_chunks / loss_launch: (frames per chunk, launches of the tree)."""
    b = 8
    while -(-T // b) * streams > 1 << 18:
        b <<= 1
    n = -(-(max(-(-(T - 1) // b), 1)) // 64)
    launches = 1
    while n > 1:
        n = -(-n // 64)
        launches += 1
    return b, launches


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------
def make_loss(y, var, m0, S0, C, n_tan, positive_noise):
    """hip_ops.Ar1Loss from host arrays y, var (K, T, O), m0 (K, D), S0 (K, D, D), C (K, O, D)."""
    import torch
    from eks_amd import hip_ops
    dev = hip_ops.require_gpu()
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=dev)      # noqa: E731
    return hip_ops.Ar1Loss(t(np.swapaxes(y, 0, 1), np.float32), t(np.swapaxes(var, 0, 1), np.float32),
                           t(m0, np.float64), t(S0, np.float64), t(C, np.float64), n_tan=n_tan,
                           positive_noise=positive_noise)


def fill(loss, a, q, da=None, dq=None):
    import torch
    loss.a.copy_(torch.as_tensor(np.asarray(a, np.float64)))
    loss.q.copy_(torch.as_tensor(np.asarray(q, np.float64)))
    if loss.n_tan:
        loss.da.copy_(torch.as_tensor(np.asarray(da, np.float64)))
        loss.dq.copy_(torch.as_tensor(np.asarray(dq, np.float64)))


def drain_scopes(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    ms = (ctypes.c_float * 4096)()
    n = lib.eks_profile_drain(buf, len(buf), ms, 4096)
    return [nm.decode() for nm in buf.raw.split(b'\0')[:n]]


def evaluate(loss, form=None):
    """One evaluation -> (nll (K,), dnll (n_tan, K)) on the host; form 'wave' / 'dual': assert which kernels ran."""
    import torch
    lib = loss.lib
    lib.eks_profile_drain(None, 0, None, 0)
    lib.eks_profile_enable(1)
    try:
        nll, dnll = loss.evaluate()
        torch.cuda.synchronize()
    finally:
        lib.eks_profile_enable(0)
    scopes = drain_scopes(lib)
    if form == 'wave':
        assert scopes == ['dense_score_summarize', 'dense_score_replay'], scopes
    elif form == 'dual':
        assert scopes == ['ar1_nll'], scopes
    return nll.cpu().numpy().copy(), (dnll.cpu().numpy().copy() if loss.n_tan else None)


def raw_status(loss):
    """eks_ar1_nll's status on the buffers of `loss` (no exception)."""
    from eks_amd.hip_ops import _ptr, _stream
    t = loss.n_tan > 0
    return loss.lib.eks_ar1_nll(ctypes.byref(loss.dims), _ptr(loss.y), _ptr(loss.var), _ptr(loss.m0), _ptr(loss.S0),
                                _ptr(loss.C), _ptr(loss.a), _ptr(loss.q), _ptr(loss.da if t else None),
                                _ptr(loss.dq if t else None), loss.n_tan, _ptr(loss.nll),
                                _ptr(loss.dnll if t else None), _ptr(loss.ws), loss.ws.numel(), _stream())


def check(tag, nll, dnll, L, G, loss_bar=1e-9, g_rtol=1e-8, g_atol=1e-9):
    """nll (K,), dnll (n_tan, K) against L (K,), G (K, n_tan): print the worst figures, then assert the bars."""
    L, G = np.asarray(L), np.asarray(G)
    eL = np.abs(nll - L) / np.maximum(np.abs(L), 1.0)
    line = f'FIGURES {tag}: K={len(L)} loss rel {eL.max():.2e}'
    if dnll is not None:
        gmax = np.abs(G).max(axis=1, keepdims=True)
        err = np.abs(dnll.T - G)
        with np.errstate(divide='ignore', invalid='ignore'):
            line += (f' grad err/max|g| {(err / gmax).max():.2e}'
                     f' err/(rtol|g|+atol max|g|) {(err / (g_rtol * np.abs(G) + g_atol * gmax)).max():.2e}')
    print(line)
    assert np.all(np.isfinite(nll)) and eL.max() < loss_bar, line
    if dnll is not None:
        assert np.all(err <= g_rtol * np.abs(G) + g_atol * gmax), line


def pupil_case(K, T, n_tan=2, positive_noise=True, us=None, seeds=None):
    """K pupil chains of T frames: seeds cycle through 11 sessions and u through US, so that neighbours always differ
    (and long lists share their references).  Returns (loss, L (K,), G (K, 2), chains, us)."""
    seeds = seeds or [10 + k % 11 for k in range(K)]
    us = us or [US[k % 3] for k in range(K)]
    ch = [chain(T, s) for s in seeds]
    loss = make_loss(np.stack([c[0] for c in ch]), np.stack([c[1] for c in ch]), np.stack([c[2] for c in ch]),
                     np.stack([c[3] for c in ch]), np.tile(orc.PUPIL_C, (K, 1, 1)), n_tan, positive_noise)
    par = [pupil_params(u, c[4]) for u, c in zip(us, ch)]
    if n_tan == 2:
        fill(loss, [p[0] for p in par], [p[1] for p in par], np.stack([p[2] for p in par], axis=1),
             np.stack([p[3] for p in par], axis=1))
    refs = [pupil_ref(T, s, tuple(u)) for s, u in zip(seeds, us)]
    return loss, np.array([r[0] for r in refs]), np.stack([r[1] for r in refs]), ch, us


def with_sentinel_workspace(loss):
    """Replace loss.ws by the first eks_ar1_nll_workspace_bytes bytes of a larger tensor filled with 0xA5; returns the
    tail that must stay untouched (as long as the reported size, at least 1 MiB: room for any level left out)."""
    import torch
    n = int(loss.lib.eks_ar1_nll_workspace_bytes(ctypes.byref(loss.dims), loss.n_tan))
    assert n >= 256
    big = torch.full((n + max(n, 1 << 20),), 0xA5, dtype=torch.uint8, device=loss.ws.device)
    loss.ws = big[:n]
    return big[n:]


def check_workspace(tag, loss, nll, dnll):
    tail = with_sentinel_workspace(loss)
    nll2, dnll2 = evaluate(loss, 'dual')
    print(f'FIGURES {tag}: workspace {loss.ws.numel()} bytes, tail {tail.numel()} bytes')
    assert np.array_equal(nll2, nll) and np.array_equal(dnll2, dnll)
    assert bool((tail == 0xA5).all()), 'eks_ar1_nll wrote past eks_ar1_nll_workspace_bytes'


# ---------------------------------------------------------------------------------------------
# 1. chunk lengths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,T,B', [(3, 9001, 4), (3, 20001, 8)])
def test_case1_natural_chunk_length(K, T, B):
    assert os.environ.get('EKS_DW_CHUNK') is None and dw_chunk_frames(T, K) == B and dw_units(T, K, B) <= 256
    loss, L, G, _, _ = pupil_case(K, T)
    check(f'case1 natural B={B} ({K},{T})', *evaluate(loss, 'wave'), L, G)


@pytest.mark.parametrize('tail', [1, 0])
@pytest.mark.parametrize('B', [2, 4, 8])
def test_case1_forced_chunk_length(set_knob, B, tail):
    """T = 64 B 3 + 1: the last chunk holds one frame and is the only live lane of the fourth 64-chunk unit;
    T = 64 B 3: every lane of three units full."""
    K, T = 2, 64 * B * 3 + tail
    set_knob('EKS_DW_CHUNK', str(B))
    assert dw_units(T, K, B) == K * (3 + tail) and (T - 1) % B == (0 if tail else B - 1)
    loss, L, G, _, _ = pupil_case(K, T)
    check(f'case1 forced B={B} ({K},{T})', *evaluate(loss, 'wave'), L, G)


# ---------------------------------------------------------------------------------------------
# 2. four-wave workgroups, 3. one long chain, 4. hand-over with many chains
# ---------------------------------------------------------------------------------------------
def test_case2_four_wave_workgroups_with_a_spare_pair():
    K, T = 33, 4097
    units = dw_units(T, K, dw_chunk_frames(T, K))
    assert dw_chunk_frames(T, K) == 8 and units == 297 and 256 < units <= 1024 and units % 2 == 1
    loss, L, G, _, _ = pupil_case(K, T)
    check('case2 (33,4097) SUBS=2', *evaluate(loss, 'wave'), L, G)


def test_case3a_one_chain_of_257_units():
    K, T = 1, 131073
    assert dw_chunk_frames(T, K) == 8 and dw_units(T, K, 8) == 257
    loss, L, G, _, _ = pupil_case(K, T)
    check('case3a (1,131073) SUBS=2', *evaluate(loss, 'wave'), L, G)


def test_case3b_one_chain_past_the_wave_form_and_case8_workspace():
    K, T = 1, 524289
    assert dw_units(T, K, dw_chunk_frames(T, K)) == 1025 and loss_tree(T, 2 * K) == (8, 3)
    loss, L, G, _, _ = pupil_case(K, T)
    nll, dnll = evaluate(loss, 'dual')
    check('case3b (1,524289) dual, flag set', nll, dnll, L, G)
    check_workspace('case8 of 3b', loss, nll, dnll)


def test_case4_many_chains_hand_over_to_dual_numbers():
    K, T = 129, 4097
    assert dw_units(T, K, dw_chunk_frames(T, K)) == 1161
    loss, L, G, _, _ = pupil_case(K, T)
    check('case4 (129,4097) dual, flag set', *evaluate(loss, 'dual'), L, G)


# ---------------------------------------------------------------------------------------------
# 5. both forms on one input
# ---------------------------------------------------------------------------------------------
def test_case5_both_forms_on_one_input_and_case8_workspace(set_knob):
    K, T = 3, 40001
    assert dw_chunk_frames(T, K) == 8 and dw_units(T, K, 8) <= 256 and loss_tree(T, 2 * K) == (8, 3)
    loss, L, G, _, _ = pupil_case(K, T, positive_noise=True)
    check('case5a (3,40001) wave B=8', *evaluate(loss, 'wave'), L, G)
    set_knob('EKS_DENSE_DUAL_GRAD', '1')
    nll_c, dnll_c = evaluate(loss, 'dual')
    check('case5c (3,40001) dual by EKS_DENSE_DUAL_GRAD, flag set', nll_c, dnll_c, L, G)
    set_knob('EKS_DENSE_DUAL_GRAD', None)
    loss, _, _, _, _ = pupil_case(K, T, positive_noise=False)
    nll, dnll = evaluate(loss, 'dual')
    check('case5b (3,40001) dual, three launches', nll, dnll, L, G)
    assert np.array_equal(nll, nll_c) and np.array_equal(dnll, dnll_c)
    check_workspace('case8 of 5b', loss, nll, dnll)


# ---------------------------------------------------------------------------------------------
# 6. chunk growth and many tangents
# ---------------------------------------------------------------------------------------------
def tangent_case(K, T, n_tan, positive_noise, seed):
    """Pupil chains at their pupil parameters with n_tan random tangents; references by the basis helper."""
    rng = np.random.default_rng(seed)
    seeds = [10 + k % 11 for k in range(K)]
    us = [US[k % 3] for k in range(K)]
    ch = [chain(T, s) for s in seeds]
    loss = make_loss(np.stack([c[0] for c in ch]), np.stack([c[1] for c in ch]), np.stack([c[2] for c in ch]),
                     np.stack([c[3] for c in ch]), np.tile(orc.PUPIL_C, (K, 1, 1)), n_tan, positive_noise)
    par = [pupil_params(u, c[4]) for u, c in zip(us, ch)]
    da, dq = rng.normal(size=(n_tan, K, 3)), rng.normal(size=(n_tan, K, 3))
    fill(loss, [p[0] for p in par], [p[1] for p in par], da, dq)
    base = [pupil_basis(T, s, tuple(u)) for s, u in zip(seeds, us)]
    L = np.array([b[0] for b in base])
    G = np.stack([combine(b[1], b[2], da[:, k], dq[:, k]) for k, b in enumerate(base)])
    return loss, L, G


def test_case6a_chunk_growth_with_1024_streams_and_case8_workspace():
    K, T, n_tan = 16, 2050, 64
    assert -(-T // 8) * K * n_tan > 1 << 18 and loss_tree(T, K * n_tan) == (16, 2)
    loss, L, G = tangent_case(K, T, n_tan, False, seed=60)
    nll, dnll = evaluate(loss, 'dual')
    check('case6a (16,2050,64) dual B=16', nll, dnll, L, G)
    check_workspace('case8 of 6a', loss, nll, dnll)


def test_case6b_wave_form_with_64_tangents():
    loss, L, G = tangent_case(16, 2050, 64, True, seed=60)
    check('case6b (16,2050,64) wave', *evaluate(loss, 'wave'), L, G)


@pytest.mark.parametrize('positive_noise', [False, True])
@pytest.mark.parametrize('n_tan', [1, 3])
def test_case6c_odd_tangent_counts(n_tan, positive_noise):
    loss, L, G = tangent_case(3, 700, n_tan, positive_noise, seed=61 + n_tan)
    check(f'case6c (3,700,{n_tan}) {"wave" if positive_noise else "dual"}',
          *evaluate(loss, 'wave' if positive_noise else 'dual'), L, G)


# ---------------------------------------------------------------------------------------------
# 7. general models on the dual path
# ---------------------------------------------------------------------------------------------
def general_model(K, T, D, O, seed):
    """Random AR(1) chains: C normal, a in (0.3, 0.99), q in (0.1, 1), observations simulated from the model with
    per-frame variances in (0.05, 1.5); y, var rounded through float32."""
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(K, O, D))
    a = rng.uniform(0.3, 0.99, size=(K, D))
    q = rng.uniform(0.1, 1.0, size=(K, D))
    m0 = rng.normal(size=(K, D))
    W = rng.normal(size=(K, D, D))
    S0 = W @ np.swapaxes(W, 1, 2) / D + 0.5 * np.eye(D)
    var = rng.uniform(0.05, 1.5, size=(K, T, O)).astype(np.float32).astype(np.float64)
    x = m0.copy()
    y = np.empty((K, T, O))
    for t in range(T):
        y[:, t] = np.einsum('kod,kd->ko', C, x) + rng.normal(size=(K, O)) * np.sqrt(var[:, t])
        x = a * x + rng.normal(size=(K, D)) * np.sqrt(q)
    return y.astype(np.float32).astype(np.float64), var, m0, S0, C, a, q


@pytest.mark.parametrize('T', [1, 2, 513, 600])
@pytest.mark.parametrize('D,O', [(1, 1), (2, 3), (4, 8), (6, 16), (3, 33), (2, 64)])
def test_case7_general_models_on_the_dual_path(D, O, T):
    K = 3
    assert [loss_tree(t, 2 * K)[1] for t in (1, 2, 513, 600)] == [1, 1, 1, 2]
    y, var, m0, S0, C, a, q = general_model(K, T, D, O, seed=1000 * D + 10 * O + T % 7)
    rng = np.random.default_rng(7)
    da, dq = rng.normal(size=(2, K, D)), rng.normal(size=(2, K, D))
    base = [ar1_basis(y[k], var[k], m0[k], S0[k], C[k], a[k], q[k]) for k in range(K)]
    L = np.array([b[0] for b in base])
    G = np.stack([combine(b[1], b[2], da[:, k], dq[:, k]) for k, b in enumerate(base)])
    loss = make_loss(y, var, m0, S0, C, 2, False)
    fill(loss, a, q, da, dq)
    check(f'case7 D={D} O={O} T={T} n_tan=2', *evaluate(loss, 'dual'), L, G)
    loss0 = make_loss(y, var, m0, S0, C, 0, False)
    fill(loss0, a, q)
    check(f'case7 D={D} O={O} T={T} n_tan=0', *evaluate(loss0, 'dual'), L, None)


# ---------------------------------------------------------------------------------------------
# 9. parameters at the clamps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('positive_noise', [True, False])
def test_case9_parameters_at_the_clamps(positive_noise):
    """u = (+-20, -+20): s = 0.999 / 0.001 to eight digits (sigmoid(20) = 1 - 2.1e-9)."""
    us = [(20.0, -20.0), (-20.0, 20.0)]
    s, _ = orc.pupil_to_stable_s(np.array(us[0]))
    assert abs(s[0] - 0.999) < 1e-8 and abs(s[1] - 0.001) < 1e-8
    loss, L, G, _, _ = pupil_case(2, 5003, positive_noise=positive_noise, us=us)
    form = 'wave' if positive_noise else 'dual'
    check(f'case9 clamps (2,5003) {form}', *evaluate(loss, form), L, G)


# ---------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------
def test_case10_refusals_and_65_tangents_with_the_flag():
    import torch
    # 65 536 streams on the dual path
    K = 32768
    z = np.zeros((K, 2, 1))
    loss = make_loss(z, z + 1.0, np.zeros((K, 1)), np.ones((K, 1, 1)), np.ones((K, 1, 1)), 2, False)
    fill(loss, np.full((K, 1), 0.5), np.ones((K, 1)), np.ones((2, K, 1)), np.ones((2, K, 1)))
    assert raw_status(loss) == EKS_ERR_UNSUPPORTED
    # state and observation sizes past the instantiated ones
    for D, O in ((7, 8), (3, 65)):
        z = np.zeros((1, 10, O))
        loss = make_loss(z, z + 1.0, np.zeros((1, D)), np.eye(D)[None], np.ones((1, O, D)), 2, False)
        loss.ws = torch.empty(1 << 20, dtype=torch.uint8, device=loss.ws.device)
        fill(loss, np.full((1, D), 0.5), np.ones((1, D)), np.ones((2, 1, D)), np.ones((2, 1, D)))
        assert raw_status(loss) == EKS_ERR_UNSUPPORTED
    # 65 tangents: one more than the wave form's finishing launch serves; with the flag on a covered shape the call
    # takes the dual-number form, as it does without the flag
    K, T = 3, 700
    assert dw_units(T, K, dw_chunk_frames(T, K)) <= 1024
    loss, L, G = tangent_case(K, T, 65, True, seed=65)
    check('case10 (3,700,65) flag set -> dual', *evaluate(loss, 'dual'), L, G)
    loss, L, G = tangent_case(K, T, 64, True, seed=65)
    check('case10 (3,700,64) flag set -> wave', *evaluate(loss, 'wave'), L, G)


# ---------------------------------------------------------------------------------------------
# 11. many chains in the optimiser
# ---------------------------------------------------------------------------------------------
# Seeds 40..47 stop after 59, 96, 88, 74, 61, 65, 30 and 140 iterations, but 41, 42, 43 and 47 come within 3.6e-7,
# 7.7e-7, 1.8e-7 and 6.7e-7 |L| of their threshold at some iteration (the condition below asks for 1e-6): replaced by
# the next seeds that keep the margin.  These eight stop after 59, 124, 69, 61, 65, 44, 30 and 48 iterations: one past
# the smaller cap (among the first five: every K has it), one at the end of a 16-iteration call.
ADAM_SEEDS = (40, 65, 54, 44, 45, 48, 46, 77)
ADAM_T, ADAM_LR, ADAM_TOL, ADAM_CAP = 300, 2e-2, 0.1, 150


@functools.lru_cache(maxsize=None)
def adam_oracle(seed):
    ys, ev, m0, S0, lv = chain(ADAM_T, seed, False)
    return pupil_trajectory(ys, m0, S0, orc.PUPIL_C, ev, lv, ADAM_LR, ADAM_TOL, ADAM_CAP)


def test_case11_inputs_make_the_stop_decisions_safe():
    """From the oracle alone: at least three distinct stopping iterations among the eight chains, all under the larger
    cap and one past the smaller, and no stop test closer to its threshold than 1e-6 |L| (a thousand loss bars)."""
    recs = [adam_oracle(s) for s in ADAM_SEEDS]
    stops = [len(r['L']) for r in recs]
    print('FIGURES case11 oracle stopping iterations', stops)
    assert all(r['stopped'] for r in recs) and len(set(stops)) >= 3
    assert sum(n > 100 for n in stops) == 1 and any(n % 16 == 0 for n in stops)
    for r in recs:
        margin = np.abs(np.abs(r['L'][1:] - r['prev'][1:]) - r['thr'][1:])
        assert np.all(margin > 1e-6 * np.abs(r['L'][1:]))


@pytest.mark.parametrize('cap', [150, 100])
@pytest.mark.parametrize('K,positive_noise', [(5, True), (64, True), (65, True), (5, False)])
def test_case11_many_chains_in_the_optimiser(K, positive_noise, cap):
    """K = 5, 64: dw_ar1_finish_step_kernel; K = 65: dw_ar1_finish_kernel + eks_pupil_adam_step; without the flag:
    the dual form + eks_pupil_adam_step.  Chain k is session ADAM_SEEDS[k % 8]."""
    import torch
    from eks_amd import hip_ops
    seeds = [ADAM_SEEDS[k % 8] for k in range(K)]
    recs = [adam_oracle(s) for s in seeds]
    ch = [chain(ADAM_T, s, False) for s in seeds]
    assert dw_units(ADAM_T, K, dw_chunk_frames(ADAM_T, K)) <= 1024
    loss = make_loss(np.stack([c[0] for c in ch]), np.stack([c[1] for c in ch]), np.stack([c[2] for c in ch]),
                     np.stack([c[3] for c in ch]), np.tile(orc.PUPIL_C, (K, 1, 1)), 2, positive_noise)
    dev = loss.y.device
    s0 = np.array([0.99, 0.98], dtype=np.float32).astype(np.float64)
    state = np.zeros((K, 9))
    state[:, 0:2] = np.log(s0 / (1.0 - s0))
    state[:, 6] = np.inf
    state = torch.as_tensor(state, device=dev)
    latent = torch.as_tensor(np.stack([c[4] for c in ch]), device=dev)
    n_active = torch.full((1,), -7, dtype=torch.int32, device=dev)
    hip_ops.pupil_adam_step(loss, latent, state, n_active, ADAM_LR, ADAM_TOL, cap, init=True)
    lib = loss.lib
    lib.eks_profile_drain(None, 0, None, 0)
    frozen, launched = {}, 0
    while launched < cap:
        lib.eks_profile_enable(1 if launched == 0 else 0)
        hip_ops.pupil_adam_run(loss, latent, state, n_active, ADAM_LR, ADAM_TOL, cap, 16)
        launched += 16
        st = state.cpu().numpy().copy()
        running = [len(r['L']) > launched and launched < cap for r in recs]
        assert int(n_active.item()) == sum(running), (launched, int(n_active.item()), sum(running))
        for k in range(K):
            if not running[k]:
                frozen.setdefault(k, st[k])
                assert st[k].tobytes() == frozen[k].tobytes(), (launched, k)
    lib.eks_profile_enable(0)
    scopes = set(drain_scopes(lib))
    assert scopes == ({'dense_score_summarize', 'dense_score_replay'} if positive_noise else {'ar1_nll'}), scopes
    want = [trajectory_at(r, cap) for r in recs]
    eu = max(np.abs(st[k, 0:2] / want[k][2] - 1).max() for k in range(K))
    eL = max(abs(st[k, 6] - want[k][3]) / max(abs(want[k][3]), 1.0) for k in range(K))
    print(f'FIGURES case11 K={K} flag={positive_noise} cap={cap}: iters {sorted(set(w[0] for w in want))} '
          f'u rel {eu:.2e} last loss rel {eL:.2e}')
    for k in range(K):
        it, done, u, last = want[k]
        assert (int(st[k, 7]), bool(st[k, 8])) == (it, done), k
        np.testing.assert_allclose(st[k, 0:2], u, rtol=1e-9)
        assert abs(st[k, 6] - last) < 1e-9 * max(abs(last), 1.0)
        assert st[k].tobytes() == st[k % 8].tobytes(), f'copy {k} of chain {k % 8} differs'
    assert len(set(w[0] for w in want)) >= 3 and any(not w[1] for w in want) == (cap == 100)
