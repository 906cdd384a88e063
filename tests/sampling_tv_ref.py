"""Float64 NumPy reference of eks_sample_tv (TEST INFRASTRUCTURE, imported by the sampling_tv tests only): the posterior
sampler of tests/sampling_ref.py under a per-frame process-noise scale w and observation weights lam,

    x_t = A x_{t-1} + N(0, s w_t Q),      y_t = C x_t + N(0, r_eff,t),      r_eff,t = clip(clip(var_t) / lam_t).

scalar_filter_smoother / scalar_deviations and their float32 transcriptions extended by w and lam, Durbin & Koopman's
simulation smoother under (r_eff, w), the joint posterior covariance of a short session by plain linear algebra, and
the linear map L from the normals to the deviations (law_error(L, S) checks the law).  w[0] is never read; the
noise of the step INTO frame t is s w_t Q.  Nothing here is compared with, or derived from, the kernels' own output."""
from __future__ import annotations

import numpy as np

import sampling_ref as ref
from sampling_ref import VAR_CEIL, VAR_FLOOR
from smooth_tv_ref import _w_cols


def r_eff(var, lam=None, dtype=np.float64):
    """clip(clip(var) * (1 / lam)) in `dtype` (robust_var of eks_smooth_robust_lane.hpp); lam None: clip(var)."""
    f = dtype
    r = np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    if lam is None:
        return r
    with np.errstate(over='ignore'):
        return np.clip(r * (f(1) / np.asarray(lam, f)), f(VAR_FLOOR), f(VAR_CEIL))


def step_noise(qs, w, T, N, D=1, dtype=np.float64):
    """q [T + 1][N]: q[t] = (s q) w[t], the noise of the step INTO frame t; q[0] is unused and q[T] = s q (w = 1 past
    the session, which no output depends on).  w None: 1; (T,) shared; (T, N / D) per keypoint."""
    f = dtype
    qs = np.broadcast_to(np.asarray(qs, f), (N,))
    wc = np.ones((T + 1, N), f)
    if w is not None:
        wc[:T] = _w_cols(np.asarray(w, np.float32), T, N, D).astype(f)
    wc[0] = 1
    return (qs[None, :] * wc).astype(f)


def scalar_filter_smoother(y, var, m0, S0, a, c, qs, w=None, lam=None, D=1, dtype=np.float64):
    """sampling_ref.scalar_filter_smoother under (r_eff, w): the predict after frame t's update adds q[t + 1].
    Returns mf, Pf, ms, Vs, G [T][N] (G[T-1] = 0)."""
    f = dtype
    y, r = np.asarray(y, f), r_eff(var, lam, f)
    a, c = (np.asarray(x, f) for x in (a, c))
    T, N = y.shape
    q = step_noise(qs, w, T, N, D, f)
    mf, Pf = np.empty((T, N), f), np.empty((T, N), f)
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    for t in range(T):
        g = 1 / (P * c * c + r[t])
        mf[t] = m + P * c * g * (y[t] - c * m)
        Pf[t] = P * r[t] * g
        m, P = a * mf[t], a * a * Pf[t] + q[t + 1]
    ms, Vs, G = np.empty_like(mf), np.empty_like(Pf), np.zeros_like(Pf)
    ms[-1], Vs[-1] = mf[-1], Pf[-1]
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + q[t + 1]
        G[t] = a * Pf[t] / Pp
        ms[t] = mf[t] + G[t] * (ms[t + 1] - a * mf[t])
        Vs[t] = Pf[t] * q[t + 1] / Pp + G[t] * G[t] * Vs[t + 1]
    return mf, Pf, ms, Vs, G


def scalar_deviations(Pf, a, qs, z, w=None, D=1, dtype=np.float64):
    """e [n_draws][T][N]: e_{T-1} = sqrt(Pf) z, e_t = G_t e_{t+1} + sqrt(Pf_t q_{t+1} / Pp_t) z_t with
    Pp_t = a^2 Pf_t + q_{t+1}: G_t and sd_t of frame t read w[t + 1]."""
    f = dtype
    Pf, a, z = np.asarray(Pf, f), np.asarray(a, f), np.asarray(z, f)
    T, N = Pf.shape
    q = step_noise(qs, w, T, N, D, f)
    e = np.empty(z.shape, f)
    e[:, -1] = np.sqrt(Pf[-1]) * z[:, -1]
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + q[t + 1]
        G = a * Pf[t] / Pp
        e[:, t] = G * e[:, t + 1] + np.sqrt(Pf[t] * (q[t + 1] / Pp)) * z[:, t]
    return e


def scalar_deviations_f32(var, S0, a, c, qs, z, w=None, lam=None, D=1):
    """The float32 transcription: r_eff, the variance filter and the recurrence in float32 throughout."""
    f = np.float32
    var = np.asarray(var, f)
    _, Pf, _, _, _ = scalar_filter_smoother(np.zeros_like(var), var, np.zeros(var.shape[1]), S0, a, c, qs, w, lam, D, dtype=f)
    return scalar_deviations(Pf, a, qs, z, w, D, dtype=f)


def scalar_law_map(var, S0, a, c, qs, w=None, lam=None):
    """One chain (var, w, lam (T,)): L [T][T] with e = L z."""
    T = len(var)
    col = lambda v: None if v is None else np.asarray(v, np.float64).reshape(T, 1)
    _, Pf, _, _, _ = scalar_filter_smoother(np.zeros((T, 1)), col(var), [0.0], [S0], [a], [c], [qs], w, col(lam))
    return scalar_deviations(Pf, [a], [qs], np.eye(T)[:, :, None], w)[:, :, 0].T


def joint_covariance(r, S0, A, C, Q, s, w=None):
    """One keypoint, T frames: the joint posterior covariance of (x_0 .. x_{T-1}) [T D][T D] by plain linear algebra
    under the variances r [T][O] (already r_eff) and P_t = A P_{t-1} A' + s w_t Q."""
    r = np.asarray(r, np.float64)
    S0, A, C, Q = (np.atleast_2d(np.asarray(x, np.float64)) for x in (S0, A, C, Q))
    T, O = r.shape
    D = A.shape[0]
    w = np.ones(T) if w is None else np.asarray(w, np.float64)
    P = [S0]
    for t in range(1, T):
        P.append(A @ P[-1] @ A.T + s * w[t] * Q)
    Sx = np.zeros((T * D, T * D))
    for i in range(T):
        Cij = P[i]
        for j in range(i, T):
            Sx[j * D:(j + 1) * D, i * D:(i + 1) * D] = Cij
            Sx[i * D:(i + 1) * D, j * D:(j + 1) * D] = Cij.T
            Cij = A @ Cij
    H = np.kron(np.eye(T), C)
    Sy = H @ Sx @ H.T + np.diag(r.ravel())
    return Sx - Sx @ H.T @ np.linalg.solve(Sy, H @ Sx)


def _rts_tv(mf, Pf, A, sQ, wk):
    """RTS pass over (K, T, D) filtered beliefs with P_pred(t+1) = A Pf_t A' + w[t+1] sQ; wk [T][K]."""
    K, T, D = mf.shape
    At = np.swapaxes(A, -1, -2)
    ms, Vs = mf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        Pp = A @ Pf[:, t] @ At + wk[t + 1][:, None, None] * sQ
        Pp = 0.5 * (Pp + np.swapaxes(Pp, -1, -2))
        # G = Pf A' Pp^+ ; a singular Pp (singular Q on a singular Pf) takes the pseudo-inverse
        G = Pf[:, t] @ At @ np.linalg.pinv(Pp, rcond=1e-13, hermitian=True)
        ms[:, t] = mf[:, t] + np.einsum('kij,kj->ki', G, ms[:, t + 1] - np.einsum('kij,kj->ki', A, mf[:, t]))
        V = Pf[:, t] + G @ (Vs[:, t + 1] - Pp) @ np.swapaxes(G, -1, -2)
        Vs[:, t] = 0.5 * (V + np.swapaxes(V, -1, -2))
    return ms, Vs


def _filter_tv(y, m0, S0, A, C, sQ, wk, R):
    """sampling_ref.filter_by_scalar_updates with the predict INTO frame t under wk[t] sQ.  y, R (K, T, O)."""
    K, T, O = y.shape
    D = m0.shape[-1]
    At = np.swapaxes(A, -1, -2)
    mf, Pf = np.empty((K, T, D)), np.empty((K, T, D, D))
    m, P = m0.copy(), S0.copy()
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + wk[t][:, None, None] * sQ
        for o in range(O):
            h = C[:, o]
            u = np.einsum('kij,kj->ki', P, h)
            g = 1.0 / (R[:, t, o] + np.einsum('ki,ki->k', h, u))
            m = m + u * (g * (y[:, t, o] - np.einsum('ki,ki->k', h, m)))[:, None]
            P = P - u[:, :, None] * u[:, None, :] * g[:, None, None]
        P = 0.5 * (P + np.swapaxes(P, -1, -2))
        mf[:, t], Pf[:, t] = m, P
    return mf, Pf


def dense_durbin_koopman(y, var, m0, S0, A, C, Q, s, z, w=None, lam=None, storage=np.float64, round_output=True):
    """sampling_ref.dense_durbin_koopman under (r_eff, w): the state noise of the step into frame t is
    sqrt(w_t) chol(s Q) z, the observation noise sqrt(r_eff) z, and both smoothing problems run under (r_eff, w).
    r_eff is the float32 value the kernels form (r_eff(var, lam, float32)).  y, var, lam [T][K][O]; w (T,) or (T, K);
    z [n_draws][T][K][D + O].  Returns ms [T][K][D], Vs [T][K][D][D], dev [n_draws][T][K][D]; storage as there."""
    st = storage
    y = np.asarray(y, np.float64)
    T, K, O = y.shape
    R = r_eff(var, lam, np.float32).astype(np.float64)
    A, C, Q, S0, m0 = (np.asarray(a, np.float64) for a in (A, C, Q, S0, m0))
    s = np.broadcast_to(np.asarray(s, np.float64), (K,))
    sQ = s[:, None, None] * Q
    wk = np.ones((T, K)) if w is None else _w_cols(np.asarray(w, np.float32), T, K).astype(np.float64).copy()
    wk[0] = 1.0
    z = np.asarray(z, np.float64)
    n, D = z.shape[0], A.shape[-1]
    assert z.shape == (n, T, K, D + O)
    L0, Lq = ref.chol_psd(S0), ref.chol_psd(sQ)
    xs = np.empty((n, T, K, D))
    x = np.zeros((n, K, D))
    for t in range(T):
        x = np.einsum('kij,nkj->nki', L0, z[:, 0, :, :D]) if t == 0 else \
            np.einsum('kij,nkj->nki', A, x) + np.sqrt(wk[t])[None, :, None] * np.einsum('kij,nkj->nki', Lq, z[:, t, :, :D])
        xs[:, t] = x
    yp = np.einsum('koj,ntkj->ntko', C, xs) + np.sqrt(R)[None] * z[..., D:]
    xs, yp = xs.astype(st).astype(np.float64), yp.astype(st).astype(np.float64)
    rep = lambda a: np.tile(a, (n + 1,) + (1,) * (a.ndim - 1))
    y_all = np.concatenate([y[None], yp]).transpose(0, 2, 1, 3).reshape((n + 1) * K, T, O)
    R_all = np.tile(R.transpose(1, 0, 2), (n + 1, 1, 1))
    m0_all = np.concatenate([m0, np.zeros((n * K, D))])
    wk_all = np.tile(wk, (1, n + 1))
    mf, Pf = _filter_tv(y_all, m0_all, rep(S0), rep(A), rep(C), rep(sQ), wk_all, R_all)
    ms_all, Vs_all = _rts_tv(mf, Pf, rep(A), rep(sQ), wk_all)
    ms = ms_all[:K].transpose(1, 0, 2)
    Vs = Vs_all[:K].transpose(1, 0, 2, 3)
    mp = ms_all[K:].reshape(n, K, T, D).transpose(0, 2, 1, 3)
    ms_st, mp = ms.astype(st).astype(np.float64), mp.astype(st).astype(np.float64)
    dev = xs - mp
    if round_output and st is not np.float64:
        dev = (ms_st[None] + dev).astype(st).astype(np.float64) - ms_st[None]
    return ms_st, Vs, dev


def dense_law_map(var, m0, S0, A, C, Q, s, w=None, lam=None):
    """One keypoint (var, lam [T][O]; w (T,)): L [T D][T (D + O)] with dev = L z, through dense_durbin_koopman on
    one-hot normals."""
    var = np.asarray(var, np.float64)
    T, O = var.shape
    D = np.shape(A)[-1]
    W = D + O
    z = np.zeros((T * W, T, 1, W))
    for t in range(T):
        for i in range(W):
            z[t * W + i, t, 0, i] = 1.0
    k1 = lambda a: None if a is None else np.asarray(a)[:, None]
    _, _, dev = dense_durbin_koopman(np.zeros((T, 1, O)), var[:, None], np.asarray(m0)[None], np.asarray(S0)[None],
                                     np.asarray(A)[None], np.asarray(C)[None], np.asarray(Q)[None], [s], z, w, k1(lam))
    return dev.reshape(T * W, T * D).T
