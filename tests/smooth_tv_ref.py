"""Float64 NumPy references of eks_smooth_tv (TEST INFRASTRUCTURE, imported by the smooth_tv tests only): the
sequential Kalman filter + RTS smoother of

    x_0 ~ N(m0, S0),      x_t = A x_{t-1} + N(0, s w_t Q)      for t = 1 .. T-1

on scalar chains and on general (D, O) models in two independent forms (observations absorbed one at a time and the
RTS gain through a solve; the gain through the innovation matrix in Joseph form and the RTS gain through an explicit
inverse), the joint Gaussian posterior of the stacked states by plain linear algebra, the padding construction of the
gap identity, and the float32 transcription of the scalar lane expressions (filter_step, rts_gain, rts_advance with
every operation in float32 as eks_math.hpp states it) from which the float32 bars are derived.  w[0] is never read.
Nothing here is compared with, or derived from, the kernels' own output."""
from __future__ import annotations

import numpy as np

from sampling_ref import VAR_CEIL, VAR_FLOOR


def _w_cols(w, T, n_cols, rep=1):
    """w (T,) or (T, n_cols / rep) -> float64 (T, n_cols): column n reads entry n // rep."""
    w = np.asarray(w, np.float64)
    if w.ndim == 1:
        return np.broadcast_to(w[:, None], (T, n_cols))
    return np.repeat(w, rep, axis=1)


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_smooth_tv(y, var, m0, S0, a, c, qs, w, D=1):
    """N independent chains (arrays over chains; y, var [T][N]); w (T,) or (T, N / D) (chain n reads column n // D).
    -> ms [T][N], Vs [T][N] float64."""
    f = np.float64
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), VAR_FLOOR, VAR_CEIL)
    T, N = y.shape
    a, c, qs = (np.broadcast_to(np.asarray(x, f), (N,)) for x in (a, c, qs))
    q = qs[None, :] * _w_cols(w, T, N, D)                       # q[t]: noise of the step INTO frame t
    mf, Pf = np.empty((T, N)), np.empty((T, N))
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    for t in range(T):
        if t:
            m, P = a * m, a * a * P + q[t]
        S = P * c * c + var[t]
        m = m + P * c / S * (y[t] - c * m)
        P = P * var[t] / S
        mf[t], Pf[t] = m, P
    ms, Vs = mf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + q[t + 1]
        G = a * Pf[t] / Pp
        ms[t] = mf[t] + G * (ms[t + 1] - a * mf[t])
        Vs[t] = Pf[t] + G * G * (Vs[t + 1] - Pp)
    return ms, Vs


def scalar_smooth_tv_f32(y, var, m0, S0, a, c, qs, w, D=1, unit=False):
    """The float32 transcription of the lane expressions, frame by frame without chunks or scan: filter_step with
    q = (s q) w[t + 1] (1 past the last frame), then from the predicted belief on the phantom frame T the steps
    rts_gain / rts_advance (the deviation-form select included) with the same q.  a x is x - (1 - a) x and a^2 x is
    x - (1 - a^2) x with the complements rounded once from float64.  -> ms, Vs [T][N] float32."""
    f = np.float32
    N = np.shape(y)[1]
    a64 = np.broadcast_to(np.asarray(a, np.float64), (N,))
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T = y.shape[0]
    a32, oma, oma2 = a64.astype(f), (1.0 - a64).astype(f), (1.0 - a64 * a64).astype(f)
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    q32 = np.broadcast_to(np.asarray(qs, np.float64), (N,)).astype(f)
    w32 = np.concatenate([_w_cols(w, T, N, D).astype(f), np.ones((1, N), f)])      # row T: 1
    one, two, quarter = f(1), f(2), f(0.25)

    def ta(x):
        return x if unit else x - oma * x

    def ta2(x):
        return x if unit else x - oma2 * x
    mf, Pf = np.empty((T, N), f), np.empty((T, N), f)
    m, P = np.asarray(m0, np.float64).astype(f), np.asarray(S0, np.float64).astype(f)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for t in range(T):
            q = q32 * w32[t + 1]
            Pc = P if unit else P * c32
            g = one / ((P + var[t]) if unit else (Pc * c32 + var[t]))
            d = (y[t] - m) if unit else (y[t] - c32 * m)
            mf[t] = m + Pc * g * d
            Pf[t] = P * var[t] * g
            m, P = ta(mf[t]), ta2(Pf[t]) + q
        ms, Vs = np.empty((T, N), f), np.empty((T, N), f)
        for t in range(T - 1, -1, -1):
            q = q32 * w32[t + 1]
            ig = one / (ta2(Pf[t]) + q)
            h = q * ig
            G = Pf[t] * ig if unit else a32 * Pf[t] * ig
            amf = ta(mf[t])
            gg = h if unit else (h - oma) * (one / a32)
            m = mf[t] + G * (m - amf)
            prod = Pf[t] * h + G * G * P
            dev = P + (Pf[t] * h - gg * (two - gg) * P)
            P = np.where((gg < quarter) & (gg > -quarter), dev, prod).astype(f)
            ms[t], Vs[t] = m, P
    return ms, Vs


# ---- general models --------------------------------------------------------------------------------------------------
def _prep(y, var, m0, S0, A, C, Q, s, w):
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
    T, K, O = y.shape
    sQ = np.broadcast_to(np.asarray(s, np.float64), (K,))[:, None, None] * Q
    wk = _w_cols(w, T, K)
    return y, R, m0, S0, A, C, sQ, wk, T, K, O


def _sym(P):
    return 0.5 * (P + np.swapaxes(P, -1, -2))


def dense_smooth_tv(y, var, m0, S0, A, C, Q, s, w):
    """Sequential-update form: observations absorbed one at a time (exact for diagonal R), the RTS gain through
    numpy.linalg.solve.  y, var [T][K][O]; w (T,) or (T, K) -> ms [T][K][D], Vs [T][K][D][D]."""
    y, R, m0, S0, A, C, sQ, wk, T, K, O = _prep(y, var, m0, S0, A, C, Q, s, w)
    D = A.shape[-1]
    At = np.swapaxes(A, -1, -2)
    mf, Pf = np.empty((T, K, D)), np.empty((T, K, D, D))
    m, P = m0.copy(), S0.copy()
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + wk[t][:, None, None] * sQ
        for o in range(O):
            h = C[:, o]
            u = np.einsum('kij,kj->ki', P, h)
            sig = R[t, :, o] + np.einsum('ki,ki->k', h, u)
            d = y[t, :, o] - np.einsum('ki,ki->k', h, m)
            m = m + u * (d / sig)[:, None]
            P = P - u[:, :, None] * u[:, None, :] / sig[:, None, None]
        P = _sym(P)
        mf[t], Pf[t] = m, P
    ms, Vs = mf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        Pp = _sym(A @ Pf[t] @ At + wk[t + 1][:, None, None] * sQ)
        Gt = np.linalg.solve(Pp, A @ Pf[t])                                   # Pp^-1 A Pf = G^T
        G = np.swapaxes(Gt, -1, -2)
        ms[t] = mf[t] + np.einsum('kij,kj->ki', G, ms[t + 1] - np.einsum('kij,kj->ki', A, mf[t]))
        Vs[t] = _sym(Pf[t] + G @ (Vs[t + 1] - Pp) @ Gt)
    return ms, Vs


def dense_smooth_tv_joint(y, var, m0, S0, A, C, Q, s, w):
    """Independent of the above: the update through the gain K = P C' S^-1 with S_t as a matrix, in Joseph form; the
    RTS gain through an explicit inverse.  Same outputs."""
    y, R, m0, S0, A, C, sQ, wk, T, K, O = _prep(y, var, m0, S0, A, C, Q, s, w)
    D = A.shape[-1]
    At, Ct = np.swapaxes(A, -1, -2), np.swapaxes(C, -1, -2)
    eye = np.eye(D)
    mf, Pf = np.empty((T, K, D)), np.empty((T, K, D, D))
    m, P = m0.copy(), S0.copy()
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + wk[t][:, None, None] * sQ
        Rt = np.zeros((K, O, O))
        Rt[:, np.arange(O), np.arange(O)] = R[t]
        S = _sym(C @ P @ Ct + Rt)
        G = np.swapaxes(np.linalg.solve(S, C @ P), -1, -2)
        m = m + np.einsum('kio,ko->ki', G, y[t] - np.einsum('koi,ki->ko', C, m))
        IGC = eye - G @ C
        P = _sym(IGC @ P @ np.swapaxes(IGC, -1, -2) + G @ Rt @ np.swapaxes(G, -1, -2))
        mf[t], Pf[t] = m, P
    ms, Vs = mf.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        Pp = _sym(A @ Pf[t] @ At + wk[t + 1][:, None, None] * sQ)
        G = Pf[t] @ At @ np.linalg.inv(Pp)
        ms[t] = mf[t] + np.einsum('kij,kj->ki', G, ms[t + 1] - np.einsum('kij,kj->ki', A, mf[t]))
        Vs[t] = _sym(Pf[t] + G @ (Vs[t + 1] - Pp) @ np.swapaxes(G, -1, -2))
    return ms, Vs


def joint_posterior(y, var, m0, S0, A, C, Q, s, w):
    """One keypoint: mean and covariance of the stacked states given the stacked observations by Gaussian
    conditioning, with the prior covariance of the stacked states built from P_t = A P_{t-1} A' + s w_t Q and
    Cov(x_u, x_t) = A^(u-t) P_t for u >= t.  y, var [T][O]; w (T,).  -> ms [T][D], Vs [T][D][D] (the diagonal blocks)."""
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
    w = np.asarray(w, np.float64)
    T, O = y.shape
    D = A.shape[0]
    Pt, mx = [S0], [m0]
    for t in range(1, T):
        Pt.append(A @ Pt[-1] @ A.T + s * w[t] * Q)
        mx.append(A @ mx[-1])
    Sx = np.zeros((T * D, T * D))
    for t in range(T):
        blk = Pt[t]
        for u in range(t, T):
            Sx[u * D:(u + 1) * D, t * D:(t + 1) * D] = blk
            Sx[t * D:(t + 1) * D, u * D:(u + 1) * D] = blk.T
            blk = A @ blk
    H = np.kron(np.eye(T), C)
    cov = H @ Sx @ H.T + np.diag(R.ravel())
    mxs = np.concatenate(mx)
    SH = Sx @ H.T
    post_m = mxs + SH @ np.linalg.solve(cov, y.ravel() - H @ mxs)
    post_S = Sx - SH @ np.linalg.solve(cov, SH.T)
    return post_m.reshape(T, D), np.stack([post_S[t * D:(t + 1) * D, t * D:(t + 1) * D] for t in range(T)])


def pad_gaps(y, var, w):
    """The gap identity's padded session: for integer w[t] = n, n - 1 frames of variance 1e30 (y = 0) are inserted in
    front of frame t.  y, var [T][...]; w (T,) of positive integers (w[0] ignored).  -> y_pad, var_pad, index of every
    original frame in the padded session."""
    w = np.asarray(w)
    T = y.shape[0]
    n = np.ones(T, np.int64)
    n[1:] = np.rint(w[1:]).astype(np.int64)
    assert np.all(n >= 1) and np.all(n[1:] == w[1:])
    idx = np.cumsum(n) - 1
    Tp = int(idx[-1]) + 1
    yp = np.zeros((Tp,) + y.shape[1:], y.dtype)
    vp = np.full((Tp,) + var.shape[1:], 1e30, var.dtype)
    yp[idx], vp[idx] = y, var
    return yp, vp, idx


# ---- bars --------------------------------------------------------------------------------------------------------------
def f32_errors(ms, Vs, ref_ms, ref_Vs, y):
    """Per chain, the worst error over its scale: ms over the chain's max |y|, Vs over its own value.  [T][N] each."""
    ymax = np.abs(np.asarray(y, np.float64)).max(axis=0)
    e_m = np.abs(np.asarray(ms, np.float64) - ref_ms).max(axis=0) / ymax
    e_V = (np.abs(np.asarray(Vs, np.float64) - ref_Vs) / ref_Vs).max(axis=0)
    return dict(ms=e_m, Vs=e_V)


def f32_bars(r32_ms, r32_Vs, ref_ms, ref_Vs, y):
    """The project's float32 rule: error / scale <= max(1e-5, 4 x the float32 transcription's own worst
    error / scale on the same inputs).  -> {name: bar}."""
    et = f32_errors(r32_ms, r32_Vs, ref_ms, ref_Vs, y)
    return {k: max(1e-5, 4.0 * float(et[k].max())) for k in et}


def f64_bar(a, b, scale):
    """The float64 rule: 100 x the disagreement of the two independent float64 reference forms over the scale, floored
    at 1e-12 and capped at 1e-8."""
    return float(min(max(100.0 * np.max(np.abs(a - b) / scale), 1e-12), 1e-8))
