"""Float64 NumPy references of eks_innovations (TEST INFRASTRUCTURE, imported by the innovations tests only): the
one-step-ahead prediction errors, their variances and the log-likelihood of the model eks_smooth runs, on scalar
chains and on general models in two independent forms (observations absorbed one at a time; S_t built as a matrix and
factored by numpy.linalg.cholesky), the Gaussian log-density of the stacked observations by plain linear algebra,
and the float32 transcription of the scalar recurrence (every operation in float32 as eks_math.hpp states it, the
frame's term in float32, the sum in float64) from which the float32 bars are derived.  Nothing here is compared with,
or derived from, the kernels' own output."""
from __future__ import annotations

import numpy as np

from sampling_ref import VAR_CEIL, VAR_FLOOR

LOG2PI = float(np.log(2.0 * np.pi))


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_innovations(y, var, m0, S0, a, c, qs):
    """em_ref.scalar_filter that returns the prediction errors: N independent chains (arrays over chains; y, var
    [T][N]) -> v [T][N], S [T][N], loglik [N]."""
    f = np.float64
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), VAR_FLOOR, VAR_CEIL)
    T, N = y.shape
    a, c, qs = (np.broadcast_to(np.asarray(x, f), (N,)) for x in (a, c, qs))
    v, S = np.empty((T, N)), np.empty((T, N))
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    ll = np.zeros(N)
    for t in range(T):
        S[t] = P * c * c + var[t]
        v[t] = y[t] - c * m
        ll += -0.5 * (np.log(2 * np.pi * S[t]) + v[t] * v[t] / S[t])
        mf = m + P * c / S[t] * v[t]
        Pf = P * var[t] / S[t]
        m, P = a * mf, a * a * Pf + qs
    return v, S, ll


def scalar_innovations_f32(y, var, m0, S0, a, c, qs, unit=False):
    """The float32 transcription: filter_step with EVERY operation in float32 as eks_math.hpp states it (a x as
    x - (1 - a) x, a^2 x as x - (1 - a^2) x with the complements rounded once from float64, the update through
    g = 1 / S), the frame's term log 2 pi + log S + d^2 g in float32, and the sum over the frames in float64.
    -> v [T][N] float32, S [T][N] float32, loglik [N] float64."""
    f = np.float32
    N = np.shape(y)[1]
    a64 = np.broadcast_to(np.asarray(a, np.float64), (N,))
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T = y.shape[0]
    oma, oma2 = (1.0 - a64).astype(f), (1.0 - a64 * a64).astype(f)
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    q32 = np.broadcast_to(np.asarray(qs, np.float64), (N,)).astype(f)
    one, log2pi = f(1), f(LOG2PI)

    def ta(x):
        return x if unit else x - oma * x

    def ta2(x):
        return x if unit else x - oma2 * x
    v, S = np.empty((T, N), f), np.empty((T, N), f)
    m, P = np.asarray(m0, np.float64).astype(f), np.asarray(S0, np.float64).astype(f)
    acc = np.zeros(N)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in range(T):
            Pc = P if unit else P * c32
            S[t] = (P + var[t]) if unit else (Pc * c32 + var[t])
            g = one / S[t]
            v[t] = (y[t] - m) if unit else (y[t] - c32 * m)
            acc += (log2pi + np.log(S[t]) + v[t] * v[t] * g).astype(np.float64)
            mf = m + Pc * g * v[t]
            Pf = P * var[t] * g
            m, P = ta(mf), ta2(Pf) + q32
    return v, S, -0.5 * acc


# ---- general models --------------------------------------------------------------------------------------------------
def _prep(y, var, m0, S0, A, C, Q, s):
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
    T, K, O = y.shape
    sQ = np.broadcast_to(np.asarray(s, np.float64), (K,))[:, None, None] * Q
    return y, R, m0, S0, A, C, sQ, T, K, O


def dense_innovations_sequential(y, var, m0, S0, A, C, Q, s):
    """The sequential-update form, as em_ref.dense_loglik: observations absorbed one at a time (exact for diagonal R);
    log det S_t = sum_o log sigma_o and nis = sum_o d_o^2 / sigma_o over the conditional scalar updates, innov and
    innov_var from the predicted belief.  y, var [T][K][O] -> dict of innov, innov_var [T][K][O], nis, frame_ll
    [T][K], loglik [K]."""
    y, R, m0, S0, A, C, sQ, T, K, O = _prep(y, var, m0, S0, A, C, Q, s)
    At = np.swapaxes(A, -1, -2)
    m, P = m0.copy(), S0.copy()
    out = dict(innov=np.empty((T, K, O)), innov_var=np.empty((T, K, O)), nis=np.empty((T, K)), frame_ll=np.empty((T, K)))
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + sQ
        out['innov'][t] = y[t] - np.einsum('koi,ki->ko', C, m)
        out['innov_var'][t] = np.einsum('koi,kij,koj->ko', C, P, C) + R[t]
        sl, sq = np.zeros(K), np.zeros(K)
        for o in range(O):
            h = C[:, o]
            u = np.einsum('kij,kj->ki', P, h)
            sig = R[t, :, o] + np.einsum('ki,ki->k', h, u)
            d = y[t, :, o] - np.einsum('ki,ki->k', h, m)
            sl += np.log(sig)
            sq += d * d / sig
            m = m + u * (d / sig)[:, None]
            P = P - u[:, :, None] * u[:, None, :] / sig[:, None, None]
        P = 0.5 * (P + np.swapaxes(P, -1, -2))
        out['nis'][t] = sq
        out['frame_ll'][t] = -0.5 * (O * LOG2PI + sl + sq)
    out['loglik'] = out['frame_ll'].sum(axis=0)
    return out


def dense_innovations_joint(y, var, m0, S0, A, C, Q, s):
    """The joint form, independent of the above: S_t = C P C' + R_t as a matrix, numpy.linalg.cholesky, log det and
    the solve from the factor, the update through the gain K = P C' S^-1 in Joseph form.  Same outputs."""
    y, R, m0, S0, A, C, sQ, T, K, O = _prep(y, var, m0, S0, A, C, Q, s)
    At, Ct = np.swapaxes(A, -1, -2), np.swapaxes(C, -1, -2)
    eye = np.eye(A.shape[-1])
    m, P = m0.copy(), S0.copy()
    out = dict(innov=np.empty((T, K, O)), innov_var=np.empty((T, K, O)), nis=np.empty((T, K)), frame_ll=np.empty((T, K)))
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + sQ
        Rt = np.zeros((K, O, O))
        Rt[:, np.arange(O), np.arange(O)] = R[t]
        S = C @ P @ Ct + Rt
        S = 0.5 * (S + np.swapaxes(S, -1, -2))
        v = y[t] - np.einsum('koi,ki->ko', C, m)
        L = np.linalg.cholesky(S)
        w = np.linalg.solve(L, v[:, :, None])[:, :, 0]                       # L^-1 v
        nis = (w * w).sum(axis=1)
        logdet = 2.0 * np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
        out['innov'][t], out['innov_var'][t] = v, np.diagonal(S, axis1=1, axis2=2)
        out['nis'][t] = nis
        out['frame_ll'][t] = -0.5 * (O * LOG2PI + logdet + nis)
        G = np.swapaxes(np.linalg.solve(S, C @ P), -1, -2)                    # P C' S^-1
        m = m + np.einsum('kio,ko->ki', G, v)
        IGC = eye - G @ C
        P = IGC @ P @ np.swapaxes(IGC, -1, -2) + G @ Rt @ np.swapaxes(G, -1, -2)
        P = 0.5 * (P + np.swapaxes(P, -1, -2))
    out['loglik'] = out['frame_ll'].sum(axis=0)
    return out


def joint_log_density(y, var, m0, S0, A, C, Q, s):
    """One keypoint: log N(y; mean, cov) of the stacked observations, with the T.O x T.O covariance H Sx H' + R built
    from the prior covariance of the stacked states (Cov(x_u, x_t) = A^(u-t) P_t for u >= t).  y, var [T][O]."""
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
    T, O = y.shape
    D = A.shape[0]
    Pt, mx = [S0], [m0]
    for _ in range(1, T):
        Pt.append(A @ Pt[-1] @ A.T + s * Q)
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
    r = y.ravel() - H @ np.concatenate(mx)
    _, logdet = np.linalg.slogdet(cov)
    return -0.5 * (T * O * LOG2PI + logdet + r @ np.linalg.solve(cov, r))


# ---- diagnostics and bars ----------------------------------------------------------------------------------------------
def lag1_autocorr(z):
    """Lag-one autocorrelation along axis 0, per column."""
    zc = z - z.mean(axis=0, keepdims=True)
    return (zc[1:] * zc[:-1]).sum(axis=0) / (zc * zc).sum(axis=0)


def f32_errors(got, ref):
    """Per chain, (innov, innov_var, loglik) errors over their scales: innov over the chain's max |y| (passed in ref),
    innov_var over its own value, loglik over max(|loglik|, T).  got, ref: dicts of v, S, ll (ref also y)."""
    T = ref['v'].shape[0]
    ymax = np.abs(ref['y']).max(axis=0)
    e_v = np.abs(np.asarray(got['v'], np.float64) - ref['v']).max(axis=0) / ymax
    e_S = (np.abs(np.asarray(got['S'], np.float64) - ref['S']) / ref['S']).max(axis=0)
    e_ll = np.abs(got['ll'] - ref['ll']) / np.maximum(np.abs(ref['ll']), T)
    return dict(v=e_v, S=e_S, ll=e_ll)


def f32_rule(got, r32, ref):
    """The project's float32 rule: per chain, error / scale <= max(1e-5, 4 x the transcription's own worst error /
    scale on the same inputs).  Returns {name: (excess ratio (<= 1 passes), worst error, transcription's worst)}."""
    eg, et = f32_errors(got, ref), f32_errors(r32, ref)
    return {k: (float((eg[k] / np.maximum(1e-5, 4.0 * et[k].max())).max()), float(eg[k].max()), float(et[k].max()))
            for k in eg}


def f64_bar(a, b, scale):
    """The float64 rule: 100 x the disagreement of the two independent float64 reference forms over the scale, floored
    at 1e-12 and capped at 1e-8."""
    return float(min(max(100.0 * np.max(np.abs(a - b) / scale), 1e-12), 1e-8))
