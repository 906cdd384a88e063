"""Float64 NumPy references of the EM entry points (TEST INFRASTRUCTURE, imported by the EM tests only): the E-step
statistic Sw = sum_t E[w_t w_t' | y] on scalar chains and general models, the filter log-likelihood with the
time-varying R, the EM loops for the scale and for a full Q, and the float32 transcription of the scalar recurrence
(float32 filter and RTS step written as eks_math.hpp states them, float64 sum) from which the float32 bars are derived.
Nothing here is compared with, or derived from, the kernels' own output."""
from __future__ import annotations

import numpy as np

from sampling_ref import VAR_CEIL, VAR_FLOOR, filter_by_scalar_updates


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_filter(y, var, m0, S0, a, c, qs):
    """N independent chains (arrays over chains; y, var [T][N]): filtered (mf, Pf) [T][N] and the log-likelihood [N]."""
    f = np.float64
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), VAR_FLOOR, VAR_CEIL)
    T, N = y.shape
    a, c, qs = (np.broadcast_to(np.asarray(x, f), (N,)) for x in (a, c, qs))
    mf, Pf = np.empty((T, N)), np.empty((T, N))
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    ll = np.zeros(N)
    for t in range(T):
        S = P * c * c + var[t]
        d = y[t] - c * m
        ll += -0.5 * (np.log(2 * np.pi * S) + d * d / S)
        mf[t] = m + P * c / S * d
        Pf[t] = P * var[t] / S
        m, P = a * mf[t], a * a * Pf[t] + qs
    return mf, Pf, ll


def scalar_loglik(y, var, m0, S0, a, c, qs):
    return scalar_filter(y, var, m0, S0, a, c, qs)[2]


def scalar_em_stats(y, var, m0, S0, a, c, qs):
    """Sw [N] = sum_{t < T-1} (E w_t)^2 + Var w_t with h = qs / Pp:  E w = h (ms' - a mf),  Var w = h^2 Vs' + a^2 Pf h."""
    mf, Pf, _ = scalar_filter(y, var, m0, S0, a, c, qs)
    T, N = mf.shape
    a, qs = (np.broadcast_to(np.asarray(x, np.float64), (N,)) for x in (a, qs))
    ms, Vs = mf[-1].copy(), Pf[-1].copy()
    Sw = np.zeros(N)
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + qs
        h, G = qs / Pp, a * Pf[t] / Pp
        ew = h * (ms - a * mf[t])
        Sw += ew * ew + (h * h * Vs + a * a * Pf[t] * h)
        ms, Vs = mf[t] + G * (ms - a * mf[t]), Pf[t] * h + G * G * Vs
    return Sw


def scalar_em_stats_f32(y, var, m0, S0, a, c, qs, unit=False):
    """The float32 transcription: the sequential filter and the backward recurrence with EVERY operation in float32 as
    eks_math.hpp states them (a x as x - (1 - a) x, a^2 x as x - (1 - a^2) x with the complements rounded once from
    float64, g = (h - (1 - a)) / a, rts_step's select between the product and the deviation form of Ps), the step's
    term (h (ms' - a mf))^2 + (h^2 Ps' + a^2 Pf h) in float32, and the sum over the steps in float64."""
    f = np.float32
    N = np.shape(y)[1]
    a64 = np.broadcast_to(np.asarray(a, np.float64), (N,))
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T = y.shape[0]
    a32, oma, oma2 = a64.astype(f), (1.0 - a64).astype(f), (1.0 - a64 * a64).astype(f)
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    q32 = np.broadcast_to(np.asarray(qs, np.float64), (N,)).astype(f)
    one, two = f(1), f(2)

    def ta(x):
        return x if unit else x - oma * x

    def ta2(x):
        return x if unit else x - oma2 * x
    mf, Pf = np.empty((T, N), f), np.empty((T, N), f)
    m, P = np.asarray(m0, np.float64).astype(f), np.asarray(S0, np.float64).astype(f)
    for t in range(T):
        Pc = P if unit else P * c32
        g = one / ((P + var[t]) if unit else (Pc * c32 + var[t]))
        d = (y[t] - m) if unit else (y[t] - c32 * m)
        mf[t] = m + Pc * g * d
        Pf[t] = P * var[t] * g
        m, P = ta(mf[t]), ta2(Pf[t]) + q32
    msn, Psn = m, P                     # frame T-1 through the phantom step from the predicted belief of frame T
    Sw = np.zeros(N)
    with np.errstate(over='ignore', invalid='ignore'):
        for t in range(T - 1, -1, -1):
            Pp = ta2(Pf[t]) + q32
            ig = one / Pp
            h = q32 * ig
            G = Pf[t] * ig if unit else a32 * Pf[t] * ig
            amf = ta(mf[t])
            g = h if unit else (h - oma) * (one / a32)
            if t < T - 1:
                ew = h * (msn - amf)
                Sw += (ew * ew + (h * h * Psn + ta2(Pf[t]) * h)).astype(np.float64)
            ms_t = mf[t] + G * (msn - amf)
            prod = Pf[t] * h + G * G * Psn
            dev = Psn + (Pf[t] * h - g * (two - g) * Psn)
            msn, Psn = ms_t, np.where((g < f(0.25)) & (g > f(-0.25)), dev, prod)
    return Sw


# ---- general models --------------------------------------------------------------------------------------------------
def dense_loglik(y, var, m0, S0, A, C, Q, s):
    """Filter log-likelihood [K] with the time-varying R, observations absorbed one at a time (exact for diagonal R).
    y, var [T][K][O]."""
    y = np.asarray(y, np.float64).transpose(1, 0, 2)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL).transpose(1, 0, 2)
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
    K, T, O = y.shape
    sQ = np.broadcast_to(np.asarray(s, np.float64), (K,))[:, None, None] * Q
    At = np.swapaxes(A, -1, -2)
    m, P = m0.copy(), S0.copy()
    ll = np.zeros(K)
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + sQ
        for o in range(O):
            h = C[:, o]
            u = np.einsum('kij,kj->ki', P, h)
            S = R[:, t, o] + np.einsum('ki,ki->k', h, u)
            d = y[:, t, o] - np.einsum('ki,ki->k', h, m)
            ll += -0.5 * (np.log(2 * np.pi * S) + d * d / S)
            m = m + u * (d / S)[:, None]
            P = P - u[:, :, None] * u[:, None, :] / S[:, None, None]
        P = 0.5 * (P + np.swapaxes(P, -1, -2))
    return ll


def dense_em_stats(y, var, m0, S0, A, C, Q, s):
    """Sw [K][D][D] in float64: with Pp = A Pf A' + sQ, G = Pf A' Pp^-1, H = sQ Pp^-1,
        E w = H (ms' - A mf),  Cov w = H Vs' H' + A (Pf - G Pp G') A',  Sw += E w E w' + Cov w.
    y, var [T][K][O]; m0 [K][D]; S0, A, Q [K][D][D]; C [K][O][D]; s [K] or scalar."""
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, K, O = y.shape
    A, C, Q, S0, m0 = (np.asarray(x, np.float64) for x in (A, C, Q, S0, m0))
    s = np.broadcast_to(np.asarray(s, np.float64), (K,))
    mf, Pf = filter_by_scalar_updates(y.transpose(1, 0, 2), m0, S0, A, C, Q, s, R.transpose(1, 0, 2))
    sQ = s[:, None, None] * Q
    At = np.swapaxes(A, -1, -2)
    ms, Vs = mf[:, -1].copy(), Pf[:, -1].copy()
    Sw = np.zeros_like(Q)
    for t in range(T - 2, -1, -1):
        Pft, mft = Pf[:, t], mf[:, t]
        Pp = A @ Pft @ At + sQ
        Pp = 0.5 * (Pp + np.swapaxes(Pp, -1, -2))
        G = np.swapaxes(np.linalg.solve(Pp, A @ Pft), -1, -2)
        H = np.swapaxes(np.linalg.solve(Pp, sQ), -1, -2)
        Gt = np.swapaxes(G, -1, -2)
        dm = ms - np.einsum('kij,kj->ki', A, mft)
        ew = np.einsum('kij,kj->ki', H, dm)
        W = Pft - G @ Pp @ Gt
        Sw += ew[:, :, None] * ew[:, None, :] + H @ Vs @ np.swapaxes(H, -1, -2) + A @ (0.5 * (W + np.swapaxes(W, -1, -2))) @ At
        ms = mft + np.einsum('kij,kj->ki', G, dm)
        V = Pft + G @ (Vs - Pp) @ Gt
        Vs = 0.5 * (V + np.swapaxes(V, -1, -2))
    return Sw


def joint_posterior_stats(y, var, m0, S0, A, C, Q, s):
    """One keypoint, Sw [D][D] by plain linear algebra on the stacked states: the joint posterior covariance
    S = (Sx^-1 + H' R^-1 H)^-1 (sampling_ref.dense_joint_posterior) and mean mu = mx + S H' R^-1 (y - H mx), then
    E[w_t w_t'] from the mean and covariance of w_t = x_{t+1} - A x_t.  y, var [T][O]."""
    from sampling_ref import dense_joint_posterior
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, O = y.shape
    D = A.shape[0]
    S = dense_joint_posterior(var, S0, A, C, Q, s)
    mx = [np.asarray(m0, np.float64)]
    for _ in range(1, T):
        mx.append(A @ mx[-1])
    mx = np.concatenate(mx)
    Hm = np.kron(np.eye(T), C)
    mu = mx + S @ Hm.T @ ((y.ravel() - Hm @ mx) / R.ravel())
    blk = lambda i, j: S[i * D:(i + 1) * D, j * D:(j + 1) * D]
    Sw = np.zeros((D, D))
    for t in range(T - 1):
        ew = mu[(t + 1) * D:(t + 2) * D] - A @ mu[t * D:(t + 1) * D]
        cw = blk(t + 1, t + 1) - A @ blk(t, t + 1) - blk(t + 1, t) @ A.T + A @ blk(t, t) @ A.T
        Sw += np.outer(ew, ew) + cw
    return Sw


# ---- the loops ---------------------------------------------------------------------------------------------------------
def trace_qinv(Q, Sw):
    """tr(Q^-1 Sw) per keypoint; Q, Sw [K][D][D]."""
    return np.trace(np.linalg.solve(Q, 0.5 * (Sw + np.swapaxes(Sw, -1, -2))), axis1=-2, axis2=-1)


def em_scale_loop(trace_fn, n_kp, log_s0, blocks, lo, hi, tol, max_iters, n_iters):
    """The scale loop as eks_em_scale_run states it.  trace_fn(s [K]) -> tr(Q^-1 Sw) [K] at those scales; n_kp: D (T-1);
    log_s0 [n_blocks]; blocks: lists of keypoints.  The first E-step runs at exp(log_s0) as given; every update is
    clipped to [lo, hi]; done = |delta log s| < tol, then ++iters; blocks done or at max_iters are left untouched.
    Returns (history [n_iters + 1][n_blocks] of log s, deltas [n_iters][n_blocks] (nan where untouched), state)."""
    K = sum(len(b) for b in blocks)
    ls = np.asarray(log_s0, np.float64).copy()
    iters, done, last = np.zeros(len(blocks), int), np.zeros(len(blocks), bool), np.zeros(len(blocks))
    hist, deltas = [ls.copy()], []
    s_k = np.empty(K)
    for b, mem in enumerate(blocks):
        s_k[list(mem)] = np.exp(ls[b])
    for _ in range(n_iters):
        tr = trace_fn(s_k.copy())
        row = np.full(len(blocks), np.nan)
        for b, mem in enumerate(blocks):
            if done[b] or iters[b] >= max_iters:
                continue
            new = np.clip(np.log(sum(tr[k] for k in mem) / (n_kp * len(mem))), lo, hi)
            row[b] = last[b] = abs(new - ls[b])
            ls[b] = new
            done[b] = row[b] < tol
            iters[b] += 1
            s_k[list(mem)] = np.exp(new)
        hist.append(ls.copy())
        deltas.append(row)
    return np.array(hist), np.array(deltas), dict(iters=iters, done=done, last=last)


def scalar_trace_fn(y, var, m0, S0, a, c, q, D, stats=scalar_em_stats, **kw):
    """trace_fn of a scalar-chain session of K keypoints x D coordinates (chain n = k D + d; a, c, q arrays over chains):
    tr(Q^-1 Sw)[k] = sum_d Sw[k D + d] / q[k D + d]."""
    def fn(s_k):
        Sw = stats(y, var, m0, S0, a, c, np.repeat(s_k, D) * q, **kw)
        return (Sw / q).reshape(-1, D).sum(axis=1)
    return fn


def dense_trace_fn(y, var, m0, S0, A, C, Q):
    return lambda s_k: trace_qinv(Q, dense_em_stats(y, var, m0, S0, A, C, Q, s_k))


def em_full_q_loop(y, var, m0, S0, A, C, Q0, n_iters):
    """Q <- sym(Sw) / (T - 1) at s = 1, n_iters times; returns the list of Q iterates (n_iters + 1 entries)."""
    T = np.shape(y)[0]
    Qs = [np.asarray(Q0, np.float64).copy()]
    for _ in range(n_iters):
        Sw = dense_em_stats(y, var, m0, S0, A, C, Qs[-1], 1.0)
        Qs.append(0.5 * (Sw + np.swapaxes(Sw, -1, -2)) / (T - 1))
    return Qs


def bar_excess(got, ref64, ref32):
    """The project's float32 rule as a ratio (<= 1 passes), per chain: |got - ref64| / |ref64| over
    max(1e-5, 4 x the transcription's own worst relative error over the chains of the case)."""
    rel = np.abs(np.asarray(got, np.float64) - ref64) / np.abs(ref64)
    trans = float((np.abs(ref32 - ref64) / np.abs(ref64)).max())
    return float(rel.max() / max(1e-5, 4.0 * trans)), float(rel.max()), trans
