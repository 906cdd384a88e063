"""Float64 NumPy references of eks_smooth_increments (TEST INFRASTRUCTURE, imported by the increments tests only):
the sequential scalar-chain smoother and the dense general-model smoother, both returning ms, Vs, lag1, dmean, dV
frame-major with row T-1 of the last three zero; the float32 transcription of the scalar recurrence (what plain
float32 arithmetic reaches without a chunk scan: it sets the float32 bars) and the float32-output transcription of
the dense reference (float64 arithmetic, one rounding)."""
from __future__ import annotations

import numpy as np

from sampling_ref import VAR_CEIL, VAR_FLOOR, filter_by_scalar_updates


def scalar_increments(y, var, m0, S0, a, c, qs):
    """N independent chains, arrays over chains; y, var [T][N].  (m, P) entering frame t is the predicted belief.
    Returns ms, Vs, lag1, dmean, dV [T][N] in float64:
        lag1[t] = G Vs[t+1],  dmean[t] = ms[t+1] - ms[t],  dV[t] = (1 - G)^2 Vs[t+1] + Pf q s / Pp,  G = a Pf / Pp."""
    f = np.float64
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), VAR_FLOOR, VAR_CEIL)
    a, c, qs = (np.broadcast_to(np.asarray(x, f), y.shape[1:]) for x in (a, c, qs))
    T, N = y.shape
    mf, Pf = np.empty((T, N)), np.empty((T, N))
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    for t in range(T):
        g = 1 / (P * c * c + var[t])
        mf[t] = m + P * c * g * (y[t] - c * m)
        Pf[t] = P * var[t] * g
        m, P = a * mf[t], a * a * Pf[t] + qs
    ms, Vs = np.empty_like(mf), np.empty_like(Pf)
    lag1, dmean, dV = np.zeros_like(Pf), np.zeros_like(Pf), np.zeros_like(Pf)
    ms[-1], Vs[-1] = mf[-1], Pf[-1]
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + qs
        G = a * Pf[t] / Pp
        inn = Pf[t] * (qs / Pp)
        ms[t] = mf[t] + G * (ms[t + 1] - a * mf[t])
        Vs[t] = inn + G * G * Vs[t + 1]
        lag1[t] = G * Vs[t + 1]
        dmean[t] = ms[t + 1] - ms[t]
        dV[t] = (1 - G) ** 2 * Vs[t + 1] + inn
    return ms, Vs, lag1, dmean, dV


def scalar_increments_f32(y, var, m0, S0, a, c, qs, unit=False):
    """The float32 transcription: the sequential filter and the backward recurrence with EVERY operation in float32,
    written as the issue's table and eks_math.hpp state them: a x formed as x - (1 - a) x and a^2 x as
    x - (1 - a^2) x with 1 - a, 1 - a^2 rounded once from float64, g = (h - (1 - a)) / a, rts_step's select between
    the product and the deviation form of Ps, and
        lag1 = G Ps',  dmean = g (ms' - a mf) - (1 - a) mf  (unit: h (ms' - mf)),  dV = g^2 Ps' + Pf h."""
    f = np.float32
    a64 = np.broadcast_to(np.asarray(a, np.float64), np.shape(y)[1:])
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T, N = y.shape
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
    ms, Vs = np.empty_like(mf), np.empty_like(Pf)
    lag1, dmean, dV = np.zeros_like(Pf), np.zeros_like(Pf), np.zeros_like(Pf)
    # frame T-1 through the phantom step from the predicted belief of frame T, as the kernels reach it
    msn, Psn = m, P
    for t in range(T - 1, -1, -1):
        Pp = ta2(Pf[t]) + q32
        ig = one / Pp
        h = q32 * ig
        G = Pf[t] * ig if unit else a32 * Pf[t] * ig
        amf = ta(mf[t])
        g = h if unit else (h - oma) * (one / a32)
        if t < T - 1:
            lag1[t] = G * Psn
            dmean[t] = g * (msn - amf) if unit else g * (msn - amf) - oma * mf[t]
            dV[t] = g * g * Psn + Pf[t] * h
        ms[t] = mf[t] + G * (msn - amf)
        prod = Pf[t] * h + G * G * Psn
        dev = Psn + (Pf[t] * h - g * (two - g) * Psn)
        Vs[t] = np.where((g < f(0.25)) & (g > f(-0.25)), dev, prod)
        msn, Psn = ms[t], Vs[t]
    return ms, Vs, lag1, dmean, dV


def dense_increments(y, var, m0, S0, A, C, Q, s):
    """General (D, O) models in float64: y, var [T][K][O]; m0 [K][D]; S0, A, Q [K][D][D]; C [K][O][D]; s [K].  The
    filter absorbs a frame's observations one at a time (sampling_ref.filter_by_scalar_updates); backwards, with
    Pp = A Pf A' + s Q and G = Pf A' Pp^-1 (only Pp is solved against: a singular Q is fine),
        lag1[t] = G Vs[t+1]            (row: coordinate of x_t, column: of x_{t+1})
        dmean[t] = ms[t+1] - ms[t]
        dV[t] = (I - G) Vs[t+1] (I - G)' + (Pf - G Pp G').
    Returns ms [T][K][D], Vs, lag1, dV [T][K][D][D], dmean [T][K][D]; row T-1 of lag1, dmean, dV is zero."""
    y = np.asarray(y, np.float64)
    R = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, K, O = y.shape
    A, C, Q, S0, m0 = (np.asarray(x, np.float64) for x in (A, C, Q, S0, m0))
    s = np.broadcast_to(np.asarray(s, np.float64), (K,))
    D = A.shape[-1]
    mf, Pf = filter_by_scalar_updates(y.transpose(1, 0, 2), m0, S0, A, C, Q, s, R.transpose(1, 0, 2))
    mf, Pf = mf.transpose(1, 0, 2), Pf.transpose(1, 0, 2, 3)
    sQ = s[:, None, None] * Q
    At = np.swapaxes(A, -1, -2)
    eye = np.eye(D)
    ms, Vs = np.empty((T, K, D)), np.empty((T, K, D, D))
    lag1, dmean, dV = np.zeros((T, K, D, D)), np.zeros((T, K, D)), np.zeros((T, K, D, D))
    ms[-1], Vs[-1] = mf[-1], Pf[-1]
    for t in range(T - 2, -1, -1):
        Pp = A @ Pf[t] @ At + sQ
        Pp = 0.5 * (Pp + np.swapaxes(Pp, -1, -2))
        G = np.swapaxes(np.linalg.solve(Pp, A @ Pf[t]), -1, -2)                 # Pf A' Pp^-1
        Gt = np.swapaxes(G, -1, -2)
        ms[t] = mf[t] + np.einsum('kij,kj->ki', G, ms[t + 1] - np.einsum('kij,kj->ki', A, mf[t]))
        V = Pf[t] + G @ (Vs[t + 1] - Pp) @ Gt
        Vs[t] = 0.5 * (V + np.swapaxes(V, -1, -2))
        lag1[t] = G @ Vs[t + 1]
        dmean[t] = ms[t + 1] - ms[t]
        ImG = eye - G
        W = Pf[t] - G @ Pp @ Gt
        X = ImG @ Vs[t + 1] @ np.swapaxes(ImG, -1, -2) + 0.5 * (W + np.swapaxes(W, -1, -2))
        dV[t] = 0.5 * (X + np.swapaxes(X, -1, -2))
    return ms, Vs, lag1, dmean, dV


def dense_increments_f32out(*args):
    """The float32-output transcription of dense_increments: float64 arithmetic, every output rounded once."""
    return tuple(o.astype(np.float32) for o in dense_increments(*args))


def bar_rule(err, trans_err, scale):
    """The issue's bar for a float32 output: |error| <= max(1e-5 scale, 4 x the transcription's own worst error),
    with scale and the transcription's error per chain (arrays over the trailing axes).  Returns worst error / bar."""
    bar = np.maximum(1e-5 * scale, 4.0 * trans_err)
    return float((err / bar).max())
