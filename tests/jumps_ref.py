"""Float64 NumPy references of eks_smooth_jumps (TEST INFRASTRUCTURE, imported by the jumps tests only): the
mean-field iteration for Student-t process noise with one weight per keypoint and frame,

    x_t = A x_{t-1} + eps_t,   eps_t | u_t ~ N(0, s Q / u_t),   u_t ~ Gamma(nu / 2, rate nu / 2),   t = 1 .. T-1,

around the sequential smoothers of tests/smooth_tv_ref.py under the per-keypoint scales w = 1 / u: scalar chains with
a shared keypoint weight, general models in two independent forms (ms, Vs from smooth_tv_ref's two forms; the filtered
beliefs delta needs from a filter of the same form, the first through solves, the second through explicit inverses),
delta_t = E[eps_t' (s Q)^-1 eps_t | y] from the joint Gaussian posterior by plain linear algebra, the float32
transcription of the scalar lane arithmetic in the lanes' own organisation (chunk elements, grouped scan, replay with
eks_smooth_jumps_lane.hpp's rts_step_jumps, every operation in float32; the combine in float64 rounded once), and the variational bound.  A call of n_iters passes smooths n_iters
times and updates the scales n_iters - 1 times: the scales returned are the ones ms, Vs were smoothed under.  Row 0 of
the scales is 1 and unused.  Nothing here is compared with, or derived from, the kernels' own output."""
from __future__ import annotations

import math

import numpy as np

import smooth_tv_ref as tref
from robust_ref import digamma, kl_gamma
from sampling_ref import VAR_CEIL, VAR_FLOOR

U_FLOOR = 1e-30


def _clip(v):
    return np.clip(v, VAR_FLOOR, VAR_CEIL)


def new_scales(delta, nu, D):
    """delta [T][K] (row 0 ignored) -> w = 1 / u, u = (nu + D) / (nu + delta) kept in [U_FLOOR, (nu + D) / nu]."""
    u = np.clip((nu + D) / (nu + delta), U_FLOOR, (nu + D) / nu)
    w = 1.0 / u
    w[0] = 1.0
    return w


def _change(w_new, w_old):
    return np.abs(1.0 / w_new[1:] - 1.0 / w_old[1:]).max(axis=0) if w_new.shape[0] > 1 else np.zeros(w_new.shape[1])


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_pass(y, var, m0, S0, a, c, qs, w, D):
    """One Gaussian pass under w [T][K] on N = K D chains.  -> ms, Vs [T][N], delta [T][K] (row 0 zero), loglik [K]."""
    f = np.float64
    y, r = np.asarray(y, f), _clip(np.asarray(var, f))
    T, N = y.shape
    a, c, qs = (np.broadcast_to(np.asarray(x, f), (N,)) for x in (a, c, qs))
    wn = np.repeat(np.asarray(w, f), D, axis=1)
    q = qs[None] * wn
    mf, Pf, ll = np.empty((T, N)), np.empty((T, N)), np.zeros(N)
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    for t in range(T):
        if t:
            m, P = a * m, a * a * P + q[t]
        S = P * c * c + r[t]
        d = y[t] - c * m
        ll += -0.5 * (np.log(2 * np.pi * S) + d * d / S)
        m = m + P * c / S * d
        P = P * r[t] / S
        mf[t], Pf[t] = m, P
    ms, Vs = tref.scalar_smooth_tv(y, var, m0, S0, a, c, qs, w, D)
    contrib = np.zeros((T, N))
    for t in range(1, T):
        Pp = a * a * Pf[t - 1] + q[t]
        h = q[t] / Pp
        dm = ms[t] - a * mf[t - 1]
        with np.errstate(invalid='ignore', divide='ignore'):
            term = (h * (dm * dm + Vs[t]) + a * a * Pf[t - 1]) / Pp
        contrib[t] = np.where(q[t] > 0, wn[t] * term, wn[t])
    return ms, Vs, contrib.reshape(T, N // D, D).sum(axis=2), ll.reshape(N // D, D).sum(axis=1)


def scalar_jumps(y, var, m0, S0, a, c, qs, nu, n_iters, D=1, w0=None, history=None, snapshots=None):
    """-> ms, Vs [T][N], w [T][K] float64 and change [K] (max |u_new - u_old| of the last update, 0 when
    n_iters == 1).  history: a list that receives (w the pass smoothed under, delta it formed, loglik) per pass.
    snapshots: a dict whose keys n <= n_iters receive what a call of n passes returns."""
    T, N = np.shape(y)
    K = N // D
    w = np.ones((T, K)) if w0 is None else np.asarray(w0, np.float64).copy()
    w[0] = 1.0
    change = np.zeros(K)
    for it in range(n_iters):
        ms, Vs, delta, ll = scalar_pass(y, var, m0, S0, a, c, qs, w, D)
        if history is not None:
            history.append((w.copy(), delta, ll))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, w.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = new_scales(delta, nu, D)
        change = _change(new, w)
        w = new
    return ms, Vs, w, change


def _pass_f32(y, var, m0, S0, a, c, qs, w32, D, unit, B=32):
    """The float32 transcription of one pass as the lanes organise it: per chunk of B frames elem_append with the
    frame's own q, the grouped scan (elem_combine over groups of ceil(sqrt(nc)) chunks, elem_apply forwards, elem_back
    backwards), then per chunk filter_step from the belief that entered it, fuse_info with the information after it
    and rts_gain / rts_advance backwards with rts_step_jumps' term - every operation in float32 as eks_math.hpp and
    eks_smooth_jumps_lane.hpp state it (a = c = 1 and zero complements reproduce the UNIT forms exactly).  The belief
    at a chunk boundary comes out of the scan in absolute coordinates, and dm = m' - a mf cancels against it: a
    frame-by-frame transcription has no such boundary and under-states the error of delta there.
    -> ms, Vs, contrib [T][N] float32 (contrib row 0 zero)."""
    f = np.float32
    N = np.shape(y)[1]
    a64 = np.ones(N) if unit else np.broadcast_to(np.asarray(a, np.float64), (N,))
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T = y.shape[0]
    a32, oma, oma2 = a64.astype(f), (1.0 - a64).astype(f), (1.0 - a64 * a64).astype(f)
    c32 = np.ones(N, f) if unit else np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    q32 = np.broadcast_to(np.asarray(qs, np.float64), (N,)).astype(f)
    wn = np.concatenate([np.repeat(np.asarray(w32, f), D, axis=1), np.ones((1, N), f)])
    one, two, quarter = f(1), f(2), f(0.25)
    ira = one / a32
    ta = lambda x: x - oma * x
    ta2 = lambda x: x - oma2 * x
    ident = lambda: [np.ones(N, f), np.zeros(N, f), np.zeros(N, f), np.zeros(N, f), np.zeros(N, f)]

    def combine(i, j):
        inv = one / (one + i[2] * j[4])
        AjI, AiI = j[0] * inv, i[0] * inv
        return [AjI * i[0], AjI * (i[1] + i[2] * j[3]) + j[1], AjI * j[0] * i[2] + j[2],
                AiI * (j[3] - j[4] * i[1]) + i[3], AiI * i[0] * j[4] + i[4]]

    def apply(e, m, P):
        AI = e[0] * (one / (one + e[4] * P))
        return AI * (m + P * e[3]) + e[1], AI * e[0] * P + e[2]

    def back(e, eta, J):
        AI = e[0] * (one / (one + e[2] * J))
        return AI * (eta - J * e[1]) + e[3], AI * e[0] * J + e[4]

    nc = (T + B - 1) // B
    gs = 1
    while gs * gs < nc:
        gs += 1
    ng = (nc + gs - 1) // gs
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        elems = []
        for j in range(nc):
            A_, b_, C_, eta, J = ident()
            for t in range(j * B, min(T, (j + 1) * B)):
                q = q32 * wn[t + 1]
                Cc = C_ * c32
                g = one / (var[t] + Cc * c32)
                d = y[t] - c32 * b_
                rg = var[t] * g
                Acg = A_ * c32 * g
                eta = eta + Acg * d
                J = J + Acg * A_ * c32
                b_ = ta(b_ + Cc * g * d)
                A_ = ta(A_ * rg)
                C_ = ta2(C_ * rg) + q
            elems.append([A_, b_, C_, eta, J])
        groups = []
        for g_ in range(ng):
            e = ident()
            for j in range(g_ * gs, min(nc, (g_ + 1) * gs)):
                e = combine(e, elems[j])
            groups.append(e)
        m, P = np.asarray(m0, np.float64).astype(f), np.asarray(S0, np.float64).astype(f)
        gm = []
        for g_ in range(ng):
            gm.append((m, P))
            m, P = apply(groups[g_], m, P)
        eta, J = np.zeros(N, f), np.zeros(N, f)
        gsuf = [None] * ng
        for g_ in range(ng - 1, -1, -1):
            gsuf[g_] = (eta, J)
            eta, J = back(groups[g_], eta, J)
        pre, suf = [None] * nc, [None] * nc
        for g_ in range(ng):
            j0, j1 = g_ * gs, min(nc, (g_ + 1) * gs)
            m, P = gm[g_]
            for j in range(j0, j1):
                pre[j] = (m, P)
                m, P = apply(elems[j], m, P)
            eta, J = gsuf[g_]
            for j in range(j1 - 1, j0 - 1, -1):
                suf[j] = (eta, J)
                eta, J = back(elems[j], eta, J)
        ms, Vs, contrib = np.empty((T, N), f), np.empty((T, N), f), np.zeros((T, N), f)
        mf, Pf = np.empty((T, N), f), np.empty((T, N), f)
        for j in range(nc):
            t0, t1 = j * B, min(T, (j + 1) * B)
            m, P = pre[j]
            for t in range(t0, t1):
                q = q32 * wn[t + 1]
                Pc = P * c32
                g = one / (Pc * c32 + var[t])
                d = y[t] - c32 * m
                mf[t] = m + Pc * g * d
                Pf[t] = P * var[t] * g
                m, P = ta(mf[t]), ta2(Pf[t]) + q
            eta, J = suf[j]
            inv = one / (one + J * P)
            m, P = (m + P * eta) * inv, P * inv
            for t in range(t1 - 1, t0 - 1, -1):
                q = q32 * wn[t + 1]
                a2Pf = ta2(Pf[t])
                ig = one / (a2Pf + q)
                h = q * ig
                G = a32 * Pf[t] * ig
                amf = ta(mf[t])
                gg = (h - oma) * ira
                if t + 1 < T:
                    dm = m - amf
                    term = (h * (dm * dm + P) + a2Pf) * ig
                    contrib[t + 1] = np.where(q > 0, wn[t + 1] * term, wn[t + 1])
                m = mf[t] + G * (m - amf)
                prod = Pf[t] * h + G * G * P
                dev = P + (Pf[t] * h - gg * (two - gg) * P)
                P = np.where((gg < quarter) & (gg > -quarter), dev, prod).astype(f)
                ms[t], Vs[t] = m, P
    return ms, Vs, contrib


def combine_f32(contrib, w32, nu, D, nd):
    """jumps_combine_lane: float64 inside, w rounded once to float32.  contrib [T][K nd] -> w [T][K] float32, change."""
    T = contrib.shape[0]
    delta = np.asarray(contrib, np.float64).reshape(T, -1, nd).sum(axis=2)
    u = np.clip((nu + D) / (nu + delta), U_FLOOR, (nu + D) / nu)
    new = (1.0 / u).astype(np.float32)
    new[0] = 1.0
    ch = np.abs(u[1:] - 1.0 / w32[1:].astype(np.float64)).max(axis=0) if T > 1 else np.zeros(new.shape[1])
    return new, ch.astype(np.float32)


def scalar_jumps_f32(y, var, m0, S0, a, c, qs, nu, n_iters, D=1, w0=None, unit=False, B=32, snapshots=None):
    """The float32 transcription of a call in chunks of B frames (the kernels': 32).  Same outputs as scalar_jumps,
    float32; snapshots as there."""
    T, N = np.shape(y)
    K = N // D
    w = np.ones((T, K), np.float32) if w0 is None else np.asarray(w0, np.float32).copy()
    w[0] = 1.0
    change = np.zeros(K, np.float32)
    for it in range(n_iters):
        ms, Vs, contrib = _pass_f32(y, var, m0, S0, a, c, qs, w, D, unit, B)
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, w.copy(), change.copy())
        if it == n_iters - 1:
            break
        w, change = combine_f32(contrib, w, nu, D, D)
    return ms, Vs, w, change


# ---- general models --------------------------------------------------------------------------------------------------
def _filter_solve(y, R, m0, S0, A, C, sQ, wk):
    """Observations absorbed one at a time (smooth_tv_ref.dense_smooth_tv's filter).  -> mf, Pf, loglik [K]."""
    T, K, O = y.shape
    D = A.shape[-1]
    At = np.swapaxes(A, -1, -2)
    mf, Pf, ll = np.empty((T, K, D)), np.empty((T, K, D, D)), np.zeros(K)
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
            ll += -0.5 * (np.log(2 * np.pi * sig) + d * d / sig)
            m = m + u * (d / sig)[:, None]
            P = P - u[:, :, None] * u[:, None, :] / sig[:, None, None]
        P = tref._sym(P)
        mf[t], Pf[t] = m, P
    return mf, Pf, ll


def _filter_joseph(y, R, m0, S0, A, C, sQ, wk):
    """The update through the gain with S_t as a matrix, Joseph form (smooth_tv_ref.dense_smooth_tv_joint's filter)."""
    T, K, O = y.shape
    D = A.shape[-1]
    At, Ct = np.swapaxes(A, -1, -2), np.swapaxes(C, -1, -2)
    eye = np.eye(D)
    mf, Pf, ll = np.empty((T, K, D)), np.empty((T, K, D, D)), np.zeros(K)
    m, P = m0.copy(), S0.copy()
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + wk[t][:, None, None] * sQ
        Rt = np.zeros((K, O, O))
        Rt[:, np.arange(O), np.arange(O)] = R[t]
        S = tref._sym(C @ P @ Ct + Rt)
        G = np.swapaxes(np.linalg.solve(S, C @ P), -1, -2)
        d = y[t] - np.einsum('koi,ki->ko', C, m)
        ll += -0.5 * (O * math.log(2 * math.pi) + np.linalg.slogdet(S)[1]
                      + np.einsum('ko,ko->k', d, np.linalg.solve(S, d[..., None])[..., 0]))
        m = m + np.einsum('kio,ko->ki', G, d)
        IGC = eye - G @ C
        P = tref._sym(IGC @ P @ np.swapaxes(IGC, -1, -2) + G @ Rt @ np.swapaxes(G, -1, -2))
        mf[t], Pf[t] = m, P
    return mf, Pf, ll


def dense_pass(y, var, m0, S0, A, C, Q, s, w, form=tref.dense_smooth_tv):
    """One Gaussian pass under w [T][K].  -> ms [T][K][D], Vs [T][K][D][D], delta [T][K] (row 0 zero), loglik [K].
    delta_t = w_t [ tr(Pp^-1 (P' + dm dm') Pp^-1 (s w_t Q)) + tr(Pp^-1 A Pf A') ]: Q is never inverted."""
    yy, R, m0, S0, A, C, sQ, wk, T, K, O = tref._prep(y, var, m0, S0, A, C, Q, s, w)
    ms, Vs = form(y, var, m0, S0, A, C, Q, s, w)
    solve = form is tref.dense_smooth_tv
    mf, Pf, ll = (_filter_solve if solve else _filter_joseph)(yy, R, m0, S0, A, C, sQ, wk)
    At = np.swapaxes(A, -1, -2)
    delta = np.zeros((T, K))
    for t in range(1, T):
        sQw = wk[t][:, None, None] * sQ
        APA = A @ Pf[t - 1] @ At
        Pp = tref._sym(APA + sQw)
        dm = ms[t] - np.einsum('kij,kj->ki', A, mf[t - 1])
        Mm = Vs[t] + dm[:, :, None] * dm[:, None, :]
        if solve:
            tr1 = np.trace(np.linalg.solve(Pp, Mm) @ np.linalg.solve(Pp, sQw), axis1=-2, axis2=-1)
            tr2 = np.trace(np.linalg.solve(Pp, APA), axis1=-2, axis2=-1)
        else:
            Pi = np.linalg.inv(Pp)
            tr1 = np.einsum('kij,kjl,klm,kmi->k', Pi, Mm, Pi, sQw)
            tr2 = np.einsum('kij,kji->k', Pi, APA)
        delta[t] = wk[t] * (tr1 + tr2)
    return ms, Vs, delta, ll


def dense_jumps(y, var, m0, S0, A, C, Q, s, nu, n_iters, w0=None, form=tref.dense_smooth_tv, history=None,
                snapshots=None, w_dtype=np.float64):
    """y, var [T][K][O] -> ms [T][K][D], Vs [T][K][D][D], w [T][K], change [K].  w_dtype = numpy.float32: every new
    scale is rounded to float32, what the C ABI's plane holds (the general path computes in float64 but keeps its
    scales there)."""
    T, K, _ = np.shape(y)
    D = np.shape(A)[-1]
    w = np.ones((T, K)) if w0 is None else np.asarray(w0, np.float64).copy()
    w[0] = 1.0
    change = np.zeros(K)
    for it in range(n_iters):
        ms, Vs, delta, ll = dense_pass(y, var, m0, S0, A, C, Q, s, w, form)
        if history is not None:
            history.append((w.copy(), delta, ll))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, w.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = new_scales(delta, nu, D)
        change = (np.abs(np.clip((nu + D) / (nu + delta[1:]), U_FLOOR, (nu + D) / nu) - 1.0 / w[1:]).max(axis=0)
                  if T > 1 else np.zeros(K))
        w = new.astype(w_dtype).astype(np.float64)
    return ms, Vs, w, change


def joint_delta(y, var, m0, S0, A, C, Q, s, w):
    """One keypoint: delta_t for t = 1 .. T-1 from the joint Gaussian posterior of the stacked states by plain linear
    algebra: eps_t = x_t - A x_{t-1}, delta_t = tr((s Q)^+ E[eps_t eps_t' | y]) + w_t (D - rank Q) - the directions Q
    does not move carry no noise and count their prior value w_t each (s q = 0 on a scalar chain).  y, var [T][O];
    w (T,).  -> delta (T,) with delta[0] = 0."""
    y = np.asarray(y, np.float64)
    R = _clip(np.asarray(var, np.float64))
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
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
    mu = mxs + SH @ np.linalg.solve(cov, y.ravel() - H @ mxs)
    Sig = Sx - SH @ np.linalg.solve(cov, SH.T)
    Qp = np.linalg.pinv(s * Q, hermitian=True)
    rank = np.linalg.matrix_rank(Q, hermitian=True)
    M = np.hstack([-A, np.eye(D)])
    out = np.zeros(T)
    for t in range(1, T):
        sl = slice((t - 1) * D, (t + 1) * D)
        e = M @ mu[sl]
        out[t] = np.trace(Qp @ (M @ Sig[sl, sl] @ M.T + np.outer(e, e))) + w[t] * (D - rank)
    return out


# ---- the bound -------------------------------------------------------------------------------------------------------
def elbo(loglik, delta_prev, nu, D):
    """The bound after the smoothing pass under u_bar_t = alpha / beta_t, alpha = (nu + D) / 2,
    beta_t = (nu + delta_prev_t) / 2 (nonsingular Q): loglik [K] is the Gaussian log-likelihood of y under the scales
    1 / u_bar, delta_prev [T][K] the delta of the pass before (row 0 carries no weight)."""
    alpha = 0.5 * (nu + D)
    beta = 0.5 * (nu + np.asarray(delta_prev, np.float64)[1:])
    terms = 0.5 * D * (digamma(alpha) - math.log(alpha)) - kl_gamma(alpha, beta, 0.5 * nu, 0.5 * nu)
    return loglik + terms.sum(axis=0)


def elbo_path(history, nu, D):
    """ELBO after passes 2 .. n of a history (pass 1 has no q(u) yet).  -> [n - 1][K]."""
    return np.array([elbo(history[i][2], history[i - 1][1], nu, D) for i in range(1, len(history))])


# ---- sessions and bars -----------------------------------------------------------------------------------------------
JUMP_FRAMES = (1, 100, 101, 250, 431, -1)


def jump_session(seed, T=600, sq=0.05):
    """The feature's session: one keypoint, two coordinates sharing one weight, a random walk with s q = sq, variances
    U(0.5, 2), displacements of +-20..40 px in both coordinates entering frames 1, 100, 101, 250, 431 and T-1.
    -> dict of truth x, y, var [T][2], the jump frames and the scalar parameters (m0, S0, a, c, qs)."""
    rng = np.random.default_rng(seed)
    step = rng.normal(0.0, math.sqrt(sq), (T, 2))
    frames = np.array([f % T for f in JUMP_FRAMES])
    step[frames] += rng.choice([-1.0, 1.0], (len(frames), 2)) * rng.uniform(20.0, 40.0, (len(frames), 2))
    x = np.cumsum(step, axis=0)
    var = rng.uniform(0.5, 2.0, (T, 2))
    y = x + rng.normal(size=(T, 2)) * np.sqrt(var)
    return dict(x=x, y=y, var=var, frames=frames, args=(np.zeros(2), np.full(2, 100.0), 1.0, 1.0, np.full(2, sq)))


def errors(got, ref, y, D):
    """Per chain or keypoint, the worst error over its scale: ms over the chain's max |y|, Vs over its own value,
    u = 1 / scales and change over 1.  got, ref: (ms, Vs [T][N], w [T][K], change [K])."""
    e = tref.f32_errors(got[0], got[1], ref[0], ref[1], y)
    e['u'] = np.abs(1.0 / np.asarray(got[2], np.float64) - 1.0 / ref[2]).max(axis=0)
    e['change'] = np.abs(np.asarray(got[3], np.float64) - ref[3])
    return e


def bars(r32, ref, y, D):
    """The project's float32 rule: error / scale <= max(1e-5, 4 x the transcription's own worst on the same inputs)."""
    et = errors(r32, ref, y, D)
    return {k: max(1e-5, 4.0 * float(np.max(et[k]))) for k in et}


def add_jumps(pb, jumps, seed=0):
    """A test_increments_cpu.make_session problem with true fast movements: for every (frame, keypoint) of `jumps`, all
    D coordinates of the keypoint are displaced by 20 .. 60 px from that frame onwards (through c), a keypoint's
    jumps alternating in sign so that it stays within 60 px of where it was."""
    rng = np.random.default_rng(seed)
    D = pb['D']
    y = pb['y'].astype(np.float64)
    sign = {}
    for t, k in sorted(jumps):
        sl = slice(k * D, (k + 1) * D)
        sign[k] = -sign.get(k, -1.0)
        y[t:, sl] += pb['c'][sl] * sign[k] * rng.uniform(20.0, 60.0, D)
    pb['y'] = np.ascontiguousarray(y, np.float32)
    return pb


def random_jumps(T, K, seed, rate=0.01):
    """About `rate` of the (frame >= 1, keypoint) pairs, at least one when T > 1."""
    rng = np.random.default_rng(seed)
    hit = np.argwhere(rng.random((T, K)) < rate)
    out = [(int(t), int(k)) for t, k in hit if t >= 1]
    return out or ([(T // 2 if T > 2 else 1, 0)] if T > 1 else [])
