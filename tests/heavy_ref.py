"""Float64 NumPy references of eks_smooth_heavy (TEST INFRASTRUCTURE, imported by the heavy tests only): the
mean-field iteration for Student-t noise on both sides,

    y_t | x_t, lam_t ~ N(C x_t, r_t / lam_t),   lam_t ~ Gamma(nu_obs / 2, rate nu_obs / 2),   r_t = clip(var_t),
    eps_t | u_t ~ N(0, s Q / u_t),              u_t ~ Gamma(nu_proc / 2, rate nu_proc / 2),   t = 1 .. T-1,

around tests/jumps_ref.py's Gaussian passes (scalar_pass, dense_pass in both forms of smooth_tv_ref) run on
clip(r / lam) under the scales w = 1 / u: both updates come from one smoothed posterior.  Also the float32
transcription of the scalar lanes' organisation (jumps_ref._pass_f32 under the reweighted variances, the weight update
as robust_ref.scalar_robust_f32 states it, the combine in float64 rounded once) and the variational bound in its
compact and its term-by-term form.  A call of n_iters passes smooths n_iters times and updates n_iters - 1 times: the
planes returned are the ones ms, Vs were smoothed under.  Nothing here is compared with, or derived from, the kernels'
own output."""
from __future__ import annotations

import math

import numpy as np

import jumps_ref as jref
import robust_ref as rref
import smooth_tv_ref as tref
from robust_ref import digamma, kl_gamma
from sampling_ref import VAR_CEIL, VAR_FLOOR

LAM_FLOOR = 1e-30


def _clip(v):
    return np.clip(v, VAR_FLOOR, VAR_CEIL)


def _planes(T, N, K, lam0, w0):
    lam = np.ones((T, N)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    w = np.ones((T, K)) if w0 is None else np.asarray(w0, np.float64).copy()
    w[0] = 1.0
    return lam, w


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_heavy(y, var, m0, S0, a, c, qs, nu_obs, nu_proc, n_iters, D=1, lam0=None, w0=None, history=None,
                 snapshots=None, update=(True, True)):
    """y, var [T][N], N = K D chains.  -> ms, Vs [T][N], lam [T][N], w [T][K] float64 and change [2][K] (row 0 max
    |lam_new - lam_old|, row 1 max |u_new - u_old| of the last update; 0 when n_iters == 1).  history: a list that
    receives (lam, w the pass smoothed under, delta_obs, delta_proc, loglik) per pass.  snapshots: a dict whose keys
    n <= n_iters receive what a call of n passes returns.  update: (weights, scales) - False switches that side's
    update off (the prototype's single-sided models)."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, N = y.shape
    K = N // D
    cc = np.broadcast_to(np.asarray(c, np.float64), (N,))
    lam, w = _planes(T, N, K, lam0, w0)
    change = np.zeros((2, K))
    for it in range(n_iters):
        ms, Vs, dproc, ll = jref.scalar_pass(y, _clip(r / lam), m0, S0, a, c, qs, w, D)
        dobs = ((y - cc * ms) ** 2 + cc * cc * Vs) / r
        if history is not None:
            history.append((lam.copy(), w.copy(), dobs, dproc, ll))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), w.copy(), change.copy())
        if it == n_iters - 1:
            break
        change = np.zeros((2, K))
        if update[0]:
            new = np.maximum((nu_obs + 1.0) / (nu_obs + dobs), LAM_FLOOR)
            change[0] = np.abs(new - lam).reshape(T, K, D).max(axis=(0, 2))
            lam = new
        if update[1]:
            new = jref.new_scales(dproc, nu_proc, D)
            change[1] = jref._change(new, w)
            w = new
    return ms, Vs, lam, w, change


def scalar_heavy_f32(y, var, m0, S0, a, c, qs, nu_obs, nu_proc, n_iters, D=1, lam0=None, w0=None, unit=False, B=32,
                     snapshots=None):
    """The float32 transcription of a call in chunks of B frames (the kernels': 32): r_eff = clip(clip(var) * (1 / lam)),
    jumps_ref._pass_f32 under it and the scales, then d = y - c m, delta = (d d + (c c) P) * (1 / r),
    lam = min(max(nu1 * (1 / (nu + delta)), 1e-30), (nu + 1) / nu) in float32 and jumps_ref.combine_f32.  Same
    outputs as scalar_heavy, float32."""
    f = np.float32
    y32 = np.asarray(y, f)
    r = np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T, N = y32.shape
    K = N // D
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    nu32, nu1, one = f(nu_obs), f(nu_obs + 1.0), f(1)
    lam = None if lam0 is None else np.asarray(lam0, f).copy()
    w = np.ones((T, K), f) if w0 is None else np.asarray(w0, f).copy()
    w[0] = 1.0
    change = np.zeros((2, K), f)
    ones = lambda: np.ones((T, N), f)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for it in range(n_iters):
            r_eff = r if lam is None else np.clip(r * (one / lam), f(VAR_FLOOR), f(VAR_CEIL))
            ms, Vs, contrib = jref._pass_f32(y32, r_eff, m0, S0, a, c, qs, w, D, unit, B)
            if snapshots is not None and it + 1 in snapshots:
                snapshots[it + 1] = (ms, Vs, ones() if lam is None else lam.copy(), w.copy(), change.copy())
            if it == n_iters - 1:
                break
            d = (y32 - ms) if unit else (y32 - c32 * ms)
            delta = (d * d + (Vs if unit else c32 * c32 * Vs)) * (one / r)
            new = np.minimum(np.maximum(nu1 * (one / (nu32 + delta)), f(LAM_FLOOR)), f((nu_obs + 1.0) / nu_obs)).astype(f)
            ch0 = np.abs(new - (one if lam is None else lam)).reshape(T, K, D).max(axis=(0, 2)).astype(f)
            lam = new
            w, ch1 = jref.combine_f32(contrib, w, nu_proc, D, D)
            change = np.stack([ch0, ch1]).astype(f)
    return ms, Vs, (ones() if lam is None else lam), w, change


# ---- general models --------------------------------------------------------------------------------------------------
def dense_heavy(y, var, m0, S0, A, C, Q, s, nu_obs, nu_proc, n_iters, lam0=None, w0=None, form=tref.dense_smooth_tv,
                history=None, snapshots=None, plane_dtype=np.float64):
    """y, var [T][K][O] -> ms [T][K][D], Vs [T][K][D][D], lam [T][K][O], w [T][K], change [2][K].  plane_dtype =
    numpy.float32: every new weight and scale is rounded to float32, what the C ABI's planes hold (the general path
    computes in float64 but keeps its planes there)."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, K, O = y.shape
    C = np.asarray(C, np.float64)
    D = np.shape(A)[-1]
    lam = np.ones((T, K, O)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    w = np.ones((T, K)) if w0 is None else np.asarray(w0, np.float64).copy()
    w[0] = 1.0
    change = np.zeros((2, K))
    for it in range(n_iters):
        ms, Vs, dproc, ll = jref.dense_pass(y, _clip(r / lam), m0, S0, A, C, Q, s, w, form)
        d = y - np.einsum('koi,tki->tko', C, ms)
        dobs = (d * d + np.einsum('koi,tkij,koj->tko', C, Vs, C)) / r
        if history is not None:
            history.append((lam.copy(), w.copy(), dobs, dproc, ll))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), w.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = np.maximum(((nu_obs + 1.0) / (nu_obs + dobs)).astype(plane_dtype), plane_dtype(LAM_FLOOR)).astype(np.float64)
        ch0 = np.abs((new - lam).astype(plane_dtype)).max(axis=(0, 2)).astype(np.float64)
        lam = new
        u = np.clip((nu_proc + D) / (nu_proc + dproc[1:]), jref.U_FLOOR, (nu_proc + D) / nu_proc)
        ch1 = np.abs(u - 1.0 / w[1:]).max(axis=0) if T > 1 else np.zeros(K)
        w = jref.new_scales(dproc, nu_proc, D).astype(plane_dtype).astype(np.float64)
        change = np.stack([ch0, ch1])
    return ms, Vs, lam, w, change


# ---- the bound -------------------------------------------------------------------------------------------------------
def elbo(loglik, dobs_prev, dproc_prev, nu_obs, nu_proc, D):
    """The bound after the smoothing pass under lam_bar = alpha / beta (alpha = (nu_obs + 1) / 2, beta =
    (nu_obs + dobs_prev) / 2) and u_bar likewise from dproc_prev with alpha = (nu_proc + D) / 2 (nonsingular Q):
    loglik [K] is the Gaussian log-likelihood of y under r / lam_bar and the scales 1 / u_bar; to it robust_ref.elbo
    adds the per-observation terms and jumps_ref.elbo the per-frame ones.  dobs_prev: frames on axis 0, the keypoint on
    axis 1 (its observations behind it); dproc_prev [T][K]."""
    K = np.shape(dproc_prev)[1]
    dobs = np.asarray(dobs_prev, np.float64)
    dobs = dobs.reshape(dobs.shape[0], K, -1)
    return jref.elbo(rref.elbo(loglik, dobs, nu_obs), dproc_prev, nu_proc, D)


def elbo_path(history, nu_obs, nu_proc, D):
    """The bound after passes 2 .. n of a history (pass 1 has no q(lam), q(u) yet).  -> [n - 1][K]."""
    return np.array([elbo(history[i][4], history[i - 1][2], history[i - 1][3], nu_obs, nu_proc, D)
                     for i in range(1, len(history))])


def elbo_direct(y, var, m0, S0, A, C, Q, s, nu_obs, nu_proc, dobs_prev, dproc_prev):
    """One keypoint, term by term from the joint posterior: E log p(y | x, lam) + E log p(x | u) + E log p(lam) +
    E log p(u) + H[q(x)] + H[q(lam)] + H[q(u)], q(lam_t,o) = Gamma(alpha_l, beta_t,o) from dobs_prev [T][O],
    q(u_t) = Gamma(alpha_u, beta_t) from dproc_prev (T,) (entry 0 unused) and q(x) the joint Gaussian posterior under
    r / lam_bar and s Q / u_bar.  Q nonsingular."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    m0, S0, A, C, Q = (np.asarray(x, np.float64) for x in (m0, S0, A, C, Q))
    T, O = y.shape
    D = A.shape[0]
    al = 0.5 * (nu_obs + 1.0)
    bl = 0.5 * (nu_obs + np.asarray(dobs_prev, np.float64))
    lam_bar, e_ln_l = al / bl, digamma(al) - np.log(bl)
    au = 0.5 * (nu_proc + D)
    bu = 0.5 * (nu_proc + np.asarray(dproc_prev, np.float64)[1:])
    u_bar, e_ln_u = au / bu, digamma(au) - np.log(bu)
    w = np.concatenate([[1.0], 1.0 / u_bar])
    # the joint Gaussian posterior under r / lam_bar and w
    Pt, mx = [S0], [m0]
    for t in range(1, T):
        Pt.append(A @ Pt[-1] @ A.T + s * w[t] * Q)
        mx.append(A @ mx[-1])
    Sx = np.zeros((T * D, T * D))
    for t in range(T):
        blk = Pt[t]
        for v in range(t, T):
            Sx[v * D:(v + 1) * D, t * D:(t + 1) * D] = blk
            Sx[t * D:(t + 1) * D, v * D:(v + 1) * D] = blk.T
            blk = A @ blk
    H = np.kron(np.eye(T), C)
    mxs = np.concatenate(mx)
    cov = H @ Sx @ H.T + np.diag((r / lam_bar).ravel())
    SH = Sx @ H.T
    mu = mxs + SH @ np.linalg.solve(cov, y.ravel() - H @ mxs)
    Sig = Sx - SH @ np.linalg.solve(cov, SH.T)
    Sig = 0.5 * (Sig + Sig.T)
    e_sq = (y.ravel() - H @ mu) ** 2 + np.einsum('ij,jk,ik->i', H, Sig, H)
    e_lik = np.sum(-0.5 * np.log(2 * np.pi * r.ravel()) + 0.5 * e_ln_l.ravel() - 0.5 * lam_bar.ravel() * e_sq / r.ravel())
    # E log p(x | u): the prior on x_0 and T - 1 transitions with precision u_t (s Q)^-1
    d0 = mu[:D] - m0
    e_px = -0.5 * (D * math.log(2 * math.pi) + np.linalg.slogdet(S0)[1]
                   + np.trace(np.linalg.solve(S0, Sig[:D, :D] + np.outer(d0, d0))))
    sQi = np.linalg.inv(s * Q)
    M = np.hstack([-A, np.eye(D)])
    for t in range(1, T):
        sl = slice((t - 1) * D, (t + 1) * D)
        e = M @ mu[sl]
        Eee = M @ Sig[sl, sl] @ M.T + np.outer(e, e)
        e_px += -0.5 * (D * math.log(2 * math.pi) + np.linalg.slogdet(s * Q)[1]) + 0.5 * D * e_ln_u[t - 1] \
            - 0.5 * u_bar[t - 1] * np.trace(sQi @ Eee)
    a0 = 0.5 * nu_obs
    e_pl = np.sum(a0 * math.log(a0) - math.lgamma(a0) + (a0 - 1.0) * e_ln_l - a0 * lam_bar)
    a1 = 0.5 * nu_proc
    e_pu = np.sum(a1 * math.log(a1) - math.lgamma(a1) + (a1 - 1.0) * e_ln_u - a1 * u_bar)
    h_x = 0.5 * (T * D * (1.0 + math.log(2 * math.pi)) + np.linalg.slogdet(Sig)[1])
    h_l = np.sum(al - np.log(bl) + math.lgamma(al) + (1.0 - al) * digamma(al))
    h_u = np.sum(au - np.log(bu) + math.lgamma(au) + (1.0 - au) * digamma(au))
    return e_lik + e_px + e_pl + e_pu + h_x + h_l + h_u


# ---- sessions and bars -----------------------------------------------------------------------------------------------
JUMP_FRAMES = (60, 100, 160, 250, 431, 520)


def heavy_session(seed, T=600, sq=0.05):
    """The feature's session: one keypoint, two unit chains sharing one scale, a random walk with s q = sq, variances
    U(0.5, 2), m0 = 0, S0 = 100; jumps of +-20..40 px in both coordinates entering JUMP_FRAMES; twelve displaced
    frames (+-20..60 px in both coordinates, observations only) at least six frames from each other and from every
    jump, none in the first three or last six frames, the first held for three consecutive frames.
    -> dict of truth x, y, var [T][2], jumps, the displaced frames `bad` (14: the held one counts three), and the scalar
    parameters (m0, S0, a, c, qs)."""
    rng = np.random.default_rng(seed)
    step = rng.normal(0.0, math.sqrt(sq), (T, 2))
    jumps = np.array(JUMP_FRAMES)
    step[jumps] += rng.choice([-1.0, 1.0], (len(jumps), 2)) * rng.uniform(20.0, 40.0, (len(jumps), 2))
    x = np.cumsum(step, axis=0)
    var = rng.uniform(0.5, 2.0, (T, 2))
    y = x + rng.normal(size=(T, 2)) * np.sqrt(var)
    starts, taken = [], list(jumps)
    while len(starts) < 12:
        hold = 3 if not starts else 1
        t = int(rng.integers(3, T - 6 - hold + 1))
        span = range(t, t + hold)
        if all(abs(u - v) >= 6 for u in span for v in taken):
            starts.append((t, hold))
            taken.extend(span)
    bad = []
    for t, hold in starts:
        off = rng.choice([-1.0, 1.0], 2) * rng.uniform(20.0, 60.0, 2)
        y[t:t + hold] += off
        bad.extend(range(t, t + hold))
    return dict(x=x, y=y, var=var, jumps=jumps, bad=np.array(sorted(bad)),
                args=(np.zeros(2), np.full(2, 100.0), 1.0, 1.0, np.full(2, sq)))


def errors(got, ref, y, D):
    """Per chain or keypoint, the worst error over its scale: ms over the chain's max |y|, Vs over its own value,
    weights, u = 1 / scales and change over 1.  got, ref: (ms, Vs, lam [T][N], w [T][K], change [2][K])."""
    e = tref.f32_errors(got[0], got[1], ref[0], ref[1], y)
    e['weights'] = np.abs(np.asarray(got[2], np.float64) - ref[2]).max(axis=0)
    e['u'] = np.abs(1.0 / np.asarray(got[3], np.float64) - 1.0 / ref[3]).max(axis=0)
    e['change'] = np.abs(np.asarray(got[4], np.float64) - ref[4]).max(axis=0)
    return e


def bars(r32, ref, y, D):
    """The project's float32 rule: error / scale <= max(1e-5, 4 x the transcription's own worst on the same inputs)."""
    et = errors(r32, ref, y, D)
    return {k: max(1e-5, 4.0 * float(np.max(et[k]))) for k in et}
