"""Float64 NumPy references of eks_smooth_robust (TEST INFRASTRUCTURE, imported by the robust tests only): the
mean-field iteration for Student-t observation noise

    y_t | x_t, lam_t ~ N(C x_t, r_t / lam_t),   lam_t ~ Gamma(nu / 2, rate nu / 2),   r_t = clip(var_t)

around the sequential smoothers of tests/smooth_tv_ref.py at w = 1: scalar chains, general models in two independent
forms, the float32 transcription of the scalar lane arithmetic (eks_smooth_robust_lane.hpp: r * (1 / lam), the clip,
delta and the weight update with every operation in float32), and the variational bound, both in the closed form the
feature states and term by term from the joint Gaussian posterior.  A call of n_iters passes smooths n_iters times and
updates the weights n_iters - 1 times: the weights returned are the ones ms, Vs were smoothed under.  Nothing here is
compared with, or derived from, the kernels' own output."""
from __future__ import annotations

import math

import numpy as np

import innovations_ref as nref
import smooth_tv_ref as tref
from sampling_ref import VAR_CEIL, VAR_FLOOR

LAM_FLOOR = 1e-30


def _clip(v):
    return np.clip(v, VAR_FLOOR, VAR_CEIL)


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_robust(y, var, m0, S0, a, c, qs, nu, n_iters, lam0=None, history=None, snapshots=None):
    """N independent chains (y, var [T][N]).  -> ms, Vs, lam [T][N] float64 and change [N] (max |lam_new - lam_old| of
    the last update, 0 when n_iters == 1).  history: a list that receives (lam the pass smoothed under, delta it
    formed) per pass.  snapshots: a dict whose keys n <= n_iters receive what a call of n passes returns (the
    iteration is the same up to its last pass)."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, N = y.shape
    c = np.broadcast_to(np.asarray(c, np.float64), (N,))
    lam = np.ones((T, N)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    change = np.zeros(N)
    w = np.ones(T)
    for it in range(n_iters):
        ms, Vs = tref.scalar_smooth_tv(y, _clip(r / lam), m0, S0, a, c, qs, w)
        delta = ((y - c * ms) ** 2 + c * c * Vs) / r
        if history is not None:
            history.append((lam.copy(), delta))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = np.maximum((nu + 1.0) / (nu + delta), LAM_FLOOR)
        change = np.abs(new - lam).max(axis=0)
        lam = new
    return ms, Vs, lam, change


def scalar_robust_f32(y, var, m0, S0, a, c, qs, nu, n_iters, lam0=None, unit=False, snapshots=None):
    """The float32 transcription: per pass r_eff = clip(clip(var) * (1 / lam)), smooth_tv_ref.scalar_smooth_tv_f32 at
    w = 1, d = y - c m, delta = (d d + (c c) P) * (1 / r), lam = min(max(nu1 * (1 / (nu + delta)), 1e-30), (nu + 1) / nu), every operation
    in float32 with nu and nu + 1 rounded once from float64.  Same outputs, float32."""
    f = np.float32
    y = np.asarray(y, f)
    r = np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T, N = y.shape
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    nu32, nu1 = f(nu), f(nu + 1.0)
    one = f(1)
    lam = None if lam0 is None else np.asarray(lam0, f).copy()
    change = np.zeros(N, f)
    w = np.ones(T, f)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for it in range(n_iters):
            r_eff = r if lam is None else np.clip(r * (one / lam), f(VAR_FLOOR), f(VAR_CEIL))
            ms, Vs = tref.scalar_smooth_tv_f32(y, r_eff, m0, S0, a, c, qs, w, unit=unit)
            if snapshots is not None and it + 1 in snapshots:
                snapshots[it + 1] = (ms, Vs, np.ones((T, N), f) if lam is None else lam.copy(), change.copy())
            if it == n_iters - 1:
                break
            d = (y - ms) if unit else (y - c32 * ms)
            delta = (d * d + (Vs if unit else c32 * c32 * Vs)) * (one / r)
            new = np.minimum(np.maximum(nu1 * (one / (nu32 + delta)), f(LAM_FLOOR)), f((nu + 1.0) / nu)).astype(f)
            change = np.abs(new - (one if lam is None else lam)).max(axis=0).astype(f)
            lam = new
    return ms, Vs, (np.ones((T, N), f) if lam is None else lam), change


# ---- general models --------------------------------------------------------------------------------------------------
def dense_robust(y, var, m0, S0, A, C, Q, s, nu, n_iters, lam0=None, form=tref.dense_smooth_tv, history=None,
                 snapshots=None, lam_dtype=np.float64):
    """y, var [T][K][O] -> ms [T][K][D], Vs [T][K][D][D], lam [T][K][O], change [K]; delta_o from the full Vs.
    lam_dtype = numpy.float32: every new weight is rounded to float32, what the C ABI's weights plane holds (the
    general path computes in float64 but keeps its weights there)."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, K, O = y.shape
    C = np.asarray(C, np.float64)
    lam = np.ones((T, K, O)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    change = np.zeros(K)
    w = np.ones(T)
    for it in range(n_iters):
        ms, Vs = form(y, _clip(r / lam), m0, S0, A, C, Q, s, w)
        d = y - np.einsum('koi,tki->tko', C, ms)
        delta = (d * d + np.einsum('koi,tkij,koj->tko', C, Vs, C)) / r
        if history is not None:
            history.append((lam.copy(), delta))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = np.maximum(((nu + 1.0) / (nu + delta)).astype(lam_dtype), lam_dtype(LAM_FLOOR)).astype(np.float64)
        change = np.abs((new - lam).astype(lam_dtype)).reshape(T, K, -1).max(axis=(0, 2)).astype(np.float64)
        lam = new
    return ms, Vs, lam, change


# ---- the bound -------------------------------------------------------------------------------------------------------
def digamma(x):
    """psi(x) for x > 0: the recurrence up to x >= 6, then the asymptotic series (error < 1e-14)."""
    x = float(x)
    acc = 0.0
    while x < 6.0:
        acc -= 1.0 / x
        x += 1.0
    i2 = 1.0 / (x * x)
    return acc + math.log(x) - 0.5 / x - i2 * (1 / 12 - i2 * (1 / 120 - i2 * (1 / 252 - i2 * (1 / 240 - i2 / 132))))


def kl_gamma(alpha, beta, a0, b0):
    """KL(Gamma(alpha, rate beta) || Gamma(a0, rate b0)); beta may be an array."""
    return ((alpha - a0) * digamma(alpha) - math.lgamma(alpha) + math.lgamma(a0) + a0 * (np.log(beta) - math.log(b0))
            + alpha * (b0 - beta) / beta)


def elbo(loglik, delta_prev, nu):
    """The bound after the smoothing pass under lam_bar = alpha / beta_t, alpha = (nu + 1) / 2,
    beta_t = (nu + delta_prev_t) / 2: loglik is the Gaussian log-likelihood of y under r_t / lam_bar_t (per chain or
    keypoint), delta_prev the delta of the pass before with the frames on axis 0 and the chain / keypoint on axis 1."""
    alpha = 0.5 * (nu + 1.0)
    beta = 0.5 * (nu + np.asarray(delta_prev, np.float64))
    terms = 0.5 * (digamma(alpha) - math.log(alpha)) - kl_gamma(alpha, beta, 0.5 * nu, 0.5 * nu)
    return loglik + terms.reshape(terms.shape[0], terms.shape[1], -1).sum(axis=(0, 2))


def scalar_elbo_path(y, var, m0, S0, a, c, qs, nu, n_iters):
    """ELBO after passes 2 .. n_iters of scalar_robust (pass 1 has no q(lam) yet).  -> [n_iters - 1][N]."""
    hist = []
    scalar_robust(y, var, m0, S0, a, c, qs, nu, n_iters, history=hist)
    r = _clip(np.asarray(var, np.float64))
    out = []
    for i in range(1, n_iters):
        lam, _ = hist[i]
        ll = nref.scalar_innovations(y, _clip(r / lam), m0, S0, a, c, qs)[2]
        out.append(elbo(ll, hist[i - 1][1], nu))
    return np.array(out)


def joint_gaussian(y, r_eff, m0, S0, A, C, Q, s):
    """One keypoint: prior mean / covariance of the stacked states and the posterior given y under variances r_eff
    [T][O], by plain Gaussian conditioning.  -> mx, Sx, mu, Sigma."""
    y = np.asarray(y, np.float64)
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
    mxs = np.concatenate(mx)
    cov = H @ Sx @ H.T + np.diag(np.asarray(r_eff, np.float64).ravel())
    SH = Sx @ H.T
    mu = mxs + SH @ np.linalg.solve(cov, y.ravel() - H @ mxs)
    Sigma = Sx - SH @ np.linalg.solve(cov, SH.T)
    return mxs, Sx, mu, 0.5 * (Sigma + Sigma.T)


def elbo_direct(y, var, m0, S0, A, C, Q, s, nu, delta_prev):
    """One keypoint, term by term: E_q log p(y | x, lam) + E_q log p(x) + E_q log p(lam) + H[q(x)] + H[q(lam)] with
    q(lam_t,o) = Gamma(alpha, beta_t,o) from delta_prev [T][O] and q(x) the joint Gaussian posterior under
    r / lam_bar."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, O = y.shape
    D = A.shape[0]
    alpha = 0.5 * (nu + 1.0)
    beta = 0.5 * (nu + np.asarray(delta_prev, np.float64))
    lam_bar = alpha / beta
    e_ln = digamma(alpha) - np.log(beta)
    mxs, Sx, mu, Sigma = joint_gaussian(y, r / lam_bar, m0, S0, A, C, Q, s)
    H = np.kron(np.eye(T), C)
    e_sq = (y.ravel() - H @ mu) ** 2 + np.einsum('ij,jk,ik->i', H, Sigma, H)
    e_lik = np.sum(-0.5 * np.log(2 * np.pi * r.ravel()) + 0.5 * e_ln.ravel() - 0.5 * lam_bar.ravel() * e_sq / r.ravel())
    dm = mu - mxs
    e_px = -0.5 * (T * D * math.log(2 * math.pi) + np.linalg.slogdet(Sx)[1]
                   + np.trace(np.linalg.solve(Sx, Sigma + np.outer(dm, dm))))
    a0 = b0 = 0.5 * nu
    e_pl = np.sum(a0 * math.log(b0) - math.lgamma(a0) + (a0 - 1.0) * e_ln - b0 * lam_bar)
    h_x = 0.5 * (T * D * (1.0 + math.log(2 * math.pi)) + np.linalg.slogdet(Sigma)[1])
    h_l = np.sum(alpha - np.log(beta) + math.lgamma(alpha) + (1.0 - alpha) * digamma(alpha))
    return e_lik + e_px + e_pl + h_x + h_l


# ---- sessions and bars -----------------------------------------------------------------------------------------------
def outlier_session(seed, T=2000, s=2.0, frac=0.02):
    """The feature's session: a = c = 1, q = 1, random walk with process noise s, var = Gamma(2, 0.4) + 0.02,
    observation noise N(0, var), `frac` of the frames displaced by +-(20 .. 60) px.  -> dict of truth x, y, var [T][1],
    the displaced mask and the scalar parameters."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0.0, math.sqrt(s), T))
    var = rng.gamma(2.0, 0.4, T) + 0.02
    y = x + rng.normal(size=T) * np.sqrt(var)
    bad = rng.random(T) < frac
    y = y + bad * rng.choice([-1.0, 1.0], T) * rng.uniform(20.0, 60.0, T)
    return dict(x=x[:, None], y=y[:, None], var=var[:, None], bad=bad,
                args=(np.zeros(1), np.full(1, 100.0), 1.0, 1.0, np.full(1, s)))


def errors(got, ref, y):
    """Per chain, the worst error over its scale: ms over the chain's max |y|, Vs over its own value, weights and
    change over 1.  got, ref: (ms, Vs, lam, change) with [T][N] planes."""
    e = tref.f32_errors(got[0], got[1], ref[0], ref[1], y)
    e['weights'] = np.abs(np.asarray(got[2], np.float64) - ref[2]).max(axis=0)
    e['change'] = np.abs(np.asarray(got[3], np.float64) - ref[3])
    return e


def bars(r32, ref, y):
    """The project's float32 rule: error / scale <= max(1e-5, 4 x the transcription's own worst on the same inputs)."""
    et = errors(r32, ref, y)
    return {k: max(1e-5, 4.0 * float(np.max(et[k]))) for k in et}
