"""Float64 NumPy references of eks_smooth_heavy_fit (TEST INFRASTRUCTURE, imported by the heavy-fit tests only):
eks_smooth_heavy's mean-field iteration (tests/heavy_ref.py, around tests/jumps_ref.py's Gaussian passes) with the
M-step for the smoothing parameter behind every middle pass' updates of the planes,

    S_k = sum_{t=1}^{T-1} u_new[t,k] delta[t,k],   log s_new = clip(log s + log(S_k / n), lo, hi),   n = D (T - 1),

delta[t,k] = E[eps_t' (s Q)^-1 eps_t | y] being what the pass formed for the update of u.  A nu of math.inf makes that
side Gaussian: its plane stays at ones and its update is skipped.  A keypoint whose S_k is not finite and >= 0 keeps
its s.  Scalar chains and general models in float64, the float32 transcription of the scalar path (heavy_ref's and
jumps_ref's float32 lanes - jumps_ref._pass_f32, the weight update as heavy_ref.scalar_heavy_f32 states it,
jumps_ref.combine_f32 - and the step in float64 on the float32 planes, as the kernels hold them), and the bound with a
Gaussian side's terms dropped.  Nothing here is compared with, or derived from, the kernels' own output."""
from __future__ import annotations

import math

import numpy as np

import heavy_ref as href
import jumps_ref as jref
import robust_ref as rref
import smooth_tv_ref as tref
from sampling_ref import VAR_CEIL, VAR_FLOOR

R = 1024                     # kFitSlab: rows of a slab of the device's sum (tests place T around it)
BOUNDS = (-8.0, 8.0)         # refine_smooth_param_em's default


def step(s, S, n, bounds):
    """The M-step on s [K] from S [K].  -> (s_new, |delta log s|); a keypoint whose S is not finite and >= 0, or
    whose s is not finite and > 0, keeps its s with 0 change; S = 0 is log s = -inf, clipped to lo."""
    s = np.asarray(s, np.float64)
    S = np.asarray(S, np.float64)
    ok = np.isfinite(S) & (S >= 0) & np.isfinite(s) & (s > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        l_old = np.log(s)
        l_new = l_old + np.log(S / n)
        l_set = np.clip(l_new, bounds[0], bounds[1])
        inside = (l_new >= bounds[0]) & (l_new <= bounds[1])
        s_new = np.where(inside, s * (S / n), np.exp(l_set))
        dl = np.abs(l_set - l_old)
    return np.where(ok, s_new, s), np.where(ok, dl, 0.0)


def statistic(w, delta):
    """S [K] = sum over rows 1 .. T-1 of delta / w."""
    return (np.asarray(delta, np.float64)[1:] / np.asarray(w, np.float64)[1:]).sum(axis=0)


def _finite(nu):
    return math.isfinite(nu)


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_fit(y, var, m0, S0, a, c, q, s0, nu_obs, nu_proc, n_iters, D=1, bounds=BOUNDS, lam0=None, w0=None,
               history=None, snapshots=None, fit=True):
    """y, var [T][N], N = K D chains; q [N] the chains' process noise at s = 1, s0 [K] the start.  -> ms, Vs [T][N],
    lam [T][N], w [T][K], s [K], change [3][K] float64 (rows 0, 1 as heavy_ref.scalar_heavy's - 0 for a Gaussian side
    - row 2 |delta log s| of the last update).  history receives (lam, w, delta_obs, delta_proc, loglik, s) per pass
    - s the one the pass smoothed under; snapshots as heavy_ref.scalar_heavy's.  fit = False: s stays (heavy_ref's
    iteration with the Gaussian sides)."""
    y = np.asarray(y, np.float64)
    r = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, N = y.shape
    K = N // D
    q = np.broadcast_to(np.asarray(q, np.float64), (N,))
    cc = np.broadcast_to(np.asarray(c, np.float64), (N,))
    s = np.broadcast_to(np.asarray(s0, np.float64), (K,)).copy()
    lam, w = href._planes(T, N, K, lam0, w0)
    change = np.zeros((3, K))
    n = D * (T - 1)
    for it in range(n_iters):
        ms, Vs, dproc, ll = jref.scalar_pass(y, np.clip(r / lam, VAR_FLOOR, VAR_CEIL), m0, S0, a, c, q * np.repeat(s, D),
                                             w, D)
        dobs = ((y - cc * ms) ** 2 + cc * cc * Vs) / r
        if history is not None:
            history.append((lam.copy(), w.copy(), dobs, dproc, ll, s.copy()))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), w.copy(), s.copy(), change.copy())
        if it == n_iters - 1:
            break
        change = np.zeros((3, K))
        if _finite(nu_obs):
            new = np.maximum((nu_obs + 1.0) / (nu_obs + dobs), href.LAM_FLOOR)
            change[0] = np.abs(new - lam).reshape(T, K, D).max(axis=(0, 2))
            lam = new
        if _finite(nu_proc):
            new = jref.new_scales(dproc, nu_proc, D)
            change[1] = jref._change(new, w)
            w = new
        if fit:
            s, change[2] = step(s, statistic(w, dproc), n, bounds)
    return ms, Vs, lam, w, s, change


def scalar_fit_f32(y, var, m0, S0, a, c, q, s0, nu_obs, nu_proc, n_iters, D=1, bounds=BOUNDS, lam0=None, w0=None,
                   unit=False, B=32, snapshots=None):
    """The float32 transcription of a call: heavy_ref.scalar_heavy_f32's pass and updates (a Gaussian side skipped),
    then the step in float64 on the float32 contributions and the float32 scales, s q rounded to float32 once per
    pass as the lanes load it.  Same outputs as scalar_fit; the planes, ms, Vs and rows 0, 1 of change float32."""
    f = np.float32
    y32 = np.asarray(y, f)
    r = np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T, N = y32.shape
    K = N // D
    q = np.broadcast_to(np.asarray(q, np.float64), (N,))
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    s = np.broadcast_to(np.asarray(s0, np.float64), (K,)).copy()
    one = f(1)
    lam = None if lam0 is None else np.asarray(lam0, f).copy()
    w = np.ones((T, K), f) if w0 is None else np.asarray(w0, f).copy()
    w[0] = 1.0
    change = np.zeros((3, K))
    ones = lambda: np.ones((T, N), f)  # noqa: E731
    n = D * (T - 1)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for it in range(n_iters):
            r_eff = r if lam is None else np.clip(r * (one / lam), f(VAR_FLOOR), f(VAR_CEIL))
            ms, Vs, contrib = jref._pass_f32(y32, r_eff, m0, S0, a, c, q * np.repeat(s, D), w, D, unit, B)
            if snapshots is not None and it + 1 in snapshots:
                snapshots[it + 1] = (ms, Vs, ones() if lam is None else lam.copy(), w.copy(), s.copy(), change.copy())
            if it == n_iters - 1:
                break
            change = np.zeros((3, K))
            if _finite(nu_obs):
                nu32, nu1 = f(nu_obs), f(nu_obs + 1.0)
                d = (y32 - ms) if unit else (y32 - c32 * ms)
                delta = (d * d + (Vs if unit else c32 * c32 * Vs)) * (one / r)
                new = np.minimum(np.maximum(nu1 * (one / (nu32 + delta)), f(href.LAM_FLOOR)),
                                 f((nu_obs + 1.0) / nu_obs)).astype(f)
                change[0] = np.abs(new - (one if lam is None else lam)).reshape(T, K, D).max(axis=(0, 2))
                lam = new
            if _finite(nu_proc):
                w, ch1 = jref.combine_f32(contrib, w, nu_proc, D, D)
                change[1] = ch1
            delta64 = np.asarray(contrib, np.float64).reshape(T, K, D).sum(axis=2)
            s, change[2] = step(s, statistic(w, delta64), n, bounds)
    return ms, Vs, (ones() if lam is None else lam), w, s, change


# ---- general models --------------------------------------------------------------------------------------------------
def dense_fit(y, var, m0, S0, A, C, Q, s0, nu_obs, nu_proc, n_iters, bounds=BOUNDS, lam0=None, w0=None,
              form=tref.dense_smooth_tv, history=None, snapshots=None, plane_dtype=np.float64):
    """heavy_ref.dense_heavy with the step.  y, var [T][K][O] -> ms, Vs, lam [T][K][O], w [T][K], s [K],
    change [3][K].  plane_dtype = numpy.float32: every new weight and scale is rounded to float32, what the C ABI's
    planes hold; the step then reads the rounded scales, as the kernels do."""
    y = np.asarray(y, np.float64)
    r = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, K, O = y.shape
    C = np.asarray(C, np.float64)
    D = np.shape(A)[-1]
    s = np.broadcast_to(np.asarray(s0, np.float64), (K,)).copy()
    lam = np.ones((T, K, O)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    w = np.ones((T, K)) if w0 is None else np.asarray(w0, np.float64).copy()
    w[0] = 1.0
    change = np.zeros((3, K))
    n = D * (T - 1)
    for it in range(n_iters):
        ms, Vs, dproc, ll = jref.dense_pass(y, np.clip(r / lam, VAR_FLOOR, VAR_CEIL), m0, S0, A, C, Q, s, w, form)
        d = y - np.einsum('koi,tki->tko', C, ms)
        dobs = (d * d + np.einsum('koi,tkij,koj->tko', C, Vs, C)) / r
        if history is not None:
            history.append((lam.copy(), w.copy(), dobs, dproc, ll, s.copy()))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), w.copy(), s.copy(), change.copy())
        if it == n_iters - 1:
            break
        change = np.zeros((3, K))
        if _finite(nu_obs):
            new = np.maximum(((nu_obs + 1.0) / (nu_obs + dobs)).astype(plane_dtype),
                             plane_dtype(href.LAM_FLOOR)).astype(np.float64)
            change[0] = np.abs((new - lam).astype(plane_dtype)).max(axis=(0, 2)).astype(np.float64)
            lam = new
        if _finite(nu_proc):
            u = np.clip((nu_proc + D) / (nu_proc + dproc[1:]), jref.U_FLOOR, (nu_proc + D) / nu_proc)
            change[1] = np.abs(u - 1.0 / w[1:]).max(axis=0)
            w = jref.new_scales(dproc, nu_proc, D).astype(plane_dtype).astype(np.float64)
        s, change[2] = step(s, statistic(w, dproc), n, bounds)
    return ms, Vs, lam, w, s, change


# ---- the bound -------------------------------------------------------------------------------------------------------
def elbo(loglik, dobs_prev, dproc_prev, nu_obs, nu_proc, D):
    """heavy_ref.elbo with a Gaussian side's terms dropped (nu = inf: q is a point mass at 1 and its terms vanish).
    loglik is the Gaussian log-likelihood under the s the pass smoothed under: with q(lam), q(u) held the expression
    is the bound at any s."""
    K = np.shape(dproc_prev)[1]
    out = np.asarray(loglik, np.float64)
    if _finite(nu_obs):
        dobs = np.asarray(dobs_prev, np.float64)
        out = rref.elbo(out, dobs.reshape(dobs.shape[0], K, -1), nu_obs)
    if _finite(nu_proc):
        out = jref.elbo(out, dproc_prev, nu_proc, D)
    return out


def elbo_path(history, nu_obs, nu_proc, D):
    """The bound after passes 2 .. n of a history.  -> [n - 1][K]."""
    return np.array([elbo(history[i][4], history[i - 1][2], history[i - 1][3], nu_obs, nu_proc, D)
                     for i in range(1, len(history))])


# ---- the feature's session -------------------------------------------------------------------------------------------
def outlier_session(seed, T=600, sq=0.05, n_bad=14):
    """One keypoint, two unit chains, a random walk with true s q = sq, variances U(0.5, 2), m0 = 0, S0 = 100; n_bad
    frames, at least six apart and six from either end, displaced by +-20 .. 60 px in both coordinates (observations
    only).  -> dict of truth x, y, var [T][2], bad, and the scalar parameters (m0, S0, a, c, q) with q = 1 per chain
    (so s IS s q)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0.0, math.sqrt(sq), (T, 2)), axis=0)
    var = rng.uniform(0.5, 2.0, (T, 2))
    y = x + rng.normal(size=(T, 2)) * np.sqrt(var)
    bad = []
    while len(bad) < n_bad:
        t = int(rng.integers(6, T - 6))
        if all(abs(t - u) >= 6 for u in bad):
            bad.append(t)
    bad = np.array(sorted(bad))
    y[bad] += rng.choice([-1.0, 1.0], (n_bad, 2)) * rng.uniform(20.0, 60.0, (n_bad, 2))
    return dict(x=x, y=y, var=var, bad=bad, args=(np.zeros(2), np.full(2, 100.0), 1.0, 1.0, np.ones(2)))


def rmse(ms, x):
    return float(np.sqrt(np.mean((np.asarray(ms, np.float64) - x) ** 2)))


# ---- errors and bars -------------------------------------------------------------------------------------------------
def errors(got, ref, y, D):
    """heavy_ref.errors on (ms, Vs, lam, w, change rows 0, 1) plus log s and row 2 of change over 1.
    got, ref: (ms, Vs, lam [T][N], w [T][K], s [K], change [3][K])."""
    g5 = (got[0], got[1], got[2], got[3], np.asarray(got[5], np.float64)[:2])
    r5 = (ref[0], ref[1], ref[2], ref[3], np.asarray(ref[5], np.float64)[:2])
    e = href.errors(g5, r5, y, D)
    e['log_s'] = np.abs(np.log(np.asarray(got[4], np.float64)) - np.log(ref[4]))
    e['dlog_s'] = np.abs(np.asarray(got[5], np.float64)[2] - np.asarray(ref[5], np.float64)[2])
    return e


def bars(r32, ref, y, D):
    """The project's float32 rule: error / scale <= max(1e-5, 4 x the transcription's own worst on the same inputs)."""
    et = errors(r32, ref, y, D)
    return {k: max(1e-5, 4.0 * float(np.max(et[k]))) for k in et}
