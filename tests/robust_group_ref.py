"""Float64 NumPy references of eks_smooth_robust_group (TEST INFRASTRUCTURE, imported by the grouped-robust tests only):
the mean-field iteration for Student-t observation noise with one Gamma factor per group of g consecutive coordinates

    y_{t,G} | x_t, lam_{t,G} ~ N(C_G x_t, diag(r_{t,o}) / lam_{t,G}),   lam_{t,G} ~ Gamma(nu / 2, rate nu / 2)

around the sequential smoothers of tests/smooth_tv_ref.py at w = 1: a scalar form, a dense form, the float32
transcription in the lanes' organisation (per-coordinate float32 delta as tests/robust_ref.py transcribes it, the group
sum and the weight in float64, the weight rounded once to float32), and the variational bound in closed form and term by
term from the joint Gaussian posterior.  A coordinate whose clipped variance sits at the ceiling is missing: it leaves its
group's factor (g_obs counts the others; g_obs = 0 keeps the prior mean 1) - so at g = 1 these references equal
tests/robust_ref.py (and the device, whose group = 1 forwards to eks_smooth_robust) only where every coordinate is
observed: there a missing coordinate's weight is (nu + 1) / nu, here 1.  Nothing here is compared with, or derived
from, the kernels' own output."""
from __future__ import annotations

import math

import numpy as np

import innovations_ref as nref
import robust_ref as rref
import smooth_tv_ref as tref
from robust_ref import LAM_FLOOR, _clip, digamma, kl_gamma
from sampling_ref import VAR_CEIL, VAR_FLOOR


def expand(lam, g):
    """[T][..., G] -> [T][..., G g]: every coordinate gets its group's weight."""
    return np.repeat(lam, g, axis=-1)


def group_weight(delta, r, nu, g, dtype=np.float64):
    """delta, r [..., O] -> lam [..., O / g] (float64 values, rounded once to dtype)."""
    seen = r < VAR_CEIL
    shp = delta.shape[:-1] + (delta.shape[-1] // g, g)
    sums = np.where(seen, delta, 0.0).reshape(shp).sum(axis=-1)
    g_obs = seen.reshape(shp).sum(axis=-1).astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        lam = np.minimum(np.maximum((nu + g_obs) / (nu + sums), LAM_FLOOR), (nu + g_obs) / nu)
    return np.where(g_obs > 0, lam, 1.0).astype(dtype).astype(np.float64)


def _change(new, old, K):
    T = new.shape[0]
    return np.abs(new - old).reshape(T, K, -1).max(axis=(0, 2))


# ---- scalar chains ---------------------------------------------------------------------------------------------------
def scalar_robust_group(y, var, m0, S0, a, c, qs, nu, g, D, n_iters, lam0=None, history=None, snapshots=None):
    """K keypoints of D chains each (y, var [T][N], N = K D, g divides D).  -> ms, Vs [T][N], lam [T][N / g] float64 and
    change [K].  history / snapshots as robust_ref.scalar_robust."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, N = y.shape
    K = N // D
    c = np.broadcast_to(np.asarray(c, np.float64), (N,))
    lam = np.ones((T, N // g)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    change = np.zeros(K)
    w = np.ones(T)
    for it in range(n_iters):
        ms, Vs = tref.scalar_smooth_tv(y, _clip(r / expand(lam, g)), m0, S0, a, c, qs, w)
        delta = ((y - c * ms) ** 2 + c * c * Vs) / r
        if history is not None:
            history.append((lam.copy(), delta))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = group_weight(delta, r, nu, g)
        change = _change(new, lam, K)
        lam = new
    return ms, Vs, lam, change


def scalar_robust_group_f32(y, var, m0, S0, a, c, qs, nu, g, D, n_iters, lam0=None, unit=False, snapshots=None):
    """The float32 transcription in the lanes' organisation: r_eff = clip(clip(var) * (1 / lam)), the float32 smoother
    at w = 1 and delta = (d d + (c c) P) * (1 / r) in float32 (robust_ref.scalar_robust_f32's arithmetic); then the
    combine: the g float32 contributions summed in float64, lam in float64, rounded once to float32; change in
    float32."""
    f = np.float32
    y = np.asarray(y, f)
    r = np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    T, N = y.shape
    K = N // D
    c32 = np.broadcast_to(np.asarray(c, np.float64), (N,)).astype(f)
    one = f(1)
    lam = None if lam0 is None else np.asarray(lam0, f).copy()
    change = np.zeros(K, f)
    w = np.ones(T, f)
    ones = np.ones((T, N // g), f)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for it in range(n_iters):
            r_eff = r if lam is None else np.clip(r * (one / expand(lam, g)), f(VAR_FLOOR), f(VAR_CEIL))
            ms, Vs = tref.scalar_smooth_tv_f32(y, r_eff, m0, S0, a, c, qs, w, unit=unit)
            if snapshots is not None and it + 1 in snapshots:
                snapshots[it + 1] = (ms, Vs, ones.copy() if lam is None else lam.copy(), change.copy())
            if it == n_iters - 1:
                break
            d = (y - ms) if unit else (y - c32 * ms)
            delta = ((d * d + (Vs if unit else c32 * c32 * Vs)) * (one / r)).astype(f)
            new = group_weight(delta.astype(np.float64), r.astype(np.float64), nu, g, dtype=f).astype(f)
            change = np.abs(new - (ones if lam is None else lam)).reshape(T, K, -1).max(axis=(0, 2)).astype(f)
            lam = new
    return ms, Vs, (ones if lam is None else lam), change


# ---- general models --------------------------------------------------------------------------------------------------
def dense_robust_group(y, var, m0, S0, A, C, Q, s, nu, g, n_iters, lam0=None, form=tref.dense_smooth_tv, history=None,
                       snapshots=None, lam_dtype=np.float64):
    """y, var [T][K][O] -> ms [T][K][D], Vs [T][K][D][D], lam [T][K][O / g], change [K]; delta_o from the full Vs.
    lam_dtype = numpy.float32: every new weight is rounded to float32, what the C ABI's plane holds."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, K, O = y.shape
    C = np.asarray(C, np.float64)
    lam = np.ones((T, K, O // g)) if lam0 is None else np.asarray(lam0, np.float64).copy()
    change = np.zeros(K)
    w = np.ones(T)
    for it in range(n_iters):
        ms, Vs = form(y, _clip(r / expand(lam, g)), m0, S0, A, C, Q, s, w)
        d = y - np.einsum('koi,tki->tko', C, ms)
        delta = (d * d + np.einsum('koi,tkij,koj->tko', C, Vs, C)) / r
        if history is not None:
            history.append((lam.copy(), delta))
        if snapshots is not None and it + 1 in snapshots:
            snapshots[it + 1] = (ms, Vs, lam.copy(), change.copy())
        if it == n_iters - 1:
            break
        new = group_weight(delta, r, nu, g, dtype=lam_dtype)
        change = np.abs((new - lam).astype(lam_dtype)).reshape(T, K, -1).max(axis=(0, 2)).astype(np.float64)
        lam = new
    return ms, Vs, lam, change


# ---- the bound -------------------------------------------------------------------------------------------------------
def group_sums(delta, g):
    return delta.reshape(delta.shape[:-1] + (delta.shape[-1] // g, g)).sum(axis=-1)


def elbo(loglik, delta_prev, nu, g):
    """The bound after the smoothing pass under lam_bar_G = alpha / beta_G, alpha = (nu + g) / 2,
    beta_G = (nu + sum_{o in G} delta_prev_o) / 2 (every coordinate observed):
        L = loglik(y under r / lam_bar) + sum_{t,G} [ (g / 2) (psi(alpha) - ln alpha) - KL(q(lam_G) || p(lam_G)) ].
    loglik per keypoint, delta_prev [T][K][O]."""
    alpha = 0.5 * (nu + g)
    beta = 0.5 * (nu + group_sums(np.asarray(delta_prev, np.float64), g))
    terms = 0.5 * g * (digamma(alpha) - math.log(alpha)) - kl_gamma(alpha, beta, 0.5 * nu, 0.5 * nu)
    return loglik + terms.sum(axis=(0, 2))


def elbo_direct(y, var, m0, S0, A, C, Q, s, nu, g, delta_prev):
    """One keypoint, term by term: E_q log p(y | x, lam) + E_q log p(x) + E_q log p(lam) + H[q(x)] + H[q(lam)] with
    q(lam_{t,G}) = Gamma(alpha, beta_{t,G}) from delta_prev [T][O] and q(x) the joint Gaussian posterior under
    r / lam_bar."""
    y = np.asarray(y, np.float64)
    r = _clip(np.asarray(var, np.float64))
    T, O = y.shape
    D = A.shape[0]
    alpha = 0.5 * (nu + g)
    beta = 0.5 * (nu + group_sums(np.asarray(delta_prev, np.float64), g))      # [T][O / g]
    lam_bar = alpha / beta
    e_ln = digamma(alpha) - np.log(beta)
    lam_o, e_ln_o = expand(lam_bar, g), expand(e_ln, g)                         # per coordinate
    mxs, Sx, mu, Sigma = rref.joint_gaussian(y, r / lam_o, m0, S0, A, C, Q, s)
    H = np.kron(np.eye(T), C)
    e_sq = (y.ravel() - H @ mu) ** 2 + np.einsum('ij,jk,ik->i', H, Sigma, H)
    e_lik = np.sum(-0.5 * np.log(2 * np.pi * r.ravel()) + 0.5 * e_ln_o.ravel() - 0.5 * lam_o.ravel() * e_sq / r.ravel())
    dm = mu - mxs
    e_px = -0.5 * (T * D * math.log(2 * math.pi) + np.linalg.slogdet(Sx)[1]
                   + np.trace(np.linalg.solve(Sx, Sigma + np.outer(dm, dm))))
    a0 = b0 = 0.5 * nu
    e_pl = np.sum(a0 * math.log(b0) - math.lgamma(a0) + (a0 - 1.0) * e_ln - b0 * lam_bar)
    h_x = 0.5 * (T * D * (1.0 + math.log(2 * math.pi)) + np.linalg.slogdet(Sigma)[1])
    h_l = np.sum(alpha - np.log(beta) + math.lgamma(alpha) + (1.0 - alpha) * digamma(alpha))
    return e_lik + e_px + e_pl + h_x + h_l


def scalar_elbo_path(y, var, m0, S0, a, c, qs, nu, g, D, n_iters):
    """ELBO per keypoint after passes 2 .. n_iters of scalar_robust_group.  -> [n_iters - 1][K]."""
    hist = []
    scalar_robust_group(y, var, m0, S0, a, c, qs, nu, g, D, n_iters, history=hist)
    r = _clip(np.asarray(var, np.float64))
    T, N = r.shape
    K = N // D
    out = []
    for i in range(1, n_iters):
        lam, _ = hist[i]
        ll = nref.scalar_innovations(y, _clip(r / expand(lam, g)), m0, S0, a, c, qs)[2]
        out.append(elbo(ll.reshape(K, D).sum(axis=1), hist[i - 1][1].reshape(T, K, D), nu, g))
    return np.array(out)


# ---- the demonstration session -------------------------------------------------------------------------------------------
def joint_session(seed, T=600, sq=0.05, n_bad=20, lo=2.5, hi=4.0):
    """One keypoint with two unit chains (a = c = 1, q = 1, s = sq), var ~ U(0.5, 2), observation noise N(0, var);
    n_bad isolated frames displaced in BOTH coordinates at once, each by lo .. hi standard deviations of the frame's own
    sqrt(var), with independent signs.  -> dict(x, y, var [T][2], bad [T], args)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0.0, math.sqrt(sq), (T, 2)), axis=0)
    var = rng.uniform(0.5, 2.0, (T, 2))
    y = x + rng.normal(size=(T, 2)) * np.sqrt(var)
    frames = 5 + 2 * rng.choice((T - 10) // 2, n_bad, replace=False)            # never adjacent
    bad = np.zeros(T, bool)
    bad[frames] = True
    y[frames] += rng.choice([-1.0, 1.0], (n_bad, 2)) * rng.uniform(lo, hi, (n_bad, 2)) * np.sqrt(var[frames])
    return dict(x=x, y=y, var=var, bad=bad, args=(np.zeros(2), np.full(2, 100.0), 1.0, 1.0, np.full(2, sq)))


# ---- bars --------------------------------------------------------------------------------------------------------------
def errors(got, ref, y):
    """Per chain / column, the worst error over its scale (robust_ref.errors; the weight plane has its own width)."""
    e = tref.f32_errors(got[0], got[1], ref[0], ref[1], y)
    e['weights'] = np.abs(np.asarray(got[2], np.float64) - ref[2]).max(axis=0)
    e['change'] = np.abs(np.asarray(got[3], np.float64) - ref[3])
    return e


def bars(r32, ref, y):
    """ms, Vs and weights: robust_ref.bars' rule on this run, error / scale <= max(1e-5, 4 x the float32 transcription's
    own worst on the same inputs).  change is max_t |lam_new - lam_old| over two weight planes of the iteration, so
    | change_got - change_ref | <= max |err(lam_new)| + max |err(lam_old)|: its bar is twice the weights' bar, derived
    from theirs and not from the transcription's error on change itself - a maximum attained at one frame, on which one
    run of the transcription is a single draw (4.8e-6 after 8 passes and 2.4e-5 after 2 on one T = 1000 session whose
    weights are off by 6.8e-5 and 4.3e-5)."""
    et = errors(r32, ref, y)
    out = {k: max(1e-5, 4.0 * float(np.max(et[k]))) for k in ('ms', 'Vs', 'weights')}
    out['change'] = 2.0 * out['weights']
    return out
