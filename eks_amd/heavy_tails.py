"""The smoother under heavy-tailed (Student-t) noise on both sides: observations and process.

eks_amd.robust discounts frames where the whole ensemble agrees on a wrong place; eks_amd.jumps lets a true fast
movement through.  A real session has both: a paw that is swapped with the other paw for a few frames also makes a
reach.  Run alone, each model breaks on the other's events - under the robust model a reach is a long run of
"outliers" whose weights go to zero while the smoother stays behind; under the jumps model a one-frame swap is two
jumps, there and back, and the smoother follows it.  The model here holds both at once:

    y_t | x_t, lam_t ~ N(C x_t, r_t / lam_t),    lam_t ~ Gamma(nu_obs / 2, rate nu_obs / 2)      every scalar observation
    eps_t | u_t      ~ N(0, s Q / u_t),          u_t   ~ Gamma(nu_proc / 2, rate nu_proc / 2)    every keypoint, t >= 1

with the Gaussian smoother's prior.  Mean field over q(x) q(lam) q(u): a Gaussian smoothing pass under r / lam and the
scales w = 1 / u, then both closed-form updates from that one smoothed posterior (given q(x) they are independent, so
the variational bound cannot drop).  The passes run on the device without a host round trip.  The reference has no
counterpart.

    smooth_heavy_tailed(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, nu_obs=4.0, nu_proc=4.0, n_iters=12, ...)
        -> ms, Vs, weights, scales, change
    smooth_singlecam_heavy_tailed(marker_array, keypoint_names, s_finals, ...) -> dict(ms, Vs, weights, scales)
    fit_heavy_tailed(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_init, nu_obs=4.0, nu_proc=4.0, n_iters=40, ...)
        -> ms, Vs, weights, scales, s_fit, change
    fit_singlecam_heavy_tailed(marker_array, keypoint_names, s_init, ...) -> dict(ms, Vs, weights, scales, s_fit)

A weight near 1 says the observation agrees with the trajectory, a weight near 0 that it was discounted; a scale near 1
says the frame moved like the rest of the session, a scale of hundreds or thousands marks a jump INTO that frame.

What the model cannot tell apart: a jump into frame 1 under a wide prior, a jump into the last frame, and two opposite
jumps in consecutive frames each have an outlier explanation that costs less, and are treated as outliers.

The smoothing parameter.  The drivers' search fits s to the Gaussian model, which explains displaced observations as
process noise: on a session with outliers that s is far too large (over a thousand times on
tests/heavy_fit_ref.py's outlier_session), and the smooth_* functions here take it as given.  The fit_* functions fit s inside the iteration: after every middle
pass' updates of the planes, s <- s sum_t u_t delta_t / (D (T - 1)), the M-step of the same bound, on the device with no
host round trip.  It is EM and nothing more: start it from a SMALL s.  Under a finite nu_proc, from a start 10 .. 100
times too large s does shrink, but the first Gaussian pass has already committed the displaced frames as jumps and the
trajectory stays where it was.  math.inf for a nu makes that side Gaussian; with both infinite the iteration is
refine_smooth_param_em's.

What it is not: neither nu is fitted; one s per keypoint - no shared s over blocks of keypoints, no grouped weights, no
h_fn models in the fit; one side cannot be frozen; the planes do not combine with a caller's own frame-interval scale,
increments or innovations (trajectory draws under them: eks_amd.posterior.sample_singlecam_heavy_tailed).
"""
from __future__ import annotations

import math
from typing import Literal

import numpy as np

from . import hip_ops
from ._problem import check_iteration_counts, linear_problem, singlecam_problem, to_caller

__all__ = ['smooth_heavy_tailed', 'smooth_singlecam_heavy_tailed', 'fit_heavy_tailed', 'fit_singlecam_heavy_tailed']


def smooth_heavy_tailed(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, nu_obs: float = 4.0, nu_proc: float = 4.0,
                        n_iters: int = 12, tol=None, max_iters: int = 64, vs_diag: bool = False,
                        return_device: bool = False, h_fn=None):
    """The smoother's marginals under Student-t observation noise (`nu_obs`) and process noise (`nu_proc`) at once, at
    the smoothing parameters s_finals (scalar or (K,)).  Arguments as smooth_robust: ys (K,T,O); m0s (K,D); S0s, As, Qs
    (K,D,D); Cs (K,O,D); ensemble_vars (T,K,O).  Runs n_iters smoothing passes; the last writes ms, Vs and updates
    nothing, so the planes returned are the ones ms, Vs were smoothed under (n_iters = 1: the Gaussian smoother).
    With `tol` the call continues through both planes in blocks of n_iters passes until both rows of `change` are
    below tol or max_iters passes have run.

    Returns (ms (K,T,D), Vs (K,T,D,D) or its diagonal (K,T,D) with vs_diag, weights (K,T,O), scales (K,T),
    change (2,K)): float32 NumPy arrays, or device tensors with return_device.  change[0] is max |lam_new - lam_old|
    and change[1] max |u_new - u_old|, u = 1 / scale, over the keypoint's frames in the last update (0 when
    n_iters = 1).  h_fn models are not supported."""
    L = linear_problem('smooth_heavy_tailed', ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn)
    nu_obs, n_iters = check_iteration_counts(nu_obs, n_iters, tol, max_iters)
    nu_proc, _ = check_iteration_counts(nu_proc, n_iters, tol, max_iters)
    P, s_dev = L.upload()

    def run(n, weights=None, scales=None):
        return hip_ops.smooth_heavy(P.y, P.var, *P.params, s_dev, nu_obs=nu_obs, nu_proc=nu_proc, n_iters=n,
                                    flags=P.flags, vs_diag=vs_diag, weights=weights, scales=scales,
                                    planes_in=0 if weights is None else 3)

    ms, Vs, weights, scales, change = run(n_iters)
    if tol is not None:
        # a continued block's first pass smooths again under the planes the previous block ended on, so a block of n
        # passes adds n - 1 to `done`: the n_iters of the single call that gives the same bits
        done = n_iters
        while float(change.max()) >= tol and done < max_iters:
            n = min(n_iters, int(max_iters) - done + 1)
            ms, Vs, weights, scales, change = run(n, weights, scales)
            done += n - 1
    return to_caller(return_device, (ms, Vs, weights, scales), (change,))


def smooth_singlecam_heavy_tailed(marker_array, keypoint_names: list, s_finals, *, nu_obs: float = 4.0,
                                  nu_proc: float = 4.0, n_iters: int = 12, tol=None, max_iters: int = 64,
                                  avg_mode: Literal['mean', 'median'] = 'median',
                                  var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """The single-camera smoother under Student-t noise on both sides.  Rebuilds the ensemble, the centring and the
    prior as ensemble_kalman_smoother_singlecam does.  Returns a dict of float32 arrays:
        ms (T, K, 2)        smoothed x, y in PIXEL coordinates (the centring mean added back, as the driver does)
        Vs (T, K, 2)        their posterior variances
        weights (T, K, 2)   the observation weights of x and y
        scales (T, K)       the process-noise scale of the step into every frame, shared by x and y
    s_finals: the smoothing parameters the driver returned - found by its search on the Gaussian model."""
    check_iteration_counts(nu_obs, n_iters, tol, max_iters)
    check_iteration_counts(nu_proc, n_iters, tol, max_iters)
    model, _, mu = singlecam_problem('smooth_singlecam_heavy_tailed', marker_array, keypoint_names, avg_mode, var_mode)
    ms, Vs, weights, scales, _ = smooth_heavy_tailed(*model, s_finals, nu_obs=nu_obs, nu_proc=nu_proc, n_iters=n_iters,
                                                     tol=tol, max_iters=max_iters, vs_diag=True)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu.astype(np.float32)[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)),
                weights=np.ascontiguousarray(np.swapaxes(weights, 0, 1)),
                scales=np.ascontiguousarray(np.swapaxes(scales, 0, 1)))


def _check_fit(nu_obs, nu_proc, n_iters, log_s_bounds):
    nus = []
    for nu in (nu_obs, nu_proc):
        nu = float(nu)
        if not nu > 0:                                      # NaN included; math.inf is a Gaussian side
            raise ValueError('nu must be positive (math.inf: that side is Gaussian)')
        nus.append(nu)
    if int(n_iters) != n_iters or n_iters < 1:
        raise ValueError('n_iters must be an integer >= 1')
    lo, hi = (float(v) for v in log_s_bounds)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):            # the C entry's rule; lo == hi pins s
        raise ValueError('log_s_bounds must be (lo, hi), finite, with lo <= hi')
    return nus[0], nus[1], int(n_iters), (lo, hi)


def fit_heavy_tailed(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_init, *, nu_obs: float = 4.0, nu_proc: float = 4.0,
                     n_iters: int = 40, log_s_bounds=(-8.0, 8.0), vs_diag: bool = False, return_device: bool = False,
                     h_fn=None):
    """smooth_heavy_tailed that also fits the smoothing parameters: n_iters smoothing passes, every one but the last
    followed by the updates of both planes and then by the M-step for s (module docstring).  s_init: scalar or (K,),
    the start - the first pass smooths under it.  Either nu may be math.inf: that side is Gaussian and its plane comes
    back as ones (general models need a finite nu_obs).  log s is kept inside log_s_bounds (refine_smooth_param_em's
    default).  Needs at least two frames.

    Returns (ms, Vs, weights, scales, s_fit (K,) float64, change (3,K)): as smooth_heavy_tailed, with s_fit the
    parameters ms, Vs were smoothed under and change[2] the |delta log s| of the last update."""
    L = linear_problem('fit_heavy_tailed', ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_init, h_fn)
    nu_obs, nu_proc, n_iters, bounds = _check_fit(nu_obs, nu_proc, n_iters, log_s_bounds)
    if L.T < 2:
        raise ValueError('fitting s needs at least two frames')
    P, s_dev = L.upload()
    ms, Vs, weights, scales, s_fit, change = hip_ops.smooth_heavy_fit(
        P.y, P.var, *P.params, s_dev, nu_obs=nu_obs, nu_proc=nu_proc, n_iters=n_iters, log_s_bounds=bounds,
        flags=P.flags, vs_diag=vs_diag)
    out = to_caller(return_device, (ms, Vs, weights, scales), (change,))
    return out[:4] + (s_fit if return_device else s_fit.cpu().numpy(), out[4])


def fit_singlecam_heavy_tailed(marker_array, keypoint_names: list, s_init, *, nu_obs: float = 4.0,
                               nu_proc: float = 4.0, n_iters: int = 40, log_s_bounds=(-8.0, 8.0),
                               avg_mode: Literal['mean', 'median'] = 'median',
                               var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """smooth_singlecam_heavy_tailed with the smoothing parameters fitted from the start s_init (fit_heavy_tailed).
    Returns its dictionary plus s_fit (K,) float64."""
    _check_fit(nu_obs, nu_proc, n_iters, log_s_bounds)
    model, _, mu = singlecam_problem('fit_singlecam_heavy_tailed', marker_array, keypoint_names, avg_mode, var_mode)
    ms, Vs, weights, scales, s_fit, _ = fit_heavy_tailed(*model, s_init, nu_obs=nu_obs, nu_proc=nu_proc, n_iters=n_iters,
                                                         log_s_bounds=log_s_bounds, vs_diag=True)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu.astype(np.float32)[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)),
                weights=np.ascontiguousarray(np.swapaxes(weights, 0, 1)),
                scales=np.ascontiguousarray(np.swapaxes(scales, 0, 1)), s_fit=s_fit)
