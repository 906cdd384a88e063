"""The smoother under heavy-tailed (Student-t) observation noise.

Every other entry point takes the ensemble variance as the variance of a Gaussian observation.  That fails where all
ensemble members jump to the same wrong place - paw swaps, reflections, occlusions: the ensemble variance is small, the
observation is wrong, and the Gaussian smoother believes the frame and drags its neighbours after it
(eks_amd.diagnostics shows such frames as |z| > 3).  The model here keeps the ensemble variance as the SCALE of a
Student-t with nu degrees of freedom, one weight per scalar observation:

    y_t | x_t, lam_t ~ N(C x_t, r_t / lam_t),      lam_t ~ Gamma(nu / 2, rate nu / 2),      r_t = clip(var_t)

and infers the states by the mean-field variational iteration of Agamennoni, Nieto and Nebot (2012): a Gaussian
smoothing pass under r_t / lam_t, then lam_t = (nu + 1) / (nu + delta_t) with delta_t the expected squared standardised
residual of the frame.  The passes run on the device without a host round trip.  The reference has no counterpart.

    smooth_robust(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, nu=4.0, n_iters=8, ...) -> ms, Vs, weights, change
    smooth_singlecam_robust(marker_array, keypoint_names, s_finals, nu=4.0, n_iters=8, ...) -> dict(ms, Vs, weights)

What it is not: nu is not fitted; s_finals comes from the drivers' search on the Gaussian model (there is no search
under the robust model); the weights do not combine with a caller's process-noise scale, the sampler, increments, EM or
innovations (with the Student-t scales of eks_amd.jumps they combine in eks_amd.heavy_tails); one weight per coordinate, not per keypoint.  A weight near (nu + 1) / nu says the frame agrees with its
neighbours, a weight near 0 that it was discounted as an outlier.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from . import hip_ops
from ._problem import check_iteration_counts, iterated_smooth, singlecam_problem

__all__ = ['smooth_robust', 'smooth_singlecam_robust']


def smooth_robust(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, nu: float = 4.0, n_iters: int = 8, tol=None,
                  max_iters: int = 64, vs_diag: bool = False, return_device: bool = False, h_fn=None):
    """The smoother's marginals under Student-t observation noise with `nu` degrees of freedom, at the smoothing
    parameters s_finals (scalar or (K,)).  Arguments as smooth_increments: ys (K,T,O); m0s (K,D); S0s, As, Qs (K,D,D);
    Cs (K,O,D); ensemble_vars (T,K,O).  Runs n_iters smoothing passes; the last writes ms, Vs and updates no weight, so
    the weights returned are the ones ms, Vs were smoothed under (n_iters = 1: the Gaussian smoother, weights 1).
    With `tol` the call continues from its own weights in blocks of n_iters passes until the largest weight change of a
    block's last update is below tol or max_iters passes have run.

    Returns (ms (K,T,D), Vs (K,T,D,D) or its diagonal (K,T,D) with vs_diag, weights (K,T,O), change (K,)): float32
    NumPy arrays, or device tensors with return_device.  change is max |lam_new - lam_old| over the keypoint's frames
    and coordinates in the last weight update (0 when n_iters = 1).  h_fn models are not supported."""
    return iterated_smooth('smooth_robust', hip_ops.smooth_robust, 'weights', (ys, m0s, S0s, As, Cs, Qs, ensemble_vars),
                           s_finals, nu, n_iters, tol, max_iters, vs_diag, return_device, h_fn)


def smooth_singlecam_robust(marker_array, keypoint_names: list, s_finals, *, nu: float = 4.0, n_iters: int = 8, tol=None,
                            max_iters: int = 64, avg_mode: Literal['mean', 'median'] = 'median',
                            var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """The single-camera smoother under Student-t observation noise.  Rebuilds the ensemble, the centring and the prior
    as ensemble_kalman_smoother_singlecam does.  Returns a dict of float32 arrays:
        ms (T, K, 2)        smoothed x, y in PIXEL coordinates (the centring mean added back, as the driver does)
        Vs (T, K, 2)        their posterior variances
        weights (T, K, 2)   the weight of every observed coordinate, in (0, (nu + 1) / nu]
    s_finals: the smoothing parameters the driver returned - found by its search on the Gaussian model."""
    check_iteration_counts(nu, n_iters, tol, max_iters)
    model, _, mu = singlecam_problem('smooth_singlecam_robust', marker_array, keypoint_names, avg_mode, var_mode)
    ms, Vs, weights, _ = smooth_robust(*model, s_finals, nu=nu, n_iters=n_iters, tol=tol, max_iters=max_iters,
                                       vs_diag=True)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu.astype(np.float32)[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)),
                weights=np.ascontiguousarray(np.swapaxes(weights, 0, 1)))
