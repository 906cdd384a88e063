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
under the robust model); the weights do not combine with a process-noise scale, the sampler, increments, EM or
innovations; one weight per coordinate, not per keypoint.  A weight near (nu + 1) / nu says the frame agrees with its
neighbours, a weight near 0 that it was discounted as an outlier.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from . import hip_ops
from .posterior import _host_flags, _validate

__all__ = ['smooth_robust', 'smooth_singlecam_robust']


def _check_counts(nu, n_iters, tol, max_iters):
    nu = float(nu)
    if not (np.isfinite(nu) and nu > 0):
        raise ValueError('nu must be positive and finite')
    if int(n_iters) != n_iters or n_iters < 1:
        raise ValueError('n_iters must be an integer >= 1')
    if tol is not None:
        if not (np.isfinite(tol) and tol > 0):
            raise ValueError('tol must be positive and finite')
        if int(max_iters) != max_iters or max_iters < n_iters:
            raise ValueError('max_iters must be an integer >= n_iters')
        if n_iters < 2:
            raise ValueError('tol needs n_iters >= 2: a single pass updates no weight')
    return nu, int(n_iters)


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
    if h_fn is not None:
        raise NotImplementedError('smooth_robust covers linear models; h_fn models are not supported')
    nu, n_iters = _check_counts(nu, n_iters, tol, max_iters)
    K, T, O, D, s = _validate(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, 1, None, 0, 0)
    flags = _host_flags(S0s, As, Cs, Qs)
    from .core import _DeviceProblem, _to_host, _torch
    torch = _torch()
    P = _DeviceProblem(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, flags=flags)
    s_dev = torch.as_tensor(s, device=P.dev)

    def run(n, weights=None):
        return hip_ops.smooth_robust(P.y, P.var, *P.params, s_dev, nu=nu, n_iters=n, flags=P.flags, vs_diag=vs_diag,
                                     weights=weights, weights_in=weights is not None)

    ms, Vs, weights, change = run(n_iters)
    if tol is not None:
        # a continued block's first pass smooths again under the weights the previous block ended on, so a block of n
        # passes adds n - 1 to `done`: the n_iters of the single call that gives the same bits
        done = n_iters
        while float(change.max()) >= tol and done < max_iters:
            n = min(n_iters, int(max_iters) - done + 1)
            ms, Vs, weights, change = run(n, weights)
            done += n - 1
    if return_device:
        return ms.transpose(0, 1), Vs.transpose(0, 1), weights.transpose(0, 1), change
    ms, Vs, weights, change = _to_host(ms, Vs, weights, change)
    return np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1), np.swapaxes(weights, 0, 1), change


def smooth_singlecam_robust(marker_array, keypoint_names: list, s_finals, *, nu: float = 4.0, n_iters: int = 8, tol=None,
                            max_iters: int = 64, avg_mode: Literal['mean', 'median'] = 'median',
                            var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """The single-camera smoother under Student-t observation noise.  Rebuilds the ensemble, the centring and the prior
    as ensemble_kalman_smoother_singlecam does.  Returns a dict of float32 arrays:
        ms (T, K, 2)        smoothed x, y in PIXEL coordinates (the centring mean added back, as the driver does)
        Vs (T, K, 2)        their posterior variances
        weights (T, K, 2)   the weight of every observed coordinate, in (0, (nu + 1) / nu]
    s_finals: the smoothing parameters the driver returned - found by its search on the Gaussian model."""
    from .core import ensemble
    from .singlecam_smoother import initialize_kalman_filter
    from .utils import center_predictions
    M, V, T, K, _ = marker_array.shape
    if V != 1:
        raise ValueError('smooth_singlecam_robust takes a single-view marker array')
    if len(keypoint_names) != K:
        raise ValueError(f'{len(keypoint_names)} keypoint names for {K} keypoints')
    _check_counts(nu, n_iters, tol, max_iters)
    ens = ensemble(marker_array, avg_mode=avg_mode, var_mode=var_mode)
    _, centered, _, means = center_predictions(ens, quantile_keep_pca=100)
    stats = np.asarray(ens.array)[0, 0]
    cen = np.asarray(centered.array)[0, 0]
    m0s, S0s, As, Qs, Cs = initialize_kalman_filter(centered)
    ms, Vs, weights, _ = smooth_robust(np.swapaxes(cen, 0, 1), m0s, S0s, As, Cs, Qs, stats[:, :, 2:4], s_finals, nu=nu,
                                       n_iters=n_iters, tol=tol, max_iters=max_iters, vs_diag=True)
    mu = np.asarray(means.array)[0, 0, 0].astype(np.float32)                     # (K,2)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)),
                weights=np.ascontiguousarray(np.swapaxes(weights, 0, 1)))
