"""The smoother under heavy-tailed (Student-t) process noise.

The drivers find one smoothing parameter s per keypoint and apply it to every frame.  A paw reach, a saccade or a
startle is a few frames of motion a hundred times larger than the rest of the session: under a single s the smoother
must either round such an event off, or follow it and under-smooth the still frames.  eks_amd.robust puts a Student-t
on the OBSERVATION side, which handles a wrong observation; the model here puts it on the PROCESS side, which handles a
true fast movement.  One weight per keypoint and frame, shared by the keypoint's D state coordinates (they jump
together):

    x_t = A x_{t-1} + eps_t,     eps_t | u_t ~ N(0, s Q / u_t),     u_t ~ Gamma(nu / 2, rate nu / 2),     t = 1 .. T-1

with the Gaussian smoother's prior and observations.  The states are inferred by the mean-field variational iteration:
a Gaussian smoothing pass under the per-keypoint scales w_t = 1 / u_t (smooth_time_varying's model), then
w_t = (nu + delta_t) / (nu + D) with delta_t = E[eps_t' (s Q)^-1 eps_t | y] under the pass's own scales.  The passes
run on the device without a host round trip.  The reference has no counterpart.

    smooth_jumps(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, nu=4.0, n_iters=12, ...) -> ms, Vs, scales, change
    smooth_singlecam_jumps(marker_array, keypoint_names, s_finals, nu=4.0, n_iters=12, ...) -> dict(ms, Vs, scales)

A scale near 1 (at most a few) says the frame moved like the rest of the session; a scale of hundreds or thousands
marks a jump INTO that frame.  The returned scales are exactly what smooth_time_varying takes as `w`.

What it is not: nu is not fitted; s_finals comes from the drivers' search on the Gaussian model (there is no search
under this model); the scales do not combine with a caller's own frame-interval scale, the sampler, increments, EM
or innovations.  With eks_amd.robust's observation weights they combine in
eks_amd.heavy_tails: a session with wrong observations AND fast movements wants that model.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from . import hip_ops
from ._problem import check_iteration_counts, iterated_smooth, singlecam_problem

__all__ = ['smooth_jumps', 'smooth_singlecam_jumps']


def smooth_jumps(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, nu: float = 4.0, n_iters: int = 12, tol=None,
                 max_iters: int = 64, vs_diag: bool = False, return_device: bool = False, h_fn=None):
    """The smoother's marginals under Student-t process noise with `nu` degrees of freedom, at the smoothing
    parameters s_finals (scalar or (K,)).  Arguments as smooth_robust: ys (K,T,O); m0s (K,D); S0s, As, Qs (K,D,D);
    Cs (K,O,D); ensemble_vars (T,K,O).  Runs n_iters smoothing passes; the last writes ms, Vs and updates no scale, so
    the scales returned are the ones ms, Vs were smoothed under (n_iters = 1: the Gaussian smoother, scales 1).
    With `tol` the call continues from its own scales in blocks of n_iters passes until the largest change of
    u = 1 / scale in a block's last update is below tol or max_iters passes have run.

    Returns (ms (K,T,D), Vs (K,T,D,D) or its diagonal (K,T,D) with vs_diag, scales (K,T), change (K,)): float32 NumPy
    arrays, or device tensors with return_device.  scales[k, t] is the process-noise scale of the step into frame t
    (entry 0 is 1 and unused): what smooth_time_varying takes as w.  change is max |u_new - u_old| over the keypoint's
    frames in the last update (0 when n_iters = 1).  h_fn models are not supported."""
    return iterated_smooth('smooth_jumps', hip_ops.smooth_jumps, 'scales', (ys, m0s, S0s, As, Cs, Qs, ensemble_vars),
                           s_finals, nu, n_iters, tol, max_iters, vs_diag, return_device, h_fn)


def smooth_singlecam_jumps(marker_array, keypoint_names: list, s_finals, *, nu: float = 4.0, n_iters: int = 12, tol=None,
                           max_iters: int = 64, avg_mode: Literal['mean', 'median'] = 'median',
                           var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """The single-camera smoother under Student-t process noise.  Rebuilds the ensemble, the centring and the prior
    as ensemble_kalman_smoother_singlecam does.  Returns a dict of float32 arrays:
        ms (T, K, 2)      smoothed x, y in PIXEL coordinates (the centring mean added back, as the driver does)
        Vs (T, K, 2)      their posterior variances
        scales (T, K)     the process-noise scale of the step into every frame, shared by x and y
    s_finals: the smoothing parameters the driver returned - found by its search on the Gaussian model."""
    check_iteration_counts(nu, n_iters, tol, max_iters)
    model, _, mu = singlecam_problem('smooth_singlecam_jumps', marker_array, keypoint_names, avg_mode, var_mode)
    ms, Vs, scales, _ = smooth_jumps(*model, s_finals, nu=nu, n_iters=n_iters, tol=tol, max_iters=max_iters,
                                     vs_diag=True)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu.astype(np.float32)[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)),
                scales=np.ascontiguousarray(np.swapaxes(scales, 0, 1)))
