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
under this model); the scales do not combine with eks_amd.robust's observation weights, a caller's own frame-interval
scale, the sampler, increments, EM or innovations.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from . import hip_ops
from .posterior import _host_flags, _validate
from .robust import _check_counts

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
    if h_fn is not None:
        raise NotImplementedError('smooth_jumps covers linear models; h_fn models are not supported')
    nu, n_iters = _check_counts(nu, n_iters, tol, max_iters)
    K, T, O, D, s = _validate(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, 1, None, 0, 0)
    flags = _host_flags(S0s, As, Cs, Qs)
    from .core import _DeviceProblem, _to_host, _torch
    torch = _torch()
    P = _DeviceProblem(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, flags=flags)
    s_dev = torch.as_tensor(s, device=P.dev)

    def run(n, scales=None):
        return hip_ops.smooth_jumps(P.y, P.var, *P.params, s_dev, nu=nu, n_iters=n, flags=P.flags, vs_diag=vs_diag,
                                    scales=scales, scales_in=scales is not None)

    ms, Vs, scales, change = run(n_iters)
    if tol is not None:
        # a continued block's first pass smooths again under the scales the previous block ended on, so a block of n
        # passes adds n - 1 to `done`: the n_iters of the single call that gives the same bits
        done = n_iters
        while float(change.max()) >= tol and done < max_iters:
            n = min(n_iters, int(max_iters) - done + 1)
            ms, Vs, scales, change = run(n, scales)
            done += n - 1
    if return_device:
        return ms.transpose(0, 1), Vs.transpose(0, 1), scales.transpose(0, 1), change
    ms, Vs, scales, change = _to_host(ms, Vs, scales, change)
    return np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1), np.swapaxes(scales, 0, 1), change


def smooth_singlecam_jumps(marker_array, keypoint_names: list, s_finals, *, nu: float = 4.0, n_iters: int = 12, tol=None,
                           max_iters: int = 64, avg_mode: Literal['mean', 'median'] = 'median',
                           var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """The single-camera smoother under Student-t process noise.  Rebuilds the ensemble, the centring and the prior
    as ensemble_kalman_smoother_singlecam does.  Returns a dict of float32 arrays:
        ms (T, K, 2)      smoothed x, y in PIXEL coordinates (the centring mean added back, as the driver does)
        Vs (T, K, 2)      their posterior variances
        scales (T, K)     the process-noise scale of the step into every frame, shared by x and y
    s_finals: the smoothing parameters the driver returned - found by its search on the Gaussian model."""
    from .core import ensemble
    from .singlecam_smoother import initialize_kalman_filter
    from .utils import center_predictions
    M, V, T, K, _ = marker_array.shape
    if V != 1:
        raise ValueError('smooth_singlecam_jumps takes a single-view marker array')
    if len(keypoint_names) != K:
        raise ValueError(f'{len(keypoint_names)} keypoint names for {K} keypoints')
    _check_counts(nu, n_iters, tol, max_iters)
    ens = ensemble(marker_array, avg_mode=avg_mode, var_mode=var_mode)
    _, centered, _, means = center_predictions(ens, quantile_keep_pca=100)
    stats = np.asarray(ens.array)[0, 0]
    cen = np.asarray(centered.array)[0, 0]
    m0s, S0s, As, Qs, Cs = initialize_kalman_filter(centered)
    ms, Vs, scales, _ = smooth_jumps(np.swapaxes(cen, 0, 1), m0s, S0s, As, Cs, Qs, stats[:, :, 2:4], s_finals, nu=nu,
                                     n_iters=n_iters, tol=tol, max_iters=max_iters, vs_diag=True)
    mu = np.asarray(means.array)[0, 0, 0].astype(np.float32)                     # (K,2)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)),
                scales=np.ascontiguousarray(np.swapaxes(scales, 0, 1)))
