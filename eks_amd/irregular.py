"""Smoothing sessions whose frames are not evenly spaced: one process-noise scale per frame.

Every other entry point assumes the same process noise s Q at every step.  Cameras drop frames, trigger pulses are
missed, sessions are cut and concatenated, and there are moments (stimulus onset, reach start) where the animal is
known to move more than its average.  The model here is

    x_0 ~ N(m0, S0),      x_t = A x_{t-1} + N(0, s w_t Q)      for t = 1 .. T-1

with one number w_t per frame (or per frame and keypoint).  The reference has no counterpart.

    process_noise_scale_from_times(frame_times, nominal_dt=None) -> w (T,) float32
    smooth_time_varying(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, process_noise_scale) -> ms (K,T,D), Vs
    smooth_singlecam_irregular(marker_array, keypoint_names, s_finals, frame_times=... | process_noise_scale=...)

What the model is, and is not:
  * With A = I (what initialize_kalman_filter and the multi-camera driver build) and w_t = the number of nominal
    frame intervals that elapsed before frame t, it is exactly Brownian motion sampled at the true frame times: a step
    over n intervals of a random walk has process noise n s Q.
  * With a decaying A it is ONLY a process-noise scale: A itself is applied once per frame whatever the elapsed time
    (a time-varying A is not implemented), so a long gap is under-decayed.
  * s_finals comes from the drivers' smoothing-parameter search, which runs on the UNIFORM model; there is no search
    under w_t.
"""
from __future__ import annotations

from typing import Literal

import numpy as np

from . import hip_ops
from ._problem import linear_problem, singlecam_problem, to_caller

__all__ = ['process_noise_scale_from_times', 'smooth_time_varying', 'smooth_singlecam_irregular', 'MAX_SCALE']

MAX_SCALE = 1e6     # the library's precondition: every w is finite and 0 <= w <= 1e6 (include/eks_hip.h)


def process_noise_scale_from_times(frame_times, nominal_dt: float | None = None) -> np.ndarray:
    """Frame timestamps (T,) -> w (T,) float32 with w[0] = 1 (never read) and w[t] = (t_t - t_{t-1}) / nominal_dt: the
    number of nominal frame intervals that elapsed before frame t.  nominal_dt defaults to the median difference, so
    a session with a few dropped frames gets w = 1 on its regular frames.  Raises ValueError on non-finite or
    non-increasing times.  For A = I this makes the smoother's model Brownian motion sampled at the true times; see
    the module docstring for what it means with a decaying A."""
    t = np.asarray(frame_times, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError(f'frame_times must be a non-empty 1-D array; got shape {t.shape}')
    if not np.all(np.isfinite(t)):
        raise ValueError('frame_times must be finite')
    dt = np.diff(t)
    if np.any(dt <= 0):
        raise ValueError('frame_times must be strictly increasing')
    if nominal_dt is None:
        nominal_dt = float(np.median(dt)) if dt.size else 1.0
    if not (np.isfinite(nominal_dt) and nominal_dt > 0):
        raise ValueError('nominal_dt must be positive and finite')
    w = np.ones(t.size, dtype=np.float32)
    w[1:] = dt / nominal_dt
    return w


def _check_scale(w, K: int, T: int) -> np.ndarray:
    """-> float32 (T,) or frame-major (T, K), from (T,) or (K, T)."""
    w = np.asarray(w, dtype=np.float64)
    if w.shape not in ((T,), (K, T)):
        raise ValueError(f'process_noise_scale must be {(T,)} or {(K, T)}; got {w.shape}')
    body = w[..., 1:]                         # entry 0 is never read
    if not np.all(np.isfinite(body)) or np.any(body < 0) or np.any(body > MAX_SCALE):
        raise ValueError(f'process_noise_scale must be finite and in [0, {MAX_SCALE:g}] (frame 0 aside)')
    w32 = w.astype(np.float32)
    w32[..., 0] = 1.0
    return np.ascontiguousarray(w32 if w32.ndim == 1 else w32.T)


def smooth_time_varying(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, process_noise_scale, *,
                        vs_diag: bool = False, return_device: bool = False, h_fn=None):
    """The smoother's marginals under x_t = A x_{t-1} + N(0, s w_t Q), at the smoothing parameters s_finals (scalar or
    (K,)).  Arguments as smooth_increments: ys (K,T,O); m0s (K,D); S0s, As, Qs (K,D,D); Cs (K,O,D); ensemble_vars
    (T,K,O).  process_noise_scale is w: (T,) shared by all keypoints or (K, T); w[t] scales the noise of the step into
    frame t, w[0] is ignored, and every other entry must be finite and in [0, 1e6] (ValueError otherwise; w = 0 says
    "no motion over this step").  Returns ms (K, T, D) and Vs (K, T, D, D), or its diagonal (K, T, D) with vs_diag:
    float32 NumPy arrays, or device tensors with return_device, views of the kernels' frame-major buffers.

    With A = I and w = elapsed frame intervals (process_noise_scale_from_times) the model is Brownian motion sampled
    at the true frame times.  With a decaying A it is only a process-noise scale: A itself is applied once per frame.
    s_finals usually comes from the drivers' search, which runs on the uniform model.  h_fn models are not
    supported."""
    L = linear_problem('smooth_time_varying', ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn)
    w = _check_scale(process_noise_scale, L.K, L.T)
    P, s_dev = L.upload()
    from .core import _torch
    ms, Vs = hip_ops.smooth_tv(P.y, P.var, _torch().as_tensor(w, device=P.dev), *P.params, s_dev, flags=P.flags,
                               vs_diag=vs_diag)
    return to_caller(return_device, (ms, Vs))


def smooth_singlecam_irregular(marker_array, keypoint_names: list, s_finals, *, frame_times=None,
                               process_noise_scale=None, avg_mode: Literal['mean', 'median'] = 'median',
                               var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """The single-camera smoother on a session with uneven frame intervals.  Takes exactly one of frame_times (T,)
    - converted by process_noise_scale_from_times - and process_noise_scale (T,) or (K, T).  Rebuilds the ensemble, the
    centring and the prior as ensemble_kalman_smoother_singlecam does.  Returns a dict of float32 arrays:
        ms (T, K, 2)   smoothed x, y in PIXEL coordinates (the centring mean added back, as the driver does)
        Vs (T, K, 2)   their posterior variances
    This driver's A is the identity, so with frame_times the model is Brownian motion sampled at the true times.
    s_finals: the smoothing parameters the driver returned - found by its search on the uniform model."""
    if (frame_times is None) == (process_noise_scale is None):
        raise ValueError('give exactly one of frame_times and process_noise_scale')
    if frame_times is not None:
        T = marker_array.shape[2]
        if np.shape(frame_times) != (T,):
            raise ValueError(f'frame_times must be {(T,)}; got {np.shape(frame_times)}')
        process_noise_scale = process_noise_scale_from_times(frame_times)
    model, _, mu = singlecam_problem('smooth_singlecam_irregular', marker_array, keypoint_names, avg_mode, var_mode)
    ms, Vs = smooth_time_varying(*model, s_finals, process_noise_scale, vs_diag=True)
    return dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu.astype(np.float32)[None],
                Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)))
