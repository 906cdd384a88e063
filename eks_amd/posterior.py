"""Joint posterior trajectories of the Kalman smoother.

Everything `run_kalman_smoother` returns is a per-frame marginal (ms[t], Vs[t]).  An error bar on anything that spans
frames or keypoints - speed, path length, the time of a peak, the distance between two paws - needs whole
trajectories from the smoothing distribution p(x_1..x_T | y_1..y_T); independent draws from N(ms[t], Vs[t]) give
white-noise paths.  The reference has no counterpart.

    sample_kalman_posterior(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, n_draws, ...) -> (K, n_draws, T, D)
    sample_singlecam(marker_array, keypoint_names, s_finals, n_draws, ...) -> (n_draws, T, K, 2) in pixels

The commonest such quantity - the frame-to-frame increment x_{t+1} - x_t behind velocity, speed and movement onsets -
has a closed form inside the smoother's backward pass and needs no draws:

    smooth_increments(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, ...) -> (ms, Vs, lag1, dmean, dV)
    velocity_singlecam(marker_array, keypoint_names, s_finals, fps=...) -> velocity, velocity_var, speed_rms
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Literal

import numpy as np

from . import hip_ops
from ._problem import linear_problem, singlecam_problem, to_caller

__all__ = ['sample_kalman_posterior', 'sample_singlecam', 'smooth_increments', 'velocity_singlecam', 'SmoothIncrements']

DEFAULT_MEMORY_BUDGET = 2 << 30     # bytes of device memory one group of draws (output + workspace) may take


def draws_per_group(K: int, T: int, D: int, O: int, flags: int, n_draws: int, memory_budget: int) -> int:
    """Largest number of draws whose output and workspace fit the budget (at least 1)."""
    from . import _lib
    lib = _lib.load()
    dims = _lib.EksDims(K, T, D, O, flags & ~_lib.FLAG_VS_DIAG)
    g = int(n_draws)
    while g > 1 and lib.eks_sample_workspace_bytes(ctypes.byref(dims), g) + g * T * K * D * 4 > memory_budget:
        g = (g + 1) // 2
    return g


def sample_kalman_posterior(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, n_draws: int, *, seed: int = 0,
                            noise=None, first_keypoint: int = 0, first_draw: int = 0, return_device: bool = False,
                            return_mean: bool = False, h_fn=None, memory_budget: int = DEFAULT_MEMORY_BUDGET):
    """n_draws trajectories from p(x_1..x_T | y_1..y_T) of the linear model run_kalman_smoother smooths, at the
    smoothing parameters s_finals (scalar or (K,)).  Arguments as run_kalman_smoother: ys (K,T,O); m0s (K,D); S0s, As,
    Qs (K,D,D); Cs (K,O,D); ensemble_vars (T,K,O).  Returns float32 (K, n_draws, T, D), a transposed view of the
    kernels' (n_draws, T, K, D) buffer (a NumPy array, or a device tensor with return_device); with return_mean also
    the smoothed mean (K, T, D) of the same pass.

    The normals come from a counter-based generator keyed by `seed` and indexed by (frame, first_keypoint + k,
    first_draw + d): keypoints [k0, k1) or draws [d0, d1) of a larger problem are reproduced bit for bit by a call on
    those alone with first_keypoint = k0 / first_draw = d0.  Draws are produced in groups whose output and workspace
    fit `memory_budget` bytes of device memory, which changes no value.  noise (n_draws, T, K, W) float32 replaces
    the generator (W = D on diagonal models, D + O otherwise; zeros return the smoothed mean)."""
    L = linear_problem('sample_kalman_posterior', ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn)
    if int(n_draws) != n_draws or n_draws < 1:
        raise ValueError('n_draws must be an integer >= 1')
    if first_keypoint < 0 or first_draw < 0:
        raise ValueError('first_keypoint and first_draw must be >= 0')
    K, T, O, D, flags, n_draws = L.K, L.T, L.O, L.D, L.flags, int(n_draws)
    W = hip_ops.sample_noise_width(D, O, flags)
    if noise is not None and tuple(np.shape(noise)) != (n_draws, T, K, W):
        raise ValueError(f'noise must be {(n_draws, T, K, W)}; got {tuple(np.shape(noise))}')
    from .core import _to_host, _torch
    torch = _torch()
    P, s_dev = L.upload()
    if noise is not None:
        noise = torch.as_tensor(noise, device=P.dev).to(torch.float32).contiguous()
    group = draws_per_group(K, T, D, O, flags, n_draws, memory_budget)
    out_dev = torch.empty((n_draws, T, K, D), dtype=torch.float32, device=P.dev) if return_device else None
    out_host = None if return_device else np.empty((n_draws, T, K, D), dtype=np.float32)
    ms = None
    for d0 in range(0, n_draws, group):
        d1 = min(n_draws, d0 + group)
        dr, m = hip_ops.sample(P.y, P.var, *P.params, s_dev, d1 - d0, seed=seed, flags=P.flags,
                               first_keypoint=first_keypoint, first_draw=first_draw + d0,
                               noise=None if noise is None else noise[d0:d1],
                               want_mean=return_mean and d0 == 0, out=None if out_dev is None else out_dev[d0:d1])
        if m is not None:
            ms = m
        if out_host is not None:
            out_host[d0:d1] = _to_host(dr)[0]
    draws = out_dev.permute(2, 0, 1, 3) if return_device else np.transpose(out_host, (2, 0, 1, 3))
    return (draws, *to_caller(return_device, (ms,))) if return_mean else draws


def sample_singlecam(marker_array, keypoint_names: list, s_finals, n_draws: int, *, seed: int = 0,
                     avg_mode: Literal['mean', 'median'] = 'median',
                     var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var',
                     memory_budget: int = DEFAULT_MEMORY_BUDGET) -> np.ndarray:
    """Posterior trajectories of the single-camera smoother in PIXEL coordinates, (n_draws, T, K, 2) float32.
    Rebuilds the ensemble, the centring and the prior as ensemble_kalman_smoother_singlecam does and adds the same
    means back: over many draws the mean approaches that driver's x, y columns and the variance its
    x_posterior_var, y_posterior_var columns.  s_finals: the smoothing parameters the driver returned."""
    model, _, mu = singlecam_problem('sample_singlecam', marker_array, keypoint_names, avg_mode, var_mode)
    draws = sample_kalman_posterior(*model, s_finals, n_draws, seed=seed, memory_budget=memory_budget)
    return np.ascontiguousarray(np.transpose(draws, (1, 2, 0, 3))) + mu.astype(np.float32)[None, None]


SmoothIncrements = namedtuple('SmoothIncrements', ['ms', 'Vs', 'lag1', 'dmean', 'dV'])


def smooth_increments(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, full_cov: bool = False,
                      return_device: bool = False, h_fn=None) -> SmoothIncrements:
    """The smoother's marginals plus the posterior of the frame-to-frame increment, at the smoothing parameters
    s_finals (scalar or (K,)), in one pass.  Arguments as sample_kalman_posterior.  Returns the named tuple
        ms (K, T, D), Vs, lag1 = Cov(x_t, x_{t+1} | y), dmean (K, T-1, D) = E[x_{t+1} - x_t | y],
        dV = Cov(x_{t+1} - x_t | y)
    with Vs (K, T, D) and lag1, dV (K, T-1, D) holding diagonals, or the D x D matrices with full_cov (lag1: row =
    coordinate of x_t, column = coordinate of x_{t+1}).  float32 NumPy arrays, or device tensors with return_device;
    all are views of the kernels' frame-major buffers, like run_kalman_smoother's.  dV is formed inside the
    backward pass as a sum of non-negative terms: Vs[t] + Vs[t+1] - 2 lag1[t] from the float32 outputs loses it to
    cancellation under heavy smoothing."""
    L = linear_problem('smooth_increments', ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn)
    from . import _lib
    from .core import _torch
    P, s_dev = L.upload()
    diag_model = bool(P.flags & _lib.FLAG_DIAG_MODEL)
    out = hip_ops.smooth_increments(P.y, P.var, *P.params, s_dev, flags=P.flags, vs_diag=diag_model or not full_cov)
    names = SmoothIncrements._fields
    embed = ('Vs', 'lag1', 'dV') if diag_model and full_cov else ()      # scalar chains: the matrices are the diagonal
    if return_device:                                                   # embedding, made before the (K, T) view is taken
        out.update({n: _torch().diag_embed(out[n]) for n in embed})
    res = dict(zip(names, to_caller(return_device, [out[n] for n in names])))
    if not return_device:
        eye = np.eye(L.D, dtype=np.float32)
        res.update({n: res[n][..., :, None] * eye for n in embed})
    T = L.T
    return SmoothIncrements(res['ms'], res['Vs'], res['lag1'][:, :T - 1], res['dmean'][:, :T - 1], res['dV'][:, :T - 1])


def velocity_singlecam(marker_array, keypoint_names: list, s_finals, *, fps: float = 1.0,
                       avg_mode: Literal['mean', 'median'] = 'median',
                       var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """Posterior of the velocity of the single-camera smoother, in pixels per second at `fps` frames per second.
    Rebuilds the ensemble, the centring and the prior as ensemble_kalman_smoother_singlecam does (the centring means
    cancel in an increment, so nothing is added back).  Returns a dict of float32 arrays:
        velocity     (T-1, K, 2)  E[x_{t+1} - x_t | y] fps
        velocity_var (T-1, K, 2)  Var(x_{t+1} - x_t | y) fps^2
        speed_rms    (T-1, K)     sqrt(E |v|^2) = fps sqrt(sum_d dmean^2 + dV): the exact root of the second moment
    s_finals: the smoothing parameters the driver returned."""
    if not fps > 0:
        raise ValueError('fps must be positive')
    model, _, _ = singlecam_problem('velocity_singlecam', marker_array, keypoint_names, avg_mode, var_mode)
    inc = smooth_increments(*model, s_finals)
    f = np.float32(fps)
    dmean = np.swapaxes(inc.dmean, 0, 1)                                        # (T-1, K, 2)
    dV = np.swapaxes(inc.dV, 0, 1)
    return dict(velocity=dmean * f, velocity_var=dV * (f * f),
                speed_rms=f * np.sqrt((dmean * dmean + dV).sum(axis=-1)))
