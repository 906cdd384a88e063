"""Joint posterior trajectories of the Kalman smoother.

Everything `run_kalman_smoother` returns is a per-frame marginal (ms[t], Vs[t]).  An error bar on anything that spans
frames or keypoints - speed, path length, the time of a peak, the distance between two paws - needs whole
trajectories from the smoothing distribution p(x_1..x_T | y_1..y_T); independent draws from N(ms[t], Vs[t]) give
white-noise paths.  The reference has no counterpart.

    sample_kalman_posterior(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, n_draws, ...) -> (K, n_draws, T, D)
    sample_singlecam(marker_array, keypoint_names, s_finals, n_draws, ...) -> (n_draws, T, K, 2) in pixels

Under the models of eks_amd.irregular, .robust, .jumps and .heavy_tails - a per-frame process-noise scale w and
observation weights lam - the Gaussian factor of the posterior is the smoothing distribution of
x_t = A x_{t-1} + N(0, s w_t Q), y_t = C x_t + N(0, r_t / lam_t), and sample_kalman_posterior(..., qscale=w, weights=lam)
draws from it (eks_sample_tv).  Three drivers build the planes and sample under them:

    sample_singlecam_irregular(marker_array, keypoint_names, s_finals, n_draws, frame_times=...)
    sample_singlecam_heavy_tailed(marker_array, keypoint_names, s, n_draws, nu_obs=4.0, nu_proc=4.0, n_iters=12, ...)
    sample_multicam_robust(marker_array, keypoint_names, camera_names, s_finals, n_draws, ...) -> (n_draws, T, K, 2V)

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

__all__ = ['sample_kalman_posterior', 'sample_singlecam', 'sample_singlecam_irregular', 'sample_singlecam_heavy_tailed',
           'sample_multicam_robust', 'smooth_increments', 'velocity_singlecam', 'SmoothIncrements']

DEFAULT_MEMORY_BUDGET = 2 << 30     # bytes of device memory one group of draws (output + workspace) may take


def draws_per_group(K: int, T: int, D: int, O: int, flags: int, n_draws: int, memory_budget: int,
                    planes: bool = False) -> int:
    """Largest number of draws whose output and workspace fit the budget (at least 1).  planes: the call goes through
    eks_sample_tv, whose own size function is asked."""
    from . import _lib
    lib = _lib.load()
    dims = _lib.EksDims(K, T, D, O, flags & ~_lib.FLAG_VS_DIAG)
    size = lib.eks_sample_workspace_bytes
    if planes:
        size = lambda d, g: hip_ops.sample_tv_workspace_bytes(K, T, D, O, flags, g)  # noqa: E731
    g = int(n_draws)
    while g > 1 and size(ctypes.byref(dims), g) + g * T * K * D * 4 > memory_budget:
        g = (g + 1) // 2
    return g


def _sample_planes(qscale, weights, K: int, T: int, O: int):
    """qscale (T,) or (K, T) and weights (K, T, O) or grouped (K, T, O / g) -> float32 frame-major host arrays (T,) or
    (T, K) and (T, K, O), each None where the argument is."""
    w = lam = None
    if qscale is not None:
        from .irregular import _check_scale
        w = _check_scale(qscale, K, T)
    if weights is not None:
        lam = np.asarray(weights, dtype=np.float64)
        if lam.ndim != 3 or lam.shape[:2] != (K, T) or lam.shape[2] < 1 or O % lam.shape[2]:
            raise ValueError(f'weights must be {(K, T, O)} or grouped (K, T, O / g); got {lam.shape}')
        if not np.all(np.isfinite(lam)) or np.any(lam <= 0):
            raise ValueError('weights must be finite and positive')
        lam = np.repeat(lam, O // lam.shape[2], axis=2)                  # one weight per coordinate
        lam = np.ascontiguousarray(np.swapaxes(lam, 0, 1), dtype=np.float32)
        if np.any(lam <= 0):
            raise ValueError('weights must be positive in float32')
    return w, lam


def sample_kalman_posterior(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, n_draws: int, *, seed: int = 0,
                            noise=None, first_keypoint: int = 0, first_draw: int = 0, return_device: bool = False,
                            return_mean: bool = False, h_fn=None, memory_budget: int = DEFAULT_MEMORY_BUDGET,
                            qscale=None, weights=None):
    """n_draws trajectories from p(x_1..x_T | y_1..y_T) of the linear model run_kalman_smoother smooths, at the
    smoothing parameters s_finals (scalar or (K,)).  Arguments as run_kalman_smoother: ys (K,T,O); m0s (K,D); S0s, As,
    Qs (K,D,D); Cs (K,O,D); ensemble_vars (T,K,O).  Returns float32 (K, n_draws, T, D), a transposed view of the
    kernels' (n_draws, T, K, D) buffer (a NumPy array, or a device tensor with return_device); with return_mean also
    the smoothed mean (K, T, D) of the same pass.

    The normals come from a counter-based generator keyed by `seed` and indexed by (frame, first_keypoint + k,
    first_draw + d): keypoints [k0, k1) or draws [d0, d1) of a larger problem are reproduced bit for bit by a call on
    those alone with first_keypoint = k0 / first_draw = d0.  Draws are produced in groups whose output and workspace
    fit `memory_budget` bytes of device memory, which changes no value.  noise (n_draws, T, K, W) float32 replaces
    the generator (W = D on diagonal models, D + O otherwise; zeros return the smoothed mean).

    qscale / weights: draw under x_t = A x_{t-1} + N(0, s w_t Q), y_t = C x_t + N(0, r_t / lam_t) instead (eks_sample_tv; with
    both None the call is eks_sample exactly).  qscale is w, (T,) or (K, T) as smooth_time_varying takes it - or the
    scales smooth_jumps / smooth_heavy_tailed return; weights is lam, (K, T, O) as smooth_robust / smooth_heavy_tailed
    return it, or grouped (K, T, O / g) as smooth_robust_grouped does (expanded here), finite and > 0.  The degrees of
    freedom do not enter: the planes ARE the model.  The generator, first_keypoint / first_draw and noise are unchanged."""
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
    planes = qscale is not None or weights is not None
    w, lam = _sample_planes(qscale, weights, K, T, O)
    P, s_dev = L.upload()
    if noise is not None:
        noise = torch.as_tensor(noise, device=P.dev).to(torch.float32).contiguous()
    group = draws_per_group(K, T, D, O, flags, n_draws, memory_budget, planes)
    if planes:
        w = None if w is None else torch.as_tensor(w, device=P.dev)
        lam = None if lam is None else torch.as_tensor(lam, device=P.dev)

        def op(*a, **kw):
            return hip_ops.sample_tv(*a, qscale=w, weights=lam, **kw)
    else:
        op = hip_ops.sample
    out_dev = torch.empty((n_draws, T, K, D), dtype=torch.float32, device=P.dev) if return_device else None
    out_host = None if return_device else np.empty((n_draws, T, K, D), dtype=np.float32)
    ms = None
    for d0 in range(0, n_draws, group):
        d1 = min(n_draws, d0 + group)
        dr, m = op(P.y, P.var, *P.params, s_dev, d1 - d0, seed=seed, flags=P.flags,
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


def _pixels(draws, mu):
    """(K, n_draws, T, D) centred draws -> (n_draws, T, K, D) with the centring means added back."""
    return np.ascontiguousarray(np.transpose(draws, (1, 2, 0, 3))) + mu.astype(np.float32)[None, None]


def sample_singlecam_irregular(marker_array, keypoint_names: list, s_finals, n_draws: int, *, frame_times=None,
                               process_noise_scale=None, seed: int = 0,
                               avg_mode: Literal['mean', 'median'] = 'median',
                               var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var',
                               memory_budget: int = DEFAULT_MEMORY_BUDGET) -> np.ndarray:
    """Posterior trajectories of smooth_singlecam_irregular's model in PIXEL coordinates, (n_draws, T, K, 2) float32.
    Takes exactly one of frame_times (T,) and process_noise_scale (T,) or (K, T), as that driver does; over many
    draws the mean approaches its ms and the variance its Vs."""
    from .irregular import process_noise_scale_from_times
    if (frame_times is None) == (process_noise_scale is None):
        raise ValueError('give exactly one of frame_times and process_noise_scale')
    if frame_times is not None:
        T = marker_array.shape[2]
        if np.shape(frame_times) != (T,):
            raise ValueError(f'frame_times must be {(T,)}; got {np.shape(frame_times)}')
        process_noise_scale = process_noise_scale_from_times(frame_times)
    model, _, mu = singlecam_problem('sample_singlecam_irregular', marker_array, keypoint_names, avg_mode, var_mode)
    return _pixels(sample_kalman_posterior(*model, s_finals, n_draws, seed=seed, memory_budget=memory_budget,
                                           qscale=process_noise_scale), mu)


def sample_singlecam_heavy_tailed(marker_array, keypoint_names: list, s, n_draws: int, *, nu_obs: float = 4.0,
                                  nu_proc: float = 4.0, n_iters: int = 12, tol=None, max_iters: int = 64, seed: int = 0,
                                  avg_mode: Literal['mean', 'median'] = 'median',
                                  var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var',
                                  memory_budget: int = DEFAULT_MEMORY_BUDGET, return_smoothed: bool = False):
    """Posterior trajectories of the single-camera smoother under Student-t noise in PIXEL coordinates,
    (n_draws, T, K, 2) float32: runs smooth_heavy_tailed (both nu finite), smooth_robust (nu_proc = math.inf) or
    smooth_jumps (nu_obs = math.inf) and samples the Gaussian factor q(x) of its posterior under the planes that call
    returns.  The draws carry the uncertainty of x GIVEN the planes, not that of lam and u themselves.
    return_smoothed: also that call's dict(ms (T, K, 2) in pixels, Vs (T, K, 2), weights / scales where the model
    has them)."""
    import math
    from .heavy_tails import smooth_heavy_tailed
    from .jumps import smooth_jumps
    from .robust import smooth_robust
    if nu_obs == math.inf and nu_proc == math.inf:
        raise ValueError('both nu infinite is the Gaussian model: use sample_singlecam')
    model, _, mu = singlecam_problem('sample_singlecam_heavy_tailed', marker_array, keypoint_names, avg_mode, var_mode)
    kw = dict(n_iters=n_iters, tol=tol, max_iters=max_iters, vs_diag=True)
    weights = scales = None
    if nu_proc == math.inf:
        ms, Vs, weights, _ = smooth_robust(*model, s, nu=nu_obs, **kw)
    elif nu_obs == math.inf:
        ms, Vs, scales, _ = smooth_jumps(*model, s, nu=nu_proc, **kw)
    else:
        ms, Vs, weights, scales, _ = smooth_heavy_tailed(*model, s, nu_obs=nu_obs, nu_proc=nu_proc, **kw)
    draws = _pixels(sample_kalman_posterior(*model, s, n_draws, seed=seed, memory_budget=memory_budget, qscale=scales,
                                            weights=weights), mu)
    if not return_smoothed:
        return draws
    out = dict(ms=np.ascontiguousarray(np.swapaxes(ms, 0, 1)) + mu.astype(np.float32)[None],
               Vs=np.ascontiguousarray(np.swapaxes(Vs, 0, 1)))
    if weights is not None:
        out['weights'] = np.ascontiguousarray(np.swapaxes(weights, 0, 1))
    if scales is not None:
        out['scales'] = np.ascontiguousarray(np.swapaxes(scales, 0, 1))
    return draws, out


def sample_multicam_robust(marker_array, keypoint_names: list, camera_names: list, s_finals, n_draws: int, *,
                           n_latent: int = 3, quantile_keep_pca: float = 50.0, avg_mode: Literal['mean', 'median'],
                           var_mode: Literal['var', 'confidence_weighted_var'], pca_object=None, nu: float = 4.0,
                           n_iters: int = 8, tol=None, max_iters: int = 64, seed: int = 0,
                           memory_budget: int = DEFAULT_MEMORY_BUDGET, return_latent: bool = False):
    """Posterior trajectories of smooth_multicam_robust's model, reprojected into every view in PIXEL coordinates:
    (n_draws, T, K, 2V) float32, the coordinates of a view adjacent as in that driver's `reprojected`.  Runs
    smooth_robust_grouped (one weight per view) and samples under its weights - the general-model path, where a draw
    costs a smoothing pass.  return_latent: also the latent draws (n_draws, T, K, n_latent)."""
    from .robust import multicam_problem, smooth_robust_grouped
    model, mu = multicam_problem(marker_array, keypoint_names, camera_names, quantile_keep_pca, avg_mode, var_mode,
                                 pca_object, n_latent)
    _, _, weights, _ = smooth_robust_grouped(*model, s_finals, group=2, nu=nu, n_iters=n_iters, tol=tol,
                                             max_iters=max_iters, vs_diag=True)
    lat = sample_kalman_posterior(*model, s_finals, n_draws, seed=seed, memory_budget=memory_budget, weights=weights)
    lat = np.ascontiguousarray(np.transpose(lat, (1, 2, 0, 3)))                    # (n_draws, T, K, D)
    pix = (np.einsum('kod,ntkd->ntko', model[4], lat.astype(np.float64)) + mu[None, None]).astype(np.float32)
    return (pix, lat) if return_latent else pix


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
