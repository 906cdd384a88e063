"""The forward filter's view of the model run_kalman_smoother smooths with: one-step-ahead prediction errors
(innovations) and the exact log-likelihood, with the time-varying R = diag(ensemble_var_t).  The reference has no
counterpart: its likelihood (the smoothing-parameter search) holds R constant and its innovations are never returned.

    filter_innovations(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals) -> innov, innov_var, nis, frame_loglik, loglik
    log_likelihood(...)          -> (K,) float64, nothing of length T is written
    innovation_summary(...)      -> per keypoint: mean nis / O, lag-one autocorrelation, fraction beyond 3 sigma
    innovations_singlecam(marker_array, keypoint_names, s_finals) -> z (T, K, 2), nis (T, K), loglik (K,)

Standardised innovations z = innov / sqrt(innov_var) are N(0, 1) and white when the model is right: a smoothing
parameter that is too small shows as mean z^2 far above 1 and a strongly positive lag-one autocorrelation, and frames
whose |z| exceeds 3 are ensemble observations the dynamics do not believe.  log_likelihood is the function
refine_smooth_param_em climbs, and compares two Q or two s on the same data."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Literal

import numpy as np

from . import hip_ops
from ._problem import linear_problem, singlecam_problem, to_caller

__all__ = ['filter_innovations', 'log_likelihood', 'innovation_summary', 'innovations_singlecam', 'FilterInnovations']

FilterInnovations = namedtuple('FilterInnovations', ['innov', 'innov_var', 'nis', 'frame_loglik', 'loglik'])


def _run(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn, what, want):
    """-> (dict of device tensors in the kernels' frame-major layout, diag_model, O)."""
    L = linear_problem(what, ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn)
    from . import _lib
    P, s_dev = L.upload()
    diag_model = bool(P.flags & _lib.FLAG_DIAG_MODEL)
    if diag_model:      # nis and frame_ll are elementwise functions of innov and innov_var there: formed by torch
        want = tuple(w for w in want if w not in ('nis', 'frame_ll'))
    out = hip_ops.innovations(P.y, P.var, *P.params, s_dev, flags=P.flags, want=want)
    return out, diag_model, L.O


def filter_innovations(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, return_device: bool = False,
                       h_fn=None) -> FilterInnovations:
    """The prediction-error decomposition at the smoothing parameters s_finals (scalar or (K,)), in one forward pass.
    Arguments as smooth_increments.  Returns the named tuple
        innov (K, T, O)        y_t - C m_{t|t-1}, from the predicted belief (frame 0: the prior)
        innov_var (K, T, O)    the diagonal of S_t = C P_{t|t-1} C' + R_t
        nis (K, T)             innov' S_t^-1 innov, chi-square with O degrees of freedom when the model is right
        frame_loglik (K, T)    log p(y_t | y_0 .. y_{t-1})
        loglik (K,) float64    their sum, accumulated in float64 on the device
    float32 NumPy arrays (loglik float64), or device tensors with return_device; the arrays of length T are views of
    the kernels' frame-major buffers, like run_kalman_smoother's."""
    out, diag_model, O = _run(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn, 'filter_innovations',
                              hip_ops.INNOVATION_OUTPUTS)
    from .core import _torch
    torch = _torch()
    loglik = out['loglik']
    if diag_model:
        z2 = out['innov'] * out['innov'] / out['innov_var']
        nis = z2.sum(dim=-1)
        frame_ll = -0.5 * ((z2 + torch.log(out['innov_var'])).sum(dim=-1) + O * math.log(2.0 * math.pi))
        loglik = loglik.sum(dim=-1)
    else:
        nis, frame_ll = out['nis'], out['frame_ll']
    res = to_caller(return_device, (out['innov'], out['innov_var'], nis, frame_ll))
    return FilterInnovations(*res, loglik if return_device else loglik.cpu().numpy())


def log_likelihood(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, return_device: bool = False, h_fn=None):
    """log p(y | s, Q) per keypoint, (K,) float64, of the model run_kalman_smoother smooths with (time-varying R): the
    function refine_smooth_param_em cannot decrease.  Arguments as filter_innovations; nothing of length T is
    written."""
    out, diag_model, _ = _run(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, h_fn, 'log_likelihood', ('loglik',))
    ll = out['loglik'].sum(dim=-1) if diag_model else out['loglik']
    return ll if return_device else ll.cpu().numpy()


def innovation_summary(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, *, h_fn=None) -> list:
    """Per keypoint, a dict of the three standard checks on the standardised innovations z = innov / sqrt(innov_var):
        mean_nis_per_dim   mean over frames of nis / O                          (1 when the model is right)
        lag1_autocorr (O,) lag-one autocorrelation of z per coordinate          (0 +- 1 / sqrt(T) when it is right)
        frac_beyond_3      the fraction of |z| > 3 over frames and coordinates  (0.0027 when it is right)
    formed by torch on the device from filter_innovations' outputs."""
    fi = filter_innovations(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals, return_device=True, h_fn=h_fn)
    z = (fi.innov / fi.innov_var.sqrt()).double()                     # (K, T, O)
    O = z.shape[-1]
    zc = z - z.mean(dim=1, keepdim=True)
    den = (zc * zc).sum(dim=1)
    lag1 = (zc[:, 1:] * zc[:, :-1]).sum(dim=1) / den
    mean_nis = fi.nis.double().mean(dim=1) / O
    frac = (z.abs() > 3.0).double().mean(dim=(1, 2))
    mean_nis, lag1, frac = mean_nis.cpu().numpy(), lag1.cpu().numpy(), frac.cpu().numpy()
    return [dict(mean_nis_per_dim=float(mean_nis[k]), lag1_autocorr=lag1[k], frac_beyond_3=float(frac[k]))
            for k in range(z.shape[0])]


def innovations_singlecam(marker_array, keypoint_names: list, s_finals, *,
                          avg_mode: Literal['mean', 'median'] = 'median',
                          var_mode: Literal['var', 'confidence_weighted_var'] = 'confidence_weighted_var') -> dict:
    """Standardised innovations of the single-camera smoother.  Rebuilds the ensemble, the centring and the prior as
    ensemble_kalman_smoother_singlecam does.  Returns a dict:
        z (T, K, 2) float32   innov / sqrt(innov_var) of the x and y coordinate
        nis (T, K) float32    z_x^2 + z_y^2
        loglik (K,) float64   log-likelihood of the keypoint's centred ensemble means
    s_finals: the smoothing parameters the driver returned."""
    model, _, _ = singlecam_problem('innovations_singlecam', marker_array, keypoint_names, avg_mode, var_mode)
    fi = filter_innovations(*model, s_finals)
    z = np.swapaxes(fi.innov / np.sqrt(fi.innov_var), 0, 1)
    return dict(z=np.ascontiguousarray(z), nis=np.ascontiguousarray(np.swapaxes(fi.nis, 0, 1)), loglik=fi.loglik)
