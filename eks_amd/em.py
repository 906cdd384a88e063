"""EM on the model the smoother runs.

Every driver picks the smoothing parameter s by minimising the filter's negative log-likelihood with a CONSTANT
observation noise (the time-median of the ensemble variances), as the reference does, and then smooths with the
time-varying R_t = diag(ensemble_var_t).  The functions here fit s - or the whole process-noise covariance Q - to the
model `eks_smooth` actually runs.  The reference has no counterpart.

    process_noise_statistics(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s) -> (Sw, n)
    refine_smooth_param_em(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_init, ...) -> s_finals (K,)
    fit_process_noise_em(ys, m0s, S0s, As, Cs, Qs_init, ensemble_vars, ...) -> Qs (K, D, D)

E-step: Sw = sum_t E[w_t w_t' | y], the smoothed second moment of the process noise w_t = x_{t+1} - A x_t, one
smoothing pass (eks_em_stats).  M-step for the scale, Q fixed: s_new = tr(Q^-1 Sw) / n with n = D (T - 1); for a full
Q (s = 1): Q_new = sym(Sw) / (T - 1).  Fisher's identity: d loglik / d log s = (tr(Q^-1 Sw) / s - n) / 2."""
from __future__ import annotations

import numpy as np

from . import hip_ops
from ._problem import linear_problem

__all__ = ['process_noise_statistics', 'refine_smooth_param_em', 'fit_process_noise_em']

EM_STRIDE = 8      # iterations enqueued between two reads of the count of blocks still running


def _problem(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s, h_fn, what):
    L = linear_problem(what, ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s, h_fn)
    if not np.all(np.isfinite(L.s)) or np.any(L.s <= 0):
        raise ValueError('the smoothing parameters must be positive and finite')
    return L


def process_noise_statistics(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s, *, return_device: bool = False, h_fn=None):
    """The E-step statistic of the model run_kalman_smoother smooths with, at the smoothing parameters s (scalar or
    (K,)): returns (Sw, n) with Sw (K, D, D) float64 = sum_{t < T-1} E[w_t w_t' | y], w_t = x_{t+1} - A x_t, and
    n = D (T - 1).  Arguments as sample_kalman_posterior.  tr(Q^-1 Sw) / (s n) is 1 at a stationary point of the
    time-varying-R likelihood in s, and (tr(Q^-1 Sw) / s - n) / 2 is that likelihood's derivative in log s.  On
    diagonal models (S0, A, C, Q all diagonal) only the diagonal is computed and the off-diagonal entries are returned
    as zeros: they are sums of products of the coordinates' means, which tr(Q^-1 Sw) with a diagonal Q never reads.
    One smoothing pass; T = 1 gives zeros."""
    L = _problem(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s, h_fn, 'process_noise_statistics')
    from . import _lib
    from .core import _torch
    P, s_dev = L.upload()
    diag_model = bool(P.flags & _lib.FLAG_DIAG_MODEL)
    Sw = hip_ops.em_stats(P.y, P.var, *P.params, s_dev, flags=P.flags, vs_diag=diag_model)
    if diag_model:
        Sw = _torch().diag_embed(Sw)
    return (Sw if return_device else Sw.cpu().numpy()), L.D * (L.T - 1)


def refine_smooth_param_em(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_init, *, blocks: list | None = None,
                           max_iters: int = 100, tol: float = 1e-4, s_bounds_log=(-8.0, 8.0),
                           return_info: bool = False, h_fn=None):
    """Refine smoothing parameters by EM on the model `eks_smooth` runs: this MAXIMISES THE LIKELIHOOD OF THE
    TIME-VARYING-R MODEL (R_t = diag(ensemble_var_t), what run_kalman_smoother smooths with), not of the constant-R
    model its search minimises.  Each iteration is one smoothing pass and one closed-form update
    s <- tr(Q^-1 Sw) / (D (T - 1)) and CANNOT DECREASE that likelihood.

    EM IS SLOW FROM A DISTANT START (hundreds of iterations when the optimum is orders of magnitude below it): start
    from the s run_kalman_smoother returned, which is close, and mind the iteration cap.

    s_init: scalar or (K,).  blocks: lists of keypoints sharing one s, as run_kalman_smoother's (empty: every keypoint
    its own; a block starts from the geometric mean of its members' s_init); a block's update pools its members'
    numerators and denominators.  A block stops when |delta log s| < tol or after max_iters iterations; log s is kept
    inside s_bounds_log.  Returns s_finals (K,) float64; with return_info also a dict of per-block arrays
    `iterations`, `last_delta_log_s`, `done`.  General models need a well-conditioned positive definite Q."""
    L = _problem(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_init, h_fn, 'refine_smooth_param_em')
    K, T, s, flags = L.K, L.T, L.s, L.flags
    if T < 2:
        raise ValueError('EM for the scale needs at least two frames')
    if int(max_iters) != max_iters or max_iters < 0:
        raise ValueError('max_iters must be an integer >= 0')
    lo, hi = (float(v) for v in s_bounds_log)
    if not lo < hi:
        raise ValueError('s_bounds_log must be (lo, hi) with lo < hi')
    from . import _lib
    from .core import _block_csr, _torch
    offs, members, of_kp = _block_csr(blocks if blocks else None, K)
    if not (flags & _lib.FLAG_DIAG_MODEL) and not (flags & _lib.FLAG_Q_PD):
        raise ValueError('refine_smooth_param_em needs a positive definite Q with cond(Q) <= 1e6 on general models')
    nb = len(offs) - 1
    log_s = np.array([np.log(s[members[offs[b]:offs[b + 1]]]).mean() for b in range(nb)])
    state = np.zeros((nb, 4))
    state[:, 0] = log_s
    torch = _torch()
    P, _ = L.upload()
    loop = hip_ops.EmScaleLoop(P.y, P.var, *P.params, torch.as_tensor(offs, device=P.dev),
                               torch.as_tensor(members, device=P.dev), torch.as_tensor(state, device=P.dev),
                               torch.as_tensor(np.exp(log_s)[of_kp], device=P.dev), lo, hi, tol, int(max_iters),
                               flags=P.flags)
    done = 0
    while done < max_iters:
        n = min(EM_STRIDE, int(max_iters) - done)
        loop.run(n)
        done += n
        if int(loop.n_active.item()) == 0:
            break
    s_out = loop.s_keypoint.cpu().numpy()
    if not return_info:
        return s_out
    st = loop.state.cpu().numpy()
    return s_out, dict(iterations=st[:, 2].astype(np.int64), last_delta_log_s=st[:, 1], done=st[:, 3] != 0)


def fit_process_noise_em(ys, m0s, S0s, As, Cs, Qs_init, ensemble_vars, *, max_iters: int = 50, tol: float = 1e-4,
                         h_fn=None):
    """EM for the whole process-noise covariance of the model `eks_smooth` runs (time-varying R), at s = 1:
    Q <- sym(Sw) / (T - 1), a torch loop around eks_em_stats, one smoothing pass per iteration; no iteration can
    decrease the likelihood.  Stops when every keypoint's relative Frobenius change of Q is below tol, or after
    max_iters iterations.  Diagonal models (S0, A, C, Q all diagonal) keep Q diagonal.  Returns Qs (K, D, D) float64.
    Like every EM it is slow from a distant start."""
    L = _problem(ys, m0s, S0s, As, Cs, Qs_init, ensemble_vars, 1.0, h_fn, 'fit_process_noise_em')
    T = L.T
    if T < 2:
        raise ValueError('EM for Q needs at least two frames')
    from . import _lib
    from .core import _torch
    torch = _torch()
    P, ones = L.upload()
    diag_model = bool(P.flags & _lib.FLAG_DIAG_MODEL)
    Q = P.params[4]
    for _ in range(int(max_iters)):
        Sw = hip_ops.em_stats(P.y, P.var, *P.params, ones, flags=P.flags, vs_diag=diag_model)
        Qn = torch.diag_embed(Sw) if diag_model else 0.5 * (Sw + Sw.transpose(1, 2))
        Qn = Qn / float(T - 1)
        change = (torch.linalg.matrix_norm(Qn - Q) / torch.linalg.matrix_norm(Q)).max()
        Q.copy_(Qn)
        if float(change) < tol:
            break
    return Q.cpu().numpy().copy()
