"""What the feature functions that take the linear-Gaussian model (ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s) share:
its validation, the way onto the device and back, the single-camera set-up, and the continuation loop of the two
iterated smoothers.  Private: posterior, irregular, robust, jumps, heavy_tails, em, diagnostics and the single-camera
driver use it.
torch and eks_amd.core are imported where a device is first needed, so every check here raises without one."""
from __future__ import annotations

import numpy as np

from . import hip_ops


def _validate(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s_finals):
    """Shapes of run_kalman_smoother's arguments -> (K, T, O, D, s as a contiguous float64 (K,))."""
    shp = tuple(np.shape(ys))
    if len(shp) != 3:
        raise ValueError(f'ys must be (K,T,O); got {shp}')
    K, T, O = shp
    if len(np.shape(m0s)) != 2 or np.shape(m0s)[0] != K:
        raise ValueError(f'm0s must be (K,D); got {tuple(np.shape(m0s))}')
    D = np.shape(m0s)[1]
    for name, a, want in (('S0s', S0s, (K, D, D)), ('As', As, (K, D, D)), ('Cs', Cs, (K, O, D)), ('Qs', Qs, (K, D, D)),
                          ('ensemble_vars', ensemble_vars, (T, K, O))):
        if tuple(np.shape(a)) != want:
            raise ValueError(f'{name} must be {want}; got {tuple(np.shape(a))}')
    s = np.broadcast_to(np.asarray(s_finals, dtype=np.float64), (K,)) if np.ndim(s_finals) == 0 \
        else np.asarray(s_finals, dtype=np.float64)
    if s.shape != (K,):
        raise ValueError(f's_finals must be a scalar or (K,); got {s.shape}')
    return K, T, O, D, np.ascontiguousarray(s)


def _host_flags(S0s, As, Cs, Qs) -> int:
    from .core import _to_numpy
    return hip_ops.model_flags(*(np.ascontiguousarray(_to_numpy(a, np.float64)) for a in (S0s, As, Cs, Qs)))


class linear_problem:
    """The host half of a model-taking call: refuses h_fn models in the name of `what`, validates the shapes and
    decides the model's flags - K, T, O, D, s (float64 (K,)) and flags are attributes, for the caller's own checks.
    Nothing here asks for a device; upload() is the step that does."""

    def __init__(self, what, ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s, h_fn=None):
        if h_fn is not None:
            raise NotImplementedError(f'{what} covers linear models; h_fn models are not supported')
        self.K, self.T, self.O, self.D, self.s = _validate(ys, m0s, S0s, As, Cs, Qs, ensemble_vars, s)
        self.flags = _host_flags(S0s, As, Cs, Qs)
        self._arrays = (ys, m0s, S0s, As, Cs, Qs, ensemble_vars)

    def upload(self):
        """-> (the _DeviceProblem, s on its device)."""
        from .core import _DeviceProblem, _torch
        P = _DeviceProblem(*self._arrays, flags=self.flags)
        return P, _torch().as_tensor(self.s, device=P.dev)


def to_caller(return_device: bool, frame_major, plain=()):
    """The kernels' device tensors as the caller gets them: every (T, K, ...) one of `frame_major` as a (K, T, ...)
    view, those of `plain` as they are; NumPy arrays through one staged copy unless return_device."""
    if return_device:
        return tuple(a.transpose(0, 1) for a in frame_major) + tuple(plain)
    from .core import _to_host
    host = _to_host(*frame_major, *plain)
    return tuple(np.swapaxes(a, 0, 1) for a in host[:len(frame_major)]) + host[len(frame_major):]


def singlecam_problem(name, marker_array, keypoint_names, avg_mode, var_mode):
    """The single-camera driver's set-up: ensemble -> centring -> prior.  Returns (model, stats, mu): model =
    (ys (K,T,2), m0s, S0s, As, Cs, Qs, ensemble_vars (T,K,2)) as run_kalman_smoother takes them, stats (T,K,5) the
    ensemble's x, y, var_x, var_y, likelihood, mu (K,2) float64 the centring means the driver adds back.  `name`: the
    function to refuse a multi-view array or a wrong count of names for (None: the driver, which checks neither)."""
    from .core import ensemble
    from .singlecam_smoother import initialize_kalman_filter
    from .utils import center_predictions
    M, V, T, K, _ = marker_array.shape
    if name is not None:
        if V != 1:
            raise ValueError(f'{name} takes a single-view marker array')
        if len(keypoint_names) != K:
            raise ValueError(f'{len(keypoint_names)} keypoint names for {K} keypoints')
    ens = ensemble(marker_array, avg_mode=avg_mode, var_mode=var_mode)       # (1,1,T,K,5) float32
    _, centered, _, means = center_predictions(ens, quantile_keep_pca=100)
    stats = np.asarray(ens.array)[0, 0]                                       # (T,K,5)
    cen = np.asarray(centered.array)[0, 0]                                    # (T,K,2)
    m0s, S0s, As, Qs, Cs = initialize_kalman_filter(centered)
    return (np.swapaxes(cen, 0, 1), m0s, S0s, As, Cs, Qs, stats[:, :, 2:4]), stats, np.asarray(means.array)[0, 0, 0]


def check_iteration_counts(nu, n_iters, tol, max_iters):
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


def iterated_smooth(what, op, plane_name, model, s_finals, nu, n_iters, tol, max_iters, vs_diag, return_device, h_fn):
    """smooth_robust and smooth_jumps: `op` is the hip_ops wrapper, `plane_name` its weights / scales argument.
    -> (ms, Vs, plane, change) as the caller gets them."""
    L = linear_problem(what, *model, s_finals, h_fn)
    nu, n_iters = check_iteration_counts(nu, n_iters, tol, max_iters)
    P, s_dev = L.upload()

    def run(n, plane=None):
        return op(P.y, P.var, *P.params, s_dev, nu=nu, n_iters=n, flags=P.flags, vs_diag=vs_diag,
                  **{plane_name: plane, plane_name + '_in': plane is not None})

    ms, Vs, plane, change = run(n_iters)
    if tol is not None:
        # a continued block's first pass smooths again under the plane the previous block ended on, so a block of n
        # passes adds n - 1 to `done`: the n_iters of the single call that gives the same bits
        done = n_iters
        while float(change.max()) >= tol and done < max_iters:
            n = min(n_iters, int(max_iters) - done + 1)
            ms, Vs, plane, change = run(n, plane)
            done += n - 1
    return to_caller(return_device, (ms, Vs, plane), (change,))
