"""User-supplied differentiable emission functions for the extended smoother.

The reference's `run_kalman_smoother(h_fn=...)` takes any observation function y_t = h_fn(x_t)
(eks/core.py:159-177, :188-190) and differentiates it with jax.  Here a HIP kernel cannot call a
Python function, so the function is evaluated by torch, in float64 and for every (chain, frame)
point of a sweep in one batched call, and the kernels consume the resulting linearisation tables
(include/eks_hip.h, eks_ekf_affine_sweep).

    h = DifferentiableEmission(fn)                        # fn: (D,) -> (O,), torch ops
    h = DifferentiableEmission(fn, jacobian=jac)          # jac: (D,) -> (O, D), replaces autodiff
    h = DifferentiableEmission(fn_n, batched=True)        # fn_n: (N, D) -> (N, O)
    run_kalman_smoother(..., h_fn=h)

Values come from torch.func.vmap(fn), Jacobians from torch.func.vmap(torch.func.jacfwd(fn)) (one
forward-mode pass gives both).  A batched fn without `jacobian` is differentiated by D forward-mode
products (torch.func.jvp), one per state coordinate.
"""
from __future__ import annotations

from typing import Callable

# Points per call of the user's function: one call evaluates fn and its Jacobian at this many states at
# most.  The forward-mode intermediates of jacfwd scale like D times fn's own; the estimate below charges
# 8 bytes x 4 x (D + O (D + 1)) per point, and a batch stays under _EVAL_BUDGET_BYTES.
_EVAL_BUDGET_BYTES = 256 << 20


def eval_batch_points(D: int, O: int, budget: int | None = None) -> int:
    """How many points one evaluation of fn and its Jacobian takes under the budget."""
    per_point = 8 * 4 * (D + O * (D + 1))
    return max(1, int((budget or _EVAL_BUDGET_BYTES) // per_point))


class DifferentiableEmission:
    """Wraps an emission function written in torch for run_kalman_smoother(h_fn=...) and
    optimize_smooth_param(h_fn_combined=...).

    fn        maps ONE state, a float64 tensor (D,), to (O,) (or, with batched=True, (N, D) -> (N, O)).
    jacobian  optional (D,) -> (O, D) (batched: (N, D) -> (N, O, D)); replaces autodiff.
    batched   fn (and jacobian) already take a leading batch axis.
    max_sweeps, lin_tol: the extended filter is solved as a fixed point over the linearisation points; a
              solve stops once no point moves by more than lin_tol (relative to max(1, |x|)) and warns when
              max_sweeps sweeps did not get there.
    """

    def __init__(self, fn: Callable, *, jacobian: Callable | None = None, batched: bool = False,
                 max_sweeps: int = 32, lin_tol: float = 1e-10):
        if not callable(fn):
            raise TypeError('fn must be callable')
        if jacobian is not None and not callable(jacobian):
            raise TypeError('jacobian must be callable or None')
        if int(max_sweeps) < 1:
            raise ValueError('max_sweeps must be at least 1')
        self.fn = fn
        self.jacobian = jacobian
        self.batched = bool(batched)
        self.max_sweeps = int(max_sweeps)
        self.lin_tol = float(lin_tol)

    def __repr__(self):
        return (f'DifferentiableEmission({getattr(self.fn, "__name__", "fn")}, '
                f'jacobian={"given" if self.jacobian is not None else "autodiff"}, batched={self.batched})')

    def __call__(self, x):
        """h(x) for one state (D,) or a batch (N, D) (torch tensors)."""
        if x.dim() == 1:
            return self.fn(x[None])[0] if self.batched else self.fn(x)
        return self.values(x)

    def values(self, x):
        """h at every row of x (N, D) -> (N, O)."""
        if self.batched:
            return self.fn(x)
        from torch.func import vmap
        return vmap(self.fn)(x)

    def values_and_jacobians(self, x):
        """(h(x) (N, O), dh/dx (N, O, D)) at every row of x (N, D), float64."""
        import torch
        from torch.func import jacfwd, jvp, vmap
        if self.jacobian is not None:
            if self.batched:
                return self.fn(x), self.jacobian(x)
            return vmap(self.fn)(x), vmap(self.jacobian)(x)
        if not self.batched:
            J, h = vmap(jacfwd(lambda v: (lambda o: (o, o))(self.fn(v)), has_aux=True))(x)
            return h, J
        D = x.shape[-1]
        cols, h = [], None
        for i in range(D):
            e = torch.zeros_like(x)
            e[:, i] = 1.0
            h, col = jvp(self.fn, (x,), (e,))
            cols.append(col)
        return h, torch.stack(cols, dim=-1)
