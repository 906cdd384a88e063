"""eks_smooth_heavy (12 passes) against 12 passes of eks_smooth_robust plus 12 of eks_smooth_jumps from the same build,
in the same process, alternating, on the two shapes of tools/smooth_jumps_time.py:

    scalar   100 000 frames x 256 keypoints, D = 2, diagonal, unit A and C, VS_DIAG (the C3 shape)
    general  50 000 frames x 4 keypoints, D = 3, O = 4, full matrices (the generic float64 kernels)

    python tools/smooth_heavy_time.py [--reps 5] [--passes 12] [--nu 4] [--skip-general] [--out FILE]

About 1 % of the (frame, keypoint) pairs carry a jump of 20 .. 60 px in all coordinates and another 1 % a displaced
observation of 20 .. 60 px, so that both planes move.  The sum of the two single-sided calls is what a user must
otherwise spend, on a different model; by planes moved a middle pass is about 9 (y, var, lam, w read in summarize and
replay, lam and the contributions written) against 7 + 6, so the expected ratio is near 0.7.  Prints one JSON line per
shape: the median of `reps` timed regions (device events, warm) of one eks_smooth_heavy call, of one eks_smooth_robust
call and of one eks_smooth_jumps call, the ratio heavy / (robust + jumps), the largest scale, the smallest weight and
the last changes, and the per-kernel split of one profiled call of each (eks_profile_enable).  On a shared box run it
under a time limit of its own:

    timeout -k 10 300 python tools/smooth_heavy_time.py --out profiles/smooth_heavy_time.json"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scalar_problem(torch, dev, _lib):
    T, K, D = 100000, 256, 2
    g = torch.Generator(device=dev).manual_seed(0)
    step = torch.randn((T, K, D), device=dev, generator=g) * 0.22
    hit = (torch.rand((T, K, 1), device=dev, generator=g) < 0.01).expand(T, K, D)
    size = (torch.rand((T, K, D), device=dev, generator=g) * 40.0 + 20.0) * torch.sign(
        torch.randn((T, K, D), device=dev, generator=g))
    x = torch.cumsum(step + hit * size, dim=0)
    var = (torch.rand((T, K, D), device=dev, generator=g) * 1.5 + 0.5).contiguous()
    bad = (torch.rand((T, K, 1), device=dev, generator=g) < 0.01).expand(T, K, D)
    off = (torch.rand((T, K, D), device=dev, generator=g) * 40.0 + 20.0) * torch.sign(
        torch.randn((T, K, D), device=dev, generator=g))
    y = (x + torch.randn((T, K, D), device=dev, generator=g) * var.sqrt() + bad * off).contiguous()
    eye = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous()
    par = (torch.zeros((K, D), dtype=torch.float64, device=dev), eye * 4.0, eye, eye, eye,
           torch.full((K,), 0.05, dtype=torch.float64, device=dev))
    return 'scalar', (T, K, D, D), _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC | _lib.FLAG_VS_DIAG, y, var, par, (T, K, D)


def general_problem(torch, dev, _lib):
    T, K, D, O = 50000, 4, 3, 4
    rng = np.random.default_rng(0)
    A = 0.95 * np.eye(D) + 0.02 * rng.normal(size=(K, D, D))
    C = rng.normal(size=(K, O, D))
    Q = np.tile(np.eye(D), (K, 1, 1)) + 0.1
    s = np.full(K, 0.05)
    x = np.zeros((K, D))
    xs = np.empty((T, K, D))
    steps = rng.normal(size=(T, K, D)) * np.sqrt(0.05)
    hit = rng.random((T, K)) < 0.01
    steps[hit] += rng.choice([-1.0, 1.0], (int(hit.sum()), D)) * rng.uniform(20.0, 60.0, (int(hit.sum()), D)) / 3.0
    for t in range(T):
        x = np.einsum('kij,kj->ki', A, x) + steps[t]
        xs[t] = x
    var = rng.uniform(0.5, 2.0, (T, K, O)).astype(np.float32)
    y = np.einsum('koj,tkj->tko', C, xs) + rng.normal(size=(T, K, O)) * np.sqrt(var)
    bad = rng.random((T, K)) < 0.01
    y[bad] += rng.choice([-1.0, 1.0], (int(bad.sum()), O)) * rng.uniform(20.0, 60.0, (int(bad.sum()), O))
    y = y.astype(np.float32)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    par = (d(np.zeros((K, D))), d(np.tile(4.0 * np.eye(D), (K, 1, 1))), d(A), d(C), d(Q), d(s))
    return 'general', (T, K, D, O), 0, d(y), d(var), par, (T, K, D, D)


def measure(a, torch, dev, _lib, hip_ops, lib, problem):
    name, (T, K, D, O), flags, y, var, par, vs_shape = problem
    dims = _lib.EksDims(K, T, D, O, flags)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    model = tuple(p(t) for t in par)
    ms = torch.empty((T, K, D), dtype=torch.float32, device=dev)
    Vs = torch.empty(vs_shape, dtype=torch.float32, device=dev)
    weights, weights_r = (torch.empty((T, K, O), dtype=torch.float32, device=dev) for _ in range(2))
    scales, scales_j = (torch.empty((T, K), dtype=torch.float32, device=dev) for _ in range(2))
    change = torch.empty((2, K), dtype=torch.float32, device=dev)
    change_1 = torch.empty((K,), dtype=torch.float32, device=dev)
    space = lambda q: torch.empty(max(int(q(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)  # noqa: E731
    ws_h, ws_r, ws_j = (space(getattr(lib, f'eks_smooth_{e}_workspace_bytes')) for e in ('heavy', 'robust', 'jumps'))
    h_args = (ctypes.byref(dims), p(y), p(var), *model, a.nu, a.nu, a.passes, p(weights), p(scales), 0, p(change), p(ms),
              p(Vs), p(ws_h), ws_h.numel())
    r_args = (ctypes.byref(dims), p(y), p(var), *model, a.nu, a.passes, p(weights_r), 0, p(change_1), p(ms), p(Vs),
              p(ws_r), ws_r.numel())
    j_args = (ctypes.byref(dims), p(y), p(var), *model, a.nu, a.passes, p(scales_j), 0, p(change_1), p(ms), p(Vs),
              p(ws_j), ws_j.numel())

    def heavy():
        _lib.check(lib.eks_smooth_heavy(*h_args, hip_ops._stream()), 'eks_smooth_heavy')

    def robust():
        _lib.check(lib.eks_smooth_robust(*r_args, hip_ops._stream()), 'eks_smooth_robust')

    def jumps():
        _lib.check(lib.eks_smooth_jumps(*j_args, hip_ops._stream()), 'eks_smooth_jumps')

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    fns = (heavy, robust, jumps)
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(a.reps):                       # alternating: all see the same neighbours on the box
        for t, fn in zip(times, fns):
            t.append(timed(fn))
    heavy()                                       # the planes and changes reported below are its own
    torch.cuda.synchronize()
    stats = dict(largest_scale=float(scales.max().item()), median_scale=float(scales.median().item()),
                 smallest_weight=float(weights.min().item()), median_weight=float(weights.median().item()),
                 last_change_max=[float(v) for v in change.max(dim=1).values.tolist()])

    def split_of(fn):
        lib.eks_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(16384)
        ms = (ctypes.c_float * 256)()
        n = lib.eks_profile_drain(names, 16384, ms, 256)
        lib.eks_profile_enable(0)
        out = {}
        for nm, v in zip([x.decode() for x in names.raw.split(b'\0')[:n]], [float(ms[i]) for i in range(n)]):
            out.setdefault(nm, []).append(v)
        return {nm: dict(launches=len(v), median_ms=round(float(np.median(v)), 4), total_ms=round(float(np.sum(v)), 4))
                for nm, v in out.items()}

    splits = [split_of(fn) for fn in fns]
    med = [float(np.median(t)) for t in times]
    rng = lambda t: [round(min(t), 4), round(max(t), 4)]  # noqa: E731
    return dict(tool='smooth_heavy_time', shape=name, frames=T, keypoints=K, state_dim=D, obs_dim=O, passes=a.passes,
                reps=a.reps, nu=a.nu, heavy_ms=round(med[0], 4), heavy_ms_min_max=rng(times[0]),
                robust_ms=round(med[1], 4), robust_ms_min_max=rng(times[1]), jumps_ms=round(med[2], 4),
                jumps_ms_min_max=rng(times[2]), heavy_over_robust_plus_jumps=round(med[0] / (med[1] + med[2]), 3),
                **stats, heavy_kernels=splits[0], robust_kernels=splits[1], jumps_kernels=splits[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--passes', type=int, default=12)
    ap.add_argument('--nu', type=float, default=4.0)
    ap.add_argument('--skip-general', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from eks_amd import _lib, hip_ops
    dev = hip_ops.require_gpu()
    lib = _lib.load()
    lines = []
    for make in (scalar_problem,) + (() if a.skip_general else (general_problem,)):
        res = measure(a, torch, dev, _lib, hip_ops, lib, make(torch, dev, _lib))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
