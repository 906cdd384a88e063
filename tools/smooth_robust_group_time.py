"""eks_smooth_robust_group (group = 2) beside eks_smooth_robust, same build, same process, 8 passes, warm:

    scalar chains   100 000 frames x 256 keypoints, D = 2, unit A and C, VS_DIAG
    general models   50 000 frames x 4 keypoints, D = 3, O = 4

    python tools/smooth_robust_group_time.py [--regions 5] [--reps 4] [--nu 4] [--out FILE]

2 % of the (frame, keypoint)s are displaced in all coordinates, so that the weights move.  Five alternating regions of
`reps` calls each between device events; prints one JSON line: per shape the median milliseconds per call of the two
and their range, the measured ratio, the ratio expected from the [T][N] planes a call moves (scalar chains; below), and
the per-launch split of one profiled call of each (eks_profile_enable).

Planes moved on scalar chains, in units of one [T][N] float plane, g = 2 (the weight plane is half a plane):
    per coordinate   first pass 2 + 3, middle pass 3 + 4, last pass 3 + 5                       8 passes: 55
    grouped          first 2 + 3 + 1.5, middle 2.5 + 3.5 + 2 (summarize, replay, combine), last 2.5 + 4.5   8 passes: 61.5
On a shared box run it under a time limit of its own:

    timeout -k 10 300 python tools/smooth_robust_group_time.py --out profiles/smooth_robust_group_time.json"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--reps', type=int, default=4)
    ap.add_argument('--nu', type=float, default=4.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from eks_amd import _lib, hip_ops
    dev = hip_ops.require_gpu()
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    gen = torch.Generator(device=dev).manual_seed(0)
    G, N_ITERS = 2, 8

    def split_of(fn):
        lib.eks_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(16384)
        ms = (ctypes.c_float * 256)()
        n = lib.eks_profile_drain(names, 16384, ms, 256)
        lib.eks_profile_enable(0)
        out = {}
        for name, v in zip([x.decode() for x in names.raw.split(b'\0')[:n]], [float(ms[i]) for i in range(n)]):
            out.setdefault(name, []).append(round(v, 4))
        return {k: dict(launches=len(v), median_ms=round(float(np.median(v)), 4), total_ms=round(float(np.sum(v)), 4))
                for k, v in out.items()}

    def measure(T, K, D, O, flags, eye_c):
        x = torch.cumsum(torch.randn((T, K, D), device=dev, generator=gen), dim=0)
        y = x if eye_c else torch.einsum('od,tkd->tko', torch.randn((O, D), device=dev, generator=gen), x)
        hit = (torch.rand((T, K, 1), device=dev, generator=gen) < 0.02).expand(T, K, O)
        jump = (torch.rand((T, K, O), device=dev, generator=gen) * 5.0 + 3.0) * torch.sign(
            torch.randn((T, K, O), device=dev, generator=gen))
        var = (torch.exp(torch.randn((T, K, O), device=dev, generator=gen)) + 0.02).contiguous()
        y = (y + torch.randn((T, K, O), device=dev, generator=gen) * var.sqrt() + hit * jump).contiguous()
        eye = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous()
        C = eye if eye_c else torch.randn((K, O, D), dtype=torch.float64, device=dev, generator=gen).contiguous()
        A = eye if eye_c else (eye * 0.95).contiguous()
        m0 = torch.zeros((K, D), dtype=torch.float64, device=dev)
        S0 = (eye * 4.0).contiguous()
        s = torch.full((K,), 2.0, dtype=torch.float64, device=dev)
        dims = _lib.EksDims(K, T, D, O, flags | _lib.FLAG_VS_DIAG)
        model = (p(m0), p(S0), p(A), p(C), p(eye))
        ms, Vs = (torch.empty((T, K, D), dtype=torch.float32, device=dev) for _ in range(2))
        lam_r = torch.empty((T, K, O), dtype=torch.float32, device=dev)
        lam_g = torch.empty((T, K, O // G), dtype=torch.float32, device=dev)
        change = torch.empty((K,), dtype=torch.float32, device=dev)
        ws_r = torch.empty(max(int(lib.eks_smooth_robust_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8,
                           device=dev)
        ws_g = torch.empty(max(int(lib.eks_smooth_robust_group_workspace_bytes(ctypes.byref(dims), G)), 256),
                           dtype=torch.uint8, device=dev)
        keep = (y, var, eye, C, A, m0, S0, s, ms, Vs, lam_r, lam_g, change, ws_r, ws_g)

        def robust():
            _lib.check(lib.eks_smooth_robust(ctypes.byref(dims), p(y), p(var), *model, p(s), a.nu, N_ITERS, p(lam_r), 0,
                                             p(change), p(ms), p(Vs), p(ws_r), ws_r.numel(), hip_ops._stream()),
                       'eks_smooth_robust')

        def grouped():
            _lib.check(lib.eks_smooth_robust_group(ctypes.byref(dims), p(y), p(var), *model, p(s), a.nu, G, N_ITERS,
                                                   p(lam_g), 0, p(change), p(ms), p(Vs), p(ws_g), ws_g.numel(),
                                                   hip_ops._stream()), 'eks_smooth_robust_group')

        def region(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.reps

        fns = (robust, grouped)
        for _ in range(2):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        marked = float((lam_g[hit[:, :, :1].expand(T, K, O // G)] <= 0.3).float().mean().item())
        times = [[] for _ in fns]
        for _ in range(a.regions):                    # alternating: both see the same neighbours on the box
            for t, fn in zip(times, fns):
                t.append(region(fn))
        med = [float(np.median(t)) for t in times]
        rng = lambda t: [round(min(t), 4), round(max(t), 4)]
        out = dict(frames=T, keypoints=K, D=D, O=O, group=G, n_iters=N_ITERS,
                   robust_ms=round(med[0], 4), robust_ms_min_max=rng(times[0]),
                   grouped_ms=round(med[1], 4), grouped_ms_min_max=rng(times[1]),
                   grouped_over_robust=round(med[1] / med[0], 3), displaced_marked=round(marked, 4),
                   robust_launches=split_of(robust), grouped_launches=split_of(grouped))
        del keep
        return out

    res = dict(tool='smooth_robust_group_time', regions=a.regions, reps=a.reps, nu=a.nu)
    res['scalar_chains'] = measure(100000, 256, 2, 2, _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC, True)
    res['scalar_chains']['expected_from_planes_moved'] = round(61.5 / 55.0, 3)
    res['general'] = measure(50000, 4, 3, 4, 0, False)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
