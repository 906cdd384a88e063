"""eks_smooth_robust against eks_smooth_tv on the C3 shape (100 000 frames x 256 keypoints, D = 2, diagonal, unit A
and C, VS_DIAG), in the same process, alternating:

    (a) eks_smooth_tv with a shared w = 1           summarize, three-launch scan, replay that writes ms and Vs
    (b) eks_smooth_robust with n_iters = 1          the same five launches without the w registers; writes the weights
    (c) eks_smooth_robust with n_iters = 8          seven middle passes (read y, var, lam twice; write lam) and (b)'s

    python tools/smooth_robust_time.py [--frames 100000] [--keypoints 256] [--reps 20] [--nu 4] [--out FILE]

2 % of the observations are displaced by +-(20 .. 60) px, so that the weights move.  Prints one JSON line: median
milliseconds and the range of the three (device events), the time of one middle pass ((c) - (b)) / 7, its ratio to (a)
(target 1.25: 7 planes moved against 6, and a margin for the quotients), (b) / (a) (target 1.1), the bits of (b)
against (a), and the per-kernel split of one profiled call of each (eks_profile_enable).  On a shared box run it under
a time limit of its own:

    timeout -k 10 300 python tools/smooth_robust_time.py --out profiles/smooth_robust_time.json"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100000)
    ap.add_argument('--keypoints', type=int, default=256)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--nu', type=float, default=4.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from eks_amd import _lib, hip_ops
    dev = hip_ops.require_gpu()
    lib = _lib.load()
    T, K, D = a.frames, a.keypoints, 2
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.cumsum(torch.randn((T, K, D), device=dev, generator=g), dim=0)
    hit = torch.rand((T, K, D), device=dev, generator=g) < 0.02
    jump = (torch.rand((T, K, D), device=dev, generator=g) * 40.0 + 20.0) * torch.sign(torch.randn((T, K, D), device=dev, generator=g))
    y = (y + hit * jump).contiguous()
    var = (torch.exp(torch.randn((T, K, D), device=dev, generator=g)) + 0.02).contiguous()
    eye = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous()
    m0 = torch.zeros((K, D), dtype=torch.float64, device=dev)
    S0 = eye * 4.0
    s = torch.full((K,), 2.0, dtype=torch.float64, device=dev)
    flags = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    dims = _lib.EksDims(K, T, D, D, flags | _lib.FLAG_VS_DIAG)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    model = (p(m0), p(S0), p(eye), p(eye), p(eye))
    ms_a, Vs_a, ms_b, Vs_b, ms_c, Vs_c, lam_b, lam_c = (torch.empty((T, K, D), dtype=torch.float32, device=dev)
                                                        for _ in range(8))
    change = torch.empty((K,), dtype=torch.float32, device=dev)
    ws_a = torch.empty(max(int(lib.eks_smooth_tv_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(max(int(lib.eks_smooth_robust_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8,
                       device=dev)
    w_one = torch.ones((T,), dtype=torch.float32, device=dev)
    tv_args = (ctypes.byref(dims), p(y), p(var), p(w_one), 0, *model, p(s), p(ms_a), p(Vs_a), p(ws_a), ws_a.numel())
    one_args = (ctypes.byref(dims), p(y), p(var), *model, p(s), a.nu, 1, p(lam_b), 0, p(change), p(ms_b), p(Vs_b), p(ws_r),
                ws_r.numel())
    eight_args = (ctypes.byref(dims), p(y), p(var), *model, p(s), a.nu, 8, p(lam_c), 0, p(change), p(ms_c), p(Vs_c),
                  p(ws_r), ws_r.numel())

    def tv_shared():
        _lib.check(lib.eks_smooth_tv(*tv_args, hip_ops._stream()), 'eks_smooth_tv')

    def robust_one():
        _lib.check(lib.eks_smooth_robust(*one_args, hip_ops._stream()), 'eks_smooth_robust')

    def robust_eight():
        _lib.check(lib.eks_smooth_robust(*eight_args, hip_ops._stream()), 'eks_smooth_robust')

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    fns = (tv_shared, robust_one, robust_eight)
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(ms_a.view(torch.int32), ms_b.view(torch.int32))
                     and torch.equal(Vs_a.view(torch.int32), Vs_b.view(torch.int32)))
    low = float((lam_c[hit] < 0.1).float().mean().item())
    last_change = float(change.max().item())
    times = [[] for _ in fns]
    for _ in range(a.reps):                       # alternating: all three see the same neighbours on the box
        for t, fn in zip(times, fns):
            t.append(timed(fn))

    def split_of(fn):
        lib.eks_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(8192)
        ms = (ctypes.c_float * 128)()
        n = lib.eks_profile_drain(names, 8192, ms, 128)
        lib.eks_profile_enable(0)
        out = {}
        for name, v in zip([x.decode() for x in names.raw.split(b'\0')[:n]], [float(ms[i]) for i in range(n)]):
            out.setdefault(name, []).append(round(v, 4))
        return out

    splits = [split_of(fn) for fn in fns]
    med = [float(np.median(t)) for t in times]
    rng = lambda t: [round(min(t), 4), round(max(t), 4)]
    per_pass = (med[2] - med[1]) / 7.0
    res = dict(tool='smooth_robust_time', frames=T, keypoints=K, reps=a.reps, nu=a.nu,
               smooth_tv_shared_ms=round(med[0], 4), smooth_tv_shared_ms_min_max=rng(times[0]),
               robust_one_pass_ms=round(med[1], 4), robust_one_pass_ms_min_max=rng(times[1]),
               robust_eight_passes_ms=round(med[2], 4), robust_eight_passes_ms_min_max=rng(times[2]),
               middle_pass_ms=round(per_pass, 4), middle_pass_over_smooth_tv=round(per_pass / med[0], 3),
               robust_one_pass_over_smooth_tv=round(med[1] / med[0], 3),
               one_pass_is_smooth_tv_bit_for_bit=same_bits, displaced_with_weight_below_0p1=round(low, 4),
               last_change_max=last_change,
               smooth_tv_shared_kernels_ms=splits[0], robust_one_pass_kernels_ms=splits[1],
               robust_eight_passes_kernels_ms=splits[2])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
