"""eks_smooth_tv against eks_smooth and eks_innovations on the C3 shape (100 000 frames x 256 keypoints, D = 2,
diagonal, unit A and C, VS_DIAG), in the same process, alternating:

    (a) eks_smooth with the windowed replay off (EKS_SMOOTH_WINDOW=0)   the fused two-launch form
    (b) eks_innovations with innov + innov_var + loglik                 summarize, three-launch scan, forward replay
                                                                        that writes two [T][N] planes, reduce
    (c) eks_smooth_tv with a shared w = 1                               summarize, the same scan, replay with the
                                                                        backward pass that writes two [T][N] planes
    (d) eks_smooth_tv with a per-keypoint random w

    python tools/smooth_tv_time.py [--frames 100000] [--keypoints 256] [--reps 20] [--out FILE]

Prints one JSON line: median milliseconds and the range of the four (device events), (c)/(b) - the yardstick: both run
the same scan and write two planes -, (c)/(a), (d)/(c) and the per-kernel split of one profiled call of each
(eks_profile_enable).  On a shared box run it under a time limit of its own:

    timeout -k 10 300 python tools/smooth_tv_time.py --out profiles/smooth_tv_time.json"""
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
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    os.environ['EKS_SMOOTH_WINDOW'] = '0'
    import torch
    from eks_amd import _lib, hip_ops
    dev = hip_ops.require_gpu()
    lib = _lib.load()
    lib.eks_knobs_reload()
    T, K, D = a.frames, a.keypoints, 2
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.cumsum(torch.randn((T, K, D), device=dev, generator=g), dim=0).contiguous()
    var = torch.exp(torch.randn((T, K, D), device=dev, generator=g)).contiguous()
    eye = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous()
    m0 = torch.zeros((K, D), dtype=torch.float64, device=dev)
    S0 = eye * 4.0
    s = torch.full((K,), 2.0, dtype=torch.float64, device=dev)
    flags = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    smooth = hip_ops.PreparedSmooth(y, var, m0, S0, eye, eye.clone(), eye.clone(), s, flags, vs_diag=True)
    # (b), (c), (d) with everything but the launches done once, like PreparedSmooth: the comparison is of device time
    dims = _lib.EksDims(K, T, D, D, flags | _lib.FLAG_VS_DIAG)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    model = (p(m0), p(S0), p(eye), p(eye), p(eye))
    innov, innov_var, ms_c, Vs_c, ms_d, Vs_d = (torch.empty((T, K, D), dtype=torch.float32, device=dev) for _ in range(6))
    ll = torch.empty((K, D), dtype=torch.float64, device=dev)
    ws_b = torch.empty(max(int(lib.eks_innovations_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(max(int(lib.eks_smooth_tv_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)
    w_one = torch.ones((T,), dtype=torch.float32, device=dev)
    w_rand = torch.exp(torch.rand((T, K), device=dev, generator=g) * float(np.log(1000.0)) + float(np.log(0.05))).contiguous()
    innov_args = (ctypes.byref(dims), p(y), p(var), *model, p(s), p(innov), p(innov_var), None, None, p(ll), p(ws_b),
                  ws_b.numel())
    tv_one = (ctypes.byref(dims), p(y), p(var), p(w_one), 0, *model, p(s), p(ms_c), p(Vs_c), p(ws_c), ws_c.numel())
    tv_rand = (ctypes.byref(dims), p(y), p(var), p(w_rand), 1, *model, p(s), p(ms_d), p(Vs_d), p(ws_c), ws_c.numel())

    def innovations():
        _lib.check(lib.eks_innovations(*innov_args, hip_ops._stream()), 'eks_innovations')

    def tv_shared():
        _lib.check(lib.eks_smooth_tv(*tv_one, hip_ops._stream()), 'eks_smooth_tv')

    def tv_per_keypoint():
        _lib.check(lib.eks_smooth_tv(*tv_rand, hip_ops._stream()), 'eks_smooth_tv')

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    fns = (smooth, innovations, tv_shared, tv_per_keypoint)
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    # w = 1 against the fused eks_smooth on the same inputs: the largest difference over the chain's scale
    gap_ms = float(((ms_c - smooth.ms).abs().amax(dim=0) / y.abs().amax(dim=0)).max().item())
    gap_Vs = float(((Vs_c - smooth.Vs).abs() / smooth.Vs).max().item())
    times = [[] for _ in fns]
    for _ in range(a.reps):                       # alternating: all four see the same neighbours on the box
        for t, fn in zip(times, fns):
            t.append(timed(fn))

    def split_of(fn):
        lib.eks_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(4096)
        ms = (ctypes.c_float * 64)()
        n = lib.eks_profile_drain(names, 4096, ms, 64)
        lib.eks_profile_enable(0)
        return dict(zip([x.decode() for x in names.raw.split(b'\0')[:n]], [round(float(ms[i]), 4) for i in range(n)]))

    splits = [split_of(fn) for fn in fns]
    med = [float(np.median(t)) for t in times]
    rng = lambda t: [round(min(t), 4), round(max(t), 4)]
    res = dict(tool='smooth_tv_time', frames=T, keypoints=K, reps=a.reps,
               smooth_ms=round(med[0], 4), smooth_ms_min_max=rng(times[0]),
               innovations_ms=round(med[1], 4), innovations_ms_min_max=rng(times[1]),
               smooth_tv_shared_ms=round(med[2], 4), smooth_tv_shared_ms_min_max=rng(times[2]),
               smooth_tv_per_keypoint_ms=round(med[3], 4), smooth_tv_per_keypoint_ms_min_max=rng(times[3]),
               smooth_tv_shared_over_innovations=round(med[2] / med[1], 3),
               smooth_tv_shared_over_smooth=round(med[2] / med[0], 3),
               smooth_tv_per_keypoint_over_shared=round(med[3] / med[2], 3),
               unit_scale_against_smooth_ms_over_max_y=gap_ms, unit_scale_against_smooth_Vs_relative=gap_Vs,
               smooth_kernels_ms=splits[0], innovations_kernels_ms=splits[1], smooth_tv_shared_kernels_ms=splits[2],
               smooth_tv_per_keypoint_kernels_ms=splits[3])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
