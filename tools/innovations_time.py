"""eks_innovations against eks_smooth and eks_em_stats on the C3 shape (100 000 frames x 256 keypoints, D = 2,
diagonal, unit A and C), in the same process, alternating:

    (a) eks_smooth with VS_DIAG                               ms, Vs
    (b) eks_em_stats                                          Sw (summarize, scan, forward + backward replay, reduce)
    (c) eks_innovations with loglik only                      the same summarize and scan, a forward-only replay, reduce
    (d) eks_innovations with innov + innov_var + loglik       (c) plus two float32 planes of stores

    python tools/innovations_time.py [--frames 100000] [--keypoints 256] [--reps 20] [--out FILE]

Prints one JSON line: median milliseconds and the range of the four (device events), (c)/(b), (d)/(c) and the
per-kernel split of one profiled call of each (eks_profile_enable).  (c) does strictly less than (b) - it has no
backward pass - so it should not exceed (b) beyond the repetitions' own spread.  On a shared box run it under a time
limit of its own:

    timeout -k 10 300 python tools/innovations_time.py --out profiles/innovations_time.json"""
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
    import torch
    from eks_amd import _lib, hip_ops
    dev = hip_ops.require_gpu()
    lib = _lib.load()
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
    model = (p(y), p(var), p(m0), p(S0), p(eye), p(eye), p(eye))
    Sw = torch.empty((K, D), dtype=torch.float64, device=dev)
    ws_b = torch.empty(max(int(lib.eks_em_stats_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)
    em_args = (ctypes.byref(dims), *model, p(s), p(Sw), p(ws_b), ws_b.numel())
    innov, innov_var = (torch.empty((T, K, D), dtype=torch.float32, device=dev) for _ in range(2))
    ll_c, ll_d = (torch.empty((K, D), dtype=torch.float64, device=dev) for _ in range(2))
    ws_c = torch.empty(max(int(lib.eks_innovations_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)
    ll_args = (ctypes.byref(dims), *model, p(s), None, None, None, None, p(ll_c), p(ws_c), ws_c.numel())
    all_args = (ctypes.byref(dims), *model, p(s), p(innov), p(innov_var), None, None, p(ll_d), p(ws_c), ws_c.numel())

    def em_stats():
        _lib.check(lib.eks_em_stats(*em_args, hip_ops._stream()), 'eks_em_stats')

    def loglik_only():
        _lib.check(lib.eks_innovations(*ll_args, hip_ops._stream()), 'eks_innovations')

    def all_outputs():
        _lib.check(lib.eks_innovations(*all_args, hip_ops._stream()), 'eks_innovations')

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    fns = (smooth, em_stats, loglik_only, all_outputs)
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(ll_c, ll_d))
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
    res = dict(tool='innovations_time', frames=T, keypoints=K, reps=a.reps,
               smooth_ms=round(med[0], 4), smooth_ms_min_max=rng(times[0]),
               em_stats_ms=round(med[1], 4), em_stats_ms_min_max=rng(times[1]),
               loglik_only_ms=round(med[2], 4), loglik_only_ms_min_max=rng(times[2]),
               all_outputs_ms=round(med[3], 4), all_outputs_ms_min_max=rng(times[3]),
               loglik_only_over_em_stats=round(med[2] / med[1], 3), all_outputs_over_loglik_only=round(med[3] / med[2], 3),
               loglik_same_bits_with_and_without_the_planes=same_bits,
               mean_loglik_per_frame=float(ll_c.sum().item() / (T * K * D)),
               smooth_kernels_ms=splits[0], em_stats_kernels_ms=splits[1], loglik_only_kernels_ms=splits[2],
               all_outputs_kernels_ms=splits[3])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
