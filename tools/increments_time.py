"""eks_smooth_increments against eks_smooth and against the Monte-Carlo route it replaces, on the C3 shape
(100 000 frames x 256 keypoints, D = 2, diagonal, fixed s, VS_DIAG), in the same process, alternating:

    (a) eks_smooth with VS_DIAG                      ms, Vs
    (b) eks_smooth_increments, all five outputs      ms, Vs, lag1, dmean, dV
    (c) eks_sample with 16 draws                     what a speed error bar cost before

    python tools/increments_time.py [--frames 100000] [--keypoints 256] [--draws 16] [--reps 20] [--out FILE]

Prints one JSON line: median milliseconds of the three (device events), (b)/(a), (b)/(c) and the per-kernel split of
one profiled call of (a) and of (b) (eks_profile_enable).  On a shared box run it under a time limit of its own:

    timeout -k 10 300 python tools/increments_time.py --out profiles/r09_increments_time.json"""
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
    ap.add_argument('--draws', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from eks_amd import _lib, hip_ops
    dev = hip_ops.require_gpu()
    lib = _lib.load()
    T, K, D, S = a.frames, a.keypoints, 2, a.draws
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.cumsum(torch.randn((T, K, D), device=dev, generator=g), dim=0).contiguous()
    var = torch.exp(torch.randn((T, K, D), device=dev, generator=g)).contiguous()
    eye = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous()
    m0 = torch.zeros((K, D), dtype=torch.float64, device=dev)
    S0 = eye * 4.0
    s = torch.full((K,), 2.0, dtype=torch.float64, device=dev)
    flags = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    smooth = hip_ops.PreparedSmooth(y, var, m0, S0, eye, eye.clone(), eye.clone(), s, flags, vs_diag=True)
    draws = torch.empty((S, T, K, D), dtype=torch.float32, device=dev)
    # (b) with everything but the launches done once, like PreparedSmooth: the comparison is of device time
    dims = _lib.EksDims(K, T, D, D, flags | _lib.FLAG_VS_DIAG)
    outs = [torch.empty((T, K, D), dtype=torch.float32, device=dev) for _ in range(5)]
    ws = torch.empty(max(int(lib.eks_smooth_increments_workspace_bytes(ctypes.byref(dims))), 256), dtype=torch.uint8,
                     device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    inc_args = (ctypes.byref(dims), p(y), p(var), p(m0), p(S0), p(eye), p(eye), p(eye), p(s), *(p(o) for o in outs), p(ws),
                ws.numel())

    def increments():
        _lib.check(lib.eks_smooth_increments(*inc_args, hip_ops._stream()), 'eks_smooth_increments')

    def sample():
        hip_ops.sample(y, var, m0, S0, eye, eye, eye, s, S, seed=1, flags=flags, out=draws)

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    for _ in range(3):
        smooth()
        increments()
        sample()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(a.reps):                       # alternating: all three see the same neighbours on the box
        ta.append(timed(smooth))
        tb.append(timed(increments))
        tc.append(timed(sample))

    def split_of(fn):
        lib.eks_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(4096)
        ms = (ctypes.c_float * 64)()
        n = lib.eks_profile_drain(names, 4096, ms, 64)
        lib.eks_profile_enable(0)
        return dict(zip([x.decode() for x in names.raw.split(b'\0')[:n]], [round(float(ms[i]), 4) for i in range(n)]))

    split_a, split_b = split_of(smooth), split_of(increments)
    m_a, m_b, m_c = (float(np.median(t)) for t in (ta, tb, tc))
    rng = lambda t: [round(min(t), 4), round(max(t), 4)]
    res = dict(tool='increments_time', frames=T, keypoints=K, draws=S, reps=a.reps,
               smooth_ms=round(m_a, 4), smooth_ms_min_max=rng(ta),
               increments_ms=round(m_b, 4), increments_ms_min_max=rng(tb),
               sample_ms=round(m_c, 4), sample_ms_min_max=rng(tc),
               increments_over_smooth=round(m_b / m_a, 3), increments_over_sample=round(m_b / m_c, 3),
               bytes_per_chain_frame=dict(smooth=[16, 8], increments=[16, 20]),
               smooth_kernels_ms=split_a, increments_kernels_ms=split_b)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
