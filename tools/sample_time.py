"""Posterior sampling against the compose-it-yourself route: n_draws joint trajectories from ONE eks_sample call
against n_draws calls of eks_smooth on the same inputs, in the same process, alternating.

    python tools/sample_time.py [--frames 100000] [--keypoints 256] [--draws 16] [--reps 20] [--out FILE]

Prints one JSON line: median milliseconds of both (device events), their ratio, the bytes eks_sample has to write
(n_draws * T * K * D * 4) over its time and that rate as a fraction of the 6.29 TB/s copy ceiling, and the
per-kernel split of one profiled call (eks_profile_enable)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_CEILING = 6.29e12


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
    T, K, D, S = a.frames, a.keypoints, 2, a.draws
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.cumsum(torch.randn((T, K, D), device=dev, generator=g), dim=0).contiguous()
    var = torch.exp(torch.randn((T, K, D), device=dev, generator=g)).contiguous()
    eye = torch.eye(D, dtype=torch.float64, device=dev).repeat(K, 1, 1).contiguous()
    m0 = torch.zeros((K, D), dtype=torch.float64, device=dev)
    s = torch.full((K,), 2.0, dtype=torch.float64, device=dev)
    flags = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    smooth = hip_ops.PreparedSmooth(y, var, m0, eye * 4.0, eye, eye.clone(), eye.clone(), s, flags)
    draws = torch.empty((S, T, K, D), dtype=torch.float32, device=dev)

    def sample():
        hip_ops.sample(y, var, m0, eye * 4.0, eye, eye, eye, s, S, seed=1, flags=flags, out=draws)

    def compose():
        for _ in range(S):
            smooth()

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    for _ in range(3):
        sample()
        compose()
    torch.cuda.synchronize()
    ts, tc = [], []
    for _ in range(a.reps):                       # alternating: both see the same neighbours on the box
        ts.append(timed(sample))
        tc.append(timed(compose))
    lib = _lib.load()
    lib.eks_profile_enable(1)
    sample()
    torch.cuda.synchronize()
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_float * 64)()
    n = lib.eks_profile_drain(names, 4096, ms, 64)
    lib.eks_profile_enable(0)
    split = dict(zip([x.decode() for x in names.raw.split(b'\0')[:n]], [round(float(ms[i]), 4) for i in range(n)]))
    t_s, t_c = float(np.median(ts)), float(np.median(tc))
    out_bytes = S * T * K * D * 4
    res = dict(tool='sample_time', frames=T, keypoints=K, draws=S, reps=a.reps, sample_ms=round(t_s, 4),
               sample_ms_min_max=[round(min(ts), 4), round(max(ts), 4)], smooth_x_draws_ms=round(t_c, 4),
               smooth_ms_min_max=[round(min(tc), 4), round(max(tc), 4)], ratio=round(t_c / t_s, 3),
               draws_bytes=out_bytes, write_rate_TBps=round(out_bytes / (t_s * 1e-3) / 1e12, 3),
               write_rate_of_copy_ceiling=round(out_bytes / (t_s * 1e-3) / COPY_CEILING, 3), kernels_ms=split)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
