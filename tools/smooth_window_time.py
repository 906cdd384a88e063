"""hip_ops.smooth alone, windowed replay against the scan-based path, on the library EKS_HIP_LIB selects (run it once
per library for an A/B against another build).  Cases on the flagship shape (100 000 frames x 256 keypoints):
s from the 64-candidate grid (every chain passes), s = exp(-8) (every chain is slow: the windowed form may cost only
its probe and the early-exit launches), one occluded chain per 64-chain tile; then 64 keypoints x 16 384 / 32 768 /
65 536 frames with EKS_SMOOTH_WINDOW_MIN_T=1024, the sizes that fix kWinMinT.  One JSON line per case:
median / min microseconds per call over `--reps` regions of `--calls` calls, EKS_SMOOTH_WINDOW = 0 and 1."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from eks_amd import _lib, hip_ops, synth  # noqa: E402


def knob(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    _lib.load().eks_knobs_reload()


def time_smooth(y, var, s, calls, reps):
    K = y.shape[1]
    dev = y.device
    eye = torch.eye(2, dtype=torch.float64, device=dev).expand(K, 2, 2).contiguous()
    m0 = torch.zeros(K, 2, dtype=torch.float64, device=dev)
    S0 = torch.diag_embed(y.double().var(dim=0, unbiased=False)).contiguous()
    flags = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    ms = torch.empty(y.shape, dtype=torch.float32, device=dev)
    Vs = torch.empty((*y.shape, 2), dtype=torch.float32, device=dev)
    prepared = hip_ops.PreparedSmooth(y, var, m0, S0, eye, eye, eye, s, flags=flags, out=(ms, Vs))
    for _ in range(3):
        prepared()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            prepared()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / calls)
    ms.fill_(float('nan'))                     # what is compared afterwards was written by one more call, not left over
    Vs.fill_(float('nan'))
    prepared()
    torch.cuda.synchronize()
    return round(float(np.median(us)), 1), round(float(np.min(us)), 1), ms, Vs


def case(name, y, var, s, args, min_t=None):
    out = {'case': name, 'T': y.shape[0], 'K': y.shape[1], 'lib': os.environ.get('EKS_HIP_LIB', 'default')}
    knob('EKS_SMOOTH_WINDOW_MIN_T', min_t)
    ref = None
    for mode in (0, 1):
        knob('EKS_SMOOTH_WINDOW', mode)
        med, lo, ms, Vs = time_smooth(y, var, s, args.calls, args.reps)
        out[f'window{mode}_us_median'], out[f'window{mode}_us_min'] = med, lo
        if ref is None:
            ref = (ms.clone(), Vs.clone())
        else:
            sc = ref[0].abs().amax(dim=(0, 2), keepdim=True)
            out['max_rel_diff_ms'] = float(((ms - ref[0]).abs() / sc).max())
            out['max_rel_diff_Vs'] = float(((Vs - ref[1]).abs() / ref[1].abs().clamp_min(1e-30)).nan_to_num(0.0).max())
            out['bit_equal'] = bool(torch.equal(ms, ref[0]) and torch.equal(Vs, ref[1]))
    knob('EKS_SMOOTH_WINDOW', None)
    knob('EKS_SMOOTH_WINDOW_MIN_T', None)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-sizes', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    T, K = 100_000, 256
    y, var = synth.singlecam_observations_torch(T, K, seed=3, device=dev)
    eye = torch.eye(2, dtype=torch.float64, device=dev).expand(K, 2, 2).contiguous()
    m0 = torch.zeros(K, 2, dtype=torch.float64, device=dev)
    S0 = torch.diag_embed(y.double().var(dim=0, unbiased=False)).contiguous()
    cand = torch.exp(torch.linspace(-8.0, 8.0, 64, dtype=torch.float64, device=dev))
    _, s, idx = hip_ops.nll_argmin(y, hip_ops.const_r(var, 1e-4), m0, S0, eye, eye, eye, cand,
                                   flags=_lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC)
    print(json.dumps({'grid_argmin_index_range': [int(idx.min()), int(idx.max())]}), flush=True)
    case('grid_s_all_pass', y, var, s, args)
    case('all_slow', y, var, torch.full((K,), float(np.exp(-8.0)), dtype=torch.float64, device=dev), args)
    occ = var.clone()
    for tile in range(2 * K // 64):
        n = tile * 64 + 11
        occ[40_000:40_300, n // 2, n % 2] *= 1e4
    case('one_occluded_chain_per_tile', y, occ, s, args)
    del occ
    if not args.skip_sizes:
        for Ts in (16_384, 32_768, 65_536):
            ys, vs = synth.singlecam_observations_torch(Ts, 64, seed=4, device=dev)
            case('min_t_size', ys, vs, torch.full((64,), 10.0, dtype=torch.float64, device=dev), args, min_t=1024)


if __name__ == '__main__':
    main()
