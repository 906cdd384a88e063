"""eks_sample_tv (per-keypoint qscale, weights present) against eks_sample, on the two shapes of tools/smooth_heavy_time.py:

    scalar   100 000 frames x 256 keypoints, D = 2, diagonal, unit A and C, n_draws = 16
    general  50 000 frames x 4 keypoints, D = 3, O = 4, full matrices, n_draws = 8 (Durbin-Koopman: correct, not tuned)

    python tools/sample_tv_time.py [--reps 5] [--rounds 3] [--parent-lib FILE] [--skip-general] [--out FILE]

Every measurement runs in a fresh child process (this file with --worker): `rounds` alternations of
  tv      this build: eks_sample and eks_sample_tv alternating in the process, `reps` timed regions each (device
          events, warm), then one profiled call of eks_sample_tv (eks_profile_enable) for the per-launch split;
  parent  with --parent-lib (a libeks_hip.so built from the parent commit): its eks_sample, the same way - the yardstick.
eks_sample of this build has to lie inside the parent's [min, max] (its kernels are the parent's text).  The ratio
eks_sample_tv / eks_sample (parent) is compared with the ratio of the bytes the two calls move on the scalar shape
(DESIGN.md 9r's launch list: the old call reads y twice and var three times and writes n_draws + 1 planes; the new one
also reads weights three times and qscale three times), the margin being the parent's own max / min.  Prints one JSON
line per shape and writes them to --out.  On a shared box run it under a time limit of its own:

    timeout -k 10 600 python tools/sample_tv_time.py --out profiles/sample_tv_time.json"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_DRAWS = dict(scalar=16, general=8)


def open_library(path, names):
    """The library at `path` with the signatures of `names` only: a parent build has no eks_sample_tv."""
    from eks_amd import _lib
    lib = ctypes.CDLL(path or _lib.LIB_PATH)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    lib.eks_profile_enable.argtypes = [ctypes.c_int]
    lib.eks_profile_drain.restype = ctypes.c_int
    return lib


def worker(a):
    import torch
    from eks_amd import _lib, hip_ops
    import smooth_heavy_time as sht
    dev = hip_ops.require_gpu()
    tv = a.worker == 'tv'
    names = ['eks_sample', 'eks_sample_workspace_bytes'] + (['eks_sample_tv', 'eks_sample_tv_workspace_bytes'] if tv else [])
    lib = open_library(a.lib, names)
    make = sht.scalar_problem if a.shape == 'scalar' else sht.general_problem
    name, (T, K, D, O), flags, y, var, par, _ = make(torch, dev, _lib)
    S = N_DRAWS[a.shape]
    dims = _lib.EksDims(K, T, D, O, flags)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    model = tuple(p(t) for t in par)
    g = torch.Generator(device=dev).manual_seed(1)
    qscale = torch.exp(torch.rand((T, K), device=dev, generator=g) * 2.0 - 1.0).contiguous()
    weights = (torch.rand((T, K, O), device=dev, generator=g) * 1.2 + 0.05).contiguous()
    ms = torch.empty((T, K, D), dtype=torch.float32, device=dev)
    draws = torch.empty((S, T, K, D), dtype=torch.float32, device=dev)
    space = lambda q: torch.empty(max(int(q(ctypes.byref(dims), S)), 256), dtype=torch.uint8, device=dev)  # noqa: E731
    ws_s = space(lib.eks_sample_workspace_bytes)
    s_args = (ctypes.byref(dims), p(y), p(var), *model, S, 7, 0, 0, None, p(ms), p(draws), p(ws_s), ws_s.numel())

    def sample():
        _lib.check(lib.eks_sample(*s_args, hip_ops._stream()), 'eks_sample')

    fns = [sample]
    if tv:
        ws_t = space(lib.eks_sample_tv_workspace_bytes)
        t_args = (ctypes.byref(dims), p(y), p(var), p(qscale), 1, p(weights), *model, S, 7, 0, 0, None, p(ms), p(draws),
                  p(ws_t), ws_t.numel())

        def sample_tv():
            _lib.check(lib.eks_sample_tv(*t_args, hip_ops._stream()), 'eks_sample_tv')
        fns.append(sample_tv)

    def timed(fn):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        fn()
        b_.record()
        b_.synchronize()
        return a_.elapsed_time(b_)

    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(a.reps):
        for t, fn in zip(times, fns):
            t.append(timed(fn))
    out = dict(shape=name, dims=[T, K, D, O], n_draws=S, sample_ms=times[0])
    if tv:
        out['tv_ms'] = times[1]
        split = {}
        for which, fn in (('eks_sample', fns[0]), ('eks_sample_tv', fns[1])):
            lib.eks_profile_enable(1)
            fn()
            torch.cuda.synchronize()
            buf = ctypes.create_string_buffer(16384)
            ms_ = (ctypes.c_float * 256)()
            n = lib.eks_profile_drain(buf, 16384, ms_, 256)
            lib.eks_profile_enable(0)
            for nm, v in zip([x.decode() for x in buf.raw.split(b'\0')[:n]], [float(ms_[i]) for i in range(n)]):
                split.setdefault(which, {}).setdefault(nm, []).append(v)
        out['launches'] = split
    print('WORKER ' + json.dumps(out), flush=True)


def run_worker(a, kind, shape, lib):
    cmd = [sys.executable, os.path.abspath(__file__), '--worker', kind, '--shape', shape, '--reps', str(a.reps)] + \
        (['--lib', lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError(f'worker {kind} {shape} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('WORKER ')][-1]
    return json.loads(line[len('WORKER '):])


def byte_ratio(T, K, D, S):
    """Bytes eks_sample_tv / eks_sample move on scalar chains, from the launch lists (the workspace planes, 1 / 32 of
    a frame plane each, left out of both): old = y x 2 + var x 3 + (S + 1) output planes of T N floats; new adds
    weights x 3 (T N floats) and qscale x 3 (T K floats)."""
    N = K * D
    old = (2 + 3 + S + 1) * T * N
    return (old + 3 * T * N + 3 * T * K) / old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--skip-general', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--worker', default=None, choices=['tv', 'parent'])
    ap.add_argument('--shape', default='scalar')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--worker-timeout', type=float, default=240.0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    lines = []
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    rng_ = lambda v: [round(min(v), 4), round(max(v), 4)]  # noqa: E731
    for shape in ('scalar',) + (() if a.skip_general else ('general',)):
        tv_ms, sample_ms, parent_ms, launches, info = [], [], [], {}, {}
        for _ in range(a.rounds):                     # alternating fresh processes: both see the same neighbours
            w = run_worker(a, 'tv', shape, None)
            tv_ms += w['tv_ms']
            sample_ms += w['sample_ms']
            info = w
            for which, per in w['launches'].items():
                for nm, v in per.items():
                    launches.setdefault(which, {}).setdefault(nm, []).extend(v)
            if a.parent_lib:
                parent_ms += run_worker(a, 'parent', shape, a.parent_lib)['sample_ms']
        T, K, D, O = info['dims']
        S = info['n_draws']
        per = {which: {nm: dict(launches_per_call=len(v) // a.rounds, median_ms=med(v)) for nm, v in d.items()}
               for which, d in launches.items()}
        res = dict(tool='sample_tv_time', shape=shape, frames=T, keypoints=K, state_dim=D, obs_dim=O, n_draws=S,
                   reps=a.reps, rounds=a.rounds, sample_tv_ms=med(tv_ms), sample_tv_ms_min_max=rng_(tv_ms),
                   sample_ms=med(sample_ms), sample_ms_min_max=rng_(sample_ms),
                   parent_sample_ms=med(parent_ms) if parent_ms else None,
                   parent_sample_ms_min_max=rng_(parent_ms) if parent_ms else None, kernels=per)
        if parent_ms:
            spread = max(parent_ms) / min(parent_ms)
            res['sample_inside_parent_range'] = bool(min(parent_ms) <= med(sample_ms) <= max(parent_ms))
            res['tv_over_parent_sample'] = round(med(tv_ms) / med(parent_ms), 3)
            res['parent_spread_max_over_min'] = round(spread, 3)
            if shape == 'scalar':
                br = byte_ratio(T, K, D, S)
                res['byte_ratio'] = round(br, 3)
                res['bound'] = round(br * spread, 3)
                res['within_bound'] = bool(med(tv_ms) / med(parent_ms) <= br * spread)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
