"""eks_smooth_heavy_fit against eks_smooth_heavy at equal n_iters, and the fit's reduction launch against the
combine launch of the same profiled call, on the two shapes of tools/smooth_heavy_time.py:

    scalar   100 000 frames x 256 keypoints, D = 2, diagonal, unit A and C, VS_DIAG (the C3 shape)
    general  50 000 frames x 4 keypoints, D = 3, O = 4, full matrices (the generic float64 kernels)

    python tools/smooth_heavy_fit_time.py [--reps 5] [--passes 12] [--nu 4] [--rounds 3] [--parent-lib FILE]
                                          [--skip-general] [--out FILE]

Every measurement runs in a fresh child process (this file with --worker): `rounds` alternations of
  fit     this build: eks_smooth_heavy_fit and eks_smooth_heavy alternating in the process, `reps` timed regions each
          (device events, warm), then one profiled call of the fit (eks_profile_enable) for the per-launch split;
  parent  with --parent-lib (a libeks_hip.so built from the parent commit): its eks_smooth_heavy, the same way.
The reduction reads the planes the combine launch has just read, once more: the bar is heavy_fit <= 2 x jumps_combine
by their medians per launch (the factor would cover a second launch at the launch floor; the reduction is one).
Prints one JSON line per shape and writes them to --out.  On a shared box run it under a time limit of its own:

    timeout -k 10 600 python tools/smooth_heavy_fit_time.py --out profiles/smooth_heavy_fit_time.json"""
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


def open_library(path, names):
    """The library at `path` with the signatures of `names` only: a parent build has no eks_smooth_heavy_fit."""
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
    fit = a.worker == 'fit'
    names = ['eks_smooth_heavy', 'eks_smooth_heavy_workspace_bytes'] + \
        (['eks_smooth_heavy_fit', 'eks_smooth_heavy_fit_workspace_bytes'] if fit else [])
    lib = open_library(a.lib, names)
    make = sht.scalar_problem if a.shape == 'scalar' else sht.general_problem
    name, (T, K, D, O), flags, y, var, par, vs_shape = make(torch, dev, _lib)
    dims = _lib.EksDims(K, T, D, O, flags)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    model = tuple(p(t) for t in par)
    ms = torch.empty((T, K, D), dtype=torch.float32, device=dev)
    Vs = torch.empty(vs_shape, dtype=torch.float32, device=dev)
    weights = torch.empty((T, K, O), dtype=torch.float32, device=dev)
    scales = torch.empty((T, K), dtype=torch.float32, device=dev)
    change = torch.empty((3, K), dtype=torch.float32, device=dev)
    s_out = torch.empty((K,), dtype=torch.float64, device=dev)
    space = lambda q: torch.empty(max(int(q(ctypes.byref(dims))), 256), dtype=torch.uint8, device=dev)  # noqa: E731
    ws_h = space(lib.eks_smooth_heavy_workspace_bytes)
    h_args = (ctypes.byref(dims), p(y), p(var), *model, a.nu, a.nu, a.passes, p(weights), p(scales), 0, p(change), p(ms),
              p(Vs), p(ws_h), ws_h.numel())

    def heavy():
        _lib.check(lib.eks_smooth_heavy(*h_args, hip_ops._stream()), 'eks_smooth_heavy')

    fns = [heavy]
    if fit:
        ws_f = space(lib.eks_smooth_heavy_fit_workspace_bytes)
        f_args = (ctypes.byref(dims), p(y), p(var), *model, a.nu, a.nu, a.passes, -8.0, 8.0, p(weights), p(scales), 0,
                  p(change), p(s_out), p(ms), p(Vs), p(ws_f), ws_f.numel())

        def fitted():
            _lib.check(lib.eks_smooth_heavy_fit(*f_args, hip_ops._stream()), 'eks_smooth_heavy_fit')
        fns.append(fitted)

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
    out = dict(shape=name, dims=[T, K, D, O], heavy_ms=times[0])
    if fit:
        out['fit_ms'] = times[1]
        torch.cuda.synchronize()
        out['s_fit_min_max'] = [float(s_out.min().item()), float(s_out.max().item())]
        out['last_dlog_s_max'] = float(change[2].max().item())
        lib.eks_profile_enable(1)
        fns[1]()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(16384)
        ms_ = (ctypes.c_float * 256)()
        n = lib.eks_profile_drain(buf, 16384, ms_, 256)
        lib.eks_profile_enable(0)
        split = {}
        for nm, v in zip([x.decode() for x in buf.raw.split(b'\0')[:n]], [float(ms_[i]) for i in range(n)]):
            split.setdefault(nm, []).append(v)
        out['launches'] = split
    print('WORKER ' + json.dumps(out), flush=True)


def run_worker(a, kind, shape, lib):
    cmd = [sys.executable, os.path.abspath(__file__), '--worker', kind, '--shape', shape, '--reps', str(a.reps),
           '--passes', str(a.passes), '--nu', str(a.nu)] + (['--lib', lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.worker_timeout)
    if r.returncode != 0:
        raise RuntimeError(f'worker {kind} {shape} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('WORKER ')][-1]
    return json.loads(line[len('WORKER '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--passes', type=int, default=12)
    ap.add_argument('--nu', type=float, default=4.0)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--skip-general', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--worker', default=None, choices=['fit', 'parent'])
    ap.add_argument('--shape', default='scalar')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--worker-timeout', type=float, default=240.0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    lines = []
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    for shape in ('scalar',) + (() if a.skip_general else ('general',)):
        fit_ms, heavy_ms, parent_ms, launches = [], [], [], {}
        info = {}
        for _ in range(a.rounds):                     # alternating fresh processes: both see the same neighbours
            w = run_worker(a, 'fit', shape, None)
            fit_ms += w['fit_ms']
            heavy_ms += w['heavy_ms']
            info = w
            for nm, v in w['launches'].items():
                launches.setdefault(nm, []).extend(v)
            if a.parent_lib:
                parent_ms += run_worker(a, 'parent', shape, a.parent_lib)['heavy_ms']
        T, K, D, O = info['dims']
        per = {nm: dict(launches_per_call=len(v) // a.rounds, median_ms=med(v)) for nm, v in launches.items()}
        red = per['heavy_fit']['median_ms']
        comb = per['jumps_combine']['median_ms']
        res = dict(tool='smooth_heavy_fit_time', shape=shape, frames=T, keypoints=K, state_dim=D, obs_dim=O,
                   passes=a.passes, reps=a.reps, rounds=a.rounds, nu=a.nu, fit_ms=med(fit_ms),
                   fit_ms_min_max=[round(min(fit_ms), 4), round(max(fit_ms), 4)], heavy_ms=med(heavy_ms),
                   heavy_ms_min_max=[round(min(heavy_ms), 4), round(max(heavy_ms), 4)],
                   fit_over_heavy=round(med(fit_ms) / med(heavy_ms), 3),
                   parent_heavy_ms=med(parent_ms) if parent_ms else None,
                   parent_heavy_ms_min_max=[round(min(parent_ms), 4), round(max(parent_ms), 4)] if parent_ms else None,
                   reduction_ms_per_step=round(red, 4), combine_ms_per_launch=comb,
                   reduction_over_combine=round(red / comb, 3), bar=2.0, within_bar=bool(red <= 2.0 * comb),
                   s_fit_min_max=info['s_fit_min_max'], last_dlog_s_max=info['last_dlog_s_max'], fit_kernels=per)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
