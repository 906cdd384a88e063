"""Timings of the extended smoother for user-supplied emission functions (eks_amd.emission.DifferentiableEmission,
eks_ekf_affine_sweep) on bench.py's `ekf` shape (T = 50 000, K = 16, V = 4, fixed s, cold start), beside the native
pinhole path (eks_ekf_smooth) on the same problem: ms per call and sweeps, how a sweep splits between the torch
evaluation of fn and its Jacobian, the table assembly and the kernels (ProfScope names ekf_affine_*), 16 against 32
frames per lane (EKS_DENSE_CHUNK), and the Adam and grid modes.  Usage: python tools/ekf_generic_time.py [out.txt]"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eks_amd import _lib, calibration as cal
from eks_amd import core, synth
from eks_amd.core import run_kalman_smoother
from eks_amd.emission import DifferentiableEmission

LINES = []


def out(msg):
    print(msg, flush=True)
    LINES.append(msg)


def drain(lib):
    names = ctypes.create_string_buffer(1 << 16)
    ms = (ctypes.c_float * 4096)()
    n = lib.eks_profile_drain(names, len(names), ms, 4096)
    keys = names.raw.split(b'\0')[:n]
    acc = {}
    for k, v in zip(keys, ms[:n]):
        acc[k.decode()] = acc.get(k.decode(), 0.0) + v
    return acc


def main():
    T, K, V = 50_000, 16, 4
    prob = synth.calibrated_multicam(T, K, V, seed=4)
    ys = np.swapaxes(prob['y_tko'], 0, 1)
    args = (ys, prob['m0s'], prob['S0s'], prob['As'], None, prob['Qs'], prob['var_tko'])
    pin = cal.PinholeProjection(prob['cams_packed'])
    gen = DifferentiableEmission(synth.torch_pinhole(prob['cams_packed']))
    lib = _lib.load()
    out(f'bench ekf shape: T={T} K={K} V={V} (O={2 * V}, D=3), cold start (x = prior mean), s fixed, '
        'device outputs')

    def timed(fn, n=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, r

    for chunk in ('16', '32'):
        os.environ['EKS_DENSE_CHUNK'] = chunk
        lib.eks_knobs_reload()
        out(f'-- frames per lane {chunk}')
        for sval in (0.1, 10.0):
            dt_p, _ = timed(lambda: run_kalman_smoother(*args, smooth_param=sval, h_fn=pin, return_device=True))
            dt_g, r = timed(lambda: run_kalman_smoother(*args, smooth_param=sval, h_fn=gen, return_device=True,
                                                        return_info=True))
            info = r[3]
            out(f's={sval:g}: PinholeProjection {dt_p:.2f} ms | DifferentiableEmission {dt_g:.2f} ms, '
                f'{info["sweeps"]} sweeps (last change {info["change"]:.1e})')
        # one sweep, split: torch evaluation of fn + Jacobian, table assembly, kernels
        dev = torch.device('cuda')
        t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)   # noqa: E731
        y = torch.as_tensor(prob['y_tko'], dtype=torch.float32, device=dev)
        var = torch.as_tensor(prob['var_tko'], dtype=torch.float32, device=dev)
        m0, S0, A, Q = t64(prob['m0s']), t64(prob['S0s']), t64(prob['As']), t64(prob['Qs'])
        s = torch.full((K,), 10.0, dtype=torch.float64, device=dev)
        runner = core._EmissionSweeps(gen, K, T, 3, 2 * V, dev, want_smoother=True)
        xlin = m0[:, None, :].expand(K, T, 3).contiguous()
        runner.solve(y, var, None, m0, S0, A, Q, s, xlin, 32, 1e-10)          # converged points
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        parts = np.zeros(3)
        n = 5
        lib.eks_profile_enable(1)
        drain(lib)
        for _ in range(n):
            ev[0].record()
            X = runner.evaluate(xlin)
            ev[1].record()
            runner.assemble(X)
            ev[2].record()
            runner.sweep(y, var, None, m0, S0, A, Q, s, xlin)
            ev[3].record()
            torch.cuda.synchronize()
            parts += [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
        kern = drain(lib)
        lib.eks_profile_enable(0)
        parts /= n
        out(f'one filter sweep: fn + Jacobian {parts[0]:.3f} ms, table assembly {parts[1]:.3f} ms, '
            f'kernels {parts[2]:.3f} ms (total {parts.sum():.3f} ms); per kernel stage: '
            + ', '.join(f'{k} {v / n:.3f}' for k, v in sorted(kern.items())))
    os.environ.pop('EKS_DENSE_CHUNK')
    lib.eks_knobs_reload()
    out('-- search modes (default frames per lane)')
    for mode in ('adam', 'grid'):
        for h, name in ((pin, 'PinholeProjection'), (gen, 'DifferentiableEmission')):
            run_kalman_smoother(ys[:2, :2000], prob['m0s'][:2], prob['S0s'][:2], prob['As'][:2], None,
                                prob['Qs'][:2], prob['var_tko'][:2000, :2], h_fn=h, s_mode=mode, n_grid=16)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = run_kalman_smoother(*args, h_fn=h, s_mode=mode, n_grid=16, return_device=True, return_info=True)
            torch.cuda.synchronize()
            info = r[3]
            extra = f', search sweeps {info["search_sweeps"]}' if 'search_sweeps' in info else ''
            out(f'{mode:4s} n_grid=16 {name}: {(time.perf_counter() - t0) * 1e3:.0f} ms, s in '
                f'[{r[0].min():.3g}, {r[0].max():.3g}]{extra}')
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
