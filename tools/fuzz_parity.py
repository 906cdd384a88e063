"""Randomised parity sweep of the scalar-chain kernels against the C oracle: random T, K, model
(unit / general diagonal), variance scales (incl. clipped zeros), smoothing parameters.
Usage: python tools/fuzz_parity.py [n_cases] [seed] [window]
With `window` the sweep is the smoother's alone, in the windowed form (EKS_SMOOTH_WINDOW_MIN_T = 1024: T from 1024 up, K
from 17 up, state width D from {1, 2, 3}): EKS_SMOOTH_WINDOW = 1 and 0 against the oracle, and from a run with
EKS_SMOOTH_WINDOW = 2 the share of (window group, chain) lanes the windowed kernel stored itself."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np
from oracle import c_oracle, eks_oracle as orc
import test_gpu_kernels as tg
from eks_amd import hip_ops, _lib

window = len(sys.argv) > 3 and sys.argv[3] == 'window'
WIN_GROUP = 256                              # frames of a window group (eks_diag.hip: kChunk * kWinG)


def knob(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    _lib.load().eks_knobs_reload()


def regroup(arrs, y_tk, var_tk, K, D):
    """The 2 * Kc scalar chains of a (T, Kc, 2) problem as K keypoints of D coordinates (chains are independent: which
    keypoint a chain belongs to only decides the s it shares)."""
    T = y_tk.shape[0]
    dg = lambda M: np.diagonal(M, axis1=1, axis2=2).reshape(-1)[:K * D].reshape(K, D)
    eye = np.eye(D)
    out = dict(m0s=arrs['m0s'].reshape(-1)[:K * D].reshape(K, D).copy())
    for k in ('S0s', 'As', 'Cs', 'Qs'):
        out[k] = eye * dg(arrs[k])[:, :, None]
    cut = lambda a: np.ascontiguousarray(a.reshape(T, -1)[:, :K * D].reshape(T, K, D))
    y_tk, var_tk = cut(y_tk), cut(var_tk)
    out['ys'] = np.transpose(y_tk, (1, 0, 2)).astype(np.float64)
    out['ensemble_vars'] = var_tk.astype(np.float64)
    return out, y_tk, var_tk


if window:
    knob('EKS_SMOOTH_WINDOW_MIN_T', '1024')
n_stored = n_lanes = 0
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
worst = dict(ms=0.0, Vs=0.0, nll=0.0, med=0.0)
for case in range(n_cases):
    if window:
        T = int(rng.choice([1024, 1025, 2049, 4097, 9000, 20011]))
        K = int(rng.choice([17, 31, 32, 33, 70, 700]))
        D = int(rng.choice([1, 2, 3]))
    else:
        T = int(rng.choice([1, 2, 3, 7, 31, 32, 33, 64, 257, 1000, 1024, 1025, 2049, 4097, 9000, 20011]))
        K = int(rng.choice([1, 2, 3, 5, 17, 31, 32, 33, 70, 700]))
        D = 2
    unit = bool(rng.integers(0, 2))
    arrs, y_tk, var_tk = tg._singlecam_problem(max(T, 2), (K * D + 1) // 2, seed=int(rng.integers(1 << 30)), unit=unit)
    if D != 2:
        arrs, y_tk, var_tk = regroup(arrs, y_tk, var_tk, K, D)
    y_tk, var_tk = y_tk[:T].copy(), var_tk[:T].copy()
    arrs['ys'] = arrs['ys'][:, :T]; arrs['ensemble_vars'] = arrs['ensemble_vars'][:T]
    scale = float(np.exp(rng.uniform(-4, 4)))
    var_tk = (var_tk * scale).astype(np.float32)
    if rng.random() < 0.4:
        var_tk[rng.random(var_tk.shape) < 0.1] = 0.0
    y_tk = (y_tk * float(np.exp(rng.uniform(-1, 2)))).astype(np.float32)
    arrs['ys'] = np.transpose(y_tk, (1, 0, 2)).astype(np.float64); arrs['ensemble_vars'] = var_tk.astype(np.float64)
    if T < 3:
        arrs['S0s'] = np.tile(np.eye(D) * 3.0, (K, 1, 1))
    else:
        arrs['S0s'] = np.eye(D) * np.maximum(np.var(arrs['ys'], axis=1), 1e-3)[:, :, None]
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    Rd = np.maximum(np.swapaxes(arrs['ensemble_vars'], 0, 1), 1e-12)
    e_nll, n_cand = 0.0, 0
    if not window:
        # constant R (exact median)
        rc = hip_ops.const_r(tg._dev(var_tk), 1e-4).cpu().numpy()
        ref_rc = orc.constant_R_from_timevarying(Rd)
        worst['med'] = max(worst['med'], float(np.abs(rc - ref_rc).max() / np.abs(ref_rc).max()))
        assert np.array_equal(rc, ref_rc), (case, T, K, 'median mismatch')
        # NLL grid
        n_cand = int(rng.choice([1, 5, 16, 64, 129, 200]))
        cand = np.exp(np.sort(rng.uniform(-8, 8, n_cand)))
        nll = hip_ops.nll(tg._dev(y_tk), tg._dev(rc), *tg._params_dev(arrs), tg._dev(cand), flags=flags).cpu().numpy()
        ref = c_oracle.nll_grid(arrs['ys'], rc, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], cand)
        # relative to the NLL or - where the log-determinant and quadratic parts cancel and the NLL itself
        # passes through zero (small R: log S < 0) - to the size of the parts, T * sum_chains (|log R| + 1):
        # against |nll| alone two such cases read 2.7e-5 / 1.5e-5 for absolute errors of 3e-5 on parts
        # of 2e3 (seed 2222, cases 18 and 21)
        gross = T * (np.abs(np.log(rc)) + 1.0).sum(axis=1, keepdims=True)
        rel = np.abs(nll - ref) / np.maximum(np.abs(ref), 1e-2 * gross)
        e_nll = float(rel.max())
        if os.environ.get('FUZZ_DETAIL') and e_nll > 3e-6:
            k, c = np.unravel_index(np.argmax(rel), rel.shape)
            print(f'   detail: keypoint {k} candidate {c} s={cand[c]:.4g} rconst={rc[k]} q={np.diagonal(arrs["Qs"][k])} '
                  f'a={np.diagonal(arrs["As"][k])} c={np.diagonal(arrs["Cs"][k])} nll gpu {nll[k, c]:.10g} oracle {ref[k, c]:.10g} '
                  f'abs {nll[k, c] - ref[k, c]:.3g} gross {gross[k, 0]:.4g}; candidates above 3e-6: '
                  f'{sorted(set(np.nonzero(rel > 3e-6)[1].tolist()))} keypoints: {len(set(np.nonzero(rel > 3e-6)[0].tolist()))}', flush=True)
    # smoother
    s = np.exp(rng.uniform(-8, 8, K))
    if window:
        knob('EKS_SMOOTH_WINDOW', '2')       # lanes the windowed kernel does not store itself come back as NaN
        nan = np.isnan(hip_ops.smooth(tg._dev(y_tk), tg._dev(var_tk), *tg._params_dev(arrs), tg._dev(s), flags=flags,
                                      vs_diag=True)[0].cpu().numpy().reshape(T, K * D))
        lanes = np.stack([nan[g:g + WIN_GROUP].all(axis=0) for g in range(0, T, WIN_GROUP)])
        assert np.array_equal(np.repeat(lanes, WIN_GROUP, axis=0)[:T], nan), (case, 'a window group is stored as a whole')
        knob('EKS_SMOOTH_WINDOW', '0')
        ms0, Vs0 = [a.cpu().numpy() for a in hip_ops.smooth(tg._dev(y_tk), tg._dev(var_tk), *tg._params_dev(arrs),
                                                            tg._dev(s), flags=flags, vs_diag=True)]
        knob('EKS_SMOOTH_WINDOW', '1')
    ms, Vs = hip_ops.smooth(tg._dev(y_tk), tg._dev(var_tk), *tg._params_dev(arrs), tg._dev(s), flags=flags, vs_diag=True)
    if window:
        d10 = max(float(np.abs(ms.cpu().numpy() - ms0).max()), float(np.abs(Vs.cpu().numpy() - Vs0).max()))
        assert np.isfinite(d10), (case, 'mode 1 left a lane unwritten or not finite')
    ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2)); Vs = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2))
    mo, Vo = orc.info_form_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, Rd)[:2]
    # scale of a keypoint: its smoothed track or its observations in state units, whichever is larger
    # (a float32 pipeline cannot resolve an output of 0.03 px better than ~1e-7 of 3 px inputs)
    cdiag = np.abs(np.diagonal(arrs['Cs'], axis1=1, axis2=2))[:, None, :]
    scale_k = np.maximum(np.abs(mo).max(axis=(1, 2), keepdims=True), (np.abs(arrs['ys']) / cdiag).max(axis=(1, 2), keepdims=True))
    # ... or the prior mean, another float32 input of the same arithmetic (seed 77 case 15: two frames with |y| = 0.005
    # beside m0 = -0.67: 4e-8 absolute read 9.5e-6 against |y| alone)
    scale_k = np.maximum(scale_k, np.abs(arrs['m0s']).max(axis=1)[:, None, None])
    rel_ms = np.abs(ms - mo) / np.maximum(scale_k, 1e-3)
    e_ms = float(rel_ms.max())
    if os.environ.get('FUZZ_DETAIL') and e_ms > 3e-6:
        k, t, d_ = np.unravel_index(np.argmax(rel_ms), rel_ms.shape)
        print(f'   detail ms: keypoint {k} frame {t} coord {d_}: gpu {ms[k, t, d_]:.9g} oracle {mo[k, t, d_]:.9g} scale {scale_k[k, 0, 0]:.4g} '
              f's={s[k]:.4g} y={arrs["ys"][k, :3, d_]} var={var_tk[:3, k, d_]} m0={arrs["m0s"][k]} S0={np.diagonal(arrs["S0s"][k])} '
              f'a={np.diagonal(arrs["As"][k])} c={np.diagonal(arrs["Cs"][k])} q={np.diagonal(arrs["Qs"][k])}; '
              f'entries above 3e-6: {int((rel_ms > 3e-6).sum())}', flush=True)
    Vd = np.diagonal(Vo, axis1=2, axis2=3)
    rel_Vs = np.abs(Vs - Vd) / Vd
    e_Vs = float(rel_Vs.max())
    if os.environ.get('FUZZ_DETAIL') and e_Vs > 3e-6:
        k, t, d_ = np.unravel_index(np.argmax(rel_Vs), rel_Vs.shape)
        t0_, t1_ = max(0, t - 2), min(T, t + 3)
        print(f'   detail Vs: case {case} T={T} K={K} keypoint {k} frame {t} coord {d_}: gpu {Vs[k, t, d_]:.9g} oracle {Vd[k, t, d_]:.9g} '
              f's={s[k]:.6g} var[t-2..t+2]={var_tk[t0_:t1_, k, d_]} S0={np.diagonal(arrs["S0s"][k])} a={np.diagonal(arrs["As"][k])} '
              f'c={np.diagonal(arrs["Cs"][k])} q={np.diagonal(arrs["Qs"][k])}; entries above 3e-6: {int((rel_Vs > 3e-6).sum())} '
              f'in keypoints {sorted(set(np.nonzero(rel_Vs > 3e-6)[0].tolist()))[:8]} frames {sorted(set(np.nonzero(rel_Vs > 3e-6)[1].tolist()))[:12]}',
              flush=True)
    worst['nll'] = max(worst['nll'], e_nll); worst['ms'] = max(worst['ms'], e_ms); worst['Vs'] = max(worst['Vs'], e_Vs)
    flag = '' if max(e_nll, e_ms, e_Vs) < 1e-5 else '   <-- above 1e-5'
    if window:
        # the scan-based path on the same input, held to the same bar
        ms0 = np.transpose(ms0.astype(np.float64), (1, 0, 2)); Vs0 = np.transpose(Vs0.astype(np.float64), (1, 0, 2))
        e0_ms, e0_Vs = float((np.abs(ms0 - mo) / np.maximum(scale_k, 1e-3)).max()), float((np.abs(Vs0 - Vd) / Vd).max())
        flag = flag or ('' if max(e0_ms, e0_Vs) < 1e-5 else '   <-- above 1e-5')
        n_stored += int((~lanes).sum()); n_lanes += lanes.size
        print(f'case {case}: T={T} K={K} D={D} unit={unit} var x{scale:.3g}: windowed ms {e_ms:.1e} Vs {e_Vs:.1e}, scan-based '
              f'ms {e0_ms:.1e} Vs {e0_Vs:.1e}, stored {int((~lanes).sum())} of {lanes.size} lanes '
              f'({100.0 * (~lanes).mean():.0f} %), max |windowed - scan-based| {d10:.3g}{flag}', flush=True)
        continue
    print(f'case {case}: T={T} K={K} unit={unit} var x{scale:.3g} n_cand={n_cand}: nll {e_nll:.1e} ms {e_ms:.1e} Vs {e_Vs:.1e}{flag}', flush=True)
if window:
    print(f'stored lanes {n_stored} of {n_lanes}')
print('worst', worst)
