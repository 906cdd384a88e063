"""CPU: the float32 lane arithmetic of the scalar-chain kernels, compiled for the host from the
SAME headers the gfx950 kernels include (eks_amd/csrc/eks_diag_lane.hpp, eks_nll_lane.hpp), against
the float64 oracle.  This pins the chunked-scan / three-regime numerics without a GPU; the kernels
themselves are tested under -m gpu.  (tests/host_sim is test infrastructure: eks_amd never loads it.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import eks_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'diag_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libdiag_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _problem(T, K, seed):
    from eks_amd import synth
    arrs = orc.singlecam_arrays(synth.singlecam_markers(T, K, seed=seed))
    y = np.ascontiguousarray(np.transpose(arrs['ys'], (1, 0, 2)).reshape(T, 2 * K).astype(np.float32))
    var = np.ascontiguousarray(arrs['ensemble_vars'].reshape(T, 2 * K).astype(np.float32))
    for k in ('m0s', 'S0s', 'As', 'Cs', 'Qs'):
        arrs[k] = np.ascontiguousarray(arrs[k], dtype=np.float64)
    ys64 = np.transpose(y.reshape(T, K, 2), (1, 0, 2)).astype(np.float64)
    ev64 = np.swapaxes(var.reshape(T, K, 2).astype(np.float64), 0, 1)
    return arrs, y, var, ys64, ev64


@pytest.mark.parametrize('B', [8, 32, 64])
@pytest.mark.parametrize('sval', [np.exp(-8.0), 0.3, 10.0, np.exp(8.0)])
def test_float32_chunked_smoother_matches_oracle(sim, B, sval):
    T, K = 1500, 5
    arrs, y, var, ys64, ev64 = _problem(T, K, seed=2)
    s = np.full(K, sval)
    ms = np.empty((T, 2 * K), np.float32)
    Vd = np.empty((T, 2 * K), np.float32)
    f, d = ctypes.c_float, ctypes.c_double
    rc = sim.sim_diag_smooth(T, 2 * K, 2, B, 1, _p(y, f), _p(var, f), _p(arrs['m0s'], d), _p(arrs['S0s'], d),
                             _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d), _p(s, d), _p(ms, f), _p(Vd, f))
    assert rc == 0
    ms_o, Vs_o, _ = orc.kalman_smoother(ys64, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'],
                                        s, orc.build_R_from_vars(ev64))
    ms_k = np.transpose(ms.reshape(T, K, 2), (1, 0, 2))
    Vd_k = np.transpose(Vd.reshape(T, K, 2), (1, 0, 2))
    assert (np.abs(ms_k - ms_o) / np.abs(ms_o).max(axis=(1, 2), keepdims=True)).max() < 2e-6
    Vo = np.diagonal(Vs_o, axis1=2, axis2=3)
    assert (np.abs(Vd_k - Vo) / Vo).max() < 3e-6


def _heavy_smoothing_problem(T, K, unit, seed=7):
    """Little process noise under a lot of observation noise (s q / r ~ 1e-5 ... 1e-3) and, for the general diagonal
    model, transitions that decay at a comparable rate (1 - a ~ 1e-2): the smoother's gain sits within 1e-2 of one."""
    rng = np.random.default_rng(seed + int(unit))
    y = (np.cumsum(rng.standard_normal((T, 2 * K)), axis=0) * 0.3 + 100).astype(np.float32)
    var = (rng.gamma(2.0, 0.5, (T, 2 * K)) * np.exp(rng.uniform(-1, 3, 2 * K))).astype(np.float32)
    eye = np.tile(np.eye(2), (K, 1, 1))
    a = np.ones((K, 2)) if unit else rng.uniform(0.9, 1.0, (K, 2))
    c = np.ones((K, 2)) if unit else rng.uniform(0.5, 1.1, (K, 2))
    q = np.ones((K, 2)) if unit else rng.uniform(0.5, 1.6, (K, 2))
    arrs = dict(As=np.ascontiguousarray(eye * a[:, :, None]), Cs=np.ascontiguousarray(eye * c[:, :, None]),
                Qs=np.ascontiguousarray(eye * q[:, :, None]), m0s=np.ascontiguousarray(y[0].reshape(K, 2).astype(np.float64)),
                S0s=np.ascontiguousarray(eye * rng.uniform(10, 6000, (K, 2))[:, :, None]))
    s = np.exp(rng.uniform(-8, -5.5, K))
    return arrs, y, var, s


@pytest.mark.parametrize('unit', [True, False])
def test_float32_smoother_under_heavy_smoothing_keeps_a_margin(sim, unit):
    """VERDICT r05 item 5.  The fuzz sweeps' worst smoothed variance (6.5e-6 of the 1e-5 bar, profiles/r05_fuzz3.txt) came
    from s ~ 5e-4: the RTS gain G = a Pf / Pp is then within 1e-2 of one, a float32 G carries 1 - G to 6e-8 / (1 - G) of
    itself and the variance recursion's fixed point divides by 1 - G^2; on decaying chains a float32 `a` biases the
    filter's fixed point the same way.  Round 6: the step in its deviation form where 1 - G is small (eks_math.hpp:
    rts_step), a x and a^2 X as x - (1 - a) x, X - (1 - a^2) X with the complements rounded once from float64.
    3.1e-6 / 2.6e-6 before on this problem; the bar here is 3e-6 on every frame."""
    T, K = 4097, 40
    arrs, y, var, s = _heavy_smoothing_problem(T, K, unit)
    ms = np.empty((T, 2 * K), np.float32)
    Vd = np.empty((T, 2 * K), np.float32)
    f, d = ctypes.c_float, ctypes.c_double
    rc = sim.sim_diag_smooth(T, 2 * K, 2, 32, int(unit), _p(y, f), _p(var, f), _p(arrs['m0s'], d), _p(arrs['S0s'], d),
                             _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d), _p(s, d), _p(ms, f), _p(Vd, f))
    assert rc == 0
    ys64 = np.transpose(y.reshape(T, K, 2), (1, 0, 2)).astype(np.float64)
    ev64 = np.maximum(np.swapaxes(var.reshape(T, K, 2).astype(np.float64), 0, 1), 1e-12)
    mo, Vo = orc.info_form_smoother(ys64, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, ev64)[:2]
    Vo = np.diagonal(Vo, axis1=2, axis2=3)
    Vk = np.transpose(Vd.reshape(T, K, 2), (1, 0, 2))
    mk = np.transpose(ms.reshape(T, K, 2), (1, 0, 2))
    assert (np.abs(Vk - Vo) / Vo).max() < 3e-6
    assert (np.abs(mk - mo) / np.abs(mo).max(axis=(1, 2), keepdims=True)).max() < 2e-6


@pytest.mark.parametrize('T,BN', [(3003, 512), (3003, 2048), (600, 4096), (9001, 2048), (12500, 3136)])
def test_float32_three_regime_nll_and_dual_gradient(sim, T, BN):
    K = 3
    arrs, y, var, ys64, ev64 = _problem(T, K, seed=5)
    Rc = orc.constant_R_from_timevarying(orc.build_R_from_vars(ev64))
    cand = np.exp(np.linspace(-8, 8, 16))
    ref = [orc.filter_nll(ys64, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'],
                          np.full(K, sc), Rc, want_grad=True) for sc in cand]
    ref_nll = np.stack([r[0] for r in ref], axis=1)
    ref_g = np.stack([r[1] for r in ref], axis=1)
    rconst = np.ascontiguousarray(Rc.reshape(-1))
    f, d = ctypes.c_float, ctypes.c_double
    for grad in (0, 1, 2):    # 0: converged-entry summaries allowed for chunks j >= 1; 2: exact entry
        nll = np.zeros((K, 16))
        dn = np.zeros((K, 16))
        sim.sim_diag_nll(T, 2 * K, 2, BN, 1, grad, _p(y, f), _p(rconst, d), _p(arrs['m0s'], d), _p(arrs['S0s'], d),
                         _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d), _p(cand, d), 16, 0,
                         _p(nll, d), _p(dn, d))
        assert (np.abs(nll - ref_nll) / np.abs(ref_nll)).max() < 1e-5
        np.testing.assert_array_equal(nll.argmin(axis=1), ref_nll.argmin(axis=1))
        if grad == 1:
            assert (np.abs(dn - ref_g) / np.abs(ref_g).max(axis=1, keepdims=True)).max() < 2e-5


@pytest.mark.parametrize('T,B0,BN,unit,var_scale', [(9001, 1024, 1600, True, 1.0), (12500, 1024, 1600, False, 1.0),
                                                    (7000, 1024, 512, True, 1.0), (4000, 512, 1600, True, 1.0),
                                                    (20000, 1024, 3200, False, 1.0), (12000, 1024, 512, True, 20.0),
                                                    (12000, 1024, 1600, False, 300.0)])
def test_grid_kernel_lane_bodies_head_plus_lean_match_oracle(sim, T, B0, BN, unit, var_scale):
    """diag_nll_grid_kernel's arithmetic on the host (round 4): chunk 0 through the general lane body at 4 candidates
    per lane, chunks j >= 1 through nll_lean_chunk at 16 candidates per lane - converged entry, the constants from
    lean_const - with the exact-entry fallback where a chunk does not qualify (the slowest candidates in short
    chunks, or too early in the sequence), all 64 candidates of BASELINE's grid.  NLL within 1e-5 of the float64
    oracle, argmin bit-exact; most units must really take the lean path."""
    K, NC = 3, 64
    arrs, y, var, ys64, ev64 = _problem(T, K, seed=6)
    ev64 = ev64 * var_scale          # large R: poles near one - early chunks fall back to exact entry, rho^t outlives
    if not unit:                     # short chunks (the lean summary then keeps A = rho^len)
        rng = np.random.default_rng(3)
        eye = np.eye(2)
        arrs['As'] = np.ascontiguousarray(eye * rng.uniform(0.93, 1.0, (K, 2))[:, :, None])
        arrs['Cs'] = np.ascontiguousarray(eye * rng.uniform(0.6, 1.4, (K, 2))[:, :, None])
        arrs['Qs'] = np.ascontiguousarray(eye * rng.uniform(0.5, 2.0, (K, 2))[:, :, None])
    Rc = orc.constant_R_from_timevarying(orc.build_R_from_vars(ev64))
    cand = np.exp(np.linspace(-8, 8, NC))
    from oracle import c_oracle          # the C twin: 64 candidates x 20 000 frames in NumPy would take minutes
    ref = c_oracle.nll_grid(ys64, Rc, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], cand)
    spot = orc.filter_nll(ys64, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], np.full(K, cand[5]), Rc)
    assert (np.abs(ref[:, 5] - spot) / np.abs(spot)).max() < 1e-10
    rconst = np.ascontiguousarray(Rc.reshape(-1))
    f, d = ctypes.c_float, ctypes.c_double
    nll = np.zeros((K, NC))
    n_lean = ctypes.c_int(0)
    sim.sim_diag_nll_lean(T, 2 * K, 2, B0, BN, int(unit), _p(y, f), _p(rconst, d), _p(arrs['m0s'], d),
                          _p(arrs['S0s'], d), _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d), _p(cand, d), NC,
                          _p(nll, d), ctypes.byref(n_lean))
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-5
    np.testing.assert_array_equal(nll.argmin(axis=1), ref.argmin(axis=1))
    units = 2 * K * (NC // 16) * (0 if T <= B0 else (T - B0 + BN - 1) // BN)
    assert n_lean.value >= (0.7 if var_scale == 1.0 else 0.3) * units, (n_lean.value, units)


@pytest.mark.parametrize('T,B0,BN,unit,var_scale,min_lag', [
    (9001, 1024, 1600, True, 1.0, 0.7), (12500, 1024, 1600, False, 1.0, 0.7), (20000, 1024, 3200, False, 1.0, 0.7),
    (12000, 1024, 512, True, 20.0, 0.5), (12000, 1024, 1600, False, 300.0, 0.1), (7000, 1024, 1024, True, 0.05, 0.7)])
def test_grid_kernel_shared_lag_form_matches_oracle(sim, T, B0, BN, unit, var_scale, min_lag):
    """The shared-lag form of the grid kernel (round 5, eks_nll_lag.hpp) on the host: the candidates whose steady-state
    pole is below lag_rho_max (0.345 for 16 lags) are summarised from the chunk's 16 lag sums and its first / last 16
    inputs in float64 (lag_summary), the others run nll_lag_chunk's recursion in four "waves" that take turns at the
    lag products; chunks that do not qualify keep the round-4 lane bodies.  NLL within 1e-5 of the float64 oracle on
    all 64 candidates, argmin bit-exact, the FAST candidates (grid indices 40 and up: poles below 0.2 at these
    variances) within 1e-7 - the lag form is the more accurate of the two; most chunks must really take it."""
    K, NC = 3, 64
    arrs, y, var, ys64, ev64 = _problem(T, K, seed=6)
    ev64 = ev64 * var_scale
    if not unit:
        rng = np.random.default_rng(3)
        eye = np.eye(2)
        arrs['As'] = np.ascontiguousarray(eye * rng.uniform(0.93, 1.0, (K, 2))[:, :, None])
        arrs['Cs'] = np.ascontiguousarray(eye * rng.uniform(0.6, 1.4, (K, 2))[:, :, None])
        arrs['Qs'] = np.ascontiguousarray(eye * rng.uniform(0.5, 2.0, (K, 2))[:, :, None])
    Rc = orc.constant_R_from_timevarying(orc.build_R_from_vars(ev64))
    cand = np.exp(np.linspace(-8, 8, NC))
    from oracle import c_oracle
    ref = c_oracle.nll_grid(ys64, Rc, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], cand)
    rconst = np.ascontiguousarray(Rc.reshape(-1))
    f, d = ctypes.c_float, ctypes.c_double
    nll = np.zeros((K, NC))
    n_lag = ctypes.c_int(0)
    sim.sim_diag_nll_lag(T, 2 * K, 2, B0, BN, int(unit), _p(y, f), _p(rconst, d), _p(arrs['m0s'], d),
                         _p(arrs['S0s'], d), _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d), _p(cand, d), NC,
                         _p(nll, d), ctypes.byref(n_lag))
    err = np.abs(nll - ref) / np.abs(ref)
    assert err.max() < 1e-5
    np.testing.assert_array_equal(nll.argmin(axis=1), ref.argmin(axis=1))
    units = 2 * K * (0 if T <= B0 else (T - B0 + BN - 1) // BN)
    assert n_lag.value >= min_lag * units, (n_lag.value, units)
    if var_scale <= 1.0:
        assert err[:, 48:].max() < 1e-7, err[:, 48:].max()


@pytest.mark.parametrize('T,BN,unit', [(6000, 392, True), (6000, 392, False), (3001, 256, True), (5000, 1000, False)])
def test_gradient_without_compositions_matches_oracle(sim, T, BN, unit):
    """gf_conv_body of diag_nll_grad_fused_kernel (round 5): chunk 0 applied to the prior, every later chunk by its
    converged-entry summary with d / d log s (nll_conv_chunk_dual), the terms summed - against the oracle's value and
    gradient.  Keypoints whose poles outlive a chunk do not qualify and are skipped (the kernel keeps the tree)."""
    K = 12
    arrs, y, var, ys64, ev64 = _problem(T, K, seed=9)
    rng = np.random.default_rng(4)
    if not unit:
        eye = np.eye(2)
        arrs['As'] = np.ascontiguousarray(eye * rng.uniform(0.9, 1.0, (K, 2))[:, :, None])
        arrs['Cs'] = np.ascontiguousarray(eye * rng.uniform(0.5, 1.5, (K, 2))[:, :, None])
        arrs['Qs'] = np.ascontiguousarray(eye * rng.uniform(0.5, 2.0, (K, 2))[:, :, None])
        arrs['m0s'] = np.ascontiguousarray(rng.standard_normal((K, 2)))
    Rc = orc.constant_R_from_timevarying(orc.build_R_from_vars(ev64))
    rconst = np.ascontiguousarray(Rc.reshape(-1))
    s = np.exp(np.linspace(-5.5, 6, K))
    ref_nll, ref_g = orc.filter_nll(ys64, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, Rc, want_grad=True)
    f, d = ctypes.c_float, ctypes.c_double
    nll = np.zeros(K)
    dn = np.zeros(K)
    n_ok = sim.sim_diag_nll_conv_grad(T, 2 * K, 2, BN, int(unit), _p(y, f), _p(rconst, d), _p(arrs['m0s'], d),
                                      _p(arrs['S0s'], d), _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d),
                                      _p(s, d), _p(nll, d), _p(dn, d))
    ok = ~np.isnan(nll)
    assert n_ok == ok.sum() and n_ok >= K - 4, n_ok
    assert (np.abs(nll[ok] - ref_nll[ok]) / np.abs(ref_nll[ok])).max() < 3e-6
    assert (np.abs(dn[ok] - ref_g[ok]) / np.maximum(np.abs(ref_g[ok]), 1e-3 * np.abs(ref_nll[ok]))).max() < 2e-5


@pytest.fixture(scope='module')
def sim_packed():
    """The same simulator with the lane bodies' PACKED forms (what the GPU runs: float32 pairs in 64-bit registers) - they
    are written with clang's vector extensions, so this build needs ROCm's clang++ (it is host code: no GPU involved)."""
    cxx = '/opt/rocm/lib/llvm/bin/clang++'
    if not os.path.exists(cxx):
        pytest.skip('no clang++ under /opt/rocm')
    src = os.path.join(ROOT, 'tests', 'host_sim', 'diag_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libdiag_sim_packed.so')
    subprocess.run([cxx, '-O0', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=fast', '-DEKS_NLL_PACKED=1', '-I',
                    os.path.join(ROOT, 'eks_amd', 'csrc'), src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


@pytest.mark.parametrize('unit', [True, False])
def test_packed_dual_lane_bodies_match_the_oracle_like_the_scalar_ones(sim, sim_packed, unit):
    """Round 5's packed (value, derivative) forms - regime 1 and the steady loop of the gradient lane, the converged-entry
    chunk with d / d log s - built for the host: against the oracle at the scalar forms' bars, and within float32 rounding
    of the scalar forms themselves (same operations, possibly contracted differently by the two compilers)."""
    T, BN, K = 6000, 392, 6
    arrs, y, var, ys64, ev64 = _problem(T, K, seed=21)
    rng = np.random.default_rng(8)
    if not unit:
        eye = np.eye(2)
        arrs['As'] = np.ascontiguousarray(eye * rng.uniform(0.9, 1.0, (K, 2))[:, :, None])
        arrs['Cs'] = np.ascontiguousarray(eye * rng.uniform(0.5, 1.5, (K, 2))[:, :, None])
        arrs['Qs'] = np.ascontiguousarray(eye * rng.uniform(0.5, 2.0, (K, 2))[:, :, None])
    Rc = orc.constant_R_from_timevarying(orc.build_R_from_vars(ev64))
    rconst = np.ascontiguousarray(Rc.reshape(-1))
    s = np.exp(np.linspace(-6.5, 5, K))           # slow poles (regime 1 lasts hundreds of frames) to fast ones
    ref_nll, ref_g = orc.filter_nll(ys64, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, Rc, want_grad=True)
    f, d = ctypes.c_float, ctypes.c_double
    out = {}
    for name, lib in (('scalar', sim), ('packed', sim_packed)):
        nll, dn = np.zeros((K, 1)), np.zeros((K, 1))
        sk = np.ascontiguousarray(s[:, None])
        lib.sim_diag_nll(T, 2 * K, 2, BN, int(unit), 1, _p(y, f), _p(rconst, d), _p(arrs['m0s'], d), _p(arrs['S0s'], d),
                         _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d), _p(sk, d), 1, 1, _p(nll, d), _p(dn, d))
        nll2, dn2 = np.zeros(K), np.zeros(K)
        lib.sim_diag_nll_conv_grad(T, 2 * K, 2, BN, int(unit), _p(y, f), _p(rconst, d), _p(arrs['m0s'], d),
                                   _p(arrs['S0s'], d), _p(arrs['As'], d), _p(arrs['Cs'], d), _p(arrs['Qs'], d),
                                   _p(s, d), _p(nll2, d), _p(dn2, d))
        out[name] = (nll[:, 0], dn[:, 0], nll2, dn2)
        assert (np.abs(nll[:, 0] - ref_nll) / np.abs(ref_nll)).max() < 3e-6
        assert (np.abs(dn[:, 0] - ref_g) / np.maximum(np.abs(ref_g), 1e-3 * np.abs(ref_nll))).max() < 3e-5
    for a, b in zip(out['scalar'], out['packed']):
        ok = ~np.isnan(a)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert (np.abs(a[ok] - b[ok]) / np.maximum(np.abs(a[ok]), 1e-3 * np.abs(ref_nll[ok]))).max() < 2e-6


def test_lag_sum_identity_is_exact_with_all_lags():
    """sum_t d_t^2 of the zero-start recursion d_t = rho d_{t-1} + u_t equals
    [c_0 + 2 sum_k rho^k c_k - rho^2 d_last^2] / (1 - rho^2) with c_k the lag sums of u - the identity the lag form
    truncates at 16 lags (eks_nll_lag.hpp); and sum_t d_t rho^t = [sum_i rho^i u_i - rho^(L+1) d_last] / (1 - rho^2)."""
    rng = np.random.default_rng(0)
    L = 300
    u = rng.normal(size=L)
    for rho in (0.05, 0.3, 0.7, 0.95):
        dd = np.zeros(L)
        acc = 0.0
        for t in range(L):
            acc = rho * acc + u[t]
            dd[t] = acc
        c = np.array([np.dot(u[k:], u[:L - k]) for k in range(L)])
        s0 = (c[0] + 2 * np.sum(rho ** np.arange(1, L) * c[1:]) - rho ** 2 * dd[-1] ** 2) / (1 - rho ** 2)
        assert abs(s0 - np.sum(dd ** 2)) < 1e-9 * np.sum(dd ** 2)
        s1 = (np.sum(rho ** np.arange(L) * u) - rho ** (L + 1) * dd[-1]) / (1 - rho ** 2)
        assert abs(s1 - np.sum(dd * rho ** np.arange(L))) < 1e-9 * max(1.0, abs(s1))


# ---------------------------------------------------------------------------------------------
# general (D, O) smoother: chunk elements -> scan -> exact replay, from the kernels' own headers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dense_sim():
    src = os.path.join(ROOT, 'tests', 'host_sim', 'dense_sim.cpp')
    lib = os.path.join(ROOT, 'tests', 'host_sim', 'libdense_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    src, '-o', lib], check=True)
    return ctypes.CDLL(lib)


@pytest.mark.parametrize('case', ['plain', 'all_clipped', 'tiny', 'one_clipped'])
@pytest.mark.parametrize('sval', [10.0, 1e-3])
def test_dense_chunked_smoother_matches_oracle_also_at_the_variance_clip(dense_sim, case, sval):
    """Predict-first chunk elements keep the boundary algebra well-scaled when an ensemble variance
    sits at the 1e-12 clip (an element that opened with such an observation gave smoothed means
    off by 1e7).  Frames entirely at tiny variances are checked against the information-form
    oracle: the covariance-form recursion itself is only good to 1e-2 there (cond(S) ~ 1e9)."""
    rng = np.random.default_rng(11)
    T, K, D, O, B = 700, 2, 3, 4, 32
    x = np.cumsum(rng.standard_normal((K, T, D)) * 0.7, axis=1)
    C = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((K, O, D)))[0])
    var = (0.25 * rng.gamma(2.0, 1.0, (T, K, O))).clip(1e-3).astype(np.float32)
    if case == 'all_clipped':
        var[2::9] = 0.0
    elif case == 'tiny':
        var[::5] = 1e-8
    elif case == 'one_clipped':
        var[::7, :, 1] = 0.0
    y = np.ascontiguousarray((np.einsum('kod,ktd->tko', C, x)
                              + rng.standard_normal((T, K, O)) * np.sqrt(np.maximum(var, 1e-12))).astype(np.float32))
    L = rng.standard_normal((K, D, D)) * 0.3
    Q = L @ np.swapaxes(L, 1, 2) + 0.2 * np.eye(D)
    m0, S0, A = np.zeros((K, D)), np.tile(4 * np.eye(D), (K, 1, 1)), np.tile(np.eye(D), (K, 1, 1))
    s = np.full(K, sval)
    ms = np.zeros((T, K, D), np.float32)
    Vs = np.zeros((T, K, D, D), np.float32)
    v = ctypes.c_void_p
    p = lambda a: a.ctypes.data_as(v)      # noqa: E731
    assert dense_sim.sim_dense_smooth(T, K, D, O, B, p(y), p(var), p(m0), p(S0), p(A), p(C), p(Q), p(s),
                                      p(ms), p(Vs)) == 0
    ys = np.swapaxes(y, 0, 1).astype(np.float64)
    Rd = np.maximum(np.swapaxes(var.astype(np.float64), 0, 1), 1e-12)
    if case in ('plain', 'one_clipped'):
        ms_o, Vs_o = orc.kalman_smoother(ys, m0, S0, A, C, Q, s, Rd)[:2]
    else:
        ms_o, Vs_o = orc.info_form_smoother(ys, m0, S0, A, C, Q, s, Rd)[:2]
    ms_k, Vs_k = np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1)
    assert (np.abs(ms_k - ms_o) / np.abs(ms_o).max(axis=(1, 2), keepdims=True)).max() < 1e-6
    assert (np.abs(Vs_k - Vs_o) / np.abs(Vs_o).max(axis=1, keepdims=True)).max() < 1e-6


@pytest.mark.parametrize('D,O', [(6, 64), (1, 1)])
def test_dense_chunked_smoother_at_the_accepted_limits_matches_oracle(dense_sim, D, O):
    """The lane bodies of eks_dense_lane.hpp at the widest and the narrowest model the library accepts (D = 6 with
    O = 64, D = O = 1), at the bars of the test above; T = 70 in 16-frame chunks: a ragged last chunk of 6."""
    rng = np.random.default_rng(100 * D + O)
    T, K, B = 70, 3, 16
    x = np.cumsum(rng.standard_normal((K, T, D)) * 0.7, axis=1)
    C = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((K, O, D)))[0])
    var = (0.25 * rng.gamma(2.0, 1.0, (T, K, O))).clip(1e-3).astype(np.float32)
    y = np.ascontiguousarray((np.einsum('kod,ktd->tko', C, x) + rng.standard_normal((T, K, O)) * np.sqrt(var)
                              ).astype(np.float32))
    L = rng.standard_normal((K, D, D)) * 0.3
    Q = L @ np.swapaxes(L, 1, 2) + 0.2 * np.eye(D)
    m0, S0 = np.zeros((K, D)), np.tile(4 * np.eye(D), (K, 1, 1))
    A = np.tile(np.eye(D), (K, 1, 1)) * 0.97 + 0.02 * rng.standard_normal((K, D, D))
    s = np.exp(rng.uniform(-3, 3, K))
    ms = np.zeros((T, K, D), np.float32)
    Vs = np.zeros((T, K, D, D), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert dense_sim.sim_dense_smooth(T, K, D, O, B, p(y), p(var), p(m0), p(S0), p(A), p(C), p(Q), p(s),
                                      p(ms), p(Vs)) == 0
    ys = np.swapaxes(y, 0, 1).astype(np.float64)
    Rd = np.maximum(np.swapaxes(var.astype(np.float64), 0, 1), 1e-12)
    ms_o, Vs_o = orc.kalman_smoother(ys, m0, S0, A, C, Q, s, Rd)[:2]
    ms_k, Vs_k = np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1)
    assert (np.abs(ms_k - ms_o) / np.abs(ms_o).max(axis=(1, 2), keepdims=True)).max() < 1e-6
    assert (np.abs(Vs_k - Vs_o) / np.abs(Vs_o).max(axis=1, keepdims=True)).max() < 1e-6


@pytest.mark.parametrize('D,O,general_A', [(3, 4, False), (2, 2, True), (4, 8, False),
                                          # the accepted limits of the general path (D <= 6, O <= 64), odd O past 32
                                          (1, 1, False), (1, 33, True), (1, 64, False), (5, 1, True), (5, 33, False),
                                          (5, 64, True), (6, 1, False), (6, 33, True), (6, 64, False)])
def test_dense_loss_and_log_s_sensitivity_match_oracle(dense_sim, D, O, general_A):
    """eks_nll on the general path: predict-first chunk elements, D pseudo-observations per frame,
    tree composition, dual-number d/dlog s - against the oracle's filter and forward sensitivity."""
    rng = np.random.default_rng(D * 10 + O)
    T, K, B = 900, 3, 8
    x = np.cumsum(rng.standard_normal((K, T, D)) * 0.5, axis=1)
    C = rng.standard_normal((K, O, D))
    # (contiguous: einsum chooses its output's strides, and astype keeps them - the simulator takes a plain pointer)
    y = np.ascontiguousarray((np.einsum('kod,ktd->tko', C, x) + rng.standard_normal((T, K, O)) * 0.7).astype(np.float32))
    L = rng.standard_normal((K, D, D)) * 0.3
    Q = L @ np.swapaxes(L, 1, 2) + 0.2 * np.eye(D)
    A = np.tile(np.eye(D), (K, 1, 1))
    if general_A:
        A = A * 0.97 + 0.02 * rng.standard_normal((K, D, D))
    m0, S0 = rng.standard_normal((K, D)), np.tile(3.0 * np.eye(D), (K, 1, 1))
    rconst = rng.uniform(0.2, 1.5, (K, O))
    s = np.exp(rng.uniform(-4, 3, K))
    nll, dn = np.zeros(K), np.zeros(K)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert dense_sim.sim_dense_nll(T, K, D, O, B, p(y), p(rconst), p(m0), p(S0), p(A), p(C), p(Q), p(s),
                                   p(nll), p(dn)) == 0
    ref, g = orc.filter_nll(np.swapaxes(y, 0, 1).astype(np.float64), m0, S0, A, C, Q, s, rconst, want_grad=True)
    np.testing.assert_allclose(nll, ref, rtol=1e-10)
    np.testing.assert_allclose(dn, g, rtol=1e-8, atol=1e-9 * np.abs(g).max())
