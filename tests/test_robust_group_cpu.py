"""CPU: eks_smooth_robust_group without a GPU - the variational bound of tests/robust_group_ref.py against its
term-by-term evaluation from the joint Gaussian posterior, its monotonicity over 32 passes, the reference's consistency
(g = 1 is tests/robust_ref.py, the dense form on a diagonal model is the scalar one, large nu is the Gaussian smoother),
the demonstration session, the float32 lane arithmetic of eks_amd/csrc/eks_smooth_student_lane.hpp run from plain
loops by the stand-alone tests/host_sim/robust_group_sim.cpp (plain and under -fsanitize=address,undefined; never loaded
into this process), the C ABI's refusals and the Python argument checks.

Float32 bar (robust_group_ref.bars), the project's rule: error / scale <= max(1e-5, 4 x the float32 NumPy
transcription's own worst error / scale on the same run) for ms, Vs and weights; change, a maximum over the difference
of two weight planes, is held to twice the weights' bar (robust_group_ref.bars derives it).  The transcription is the
yardstick, never the simulator.

Recorded (float64): bound against its direct evaluation 2.2e-16 (D, O, g = 2, 2, 2), 2.1e-16 (2, 4, 2), 2.9e-16
(3, 6, 3) relative; smallest step of the bound over 32 passes, seeds 0..7, -2.3e-12 (of bounds near -2e3: rounding at
convergence); g = 1 against robust_ref 0; dense against scalar reference 6.2e-15; nu = 1e12 against the Gaussian
smoother 5.0e-11.  Demonstration session (T = 600, twenty frames displaced by 2.5 .. 4 sd in both coordinates, nu = 4,
8 passes, seeds 0..7; g = 1 | g = 2): RMSE to the truth 0.346 - 0.385 | 0.342 - 0.379 (Gaussian 0.357 - 0.385); mean weight
on displaced frames 0.38 - 0.47 | 0.22 - 0.31, on clean frames 1.04 - 1.05 | 1.06 - 1.08; frames marked (weight <= 0.3;
g = 1: both coordinates) 1 - 5 | 12 - 18 of 20, g = 1 in at least one coordinate 10 - 16; clean frames marked 0 - 1 | 0.
Host simulator, worst error / scale over all cases (transcription's worst on that case): UNIT ms 2.0e-7 (1.0e-7), Vs
2.7e-5 (2.3e-5), weights 4.5e-5 (3.4e-5), change 2.1e-5 (2.1e-5); a = 0.98, c = 1.3: ms 6.3e-7 (2.3e-7), Vs 5.8e-5
(5.2e-5), weights 7.5e-5 (6.6e-5), change 5.4e-5 (3.6e-5)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import innovations_ref as nref  # noqa: E402
import robust_group_ref as gref  # noqa: E402
import robust_ref as rref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402

PARAMS = ('m0', 'S0', 'A', 'C', 'Q', 's')
SEEDS = tuple(range(8))


# ---- the bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,O,g', [(2, 2, 2), (2, 4, 2), (3, 6, 3)])
def test_bound_formula_against_its_terms_from_the_joint_posterior(D, O, g):
    T, K, nu = 6, 2, 4.0
    M = dense_case(K, D, O, False, seed=D + O)
    rng = np.random.default_rng(O)
    y = rng.normal(size=(T, K, O)) * 2
    y[3, :, :g] += 6.0                                                       # one group displaced together
    var = np.exp(rng.normal(0.0, 0.7, (T, K, O)))
    par = tuple(M[k] for k in PARAMS)
    hist = []
    gref.dense_robust_group(y, var, *par, nu, g, 4, history=hist)
    worst = 0.0
    for i in (1, 3):
        lam, _ = hist[i]
        delta_prev = hist[i - 1][1]
        assert np.allclose(lam, (nu + g) / (nu + gref.group_sums(delta_prev, g)), rtol=1e-14)
        ll = nref.dense_innovations_sequential(y, rref._clip(var) / gref.expand(lam, g), *par)['loglik']
        got = gref.elbo(ll, delta_prev, nu, g)
        for k in range(K):
            want = gref.elbo_direct(y[:, k], var[:, k], *(p[k] for p in par), nu, g, delta_prev[:, k])
            worst = max(worst, abs(got[k] - want) / abs(want))
    print(f'D={D} O={O} g={g}: bound against its direct evaluation {worst:.3g}')
    assert worst < 1e-9


@pytest.fixture(scope='module')
def demo():
    """The demonstration session, seeds 0..7, as eight keypoints of one problem, under g = 1 and g = 2."""
    S = [gref.joint_session(seed) for seed in SEEDS]
    y, var, x = (np.concatenate([s[k] for s in S], axis=1) for k in ('y', 'var', 'x'))
    bad = np.stack([s['bad'] for s in S], axis=1)                            # [T][K]
    N = 2 * len(S)
    args = (np.zeros(N), np.full(N, 100.0), 1.0, 1.0, np.full(N, 0.05))
    out = dict(y=y, var=var, x=x, bad=bad, args=args)
    out['gauss'] = gref.scalar_robust_group(y, var, *args, 4.0, 2, 2, 1)
    for g in (1, 2):
        out[g] = gref.scalar_robust_group(y, var, *args, 4.0, g, 2, 8)
    return out


def test_bound_never_drops_over_32_passes(demo):
    path = gref.scalar_elbo_path(demo['y'], demo['var'], *demo['args'], 4.0, 2, 2, 32)
    steps = np.diff(path, axis=0)
    print(f'smallest step of the bound over 32 passes, seeds {SEEDS}: {steps.min():+.3g}')
    assert np.all(steps >= -1e-9 * np.abs(path[1:]))


# ---- the reference against the references it generalises -------------------------------------------------------------
def test_group_of_one_is_the_per_coordinate_reference():
    pb = make_session(150, 3, 2, 2.0, False, seed=5, centre=3.0)
    pb['y'][::37] += 30.0
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], 4.0)
    want = rref.scalar_robust(*args, 8)
    got = gref.scalar_robust_group(*args, 1, pb['D'], 8)
    worst = max(np.abs(got[i] - want[i]).max() for i in range(3))
    worst = max(worst, np.abs(got[3] - want[3].reshape(pb['K'], pb['D']).max(axis=1)).max())
    T, K, D = pb['T'], pb['K'], pb['D']
    dn = gref.dense_robust_group(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS),
                                 4.0, 1, 8)
    dw = rref.dense_robust(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS), 4.0, 8)
    worst = max(worst, max(np.abs(dn[i] - dw[i]).max() for i in range(4)))
    print(f'g = 1 against robust_ref: {worst:.3g}')
    assert worst < 1e-12


@pytest.mark.parametrize('D,g', [(2, 2), (6, 3), (6, 2)])
def test_dense_reference_on_a_diagonal_model_is_the_scalar_one(D, g):
    pb = make_session(150, 3, D, 2.0, False, seed=5, centre=3.0)
    T, K = pb['T'], pb['K']
    pb['y'][::37] += 6.0
    sc = gref.scalar_robust_group(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], 4.0, g, D, 8)
    dn = gref.dense_robust_group(pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), *(pb['par'][k] for k in PARAMS),
                                 4.0, g, 8)
    worst = max(np.abs(dn[0].reshape(T, -1) - sc[0]).max() / np.abs(pb['y']).max(),
                np.abs(np.diagonal(dn[1], axis1=2, axis2=3).reshape(T, -1) / sc[1] - 1).max(),
                np.abs(dn[2].reshape(T, -1) - sc[2]).max(), np.abs(dn[3] - sc[3]).max())
    print(f'dense against scalar reference, D={D} g={g}: {worst:.3g}')
    assert worst < 1e-10


def test_large_nu_is_the_gaussian_smoother(demo):
    y, var, args = demo['y'], demo['var'], demo['args']
    ms, Vs, lam, _ = gref.scalar_robust_group(y, var, *args, 1e12, 2, 2, 8)
    gm, gV = demo['gauss'][:2]
    worst = max(np.abs(ms - gm).max() / np.abs(y).max(), (np.abs(Vs - gV) / gV).max(), np.abs(lam - 1).max())
    print(f'nu = 1e12, 8 passes, against the Gaussian smoother: {worst:.3g}')
    assert worst < 1e-8


def test_continuation_pass_count_in_the_reference(demo):
    """n1 passes then n2 passes from the returned weights are one call of n1 + n2 - 1 passes."""
    y, var, args = demo['y'][:200], demo['var'][:200], demo['args']
    whole = gref.scalar_robust_group(y, var, *args, 4.0, 2, 2, 8)
    first = gref.scalar_robust_group(y, var, *args, 4.0, 2, 2, 3)
    cont = gref.scalar_robust_group(y, var, *args, 4.0, 2, 2, 6, lam0=first[2])
    for a, b in zip(whole, cont):
        assert np.array_equal(a, b)


def test_unobserved_coordinates_leave_the_group():
    """A coordinate at the variance ceiling is no evidence: a group with nothing observed keeps weight 1, a group with
    one coordinate left is that coordinate's own Student-t factor."""
    s = gref.joint_session(3, T=60, n_bad=4)
    var = s['var'].copy()
    var[10:20] = np.inf
    var[30:40, 1] = 1e30
    ms, Vs, lam, _ = gref.scalar_robust_group(s['y'], var, *s['args'], 4.0, 2, 2, 8)
    assert np.all(lam[10:20] == 1.0)
    assert np.all(lam > 0) and np.all(lam <= 1.5) and np.all(lam[30:40] <= 1.25)


# ---- the demonstration session -----------------------------------------------------------------------------------------
def demo_figures(demo, res1, res2):
    """Per seed: RMSE to the truth, mean weight on displaced / clean frames, frames marked (weight <= 0.3)."""
    x, bad = demo['x'], demo['bad']
    K = bad.shape[1]
    rmse = lambda ms: np.sqrt(((ms - x) ** 2).reshape(len(x), K, 2).mean(axis=(0, 2)))
    l1, l2 = res1[2].reshape(len(x), K, 2), res2[2]
    fig = dict(rmse1=rmse(res1[0]), rmse2=rmse(res2[0]))
    for name, fn in (('bad', lambda a, k: a[bad[:, k], k]), ('clean', lambda a, k: a[~bad[:, k], k])):
        fig[name + '1'] = np.array([fn(l1, k).mean() for k in range(K)])
        fig[name + '2'] = np.array([fn(l2, k).mean() for k in range(K)])
        fig[name + '_marked1_both'] = np.array([(fn(l1, k) <= 0.3).all(axis=1).sum() for k in range(K)])
        fig[name + '_marked1_any'] = np.array([(fn(l1, k) <= 0.3).any(axis=1).sum() for k in range(K)])
        fig[name + '_marked2'] = np.array([(fn(l2, k) <= 0.3).sum() for k in range(K)])
    return fig


def test_one_weight_per_keypoint_marks_the_jointly_displaced_frames(demo):
    """What the float64 reference shows on all eight seeds, each threshold a factor 2 inside its worst seed: g = 2 marks
    12 - 18 of the twenty frames (asserted: >= 6), at least 9 more than g = 1 marks in both coordinates (>= 4); its mean
    weight on the displaced frames is 0.22 - 0.31 (<= 0.62), at most 0.67 of g = 1's (<= 0.83); clean frames keep a
    mean weight of 1.06 or more (>= 0.53) and none is marked."""
    f = demo_figures(demo, demo[1], demo[2])
    g = np.sqrt(((demo['gauss'][0] - demo['x']) ** 2).reshape(len(demo['x']), -1, 2).mean(axis=(0, 2)))
    for k, v in f.items():
        print(k, np.round(v, 3))
    print('rmse gauss', np.round(g, 3))
    assert np.all(f['bad_marked2'] >= 6)
    assert np.all(f['bad_marked2'] - f['bad_marked1_both'] >= 4)
    assert np.all(f['bad2'] <= 0.62) and np.all(f['bad2'] <= 0.83 * f['bad1'])
    assert np.all(f['clean2'] >= 0.53) and not f['clean_marked2'].any()


# ---- the lane header from plain loops: a stand-alone program -----------------------------------------------------------
def _build_sim(path, extra):
    subprocess.run(['g++', '-std=c++17', *extra, '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'host_sim', 'robust_group_sim.cpp'), '-o', path], check=True)
    return path


@pytest.fixture(scope='module')
def sims(tmp_path_factory):
    d = tmp_path_factory.mktemp('robust_group_sim')
    return dict(dir=d, plain=_build_sim(str(d / 'robust_group_sim'), ['-O2']),
                san=_build_sim(str(d / 'robust_group_sim_san'),
                               ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']))


@pytest.mark.parametrize('which', ['plain', 'san'])
def test_simulator_self_check(sims, which):
    """n_iters = 1 is bit for bit the smooth_tv bodies at w = 1, weights 1 and change 0; a middle pass rewrites every
    entry of a poisoned contribution plane; 2 and 8 passes finite and in range; 3 then 6 passes are the bits of 8 - on
    buffers of exactly the reported size, plain and under AddressSanitizer + UBSan."""
    r = subprocess.run([sims[which]], capture_output=True, text=True)
    assert r.returncode == 0 and 'robust_group_sim: ok' in r.stdout, r.stdout + r.stderr


def run_sim(sims, which, pb, B, nu, g, n_iters, lam0=None):
    T, N, D, K = pb['T'], pb['N'], pb['D'], pb['K']
    fin, fout = str(sims['dir'] / 'in.bin'), str(sims['dir'] / 'out.bin')
    par = pb['par']
    with open(fin, 'wb') as f:
        f.write(np.array([T, N, D, g, B, int(pb['unit']), n_iters, int(lam0 is not None)], np.int32).tobytes())
        f.write(np.array([nu], np.float64).tobytes())
        for a in (pb['y'], pb['var']) + (() if lam0 is None else (lam0,)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        for k in PARAMS:
            f.write(np.ascontiguousarray(par[k], np.float64).tobytes())
    r = subprocess.run([sims[which], fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(fout, np.float32)
    TN, TG = T * N, T * N // g
    assert out.size == 2 * TN + TG + K
    return (out[:TN].reshape(T, N), out[TN:2 * TN].reshape(T, N), out[2 * TN:2 * TN + TG].reshape(T, N // g),
            out[2 * TN + TG:])


def displace_jointly(pb, seed, g):
    """About 2 % of the (frame, group)s moved in all g coordinates at once, by 3 .. 8 px each (var is 0.5 .. 4)."""
    rng = np.random.default_rng(seed)
    T, N = pb['y'].shape
    hit = np.repeat(rng.random((T, N // g)) < 0.02, g, axis=1)
    pb['y'] = (pb['y'] + hit * rng.choice([-1.0, 1.0], hit.shape) * rng.uniform(3, 8, hit.shape)).astype(np.float32)
    return pb


@pytest.mark.parametrize('unit', [True, False])
def test_host_simulator_meets_the_float32_bar(sims, unit):
    worst = {}
    cases = [(T, B) for T in (1, 2, 5, 31, 32, 33, 129, 1000) for B in (4, 8, 16, 32)]
    for i, (T, B) in enumerate(cases):
        K, (D, g) = 3, ((2, 2), (6, 3), (6, 2))[i % 3]
        pb = displace_jointly(make_session(T, K, D, 2.0, unit, seed=i), i, g)
        nu = (1.0, 4.0, 30.0)[(i // 3) % 3]
        args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu, g, D)
        for n_iters in (2, 8):
            ref = gref.scalar_robust_group(*args, n_iters)
            r32 = gref.scalar_robust_group_f32(*args, n_iters, unit=unit)
            bars = gref.bars(r32, ref, pb['y'])
            got = run_sim(sims, 'san' if i % 8 == 0 else 'plain', pb, B, nu, g, n_iters)
            err, et = gref.errors(got, ref, pb['y']), gref.errors(r32, ref, pb['y'])
            for k in err:
                e = float(np.max(err[k]))
                if e > worst.get(k, (0.0, 0.0))[0]:
                    worst[k] = (e, float(np.max(et[k])))
                assert e <= bars[k], f'{k}: {e:.3g} over the bar {bars[k]:.3g} at T={T} B={B} nu={nu} g={g} n_iters={n_iters}'
            assert np.all(got[2] > 0) and np.all(got[2] <= np.float32((nu + g) / nu))
    print(f'unit={unit}: host simulator worst error / scale (transcription on that case): '
          + ', '.join(f'{k} {v[0]:.2g} ({v[1]:.2g})' for k, v in worst.items()))


def test_simulator_single_pass_under_given_weights_is_the_smoother_on_var_over_weights(sims):
    pb = make_session(200, 3, 2, 2.0, True, seed=3)
    lam = np.random.default_rng(0).uniform(0.05, 1.5, (200, 3)).astype(np.float32)
    ms, Vs, out_lam, change = run_sim(sims, 'plain', pb, 32, 4.0, 2, 1, lam0=lam)
    assert np.array_equal(out_lam, lam) and not change.any()
    args = (pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], np.ones(200))
    lam_o = gref.expand(lam, 2)
    rms, rVs = tref.scalar_smooth_tv(pb['y'], pb['var'].astype(np.float64) / lam_o, *args)
    bars = tref.f32_bars(*tref.scalar_smooth_tv_f32(pb['y'], (pb['var'] * (np.float32(1) / lam_o)), *args, unit=True),
                         rms, rVs, pb['y'])
    err = tref.f32_errors(ms, Vs, rms, rVs, pb['y'])
    assert float(err['ms'].max()) <= bars['ms'] and float(err['Vs'].max()) <= bars['Vs']


# ---- the C ABI's refusals (returned before anything touches a device) ------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_c_abi_refusals_need_no_device(lib):
    """Every defect of tests/test_api_refusals_cpu.py's block for eks_smooth_robust, handed to eks_smooth_robust and to
    eks_smooth_robust_group (group = 2, and group = 1, which forwards): equal statuses, none from the runtime; then the
    group's own."""
    from eks_amd import _lib
    import test_api_refusals_cpu as tab
    buf = ctypes.create_string_buffer(64)
    one, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    dref = lambda dims: None if dims is None else ctypes.byref(_lib.EksDims(*dims))

    def call(group, dims, ws=one, ws_bytes=1 << 40, **over):
        v = dict(nu=4.0, n_iters=8, weights=null, weights_in=0, change=null, **{k: one for k in tab.MODEL + ['ms', 'Vs']})
        for k, x in over.items():
            assert k in v
            v[k] = null if x is None else x
        model = [v[k] for k in tab.MODEL]
        rest = (v['n_iters'], v['weights'], v['weights_in'], v['change'], v['ms'], v['Vs'], ws, ws_bytes, None)
        if group is None:
            return int(lib.eks_smooth_robust(dref(dims), *model, v['nu'], *rest))
        return int(lib.eks_smooth_robust_group(dref(dims), *model, v['nu'], group, *rest))

    def query(group, dims):
        if group is None:
            return int(lib.eks_smooth_robust_workspace_bytes(dref(dims)))
        return int(lib.eks_smooth_robust_group_workspace_bytes(dref(dims), group))

    chain_T = tab._first_refused_T(lib, 1 << 22, 2, 2, tab.DIAG | tab.VSD)
    dense_T = tab._first_refused_T(lib, 5000000, 3, 4, 0)
    chain_limit, dense_limit = (1 << 22, chain_T, 2, 2, tab.DIAG | tab.VSD), (5000000, dense_T, 3, 4, 0)
    shapes = dict(chains=tab.CHAINS, chains_no_vs_diag=tab.CHAINS[:4] + (tab.DIAG,), general=tab.GENERAL,
                  **tab.UNSUPPORTED_DIMS, **tab.BAD_DIMS, chain_limit=chain_limit, dense_limit=dense_limit)
    defects = []                                                             # (dims, kwargs)
    for dims in tab.BAD_DIMS.values():
        defects += [(dims, {}), (dims, dict(y=None))]
    defects += [(dims, {}) for dims in tab.UNSUPPORTED_DIMS.values()]
    defects += [(chain_limit, {}), (chain_limit[:1] + (chain_T - 1,) + chain_limit[2:], dict(ws=null)),
                (dense_limit, {}), (dense_limit[:1] + (dense_T - 1,) + dense_limit[2:], dict(ws=null))]
    for dims in (tab.CHAINS, tab.GENERAL):
        defects += [(dims, {a: None}) for a in tab.MODEL + ['ms', 'Vs']]
        defects += [(dims, dict(ws=null)), (dims, dict(y=None, ws=null))]
        for nu in (0.0, -1.0, float('inf'), float('nan')):
            defects += [(dims, dict(nu=nu)), (dims, dict(nu=nu, y=None))]
        defects += [(dims, dict(n_iters=0)), (dims, dict(n_iters=0, Vs=None)), (dims, dict(weights_in=1)),
                    (dims, dict(weights_in=1, s=None)), (dims, dict(weights_in=1, ws=null))]
    for group in (2, 1):
        for name, dims in shapes.items():
            assert (query(group, dims) > 0) == (query(None, dims) > 0), (group, name)
        for dims, kw in defects:
            want, got = call(None, dims, **kw), call(group, dims, **kw)
            assert got == want and tab.EKS_ERR_HIP_BASE < got < 0, (group, dims, kw, got, want)
        for dims in (tab.CHAINS, tab.GENERAL):                               # the size, tested in the entry
            need = query(group, dims)
            assert call(group, dims, ws_bytes=need - 1) == -4 and call(group, dims, ws=null, ws_bytes=need - 1) == -4
    # the group's own: below 1, or no divisor of O - behind the shapes, in front of everything else
    for dims in (tab.GENERAL, (3, 20, 4, 4, tab.DIAG | tab.VSD)):            # O = 4
        for group in (0, -1, 3):
            assert query(group, dims) == 0
            assert call(group, dims) == -2 and call(group, dims, y=None) == -2 and call(group, dims, ws=null) == -2
        assert query(2, dims) > 0 and query(4, dims) > 0
    assert call(0, tab.BAD_DIMS['unit_without_diag']) == -3                  # the shapes come first
    assert call(3, tab.UNSUPPORTED_DIMS['D7']) == -3
    # sizes: eks_smooth_robust's with the narrower plane, plus the contribution plane on scalar chains
    plane = lambda n: (n * 4 + 255) // 256 * 256
    tvb = lambda dims: int(lib.eks_smooth_tv_workspace_bytes(dref(dims)))
    assert query(2, tab.CHAINS) == tvb(tab.CHAINS) + plane(20 * 3) + plane(20) + plane(20 * 6)
    assert query(2, tab.GENERAL) == tvb(tab.GENERAL) + plane(20 * 3 * 2)
    assert query(1, tab.CHAINS) == query(None, tab.CHAINS) and query(1, tab.GENERAL) == query(None, tab.GENERAL)


# ---- the Python surface's argument checks (raised before a device is asked for) --------------------------------------
def test_python_argument_checks():
    import eks_amd
    from eks_amd import robust
    for name in ('smooth_robust_grouped', 'smooth_singlecam_robust_grouped', 'smooth_multicam_robust'):
        assert getattr(eks_amd, name) is getattr(robust, name)
    K, T, D = 2, 6, 2
    eye = np.tile(np.eye(D), (K, 1, 1))
    args = (np.zeros((K, T, D)), np.zeros((K, D)), eye, eye, eye, eye, np.ones((T, K, D)), 1.0)
    for kw in (dict(group=0), dict(group=-1), dict(group=3), dict(group=1.5), dict(group=2, nu=0.0),
               dict(group=2, nu=np.nan), dict(group=2, n_iters=0), dict(group=2, tol=0.0),
               dict(group=2, tol=1e-3, max_iters=4), dict(group=2, tol=1e-3, n_iters=1)):
        with pytest.raises(ValueError):
            robust.smooth_robust_grouped(*args, **kw)
    with pytest.raises(TypeError):
        robust.smooth_robust_grouped(*args)                                  # group has no default
    with pytest.raises(ValueError):
        robust.smooth_robust_grouped(args[0], args[1], eye, eye, eye, eye, np.ones((T + 1, K, D)), 1.0, group=2)
    from eks_amd.marker_array import MarkerArray
    ma = MarkerArray(np.zeros((2, 1, T, K, 3)), data_fields=['x', 'y', 'likelihood'])
    with pytest.raises(ValueError):
        robust.smooth_singlecam_robust_grouped(ma, ['a'], 1.0)
    with pytest.raises(ValueError):
        robust.smooth_singlecam_robust_grouped(ma, ['a', 'b'], 1.0, nu=0.0)
    ma2 = MarkerArray(np.zeros((2, 2, T, K, 3)), data_fields=['x', 'y', 'likelihood'])
    with pytest.raises(ValueError):
        robust.smooth_singlecam_robust_grouped(ma2, ['a', 'b'], 1.0)
    with pytest.raises(ValueError):
        robust.smooth_multicam_robust(ma2, ['a'], ['c0', 'c1'], 1.0, avg_mode='median', var_mode='var')
    with pytest.raises(ValueError):
        robust.smooth_multicam_robust(ma2, ['a', 'b'], ['c0'], 1.0, avg_mode='median', var_mode='var')
    with pytest.raises(ValueError):
        robust.smooth_multicam_robust(ma2, ['a', 'b'], ['c0', 'c1'], 1.0, avg_mode='median', var_mode='var', nu=-1.0)
