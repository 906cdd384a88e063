"""CPU: eks_sample_tv without a GPU - the law of the float64 reference (tests/sampling_tv_ref.py) under random planes,
which pins the w[t + 1] convention; the float32 lane arithmetic of eks_amd/csrc/eks_sample_tv_lane.hpp run from plain
loops (tests/host_sim/sample_tv_sim.cpp) against that reference for every chunk length; the stand-alone simulator
plain and under -fsanitize=address,undefined (never loaded into this process); the C ABI surface, every refusal
against tests/golden/sample_tv_refusals.json and the pairs of defects that fix their order; the workspace query.

Float32 bars as in tests/test_sampling_cpu.py: max(1e-5, 4 x the worst error of the float32 NumPy transcription on
the same inputs), on the deviations relative to the posterior sd; the raw figure against the transcription read
through the float32 output, and dev_error beyond the output's own rounding.  Nothing is compared with the kernels'
own output.

Every refusal row is returned before the first HIP call (eks_api.hip: eks_sample_tv; eks_sample_dense.hip:
dense_sample_tv's checks precede its first launch), so the pointers are small host buffers nobody dereferences.
`python tests/test_sampling_tv_cpu.py --record` rewrites the table from the library."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_ref as ref  # noqa: E402
import sampling_tv_ref as tvref  # noqa: E402
import smooth_tv_ref as stv  # noqa: E402
from test_sampling_cpu import _p, dense_model, dev_error, make_chains  # noqa: E402

TABLE = os.path.join(ROOT, 'tests', 'golden', 'sample_tv_refusals.json')
SIM_SRC = os.path.join(ROOT, 'tests', 'host_sim', 'sample_tv_sim.cpp')
CHUNKS = (4, 8, 12, 16, 20, 24, 28, 32)


# ---- planes for the parity tests (shared with tests/test_gpu_sampling_tv.py) --------------------------------------------
def make_planes(T, K, D, seed, per_keypoint, B=32, nu=4.0):
    """w float32 (T,) or (T, K): log-uniform in [0.2, 5] with 1e-3 on the first and 1e3 on the last step a chunk of B
    frames reads (frame t0 + i reads w[t0 + i + 1]) and NaN in row 0; lam float32 (T, K D) uniform in
    [0.05, (nu + 1) / nu] with entries at 1e-30 and at (nu + 1) / nu."""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(np.log(0.2), np.log(5.0), (T, K) if per_keypoint else (T,))).astype(np.float32)
    for t0 in range(0, T, B):
        if t0 + 1 < T:
            w[t0 + 1] = 1e-3
        if t0 + B < T:
            w[t0 + B] = 1e3
    w[0] = np.nan
    lam_max = np.float32((nu + 1.0) / nu)
    lam = rng.uniform(0.05, float(lam_max), (T, K * D)).astype(np.float32)
    hit = rng.random((T, K * D))
    lam[hit < 0.03] = 1e-30
    lam[hit > 0.97] = lam_max
    return w, np.minimum(lam, lam_max)


def set_ac(pb, a, c):
    """The chains of make_chains with every a and c replaced (y is re-centred on the new c)."""
    K, D = pb['K'], pb['D']
    y = pb['y'].astype(np.float64) / pb['c'] * c
    pb['a'], pb['c'] = np.full(pb['N'], float(a)), np.full(pb['N'], float(c))
    for name, v in (('A', a), ('C', c)):
        pb['par'][name] = np.zeros((K, D, D))
        pb['par'][name][:, np.arange(D), np.arange(D)] = v
    pb['y'] = np.ascontiguousarray(y, np.float32)
    return pb


def reference(pb, z, w, lam):
    """-> ms64, sd, e64, and the bars (bar, bar_raw) from the float32 transcription on the same inputs."""
    D = pb['D']
    _, Pf, ms64, Vs64, _ = tvref.scalar_filter_smoother(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'],
                                                        pb['qs'], w, lam, D)
    sd = np.sqrt(Vs64)
    e64 = tvref.scalar_deviations(Pf, pb['a'], pb['qs'], z, w, D)
    e32 = tvref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z, w, lam, D)
    trans = float(np.abs((e32 - e64) / sd).max())
    trans_out = float(np.abs((ref.read_through_f32_output(ms64, e32) - e64) / sd).max())
    return ms64, sd, e64, max(1e-5, 4 * trans), max(1e-5, 4 * trans_out), trans


def ms_error_and_bar(pb, ms, ms64, w, lam):
    """The means under planes are eks_smooth_tv's arithmetic and are held to its rule: the error over the
    scale of the chain's operands, under max(1e-5, 4 x the error of the float32 transcription of the filter and RTS
    pass on r_eff formed in float32, smooth_tv_ref.scalar_smooth_tv_f32).  The scale is the largest of the chain's
    |y|, |ms| and |m0|, the magnitudes float32 rounds: the sessions here hold a chain with s q = 0, whose smoothed
    mean is one weighted average of all T observations and can lie far below them - it owes eps |y|, not eps |ms| -
    and with one to three frames ms_0 = (1 - k c) m0 + k y is such a value too.  -> (error, bar)."""
    T, D = pb['T'], pb['D']
    wq = np.ones(T, np.float32) if w is None else np.where(np.isnan(w), np.float32(1), w)
    t_ms, _ = stv.scalar_smooth_tv_f32(pb['y'], tvref.r_eff(pb['var'], lam, np.float32), pb['m0f'], pb['S0d'], pb['a'],
                                       pb['c'], pb['qs'], wq, D, pb['unit'])
    scale = np.maximum(np.maximum(np.abs(pb['y'].astype(np.float64)).max(axis=0), np.abs(ms64).max(axis=0)),
                       np.abs(pb['m0f']))
    err = lambda m: float((np.abs(np.asarray(m, np.float64) - ms64) / scale).max())  # noqa: E731
    return err(ms), max(1e-5, 4 * err(t_ms))


# ---- the reference's own law -------------------------------------------------------------------------------------------
def test_reference_law_scalar_chains_under_random_planes():
    rng = np.random.default_rng(7)
    worst = 0.0
    for T, a, c in ((1, 1.0, 1.0), (2, 1.0, 1.0), (9, 1.0, 1.0), (14, 0.98, -1.3), (14, 0.9, 0.6)):
        var = np.exp(rng.normal(0.0, 1.0, T))
        w = np.exp(rng.uniform(np.log(0.1), np.log(1000.0), T)).astype(np.float32)
        lam = np.exp(rng.uniform(np.log(1e-3), np.log(1.5), T))
        S0, qs = 3.0, 0.7
        L = tvref.scalar_law_map(var, S0, a, c, qs, w, lam)
        r = tvref.r_eff(var, lam)
        S = tvref.joint_covariance(r[:, None], S0, a, c, 1.0, qs, w)
        worst = max(worst, ref.law_error(L, S))
        # the diagonal against smooth_tv_ref.joint_posterior, an independent construction under the same r
        _, Vs = stv.joint_posterior(np.zeros((T, 1)), r[:, None], np.zeros(1), [[S0]], [[a]], [[c]], [[1.0]], qs, w)
        assert np.abs(np.diag(S) / Vs[:, 0, 0] - 1).max() < 1e-10
        if T >= 9:
            # the convention is visible: G_t, sd_t read from w[t] instead of w[t + 1] is a different law
            shifted = tvref.scalar_deviations(
                tvref.scalar_filter_smoother(np.zeros((T, 1)), var[:, None], [0.0], [S0], [a], [c], [qs], w, lam[:, None])[1],
                [a], [qs], np.eye(T)[:, :, None], np.concatenate([w[:1], w[:-1]]))[:, :, 0].T
            assert ref.law_error(shifted, S) > 1e-3
    print(f'law of the float64 reference, scalar chains: {worst:.3g}')
    assert worst < 1e-12


def test_reference_law_dense_model_under_random_planes():
    D, O, T = 3, 4, 7
    M = dense_model(1, D, O, seed=5)
    rng = np.random.default_rng(8)
    var = np.exp(rng.normal(0.0, 0.7, (T, O)))
    w = np.exp(rng.uniform(np.log(0.1), np.log(1000.0), T)).astype(np.float32)
    lam = np.exp(rng.uniform(np.log(1e-3), np.log(1.5), (T, O))).astype(np.float32)
    L = tvref.dense_law_map(var, M['m0'][0], M['S0'][0], M['A'][0], M['C'][0], M['Q'][0], M['s'][0], w, lam)
    r = tvref.r_eff(var, lam, np.float32).astype(np.float64)
    S = tvref.joint_covariance(r, M['S0'][0], M['A'][0], M['C'][0], M['Q'][0], M['s'][0], w)
    err = ref.law_error(L, S)
    _, Vs = stv.joint_posterior(np.zeros((T, O)), r, M['m0'][0], M['S0'][0], M['A'][0], M['C'][0], M['Q'][0], M['s'][0], w)
    blocks = np.stack([S[t * D:(t + 1) * D, t * D:(t + 1) * D] for t in range(T)])
    assert np.abs(blocks - Vs).max() < 1e-10 * np.abs(Vs).max()
    print(f'law of the float64 reference, D={D} O={O}: {err:.3g}')
    assert err < 1e-9


# ---- the lanes from plain loops ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sim(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp('sample_tv_sim') / 'libsample_tv_sim.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    '-I', os.path.join(ROOT, 'tests', 'host_sim'), SIM_SRC, '-o', lib], check=True)
    return ctypes.CDLL(lib)


def run_sim(sim, pb, B, n_draws, noise, w=None, lam=None, gs=0):
    T, N, D = pb['T'], pb['N'], pb['D']
    ms = np.full((T, N), np.nan, np.float32)
    draws = np.full((n_draws, T, N), np.nan, np.float32)
    f, d = ctypes.c_float, ctypes.c_double
    par = pb['par']
    nz = np.ascontiguousarray(noise, np.float32)
    wq = None if w is None else np.ascontiguousarray(w, np.float32)
    lm = None if lam is None else np.ascontiguousarray(lam, np.float32)
    rc = sim.sim_sample_tv(T, N, D, B, gs, int(pb['unit']), _p(pb['y'], f), _p(pb['var'], f), _p(wq, f),
                           int(wq is not None and wq.ndim == 2), _p(lm, f), _p(par['m0'], d), _p(par['S0'], d),
                           _p(par['A'], d), _p(par['C'], d), _p(par['Q'], d), _p(par['s'], d), n_draws,
                           ctypes.c_ulonglong(0), 0, 0, _p(nz, f), _p(ms, f), _p(draws, f))
    assert rc == 0
    return ms, draws


@pytest.mark.parametrize('unit', [True, False])
@pytest.mark.parametrize('T,planes', [(2, 'both'), (37, 'both'), (37, 'w'), (37, 'lam'), (37, 'none'), (301, 'both_pk')])
def test_host_sim_matches_float64_reference_for_every_chunk_length(sim, T, planes, unit):
    K, D, S = 3, 2, 3
    pb = make_chains(T, K, D, 2.0, unit, seed=T + 3)
    if T > 2:
        pb['var'][T // 2, 1] = 1e30                                       # a missing frame
    z32 = np.random.default_rng(5).normal(size=(S, T, pb['N'])).astype(np.float32)
    for B in CHUNKS:
        w, lam = make_planes(T, K, D, seed=T + B, per_keypoint=planes == 'both_pk', B=B)
        w = w if planes in ('both', 'both_pk', 'w') else None
        lam = lam if planes in ('both', 'both_pk', 'lam') else None
        ms64, sd, e64, bar, bar_raw, trans = reference(pb, z32, w, lam)
        ms0, d0 = run_sim(sim, pb, B, S, np.zeros_like(z32), w, lam)
        assert np.array_equal(d0, np.broadcast_to(ms0, d0.shape))          # z = 0 returns the smoothed mean
        ms_err, bar_ms = ms_error_and_bar(pb, ms0, ms64, w, lam)
        assert ms_err < bar_ms
        ms, dr = run_sim(sim, pb, B, S, z32, w, lam, gs=3 if B == 8 else 0)
        assert np.array_equal(ms, ms0)
        err = dev_error(dr - ms[None], e64, dr, sd)
        raw = float(np.abs((dr - ms[None] - e64) / sd).max())
        print(f'T={T} planes={planes} unit={unit} B={B}: e/sd error {err:.3g} beyond the output rounding (transcription '
              f'{trans:.3g}, bar {bar:.3g}); raw {raw:.3g}, bar {bar_raw:.3g}')
        assert err < bar
        assert raw < bar_raw
        if planes == 'none':                                               # the plain sampler's reference, too
            _, Pf, _, _, _ = ref.scalar_filter_smoother(pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
            assert dev_error(dr - ms[None], ref.scalar_deviations(Pf, pb['a'], pb['qs'], z32), dr, sd) < bar


@pytest.mark.parametrize('which', ['plain', 'san'])
def test_host_simulator_stand_alone(which, tmp_path):
    """Exactly sized buffers through every chunk length, planes present and absent, NaN in w[0]; generator == injected."""
    extra = ['-O2'] if which == 'plain' else ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    exe = str(tmp_path / f'sample_tv_sim_{which}')
    subprocess.run(['g++', '-std=c++17', *extra, '-DSAMPLE_TV_SIM_MAIN', '-I', os.path.join(ROOT, 'eks_amd', 'csrc'),
                    '-I', os.path.join(ROOT, 'tests', 'host_sim'), SIM_SRC, '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'sample_tv_sim: ok' in r.stdout, r.stdout + r.stderr


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_entry_points_declared_bound_and_exported(lib):
    from eks_amd import _build, _lib
    header = open(os.path.join(ROOT, 'include', 'eks_hip.h')).read()
    for name in ('eks_sample_tv', 'eks_sample_tv_workspace_bytes'):
        assert name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert 'eks_sample_tv.hip' in _build.SOURCES
    assert '-fno-slp-vectorize' in _build.PER_FILE_FLAGS['eks_sample_tv.hip']
    import eks_amd
    for name in ('sample_singlecam_irregular', 'sample_singlecam_heavy_tailed', 'sample_multicam_robust'):
        assert callable(getattr(eks_amd, name))


DIAG, VSD, UNIT = 1, 2, 4
MODEL = ['y', 'var', 'm0', 'S0', 'A', 'C', 'Q', 's']
# the C order between dims and (workspace, workspace_bytes, stream); (name, None): may be NULL; (name, value): a scalar
ARGS = ['y', 'var', ('qscale', None), ('qscale_per_keypoint', 0), ('weights', None)] + MODEL[2:] + \
    [('n_draws', 2), ('seed', 0), ('first_keypoint', 0), ('first_draw', 0), ('noise', None), 'ms', 'draws']
CHAINS = (3, 20, 2, 2, DIAG | VSD)
GENERAL = (3, 20, 3, 4, 0)
BAD_DIMS = {'no_keypoints': (0, 20, 2, 2, 0), 'diag_D_ne_O': (3, 20, 2, 3, DIAG), 'unit_without_diag': (3, 20, 2, 2, UNIT),
            'null_dims': None}
SENTINEL = 7.25


def rows(lib):
    """{row id: status} of every refusal, in a fixed order; the outputs' sentinels are checked on the way."""
    from eks_amd import _lib
    from test_api_refusals_cpu import _first_refused_T
    buf = ctypes.create_string_buffer(64)
    one, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    ms = np.full(64, SENTINEL, np.float32)
    draws = np.full(64, SENTINEL, np.float32)
    out = {}

    def dims_ref(dims):
        return None if dims is None else ctypes.byref(_lib.EksDims(*dims))

    def query(dims, n_draws=2):
        return int(lib.eks_sample_tv_workspace_bytes(dims_ref(dims), n_draws))

    def call(dims, ws=one, ws_bytes=1 << 40, **over):
        args = []
        for a in ARGS:
            name, dflt = (a, one) if isinstance(a, str) else (a[0], null if a[1] is None else a[1])
            if name == 'ms':
                dflt = ctypes.c_void_p(ms.ctypes.data)
            if name == 'draws':
                dflt = ctypes.c_void_p(draws.ctypes.data)
            v = over.pop(name, dflt)
            args.append(null if v is None else v)
        assert not over, over
        rc = int(lib.eks_sample_tv(dims_ref(dims), *args, ws, ws_bytes, None))
        assert np.all(ms == SENTINEL) and np.all(draws == SENTINEL)
        return rc

    def row(rid, status):
        assert rid not in out, rid
        out[rid] = status

    chain_T = _first_refused_T(lib, 1 << 22, 2, 2, DIAG | VSD)
    dense_T = _first_refused_T(lib, 5000000, 3, 4, 0)
    chain_limit = (1 << 22, chain_T, 2, 2, DIAG | VSD)
    dense_limit = (5000000, dense_T, 3, 4, 0)
    d9 = (3, 20, 9, 9, DIAG)                                   # eks_smooth_tv: full Vs rows stop at D = 8
    wide = (1 << 20, 4, 3, 4, 0)                               # (n_draws + 1) K D > 2^24 at n_draws = 7
    shapes = dict(chains=CHAINS, chains_no_vs_diag=CHAINS[:4] + (DIAG,), general=GENERAL, D7=(3, 20, 7, 4, 0),
                  O65=(3, 20, 3, 65, 0), D9_chains_no_vs_diag=d9, D9_chains_vs_diag=d9[:4] + (DIAG | VSD,), **BAD_DIMS,
                  chain_limit=chain_limit, dense_limit=dense_limit)
    for name, dims in shapes.items():
        row(f'size|{name}', int(query(dims) > 0))
    for n in (0, -1):
        row(f'size|chains|n_draws={n}', int(query(CHAINS, n) > 0))
        row(f'size|general|n_draws={n}', int(query(GENERAL, n) > 0))
    row('size|wide|n_draws=7', int(query(wide, 7) > 0))
    row('size|wide|n_draws=4', int(query(wide, 4) > 0))
    row('size|wide|n_draws=0x7fffffff', int(query(wide, 0x7fffffff) > 0))
    for name, dims in BAD_DIMS.items():
        row(f'{name}', call(dims))
        row(f'{name}|y=NULL', call(dims, y=None))
        row(f'{name}|n_draws=0', call(dims, n_draws=0))
    for sname, dims in (('chains', CHAINS), ('general', GENERAL)):
        for a in ARGS:
            if isinstance(a, str) and a != 'ms':              # (ms may be NULL: that call would run)
                row(f'{sname}|{a}=NULL', call(dims, **{a: None}))
        row(f'{sname}|ws=NULL', call(dims, ws=null))
        row(f'{sname}|y=NULL,ws=NULL', call(dims, y=None, ws=null))
        row(f'{sname}|draws=NULL,ws=NULL', call(dims, draws=None, ws=null))
        row(f'{sname}|draws=NULL,s=NULL', call(dims, draws=None, s=None))
        need = query(dims)
        assert need > 1
        row(f'{sname}|ws_bytes=need-1', call(dims, ws_bytes=need - 1))
        row(f'{sname}|ws=NULL,ws_bytes=need-1', call(dims, ws=null, ws_bytes=need - 1))
        row(f'{sname}|draws=NULL,ws_bytes=need-1', call(dims, draws=None, ws_bytes=need - 1))
        for k in ('n_draws', 'first_keypoint', 'first_draw'):
            bad = 0 if k == 'n_draws' else -1
            row(f'{sname}|{k}={bad}', call(dims, **{k: bad}))
            row(f'{sname}|{k}={bad},y=NULL', call(dims, **{k: bad, 'y': None}))
            row(f'{sname}|{k}={bad},ws=NULL', call(dims, **{k: bad}, ws=null))
    # eks_sample's per-path refusals in its order, then eks_smooth_tv's shapes
    for name in ('D7', 'O65'):
        row(f'{name}', call(shapes[name]))
        row(f'{name}|ws_bytes=16', call(shapes[name], ws_bytes=16))
        row(f'{name}|y=NULL', call(shapes[name], y=None))
        row(f'{name}|ws=NULL', call(shapes[name], ws=null))
    row('wide|n_draws=7', call(wide, n_draws=7))
    row('wide|n_draws=7,ws_bytes=16', call(wide, n_draws=7, ws_bytes=16))
    row('wide|n_draws=0x7fffffff,ws_bytes=16', call(wide, n_draws=0x7fffffff, ws_bytes=16))
    row('chain_limit', call(chain_limit))
    row('chain_limit|ws_bytes=16', call(chain_limit, ws_bytes=16))
    row('chain_limit|draws=NULL', call(chain_limit, draws=None))
    row('dense_limit', call(dense_limit))
    row('dense_limit|ws=NULL', call(dense_limit, ws=null))
    row('D9_chains_no_vs_diag', call(d9))
    row('D9_chains_no_vs_diag|ws_bytes=16', call(d9, ws_bytes=16))
    row('D9_chains_no_vs_diag|Q=NULL', call(d9, Q=None))
    return out


def test_every_refusal_matches_the_recorded_table_and_leaves_the_outputs_alone(lib):
    with open(TABLE) as f:
        want = json.load(f)
    got = rows(lib)
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    for rid, status in got.items():
        assert status > -1000, f'{rid}: status {status} came from the HIP runtime'
        if not rid.startswith('size|'):
            assert status != 0, f'{rid}: a row must be refused, not run'
    wrong = {rid: (got[rid], want[rid]) for rid in got if got[rid] != want[rid]}
    assert not wrong, f'(got, recorded): {wrong}'
    # the order, stated here and not only recorded: eks_sample's refusals in eks_sample's order, then eks_smooth_tv's
    NULL, SHAPE, UNSUP, WS = -1, -2, -3, -4
    literal = {'null_dims': NULL, 'no_keypoints|y=NULL': SHAPE, 'chains|n_draws=0,y=NULL': SHAPE,
               'general|first_draw=-1,ws=NULL': SHAPE, 'chains|y=NULL,ws=NULL': NULL, 'chains|draws=NULL,ws=NULL': NULL,
               'general|draws=NULL,ws_bytes=need-1': NULL, 'chains|ws=NULL,ws_bytes=need-1': WS,
               'chains|ws_bytes=need-1': WS, 'general|ws_bytes=need-1': WS, 'D7': UNSUP, 'D7|ws_bytes=16': UNSUP,
               'D7|y=NULL': NULL, 'D7|ws=NULL': WS, 'wide|n_draws=7,ws_bytes=16': SHAPE, 'chain_limit': SHAPE,
               'chain_limit|ws_bytes=16': WS, 'dense_limit': SHAPE, 'D9_chains_no_vs_diag': UNSUP,
               'D9_chains_no_vs_diag|ws_bytes=16': WS, 'D9_chains_no_vs_diag|Q=NULL': NULL,
               'size|D9_chains_no_vs_diag': 0, 'size|D9_chains_vs_diag': 1, 'size|chain_limit': 0, 'size|dense_limit': 0,
               'size|wide|n_draws=7': 0, 'size|wide|n_draws=4': 1, 'size|chains|n_draws=0': 0, 'size|D7': 0}
    for rid, status in literal.items():
        assert got[rid] == status, (rid, got[rid], status)


def test_workspace_query_is_monotone_in_n_draws_and_zero_for_refused_shapes(lib):
    from eks_amd import _lib
    for dims in (CHAINS, GENERAL, (70, 1025, 3, 3, DIAG | VSD | UNIT), (5, 70, 6, 8, 0)):
        d = _lib.EksDims(*dims)
        sizes = [int(lib.eks_sample_tv_workspace_bytes(ctypes.byref(d), n)) for n in range(1, 40)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        if dims[4] & DIAG:                                      # scalar chains: eks_sample's workspace
            assert sizes == [int(lib.eks_sample_workspace_bytes(ctypes.byref(d), n)) for n in range(1, 40)]
    for dims in list(BAD_DIMS.values()) + [(3, 20, 7, 4, 0), (3, 20, 3, 65, 0), (3, 20, 9, 9, DIAG)]:
        d = None if dims is None else ctypes.byref(_lib.EksDims(*dims))
        assert int(lib.eks_sample_tv_workspace_bytes(d, 2)) == 0


def test_sample_kalman_posterior_validates_the_planes_before_any_device_call():
    from eks_amd.posterior import _sample_planes, sample_kalman_posterior
    K, T, O = 2, 5, 4
    w, lam = _sample_planes(np.ones((K, T)), np.full((K, T, 2), 0.5), K, T, O)
    assert w.shape == (T, K) and w.dtype == np.float32
    assert lam.shape == (T, K, O) and lam.dtype == np.float32 and np.all(lam == 0.5)
    g = np.arange(1, K * T * 2 + 1, dtype=np.float64).reshape(K, T, 2)
    _, lam = _sample_planes(None, g, K, T, O)                    # a grouped plane: coordinate o reads group o // 2
    assert np.array_equal(lam[:, :, 0], lam[:, :, 1]) and np.array_equal(lam[:, :, 2], lam[:, :, 3])
    assert np.array_equal(lam[:, :, ::2], np.swapaxes(g, 0, 1).astype(np.float32))
    wn = np.ones(T)
    wn[0] = np.nan
    assert _sample_planes(wn, None, K, T, O)[0][0] == 1.0        # row 0 is never read
    for bad_w in (np.ones(T + 1), np.full(T, -1.0), np.full(T, np.inf)):
        with pytest.raises(ValueError):
            _sample_planes(bad_w, None, K, T, O)
    for bad_l in (np.ones((K, T, 3)), np.zeros((K, T, O)), np.full((K, T, O), np.nan), np.ones((T, K, O)),
                  np.full((K, T, O), 1e-60)):
        with pytest.raises(ValueError):
            _sample_planes(None, bad_l, K, T, O)
    with pytest.raises(NotImplementedError):
        sample_kalman_posterior(np.zeros((K, T, 2)), np.zeros((K, 2)), np.eye(2)[None].repeat(K, 0),
                                np.eye(2)[None].repeat(K, 0), np.eye(2)[None].repeat(K, 0), np.eye(2)[None].repeat(K, 0),
                                np.ones((T, K, 2)), 1.0, 2, qscale=np.ones(T), h_fn=lambda x: x)


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, ROOT)
    from eks_amd import _lib as _l
    table = rows(_l.load())
    with open(TABLE, 'w') as f:
        json.dump(table, f, indent=0)
        f.write('\n')
    print(f'{len(table)} rows -> {TABLE}')
