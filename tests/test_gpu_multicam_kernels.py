"""GPU: the four kernels around the Kalman path of the multi-camera driver, each against a plain float64 reference of
the same operation (tests/multicam_ref.py, validated without a GPU by tests/test_multicam_ref_cpu.py), at small shapes
that run every template instantiation, the block tails and the refusals.

* eks_ensemble (ensemble_kernel<1..8, 16>): M = 1..16, both averages, both variances, 258 lanes and 1 lane, every count
  of valid members for x and y, against oracle.ensemble.  Bar: 1 float32 ulp of the float32-rounded oracle (every
  output is one float64 quantity rounded once; the median is one float32 addition and an exact halving); NaN
  positions and the nan_replacement / float32-max substitutions identical.
* eks_maha_inflate (maha_inflate_kernel<1..6>, 2..8 views): distances within multicam_ref.MAHA_BAR = 1.2e-9 relative
  (denominator floored at 1e-3): 100 x the 1.13e-11 by which the float64 reference itself differs from Gaussian
  elimination in np.longdouble on these inputs (measured by the CPU file).  The variances after the call bit for bit,
  the counts of inflated frames, inactive keypoints untouched.
* eks_multicam_tables (multicam_tables_kernel<1..6>, 1..8 views): pass-through columns and the latent table bit for
  bit; C m + mean and diag(C V C') + ev within 4 n 2^-53 sum |terms| (n additions: D + 1 and D^2 + D).
* eks_argmin_s: numpy.argmin bit for bit - ties, infinities and NaNs included (the first NaN wins).

Measured on the MI355X: the ensemble 0 ulp from the rounded oracle in every case; distances 1.9e-14 .. 9.0e-12 (worst at
(C, L) = (2, 3), N = 1000; 1.4e-22 at L = 2C).  Every printed figure is the kernel's distance from the reference."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multicam_ref as mr  # noqa: E402
from oracle import eks_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3
MODES = [(a, v) for a in ('median', 'mean') for v in ('confidence_weighted_var', 'var')]
SENTINEL = -4321.0


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _lib():
    from eks_amd import _lib as lib_mod
    return lib_mod.load()


def _stream():
    from eks_amd import hip_ops
    return hip_ops._stream()


# ---------------------------------------------------------------------------------------------------------------------
# eks_ensemble
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', range(1, 17))
def test_ensemble_every_member_count_within_one_ulp_of_the_oracle(M):
    """ensemble_kernel<M> for M <= 8, ensemble_kernel<16> for M = 9..16."""
    from eks_amd import hip_ops
    worst = 0.0
    for shape in mr.ENS_SHAPES:
        a = mr.ensemble_case(M, shape)
        for avg, var in MODES:
            got = hip_ops.ensemble(_dev(a), avg, var, mr.NAN_REP).cpu().numpy()
            ref = orc.ensemble(a, avg, var, mr.NAN_REP)[0]
            assert got.dtype == np.float32 and got.shape == ref.shape == (*shape, 5)
            with np.errstate(over='ignore'):
                r32 = ref.astype(np.float32)
            assert np.array_equal(np.isnan(got), np.isnan(r32)), (shape, avg, var)
            for sub in (np.float32(mr.NAN_REP), np.float32(mr.FMAX)):
                assert np.array_equal(got[..., 2:4] == sub, r32[..., 2:4] == sub), (shape, avg, var, sub)
            err = mr.f32_ulp_error(got, r32)
            worst = max(worst, err.max())
            lanes = np.argwhere(err > 1.0)
            assert err.max() <= 1.0, (shape, avg, var, lanes[:5], got[err > 1.0][:5], r32[err > 1.0][:5])
    print(f'M={M}: worst {worst:.0f} float32 ulp')


def test_ensemble_refusals_leave_the_output_alone():
    lib = _lib()
    V, T, K = 1, 3, 2
    mk = torch.rand((17, V, T, K, 3), dtype=torch.float32, device='cuda')
    out = torch.full((V, T, K, 5), SENTINEL, dtype=torch.float32, device='cuda')

    def call(M=2, V=V, T=T, K=K, markers=mk, avg=0, var=0, stats=out):
        return lib.eks_ensemble(M, V, T, K, _p(markers), avg, var, mr.NAN_REP, _p(stats), _stream())

    assert call(M=17) == ERR_UNSUPPORTED
    for kw in (dict(M=0), dict(V=0), dict(T=0), dict(K=0)):
        assert call(**kw) == ERR_SHAPE, kw
    assert call(markers=None) == ERR_NULL and call(stats=None) == ERR_NULL
    for kw in (dict(avg=2), dict(avg=-1), dict(var=2)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call(M=16) == 0                                   # (the same buffers are accepted)
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any()


# ---------------------------------------------------------------------------------------------------------------------
# eks_maha_inflate
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _maha_problem(C, L, K, N, seed, active):
    x, v, W, mu = mr.maha_case(C, L, K, N, seed)
    ref = mr.maha_inflate_ref(x, v, W, mu, None if active is None else np.array(active))
    return (x, v, W, mu), ref


def _maha_call(x, v, W, mu, active, want_maha):
    """The entry point itself on sentinel-filled outputs: (status, maha or None, v after, n_inflated)."""
    K, N, O = x.shape
    L = W.shape[-1]
    vd = _dev(v)
    maha = torch.full((K, N, O // 2), SENTINEL, dtype=torch.float64, device='cuda') if want_maha else None
    n_inf = torch.full((K,), 777, dtype=torch.int32, device='cuda')
    act = None if active is None else _dev(np.asarray(active, np.int32))
    xd, Wd, mud = _dev(x), _dev(W), _dev(mu)
    rc = _lib().eks_maha_inflate(K, N, O // 2, L, _p(xd), _p(vd), _p(Wd), _p(mud), _p(act), mr.MAHA_EPS,
                                 mr.MAHA_THRESHOLD, mr.MAHA_SCALAR, _p(maha), _p(n_inf), _stream())
    torch.cuda.synchronize()
    return rc, None if maha is None else maha.cpu().numpy(), vd.cpu().numpy(), n_inf.cpu().numpy()


def _check_maha(C, L, K, N, seed, active, want_maha):
    (x, v, W, mu), (ref, v_ref, n_ref) = _maha_problem(C, L, K, N, seed, active)
    rc, maha, v_got, n_got = _maha_call(x, v, W, mu, active, want_maha)
    assert rc == 0
    on = np.ones(K, bool) if active is None else np.array(active, bool)
    if want_maha:
        err = mr.maha_relative_error(maha[on], ref[on]).max()
        print(f'C={C} L={L} N={N}: distances {err:.2e} (bar {mr.MAHA_BAR:.1e})')
        assert err <= mr.MAHA_BAR
        assert (maha[~on] == SENTINEL).all()                 # an inactive keypoint's slice is not written
    assert np.array_equal(v_got, v_ref)                      # inflated where the reference inflates, bit for bit
    assert np.array_equal(v_got[~on], v[~on])
    assert np.array_equal(n_got, n_ref) and not n_got[~on].any()
    return n_got


@pytest.mark.parametrize('C,L', sorted(mr.MAHA_PAIRS))
def test_maha_inflate_every_latent_and_view_count(C, L):
    """maha_inflate_kernel<L> for L = 1..6 at 2..8 views; K = 3 keypoints with different W and mu, the middle one
    inactive; N = 130: three ballots in one block, the last partly filled."""
    n = _check_maha(C, L, mr.MAHA_K, mr.MAHA_N, mr.MAHA_PAIRS[(C, L)], (1, 0, 1), True)
    assert (n[[0, 2]] > 0).all() or L == 2 * C               # (3, 6): exact reconstruction, nothing inflates


@pytest.mark.parametrize('N', mr.MAHA_EDGE_N)
@pytest.mark.parametrize('C,L', mr.MAHA_EDGE_PAIRS)
def test_maha_inflate_frame_count_edges_all_active_and_without_distances(C, L, N):
    seed = mr.MAHA_EDGE_SEEDS.get((C, L, N), 0)
    _check_maha(C, L, mr.MAHA_K, N, seed, None, True)
    _check_maha(C, L, mr.MAHA_K, N, seed, None, False)       # maha = NULL


@pytest.mark.parametrize('column', [0, 3])
def test_maha_inflate_non_positive_pivot_gives_nan_and_inflates_nothing(column):
    C, L, K, N = 3, 4, mr.MAHA_K, mr.MAHA_N
    x, v, W, mu = mr.maha_case(C, L, K, N, mr.MAHA_PAIRS[(C, L)])
    W = W.copy()
    W[1, :, column] = 0.0                                    # W' P W of keypoint 1 has a zero row and column
    ref, v_ref, n_ref = mr.maha_inflate_ref(x, v, W, mu, np.array([1, 0, 1]))      # the other keypoints
    rc, maha, v_got, n_got = _maha_call(x, v, W, mu, None, True)
    assert rc == 0
    assert np.isnan(maha[1]).all() and np.array_equal(v_got[1], v[1]) and n_got[1] == 0
    assert mr.maha_relative_error(maha[[0, 2]], ref[[0, 2]]).max() <= mr.MAHA_BAR
    assert np.array_equal(v_got, v_ref) and np.array_equal(n_got, n_ref) and (n_got[[0, 2]] > 0).all()


def test_maha_inflate_refusals_leave_the_variances_alone():
    lib = _lib()
    K, N = 2, 5
    x = torch.rand((K, N, 18), dtype=torch.float64, device='cuda')
    W = torch.rand((K, 18, 7), dtype=torch.float64, device='cuda')
    mu = torch.rand((K, 18), dtype=torch.float64, device='cuda')
    v = torch.full((K, N, 18), 0.5, dtype=torch.float32, device='cuda')
    maha = torch.full((K, N, 9), SENTINEL, dtype=torch.float64, device='cuda')
    n_inf = torch.zeros(K, dtype=torch.int32, device='cuda')
    bufs = dict(x=x, v=v, W=W, mu=mu, n_inf=n_inf)

    def call(K=K, N=N, C=3, L=3, **null):
        b = {**bufs, **null}
        return lib.eks_maha_inflate(K, N, C, L, _p(b['x']), _p(b['v']), _p(b['W']), _p(b['mu']), None, mr.MAHA_EPS,
                                    mr.MAHA_THRESHOLD, mr.MAHA_SCALAR, _p(maha), _p(b['n_inf']), _stream())

    assert call(C=1) == ERR_UNSUPPORTED and call(C=9) == ERR_UNSUPPORTED and call(L=7) == ERR_UNSUPPORTED
    for kw in (dict(K=0), dict(N=0), dict(C=0), dict(L=0)):
        assert call(**kw) == ERR_SHAPE, kw
    for name in bufs:
        assert call(**{name: None}) == ERR_NULL, name
    torch.cuda.synchronize()
    assert (v == 0.5).all() and (maha == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# eks_multicam_tables
# ---------------------------------------------------------------------------------------------------------------------
TAB_SHAPES = [(V, mr.TAB_T, mr.TAB_K) for V in mr.TAB_VIEWS] + [(2, 1, 1)]


@pytest.mark.parametrize('V,T,K', TAB_SHAPES)
@pytest.mark.parametrize('D', range(1, 7))
def test_multicam_tables_every_state_dim_and_view_count(D, V, T, K):
    """multicam_tables_kernel<D>; V = 3 is 555 lanes: a 43-lane tail in the third block."""
    from eks_amd import hip_ops
    case = mr.tables_case(V, T, K, D)
    ref, lat_ref, bound = mr.multicam_tables_ref(*case)
    dev = [_dev(a) for a in case]
    tables, latent = hip_ops.multicam_tables(*dev, want_latent=True)
    tables, latent = tables.cpu().numpy(), latent.cpu().numpy()
    assert tables.shape == (V, T, K, 9) and latent.shape == (T, K, 2 * D) and tables.dtype == latent.dtype == np.float64
    assert np.array_equal(tables[..., 2:7], ref[..., 2:7])                    # float32 inputs widened: bit for bit
    assert np.array_equal(latent, lat_ref, equal_nan=True)
    assert np.array_equal(np.isnan(tables), np.isnan(ref)) and np.array_equal(np.isnan(latent), np.isnan(lat_ref))
    if T > mr.TAB_NAN_AT[0]:
        assert np.isnan(tables[:, mr.TAB_NAN_AT[0], mr.TAB_NAN_AT[1], :2]).all() and np.isnan(tables).sum() == 2 * V
        assert np.isnan(latent).sum() == D
    for q in (0, 1, 7, 8):
        ok = ~np.isnan(ref[..., q])
        excess = (np.abs(tables[..., q] - ref[..., q]) / bound[..., q])[ok].max()
        assert excess <= 1.0, (q, excess)
    only, none = hip_ops.multicam_tables(*dev, want_latent=False)              # latent = NULL
    assert none is None and np.array_equal(only.cpu().numpy(), tables, equal_nan=True)


def test_multicam_tables_takes_the_drivers_transposed_views():
    from eks_amd import hip_ops
    V, T, K, D = 3, mr.TAB_T, mr.TAB_K, 3
    stats, ev, ms, Vs, C, mean = (_dev(a) for a in mr.tables_case(V, T, K, D))
    ms_kt, Vs_kt = ms.transpose(0, 1).contiguous(), Vs.transpose(0, 1).contiguous()       # (K, T, ...) as eks_smooth
    assert not ms_kt.transpose(0, 1).is_contiguous()
    a = hip_ops.multicam_tables(stats, ev, ms_kt.transpose(0, 1), Vs_kt.transpose(0, 1), C, mean)
    b = hip_ops.multicam_tables(stats, ev, ms, Vs, C, mean)
    for got, want in zip(a, b):
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy(), equal_nan=True)


def test_multicam_tables_refusals_leave_the_output_alone():
    lib = _lib()
    V, T, K = 2, 3, 2
    f32 = lambda *s: torch.rand(s, dtype=torch.float32, device='cuda')  # noqa: E731
    bufs = dict(stats=f32(V, T, K, 5), ev=f32(T, K, 2 * V), ms=f32(T, K, 7), Vs=f32(T, K, 7, 7),
                C=torch.rand((K, 2 * V, 7), dtype=torch.float64, device='cuda'),
                mean=torch.rand((V, K, 2), dtype=torch.float64, device='cuda'),
                tables=torch.full((V, T, K, 9), SENTINEL, dtype=torch.float64, device='cuda'))
    latent = torch.full((T, K, 14), SENTINEL, dtype=torch.float64, device='cuda')

    def call(V=V, T=T, K=K, D=3, **null):
        b = {**bufs, **null}
        return lib.eks_multicam_tables(V, T, K, D, *[_p(b[n]) for n in ('stats', 'ev', 'ms', 'Vs', 'C', 'mean', 'tables')],
                                       _p(latent), _stream())

    assert call(D=7) == ERR_UNSUPPORTED
    for kw in (dict(V=0), dict(T=0), dict(K=0), dict(D=0)):
        assert call(**kw) == ERR_SHAPE, kw
    for name in bufs:
        assert call(**{name: None}) == ERR_NULL, name
    torch.cuda.synchronize()
    assert (bufs['tables'] == SENTINEL).all() and (latent == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# eks_argmin_s
# ---------------------------------------------------------------------------------------------------------------------
def _argmin_rows(n, rng):
    """name -> row of n values: ties, minima at the ends, infinities and NaNs (lanes stride over the candidates by 64:
    c and c + 64 meet inside one lane, c and c + 1 in the wave's reduction)."""
    base = lambda: rng.standard_normal(n) * 50.0 + 300.0  # noqa: E731
    rows = {'random': base(), 'all_1e12': np.full(n, 1e12), 'all_plus_inf': np.full(n, np.inf)}

    def put(name, at, value=-7.0):
        r = base()
        r[[c for c in at if 0 <= c < n]] = value
        rows[name] = r

    put('min_first', [0])
    put('min_last', [n - 1])
    put('tie_two_lanes', [n // 3, n - 1])
    put('tie_one_lane', [n // 3, n // 3 + 64, n // 3 + 128])
    put('tie_second_pass_first', [70, 70 - 64 + 5])                    # index 11 (lane 11) before 70 (lane 6)
    put('tie_signed_zero', [n // 2, n - 1])
    rows['tie_signed_zero'] = np.abs(rows['tie_signed_zero'])
    rows['tie_signed_zero'][n // 2], rows['tie_signed_zero'][n - 1] = 0.0, -0.0
    put('plus_inf_entries', [0, n // 2, n - 1], np.inf)
    put('minus_inf_twice', [n // 2, n - 1], -np.inf)
    put('nan_first', [0], np.nan)
    put('nan_interior', [min(17, n - 1)], np.nan)
    put('nan_last', [n - 1], np.nan)
    put('nan_at_64', [64], np.nan)
    put('nan_twice', [n - 1, n // 2], np.nan)
    put('nan_70_and_9', [70, 9], np.nan)
    rows['nan_and_minus_inf'] = rows['minus_inf_twice'].copy()
    rows['nan_and_minus_inf'][n - 1] = np.nan                          # the NaN wins over -inf before it
    rows['all_nan'] = np.full(n, np.nan)
    return rows


@pytest.mark.parametrize('n_cand', [1, 2, 63, 64, 65, 130, 200])
@pytest.mark.parametrize('K', [1, 3, 4, 5, 9])
def test_argmin_s_is_numpys_argmin_with_ties_infinities_and_nans(K, n_cand):
    """Every row kind at every K (a block holds 4 keypoints) and n_cand (a lane holds ceil(n_cand / 64) candidates)."""
    lib = _lib()
    rng = np.random.default_rng(100 * K + n_cand)
    rows = _argmin_rows(n_cand, rng)
    names = list(rows)
    pad = -len(names) % K
    table = np.stack([rows[n] for n in names] + [rng.standard_normal(n_cand) for _ in range(pad)])
    names += ['random'] * pad
    cand = np.exp(np.linspace(-8.0, 8.0, n_cand)) if n_cand > 1 else np.array([0.37])
    want = np.argmin(table, axis=1)
    assert want[names.index('all_1e12')] == 0 and want[names.index('all_nan')] == 0
    if n_cand > 17:
        assert want[names.index('nan_interior')] == 17 and want[names.index('nan_and_minus_inf')] == n_cand - 1
    cand_d = _dev(cand)
    for r0 in range(0, len(names), K):
        nll = _dev(table[r0:r0 + K])
        s_out = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
        s_only = torch.full((K,), SENTINEL, dtype=torch.float64, device='cuda')
        idx = torch.full((K,), -1, dtype=torch.int32, device='cuda')
        assert lib.eks_argmin_s(K, n_cand, _p(nll), _p(cand_d), _p(s_out), _p(idx), _stream()) == 0
        assert lib.eks_argmin_s(K, n_cand, _p(nll), _p(cand_d), _p(s_only), None, _stream()) == 0       # idx_out = NULL
        got = idx.cpu().numpy()
        wrong = [(names[r0 + j], int(got[j]), int(want[r0 + j])) for j in range(K) if got[j] != want[r0 + j]]
        assert not wrong, wrong
        assert np.array_equal(s_out.cpu().numpy(), cand[want[r0:r0 + K]])
        assert np.array_equal(s_only.cpu().numpy(), cand[want[r0:r0 + K]])


def test_argmin_s_refusals():
    lib = _lib()
    nll = torch.rand((2, 5), dtype=torch.float64, device='cuda')
    cand = torch.rand(5, dtype=torch.float64, device='cuda')
    s_out = torch.full((2,), SENTINEL, dtype=torch.float64, device='cuda')
    assert lib.eks_argmin_s(0, 5, _p(nll), _p(cand), _p(s_out), None, _stream()) == ERR_SHAPE
    assert lib.eks_argmin_s(2, 0, _p(nll), _p(cand), _p(s_out), None, _stream()) == ERR_SHAPE
    for null in range(3):
        args = [None if i == null else _p(t) for i, t in enumerate((nll, cand, s_out))]
        assert lib.eks_argmin_s(2, 5, *args, None, _stream()) == ERR_NULL
    torch.cuda.synchronize()
    assert (s_out == SENTINEL).all()
