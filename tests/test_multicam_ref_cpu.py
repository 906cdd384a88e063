"""CPU: the references and inputs of tests/multicam_ref.py, which tests/test_gpu_multicam_kernels.py holds the
eks_ensemble, eks_maha_inflate and eks_multicam_tables kernels to.

* ensemble: the inputs contain every count of valid members (x and y apart), NaNs at the first, last and interior
  members, and the named edge lanes; on them oracle.ensemble (float64) is within 1e-3 float32 ulp of the np.longdouble
  restatement, so the GPU test's 1-ulp bar measures the kernel and not cancellation in the variance.
* Mahalanobis distances: the float64 per-frame loop against Gaussian elimination in np.longdouble on every case of the
  GPU test: worst relative difference (denominator floored at 1e-3) 1.13e-11 - multicam_ref.MAHA_SPREAD, the GPU bar
  is 100 x that; no distance within 1e-4 (relative) of the threshold, so the inflation mask is decided by the inputs
  and not by rounding; the loop also agrees with the library's host implementation (eks_amd.stats).
* tables: the einsum reference against the sums written out entry by entry."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multicam_ref as mr  # noqa: E402
from oracle import eks_oracle as orc  # noqa: E402

MODES = [(a, v) for a in ('median', 'mean') for v in ('confidence_weighted_var', 'var')]


@pytest.mark.parametrize('M', range(1, 17))
def test_ensemble_inputs_hold_every_count_position_and_edge(M):
    a = mr.ensemble_case(M, mr.ENS_SHAPES[0]).reshape(M, -1, 3)
    n = a.shape[1]
    body = a[:, :n - mr.ENS_N_SPECIAL]
    for f in (0, 1):
        nan = np.isnan(body[..., f])
        assert set(nan.sum(axis=0)) == set(range(M + 1))                   # every count of valid members 0..M
        partly = nan[:, (nan.sum(axis=0) > 0) & (nan.sum(axis=0) < M)]
        if M >= 2:
            assert partly[0].any() and partly[-1].any()                    # a NaN first, a NaN last
        if M >= 3:
            assert partly[1:-1].any() and (partly[1:-1].any(axis=0) & ~partly[0] & ~partly[-1]).any()   # interior only
    kx, ky = (np.isnan(body[..., f]).sum(axis=0) for f in (0, 1))
    assert len(set(zip(kx.tolist(), ky.tolist()))) > M + 1                 # the two counts are not tied together
    s = {name: n - mr.ENS_N_SPECIAL + j for j, name in enumerate(mr.ENS_SPECIAL)}
    assert np.isposinf(a[:, s['plus_inf'], 0]).sum() == 1 and np.isneginf(a[:, s['minus_inf'], 1]).sum() == 1
    assert (a[:, s['zero_lik_spread'], 2] == 0).all() and (a[:, s['zero_lik_flat'], 2] == 0).all()
    assert np.isnan(a[:, s['nan_lik'], 2]).sum() == 1
    assert len(set(a[:, s['duplicates'], 0])) == 1
    if M >= 2:
        assert np.ptp(a[:, s['zero_lik_spread'], 0]) > 0 and np.ptp(a[:, s['zero_lik_flat'], 0]) == 0
        assert len(set(a[:, s['duplicates'], 1])) < M
        z = a[:, s['signed_zeros'], 0]
        assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    # the substitutions the kernel has to reproduce all occur (confidence-weighted variance)
    ref = orc.ensemble(a.reshape(M, 1, n, 1, 3), 'median', 'confidence_weighted_var', mr.NAN_REP)[0, 0, :, 0]
    assert ref[s['nan_lik'], 2] == mr.NAN_REP
    if M >= 2:                                           # (one member: the variance is 1 / max(likelihood, 1e-5))
        assert ref[s['zero_lik_flat'], 2] == mr.NAN_REP and ref[s['zero_lik_flat'], 3] == mr.NAN_REP
        assert ref[s['zero_lik_spread'], 2] == mr.FMAX and ref[s['zero_lik_spread'], 3] == mr.FMAX


@pytest.mark.parametrize('M', range(1, 17))
def test_ensemble_oracle_is_within_a_thousandth_ulp_of_longdouble(M):
    worst = 0.0
    for shape in mr.ENS_SHAPES:
        a = mr.ensemble_case(M, shape)
        for avg, var in MODES:
            ref = orc.ensemble(a, avg, var, mr.NAN_REP)[0]
            ld = mr.ensemble_longdouble(a, avg, var, mr.NAN_REP)
            assert np.array_equal(np.isnan(ref), np.isnan(ld))
            worst = max(worst, mr.f32_ulp_error(ref, ld).max())
    print(f'M={M}: oracle vs longdouble {worst:.2e} float32 ulp')
    assert worst < 1e-3


def test_f32_ulp_error_counts_ulps():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    got = np.array([one, up, np.nan, np.inf, 3.0, np.nan], np.float32)
    ref = np.array([1.0, 1.0, np.nan, np.inf, np.nan, 3.0])
    assert mr.f32_ulp_error(got, ref).tolist() == [0.0, 1.0, 0.0, 0.0, np.inf, np.inf]


def test_maha_reference_spread_margin_and_hit_rates():
    """Prints, per case, the float64 loop's distance from the longdouble restatement, the closest approach of a
    distance to the threshold and the fraction of frames with a hit."""
    worst = 0.0
    for C, L, K, N, seed in mr.maha_cases():
        x, v, W, mu = mr.maha_case(C, L, K, N, seed)
        assert all(not np.array_equal(W[0], W[k]) and not np.array_equal(mu[0], mu[k]) for k in range(1, K))
        ref, v_out, n_inf = mr.maha_inflate_ref(x, v, W, mu)
        ld = mr.maha_longdouble(x, v, W, mu)
        spread = mr.maha_relative_error(ref, ld).max()
        margin = np.abs(ref / mr.MAHA_THRESHOLD - 1.0).min()
        hits = n_inf / N
        print(f'C={C} L={L} N={N}: spread {spread:.2e} margin {margin:.2e} hit rate {np.round(hits, 2)}')
        worst = max(worst, spread)
        assert margin > mr.MAHA_MARGIN
        assert np.array_equal(ref > mr.MAHA_THRESHOLD, np.asarray(ld, np.float64) > mr.MAHA_THRESHOLD)
        if L == 2 * C:                                     # exact reconstruction: the degenerate case
            assert np.abs(ref).max() < 1e-20 and not n_inf.any() and np.array_equal(v_out, v)
        elif N == mr.MAHA_N:
            assert hits.min() > 0.09 and hits.max() < 0.51
        elif N >= 63:
            assert n_inf.min() > 0 and n_inf.max() < N
    print(f'worst spread {worst:.3e}; bar {mr.MAHA_BAR:.2e}')
    assert worst <= mr.MAHA_SPREAD
    assert worst > mr.MAHA_SPREAD / 10                     # (the constant is the measurement, not a loose ceiling)


def test_maha_reference_inflation_rule_and_active_mask():
    x, v, W, mu = mr.maha_case(2, 3, 3, 65, 0)
    ref, v_out, n_inf = mr.maha_inflate_ref(x, v, W, mu, active=np.array([1, 0, 1]))
    assert np.isnan(ref[1]).all() and np.array_equal(v_out[1], v[1]) and n_inf[1] == 0
    hit = (ref[0] > mr.MAHA_THRESHOLD).any(axis=1)
    assert hit.any() and not hit.all()
    assert np.array_equal(v_out[0][hit], v[0][hit] * np.float32(mr.MAHA_SCALAR))       # two views: the whole frame
    assert np.array_equal(v_out[0][~hit], v[0][~hit])
    x, v, W, mu = mr.maha_case(3, 4, 3, 65, 0)
    ref, v_out, n_inf = mr.maha_inflate_ref(x, v, W, mu)
    hit = np.repeat(ref > mr.MAHA_THRESHOLD, 2, axis=-1)
    assert (hit.any(axis=-1) & ~hit.all(axis=-1)).any()                                 # frames with some views hit
    assert np.array_equal(v_out[hit], v[hit] * np.float32(10.0)) and np.array_equal(v_out[~hit], v[~hit])
    assert np.array_equal(n_inf, hit.any(axis=-1).sum(axis=-1))


@pytest.mark.parametrize('C,L', [(2, 3), (3, 4), (8, 6)])
def test_maha_reference_agrees_with_the_host_implementation(C, L):
    from eks_amd.stats import compute_mahalanobis
    x, v, W, mu = mr.maha_case(C, L, 2, 40, 3)
    ref = mr.maha_inflate_ref(x, v, W, mu)[0]
    for k in range(2):
        res = compute_mahalanobis(x[k], v[k], n_latent=L, loading_matrix=W[k], mean=mu[k])
        got = np.stack([res['mahalanobis'][c][:, 0] for c in range(C)], axis=1)
        assert mr.maha_relative_error(got, ref[k]).max() < 1e-9


@pytest.mark.parametrize('V,D', [(1, 1), (2, 3), (3, 6), (8, 4)])
def test_tables_reference_is_the_sums_written_out(V, D):
    T, K = 13, 5
    stats, ev, ms, Vs, C, mean = mr.tables_case(V, T, K, D)
    assert np.array_equal(Vs, np.swapaxes(Vs, -1, -2)) and (np.linalg.eigvalsh(Vs.astype(np.float64)) > 0).all()
    tables, latent, bound = mr.multicam_tables_ref(stats, ev, ms, Vs, C, mean)
    assert tables.shape == (V, T, K, 9) and latent.shape == (T, K, 2 * D)
    t_nan, k_nan = mr.TAB_NAN_AT
    nan = np.zeros(tables.shape, bool)
    nan[:, t_nan, k_nan, :2] = True
    assert np.array_equal(np.isnan(tables), nan)
    lnan = np.zeros(latent.shape, bool)
    lnan[t_nan, k_nan, :D] = True
    assert np.array_equal(np.isnan(latent), lnan)
    rng = np.random.default_rng(0)
    for _ in range(40):
        c, t, k, q = rng.integers(V), rng.integers(T), rng.integers(K), rng.integers(2)
        o = 2 * c + q
        m, S, Cr = ms[t, k].astype(np.float64), Vs[t, k].astype(np.float64), C[k, o]
        want = [sum(Cr[a] * m[a] for a in range(D)) + mean[c, k, q], stats[c, t, k, 4], stats[c, t, k, 0],
                stats[c, t, k, 1], ev[t, k, 2 * c], ev[t, k, 2 * c + 1],
                sum(Cr[a] * S[a, b] * Cr[b] for a in range(D) for b in range(D)) + float(ev[t, k, o])]
        got = tables[c, t, k, [q, 2, 3, 4, 5, 6, 7 + q]]
        b = bound[c, t, k, [q, 2, 3, 4, 5, 6, 7 + q]]
        assert np.array_equal(got[1:6], np.asarray(want[1:6], np.float64)) and not b[1:6].any()
        for g, w, bb in ((got[0], want[0], b[0]), (got[6], want[6], b[6])):
            assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= bb
        assert np.array_equal(latent[t, k, :D], m, equal_nan=True) and np.array_equal(latent[t, k, D:], np.diag(S))
    finite = ~np.isnan(tables)
    assert (bound[..., [0, 1, 7, 8]][finite[..., [0, 1, 7, 8]]] > 0).all()
    assert (bound[finite] < 1e-11 * np.maximum(np.abs(tables[finite]), 1.0) + 1e-9).all()    # a rounding bound, not slack
