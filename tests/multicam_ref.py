"""Plain NumPy references and seeded inputs for the four kernels around the Kalman path of the multi-camera driver:
eks_ensemble, eks_maha_inflate, eks_multicam_tables (and the bars of tests/test_gpu_multicam_kernels.py).  The float64
references are what the kernels are compared with; the np.longdouble restatements measure the references' own error
(tests/test_multicam_ref_cpu.py), so that every bar is a statement about the kernel."""
import numpy as np

LD = np.longdouble
FMAX = float(np.finfo(np.float32).max)


# =====================================================================================================================
# eks_ensemble
# =====================================================================================================================
NAN_REP = 123.5                                  # not the default 1000
ENS_SHAPES = ((2, 129, 1), (1, 1, 1))            # 258 lanes: a two-lane tail in the second block; one lane
ENS_N_SPECIAL = 8                                # the last lanes of the large shape carry the hand-made edges
ENS_SPECIAL = ('duplicates', 'signed_zeros', 'plus_inf', 'minus_inf', 'zero_lik_spread', 'zero_lik_flat', 'nan_lik',
               'plain')


def ensemble_invalid_counts(M, n):
    """Number of NaN members of x and of y per lane: every count 0..M occurs for x, and for y with another period."""
    off = 1 if n == 1 else 0
    i = np.arange(n) + off
    kx = i % (M + 1)
    ky = (3 * i + i // (M + 1)) % (M + 1)
    if n > ENS_N_SPECIAL:
        kx[n - ENS_N_SPECIAL:] = 0
        ky[n - ENS_N_SPECIAL:] = 0
    return kx, ky


def ensemble_case(M, shape):
    """markers (M, V, T, K, 3) float32 for one member count: NaN members at the first, the last and random positions,
    and (large shape) the lanes named in ENS_SPECIAL."""
    V, T, K = shape
    n = V * T * K
    rng = np.random.default_rng(1000 * M + n)
    a = np.empty((M, n, 3), np.float32)
    a[..., 0] = rng.uniform(20.0, 300.0, (M, n))
    a[..., 1] = rng.uniform(-300.0, 300.0, (M, n))
    a[..., 2] = rng.uniform(0.05, 1.0, (M, n))
    kx, ky = ensemble_invalid_counts(M, n)
    for i in range(n):
        for f, kk in ((0, kx[i]), (1, ky[i])):
            how = (i // (M + 1) + f) % 3
            where = (np.arange(kk) if how == 0 else M - 1 - np.arange(kk) if how == 1
                     else rng.permutation(M)[:kk])
            a[where, i, f] = np.nan
    if n > ENS_N_SPECIAL:
        s = {name: n - ENS_N_SPECIAL + j for j, name in enumerate(ENS_SPECIAL)}
        m = np.arange(M)
        a[:, s['duplicates'], 0] = 77.25                                          # every member the same
        a[:, s['duplicates'], 1] = np.array([5.5, -3.25, 5.5, 100.0], np.float32)[(m // 2) % 4]   # pairs
        a[:, s['signed_zeros'], 0] = np.where(m % 2 == 0, 0.0, -0.0)
        a[:, s['signed_zeros'], 1] = np.array([-0.0, 7.0, 0.0, -7.0, 0.0], np.float32)[m % 5]
        a[0, s['plus_inf'], 0] = np.inf
        a[M - 1, s['minus_inf'], 1] = -np.inf
        a[:, s['zero_lik_spread'], 2] = 0.0                                       # var / 0 = inf -> float32 max
        a[:, s['zero_lik_flat'], 2] = 0.0                                         # 0 / 0 -> nan_replacement
        a[:, s['zero_lik_flat'], 0] = 12.5
        a[:, s['zero_lik_flat'], 1] = -8.0
        a[M // 2, s['nan_lik'], 2] = np.nan
    return a.reshape(M, V, T, K, 3)


def ensemble_longdouble(arr, avg_mode, var_mode, nan_replacement):
    """The formulas of oracle.ensemble (eks/core.py:58-85) in np.longdouble, member by member: (V, T, K, 5)."""
    a = np.asarray(arr, np.float32).astype(LD)
    M = a.shape[0]
    out = []
    with np.errstate(all='ignore'):
        conf = a[..., 2].sum(axis=0) / LD(M)
        for f in (0, 1):
            x = a[..., f]
            ok = ~np.isnan(x)
            cnt = ok.sum(axis=0)
            mean = np.where(ok, x, LD(0)).sum(axis=0) / cnt.astype(LD)
            d = np.where(ok, x - mean, LD(0))
            var = (d * d).sum(axis=0) / cnt.astype(LD)
            if avg_mode == 'median':
                s = np.sort(np.where(ok, x, LD(np.inf)), axis=0)                  # NaNs (as +inf) last
                lo = np.take_along_axis(s, np.maximum(cnt - 1, 0)[None] // 2, axis=0)[0]
                hi = np.take_along_axis(s, cnt[None] // 2, axis=0)[0]
                avg = np.where(cnt > 0, (lo + hi) / LD(2), LD(np.nan))
            else:
                avg = mean
            if M == 1:
                var = LD(1) / np.maximum(conf, LD(1e-5))
            elif var_mode in ('conf_weighted_var', 'confidence_weighted_var'):
                var = var / conf
            var = np.where(np.isnan(var), LD(nan_replacement), var)
            out.append((avg, np.clip(var, -LD(FMAX), LD(FMAX))))
    return np.stack([out[0][0], out[1][0], out[0][1], out[1][1], conf], axis=-1)


def f32_ulp_error(got, ref):
    """|got - ref| in units of np.spacing of the float32-rounded reference; 0 where both are NaN or equal (infinities
    included), inf where exactly one is NaN or infinite."""
    with np.errstate(all='ignore'):
        r32 = np.asarray(ref).astype(np.float32)
        g, r = np.asarray(got).astype(LD), np.asarray(ref).astype(LD)
        err = np.abs(g - r) / np.spacing(np.abs(r32)).astype(LD)
    same = (g == r) | (np.isnan(g) & np.isnan(r))
    err = np.where(same, LD(0), err)
    return np.where(np.isnan(err), LD(np.inf), err).astype(np.float64)


# =====================================================================================================================
# eks_maha_inflate
# =====================================================================================================================
MAHA_EPS, MAHA_THRESHOLD, MAHA_SCALAR = 1e-6, 5.0, 10.0
MAHA_FLOOR = 1e-3                                # floor of the denominator of a distance's relative error
MAHA_MARGIN = 1e-4                               # no reference distance this close (relative) to the threshold
# (C, L) -> seed, at K = 3, N = 130; (3, 6) has L = 2C: exact reconstruction, distances ~ 0, nothing inflates
MAHA_PAIRS = {(2, 1): 0, (2, 2): 0, (2, 3): 9, (3, 1): 0, (3, 4): 0, (3, 6): 0, (4, 6): 1, (5, 5): 0, (6, 2): 0,
              (7, 6): 0, (8, 1): 1, (8, 6): 0}
MAHA_K, MAHA_N = 3, 130
MAHA_EDGE_PAIRS = ((2, 3), (3, 4))
MAHA_EDGE_N = (1, 63, 64, 65, 257, 1000)
MAHA_EDGE_SEEDS = {(3, 4, 1000): 1}                # every other edge case: seed 0
# worst |float64 reference - longdouble restatement| / max(|longdouble|, MAHA_FLOOR) over every case below, as
# tests/test_multicam_ref_cpu.py measures it: 1.13e-11, at (C, L) = (2, 3), N = 130 (the other cases: 4e-14 .. 6e-12);
# the kernel's bar is 100 x this
MAHA_SPREAD = 1.2e-11
MAHA_BAR = 100.0 * MAHA_SPREAD


def maha_cases():
    """(C, L, K, N, seed) of every case the GPU test runs."""
    out = [(C, L, MAHA_K, MAHA_N, seed) for (C, L), seed in MAHA_PAIRS.items()]
    out += [(C, L, MAHA_K, N, MAHA_EDGE_SEEDS.get((C, L, N), 0)) for (C, L) in MAHA_EDGE_PAIRS for N in MAHA_EDGE_N]
    return out


def maha_case(C, L, K, N, seed):
    """x (K, N, 2C) float64, v (K, N, 2C) float32, W (K, 2C, L), mu (K, 2C) float64: a factor model per keypoint (all
    different), 10 % of the frames shifted off it."""
    rng = np.random.default_rng([seed, C, L, K, N])
    O = 2 * C
    W = rng.standard_normal((K, O, L))
    mu = 0.5 * rng.standard_normal((K, O))
    v = (0.3 * rng.gamma(2.0, 1.0, (K, N, O)) + 0.05).astype(np.float32)
    z = rng.standard_normal((K, N, L))
    x = 3.0 * np.einsum('kol,knl->kno', W, z) + mu[:, None, :] + np.sqrt(v) * rng.standard_normal((K, N, O))
    shifted = rng.random((K, N)) < 0.1
    x[shifted] += 6.0 * rng.standard_normal((int(shifted.sum()), O))
    return x, v, W, mu


def maha_inflate_ref(x, v, W, mu, active=None, eps=MAHA_EPS, threshold=MAHA_THRESHOLD, scalar=MAHA_SCALAR):
    """One pass of the variance-inflation loop, frame by frame (eks/stats.py:119-151, eks/multicam_smoother.py:724-764):
    1 / (v + eps) in float32 as NumPy forms it for float32 variances, everything else float64, np.linalg.inv.
    Returns maha (K, N, C) (NaN for inactive keypoints), v after the pass, n_inflated (K,)."""
    K, N, O = x.shape
    C = O // 2
    maha = np.full((K, N, C), np.nan)
    v_out = v.copy()
    n_inf = np.zeros(K, np.int32)
    for k in range(K):
        if active is not None and not active[k]:
            continue
        Wk, muk = W[k], mu[k]
        for i in range(N):
            Dinv = np.diag((np.float32(1.0) / (v[k, i] + np.float32(eps))).astype(np.float64))
            B = np.linalg.inv(Wk.T @ Dinv @ Wk)
            zz = B @ Wk.T @ Dinv @ (x[k, i] - muk)
            diff = x[k, i] - (Wk @ zz + muk)
            for c in range(C):
                sl = slice(2 * c, 2 * c + 2)
                Qc = np.diag(v[k, i, sl].astype(np.float64)) + Wk[sl] @ B @ Wk[sl].T
                maha[k, i, c] = diff[sl] @ np.linalg.inv(Qc) @ diff[sl]
        hit = maha[k] > threshold
        mask = np.repeat(hit, 2, axis=1)
        if C == 2:                                                  # two views: a hit in either inflates the frame
            mask = mask | mask.any(axis=1, keepdims=True)
        v_out[k][mask] *= np.float32(scalar)
        n_inf[k] = hit.any(axis=1).sum()
    return maha, v_out, n_inf


def _inv_longdouble(A):
    """Batched Gauss-Jordan inverse of (..., L, L) symmetric positive definite matrices in np.longdouble."""
    L = A.shape[-1]
    M = np.concatenate([A.astype(LD), np.broadcast_to(np.eye(L, dtype=LD), A.shape)], axis=-1)
    for i in range(L):
        M[..., i, :] = M[..., i, :] / M[..., i, i:i + 1]
        for j in range(L):
            if j != i:
                M[..., j, :] = M[..., j, :] - M[..., j, i:i + 1] * M[..., i, :]
    return M[..., L:]


def maha_longdouble(x, v, W, mu, eps=MAHA_EPS):
    """The distances of maha_inflate_ref in np.longdouble by Gaussian elimination, all frames at once: (K, N, C)."""
    K, N, O = x.shape
    C = O // 2
    p = (np.float32(1.0) / (v + np.float32(eps))).astype(LD)                     # (K, N, O)
    Wl, vl = W.astype(LD), v.astype(LD)
    r = x.astype(LD) - mu.astype(LD)[:, None, :]
    WP = Wl[:, None, :, :] * p[..., None]                                        # (K, N, O, L)
    A = (WP[..., :, None] * Wl[:, None, :, None, :]).sum(axis=2)                 # (K, N, L, L)
    B = _inv_longdouble(A)
    b = (WP * r[..., None]).sum(axis=2)                                          # (K, N, L)
    z = (B * b[..., None, :]).sum(axis=-1)
    diff = r - (Wl[:, None, :, :] * z[..., None, :]).sum(axis=-1)                # (K, N, O)
    WB = (Wl[:, None, :, :, None] * B[:, :, None, :, :]).sum(axis=3)             # (K, N, O, L)
    out = np.empty((K, N, C), LD)
    for c in range(C):
        o0, o1 = 2 * c, 2 * c + 1
        q00 = vl[..., o0] + (WB[..., o0, :] * Wl[:, None, o0, :]).sum(axis=-1)
        q01 = (WB[..., o0, :] * Wl[:, None, o1, :]).sum(axis=-1)
        q11 = vl[..., o1] + (WB[..., o1, :] * Wl[:, None, o1, :]).sum(axis=-1)
        # 2 x 2 elimination: Q^-1 d = (d1', (d1 - q01 / q00 d0) / (q11 - q01^2 / q00))
        d0, d1 = diff[..., o0], diff[..., o1]
        piv = q11 - q01 * q01 / q00
        y1 = (d1 - q01 / q00 * d0) / piv
        y0 = (d0 - q01 * y1) / q00
        out[..., c] = d0 * y0 + d1 * y1
    return out


def maha_relative_error(got, ref):
    ref = np.asarray(ref)
    return np.asarray(np.abs(got - ref) / np.maximum(np.abs(ref), MAHA_FLOOR), np.float64)


# =====================================================================================================================
# eks_multicam_tables
# =====================================================================================================================
TAB_T, TAB_K = 37, 5
TAB_VIEWS = (1, 2, 3, 8)
TAB_NAN_AT = (11, 3)                             # the (t, k) whose smoothed means are NaN


def tables_case(V, T, K, D, with_nan=True):
    """stats (V, T, K, 5), ev (T, K, 2V), ms (T, K, D), Vs (T, K, D, D) float32; C (K, 2V, D), mean (V, K, 2) float64:
    every entry random and different per view, keypoint and coordinate; Vs symmetric positive definite."""
    rng = np.random.default_rng([V, T, K, D])
    stats = rng.uniform(1.0, 300.0, (V, T, K, 5)).astype(np.float32)
    ev = rng.uniform(0.5, 9.0, (T, K, 2 * V)).astype(np.float32)
    ms = rng.standard_normal((T, K, D)).astype(np.float32) * 20
    G = rng.standard_normal((T, K, D, D))
    S = (G @ np.swapaxes(G, -1, -2) + 0.5 * np.eye(D)).astype(np.float32)
    Vs = np.maximum(S, np.swapaxes(S, -1, -2))                                   # symmetric after the rounding
    C = rng.standard_normal((K, 2 * V, D))
    mean = rng.uniform(50.0, 250.0, (V, K, 2))
    if with_nan and T > TAB_NAN_AT[0] and K > TAB_NAN_AT[1]:
        ms[TAB_NAN_AT] = np.nan
    return stats, ev, ms, Vs, C, mean


def multicam_tables_ref(stats, ev, ms, Vs, C, mean):
    """tables (V, T, K, 9) = x, y = C m + mean | likelihood | x, y ensemble average | x, y ensemble variance (ev) |
    x, y = diag(C V C') + ev; latent (T, K, 2D) = (m, diag V); and the rounding bound of columns 0, 1, 7, 8:
    4 n 2^-53 sum |terms| with n = D + 1 additions for the mean, D^2 + D for the variance (0 in the other columns)."""
    V, T, K, _ = stats.shape
    D = ms.shape[-1]
    Cv = C.reshape(K, V, 2, D)
    m, S = ms.astype(np.float64), Vs.astype(np.float64)
    e = ev.astype(np.float64).reshape(T, K, V, 2).transpose(2, 0, 1, 3)          # (V, T, K, 2)
    st = stats.astype(np.float64)
    mean_b = mean[:, None, :, :]
    ym = np.einsum('kvqa,tka->vtkq', Cv, m) + mean_b
    yv = np.einsum('kvqa,tkab,kvqb->vtkq', Cv, S, Cv) + e
    tables = np.concatenate([ym, st[..., 4:5], st[..., 0:2], e, yv], axis=-1)
    latent = np.concatenate([m, np.einsum('tkaa->tka', S)], axis=-1)
    u = 2.0 ** -53
    bm = 4 * (D + 1) * u * (np.einsum('kvqa,tka->vtkq', np.abs(Cv), np.abs(m)) + np.abs(mean_b))
    bv = 4 * (D * D + D) * u * (np.einsum('kvqa,tkab,kvqb->vtkq', np.abs(Cv), np.abs(S), np.abs(Cv)) + np.abs(e))
    bound = np.concatenate([bm, np.zeros_like(st[..., :5]), bv], axis=-1)
    return tables, latent, bound
