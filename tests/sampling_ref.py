"""Float64 NumPy reference of the posterior sampler (TEST INFRASTRUCTURE, imported by the sampling tests only):
Philox4x32-10 and the Box-Muller transform the kernels use, the sequential scalar filter and the backward-sampling
recurrence, a float32 transcription of that recurrence (what plain float32 arithmetic reaches: it sets the float32
bars), the dense joint posterior covariance of a short session by plain linear algebra, and Durbin & Koopman's
simulation smoother for general models with its float32-storage transcription (dense_durbin_koopman)."""
from __future__ import annotations

import numpy as np

VAR_FLOOR, VAR_CEIL = 1e-12, 1e30
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 ints.  Returns 4 uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & np.uint64(MASK), n2, p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def box_muller(a, b):
    """two 32-bit words -> two standard normals (float64), the kernels' construction: u = (top 24 bits + 1/2) 2^-24,
    angle = top 24 bits 2^-24 of a revolution."""
    u = ((np.asarray(a, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    v = (np.asarray(b, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return r * np.cos(2 * np.pi * v), r * np.sin(2 * np.pi * v)


def scalar_noise(seed, T, N, n_draws, first_chain=0, first_draw=0):
    """The normals of the scalar-chain path, [n_draws][T][N]: counter (frame // 4, chain, draw, 0); words (0, 1) give
    frames 4 q, 4 q + 1 and words (2, 3) frames 4 q + 2, 4 q + 3."""
    nq = (T + 3) // 4
    tq = np.arange(nq)[None, :, None]
    ch = (first_chain + np.arange(N))[None, None, :]
    dr = (first_draw + np.arange(n_draws))[:, None, None]
    w = philox4x32_10((tq, ch, dr, 0), (seed & MASK, (seed >> 32) & MASK))
    z0, z1 = box_muller(w[0], w[1])
    z2, z3 = box_muller(w[2], w[3])
    z = np.stack([z0, z1, z2, z3], axis=2).reshape(n_draws, 4 * nq, N)
    return z[:, :T]


def dense_noise(seed, T, K, W, n_draws, first_keypoint=0, first_draw=0):
    """The normals of the general path, [n_draws][T][K][W]: counter (frame, keypoint, draw, b) gives normals 4 b .. 4 b + 3."""
    nb = (W + 3) // 4
    t = np.arange(T)[None, :, None, None]
    kp = (first_keypoint + np.arange(K))[None, None, :, None]
    dr = (first_draw + np.arange(n_draws))[:, None, None, None]
    b = np.arange(nb)[None, None, None, :]
    w = philox4x32_10((t, kp, dr, b), (seed & MASK, (seed >> 32) & MASK))
    z0, z1 = box_muller(w[0], w[1])
    z2, z3 = box_muller(w[2], w[3])
    z = np.stack([z0, z1, z2, z3], axis=-1).reshape(n_draws, T, K, 4 * nb)
    return z[..., :W]


def scalar_filter_smoother(y, var, m0, S0, a, c, qs, dtype=np.float64):
    """Sequential filter + RTS on N independent chains (arrays over chains; y, var [T][N]).  (m, P) entering frame t
    is the predicted belief; the filtered variance is formed as P r / (P c^2 + r) as in the kernels.
    Returns mf, Pf, ms, Vs, G [T][N] (G[T-1] = 0)."""
    f = dtype
    y, var = np.asarray(y, f), np.clip(np.asarray(var, f), f(VAR_FLOOR), f(VAR_CEIL))
    a, c, qs = (np.asarray(x, f) for x in (a, c, qs))
    T, N = y.shape
    mf, Pf = np.empty((T, N), f), np.empty((T, N), f)
    m, P = np.asarray(m0, f).copy(), np.asarray(S0, f).copy()
    for t in range(T):
        g = 1 / (P * c * c + var[t])
        mf[t] = m + P * c * g * (y[t] - c * m)
        Pf[t] = P * var[t] * g
        m, P = a * mf[t], a * a * Pf[t] + qs
    ms, Vs, G = np.empty_like(mf), np.empty_like(Pf), np.zeros_like(Pf)
    ms[-1], Vs[-1] = mf[-1], Pf[-1]
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + qs
        G[t] = a * Pf[t] / Pp
        ms[t] = mf[t] + G[t] * (ms[t + 1] - a * mf[t])
        Vs[t] = Pf[t] * qs / Pp + G[t] * G[t] * Vs[t + 1]
    return mf, Pf, ms, Vs, G


def scalar_deviations(Pf, a, qs, z, dtype=np.float64):
    """e [n_draws][T][N] from the filtered variances and normals z [n_draws][T][N]:
    e_{T-1} = sqrt(Pf) z, e_t = G_t e_{t+1} + sqrt(Pf_t s q / Pp_{t+1}) z_t (the cancellation-free innovation variance)."""
    f = dtype
    Pf, a, qs, z = np.asarray(Pf, f), np.asarray(a, f), np.asarray(qs, f), np.asarray(z, f)
    T = Pf.shape[0]
    e = np.empty(z.shape, f)
    e[:, -1] = np.sqrt(Pf[-1]) * z[:, -1]
    for t in range(T - 2, -1, -1):
        Pp = a * a * Pf[t] + qs
        G = a * Pf[t] / Pp
        e[:, t] = G * e[:, t + 1] + np.sqrt(Pf[t] * (qs / Pp)) * z[:, t]
    return e


def scalar_deviations_f32(var, S0, a, c, qs, z):
    """The float32 transcription: the variance filter and the recurrence in float32 throughout."""
    f = np.float32
    var = np.asarray(var, f)
    zero = np.zeros_like(var)
    _, Pf, _, _, _ = scalar_filter_smoother(zero, var, np.zeros(var.shape[1]), S0, a, c, qs, dtype=f)
    return scalar_deviations(Pf, a, qs, z, dtype=f)


def read_through_f32_output(ms, e):
    """What a deviation looks like once it has been through the float32 output: x = ms + e formed in float32, read
    back as x - ms.  ms [T][N], e [n_draws][T][N]."""
    m = np.asarray(ms, np.float32)
    x = m[None] + np.asarray(e, np.float32)
    return x.astype(np.float64) - m[None].astype(np.float64)


def dense_joint_posterior(var, S0, A, C, Q, s):
    """One keypoint, T frames: the joint posterior covariance of (x_0 .. x_{T-1}) [T D][T D] by plain linear algebra.
    var [T][O]; the belief entering frame 0 is N(m0, S0), x_{t+1} = A x_t + N(0, s Q), y_t = C x_t + N(0, diag var)."""
    var = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, O = var.shape
    D = A.shape[0]
    # prior covariance of the stacked states
    P = [np.asarray(S0, np.float64)]
    for _ in range(1, T):
        P.append(A @ P[-1] @ A.T + s * Q)
    Sx = np.zeros((T * D, T * D))
    for i in range(T):
        Cij = P[i]
        for j in range(i, T):
            Sx[j * D:(j + 1) * D, i * D:(i + 1) * D] = Cij
            Sx[i * D:(i + 1) * D, j * D:(j + 1) * D] = Cij.T
            Cij = A @ Cij
    H = np.kron(np.eye(T), C)
    R = np.diag(var.ravel())
    Sy = H @ Sx @ H.T + R
    return Sx - Sx @ H.T @ np.linalg.solve(Sy, H @ Sx)


def law_error(Lmat, S):
    """max |(L L' - S)_ij| / sqrt(S_ii S_jj)"""
    sd = np.sqrt(np.diag(S))
    return float(np.max(np.abs(Lmat @ Lmat.T - S) / np.outer(sd, sd)))


def chol_psd(M):
    """Lower Cholesky factors of symmetric PSD matrices [K][D][D] by the kernels' documented rule: a non-positive
    pivot gives a zero column (a singular Q draws nothing along that direction)."""
    M = np.asarray(M, np.float64)
    K, D, _ = M.shape
    L = np.zeros_like(M)
    for j in range(D):
        dj = M[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        ok = dj > 0.0
        r = np.sqrt(np.where(ok, dj, 1.0))
        L[:, j, j] = np.where(ok, r, 0.0)
        for i in range(j + 1, D):
            v = M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)
            L[:, i, j] = np.where(ok, v / r, 0.0)
    return L


def filter_by_scalar_updates(y, m0, S0, A, C, Q, s, R):
    """float64 Kalman filter, update-then-predict as oracle.eks_oracle.kalman_filter (frame 0 updates the prior), with
    the O observations of a frame absorbed one at a time - exact for the diagonal R of this project, and free of the
    O x O inverse of the innovation covariance.  kalman_filter forms np.linalg.inv(S) and P - K S K': with one variance
    of a frame at the 1e30 clip and the others near one, cond(S) ~ 1e30, and its means around that frame are off by up
    to 7e-5 of the chain's largest |ms| in float64 (against the information-form smoother of the oracle and against
    this filter, which agree); where a frame's variances lie within a few decades the two filters agree to rounding
    (tests/test_sampling_cpu.py).  y, R (K, T, O); m0 (K, D); S0, A, Q (K, D, D); C (K, O, D); s (K,).
    Returns mf (K, T, D), Pf (K, T, D, D)."""
    y, R, m0, S0, A, C, Q = (np.asarray(a, np.float64) for a in (y, R, m0, S0, A, C, Q))
    K, T, O = y.shape
    D = m0.shape[-1]
    sQ = np.broadcast_to(np.asarray(s, np.float64), (K,))[:, None, None] * Q
    At = np.swapaxes(A, -1, -2)
    mf, Pf = np.empty((K, T, D)), np.empty((K, T, D, D))
    m, P = m0.copy(), S0.copy()
    for t in range(T):
        if t:
            m = np.einsum('kij,kj->ki', A, m)
            P = A @ P @ At + sQ
        for o in range(O):
            h = C[:, o]
            u = np.einsum('kij,kj->ki', P, h)
            g = 1.0 / (R[:, t, o] + np.einsum('ki,ki->k', h, u))
            m = m + u * (g * (y[:, t, o] - np.einsum('ki,ki->k', h, m)))[:, None]
            P = P - u[:, :, None] * u[:, None, :] * g[:, None, None]
        P = 0.5 * (P + np.swapaxes(P, -1, -2))
        mf[:, t], Pf[:, t] = m, P
    return mf, Pf


def dense_durbin_koopman(y, var, m0, S0, A, C, Q, s, z, storage=np.float64, round_output=True):
    """Durbin & Koopman's simulation smoother as eks_sample composes it for general models, a plain sequential
    construction in float64: y, var [T][K][O]; m0 [K][D]; S0, A, Q [K][D][D]; C [K][O][D]; s [K];
    z [n_draws][T][K][D + O] (D state normals - chol(S0) at frame 0, chol(s Q) afterwards - then O observation
    normals).  x+ / y+ are simulated from the zero-mean model with the data's variances clipped to
    [VAR_FLOOR, VAR_CEIL], the data and every y+ are smoothed by a float64 filter (filter_by_scalar_updates) and the
    RTS pass of oracle.eks_oracle, and dev = x+ - E[x+ | y+].  Returns ms [T][K][D], Vs [T][K][D][D], dev [n_draws][T][K][D].

    storage = np.float32 is the float32-storage transcription: the same code with x+, y+, the stacked means and the
    final ms + dev rounded to float32 where the kernels store float32 (dev is then read back off that output as
    (ms + dev) - ms; round_output = False leaves the last rounding out).  Everything else stays float64."""
    from oracle.eks_oracle import rts_smoother
    st = storage
    y = np.asarray(y, np.float64)
    var = np.clip(np.asarray(var, np.float64), VAR_FLOOR, VAR_CEIL)
    T, K, O = y.shape
    A, C, Q, S0 = (np.asarray(a, np.float64) for a in (A, C, Q, S0))
    m0 = np.asarray(m0, np.float64)
    s = np.broadcast_to(np.asarray(s, np.float64), (K,))
    z = np.asarray(z, np.float64)
    n, D = z.shape[0], A.shape[-1]
    assert z.shape == (n, T, K, D + O)
    L0, Lq = chol_psd(S0), chol_psd(s[:, None, None] * Q)
    xs = np.empty((n, T, K, D))
    x = np.zeros((n, K, D))
    for t in range(T):                                     # the recursion itself runs on the unrounded state
        x = np.einsum('kij,nkj->nki', L0, z[:, 0, :, :D]) if t == 0 else \
            np.einsum('kij,nkj->nki', A, x) + np.einsum('kij,nkj->nki', Lq, z[:, t, :, :D])
        xs[:, t] = x
    yp = np.einsum('koj,ntkj->ntko', C, xs) + np.sqrt(var)[None] * z[..., D:]
    xs, yp = xs.astype(st).astype(np.float64), yp.astype(st).astype(np.float64)
    # one stacked problem of (n + 1) K chains: set 0 the data, set 1 + d the simulated observations with m0 = 0
    rep = lambda a: np.tile(a, (n + 1,) + (1,) * (a.ndim - 1))
    y_all = np.concatenate([y[None], yp]).transpose(0, 2, 1, 3).reshape((n + 1) * K, T, O)
    R_all = np.tile(var.transpose(1, 0, 2), (n + 1, 1, 1))
    m0_all = np.concatenate([m0, np.zeros((n * K, D))])
    mf, Pf = filter_by_scalar_updates(y_all, m0_all, rep(S0), rep(A), rep(C), rep(Q), rep(s), R_all)
    ms_all, Vs_all = rts_smoother(mf, Pf, rep(A), rep(Q), rep(s))
    ms = ms_all[:K].transpose(1, 0, 2)
    Vs = Vs_all[:K].transpose(1, 0, 2, 3)
    mp = ms_all[K:].reshape(n, K, T, D).transpose(0, 2, 1, 3)
    ms_st, mp = ms.astype(st).astype(np.float64), mp.astype(st).astype(np.float64)
    dev = xs - mp
    if round_output and st is not np.float64:
        dev = (ms_st[None] + dev).astype(st).astype(np.float64) - ms_st[None]
    return ms_st, Vs, dev
