"""Float64 restatement of the windowed replay of the scalar-chain smoother (eks_diag.hip: replay_window_block), shared
by tests/test_window_bound_cpu.py (the bound itself) and tests/test_gpu_smooth_window.py (the kernel against it), with
the inputs both use.  NumPy only: nothing here touches the device.

An element (A, b, C, eta, J) summarises a run of frames (eks_math.hpp); `_append` adds a frame, `_combine` composes two
runs in time order, `_apply` pushes a predicted belief through a run, `_back` pulls information about the state behind
a run to the state in front of it.  Chains are the last axis everywhere: a keypoint's D coordinates are D chains,
chain n = keypoint * D + coordinate, as in the kernels."""
import numpy as np

B, H, G = 32, 2, 8                # frames per chunk, halo chunks per side, own chunks per window group
GROUP = B * G
TOL = 2.0 ** -30                  # eks_diag.hip: kWinTol
BAR = 2.0 ** -29
VAR_LO, VAR_HI = 1e-12, 1e30      # eks_diag_lane.hpp: clip_var


def _identity(n):
    return dict(A=np.ones(n), b=np.zeros(n), C=np.zeros(n), eta=np.zeros(n), J=np.zeros(n))


def _append(e, y, r, a, c, q):
    g = 1.0 / (r + e['C'] * c * c)
    d = y - c * e['b']
    rg = r * g
    Acg = e['A'] * c * g
    return dict(eta=e['eta'] + Acg * d, J=e['J'] + Acg * e['A'] * c, b=a * (e['b'] + e['C'] * c * g * d),
                A=a * e['A'] * rg, C=a * a * e['C'] * rg + q)


def _combine(i, j):
    inv = 1.0 / (1.0 + i['C'] * j['J'])
    return dict(A=j['A'] * inv * i['A'], b=j['A'] * inv * (i['b'] + i['C'] * j['eta']) + j['b'],
                C=j['A'] * inv * j['A'] * i['C'] + j['C'], eta=i['A'] * inv * (j['eta'] - j['J'] * i['b']) + i['eta'],
                J=i['A'] * inv * i['A'] * j['J'] + i['J'])


def _apply(e, m, P):
    inv = 1.0 / (1.0 + e['J'] * P)
    return e['A'] * inv * (m + P * e['eta']) + e['b'], e['A'] * inv * e['A'] * P + e['C']


def _back(e, eta, J):
    inv = 1.0 / (1.0 + e['C'] * J)
    return e['A'] * inv * (eta - J * e['b']) + e['eta'], e['A'] * inv * e['A'] * J + e['J']


def _smooth_segment(y, r, a, c, q, m, P, eta, J):
    """Filter frames y, r [L][n] from the predicted belief (m, P), fuse with the information (eta, J) about the state
    behind them, RTS backwards.  Returns the smoothed means, variances [L][n] and the predicted belief behind."""
    L = y.shape[0]
    mf, Pf = np.empty_like(y), np.empty_like(y)
    for t in range(L):
        g = 1.0 / (P * c * c + r[t])
        mf[t] = m + P * c * g * (y[t] - c * m)
        Pf[t] = P * r[t] * g
        m, P = a * mf[t], a * a * Pf[t] + q
    m_out, P_out = m, P
    inv = 1.0 / (1.0 + J * P)
    ms_n, Ps_n = (m + P * eta) * inv, P * inv
    ms, Ps = np.empty_like(y), np.empty_like(y)
    for t in range(L - 1, -1, -1):
        Pp = a * a * Pf[t] + q
        Gn = a * Pf[t] / Pp
        ms_n = mf[t] + Gn * (ms_n - a * mf[t])
        Ps_n = Pf[t] * q / Pp + Gn * Gn * Ps_n
        ms[t], Ps[t] = ms_n, Ps_n
    return ms, Ps, m_out, P_out


def chunk_elems(y, var, a, c, q_s, T):
    """The element of every chunk of B frames: y, var [T][n] float64 (var already clipped), a, c, q_s scalars or [n]."""
    n = y.shape[1]
    elems = []
    for j in range((T + B - 1) // B):
        e = _identity(n)
        for t in range(j * B, min(T, (j + 1) * B)):
            e = _append(e, y[t], var[t], a, c, q_s)
        elems.append(e)
    return elems


def _halos(elems, wg):
    """Composed elements of the halo in front of and behind window group `wg` (chunks outside the sequence are
    identities) and the kernel's two cut flags."""
    nc, n = len(elems), elems[0]['A'].shape[0]
    jh0, g1 = wg * G - H, (wg + 1) * G
    hf, hb = _identity(n), _identity(n)
    for j in range(max(jh0, 0), wg * G):
        hf = _combine(hf, elems[j])
    for j in range(min(g1, nc), min(g1 + H, nc)):
        hb = _combine(hb, elems[j])
    return hf, hb, jh0 <= 0, g1 + H >= nc


def classify(y, var, a, c, q_s, T, elems=None):
    """Per (window group, chain): |A| of the halo in front and of the halo behind, in float64, and per window group the
    kernel's cut flags (`jh0 <= 0`, `(wg + 1) * kWinG + kWinH >= nc`): a cut halo is exact and passes without a check.
    `fail` is what the kernel's rule gives in exact arithmetic: a halo that is not cut and has |A| > 2^-30."""
    if elems is None:
        elems = chunk_elems(y, var, a, c, q_s, T)
    nc, n = len(elems), y.shape[1]
    nwg = (nc + G - 1) // G
    A_f, A_b = np.empty((nwg, n)), np.empty((nwg, n))
    cut_f, cut_b = np.empty(nwg, bool), np.empty(nwg, bool)
    for wg in range(nwg):
        hf, hb, cut_f[wg], cut_b[wg] = _halos(elems, wg)
        A_f[wg], A_b[wg] = np.abs(hf['A']), np.abs(hb['A'])
    fail = (~cut_f[:, None] & ~(A_f <= TOL)) | (~cut_b[:, None] & ~(A_b <= TOL))
    return dict(A_front=A_f, A_back=A_b, cut_front=cut_f, cut_back=cut_b, fail=fail)


def exact_smooth(y, var, a, c, q_s, m0, S0):
    n = y.shape[1]
    return _smooth_segment(y, var, a, c, q_s, m0, S0, np.zeros(n), np.zeros(n))[:2]


def windowed_smooth(y, var, a, c, q_s, m0, S0, T):
    """The whole windowed form in float64: every window group starts `y[first halo frame] / c` with variance S0 in front
    of its front halo (the prior itself where frame 0 cuts the halo) and zero information behind its back halo.
    Returns the smoothed means and variances [T][n] of every lane, the kernel's verdict `fail` [groups][n] (lanes it
    would not store) and `bound` [groups][n]: 2^-29 (front spread + back spread) / min(1, |a|), the bound of
    tests/test_window_bound_cpu.py on the means of a stored lane (0 where both halos are cut)."""
    n = y.shape[1]
    elems = chunk_elems(y, var, a, c, q_s, T)
    nc = len(elems)
    cls = classify(y, var, a, c, q_s, T, elems)
    # exact predicted belief entering every chunk, exact information about the state entering every chunk
    pm = [(np.broadcast_to(m0, (n,)).astype(float), np.broadcast_to(S0, (n,)).astype(float))]
    for j in range(nc):
        pm.append(_apply(elems[j], *pm[-1]))
    info = [(np.zeros(n), np.zeros(n))]
    for j in range(nc - 1, -1, -1):
        info.append(_back(elems[j], *info[-1]))
    info = info[::-1]
    ms, Ps = np.empty((T, n)), np.empty((T, n))
    bound = np.zeros_like(cls['A_front'])
    for wg in range(cls['fail'].shape[0]):
        hf, hb, cut_f, cut_b = _halos(elems, wg)
        g0, g1 = wg * G, min((wg + 1) * G, nc)
        m_s = pm[0][0] if cut_f else y[(g0 - H) * B] / c
        m_e, P_e = _apply(hf, m_s, pm[0][1])
        eta_e, J_e = _back(hb, np.zeros(n), np.zeros(n))
        t0, t1 = g0 * B, min(g1 * B, T)
        ms[t0:t1], Ps[t0:t1], _, _ = _smooth_segment(y[t0:t1], var[t0:t1], a, c, q_s, m_e, P_e, eta_e, J_e)
        with np.errstate(divide='ignore', invalid='ignore'):
            spread = np.zeros(n)
            if not cut_f:
                x_ml = hf['eta'] / hf['J']
                spread = spread + np.abs(pm[g0 - H][0] - x_ml) + np.abs(m_s - x_ml)
            if not cut_b:
                eta_x, J_x = info[min(g1 + H, nc)]
                spread = spread + np.abs(eta_x / J_x - hb['b'])
        bound[wg] = BAR * spread / np.minimum(1.0, np.abs(a))
    return ms, Ps, cls['fail'], bound


# ---- inputs shared by the CPU test of the restatement and the GPU tests of the kernel ---------------------------------

def problem(T, K, D, seed, general=False, s=None, neg_c=False, var_scale=0.3):
    """y, var (T, K, D) float32 and the diagonal model of K keypoints x D coordinates.  general=False: A = C = Q = I,
    m0 = 50, S0 = 25 I, a random walk near 50.  general=True: per-chain a in [0.9, 1], |c| in [0.5, 1.5] (negative for a
    third of the chains with neg_c), q in [0.5, 2], m0 != 0 and S0 in [5, 50] differing per chain."""
    rng = np.random.default_rng(seed)
    eye = np.eye(D)
    if general:
        a = rng.uniform(0.9, 1.0, (K, D))
        c = rng.uniform(0.5, 1.5, (K, D))
        if neg_c:
            c = np.where(rng.random((K, D)) < 1 / 3, -c, c)
        q = rng.uniform(0.5, 2.0, (K, D))
        m0 = 2.0 * rng.standard_normal((K, D))
        S0 = rng.uniform(5.0, 50.0, (K, D))
        x = 3.0 * rng.standard_normal((T, K, D))
    else:
        a = c = q = np.ones((K, D))
        m0 = np.full((K, D), 50.0)
        S0 = np.full((K, D), 25.0)
        x = 50.0 + np.cumsum(0.5 * rng.standard_normal((T, K, D)), axis=0)
    var = (var_scale * rng.gamma(2.0, 1.0, (T, K, D)) + 0.02).astype(np.float32)
    y = (c * x + np.sqrt(var) * rng.standard_normal((T, K, D))).astype(np.float32)
    if s is None:
        s = np.exp(rng.uniform(0.0, 4.0, K))
    return dict(y=y, var=var, m0=m0, S0=eye * S0[:, :, None], A=eye * a[:, :, None], C=eye * c[:, :, None],
                Q=eye * q[:, :, None], s=np.asarray(s, np.float64))


def chains(p):
    """A problem as scalar chains for the restatement: y, var [T][N] float64 (var clipped as the kernels clip it), a, c,
    q * s, m0, S0 [N]."""
    T, K, D = p['y'].shape
    dg = lambda M: np.diagonal(M, axis1=1, axis2=2).reshape(K * D)
    y = p['y'].astype(np.float64).reshape(T, K * D)
    var = np.clip(p['var'].astype(np.float64).reshape(T, K * D), VAR_LO, VAR_HI)
    return dict(y=y, var=var, a=dg(p['A']), c=dg(p['C']), q_s=dg(p['Q']) * np.repeat(p['s'], D),
                m0=p['m0'].reshape(K * D), S0=dg(p['S0']), T=T)


def restate(p):
    """windowed_smooth and exact_smooth of a problem: dict(ms, Ps, fail, bound, ms_x, Ps_x), chains last."""
    ch = chains(p)
    ms, Ps, fail, bound = windowed_smooth(ch['y'], ch['var'], ch['a'], ch['c'], ch['q_s'], ch['m0'], ch['S0'], ch['T'])
    ms_x, Ps_x = exact_smooth(ch['y'], ch['var'], ch['a'], ch['c'], ch['q_s'], ch['m0'], ch['S0'])
    return dict(ms=ms, Ps=Ps, fail=fail, bound=bound, ms_x=ms_x, Ps_x=Ps_x)


def classify_problem(p):
    ch = chains(p)
    return classify(ch['y'], ch['var'], ch['a'], ch['c'], ch['q_s'], ch['T'])


def group_mask(fail, T):
    """[groups][n] -> [T][n]."""
    return np.repeat(fail, GROUP, axis=0)[:T]


# (a) every state width: N = K * D is no multiple of 64 and a 64-chain tile boundary falls inside a keypoint
WIDTH_K = {1: 67, 2: 33, 3: 43, 4: 17, 5: 13, 6: 11, 7: 19, 8: 9}
WIDTH_T = 1100


def width_problem(D, general):
    K = WIDTH_K[D]
    assert (K * D) % 64 != 0 and K * D > 64
    return problem(WIDTH_T, K, D, seed=100 + 2 * D + int(general), general=general)


# (b) general diagonal models, per-chain parameters, occlusions, fast and slow s inside one tile
def general_problem():
    T, K, D = 2117, 48, 2
    rng = np.random.default_rng(21)
    s = np.where(rng.random(K) < 0.3, np.exp(-8.0), np.exp(rng.uniform(0.0, 4.0, K)))
    p = problem(T, K, D, seed=22, general=True, s=s, neg_c=True)
    for kp in (2, 9, 20, 33, 47):
        t0 = 150 + 37 * kp
        p['var'][t0:t0 + 250, kp] *= 1e4
    return p


# (c) variances at the edges of clip_var: in own chunks, inside halos, on the first frame of a halo
CLIP_T, CLIP_K = 2117, 20         # (33 chains and more: narrower problems do not take the fused path)


def clip_problem(kind):
    """kind 'low': zeros (clipped to 1e-12) and 1e-9; kind 'high': inf and 3e38 (clamped to 1e30: no weight).
    Keypoint 0: single frames in own chunks, inside both halos, on the first frame of a front halo; keypoint 1: a run of
    40 frames inside an own stretch, one inside a front halo, one inside a back halo; keypoint 2: a run of 70 frames over
    the whole front halo of group 3 and one over the whole back halo of group 5; keypoint 3: the stand-in frame of every
    group; keypoint 4: frame 0 and the last frame; the rest untouched."""
    p = problem(CLIP_T, CLIP_K, 2, seed=31, s=np.full(CLIP_K, 3.0))
    v = p['var']
    e0, e1 = (0.0, 1e-9) if kind == 'low' else (np.inf, 3e38)
    v[[300, 301, 345], 0, 0] = e0                       # own chunks of group 1
    v[[256 * 2 - 30, 256 * 3 + 11], 0, 1] = e1          # inside the front halo of group 2 and the back halo of group 2
    v[256 * 4 - 64, 0] = e0                             # the stand-in frame of group 4
    v[256 * 5 - 64, 0, 1] = e1
    v[600:640, 1] = e0                                  # own frames of group 2
    v[256 * 4 - 52:256 * 4 - 12, 1, 0] = e1             # inside the front halo of group 4
    v[256 * 6 + 10:256 * 6 + 50, 1, 1] = e0             # inside the back halo of group 5
    v[256 * 3 - 67:256 * 3 + 3, 2, 0] = e0              # the whole front halo of group 3
    v[256 * 6 - 3:256 * 6 + 67, 2, 1] = e1              # the whole back halo of group 5
    for g in range(1, 9):
        v[256 * g - 64, 3, g % 2] = e0 if g % 3 else e1
    v[0, 4] = e0
    v[CLIP_T - 1, 4, 0] = e1
    return p


# (d) the fail pattern: occlusions (variance x 1e4) of at least 64 frames, one case per chain
def fail_pattern_problem(T):
    """T = 4165: 131 chunks, 17 window groups, the last of three chunks; the back halo of group 15 is two whole chunks
    (not cut).  T = 1317: 42 chunks = 8 * 5 + 2, the back halo of group 4 ends exactly with the sequence (cut: `>=`).
    T = 1029: 33 chunks, the last group is ONE chunk of five frames (its only own wave is the first)."""
    K = 33                                              # 66 chains: the second tile holds keypoint 32 alone
    rng = np.random.default_rng(41)
    p = problem(T, K, 2, seed=40 + T, s=np.exp(rng.uniform(0.0, 1.5, K)), var_scale=0.05)
    nwg = ((T + B - 1) // B + G - 1) // G
    last = nwg - 1
    spans = [
        (1, 0, 256 * 3 - 64, 256 * 3),                  # exactly the front halo of group 3
        (2, 1, 256 * 3, 256 * 3 + 64),                  # exactly the back halo of group 2
        (3, 0, 256 * 2 - 40, 256 * 2 + 40),             # across a group boundary, 24 clean frames left in either halo
        (4, 1, 256 * 2 - 74, 256 * 2 + 74),             # across a group boundary, both halos whole
        (5, 0, 0, 64),                                  # inside frames 0..63: group 0's front is cut
        (6, 1, 192, 256),                               # the front halo of group 1: not cut
        (7, 0, 256, 320),                               # the back halo of group 0: cut in front only
        (8, 1, T - 64, T),                              # inside the last 64 frames
        (9, 0, 256 * last, T),                          # the whole of the last, ragged group
        (10, 1, 256 * last - 64, 256 * last),           # the front halo of the last group: not cut
        (11, 0, 256 * (last - 1) - 64, 256 * (last - 1)),   # the front halo of the group before it
        (32, 1, 256 * 2, 256 * 2 + 64),                 # second tile: the back halo of group 1
        (32, 0, T - 70, T),
    ]
    for kp, d, t0, t1 in spans:
        p['var'][max(t0, 0):t1, kp, d] *= 1e4
    return p


FAIL_T = (4165, 1317, 1029)


# (f) an outlier on the stand-in frame of every window group, halos just inside the tolerance
OUTLIER_T = B * 41 + 5
OUTLIERS = ((3e4, 1e8), (1e6, 1e10))


def outlier_problem(M, r0):
    T, K = OUTLIER_T, 20
    rng = np.random.default_rng(51)
    x = 50.0 + np.cumsum(0.4 * rng.standard_normal((T, K, 2)), axis=0)
    var = np.ones((T, K, 2), np.float32)
    y = (x + rng.standard_normal((T, K, 2))).astype(np.float32)
    for g in range(1, (T + GROUP - 1) // GROUP):
        y[256 * g - 64] = M
        var[256 * g - 64] = r0
    eye = np.tile(np.eye(2), (K, 1, 1))
    return dict(y=y, var=var, m0=np.full((K, 2), 50.0), S0=eye * 25.0, A=eye.copy(), C=eye.copy(), Q=eye.copy(),
                s=np.full(K, 0.12))


# the stand-in itself: made visible.  Halos at 0.7 of the tolerance and a stand-in frame that carries 1e11 with no
# weight (variance 1e30): the windowed result is then 1e-3 .. 1e-2 of the magnitude from the exact one, all of it
# A x inv x (y / c) - what the kernel must reproduce from the restatement, not from the oracle.
def stand_in_problem(general):
    T, K = OUTLIER_T, 20
    rng = np.random.default_rng(61)
    c = np.ones((K, 2))
    if general:
        c = rng.uniform(0.5, 1.5, (K, 2)) * np.where(rng.random((K, 2)) < 0.5, -1.0, 1.0)
    lo, hi = np.full((K, 2), -6.0), np.full((K, 2), 6.0)         # log q: |A| of 64 frames at r = 1 falls with q
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        A, C = np.ones((K, 2)), np.zeros((K, 2))
        for _t in range(H * B):
            rg = 1.0 / (1.0 + C * c * c)
            A, C = A * rg, C * rg + np.exp(mid)
        lo, hi = np.where(A > 0.7 * TOL, mid, lo), np.where(A > 0.7 * TOL, hi, mid)
    q = np.exp(hi)
    x = 50.0 + np.cumsum(0.4 * rng.standard_normal((T, K, 2)), axis=0)
    var = np.ones((T, K, 2), np.float32)
    y = (c * x + rng.standard_normal((T, K, 2))).astype(np.float32)
    for g in range(1, (T + GROUP - 1) // GROUP):
        y[256 * g - 64] = 1e11 * (-1.0) ** g
        var[256 * g - 64] = 1e30
    eye = np.eye(2)
    return dict(y=y, var=var, m0=np.full((K, 2), 50.0), S0=np.tile(eye * 25.0, (K, 1, 1)), A=np.tile(eye, (K, 1, 1)),
                C=eye * c[:, :, None], Q=eye * q[:, :, None], s=np.ones(K))
