"""The bound behind the windowed replay of the scalar-chain smoother (eks_diag.hip: replay_window_block), restated in
NumPy float64 and checked on chains that cover both sides of its premise.

An element (A, b, C, eta, J) summarises a run of frames (eks_math.hpp).  Whatever lies beyond the run reaches the far
side only through A:

  forward   elem_apply:  m' = A (m + P eta) / (1 + J P) + b,   P' = A^2 P / (1 + J P) + C
            (m + P eta) / (1 + J P) is the posterior mean of x_in under the prior (m, P) and the run's own data; it lies
            between m and the run's own estimate x_ml = eta / J.  Two priors (m1, P1), (m2, P2) therefore leave beliefs
            whose means differ by at most |A| (|m1 - x_ml| + |m2 - x_ml|)  =: |A| * front spread
            and whose variances differ by at most A^2 / J.
  backward  elem_back:   eta' = A (eta - J b) / (1 + C J) + e.eta,   J' = A^2 J / (1 + C J) + e.J
            dropping the future's (eta, J) changes eta' by A k (x_ml* - b) with k = J / (1 + C J) <= 1 / C and
            x_ml* = eta / J the future's own estimate of the state behind the run, and J' by A^2 k.  Fused with the
            predicted belief (variance P = C + O(A^2)) the smoothed mean behind the run moves by at most
            |A| |x_ml* - b| (1 + O(A))  =: |A| * back spread.

Inside the group the errors only shrink: the smoothed mean of the first frame depends on the entering mean with
coefficient 1 / (1 + J_total P) <= 1, the RTS gain is a Pf / (a^2 Pf + q) < 1 / |a|.  With |A| <= 2^-30 on both sides
every smoothed mean of the group is within 2^-30 (front + back spread) / min(1, |a|) of the exact one; the test asks
2^-29 (the factor 2 covers the second-order terms and float64 rounding on means near 1e4), and 2^-29 relative on the
variances."""
import numpy as np

import window_ref as wr
from window_ref import B, BAR, G, H, TOL, _apply, _back, _combine, _identity, _append, _smooth_segment


def _chains(seed, n, T, a, c, offset):
    rng = np.random.default_rng(seed)
    x = offset + np.cumsum(0.4 * rng.standard_normal((T, n)), axis=0)
    if a != 1.0:
        x = offset + 3.0 * rng.standard_normal((T, n))          # a decaying chain has no random walk to follow
    r = 0.3 * rng.gamma(2.0, 1.0, (T, n)) + 0.02
    for k in range(n):
        for _ in range(rng.integers(0, 4)):
            t0, ln = rng.integers(0, T), rng.integers(1, 301)
            r[t0:t0 + ln, k] *= 1e4                              # occlusions of 1 - 300 frames
    y = c * x + np.sqrt(np.minimum(r, 50.0)) * rng.standard_normal((T, n))
    s = np.exp(rng.uniform(-8.0, 8.0, n))
    m0 = np.full(n, float(offset))
    S0 = np.full(n, 25.0)
    return y, r, s, m0, S0


def _check(seed, a, c, offset, n=48, T=B * 41 + 5, record=None):
    y, r, q, m0, S0 = _chains(seed, n, T, a, c, offset)
    nc = (T + B - 1) // B
    elems = []
    for j in range(nc):
        e = _identity(n)
        for t in range(j * B, min(T, (j + 1) * B)):
            e = _append(e, y[t], r[t], a, c, q)
        elems.append(e)
    ms_x, Ps_x, _, _ = _smooth_segment(y, r, a, c, q, m0, S0, np.zeros(n), np.zeros(n))
    # exact predicted belief entering every chunk, exact information behind every chunk
    pm, pP = [m0], [S0]
    for j in range(nc):
        m, P = _apply(elems[j], pm[-1], pP[-1])
        pm.append(m)
        pP.append(P)
    info = [(np.zeros(n), np.zeros(n))]
    for j in range(nc - 1, -1, -1):
        info.append(_back(elems[j], *info[-1]))
    info = info[::-1]                                            # info[j]: about the state entering chunk j
    n_pass = n_fail = 0
    worst_m = worst_P = 0.0
    for g0 in range(0, nc, G):
        g1 = min(g0 + G, nc)
        cut_f, cut_b = g0 - H <= 0, g1 + H >= nc
        hf, hb = _identity(n), _identity(n)
        for j in range(max(g0 - H, 0), g0):
            hf = _combine(hf, elems[j])
        for j in range(g1, min(g1 + H, nc)):
            hb = _combine(hb, elems[j])
        ok_f = np.full(n, True) if cut_f else np.abs(hf['A']) <= TOL
        ok_b = np.full(n, True) if cut_b else np.abs(hb['A']) <= TOL
        if record is not None:
            record.append((cut_f, cut_b, np.abs(hf['A']), np.abs(hb['A']), ok_f & ok_b))
        for ok, cut in ((ok_f, cut_f), (ok_b, cut_b)):
            if not cut:
                n_pass += int(ok.sum())
                n_fail += int((~ok).sum())
        # front: stand-in belief in front of the halo (the prior where the halo reaches frame 0)
        m_s = m0 if cut_f else y[(g0 - H) * B] / c
        m_e, P_e = _apply(hf, m_s, S0)
        spread_f = np.zeros(n)
        if not cut_f:
            x_ml = hf['eta'] / hf['J']
            spread_f = np.abs(pm[g0 - H] - x_ml) + np.abs(m_s - x_ml)
        # back: no information behind the halo
        eta_e, J_e = _back(hb, np.zeros(n), np.zeros(n))
        spread_b = np.zeros(n)
        eta_x, J_x = info[min(g1 + H, nc)]
        if not cut_b:
            spread_b = np.abs(eta_x / J_x - hb['b'])
        sel = ok_f & ok_b
        if not sel.any():
            continue
        t0, t1 = g0 * B, min(g1 * B, T)
        ms_w, Ps_w, _, _ = _smooth_segment(y[t0:t1], r[t0:t1], a, c, q, m_e, P_e, eta_e, J_e)
        bar_m = BAR * (spread_f + spread_b) / min(1.0, abs(a))
        # the entry belief, then the smoothed belief on the group's first and last frame
        em = np.abs(m_e - pm[g0])[sel] / np.maximum(bar_m[sel], 1e-300)
        eP = (np.abs(P_e - pP[g0]) / pP[g0])[sel] / BAR
        for t in (t0, t1 - 1):
            em = np.maximum(em, np.abs(ms_w[t - t0] - ms_x[t])[sel] / np.maximum(bar_m[sel], 1e-300))
            eP = np.maximum(eP, (np.abs(Ps_w[t - t0] - Ps_x[t]) / Ps_x[t])[sel] / BAR)
        # (groups whose halos are both cut are exact: spread 0, error 0 up to float64 rounding of the other order of
        #  composition - measured against the size of the means instead)
        exact = (spread_f + spread_b)[sel] == 0
        if exact.any():
            scale = np.abs(ms_x[t0:t1]).max(axis=0)[sel][exact] + 1.0
            assert (np.abs(ms_w[0] - ms_x[t0])[sel][exact] <= 1e-11 * scale).all()
            em = em[~exact]
        worst_m = max(worst_m, em.max(initial=0.0))
        worst_P = max(worst_P, eP.max(initial=0.0))
    return n_pass, n_fail, worst_m, worst_P


CASES = [(11, 1.0, 1.0, 0.0), (12, 1.0, 1.0, 1e4), (13, 0.98, 1.3, 0.0), (14, 0.98, 1.3, 1e4)]


def test_windows_that_forget_reproduce_the_exact_entry_and_edge_beliefs():
    n_pass = n_fail = 0
    for seed, a, c, offset in CASES:
        p, f, wm, wP = _check(seed, a, c, offset)
        print(f'a={a} c={c} offset={offset}: {p} windows qualify, {f} do not; worst mean error {wm:.3g} of the bar, '
              f'worst variance error {wP:.3g} of the bar')
        assert wm <= 1.0, (seed, a, c, offset, wm)
        assert wP <= 1.0, (seed, a, c, offset, wP)
        n_pass += p
        n_fail += f
    share = n_pass / (n_pass + n_fail)
    print(f'{n_pass} of {n_pass + n_fail} windows qualify ({100 * share:.1f} %)')
    assert n_pass > 0 and n_fail > 0
    assert 0.2 <= share <= 0.8, share


def test_classify_agrees_with_the_restatement_of_the_check():
    """window_ref.classify (what the GPU tests predict the kernel's fail marks with) against the halo compositions,
    cut rules and verdicts that _check derives on its own."""
    for seed, a, c, offset in CASES:
        n, T = 48, B * 41 + 5
        y, r, q, _, _ = _chains(seed, n, T, a, c, offset)
        rec = []
        _check(seed, a, c, offset, record=rec)
        cls = wr.classify(y, r, a, c, q, T)
        assert cls['fail'].shape == (len(rec), n)
        for wg, (cut_f, cut_b, A_f, A_b, ok) in enumerate(rec):
            assert (cls['cut_front'][wg], cls['cut_back'][wg]) == (cut_f, cut_b), wg
            if not cut_f:
                np.testing.assert_array_equal(cls['A_front'][wg], A_f)
            if not cut_b:
                np.testing.assert_array_equal(cls['A_back'][wg], A_b)
            np.testing.assert_array_equal(cls['fail'][wg], ~ok)
        assert cls['cut_front'].tolist() == [True] + [False] * (len(rec) - 1)
        assert cls['cut_back'].tolist() == [False] * (len(rec) - 2) + [True, True]      # 42 chunks = 8 * 5 + 2


def _gpu_inputs():
    yield 'general', wr.general_problem()
    for D in (1, 3, 8):
        yield f'width D={D} unit', wr.width_problem(D, False)
        yield f'width D={D} general', wr.width_problem(D, True)
    for kind in ('low', 'high'):
        yield f'clip {kind}', wr.clip_problem(kind)
    for T in wr.FAIL_T:
        yield f'fail pattern T={T}', wr.fail_pattern_problem(T)
    for M, r0 in wr.OUTLIERS:
        yield f'outlier {M:g}', wr.outlier_problem(M, r0)


def test_the_windowed_restatement_stays_within_the_bound_on_the_inputs_of_the_gpu_tests():
    """window_ref.windowed_smooth (the float64 statement of what replay_window_block computes) against the exact
    smoother on the inputs tests/test_gpu_smooth_window.py feeds the kernel: on every lane the check lets through, the
    means within 2^-29 (front spread + back spread) / min(1, |a|) - and within 1e-7 of the chain's magnitude, a
    hundredth of the bar the kernel is held to - and the variances within 2^-29 relative.  Lanes whose halos are both
    cut are exact (float64 rounding of the other order of composition: 1e-11 of the magnitude)."""
    n_stored = n_failed = 0
    for name, p in _gpu_inputs():
        r = wr.restate(p)
        T = p['y'].shape[0]
        stored = ~wr.group_mask(r['fail'], T)
        scale = np.abs(r['ms_x']).max(axis=0) + 1.0
        err = np.abs(r['ms'] - r['ms_x'])
        bound = wr.group_mask(r['bound'], T) + 1e-11 * scale
        worst_b = float((err / bound)[stored].max())
        worst_s = float((err / scale)[stored].max())
        worst_P = float((np.abs(r['Ps'] - r['Ps_x']) / r['Ps_x'])[stored].max())
        print(f'{name}: {int(r["fail"].sum())} of {r["fail"].size} lanes fail; stored lanes: means {worst_b:.3g} of the '
              f'bound, {worst_s:.3g} of the magnitude, variances {worst_P:.3g} relative')
        assert worst_b <= 1.0, (name, worst_b)
        assert worst_s <= 1e-7, (name, worst_s)
        assert worst_P <= BAR, (name, worst_P)
        n_stored += int((~r['fail']).sum())
        n_failed += int(r['fail'].sum())
    assert n_stored > 0 and n_failed > 0


def test_the_fail_pattern_inputs_have_no_borderline_halo():
    """The GPU test of the fail pattern asks the kernel's float32 verdicts to EQUAL the float64 ones: every halo of
    its inputs is far from the tolerance (|A| <= 2^-34 or >= 2^-26)."""
    for T in wr.FAIL_T:
        ch = wr.chains(wr.fail_pattern_problem(T))
        cls = wr.classify(ch['y'], ch['var'], ch['a'], ch['c'], ch['q_s'], T)
        for A, cut in ((cls['A_front'], cls['cut_front']), (cls['A_back'], cls['cut_back'])):
            A = A[~cut]
            assert ((A <= 2.0 ** -34) | (A >= 2.0 ** -26)).all(), (T, A[(A > 2.0 ** -34) & (A < 2.0 ** -26)])
        print(T, 'failing lanes per group:', cls['fail'].sum(axis=1).tolist())
