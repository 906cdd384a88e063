"""GPU: eks_smooth_robust (eks_amd/csrc/eks_smooth_student.hip on scalar chains, dense_smooth_robust in eks_dense.hip
on general models) and eks_amd.robust against the references of tests/robust_ref.py, through the C ABI.

Bars.  Scalar chains (float32 lanes), the project's rule (robust_ref.bars): error / scale <= max(1e-5, 4 x the float32
NumPy transcription's own worst error / scale on the same inputs); scale of ms: the chain's max |y|; of Vs: its own
value; of weights and change: 1.  General models (float64 in the lane, weights kept in float32 - the reference rounds
them there too): 100 x the disagreement of the two independent float64 reference forms on the same inputs, floored at
1e-12 and capped at 1e-8 (smooth_tv_ref.f64_bar), relative to the keypoint's largest |ms| / |Vs| entry (1 for weights
and change), plus one float32 ulp of the reference value.  Inputs keep var >= 0.02 and |y| <= 400 with about 2 % of
the frames displaced by 20 .. 60 px (include/eks_hip.h states why nothing is asked of the weights at var ~ 1e-12).
Nothing is compared with the kernels' own output, except where the test is about bits (n_iters = 1 against
eks_smooth_tv, continuation, determinism, subsets, optional outputs).

Pass counts: a call of n passes updates the weights n - 1 times and a continued call's first pass smooths again under
the weights it was given, so n1 passes followed by n2 passes are one call of n1 + n2 - 1 passes: 3 then 6 give the
bits of 8 (and 3 then 5 those of 7).

Measured on the MI355X: DESIGN.md 9i has the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_guard as bg  # noqa: E402
import robust_ref as rref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402
from test_gpu_increments import PARAMS, _dev, dense_session, diag_flags, edge_session, stable  # noqa: E402,F401
from test_gpu_em import subset  # noqa: E402
from dense_forms import general_grid, general_seed  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B = 32                                        # kChainChunk: frames per lane of the scalar-chain kernels
T_EDGES = (1, 2, B - 1, B, B + 1, 33 * B + 1)
N_ITERS = (1, 2, 8)
NUS = (1.0, 4.0, 30.0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def raw_call(dims_args, ins, nu, n_iters, weights, weights_in, change, ms, Vs, ws=None, ws_bytes=None):
    """eks_smooth_robust itself: ins = y, var, m0 .. s.  Returns the status."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*dims_args)
    if ws is None:
        need = int(lib.eks_smooth_robust_workspace_bytes(ctypes.byref(dims)))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda')
    p = hip_ops._ptr
    rc = lib.eks_smooth_robust(ctypes.byref(dims), *[p(t) for t in ins], float(nu), int(n_iters), p(weights), int(weights_in),
                               p(change), p(ms), p(Vs), p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                               hip_ops._stream())
    torch.cuda.synchronize()
    return rc


def scalar_ins(pb):
    T, K, D = pb['T'], pb['K'], pb['D']
    return [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]


def gpu_scalar(pb, nu, n_iters, vs_diag=True, lam0=None, want_weights=True, want_change=True, ins=None):
    """eks_smooth_robust on the chains of make_session -> ms (T, N), Vs (T, N) or (T, K, D, D), weights (T, N),
    change (K,) as NumPy float32 (None for an output that was not asked for)."""
    from eks_amd import _lib
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = scalar_ins(pb) if ins is None else ins
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    if lam0 is not None:
        wt = _dev(np.ascontiguousarray(lam0, np.float32).reshape(T, K, D))
    else:
        wt = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda') if want_weights else None
    ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda') if want_change else None
    rc = raw_call((K, T, D, D, diag_flags(pb) | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, nu, n_iters, wt,
                  lam0 is not None, ch, ms, Vs)
    assert rc == 0
    Vs = Vs.cpu().numpy()
    return (ms.cpu().numpy().reshape(T, K * D), Vs.reshape(T, K * D) if vs_diag else Vs,
            None if wt is None else wt.cpu().numpy().reshape(T, K * D), None if ch is None else ch.cpu().numpy())


def displaced(pb, seed, spots=()):
    """About 2 % of the entries moved by +-(20 .. 60) px, and every frame of `spots` in one chain each."""
    rng = np.random.default_rng(seed)
    T, N = pb['y'].shape
    hit = rng.random((T, N)) < 0.02
    for i, t in enumerate(spots):
        hit[t, i % N] = True
        pb['var'][t, i % N] = 1.0                     # (make_session puts 1e3 on 2 % of the frames: not on these)
    pb['y'] = (pb['y'] + hit * rng.choice([-1.0, 1.0], (T, N)) * rng.uniform(20, 60, (T, N))).astype(np.float32)
    pb['hit'] = hit
    assert np.abs(pb['y']).max() <= 400 and pb['var'].min() >= 0.02
    return pb


def edge_spots(T):
    """jB - 1, jB, jB + 1 of the first, a middle and the last chunk, frame 0 and frame T - 1."""
    nc = -(-T // B)
    spots = {0, T - 1}
    for j in {1, nc // 2, nc - 1}:
        spots |= {j * B - 1, j * B, j * B + 1}
    return sorted(t for t in spots if 0 <= t < T)


def session(T, K, D, kind, seed):
    """make_session centred at 50 px ('general': a = 0.98, c = 1.3 and a q of its own per chain, as edge_session), with
    displaced frames.  The centre keeps every chain's max |y| - the scale ms is held to - of the size of the values
    the lane computes with: centred at 3 px a single-frame chain can have |y| = 0.03 next to m0 = 3, and one float32
    ulp of 3 is then 1e-5 of the scale whatever the arithmetic does."""
    pb = make_session(T, K, D, 2.0, kind == 'unit', seed, a=0.98, c=1.3, centre=50.0)
    if kind != 'unit':
        q = np.random.default_rng(seed + 1).uniform(0.5, 2.0, K * D)
        pb['par']['Q'][:, np.arange(D), np.arange(D)] = q.reshape(K, D)
        pb['qs'] = q * 2.0
    return displaced(pb, seed, edge_spots(T))


def scalar_refs(pb, nu, counts, lam0=None):
    """{n: (float64 result, float32 transcription's result, bars)} for calls of n passes, change per keypoint."""
    K, D = pb['K'], pb['D']
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu, max(counts))
    s64, s32 = dict.fromkeys(counts), dict.fromkeys(counts)
    rref.scalar_robust(*args, lam0=lam0, snapshots=s64)
    rref.scalar_robust_f32(*args, lam0=lam0, unit=pb['unit'], snapshots=s32)
    out = {}
    for n in counts:
        r64, r32 = (list(s[n][:3]) + [s[n][3].reshape(K, D).max(axis=1)] for s in (s64, s32))
        out[n] = (r64, r32, rref.bars(r32, r64, pb['y']))
    return out


def check_scalar(label, pb, got, ref, worst=None, slack=1.0):
    r64, r32, bars = ref
    ms, Vs, lam, ch = got
    assert all(np.isfinite(x).all() for x in got) and (Vs > 0).all() and (lam > 0).all(), f'{label}: non-finite output'
    err, et = rref.errors(got, r64, pb['y']), rref.errors(r32, r64, pb['y'])
    for k in err:
        e, t = float(np.max(err[k])), float(np.max(et[k]))
        if worst is not None:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e, t))
        assert e <= slack * bars[k], f'{label}: {k} {e:.3g} over {slack} x bar {bars[k]:.3g} (transcription {t:.3g})'
    return bars


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 2), (21, 3), (65, 1), (65, 2)])
def test_scalar_chain_edge_shapes(K, D, kind):
    worst = {}
    for T in T_EDGES:
        pb = session(T, K, D, kind, seed=T + K)
        ins = scalar_ins(pb)
        for nu in NUS:
            refs = scalar_refs(pb, nu, N_ITERS)
            for n in N_ITERS:
                got = gpu_scalar(pb, nu, n, ins=ins)
                label = f'N={K * D} D={D} T={T} {kind} nu={nu} n_iters={n}'
                check_scalar(label, pb, got, refs[n], worst)
                assert (got[2] <= np.float32((nu + 1) / nu)).all(), label
                if n == 1:
                    assert (got[2] == 1).all() and not got[3].any(), label
    print(f'N={K * D} D={D} {kind}, worst kernels (transcription on that case): '
          + ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (e, t) in worst.items()))


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_displaced_frames_at_the_chunk_edges_get_their_own_weights(kind):
    """The frames displaced at jB - 1, jB, jB + 1, 0 and T - 1 carry small weights in exactly their own chain and
    frame: a weight stored one frame or one chain off would sit far outside the bar, and is shown here directly."""
    T, K, D = 33 * B + 1, 3, 1
    pb = session(T, K, D, kind, seed=5)
    lam = gpu_scalar(pb, 4.0, 8)[2]
    ref = scalar_refs(pb, 4.0, (8,))[8][0][2]
    spots = edge_spots(T)
    for i, t in enumerate(spots):
        n = i % (K * D)
        assert ref[t, n] < 0.2, (t, n, ref[t, n])                       # (the reference itself discounts the frame)
        assert lam[t, n] < 0.2, f'{kind}: displaced frame {t} of chain {n} kept weight {lam[t, n]:.3g}'
    check_scalar(f'{kind} displaced frames', pb, gpu_scalar(pb, 4.0, 8), scalar_refs(pb, 4.0, (8,))[8])


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('vs_diag', [True, False])
def test_one_pass_is_eks_smooth_tv_at_unit_scale_bit_for_bit(kind, vs_diag):
    from eks_amd import hip_ops
    for T, K, D in ((33 * B + 1, 21, 3), (B + 1, 3, 2), (700, 65, 1)):
        pb = session(T, K, D, kind, seed=T)
        ins = scalar_ins(pb)
        ms, Vs, lam, ch = gpu_scalar(pb, 4.0, 1, vs_diag=vs_diag, ins=ins)
        tm, tV = hip_ops.smooth_tv(ins[0], ins[1], _dev(np.ones(T, np.float32)), *ins[2:], flags=diag_flags(pb),
                                   vs_diag=vs_diag)
        torch.cuda.synchronize()
        assert np.array_equal(ms, tm.cpu().numpy().reshape(T, -1)), (kind, T)
        assert np.array_equal(Vs.reshape(T, -1), tV.cpu().numpy().reshape(T, -1)), (kind, T)
        assert (lam == 1).all() and (ch == 0).all()


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_continuation_through_the_weights_gives_the_single_calls_bits(kind):
    T, K, D = 5 * B + 7, 5, 2
    pb = session(T, K, D, kind, seed=11)
    ins = scalar_ins(pb)
    whole8, whole7 = gpu_scalar(pb, 4.0, 8, ins=ins), gpu_scalar(pb, 4.0, 7, ins=ins)
    first = gpu_scalar(pb, 4.0, 3, ins=ins)
    for n2, whole in ((6, whole8), (5, whole7)):
        cont = gpu_scalar(pb, 4.0, n2, lam0=first[2], ins=ins)
        for a, b in zip(cont, whole):
            assert np.array_equal(a, b), (kind, n2)
    assert not np.array_equal(whole7[2], whole8[2])


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_one_pass_under_given_weights_is_eks_smooth_on_var_over_weights(kind, set_knob):
    from eks_amd import hip_ops
    set_knob('EKS_SMOOTH_WINDOW', '0')
    T, K, D = 33 * B + 1, 21, 2
    pb = session(T, K, D, kind, seed=3)
    lam0 = np.random.default_rng(1).uniform(0.02, 1.25, pb['y'].shape).astype(np.float32)
    ms, Vs, lam, ch = gpu_scalar(pb, 4.0, 1, lam0=lam0)
    assert np.array_equal(lam, lam0) and not ch.any()
    veff = (pb['var'] / lam0).astype(np.float32)
    args = (pb['y'], veff, pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], np.ones(T))
    r64 = tref.scalar_smooth_tv(*args)
    bars = tref.f32_bars(*tref.scalar_smooth_tv_f32(*args, unit=pb['unit']), *r64, pb['y'])
    sm, sV = hip_ops.smooth(_dev(pb['y'].reshape(T, K, D)), _dev(veff.reshape(T, K, D)), *(_dev(pb['par'][k]) for k in PARAMS),
                            flags=diag_flags(pb), vs_diag=True)
    torch.cuda.synchronize()
    sm, sV = sm.cpu().numpy().reshape(T, -1).astype(np.float64), sV.cpu().numpy().reshape(T, -1).astype(np.float64)
    e_m = float((np.abs(ms - sm).max(axis=0) / np.abs(pb['y']).max(axis=0)).max())
    e_V = float((np.abs(Vs - sV) / sV).max())
    print(f'{kind}: one pass under given weights against eks_smooth on var / weights: ms {e_m:.3g} (bar {bars["ms"]:.3g}), '
          f'Vs {e_V:.3g} ({bars["Vs"]:.3g})')
    assert e_m <= 2 * bars['ms'] and e_V <= 2 * bars['Vs']
    err = tref.f32_errors(ms, Vs, *r64, pb['y'])
    assert float(err['ms'].max()) <= bars['ms'] and float(err['Vs'].max()) <= bars['Vs']


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_optional_outputs_two_calls_and_a_subset_of_the_keypoints(kind):
    """weights = NULL and / or change = NULL leave the other outputs' bits; two calls give the same bits; keypoints
    [3, 67) of K = 70 alone (another lane mapping) give the full call's bits."""
    T, K, D = 35 * B + 1, 70, 2
    pb = session(T, K, D, kind, seed=21)
    ins = scalar_ins(pb)
    full, again = gpu_scalar(pb, 4.0, 4, ins=ins), gpu_scalar(pb, 4.0, 4, ins=ins)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for ww, wc in ((False, True), (True, False), (False, False)):
        part = gpu_scalar(pb, 4.0, 4, want_weights=ww, want_change=wc, ins=ins)
        for a, b in zip(part, full):
            assert a is None or np.array_equal(a, b), (ww, wc)
    k0, k1 = 3, 67
    sub = gpu_scalar(subset(pb, k0, k1), 4.0, 4)
    for a, b in zip(sub[:3], full[:3]):
        assert np.array_equal(a, b[:, D * k0:D * k1])
    assert np.array_equal(sub[3], full[3][k0:k1])


@pytest.mark.parametrize('diag', [True, False])
def test_guarded_workspace_and_outputs_at_an_offset(diag):
    """A workspace of exactly the queried size filled with 0xFF between guards, and ms, Vs, weights, change one
    element off their allocations' alignment: nothing outside their extents is touched, and the result is the bits
    of the plain call."""
    from eks_amd import _lib
    if diag:
        pb = session(3 * B + 5, 5, 2, 'unit', seed=2)
        T, K, D, O = pb['T'], pb['K'], pb['D'], pb['D']
        ins, flags = scalar_ins(pb), diag_flags(pb) | _lib.FLAG_VS_DIAG
        plain = gpu_scalar(pb, 4.0, 3, ins=ins)
    else:
        M = stable(dense_case(3, 3, 4, False, seed=5))
        T, K, D, O = 70, 3, 3, 4
        y, var = dense_session(M, T, O, seed=2)
        ins, flags = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS], _lib.FLAG_VS_DIAG
        plain = gpu_dense(M, y, var, 4.0, 3, vs_diag=True)
    dims = _lib.EksDims(K, T, D, O, flags)
    need = int(_lib.load().eks_smooth_robust_workspace_bytes(ctypes.byref(dims)))
    gw = bg.GuardedWorkspaces(0xFF)
    entry = 'eks_smooth_robust'                                              # (named for buffer_guard's messages)
    ws = gw(need, 'cuda')
    assert ws.numel() == need and entry
    for weights_given in (True, False):
        outs = dict(ms=bg.guarded_output((T, K, D), offset=1, name='ms'), Vs=bg.guarded_output((T, K, D), offset=1, name='Vs'),
                    weights=bg.guarded_output((T, K, O), offset=1, name='weights'),
                    change=bg.guarded_output((K,), offset=1, name='change'))
        rc = raw_call((K, T, D, O, flags), ins, 4.0, 3, outs['weights'].tensor if weights_given else None, 0,
                      outs['change'].tensor, outs['ms'].tensor, outs['Vs'].tensor, ws=ws)
        assert rc == 0
        gw.assert_intact()
        for o in outs.values():
            o.assert_intact()
        names = ('ms', 'Vs', 'weights', 'change') if weights_given else ('ms', 'Vs', 'change')
        for name in names:
            want = plain[('ms', 'Vs', 'weights', 'change').index(name)]
            assert np.array_equal(outs[name].tensor.cpu().numpy().reshape(want.shape), want), (name, weights_given)


def test_refusals_leave_the_outputs_untouched():
    from eks_amd import _lib
    pb = edge_session(100, 3, 2, 2.0, 'unit', seed=2)
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = scalar_ins(pb)
    outs = [torch.full(shape, 7.0, dtype=torch.float32, device='cuda') for shape in ((T, K, D), (K,), (T, K, D), (T, K, D, D))]
    wt, ch, ms, Vs = outs
    diag = diag_flags(pb)
    untouched = lambda: all(bool((o == 7.0).all()) for o in outs)  # noqa: E731
    call = lambda dims, tensors=ins, nu=4.0, n=8, w=wt, w_in=0, c=ch, m=ms, V=Vs, **kw: raw_call(  # noqa: E731
        dims, tensors, nu, n, w, w_in, c, m, V, **kw)
    good = (K, T, D, D, diag)
    cases = [
        (call(good, nu=0.0), -2), (call(good, nu=-1.0), -2), (call(good, nu=float('nan')), -2),
        (call(good, nu=float('inf')), -2), (call(good, n=0), -2), (call(good, n=-1), -2),
        (call((K, T, D, D, 0), nu=0.0), -2), (call((K, T, D, D, 0), n=0), -2),
        (call(good, w=None, w_in=1), -1), (call((K, T, D, D, 0), w=None, w_in=1), -1),
        (call(good, tensors=ins[:3] + [None] + ins[4:]), -1), (call(good, m=None), -1), (call(good, V=None), -1),
        (call((0, T, D, D, diag)), -2), (call((K, 0, D, D, diag)), -2), (call((K, T, D, D + 1, diag)), -2),
        (call((K, T, D, D, _lib.FLAG_UNIT_AC)), -3), (call((K, T, 7, 7, 0)), -3), (call((K, T, D, 65, 0)), -3),
        (call((K, T, 9, 9, diag)), -3), (call(good, ws_bytes=255), -4), (call((K, T, D, D, 0), ws_bytes=255), -4),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, (i, got, want)
    assert untouched()
    tv = int(_lib.load().eks_smooth_tv_workspace_bytes(ctypes.byref(_lib.EksDims(*good))))
    assert call(good, ws_bytes=tv) == -4 and untouched()                     # eks_smooth_tv's size lacks the plane
    assert call(good) == 0
    assert not any(bool((o == 7.0).any()) for o in outs)


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_extreme_variances_keep_every_output_finite_and_the_weights_in_range(kind):
    """var at 1e-12, 1e30 and inf: no parity bar (delta's cancellation error is (2^-24 |y|)^2 / r), but everything is
    finite, variances positive and 0 < weights <= (nu + 1) / nu; a frame at 1e30 stays missing."""
    T, K, D = 7 * B + 3, 5, 2
    for nu in NUS:
        pb = session(T, K, D, kind, seed=9)
        rng = np.random.default_rng(2)
        pick = rng.random(pb['var'].shape)
        pb['var'][pick < 0.05] = 1e-12
        pb['var'][(pick > 0.05) & (pick < 0.10)] = 1e30
        pb['var'][(pick > 0.10) & (pick < 0.15)] = np.inf
        pb['var'][3 * B:4 * B, 0] = 1e30                                    # a whole chunk of one chain missing
        pb['var'][:, 1] = np.inf                                           # a chain that is never observed
        for n in (2, 8):
            ms, Vs, lam, ch = gpu_scalar(pb, nu, n)
            assert np.isfinite(ms).all() and np.isfinite(Vs).all() and (Vs > 0).all()
            assert np.isfinite(lam).all() and (lam > 0).all() and (lam <= np.float32((nu + 1) / nu)).all()
            assert np.isfinite(ch).all() and (ch >= 0).all()
            gone = pb['var'] >= 1e30
            assert (lam[gone] > 0.999 * (nu + 1) / nu).all()                 # delta ~ 0: the weight sits at its ceiling


# ---- general models ------------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, nu, n_iters, vs_diag=False, lam0=None, flags=0):
    from eks_amd import _lib
    T, K, O = y.shape
    D = M['m0'].shape[1]
    ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    wt = torch.full((T, K, O), np.nan, dtype=torch.float32, device='cuda') if lam0 is None else _dev(lam0.astype(np.float32))
    ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda')
    assert raw_call((K, T, D, O, flags | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, nu, n_iters, wt, lam0 is not None, ch,
                    ms, Vs) == 0
    return ms.cpu().numpy(), Vs.cpu().numpy(), wt.cpu().numpy(), ch.cpu().numpy()


def dense_displaced(M, T, O, seed):
    y, var = dense_session(M, T, O, seed)
    rng = np.random.default_rng(seed + 100)
    hit = rng.random(y.shape) < 0.02
    if T > 3:
        hit[T // 2, 0, 0] = True
    y = (y + hit * rng.choice([-1.0, 1.0], y.shape) * rng.uniform(20, 60, y.shape)).astype(np.float32)
    return y, np.maximum(var, np.float32(0.02))


def dense_excess(got, seq, joint, unit_scale=False):
    """worst |got - seq| / (bar x scale + one float32 ulp), and the bar; scale: the keypoint's largest entry, or 1."""
    K = seq.shape[1] if seq.ndim > 1 else seq.shape[0]
    if unit_scale:
        scale = np.ones_like(seq)
    else:
        scale = np.abs(seq).transpose(1, 0, *range(2, seq.ndim)).reshape(K, -1).max(axis=1)
        scale = scale.reshape((1, K) + (1,) * (seq.ndim - 2)) * np.ones_like(seq)
    bar = tref.f64_bar(seq, joint, scale)
    ulp = np.spacing(np.abs(seq).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - seq) / (bar * scale + ulp)).max()), bar


def dense_refs(M, y, var, nu, counts):
    par = tuple(M[k] for k in PARAMS)
    out = []
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        snaps = dict.fromkeys(counts)
        rref.dense_robust(y, var, *par, nu, max(counts), form=form, snapshots=snaps, lam_dtype=np.float32)
        out.append(snaps)
    return out


def check_dense(label, got, seq, joint, worst=None):
    for i, name in enumerate(('ms', 'Vs', 'weights', 'change')):
        g, a, b = got[i], seq[i], joint[i]
        assert np.isfinite(g).all(), f'{label}: {name} is not finite'
        if name == 'Vs' and g.ndim == 3:                                      # VS_DIAG
            a, b = (np.diagonal(x, axis1=2, axis2=3) for x in (a, b))
        excess, bar = dense_excess(g, a, b, unit_scale=i >= 2)
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), excess)
        assert excess <= 1.0, f'{label}: {name} is {excess:.3g} x its bar {bar:.3g} (+ one float32 ulp)'


# (and the accepted width, odd O past 32 and the smallest odd O, at K = 3: tests/dense_forms.py WIDE_PAIRS)
@pytest.mark.parametrize('D,O,K', general_grid([(1, 1), (2, 3), (3, 4), (6, 12)]))
def test_general_models_against_the_two_float64_forms(D, O, K, set_knob):
    M = stable(dense_case(K, D, O, False, seed=general_seed(D, O, K)))
    worst = {}
    for i, T in enumerate((1, 2, 17, 33, 100)):
        y, var = dense_displaced(M, T, O, seed=T)
        seq, joint = dense_refs(M, y, var, 4.0, (1, 3))
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            for n in (1, 3):
                got = gpu_dense(M, y, var, 4.0, n, vs_diag=(i % 2 == 0))
                check_dense(f'D={D} O={O} K={K} T={T} chunk={chunk} n_iters={n}', got, seq[n], joint[n], worst)
                if n == 1:
                    assert (got[2] == 1).all() and not got[3].any()
    print(f'general D={D} O={O} K={K}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('variant', ['two_scan_blocks', 'unit_root', 'singular_q'])
def test_general_model_variants(variant, set_knob):
    """ceil(T / 16) > 64 chunks (two blocks of dense_scan_kernel); A = I; a rank D - 1 Q."""
    D, O, K = 3, 4, 3
    T = 1100 if variant == 'two_scan_blocks' else 100
    set_knob('EKS_DENSE_CHUNK', '16')
    M = stable(dense_case(K, D, O, variant == 'singular_q', seed=8), unit_root=variant == 'unit_root')
    if variant == 'singular_q':
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    y, var = dense_displaced(M, T, O, seed=3)
    seq, joint = dense_refs(M, y, var, 4.0, (1, 3))
    worst = {}
    for n in (1, 3):
        check_dense(f'{variant} n_iters={n}', gpu_dense(M, y, var, 4.0, n), seq[n], joint[n], worst)
    print(f'{variant}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('D,O', [(1, 1), (2, 3), (3, 4), (6, 12)])
def test_general_model_single_pass_agrees_with_the_generic_eks_smooth_tv(D, O):
    """n_iters = 1 against the generic eks_smooth_tv at w = 1: the same float64 arithmetic around another summarize
    kernel, so within one float32 ulp of each other."""
    from eks_amd import hip_ops
    M = stable(dense_case(3, D, O, False, seed=12))
    T = 300
    y, var = dense_displaced(M, T, O, seed=4)
    ms, Vs, _, _ = gpu_dense(M, y, var, 4.0, 1)
    tm, tV = hip_ops.smooth_tv(_dev(y), _dev(var), _dev(np.ones(T, np.float32)), *(_dev(M[k]) for k in PARAMS), flags=0)
    torch.cuda.synchronize()
    for g, t in ((ms, tm.cpu().numpy()), (Vs, tV.cpu().numpy())):
        assert (np.abs(g.astype(np.float64) - t) <= np.spacing(np.abs(t))).all()


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_a_diagonal_model_down_the_general_path_agrees_with_the_scalar_path(kind):
    T, K, D = 5 * B + 7, 5, 2
    pb = session(T, K, D, kind, seed=4)
    par = pb['par']
    refs = scalar_refs(pb, 4.0, (8,))[8]
    sc = gpu_scalar(pb, 4.0, 8)
    check_scalar(f'{kind} scalar path', pb, sc, refs)
    dn = gpu_dense(par, pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), 4.0, 8, vs_diag=True, flags=0)
    dn = (dn[0].reshape(T, -1), dn[1].reshape(T, -1), dn[2].reshape(T, -1), dn[3])
    check_scalar(f'{kind} general path', pb, dn, refs)
    bars = refs[2]
    err = rref.errors(dn, [x.astype(np.float64) for x in sc], pb['y'])
    for k in err:
        assert float(np.max(err[k])) <= 2 * bars[k], (k, float(np.max(err[k])), bars[k])


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_smooth_robust_matches_the_references_on_both_paths():
    from eks_amd import smooth_robust
    pb = session(200, 3, 2, 'unit', seed=9)
    T, K, D = pb['T'], pb['K'], pb['D']
    par = pb['par']
    ms, Vs, lam, ch = smooth_robust(np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'],
                                    par['Q'], pb['var'].reshape(T, K, D), par['s'], nu=4.0, n_iters=8, vs_diag=True)
    assert ms.shape == (K, T, D) and Vs.shape == (K, T, D) and lam.shape == (K, T, D) and ch.shape == (K,)
    assert ms.dtype == np.float32 and lam.dtype == np.float32
    flat = lambda x: np.swapaxes(x, 0, 1).reshape(T, -1)  # noqa: E731
    check_scalar('smooth_robust', pb, (flat(ms), flat(Vs), flat(lam), ch), scalar_refs(pb, 4.0, (8,))[8])
    M = stable(dense_case(3, 3, 4, False, seed=2))
    y, var = dense_displaced(M, 120, 4, seed=5)
    ms, Vs, lam, ch = smooth_robust(np.swapaxes(y, 0, 1), M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'], n_iters=3)
    assert ms.shape == (3, 120, 3) and Vs.shape == (3, 120, 3, 3) and lam.shape == (3, 120, 4)
    seq, joint = dense_refs(M, y, var, 4.0, (3,))
    check_dense('smooth_robust, general', (np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1), np.swapaxes(lam, 0, 1), ch),
                seq[3], joint[3])


def test_tolerance_loop_stops_below_tol_and_is_a_single_call_of_the_same_pass_count():
    from eks_amd import smooth_robust
    pb = session(300, 3, 2, 'unit', seed=13)
    T, K, D = pb['T'], pb['K'], pb['D']
    par = pb['par']
    args = (np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'], par['Q'],
            pb['var'].reshape(T, K, D), par['s'])
    tol, n = 1e-3, 4
    looped = smooth_robust(*args, nu=4.0, n_iters=n, tol=tol, max_iters=64, vs_diag=True)
    assert float(looped[3].max()) < tol
    total = n
    while True:                                   # blocks of n passes: each continued block adds n - 1 updates
        single = smooth_robust(*args, nu=4.0, n_iters=total, vs_diag=True)
        if float(single[3].max()) < tol:
            break
        total += n - 1
        assert total <= 64
    assert total > n, 'the first block already met the tolerance: the loop was not exercised'
    for a, b in zip(looped, single):
        assert np.array_equal(a, b)
    capped = smooth_robust(*args, nu=4.0, n_iters=n, tol=1e-30, max_iters=9, vs_diag=True)
    for a, b in zip(capped, smooth_robust(*args, nu=4.0, n_iters=9, vs_diag=True)):
        assert np.array_equal(a, b)


def test_smooth_singlecam_robust_on_the_golden_markers_with_a_displaced_keypoint(golden_dir):
    """40 frames of one keypoint moved by 30 px in every ensemble member (the ensemble agrees on the wrong place):
    on that keypoint the robust smoother is closer to the undisturbed session's Gaussian result than the Gaussian
    smoother run on the disturbed session."""
    from eks_amd import smooth_singlecam_robust
    from eks_amd.marker_array import MarkerArray
    from eks_amd.singlecam_smoother import ensemble_kalman_smoother_singlecam
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers'].astype(np.float64)
    names = [str(k) for k in g['keypoints']]
    M_, V, T, K, _ = mk.shape
    fields = ['x', 'y', 'likelihood']
    df, s = ensemble_kalman_smoother_singlecam(MarkerArray(mk, data_fields=fields), names, smooth_param=10.0)
    clean = df.to_numpy().reshape(T, K, 9)[:, :, 0:2]
    rng = np.random.default_rng(0)
    frames = rng.choice(np.arange(5, T - 5), size=40, replace=False)
    bad = mk.copy()
    bad[:, :, frames, 1, 0] += 30.0
    ma = MarkerArray(bad, data_fields=fields)
    rob = smooth_singlecam_robust(ma, names, s, nu=4.0, n_iters=8)
    gau = smooth_singlecam_robust(ma, names, s, nu=4.0, n_iters=1)
    assert rob['ms'].shape == (T, K, 2) and rob['Vs'].shape == (T, K, 2) and rob['weights'].shape == (T, K, 2)
    assert (gau['weights'] == 1).all() and (rob['weights'] > 0).all() and (rob['weights'] <= 1.25).all()
    e_rob = float(np.sqrt(np.mean((rob['ms'][:, 1] - clean[:, 1]) ** 2)))
    e_gau = float(np.sqrt(np.mean((gau['ms'][:, 1] - clean[:, 1]) ** 2)))
    print(f'golden markers, 40 frames of keypoint 1 displaced by 30 px: rms distance to the undisturbed Gaussian result '
          f'{e_rob:.4g} px (robust) against {e_gau:.4g} px (Gaussian); median weight on the displaced frames '
          f'{np.median(rob["weights"][frames, 1, 0]):.3g}, elsewhere {np.median(np.delete(rob["weights"][:, 1, 0], frames)):.3g}')
    assert e_rob < e_gau
