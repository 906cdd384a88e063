"""GPU: eks_smooth_jumps (eks_amd/csrc/eks_smooth_student.hip on scalar chains, dense_smooth_jumps in eks_dense.hip on
general models) and eks_amd.jumps against the references of tests/jumps_ref.py, through the C ABI.

Bars.  Scalar chains (float32 lanes), the project's rule (jumps_ref.bars): error / scale <= max(1e-5, 4 x the float32
NumPy transcription's own worst error / scale on the same inputs); scale of ms: the chain's max |y|; of Vs: its own
value; of u = 1 / scales and of change: 1.  The transcription follows the lanes' organisation (chunks of 32 frames and
the grouped scan): the belief at a chunk boundary comes out of the scan in absolute coordinates and dm = m' - a mf
cancels against it, which a frame-by-frame transcription does not see.  General models (float64 in the lane, scales
kept in float32 - the reference rounds them there too): 100 x the disagreement of the two independent float64 reference
forms on the same inputs, floored at 1e-12 and capped at 1e-8 (smooth_tv_ref.f64_bar), relative to the keypoint's
largest |ms| / |Vs| entry (1 for u and change), plus one float32 ulp of the reference value.  Inputs keep var >= 0.02,
|y| <= 400 centred at 50 px, s q >= 1e-3 and jumps of 20 .. 60 px applied to all coordinates of a keypoint.  Nothing is
compared with the kernels' own output, except where the test is about bits (n_iters = 1 and the last pass against
eks_smooth_tv, continuation, determinism, subsets, optional outputs, workspaces).

Pass counts: a call of n passes updates the scales n - 1 times and a continued call's first pass smooths again under
the scales it was given, so n1 passes followed by n2 passes are one call of n1 + n2 - 1 passes: 3 then 6 give the
bits of 8.

Measured on the MI355X: DESIGN.md 9j has the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_guard as bg  # noqa: E402
import jumps_ref as jref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402
from test_gpu_increments import PARAMS, _dev, dense_session, diag_flags, stable  # noqa: E402
from test_gpu_em import subset  # noqa: E402
from dense_forms import general_grid, general_seed  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B = 32                                        # kChainChunk: frames per lane of the scalar-chain kernels
T_EDGES = (1, 2, B - 1, B, B + 1, 33 * B + 1)
N_ITERS = (1, 2, 8)
NUS = (1.0, 4.0, 30.0)
NAMES = ('ms', 'Vs', 'scales', 'change')


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def raw_call(dims_args, ins, nu, n_iters, scales, scales_in, change, ms, Vs, ws=None, ws_bytes=None):
    """eks_smooth_jumps itself: ins = y, var, m0 .. s.  Returns the status."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*dims_args)
    if ws is None:
        need = int(lib.eks_smooth_jumps_workspace_bytes(ctypes.byref(dims)))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda')
    p = hip_ops._ptr
    rc = lib.eks_smooth_jumps(ctypes.byref(dims), *[p(t) for t in ins], float(nu), int(n_iters), p(scales), int(scales_in),
                              p(change), p(ms), p(Vs), p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                              hip_ops._stream())
    torch.cuda.synchronize()
    return rc


def scalar_ins(pb):
    T, K, D = pb['T'], pb['K'], pb['D']
    return [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]


def gpu_scalar(pb, nu, n_iters, vs_diag=True, w0=None, want_scales=True, want_change=True, ins=None, ws=None):
    """eks_smooth_jumps on the chains of make_session -> ms (T, N), Vs (T, N) or (T, K, D, D), scales (T, K),
    change (K,) as NumPy float32 (None for an output that was not asked for)."""
    from eks_amd import _lib
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = scalar_ins(pb) if ins is None else ins
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    if w0 is not None:
        sc = _dev(np.ascontiguousarray(w0, np.float32).reshape(T, K))
    else:
        sc = torch.full((T, K), np.nan, dtype=torch.float32, device='cuda') if want_scales else None
    ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda') if want_change else None
    rc = raw_call((K, T, D, D, diag_flags(pb) | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, nu, n_iters, sc,
                  w0 is not None, ch, ms, Vs, ws=ws)
    assert rc == 0
    Vs = Vs.cpu().numpy()
    return (ms.cpu().numpy().reshape(T, K * D), Vs.reshape(T, K * D) if vs_diag else Vs,
            None if sc is None else sc.cpu().numpy(), None if ch is None else ch.cpu().numpy())


def edge_spots(T):
    """Frames 1 and T - 1, and jB - 1, jB, jB + 1 of the first, a middle and the last chunk."""
    nc = -(-T // B)
    spots = {1, T - 1}
    for j in {1, nc // 2, nc - 1}:
        spots |= {j * B - 1, j * B, j * B + 1}
    return sorted(t for t in spots if 1 <= t < T)


def session(T, K, D, kind, seed, sval=None, extra=True):
    """make_session centred at 50 px ('general': a = 0.98, c = 1.3 and a q of its own per chain), with jumps of all
    the coordinates of a keypoint: the edge frames on the even keypoints in turn (their neighbours keep none there) and
    about 1 % of the other (frame, keypoint) pairs.  s = 0.05 on unit chains; 2 on the decaying ones (s q in [1, 4]),
    whose model pulls towards 0 while the session stays near 50 px: a steady 1 px per frame that a smaller s q would
    itself count as a jump at every frame."""
    sval = (0.05 if kind == 'unit' else 2.0) if sval is None else sval
    spots = edge_spots(T)
    evens = list(range(0, K, 2))
    jumps = {(t, evens[i % len(evens)]) for i, t in enumerate(spots)}
    if extra and T > 2:
        taken = set(spots)
        jumps |= {(t, k) for t, k in jref.random_jumps(T, K, seed) if t not in taken}
    pb = make_session(T, K, D, sval, kind == 'unit', seed, a=0.98, c=1.3, centre=50.0)
    for t, k in jumps:          # make_session marks 2 % of the entries missing (var = 1e3, noise to match): not around
        sl = slice(k * D, (k + 1) * D)                           # a jump - the nearest observed frame stands in for them
        seen = np.flatnonzero((pb['var'][:, sl] <= 50).all(axis=1))
        for u in (t - 1, t):
            if (pb['var'][u, sl] > 50).any() and seen.size:
                near = seen[np.argmin(np.abs(seen - u))]
                pb['y'][u, sl], pb['var'][u, sl] = pb['y'][near, sl], pb['var'][near, sl]
    if kind != 'unit':
        q = np.random.default_rng(seed + 1).uniform(0.5, 2.0, K * D)
        pb['par']['Q'][:, np.arange(D), np.arange(D)] = q.reshape(K, D)
        pb['qs'] = q * sval
    pb = jref.add_jumps(pb, sorted(jumps), seed)
    pb['jumps'] = sorted(jumps)
    assert np.abs(pb['y']).max() <= 400 and pb['var'].min() >= 0.02 and pb['qs'].min() >= 1e-3
    return pb


def scalar_refs(pb, nu, counts, w0=None):
    """{n: (float64 result, float32 transcription's result, bars)} for calls of n passes."""
    D = pb['D']
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu, max(counts))
    s64, s32 = dict.fromkeys(counts), dict.fromkeys(counts)
    jref.scalar_jumps(*args, D=D, w0=w0, snapshots=s64)
    jref.scalar_jumps_f32(*args, D=D, w0=w0, unit=pb['unit'], B=B, snapshots=s32)
    return {n: (s64[n], s32[n], jref.bars(s32[n], s64[n], pb['y'], D)) for n in counts}


def check_scalar(label, pb, got, ref, worst=None, slack=1.0):
    r64, r32, bars = ref
    ms, Vs, w, ch = got
    assert all(np.isfinite(x).all() for x in got) and (Vs > 0).all() and (w > 0).all(), f'{label}: non-finite output'
    err, et = jref.errors(got, r64, pb['y'], pb['D']), jref.errors(r32, r64, pb['y'], pb['D'])
    for k in err:
        e, t = float(np.max(err[k])), float(np.max(et[k]))
        print(f'{label}: {k} {e:.3g} (transcription {t:.3g}, bar {bars[k]:.3g})')
        if worst is not None:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e, t))
        assert e <= slack * bars[k], f'{label}: {k} {e:.3g} over {slack} x bar {bars[k]:.3g} (transcription {t:.3g})'
    return bars


def u_in_range(w, nu, D):
    u = 1.0 / w.astype(np.float64)
    return bool(np.isfinite(w).all() and (u > 0).all() and (u <= (nu + D) / nu * (1 + 2.0 ** -23)).all())


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 2), (21, 3), (65, 1), (65, 2), (2, 8)])
def test_scalar_chain_edge_shapes(K, D, kind):
    """(2, 8): the largest D whose full Vs rows the scalar path writes."""
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
                assert u_in_range(got[2], nu, D) and (got[2][0] == 1).all(), label
                if n == 1:
                    assert (got[2] == 1).all() and not got[3].any(), label
    print(f'N={K * D} D={D} {kind}, worst kernels (transcription on that case): '
          + ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (e, t) in worst.items()))


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_jumps_at_the_chunk_edges_raise_their_own_frame_and_keypoint_only(kind):
    """Jumps entering frames 1, T - 1 and jB - 1, jB, jB + 1 of the first, a middle and the last chunk: the scale of
    that frame and keypoint is large (>= 20: a jump of 20 px in two coordinates has delta >= 2 x 400 / (s q) >= 200,
    and w = (4 + delta) / 6), in the reference and on the device, and every other scale - the keypoint next to it at
    that frame among them - stays calm: a contribution stored one frame or one keypoint off is shown here directly.
    Calm is <= 3 on the unit chains (s q = 0.05 against variances of 0.5 .. 4: heavy smoothing, delta near D); on the
    decaying chains s q is of the size of the observation noise, a 3-sigma step of the walk itself earns 4 .. 9 under
    nu = 4 in the reference, and calm is <= 12."""
    T, K, D = 33 * B + 1, 4, 2
    calm_max = 3 if kind == 'unit' else 12
    pb = session(T, K, D, kind, seed=5, extra=False)
    got = gpu_scalar(pb, 4.0, 8)
    ref = scalar_refs(pb, 4.0, (8,))[8]
    w, rw = got[2], ref[0][2]
    assert len(pb['jumps']) == len(edge_spots(T)) == 9
    calm = np.ones((T, K), bool)
    for t, k in pb['jumps']:
        calm[t, k] = False
        assert rw[t, k] >= 20 and rw[t, k + 1] <= calm_max, (t, k, rw[t, k], rw[t, k + 1])  # (the reference itself)
        assert w[t, k] >= 20, f'{kind}: the jump into frame {t} of keypoint {k} left the scale at {w[t, k]:.3g}'
        assert w[t, k + 1] <= calm_max, f'{kind}: keypoint {k + 1} has scale {w[t, k + 1]:.3g} at frame {t}'
    print(f'{kind}: scales at the jumps {w[~calm].min():.4g} .. {w[~calm].max():.4g}, elsewhere <= {w[calm].max():.3g}')
    assert rw[calm].max() <= calm_max and w[calm].max() <= calm_max
    check_scalar(f'{kind} jumps at the edges', pb, got, ref)


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('vs_diag', [True, False])
def test_outputs_are_eks_smooth_tv_under_the_returned_scales_bit_for_bit(kind, vs_diag):
    """n_iters = 1: scales all 1 and eks_smooth_tv's bits at w = 1; any n_iters: ms, Vs are eks_smooth_tv called with the
    returned scales as per-keypoint qscale."""
    from eks_amd import hip_ops
    for T, K, D in ((33 * B + 1, 21, 3), (B + 1, 3, 2), (700, 65, 1)):
        pb = session(T, K, D, kind, seed=T)
        ins = scalar_ins(pb)
        for n in (1, 4):
            ms, Vs, w, ch = gpu_scalar(pb, 4.0, n, vs_diag=vs_diag, ins=ins)
            if n == 1:
                assert (w == 1).all() and (ch == 0).all()
            else:
                assert w.max() >= 20 and ch.max() > 0
            tm, tV = hip_ops.smooth_tv(ins[0], ins[1], _dev(w), *ins[2:], flags=diag_flags(pb), vs_diag=vs_diag)
            torch.cuda.synchronize()
            assert np.array_equal(ms, tm.cpu().numpy().reshape(T, -1)), (kind, T, n)
            assert np.array_equal(Vs.reshape(T, -1), tV.cpu().numpy().reshape(T, -1)), (kind, T, n)


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_continuation_through_the_scales_gives_the_single_calls_bits(kind):
    T, K, D = 5 * B + 7, 5, 2
    pb = session(T, K, D, kind, seed=11)
    ins = scalar_ins(pb)
    whole8, whole7 = gpu_scalar(pb, 4.0, 8, ins=ins), gpu_scalar(pb, 4.0, 7, ins=ins)
    first = gpu_scalar(pb, 4.0, 3, ins=ins)
    cont = gpu_scalar(pb, 4.0, 6, w0=first[2], ins=ins)
    for a, b in zip(cont, whole8):
        assert np.array_equal(a, b), kind
    assert not np.array_equal(whole7[2], whole8[2])


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_one_pass_under_given_scales_smooths_under_them_and_returns_them(kind):
    T, K, D = 33 * B + 1, 21, 2
    pb = session(T, K, D, kind, seed=3)
    w0 = np.exp(np.random.default_rng(1).normal(0.0, 1.5, (T, K))).astype(np.float32)
    ms, Vs, w, ch = gpu_scalar(pb, 4.0, 1, w0=w0)
    assert np.array_equal(w[1:], w0[1:]) and (w[0] == 1).all() and not ch.any()
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], w0)
    r64 = tref.scalar_smooth_tv(*args, D=D)
    bars = tref.f32_bars(*tref.scalar_smooth_tv_f32(*args, D=D, unit=pb['unit']), *r64, pb['y'])
    err = tref.f32_errors(ms, Vs, *r64, pb['y'])
    assert float(err['ms'].max()) <= bars['ms'] and float(err['Vs'].max()) <= bars['Vs']


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_optional_outputs_two_calls_and_a_subset_of_the_keypoints(kind):
    """scales = NULL and / or change = NULL leave the other outputs' bits; two calls give the same bits; keypoints
    [3, 67) of K = 70 alone (another lane mapping) give the full call's bits."""
    T, K, D = 35 * B + 1, 70, 2
    pb = session(T, K, D, kind, seed=21)
    ins = scalar_ins(pb)
    full, again = gpu_scalar(pb, 4.0, 4, ins=ins), gpu_scalar(pb, 4.0, 4, ins=ins)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for ww, wc in ((False, True), (True, False), (False, False)):
        part = gpu_scalar(pb, 4.0, 4, want_scales=ww, want_change=wc, ins=ins)
        for a, b in zip(part, full):
            assert a is None or np.array_equal(a, b), (ww, wc)
    k0, k1 = 3, 67
    sub = gpu_scalar(subset(pb, k0, k1), 4.0, 4)
    assert np.array_equal(sub[0], full[0][:, D * k0:D * k1]) and np.array_equal(sub[1], full[1][:, D * k0:D * k1])
    assert np.array_equal(sub[2], full[2][:, k0:k1]) and np.array_equal(sub[3], full[3][k0:k1])


# ---- buffers and refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('diag', [True, False])
def test_guarded_workspace_and_outputs_at_an_offset(diag):
    """A workspace of exactly the queried size filled with 0xFF between guards, and ms, Vs, scales, change one element
    off their allocations' alignment: nothing outside their extents is touched, and the result is the bits of the plain
    call - with the caller's scales and with the workspace's plane."""
    from eks_amd import _lib
    if diag:
        pb = session(3 * B + 5, 5, 2, 'unit', seed=2)
        T, K, D, O = pb['T'], pb['K'], pb['D'], pb['D']
        ins, flags = scalar_ins(pb), diag_flags(pb) | _lib.FLAG_VS_DIAG
        plain = gpu_scalar(pb, 4.0, 3, ins=ins)
    else:
        M = stable(dense_case(3, 3, 4, False, seed=5))
        T, K, D, O = 70, 3, 3, 4
        y, var = dense_jumpy(M, T, O, seed=2)
        ins, flags = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS], _lib.FLAG_VS_DIAG
        plain = gpu_dense(M, y, var, 4.0, 3, vs_diag=True)
    dims = _lib.EksDims(K, T, D, O, flags)
    need = int(_lib.load().eks_smooth_jumps_workspace_bytes(ctypes.byref(dims)))
    gw = bg.GuardedWorkspaces(0xFF)
    ws = gw(need, 'cuda')
    assert ws.numel() == need
    for scales_given in (True, False):
        outs = dict(ms=bg.guarded_output((T, K, D), offset=1, name='ms'), Vs=bg.guarded_output((T, K, D), offset=1, name='Vs'),
                    scales=bg.guarded_output((T, K), offset=1, name='scales'),
                    change=bg.guarded_output((K,), offset=1, name='change'))
        rc = raw_call((K, T, D, O, flags), ins, 4.0, 3, outs['scales'].tensor if scales_given else None, 0,
                      outs['change'].tensor, outs['ms'].tensor, outs['Vs'].tensor, ws=ws)
        assert rc == 0
        gw.assert_intact()
        for o in outs.values():
            o.assert_intact()
        for name in (NAMES if scales_given else ('ms', 'Vs', 'change')):
            want = plain[NAMES.index(name)]
            assert np.array_equal(outs[name].tensor.cpu().numpy().reshape(want.shape), want), (name, scales_given)


@pytest.mark.parametrize('diag', [True, False])
def test_stale_and_poisoned_workspaces_give_the_same_bits(diag):
    from eks_amd import _lib
    if diag:
        pb = session(3 * B + 5, 5, 2, 'general', seed=6)
        other = session(3 * B + 5, 5, 2, 'general', seed=7)
        dims = _lib.EksDims(5, pb['T'], 2, 2, diag_flags(pb) | _lib.FLAG_VS_DIAG)
        run = lambda p, ws: gpu_scalar(p, 4.0, 4, want_scales=False, ws=ws)  # noqa: E731
        a, b = pb, other
    else:
        M = stable(dense_case(3, 3, 4, False, seed=5))
        dims = _lib.EksDims(3, 70, 3, 4, _lib.FLAG_VS_DIAG)
        a, b = dense_jumpy(M, 70, 4, seed=2), dense_jumpy(M, 70, 4, seed=3)
        run = lambda p, ws: gpu_dense(M, p[0], p[1], 4.0, 4, vs_diag=True, want_scales=False, ws=ws)  # noqa: E731
    need = int(_lib.load().eks_smooth_jumps_workspace_bytes(ctypes.byref(dims)))
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    clean = run(a, ws)
    run(b, ws)                                   # stale: another problem's planes, scales included
    stale = run(a, ws)
    ws.fill_(0xFF)                               # poisoned: NaN in every plane
    poisoned = run(a, ws)
    for other_run in (stale, poisoned):
        for x, y_ in zip(clean, other_run):
            assert x is None or np.array_equal(x, y_)


def test_refusals_leave_the_outputs_untouched():
    from eks_amd import _lib
    pb = session(100, 3, 2, 'unit', seed=2)
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = scalar_ins(pb)
    outs = [torch.full(shape, 7.0, dtype=torch.float32, device='cuda') for shape in ((T, K), (K,), (T, K, D), (T, K, D, D))]
    sc, ch, ms, Vs = outs
    diag = diag_flags(pb)
    untouched = lambda: all(bool((o == 7.0).all()) for o in outs)  # noqa: E731
    call = lambda dims, tensors=ins, nu=4.0, n=8, w=sc, w_in=0, c=ch, m=ms, V=Vs, **kw: raw_call(  # noqa: E731
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
    assert call(good, ws_bytes=tv) == -4 and untouched()                     # eks_smooth_tv's size lacks the planes
    assert call(good) == 0
    assert not any(bool((o == 7.0).any()) for o in outs)


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_extreme_inputs_keep_every_output_finite_and_u_in_range(kind):
    """var at 1e-12 and 1e30 and one chain with s q = 0: no parity bar (delta's cancellation error grows as var falls),
    but everything is finite, variances positive and u in (0, (nu + D) / nu]; a keypoint that is never observed keeps
    w = 1, the fixed point without data."""
    T, K, D = 7 * B + 3, 5, 2
    for nu in NUS:
        pb = session(T, K, D, kind, seed=9)
        rng = np.random.default_rng(2)
        pick = rng.random(pb['var'].shape)
        pb['var'][pick < 0.05] = 1e-12
        pb['var'][(pick > 0.05) & (pick < 0.10)] = 1e30
        pb['var'][3 * B:4 * B, 0] = 1e30                                    # a whole chunk of one chain missing
        pb['var'][:, 2:4] = 1e30                                            # keypoint 1 is never observed
        pb['par']['Q'][2, 1, 1] = 0.0                                       # chain 5: s q = 0
        for n in (2, 8):
            ms, Vs, w, ch = gpu_scalar(pb, nu, n)
            assert np.isfinite(ms).all() and np.isfinite(Vs).all() and (Vs > 0).all()
            assert u_in_range(w, nu, D)
            assert np.isfinite(ch).all() and (ch >= 0).all()
            assert np.abs(w[:, 1] - 1).max() < 1e-4


# ---- general models ------------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, nu, n_iters, vs_diag=False, w0=None, flags=0, want_scales=True, ws=None):
    from eks_amd import _lib
    T, K, O = y.shape
    D = M['m0'].shape[1]
    ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    if w0 is not None:
        sc = _dev(w0.astype(np.float32))
    else:
        sc = torch.full((T, K), np.nan, dtype=torch.float32, device='cuda') if want_scales else None
    ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda')
    assert raw_call((K, T, D, O, flags | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, nu, n_iters, sc, w0 is not None, ch,
                    ms, Vs, ws=ws) == 0
    return ms.cpu().numpy(), Vs.cpu().numpy(), None if sc is None else sc.cpu().numpy(), ch.cpu().numpy()


def dense_jumpy(M, T, O, seed):
    """dense_session with the state of about 2 % of the (frame, keypoint) pairs - frame T // 2 of keypoint 0 among
    them - displaced from that frame onwards by a random vector, seen through C, whose largest observed coordinate moves
    by 20 .. 60 px; a keypoint's jumps alternate in sign."""
    y, var = dense_session(M, T, O, seed)
    rng = np.random.default_rng(seed + 100)
    K, D = M['m0'].shape
    hit = rng.random((T, K)) < 0.02
    hit[0] = False
    if T > 3:
        hit[T // 2, 0] = True
    y = y.astype(np.float64)
    sign = np.ones(K)
    for t, k in np.argwhere(hit):
        dy = M['C'][k] @ rng.normal(size=D)
        y[t:, k] += dy * (sign[k] * rng.uniform(20.0, 60.0) / np.abs(dy).max())
        sign[k] = -sign[k]
    assert np.abs(y).max() <= 400
    return y.astype(np.float32), np.maximum(var, np.float32(0.02))


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


def dense_refs(M, y, var, nu, counts, w0=None):
    par = tuple(M[k] for k in PARAMS)
    out = []
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        snaps = dict.fromkeys(counts)
        jref.dense_jumps(y, var, *par, nu, max(counts), w0=w0, form=form, snapshots=snaps, w_dtype=np.float32)
        out.append(snaps)
    return out


def check_dense(label, got, seq, joint, worst=None):
    for i, name in enumerate(('ms', 'Vs', 'u', 'change')):
        g, a, b = got[i], seq[i], joint[i]
        assert np.isfinite(g).all(), f'{label}: {name} is not finite'
        if name == 'Vs' and g.ndim == 3:                                      # VS_DIAG
            a, b = (np.diagonal(x, axis1=2, axis2=3) for x in (a, b))
        if name == 'u':
            g, a, b = 1.0 / g.astype(np.float64), 1.0 / a, 1.0 / b
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
        y, var = dense_jumpy(M, T, O, seed=T)
        seq, joint = dense_refs(M, y, var, 4.0, (1, 3))
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            for n in (1, 3):
                got = gpu_dense(M, y, var, 4.0, n, vs_diag=(i % 2 == 0))
                check_dense(f'D={D} O={O} K={K} T={T} chunk={chunk} n_iters={n}', got, seq[n], joint[n], worst)
                assert u_in_range(got[2], 4.0, D)
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
    y, var = dense_jumpy(M, T, O, seed=3)
    seq, joint = dense_refs(M, y, var, 4.0, (1, 3))
    worst = {}
    for n in (1, 3):
        check_dense(f'{variant} n_iters={n}', gpu_dense(M, y, var, 4.0, n), seq[n], joint[n], worst)
    print(f'{variant}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('D,O', [(1, 1), (2, 3), (3, 4), (6, 12)])
def test_general_model_single_pass_agrees_with_the_generic_eks_smooth_tv(D, O):
    """n_iters = 1 is the generic eks_smooth_tv at w = 1 run on the plane, and a call of 3 passes ends on it under the
    returned scales: the same launches, the same bits."""
    from eks_amd import hip_ops
    M = stable(dense_case(3, D, O, False, seed=12))
    T = 300
    y, var = dense_jumpy(M, T, O, seed=4)
    for n in (1, 3):
        ms, Vs, w, _ = gpu_dense(M, y, var, 4.0, n)
        tm, tV = hip_ops.smooth_tv(_dev(y), _dev(var), _dev(w), *(_dev(M[k]) for k in PARAMS), flags=0)
        torch.cuda.synchronize()
        assert np.array_equal(ms, tm.cpu().numpy()) and np.array_equal(Vs, tV.cpu().numpy())


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_a_diagonal_model_down_the_general_path_agrees_with_the_scalar_path(kind):
    T, K, D = 5 * B + 7, 5, 2
    pb = session(T, K, D, kind, seed=4)
    refs = scalar_refs(pb, 4.0, (8,))[8]
    sc = gpu_scalar(pb, 4.0, 8)
    check_scalar(f'{kind} scalar path', pb, sc, refs)
    dn = gpu_dense(pb['par'], pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), 4.0, 8, vs_diag=True, flags=0)
    dn = (dn[0].reshape(T, -1), dn[1].reshape(T, -1), dn[2], dn[3])
    check_scalar(f'{kind} general path', pb, dn, refs)
    err = jref.errors(dn, [x.astype(np.float64) for x in sc], pb['y'], D)
    for k in err:
        assert float(np.max(err[k])) <= 2 * refs[2][k], (k, float(np.max(err[k])), refs[2][k])


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_smooth_jumps_matches_the_references_on_both_paths():
    from eks_amd import smooth_jumps
    pb = session(200, 3, 2, 'unit', seed=9)
    T, K, D = pb['T'], pb['K'], pb['D']
    par = pb['par']
    ms, Vs, w, ch = smooth_jumps(np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'],
                                 par['Q'], pb['var'].reshape(T, K, D), par['s'], nu=4.0, n_iters=8, vs_diag=True)
    assert ms.shape == (K, T, D) and Vs.shape == (K, T, D) and w.shape == (K, T) and ch.shape == (K,)
    assert ms.dtype == np.float32 and w.dtype == np.float32
    flat = lambda x: np.swapaxes(x, 0, 1).reshape(T, -1)  # noqa: E731
    check_scalar('smooth_jumps', pb, (flat(ms), flat(Vs), w.T, ch), scalar_refs(pb, 4.0, (8,))[8])
    M = stable(dense_case(3, 3, 4, False, seed=2))
    y, var = dense_jumpy(M, 120, 4, seed=5)
    ms, Vs, w, ch = smooth_jumps(np.swapaxes(y, 0, 1), M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'], n_iters=3)
    assert ms.shape == (3, 120, 3) and Vs.shape == (3, 120, 3, 3) and w.shape == (3, 120)
    seq, joint = dense_refs(M, y, var, 4.0, (3,))
    check_dense('smooth_jumps, general', (np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1), w.T, ch), seq[3], joint[3])


def test_tolerance_loop_stops_below_tol_and_is_a_single_call_of_the_same_pass_count():
    from eks_amd import smooth_jumps
    pb = session(300, 3, 2, 'unit', seed=13)
    T, K, D = pb['T'], pb['K'], pb['D']
    par = pb['par']
    args = (np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'], par['Q'],
            pb['var'].reshape(T, K, D), par['s'])
    tol, n = 0.05, 4
    looped = smooth_jumps(*args, nu=4.0, n_iters=n, tol=tol, max_iters=64, vs_diag=True)
    assert float(looped[3].max()) < tol
    total = n
    while True:                                   # blocks of n passes: each continued block adds n - 1 updates
        single = smooth_jumps(*args, nu=4.0, n_iters=total, vs_diag=True)
        if float(single[3].max()) < tol:
            break
        total += n - 1
        assert total <= 64
    assert total > n, 'the first block already met the tolerance: the loop was not exercised'
    for a, b in zip(looped, single):
        assert np.array_equal(a, b)
    capped = smooth_jumps(*args, nu=4.0, n_iters=n, tol=1e-30, max_iters=9, vs_diag=True)
    for a, b in zip(capped, smooth_jumps(*args, nu=4.0, n_iters=9, vs_diag=True)):
        assert np.array_equal(a, b)


def test_smooth_singlecam_jumps_on_the_golden_markers_with_a_displaced_keypoint(golden_dir):
    """Keypoint 1 moved by 40 px in every ensemble member from a chosen frame onwards - a true jump: that frame's scale
    is the keypoint's largest, and the result is what smooth_time_varying gives under the returned scales."""
    from eks_amd import smooth_singlecam_jumps
    from eks_amd.marker_array import MarkerArray
    from eks_amd.singlecam_smoother import ensemble_kalman_smoother_singlecam
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers'].astype(np.float64)
    names = [str(k) for k in g['keypoints']]
    M_, V, T, K, _ = mk.shape
    fields = ['x', 'y', 'likelihood']
    _, s = ensemble_kalman_smoother_singlecam(MarkerArray(mk, data_fields=fields), names, smooth_param=10.0)
    frame = T // 2 + 3
    moved = mk.copy()
    moved[:, :, frame:, 1, 0:2] += 40.0
    ma = MarkerArray(moved, data_fields=fields)
    out = smooth_singlecam_jumps(ma, names, s, nu=4.0, n_iters=12)
    gau = smooth_singlecam_jumps(ma, names, s, nu=4.0, n_iters=1)
    assert out['ms'].shape == (T, K, 2) and out['Vs'].shape == (T, K, 2) and out['scales'].shape == (T, K)
    assert (gau['scales'] == 1).all() and u_in_range(out['scales'], 4.0, 2) and (out['scales'][0] == 1).all()
    w = out['scales'][:, 1]
    print(f'golden markers, keypoint 1 moved by 40 px from frame {frame}: scale there {w[frame]:.4g}, next largest '
          f'{np.delete(w, frame).max():.4g}, median {np.median(w):.3g}')
    assert int(np.argmax(w)) == frame
