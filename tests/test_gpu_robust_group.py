"""GPU: eks_smooth_robust_group (eks_amd/csrc/eks_smooth_student.hip on scalar chains, dense_smooth_robust_group in
eks_dense.hip on general models) and the grouped functions of eks_amd.robust against the references of
tests/robust_group_ref.py, through the C ABI.

Bars.  Scalar chains (float32 lanes), the project's rule (robust_group_ref.bars): error / scale <= max(1e-5, 4 x the
float32 NumPy transcription's own worst error / scale on the same run) for ms, Vs and weights, and twice the weights'
bar for change, a maximum over the difference of two weight planes; scale of ms: the chain's max |y|; of Vs: its own
value; of weights and change: 1.
General models (float64 in the lane, weights kept in float32 - the reference rounds them there too): tests/
test_gpu_robust.py's rule, 100 x the disagreement of the two independent float64 reference forms, floored at 1e-12 and
capped at 1e-8, plus one float32 ulp of the reference value.  Inputs keep var >= 0.02 and |y| <= 400; about 2 % of the
(frame, group)s are displaced in all their coordinates at once by 3 .. 8 px, and the frames at the chunk edges by
20 .. 60 px.  Nothing is compared with the kernels' own output, except where the test is about bits.

Measured on the MI355X: DESIGN.md 9o has the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buffer_guard as bg  # noqa: E402
import robust_group_ref as gref  # noqa: E402
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402
from test_gpu_increments import PARAMS, _dev, dense_session, diag_flags, stable  # noqa: E402
from test_gpu_em import subset  # noqa: E402
from test_gpu_robust import check_dense, edge_spots, scalar_ins  # noqa: E402
from test_gpu_robust import raw_call as robust_raw_call  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B = 32                                        # kChainChunk: frames per lane of the scalar-chain kernels
T_EDGES = (1, 2, B - 1, B, B + 1, 33 * B + 1)
N_ITERS = (1, 2, 8)
NUS = (1.0, 4.0, 30.0)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def raw_call(dims_args, ins, nu, g, n_iters, weights, weights_in, change, ms, Vs, ws=None, ws_bytes=None):
    """eks_smooth_robust_group itself: ins = y, var, m0 .. s.  Returns the status."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*dims_args)
    if ws is None:
        need = int(lib.eks_smooth_robust_group_workspace_bytes(ctypes.byref(dims), int(g)))
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda')
    p = hip_ops._ptr
    rc = lib.eks_smooth_robust_group(ctypes.byref(dims), *[p(t) for t in ins], float(nu), int(g), int(n_iters), p(weights),
                                     int(weights_in), p(change), p(ms), p(Vs), p(ws),
                                     ws.numel() if ws_bytes is None else ws_bytes, hip_ops._stream())
    torch.cuda.synchronize()
    return rc


def gpu_scalar(pb, nu, g, n_iters, vs_diag=True, lam0=None, want_weights=True, want_change=True, ins=None, ws=None):
    """-> ms (T, N), Vs (T, N) or (T, K, D, D), weights (T, N / g), change (K,) as NumPy float32 (None: not asked for)."""
    from eks_amd import _lib
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = scalar_ins(pb) if ins is None else ins
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    if lam0 is not None:
        wt = _dev(np.ascontiguousarray(lam0, np.float32).reshape(T, K, D // g))
    else:
        wt = torch.full((T, K, D // g), np.nan, dtype=torch.float32, device='cuda') if want_weights else None
    ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda') if want_change else None
    rc = raw_call((K, T, D, D, diag_flags(pb) | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, nu, g, n_iters, wt,
                  lam0 is not None, ch, ms, Vs, ws=ws)
    assert rc == 0
    Vs = Vs.cpu().numpy()
    return (ms.cpu().numpy().reshape(T, K * D), Vs.reshape(T, K * D) if vs_diag else Vs,
            None if wt is None else wt.cpu().numpy().reshape(T, K * D // g), None if ch is None else ch.cpu().numpy())


def session(T, K, D, g, kind, seed, spots=None):
    """make_session centred at 50 px ('general': a = 0.98, c = 1.3 and a q of its own per chain); about 2 % of the
    (frame, group)s displaced in all g coordinates by 3 .. 8 px, and the group i of every frame of `spots` (default:
    edge_spots) by +(20 .. 60) px with var = 1 there - upwards, away from zero: ms is held to the chain's max |y|, and
    a single-frame chain moved from 50 px to 0.4 px has one float32 ulp of its ms = 31 at 1e-5 of that scale whatever
    the arithmetic does.  pb['hit']: (T, N / g), the displaced groups."""
    pb = make_session(T, K, D, 2.0, kind == 'unit', seed, a=0.98, c=1.3, centre=50.0)
    if kind != 'unit':
        q = np.random.default_rng(seed + 1).uniform(0.5, 2.0, K * D)
        pb['par']['Q'][:, np.arange(D), np.arange(D)] = q.reshape(K, D)
        pb['qs'] = q * 2.0
    rng = np.random.default_rng(seed)
    N, NG = K * D, K * D // g
    hit = rng.random((T, NG)) < 0.02
    amp = rng.uniform(3, 8, (T, N))
    sign = rng.choice([-1.0, 1.0], (T, N))
    for i, t in enumerate(edge_spots(T) if spots is None else spots):
        q = i % NG
        hit[t, q] = True
        pb['var'][t, q * g:(q + 1) * g] = 1.0
        amp[t, q * g:(q + 1) * g] = rng.uniform(20, 60, g)
        sign[t, q * g:(q + 1) * g] = 1.0
    pb['y'] = (pb['y'] + np.repeat(hit, g, axis=1) * sign * amp).astype(np.float32)
    pb['hit'] = hit
    assert np.abs(pb['y']).max() <= 400 and pb['var'].min() >= 0.02
    return pb


def scalar_refs(pb, nu, g, counts, lam0=None):
    """{n: (float64 result, float32 transcription's result)} and {n: bars} for calls of n passes."""
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], nu, g, pb['D'], max(counts))
    s64, s32 = dict.fromkeys(counts), dict.fromkeys(counts)
    gref.scalar_robust_group(*args, lam0=lam0, snapshots=s64)
    gref.scalar_robust_group_f32(*args, lam0=lam0, unit=pb['unit'], snapshots=s32)
    out = {n: (s64[n], s32[n]) for n in counts}
    return out, {n: gref.bars(s32[n], s64[n], pb['y']) for n in counts}


def check_scalar(label, pb, got, ref, bars, worst=None, slack=1.0):
    r64, r32 = ref
    ms, Vs, lam, ch = got
    assert all(np.isfinite(x).all() for x in got) and (Vs > 0).all() and (lam > 0).all(), f'{label}: non-finite output'
    err, et = gref.errors(got, r64, pb['y']), gref.errors(r32, r64, pb['y'])
    for k in err:
        e, t = float(np.max(err[k])), float(np.max(et[k]))
        if worst is not None:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e, t))
        assert e <= slack * bars[k], f'{label}: {k} {e:.3g} over {slack} x bar {bars[k]:.3g} (transcription {t:.3g})'


SHAPES = [(1, 2, 2), (3, 2, 2), (21, 3, 3), (21, 3, 1), (65, 2, 2), (33, 4, 2), (11, 6, 3), (11, 6, 2)]


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('K,D,g', SHAPES)
def test_scalar_chain_edge_shapes(K, D, g, kind):
    worst = {}
    for T in T_EDGES:
        pb = session(T, K, D, g, kind, seed=T + K)
        ins = scalar_ins(pb)
        for nu in NUS:
            refs, bars = scalar_refs(pb, nu, g, N_ITERS)
            for n in N_ITERS:
                got = gpu_scalar(pb, nu, g, n, ins=ins)
                label = f'K={K} D={D} g={g} T={T} {kind} nu={nu} n_iters={n}'
                check_scalar(label, pb, got, refs[n], bars[n], worst)
                assert (got[2] <= np.float32((nu + g) / nu)).all(), label
                if n == 1:
                    assert (got[2] == 1).all() and not got[3].any(), label
    print(f'K={K} D={D} g={g} {kind}, worst kernels (transcription on that case): '
          + ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (e, t) in worst.items()))


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_displaced_groups_at_the_chunk_edges_get_their_own_weight_and_leave_the_other_groups_alone(kind):
    """Events isolated: the groups displaced at jB - 1, jB, jB + 1, 0 and T - 1 carry a small weight in exactly their own
    column and frame, in the reference and on the device alike; the OTHER groups of the same keypoint and frame sit at
    the reference's value within the bar (a contribution summed one chain or one frame off would show here)."""
    T, K, D, g = 33 * B + 1, 2, 6, 2
    pb = session(T, K, D, g, kind, seed=5)
    refs, bars = scalar_refs(pb, 4.0, g, (8,))
    bars = bars[8]
    got = gpu_scalar(pb, 4.0, g, 8)
    lam, ref = got[2], refs[8][0][2]
    per = D // g
    others = []
    for i, t in enumerate(edge_spots(T)):
        q = i % (K * per)
        assert ref[t, q] < 0.2 and lam[t, q] < 0.2, f'{kind}: displaced group {q} of frame {t}: {ref[t, q]:.3g}, {lam[t, q]:.3g}'
        k = q // per
        for o in range(k * per, (k + 1) * per):
            if o != q and not pb['hit'][t, o]:
                others.append((ref[t, o], lam[t, o]))
    others = np.array(others)
    print(f'{kind}: other groups of the displaced frames: reference {others[:, 0].min():.3g} .. {others[:, 0].max():.3g}, '
          f'worst device - reference {np.abs(others[:, 1] - others[:, 0]).max():.3g} (bar {bars["weights"]:.3g})')
    assert others[:, 0].min() > 0.3                                          # (the reference leaves them unmarked)
    assert np.abs(others[:, 1] - others[:, 0]).max() <= bars['weights']
    check_scalar(f'{kind} displaced groups', pb, got, refs[8], bars)


# ---- equal bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_group_of_one_returns_the_bits_of_eks_smooth_robust(kind):
    from eks_amd import _lib
    for T, K, D in ((5 * B + 7, 21, 3), (B + 1, 3, 2)):
        pb = session(T, K, D, 1, kind, seed=T)
        ins = scalar_ins(pb)
        got = gpu_scalar(pb, 4.0, 1, 4, ins=ins)
        ms, Vs, wt = (torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda') for _ in range(3))
        ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda')
        assert robust_raw_call((K, T, D, D, diag_flags(pb) | _lib.FLAG_VS_DIAG), ins, 4.0, 4, wt, 0, ch, ms, Vs) == 0
        for a, b in zip(got, (ms, Vs, wt, ch)):
            assert np.array_equal(a.ravel(), b.cpu().numpy().ravel()), (kind, T)
    M = stable(dense_case(3, 3, 4, False, seed=5))
    y, var = dense_displaced(M, 70, 4, 1, seed=2)
    got = gpu_dense(M, y, var, 4.0, 1, 3)
    ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
    ms, Vs = torch.zeros((70, 3, 3), device='cuda'), torch.zeros((70, 3, 3, 3), device='cuda')
    wt, ch = torch.zeros((70, 3, 4), device='cuda'), torch.zeros((3,), device='cuda')
    assert robust_raw_call((3, 70, 3, 4, 0), ins, 4.0, 3, wt, 0, ch, ms, Vs) == 0
    for a, b in zip(got, (ms, Vs, wt, ch)):
        assert np.array_equal(a, b.cpu().numpy())


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_continuation_through_the_weights_gives_the_single_calls_bits(kind):
    T, K, D, g = 5 * B + 7, 5, 2, 2
    pb = session(T, K, D, g, kind, seed=11)
    ins = scalar_ins(pb)
    whole8, whole7 = gpu_scalar(pb, 4.0, g, 8, ins=ins), gpu_scalar(pb, 4.0, g, 7, ins=ins)
    first = gpu_scalar(pb, 4.0, g, 3, ins=ins)
    for n2, whole in ((6, whole8), (5, whole7)):
        cont = gpu_scalar(pb, 4.0, g, n2, lam0=first[2], ins=ins)
        for a, b in zip(cont, whole):
            assert np.array_equal(a, b), (kind, n2)
    assert not np.array_equal(whole7[2], whole8[2])


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_optional_outputs_two_calls_and_a_subset_of_the_keypoints(kind):
    """weights = NULL or change = NULL leave the other outputs' bits; two calls give the same bits; keypoints [3, 67)
    of K = 70 alone (another lane mapping, in the chains and in the combine) give the full call's bits."""
    T, K, D, g = 35 * B + 1, 70, 2, 2
    pb = session(T, K, D, g, kind, seed=21)
    ins = scalar_ins(pb)
    full, again = gpu_scalar(pb, 4.0, g, 4, ins=ins), gpu_scalar(pb, 4.0, g, 4, ins=ins)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for ww, wc in ((False, True), (True, False)):
        part = gpu_scalar(pb, 4.0, g, 4, want_weights=ww, want_change=wc, ins=ins)
        for a, b in zip(part, full):
            assert a is None or np.array_equal(a, b), (ww, wc)
    k0, k1 = 3, 67
    sub = gpu_scalar(subset(pb, k0, k1), 4.0, g, 4)
    for a, b in zip(sub[:2], full[:2]):
        assert np.array_equal(a, b[:, D * k0:D * k1])
    assert np.array_equal(sub[2], full[2][:, k0 * D // g:k1 * D // g]) and np.array_equal(sub[3], full[3][k0:k1])


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('vs_diag', [True, False])
def test_one_pass_under_caller_weights_against_eks_smooth_tv(kind, vs_diag):
    """weights_in, n_iters = 1: the weights come back as they went in, change stays 0, and ms, Vs agree with
    eks_smooth_tv at w = 1 on clip(var) / weights expanded to coordinates: bar 1e-5, twice allowed between two
    kernels."""
    from eks_amd import hip_ops
    T, K, D, g = 33 * B + 1, 21, 4, 2
    pb = session(T, K, D, g, kind, seed=3)
    lam0 = np.random.default_rng(1).uniform(0.01, 1.5, (T, K * D // g)).astype(np.float32)
    ins = scalar_ins(pb)
    ms, Vs, lam, ch = gpu_scalar(pb, 4.0, g, 1, vs_diag=vs_diag, lam0=lam0, ins=ins)
    assert np.array_equal(lam, lam0) and not ch.any()
    r_eff = np.clip(pb['var'], np.float32(1e-12), np.float32(1e30)) / gref.expand(lam0, g)
    tm, tV = hip_ops.smooth_tv(ins[0], _dev(r_eff.reshape(T, K, D)), _dev(np.ones(T, np.float32)), *ins[2:],
                               flags=diag_flags(pb), vs_diag=vs_diag)
    torch.cuda.synchronize()
    tm, tV = tm.cpu().numpy().reshape(T, -1).astype(np.float64), tV.cpu().numpy().astype(np.float64)
    e_ms = (np.abs(ms - tm).max(axis=0) / np.abs(pb['y']).max(axis=0)).max()
    if vs_diag:
        e_Vs = np.abs(Vs / tV.reshape(T, -1) - 1).max()
    else:
        e_Vs = np.abs(np.diagonal(Vs, axis1=2, axis2=3) / np.diagonal(tV, axis1=2, axis2=3) - 1).max()
        assert np.array_equal(Vs == 0, tV == 0)
    print(f'{kind} vs_diag={vs_diag}: one pass under caller weights against eks_smooth_tv: ms {e_ms:.3g}, Vs {e_Vs:.3g}')
    assert e_ms <= 2e-5 and e_Vs <= 2e-5


# ---- edge inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_extreme_inputs_keep_every_output_finite_and_the_weights_in_range(kind):
    """var at 1e-12 and 1e30, a keypoint that is never observed, a chain with s q = 0: no parity bar (delta's
    cancellation error is (2^-24 |y|)^2 / r), but everything is finite, variances positive, 0 < weights <= (nu + g) / nu,
    and the keypoint that is never observed keeps weight 1."""
    T, K, D, g = 7 * B + 3, 5, 2, 2
    for nu in NUS:
        pb = session(T, K, D, g, kind, seed=9)
        pick = np.random.default_rng(2).random(pb['var'].shape)
        pb['var'][pick < 0.05] = 1e-12
        pb['var'][(pick > 0.05) & (pick < 0.10)] = 1e30
        pb['var'][3 * B:4 * B, 0] = 1e30                                    # a whole chunk of one chain missing
        pb['var'][:, 2:4] = np.inf                                          # keypoint 1 is never observed
        pb['par']['Q'][2, 0, 0] = 0.0                                       # a chain with s q = 0
        for n in (2, 8):
            ms, Vs, lam, ch = gpu_scalar(pb, nu, g, n)
            assert np.isfinite(ms).all() and np.isfinite(Vs).all() and (Vs > 0).all()
            assert np.isfinite(lam).all() and (lam > 0).all() and (lam <= np.float32((nu + g) / nu)).all()
            assert np.isfinite(ch).all() and (ch >= 0).all() and ch[1] == 0
            assert (lam[:, 1] == 1).all()
            gone = (pb['var'].reshape(T, K, D) >= 1e30).all(axis=2)
            assert (lam[gone] == 1).all()
    M = stable(dense_case(3, 3, 4, False, seed=5))
    y, var = dense_displaced(M, 70, 4, 2, seed=2)
    var[:, 1] = np.inf
    var[10:20, 0, 0] = 1e-12
    var[30:40, 0, 2:] = 1e30
    ms, Vs, lam, ch = gpu_dense(M, y, var, 4.0, 2, 3)
    assert np.isfinite(ms).all() and np.isfinite(Vs).all() and (np.diagonal(Vs, axis1=2, axis2=3) > 0).all()
    assert (lam > 0).all() and (lam <= np.float32(1.5)).all() and (lam[:, 1] == 1).all() and (lam[30:40, 0, 1] == 1).all()


# ---- general models ------------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, nu, g, n_iters, vs_diag=False, lam0=None, flags=0, ws=None):
    from eks_amd import _lib
    T, K, O = y.shape
    D = M['m0'].shape[1]
    ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    wt = torch.full((T, K, O // g), np.nan, dtype=torch.float32, device='cuda') if lam0 is None \
        else _dev(lam0.astype(np.float32))
    ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda')
    assert raw_call((K, T, D, O, flags | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, nu, g, n_iters, wt, lam0 is not None,
                    ch, ms, Vs, ws=ws) == 0
    return ms.cpu().numpy(), Vs.cpu().numpy(), wt.cpu().numpy(), ch.cpu().numpy()


def dense_displaced(M, T, O, g, seed):
    """dense_session with about 2 % of the (frame, keypoint, group)s displaced in all g coordinates by 20 .. 60 px."""
    y, var = dense_session(M, T, O, seed)
    rng = np.random.default_rng(seed + 100)
    hit = rng.random((T, y.shape[1], O // g)) < 0.02
    if T > 3:
        hit[T // 2, 0, 0] = True
    hit = np.repeat(hit, g, axis=2)
    y = (y + hit * rng.choice([-1.0, 1.0], y.shape) * rng.uniform(20, 60, y.shape)).astype(np.float32)
    return y, np.maximum(var, np.float32(0.02))


def dense_refs(M, y, var, nu, g, counts):
    par = tuple(M[k] for k in PARAMS)
    out = []
    for form in (tref.dense_smooth_tv, tref.dense_smooth_tv_joint):
        snaps = dict.fromkeys(counts)
        gref.dense_robust_group(y, var, *par, nu, g, max(counts), form=form, snapshots=snaps, lam_dtype=np.float32)
        out.append(snaps)
    return out


@pytest.mark.parametrize('K', [1, 3, 65])
@pytest.mark.parametrize('D,O,g', [(1, 1, 1), (2, 4, 2), (3, 4, 4), (3, 6, 2), (3, 6, 3), (6, 12, 2), (3, 64, 2)])
def test_general_models_against_the_two_float64_forms(D, O, g, K, set_knob):
    M = stable(dense_case(K, D, O, False, seed=7 * D + O + K))
    worst = {}
    for i, T in enumerate((1, 2, 17, 33, 70) if O < 64 else (1, 33)):
        y, var = dense_displaced(M, T, O, g, seed=T)
        seq, joint = dense_refs(M, y, var, 4.0, g, (1, 3))
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            for n in (1, 3):
                got = gpu_dense(M, y, var, 4.0, g, n, vs_diag=(i % 2 == 0))
                check_dense(f'D={D} O={O} g={g} K={K} T={T} chunk={chunk} n_iters={n}', got, seq[n], joint[n], worst)
                if n == 1:
                    assert (got[2] == 1).all() and not got[3].any()
    print(f'general D={D} O={O} g={g} K={K}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('variant', ['two_scan_blocks', 'unit_root', 'singular_q'])
def test_general_model_variants(variant, set_knob):
    """ceil(T / 16) > 64 chunks (two blocks of dense_scan_kernel); A = I; a rank D - 1 Q."""
    D, O, K, g = 3, 4, 3, 2
    T = 1100 if variant == 'two_scan_blocks' else 100
    set_knob('EKS_DENSE_CHUNK', '16')
    M = stable(dense_case(K, D, O, variant == 'singular_q', seed=8), unit_root=variant == 'unit_root')
    if variant == 'singular_q':
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    y, var = dense_displaced(M, T, O, g, seed=3)
    seq, joint = dense_refs(M, y, var, 4.0, g, (1, 3))
    worst = {}
    for n in (1, 3):
        check_dense(f'{variant} n_iters={n}', gpu_dense(M, y, var, 4.0, g, n), seq[n], joint[n], worst)
    print(f'{variant}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


def test_general_model_continuation_bit_for_bit():
    M = stable(dense_case(3, 3, 6, False, seed=5))
    y, var = dense_displaced(M, 70, 6, 3, seed=2)
    whole = gpu_dense(M, y, var, 4.0, 3, 8)
    first = gpu_dense(M, y, var, 4.0, 3, 3)
    cont = gpu_dense(M, y, var, 4.0, 3, 6, lam0=first[2])
    for a, b in zip(cont, whole):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('D,g', [(2, 2), (6, 3)])
def test_a_diagonal_model_down_the_general_path_agrees_with_the_scalar_path(kind, D, g):
    T, K = 5 * B + 7, 5
    pb = session(T, K, D, g, kind, seed=4)
    refs, bars = scalar_refs(pb, 4.0, g, (8,))
    bars = bars[8]
    sc = gpu_scalar(pb, 4.0, g, 8)
    check_scalar(f'{kind} scalar path', pb, sc, refs[8], bars)
    dn = gpu_dense(pb['par'], pb['y'].reshape(T, K, D), pb['var'].reshape(T, K, D), 4.0, g, 8, vs_diag=True, flags=0)
    dn = (dn[0].reshape(T, -1), dn[1].reshape(T, -1), dn[2].reshape(T, -1), dn[3])
    check_scalar(f'{kind} general path', pb, dn, refs[8], bars)
    err = gref.errors(dn, [x.astype(np.float64) for x in sc], pb['y'])
    for k in err:
        assert float(np.max(err[k])) <= 2 * bars[k], (k, float(np.max(err[k])), bars[k])


# ---- the demonstration session -------------------------------------------------------------------------------------------
def test_demonstration_session_on_the_device():
    """tests/test_robust_group_cpu.py's session (seeds 0..7 as eight keypoints): the device agrees with the float64
    reference within the bars under g = 1 and g = 2, and marks the frames the reference marks, one either way."""
    S = [gref.joint_session(seed) for seed in range(8)]
    y, var = (np.concatenate([s[k] for s in S], axis=1).astype(np.float32) for k in ('y', 'var'))
    bad = np.stack([s['bad'] for s in S], axis=1)
    T, K, D = y.shape[0], 8, 2
    eye = np.tile(np.eye(2), (K, 1, 1))
    pb = dict(T=T, K=K, D=D, N=K * D, unit=True, y=y, var=var, m0f=np.zeros(K * D), S0d=np.full(K * D, 100.0), a=np.ones(K * D),
              c=np.ones(K * D), qs=np.full(K * D, 0.05),
              par=dict(m0=np.zeros((K, D)), S0=100.0 * eye, A=eye, C=eye, Q=eye, s=np.full(K, 0.05)))
    for g in (1, 2):
        refs, bars = scalar_refs(pb, 4.0, g, (8,))
        bars = bars[8]
        got = gpu_scalar(pb, 4.0, g, 8)
        check_scalar(f'demonstration g={g}', pb, got, refs[8], bars)
        if g == 2:
            for k in range(K):
                want, have = (int((lam[bad[:, k], k] <= 0.3).sum()) for lam in (refs[8][0][2], got[2]))
                assert abs(want - have) <= 1 and want >= 6, (k, want, have)


# ---- buffers and refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('diag', [True, False])
def test_guarded_workspace_and_outputs_at_an_offset(diag):
    """A workspace of exactly the queried size filled with 0xFF between guards, and ms, Vs, weights, change one element
    off their allocations' alignment: nothing outside their extents is touched, and the result is the bits of the plain
    call - with the caller's plane and with the workspace's."""
    from eks_amd import _lib
    g = 2
    if diag:
        pb = session(3 * B + 5, 5, 4, g, 'unit', seed=2)
        T, K, D, O = pb['T'], pb['K'], pb['D'], pb['D']
        ins, flags = scalar_ins(pb), diag_flags(pb) | _lib.FLAG_VS_DIAG
        plain = gpu_scalar(pb, 4.0, g, 3, ins=ins)
    else:
        M = stable(dense_case(3, 3, 4, False, seed=5))
        T, K, D, O = 70, 3, 3, 4
        y, var = dense_displaced(M, T, O, g, seed=2)
        ins, flags = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS], _lib.FLAG_VS_DIAG
        plain = gpu_dense(M, y, var, 4.0, g, 3, vs_diag=True)
    dims = _lib.EksDims(K, T, D, O, flags)
    need = int(_lib.load().eks_smooth_robust_group_workspace_bytes(ctypes.byref(dims), g))
    gw = bg.GuardedWorkspaces(0xFF)
    ws = gw(need, 'cuda')
    assert ws.numel() == need
    for weights_given in (True, False):
        outs = dict(ms=bg.guarded_output((T, K, D), offset=1, name='ms'), Vs=bg.guarded_output((T, K, D), offset=1, name='Vs'),
                    weights=bg.guarded_output((T, K, O // g), offset=1, name='weights'),
                    change=bg.guarded_output((K,), offset=1, name='change'))
        rc = raw_call((K, T, D, O, flags), ins, 4.0, g, 3, outs['weights'].tensor if weights_given else None, 0,
                      outs['change'].tensor, outs['ms'].tensor, outs['Vs'].tensor, ws=ws)
        assert rc == 0
        gw.assert_intact()
        for o in outs.values():
            o.assert_intact()
        names = ('ms', 'Vs', 'weights', 'change') if weights_given else ('ms', 'Vs', 'change')
        for name in names:
            want = plain[('ms', 'Vs', 'weights', 'change').index(name)]
            assert np.array_equal(outs[name].tensor.cpu().numpy().reshape(want.shape), want), (name, weights_given)


@pytest.mark.parametrize('diag', [True, False])
def test_stale_and_poisoned_workspaces_give_the_same_bits(diag):
    from eks_amd import _lib
    g = 2
    if diag:
        pb, other = session(3 * B + 5, 5, 4, g, 'general', seed=6), session(3 * B + 5, 5, 4, g, 'general', seed=7)
        dims = _lib.EksDims(5, pb['T'], 4, 4, diag_flags(pb) | _lib.FLAG_VS_DIAG)
        run = lambda p, ws: gpu_scalar(p, 4.0, g, 4, want_weights=False, ws=ws)  # noqa: E731
        a, b = pb, other
    else:
        M = stable(dense_case(3, 3, 4, False, seed=5))
        dims = _lib.EksDims(3, 70, 3, 4, _lib.FLAG_VS_DIAG)
        a, b = dense_displaced(M, 70, 4, g, seed=2), dense_displaced(M, 70, 4, g, seed=3)

        def run(p, ws):
            T, K, D, O = 70, 3, 3, 4
            ins = [_dev(p[0]), _dev(p[1])] + [_dev(M[k]) for k in PARAMS]
            ms, Vs = (torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda') for _ in range(2))
            ch = torch.full((K,), np.nan, dtype=torch.float32, device='cuda')
            assert raw_call((K, T, D, O, _lib.FLAG_VS_DIAG), ins, 4.0, g, 4, None, 0, ch, ms, Vs, ws=ws) == 0
            return ms.cpu().numpy(), Vs.cpu().numpy(), None, ch.cpu().numpy()
    need = int(_lib.load().eks_smooth_robust_group_workspace_bytes(ctypes.byref(dims), g))
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    clean = run(a, ws)
    run(b, ws)                                   # stale: another problem's planes, the weights included
    stale = run(a, ws)
    ws.fill_(0xFF)                               # poisoned: NaN in every plane
    poisoned = run(a, ws)
    for other_run in (stale, poisoned):
        for x, y_ in zip(clean, other_run):
            assert x is None or np.array_equal(x, y_)


def test_refusals_leave_the_outputs_untouched():
    from eks_amd import _lib
    pb = session(100, 3, 4, 2, 'unit', seed=2)
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = scalar_ins(pb)
    outs = [torch.full(shape, 7.0, dtype=torch.float32, device='cuda') for shape in ((T, K, D // 2), (K,), (T, K, D), (T, K, D, D))]
    wt, ch, ms, Vs = outs
    diag = diag_flags(pb)
    untouched = lambda: all(bool((o == 7.0).all()) for o in outs)  # noqa: E731
    call = lambda dims, tensors=ins, nu=4.0, g=2, n=8, w=wt, w_in=0, c=ch, m=ms, V=Vs, **kw: raw_call(  # noqa: E731
        dims, tensors, nu, g, n, w, w_in, c, m, V, **kw)
    good = (K, T, D, D, diag)
    cases = [
        (call(good, g=0), -2), (call(good, g=-1), -2), (call(good, g=3), -2), (call((K, T, 3, 4, 0), g=3), -2),
        (call(good, nu=0.0), -2), (call(good, nu=-1.0), -2), (call(good, nu=float('nan')), -2),
        (call(good, nu=float('inf')), -2), (call(good, n=0), -2), (call(good, n=-1), -2),
        (call((K, T, 3, 4, 0), nu=0.0), -2), (call((K, T, 3, 4, 0), n=0), -2),
        (call(good, w=None, w_in=1), -1), (call((K, T, 3, 4, 0), w=None, w_in=1), -1),
        (call(good, tensors=ins[:3] + [None] + ins[4:]), -1), (call(good, m=None), -1), (call(good, V=None), -1),
        (call((0, T, D, D, diag)), -2), (call((K, 0, D, D, diag)), -2), (call((K, T, D, D + 1, diag)), -2),
        (call((K, T, D, D, _lib.FLAG_UNIT_AC)), -3), (call((K, T, 7, 8, 0)), -3), (call((K, T, D, 66, 0)), -3),
        (call((K, T, 10, 10, diag)), -3), (call(good, ws_bytes=255), -4), (call((K, T, 3, 4, 0), ws_bytes=255), -4),
    ]
    for i, (got, want) in enumerate(cases):
        assert got == want, (i, got, want)
    assert untouched()
    rb = int(_lib.load().eks_smooth_robust_workspace_bytes(ctypes.byref(_lib.EksDims(*good))))
    assert call(good, ws_bytes=rb) == -4 and untouched()                     # eks_smooth_robust's size lacks the contribution plane
    assert call(good) == 0
    assert not any(bool((o == 7.0).any()) for o in outs)


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_smooth_robust_grouped_matches_the_references_and_its_tolerance_loop_is_a_single_call():
    from eks_amd import smooth_robust_grouped
    pb = session(300, 3, 4, 2, 'unit', seed=9)
    T, K, D = pb['T'], pb['K'], pb['D']
    par = pb['par']
    args = (np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'], par['Q'],
            pb['var'].reshape(T, K, D), par['s'])
    ms, Vs, lam, ch = smooth_robust_grouped(*args, group=2, nu=4.0, n_iters=8, vs_diag=True)
    assert ms.shape == (K, T, D) and Vs.shape == (K, T, D) and lam.shape == (K, T, D // 2) and ch.shape == (K,)
    assert ms.dtype == np.float32 and lam.dtype == np.float32
    flat = lambda x: np.swapaxes(x, 0, 1).reshape(T, -1)  # noqa: E731
    refs, bars = scalar_refs(pb, 4.0, 2, (8,))
    bars = bars[8]
    check_scalar('smooth_robust_grouped', pb, (flat(ms), flat(Vs), flat(lam), ch), refs[8], bars)
    tol, n = 1e-3, 4
    looped = smooth_robust_grouped(*args, group=2, nu=4.0, n_iters=n, tol=tol, max_iters=64, vs_diag=True)
    assert float(looped[3].max()) < tol
    total = n
    while True:                                   # blocks of n passes: each continued block adds n - 1 updates
        single = smooth_robust_grouped(*args, group=2, nu=4.0, n_iters=total, vs_diag=True)
        if float(single[3].max()) < tol:
            break
        total += n - 1
        assert total <= 64
    assert total > n, 'the first block already met the tolerance: the loop was not exercised'
    for a, b in zip(looped, single):
        assert np.array_equal(a, b)
    M = stable(dense_case(3, 3, 4, False, seed=2))
    y, var = dense_displaced(M, 120, 4, 2, seed=5)
    ms, Vs, lam, ch = smooth_robust_grouped(np.swapaxes(y, 0, 1), M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'],
                                            group=2, n_iters=3)
    assert ms.shape == (3, 120, 3) and Vs.shape == (3, 120, 3, 3) and lam.shape == (3, 120, 2)
    seq, joint = dense_refs(M, y, var, 4.0, 2, (3,))
    check_dense('smooth_robust_grouped, general', (np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1), np.swapaxes(lam, 0, 1), ch),
                seq[3], joint[3])


def test_smooth_singlecam_robust_grouped_on_the_golden_markers_with_a_displaced_keypoint(golden_dir):
    """40 isolated frames of one keypoint moved by 30 px in both coordinates in every ensemble member, s the one
    recorded with the markers: the driver agrees with the float64 reference on the model it builds within the bars, and
    marks (weight <= 0.3) the frames the reference marks, one either way - on the displaced keypoint and, falsely, on
    the others."""
    from eks_amd import smooth_singlecam_robust_grouped
    from eks_amd._problem import singlecam_problem
    from eks_amd.marker_array import MarkerArray
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers'].astype(np.float64)
    names = [str(k) for k in g['keypoints']]
    s = g['adam_s'].astype(np.float64)
    M_, V, T, K, _ = mk.shape
    frames = 5 + 3 * np.random.default_rng(0).choice((T - 10) // 3, size=40, replace=False)   # isolated
    mk[:, :, frames, 1, 0:2] += 30.0
    ma = MarkerArray(mk, data_fields=['x', 'y', 'likelihood'])
    out = smooth_singlecam_robust_grouped(ma, names, s, nu=4.0, n_iters=8)
    assert out['ms'].shape == (T, K, 2) and out['Vs'].shape == (T, K, 2) and out['weights'].shape == (T, K)
    (ys, m0s, S0s, As, Cs, Qs, evs), _, mu = singlecam_problem(None, ma, names, 'median', 'confidence_weighted_var')
    dg = lambda a: np.diagonal(a, axis1=1, axis2=2).reshape(-1)  # noqa: E731
    y2 = np.swapaxes(ys, 0, 1).reshape(T, K * 2).astype(np.float32)
    v2 = np.asarray(evs, np.float32).reshape(T, K * 2)
    pb = dict(y=y2, var=v2, D=2, unit=True, m0f=np.asarray(m0s).reshape(-1), S0d=dg(S0s), a=dg(As), c=dg(Cs),
              qs=dg(Qs) * np.repeat(s, 2))
    assert (pb['a'] == 1).all() and (pb['c'] == 1).all()
    refs, bars = scalar_refs(pb, 4.0, 2, (8,))
    bars = bars[8]
    r64 = refs[8][0]
    got = ((out['ms'] - mu.astype(np.float32)[None]).reshape(T, -1), out['Vs'].reshape(T, -1), out['weights'],
           r64[3].astype(np.float32))                                        # (the driver returns no change)
    err = gref.errors(got, r64, y2)
    # ms was shifted by the centring mean in float32: one ulp of the pixel coordinate on top of the bar
    ulp = float(np.spacing(np.float32(np.abs(out['ms']).max()))) / float(np.abs(y2).max(axis=0).min())
    assert float(err['ms'].max()) <= bars['ms'] + ulp and float(err['Vs'].max()) <= bars['Vs']
    assert float(err['weights'].max()) <= bars['weights']
    hit = np.zeros(T, bool)
    hit[frames] = True
    counts = {}
    for name, lam in (('reference', r64[2]), ('device', out['weights'])):
        counts[name] = (int((lam[hit, 1] <= 0.3).sum()), int((lam[~hit, 1] <= 0.3).sum()),
                        int((np.delete(lam, 1, axis=1) <= 0.3).sum()))
    print(f'golden ibl-pupil markers, 40 frames of keypoint 1 displaced by 30 px in x and y: (marked of the 40, marked '
          f'elsewhere on the keypoint, marked on the other keypoints) {counts}')
    for a, b in zip(counts['reference'], counts['device']):
        assert abs(a - b) <= 1


def test_smooth_multicam_robust_on_the_golden_markers_with_a_displaced_view(golden_dir):
    """One view of one keypoint moved by 30 px on 40 isolated frames in every ensemble member, s the one recorded with
    the markers: the driver agrees with the float64 reference on the model it builds, and the counts of marked frames
    of that view and of falsely marked views are the reference's, one either way."""
    from eks_amd import smooth_multicam_robust
    from eks_amd.marker_array import MarkerArray
    from eks_amd.robust import multicam_problem
    g = np.load(os.path.join(golden_dir, 'mirror_mouse_multicam.npz'))
    mk = g['markers'].astype(np.float64)
    names, cams = [str(k) for k in g['keypoints']], [str(c) for c in g['cameras']]
    s = g['adam_s'].astype(np.float64)
    M_, V, T, K, _ = mk.shape
    frames = 5 + 3 * np.random.default_rng(0).choice((T - 10) // 3, size=40, replace=False)
    mk[:, 1, frames, 2, 0:2] += 30.0                                         # view 1 of keypoint 2
    ma = MarkerArray(mk, data_fields=['x', 'y', 'likelihood'])
    kw = dict(avg_mode='median', var_mode='confidence_weighted_var')
    out = smooth_multicam_robust(ma, names, cams, s, nu=4.0, n_iters=8, **kw)
    assert out['ms'].shape == (T, K, 3) and out['Vs'].shape == (T, K, 3) and out['weights'].shape == (T, K, V)
    assert out['reprojected'].shape == (T, K, 2 * V)
    model, mu = multicam_problem(ma, names, cams, 50.0, kw['avg_mode'], kw['var_mode'], None, 3)
    ys, m0s, S0s, As, Cs, Qs, evs = model
    y = np.swapaxes(ys, 0, 1).astype(np.float32)
    var = np.asarray(evs, np.float32)
    Mref = dict(m0=m0s, S0=S0s, A=As, C=Cs, Q=Qs, s=s)
    seq, joint = dense_refs(Mref, y, var, 4.0, 2, (8,))
    check_dense('smooth_multicam_robust', (out['ms'], out['Vs'], out['weights'], seq[8][3].astype(np.float32)),
                seq[8], joint[8])                                            # (the driver returns no change)
    rep = np.einsum('kod,tkd->tko', Cs, seq[8][0]) + mu[None]
    assert np.abs(out['reprojected'] - rep).max() <= 1e-5 * np.abs(rep).max()
    # (the layout of `reprojected` and of the centring means is anchored on the reference's own output in
    #  test_multicam_model_and_a_single_pass_against_the_golden_driver_output)
    hit = np.zeros(T, bool)
    hit[frames] = True
    counts = {}
    for name, lam in (('reference', seq[8][2]), ('device', out['weights'])):
        mask = np.zeros(lam.shape, bool)
        mask[hit, 2, 1] = True
        counts[name] = (int((lam[mask] <= 0.3).sum()), int((lam[hit, 2, 0] <= 0.3).sum()), int((lam[~mask] <= 0.3).sum()))
    print(f'golden mirror-mouse markers, view 1 of keypoint 2 displaced by 30 px on 40 frames: (marked of the 40, the other '
          f'view marked on those frames, views marked anywhere else) {counts}')
    for a, b in zip(counts['reference'], counts['device']):
        assert abs(a - b) <= 1


def test_multicam_model_and_a_single_pass_against_the_golden_driver_output(golden_dir):
    """smooth_multicam_robust rebuilds the model ensemble_kalman_smoother_multicam's host branch builds.  Anchored on
    vectors recorded from the reference driver (smooth_param = 10, quantile_keep_pca = 95), not on the code under
    test: C, Q, S0 equal the recorded ones up to the PCA sign, and with n_iters = 1 - the Gaussian smoother - the
    pixel-coordinate `reprojected` (T, K, 2V), view by view, and the latent variances are the recorded driver output at
    tests/test_gpu_drivers.py's tolerance (1e-5 of each column's scale).  A centring mean laid out (V, K, 2) in the
    place of (K, 2V) would be off by the distance between the views' keypoints."""
    from eks_amd import smooth_multicam_robust
    from eks_amd.marker_array import MarkerArray
    from eks_amd.robust import multicam_problem
    g = np.load(os.path.join(golden_dir, 'mirror_mouse_multicam.npz'))
    ma = MarkerArray(g['markers'].astype(np.float64), data_fields=['x', 'y', 'likelihood'])
    names, cams = [str(k) for k in g['keypoints']], [str(c) for c in g['cameras']]
    kw = dict(avg_mode='median', var_mode='confidence_weighted_var')
    model, mu = multicam_problem(ma, names, cams, 95.0, kw['avg_mode'], kw['var_mode'], None, 3)
    worst = {}
    for name, got, want in (('C', model[4], g['Cs']), ('Q', model[5], g['Qs']), ('S0', model[2], g['S0s'])):
        want = want.astype(np.float64)
        worst[name] = float((np.abs(np.abs(got) - np.abs(want)) / np.abs(want).max()).max())
    out = smooth_multicam_robust(ma, names, cams, 10.0, quantile_keep_pca=95.0, n_iters=1, **kw)
    assert (out['weights'] == 1).all()
    keep = g['keep_idx']
    for c in range(2):
        ref = g[f's10_cam{c}_rows'].astype(np.float64).reshape(len(keep), 4, 9)[:, :, 0:2]
        got = out['reprojected'][keep][:, :, 2 * c:2 * c + 2].astype(np.float64)
        worst[f'view {c}'] = float((np.abs(got - ref) / np.abs(ref).max(axis=0)).max())
    ref = g['s10_latent_rows'].astype(np.float64).reshape(len(keep), 4, 6)
    worst['latent'] = float((np.abs(np.abs(out['ms'][keep]) - np.abs(ref[..., :3])) / np.abs(ref[..., :3]).max()).max())
    worst['latent var'] = float((np.abs(out['Vs'][keep] - ref[..., 3:]) / ref[..., 3:].max()).max())
    print('smooth_multicam_robust against the recorded driver output: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) < 1e-5
