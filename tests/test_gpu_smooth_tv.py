"""GPU: eks_smooth_tv (eks_amd/csrc/eks_smooth_tv.hip on scalar chains, dense_smooth_tv in eks_dense.hip on general
models) and eks_amd.irregular against the float64 references of tests/smooth_tv_ref.py, through the C ABI.

Bars.  Scalar chains (float32 lanes), the project's rule (smooth_tv_ref.f32_bars): error / scale <= max(1e-5, 4 x the
float32 NumPy transcription's own worst error / scale on the same inputs); scale of ms: the chain's max |y|; of Vs: its
own value.  General models (float64 in the lane): 100 x the disagreement of the two independent float64 reference
forms (sequential updates and a solve; the gain through S_t in Joseph form and an explicit inverse) on the same inputs,
floored at 1e-12 and capped at 1e-8 (smooth_tv_ref.f64_bar), relative to the keypoint's largest |ms| / |Vs| entry,
plus one float32 ulp of the reference value, because the outputs are rounded once.  Nothing is compared with the
kernels' own output, except where the test is about bits (determinism, subsets, entry 0) or about the existing
eks_smooth (w = 1, the gap identity: within twice the bar, both sides being float32 results).

Measured on the MI355X: DESIGN.md 9g has the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import smooth_tv_ref as tref  # noqa: E402
from test_increments_cpu import dense_case, make_session  # noqa: E402
from test_gpu_increments import PARAMS, _dev, dense_session, diag_flags, edge_session, stable  # noqa: E402
from test_gpu_em import subset  # noqa: E402
from test_smooth_tv_cpu import random_w  # noqa: E402
from dense_forms import general_grid, general_seed  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B = 32                                        # kChainChunk: frames per lane of the scalar-chain kernels
T_EDGES = (1, 2, 3, B - 1, B, B + 1, 64 * B - 1, 64 * B + 1, 2 * 64 * B + 5)   # .., the 64-chunk edge, three blocks of 64


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def raw_call(dims_args, ins, qscale, per_keypoint, ms, Vs, ws_bytes=None):
    """eks_smooth_tv itself: ins = y, var; then m0 .. s.  Returns the status."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*dims_args)
    need = int(lib.eks_smooth_tv_workspace_bytes(ctypes.byref(dims)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device='cuda')
    p = hip_ops._ptr
    rc = lib.eks_smooth_tv(ctypes.byref(dims), p(ins[0]), p(ins[1]), p(qscale), int(per_keypoint), *[p(t) for t in ins[2:]],
                           p(ms), p(Vs), p(ws), ws.numel() if ws_bytes is None else ws_bytes, hip_ops._stream())
    torch.cuda.synchronize()
    return rc


def gpu_scalar(pb, w, vs_diag=True):
    """eks_smooth_tv on the chains of make_session -> ms (T, N), Vs (T, N) or (T, K, D, D) float32."""
    from eks_amd import _lib
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    w = np.ascontiguousarray(w, np.float32)
    rc = raw_call((K, T, D, D, diag_flags(pb) | (_lib.FLAG_VS_DIAG if vs_diag else 0)), ins, _dev(w), w.ndim == 2, ms, Vs)
    assert rc == 0
    ms, Vs = ms.cpu().numpy().reshape(T, K * D), Vs.cpu().numpy()
    return ms, (Vs.reshape(T, K * D) if vs_diag else Vs)


def scalar_refs(pb, w):
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'], w)
    r64 = tref.scalar_smooth_tv(*args, D=pb['D'])
    r32 = tref.scalar_smooth_tv_f32(*args, D=pb['D'], unit=pb['unit'])
    return r64, r32, tref.f32_bars(*r32, *r64, pb['y'])


def check_scalar(label, pb, w, got, worst=None, slack=1.0):
    ms, Vs = got
    assert np.isfinite(ms).all() and np.isfinite(Vs).all() and (Vs > 0).all(), f'{label}: non-finite or non-positive'
    r64, r32, bars = scalar_refs(pb, w)
    err, et = tref.f32_errors(ms, Vs, *r64, pb['y']), tref.f32_errors(*r32, *r64, pb['y'])
    for k in err:
        e, t = float(err[k].max()), float(et[k].max())
        if worst is not None:
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e, t))
        assert e <= slack * bars[k], f'{label}: {k} {e:.3g} over {slack} x bar {bars[k]:.3g} (transcription {t:.3g})'
    return bars


def general_session(T, K, D, sval, seed):
    """a = 0.98, c = 1.3, a q of its own per chain, and a NEGATIVE c in chain 0 (its data mirrored with it)."""
    pb = edge_session(T, K, D, sval, 'decay', seed)
    pb['c'] = pb['c'].copy()
    pb['c'][0] = -1.3
    pb['par']['C'][0, 0, 0] = -1.3
    pb['y'][:, 0] = -pb['y'][:, 0]
    return pb


def session(T, K, D, sval, kind, seed):
    return edge_session(T, K, D, sval, 'unit', seed) if kind == 'unit' else general_session(T, K, D, sval, seed)


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 1), (3, 2), (21, 3), (65, 1), (65, 2)])
def test_scalar_chain_edge_shapes(K, D, kind):
    worst = {}
    for i, T in enumerate(T_EDGES):
        for sval in (1e-2, 2.0, 300.0):
            pb = session(T, K, D, sval, kind, seed=T + K)
            rng = np.random.default_rng(T + K + D)
            w = random_w(rng, (T, K) if (i + D) % 2 else (T,))
            label = f'N={K * D} D={D} T={T} s={sval} {kind} w{w.shape}'
            ms, Vs = gpu_scalar(pb, w)
            check_scalar(label, pb, w, (ms, Vs), worst)
            if sval == 2.0:                                       # full rows: PointerStore's contract
                msf, Vsf = gpu_scalar(pb, w, vs_diag=False)
                assert np.array_equal(msf, ms), label
                assert np.array_equal(np.diagonal(Vsf, axis1=2, axis2=3).reshape(T, K * D), Vs), label
                assert not Vsf[:, :, ~np.eye(D, dtype=bool)].any(), f'{label}: off-diagonal entries are not zero'
    print(f'N={K * D} D={D} {kind}, worst kernels (transcription on that case): '
          + ', '.join(f'{k} {e:.3g} ({t:.3g})' for k, (e, t) in worst.items()))


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_a_spike_lands_on_its_own_frame(kind):
    """A single w = 400 at frame p around the edges of the first, a middle and the last chunk and at both ends: the
    output matches the reference with the same p and misses the references with p - 1 and p + 1 by more than ten bars."""
    T, K, D = 5 * B + 7, 3, 1
    pb = session(T, K, D, 2.0, kind, seed=31)
    spots = [1, T - 1] + [j * B + o for j in (1, 3, 5) for o in (-1, 0, 1)]
    vs = {}
    for p in sorted(set(spots + [q for p in spots for q in (p - 1, p + 1) if 1 <= q < T])):
        w = np.ones(T, np.float32)
        w[p] = 400.0
        vs[p] = (w, scalar_refs(pb, w))
    closest = np.inf
    for p in spots:
        w, (r64, _, bars) = vs[p]
        ms, Vs = gpu_scalar(pb, w)
        check_scalar(f'{kind} spike at {p}', pb, w, (ms, Vs))
        for q in (p - 1, p + 1):
            if 1 <= q < T:
                miss = float(tref.f32_errors(ms, Vs, *vs[q][1][0], pb['y'])['Vs'].max()) / bars['Vs']
                closest = min(closest, miss)
                assert miss > 10.0, f'{kind}: a spike at {p} is within {miss:.3g} bars of the reference at {q}'
    print(f'{kind}: the nearest wrong-frame reference is {closest:.3g} bars away')


@pytest.mark.parametrize('kind', ['unit', 'general'])
@pytest.mark.parametrize('D', [2, 3])
def test_per_keypoint_scale_reads_column_n_over_D(D, kind):
    """w (T, K), every keypoint with a spike frame of its own: matches the reference; the reference with the columns
    read by n instead of n / D (chain n -> column n % K) is more than ten bars away."""
    T, K = 3 * B + 5, 5
    pb = session(T, K, D, 2.0, kind, seed=40 + D)
    w = np.ones((T, K), np.float32)
    for k in range(K):
        w[B - 2 + 7 * k, k] = 400.0
    got = gpu_scalar(pb, w)
    bars = check_scalar(f'{kind} D={D} per-keypoint spikes', pb, w, got)
    wrong = np.stack([w[:, n % K] for n in range(K * D)], axis=1)              # (T, N): what `n` would read
    args = (pb['y'], pb['var'], pb['m0f'], pb['S0d'], pb['a'], pb['c'], pb['qs'])
    wms, wVs = tref.scalar_smooth_tv(*args, wrong, D=1)
    assert float(tref.f32_errors(*got, wms, wVs, pb['y'])['Vs'].max()) > 10.0 * bars['Vs']


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_unit_scale_agrees_with_eks_smooth(kind, set_knob):
    """w = 1 against eks_smooth with the windowed replay off: within twice the bar (the fused form associates the
    scan differently, so bits are not required)."""
    from eks_amd import hip_ops
    set_knob('EKS_SMOOTH_WINDOW', '0')
    for T, K, D in ((2 * 64 * B + 5, 65, 2), (B + 1, 3, 1), (700, 21, 3)):
        pb = session(T, K, D, 2.0, kind, seed=T)
        w = np.ones(T, np.float32)
        ms, Vs = gpu_scalar(pb, w)
        bars = check_scalar(f'{kind} w = 1 T={T}', pb, w, (ms, Vs))
        sm, sV = hip_ops.smooth(_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)),
                                *(_dev(pb['par'][k]) for k in PARAMS), flags=diag_flags(pb), vs_diag=True)
        torch.cuda.synchronize()
        sm, sV = sm.cpu().numpy().reshape(T, -1).astype(np.float64), sV.cpu().numpy().reshape(T, -1).astype(np.float64)
        e_m = float((np.abs(ms - sm).max(axis=0) / np.abs(pb['y']).max(axis=0)).max())
        e_V = float((np.abs(Vs - sV) / sV).max())
        print(f'{kind} T={T} N={K * D}: w = 1 against eks_smooth ms {e_m:.3g} (bar {bars["ms"]:.3g}), Vs {e_V:.3g} ({bars["Vs"]:.3g})')
        assert e_m <= 2 * bars['ms'] and e_V <= 2 * bars['Vs']


def test_gap_identity_on_the_device(set_knob):
    """UNIT chains: eks_smooth_tv on the compact session with w = n at the gaps against the existing eks_smooth on the
    session padded with n - 1 frames of variance 1e30, on the shared frames, within twice the bar."""
    from eks_amd import hip_ops
    set_knob('EKS_SMOOTH_WINDOW', '0')
    T, K, D = 900, 4, 2
    pb = session(T, K, D, 2.0, 'unit', seed=77)
    rng = np.random.default_rng(5)
    w = np.ones(T, np.float32)
    w[rng.choice(np.arange(1, T), size=60, replace=False)] = rng.integers(2, 7, size=60)
    w[[B, 2 * B - 1, T - 1]] = (3, 4, 5)
    ms, Vs = gpu_scalar(pb, w)
    bars = check_scalar('gap identity, compact', pb, w, (ms, Vs))
    yp, vp, idx = tref.pad_gaps(pb['y'], pb['var'], w)
    Tp = yp.shape[0]
    pm, pV = hip_ops.smooth(_dev(yp.reshape(Tp, K, D)), _dev(vp.reshape(Tp, K, D)), *(_dev(pb['par'][k]) for k in PARAMS),
                            flags=diag_flags(pb), vs_diag=True)
    torch.cuda.synchronize()
    pm, pV = pm.cpu().numpy().reshape(Tp, -1)[idx].astype(np.float64), pV.cpu().numpy().reshape(Tp, -1)[idx].astype(np.float64)
    e_m = float((np.abs(ms - pm).max(axis=0) / np.abs(pb['y']).max(axis=0)).max())
    e_V = float((np.abs(Vs - pV) / pV).max())
    print(f'gap identity, {T} -> {Tp} frames: ms {e_m:.3g} (bar {bars["ms"]:.3g}), Vs {e_V:.3g} ({bars["Vs"]:.3g})')
    assert e_m <= 2 * bars['ms'] and e_V <= 2 * bars['Vs']


@pytest.mark.parametrize('kind', ['unit', 'general'])
def test_two_calls_a_subset_of_the_keypoints_and_entry_zero(kind):
    """Two calls give the same bits; keypoints [3, 67) of K = 70 alone (another lane mapping) give the full call's
    bits, with a shared and with a per-keypoint w; a NaN in entry 0 of qscale changes nothing."""
    T, K, D = 35 * B + 1, 70, 2
    pb = session(T, K, D, 2.0, kind, seed=21)
    rng = np.random.default_rng(3)
    k0, k1 = 3, 67
    for shape in ((T,), (T, K)):
        w = random_w(rng, shape)
        w[0] = 1.0
        full, again = gpu_scalar(pb, w), gpu_scalar(pb, w)
        assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])
        sub = gpu_scalar(subset(pb, k0, k1), w if w.ndim == 1 else w[:, k0:k1])
        assert np.array_equal(sub[0], full[0][:, D * k0:D * k1]) and np.array_equal(sub[1], full[1][:, D * k0:D * k1])
        w[0] = np.nan
        nan0 = gpu_scalar(pb, w)
        assert np.array_equal(nan0[0], full[0]) and np.array_equal(nan0[1], full[1])


# ---- general models ------------------------------------------------------------------------------------------------------
def gpu_dense(M, y, var, w, vs_diag=False):
    from eks_amd import _lib
    T, K, O = y.shape
    D = M['m0'].shape[1]
    ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
    ms = torch.full((T, K, D), np.nan, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D) if vs_diag else (T, K, D, D), np.nan, dtype=torch.float32, device='cuda')
    w = np.ascontiguousarray(w, np.float32)
    assert raw_call((K, T, D, O, _lib.FLAG_VS_DIAG if vs_diag else 0), ins, _dev(w), w.ndim == 2, ms, Vs) == 0
    return ms.cpu().numpy(), Vs.cpu().numpy()


def dense_excess(got, seq, joint):
    """worst |got - seq| / (bar x the keypoint's largest entry + one float32 ulp), and the bar."""
    K = seq.shape[1]
    scale = np.abs(seq).transpose(1, 0, *range(2, seq.ndim)).reshape(K, -1).max(axis=1)
    scale = scale.reshape((1, K) + (1,) * (seq.ndim - 2)) * np.ones_like(seq)
    bar = tref.f64_bar(seq, joint, scale)
    ulp = np.spacing(np.abs(seq).astype(np.float32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - seq) / (bar * scale + ulp)).max()), bar


def check_dense(label, M, y, var, w, got, worst=None):
    par = tuple(M[k] for k in PARAMS)
    seq, joint = tref.dense_smooth_tv(y, var, *par, w), tref.dense_smooth_tv_joint(y, var, *par, w)
    figs = []
    for name, g, a, b in (('ms', got[0], seq[0], joint[0]), ('Vs', got[1], seq[1], joint[1])):
        assert np.isfinite(g).all(), f'{label}: {name} is not finite'
        if name == 'Vs' and g.ndim == 3:                                      # VS_DIAG
            a, b = (np.diagonal(x, axis1=2, axis2=3) for x in (a, b))
        excess, bar = dense_excess(g, a, b)
        figs.append(f'{name} {excess:.2g} x (bar {bar:.2g})')
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), excess)
        assert excess <= 1.0, f'{label}: {name} is {excess:.3g} x its bar {bar:.3g} (+ one float32 ulp)'
    return ', '.join(figs)


# (and the accepted width, odd O past 32 and the smallest odd O, at K = 3: tests/dense_forms.py WIDE_PAIRS)
@pytest.mark.parametrize('D,O,K', general_grid([(1, 1), (2, 3), (3, 4), (6, 12)]))
def test_general_models_against_the_two_float64_forms(D, O, K, set_knob):
    M = stable(dense_case(K, D, O, False, seed=general_seed(D, O, K)))
    worst = {}
    for i, T in enumerate((1, 2, 16, 17, 33, 100)):
        y, var = dense_session(M, T, O, seed=T)
        w = random_w(np.random.default_rng(T + K), (T, K) if i % 2 else (T,))
        for chunk in ('16', '32'):
            set_knob('EKS_DENSE_CHUNK', chunk)
            got = gpu_dense(M, y, var, w, vs_diag=(i % 3 == 0))
            check_dense(f'D={D} O={O} K={K} T={T} chunk={chunk} w{w.shape}', M, y, var, w, got, worst)
    print(f'general D={D} O={O} K={K}: worst fraction of the bar ' + ', '.join(f'{k} {v:.2g}' for k, v in worst.items()))


@pytest.mark.parametrize('chunk,T', [('16', 1100), ('32', 2100)])
def test_general_model_spanning_more_than_one_scan_block(chunk, T, set_knob):
    """ceil(T / chunk) > 64 chunks: two blocks of dense_scan_kernel, boundaries through dense_scan_blocks_kernel."""
    set_knob('EKS_DENSE_CHUNK', chunk)
    assert -(-T // int(chunk)) > 64
    M = stable(dense_case(3, 3, 4, False, seed=5))
    y, var = dense_session(M, T, 4, seed=2)
    w = random_w(np.random.default_rng(T), (T, 3))
    print(f'T={T} chunk={chunk}: ' + check_dense(f'T={T} chunk={chunk}', M, y, var, w, gpu_dense(M, y, var, w)))


@pytest.mark.parametrize('variant', ['unit_root', 'singular_q'])
@pytest.mark.parametrize('D,O', [(2, 3), (3, 4), (6, 12)])
def test_general_model_variants(D, O, variant):
    """A = I, and a rank D-1 Q, both with exact zeros in w: only Pp is factored, never Q."""
    M = stable(dense_case(3, D, O, variant == 'singular_q', seed=8), unit_root=variant == 'unit_root')
    if variant == 'singular_q':
        assert np.linalg.matrix_rank(M['Q'][0]) == D - 1
    y, var = dense_session(M, 100, O, seed=3)
    for shape in ((100,), (100, 3)):
        w = random_w(np.random.default_rng(D), shape)
        assert (w[1:] == 0).any()
        print(f'{variant} D={D} O={O} w{shape}: ' + check_dense(f'{variant} D={D} O={O}', M, y, var, w, gpu_dense(M, y, var, w)))


@pytest.mark.parametrize('D,O', [(2, 3), (6, 12)])
def test_general_model_unit_scale_agrees_with_the_generic_eks_smooth(D, O, set_knob):
    """w = 1 against eks_smooth held to its generic kernels (EKS_DENSE_LEGACY): within the bar."""
    from eks_amd import hip_ops
    set_knob('EKS_DENSE_LEGACY', '1')
    M = stable(dense_case(3, D, O, False, seed=12))
    T = 300
    y, var = dense_session(M, T, O, seed=4)
    w = np.ones(T, np.float32)
    got = gpu_dense(M, y, var, w)
    check_dense(f'w = 1 D={D}', M, y, var, w, got)
    sm, sV = hip_ops.smooth(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), flags=0, vs_diag=False)
    torch.cuda.synchronize()
    par = tuple(M[k] for k in PARAMS)
    seq, joint = tref.dense_smooth_tv(y, var, *par, w), tref.dense_smooth_tv_joint(y, var, *par, w)
    for g, s_, a, b in ((got[0], sm, seq[0], joint[0]), (got[1], sV, seq[1], joint[1])):
        s64 = s_.cpu().numpy().astype(np.float64)
        K = a.shape[1]
        scale = np.abs(a).transpose(1, 0, *range(2, a.ndim)).reshape(K, -1).max(axis=1).reshape((1, K) + (1,) * (a.ndim - 2))
        bar = tref.f64_bar(a, b, scale * np.ones_like(a))
        ulp = np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
        assert (np.abs(g.astype(np.float64) - s64) <= bar * scale + ulp).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from eks_amd import _lib
    pb = edge_session(100, 3, 2, 2.0, 'unit', seed=2)
    T, K, D = pb['T'], pb['K'], pb['D']
    ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
    w = _dev(np.ones(T, np.float32))
    ms = torch.full((T, K, D), 7.0, dtype=torch.float32, device='cuda')
    Vs = torch.full((T, K, D, D), 7.0, dtype=torch.float32, device='cuda')
    diag = diag_flags(pb)
    cases = [
        ((K, T, D, D, diag), ins, None, -1),                                                    # NULL qscale
        ((K, T, D, D, 0), ins, None, -1),                                                      # .. on the general path
        ((K, T, D, D, diag), ins[:3] + [None] + ins[4:], w, -1),                               # NULL S0
        ((0, T, D, D, diag), ins, w, -2), ((K, 0, D, D, diag), ins, w, -2), ((K, T, D, D + 1, diag), ins, w, -2),
        ((K, T, D, D, _lib.FLAG_UNIT_AC), ins, w, -3),                                         # UNIT_AC without DIAG_MODEL
        ((K, T, 7, 7, 0), ins, w, -3), ((K, T, D, 65, 0), ins, w, -3), ((K, T, 9, 9, diag), ins, w, -3),
    ]
    for dims, tensors, q, want in cases:
        assert raw_call(dims, tensors, q, 0, ms, Vs) == want, dims
        assert bool((ms == 7.0).all()) and bool((Vs == 7.0).all()), dims
    for dims in ((K, T, D, D, diag), (K, T, D, D, 0)):
        assert raw_call(dims, ins, w, 0, ms, Vs, ws_bytes=255) == -4                           # workspace too small
        assert raw_call(dims, ins, w, 0, None, Vs) == -1 and raw_call(dims, ins, w, 0, ms, None) == -1
        assert bool((ms == 7.0).all()) and bool((Vs == 7.0).all()), dims
    assert raw_call((K, T, D, D, diag), ins, w, 0, ms, Vs) == 0
    assert not bool((ms == 7.0).any()) and not bool((Vs == 7.0).any())


# ---- the Python surface --------------------------------------------------------------------------------------------------
def test_process_noise_scale_from_times_on_a_60_hz_clock():
    from eks_amd import process_noise_scale_from_times
    t = np.arange(600) / 60.0
    keep = np.ones(600, bool)
    keep[[50, 200, 410]] = False                                   # three dropped frames
    keep[300:304] = False                                          # and one 5-frame gap
    w = process_noise_scale_from_times(t[keep])
    assert w.dtype == np.float32 and w.shape == (593,) and w[0] == 1.0
    gaps = np.flatnonzero(w > 1.5)
    assert np.allclose(w[gaps], [2, 2, 5, 2]) and np.allclose(np.delete(w, gaps), 1.0)
    assert np.allclose(process_noise_scale_from_times(t[keep], nominal_dt=1 / 60.0), w)


def test_smooth_time_varying_matches_the_reference_on_both_paths():
    from eks_amd import smooth_time_varying
    pb = edge_session(200, 3, 2, 2.0, 'unit', seed=9)
    T, K, D = pb['T'], pb['K'], pb['D']
    w = random_w(np.random.default_rng(1), (T, K))
    par = pb['par']
    ms, Vs = smooth_time_varying(np.swapaxes(pb['y'].reshape(T, K, D), 0, 1), par['m0'], par['S0'], par['A'], par['C'],
                                 par['Q'], pb['var'].reshape(T, K, D), par['s'], w.T, vs_diag=True)
    assert ms.shape == (K, T, D) and Vs.shape == (K, T, D) and ms.dtype == np.float32
    check_scalar('smooth_time_varying', pb, w, (np.swapaxes(ms, 0, 1).reshape(T, -1), np.swapaxes(Vs, 0, 1).reshape(T, -1)))
    M = stable(dense_case(3, 3, 4, False, seed=2))
    y, var = dense_session(M, 120, 4, seed=5)
    w1 = random_w(np.random.default_rng(2), (120,))
    ms, Vs = smooth_time_varying(np.swapaxes(y, 0, 1), M['m0'], M['S0'], M['A'], M['C'], M['Q'], var, M['s'], w1)
    assert ms.shape == (3, 120, 3) and Vs.shape == (3, 120, 3, 3)
    check_dense('smooth_time_varying, general', M, y, var, w1, (np.swapaxes(ms, 0, 1), np.swapaxes(Vs, 0, 1)))


def test_smooth_singlecam_irregular_on_the_golden_markers_with_frames_deleted(golden_dir):
    """3 % of the frames deleted: on the kept frames the irregular smoother is closer to the full session's driver
    result than the uniform smoother run on the same deleted session, and its posterior variance is larger across
    every gap."""
    from eks_amd import smooth_singlecam_irregular
    from eks_amd.marker_array import MarkerArray
    from eks_amd.singlecam_smoother import ensemble_kalman_smoother_singlecam
    g = np.load(os.path.join(golden_dir, 'ibl_pupil_singlecam.npz'))
    mk = g['markers'].astype(np.float64)
    names = [str(k) for k in g['keypoints']]
    M_, V, T, K, _ = mk.shape
    fields = ['x', 'y', 'likelihood']
    df, s = ensemble_kalman_smoother_singlecam(MarkerArray(mk, data_fields=fields), names, smooth_param=10.0)
    full = df.to_numpy().reshape(T, K, 9)[:, :, 0:2]
    rng = np.random.default_rng(0)
    drop = rng.choice(np.arange(1, T - 1), size=int(round(0.03 * T)), replace=False)
    keep = np.ones(T, bool)
    keep[drop] = False
    times = np.flatnonzero(keep).astype(np.float64)
    ma = MarkerArray(np.ascontiguousarray(mk[:, :, keep]), data_fields=fields)
    irr = smooth_singlecam_irregular(ma, names, s, frame_times=times)
    uni = smooth_singlecam_irregular(ma, names, s, process_noise_scale=np.ones(times.size))
    assert irr['ms'].shape == (times.size, K, 2) and irr['Vs'].shape == (times.size, K, 2) and irr['ms'].dtype == np.float32
    udf, _ = ensemble_kalman_smoother_singlecam(ma, names, smooth_param=10.0)
    udrv = udf.to_numpy().reshape(times.size, K, 9)
    # (w = 1 through the new call is the driver's own smoother on the deleted session, up to float32 rounding)
    assert np.abs(uni['ms'] - udrv[:, :, 0:2]).max() < 1e-3 * np.abs(full).max()
    e_irr = float(np.sqrt(np.mean((irr['ms'] - full[keep]) ** 2)))
    e_uni = float(np.sqrt(np.mean((uni['ms'] - full[keep]) ** 2)))
    after = np.flatnonzero(np.diff(times) > 1.5) + 1                     # kept frames that follow a gap
    ratio = irr['Vs'][after] / uni['Vs'][after]
    ratio_before = irr['Vs'][after - 1] / uni['Vs'][after - 1]
    print(f'golden markers, {T - times.size} of {T} frames deleted, {after.size} gaps: rms distance to the full session '
          f'{e_irr:.4g} px (irregular) against {e_uni:.4g} px (uniform); Vs ratio across gaps min {ratio.min():.4g} '
          f'median {np.median(ratio):.4g}, on the frame before min {ratio_before.min():.4g}')
    assert e_irr < e_uni
    assert (ratio > 1.0).all() and (ratio_before > 1.0).all()
