"""Windowed replay of the scalar-chain smoother (eks_diag.hip: replay_window_block, the probe and the gated exact
launches behind it) at small shapes: EKS_SMOOTH_WINDOW_MIN_T=1024 lets sequences of a few thousand frames take the
form that long sessions take by default.  EKS_SMOOTH_WINDOW: 0 the scan-based path alone, 1 windowed + fallback,
2 test mode (no probe, no fallback, lanes that fail the check store NaN)."""
import ctypes

import numpy as np
import pytest

import window_ref as wr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

B, G = 32, 8                      # frames per chunk, chunks per window group (eks_diag.hip: kChunk, kWinG)
GROUP = B * G
_ORACLE = {}


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _problem(T, K, seed, a=1.0, c=1.0, s=None):
    rng = np.random.default_rng(seed)
    if a == 1.0:
        x = 50.0 + np.cumsum(0.5 * rng.standard_normal((T, K, 2)), axis=0)
        m0 = np.full((K, 2), 50.0)
    else:
        x = 3.0 * rng.standard_normal((T, K, 2))
        m0 = np.zeros((K, 2))
    var = (0.3 * rng.gamma(2.0, 1.0, (T, K, 2)) + 0.02).astype(np.float32)
    y = (c * x + np.sqrt(var) * rng.standard_normal((T, K, 2))).astype(np.float32)
    eye = np.tile(np.eye(2), (K, 1, 1))
    if s is None:
        s = np.exp(rng.uniform(0.0, 4.0, K))
    return dict(y=y, var=var, m0=m0, S0=eye * 25.0, A=eye * a, C=eye * c, Q=eye.copy(), s=np.asarray(s, np.float64))


def _oracle(tag, p):
    """c_oracle.smooth of a problem, computed once per tag and shared (never modified)."""
    if tag not in _ORACLE:
        from oracle import c_oracle
        ms, Vs, _ = c_oracle.smooth(np.transpose(p['y'], (1, 0, 2)).astype(np.float64),
                                    np.clip(np.transpose(p['var'], (1, 0, 2)).astype(np.float64), 1e-12, 1e30),
                                    p['m0'], p['S0'], p['A'], p['C'], p['Q'], p['s'])
        _ORACLE[tag] = (ms, np.diagonal(Vs, axis1=2, axis2=3))
    return _ORACLE[tag]


def _run(set_knob, p, mode, vs_diag=True, min_t='1024', probe=None, sel=slice(None)):
    from eks_amd import hip_ops
    set_knob('EKS_SMOOTH_WINDOW', None if mode is None else str(mode))
    set_knob('EKS_SMOOTH_WINDOW_MIN_T', min_t)
    set_knob('EKS_SMOOTH_WINDOW_PROBE', probe)
    flags = hip_ops.model_flags(p['S0'], p['A'], p['C'], p['Q'])
    f64 = [_dev(p[k][sel], torch.float64) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')]
    y = _dev(p['y'][:, sel])
    T, K, D = y.shape
    out = (torch.full((T, K, D), float('nan'), device='cuda'),             # a lane nobody stores stays NaN
           torch.full((T, K, D) if vs_diag else (T, K, D, D), float('nan'), device='cuda'))
    ms, Vs = hip_ops.smooth(y, _dev(p['var'][:, sel]), *f64, flags=flags, vs_diag=vs_diag, out=out)
    torch.cuda.synchronize()
    return ms, Vs


def _diag(Vs, vs_diag):
    return Vs if vs_diag else torch.diagonal(Vs, dim1=2, dim2=3)


def _assert_oracle(tag, p, ms, Vs, vs_diag, stored=None, oracle=None):
    """Every frame (of the lanes in `stored` (T, K, D), where given) against the float64 oracle: means within 1e-5 of
    the keypoint's magnitude, variances within 1e-5 relative."""
    ms_o, Vd_o = (oracle or _oracle)(tag, p)
    ms_k = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vd = np.transpose(_diag(Vs, vs_diag).cpu().numpy().astype(np.float64), (1, 0, 2))
    sc = np.abs(ms_o).max(axis=(1, 2), keepdims=True)
    sel = np.ones(ms_o.shape, bool) if stored is None else np.transpose(stored, (1, 0, 2))
    assert sel.any(), tag
    em = float((np.abs(ms_k - ms_o) / sc)[sel].max())
    eV = float((np.abs(Vd - Vd_o) / Vd_o)[sel].max())
    print(f'{tag}: ms {em:.3g}, Vs {eV:.3g} of the oracle (bar 1e-5)')
    assert em < 1e-5, (tag, em)
    assert eV < 1e-5, (tag, eV)
    return em, eV


def _scopes(fn):
    """Names of the library's timing scopes that `fn` passes through."""
    from eks_amd import _lib
    lib = _lib.load()
    lib.eks_profile_drain(None, 0, None, 0)
    lib.eks_profile_enable(1)
    try:
        fn()
    finally:
        lib.eks_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 12)
    ms = (ctypes.c_float * 64)()
    n = lib.eks_profile_drain(buf, len(buf), ms, 64)
    return [b.decode() for b in buf.raw.split(b'\0')[:n]]


@pytest.mark.parametrize('vs_diag,a,c', [(True, 1.0, 1.0), (False, 1.0, 1.0), (True, 0.98, 1.3)])
def test_every_chain_passes(set_knob, vs_diag, a, c):
    T, K = 4099, 64
    p = _problem(T, K, seed=5, a=a, c=c)
    tag = ('pass', a, c)
    ms2, Vs2 = _run(set_knob, p, 2, vs_diag)
    assert not bool(torch.isnan(ms2).any()) and not bool(torch.isnan(Vs2).any())
    _assert_oracle(tag, p, ms2, Vs2, vs_diag)              # the windowed arithmetic itself, nothing replayed behind it
    ms1, Vs1 = _run(set_knob, p, 1, vs_diag)
    _assert_oracle(tag, p, ms1, Vs1, vs_diag)
    ms1b, Vs1b = _run(set_knob, p, 1, vs_diag)
    assert torch.equal(ms1, ms1b) and torch.equal(Vs1, Vs1b)
    if not vs_diag:
        assert not bool(Vs1[:, :, 0, 1].any()) and not bool(Vs1[:, :, 1, 0].any())


def test_one_occluded_chain_is_replayed_exactly_where_its_windows_fail(set_knob):
    T, K = 4099, 64
    p = _problem(T, K, seed=6)
    kp, d = 37, 1
    p['var'][1500:1701, kp, d] *= 1e4
    ms2, Vs2 = _run(set_knob, p, 2)
    nan_m, nan_V = torch.isnan(ms2), torch.isnan(Vs2)
    assert torch.equal(nan_m, nan_V)
    assert bool(nan_m.any())
    others = nan_m.clone()
    others[:, kp, d] = False
    assert not bool(others.any()), 'only the occluded chain may fail'
    col = nan_m[:, kp, d].cpu().numpy()
    for g0 in range(0, T, GROUP):
        grp = col[g0:g0 + GROUP]
        assert grp.all() or not grp.any(), ('whole window groups', g0)
        if grp.any():                                     # the group or one of its 64-frame halos meets the stretch
            assert g0 - 2 * B <= 1700 and g0 + GROUP + 2 * B > 1500, g0
    ms0, Vs0 = _run(set_knob, p, 0)
    ms1, Vs1 = _run(set_knob, p, 1)
    assert bool(torch.isfinite(ms1).all()) and bool(torch.isfinite(Vs1).all())
    _assert_oracle('occluded', p, ms1, Vs1, True)
    assert torch.equal(ms1[nan_m], ms0[nan_m]) and torch.equal(Vs1[nan_m], Vs0[nan_m])


@pytest.mark.parametrize('probe', ['1', '0'])
def test_slow_chains_take_the_exact_path_bit_for_bit(set_knob, probe):
    T, K = 4099, 64
    p = _problem(T, K, seed=7, s=np.full(K, np.exp(-8.0)))
    ms0, Vs0 = _run(set_knob, p, 0)
    ms1, Vs1 = _run(set_knob, p, 1, probe=probe)
    assert torch.equal(ms1, ms0) and torch.equal(Vs1, Vs0)


def test_keypoint_subsets_reproduce_their_slice_of_the_wide_run(set_knob):
    T, K = 4099, 96
    rng = np.random.default_rng(8)
    s = np.where(rng.random(K) < 0.3, np.exp(-8.0), np.exp(rng.uniform(0.0, 4.0, K)))   # slow and fast chains
    p = _problem(T, K, seed=8, s=s)
    for kp in (3, 20, 40, 70, 95):                                                       # occluded ones
        t0 = 300 + 37 * kp
        p['var'][t0:t0 + 250, kp] *= 1e4
    ms, Vs = _run(set_knob, p, 1, vs_diag=False)
    assert bool(torch.isfinite(ms).all()) and bool(torch.isfinite(Vs).all())
    for sel in (slice(0, 32), slice(17, 49), slice(64, 96)):
        ms_s, Vs_s = _run(set_knob, p, 1, vs_diag=False, sel=sel)
        assert torch.equal(ms_s, ms[:, sel]), ('ms', sel)
        assert torch.equal(Vs_s, Vs[:, sel]), ('Vs', sel)


@pytest.mark.parametrize('T,K', [(1025, 64), (GROUP * 4 + 5, 64), (4099, 33)])
def test_edges_of_the_window_geometry(set_knob, T, K):
    """One frame past the threshold; a last window group of one chunk of 5 frames; a second tile holding two chains."""
    p = _problem(T, K, seed=T + K)
    tag = ('edge', T, K)
    ms2, Vs2 = _run(set_knob, p, 2)
    assert not bool(torch.isnan(ms2).any()) and not bool(torch.isnan(Vs2).any())
    _assert_oracle(tag, p, ms2, Vs2, True)
    ms1, Vs1 = _run(set_knob, p, 1)
    _assert_oracle(tag, p, ms1, Vs1, True)


def test_below_the_threshold_the_scan_based_path_runs(set_knob):
    p = _problem(1023, 64, seed=9)
    ms0, Vs0 = _run(set_knob, p, 0)
    ms1, Vs1 = _run(set_knob, p, 1)
    assert torch.equal(ms1, ms0) and torch.equal(Vs1, Vs0)
    names = _scopes(lambda: _run(set_knob, p, 1))
    assert 'diag_window_probe' not in names and 'diag_replay_exact' not in names, names


def test_default_threshold_at_32768_frames(set_knob):
    """No knob: T >= 32 768 takes the windowed form (its probe and gated launches are in the timing scopes), 10 000
    frames do not."""
    T, K = 32_768 + 37, 33
    p = _problem(T, K, seed=10)
    out = {}
    names = _scopes(lambda: out.update(r=_run(set_knob, p, None, min_t=None)))
    assert names == ['diag_window_probe', 'diag_replay', 'diag_summarize', 'diag_scan', 'diag_replay_exact'], names
    _assert_oracle('default', p, *out['r'], True)
    q = _problem(10_000, 33, seed=11)
    names = _scopes(lambda: _run(set_knob, q, None, min_t=None))
    assert names == ['diag_summarize', 'diag_scan', 'diag_replay'], names


# ---- the windowed form at every model, width and edge the scan-based path is held to ----------------------------------
# Inputs and the float64 restatement of the kernel's rules come from tests/window_ref.py; tests/test_window_bound_cpu.py
# holds the restatement itself to the bound on the same inputs.

_RESTATED = {}


def _restated(tag, p):
    if tag not in _RESTATED:
        _RESTATED[tag] = wr.restate(p)
    return _RESTATED[tag]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _nan_groups(ms, Vs, vs_diag=True):
    """The (window group, chain) lanes a mode-2 run stored as NaN: whole groups, means and variances alike."""
    T, K, D = ms.shape
    nan = torch.isnan(ms)
    assert torch.equal(nan, torch.isnan(_diag(Vs, vs_diag)))
    col = nan.reshape(T, K * D).cpu().numpy()
    nwg = (T + GROUP - 1) // GROUP
    grp = np.stack([col[g * GROUP:(g + 1) * GROUP].all(axis=0) for g in range(nwg)])
    assert np.array_equal(wr.group_mask(grp, T), col), 'a window group is stored or not as a whole'
    return grp, col.reshape(T, K, D)


def _assert_same_lanes(grp, fail):
    wrong = np.argwhere(grp != fail)
    assert wrong.size == 0, ('(group, chain, NaN in mode 2, predicted to fail)',
                             [(int(g), int(n), bool(grp[g, n]), bool(fail[g, n])) for g, n in wrong[:20]])


def _info_form_oracle(tag, p):
    """oracle.eks_oracle.info_form_smoother: variances at the 1e-12 clip are beyond the covariance form's resolution."""
    if tag not in _ORACLE:
        from oracle import eks_oracle as orc
        Rd = np.clip(np.transpose(p['var'], (1, 0, 2)).astype(np.float64), 1e-12, 1e30)
        ms, Vs = orc.info_form_smoother(np.transpose(p['y'], (1, 0, 2)).astype(np.float64), p['m0'], p['S0'], p['A'],
                                        p['C'], p['Q'], p['s'], Rd)[:2]
        _ORACLE[tag] = (ms, np.diagonal(Vs, axis1=2, axis2=3))
    return _ORACLE[tag]


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_state_width_with_diagonal_and_full_covariance_rows(set_knob, D, general):
    """VS_ROW = 0 (vs_diag) and VS_ROW = D of the windowed kernel, UNIT and general - case [D-False] runs
    diag_replay_blk_kernel<32, true, 0 and D, kFormWindow>, case [D-True] <32, false, 0 and D, kFormWindow>: K * D chains
    are no multiple of 64 and, where D does not divide 64, the tile boundary falls inside a keypoint.  The full rows
    carry the vs_diag run's variances bit for bit and +0.0 elsewhere (rows of three floats and more once left as 12- and
    16-byte stores whose first element was lost on some lanes: BufferStore in eks_diag.hip)."""
    p = wr.width_problem(D, general)
    tag = ('width', D, general)
    eye = torch.eye(D, dtype=torch.bool, device='cuda')
    for mode in (2, 1):
        ms_d, Vs_d = _run(set_knob, p, mode, True)
        assert bool(torch.isfinite(ms_d).all()) and bool(torch.isfinite(Vs_d).all()), mode
        _assert_oracle(tag, p, ms_d, Vs_d, True)
        ms_f, Vs_f = _run(set_knob, p, mode, False)
        assert _same_bits(ms_f, ms_d), mode
        assert _same_bits(torch.diagonal(Vs_f, dim1=2, dim2=3), Vs_d), mode
        assert int(torch.count_nonzero(_bits(Vs_f)[..., ~eye])) == 0 if D > 1 else True, mode   # +0.0 everywhere off it


def test_general_models_with_per_chain_parameters_slow_and_occluded_chains(set_knob):
    """a in [0.9, 1], c in +-[0.5, 1.5], q in [0.5, 2], m0 != 0, S0 per chain; a third of the keypoints slow (s = e^-8)
    beside fast ones in the same tile, five occluded."""
    from eks_amd import _lib, hip_ops
    p = wr.general_problem()
    assert (np.diagonal(p['C'], axis1=1, axis2=2) < 0).any()
    assert hip_ops.model_flags(p['S0'], p['A'], p['C'], p['Q']) & _lib.FLAG_DIAG_MODEL      # negative c is accepted
    r = _restated('general', p)
    ms2, Vs2 = _run(set_knob, p, 2)
    grp, nan = _nan_groups(ms2, Vs2)
    assert grp.any() and not grp.all()
    _assert_oracle('general', p, ms2, Vs2, True, stored=~nan)
    # wherever float64 is clear of the tolerance the kernel's verdict is the restatement's
    cls = wr.classify_problem(p)
    A = np.maximum(np.where(cls['cut_front'][:, None], 0.0, cls['A_front']),
                   np.where(cls['cut_back'][:, None], 0.0, cls['A_back']))
    clear = (A <= 2.0 ** -34) | (A >= 2.0 ** -26)
    assert ((A >= 2.0 ** -26) & (A < 2.0 ** -6)).any() and (A <= 2.0 ** -34).any()
    assert np.array_equal(grp[clear], r['fail'][clear])
    ms0, Vs0 = _run(set_knob, p, 0)
    ms1, Vs1 = _run(set_knob, p, 1)
    assert bool(torch.isfinite(ms1).all()) and bool(torch.isfinite(Vs1).all())
    _assert_oracle('general', p, ms1, Vs1, True)
    nan_t = torch.as_tensor(nan).cuda()
    assert torch.equal(ms1[nan_t], ms0[nan_t]) and torch.equal(Vs1[nan_t], Vs0[nan_t])


@pytest.mark.parametrize('kind', ['low', 'high'])
def test_variances_at_the_edges_of_the_clip_in_own_chunks_halos_and_on_the_stand_in_frame(set_knob, kind):
    """Zeros (clipped to 1e-12) and 1e-9 against the information-form oracle; inf and 3e38 (clamped to 1e30: no weight)
    against the oracle fed 1e30.  A whole halo without weight does not forget and must fail the check."""
    p = wr.clip_problem(kind)
    tag = ('clip', kind)
    oracle = _info_form_oracle if kind == 'low' else _oracle
    r = _restated(tag, p)
    ms2, Vs2 = _run(set_knob, p, 2)
    grp, nan = _nan_groups(ms2, Vs2)
    _assert_same_lanes(grp, r['fail'])
    if kind == 'high':
        assert grp[3, 2 * 2 + 0] and grp[5, 2 * 2 + 1] and grp.sum() == 2       # the two whole halos of keypoint 2
    else:
        assert not grp.any()                                                    # a halo of exact frames forgets at once
    _assert_oracle(tag, p, ms2, Vs2, True, stored=~nan, oracle=oracle)
    ms1, Vs1 = _run(set_knob, p, 1)
    assert bool(torch.isfinite(ms1).all()) and bool(torch.isfinite(Vs1).all())
    _assert_oracle(tag, p, ms1, Vs1, True, oracle=oracle)


@pytest.mark.parametrize('T', wr.FAIL_T)
def test_the_lanes_that_fail_are_exactly_those_the_rules_predict(set_knob, T):
    """Occlusions over whole halos, across group boundaries, at both ends of the sequence: the (group, chain) lanes mode
    2 stores as NaN EQUAL the set window_ref.classify predicts - no lane more (a cut halo passes without a check) and no
    lane less.  Every halo of the input is far from the tolerance in float64, so float32 cannot decide otherwise."""
    p = wr.fail_pattern_problem(T)
    cls = wr.classify_problem(p)
    for A, cut in ((cls['A_front'], cls['cut_front']), (cls['A_back'], cls['cut_back'])):
        assert ((A[~cut] <= 2.0 ** -34) | (A[~cut] >= 2.0 ** -26)).all()
    nwg = cls['fail'].shape[0]
    assert cls['cut_front'].tolist() == [True] + [False] * (nwg - 1)
    assert cls['cut_back'].tolist() == [False] * (nwg - 2) + [(T != 4165), True]
    fail = cls['fail']
    assert fail[:2].any() and fail[-2:].any() and not fail[:, 5 * 2 + 0].any()   # (frames 0..63 occluded: nobody fails)
    ms2, Vs2 = _run(set_knob, p, 2)
    grp, nan = _nan_groups(ms2, Vs2)
    _assert_same_lanes(grp, fail)
    tag = ('fail', T)
    _assert_oracle(tag, p, ms2, Vs2, True, stored=~nan)
    ms0, Vs0 = _run(set_knob, p, 0)
    ms1, Vs1 = _run(set_knob, p, 1)
    assert bool(torch.isfinite(ms1).all()) and bool(torch.isfinite(Vs1).all())
    _assert_oracle(tag, p, ms1, Vs1, True)
    nan_t = torch.as_tensor(nan).cuda()
    assert torch.equal(ms1[nan_t], ms0[nan_t]) and torch.equal(Vs1[nan_t], Vs0[nan_t])


def _shifted(like):
    """A copy of `like` that starts at an odd float of a larger allocation."""
    buf = torch.zeros(like.numel() + 3, dtype=torch.float32, device='cuda')
    v = buf[1:1 + like.numel()]
    assert v.data_ptr() % 8 == 4
    v.copy_(like.reshape(-1))
    return v.view(like.shape)


def _row_offset(like):
    """A copy of `like` (T, K, ...) that is rows 1.. of an allocation one frame longer: offset by K * D floats."""
    buf = torch.zeros((like.shape[0] + 1,) + tuple(like.shape[1:]), dtype=torch.float32, device='cuda')
    v = buf[1:]
    v.copy_(like)
    return v


@pytest.mark.parametrize('D,vs_diag,view', [(2, True, 'odd'), (2, False, 'odd'), (3, False, 'odd'), (3, False, 'row'),
                                           (1, True, 'row')])
def test_views_that_are_only_4_byte_aligned_give_the_same_bits(set_knob, D, vs_diag, view):
    """y, var, ms and Vs as views of larger buffers (an odd float in, or one row of K * D floats in: 4-byte aligned
    only): the windowed kernel builds its buffer resources from y + first and stores Vs rows of D floats."""
    from eks_amd import hip_ops
    K = {1: 67, 2: 35, 3: 43}[D]
    s = np.exp(np.random.default_rng(70).uniform(0.0, 4.0, K))
    s[::5] = np.exp(-8.0)                                                  # slow chains: the exact launches store too
    p = wr.problem(1100, K, D, seed=71 + D, s=s)
    p['var'][300:600, 3] *= 1e4
    shift = _shifted if view == 'odd' else _row_offset
    flags = hip_ops.model_flags(p['S0'], p['A'], p['C'], p['Q'])
    f64 = [_dev(p[k], torch.float64) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')]
    for mode in (1, 2):
        ms0, Vs0 = _run(set_knob, p, mode, vs_diag)
        out = (shift(torch.full_like(ms0, float('nan'))), shift(torch.full_like(Vs0, float('nan'))))
        assert (view == 'row' and (K * D) % 2 == 1) or out[0].data_ptr() % 8 == 4
        ms1, Vs1 = hip_ops.smooth(shift(_dev(p['y'])), shift(_dev(p['var'])), *f64, flags=flags, vs_diag=vs_diag,
                                  out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ms0).any()) == (mode == 2)
        assert _same_bits(ms1, ms0) and _same_bits(Vs1, Vs0), mode


@pytest.mark.parametrize('M,r0', wr.OUTLIERS)
def test_an_outlier_on_the_stand_in_frame_stays_inside_the_bar(set_knob, M, r0):
    """The check bounds |A|, not |A| x spread, and the stand-in is one observation.  Halos just inside the tolerance
    (unit model, r = 1, s = 0.12: |A| = 6.3e-10 of 9.3e-10) behind an outlier of 3e4 / 1e6 on a track near 50: float64
    puts the windowed form 2.4e-9 / 8.1e-8 of the magnitude from the exact smoother."""
    p = wr.outlier_problem(M, r0)
    tag = ('outlier', M)
    r = _restated(tag, p)
    assert not r['fail'].any() and 0.5 * wr.TOL < wr.classify_problem(p)['A_front'][1:].max() < wr.TOL
    T, K, D = p['y'].shape
    scale = np.abs(r['ms_x']).max(axis=0)
    e64 = float((np.abs(r['ms'] - r['ms_x']) / scale).max())
    for mode in (2, 1):
        ms, Vs = _run(set_knob, p, mode)
        assert bool(torch.isfinite(ms).all()), 'every lane is stored'
        e32 = float((np.abs(ms.cpu().numpy().reshape(T, K * D).astype(np.float64) - r['ms_x']) / scale).max())
        print(f'outlier {M:g} (variance {r0:g}), mode {mode}: kernel {e32:.3g}, float64 restatement {e64:.3g} of the '
              f'magnitude from the exact smoother')
        _assert_oracle(tag, p, ms, Vs, True)


@pytest.mark.parametrize('general', [False, True])
def test_the_stand_in_is_what_the_first_halo_frame_saw_over_c(set_knob, general):
    """Where the halo forgets, nothing of the stand-in is left to see - so this input lets it through: halos at 0.7 of
    the tolerance and 1e11 (without weight) on the first frame of every front halo.  The windowed result then differs
    from the exact smoother by 1e-3 of the magnitude and more, all of it A x inv x (y / c), and the kernel must agree
    with the float64 restatement of the windowed form: 1e-5 of the magnitude (float32 carries A, a product of 64
    factors, to 4e-6 relative, of a term that is 1e-2 of the magnitude), variances 1e-5 relative."""
    p = wr.stand_in_problem(general)
    r = _restated(('stand-in', general), p)
    T, K, D = p['y'].shape
    assert not r['fail'].any()
    scale = np.abs(r['ms_x']).max(axis=0)
    seen = (np.abs(r['ms'] - r['ms_x']) / scale)[GROUP:].max(axis=0)
    assert (seen > 1e-3).all(), seen
    ms2, Vs2 = _run(set_knob, p, 2)
    assert bool(torch.isfinite(ms2).all()) and bool(torch.isfinite(Vs2).all()), 'every lane is stored'
    em = float((np.abs(ms2.cpu().numpy().reshape(T, K * D).astype(np.float64) - r['ms']) / scale).max())
    eV = float((np.abs(Vs2.cpu().numpy().reshape(T, K * D).astype(np.float64) - r['Ps']) / r['Ps']).max())
    print(f'stand-in visible at {seen.min():.3g} .. {seen.max():.3g} of the magnitude; kernel against the restatement: '
          f'ms {em:.3g}, Vs {eV:.3g}')
    assert em < 1e-5 and eV < 1e-5, (em, eV)


def _workspace_problems():
    T, K = 1100, 64                                                        # 128 chains, two tiles, five window groups
    fast = np.exp(np.random.default_rng(80).uniform(0.0, 4.0, K))
    ps = [wr.problem(T, K, 2, seed=81, s=np.full(K, np.exp(-8.0))), wr.problem(T, K, 2, seed=82, s=fast),
          wr.problem(T, K, 2, seed=83, s=fast[::-1].copy())]
    ps[2]['var'][400:700, 37, 1] *= 1e4
    return ps + [ps[1]]


def test_the_slow_fail_and_gate_planes_of_a_reused_workspace_do_not_leak_between_calls(set_knob, monkeypatch):
    """All chains slow, all fast, fast with one occluded chain, the second again - same shapes, different data, one
    process: through hip_ops.smooth (the allocator hands the same workspace back) and through ONE PreparedSmooth whose
    tensors are overwritten in place.  Every call gives the bits it gives on a workspace of zeros, and on one of 0xFF
    bytes: only the probe clears the planes."""
    from eks_amd import hip_ops
    ps = _workspace_problems()
    plain = hip_ops._workspace
    fresh = []
    for fill in (0, 255):
        monkeypatch.setattr(hip_ops, '_workspace',
                            lambda n, dev, fill=fill: torch.full((max(int(n), 256),), fill, dtype=torch.uint8, device=dev))
        fresh.append([_run(set_knob, p, 1) for p in ps])
    monkeypatch.setattr(hip_ops, '_workspace', plain)
    for a, b in zip(*fresh):
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    fresh = fresh[0]
    for ms, Vs in fresh:
        assert bool(torch.isfinite(ms).all()) and bool(torch.isfinite(Vs).all())
    ms0, Vs0 = _run(set_knob, ps[0], 0)
    assert torch.equal(fresh[0][0], ms0) and torch.equal(fresh[0][1], Vs0)            # all slow: the exact path
    for i, p in enumerate(ps):
        ms, Vs = _run(set_knob, p, 1)
        assert torch.equal(ms, fresh[i][0]) and torch.equal(Vs, fresh[i][1]), ('hip_ops.smooth, call', i + 1)
    flags = hip_ops.model_flags(ps[0]['S0'], ps[0]['A'], ps[0]['C'], ps[0]['Q'])
    y, var = _dev(ps[0]['y']), _dev(ps[0]['var'])
    f64 = [_dev(ps[0][k], torch.float64) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')]
    call = hip_ops.PreparedSmooth(y, var, *f64, flags=flags, vs_diag=True)
    for i, p in enumerate(ps):
        y.copy_(_dev(p['y']))
        var.copy_(_dev(p['var']))
        f64[5].copy_(_dev(p['s'], torch.float64))
        call.ms.fill_(float('nan'))
        call.Vs.fill_(float('nan'))
        ms, Vs = call()
        torch.cuda.synchronize()
        assert torch.equal(ms, fresh[i][0]) and torch.equal(Vs, fresh[i][1]), ('PreparedSmooth, call', i + 1)
    assert torch.equal(fresh[3][0], fresh[1][0]) and torch.equal(fresh[3][1], fresh[1][1])


def test_launch_order_is_not_arithmetic(set_knob):
    """EKS_REPLAY_FORWARD and EKS_SUMMARIZE_REVERSE walk the blocks in the other direction: identical bits in mode 1."""
    p = wr.general_problem()
    ms, Vs = _run(set_knob, p, 1)
    for knob in ('EKS_REPLAY_FORWARD', 'EKS_SUMMARIZE_REVERSE'):
        for value in ('0', '1'):
            set_knob(knob, value)
            ms_k, Vs_k = _run(set_knob, p, 1)
            assert torch.equal(ms_k, ms) and torch.equal(Vs_k, Vs), (knob, value)
        set_knob(knob, None)


def test_host_arrays_pipelined_over_keypoint_tiles_in_the_windowed_form(set_knob, monkeypatch):
    """run_kalman_smoother on NumPy arrays cut into four keypoint tiles of 17 (34 chains, the narrowest that take the
    fused path: no tile of the pipeline holds the chains a 64-chain tile of the untiled call holds), slow and occluded
    chains among them: bit for bit the untiled call, and the oracle's numbers on a sample of keypoints."""
    from eks_amd import core
    from oracle import c_oracle
    set_knob('EKS_SMOOTH_WINDOW_MIN_T', '1024')
    set_knob('EKS_SMOOTH_WINDOW', '1')
    T, K = 2117, 68
    rng = np.random.default_rng(90)
    s = np.where(rng.random(K) < 0.25, np.exp(-8.0), np.exp(rng.uniform(0.0, 4.0, K)))
    p = wr.problem(T, K, 2, seed=91, s=s)
    for kp in (1, 16, 17, 40, 67):
        p['var'][200 + 20 * kp:500 + 20 * kp, kp] *= 1e4
    monkeypatch.setattr(core, '_TILE_MIN_BYTES', 1 << 20)
    monkeypatch.setattr(core, '_TILE_TARGET_BYTES', 17 * T * 10 * 4)
    ys = np.ascontiguousarray(np.transpose(p['y'], (1, 0, 2)))
    args = (ys, p['m0'], p['S0'], p['A'], p['C'], p['Q'], p['var'])
    s1, ms1, Vs1, info = core.run_kalman_smoother(*args, smooth_param=list(s), return_info=True)
    assert info.get('mode') == 'tiled' and len(info['tiles']) == 4, info.get('mode')
    monkeypatch.setenv('EKS_HOST_UNTILED', '1')
    out = {}
    names = _scopes(lambda: out.update(r=core.run_kalman_smoother(*args, smooth_param=list(s), return_info=True)))
    assert 'diag_window_probe' in names and 'diag_replay_exact' in names, names          # the windowed form ran
    s0, ms0, Vs0, info0 = out['r']
    assert info0.get('mode') != 'tiled'
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(ms1, ms0)
    np.testing.assert_array_equal(Vs1, Vs0)
    sel = [0, 1, 16, 17, 33, 40, 66, 67]
    slow = [k for k in range(K) if s[k] < 1.0][:3]
    sel = sorted(set(sel + slow))
    ms_o, Vs_o, _ = c_oracle.smooth(ys[sel].astype(np.float64), np.transpose(p['var'], (1, 0, 2))[sel].astype(np.float64),
                                    p['m0'][sel], p['S0'][sel], p['A'][sel], p['C'][sel], p['Q'][sel], s[sel])
    em = float((np.abs(ms0[sel] - ms_o) / np.abs(ms_o).max(axis=(1, 2), keepdims=True)).max())
    Vd, Vd_o = np.diagonal(Vs0[sel], axis1=2, axis2=3), np.diagonal(Vs_o, axis1=2, axis2=3)
    eV = float((np.abs(Vd - Vd_o) / Vd_o).max())
    print(f'host boundary, windowed: ms {em:.3g}, Vs {eV:.3g} of the oracle (bar 1e-5)')
    assert em < 1e-5 and eV < 1e-5, (em, eV)
    assert not Vs0[:, :, 0, 1].any() and not Vs0[:, :, 1, 0].any()
