"""Windowed replay of the scalar-chain smoother (eks_diag.hip: replay_window_block, the probe and the gated exact
launches behind it) at small shapes: EKS_SMOOTH_WINDOW_MIN_T=1024 lets sequences of a few thousand frames take the
form that long sessions take by default.  EKS_SMOOTH_WINDOW: 0 the scan-based path alone, 1 windowed + fallback,
2 test mode (no probe, no fallback, lanes that fail the check store NaN)."""
import ctypes

import numpy as np
import pytest

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
                                    np.clip(np.transpose(p['var'], (1, 0, 2)).astype(np.float64), 1e-12, None),
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
    ms, Vs = hip_ops.smooth(_dev(p['y'][:, sel]), _dev(p['var'][:, sel]), *f64, flags=flags, vs_diag=vs_diag)
    torch.cuda.synchronize()
    return ms.clone(), Vs.clone()


def _diag(Vs, vs_diag):
    return Vs if vs_diag else torch.diagonal(Vs, dim1=2, dim2=3)


def _assert_oracle(tag, p, ms, Vs, vs_diag):
    ms_o, Vd_o = _oracle(tag, p)
    ms_k = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vd = np.transpose(_diag(Vs, vs_diag).cpu().numpy().astype(np.float64), (1, 0, 2))
    sc = np.abs(ms_o).max(axis=(1, 2), keepdims=True)
    em = float((np.abs(ms_k - ms_o) / sc).max())
    eV = float((np.abs(Vd - Vd_o) / Vd_o).max())
    print(f'{tag}: ms {em:.3g}, Vs {eV:.3g} of the oracle (bar 1e-5)')
    assert em < 1e-5, (tag, em)
    assert eV < 1e-5, (tag, eV)


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
