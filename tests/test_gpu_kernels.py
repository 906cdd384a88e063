"""GPU parity tests: every entry point of libeks_hip.so against the float64 CPU oracle on seeded
inputs small enough for the oracle to finish in seconds.  Tolerances (stated per test) derive from
BASELINE.json's bar: smoothed means / covariances within 1e-5 relative, indices bit-exact."""
import os
import sys

import numpy as np
import pytest

from oracle import eks_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_forms import dense_problem as _dense_problem, rel as _rel  # noqa: E402  (shared with tests/test_gpu_dense_forms.py)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _singlecam_problem(T, K, seed, unit=True):
    from eks_amd import synth
    mk = synth.singlecam_markers(T, K, seed=seed)
    arrs = orc.singlecam_arrays(mk)
    rng = np.random.default_rng(seed)
    if not unit:
        eye = np.eye(2)
        arrs['As'] = eye * rng.uniform(0.9, 1.0, (K, 2))[:, :, None]
        arrs['Cs'] = eye * rng.uniform(0.5, 1.5, (K, 2))[:, :, None]
        arrs['Qs'] = eye * rng.uniform(0.5, 2.0, (K, 2))[:, :, None]
        arrs['m0s'] = rng.standard_normal((K, 2))
    y_tk = np.transpose(arrs['ys'], (1, 0, 2)).astype(np.float32)          # (T,K,2)
    var_tk = arrs['ensemble_vars'].astype(np.float32)                      # (T,K,2)
    arrs['ys'] = np.transpose(y_tk, (1, 0, 2)).astype(np.float64)          # oracle sees f32 inputs
    arrs['ensemble_vars'] = var_tk.astype(np.float64)
    return arrs, y_tk, var_tk


def _params_dev(arrs):
    return [_dev(arrs[k], torch.float64) for k in ('m0s', 'S0s', 'As', 'Cs', 'Qs')]


_NLL_GRID_MEMO = {}


def _nll_grid_oracle(ys, Rc, m0s, S0s, As, Cs, Qs, cand):
    """c_oracle.nll_grid, remembered per input: several tests run the same problem through different kernels (the
    EKS_NLL_LEGACY / EKS_NLL_NOLAG parametrisations, repeated calls) - the C port took most of their time."""
    import hashlib
    from oracle import c_oracle
    h = hashlib.sha1()
    for a in (ys, Rc, m0s, S0s, As, Cs, Qs, cand):
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    key = h.hexdigest()
    if key not in _NLL_GRID_MEMO:
        if len(_NLL_GRID_MEMO) > 8:
            _NLL_GRID_MEMO.clear()
        _NLL_GRID_MEMO[key] = c_oracle.nll_grid(ys, Rc, m0s, S0s, As, Cs, Qs, cand)
    return _NLL_GRID_MEMO[key]


def test_smooth_diag_long_sequence_fused_and_unfused_scan_agree_with_oracle(set_knob):
    """T = 140 000 (4 375 chunks): the fused path's group scan re-reads its aggregates in batches
    (more than 16 per slot); both scan organisations against the C oracle on every frame."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    T, K = 140_000, 40
    rng = np.random.default_rng(9)
    y = np.cumsum(rng.standard_normal((T, K, 2)), axis=0).astype(np.float32)
    var = (0.3 * rng.gamma(2.0, 1.0, (T, K, 2)) + 0.02).astype(np.float32)
    eye = np.tile(np.eye(2), (K, 1, 1))
    m0, S0 = np.zeros((K, 2)), eye * 25.0
    s = np.exp(rng.uniform(-6, 6, K))
    flags = hip_ops.model_flags(S0, eye, eye, eye)
    ms_o, Vs_o, _ = c_oracle.smooth(np.transpose(y, (1, 0, 2)).astype(np.float64),
                                    np.clip(np.transpose(var, (1, 0, 2)).astype(np.float64), 1e-12, None),
                                    m0, S0, eye, eye, eye, s)
    Vd_o = np.diagonal(Vs_o, axis1=2, axis2=3)
    for unfused in ('0', '1'):
        set_knob('EKS_SMOOTH_UNFUSED', unfused)
        ms, Vs = hip_ops.smooth(_dev(y), _dev(var), _dev(m0), _dev(S0), _dev(eye), _dev(eye), _dev(eye), _dev(s),
                                flags=flags, vs_diag=True)
        ms_k = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
        Vd = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2))
        assert _rel(ms_k, ms_o, axis_scale=(1, 2)) < 1e-5
        assert (np.abs(Vd - Vd_o) / Vd_o).max() < 1e-5


@pytest.mark.parametrize('unit', [True, False])
def test_smooth_diag_under_heavy_smoothing_keeps_a_margin(unit):
    """VERDICT r05 item 5 on the device: s q / r ~ 1e-5 ... 1e-3 (and 1 - a ~ 1e-2 for the general diagonal model) - the
    regime of the fuzz sweeps' worst smoothed variance (6.5e-6, s ~ 5e-4).  Round 6's deviation form of the RTS step
    and complement forms of a x / a^2 X (eks_math.hpp): every frame within 3e-6 of the C oracle (tests/test_host_sim.py
    pins the same problem on the CPU)."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    from test_host_sim import _heavy_smoothing_problem
    T, K = 4097, 40
    arrs, y, var, s = _heavy_smoothing_problem(T, K, unit)
    y_tk, var_tk = y.reshape(T, K, 2), var.reshape(T, K, 2)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    ms, Vs = hip_ops.smooth(_dev(y_tk), _dev(var_tk), *_params_dev(arrs), _dev(s), flags=flags, vs_diag=True)
    ms_o, Vd_o, _ = c_oracle.smooth_diag(np.transpose(y_tk, (1, 0, 2)).astype(np.float64),
                                         np.clip(np.transpose(var_tk, (1, 0, 2)).astype(np.float64), 1e-12, None),
                                         arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s)
    ms_k = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vd = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2))
    assert (np.abs(Vd - Vd_o) / Vd_o).max() < 3e-6
    assert _rel(ms_k, ms_o, axis_scale=(1, 2)) < 3e-6


@pytest.mark.parametrize('T,K,vs_diag', [(10_007, 64, True), (2_100, 500, False), (16_000, 33, False)])
def test_smooth_diag_fused_and_three_kernel_scan_match_oracle(set_knob, T, K, vs_diag):
    """Both organisations of the scan (folded into summarize / replay, and the separate three-kernel
    scan) on observations far from the origin, ragged T and ragged tiles: each within 1e-5 of the
    C oracle on every frame."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    rng = np.random.default_rng(T)
    y = (np.cumsum(rng.standard_normal((T, K, 2)), axis=0) + 300.0).astype(np.float32)
    var = (0.3 * rng.gamma(2.0, 1.0, (T, K, 2)) + 0.02).astype(np.float32)
    eye = np.tile(np.eye(2), (K, 1, 1))
    m0, S0 = np.full((K, 2), 300.0), eye * 25.0
    s = np.exp(rng.uniform(-6, 6, K))
    flags = hip_ops.model_flags(S0, eye, eye, eye)
    ms_o, Vs_o, _ = c_oracle.smooth(np.transpose(y, (1, 0, 2)).astype(np.float64),
                                    np.clip(np.transpose(var, (1, 0, 2)).astype(np.float64), 1e-12, None),
                                    m0, S0, eye, eye, eye, s)
    Vd_o = np.diagonal(Vs_o, axis1=2, axis2=3)
    kept = {}
    for unfused, recompute in (('0', '0'), ('0', '1'), ('1', '0')):
        set_knob('EKS_SMOOTH_UNFUSED', unfused)
        # fused form: chunk elements kept between summarize and replay, or summarised again in replay
        # (what wide problems run) - the same arithmetic, so bit-identical outputs
        set_knob('EKS_REPLAY_RECOMPUTE', recompute)
        ms_d, Vs_d = hip_ops.smooth(_dev(y), _dev(var), _dev(m0), _dev(S0), _dev(eye), _dev(eye), _dev(eye),
                                    _dev(s), flags=flags, vs_diag=vs_diag)
        if unfused == '0':
            kept[recompute] = (ms_d.clone(), Vs_d.clone())
        ms, Vs = ms_d.cpu().numpy().astype(np.float64), Vs_d.cpu().numpy().astype(np.float64)
        ms_k = np.transpose(ms, (1, 0, 2))
        assert _rel(ms_k - 300.0, ms_o - 300.0, axis_scale=(1, 2)) < 1e-5
        Vd = np.transpose(Vs, (1, 0, 2)) if vs_diag else \
            np.diagonal(np.transpose(Vs, (1, 0, 2, 3)), axis1=2, axis2=3)
        assert (np.abs(Vd - Vd_o) / Vd_o).max() < 1e-5
    assert torch.equal(kept['0'][0], kept['1'][0]) and torch.equal(kept['0'][1], kept['1'][1])


@pytest.mark.parametrize('T,K,unit,vs_diag', [
    (2000, 4, True, False),      # ibl-pupil-like: 8 chains, several chunks per wave
    (1537, 37, True, True),      # ragged T (not a multiple of the 32-frame chunk), ragged N
    (3000, 64, False, False),    # general diagonal a, c, q
    (33, 3, True, False),        # two chunks
    (1, 2, True, False),         # single frame
    (700, 200, False, True),     # several chain tiles
])
@pytest.mark.parametrize('recompute', ['0', '1'])
def test_smooth_diag_matches_oracle(T, K, unit, vs_diag, recompute, set_knob):
    from eks_amd import hip_ops
    # fused form (>= 64 chains): chunk elements kept between the two kernels or summarised again
    set_knob('EKS_REPLAY_RECOMPUTE', recompute)
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=T + K, unit=unit)
    rng = np.random.default_rng(1)
    if T == 1:      # nanvar over one frame is 0: give the prior a real variance
        arrs['S0s'] = np.tile(np.eye(2) * 3.0, (K, 1, 1))
    s = np.exp(rng.uniform(-8, 8, K))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    assert flags & 1 and bool(flags & 4) == unit
    ms, Vs = hip_ops.smooth(_dev(y_tk), _dev(var_tk), *_params_dev(arrs), _dev(s), flags=flags,
                            vs_diag=vs_diag)
    ms = ms.cpu().numpy().astype(np.float64)
    Vs = Vs.cpu().numpy().astype(np.float64)
    Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
    ms_o, Vs_o, _ = orc.kalman_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'],
                                        arrs['Cs'], arrs['Qs'], s, Rd)
    ms_k = np.transpose(ms, (1, 0, 2))
    assert _rel(ms_k, ms_o, axis_scale=(1, 2)) < 1e-5
    if vs_diag:
        Vd_o = np.diagonal(Vs_o, axis1=2, axis2=3)
        assert (np.abs(np.transpose(Vs, (1, 0, 2)) - Vd_o) / Vd_o).max() < 1e-5   # elementwise
    else:
        Vk = np.transpose(Vs, (1, 0, 2, 3))
        assert np.all(Vk[:, :, 0, 1] == 0) and np.all(Vk[:, :, 1, 0] == 0)
        Vd = np.diagonal(Vk, axis1=2, axis2=3)
        Vd_o = np.diagonal(Vs_o, axis1=2, axis2=3)
        assert (np.abs(Vd - Vd_o) / Vd_o).max() < 1e-5

@pytest.mark.parametrize('T,K', [(3000, 64), (700, 5)])
def test_smooth_diag_into_buffers_at_odd_float_offsets(T, K):
    """The C ABI takes plain pointers: inputs and outputs that are only 4-byte aligned (views starting
    at an odd float of a larger allocation) must give bit-identical results to aligned ones - the 2x2
    covariance rows leave as 8-byte stores, the rows are addressed through buffer resources."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=T + K, unit=True)
    s = _dev(np.exp(np.random.default_rng(2).uniform(-4, 4, K)))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, var = _dev(y_tk), _dev(var_tk)
    ms0, Vs0 = hip_ops.smooth(y, var, *_params_dev(arrs), s, flags=flags)

    def shifted(n, like=None):
        buf = torch.zeros(n + 3, dtype=torch.float32, device='cuda')
        v = buf[1:1 + n]
        assert v.data_ptr() % 8 == 4
        if like is not None:
            v.copy_(like.reshape(-1))
        return v

    y1 = shifted(y.numel(), y).view(T, K, 2)
    var1 = shifted(var.numel(), var).view(T, K, 2)
    ms1 = shifted(ms0.numel()).view(T, K, 2)
    Vs1 = shifted(Vs0.numel()).view(T, K, 2, 2)
    hip_ops.smooth(y1, var1, *_params_dev(arrs), s, flags=flags, out=(ms1, Vs1))
    assert torch.equal(ms1, ms0) and torch.equal(Vs1, Vs0)


@pytest.mark.parametrize('sval', [np.exp(-8.0), 0.3, 2980.0])
def test_smooth_diag_with_variances_at_the_clip(sval):
    """Ensemble variance 0 -> 1e-12 (eks/utils.py:373) on the scalar-chain path: whole frames,
    single coordinates and runs of frames at the clip; posterior variances compared ELEMENTWISE
    (they span 12 decades along time)."""
    from eks_amd import hip_ops
    T, K = 2500, 6
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=91, unit=True)
    var_tk = var_tk.copy()
    var_tk[::7, :, 0] = 0.0
    var_tk[3::11] = 1e-9
    var_tk[1000:1040, 2] = 0.0
    arrs['ensemble_vars'] = var_tk.astype(np.float64)
    s = np.full(K, sval)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    ms, Vs = hip_ops.smooth(_dev(y_tk), _dev(var_tk), *_params_dev(arrs), _dev(s), flags=flags, vs_diag=True)
    ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vs = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2))
    # information-form oracle: the covariance-form P - K S K' cannot resolve a 1e-12 posterior
    # variance under a 1e4 prior (its own rounding is 100 % of the result there)
    Rd = np.maximum(np.swapaxes(arrs['ensemble_vars'], 0, 1), 1e-12)
    ms_o, Vs_o = orc.info_form_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                                        arrs['Qs'], s, Rd)[:2]
    assert _rel(ms, ms_o, axis_scale=(1, 2)) < 1e-5
    Vd_o = np.diagonal(Vs_o, axis1=2, axis2=3)
    assert (np.abs(Vs - Vd_o) / Vd_o).max() < 1e-5


@pytest.mark.parametrize('T,K,D,O,general_A', [
    (1200, 4, 3, 4, False),      # mirror-mouse shape: 2 views, n_latent 3
    (300, 3, 3, 6, False),
    (257, 2, 4, 8, False),       # 4 cameras, n_latent 4
    (200, 2, 5, 8, True),
    (150, 5, 2, 2, True),        # non-diagonal 2x2 goes through the dense path
    (64, 2, 1, 3, False),
    (100, 2, 6, 8, False),
    (1, 3, 3, 4, False),         # a single frame: the prior updated once, nothing to scan
    (2, 2, 3, 4, False),
    (7, 5, 2, 6, False),         # one ragged 8-frame chunk
    (9, 4, 3, 2, False),         # two chunks, the second of one frame
    (513, 2, 3, 4, True),        # 65 chunks: two 64-chunk units per keypoint, the second nearly empty
    (400, 2, 3, 12, False),      # six cameras (the fly rig without a calibration): the narrow kernels' widest rows
    (257, 3, 3, 10, True),       # five cameras, 8-byte row pieces
])
def test_smooth_dense_matches_oracle(T, K, D, O, general_A):
    from eks_amd import hip_ops
    arrs, y, var = _dense_problem(T, K, D, O, seed=T + D)
    if general_A:
        rng = np.random.default_rng(9)
        arrs['As'] = arrs['As'] * 0.97 + 0.02 * rng.standard_normal((K, D, D))
    s = np.exp(np.random.default_rng(2).uniform(-3, 4, K))
    for vs_diag in (False, True):
        ms, Vs = hip_ops.smooth(_dev(y), _dev(var), *_params_dev(arrs), _dev(s), flags=0,
                                vs_diag=vs_diag)
        ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
        Vs = Vs.cpu().numpy().astype(np.float64)
        Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
        ms_o, Vs_o, _ = orc.kalman_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'],
                                            arrs['Cs'], arrs['Qs'], s, Rd)
        assert _rel(ms, ms_o, axis_scale=(1, 2)) < 1e-5
        if vs_diag:
            Vk = np.transpose(Vs, (1, 0, 2))
            ref = np.diagonal(Vs_o, axis1=2, axis2=3)
        else:
            Vk = np.transpose(Vs, (1, 0, 2, 3))
            ref = Vs_o
        assert _rel(Vk, ref, axis_scale=tuple(range(1, ref.ndim))) < 1e-5

@pytest.mark.parametrize('chunk', ['2', '4', '8'])
@pytest.mark.parametrize('T,K,D,O,general_A', [(1201, 4, 3, 4, False), (515, 2, 2, 6, True), (131, 3, 3, 8, False),
                                               (3, 2, 3, 4, False)])
def test_dense_wave_kernels_at_every_chunk_length_match_oracle(T, K, D, O, general_A, chunk, set_knob):
    """The narrow-session kernels choose 2, 4 or 8 frames per lane from the problem's size (round 4: short sessions
    are depth-bound and want short chunks); here every choice is forced (EKS_DW_CHUNK) on ragged shapes: the
    smoother against the oracle at 1e-5, the loss and its smoothing-distribution gradient at the float64 bars."""
    from eks_amd import _lib, hip_ops
    set_knob('EKS_DW_CHUNK', chunk)
    arrs, y, var = _dense_problem(T, K, D, O, seed=31 + T)
    if general_A:
        arrs['As'] = arrs['As'] * 0.97 + 0.02 * np.random.default_rng(9).standard_normal((K, D, D))
    s = np.exp(np.random.default_rng(3).uniform(-3, 4, K))
    ms, Vs = hip_ops.smooth(_dev(y), _dev(var), *_params_dev(arrs), _dev(s), flags=0)
    ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vs = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2, 3))
    Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
    ms_o, Vs_o, _ = orc.kalman_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, Rd)
    assert _rel(ms, ms_o, axis_scale=(1, 2)) < 1e-5
    assert _rel(Vs, Vs_o, axis_scale=(1, 2, 3)) < 1e-5
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    assert flags == _lib.FLAG_Q_PD
    rconst = hip_ops.const_r(_dev(var), 1e-4)
    nll1, g1 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(_dev(y), rconst, *_params_dev(arrs), _dev(s[:, None]),
                                                           per_keypoint=True, want_grad=True, flags=flags)]
    ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s,
                               rconst.cpu().numpy(), want_grad=True)
    assert (np.abs(nll1 - ref) / np.abs(ref)).max() < 1e-8
    assert (np.abs(g1 - gref) / np.abs(gref).max()).max() < 1e-7


@pytest.mark.parametrize('T,K,D,O,general_A', [
    (100, 1200, 3, 4, False),   # 1 200 (keypoint, 64-chunk) units > 1 024: keypoint-major kernels, 16-frame chunks
    (8000, 600, 3, 4, False),   # K T / 16 > 2^18: 32-frame chunks, eight checkpoints per lane, scan over 250 chunks
    (131, 1100, 2, 6, False),   # ragged last chunk and last group, D = 2, three cameras
    (70, 1100, 3, 8, True),     # non-identity dynamics, four cameras
    (1, 1500, 3, 4, False),     # a single frame
    (3, 1300, 2, 2, False),     # one ragged group
])
def test_smooth_dense_wide_sessions_match_oracle(T, K, D, O, general_A, set_knob):
    """Wide sessions run the keypoint-major kernels: rows prefetched a group of four frames ahead, filtered beliefs
    as LDS checkpoints per group with the group filtered again on the way back, a per-lane sequential two-level
    scan in between (eks_dense_wide.hip); the same with the narrow path's tree scan (EKS_DENSE_TREE_SCAN=1), and
    (EKS_DENSE_LEGACY=1) the round-1 kernels with their scratch stream; all against the C port of the reference
    recursion on every frame."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    arrs, y, var = _dense_problem(T, K, D, O, seed=T + K)
    if general_A:
        arrs['As'] = arrs['As'] * 0.97 + 0.02 * np.random.default_rng(9).standard_normal((K, D, D))
    s = np.exp(np.random.default_rng(3).uniform(-3, 4, K))
    Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
    ms_o, Vs_o, _ = c_oracle.smooth(arrs['ys'], Rd, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s)
    for legacy, tree in (('0', '0'), ('0', '1'), ('1', '0')):
        set_knob('EKS_DENSE_LEGACY', legacy)
        set_knob('EKS_DENSE_TREE_SCAN', tree)        # the narrow path's tree scan under the wide kernels
        ms, Vs = hip_ops.smooth(_dev(y), _dev(var), *_params_dev(arrs), _dev(s), flags=0)
        ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
        Vs = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2, 3))
        assert _rel(ms, ms_o, axis_scale=(1, 2)) < 1e-5
        assert _rel(Vs, Vs_o, axis_scale=(1, 2, 3)) < 1e-5


@pytest.mark.parametrize('T,K,D,O', [(500, 3, 2, 2), (40, 1301, 2, 2), (300, 5, 3, 6)])
def test_smooth_dense_accepts_views_that_are_only_4_byte_aligned(T, K, D, O):
    """y / var as row-offset views of larger arrays (K O 4 bytes per row is not a multiple of 16 here): the narrow
    and the keypoint-major kernels read a keypoint's O values as 8- / 16-byte pieces whose load type only promises
    4 bytes - same bits as from freshly allocated (256-byte aligned) copies."""
    from eks_amd import hip_ops
    arrs, y, var = _dense_problem(T + 1, K, D, O, seed=3 + T)
    s = _dev(np.exp(np.random.default_rng(2).uniform(-2, 2, K)))
    yb, vb = _dev(y), _dev(var)
    yv, vv = yb[1:], vb[1:]
    assert yv.data_ptr() % 16 != 0 and yv.is_contiguous()
    ms_v, Vs_v = hip_ops.smooth(yv, vv, *_params_dev(arrs), s, flags=0)
    ms_a, Vs_a = hip_ops.smooth(yv.clone(), vv.clone(), *_params_dev(arrs), s, flags=0)
    assert torch.equal(ms_v, ms_a) and torch.equal(Vs_v, Vs_a)


@pytest.mark.parametrize('case', ['all_clipped', 'tiny', 'one_clipped'])
@pytest.mark.parametrize('sval', [10.0, 1e-3])
def test_smooth_dense_with_variances_at_the_clip(case, sval):
    """Ensemble variance 0 (identical members) is clipped to 1e-12 upstream (eks/utils.py:373).
    Whole frames at the clip / at 1e-8 are compared with the information-form oracle (the
    covariance-form recursion itself loses 1e-2 there: cond(S) ~ 1e9 with O > D); a single
    clipped coordinate among ordinary ones with the covariance form (the information form is the
    inaccurate one when scales are mixed inside a frame)."""
    from eks_amd import hip_ops
    T, K, D, O = 1500, 3, 3, 4
    arrs, y, var = _dense_problem(T, K, D, O, seed=77)
    arrs['Cs'] = np.ascontiguousarray(np.linalg.qr(arrs['Cs'])[0])
    if case == 'all_clipped':
        var[2::9] = 0.0
    elif case == 'tiny':
        var[::5] = 1e-8
    else:
        var[::7, :, 1] = 0.0
    rng = np.random.default_rng(5)
    x = np.cumsum(rng.standard_normal((K, T, D)) * 0.5, axis=1)
    y = (np.einsum('kod,ktd->tko', arrs['Cs'], x)
         + rng.standard_normal((T, K, O)) * np.sqrt(np.maximum(var, 1e-12))).astype(np.float32)
    arrs['ys'] = np.transpose(y, (1, 0, 2)).astype(np.float64)
    s = np.full(K, sval)
    ms, Vs = hip_ops.smooth(_dev(y), _dev(var), *_params_dev(arrs), _dev(s), flags=0)
    ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vs = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2, 3))
    Rd = np.maximum(np.swapaxes(var.astype(np.float64), 0, 1), 1e-12)
    args = (arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, Rd)
    ms_o, Vs_o = orc.kalman_smoother(*args)[:2] if case == 'one_clipped' else orc.info_form_smoother(*args)[:2]
    assert _rel(ms, ms_o, axis_scale=(1, 2)) < 1e-5
    assert (np.abs(Vs - Vs_o) / np.abs(Vs_o).max(axis=1, keepdims=True)).max() < 1e-5


@pytest.mark.parametrize('T,N', [(2001, 7), (2000, 70), (1, 3), (2, 5), (300, 130), (1024, 5), (1025, 66),
                                 (30011, 130)])
def test_const_r_is_exact_median(T, N):
    from eks_amd import hip_ops
    rng = np.random.default_rng(T + N)
    var = rng.gamma(2.0, 0.3, (T, N, 1)).astype(np.float32)
    var[rng.random((T, N, 1)) < 0.05] = 0.0                    # below the 1e-12 clip
    if T > 10:
        var[3:9, 0, 0] = var[5, 0, 0]                          # duplicates around the middle
        var[:, 1, 0] = 0.25                                    # constant column (radix fallback)
        var[rng.random(T) < 0.3, 2, 0] = np.nan                # NaNs are ignored (nanmedian)
        var[:, 3, 0] = np.round(var[:, 3, 0], 1)               # heavily quantised values
        var[: T // 2, 4, 0] *= 1e-3                            # bimodal: median sits in a gap
    got = hip_ops.const_r(_dev(var), 1e-4).cpu().numpy()
    ref = orc.constant_R_from_timevarying(
        np.clip(var.astype(np.float64), 1e-12, None)[:, :, 0].T[:, :, None], 1e-4)[:, 0]
    # selection is exact: the only arithmetic is the mean of the two middle float32 values
    np.testing.assert_allclose(got[:, 0], ref, rtol=1e-15, atol=0)


@pytest.mark.parametrize('T', [400_000, 1_000_003])
def test_const_r_long_sequences_select_from_the_list_in_global_memory(T):
    """Sequences whose bracket (~7 % of the frames) outgrows the finish kernel's LDS list (T > ~230 000): the exact
    median comes from a radix select over the chain's list in global memory (round 4; before, from five strided
    sweeps of the whole column).  Bit-exact against numpy on continuous, NaN-carrying, quantised (the list overflows
    its capacity too: whole-column fallback) and constant columns."""
    from eks_amd import hip_ops
    rng = np.random.default_rng(T)
    N = 6
    var = rng.gamma(2.0, 0.3, (T, N, 1)).astype(np.float32)
    var[rng.random(T) < 0.2, 1, 0] = np.nan
    var[:, 2, 0] = np.round(var[:, 2, 0], 1)                   # ~13 % of the frames share the median's value
    var[:, 3, 0] = 0.5
    var[: T // 2, 4, 0] *= 1e-3                                # bimodal: the median sits in a gap
    var[rng.random(T) < 0.05, 5, 0] = 0.0                      # below the 1e-12 clip
    got = hip_ops.const_r(_dev(var), 1e-4).cpu().numpy()[:, 0]
    ref = np.maximum(np.nanmedian(np.clip(var[:, :, 0].astype(np.float64), 1e-12, None), axis=0), 1e-4)
    np.testing.assert_array_equal(got, ref)


def test_const_r_all_nan_column():
    from eks_amd import hip_ops
    var = np.full((50, 2, 1), np.nan, np.float32)
    var[:, 1, 0] = 2.0
    got = hip_ops.const_r(_dev(var), 1e-4).cpu().numpy()
    assert np.isnan(got[0, 0]) and got[1, 0] == 2.0


@pytest.mark.parametrize('T,K,unit,n_cand', [(5000, 6, True, 64), (2500, 3, False, 64), (100, 2, True, 64),
                                             (3000, 40, True, 10), (1200, 4, False, 3)])
def test_nll_grid_diag_matches_oracle(T, K, unit, n_cand):
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=7 + T, unit=unit)
    cand = np.exp(np.linspace(-8, 8, n_cand))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    Rc = orc.constant_R_from_timevarying(orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1)))
    np.testing.assert_allclose(rconst.cpu().numpy(), Rc, rtol=1e-15)
    nll = hip_ops.nll(_dev(y_tk), rconst, *_params_dev(arrs), _dev(cand), flags=flags).cpu().numpy()
    ref = np.stack([orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                                   arrs['Qs'], np.full(K, sc), Rc) for sc in cand], axis=1)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-5
    # indices bit-exact wherever the oracle's own margin is above the value tolerance
    srt = np.sort(ref, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 2e-5 * np.abs(srt[:, 0])
    s_sel, idx = hip_ops.argmin_s(_dev(nll), _dev(cand))
    np.testing.assert_array_equal(idx.cpu().numpy(), nll.argmin(axis=1))
    np.testing.assert_array_equal(idx.cpu().numpy()[clear], ref.argmin(axis=1)[clear])
    np.testing.assert_array_equal(s_sel.cpu().numpy(), cand[nll.argmin(axis=1)])
    assert clear.all()


@pytest.mark.parametrize('legacy', ['0', '1'])
@pytest.mark.parametrize('T,K,unit', [(700, 40, True), (1300, 70, False), (4500, 33, True)])
def test_nll_grid_staged_kernel_matches_c_oracle(T, K, unit, legacy, set_knob):
    """>= 64 chains and 64 candidates take the tile kernels (ragged last chunk / tile / 8-frame block, partially
    filled last chain tile): the general kernel (8 candidate groups per block; EKS_NLL_LEGACY=1, and by itself on
    sequences too short for chunks past the first) and the head + lean grid kernel of round 4."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    set_knob('EKS_NLL_LEGACY', legacy)
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=17 + T, unit=unit)
    cand = np.exp(np.linspace(-8, 8, 64))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    nll = hip_ops.nll(_dev(y_tk), rconst, *_params_dev(arrs), _dev(cand), flags=flags).cpu().numpy()
    ref = _nll_grid_oracle(arrs['ys'], rconst.cpu().numpy(), arrs['m0s'], arrs['S0s'], arrs['As'],
                            arrs['Cs'], arrs['Qs'], cand)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-5
    srt = np.sort(ref, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 2e-5 * np.abs(srt[:, 0])
    np.testing.assert_array_equal(nll.argmin(axis=1)[clear], ref.argmin(axis=1)[clear])
    assert clear.mean() > 0.9

@pytest.mark.parametrize('legacy', ['0', '1'])
@pytest.mark.parametrize('T,K,unit,var_scale', [(40000, 32, True, 1.0), (26001, 40, False, 1.0),
                                                (40000, 32, True, 60.0), (9000, 70, True, 0.05),
                                                (20011, 70, False, 9.0), (20011, 70, True, 44.0)])
def test_nll_grid_converged_entry_chunks_match_c_oracle(T, K, unit, var_scale, legacy, set_knob):
    """Long sequences: chunks after the first are summarised for an entering belief N(m, P_inf)
    (no start-up transient), the first chunk is short, rows are read through buffer resources.
    var_scale moves the candidates' closed-loop poles: large R makes the slow candidates fall back
    to exact-entry summaries in the early chunks, small R makes every candidate fast.  The last two
    cases are the corner a fuzz sweep found (tools/fuzz_parity.py 40 77): poles within 1e-2 of one,
    where a pole assembled in float32 cost 1.1e-5 / 8.9e-6 on the NLL (round 2: formed in float64, rounded
    once; round 5: the recursion in the complement form for poles above 0.98 and the variance tracked as its deviation
    from the fixed point - bound 3e-6 there)."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    set_knob('EKS_NLL_LEGACY', legacy)       # 1: the general kernel; 0: the head + lean grid kernel (round 4)
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=5 + T, unit=unit)
    var_tk = (var_tk * var_scale).astype(np.float32)
    cand = np.exp(np.linspace(-8, 8, 64))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    nll = hip_ops.nll(_dev(y_tk), rconst, *_params_dev(arrs), _dev(cand), flags=flags).cpu().numpy()
    ref = _nll_grid_oracle(arrs['ys'], rconst.cpu().numpy(), arrs['m0s'], arrs['S0s'], arrs['As'],
                            arrs['Cs'], arrs['Qs'], cand)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < (3e-6 if T == 20011 else 1e-5)
    srt = np.sort(ref, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 2e-5 * np.abs(srt[:, 0])
    np.testing.assert_array_equal(nll.argmin(axis=1)[clear], ref.argmin(axis=1)[clear])
    assert clear.mean() > 0.9


@pytest.mark.parametrize('legacy', ['0', '1'])
@pytest.mark.parametrize('unit', [True, False])
def test_nll_grid_slow_poles_keep_a_margin(unit, legacy, set_knob):
    """VERDICT r04 item 2.  Variances x 1000 (median R ~ 270: what a recording full of NaN -> 1000 replacements looks
    like, eks/core.py:82-83) put the poles of the slowest third of the grid within 1e-3 ... 1e-2 of one, where a float32
    pole is off by 3e-8 / (1 - rho) of the gain: 7.0e-6 on the grid kernel and 1.05e-5 on the general kernel at the end
    of round 4.  Round 5: the recursion runs in the complement form d' = d + (u - (1 - rho) d) for poles above 0.98
    (1 - rho rounded once from float64), in every regime, and the transient tracks the variance's deviation from its
    fixed point (a product of factors below one: no stall, so the snap onto the fixed point happens at 1e-6 of it,
    not at 1e-4).  Both kernels (EKS_NLL_LEGACY 0 / 1), unit and general diagonal model: <= 3e-6."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    set_knob('EKS_NLL_LEGACY', legacy)
    T, K = 20_000, 40
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=9, unit=unit)
    var_tk = (var_tk * 1000.0).astype(np.float32)
    cand = np.exp(np.linspace(-8, 8, 64))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    nll = hip_ops.nll(_dev(y_tk), rconst, *_params_dev(arrs), _dev(cand), flags=flags).cpu().numpy()
    ref = _nll_grid_oracle(arrs['ys'], rconst.cpu().numpy(), arrs['m0s'], arrs['S0s'], arrs['As'],
                            arrs['Cs'], arrs['Qs'], cand)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 3e-6
    np.testing.assert_array_equal(nll.argmin(axis=1), ref.argmin(axis=1))


@pytest.mark.parametrize('T,K,D,unit,n_cand,per_kp,var_scale,chunk', [
    (30000, 33, 2, True, 64, False, 1.0, 0),        # one ragged tile beside a full one
    (9000, 40, 2, False, 40, False, 1.0, 0),        # candidates not a multiple of 16: the last lean wave is half used
    (5000, 70, 2, True, 17, False, 1.0, 0),         # one full lean wave + one candidate
    (12000, 36, 2, True, 64, True, 1.0, 0),         # a grid per keypoint
    (16000, 17, 4, False, 32, False, 1.0, 0),       # four chains per keypoint (shuffle sum over 4 lanes)
    (2100, 64, 2, True, 64, False, 1.0, 0),         # just past the shortest sequence the kernel takes
    (30000, 40, 2, True, 64, False, 400.0, 0),      # poles at 0.999: the slow groups' chunks fall back to exact entry
    (30000, 40, 2, False, 64, False, 30.0, 512),    # short chunks: rho^t outlives them for the slow groups
    (20000, 64, 1, True, 64, False, 1.0, 800),      # one chain per keypoint, two rounds of blocks
    (9000, 40, 2, True, 96, False, 1.0, 0),         # more than 64 candidates: the general kernel takes the call
    (6000, 33, 2, True, 16, False, 1.0, 0),         # exactly one lean wave of candidates
])
def test_nll_grid_lean_kernel_shapes_and_fallbacks(T, K, D, unit, n_cand, per_kp, var_scale, chunk, set_knob):
    """diag_nll_grid_kernel (round 4): head role (chunk 0 at 4 candidates per lane) + lean role (16 candidates per
    lane, converged entry, constants in LDS) + the exact-entry fallback of a wave whose chunk does not qualify
    (flagged: its (tile, candidate) blocks of the assembly take the sequential walk) - against the C oracle, and
    against the general kernel (EKS_NLL_LEGACY=1) the two must agree far inside the bar."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    rng = np.random.default_rng(T + K)
    if D == 2:
        arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=3 + T, unit=unit)
    else:
        # K keypoints of D independent coordinates each (a diagonal model with D chains per keypoint)
        sub = [_singlecam_problem(T, K, seed=3 + T + 7 * i, unit=unit) for i in range((D + 1) // 2)]
        y_tk = np.concatenate([s_[1] for s_ in sub], axis=2)[:, :, :D].copy()
        var_tk = np.concatenate([s_[2] for s_ in sub], axis=2)[:, :, :D].copy()
        eye = np.eye(D)
        diag = lambda lo, hi: eye * rng.uniform(lo, hi, (K, D))[:, :, None]
        arrs = dict(m0s=np.zeros((K, D)), S0s=diag(1.0, 5.0), As=np.tile(eye, (K, 1, 1)) if unit else diag(0.93, 1.0),
                    Cs=np.tile(eye, (K, 1, 1)) if unit else diag(0.6, 1.4),
                    Qs=np.tile(eye, (K, 1, 1)) if unit else diag(0.5, 2.0))
        arrs['ys'] = np.transpose(y_tk, (1, 0, 2)).astype(np.float64)
    var_tk = (var_tk * var_scale).astype(np.float32)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    if per_kp:
        cand = np.exp(rng.uniform(-8, 8, (K, n_cand)))
    else:
        cand = np.exp(np.linspace(-8, 8, n_cand))
    if chunk:
        set_knob('EKS_NLL_CHUNK', str(chunk))
    args = (_dev(y_tk), rconst, *_params_dev(arrs), _dev(cand))
    nll = hip_ops.nll(*args, per_keypoint=per_kp, flags=flags).cpu().numpy()
    Rc = rconst.cpu().numpy()
    if per_kp:
        ref = np.stack([c_oracle.nll_grid(arrs['ys'][k:k + 1], Rc[k:k + 1], arrs['m0s'][k:k + 1], arrs['S0s'][k:k + 1],
                                          arrs['As'][k:k + 1], arrs['Cs'][k:k + 1], arrs['Qs'][k:k + 1], cand[k])[0]
                        for k in range(K)])
    else:
        ref = _nll_grid_oracle(arrs['ys'], Rc, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], cand)
    assert np.isfinite(nll).all()
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-5
    srt = np.sort(ref, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 2e-5 * np.abs(srt[:, 0])
    np.testing.assert_array_equal(nll.argmin(axis=1)[clear], ref.argmin(axis=1)[clear])
    set_knob('EKS_NLL_LEGACY', '1')
    nll_old = hip_ops.nll(*args, per_keypoint=per_kp, flags=flags).cpu().numpy()
    assert (np.abs(nll - nll_old) / np.abs(ref)).max() < 1e-5          # (each is within 1e-5 of the oracle)


@pytest.mark.parametrize('T,K,unit,n_cand,var_scale,nolag', [
    (30000, 33, True, 64, 1.0, '0'),       # the shared-lag form with a ragged tile and a ragged last chunk
    (30000, 33, True, 64, 1.0, '1'),       # the same call with the form switched off: the round-4 summaries
    (9000, 40, False, 40, 1.0, '0'),       # 40 candidates: the last candidate group is half used
    (30000, 40, True, 64, 400.0, '0'),     # poles at 0.999: flagged (tile, candidate)s take the sequential walk
    (2100, 64, True, 64, 1.0, '0'),        # two chunks
    (1500, 8, True, 64, 1.0, '0'),         # too short / too narrow for the grid kernel: nll + argmin one after the other
])
def test_nll_argmin_is_the_table_plus_numpys_argmin(T, K, unit, n_cand, var_scale, nolag, set_knob):
    """eks_nll_argmin (round 5: the argmin is taken inside the assembly of the table by the block that finishes a
    tile last): the table within 1e-5 of the C oracle, the indices EXACTLY numpy.argmin of the table it returns, s the
    candidate at that index; and the table equals eks_nll's bit for bit."""
    from eks_amd import hip_ops
    from oracle import c_oracle
    set_knob('EKS_NLL_NOLAG', nolag)
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=11 + T, unit=unit)
    var_tk = (var_tk * var_scale).astype(np.float32)
    cand = np.exp(np.linspace(-8, 8, n_cand))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    args = (_dev(y_tk), rconst, *_params_dev(arrs), _dev(cand))
    for rep in range(3):                   # (the assembly's tickets must come back to zero)
        nll, s_sel, idx = hip_ops.nll_argmin(*args, flags=flags)
        nll, s_sel, idx = nll.cpu().numpy(), s_sel.cpu().numpy(), idx.cpu().numpy()
        ref = _nll_grid_oracle(arrs['ys'], rconst.cpu().numpy(), arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                                arrs['Qs'], cand)
        assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-5
        np.testing.assert_array_equal(idx, nll.argmin(axis=1))
        np.testing.assert_array_equal(s_sel, cand[idx])
        np.testing.assert_array_equal(nll, hip_ops.nll(*args, flags=flags).cpu().numpy())


@pytest.mark.parametrize('T,K,unit', [(3000, 5, True), (1500, 3, False)])
def test_nll_grad_diag_matches_oracle(T, K, unit):
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=3 + T, unit=unit)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    Rc = rconst.cpu().numpy()
    s = np.exp(np.random.default_rng(0).uniform(-6, 6, K))
    nll, g = hip_ops.nll(_dev(y_tk), rconst, *_params_dev(arrs), _dev(s[:, None]), per_keypoint=True,
                         want_grad=True, flags=flags)
    ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                               arrs['Qs'], s, Rc, want_grad=True)
    assert (np.abs(nll.cpu().numpy()[:, 0] - ref) / np.abs(ref)).max() < 1e-5
    assert (np.abs(g.cpu().numpy()[:, 0] - gref) / np.abs(gref).max()).max() < 1e-4


@pytest.mark.parametrize('T,K,unit', [(5000, 40, True), (2111, 33, False)])
def test_nll_grad_single_launch_matches_oracle_and_two_launch_form(T, K, unit, set_knob):
    """More than 32 chains: value + gradient come from ONE launch (diag_nll_grad_fused_kernel: chunk summaries
    composed in the block, the tile's last block finishes) - against the oracle, and against the two-launch
    form (float32 summary planes + tree kernel) it replaces.  K = 40 / 33: the last 64-chain tile is partial."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=5 + T, unit=unit)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    s = np.exp(np.random.default_rng(1).uniform(-6, 6, K))
    args = (_dev(y_tk), rconst, *_params_dev(arrs), _dev(s[:, None]))
    nll, g = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
    ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s,
                               rconst.cpu().numpy(), want_grad=True)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-5
    assert (np.abs(g - gref) / np.abs(gref).max()).max() < 1e-4
    set_knob('EKS_NLL_GRAD_UNFUSED', '1')
    nll2, g2 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
    assert (np.abs(nll - nll2) / np.abs(ref)).max() < 2e-6
    assert (np.abs(g - g2) / np.abs(gref).max()).max() < 2e-5
    # round 5: where a tile's poles allow, the launch sums converged-entry chunk terms instead of composing chunk
    # summaries (gf_conv_body); EKS_NLL_GRAD_TREE=1 keeps the compositions everywhere
    set_knob('EKS_NLL_GRAD_UNFUSED', None)
    set_knob('EKS_NLL_GRAD_TREE', '1')
    nll3, g3 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
    assert (np.abs(nll - nll3) / np.abs(ref)).max() < 2e-6
    assert (np.abs(g - g3) / np.abs(gref).max()).max() < 2e-5


@pytest.mark.parametrize('unit', [True, False])
def test_nll_grad_sum_of_chunk_terms_matches_oracle_on_fast_poles(unit, set_knob):
    """Every keypoint's pole dies within a chunk (s >= 0.05 at R ~ 0.3: rho < 0.8): all tiles take gf_conv_body.
    Against the oracle and against the tree form (which must differ in the low bits - or the new path did not run)."""
    from eks_amd import hip_ops
    T, K = 30_000, 70
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=77, unit=unit)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rconst = hip_ops.const_r(_dev(var_tk), 1e-4)
    s = np.exp(np.random.default_rng(2).uniform(-3, 6, K))
    args = (_dev(y_tk), rconst, *_params_dev(arrs), _dev(s[:, None]))
    nll, g = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
    ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s,
                               rconst.cpu().numpy(), want_grad=True)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 3e-6
    assert (np.abs(g - gref) / np.maximum(np.abs(gref), 1e-3 * np.abs(ref))).max() < 3e-5
    set_knob('EKS_NLL_GRAD_TREE', '1')
    nll3, g3 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
    assert (np.abs(nll3 - ref) / np.abs(ref)).max() < 3e-6
    assert not np.array_equal(nll, nll3)


def test_nll_grad_single_launch_is_bit_reproducible():
    """The tile's last block - whichever block that is in a given launch - reads the group summaries the other
    blocks (on other XCDs) published without an L2 write-back (agent-scope atomic stores, see gf_publish): the
    composition order is fixed, so every evaluation of the same problem must return the same bits.  A summary
    read before it was visible would show up here."""
    from eks_amd import _lib, hip_ops, synth
    T, K = 60_000, 128
    y, var = synth.singlecam_observations_torch(T, K, seed=9, device=torch.device('cuda', 0))
    eye = torch.eye(2, dtype=torch.float64, device=y.device).expand(K, 2, 2).contiguous()
    m0 = torch.zeros(K, 2, dtype=torch.float64, device=y.device)
    rconst = hip_ops.const_r(var)
    s = torch.exp(torch.linspace(-5, 5, K, dtype=torch.float64, device=y.device))[:, None].contiguous()
    flags = _lib.FLAG_DIAG_MODEL | _lib.FLAG_UNIT_AC
    first = hip_ops.nll(y, rconst, m0, eye * 4.0, eye, eye, eye, s, per_keypoint=True, want_grad=True, flags=flags)
    first = [a.clone() for a in first]
    assert bool(torch.isfinite(first[0]).all()) and bool(torch.isfinite(first[1]).all())
    for _ in range(200):
        out = hip_ops.nll(y, rconst, m0, eye * 4.0, eye, eye, eye, s, per_keypoint=True, want_grad=True, flags=flags)
        assert torch.equal(out[0], first[0]) and torch.equal(out[1], first[1])


@pytest.mark.parametrize('T,K,D,O', [(800, 3, 3, 4), (300, 2, 4, 8), (200, 2, 2, 2)])
def test_nll_dense_matches_oracle(T, K, D, O):
    from eks_amd import hip_ops
    arrs, y, var = _dense_problem(T, K, D, O, seed=11 + T)
    rconst = hip_ops.const_r(_dev(var), 1e-4)
    Rc = rconst.cpu().numpy()
    cand = np.exp(np.linspace(-8, 8, 9))
    nll = hip_ops.nll(_dev(y), rconst, *_params_dev(arrs), _dev(cand), flags=0).cpu().numpy()
    ref = np.stack([orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                                   arrs['Qs'], np.full(K, sc), Rc) for sc in cand], axis=1)
    assert (np.abs(nll - ref) / np.abs(ref)).max() < 1e-8          # float64 path
    s = np.exp(np.random.default_rng(0).uniform(-4, 4, K))
    nll1, g1 = hip_ops.nll(_dev(y), rconst, *_params_dev(arrs), _dev(s[:, None]), per_keypoint=True,
                           want_grad=True, flags=0)
    ref1, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'],
                                arrs['Qs'], s, Rc, want_grad=True)
    assert (np.abs(nll1.cpu().numpy()[:, 0] - ref1) / np.abs(ref1)).max() < 1e-8
    assert (np.abs(g1.cpu().numpy()[:, 0] - gref) / np.abs(gref).max()).max() < 1e-7


@pytest.mark.parametrize('T,K,D,O,general_A', [(800, 3, 3, 4, False), (1500, 5, 3, 4, True), (131, 2, 2, 2, False),
                                               (9, 2, 3, 8, False), (2, 3, 2, 6, False), (20000, 4, 3, 4, False),
                                               # wide sessions: the keypoint-major kernels' SCORE form
                                               (600, 1500, 3, 4, False), (1100, 700, 2, 6, True), (70, 1100, 3, 8, True),
                                               (3, 1300, 2, 2, False),
                                               (700, 3, 3, 12, False), (300, 2, 3, 10, True),    # five / six cameras
                                               # no specialised kernels: the generic ones in their SCORE form
                                               (600, 3, 4, 8, False), (257, 2, 5, 8, True), (100, 2, 6, 8, False),
                                               (400, 3, 3, 5, False), (64, 2, 1, 3, False), (900, 40, 4, 6, True)])
def test_nll_dense_score_gradient_matches_oracle_and_dual_numbers(T, K, D, O, general_A):
    """EKS_FLAG_Q_PD: value from the exact filter inside the smoother's kernels, gradient from the smoothing
    distribution (Fisher's identity; SCORE forms of eks_dense_wave.hip and eks_dense_wide.hip) - against the oracle's forward-mode gradient
    at the bars of the dual-number kernels, and against those kernels themselves (flags without Q_PD)."""
    from eks_amd import _lib, hip_ops
    arrs, y, var = _dense_problem(T, K, D, O, seed=17 + T)
    if general_A:
        arrs['As'] = arrs['As'] * 0.97 + 0.02 * np.random.default_rng(9).standard_normal((K, D, D))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    assert flags == _lib.FLAG_Q_PD
    rconst = hip_ops.const_r(_dev(var), 1e-4)
    s = np.exp(np.random.default_rng(T).uniform(-4, 4, K))
    args = (_dev(y), rconst, *_params_dev(arrs), _dev(s[:, None]))
    nll1, g1 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
    nll0, g0 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=0)]
    ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s,
                               rconst.cpu().numpy(), want_grad=True)
    assert (np.abs(nll1 - ref) / np.abs(ref)).max() < 1e-8
    assert (np.abs(g1 - gref) / np.abs(gref).max()).max() < 1e-7
    assert (np.abs(nll1 - nll0) / np.abs(ref)).max() < 1e-10
    assert (np.abs(g1 - g0) / np.abs(gref).max()).max() < 1e-7


@pytest.mark.parametrize('knob', ['EKS_DENSE_LEGACY', 'EKS_DENSE_TREE_SCAN'])
@pytest.mark.parametrize('T,K', [(900, 4), (300, 1200)])
def test_nll_dense_score_generic_kernels_on_specialised_shapes(T, K, knob, set_knob):
    """D = 3, O = 4 through the GENERIC kernels' SCORE form (the specialised narrow / keypoint-major kernels switched
    off, or the keypoint-major ones with the tree scan): the same value and gradient as the specialised forms."""
    from eks_amd import _lib, hip_ops
    arrs, y, var = _dense_problem(T, K, 3, 4, seed=23 + T)
    rconst = hip_ops.const_r(_dev(var), 1e-4)
    s = np.exp(np.random.default_rng(T).uniform(-4, 4, K))
    args = (_dev(y), rconst, *_params_dev(arrs), _dev(s[:, None]))
    n0, g0 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=_lib.FLAG_Q_PD)]
    set_knob(knob, '1')
    n1, g1 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=_lib.FLAG_Q_PD)]
    assert (np.abs(n1 - n0) / np.abs(n0)).max() < 1e-11
    assert (np.abs(g1 - g0) / np.abs(g0).max()).max() < 1e-9


def test_adam_step_matches_oracle_sequence():
    """Drive eks_adam_step with a synthetic quadratic loss and compare the whole trajectory with
    the oracle's restatement of eks/core.py:652-681 (including blocks and the clip gradient)."""
    from eks_amd import hip_ops
    blocks = [[0, 2], [1], [3]]
    u0 = np.array([2.5, -9.0, 0.3])           # block 1 starts outside the [-8, 8] bounds
    centers = np.array([1.0, -2.0, 0.5, 1.5])  # per keypoint

    def per_kp(u_kp):
        return 50.0 + (u_kp - centers) ** 2, 2.0 * (u_kp - centers)

    member_block = np.array([0, 1, 0, 2])

    def lg(u_b):
        L, g = per_kp(u_b[member_block])
        Lb = np.zeros(3)
        gb = np.zeros(3)
        np.add.at(Lb, member_block, L)
        np.add.at(gb, member_block, g)
        return Lb, gb

    u_ref, last_ref, it_ref = orc.adam_optimize_s(lg, u0, tol=1e-3, safety_cap=40)
    offs = _dev(np.array([0, 2, 3, 4], np.int32))
    mem = _dev(np.array([0, 2, 1, 3], np.int32))
    state = np.zeros((3, 6))
    state[:, 0] = u0
    state[:, 3] = np.inf
    state = _dev(state)
    s_kp = torch.empty(4, dtype=torch.float64, device='cuda')
    n_act = torch.zeros(1, dtype=torch.int32, device='cuda')
    u_now = u0.copy()
    for it in range(60):
        L, g = per_kp(np.clip(u_now, -8, 8)[member_block])
        hip_ops.adam_step(offs, mem, _dev(L), _dev(g), state, s_kp, n_act, 0.25, -8.0, 8.0, 1e-3, 40)
        u_now = state.cpu().numpy()[:, 0]
        if int(n_act.item()) == 0:
            break
    st = state.cpu().numpy()
    np.testing.assert_allclose(st[:, 0], u_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(st[:, 4].astype(int), it_ref)
    np.testing.assert_allclose(st[:, 3], last_ref, rtol=1e-12)
    np.testing.assert_allclose(s_kp.cpu().numpy(), np.exp(np.clip(u_ref, -8, 8))[member_block], rtol=1e-12)


@pytest.mark.parametrize('nb', [300, 5000])
def test_adam_step_both_launch_forms_count_running_blocks(nb):
    """eks_adam_step walks up to 4096 optimiser blocks with ONE workgroup that writes the number still
    running itself, and uses a grid with an atomic counter beyond that: both against the oracle's
    trajectory on singleton blocks with a quadratic loss, and n_active against the count of blocks that
    have neither stopped nor reached the cap after every step."""
    from eks_amd import hip_ops
    rng = np.random.default_rng(nb)
    centers = rng.uniform(-3, 3, nb)
    u0 = rng.uniform(-6, 6, nb)
    cap = 25

    def lg(u):
        return 50.0 + (u - centers) ** 2, 2.0 * (u - centers)

    u_ref, last_ref, it_ref = orc.adam_optimize_s(lg, u0, tol=1e-3, safety_cap=cap)
    offs = _dev(np.arange(nb + 1, dtype=np.int32))
    mem = _dev(np.arange(nb, dtype=np.int32))
    state = np.zeros((nb, 6))
    state[:, 0] = u0
    state[:, 3] = np.inf
    state = _dev(state)
    s_kp = torch.empty(nb, dtype=torch.float64, device='cuda')
    n_act = torch.full((1,), -7, dtype=torch.int32, device='cuda')     # garbage: the launch must overwrite it
    for it in range(cap + 3):
        u_now = state[:, 0].cpu().numpy()
        L, g = lg(np.clip(u_now, -8, 8))
        hip_ops.adam_step(offs, mem, _dev(L), _dev(g), state, s_kp, n_act, 0.25, -8.0, 8.0, 1e-3, cap)
        st = state.cpu().numpy()
        assert int(n_act.item()) == int(((st[:, 5] == 0) & (st[:, 4] < cap)).sum())
        if int(n_act.item()) == 0:
            break
    np.testing.assert_allclose(st[:, 0], u_ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(st[:, 4].astype(int), it_ref)


@pytest.mark.parametrize('M,avg,varm', [(5, 'median', 'confidence_weighted_var'), (4, 'mean', 'var'),
                                        (1, 'median', 'confidence_weighted_var'), (9, 'median', 'var'),
                                        (2, 'median', 'confidence_weighted_var')])
def test_ensemble_matches_oracle(M, avg, varm):
    from eks_amd import hip_ops
    rng = np.random.default_rng(M)
    a = rng.random((M, 2, 40, 5, 3)).astype(np.float32)
    a[..., :2] *= 300
    if M > 1:
        a[0, 0, 3, 1, 0] = np.nan            # one member missing
        a[:, 1, 5, 2, 1] = np.nan            # all members missing -> var replaced by 1000
        a[:, 0, 7, 0, 2] = 0.0               # zero confidence -> inf -> float32 max
    got = hip_ops.ensemble(_dev(a), avg, varm).cpu().numpy().astype(np.float64)
    ref = orc.ensemble(a, avg, varm)[0]
    both_nan = np.isnan(got) & np.isnan(ref)
    np.testing.assert_allclose(np.where(both_nan, 0, got), np.where(both_nan, 0, ref), rtol=2e-6)
    if M > 1:
        assert got[1, 5, 2, 3] == 1000.0 and np.isnan(got[1, 5, 2, 1])


def test_abi_error_codes():
    import ctypes
    from eks_amd import _lib
    lib = _lib.load()
    d = _lib.EksDims(4, 0, 2, 2, 1)
    assert lib.eks_smooth_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.eks_smooth(ctypes.byref(d), *([None] * 11), 0, None) == -2       # bad shape
    d = _lib.EksDims(4, 10, 2, 2, 1)
    assert lib.eks_smooth(ctypes.byref(d), *([None] * 11), 0, None) == -1       # null pointers
    d = _lib.EksDims(4, 10, 2, 3, 1)
    assert lib.eks_smooth_workspace_bytes(ctypes.byref(d)) == 0                 # DIAG needs D == O
    d = _lib.EksDims(2, 10, 7, 7, 0)
    x = torch.zeros(10 * 2 * 7 * 7, dtype=torch.float64, device='cuda')
    xf = torch.zeros(10 * 2 * 7 * 7, dtype=torch.float32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.eks_smooth(ctypes.byref(d), p(xf), p(xf), p(x), p(x), p(x), p(x), p(x), p(x), p(xf), p(xf),
                        p(x), x.numel() * 8, None)
    assert rc == -3                                                             # D = 7 not built
    assert b'unsupported' in lib.eks_status_string(rc)


@pytest.mark.parametrize('T,N', [(1, 3), (2, 1), (257, 5), (5000, 8), (50_000, 4), (4097, 70)])
def test_order_stats_and_percentile_match_numpy_bit_for_bit(T, N):
    """eks_order_stats (exact selection, NaNs last) against numpy.sort, and hip_ops.percentile against
    numpy.percentile(x, q, axis=0) - the thresholds of center_predictions and of the variance-inflation loop
    (reference eks/utils.py:318-322, eks/stats.py:109-112): float32 in, float32 out, the same bits; columns
    with NaNs, infinities, negative values, zeros of both signs and heavy duplicates."""
    from eks_amd import hip_ops
    rng = np.random.default_rng(T * 31 + N)
    x = (rng.gamma(2.0, 1.0, (T, N)) * 10.0 ** rng.integers(-6, 4, (1, N))).astype(np.float32)
    if N > 1:
        x[:, 1] = np.round(x[:, 1] / x[:, 1].max() * 3)                  # four distinct values
    if N > 2:
        x[:, 2] = rng.standard_normal(T).astype(np.float32)             # negative values
        x[::3, 2] = 0.0
        x[1::7, 2] = -0.0
    if N > 3 and T > 4:
        x[rng.integers(0, T, 3), 3] = np.inf
    if N > 4:
        x[rng.integers(0, T, 2), 4] = np.nan
    xd = _dev(x, torch.float32)
    srt = np.sort(x, axis=0)
    for r in sorted({0, T // 2, (T - 1) // 2, max(T - 2, 0), T - 1}):
        r_hi = min(r + 1, T - 1)
        vals, nans = hip_ops.order_stats(xd, r, r_hi)
        np.testing.assert_array_equal(nans.cpu().numpy(), np.isnan(x).sum(axis=0))
        got = vals.cpu().numpy()
        want = np.stack([srt[r], srt[r_hi]], axis=1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) or \
            np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want)) or \
            np.array_equal(np.where(got == 0, 0.0, got), np.where(want == 0, 0.0, want), equal_nan=True)
    for q in (0.0, 12.5, 50.0, 95.0, 99.99, 100.0):
        got = hip_ops.percentile(xd, q)
        ref = np.percentile(x, q, axis=0)
        assert got.dtype == ref.dtype and np.array_equal(got, ref, equal_nan=True), (q, got, ref)


@pytest.mark.parametrize('dense', [False, True])
def test_smooth_with_infinite_and_huge_variances_gives_those_frames_no_weight(dense):
    """an infinite ensemble variance (a frame no member could place) used to poison the chain - the
    fast reciprocals return NaN at inf, and r g = inf * 0 is NaN in every form of the update, the reference's
    included.  Variances are clamped to 1e30 at load (eks_diag_lane.hpp: clip_var): such a frame gets zero weight.
    Compared with the float64 oracle fed 1e30 in those places; every output must be finite."""
    from eks_amd import hip_ops
    if dense:
        T, K, D, O = 1200, 3, 3, 4
        arrs, y_tk, var_tk = _dense_problem(T, K, D, O, seed=5)
    else:
        T, K = 2500, 5
        arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=93, unit=True)
    var_tk = var_tk.copy()
    var_tk[5::37, 0, :] = np.inf                     # whole frames of one keypoint
    var_tk[11::53, 1, 0] = np.inf                    # single coordinates
    var_tk[700:740, 2] = 3e38                        # a run of frames beyond the clamp, finite
    var_tk[0, 0] = np.inf                            # the very first frame: the prior passes through
    var_tk[T - 1, 1] = np.inf                        # and the last
    s = np.full(K, 3.0)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    ms, Vs = hip_ops.smooth(_dev(y_tk), _dev(var_tk), *_params_dev(arrs), _dev(s), flags=flags)
    ms = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vs = np.transpose(Vs.cpu().numpy().astype(np.float64), (1, 0, 2, 3))
    assert np.isfinite(ms).all() and np.isfinite(Vs).all()
    Rd = np.clip(np.swapaxes(var_tk.astype(np.float64), 0, 1), 1e-12, 1e30)
    ms_o, Vs_o = orc.kalman_smoother(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], s, Rd)[:2]
    assert _rel(ms, ms_o, axis_scale=(1, 2)) < 1e-5
    assert (np.abs(Vs - Vs_o) / np.abs(Vs_o).max(axis=(2, 3), keepdims=True)).max() < 1e-5


def test_score_gradient_at_the_conditioning_threshold():
    """hip_ops.model_flags asserts EKS_FLAG_Q_PD up to cond(Q) = 1e6.  At that conditioning and
    T = 50 000 the smoothing-distribution gradient - tr((sQ)^-1 E[w w']) - D summed over the frames - must still
    agree with the dual-number kernels (which never invert Q) well inside what moves Adam's stop test."""
    from eks_amd import _lib, hip_ops
    T, K, D, O = 50_000, 4, 3, 4
    arrs, y, var = _dense_problem(T, K, D, O, seed=123)
    rng = np.random.default_rng(7)
    U = np.linalg.qr(rng.standard_normal((K, D, D)))[0]
    lam = np.array([1.0, 3e-3, 1.2e-6])              # cond 8e5: just inside the threshold
    arrs['Qs'] = np.ascontiguousarray(U @ (lam[None, :, None] * np.swapaxes(U, 1, 2)))
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    assert flags == _lib.FLAG_Q_PD
    rconst = hip_ops.const_r(_dev(var), 1e-4)
    for u in (-6.0, 0.0, 5.0):
        s = np.full(K, np.exp(u))
        args = (_dev(y), rconst, *_params_dev(arrs), _dev(s[:, None]))
        nll1, g1 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=flags)]
        nll0, g0 = [a.cpu().numpy()[:, 0] for a in hip_ops.nll(*args, per_keypoint=True, want_grad=True, flags=0)]
        assert (np.abs(nll1 - nll0) / np.abs(nll0)).max() < 1e-9
        # the optimiser sees lr * g through Adam's normalisation; a relative 1e-5 of the gradient's own size (or of
        # 1e-6 of the loss where the gradient vanishes) cannot move a step or the stop test
        assert (np.abs(g1 - g0) / np.maximum(np.abs(g0), 1e-6 * np.abs(nll0))).max() < 1e-5, (u, g1, g0)


def test_prepared_smooth_is_the_same_call_and_follows_changed_contents():
    """hip_ops.PreparedSmooth (arguments checked and packed once, for callers that smooth small sessions in a loop)
    enqueues exactly eks_smooth: bit-identical to hip_ops.smooth, and a second call after new smoothing parameters
    were written INTO the prepared `s` tensor gives what a fresh call with them gives."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(3000, 9, seed=77)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, var = _dev(y_tk), _dev(var_tk)
    params = _params_dev(arrs)
    s = _dev(np.full(9, 3.0))
    call = hip_ops.PreparedSmooth(y, var, *params, s, flags=flags)
    ms1, Vs1 = (t.clone() for t in call())
    ref = hip_ops.smooth(y, var, *params, s, flags=flags)
    assert torch.equal(ms1, ref[0]) and torch.equal(Vs1, ref[1])
    s.copy_(_dev(np.linspace(0.1, 40.0, 9)))
    ms2, Vs2 = call()
    ref2 = hip_ops.smooth(y, var, *params, s.clone(), flags=flags)
    assert torch.equal(ms2, ref2[0]) and torch.equal(Vs2, ref2[1])
    assert not torch.equal(ms2, ms1)


@pytest.mark.parametrize('K,n', [(5, 1), (3, 7), (4, 130), (256, 3998), (40, 7996), (2, 8192)])
def test_np_nanstd_rows_is_numpys_value_bit_for_bit(K, n):
    """eks_np_nanstd_rows against numpy.nanstd(x, axis=1) on float32 rows with NaNs, an all-NaN row, a constant row
    and values over four decades: identical bits (the optimiser's initial guess is this number rounded to five
    decimals and cast to float32, reference eks/core.py:104-133, :612-613)."""
    import warnings
    from eks_amd import hip_ops
    rng = np.random.default_rng(K * 100003 + n)
    x = (rng.standard_normal((K, n)) * np.exp(rng.uniform(-4, 5, (K, 1)))).astype(np.float32)
    x[rng.random((K, n)) < 0.03] = np.nan
    if K > 3:
        x[1] = np.nan
        x[2] = 0.75
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = np.nanstd(x, axis=1)
    got = hip_ops.np_nanstd_rows(_dev(x)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, ref, equal_nan=True)


@pytest.mark.parametrize('Tn,K,O', [(2000, 64, 2), (2, 5, 2), (777, 33, 3), (2000, 7, 4)])
def test_np_nanstd_diff_rows_is_numpys_value_of_the_frame_differences(Tn, K, O):
    """eks_np_nanstd_diff_rows - compute_initial_guesses' reduction (reference eks/core.py:128-130) with the frame-to-frame
    differences formed inside the launch from the frame-major (T', K, O) tensor - against numpy.nanstd of
    ev[1:, k] - ev[:-1, k] per keypoint: identical bits, NaN frames and an all-NaN keypoint included, on the first call
    (which goes through the row-matrix form and checks the summation order) and on the second (the fused launch)."""
    import warnings
    from eks_amd import hip_ops
    rng = np.random.default_rng(Tn * 31 + K)
    ev = (rng.gamma(2.0, 0.25, (Tn, K, O)) * np.exp(rng.uniform(-3, 4, (1, K, 1)))).astype(np.float32)
    ev[rng.random((Tn, K, O)) < 0.02] = np.nan
    if K > 3:
        ev[:, 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = np.array([np.nanstd(ev[1:, k] - ev[:-1, k]) for k in range(K)], dtype=np.float32)
    x = _dev(ev)
    for _ in range(2):
        got = hip_ops.np_nanstd_diff_rows(x).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, ref, equal_nan=True)


def test_np_nanstd_rows_declines_rows_numpy_would_reduce_in_buffered_pieces():
    from eks_amd import hip_ops
    assert hip_ops.np_nanstd_rows(_dev(np.ones((2, 8193), np.float32))) is None


def test_initial_guesses_reduced_on_the_device_equal_the_host_reduction():
    """core._guess_std_on_device + _initial_guesses_per_keypoint(sd=...) - what run_kalman_smoother uses for device
    tensors - against the host form on the same float32 variances (NaNs, an all-NaN keypoint, a constant one)."""
    from eks_amd import core
    rng = np.random.default_rng(5)
    ev = rng.gamma(2, 1, (2500, 70, 2)).astype(np.float32)
    ev[rng.random(ev.shape) < 0.02] = np.nan
    ev[:, 2, :] = np.nan
    ev[:, 3, :] = 1.0
    sd = core._guess_std_on_device(_dev(ev))
    assert sd is not None
    assert np.array_equal(core._initial_guesses_per_keypoint(sd=sd), core._initial_guesses_per_keypoint(ev))


def _adam_search(y, rc, params, flags, K, u0, cap=300, stride=None, tol=1e-2, prepare=False, lo=-8.0, hi=8.0):
    """One search through hip_ops.AdamLoop in calls of `stride` iterations (None: what the library asks for).  Returns the
    library's stride, state, s, last loss / gradient and the running count after every call."""
    from eks_amd import hip_ops
    offs = torch.arange(K + 1, dtype=torch.int32, device='cuda')
    mem = torch.arange(K, dtype=torch.int32, device='cuda')
    state = np.zeros((K, 6))
    state[:, 0] = u0
    state[:, 3] = np.inf
    state = _dev(state)
    s_kp = _dev(np.exp(np.clip(u0, lo, hi)))
    loop = hip_ops.AdamLoop(y, rc, *params, offs, mem, state, s_kp, 0.25, lo, hi, tol, cap, flags=flags)
    if prepare:
        assert loop.prepare()
    n = stride or loop.stride()
    left, it = [], 0
    while it < cap:
        loop.run(min(n, cap - it))
        it += n
        left.append(int(loop.n_active.item()))
        assert left[-1] >= 0
        if left[-1] == 0:
            break
    return loop.stride(), state.cpu().numpy(), s_kp.cpu().numpy(), loop.nll.cpu().numpy(), loop.dnll.cpu().numpy(), left


def _oracle_adam(arrs, y_tk, rc, ks, u0, cap=300, tol=1e-2, lo=-8.0, hi=8.0):
    """oracle/eks_oracle.py: adam_optimize_s fed by the C port's complex-step gradient, keypoints `ks`."""
    from oracle import c_oracle
    D = arrs['As'].shape[-1]
    ys = np.transpose(y_tk, (1, 0, 2)).astype(np.float64)
    Rc = rc.cpu().numpy()
    zero = np.zeros((1, D, D))

    def loss_and_grad(u):
        out = []
        for j, k in enumerate(ks):
            sQ = np.exp(u[j]) * arrs['Qs'][k]
            L, g = c_oracle.nll_directional(ys[k], Rc[k], arrs['m0s'][k], arrs['S0s'][k], arrs['As'][k], arrs['Cs'][k],
                                            sQ, zero, sQ[None])
            out.append((L, g[0]))
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])

    u_o, last_o, it_o = orc.adam_optimize_s(loss_and_grad, u0[ks], tol=tol, safety_cap=cap, s_bounds_log=(lo, hi))
    return np.clip(u_o, lo, hi), last_o, it_o


@pytest.mark.parametrize('T,K,unit,stride,cap', [(30_000, 70, True, 24, 300), (20_011, 33, False, 7, 300),
                                                 (50_000, 128, True, None, 300), (1_024, 3, True, None, 300),
                                                 (4_500, 40, False, 9, 300), (30_000, 70, True, 5, 13),
                                                 (3_000, 600, True, None, 300)])
def test_adam_from_cached_lag_sums_is_the_streaming_search_and_the_oracles(T, K, unit, stride, cap, set_knob):
    """Round 6 (eks_lag_adam.hip): one keypoint per optimiser block and at least 1 024 frames - eks_adam_run makes ONE
    pass over y (256 lag sums of the inputs u_t = y_t - a y_{t-1} per chain, which do not depend on s) and then runs all
    of a call's iterations in one launch, a workgroup per keypoint, evaluating loss and d / d log s from those sums and
    the first / last 257 rows.  Against the kernels that read y every iteration (EKS_ADAM_STREAM=1) on the same problem:
    the same stopping iteration for every keypoint, the same count of running keypoints after every call - also when
    calls end mid-search (stride 7 / 24), with a partial last tile and when the safety cap ends the search (cap 13) - and
    log s within 2e-6 (the lag sums are sums of float32 products: 1e-8 of noise in the loss).  Against the oracle's
    optimiser on the C port's complex-step gradient (three keypoints): the same stopping iteration, log s within 2e-6,
    the last loss within 1e-7."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=31 + T, unit=unit)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, rc = _dev(y_tk), hip_ops.const_r(_dev(var_tk), 1e-4)
    params = _params_dev(arrs)
    u0 = np.log(np.random.default_rng(T).uniform(0.05, 50.0, K))
    n_l, st_l, s_l, nll_l, g_l, left_l = _adam_search(y, rc, params, flags, K, u0, cap, stride)
    assert n_l == 4096                       # (the lag-sum search is what ran: the whole search in one call)
    if K >= 256:
        # (the wide session: 19 tiles x 14 chunks.  Its reference is the in-kernel float64 evaluation of every frame -
        #  EKS_ADAM_LAG_RHO_PPM=0 - which the lag form follows to 1e-6 with the same stopping iteration on 600 of 600
        #  keypoints; round 5's streaming kernels are the noisier of the two there: 2e-5, one keypoint 30 iterations off)
        set_knob('EKS_ADAM_LAG_RHO_PPM', '0')
        n_s, st_s, s_s, nll_s, g_s, left_s = _adam_search(y, rc, params, flags, K, u0, cap, stride)
        assert n_s == 4096
    else:
        set_knob('EKS_ADAM_STREAM', '1')
        n_s, st_s, s_s, nll_s, g_s, left_s = _adam_search(y, rc, params, flags, K, u0, cap, stride or 16)
        assert n_s in (16, 64)
    if cap == 300:
        assert st_l[:, 4].max() > 20 and np.all(st_l[:, 5] == 1.0)
    else:
        assert np.all(st_l[:, 4] == cap) and np.all(st_l[:, 5] == 0.0) and left_l[-1] == 0
    np.testing.assert_array_equal(st_l[:, 4:], st_s[:, 4:])                  # iterations taken, stopped by the rule
    if stride:
        assert left_l == left_s                                              # keypoints still running after every call
    assert np.abs(np.log(s_l) - np.log(s_s)).max() < 2e-6
    assert np.abs(nll_l / nll_s - 1).max() < 1e-7
    assert np.abs(g_l - g_s).max() <= 2e-5 * np.abs(g_s).max() + 1e-3
    if cap == 300 and T <= 30_000:
        ks = list(range(min(K, 3)))
        u_o, last_o, it_o = _oracle_adam(arrs, y_tk, rc, ks, u0, cap)
        np.testing.assert_array_equal(st_l[ks, 4].astype(int), it_o)
        assert np.abs(np.log(s_l[ks]) - u_o).max() < 2e-6
        assert np.abs(st_l[ks, 3] / last_o - 1).max() < 1e-7


@pytest.mark.parametrize('T,K,unit', [(12_000, 48, True), (6_011, 21, False)])
def test_adam_from_lag_sums_head_length_follows_the_pole(T, K, unit, set_knob):
    """The frames evaluated one by one from the prior (the head) are 64, 128 or 256 per evaluation, as many as the
    variance's transient w_0 kappa^t needs to die; the lag sums of the region behind a shorter head are the cached
    ones plus the products of the frames in between (formed once per search in LDS).  With the head forced to 256
    frames for every evaluation (EKS_ADAM_LAG_HEAD=256: round 6's first form) the searches stop at the same iteration and
    end within 1e-9 in log s; forcing 128 is as good on these poles; both within 1e-6 of the in-kernel float64
    fallback that streams every frame (EKS_ADAM_LAG_RHO_PPM=0)."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=5 + T, unit=unit)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, rc = _dev(y_tk), hip_ops.const_r(_dev(var_tk), 1e-4)
    params = _params_dev(arrs)
    u0 = np.log(np.random.default_rng(T).uniform(0.05, 50.0, K))
    _, st_a, s_a, nll_a, g_a, _ = _adam_search(y, rc, params, flags, K, u0)
    set_knob('EKS_ADAM_LAG_HEAD', '256')
    _, st_f, s_f, nll_f, g_f, _ = _adam_search(y, rc, params, flags, K, u0)
    set_knob('EKS_ADAM_LAG_HEAD', '128')
    _, st_h, s_h, _, _, _ = _adam_search(y, rc, params, flags, K, u0)
    set_knob('EKS_ADAM_LAG_HEAD', None)
    set_knob('EKS_ADAM_LAG_RHO_PPM', '0')
    _, st_x, s_x, _, _, _ = _adam_search(y, rc, params, flags, K, u0)
    assert np.all(st_a[:, 5] == 1.0) and st_a[:, 4].max() > 20
    np.testing.assert_array_equal(st_a[:, 4:], st_f[:, 4:])
    np.testing.assert_array_equal(st_a[:, 4:], st_x[:, 4:])
    assert np.abs(np.log(s_a) - np.log(s_f)).max() < 1e-9
    assert np.abs(nll_a / nll_f - 1).max() < 1e-12
    assert np.abs(g_a - g_f).max() <= 1e-9 * np.abs(g_f).max() + 1e-9
    assert np.abs(np.log(s_a) - np.log(s_x)).max() < 1e-6
    # (a 128-frame head everywhere is NOT exact for the slowest poles these searches visit: it only has to stay close)
    assert np.abs(np.log(s_h) - np.log(s_x)).max() < 1e-4 and np.abs(st_h[:, 4] - st_x[:, 4]).max() <= 1


@pytest.mark.parametrize('T,K,unit,ppm', [(20_000, 40, True, 0), (9_000, 33, False, 0), (20_000, 40, True, 450_000),
                                         (3_000, 5, False, 300_000)])
def test_adam_chains_outside_the_lag_range_stream_their_own_frames_exactly(T, K, unit, ppm, set_knob):
    """A chain whose pole leaves the range the 256 lag sums cover (|rho| > 0.906) is evaluated by its own wave from a
    private chain-major copy of its frames - closed-form variances, lane = time chunk, the same 64-lane scan - in float64
    throughout.  EKS_ADAM_LAG_RHO_PPM moves that bound: 0 streams every evaluation, 450 000 / 300 000 switch between the
    two forms in the middle of most searches (poles of these problems run from 0.05 to 0.8).  Against the oracle's
    optimiser: the same stopping iteration and log s within 1e-6 whatever the mixture (all-streamed: within 1e-9 - that
    form rounds nothing to float32)."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=77 + T, unit=unit)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, rc = _dev(y_tk), hip_ops.const_r(_dev(var_tk), 1e-4)
    params = _params_dev(arrs)
    u0 = np.log(np.random.default_rng(T).uniform(0.05, 50.0, K))
    set_knob('EKS_ADAM_LAG_RHO_PPM', str(ppm))
    n_f, st_f, s_f, nll_f, g_f, _ = _adam_search(y, rc, params, flags, K, u0)
    assert n_f == 4096 and np.all(st_f[:, 5] == 1.0)
    ks = list(range(min(K, 4)))
    u_o, last_o, it_o = _oracle_adam(arrs, y_tk, rc, ks, u0)
    np.testing.assert_array_equal(st_f[ks, 4].astype(int), it_o)
    assert np.abs(np.log(s_f[ks]) - u_o).max() < (1e-9 if ppm == 0 else 1e-6)
    assert np.abs(st_f[ks, 3] / last_o - 1).max() < (1e-11 if ppm == 0 else 1e-7)
    set_knob('EKS_ADAM_LAG_RHO_PPM', None)
    _, st_l, s_l, _, _, _ = _adam_search(y, rc, params, flags, K, u0)
    np.testing.assert_array_equal(st_l[:, 4:], st_f[:, 4:])
    assert np.abs(np.log(s_l) - np.log(s_f)).max() < 2e-6


def _diag_problem(T, K, D, seed, slow=False):
    """A diagonal model with D chains per keypoint (a, c, q per chain) on random-walk data; `slow`: little process noise
    under a lot of observation noise - the optimum's pole sits above 0.93, outside the lag sums' range."""
    rng = np.random.default_rng(seed)
    q_true = (1e-3 if slow else 1.0) * np.exp(rng.uniform(-1.0, 1.0, (K, D)))
    lat = np.cumsum(rng.standard_normal((T, K, D)) * np.sqrt(q_true), axis=0) + rng.uniform(50, 400, (1, K, D))
    var_tk = ((2.0 if slow else 0.3) * rng.gamma(2.0, 1.0, (T, K, D)) + 0.02).astype(np.float32)
    y_tk = (lat + rng.standard_normal((T, K, D)) * np.sqrt(var_tk)).astype(np.float32)
    eye = np.tile(np.eye(D), (K, 1, 1))
    a = rng.uniform(0.97, 1.0, (K, D)) if not slow else np.ones((K, D))
    arrs = dict(m0s=y_tk[0].astype(np.float64) + rng.standard_normal((K, D)), S0s=eye * rng.uniform(5.0, 400.0, (K, D))[:, :, None],
                As=eye * a[:, :, None], Cs=eye * (rng.uniform(0.7, 1.3, (K, D)) if not slow else np.ones((K, D)))[:, :, None],
                Qs=eye * rng.uniform(0.5, 2.0, (K, D))[:, :, None])
    return arrs, y_tk, var_tk


@pytest.mark.parametrize('T,K,D,slow', [(6_000, 9, 1, False), (5_000, 7, 3, False), (4_096, 5, 4, False),
                                       (12_000, 6, 2, True), (1_025, 2, 2, False)])
def test_adam_from_lag_sums_other_chain_counts_and_slow_poles(T, K, D, slow):
    """One to four chains per keypoint (a wave each), general diagonal (a, c, q), and a problem whose optimum has a pole
    above 0.93 - there the search streams by itself for most of its iterations.  Against the oracle's optimiser on every
    keypoint: the same stopping iteration, log s within 2e-6."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _diag_problem(T, K, D, seed=5 * T + D, slow=slow)
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, rc = _dev(y_tk), hip_ops.const_r(_dev(var_tk), 1e-4)
    params = _params_dev(arrs)
    u0 = np.log(np.random.default_rng(T).uniform(0.05, 20.0, K)) - (5.0 if slow else 0.0)
    n_l, st_l, s_l, _, _, _ = _adam_search(y, rc, params, flags, K, u0)
    assert n_l == 4096 and np.all(st_l[:, 5] == 1.0)
    ks = list(range(K))
    u_o, last_o, it_o = _oracle_adam(arrs, y_tk, rc, ks, u0)
    np.testing.assert_array_equal(st_l[:, 4].astype(int), it_o)
    assert np.abs(np.log(s_l) - u_o).max() < 2e-6
    if slow:
        a, r = 1.0, rc.cpu().numpy()
        sq = s_l[:, None] * np.diagonal(arrs['Qs'], axis1=1, axis2=2)
        Pinf = (sq + np.sqrt(sq * sq + 4 * sq * r)) / 2
        assert (r / (r + Pinf)).min() > 0.92            # (the poles at the optimum: the lag form never applied there)


def test_adam_from_lag_sums_nan_keypoint_bounds_and_prepared_pass(set_knob):
    """(a) A keypoint with a NaN observation has a non-finite loss: 1e12 with zero gradient (eks/core.py:650) - it stops
    at its second iteration, the others are untouched, exactly as with the streaming kernels.  (b) Starting points outside
    [lo, hi] get a zero gradient (jnp.clip) until the bias-corrected momentum is all there is: same iterations as the
    streaming form.  (c) eks_adam_prepare ahead of the state's upload + EKS_FLAG_ADAM_PREPARED: bit for bit the
    unprepared call."""
    from eks_amd import hip_ops
    T, K = 8_000, 12
    arrs, y_tk, var_tk = _singlecam_problem(T, K, seed=4321, unit=True)
    y_bad = y_tk.copy()
    y_bad[5000, 3, 1] = np.nan
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    rc = hip_ops.const_r(_dev(var_tk), 1e-4)
    params = _params_dev(arrs)
    u0 = np.log(np.random.default_rng(1).uniform(0.05, 50.0, K))
    u0[7], u0[8] = 9.5, -8.7                              # outside the bounds
    ref = _adam_search(_dev(y_tk), rc, params, flags, K, u0)
    bad = _adam_search(_dev(y_bad), rc, params, flags, K, u0)
    assert bad[1][3, 3] == 1e12 and bad[1][3, 4] == 2 and bad[1][3, 5] == 1.0
    others = [k for k in range(K) if k != 3]
    np.testing.assert_array_equal(bad[1][others], ref[1][others])
    prep = _adam_search(_dev(y_tk), rc, params, flags, K, u0, prepare=True)
    np.testing.assert_array_equal(prep[1], ref[1])
    np.testing.assert_array_equal(prep[2], ref[2])
    set_knob('EKS_ADAM_STREAM', '1')
    strm = _adam_search(_dev(y_tk), rc, params, flags, K, u0, stride=16)
    bad_s = _adam_search(_dev(y_bad), rc, params, flags, K, u0, stride=16)
    np.testing.assert_array_equal(ref[1][:, 4:], strm[1][:, 4:])
    assert bad_s[1][3, 3] == 1e12 and bad_s[1][3, 4] == 2
    assert np.abs(np.log(ref[2]) - np.log(strm[2])).max() < 2e-6


@pytest.mark.parametrize('T,K,unit', [(2000, 4, True), (700, 3, False), (9000, 20, True), (16384, 2, False),
                                      (130, 5, True), (2, 2, True)])
def test_adam_whole_loop_in_one_launch_reproduces_the_per_iteration_loop(T, K, unit, set_knob):
    """Sessions of up to 16 384 frames with one keypoint per optimiser block run all iterations of an eks_adam_run
    call in ONE launch, a workgroup per keypoint (diag_nll_adam_persist_kernel).  Against the per-iteration kernels
    (EKS_ADAM_PER_ITERATION=1) on the same problem: the same number of iterations per keypoint and log s within
    2e-6 (the chunking differs - 64 chunks of T / 64 frames instead of 512-frame chunks - so the float32 summaries
    round differently), and against the oracle's Adam (oracle/eks_oracle.py: adam_optimize_s on the C port's
    complex-step gradient) with the same stopping iteration and log s within 1e-5."""
    from eks_amd import hip_ops
    arrs, y_tk, var_tk = _singlecam_problem(max(T, 2), K, seed=900 + T, unit=unit)
    y_tk, var_tk = y_tk[:T], var_tk[:T]
    flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
    y, rc = _dev(y_tk), hip_ops.const_r(_dev(var_tk), 1e-4)
    params = _params_dev(arrs)
    offs = torch.arange(K + 1, dtype=torch.int32, device='cuda')
    mem = torch.arange(K, dtype=torch.int32, device='cuda')
    u0 = np.log(np.random.default_rng(T).uniform(0.05, 20.0, K))

    def run():
        state = np.zeros((K, 6))
        state[:, 0] = u0
        state[:, 3] = np.inf
        state = _dev(state)
        s_kp = _dev(np.exp(u0))
        loop = hip_ops.AdamLoop(y, rc, *params, offs, mem, state, s_kp, 0.25, -8.0, 8.0, 1e-2, 300, flags=flags)
        for _ in range(40):
            loop.run(8)
            if int(loop.n_active.item()) == 0:
                break
        return state.cpu().numpy(), s_kp.cpu().numpy()

    st_p, s_p = run()
    set_knob('EKS_ADAM_PER_ITERATION', '1')
    st_i, s_i = run()
    assert np.array_equal(st_p[:, 4], st_i[:, 4]), (st_p[:, 4], st_i[:, 4])          # iterations taken
    assert np.array_equal(st_p[:, 5], st_i[:, 5])
    assert np.abs(np.log(s_p) - np.log(s_i)).max() < 2e-6
    if T >= 100:
        from oracle import c_oracle
        ks = list(range(min(K, 4)))
        ys = np.transpose(y_tk, (1, 0, 2)).astype(np.float64)
        Rc = rc.cpu().numpy()
        zero = np.zeros((1, 2, 2))

        def loss_and_grad(u):
            out = []
            for j, k in enumerate(ks):
                sQ = np.exp(u[j]) * arrs['Qs'][k]
                L, g = c_oracle.nll_directional(ys[k], Rc[k], arrs['m0s'][k], arrs['S0s'][k], arrs['As'][k],
                                                arrs['Cs'][k], sQ, zero, sQ[None])
                out.append((L, g[0]))
            return np.array([o[0] for o in out]), np.array([o[1] for o in out])

        u_o, _, it_o = orc.adam_optimize_s(loss_and_grad, u0[ks], tol=1e-2, safety_cap=300)
        s_o = np.exp(np.clip(u_o, -8.0, 8.0))
        assert np.array_equal(st_p[ks, 4].astype(int), it_o)
        assert np.abs(np.log(s_p[ks]) - np.log(s_o)).max() < 1e-5
