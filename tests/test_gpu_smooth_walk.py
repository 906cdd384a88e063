"""Walk form of the windowed replay (eks_diag.hip: replay_walk_block - a block takes a run of window groups one per
step, every chunk loaded and summarised once per run) against the block-per-group form (replay_window_block,
EKS_SMOOTH_WINDOW_WALK=0): per lane the two do the same operations in the same order, so every output bit is equal,
for every run length (EKS_SMOOTH_WINDOW_RUN).  EKS_SMOOTH_WINDOW_MIN_T=1024 lets a few thousand frames take the form.

T = 1 029 / 2 817 / 4 165 frames are 5 / 12 / 17 window groups: a last group of one chunk of five frames, a ragged last
chunk (2 817 = 88 chunks + 1 frame), and more than three turns of the three-step rotation of the chunks over the waves
(chunk j is wave j mod 12's, a group is 8 chunks)."""
import numpy as np
import pytest

import window_ref as wr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

TS = (1029, 2817, 4165)
K2 = 33                           # x D = 2: 66 chains, two tiles, the second holds one keypoint


def _nwg(T):
    return ((T + wr.B - 1) // wr.B + wr.G - 1) // wr.G


def _runs(T):
    n = _nwg(T)
    return (1, 2, 3, 4, n, n + 5)


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _prepared(p, vs_diag):
    from eks_amd import hip_ops
    flags = hip_ops.model_flags(p['S0'], p['A'], p['C'], p['Q'])
    f64 = [_dev(p[k], torch.float64) for k in ('m0', 'S0', 'A', 'C', 'Q', 's')]
    y = _dev(p['y'])
    T, K, D = y.shape
    out = (torch.full((T, K, D), float('nan'), device='cuda'),             # a lane nobody stores stays NaN
           torch.full((T, K, D) if vs_diag else (T, K, D, D), float('nan'), device='cuda'))
    return hip_ops.PreparedSmooth(y, _dev(p['var']), *f64, flags=flags, vs_diag=vs_diag, out=out)


def _run(set_knob, p, mode, vs_diag, walk, run=None, forward=None):
    set_knob('EKS_SMOOTH_WINDOW', str(mode))
    set_knob('EKS_SMOOTH_WINDOW_MIN_T', '1024')
    set_knob('EKS_SMOOTH_WINDOW_WALK', str(walk))
    set_knob('EKS_SMOOTH_WINDOW_RUN', None if run is None else str(run))
    set_knob('EKS_REPLAY_FORWARD', forward)
    ms, Vs = _prepared(p, vs_diag)()
    torch.cuda.synchronize()
    return ms, Vs


def _same_bits(a, b):
    """Equal NaN masks and equal bits elsewhere."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a).view(torch.int32),
                                               torch.where(nb, torch.zeros_like(b), b).view(torch.int32))


def _check_all_runs(set_knob, p, vs_diag, runs, modes=(1, 2), forwards=(None, '1'), want_nan=None):
    for forward in forwards:
        for mode in modes:
            ms0, Vs0 = _run(set_knob, p, mode, vs_diag, walk=0, forward=forward)
            if mode == 1:
                assert not bool(torch.isnan(ms0).any()) and not bool(torch.isnan(Vs0).any())
            elif want_nan is not None:
                assert bool(torch.isnan(ms0).any()) == want_nan
            for run in runs:
                ms1, Vs1 = _run(set_knob, p, mode, vs_diag, walk=1, run=run, forward=forward)
                what = (mode, run, forward)
                if mode == 1:
                    assert torch.equal(ms1, ms0), what
                    assert torch.equal(Vs1, Vs0), what
                else:
                    assert _same_bits(ms1, ms0), what
                    assert _same_bits(Vs1, Vs0), what


@pytest.mark.parametrize('general', [False, True], ids=['unit', 'per_chain'])
@pytest.mark.parametrize('vs_diag', [True, False], ids=['diag', 'full'])
@pytest.mark.parametrize('T', TS)
def test_same_bits_as_the_block_per_group_form_for_every_run_length(set_knob, T, vs_diag, general):
    p = wr.problem(T, K2, 2, seed=300 + T + int(general), general=general, neg_c=general)
    assert (K2 * 2) % 64 != 0 and K2 * 2 > 64
    _check_all_runs(set_knob, p, vs_diag, _runs(T))


def test_the_rule_itself_chooses_the_form_and_the_bits_stay(set_knob):
    """No run length forced: whatever walk_run_length picks for the launch, the outputs are the block-per-group form's."""
    p = wr.problem(4165, K2, 2, seed=77)
    _check_all_runs(set_knob, p, True, (None,))


@pytest.mark.parametrize('T', sorted(set(wr.FAIL_T + TS)))
def test_failing_lanes_at_a_runs_first_group_inside_it_at_its_last_and_in_the_ragged_end(set_knob, T):
    """window_ref.fail_pattern_problem: lanes fail in groups 0 .. 3, in the last three groups and in the ragged end; with
    runs of 1, 2, 3, 4 groups and one run over all of them each of those is a run's first group, an inner one and its
    last.  Mode 2: the NaN pattern (the verdict per group and chain) and every stored bit; mode 1: fail plane and gate
    drive the exact launches to the same outputs."""
    p = wr.fail_pattern_problem(T)
    _check_all_runs(set_knob, p, True, _runs(T), want_nan=True)


def test_general_models_with_occlusions_and_slow_chains_inside_a_tile(set_knob):
    p = wr.general_problem()
    T = p['y'].shape[0]
    for vs_diag in (True, False):
        _check_all_runs(set_knob, p, vs_diag, _runs(T), want_nan=True)


@pytest.mark.parametrize('general', [False, True], ids=['unit', 'per_chain'])
def test_one_run_over_every_group_still_enters_each_from_its_stand_in(set_knob, general):
    """window_ref.stand_in_problem makes the stand-in visible (1e-3 .. 1e-2 of the magnitude from the exact smoother):
    a walk that carried its belief from group to group would differ from the block-per-group form here."""
    p = wr.stand_in_problem(general)
    n = _nwg(p['y'].shape[0])
    _check_all_runs(set_knob, p, True, (n, 3), forwards=(None,))
    ms2, _ = _run(set_knob, p, 2, True, walk=1, run=n)
    r = wr.restate(p)
    stored = ~wr.group_mask(r['fail'], p['y'].shape[0])
    got = ms2.cpu().numpy().astype(np.float64).reshape(r['ms'].shape)
    assert stored.any()
    scale = np.abs(r['ms_x']).max()
    away = np.abs(r['ms'] - r['ms_x'])[stored].max() / scale
    err = np.abs(got - r['ms'])[stored].max() / scale
    print(f'stand-in: restatement {away:.3g} of the magnitude from the exact smoother, kernel {err:.3g} from the restatement')
    assert away > 1e-4, 'the problem no longer shows the stand-in'
    assert err < 1e-5 < away


@pytest.mark.parametrize('kind', ['low', 'high'])
def test_variances_at_the_edges_of_the_clip(set_knob, kind):
    p = wr.clip_problem(kind)
    _check_all_runs(set_knob, p, True, (2, 3, _nwg(wr.CLIP_T)), forwards=(None,))


def test_an_all_slow_tile_beside_a_fast_one(set_knob):
    """100 chains: tile 0 is keypoints 0 .. 31, every one slow by the probe (s = exp(-8)): its blocks return before any
    row is requested, for the whole run; tile 1 is fast."""
    K = 50
    s = np.where(np.arange(K) < 32, np.exp(-8.0), 3.0)
    p = wr.problem(2817, K, 2, seed=91, s=s)
    _check_all_runs(set_knob, p, True, (1, 3, _nwg(2817)), modes=(1,))
    _check_all_runs(set_knob, p, False, (4,), modes=(1,), forwards=(None,))


_WIDTH_ORACLE = {}


def _width_oracle(D, general, p):
    if (D, general) not in _WIDTH_ORACLE:
        from oracle import c_oracle
        ms, Vs, _ = c_oracle.smooth(np.transpose(p['y'], (1, 0, 2)).astype(np.float64),
                                    np.clip(np.transpose(p['var'], (1, 0, 2)).astype(np.float64), 1e-12, 1e30),
                                    p['m0'], p['S0'], p['A'], p['C'], p['Q'], p['s'])
        _WIDTH_ORACLE[(D, general)] = (ms, np.diagonal(Vs, axis1=2, axis2=3))
    return _WIDTH_ORACLE[(D, general)]


@pytest.mark.parametrize('vs_diag', [True, False], ids=['diag', 'full'])
@pytest.mark.parametrize('general', [False, True], ids=['unit', 'per_chain'])
@pytest.mark.parametrize('D', [1, 3, 5, 8])
def test_every_state_width(set_knob, D, general, vs_diag):
    """Rows of one, three, five and eight floats (the stores of three floats and more leave in pieces of 8 bytes): the
    block-per-group form's bits, the oracle within 1e-5, exact zeros off the diagonal."""
    T, K = 2817, wr.WIDTH_K[D]
    assert (K * D) % 64 != 0 and K * D > 64
    p = wr.problem(T, K, D, seed=500 + 2 * D + int(general), general=general)
    _check_all_runs(set_knob, p, vs_diag, (1, 3, 5, _nwg(T)), forwards=(None,))
    ms, Vs = _run(set_knob, p, 1, vs_diag, walk=1, run=3)
    ms_o, Vd_o = _width_oracle(D, general, p)
    ms_k = np.transpose(ms.cpu().numpy().astype(np.float64), (1, 0, 2))
    Vd = Vs if vs_diag else torch.diagonal(Vs, dim1=2, dim2=3)
    Vd = np.transpose(Vd.cpu().numpy().astype(np.float64), (1, 0, 2))
    em = float((np.abs(ms_k - ms_o) / np.abs(ms_o).max(axis=(1, 2), keepdims=True)).max())
    eV = float((np.abs(Vd - Vd_o) / Vd_o).max())
    print(f'D = {D}: ms {em:.3g}, Vs {eV:.3g} of the oracle (bar 1e-5)')
    assert em < 1e-5 and eV < 1e-5
    if not vs_diag:
        off = ~torch.eye(D, dtype=torch.bool, device='cuda')
        assert not bool(Vs[:, :, off].any())


@pytest.mark.parametrize('mode', [1, 2])
def test_a_second_call_and_a_dirty_workspace_give_the_same_bits(set_knob, mode):
    p = wr.fail_pattern_problem(2817 if mode == 1 else 4165)
    set_knob('EKS_SMOOTH_WINDOW', str(mode))
    set_knob('EKS_SMOOTH_WINDOW_MIN_T', '1024')
    set_knob('EKS_SMOOTH_WINDOW_WALK', '1')
    set_knob('EKS_SMOOTH_WINDOW_RUN', '3')
    ps = _prepared(p, False)
    ms, Vs = (t.clone() for t in ps())
    ms_b, Vs_b = (t.clone() for t in ps())
    assert _same_bits(ms, ms_b) and _same_bits(Vs, Vs_b)
    ps._keep[-1].fill_(0xFF)                          # the workspace: fail plane, gate, slow flags, scan planes
    ps.ms.fill_(float('nan'))
    ps.Vs.fill_(float('nan'))
    ms_c, Vs_c = ps()
    torch.cuda.synchronize()
    assert _same_bits(ms, ms_c) and _same_bits(Vs, Vs_c)
    if mode == 1:
        assert not bool(torch.isnan(ms_c).any()) and not bool(torch.isnan(Vs_c).any())
