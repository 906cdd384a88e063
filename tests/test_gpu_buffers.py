"""GPU: the workspace and output-buffer contract of every C entry point that takes a workspace (DESIGN.md 9h has the
audit these tests confirm).

Workspace state.  Every case runs on a workspace whose body is 0x00 bytes, on the bytes another call of the same shape
left behind ("stale": the same entry point on another seed and another s regime and, where entry points share a
workspace size, the other entry point), and on 0xFF bytes (NaN as float32 / float64, -1 as an int, 255 as a flag).  The
body is exactly the queried size with 0xA5 guards around it (tests/buffer_guard.py).  Asserted: the outputs of the
three runs are bit-identical, the guards are intact, no input changed, and the 0xFF run passes the reference check of
the entry point's own test file, through that file's function and at that file's bar.  Bit equality between the runs is
the only comparison of kernel output with kernel output.

Output guards.  Every output lies between 0xA5 guards of at least one full row, at the shapes where the last stored
row or vector is partial, at an even and at an odd float offset; NULL optional outputs in every combination the header
allows.  Asserted: guards intact, the outputs pass the file's reference check, a NULL output changes no bit elsewhere.

Order in the file = order to run in: all 0x00 and stale cases, the output guards, then 0xFF."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_ref  # noqa: E402
import sampling_ref as sref  # noqa: E402
import test_gpu_ekf as ekf  # noqa: E402
import test_gpu_ekf_generic as ekfg  # noqa: E402
import test_gpu_em as em  # noqa: E402
import test_gpu_increments as inc  # noqa: E402
import test_gpu_innovations as innov  # noqa: E402
import test_gpu_kernels as kern  # noqa: E402
import test_gpu_pupil_forms as pupil  # noqa: E402
import test_gpu_sampling as samp  # noqa: E402
import test_gpu_sampling_dense as sampd  # noqa: E402
import test_gpu_smooth_tv as tv  # noqa: E402
import test_gpu_smooth_window as win  # noqa: E402
from buffer_guard import guarded_output, guarded_workspaces, same_bits, stale_fill  # noqa: E402
from test_increments_cpu import dense_case  # noqa: E402
from test_sampling_cpu import dev_error, make_chains  # noqa: E402
from test_smooth_tv_cpu import random_w  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

PARAMS = inc.PARAMS
_dev = inc._dev
B = 32                  # frames per lane of the scalar-chain kernels (kChunk, kChainChunk)
B_DENSE = 16            # dense_chunk() of a small general model
T_LANES = (B + 1, 64 * B + 1)                 # one frame past a chunk, one frame past 64 chunks
CHAINS = ((1, 1), (65, 1), (3 * 64 + 1, 1))   # N = 1 (packed lanes), one chain past a tile, one past three tiles


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _scopes(fn):
    def synced():
        fn()
        torch.cuda.synchronize()
    return win._scopes(synced)


def _ws_bytes(query, dims_args, *extra):
    from eks_amd import _lib
    d = _lib.EksDims(*[int(x) for x in dims_args])
    return int(getattr(_lib.load(), query)(ctypes.byref(d), *extra))


# ==========================================================================================================================
# the cases: problem(variant) on the host ('a' is checked against the reference, 'b' only leaves its workspace behind),
# device(pb) -> tensors (dev['inputs']: what must not change), run(pb, dev) -> outputs, check(pb, outputs on the host)
# ==========================================================================================================================
class Case:
    entry = ''           # the C entry point
    knobs = {}           # EKS_* variables of the case
    partner = None       # () -> a Case of another entry point with the same workspace size

    def __init__(self, cid):
        self.id = cid

    def premise(self, pb, dev):
        """Confirm the path the case is about (profile scopes, sizes); runs once, on a plain workspace."""

    def after_zero(self, gw):
        """Look at the workspace the 0x00 run left behind (path confirmation from the workspace itself)."""


class ScalarChains(Case):
    """eks_smooth_tv / eks_smooth_increments / eks_em_stats / eks_innovations on the scalar chains of edge_session."""
    ENTRY = dict(smooth_tv='eks_smooth_tv', increments='eks_smooth_increments', em_stats='eks_em_stats',
                 innovations='eks_innovations')
    SHARED = ('em_stats', 'innovations', 'smooth_tv')          # diag_em_workspace_bytes: one size for the three

    def __init__(self, op, T, K, D, kind):
        super().__init__(f'{op}-chains-T{T}-N{K * D}-{kind}')
        self.op, self.T, self.K, self.D, self.kind, self.entry = op, T, K, D, kind, self.ENTRY[op]
        if op in self.SHARED:
            other = self.SHARED[(self.SHARED.index(op) + 1) % 3]
            self.partner = lambda: ScalarChains(other, T, K, D, kind)

    def problem(self, variant):
        T, K, D = self.T, self.K, self.D
        sval, seed = (2.0, 100 + T + K) if variant == 'a' else (1e-4, 900 + T + K)
        if self.op == 'smooth_tv':
            pb = tv.session(T, K, D, sval, 'unit' if self.kind == 'unit' else 'general', seed)
            pb['w'] = random_w(np.random.default_rng(seed + 1), (T, K) if K % 2 else (T,))
        else:
            pb = inc.edge_session(T, K, D, sval, self.kind, seed)
        return pb

    def device(self, pb):
        T, K, D = self.T, self.K, self.D
        dev = dict(y=_dev(pb['y'].reshape(T, K, D)), var=_dev(pb['var'].reshape(T, K, D)),
                   par=[_dev(pb['par'][k]) for k in PARAMS])
        dev['inputs'] = [dev['y'], dev['var']] + dev['par']
        if self.op == 'smooth_tv':
            dev['w'] = _dev(pb['w'])
            dev['inputs'].append(dev['w'])
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        args, flags = (dev['y'], dev['var'], *dev['par']), inc.diag_flags(pb)
        if self.op == 'smooth_tv':
            ms, Vs = hip_ops.smooth_tv(dev['y'], dev['var'], dev['w'], *dev['par'], flags=flags, vs_diag=True)
            return dict(ms=ms, Vs=Vs)
        if self.op == 'increments':
            return hip_ops.smooth_increments(*args, flags=flags, vs_diag=True)
        if self.op == 'em_stats':
            return dict(Sw=hip_ops.em_stats(*args, flags=flags, vs_diag=True))
        return hip_ops.innovations(*args, flags=flags, want=innov.SCALAR_OUT)

    def check(self, pb, out):
        T, N = self.T, self.K * self.D
        if self.op == 'smooth_tv':
            tv.check_scalar(self.id, pb, pb['w'], (out['ms'].reshape(T, N), out['Vs'].reshape(T, N)))
        elif self.op == 'increments':
            print(inc.check_scalar(self.id, pb, {n: v.reshape(T, N) for n, v in out.items()}))
        elif self.op == 'em_stats':
            print(em.check_scalar(self.id, pb, out['Sw'].reshape(N)))
        else:
            print(innov.check_scalar(self.id, pb, dict(v=out['innov'].reshape(T, N), S=out['innov_var'].reshape(T, N),
                                                       ll=out['loglik'].reshape(N))))

    def premise(self, pb, dev):
        names = dict(smooth_tv=['smooth_tv_summarize', 'em_scan', 'smooth_tv_replay'],
                     increments=['increments_summarize', 'increments_scan', 'increments_replay'],
                     em_stats=['em_summarize', 'em_scan', 'em_replay', 'em_reduce'],
                     innovations=['em_summarize', 'em_scan', 'innov_replay', 'em_reduce'])[self.op]
        assert _scopes(lambda: self.run(pb, dev)) == names


class SampleChains(Case):
    """eks_sample on the scalar chains of make_chains, injected normals (the arithmetic the generator path shares)."""
    entry = 'eks_sample'

    def __init__(self, T, K, D, unit, n_draws):
        super().__init__(f'sample-chains-T{T}-N{K * D}-{"unit" if unit else "general"}-draws{n_draws}')
        self.T, self.K, self.D, self.unit, self.S = T, K, D, unit, n_draws

    def problem(self, variant):
        T, K, D, N = self.T, self.K, self.D, self.K * self.D
        sval = (2.0 if self.unit else 0.7) if variant == 'a' else 1e-3
        pb = make_chains(T, K, D, sval, self.unit, seed=(1000 if variant == 'a' else 5000) * N + T)
        pb['z'] = np.random.default_rng(N + T + len(variant)).normal(size=(self.S, T, N)).astype(np.float32)
        return pb

    def device(self, pb):
        T, K, D = self.T, self.K, self.D
        dev = dict(y=_dev(pb['y'].reshape(T, K, D)), var=_dev(pb['var'].reshape(T, K, D)),
                   par=[_dev(pb['par'][k]) for k in PARAMS], z=_dev(pb['z'].reshape(self.S, T, K, D)))
        dev['inputs'] = [dev['y'], dev['var'], dev['z']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        dr, ms = hip_ops.sample(dev['y'], dev['var'], *dev['par'], self.S, flags=samp._flags(pb), noise=dev['z'],
                                want_mean=True)
        return dict(draws=dr, ms=ms)

    def check(self, pb, out):
        check_sample_chains(self.id, pb, out['draws'].reshape(self.S, self.T, -1), out['ms'].reshape(self.T, -1), pb['z'])

    def premise(self, pb, dev):
        assert _scopes(lambda: self.run(pb, dev)) == ['sample_summarize', 'sample_kalman_scan', 'sample_beta',
                                                      'sample_draw_scan', 'sample_replay']


def check_sample_chains(label, pb, dr, ms, z):
    """The same-noise parity of tests/test_gpu_sampling.py (its references, its bar rule) for injected normals."""
    Pf, ms64, Vs64, _ = samp.ref_chain(pb)
    sd = np.sqrt(Vs64)
    e64 = sref.scalar_deviations(Pf, pb['a'], pb['qs'], z)
    e32 = sref.scalar_deviations_f32(pb['var'], pb['S0d'], pb['a'], pb['c'], pb['qs'], z)
    trans = float(np.abs((e32 - e64) / sd).max())
    trans_out = float(np.abs((sref.read_through_f32_output(ms64, e32) - e64) / sd).max())
    bar, bar_raw = max(1e-5, 4 * trans), max(1e-5, 4 * trans_out)
    assert np.isfinite(dr).all() and np.isfinite(ms).all(), label
    err = dev_error(dr - ms[None], e64, dr, sd)
    raw = float(np.abs((dr - ms[None] - e64) / sd).max())
    scale = np.abs(ms64).max(axis=0)
    if pb['T'] <= 3:
        scale = np.maximum(scale, np.abs(pb['m0f']))
    e_ms = float((np.abs(ms - ms64) / scale).max())
    print(f'{label}: kernels {err:.3g} beyond the output rounding (bar {bar:.3g}), raw {raw:.3g} (bar {bar_raw:.3g}), '
          f'ms {e_ms:.3g} (bar 1e-05)')
    assert err < bar and raw < bar_raw and e_ms < 1e-5, label


class GeneralModel(Case):
    """The same four entry points on one general model (stable dense_case, data simulated from the model)."""
    K, D, O = 3, 3, 4

    def __init__(self, op, T):
        super().__init__(f'{op}-general-T{T}')
        self.op, self.T, self.entry = op, T, ScalarChains.ENTRY[op]

    def problem(self, variant):
        a = variant == 'a'
        M = inc.stable(dense_case(self.K, self.D, self.O, False, seed=35 if a else 53))
        if not a:
            M['s'] = M['s'] * 1e-3
        y, var = inc.dense_session(M, self.T, self.O, seed=self.T + (0 if a else 7))
        return dict(M=M, y=y, var=var, w=random_w(np.random.default_rng(self.T), (self.T, self.K)))

    def device(self, pb):
        dev = dict(y=_dev(pb['y']), var=_dev(pb['var']), par=[_dev(pb['M'][k]) for k in PARAMS], w=_dev(pb['w']))
        dev['inputs'] = [dev['y'], dev['var'], dev['w']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        args = (dev['y'], dev['var'], *dev['par'])
        if self.op == 'smooth_tv':
            ms, Vs = hip_ops.smooth_tv(dev['y'], dev['var'], dev['w'], *dev['par'], flags=0, vs_diag=False)
            return dict(ms=ms, Vs=Vs)
        if self.op == 'increments':
            return hip_ops.smooth_increments(*args, flags=0, vs_diag=False)
        if self.op == 'em_stats':
            return dict(Sw=hip_ops.em_stats(*args, flags=0, vs_diag=False))
        return hip_ops.innovations(*args, flags=0, want=innov.DENSE_OUT)

    def check(self, pb, out):
        M, y, var = pb['M'], pb['y'], pb['var']
        if self.op == 'smooth_tv':
            print(tv.check_dense(self.id, M, y, var, pb['w'], (out['ms'], out['Vs'])))
        elif self.op == 'increments':
            print(inc.check_dense(self.id, M, y, var, out, False)[0])
        elif self.op == 'em_stats':
            em.check_dense(self.id, M, y, var, out['Sw'], False)
        else:
            print(innov.check_dense(self.id, M, y, var, out))

    def premise(self, pb, dev):
        stem = dict(smooth_tv='dense_tv', increments='dense_increments', em_stats='dense_em', innovations='dense_innov')
        names = [f'{stem[self.op]}_{p}' for p in ('summarize', 'scan', 'replay')]
        if self.op in ('em_stats', 'innovations'):
            names.append('em_reduce')
        assert _scopes(lambda: self.run(pb, dev)) == names
        assert -(-self.T // B_DENSE) == (2 if self.T == B_DENSE + 1 else 65)      # 16-frame chunks: one past 1, past 64


class SampleGeneral(Case):
    entry = 'eks_sample'
    K, D, O = 3, 3, 4

    def __init__(self, T, n_draws):
        super().__init__(f'sample-general-T{T}-draws{n_draws}')
        self.T, self.S = T, n_draws

    def problem(self, variant):
        seed = 300 if variant == 'a' else 400
        M = sampd.stable_model(self.K, self.D, self.O, seed)
        if variant == 'b':
            M['s'] = M['s'] * 1e-3
        y, var = sampd.session(M, self.T, self.O, seed + 2)
        z = np.random.default_rng(seed + 3).normal(size=(self.S, self.T, self.K, self.D + self.O)).astype(np.float32)
        return dict(M=M, y=y, var=var, z=z)

    def device(self, pb):
        dev = dict(y=_dev(pb['y']), var=_dev(pb['var']), par=[_dev(pb['M'][k]) for k in PARAMS], z=_dev(pb['z']))
        dev['inputs'] = [dev['y'], dev['var'], dev['z']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        dr, ms = hip_ops.sample(dev['y'], dev['var'], *dev['par'], self.S, flags=0, noise=dev['z'], want_mean=True)
        return dict(draws=dr, ms=ms)

    def check(self, pb, out):
        sampd.check_parity(self.id, ('buffers', self.T, self.S), pb['M'], pb['y'], pb['var'], out['draws'], out['ms'],
                           pb['z'], np.arange(self.K))

    def premise(self, pb, dev):
        got = _scopes(lambda: self.run(pb, dev))
        assert got[0] == 'dense_sample_simulate' and got[-1] == 'dense_sample_combine', got


def smooth_problem(T, K, D, seed, unit, slow=False):
    """win._problem for any D: the keys win._oracle / win._assert_oracle read."""
    rng = np.random.default_rng(seed)
    a, c = (1.0, 1.0) if unit else (0.98, 1.3)
    if unit:
        x = 50.0 + np.cumsum(0.5 * rng.standard_normal((T, K, D)), axis=0)
        m0 = np.full((K, D), 50.0)
    else:
        x = 3.0 * rng.standard_normal((T, K, D))
        m0 = np.zeros((K, D))
    var = (0.3 * rng.gamma(2.0, 1.0, (T, K, D)) + 0.02).astype(np.float32)
    y = (c * x + np.sqrt(var) * rng.standard_normal((T, K, D))).astype(np.float32)
    eye = np.tile(np.eye(D), (K, 1, 1))
    s = np.full(K, np.exp(-8.0)) if slow else np.exp(rng.uniform(0.0, 4.0, K))
    return dict(y=y, var=var, m0=m0, S0=eye * 25.0, A=eye * a, C=eye * c, Q=eye.copy(), s=s)


class SmoothChains(Case):
    """eks_smooth on scalar chains: packed lanes, the fused scan, the three-kernel scan, elements kept / recomputed."""
    entry = 'eks_smooth'

    def __init__(self, name, T, K, D, unit, knobs):
        super().__init__(f'smooth-{name}-T{T}-N{K * D}-{"unit" if unit else "general"}')
        self.T, self.K, self.D, self.unit, self.knobs, self.name = T, K, D, unit, knobs, name

    def problem(self, variant):
        return smooth_problem(self.T, self.K, self.D, seed=11 if variant == 'a' else 12, unit=self.unit,
                              slow=variant == 'b')

    def device(self, p):
        from eks_amd import hip_ops
        dev = dict(y=_dev(p['y']), var=_dev(p['var']), par=[_dev(p[k], torch.float64) for k in PARAMS],
                   flags=hip_ops.model_flags(p['S0'], p['A'], p['C'], p['Q']))
        dev['inputs'] = [dev['y'], dev['var']] + dev['par']
        return dev

    def run(self, p, dev):
        from eks_amd import hip_ops
        ms, Vs = hip_ops.smooth(dev['y'], dev['var'], *dev['par'], flags=dev['flags'], vs_diag=True)
        return dict(ms=ms, Vs=Vs)

    def check(self, p, out):
        win._assert_oracle(('buffers', self.id), p, torch.as_tensor(out['ms']), torch.as_tensor(out['Vs']), True)

    def premise(self, p, dev):
        from eks_amd import _lib
        N = self.K * self.D
        assert bool(dev['flags'] & _lib.FLAG_UNIT_AC) == self.unit and dev['flags'] & _lib.FLAG_DIAG_MODEL
        # eks_diag.hip diag_smooth: the fused scan where a wave holds 64 chains (N > 32) unless EKS_SMOOTH_UNFUSED=1; the
        # three forms share their scope names, so the shape and the knob are the premise; no windowed replay at this T
        assert {'packed': N < 64 and N <= 32, 'fused': 32 < N <= 64, 'unfused': N > 64 and N % 64 != 0}[self.name]
        assert (self.knobs.get('EKS_SMOOTH_UNFUSED') == '1') == (self.name == 'unfused')
        assert _scopes(lambda: self.run(p, dev)) == ['diag_summarize', 'diag_scan', 'diag_replay']


class SmoothGeneral(Case):
    """eks_smooth on general models: the wave, runs and generic organisations of dense_smooth."""
    entry = 'eks_smooth'

    def __init__(self, name, T, K, D, O, general_A, knobs):
        super().__init__(f'smooth-{name}-T{T}-K{K}-D{D}-O{O}')
        self.name, self.T, self.K, self.D, self.O, self.general_A, self.knobs = name, T, K, D, O, general_A, knobs

    def problem(self, variant):
        a = variant == 'a'
        arrs, y, var = kern._dense_problem(self.T, self.K, self.D, self.O, seed=self.T + self.K + (0 if a else 50))
        if self.general_A:
            arrs['As'] = arrs['As'] * 0.97 + 0.02 * np.random.default_rng(9).standard_normal((self.K, self.D, self.D))
        s = np.exp(np.random.default_rng(3).uniform(-3, 4, self.K)) * (1.0 if a else 1e-4)
        return dict(arrs=arrs, y=y, var=var, s=s)

    def device(self, pb):
        dev = dict(y=_dev(pb['y']), var=_dev(pb['var']), par=kern._params_dev(pb['arrs']) + [_dev(pb['s'])])
        dev['inputs'] = [dev['y'], dev['var']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        ms, Vs = hip_ops.smooth(dev['y'], dev['var'], *dev['par'], flags=0)
        return dict(ms=ms, Vs=Vs)

    def check(self, pb, out):
        check_smooth_general(self.id, pb, out['ms'], out['Vs'])

    def premise(self, pb, dev):
        from eks_amd import _lib
        dims = (self.K, self.T, self.D, self.O, 0)
        got = _scopes(lambda: self.run(pb, dev))
        size = _ws_bytes('eks_smooth_workspace_bytes', dims)
        lib = _lib.load()
        saved = {k: os.environ.pop(k) for k in self.knobs}           # the size the shape takes by itself
        lib.eks_knobs_reload()
        plain = _ws_bytes('eks_smooth_workspace_bytes', dims)
        os.environ.update(saved)
        lib.eks_knobs_reload()
        if self.name == 'wave':
            assert got == ['dense_summarize', 'dense_replay'], got
        else:
            assert got == ['dense_summarize', 'dense_scan', 'dense_replay'], got
        if self.name == 'tree':           # the generic layout (with its filtered-belief stream) instead of the runs layout
            assert size != plain
        if self.name == 'blocks':
            chunk = int(self.knobs['EKS_DENSE_CHUNK'])
            assert -(-self.T // chunk) > 64 and size != plain


def check_smooth_general(label, pb, ms, Vs):
    """tests/test_gpu_kernels.py test_smooth_dense_wide_sessions_match_oracle: the C port on every frame, 1e-5."""
    from oracle import c_oracle
    from oracle import eks_oracle as orc
    arrs = pb['arrs']
    Rd = orc.build_R_from_vars(np.swapaxes(arrs['ensemble_vars'], 0, 1))
    ms_o, Vs_o, _ = c_oracle.smooth(arrs['ys'], Rd, arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], pb['s'])
    ms = np.transpose(ms.astype(np.float64), (1, 0, 2))
    Vs = np.transpose(Vs.astype(np.float64), (1, 0, 2, 3))
    e_m, e_V = kern._rel(ms, ms_o, axis_scale=(1, 2)), kern._rel(Vs, Vs_o, axis_scale=(1, 2, 3))
    print(f'{label}: ms {e_m:.3g}, Vs {e_V:.3g} of the C port (bar 1e-5)')
    assert e_m < 1e-5 and e_V < 1e-5, label


class EmLoop(Case):
    """eks_em_scale_run through EmScaleLoop: twelve iterations, blocks of two and three keypoints."""
    entry = 'eks_em_scale_run'
    BLOCKS = [[0, 3], [1, 2, 4]]

    def __init__(self, kind):
        super().__init__(f'em_scale_run-{kind}')
        self.kind = kind

    def problem(self, variant):
        pb, q, args = em.scalar_loop_problem(600, 5, self.kind, seed=33 if variant == 'a' else 34,
                                             sval=2.0 if variant == 'a' else 1e-3)
        pb['loop_args'] = args
        return pb

    def device(self, pb):
        T, K, D = pb['T'], pb['K'], pb['D']
        dev = dict(y=_dev(pb['y'].reshape(T, K, D)), var=_dev(pb['var'].reshape(T, K, D)),
                   par=[_dev(pb['par'][k]) for k in ('m0', 'S0', 'A', 'C', 'Q')])
        dev['inputs'] = [dev['y'], dev['var']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        blocks, log_s0 = self.BLOCKS, np.log([0.5, 3.0])
        offs = np.zeros(len(blocks) + 1, np.int32)
        offs[1:] = np.cumsum([len(b) for b in blocks])
        members = np.concatenate([np.asarray(b, np.int32) for b in blocks])
        state = np.zeros((len(blocks), 4))
        state[:, 0] = log_s0
        s_k = np.empty(pb['K'])
        for b, mem in enumerate(blocks):
            s_k[list(mem)] = np.exp(log_s0[b])
        loop = hip_ops.EmScaleLoop(dev['y'], dev['var'], *dev['par'], _dev(offs), _dev(members), _dev(state), _dev(s_k),
                                   -8.0, 8.0, 0.0, 12, flags=inc.diag_flags(pb))
        loop.run(12)
        return dict(state=loop.state, s_keypoint=loop.s_keypoint, Sw=loop.Sw, n_active=loop.n_active)

    def check(self, pb, out):
        """tests/test_gpu_em.py test_blocks_of_two_and_three_keypoints..: log s against the float64 loop, the float32
        transcription run through the same loop setting the bar."""
        args, n, log_s0 = pb['loop_args'], 2 * 599, np.log([0.5, 3.0])
        h64, _, _ = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args), n, log_s0, self.BLOCKS, -8, 8, 0.0, 12, 12)
        h32, _, _ = em_ref.em_scale_loop(em_ref.scalar_trace_fn(*args, stats=em_ref.scalar_em_stats_f32, unit=pb['unit']),
                                         n, log_s0, self.BLOCKS, -8, 8, 0.0, 12, 12)
        st = out['state']
        err, trans = np.abs(st[:, 0] - h64[-1]).max(), np.abs(h32[-1] - h64[-1]).max()
        print(f'{self.id}: log s after 12 iterations {err:.3g} (transcription loop {trans:.3g})')
        assert err <= max(1e-5, 4 * trans)
        assert (st[:, 2] == 12).all() and not st[:, 3].any() and int(out['n_active'][0]) == 0
        for b, mem in enumerate(self.BLOCKS):
            assert (out['s_keypoint'][mem] == np.exp(st[b, 0])).all()


# eks_misc.hip: the finish kernel selects from a chain's list IN GLOBAL MEMORY when more than kMedList = 16 384 frames lie
# in the bracket, which holds 2 (2.25 sqrt(4096) + 1) + 1 = 291 of 4096 sample ranks = 7.1 % of the frames: T > 230 600.
# 300 000 frames put 21 300 in it (the count itself is read back from the workspace and asserted).
CONST_R_LIST_T, K_MED_LIST = 300_000, 16384


class ConstR(Case):
    entry = 'eks_const_r'

    def __init__(self, T, N):
        super().__init__(f'const_r-T{T}-N{N}')
        self.T, self.N = T, N

    def problem(self, variant):
        T, N = self.T, self.N
        rng = np.random.default_rng(T + N + (0 if variant == 'a' else 1))
        var = rng.gamma(2.0, 0.3 if variant == 'a' else 30.0, (T, N, 1)).astype(np.float32)
        var[rng.random((T, N, 1)) < 0.05] = 0.0                    # below the 1e-12 clip
        if T > 10 and N >= 5:                                      # the columns of test_const_r_is_exact_median
            var[3:9, 0, 0] = var[5, 0, 0]
            var[:, 1, 0] = 0.25
            var[rng.random(T) < 0.3, 2, 0] = np.nan
            var[:, 3, 0] = np.round(var[:, 3, 0], 1)
            var[: T // 2, 4, 0] *= 1e-3
        return dict(var=var)

    def device(self, pb):
        v = _dev(pb['var'])
        return dict(var=v, inputs=[v])

    def run(self, pb, dev):
        from eks_amd import hip_ops
        return dict(rconst=hip_ops.const_r(dev['var'], 1e-4))

    def check(self, pb, out):
        """tests/test_gpu_kernels.py: test_const_r_is_exact_median / .._select_from_the_list_in_global_memory."""
        from oracle import eks_oracle as orc
        var = pb['var']
        if self.T == CONST_R_LIST_T:
            ref = np.maximum(np.nanmedian(np.clip(var[:, :, 0].astype(np.float64), 1e-12, None), axis=0), 1e-4)
            np.testing.assert_array_equal(out['rconst'][:, 0], ref)
        else:
            ref = orc.constant_R_from_timevarying(np.clip(var.astype(np.float64), 1e-12, None)[:, :, 0].T[:, :, None], 1e-4)[:, 0]
            np.testing.assert_allclose(out['rconst'][:, 0], ref, rtol=1e-15, atol=0)

    def after_zero(self, gw):
        if self.T != CONST_R_LIST_T:
            return
        ab = -(-4 * self.N // 256) * 256                          # arr_bytes(N); arrays: lo, hi, less, valid, cnt, fallback
        body = gw.buffers[-1].body
        cnt = body[4 * ab:4 * ab + 4 * self.N].view(torch.int32).cpu().numpy()
        fallback = body[5 * ab:5 * ab + 4 * self.N].view(torch.int32).cpu().numpy()
        cap = -(-(self.T * 9 // 100 + 1024) // 64) * 64            # list_capacity(T)
        print(f'{self.id}: frames in the bracket {cnt}, capacity {cap}, fallback {fallback}')
        assert not fallback.any() and (cnt > K_MED_LIST).all() and (cnt <= cap).all()


class NllGrid(Case):
    """eks_nll / eks_nll_argmin on scalar chains, 64 candidates."""

    def __init__(self, name, T, K, unit, knobs, argmin=False):
        super().__init__(f'{"nll_argmin" if argmin else "nll"}-grid-{name}-T{T}-K{K}')
        self.name, self.T, self.K, self.unit, self.knobs, self.argmin = name, T, K, unit, knobs, argmin
        self.entry = 'eks_nll_argmin' if argmin else 'eks_nll'

    def problem(self, variant):
        a = variant == 'a'
        arrs, y_tk, var_tk = kern._singlecam_problem(self.T, self.K, seed=(17 if a else 71) + self.T, unit=self.unit)
        if not a:
            var_tk = (var_tk * 400.0).astype(np.float32)            # poles at 0.999: the other regime
        return dict(arrs=arrs, y=y_tk, var=var_tk, cand=np.exp(np.linspace(-8, 8, 64)))

    def device(self, pb):
        from eks_amd import hip_ops
        arrs = pb['arrs']
        dev = dict(y=_dev(pb['y']), rconst=hip_ops.const_r(_dev(pb['var']), 1e-4), par=kern._params_dev(arrs),
                   cand=_dev(pb['cand']), flags=hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs']))
        torch.cuda.synchronize()
        pb['Rc'] = dev['rconst'].cpu().numpy()
        dev['inputs'] = [dev['y'], dev['rconst'], dev['cand']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        args = (dev['y'], dev['rconst'], *dev['par'], dev['cand'])
        if self.argmin:
            nll, s, idx = hip_ops.nll_argmin(*args, flags=dev['flags'])
            return dict(nll=nll, s=s, idx=idx)
        return dict(nll=hip_ops.nll(*args, flags=dev['flags']))

    def check(self, pb, out):
        arrs, nll = pb['arrs'], out['nll']
        ref = kern._nll_grid_oracle(arrs['ys'], pb['Rc'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'],
                                    pb['cand'])
        err = float((np.abs(nll - ref) / np.abs(ref)).max())
        print(f'{self.id}: table {err:.3g} of the C oracle (bar 1e-5)')
        assert np.isfinite(nll).all() and err < 1e-5
        if self.argmin:
            np.testing.assert_array_equal(out['idx'], nll.argmin(axis=1))
            np.testing.assert_array_equal(out['s'], pb['cand'][out['idx']])

    def premise(self, pb, dev):
        from eks_amd import _lib
        assert _scopes(lambda: self.run(pb, dev))[:2] == ['diag_nll_summarize', 'diag_nll_assemble']
        if self.name in ('lag', 'nolag'):
            # the head + lean grid kernel and the general kernel share their scope names: with EKS_NLL_LEGACY=1 the same
            # call gives a table that differs in its low bits, or the grid kernel was not what ran
            mine = self.run(pb, dev)['nll'].clone()
            os.environ['EKS_NLL_LEGACY'] = '1'
            _lib.load().eks_knobs_reload()
            try:
                other = self.run(pb, dev)['nll'].clone()
            finally:
                del os.environ['EKS_NLL_LEGACY']
                _lib.load().eks_knobs_reload()
            assert not torch.equal(mine, other)


class NllGrad(Case):
    """eks_nll with the gradient on scalar chains: the single launch, the two-launch form, the tree of few chains."""
    entry = 'eks_nll'

    def __init__(self, name, T, K, unit, knobs):
        super().__init__(f'nll-grad-{name}-T{T}-K{K}')
        self.name, self.T, self.K, self.unit, self.knobs = name, T, K, unit, knobs

    def problem(self, variant):
        a = variant == 'a'
        arrs, y_tk, var_tk = kern._singlecam_problem(self.T, self.K, seed=(5 if a else 55) + self.T, unit=self.unit)
        rng = np.random.default_rng(1)
        s = np.exp(rng.uniform(-6, 6, self.K)) if a else np.exp(rng.uniform(-8, -6, self.K))
        return dict(arrs=arrs, y=y_tk, var=var_tk, s=s)

    def device(self, pb):
        from eks_amd import hip_ops
        arrs = pb['arrs']
        dev = dict(y=_dev(pb['y']), rconst=hip_ops.const_r(_dev(pb['var']), 1e-4), par=kern._params_dev(arrs),
                   s=_dev(pb['s'][:, None]), flags=hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs']))
        torch.cuda.synchronize()
        pb['Rc'] = dev['rconst'].cpu().numpy()
        dev['inputs'] = [dev['y'], dev['rconst'], dev['s']] + dev['par']
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        nll, g = hip_ops.nll(dev['y'], dev['rconst'], *dev['par'], dev['s'], per_keypoint=True, want_grad=True,
                             flags=dev['flags'])
        return dict(nll=nll, dnll=g)

    def check(self, pb, out):
        from oracle import eks_oracle as orc
        arrs = pb['arrs']
        ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], pb['s'], pb['Rc'],
                                   want_grad=True)
        e, eg = (np.abs(out['nll'][:, 0] - ref) / np.abs(ref)).max(), (np.abs(out['dnll'][:, 0] - gref) / np.abs(gref).max()).max()
        print(f'{self.id}: nll {e:.3g} (bar 1e-5), gradient {eg:.3g} (bar 1e-4)')
        assert e < 1e-5 and eg < 1e-4

    def premise(self, pb, dev):
        got = _scopes(lambda: self.run(pb, dev))
        assert got == (['diag_nll_grad_fused'] if self.name == 'single' else ['diag_nll_summarize', 'diag_nll_assemble']), got


class NllGeneral(Case):
    """eks_nll on general models: Q_PD (dense_score: wave or generic, the latter keeps its sums where the chunk
    elements were) and the dual-number kernels."""
    entry = 'eks_nll'

    def __init__(self, name, T, K, D, O, q_pd):
        super().__init__(f'nll-general-{name}-{"score" if q_pd else "dual"}-T{T}-D{D}-O{O}')
        self.name, self.T, self.K, self.D, self.O, self.q_pd = name, T, K, D, O, q_pd

    def problem(self, variant):
        a = variant == 'a'
        arrs, y, var = kern._dense_problem(self.T, self.K, self.D, self.O, seed=(17 if a else 71) + self.T)
        s = np.exp(np.random.default_rng(self.T).uniform(-4, 4, self.K)) * (1.0 if a else 1e-3)
        return dict(arrs=arrs, y=y, var=var, s=s)

    def device(self, pb):
        from eks_amd import _lib, hip_ops
        arrs = pb['arrs']
        flags = hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'])
        assert flags == _lib.FLAG_Q_PD
        dev = dict(y=_dev(pb['y']), rconst=hip_ops.const_r(_dev(pb['var']), 1e-4), par=kern._params_dev(arrs),
                   s=_dev(pb['s'][:, None]), flags=flags if self.q_pd else 0)
        torch.cuda.synchronize()
        pb['Rc'] = dev['rconst'].cpu().numpy()
        dev['inputs'] = [dev['y'], dev['rconst'], dev['s']] + dev['par']
        return dev

    run = NllGrad.run

    def check(self, pb, out):
        from oracle import eks_oracle as orc
        arrs = pb['arrs']
        ref, gref = orc.filter_nll(arrs['ys'], arrs['m0s'], arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs'], pb['s'], pb['Rc'],
                                   want_grad=True)
        e, eg = (np.abs(out['nll'][:, 0] - ref) / np.abs(ref)).max(), (np.abs(out['dnll'][:, 0] - gref) / np.abs(gref).max()).max()
        print(f'{self.id}: nll {e:.3g} (bar 1e-8), gradient {eg:.3g} (bar 1e-7)')
        assert e < 1e-8 and eg < 1e-7

    def premise(self, pb, dev):
        got = _scopes(lambda: self.run(pb, dev))
        if self.q_pd:
            want = ['dense_score_summarize', 'dense_score_replay']
            if self.name == 'generic':
                want.insert(1, 'dense_score_scan')
            assert got == want, got
        else:
            assert not any(g.startswith('dense_score') for g in got), got


class AdamSearch(Case):
    """eks_adam_prepare + eks_adam_run through AdamLoop (kern._adam_search builds the loop, so the body is what the
    constructor got: poisoned before prepare, never between prepare and run)."""
    entry = 'eks_adam_prepare + eks_adam_run'

    def __init__(self, name, T, K, unit, knobs, prepare, stride, bar):
        super().__init__(f'adam-{name}-T{T}-K{K}')
        self.name, self.T, self.K, self.unit, self.knobs, self.prepare, self.stride, self.bar = \
            name, T, K, unit, knobs, prepare, stride, bar

    def problem(self, variant):
        a = variant == 'a'
        arrs, y_tk, var_tk = kern._singlecam_problem(self.T, self.K, seed=(77 if a else 177) + self.T, unit=self.unit)
        u0 = np.log(np.random.default_rng(self.T + (0 if a else 1)).uniform(0.05, 50.0 if a else 0.5, self.K))
        return dict(arrs=arrs, y=y_tk, var=var_tk, u0=u0)

    def device(self, pb):
        from eks_amd import hip_ops
        arrs = pb['arrs']
        dev = dict(y=_dev(pb['y']), rc=hip_ops.const_r(_dev(pb['var']), 1e-4), par=kern._params_dev(arrs),
                   flags=hip_ops.model_flags(arrs['S0s'], arrs['As'], arrs['Cs'], arrs['Qs']))
        torch.cuda.synchronize()
        dev['inputs'] = [dev['y'], dev['rc']] + dev['par']
        return dev

    def run(self, pb, dev):
        n, st, s, nll, dnll, left = kern._adam_search(dev['y'], dev['rc'], dev['par'], dev['flags'], self.K, pb['u0'],
                                                      prepare=self.prepare)
        assert n == self.stride, (n, self.stride)                  # eks_adam_run_stride: 4096 lag sums, 64 one launch
        return dict(state=st, s=s, nll=nll, dnll=dnll, left=np.asarray(left, np.int64))

    def check(self, pb, out):
        ks = list(range(min(self.K, 4)))
        u_o, last_o, it_o = kern._oracle_adam(pb['arrs'], pb['y'], self._rc, ks, pb['u0'])
        st, s = out['state'], out['s']
        if self.name == 'lag_and_stream':
            assert np.all(st[:, 5] == 1.0)
        np.testing.assert_array_equal(st[ks, 4].astype(int), it_o)
        err = np.abs(np.log(s[ks]) - u_o).max()
        print(f'{self.id}: iterations {it_o}, log s {err:.3g} of the oracle (bar {self.bar:.0e})')
        assert err < self.bar

    def premise(self, pb, dev):
        self._rc = dev['rc']


class PupilAdam(Case):
    """eks_pupil_adam_run: tests/test_gpu_pupil_forms.py case 11 with five chains."""
    entry = 'eks_pupil_adam_run'
    K, CAP = 5, 100

    def __init__(self, positive_noise):
        super().__init__(f'pupil_adam_run-{"wave" if positive_noise else "dual"}')
        self.flag = positive_noise

    def problem(self, variant):
        seeds = [pupil.ADAM_SEEDS[(k + (0 if variant == 'a' else 3)) % 8] for k in range(self.K)]
        ch = [pupil.chain(pupil.ADAM_T, s, False) for s in seeds]
        return dict(seeds=seeds, ch=ch)

    def device(self, pb):
        from eks_amd import hip_ops
        from oracle import eks_oracle as orc
        ch, dv = pb['ch'], hip_ops.require_gpu()
        t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=dv)      # noqa: E731
        dev = dict(y=t(np.swapaxes(np.stack([c[0] for c in ch]), 0, 1), np.float32),
                   var=t(np.swapaxes(np.stack([c[1] for c in ch]), 0, 1), np.float32),
                   m0=t(np.stack([c[2] for c in ch]), np.float64), S0=t(np.stack([c[3] for c in ch]), np.float64),
                   C=t(np.tile(orc.PUPIL_C, (self.K, 1, 1)), np.float64), latent=t(np.stack([c[4] for c in ch]), np.float64))
        dev['inputs'] = [dev[k] for k in ('y', 'var', 'm0', 'S0', 'C', 'latent')]
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        loss = hip_ops.Ar1Loss(dev['y'], dev['var'], dev['m0'], dev['S0'], dev['C'], n_tan=2, positive_noise=self.flag)
        s0 = np.array([0.99, 0.98], dtype=np.float32).astype(np.float64)
        state = np.zeros((self.K, 9))
        state[:, 0:2] = np.log(s0 / (1.0 - s0))
        state[:, 6] = np.inf
        state = torch.as_tensor(state, device=dev['y'].device)
        n_active = torch.full((1,), -7, dtype=torch.int32, device=dev['y'].device)
        hip_ops.pupil_adam_step(loss, dev['latent'], state, n_active, pupil.ADAM_LR, pupil.ADAM_TOL, self.CAP, init=True)
        for _ in range(-(-self.CAP // 16)):
            hip_ops.pupil_adam_run(loss, dev['latent'], state, n_active, pupil.ADAM_LR, pupil.ADAM_TOL, self.CAP, 16)
        return dict(state=state, n_active=n_active, nll=loss.nll, dnll=loss.dnll)

    def check(self, pb, out):
        st = out['state']
        for k, seed in enumerate(pb['seeds']):
            it, done, u, last = pupil.trajectory_at(pupil.adam_oracle(seed), self.CAP)
            assert (int(st[k, 7]), bool(st[k, 8])) == (it, done), k
            np.testing.assert_allclose(st[k, 0:2], u, rtol=1e-9)
            assert abs(st[k, 6] - last) < 1e-9 * max(abs(last), 1.0)

    def premise(self, pb, dev):
        got = set(_scopes(lambda: self.run(pb, dev)))
        assert got == ({'dense_score_summarize', 'dense_score_replay'} if self.flag else {'ar1_nll'}), got


class EkfSmooth(Case):
    entry = 'eks_ekf_smooth'
    T, K, V = 37, 2, 2

    def __init__(self, want_smoother):
        super().__init__(f'ekf_smooth-{"smoother" if want_smoother else "filter"}')
        self.smoother = want_smoother

    def problem(self, variant):
        from eks_amd import synth
        prob = synth.calibrated_multicam(self.T, self.K, self.V, seed=self.T + (0 if variant == 'a' else 1))
        return dict(prob=prob, s=np.exp(np.linspace(-4, 5, self.K)) * (1.0 if variant == 'a' else 1e-3))

    def device(self, pb):
        prob = pb['prob']
        d = ekf._dev
        dev = dict(y=d(prob['y_tko'], torch.float32), var=d(prob['var_tko'], torch.float32), m0=d(prob['m0s']),
                   S0=d(prob['S0s']), A=d(prob['As']), Q=d(prob['Qs']), s=d(pb['s']), cams=d(prob['cams_packed']))
        dev['inputs'] = [dev[k] for k in ('y', 'var', 'm0', 'S0', 'A', 'Q', 's', 'cams')]
        return dev

    def run(self, pb, dev):
        from eks_amd import hip_ops
        xlin = dev['m0'][:, None, :].expand(self.K, self.T, 3).contiguous()
        ms, Vs, nll, info = hip_ops.ekf_smooth(dev['y'], dev['var'], None, dev['m0'], dev['S0'], dev['A'], dev['Q'], dev['s'],
                                               dev['cams'], xlin, max_sweeps=24, tol=1e-10, want_smoother=self.smoother)
        return dict(ms=ms, Vs=Vs, nll=nll, info=info, xlin=xlin)

    def check(self, pb, out):
        from oracle import ekf_oracle as ek
        prob, s = pb['prob'], pb['s']
        y, var = prob['y_tko'], prob['var_tko']
        assert out['info'][1] <= 1e-10 and 1 <= out['info'][0] <= 12
        h = ekf._oracle_h(prob)
        for k in range(self.K):
            args = (ekf._f32(y[:, k]), np.maximum(ekf._f32(var[:, k]), 1e-12), prob['m0s'][k], prob['S0s'][k],
                    prob['As'][k], prob['Qs'][k], s[k], h)
            mo, Vo, ll = ek.eks_smoother(*args)
            mp = ek.ekf_filter(*args)[3]
            assert np.abs(out['xlin'][k] - mp).max() < 1e-7 * max(1.0, np.abs(mp).max())
            assert abs(out['nll'][k] + ll) < 1e-9 * abs(ll)
            if self.smoother:
                assert np.abs(out['ms'][:, k] - mo).max() < 1e-5 * np.abs(mo).max()
                assert np.abs(out['Vs'][:, k] - Vo).max() < 1e-5 * np.abs(Vo).max()

    def premise(self, pb, dev):
        got = _scopes(lambda: self.run(pb, dev))
        assert got == (['ekf_filter_sweeps', 'ekf_smooth_sweep'] if self.smoother else ['ekf_filter_sweeps']), got


class EkfAffine(Case):
    """eks_ekf_affine_sweep driven to its fixed point (ekfg._abi_fixed_point: a fresh workspace every sweep)."""
    entry = 'eks_ekf_affine_sweep'
    T, K = 37, 2

    def __init__(self, want_smoother):
        super().__init__(f'ekf_affine_sweep-{"smoother" if want_smoother else "filter"}')
        self.smoother = want_smoother

    def problem(self, variant):
        from eks_amd import synth
        prob = synth.emission_problem('quad', self.T, self.K, seed=11 if variant == 'a' else 12, V=2)
        rconst = np.maximum(np.median(ekfg._f32(prob['var_tko']), axis=0), 1e-4)
        return dict(prob=prob, s=np.exp(np.linspace(-4, 5, self.K)) * (1.0 if variant == 'a' else 1e-3), rconst=rconst)

    def device(self, pb):
        prob, d = pb['prob'], ekfg._dev
        dev = dict(y=d(prob['y_tko'], torch.float32), var=d(prob['var_tko'], torch.float32), rconst=d(pb['rconst']),
                   m0=d(prob['m0s']), S0=d(prob['S0s']), A=d(prob['As']), Q=d(prob['Qs']), s=d(pb['s']))
        dev['inputs'] = [dev[k] for k in ('y', 'var', 'rconst', 'm0', 'S0', 'A', 'Q', 's')]
        return dev

    def run(self, pb, dev):
        var, rconst = (dev['var'], None) if self.smoother else (None, dev['rconst'])
        n, ch, nll, ms, Vs, xlin = ekfg._abi_fixed_point(pb['prob'], dev['y'], var, rconst, dev['m0'], dev['S0'], dev['A'],
                                                         dev['Q'], dev['s'], self.K)
        assert ch <= 1e-10 and n <= 16, (n, ch)
        return dict(nll=nll, ms=ms, Vs=Vs, xlin=xlin)

    def check(self, pb, out):
        from oracle import ekf_oracle as ek
        prob, s = pb['prob'], pb['s']
        y, var = prob['y_tko'], prob['var_tko']
        for k in range(self.K):
            if not self.smoother:
                ref = ek.ekf_nll(ekfg._f32(y[:, k]), pb['rconst'][k], prob['m0s'][k], prob['S0s'][k], prob['As'][k],
                                 prob['Qs'][k], s[k], prob['h_np'])
                assert abs(out['nll'][k] - ref) < 1e-9 * abs(ref)
                continue
            args = (ekfg._f32(y[:, k]), np.maximum(ekfg._f32(var[:, k]), 1e-12), prob['m0s'][k], prob['S0s'][k],
                    prob['As'][k], prob['Qs'][k], s[k], prob['h_np'])
            mo, Vo, ll = ek.eks_smoother(*args)
            mp = ek.ekf_filter(*args)[3]
            assert np.abs(out['xlin'][k] - mp).max() < 1e-7 * max(1.0, np.abs(mp).max())
            assert np.abs(out['ms'][:, k] - mo).max() < 1e-5 * np.abs(mo).max()
            assert np.abs(out['Vs'][:, k] - Vo).max() < 1e-5 * np.abs(Vo).max()
            assert abs(out['nll'][k] + ll) < 1e-9 * abs(ll)


def _cases():
    cs = []
    # eks_smooth, scalar chains: (700, 5, 2) packed lanes; 17 x 2 = 34 chains, the narrowest the fused scan takes; 35 x 2 =
    # 70 chains through the three-kernel scan; elements kept (EKS_REPLAY_RECOMPUTE=0) and summarised again (1)
    for unit in (True, False):
        cs.append(SmoothChains('packed', 700, 5, 2, unit, {}))
        for rc in ('0', '1'):
            cs.append(SmoothChains('fused', 700, 17, 2, unit, {'EKS_REPLAY_RECOMPUTE': rc}))
            cs[-1].id += f'-recompute{rc}'
        cs.append(SmoothChains('unfused', 700, 35, 2, unit, {'EKS_SMOOTH_UNFUSED': '1'}))
    # eks_smooth, general models
    cs.append(SmoothGeneral('wave', 131, 3, 3, 8, False, {}))
    cs.append(SmoothGeneral('runs', 131, 1100, 2, 6, False, {}))
    cs.append(SmoothGeneral('tree', 131, 1100, 2, 6, False, {'EKS_DENSE_TREE_SCAN': '1'}))     # generic, wide covers
    cs.append(SmoothGeneral('generic', 100, 2, 6, 8, False, {}))                               # generic, wide does not
    cs.append(SmoothGeneral('blocks', 700, 2, 4, 8, False, {'EKS_DENSE_CHUNK': '8'}))          # 88 chunks: two scan blocks
    for op in ('smooth_tv', 'increments', 'em_stats', 'innovations'):
        for i, (K, D) in enumerate(CHAINS):
            for j, T in enumerate(T_LANES):
                cs.append(ScalarChains(op, T, K, D, 'unit' if (i + j) % 2 else ('general' if op == 'smooth_tv' else 'decay')))
        for T in (B_DENSE + 1, 64 * B_DENSE + 1):
            cs.append(GeneralModel(op, T))
    for n_draws in (1, 3):
        for i, (K, D) in enumerate(CHAINS):
            for j, T in enumerate(T_LANES):
                cs.append(SampleChains(T, K, D, bool((i + j) % 2), n_draws))
        for T in (B_DENSE + 1, 64 * B_DENSE + 1):
            cs.append(SampleGeneral(T, n_draws))
    cs += [EmLoop('unit'), EmLoop('decay')]
    cs += [ConstR(2, 5), ConstR(1025, 66), ConstR(CONST_R_LIST_T, 2)]
    # the grid: (2100, 64) is just past the shortest sequence the head + lean kernel takes (two chunks, the shared-lag
    # form in the second), EKS_NLL_NOLAG=1 the round-4 summaries, EKS_NLL_LEGACY=1 the general kernel; (700, 40): too
    # short for chunks past the first, the staged general kernel by itself
    cs.append(NllGrid('lag', 2100, 64, True, {}))
    cs.append(NllGrid('nolag', 2100, 64, True, {'EKS_NLL_NOLAG': '1'}))
    cs.append(NllGrid('legacy', 2100, 64, True, {'EKS_NLL_LEGACY': '1'}))
    cs.append(NllGrid('staged', 700, 40, False, {}))
    cs.append(NllGrid('lag', 2100, 64, True, {}, argmin=True))
    cs.append(NllGrid('staged', 1500, 8, True, {}, argmin=True))
    cs.append(NllGrad('single', 2111, 33, False, {}))
    cs.append(NllGrad('two', 2111, 33, False, {'EKS_NLL_GRAD_UNFUSED': '1'}))
    cs.append(NllGrad('tree', 1500, 3, False, {}))
    for q_pd in (True, False):
        cs.append(NllGeneral('wave', 131, 2, 2, 2, q_pd))
        cs.append(NllGeneral('generic', 100, 2, 6, 8, q_pd))
    # lag sums with chains that leave the lag range and stream (ppm as in test_adam_chains_outside_the_lag_range_..), the
    # pass over y enqueued by eks_adam_prepare; and the whole loop in one launch
    cs.append(AdamSearch('lag_and_stream', 3000, 5, False, {'EKS_ADAM_LAG_RHO_PPM': '300000'}, True, 4096, 1e-6))
    cs.append(AdamSearch('one_launch', 700, 3, False, {}, False, 64, 1e-5))
    cs += [PupilAdam(True), PupilAdam(False)]
    cs += [EkfSmooth(True), EkfSmooth(False), EkfAffine(True), EkfAffine(False)]
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
_PROBLEMS, _ZERO = {}, {}


def _problem(case, variant):
    key = (case.id, variant)
    if key not in _PROBLEMS:
        if len(_PROBLEMS) > 6:
            _PROBLEMS.clear()
        _PROBLEMS[key] = case.problem(variant)
    return _PROBLEMS[key]


def _tensors(out):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.clone())
            for k, v in out.items() if v is not None}


def _call(case, monkeypatch, fill, pb, dev):
    """One call of the case on guarded workspaces that start as `fill`: outputs (clones), the guard object."""
    gw = guarded_workspaces(monkeypatch, fill)
    before = [t.clone() for t in dev['inputs']]
    out = case.run(pb, dev)
    torch.cuda.synchronize()
    out = _tensors(out)
    gw.assert_intact()
    for i, (a, b) in enumerate(zip(before, dev['inputs'])):
        assert same_bits(a, b), f'{case.entry}: input {i} of the call changed'
    return out, gw


def _assert_same(case, what, ref, got):
    assert sorted(ref) == sorted(got), (case.id, what)
    for name in ref:
        assert same_bits(ref[name], got[name]), f'{case.entry} ({case.id}): {name} on {what} differs from the 0x00 workspace'


def _setup(case, set_knob):
    for k, v in case.knobs.items():
        set_knob(k, v)
    pb = _problem(case, 'a')
    return pb, case.device(pb)


def _zero_run(case, monkeypatch, pb, dev):
    if case.id not in _ZERO:
        out, gw = _call(case, monkeypatch, 0x00, pb, dev)
        case.after_zero(gw)
        _ZERO[case.id] = out
    return _ZERO[case.id]


# ==========================================================================================================================
# 1. workspaces of zeros and stale workspaces
# ==========================================================================================================================
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_zero_and_stale_workspace(case, set_knob, monkeypatch):
    pb, dev = _setup(case, set_knob)
    case.premise(pb, dev)
    zero = _zero_run(case, monkeypatch, pb, dev)
    # the body the same entry point leaves on another problem of the same shape (another seed, the other s regime)
    pb_b = _problem(case, 'b')
    _, gw_b = _call(case, monkeypatch, 0x00, pb_b, case.device(pb_b))
    stale, _ = _call(case, monkeypatch, stale_fill(gw_b.bodies()), pb, dev)
    _assert_same(case, 'the body the same entry point left behind', zero, stale)
    if case.partner is not None:      # .. and the one the entry point it shares its workspace size with leaves
        other = case.partner()
        pb_o = other.problem('b')
        _, gw_o = _call(other, monkeypatch, 0x00, pb_o, other.device(pb_o))
        sizes = [g.nbody for g in gw_o.buffers], [g.nbody for g in gw_b.buffers]
        assert sizes[0] == sizes[1], (case.entry, other.entry, sizes)
        stale, _ = _call(case, monkeypatch, stale_fill(gw_o.bodies()), pb, dev)
        _assert_same(case, f'the body {other.entry} left behind', zero, stale)


def test_one_workspace_serves_em_stats_innovations_and_smooth_tv_in_turn(monkeypatch):
    """eks_em_stats, eks_innovations and eks_smooth_tv share diag_em_workspace_bytes: ONE guarded body is handed to the
    three in turn, on three different problems of one shape, twice round; each call gives the bits it gives on a fresh
    0x00 body."""
    from eks_amd import hip_ops
    T, K, D = 33 * B + 5, 65, 1
    cases = [ScalarChains(op, T, K, D, 'decay' if op != 'smooth_tv' else 'general') for op in ScalarChains.SHARED]
    pbs = []
    for i, c in enumerate(cases):
        pb = c.problem('a' if i != 1 else 'b')
        pbs.append((pb, c.device(pb)))
    fresh, sizes = [], []
    for c, (pb, dev) in zip(cases, pbs):
        out, gw = _call(c, monkeypatch, 0x00, pb, dev)
        fresh.append(out)
        sizes.append(gw.buffers[-1].nbody)
    assert len(set(sizes)) == 1, sizes             # (the largest of the three is every one of them)
    gw = guarded_workspaces(monkeypatch, 0x00)
    shared = gw(max(sizes), 'cuda')
    monkeypatch.setattr(hip_ops, '_workspace', lambda n, device: shared[:max(int(n), 256)])
    for rnd in range(2):
        for c, (pb, dev), ref in zip(cases, pbs, fresh):
            out = _tensors(c.run(pb, dev))
            torch.cuda.synchronize()
            _assert_same(c, f'the shared body, round {rnd + 1}', ref, out)
            gw.assert_intact()


# ==========================================================================================================================
# 2. output guards
# ==========================================================================================================================
def _outputs(specs, offset, row_elems):
    """name -> GuardedOutput for every (name, shape, dtype) whose shape is not None."""
    return {n: guarded_output(shape, dt, offset=offset, row_elems=row_elems, name=n) for n, shape, dt in specs
            if shape is not None}


def _ptrs(outs, names):
    from eks_amd import hip_ops
    return [hip_ops._ptr(outs[n].tensor if n in outs else None) for n in names]


def _raw(entry, query, dims_args, ins, out_ptrs, *extra):
    """The C entry point itself on a guarded workspace: ins = device tensors, out_ptrs = pointers (NULL where absent)."""
    from eks_amd import _lib, hip_ops
    lib = _lib.load()
    dims = _lib.EksDims(*[int(x) for x in dims_args])
    ws = hip_ops._workspace(getattr(lib, query)(ctypes.byref(dims)), 'cuda')
    rc = getattr(lib, entry)(ctypes.byref(dims), *[hip_ops._ptr(t) for t in ins], *extra, *out_ptrs, hip_ops._ptr(ws),
                             ws.numel(), hip_ops._stream())
    torch.cuda.synchronize()
    return rc


def _intact(outs, gw):
    for o in outs.values():
        o.assert_intact()
    gw.assert_intact()


# scalar chains: K D in {1, 3, 65} with diagonal Vs; full Vs rows at D = 3 and 8 (PointerStore<3>, <8>)
GUARD_CHAINS = [(1, 1, True), (3, 1, True), (65, 1, True), (1, 3, False), (2, 8, False)]
GUARD_T = (1, B - 1, B + 1)
GUARD_T_DENSE = (1, B_DENSE - 1, B_DENSE + 1)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('K,D,vs_diag', GUARD_CHAINS)
@pytest.mark.parametrize('prepared', [False, True])
def test_output_guards_smooth_on_chains(K, D, vs_diag, prepared, offset, monkeypatch):
    from eks_amd import hip_ops
    gw = guarded_workspaces(monkeypatch, 0xFF)
    for T in GUARD_T:
        for unit in (True, False):
            p = smooth_problem(T, K, D, seed=T + K + D, unit=unit)
            vshape = (T, K, D) if vs_diag else (T, K, D, D)
            outs = _outputs([('ms', (T, K, D), torch.float32), ('Vs', vshape, torch.float32)], offset, K * D * D)
            args = (_dev(p['y']), _dev(p['var']), *[_dev(p[k], torch.float64) for k in PARAMS])
            kw = dict(flags=hip_ops.model_flags(p['S0'], p['A'], p['C'], p['Q']), vs_diag=vs_diag,
                      out=(outs['ms'].tensor, outs['Vs'].tensor))
            ms, Vs = hip_ops.PreparedSmooth(*args, **kw)() if prepared else hip_ops.smooth(*args, **kw)
            _intact(outs, gw)
            win._assert_oracle(('guards', T, K, D, unit), p, ms, Vs, vs_diag)
            if not vs_diag:
                off = ~torch.eye(D, dtype=torch.bool, device=Vs.device)
                assert not bool(Vs[:, :, off].any()), 'off-diagonal entries are not zero'


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('K,D,vs_diag', GUARD_CHAINS)
def test_output_guards_smooth_tv_on_chains(K, D, vs_diag, offset):
    from eks_amd import _lib
    for T in GUARD_T:
        for kind in ('unit', 'general'):
            pb = tv.session(T, K, D, 2.0, kind, seed=T + K + D)
            w = random_w(np.random.default_rng(T + K), (T, K) if T % 2 else (T,))
            vshape = (T, K, D) if vs_diag else (T, K, D, D)
            outs = _outputs([('ms', (T, K, D), torch.float32), ('Vs', vshape, torch.float32)], offset, K * D * D)
            ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
            flags = inc.diag_flags(pb) | (_lib.FLAG_VS_DIAG if vs_diag else 0)
            assert tv.raw_call((K, T, D, D, flags), ins, _dev(w), w.ndim == 2, outs['ms'].tensor, outs['Vs'].tensor) == 0
            for o in outs.values():
                o.assert_intact()
            ms, Vs = outs['ms'].tensor.cpu().numpy().reshape(T, K * D), outs['Vs'].tensor.cpu().numpy()
            if not vs_diag:
                assert not Vs[:, :, ~np.eye(D, dtype=bool)].any(), 'off-diagonal entries are not zero'
                Vs = np.diagonal(Vs, axis1=2, axis2=3)
            tv.check_scalar(f'guards T={T} N={K * D} {kind}', pb, w, (ms, Vs.reshape(T, K * D)))


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 1), (65, 1), (1, 3)])
def test_output_guards_increments_em_stats_and_innovations_on_chains(K, D, offset, monkeypatch):
    from eks_amd import _lib
    gw = guarded_workspaces(monkeypatch, 0xFF)
    f32, f64 = torch.float32, torch.float64
    for T in GUARD_T:
        pb = inc.edge_session(T, K, D, 2.0, 'decay' if T % 2 else 'unit', seed=T + K + D)
        ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
        dims, N = (K, T, D, D, inc.diag_flags(pb) | _lib.FLAG_VS_DIAG), K * D
        names = ('ms', 'Vs', 'lag1', 'dmean', 'dV')
        outs = _outputs([(n, (T, K, D), f32) for n in names], offset, N)
        assert _raw('eks_smooth_increments', 'eks_smooth_increments_workspace_bytes', dims, ins, _ptrs(outs, names)) == 0
        _intact(outs, gw)
        inc.check_scalar(f'guards T={T} N={N}', pb, {n: o.tensor.cpu().numpy().reshape(T, N) for n, o in outs.items()})
        outs = _outputs([('Sw', (K, D), f64)], offset, N)
        assert _raw('eks_em_stats', 'eks_em_stats_workspace_bytes', dims, ins, _ptrs(outs, ('Sw',))) == 0
        _intact(outs, gw)
        em.check_scalar(f'guards T={T} N={N}', pb, outs['Sw'].tensor.cpu().numpy().reshape(N))
        names = ('innov', 'innov_var', 'nis', 'frame_ll', 'loglik')
        outs = _outputs([('innov', (T, K, D), f32), ('innov_var', (T, K, D), f32), ('loglik', (K, D), f64)], offset, N)
        assert innov.raw_call(dims[:4] + (inc.diag_flags(pb),), ins, [outs[n].tensor if n in outs else None for n in names]) == 0
        for o in outs.values():
            o.assert_intact()
        innov.check_scalar(f'guards T={T} N={N}', pb, dict(v=outs['innov'].tensor.cpu().numpy().reshape(T, N),
                                                           S=outs['innov_var'].tensor.cpu().numpy().reshape(T, N),
                                                           ll=outs['loglik'].tensor.cpu().numpy().reshape(N)))


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('K,D', [(1, 1), (3, 1), (65, 1), (1, 3)])
def test_output_guards_sample_on_chains(K, D, offset, monkeypatch):
    from eks_amd import hip_ops
    gw = guarded_workspaces(monkeypatch, 0xFF)
    S, N = 3, K * D
    for T in GUARD_T:
        pb = make_chains(T, K, D, 0.7 if T % 2 else 2.0, not T % 2, seed=1000 * N + T)
        z = np.random.default_rng(N + T).normal(size=(S, T, N)).astype(np.float32)
        out = guarded_output((S, T, K, D), torch.float32, offset=offset, row_elems=N, name='draws')
        dr, ms = hip_ops.sample(_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D)),
                                *(_dev(pb['par'][k]) for k in PARAMS), S, flags=samp._flags(pb),
                                noise=_dev(z.reshape(S, T, K, D)), want_mean=True, out=out.tensor)
        assert dr.data_ptr() == out.tensor.data_ptr()
        _intact({'draws': out}, gw)
        check_sample_chains(f'guards T={T} N={N}', pb, dr.cpu().numpy().reshape(S, T, N), ms.cpu().numpy().reshape(T, N), z)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('K', [1, 3])
def test_output_guards_general_models_d6_o12(K, offset, monkeypatch):
    """D = 6, O = 12: rows of 6, 36 and 12 floats; the last chunk holds one frame, fifteen, or there is one frame."""
    from eks_amd import hip_ops
    gw = guarded_workspaces(monkeypatch, 0xFF)
    D, O, f32, f64 = 6, 12, torch.float32, torch.float64
    M = inc.stable(dense_case(K, D, O, False, seed=60 + K))
    par = [_dev(M[k]) for k in PARAMS]
    for T in GUARD_T_DENSE:
        y, var = inc.dense_session(M, T, O, seed=T)
        ins, row = [_dev(y), _dev(var)] + par, K * D * D
        # eks_smooth (out=) and eks_smooth_tv at w = 1: the same reference
        w = np.ones(T, np.float32)
        outs = _outputs([('ms', (T, K, D), f32), ('Vs', (T, K, D, D), f32)], offset, row)
        hip_ops.smooth(*ins, flags=0, out=(outs['ms'].tensor, outs['Vs'].tensor))
        torch.cuda.synchronize()
        _intact(outs, gw)
        tv.check_dense(f'guards eks_smooth T={T} K={K}', M, y, var, w, (outs['ms'].tensor.cpu().numpy(), outs['Vs'].tensor.cpu().numpy()))
        w = random_w(np.random.default_rng(T), (T, K))
        outs = _outputs([('ms', (T, K, D), f32), ('Vs', (T, K, D, D), f32)], offset, row)
        assert tv.raw_call((K, T, D, O, 0), ins, _dev(w), True, outs['ms'].tensor, outs['Vs'].tensor) == 0
        for o in outs.values():
            o.assert_intact()
        tv.check_dense(f'guards eks_smooth_tv T={T} K={K}', M, y, var, w, (outs['ms'].tensor.cpu().numpy(), outs['Vs'].tensor.cpu().numpy()))
        names = ('ms', 'Vs', 'lag1', 'dmean', 'dV')
        outs = _outputs([(n, (T, K, D) if n in ('ms', 'dmean') else (T, K, D, D), f32) for n in names], offset, row)
        assert _raw('eks_smooth_increments', 'eks_smooth_increments_workspace_bytes', (K, T, D, O, 0), ins, _ptrs(outs, names)) == 0
        _intact(outs, gw)
        inc.check_dense(f'guards increments T={T} K={K}', M, y, var, {n: o.tensor.cpu().numpy() for n, o in outs.items()}, False)
        outs = _outputs([('Sw', (K, D, D), f64)], offset, row)
        assert _raw('eks_em_stats', 'eks_em_stats_workspace_bytes', (K, T, D, O, 0), ins, _ptrs(outs, ('Sw',))) == 0
        _intact(outs, gw)
        em.check_dense(f'guards em_stats T={T} K={K}', M, y, var, outs['Sw'].tensor.cpu().numpy(), False)
        names = innov.DENSE_OUT
        outs = _outputs([('innov', (T, K, O), f32), ('innov_var', (T, K, O), f32), ('nis', (T, K), f32),
                         ('frame_ll', (T, K), f32), ('loglik', (K,), f64)], offset, K * O)
        assert innov.raw_call((K, T, D, O, 0), ins, [outs[n].tensor for n in names]) == 0
        for o in outs.values():
            o.assert_intact()
        innov.check_dense(f'guards innovations T={T} K={K}', M, y, var, {n: o.tensor.cpu().numpy() for n, o in outs.items()})


@pytest.mark.parametrize('offset', [0, 1])
def test_output_guards_sample_on_a_general_model(offset, monkeypatch):
    from eks_amd import hip_ops
    gw = guarded_workspaces(monkeypatch, 0xFF)
    K, D, O, S = 3, 3, 4, 3
    M = sampd.stable_model(K, D, O, 300)
    for T in GUARD_T_DENSE:
        y, var = sampd.session(M, T, O, 302 + T)
        z = np.random.default_rng(T).normal(size=(S, T, K, D + O)).astype(np.float32)
        out = guarded_output((S, T, K, D), torch.float32, offset=offset, row_elems=K * D, name='draws')
        dr, ms = hip_ops.sample(_dev(y), _dev(var), *(_dev(M[k]) for k in PARAMS), S, flags=0, noise=_dev(z), want_mean=True,
                                out=out.tensor)
        _intact({'draws': out}, gw)
        sampd.check_parity(f'guards T={T}', ('guards', T, offset), M, y, var, dr.cpu().numpy(), ms.cpu().numpy(), z,
                           np.arange(K))


# ---- NULL optional outputs: every subset the header allows ----------------------------------------------------------------
INC_NAMES = ('ms', 'Vs', 'lag1', 'dmean', 'dV')
INC_NEW_SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(INC_NAMES[2:], r)]


def _subset_call(entry, query, dims, ins, specs, names, present, row, offset, gw):
    outs = _outputs([(n, sh, dt) for n, sh, dt in specs if n in present], offset, row)
    assert _raw(entry, query, dims, ins, _ptrs(outs, names)) == 0, (entry, present)
    _intact(outs, gw)
    return {n: o.tensor.clone() for n, o in outs.items()}


@pytest.mark.parametrize('smooth_outputs', [('ms', 'Vs'), ('ms',), ('Vs',), ()])
@pytest.mark.parametrize('model', ['chains', 'general'])
def test_null_outputs_of_smooth_increments(model, smooth_outputs, monkeypatch):
    """ms and Vs may each be NULL, any of lag1 / dmean / dV but not all three: 4 x 7 subsets.  The outputs that remain
    keep their bits and their guards; the full call passes the file's reference check."""
    from eks_amd import _lib
    gw = guarded_workspaces(monkeypatch, 0xFF)
    f32 = torch.float32
    if model == 'chains':
        T, K, D = B + 1, 5, 2
        pb = inc.edge_session(T, K, D, 2.0, 'decay', seed=12)
        ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
        dims, row = (K, T, D, D, inc.diag_flags(pb) | _lib.FLAG_VS_DIAG), K * D
        specs = [(n, (T, K, D), f32) for n in INC_NAMES]
    else:
        T, K, D, O = B_DENSE + 1, 3, 3, 4
        M = inc.stable(dense_case(K, D, O, False, seed=3))
        y, var = inc.dense_session(M, T, O, seed=1)
        ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
        dims, row = (K, T, D, O, 0), K * D * D
        specs = [(n, (T, K, D) if n in ('ms', 'dmean') else (T, K, D, D), f32) for n in INC_NAMES]
    call = lambda present: _subset_call('eks_smooth_increments', 'eks_smooth_increments_workspace_bytes', dims, ins, specs,  # noqa: E731
                                        INC_NAMES, present, row, 1, gw)
    full = call(INC_NAMES)
    host = {n: v.cpu().numpy() for n, v in full.items()}
    if model == 'chains':
        inc.check_scalar('full call', pb, {n: v.reshape(T, K * D) for n, v in host.items()})
    else:
        inc.check_dense('full call', M, y, var, host, False)
    for new in INC_NEW_SUBSETS:
        part = call(smooth_outputs + new)
        assert sorted(part) == sorted(smooth_outputs + new)
        for n, v in part.items():
            assert same_bits(v, full[n]), f'{n} with only {smooth_outputs + new} present'


@pytest.mark.parametrize('model,r', [('chains', 1), ('chains', 2), ('general', 1), ('general', 2), ('general', 3),
                                     ('general', 4)])
def test_null_outputs_of_innovations(model, r, monkeypatch):
    """Every subset of r outputs (scalar chains: innov, innov_var, loglik; general models: all five)."""
    gw = guarded_workspaces(monkeypatch, 0xFF)
    f32, f64 = torch.float32, torch.float64
    names = innov.DENSE_OUT
    if model == 'chains':
        T, K, D = B + 1, 21, 3
        pb = inc.edge_session(T, K, D, 2.0, 'decay', seed=12)
        ins = [_dev(pb['y'].reshape(T, K, D)), _dev(pb['var'].reshape(T, K, D))] + [_dev(pb['par'][k]) for k in PARAMS]
        dims, row, allowed = (K, T, D, D, inc.diag_flags(pb)), K * D, innov.SCALAR_OUT
        specs = [('innov', (T, K, D), f32), ('innov_var', (T, K, D), f32), ('loglik', (K, D), f64)]
    else:
        T, K, D, O = B_DENSE + 1, 3, 3, 4
        M = inc.stable(dense_case(K, D, O, False, seed=3))
        y, var = inc.dense_session(M, T, O, seed=1)
        ins = [_dev(y), _dev(var)] + [_dev(M[k]) for k in PARAMS]
        dims, row, allowed = (K, T, D, O, 0), K * O, innov.DENSE_OUT
        specs = [('innov', (T, K, O), f32), ('innov_var', (T, K, O), f32), ('nis', (T, K), f32), ('frame_ll', (T, K), f32),
                 ('loglik', (K,), f64)]
    call = lambda present: _subset_call('eks_innovations', 'eks_innovations_workspace_bytes', dims, ins, specs, names,  # noqa: E731
                                        present, row, 1, gw)
    full = call(allowed)
    host = {n: v.cpu().numpy() for n, v in full.items()}
    if model == 'chains':
        innov.check_scalar('full call', pb, dict(v=host['innov'].reshape(T, -1), S=host['innov_var'].reshape(T, -1),
                                                 ll=host['loglik'].reshape(-1)))
    else:
        innov.check_dense('full call', M, y, var, host)
    for present in itertools.combinations(allowed, r):
        part = call(present)
        assert sorted(part) == sorted(present)
        for n, v in part.items():
            assert same_bits(v, full[n]), f'{n} with only {present} present'


# ==========================================================================================================================
# 3. workspaces of 0xFF bytes
# ==========================================================================================================================
@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_poisoned_workspace(case, set_knob, monkeypatch):
    pb, dev = _setup(case, set_knob)
    case.premise(pb, dev)
    zero = _zero_run(case, monkeypatch, pb, dev)
    poisoned, _ = _call(case, monkeypatch, 0xFF, pb, dev)
    _assert_same(case, 'a workspace of 0xFF bytes', zero, poisoned)
    case.check(pb, _host(poisoned))
    _ZERO.pop(case.id, None)
