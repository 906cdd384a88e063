"""The general-model kernels, one compiled form at a time (a helper module for tests/test_dense_forms_cpu.py and
tests/test_gpu_dense_forms.py; not a conftest).

Three things live here:

  * a plain-Python transcription of the host's dispatch (eks_amd/csrc/eks_dense.hip dense_path, dense_chunk and the
    three workspace layouts; eks_dense_wave.hip dw_units, dw_chunk_frames, dense_wave_covers and the `two` decision of
    dense_wave_run; eks_dense_wide.hip dense_wide_covers and the scan plan), which turns (T, K, D, O, mode, knobs) into
    a form label: ('wave', D, O, SUBS, B), ('runs', D, O, B) or ('generic', D, B);
  * the hand-written list of the instantiations the macros EKS_DW*, EKS_WS / EKS_WR and EKS_DISPATCH_D compile;
  * the case table: the smallest shapes that select each form and still have a ragged edge.

The transcription is held against the library by the CPU test (through the size queries) and by the GPU test (through
the profile scopes of a call), so a change of the dispatch that this file does not follow fails there."""
import numpy as np

SMOOTH, SCORE = 0, 1           # MODE of the wave kernels; the runs kernels' SCORE flag


# ---------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------
def dense_problem(T, K, D, O, seed):
    """A random-walk session seen through a random C with per-frame variances: (arrs for the oracle, y, var (T, K, O)
    float32).  A = I; general_a() below gives the non-identity variant."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((K, T, D)) * 0.5, axis=1)
    C = rng.standard_normal((K, O, D))
    var = (rng.gamma(2.0, 0.4, (T, K, O)) + 0.02).astype(np.float32)
    y = np.einsum('kod,ktd->tko', C, x) + rng.standard_normal((T, K, O)) * np.sqrt(var)
    y = y.astype(np.float32)
    L = rng.standard_normal((K, D, D)) * 0.3
    Q = L @ np.swapaxes(L, 1, 2) + 0.2 * np.eye(D)
    Q = Q / np.abs(Q).max(axis=(1, 2), keepdims=True)
    S0 = np.eye(D) * rng.uniform(1.0, 5.0, (K, D))[:, :, None]
    A = np.tile(np.eye(D), (K, 1, 1))
    m0 = np.zeros((K, D))
    return dict(ys=np.transpose(y, (1, 0, 2)).astype(np.float64), m0s=m0, S0s=S0, As=A, Cs=C, Qs=Q,
                ensemble_vars=var.astype(np.float64)), y, var


def rel(a, b, axis_scale=None):
    """max |a-b| relative to the per-keypoint max magnitude of b (BASELINE's 'relative', H4)."""
    sc = np.abs(b).max(axis=axis_scale, keepdims=True) if axis_scale is not None else np.abs(b).max()
    return float((np.abs(a - b) / np.maximum(sc, 1e-300)).max())


def general_a(arrs):
    """The suite's non-identity dynamics: 0.97 A + 0.02 noise, in place."""
    K, D = arrs['As'].shape[:2]
    arrs['As'] = arrs['As'] * 0.97 + 0.02 * np.random.default_rng(9).standard_normal((K, D, D))


# The features that always take the generic organisation (eks_smooth_tv, _robust, _jumps, _increments, eks_em_stats,
# eks_innovations) at the accepted width: O = 64, an odd O past 32 under D = 6, and the smallest odd O that is neither
# wave nor runs.  Their tests run these pairs at K = 3 only (seconds, not minutes, of float64 reference).
WIDE_PAIRS = [(1, 64), (6, 33), (3, 5)]
# The models of those tests are seeded 10 D + K; the wide pairs take the third seed after it: of the first six it is
# the one at which the two float64 reference forms of every file agree best at (6, 33) - 5e-12 or better, against
# 3e-11 at the seed itself, which would leave less than three decades under the 1e-8 cap of the bar they set
# (tests/test_dense_forms_cpu.py holds the inputs to 1e-11).
WIDE_SEED_SHIFT = 3


def general_grid(pairs, Ks=(1, 3, 65)):
    """(D, O, K) of a test_general_models_against_... test: its own pairs at every K, the wide pairs at K = 3."""
    return [(D, O, K) for K in Ks for D, O in pairs] + [(D, O, 3) for D, O in WIDE_PAIRS]


def general_seed(D, O, K):
    return 10 * D + K + (WIDE_SEED_SHIFT if (D, O) in WIDE_PAIRS else 0)


# ---------------------------------------------------------------------------------------------
# the dispatch, transcribed
# ---------------------------------------------------------------------------------------------
def _knob(knobs, name):
    return int((knobs or {}).get(name, 0))


def _cdiv(a, b):
    return -(-a // b)


def _align(n, a=256):
    return _cdiv(n, a) * a


def dw_units(T, K, B):
    """(keypoint, 64-chunk) units of the wave kernels at B frames per lane."""
    return K * _cdiv(_cdiv(T, B), 64)


DW_UNITS_SHORT = 160           # kDwUnitsShort: natural choice of a short chunk
DW_UNITS_PAIR = 256            # kDwUnitsPair: more units take four-wave workgroups, which exist for 8 frames only
DW_UNITS_MAX = 1024            # dense_wave_covers


def dw_chunk_frames(T, K, O, knobs=None):
    """Frames per lane of the wave kernels, EKS_DW_CHUNK included: a forced 2 or 4 holds while its units fit the
    one-pair workgroups, the only form the short chunks are compiled in."""
    if O > 8:
        return 8
    forced = _knob(knobs, 'EKS_DW_CHUNK')
    if forced == 8 or (forced in (2, 4) and dw_units(T, K, forced) <= DW_UNITS_PAIR):
        return forced
    if forced in (2, 4):
        return 8
    if dw_units(T, K, 2) <= DW_UNITS_SHORT:
        return 2
    if dw_units(T, K, 4) <= DW_UNITS_SHORT:
        return 4
    return 8


def dense_wave_covers(T, K, D, O, knobs=None):
    if _knob(knobs, 'EKS_DENSE_LEGACY'):
        return False
    if not ((D in (2, 3) and O in (2, 4, 6, 8)) or (D == 3 and O in (10, 12))):
        return False
    return dw_units(T, K, dw_chunk_frames(T, K, O, knobs)) <= DW_UNITS_MAX


def dense_wave_two(T, K, O, knobs=None):
    """dense_wave_run: four-wave workgroups (SUBS = 2)."""
    return dw_units(T, K, dw_chunk_frames(T, K, O, knobs)) > DW_UNITS_PAIR and O <= 8


def dense_chunk(T, K, knobs=None):
    forced = _knob(knobs, 'EKS_DENSE_CHUNK')
    if 2 <= forced <= 256:
        return forced
    return 16 if K * _cdiv(T, 16) <= (1 << 18) else 32


def dense_wide_covers(D, O, B, knobs=None):
    return D in (2, 3) and O in (2, 4, 6, 8) and B <= 32 and B % 4 == 0 and not _knob(knobs, 'EKS_DENSE_LEGACY')


def dense_path(T, K, D, O, knobs=None):
    if dense_wave_covers(T, K, D, O, knobs):
        return 'wave'
    if dense_wide_covers(D, O, dense_chunk(T, K, knobs), knobs) and not _knob(knobs, 'EKS_DENSE_TREE_SCAN'):
        return 'runs'
    return 'generic'


def dense_form(T, K, D, O, mode=SMOOTH, knobs=None):
    """The form label of eks_smooth (mode SMOOTH) or of eks_nll's score form (mode SCORE: one s per keypoint, gradient
    wanted, EKS_FLAG_Q_PD); None where the score form does not exist (T < 2: the dual-number kernels serve)."""
    if not (1 <= D <= 6 and 1 <= O <= 64):
        return None
    if mode == SCORE and T < 2:
        return None
    path = dense_path(T, K, D, O, knobs)
    if path == 'wave':
        cb = dw_chunk_frames(T, K, O, knobs)
        subs = 2 if dense_wave_two(T, K, O, knobs) else 1
        return ('wave', D, O, subs, cb if (subs == 1 and O <= 8 and cb in (2, 4)) else 8)
    if path == 'runs':
        return ('runs', D, O, dense_chunk(T, K, knobs))
    return ('generic', D, dense_chunk(T, K, knobs))


def _nv(D):
    return 3 * D * D + 2 * D + 1          # doubles of a chunk element


def _rec(D):
    return D + D * D                      # doubles of a belief / information record


def dw_layout_bytes(T, K, D, cb):
    nc = _cdiv(T, cb)
    nwb = _cdiv(nc, 64)
    doubles = (nc * K * _nv(D), nc * K * _nv(D), nwb * K * _nv(D), K * _rec(D), nwb * K * (1 + 2 * D))
    return sum(_align(8 * d) for d in doubles)


def wide_scan_plan(nc):
    """eks_dense_wide.hip wide_scan_plan: (levels, rows per run, rows per level)."""
    best, best_cost = None, 1e300
    for L in range(0, 7):
        for R in range(2, 33):
            n = [nc]
            for _ in range(L):
                n.append(_cdiv(n[-1], R))
            if n[L] <= 64:
                cost = L * ((R - 1) * 4.1 + 8.0) + sum(0.032 * v for v in n[1:])
                if cost < best_cost:
                    best, best_cost = (L, R, n), cost
            if L == 0:
                break
    return best


def runs_layout_bytes(K, D, nc):
    scratch = sum(wide_scan_plan(nc)[2][1:]) * K * (_nv(D) + 2 * _rec(D))
    doubles = (nc * K * _nv(D), nc * K * _rec(D), nc * K * _rec(D), scratch, K * _rec(D), nc * K, nc * K)
    return sum(_align(8 * d) for d in doubles)


def generic_layout_bytes(T, K, D, nc):
    nblk = _cdiv(nc, 64)
    doubles = (nc * K * _nv(D),) * 3 + (nblk * K * _nv(D), nblk * K * _rec(D), nblk * K * _rec(D), T * K * _rec(D),
                                        K * _rec(D))
    return sum(_align(8 * d) for d in doubles)


def smooth_workspace_bytes(T, K, D, O, knobs=None):
    """dense_smooth_workspace_bytes (and dense_score_workspace_bytes, which is the same number)."""
    path = dense_path(T, K, D, O, knobs)
    if path == 'wave':
        return dw_layout_bytes(T, K, D, dw_chunk_frames(T, K, 0, knobs))
    B = dense_chunk(T, K, knobs)
    nc = _cdiv(T, B)
    return runs_layout_bytes(K, D, nc) if path == 'runs' else generic_layout_bytes(T, K, D, nc)


# ---------------------------------------------------------------------------------------------
# what is compiled (read off the macros; each per mode SMOOTH and SCORE)
# ---------------------------------------------------------------------------------------------
PAIRS = [(D, O) for D in (2, 3) for O in (2, 4, 6, 8)]
WAVE_FORMS = ([('wave', D, O, 1, B) for D, O in PAIRS for B in (2, 4, 8)]          # EKS_DW_S: SUBS = 1, B = 2 / 4 / 8
              + [('wave', D, O, 2, 8) for D, O in PAIRS]                           # EKS_DW: SUBS = 2 at kDwBMax only
              + [('wave', 3, 10, 1, 8), ('wave', 3, 12, 1, 8)])                    # EKS_DW1
RUNS_FORMS = [(D, O) for D, O in PAIRS]                                            # EKS_WS_O / EKS_WR_O, B at run time
GENERIC_D = [1, 2, 3, 4, 5, 6]                                                     # EKS_DISPATCH_D
assert len(WAVE_FORMS) == 34 and len(set(WAVE_FORMS)) == 34 and len(RUNS_FORMS) == 8


def compiled(form):
    if form[0] == 'wave':
        return form in WAVE_FORMS
    if form[0] == 'runs':
        return form[1:3] in RUNS_FORMS and form[3] % 4 == 0 and form[3] <= 32
    return form[0] == 'generic' and form[1] in GENERIC_D


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
class Case:
    def __init__(self, group, T, K, D, O, form, knobs=None):
        self.group, self.T, self.K, self.D, self.O, self.form = group, T, K, D, O, form
        self.knobs = dict(knobs or {})
        self.general_a = False
        self.seed = 0
        kn = ''.join(f'-{k[4:].lower()}{v}' for k, v in sorted(self.knobs.items()))
        self.id = f'{group}-D{D}O{O}-T{T}K{K}{kn}'

    def forms(self):
        """The form per mode this case's shape and knobs select, by the transcription."""
        return {m: dense_form(self.T, self.K, self.D, self.O, m, self.knobs) for m in (SMOOTH, SCORE)}

    def problem(self):
        """(arrs, y, var, s): dense_problem's inputs, with general_a() on every other case, and one s per keypoint."""
        arrs, y, var = dense_problem(self.T, self.K, self.D, self.O, seed=self.seed)
        if self.general_a:
            general_a(arrs)
        s = np.exp(np.random.default_rng(3 + self.seed).uniform(-3, 4, self.K))
        return arrs, y, var, s

    def __repr__(self):
        return self.id


def _cases():
    out = []
    # wave, one pair per workgroup: every (D, O) at every chunk length; two units per keypoint, the second with one
    # ragged chunk of three frames
    for D, O in PAIRS:
        for B in (2, 4, 8):
            out.append(Case('wave1', 64 * B + 3, 2, D, O, ('wave', D, O, 1, B), {'EKS_DW_CHUNK': str(B)}))
    for O in (10, 12):
        out.append(Case('wave1', 515, 2, 3, O, ('wave', 3, O, 1, 8)))
    # wave, four-wave workgroups at the natural chunk: 257 units (the last workgroup has a spare pair), and 258 units
    # with two per keypoint
    for D, O in PAIRS:
        out.append(Case('wave2', 9, 257, D, O, ('wave', D, O, 2, 8)))
        out.append(Case('wave2', 517, 129, D, O, ('wave', D, O, 2, 8)))
    # five and six cameras with more than 256 units: still one pair per workgroup, 257 of them
    for O in (10, 12):
        out.append(Case('wave1many', 9, 257, 3, O, ('wave', 3, O, 1, 8)))
    # the knob path: a forced short chunk with more units than the one-pair form takes
    for B in (2, 4):
        for D, O in ((3, 4), (2, 8)):
            out.append(Case('waveknob', 9, 257, D, O, ('wave', D, O, 2, 8), {'EKS_DW_CHUNK': str(B)}))
    # runs: every pair at the natural 16 frames (19 = 16 + 3: a ragged group), at one and at eight checkpoints per lane
    for D, O in PAIRS:
        out.append(Case('runs', 19, 1025, D, O, ('runs', D, O, 16)))
        for B in (4, 32):
            out.append(Case('runs', 37, 1025, D, O, ('runs', D, O, B), {'EKS_DENSE_CHUNK': str(B)}))
    out.append(Case('runs', 37, 1025, 3, 6, ('runs', 3, 6, 12), {'EKS_DENSE_CHUNK': '12'}))
    out.append(Case('runs', 37, 1025, 2, 4, ('runs', 2, 4, 28), {'EKS_DENSE_CHUNK': '28'}))
    out.append(Case('runs', 1, 1025, 2, 8, ('runs', 2, 8, 16)))
    out.append(Case('runs', 3, 1025, 2, 8, ('runs', 2, 8, 16)))
    # generic, narrow: the accepted limits of D and O, odd O, O past 32
    for D, O in ((1, 1), (1, 64), (6, 1), (6, 64), (4, 16), (5, 5), (3, 33), (2, 7), (3, 9), (2, 64), (3, 5)):
        for T in (1, 2, 33, 70):
            out.append(Case('generic', T, 3, D, O, ('generic', D, 16)))
    # generic, many keypoints: five / six cameras handed over from the wave kernels past 1024 units, and D = 4
    for D, O in ((3, 10), (3, 12), (4, 5)):
        out.append(Case('genericmany', 19, 1025, D, O, ('generic', D, 16)))
    for i, c in enumerate(out):
        c.seed = 1000 + i
        c.general_a = i % 2 == 1
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
