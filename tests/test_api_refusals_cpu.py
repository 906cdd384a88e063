"""CPU: every refusal of the model-taking C entries, against a literal table.

The entries that take the linear-Gaussian model (y, var, m0, S0, A, C, Q, s) - eks_smooth, _tv, _robust, _jumps,
_increments, eks_em_stats, eks_innovations, eks_sample and the two NLL entries that take it with rconst - share their
argument checks in eks_amd/csrc/eks_api.hip.  The ORDER of those checks is part of each entry's contract (a caller
that hands over two defects gets the status of the first), so this test calls every entry with one defect, and with the
pairs of defects that fix the order, and compares each status with tests/golden/api_refusals.json: a table recorded
once from the library as it stood before the checks were gathered into helpers
(`python tests/test_api_refusals_cpu.py --record` rewrites it from the library EKS_HIP_LIB names).

Every row is refused inside eks_api.hip, before the first HIP call (read there: each is a return in front of the
dispatch into diag_X / dense_X), so the pointers are small host buffers nobody dereferences and no device is needed.
A row is never a valid call: those would launch.  Statuses at or below EKS_ERR_HIP_BASE would mean a row reached the
runtime and fail the test whatever the table says."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'tests', 'golden', 'api_refusals.json')
EKS_ERR_HIP_BASE = -1000
DIAG, VSD, UNIT = 1, 2, 4

MODEL = ['y', 'var', 'm0', 'S0', 'A', 'C', 'Q', 's']
NLL_MODEL = ['y', 'rconst', 'm0', 'S0', 'A', 'C', 'Q', 's_cand']
# Arguments between `dims` and (workspace, workspace_bytes, stream), in the C order.  A bare name is a pointer every
# valid call needs; (name, None) a pointer that may be NULL (NULL by default here); (name, value) a scalar.
ENTRIES = {
    'eks_smooth': MODEL + ['ms', 'Vs'],
    'eks_smooth_tv': ['y', 'var', 'qscale', ('qscale_per_keypoint', 0)] + MODEL[2:] + ['ms', 'Vs'],
    'eks_smooth_robust': MODEL + [('nu', 4.0), ('n_iters', 8), ('weights', None), ('weights_in', 0), ('change', None),
                                  'ms', 'Vs'],
    'eks_smooth_jumps': MODEL + [('nu', 4.0), ('n_iters', 8), ('scales', None), ('scales_in', 0), ('change', None),
                                 'ms', 'Vs'],
    'eks_smooth_increments': MODEL + [('ms', None), ('Vs', None), 'lag1', ('dmean', None), ('dV', None)],
    'eks_em_stats': MODEL + ['Sw'],
    'eks_innovations': MODEL + ['innov', ('innov_var', None), ('nis', None), ('frame_ll', None), ('loglik', None)],
    'eks_sample': MODEL + [('n_draws', 2), ('seed', 0), ('first_keypoint', 0), ('first_draw', 0), ('noise', None),
                           ('ms', None), 'draws'],
    'eks_nll': NLL_MODEL + [('n_cand', 3), ('per_keypoint', 0), 'nll', ('dnll', None)],
    'eks_nll_argmin': NLL_MODEL + [('n_cand', 3), 'nll', 's_out', ('idx_out', None)],
}
SIZE_QUERY = {e: e + '_workspace_bytes' for e in ENTRIES}
SIZE_QUERY['eks_nll_argmin'] = 'eks_nll_workspace_bytes'
SIZE_ARG = {'eks_sample': 2, 'eks_nll': 3, 'eks_nll_argmin': 3}          # the query's second argument
SIZE_TESTED_IN_API = ('eks_smooth_tv', 'eks_smooth_robust', 'eks_smooth_jumps', 'eks_em_stats', 'eks_innovations')
# entries whose own shape check refuses D > 6, O > 64 and a launch index past an int (the others leave that to diag_X /
# dense_X, which this test does not enter)
SHAPE_CHECKED_IN_API = SIZE_TESTED_IN_API + ('eks_smooth_increments',)
NEEDS_VS_DIAG_ON_CHAINS = ('eks_smooth_increments', 'eks_em_stats')

CHAINS = (3, 20, 2, 2, DIAG | VSD)
GENERAL = (3, 20, 3, 4, 0)
BAD_DIMS = {                                       # refused by every entry
    'no_keypoints': (0, 20, 2, 2, 0),
    'diag_D_ne_O': (3, 20, 2, 3, DIAG),
    'unit_without_diag': (3, 20, 2, 2, UNIT),
    'null_dims': None,
}
UNSUPPORTED_DIMS = {'D7': (3, 20, 7, 4, 0), 'O65': (3, 20, 3, 65, 0)}


@pytest.fixture(scope='module')
def lib():
    from eks_amd import _build, _lib
    _build.build()
    return _lib.load()


def _first_refused_T(lib, K, D, O, flags):
    """Smallest T whose eks_em_stats workspace query is 0 at (K, D, O, flags): one frame past the launch-index limit
    (diag_chain_covers on chains, K x chunks < 2^30 on general models).  The query is arithmetic only."""
    from eks_amd import _lib
    q = lambda T: lib.eks_em_stats_workspace_bytes(ctypes.byref(_lib.EksDims(K, T, D, O, flags)))
    lo, hi = 1, 1 << 30                            # q(lo) > 0, q(hi) == 0
    assert q(lo) > 0 and q(hi) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if q(mid) > 0 else (lo, mid)
    return hi


def rows(lib):
    """{row id: status} of every refusal, in a fixed order."""
    from eks_amd import _lib
    buf = ctypes.create_string_buffer(64)
    one, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    out = {}

    def dims_ref(dims):
        return None if dims is None else ctypes.byref(_lib.EksDims(*dims))

    def query(entry, dims):
        extra = (SIZE_ARG[entry],) if entry in SIZE_ARG else ()
        return int(getattr(lib, SIZE_QUERY[entry])(dims_ref(dims), *extra))

    def call(entry, dims, ws=one, ws_bytes=1 << 40, **over):
        args = []
        for a in ENTRIES[entry]:
            name, dflt = (a, one) if isinstance(a, str) else (a[0], null if a[1] is None else a[1])
            v = over.pop(name, dflt)
            args.append(null if v is None else v)
        assert not over, over
        return int(getattr(lib, entry)(dims_ref(dims), *args, ws, ws_bytes, None))

    def row(rid, status):
        assert rid not in out, rid
        out[rid] = status

    chain_T = _first_refused_T(lib, 1 << 22, 2, 2, DIAG | VSD)
    dense_T = _first_refused_T(lib, 5000000, 3, 4, 0)
    assert chain_T > 2 and dense_T > 2
    chain_limit = (1 << 22, chain_T, 2, 2, DIAG | VSD)
    dense_limit = (5000000, dense_T, 3, 4, 0)

    for entry, spec in ENTRIES.items():
        # -- the size query over the shapes
        for name, dims in dict(chains=CHAINS, chains_no_vs_diag=CHAINS[:4] + (DIAG,), general=GENERAL, **UNSUPPORTED_DIMS,
                               **BAD_DIMS, chain_limit=chain_limit, dense_limit=dense_limit).items():
            row(f'{SIZE_QUERY[entry]}|{entry}|{name}', int(query(entry, dims) > 0))
        if entry == 'eks_sample':
            row('eks_sample_workspace_bytes|eks_sample|chains|n_draws=0',
                int(lib.eks_sample_workspace_bytes(dims_ref(CHAINS), 0) > 0))
        # -- shapes every entry refuses itself, and a second defect behind them
        for name, dims in BAD_DIMS.items():
            row(f'{entry}|{name}', call(entry, dims))
            row(f'{entry}|{name}|y=NULL', call(entry, dims, y=None))
        if entry in SHAPE_CHECKED_IN_API:
            for name, dims in UNSUPPORTED_DIMS.items():
                row(f'{entry}|{name}', call(entry, dims))
            row(f'{entry}|chain_limit', call(entry, chain_limit))
            row(f'{entry}|chain_limit_minus_1|ws=NULL', call(entry, chain_limit[:1] + (chain_T - 1,) + chain_limit[2:],
                                                             ws=null))
            if entry != 'eks_smooth_increments':       # (dense_increments refuses that shape itself)
                row(f'{entry}|dense_limit', call(entry, dense_limit))
                row(f'{entry}|dense_limit_minus_1|ws=NULL',
                    call(entry, dense_limit[:1] + (dense_T - 1,) + dense_limit[2:], ws=null))
        if entry in NEEDS_VS_DIAG_ON_CHAINS:
            row(f'{entry}|chains_no_vs_diag', call(entry, CHAINS[:4] + (DIAG,)))
        # -- one defect at a time on the two valid shapes
        for sname, dims in (('chains', CHAINS), ('general', GENERAL)):
            pre = f'{entry}|{sname}'
            for a in spec:
                if isinstance(a, str):
                    row(f'{pre}|{a}=NULL', call(entry, dims, **{a: None}))
            row(f'{pre}|ws=NULL', call(entry, dims, ws=null))
            row(f'{pre}|y=NULL,ws=NULL', call(entry, dims, y=None, ws=null))
            if entry in SIZE_TESTED_IN_API:
                need = query(entry, dims)
                assert need > 1
                row(f'{pre}|ws_bytes=need-1', call(entry, dims, ws_bytes=need - 1))
                row(f'{pre}|ws=NULL,ws_bytes=need-1', call(entry, dims, ws=null, ws_bytes=need - 1))
            if entry in ('eks_smooth_robust', 'eks_smooth_jumps'):
                plane = 'weights' if entry == 'eks_smooth_robust' else 'scales'
                for nu in (0.0, -1.0, float('inf'), float('nan')):
                    row(f'{pre}|nu={nu}', call(entry, dims, nu=nu))
                    row(f'{pre}|nu={nu},y=NULL', call(entry, dims, nu=nu, y=None))
                row(f'{pre}|n_iters=0', call(entry, dims, n_iters=0))
                row(f'{pre}|n_iters=0,Vs=NULL', call(entry, dims, n_iters=0, Vs=None))
                row(f'{pre}|{plane}_in=1', call(entry, dims, **{plane + '_in': 1}))
                row(f'{pre}|{plane}_in=1,s=NULL', call(entry, dims, **{plane + '_in': 1, 's': None}))
                row(f'{pre}|{plane}_in=1,ws=NULL', call(entry, dims, **{plane + '_in': 1}, ws=null))
            if entry == 'eks_smooth_increments':
                row(f'{pre}|no_output', call(entry, dims, lag1=None))
                row(f'{pre}|no_output,ms=set', call(entry, dims, lag1=None, ms=one, Vs=one))
                row(f'{pre}|no_output,ws=NULL', call(entry, dims, lag1=None, ws=null))
                row(f'{pre}|no_output,y=NULL', call(entry, dims, lag1=None, y=None))
            if entry == 'eks_innovations':
                row(f'{pre}|no_output', call(entry, dims, innov=None))
                row(f'{pre}|no_output,ws=NULL', call(entry, dims, innov=None, ws=null))
                row(f'{pre}|no_output,Q=NULL', call(entry, dims, innov=None, Q=None))
                if sname == 'chains':
                    for o in ('nis', 'frame_ll'):
                        row(f'{pre}|{o}=set', call(entry, dims, **{o: one}))
                        row(f'{pre}|{o}=set,ws=NULL', call(entry, dims, **{o: one}, ws=null))
                        row(f'{pre}|{o}=set,C=NULL', call(entry, dims, **{o: one, 'C': None}))
                        row(f'{pre}|{o}=only', call(entry, dims, **{o: one, 'innov': None}))
            if entry == 'eks_sample':
                for k in ('n_draws', 'first_keypoint', 'first_draw'):
                    bad = 0 if k == 'n_draws' else -1
                    row(f'{pre}|{k}={bad}', call(entry, dims, **{k: bad}))
                    row(f'{pre}|{k}={bad},y=NULL', call(entry, dims, **{k: bad, 'y': None}))
                    row(f'{pre}|{k}={bad},ws=NULL', call(entry, dims, **{k: bad}, ws=null))
            if entry in ('eks_nll', 'eks_nll_argmin'):
                row(f'{pre}|n_cand=0', call(entry, dims, n_cand=0))
                row(f'{pre}|n_cand=0,y=NULL', call(entry, dims, n_cand=0, y=None))
    return out


def test_every_refusal_matches_the_recorded_table(lib):
    with open(TABLE) as f:
        want = json.load(f)
    got = rows(lib)
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    for rid, status in got.items():
        assert status > EKS_ERR_HIP_BASE, f'{rid}: status {status} came from the HIP runtime'
        if '_workspace_bytes|' not in rid:
            assert status != 0, f'{rid}: a row must be refused, not run'
    wrong = {rid: (got[rid], want[rid]) for rid in got if got[rid] != want[rid]}
    assert not wrong, f'(got, recorded): {wrong}'


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, ROOT)
    from eks_amd import _lib as _l
    table = rows(_l.load())
    with open(TABLE, 'w') as f:
        json.dump(table, f, indent=0)
        f.write('\n')
    print(f'{len(table)} rows -> {TABLE}')
