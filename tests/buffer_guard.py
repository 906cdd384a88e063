"""Guarded device buffers for the GPU tests (a helper module, not a conftest).

guarded_workspaces(monkeypatch, fill) replaces hip_ops._workspace for the rest of a test: every workspace the wrappers
ask for is the body of one uint8 tensor laid out as [head guard | body | tail guard].  The body is exactly the number
of bytes the entry point's *_workspace_bytes query reported (256 where it reported 0), so the library is told the
queried size and not a byte more; both guards hold 0xA5 and the body holds `fill`.  An overrun lands in memory the test
owns and shows up as a failed assertion of assert_intact(), which names the entry point and the first damaged byte.

guarded_output(shape, dtype) is the same idea for an output tensor.

GUARD is 0xA5: as float32 -1.43e-16 and as float64 -1.2e-130 (tiny, finite), as an int32 index -1 515 870 811."""
import sys

import torch

GUARD = 0xA5
HEAD_BYTES = 4096                      # keeps the body on the allocator's base alignment
MIN_TAIL_BYTES = 1 << 20               # tail: max(n, 1 MiB) - room for any level a size query left out
MIN_BODY_BYTES = 256                   # what hip_ops._workspace hands out for a query of 0

_ENTRY = {                             # hip_ops function / class that asked -> the C entry point(s) it serves
    'PreparedSmooth': 'eks_smooth', 'smooth_tv': 'eks_smooth_tv', 'smooth_increments': 'eks_smooth_increments',
    'em_stats': 'eks_em_stats', 'innovations': 'eks_innovations', 'EmScaleLoop': 'eks_em_scale_run',
    'sample': 'eks_sample', 'const_r': 'eks_const_r', 'nll': 'eks_nll', 'nll_argmin': 'eks_nll_argmin',
    'AdamLoop': 'eks_adam_prepare + eks_adam_run', 'Ar1Loss': 'eks_ar1_nll / eks_pupil_adam_run',
    'ekf_smooth': 'eks_ekf_smooth', 'ekf_affine_workspace': 'eks_ekf_affine_sweep',
}


def _first_damage(region):
    """Offset of the first byte of a guard region that is not GUARD, or None."""
    bad = region != GUARD
    if not bool(bad.any()):
        return None
    return int(torch.nonzero(bad)[0, 0])


def _caller_entry(depth=2):
    """The C entry point behind the hip_ops function (or class constructor) that is asking for a workspace."""
    f = sys._getframe(depth)
    name = f.f_code.co_name
    if name == '__init__' and 'self' in f.f_locals:
        name = type(f.f_locals['self']).__name__
    if name not in _ENTRY and isinstance(f.f_locals.get('entry'), str):     # a test's own call of the C ABI names it
        name = f.f_locals['entry']
    return _ENTRY.get(name, name)


class _Guarded:
    """One [head | body | tail] allocation; body is the view handed out."""

    def __init__(self, entry, whole, head, nbody):
        self.entry, self.whole, self.head_bytes, self.nbody = entry, whole, head, nbody
        self.body = whole[head:head + nbody]

    def damage(self):
        """None, or a description of the first damaged guard byte."""
        off = _first_damage(self.whole[:self.head_bytes])
        if off is not None:
            return (f'{self.entry}: head guard damaged {self.head_bytes - off} bytes in front of the buffer '
                    f'(value {int(self.whole[off])})')
        tail = self.whole[self.head_bytes + self.nbody:]
        off = _first_damage(tail)
        if off is not None:
            return (f'{self.entry}: tail guard damaged at offset {self.nbody + off} of a buffer of {self.nbody} bytes '
                    f'({off} bytes past its end, value {int(tail[off])})')
        return None


class GuardedWorkspaces:
    """The replacement of hip_ops._workspace.  buffers: every allocation handed out, in order."""

    def __init__(self, fill):
        self.fill = fill
        self.buffers = []

    def __call__(self, nbytes, device):
        n = int(nbytes)
        nbody = n if n > 0 else MIN_BODY_BYTES
        whole = torch.full((HEAD_BYTES + nbody + max(n, MIN_TAIL_BYTES),), GUARD, dtype=torch.uint8, device=device)
        g = _Guarded(_caller_entry(), whole, HEAD_BYTES, nbody)
        assert g.body.data_ptr() - whole.data_ptr() == HEAD_BYTES and g.body.numel() == nbody
        if callable(self.fill):
            self.fill(g.body)
        else:
            g.body.fill_(int(self.fill))
        self.buffers.append(g)
        return g.body

    def bodies(self):
        """Clones of the bodies as they stand now (the state a call left behind), in the order handed out."""
        torch.cuda.synchronize()
        return [g.body.clone() for g in self.buffers]

    def assert_intact(self):
        torch.cuda.synchronize()
        assert self.buffers, 'no workspace was requested through hip_ops._workspace'
        for g in self.buffers:
            bad = g.damage()
            assert bad is None, bad


def guarded_workspaces(monkeypatch, fill):
    """Route hip_ops._workspace (smooth, PreparedSmooth, EmScaleLoop, AdamLoop, Ar1Loss, ... alike: they all call it when
    they allocate) through guarded buffers until the test ends or the next call of this function.  fill: the byte the
    body starts with, or a callable body -> None that writes it (e.g. the bytes another call left behind)."""
    from eks_amd import hip_ops
    gw = GuardedWorkspaces(fill)
    monkeypatch.setattr(hip_ops, '_workspace', gw)
    return gw


def stale_fill(bodies):
    """A fill that hands out, one after the other, the bytes of `bodies` (GuardedWorkspaces.bodies() of an earlier
    call); a body of another size is tiled / truncated to fit, so that a neighbour's leftovers can be used too."""
    queue = list(bodies)

    def fill(body):
        src = queue.pop(0) if len(queue) > 1 else queue[0]
        n = body.numel()
        if src.numel() >= n:
            body.copy_(src[:n])
        else:
            reps = -(-n // src.numel())
            body.copy_(src.repeat(reps)[:n])
    return fill


class GuardedOutput:
    """tensor: a contiguous view of `shape` with GUARD bytes in front and behind."""

    def __init__(self, name, shape, dtype, offset_elems=0, row_elems=None, device='cuda'):
        item = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= int(s)
        row = int(row_elems) if row_elems is not None else (numel // int(shape[0]) if len(shape) > 1 and shape[0] else numel)
        guard = max(HEAD_BYTES, -(-row * item // HEAD_BYTES) * HEAD_BYTES)          # >= one full row, >= 4096, aligned
        self.name, self.head_bytes, self.nbody = name, guard + offset_elems * item, numel * item
        self.whole = torch.full((guard + offset_elems * item + numel * item + guard,), GUARD, dtype=torch.uint8,
                                device=device)
        body = self.whole[self.head_bytes:self.head_bytes + self.nbody]
        self.tensor = body.view(dtype).view(*shape)
        assert self.tensor.is_contiguous() and self.tensor.data_ptr() % item == 0

    def assert_intact(self):
        torch.cuda.synchronize()
        bad = _Guarded(self.name, self.whole, self.head_bytes, self.nbody).damage()
        assert bad is None, bad


def guarded_output(shape, dtype=torch.float32, offset=0, row_elems=None, name='output', device='cuda'):
    """A GuardedOutput for an output of `shape`: guards of at least one full row (row_elems elements; default: one row
    of this tensor - pass the widest layout in play where outputs of several widths share a call) and at least 4096
    bytes; offset: elements by which the view is shifted off the allocation's alignment (1: the 4-byte-aligned case).
    The view starts as GUARD bytes, so that an element nobody stores shows as well."""
    return GuardedOutput(name, tuple(shape), dtype, offset, row_elems, device)


def bits(t):
    """The raw bits of a float tensor as integers (NaN payloads compare like everything else)."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))
