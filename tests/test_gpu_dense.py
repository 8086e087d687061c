"""The dense-argument scenes of tests/dense_values.py on the device: sqrt, recip, a multiply-add, exp, ln and the bounded and
unbounded sine forms on full 53-bit mantissas, x-varying (the PIXEL kernels) and y-only (the ROW kernels, rows as lanes), on
all three back-ends against the CPU oracle on every pixel -- f64 planes bit for bit (all NaNs equal), RGB8 byte for byte, no
tolerance -- and rendered RGB8-only as well.  The last bits of a result do not show in the bytes: that the device's
arithmetic is the oracle's to the bit rests on the f64 planes.

The interpreters are built by hipcc, the specialised kernels by the hiprtc of the process: PyTorch's where PyTorch was
imported first (every child process here but the last), the system's otherwise -- all three builds meet dense operands, on
which a multiply-add fused behind the tape's back, a reduction constant off by one digit or a sqrt that rounds the other way
change bits.  tests/test_dense.py holds the scenes' inputs, lowering and generated sources to account on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_values as D
import maray_amd as M
from params import same_f64
from test_gpu_launches import _run

pytestmark = pytest.mark.gpu

BACKENDS = {'JIT': M.BACKEND_JIT, 'TAPE': M.BACKEND_TAPE, 'INTERP': M.BACKEND_TAPE_SMEM}


def run_cells(names, forms, backends, render):
    """Every frame of every (scene, form) cell on every back-end of `backends` (names of BACKENDS) against the oracle.
    render(ctx, w, h, f64) -> (rgb8, f64 planes or None) as numpy arrays.  One tape and one context per cell and back-end;
    the specialised contexts are built side by side.  Returns the number of renders compared."""
    from test_fuzz import _jit_contexts
    cells = [(n, f) for n in names for f in forms]
    tapes = [D.scene(n, f).lower() for n, f in cells]
    tex = D.textures()
    jit = _jit_contexts([(t, tex) for t in tapes]) if 'JIT' in backends else [None] * len(cells)
    done = 0
    for (name, form), tape, jctx in zip(cells, tapes, jit):
        w, h = D.size(name, form)
        for b in backends:
            ctx = jctx if b == 'JIT' else M.Context(tape, textures=tex, backend=BACKENDS[b])
            for values in D.frames(name):
                if values:
                    ctx.set_params(list(values))
                want8, want64 = D.oracle(name, form, values)
                for f64 in (True, False):
                    got8, got64 = render(ctx, w, h, f64)
                    where = (name, form, b, ctx.kernel_name, values, 'f64 planes' if f64 else 'RGB8 only')
                    if f64:
                        assert same_f64(got64, want64), (where, D.first_mismatch(got64, want64))
                    assert np.array_equal(got8, want8), (where, np.argwhere(got8 != want8)[:4].tolist())
                    done += 1
            ctx.close()
    return done


_CELLS = r"""
import dense_values as D
import test_gpu_dense as G
os.environ.update(%(knobs)r)


def guarded(ctx, w, h, f64):
    got8, got64 = render(ctx, w, h, ('rows', 0, h), f64=f64)
    return got8.cpu().numpy(), got64.cpu().numpy() if f64 else None


n = G.run_cells(%(names)r, %(forms)r, %(backends)r, guarded)
assert 'torch' in sys.modules
print('dense ok', n)
"""


def _cells(names, forms=D.FORMS, backends=('JIT', 'TAPE', 'INTERP'), knobs=None):
    """In a child process that imported PyTorch first (its hiprtc builds the specialised kernels), into buffers with guard
    bands (the render prelude of test_gpu_launches.py)."""
    _run(_CELLS, 'dense ok', 900, names=tuple(names), forms=tuple(forms), backends=tuple(backends), knobs=dict(knobs or {}))


@pytest.mark.parametrize('name', D.NAMES)
def test_dense_scene_on_every_back_end(name):
    """Both forms of the scene on the interpreter, the scalar-cache interpreter and the specialised kernels, with f64 planes
    and RGB8-only; sin_bounded: its 29 frames on one context per back-end."""
    _cells([name])


@pytest.mark.parametrize('knobs,names,backends', [
    ({'MARAY_JIT_WIDE_APP': '0'}, ('algebra',), ('JIT',)),                       # sqrt, recip, multiply-add one pixel per lane
    ({'MARAY_TAPE_GENERIC': '1'}, D.NAMES, ('TAPE', 'INTERP')),                  # the interpreters' generic loop
], ids=['wide_app0', 'tape_generic'])
def test_dense_scenes_under_knobs(knobs, names, backends):
    """The other form of the same ops a knob selects: by default the algebra scene runs four pixels per lane (mr_sqrt's own
    four-wide form), under MARAY_JIT_WIDE_APP=0 one; MARAY_TAPE_GENERIC=1 takes the interpreters' generic loop."""
    _cells(names, ('x',), backends, knobs)


_NO_TORCH = r"""
import os, sys
sys.path[:0] = [%(root)r, %(tests)r]
import dense_values as D
import test_gpu_dense as G
n = G.run_cells(D.NAMES, ('x',), ('JIT',), lambda ctx, w, h, f64: ctx.render_rows(w, h, 0, h, want_f64=f64))
assert 'torch' not in sys.modules
print('no torch ok', n)
"""


def test_dense_scenes_in_a_process_without_pytorch():
    """The x-varying scenes on the specialised kernels built by the system's hiprtc: the process never imports PyTorch."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, '-c', _NO_TORCH % dict(root=os.path.dirname(here), tests=here)], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and 'no torch ok' in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
