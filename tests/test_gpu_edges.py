"""The edge-value matrix of tests/edge_values.py on the device: every (op, form) cell on all three back-ends, with f64
planes (bit for bit, all NaNs equal) and without them (RGB8 only: the specialised kernel's four-pixels-per-lane layout and
dwordx3 stores), at widths ragged modulo 4, 64 and 256, against the CPU oracle.  Renders land in buffers with guard bands
(the PAD / render prelude of test_gpu_launches.py), whole images and single rows.  Then the knobs that select other
code, and a process that never imported PyTorch (the specialised kernels built by the system's hiprtc, not PyTorch's)."""
import os

import numpy as np
import pytest

import edge_values as E
import maray_amd as M
from oracle_ffi import Scene as OScene
from test_gpu_launches import _run
from test_lowering import same_f64

pytestmark = pytest.mark.gpu

_MATRIX = r"""
import time
from concurrent.futures import ThreadPoolExecutor
import edge_values as E
knobs = %(knobs)r
os.environ.update(knobs)
cases = [c for c in E.cases() if (not %(only)r or c.form in %(only)r) and (not %(ops)r or c.op in %(ops)r)]
backends = %(backends)r
tex = E.textures()
t0 = time.time()
tapes = [M.Scene(c.data()).lower(hoist_rows=c.hoist) for c in cases]
with ThreadPoolExecutor(8) as pool:          # the specialised builds side by side (two compiler processes each)
    jit = list(pool.map(lambda ct: M.Context(ct[1], textures=tex if ct[0].textures else None, backend=JIT) if JIT in backends else None,
                        zip(cases, tapes)))
t_build = time.time() - t0
n = 0
for c, tape, jctx in zip(cases, tapes, jit):
    t = tex if c.textures else None
    data = c.data()
    o = OScene(data)
    widths = (257, 302, 512) if c.w == 512 else E.WIDTHS
    for b in backends:
        ctx = jctx if b == JIT else M.Context(tape, textures=t, backend=b)
        for w in widths:
            want8, want64 = o.render_rows(w, c.h, 0, c.h, t, threads=THREADS)
            for f64 in (True, False):
                got8, got64 = render(ctx, w, c.h, ('rows', 0, c.h), f64=f64)
                got8 = got8.cpu().numpy()
                assert np.array_equal(got8, want8), (c.id, b, w, f64, knobs, np.argwhere(got8 != want8)[:4].tolist())
                if f64:
                    assert same_f64(got64.cpu().numpy(), want64), (c.id, b, w, knobs)
                n += 1
            # single rows: a store past the end of a row lands in a band
            for y in sorted({0, c.h // 2, c.h - 1}):
                got8, got64 = render(ctx, w, c.h, ('rows', y, y + 1))
                assert np.array_equal(got8.cpu().numpy(), want8[y:y + 1]), (c.id, b, w, y, knobs)
                assert same_f64(got64.cpu().numpy(), want64[y:y + 1]), (c.id, b, w, y, knobs)
                got8, _ = render(ctx, w, c.h, ('rows', y, y + 1), f64=False)
                assert np.array_equal(got8.cpu().numpy(), want8[y:y + 1]), (c.id, b, w, y, 'RGB8 only', knobs)
        ctx.close()
print('edges ok', len(cases), n, 'build %%.1f s' %% t_build, 'total %%.1f s' %% (time.time() - t0))
"""


def _matrix(knobs=None, only=(), backends=('JIT', 'TAPE', 'INTERP'), ops=(), timeout=1200):
    """The cells of the forms in `only` (all if empty) and of the ops in `ops` (all if empty), in a child process."""
    names = {'JIT': 'JIT', 'TAPE': 'M.BACKEND_TAPE', 'INTERP': 'INTERP'}
    body = _MATRIX.replace('%(backends)r', '[' + ', '.join(names[b] for b in backends) + ']')
    _run(body, 'edges ok', timeout, knobs=dict(knobs or {}), only=tuple(only), ops=tuple(ops))


def test_edge_matrix_on_every_back_end():
    """Every cell (tests/edge_values.py: cases) on the specialised kernels, the interpreter and the scalar-cache interpreter:
    f64 planes and RGB8 only, widths 1, 3, 63, 65, 257 and 302 (257, 302 and 512 for the guarded scenes), whole images and
    rows 0, h/2 and h-1 alone, into guarded buffers.  This process imports PyTorch first: PyTorch's hiprtc builds."""
    _matrix()


@pytest.mark.parametrize('knobs,only,backends', [
    ({'MARAY_JIT_WIDE_APP': '0'}, ('texel', 'texel-wide', 'guarded'), ('JIT',)),         # texel lookups one pixel per lane
    ({'MARAY_JIT_TEXEL_ONCE': '0'}, ('texel', 'texel-wide', 'guarded'), ('JIT',)),       # a call of mr_app per channel
    ({'MARAY_TAPE_GENERIC': '1'}, (), ('TAPE', 'INTERP')),                               # the interpreter's generic loop
    ({'MARAY_TAPE_ROW_GUARDS': '1'}, ('guarded', 'x-narrow', 'y-row'), ('TAPE', 'INTERP')),   # guards per row as y values
], ids=['wide_app0', 'texel_once0', 'tape_generic', 'tape_row_guards'])
def test_edge_matrix_under_knobs(knobs, only, backends):
    """The cells a knob changes the code of, on the back-ends it applies to."""
    _matrix(knobs, only, backends)


_NO_TORCH = r"""
import os, sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import edge_values as E
import maray_amd as M
from oracle_ffi import Scene as OScene
from test_fuzz import _jit_contexts
from test_lowering import same_f64
cases = [c for c in E.cases() if c.op in E.LIBM and c.form in ('x-narrow', 'y-row', 'const-row', 'const-pixel')]
ctxs = _jit_contexts([(M.Scene(c.data()).lower(hoist_rows=c.hoist), None) for c in cases])
for c, ctx in zip(cases, ctxs):
    for w in (65, 302):
        want8, want64 = OScene(c.data()).render_rows(w, c.h, 0, c.h, threads=min(16, os.cpu_count() or 1))
        got8, got64 = ctx.render_rows(w, c.h, 0, c.h)
        assert np.array_equal(got8, want8) and same_f64(got64, want64), (c.id, w)
        got8, _ = ctx.render_rows(w, c.h, 0, c.h, want_f64=False)
        assert np.array_equal(got8, want8), (c.id, w, 'RGB8 only')
    ctx.close()
assert 'torch' not in sys.modules
print('no torch ok', len(cases))
"""


def test_libm_edges_in_a_process_without_pytorch():
    """sin, step(sin), exp and ln at their hard points (x-varying, y-only and constant operands) built by the system's
    hiprtc -- the process never imports PyTorch -- against the oracle, with and without f64 planes."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, '-c', _NO_TORCH % dict(root=os.path.dirname(here), tests=here)], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and 'no torch ok' in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
