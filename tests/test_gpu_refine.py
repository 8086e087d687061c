"""maray_jit_refine on the device (maray_amd/csrc/jit_source.cpp, jit_source_refine): the guard words it leaves
are the numpy evaluator's (tests/refine_eval.py) bit for bit -- the device sine is glibc's -- and every raster equals the one
of a context created with MARAY_JIT_GUARD_REFINE=0, and the oracle's or the committed golden."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import params as PR
import refine_eval as RE
import refine_scenes as RS
from conftest import GOLDEN
from marayb import encode
from oracle_ffi import Scene as OScene
from test_gpu_supersample import box

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = RS.W, RS.H


def context(tape, refine=True, **kw):
    """A MARAY_BACKEND_JIT context; refine=False: created with MARAY_JIT_GUARD_REFINE=0 (read when the context is created)."""
    old = os.environ.get('MARAY_JIT_GUARD_REFINE')
    os.environ['MARAY_JIT_GUARD_REFINE'] = '1' if refine else '0'
    try:
        return M.Context(tape, backend=M.BACKEND_JIT, **kw)
    finally:
        if old is None:
            del os.environ['MARAY_JIT_GUARD_REFINE']
        else:
            os.environ['MARAY_JIT_GUARD_REFINE'] = old


def rows(ctx, w, h, y0, y1, values=None):
    if values is not None:
        ctx.set_params(list(values))
    return ctx.render_rows(w, h, y0, y1, want_f64=False)[0]


def numpy_words(tape, w, rows_, refined=True, params=None):
    pos, n_words, gw, gh = tape.guard_layout()
    geo, second, _ = RE.guard_bits(tape, w, 0, rows_, gw, gh, params=params)
    return RE.pack_words(geo & second if refined else geo, pos, n_words)


_family = {}


def family(kind, seed=0):
    """(tape, the oracle's raster) of a scene of the family."""
    if (kind, seed) not in _family:
        data = RS.data(kind, seed)
        _family[(kind, seed)] = (M.Scene(data).lower(), OScene(data).render_rows(W, H, 0, H, want_f64=False)[0])
    return _family[(kind, seed)]


_chess = {}


def chess():
    if not _chess:
        _chess['tape'] = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()
    return _chess['tape']


@pytest.mark.parametrize('kind', ['mixed', 'zero', 'huge', 'square'])
def test_family_words_and_raster(kind):
    """320 x 72: a ragged last tile, two full groups of rows and one of 8."""
    tape, want = family(kind)
    on, off = context(tape), context(tape, refine=False)
    assert np.array_equal(rows(on, W, H, 0, H), want)
    assert np.array_equal(rows(off, W, H, 0, H), want)
    assert (on.refine_count, off.refine_count) == (1, 0)
    got, plain = on.debug_guard_words(), off.debug_guard_words()
    assert np.array_equal(plain, numpy_words(tape, W, H, refined=False))
    assert np.array_equal(got, numpy_words(tape, W, H))
    assert not (got & ~plain).any()                         # a subset, bit by bit
    if kind != 'square':
        assert (plain & ~got).any()                         # ... and a proper one
    on.close()
    off.close()


def test_shapes_behind_one_bound():
    """refine_scenes.shared_bound: a shape that only its group's SKIP skips shares the guard of shapes with other patterns."""
    data = encode((W, H), RS.shared_bound())
    tape, want = M.Scene(data).lower(), OScene(data).render_rows(W, H, 0, H, want_f64=False)[0]
    assert tape.refine.n_outs
    on, off = context(tape), context(tape, refine=False)
    assert np.array_equal(rows(on, W, H, 0, H), want) and np.array_equal(rows(off, W, H, 0, H), want)
    assert np.array_equal(on.debug_guard_words(), numpy_words(tape, W, H)) and on.refine_count == 1
    parts = np.concatenate([rows(on, W, H, 0, 16), rows(on, W, H, 16, H)])
    assert np.array_equal(parts, want)
    on.close()
    off.close()


def test_chess_1024_words_and_golden():
    tape = chess()
    on, off = context(tape), context(tape, refine=False)
    a, b = rows(on, 1024, 1024, 0, 1024), rows(off, 1024, 1024, 0, 1024)
    with open(os.path.join(GOLDEN, 'chess_1024.json')) as f:
        sha = json.load(f)['rgb8_sha256']
    assert hashlib.sha256(a.tobytes()).hexdigest() == sha and np.array_equal(a, b)
    got = on.debug_guard_words()
    assert np.array_equal(got, numpy_words(tape, 1024, 1024))
    assert np.array_equal(off.debug_guard_words(), numpy_words(tape, 1024, 1024, refined=False))
    assert on.refine_count == 1
    # rows in two parts: each part is a geometry of its own, with its own pass
    parts = np.concatenate([rows(on, 1024, 1024, 0, 416), rows(on, 1024, 1024, 416, 1024)])
    assert np.array_equal(parts, a) and on.refine_count == 3
    on.close()
    off.close()


def test_rows_in_two_parts_of_a_ragged_picture():
    tape, want = family('mixed', 1)
    on = context(tape)
    assert np.array_equal(np.concatenate([rows(on, W, H, 0, 40), rows(on, W, H, 40, H)]), want)
    assert np.array_equal(on.debug_guard_words(), numpy_words_at(tape, 40, H))
    on.close()


def numpy_words_at(tape, y0, y1):
    pos, n_words, gw, gh = tape.guard_layout()
    geo, second, _ = RE.guard_bits(tape, W, y0, y1 - y0, gw, gh)
    return RE.pack_words(geo & second, pos, n_words)


def test_supersampled_k2():
    """k = 2: the ROW stage, and the pass behind it, cover the 640 x 144 sample grid."""
    data = RS.data('mixed', 0)
    s = M.Scene(data)
    s.supersample(2)
    tape = s.lower()
    assert tape.refine.n_outs
    want = box(OScene(s.encode()).render_rows(2 * W, 2 * H, 0, 2 * H, want_f64=False)[0], 2)
    on, off = context(tape, samples=2), context(tape, refine=False, samples=2)
    a, b = rows(on, W, H, 0, H), rows(off, W, H, 0, H)
    assert on.kernel_name == 'maray_jit_pixels_ss' and (on.refine_count, off.refine_count) == (1, 0)
    assert np.array_equal(a, b)
    assert np.array_equal(a, want)
    on.close()
    off.close()


def test_counts():
    """Ten launches of one geometry: one pass.  A changed ROW-read parameter: another, and the oracle's pixels.  A changed
    PIXEL-only parameter: none.  The knob at 0: none."""
    color, decl = RS.moving()
    spec = dict(color=color, params=decl)
    scene, names = PR.declared(spec, (W, H))
    tape = scene.lower()
    assert tape.info['row_params'] == 1 and tape.refine.n_outs

    def oracle(values):
        return PR.oracle_frame(spec, (W, H), values, want_f64=False)[0]

    on, off = context(tape), context(tape, refine=False)
    first = oracle((3.0, 0.5))
    for i in range(10):
        assert np.array_equal(rows(on, W, H, 0, H, (3.0, 0.5)), first), i
    assert on.refine_count == 1 and on.launch_counts[0] == 1
    assert np.array_equal(on.debug_guard_words(), numpy_words(tape, W, H, params=(3.0, 0.5)))
    assert np.array_equal(rows(on, W, H, 0, H, (-40.5, 0.5)), oracle((-40.5, 0.5)))         # ROW-read
    assert on.refine_count == 2
    assert np.array_equal(on.debug_guard_words(), numpy_words(tape, W, H, params=(-40.5, 0.5)))
    assert np.array_equal(rows(on, W, H, 0, H, (-40.5, 1.0)), oracle((-40.5, 1.0)))         # PIXEL only
    assert on.refine_count == 2
    for v in ((3.0, 0.5), (-40.5, 0.5)):
        assert np.array_equal(rows(off, W, H, 0, H, v), oracle(v))
    assert off.refine_count == 0 and off.launch_counts[0] == 2
    on.close()
    off.close()


_BLOCKS = r"""
import hashlib, json, os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from test_gpu_refine import context, chess, family, W, H
for tape, w, h, blk, stride, n, want in ((chess(), 1024, 1024, 32, 64, 16, None), (family('mixed')[0], W, H, 8, 24, 3, family('mixed')[1])):
    pick = (np.arange(n)[:, None] * stride + np.arange(blk)[None, :]).reshape(-1)
    outs = []
    for refine in (True, False):
        ctx = context(tape, refine=refine)
        d = torch.zeros((n * blk, w, 3), dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()
        ctx.render_blocks_device(w, h, 0, blk, stride, n, d_rgb8=d.data_ptr())
        torch.cuda.synchronize()
        outs.append(d.cpu().numpy())
        assert ctx.refine_count == (1 if refine else 0)
        if want is None:
            want = ctx.render_rows(w, h, 0, h, want_f64=False)[0]
            assert hashlib.sha256(want.tobytes()).hexdigest() == json.load(open(os.path.join(%(golden)r, 'chess_1024.json')))['rgb8_sha256']
        ctx.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want[pick])
print('blocks ok')
"""


def test_blocks_with_a_stride():
    """render_blocks_device, an interleaved share in one launch: chess in blocks of 32 rows 64 apart, the family in blocks of
    8 rows 24 apart (guards per row there: a group may not straddle two blocks).  A process of its own: the device buffers
    come from PyTorch, imported before the library."""
    code = _BLOCKS % {'root': ROOT, 'tests': HERE, 'golden': GOLDEN}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('blocks ok'), r.stdout[-2000:] + r.stderr[-4000:]
