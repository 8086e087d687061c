"""The census of guard bits on the device (maray_jit_census, maray_jit_census_apply): the first launch that finds a
set of ROW outputs filled writes the set's guard words without the eligible bits of the shapes that are zero on every pixel of
a rectangle into the table that launch and the later ones read (Context.debug_census_words; the ROW pass's own words,
Context.debug_guard_words, stay the refined ones: tests/test_gpu_refine.py reads them after ten launches).  The words it
leaves are the numpy evaluator's (tests/census_scenes.py, tests/refine_eval.py) bit for bit; every
raster, before and after, equals the oracle's (or the committed golden) and the raster of a context created with
MARAY_JIT_GUARD_CENSUS=0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import census_scenes as CS
import params as PR
import refine_scenes as RS
from conftest import GOLDEN
from marayb import encode
from oracle_ffi import Scene as OScene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = CS.W, CS.H


def context(tape, census=True, reuse=True, **kw):
    """A MARAY_BACKEND_JIT context; census=False: created with MARAY_JIT_GUARD_CENSUS=0, reuse=False: with MARAY_JIT_ROW_REUSE=0
    (both are read when the context is created)."""
    want = {'MARAY_JIT_GUARD_CENSUS': '1' if census else '0', 'MARAY_JIT_ROW_REUSE': '1' if reuse else '0'}
    old = {k: os.environ.get(k) for k in want}
    os.environ.update(want)
    try:
        return M.Context(tape, backend=M.BACKEND_JIT, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def rows(ctx, w, h, y0, y1, values=None):
    if values is not None:
        ctx.set_params(list(values))
    return ctx.render_rows(w, h, y0, y1, want_f64=False)[0]


def popcount(words):
    return sum(bin(int(v)).count('1') for v in words.reshape(-1))


def three_renders(tape, want, w=W, h=H, y0=0, y1=H, must_clear=True):
    """Three renders of one geometry: words and counts after each, every raster equal to `want` and to the knob-off context's.
    Returns (the census'd words, their numpy counterpart)."""
    refined, exact = CS.words(tape, w, y0, y1 - y0, census=False), CS.words(tape, w, y0, y1 - y0)
    has_kernel = bool(tape.census_eligible().any())
    assert not (exact & ~refined).any()
    if must_clear:
        assert (refined & ~exact).any()                 # the scene has something for the census to clear
    on, off = context(tape), context(tape, census=False)
    try:
        assert np.array_equal(rows(on, w, h, y0, y1), want)
        assert np.array_equal(on.debug_census_words(), refined) and on.census_count == 0        # one render: still the refined words
        assert np.array_equal(rows(on, w, h, y0, y1), want)
        got = on.debug_census_words()
        assert on.census_count == (1 if has_kernel else 0)
        assert np.array_equal(got, exact), (popcount(refined), popcount(got), popcount(exact))
        assert np.array_equal(rows(on, w, h, y0, y1), want)
        assert on.census_count == (1 if has_kernel else 0) and np.array_equal(on.debug_census_words(), exact)
        assert np.array_equal(on.debug_guard_words(), refined)         # what the ROW pass and the second bounds wrote is kept
        for _ in range(3):
            assert np.array_equal(rows(off, w, h, y0, y1), want)
        assert off.census_count == 0 and np.array_equal(off.debug_census_words(), refined) and np.array_equal(off.debug_guard_words(), refined)
    finally:
        on.close()
        off.close()
    return got, exact


def lowered(color):
    data = encode((W, H), color)
    return M.Scene(data).lower(), OScene(data).render_rows(W, H, 0, H, want_f64=False)[0]


@pytest.mark.parametrize('kind', ['mixed', 'zero', 'huge', 'square'])
def test_family_words_and_rasters(kind):
    """320 x 72: a ragged last tile, two full groups of rows and one of 8."""
    data = RS.data(kind, 0)
    three_renders(M.Scene(data).lower(), OScene(data).render_rows(W, H, 0, H, want_f64=False)[0])


def test_shapes_behind_one_bound():
    """refine_scenes.shared_bound: its one bit with a leaf also gates the group's plain SKIP -- not eligible, no census."""
    tape, want = lowered(RS.shared_bound())
    assert not tape.census_eligible().any()
    three_renders(tape, want, must_clear=False)


_chess = {}


def chess():
    if not _chess:
        data = open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()
        _chess['tape'], _chess['oracle'] = M.Scene(data).lower(), OScene(data)
    return _chess['tape'], _chess['oracle']


@pytest.mark.parametrize('w,y0,y1', [(256, 640, 896), (320, 600, 672)])
def test_chess_windows(w, y0, y1):
    """256 x 256 and 320 x 72 of the board of the committed chess scene (columns from 0, rows from y0)."""
    tape, oracle = chess()
    three_renders(tape, oracle.render_rows(w, 1024, y0, y1, want_f64=False)[0], w=w, h=1024, y0=y0, y1=y1)


def test_chess_1024_golden():
    """The whole committed picture, before and after its census."""
    tape, _ = chess()
    with open(os.path.join(GOLDEN, 'chess_1024.json')) as f:
        sha = json.load(f)['rgb8_sha256']
    on = context(tape)
    for i in range(3):
        assert hashlib.sha256(rows(on, 1024, 1024, 0, 1024).tobytes()).hexdigest() == sha, i
        assert on.census_count == (0 if i == 0 else 1)
    on.close()


def test_one_pixel():
    """A leaf that is != 0 on exactly one pixel of its rectangle -- lane 0, lane 63, the first and the last row of a group, the
    ragged last rectangle -- keeps its bit."""
    tape, want = lowered(CS.one_pixel())
    counts, el = CS.nonzero_counts(tape, W, 0, H), CS.eligible_guards(tape)
    single = (counts == 1) & el[None, :]
    assert single.sum() == len(CS.ONE_PIXELS) and set(np.nonzero(single)[0]) == {2, 8 + 2, 8 + 1, 16 + 4}       # 8 rectangles per group
    got, _ = three_renders(tape, want)
    pos, _, _, _ = tape.guard_layout()
    for r, g in zip(*np.nonzero(single)):
        assert (int(got[r, pos[g] // 64]) >> int(pos[g] % 64)) & 1, (r, g)


def test_a_leaf_under_another():
    """An OR of booleans in which two shapes cover every pixel: whichever the loop enters second is != 0 only under the first.
    The census does not leave on "every lane covered", so both keep their bits wherever they are 1."""
    tape, want = lowered(CS.covered())
    assert 'mr_mask mr_racc' in tape.jit_source_census and ' && !mr_covered(' not in tape.jit_source_census
    counts, el = CS.nonzero_counts(tape, W, 0, H), CS.eligible_guards(tape)
    inside = np.zeros(counts.shape[0], np.int64)         # pixels of each rectangle inside the picture
    for r in range(counts.shape[0]):
        grp, tile = divmod(r, 8)
        inside[r] = max(0, min(64, W - 64 * tile)) * min(32, H - 32 * grp)
    full = (counts == inside[:, None]) & (inside[:, None] > 0) & el[None, :]
    assert full[inside > 0].all(axis=0).sum() == 2      # two shapes are 1 on every pixel of every rectangle that has pixels
    got, _ = three_renders(tape, want)
    pos, _, _, _ = tape.guard_layout()
    for r, g in zip(*np.nonzero(full)):
        assert (int(got[r, pos[g] // 64]) >> int(pos[g] % 64)) & 1, (r, g)


def test_three_colours():
    """An f64 max reduction: three colours, one of them on a shape that shows in no pixel of some of its rectangles."""
    tape, want = lowered(CS.three_colours())
    assert 'double mr_racc' in tape.jit_source_census
    three_renders(tape, want)


def test_parameters():
    """A leaf that reads a PIXEL-read parameter keeps its bit -- at c = 0 it is zero on every pixel -- and renders under two
    values of it share one census; another value of the ROW-read parameter is another key with a census of its own."""
    color, decl = CS.pixel_param()
    spec = dict(color=color, params=decl)
    scene, _ = PR.declared(spec, (W, H))
    tape = scene.lower()
    assert tape.info['row_params'] == 1
    el, (pos, _, _, _) = CS.eligible_guards(tape), tape.guard_layout()
    assert el.sum() == 3 and ((pos >= 0) & ~el).sum() == 1

    def oracle(values):
        return PR.oracle_frame(spec, (W, H), values, want_f64=False)[0]

    on, off = context(tape), context(tape, census=False)
    for i in range(3):
        assert np.array_equal(rows(on, W, H, 0, H, (3.0, 0.0)), oracle((3.0, 0.0))), i
    assert on.census_count == 1 and on.launch_counts[0] == 1
    a = on.debug_census_words()
    assert np.array_equal(a, CS.words(tape, W, 0, H, params=(3.0, 0.0)))
    # the leaf with the parameter is zero everywhere at c = 0, and the numpy side keeps its bit because it is not eligible
    assert np.array_equal(a, CS.words(tape, W, 0, H, params=(3.0, 1.0)))
    for c in (1.0, 0.5, 0.0):
        assert np.array_equal(rows(on, W, H, 0, H, (3.0, c)), oracle((3.0, c))), c
    assert on.census_count == 1 and on.launch_counts[0] == 1 and np.array_equal(on.debug_census_words(), a)
    for i in range(2):                                  # ROW-read: a new key, its ROW pass, and on its second launch its census
        assert np.array_equal(rows(on, W, H, 0, H, (-40.5, 1.0)), oracle((-40.5, 1.0)))
        assert (on.census_count, on.launch_counts[0]) == (1 + i, 2)
    b = on.debug_census_words()
    assert np.array_equal(b, CS.words(tape, W, 0, H, params=(-40.5, 1.0))) and not np.array_equal(a, b)
    for v in ((3.0, 0.0), (3.0, 1.0), (-40.5, 1.0)):
        assert np.array_equal(rows(off, W, H, 0, H, v), oracle(v))
    assert off.census_count == 0
    on.close()
    off.close()


def test_without_row_reuse():
    """MARAY_JIT_ROW_REUSE=0: every launch writes the words again -- no census launch, the same pixels."""
    data = RS.data('mixed', 0)
    tape, want = M.Scene(data).lower(), OScene(data).render_rows(W, H, 0, H, want_f64=False)[0]
    ctx = context(tape, reuse=False)
    for i in range(3):
        assert np.array_equal(rows(ctx, W, H, 0, H), want), i
    assert ctx.census_count == 0 and ctx.launch_counts[0] == 3
    assert np.array_equal(ctx.debug_census_words(), CS.words(tape, W, 0, H, census=False))
    ctx.close()


_BLOCKS = r"""
import hashlib, json, os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from test_gpu_census import context, chess
tape, _ = chess()
w = h = 1024
blk, stride, n = 64, 128, 8
pick = (np.arange(n)[:, None] * stride + np.arange(blk)[None, :]).reshape(-1)
whole = context(tape, census=False).render_rows(w, h, 0, h, want_f64=False)[0]
assert hashlib.sha256(whole.tobytes()).hexdigest() == json.load(open(os.path.join(%(golden)r, 'chess_1024.json')))['rgb8_sha256']
for census in (True, False):
    ctx = context(tape, census=census)
    d = torch.zeros((n * blk, w, 3), dtype=torch.uint8, device='cuda')
    for i in range(3):
        d.zero_()
        torch.cuda.synchronize()
        ctx.render_blocks_device(w, h, 0, blk, stride, n, d_rgb8=d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), whole[pick]), (census, i)
        assert ctx.census_count == (1 if census and i else 0), (census, i, ctx.census_count)
    words = ctx.debug_census_words()
    ctx.close()
    if census: after = words
    else: assert not (after & ~words).any() and (words & ~after).any()          # a proper subset of the refined words
print('blocks ok')
"""


def test_interleaved_blocks():
    """render_blocks_device with blocks of 64 rows 128 apart in one launch, as the benchmark issues it, against the rows of
    the whole frame.  A process of its own: the device buffers come from PyTorch, imported before the library."""
    code = _BLOCKS % {'root': ROOT, 'tests': HERE, 'golden': GOLDEN}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('blocks ok'), r.stdout[-2000:] + r.stderr[-4000:]
