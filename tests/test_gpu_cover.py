"""The cover of guarded ORs on the device (maray_jit_cover, maray_jit_cover_apply, maray_jit_pixels_cov): behind a
set's census the set gets a third table of guard words in which a rectangle that an OR of shapes covers on every pixel has the
OR's cover bit set and the OR's eligible leaf bits cleared, and a set with such a bit is rendered by maray_jit_pixels_cov over
that table.  The words the third launch of a geometry read (Context.debug_cover_words) are the numpy evaluator's
(tests/cover_scenes.py) bit for bit; the census'd and the refined words stay what they were; every raster equals the oracle's
and the raster of a context created with MARAY_JIT_GUARD_COVER=0."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import census_scenes as CS
import cover_scenes as CV
import params as PR
from conftest import GOLDEN
from marayb import encode
from oracle_ffi import Scene as OScene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = CV.W, CV.H


def context(tape, cover=True, **kw):
    """A MARAY_BACKEND_JIT context; cover=False: created with MARAY_JIT_GUARD_COVER=0 (read when the context is created)."""
    old = os.environ.get('MARAY_JIT_GUARD_COVER')
    os.environ['MARAY_JIT_GUARD_COVER'] = '1' if cover else '0'
    try:
        return M.Context(tape, backend=M.BACKEND_JIT, **kw)
    finally:
        if old is None:
            del os.environ['MARAY_JIT_GUARD_COVER']
        else:
            os.environ['MARAY_JIT_GUARD_COVER'] = old


def rows(ctx, w, h, y0, y1, values=None, want_f64=False):
    if values is not None:
        ctx.set_params(list(values))
    return ctx.render_rows(w, h, y0, y1, want_f64=want_f64)


def three_renders(tape, want, w=W, h=H, y0=0, y1=H, values=None, want64=None):
    """Three renders of one geometry with the knob on and off; returns (the words the third launch read, covered by numpy)."""
    vb, cb, cov = CV.words(tape, w, y0, y1 - y0, params=values)
    refined = CS.words(tape, w, y0, y1 - y0, params=values, census=False)
    assert tape.cover_bits()
    on, off = context(tape), context(tape, cover=False)
    try:
        for i in range(3):
            got8, got64 = rows(on, w, h, y0, y1, values, want_f64=want64 is not None)
            assert np.array_equal(got8, want), i
            if want64 is not None:
                assert np.array_equal(got64.view(np.uint64), want64.view(np.uint64)), i
            # (the accessors wait for the context's work: the count of the second launch's cover has arrived by the third)
            assert np.array_equal(on.debug_census_words(), cb if i else refined), i
            assert (on.census_count, on.cover_count) == ((1, 1) if i else (0, 0)), i
        got = on.debug_cover_words()
        assert np.array_equal(got, vb), (cov.sum(), [(hex(int(a)), hex(int(b))) for a, b in zip(got.reshape(-1), vb.reshape(-1)) if a != b][:8])
        assert np.array_equal(on.debug_census_words(), cb) and np.array_equal(on.debug_guard_words(), refined)
        for i in range(3):
            got8, got64 = rows(off, w, h, y0, y1, values, want_f64=want64 is not None)
            assert np.array_equal(got8, want), i
            if want64 is not None:
                assert np.array_equal(got64.view(np.uint64), want64.view(np.uint64)), i
        assert (off.census_count, off.cover_count) == (1, 0)
        assert np.array_equal(off.debug_cover_words(), cb) and np.array_equal(off.debug_census_words(), cb)
    finally:
        on.close()
        off.close()
    return got, cov


def lowered(color, want_f64=False):
    data = encode((W, H), color)
    o8, o64 = OScene(data).render_rows(W, H, 0, H, want_f64=want_f64)
    return M.Scene(data).lower(), o8, o64


def rect(tile, group):
    return group * 8 + tile         # 320 pixels: two tiles of four rectangles


def test_one_shape():
    """A shape that holds one whole rectangle by itself (and four of its neighbours)."""
    tape, want, _ = lowered(CV.one_shape())
    got, cov = three_renders(tape, want)
    assert cov[rect(1, 0), 0] and cov[:, 0].sum() == 5
    # no word has a bit that no guard uses, but for the cover bit; the ROW pass and the second bounds leave those bits 0
    pos, n_words, _, _ = tape.guard_layout()
    used = np.zeros(n_words, np.uint64)
    for p in pos[pos >= 0]:
        used[int(p) // 64] |= np.uint64(1) << np.uint64(int(p) % 64)
    bit = tape.cover_bits()[0]
    assert not (got[:, -1] & ~used[-1] & ~(np.uint64(1) << np.uint64(bit % 64))).any()


def test_two_shapes_together():
    """Two shapes hold one rectangle only together, along a diagonal through it."""
    tape, want, _ = lowered(CV.two_together())
    _, cov = three_renders(tape, want)
    assert cov[:, 0].sum() == 1 and cov[rect(1, 0), 0]
    # neither does alone
    one = M.Scene(encode((W, H), CV._scene([CV._tri([(60, -4), (130, -4), (60, 66)])]))).lower()
    two = M.Scene(encode((W, H), CV._scene([CV._tri([(130, 40), (80, 40), (130, -10)])]))).lower()
    assert not CV.covered(one, W, 0, H).any() and not CV.covered(two, W, 0, H).any()


def test_all_but_one_pixel():
    """A shape over the whole picture but for one pixel in each of three rectangles: lane 0 of a first row, lane 63 of a last
    row, a middle row.  Those three are not covered, every other rectangle with pixels is."""
    tape, want, _ = lowered(CV.holes())
    _, cov = three_renders(tape, want)
    missing = {rect(px // 64, py // 32) for px, py in CV.HOLES}
    assert len(missing) == 3
    for g in range(3):
        for t in range(5):
            assert cov[rect(t, g), 0] == (rect(t, g) not in missing), (t, g)
    assert not cov[[rect(t, g) for g in range(3) for t in (5, 6, 7)], 0].any()           # no pixel inside the picture: not covered


def test_ragged_rectangle_and_last_group():
    """300 pixels: the fifth rectangle has 44 lanes inside the picture, and is covered; so are the rectangles of the 8-row group."""
    data = encode((W, H), CV.whole())
    tape = M.Scene(data).lower()
    _, cov = three_renders(tape, OScene(data).render_rows(300, H, 0, H, want_f64=False)[0], w=300)
    assert cov[[rect(t, g) for g in range(3) for t in range(5)], 0].all() and cov.sum() == 15


def test_y_factor_fails_on_a_row():
    """The covering leaf is 0 on row 10 through a y factor: the first group's rectangles are not covered."""
    tape, want, _ = lowered(CV.row_out())
    _, cov = three_renders(tape, want)
    assert not cov[:8, 0].any() and cov[8:, 0].sum() == 10


def test_f64_planes():
    tape, want, want64 = lowered(CV.one_shape(), want_f64=True)
    three_renders(tape, want, want64=want64)


def test_f64_reduction_beside_a_boolean_one():
    tape, want, _ = lowered(CV.with_colours())
    assert len(tape.cover_bits()) == 1
    _, cov = three_renders(tape, want)
    assert cov.any()


def test_two_boolean_reductions():
    tape, want, _ = lowered(CV.two_ors())
    assert len(tape.cover_bits()) == 2
    _, cov = three_renders(tape, want)
    assert cov[:, 0].sum() != cov[:, 1].sum() and cov[:, 0].any() and cov[:, 1].any()


def test_parameter_in_a_covering_leaf():
    """The covering leaf reads a parameter c.  A boolean leaf's guard bounds the leaf over its rectangles, so the ROW section reads
    c as well (no scene made here has a boolean leaf with a parameter that only PIXEL ops read; the emitter leaves such a leaf
    out of the measurement like the census does, tape.cover_plan() says which): c is part of the set's key, the leaf counts, and
    the value at which it stops covering is another key with a cover of its own.  Every raster follows the oracle."""
    color, decl = CV.pixel_param()
    spec = dict(color=color, params=decl)
    scene, _ = PR.declared(spec, (W, H))
    tape = scene.lower()
    assert tape.info['row_params'] == 3 and not any(l[2] for r in tape.cover_plan() for l in r['leaves'])
    _, cov = three_renders(tape, PR.oracle_frame(spec, (W, H), (3.0, 1.0), want_f64=False)[0], values=(3.0, 1.0))
    assert cov.sum() == 15
    on = context(tape)
    for n, c in enumerate((1.0, 1.0, 1.0, 0.25, 0.25, 0.25)):
        assert np.array_equal(rows(on, W, H, 0, H, (3.0, c))[0], PR.oracle_frame(spec, (W, H), (3.0, c), want_f64=False)[0]), c
        on.debug_census_words()
    assert on.cover_count == 2
    vb, _, cov = CV.words(tape, W, 0, H, params=(3.0, 0.25))
    assert 0 < cov.sum() < 15 and np.array_equal(on.debug_cover_words(), vb)
    assert np.array_equal(rows(on, W, H, 0, H, (3.0, 1.0))[0], PR.oracle_frame(spec, (W, H), (3.0, 1.0), want_f64=False)[0])
    on.close()


def test_row_read_parameter():
    """Another value of a parameter the ROW section reads is another key: its own census and its own cover."""
    color, decl = CV.row_param()
    spec = dict(color=color, params=decl)
    scene, _ = PR.declared(spec, (W, H))
    tape = scene.lower()
    assert tape.info['row_params'] == 1
    on = context(tape)
    seen = []
    for n, t in enumerate((3.0, -40.0)):
        vb, _, cov = CV.words(tape, W, 0, H, params=(t,))
        assert cov.any()
        for i in range(3):
            assert np.array_equal(rows(on, W, H, 0, H, (t,))[0], PR.oracle_frame(spec, (W, H), (t,), want_f64=False)[0]), (t, i)
            on.debug_census_words()
        assert (on.census_count, on.cover_count) == (n + 1, n + 1)
        assert np.array_equal(on.debug_cover_words(), vb)
        seen.append(vb)
    assert not np.array_equal(seen[0], seen[1])
    on.close()


def test_tainted_leaf_is_not_counted():
    """The one leaf that is 1 on every pixel holds a Sin whose argument is not provably bounded: tainted (it may defer its tile),
    left out of the measurement, and so nothing is covered although the OR is 1 everywhere."""
    tape, want, _ = lowered(CV.tainted())
    assert [sum(l[2] for l in r['leaves']) for r in tape.cover_plan()] == [1]
    _, cov = three_renders(tape, want)
    assert not cov.any()


@pytest.mark.parametrize('scene', ['shared_ors', 'shared_with_colours'])
def test_reductions_that_share_guard_bits(scene):
    """Two reductions over the same geometry have leaves on the same guard bits.  The OR that is covered everywhere gets its cover
    bit in every rectangle; the shared bits stay set there, and the other reduction -- covered nowhere -- paints what it painted."""
    tape, want, _ = lowered(getattr(CV, scene)())
    plan = tape.cover_plan()
    shared = [l[1] for l in plan[0]['leaves'] if not l[3]]
    assert len(shared) == 4 and len(plan[0]['leaves']) == 5
    got, cov = three_renders(tape, want)
    assert cov[:, 0].sum() == 15 and not cov[:, 1:].any()
    _, cb, _ = CV.words(tape, W, 0, H)
    keep = np.uint64(sum(1 << b for b in shared))
    assert np.array_equal(got[:, 0] & keep, cb[:, 0] & keep) and (cb[:, 0] & keep).any()


_chess = {}


def chess(scale=1):
    if scale not in _chess:
        s = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read())
        if scale > 1:
            s.rescale(scale, scale)
        _chess[scale] = (s.lower(), OScene(s.encode()))
    return _chess[scale]


@pytest.mark.parametrize('scale,w,y0,y1', [(1, 256, 640, 896), (1, 320, 600, 672), (4, 1024, 2560, 2816), (4, 1280, 2400, 2472)])
def test_chess_windows(scale, w, y0, y1):
    """256 x 256 at rows 640-896 and 320 x 72 at rows 600-672 of the board of the committed 1024^2 chess scene, and the same two
    regions of the scene rescaled to 4096^2 (1024 x 256 and 1280 x 72).  Three of the four hold covered rectangles (1, 28 and 15).
    The 256 x 256 window at 1024^2 holds none: there the board's OR is 1 on at most 0.946 of the in-picture pixels of any of its
    32 rectangles (every leaf on every pixel), so that window checks words and rasters, and its region is asserted at 4096^2."""
    tape, oracle = chess(scale)
    _, cov = three_renders(tape, oracle.render_rows(w, 1024 * scale, y0, y1, want_f64=False)[0], w=w, h=1024 * scale, y0=y0, y1=y1)
    if (scale, w) != (1, 256):
        assert cov.any()
    if scale == 4:
        assert cov.sum() >= 15


_BLOCKS = r"""
import hashlib, json, os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
from test_gpu_cover import context, chess
tape, _ = chess()
w = h = 1024
blk, stride, n = 64, 128, 8
pick = (np.arange(n)[:, None] * stride + np.arange(blk)[None, :]).reshape(-1)
whole = context(tape, cover=False).render_rows(w, h, 0, h, want_f64=False)[0]
assert hashlib.sha256(whole.tobytes()).hexdigest() == json.load(open(os.path.join(%(golden)r, 'chess_1024.json')))['rgb8_sha256']
for cover in (True, False):
    ctx = context(tape, cover=cover)
    d = torch.zeros((n * blk, w, 3), dtype=torch.uint8, device='cuda')
    for i in range(4):
        d.zero_()
        torch.cuda.synchronize()
        ctx.render_blocks_device(w, h, 0, blk, stride, n, d_rgb8=d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), whole[pick]), (cover, i)
        assert ctx.cover_count == (1 if cover and i else 0), (cover, i, ctx.cover_count)
    words, census = ctx.debug_cover_words(), ctx.debug_census_words()
    bit = tape.cover_bits()[0]
    has = ((words[:, bit // 64] >> np.uint64(bit %% 64)) & np.uint64(1)).astype(bool)
    assert has.any() == cover and (cover or np.array_equal(words, census))
    ctx.close()
print('blocks ok')
"""


def test_interleaved_blocks():
    """render_blocks_device with blocks of 64 rows 128 apart in one launch, as the benchmark issues it, against the rows of the
    whole frame: the fourth launch has read words with cover bits.  A process of its own: the device buffers come from PyTorch."""
    code = _BLOCKS % {'root': ROOT, 'tests': HERE, 'golden': GOLDEN}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('blocks ok'), r.stdout[-2000:] + r.stderr[-4000:]
