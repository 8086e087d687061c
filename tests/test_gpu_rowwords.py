"""Row words on the device (maray_jit_rowscan, maray_jit_rowscan_apply, maray_jit_pixels_rw): behind a set's cover the
set gets the words of every (rectangle, row) and a fourth table of guard words in which the rectangles whose rows differ from
their band carry the row flag; a set with a flag is rendered by maray_jit_pixels_rw.  The fourth table and the flagged
rectangles' row words (Context.debug_row_words) are the numpy model's (tests/rowwords_scenes.py) bit for bit; every raster equals
the oracle's and the raster of a context created with MARAY_JIT_ROW_WORDS=0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import cover_scenes as CV
import params as PR
import rowwords_scenes as RW
from conftest import GOLDEN
from marayb import encode
from oracle_ffi import Scene as OScene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = RW.W, RW.H


def context(tape, rowwords=True, env=None, **kw):
    """A MARAY_BACKEND_JIT context; rowwords=False: created with MARAY_JIT_ROW_WORDS=0 (read when the context is created)."""
    env = dict(env or {}, MARAY_JIT_ROW_WORDS='1' if rowwords else '0')
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return M.Context(tape, backend=M.BACKEND_JIT, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def rows(ctx, w, h, y0, y1, values=None, want_f64=False):
    if values is not None:
        ctx.set_params(list(values))
    return ctx.render_rows(w, h, y0, y1, want_f64=want_f64)


def check_words(ctx, model):
    """The context's fourth table and row words against the model's; returns whether the last launch ran maray_jit_pixels_rw."""
    xb, rw, used = ctx.debug_row_words()
    assert np.array_equal(xb, model['xbits']), [(i, hex(int(a)), hex(int(b))) for i, (a, b) in enumerate(zip(xb.reshape(-1), model['xbits'].reshape(-1))) if a != b][:8]
    sel = RW.flagged_rows(model)
    got = rw.reshape(model['rwords'].shape)
    assert np.array_equal(got[sel], model['rwords'][sel]), [(int(r), int(t), [hex(int(v)) for v in got[r, t]], [hex(int(v)) for v in model['rwords'][r, t]])
                                                             for r, t in zip(*np.nonzero((got != model['rwords']).any(axis=2) & sel))][:6]
    return used


def four_renders(tape, want, w=W, h=H, y0=0, y1=H, values=None, want64=None, threshold=None):
    """Four renders of one geometry with the knob on and off: the second takes census, cover and scan, the third (which waits
    for nothing: the accessor between the launches has) and the fourth read the row words where a rectangle is flagged."""
    model = RW.row_words(tape, w, y0, y1 - y0, params=values, threshold=threshold)
    env = {} if threshold is None else {'MARAY_ROW_WORDS_T': str(threshold)}
    on, off = context(tape, env=env), context(tape, rowwords=False)
    try:
        for i in range(4):
            got8, got64 = rows(on, w, h, y0, y1, values, want_f64=want64 is not None)
            assert np.array_equal(got8, want), i
            if want64 is not None:
                assert PR.same_f64(got64, want64), i
            assert on.rowscan_count == (1 if i else 0), i
            xb, _, used = on.debug_row_words()
            assert (len(xb) > 0) == (i > 0) and used == (i >= 2 and bool(model['flagged'].any())), (i, used)
        assert check_words(on, model) == bool(model['flagged'].any())
        for i in range(3):
            got8, got64 = rows(off, w, h, y0, y1, values, want_f64=want64 is not None)
            assert np.array_equal(got8, want), i
            if want64 is not None:
                assert PR.same_f64(got64, want64), i
        assert off.rowscan_count == 0 and len(off.debug_row_words()[0]) == 0 and off.cover_count == on.cover_count == 1
    finally:
        on.close()
        off.close()
    return model


def lowered(color, want_f64=False, w=W):
    data = encode((W, H), color)
    o8, o64 = OScene(data).render_rows(w, H, 0, H, want_f64=want_f64)
    return M.Scene(data).lower(), o8, o64


def rect(tile, group):
    return group * 8 + tile         # 320 pixels: two tiles of four rectangles


def test_edge_in_the_middle_of_a_band():
    """Rows 0 .. 15 covered, 16 .. 31 empty: the five rectangles of the first band are flagged, each row is all or nothing."""
    tape, want, _ = lowered(RW.edge_mid_band())
    m = four_renders(tape, want)
    assert m['flagged'][:5].all() and m['changed'][:5].all()
    assert m['cover_rows'][0][:16, :5].all() and not m['cover_rows'][0][16:].any()


def test_edge_on_a_band_boundary():
    tape, want, _ = lowered(RW.edge_on_boundary())
    m = four_renders(tape, want)
    assert not m['changed'][:8].any() and not m['flagged'][:8].any()            # (the filler's triangles end inside the second band)


def test_slanted_edge_alone():
    """No row changes, nothing is flagged, maray_jit_pixels_rw is not taken."""
    tape, want, _ = lowered(RW.slanted())
    m = four_renders(tape, want)
    assert not m['flagged'].any() and not m['changed'].any()


@pytest.mark.parametrize('scene', ['all_but_one', 'one_row'])
def test_both_sides_of_the_threshold_by_rows(scene):
    """31 of a band's 32 rows covered, and one row alone: the band is mixed, every row of it is all or nothing."""
    tape, want, _ = lowered(getattr(RW, scene)())
    m = four_renders(tape, want)
    assert m['flagged'].any() and m['changed'].sum(axis=1).max() == 32 and int(m['cover_rows'][0].sum()) in (5 * 31, 5)


@pytest.mark.parametrize('threshold,some', [(1, True), (8, False), (16, False)])
def test_both_sides_of_the_threshold(threshold, some):
    """A few changed rows in a rectangle that a slanted shape keeps mixed: flagged from a threshold of 1, not from 8 or 16."""
    tape, want, _ = lowered(RW.few_rows())
    m = four_renders(tape, want, threshold=threshold)
    assert 0 < m['changed'].sum(axis=1).max() < 8
    assert bool(m['flagged'].any()) == some


def test_ragged_rectangle_and_last_band():
    """300 pixels wide: the fifth rectangle has 44 lanes inside the picture; rows 60 .. 67 cross the 8-row band."""
    tape, want, _ = lowered(RW.ragged(), w=300)
    m = four_renders(tape, want, w=300)
    assert m['flagged'][[rect(4, 1), rect(4, 2), rect(0, 2)]].all() and not m['flagged'][[rect(5, 1), rect(7, 2)]].any()


def test_y_factor_fails_on_a_row():
    tape, want, _ = lowered(CV.row_out())
    m = four_renders(tape, want)
    assert m['flagged'][:5].all() and not m['cover_rows'][0][10].any() and m['cover_rows'][0][9, :5].all()


def test_tainted_leaf_is_not_counted():
    tape, want, _ = lowered(RW.tainted_rows())
    assert [sum(l[2] for l in r['leaves']) for r in tape.cover_plan()] == [1]
    m = four_renders(tape, want)
    assert not any(c.any() for c in m['cover_rows'])


def test_two_boolean_reductions():
    tape, want, _ = lowered(RW.two_ors())
    assert len(tape.cover_bits()) == 2
    m = four_renders(tape, want)
    assert m['cover_rows'][0].any() and m['cover_rows'][1].any() and m['flagged'].any()


def test_reductions_that_share_guard_bits():
    """The shared leaf bits are not cleared on a covered row: the other OR still paints from them."""
    tape, want, _ = lowered(RW.shared_ors())
    plan = tape.cover_plan()
    shared = [l[1] for l in plan[0]['leaves'] if not l[3]] + [l[1] for l in plan[1]['leaves'] if not l[3]]
    assert shared
    m = four_renders(tape, want)
    sel = RW.flagged_rows(m)
    band = m['band'][(np.arange(H) // 32)[:, None] * 8 + np.arange(8)[None, :]]
    kept_under_cover = False
    for b in set(shared):           # a shared bit goes only where every leaf on it is 0 on the row (the census's rule), never under a cover
        assert np.array_equal(RW._bit(m['rwords'], b)[sel], (RW._bit(band, b) & m['hit_rows'][b])[sel]), b
        kept_under_cover |= bool((RW._bit(m['rwords'], b) & (m['cover_rows'][0] | m['cover_rows'][1]) & sel).any())
    assert m['flagged'].any() and (m['cover_rows'][0] | m['cover_rows'][1]).any() and kept_under_cover


def test_f64_reduction_beside_a_boolean_one():
    tape, want, _ = lowered(RW.with_colours())
    m = four_renders(tape, want)
    assert m['flagged'].any()


def test_f64_planes():
    tape, want, want64 = lowered(RW.edge_mid_band(), want_f64=True)
    four_renders(tape, want, want64=want64)


def test_pixel_read_parameter():
    """census_scenes.pixel_param: an f64 max tree whose first shape is scaled by c, a parameter only PIXEL ops read.  That leaf
    is tainted: its bit is not eligible and no row clears it, whatever c is -- at c = 0 the leaf is 0 on every pixel.  The program
    has no cover bit, so the scan runs behind the census; one scan serves the whole sweep of c, and every raster follows the
    oracle."""
    import census_scenes as CS
    color, decl = CS.pixel_param()
    spec = dict(color=color, params=decl)
    scene, _ = PR.declared(spec, (W, H))
    tape = scene.lower()
    pos, el = [int(p) for p in tape.guard_layout()[0]], tape.census_eligible()
    kept = [p for p in pos if p >= 0 and not (int(el[p // 64]) >> (p % 64)) & 1]
    assert tape.rowwords_flag() >= 0 and tape.info['row_params'] == 1 and tape.cover_bits() == [] and len(kept) == 1
    model = RW.row_words(tape, W, 0, H, params=(3.0, 0.0))
    band = model['band'][(np.arange(H) // model['gh'])[:, None] * model['n_rect'] + np.arange(model['n_rect'])[None, :]]
    assert model['flagged'].any() and np.array_equal(RW._bit(model['rwords'], kept[0]), RW._bit(band, kept[0])) and RW._bit(band, kept[0]).any()
    assert np.array_equal(model['rwords'], RW.row_words(tape, W, 0, H, params=(3.0, 1.0))['rwords'])
    on, off = context(tape), context(tape, rowwords=False)
    try:
        for c in (1.0, 1.0, 1.0, 0.25, 0.1, 0.25, 1.0, 0.0):
            want = PR.oracle_frame(spec, (W, H), (3.0, c), want_f64=False)[0]
            assert np.array_equal(rows(on, W, H, 0, H, (3.0, c))[0], want), c
            assert np.array_equal(rows(off, W, H, 0, H, (3.0, c))[0], want), c
            on.debug_row_words()
        assert on.rowscan_count == 1 and on.cover_count == 0 and on.census_count == 1
        assert check_words(on, model)
    finally:
        on.close()
        off.close()


def test_row_read_parameter():
    """Another value of a parameter the ROW section reads is another key: the flag is withdrawn with the census, a second scan."""
    color, decl = RW.row_param()
    spec = dict(color=color, params=decl)
    scene, _ = PR.declared(spec, (W, H))
    tape = scene.lower()
    assert tape.info['row_params'] == 1
    on = context(tape)
    try:
        for n, t in enumerate((0.0, 5.0)):
            model = RW.row_words(tape, W, 0, H, params=(t,))
            assert model['flagged'].any()
            for i in range(4):
                assert np.array_equal(rows(on, W, H, 0, H, (t,))[0], PR.oracle_frame(spec, (W, H), (t,), want_f64=False)[0]), (t, i)
                on.debug_row_words()
            assert on.rowscan_count == n + 1
            assert check_words(on, model)
    finally:
        on.close()


_STREAMS = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
import rowwords_scenes as RW
from test_gpu_rowwords import context, lowered, check_words, W, H
tape, want, _ = lowered(RW.edge_mid_band())
model = RW.row_words(tape, W, 0, H)
on = context(tape)
streams = [torch.cuda.Stream(), torch.cuda.Stream()]
d = torch.zeros((H, W, 3), dtype=torch.uint8, device='cuda')
for i in range(6):
    s = streams[i %% 2]
    d.zero_()
    torch.cuda.synchronize()
    on.render_rows_device(W, H, 0, H, d_rgb8=d.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(d.cpu().numpy().reshape(want.shape), want), i
assert on.rowscan_count == 1 and check_words(on, model)
on.close()
print('streams ok')
"""


def test_two_streams_in_turn():
    """Launches that alternate between two streams: the scan's kernels and the flag count follow the context's hand-over.  A
    process of its own: the streams and the buffer come from PyTorch."""
    code = _STREAMS % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('streams ok'), r.stdout[-2000:] + r.stderr[-4000:]


def test_budget_too_small():
    """A budget the row words do not fit: the set takes none, rasters are what they were."""
    tape, want, _ = lowered(RW.edge_mid_band())
    on = context(tape, env={'MARAY_ROW_KEPT_BYTES': '4096'})
    try:
        for i in range(4):
            assert np.array_equal(rows(on, W, H, 0, H)[0], want), i
        xb, _, used = on.debug_row_words()
        assert on.rowscan_count == 0 and len(xb) == 0 and not used and on.census_count == 1
    finally:
        on.close()


_chess = {}


def chess(scale=1):
    if scale not in _chess:
        s = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read())
        if scale > 1:
            s.rescale(scale, scale)
        _chess[scale] = (s.lower(), OScene(s.encode()))
    return _chess[scale]


@pytest.mark.parametrize('scale,w,y0,y1', [(1, 1024, 512, 576), (1, 320, 600, 672), (4, 4096, 2176, 2240)])
def test_chess_windows(scale, w, y0, y1):
    """Windows of the committed chess scene over a horizontal cell boundary: at 1024^2, and band 68 (64 rows) of the scene
    rescaled to 4096^2."""
    tape, oracle = chess(scale)
    m = four_renders(tape, oracle.render_rows(w, 1024 * scale, y0, y1, want_f64=False)[0], w=w, h=1024 * scale, y0=y0, y1=y1)
    assert m['flagged'].any()


_BLOCKS = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
import cover_fuzz_scenes as F
import rowwords_scenes as RW
from test_gpu_cover_fuzz import oracle
from test_gpu_rowwords import context
case = ('two', 0, F.B)
tape, color, _, _, _ = F.lowered(case)
w, h = case[2][:2]
y0, blk, stride, n = 0, 32, 64, 3
want = np.concatenate([oracle(color, None, None, (w, h, y0 + i * stride, y0 + i * stride + blk), want_f64=False)[0] for i in range(n)])
# the model of the launch: a band never straddles two blocks, so its tables are the blocks' own, one after the other
parts = [RW.row_words(tape, w, y0 + i * stride, blk) for i in range(n)]
xbits, rwords = np.concatenate([p['xbits'] for p in parts]), np.concatenate([p['rwords'] for p in parts])
flagged = np.concatenate([RW.flagged_rows(p) for p in parts])
assert all(p['flagged'].any() for p in parts)                     # every block holds a flagged rectangle: rows of all three are read from rwords
for on in (True, False):
    ctx = context(tape, rowwords=on)
    d = torch.zeros((n * blk, w, 3), dtype=torch.uint8, device='cuda')
    for i in range(4):
        d.zero_()
        torch.cuda.synchronize()
        ctx.render_blocks_device(w, h, y0, blk, stride, n, d_rgb8=d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), want), (on, i)
        assert ctx.rowscan_count == (1 if on and i else 0), (on, i, ctx.rowscan_count)
        xb, rw, used = ctx.debug_row_words()
        assert used == (on and i >= 2), (on, i, used)
    assert (len(xb) > 0) == on
    if on:
        assert np.array_equal(xb, xbits)
        got = rw.reshape(rwords.shape)
        assert np.array_equal(got[flagged], rwords[flagged])
        print('flagged', int(sum(p['flagged'].sum() for p in parts)), 'used', used)
    ctx.close()
print('blocks ok')
"""


def test_interleaved_blocks():
    """render_blocks_device with three blocks of 32 rows 64 apart in one launch, interleaved as the benchmark deals them, over a
    soup of the fuzz (300 x 200): the rasters against the oracle's rows, the fourth table and the flagged rectangles' row words
    against the model of the blocks (every block holds a flagged rectangle), and maray_jit_pixels_rw taken from the third launch
    on.  A process of its own: the device buffers come from PyTorch."""
    code = _BLOCKS % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('blocks ok'), r.stdout[-2000:] + r.stderr[-4000:]
