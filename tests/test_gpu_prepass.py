"""The wide pre-pass on the device (maray_jit_pixels_pp): a busy tile's leafless rectangles -- guard words zero apart
from cover bits -- are rendered four pixels per lane in one pass and the narrow loop runs the leafy rectangles only.  Every
raster equals the oracle's and the raster of a context created with MARAY_JIT_PREPASS=0, byte for byte; prepass_count advances;
the tile-row classes computed from the words the launch read (Context.debug_row_words) are the numpy model's
(tests/prepass_scenes.py).  Every scene carries a background that varies in x and in y, so that a wrong lane-to-pixel mapping
of the pre-pass shows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import params as PR
import prepass_scenes as PP
import rowwords_scenes as RW
from conftest import GOLDEN
from marayb import encode
from oracle_ffi import Scene as OScene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = PP.W, PP.H


def context(tape, prepass=True, env=None, **kw):
    """A MARAY_BACKEND_JIT context; prepass=False: created with MARAY_JIT_PREPASS=0 (read when the context is created)."""
    env = dict(env or {}, MARAY_JIT_PREPASS='1' if prepass else '0')
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


def device_classes(ctx, tape, n_rows):
    """prepass_scenes.classify of the words the context's last launch read."""
    _, _, _, gh = tape.guard_layout()
    xb, rw, _ = ctx.debug_row_words()
    if not len(xb):                             # a set without row words: the third table
        xb, rw = ctx.debug_cover_words(), np.zeros((0, 1), np.uint64)
    return PP.classify(PP.launch_words(xb, rw, tape.rowwords_flag(), n_rows, gh), tape.cover_bits())


def renders(tape, want, w=W, h=H, y0=0, y1=H, values=None, want64=None, threshold=None, classes=PP.CLASSES[1:], pre_passes=True):
    """Four launches with the knob on, three with it off: rasters against `want`, the counter, the classes against the model."""
    env = {} if threshold is None else {'MARAY_ROW_WORDS_T': str(threshold)}
    want_cls, _ = PP.model(tape, w, y0, y1 - y0, params=values, threshold=threshold)
    for k in classes:
        assert want_cls['tile_rows'][k] > 0, (k, want_cls)
    on, off = context(tape, env=env), context(tape, prepass=False, env=env)
    try:
        for ctx, n in ((on, 4), (off, 3)):
            for i in range(n):
                got8, got64 = rows(ctx, w, h, y0, y1, values, want_f64=want64 is not None)
                assert np.array_equal(got8, want), (ctx is on, i, np.argwhere((got8 != want).any(axis=2))[:8])
                if want64 is not None:
                    assert PR.same_f64(got64, want64), (ctx is on, i)
                ctx.debug_row_words()           # (waits: the next launch finds the cover's and the scan's counts)
        assert off.prepass_count == 0 and on.rowscan_count == off.rowscan_count and on.cover_count == off.cover_count
        assert on.prepass_count >= 1, on.prepass_count
        got_cls = device_classes(on, tape, y1 - y0)
        assert got_cls == want_cls, (got_cls, want_cls)
        assert (got_cls['pre_passes'] > 0) == pre_passes
    finally:
        on.close()
        off.close()
    return want_cls


def lowered(color, w=W, h=H, y0=0, y1=None, want_f64=False):
    y1 = h if y1 is None else y1
    data = encode((w, h), color)
    o8, o64 = OScene(data).render_rows(w, h, y0, y1, want_f64=want_f64)
    return M.Scene(data).lower(), o8, o64


# cases 1, 2, 3, 5, 6, 7, 9a of the scenes; case 4 (all four leafy: the narrow loop alone) is a tile-row of every one of them
@pytest.mark.parametrize('scene', ['one_leafy', 'covered_leafy_empty', 'covered_and_empty', 'two_ors', 'with_colours', 'free_leaf', 'sin_in_leaf'])
def test_scene(scene):
    tape, want, _ = lowered(PP.PLAIN[scene]())
    classes = PP.CLASSES[1:] if scene != 'sin_in_leaf' else ('all_leafy', 'mixed')
    c = renders(tape, want, classes=classes)
    assert c['narrow_passes_after'] < c['narrow_passes_before']
    if scene == 'two_ors':
        assert len(tape.cover_bits()) == 2


@pytest.mark.parametrize('scene,w,h,y0,y1', [('covered_leafy_empty', 600, 72, 0, 72), ('two_ors', 600, 72, 0, 72), ('one_leafy', 512, 200, 37, 101)])
def test_other_geometries(scene, w, h, y0, y1):
    """600 x 72: a ragged third tile (slow path) and a last band of 8 rows; rows 37 .. 101 of a 200-row picture."""
    tape, want, _ = lowered(PP.PLAIN[scene](), w=w, h=h, y0=y0, y1=y1)
    renders(tape, want, w=w, h=h, y0=y0, y1=y1, classes=('mixed',))


def test_all_four_leafy_alone():
    """Case 4: a picture whose busy tile-rows are all leafy or all zero takes no pre-pass; the kernel is the new one all the same."""
    import cover_scenes as CV
    u = CV._or(PP._stripe())                    # tile 1 alone holds shapes, one in each of its rectangles
    color = [PP._paint(u), PP._paint(u, 40), PP.gradient()]
    tape, want, _ = lowered(color, h=96, y0=32, y1=64)
    c, _ = PP.model(tape, W, 32, 32)
    if c['tile_rows']['mixed'] or c['tile_rows']['leafless_only']:
        pytest.fail('the scene is meant to have no leafless rectangle in a busy tile: %r' % (c,))
    renders(tape, want, h=96, y0=32, y1=64, classes=('all_leafy',), pre_passes=False)


@pytest.mark.parametrize('threshold,flagged', [(1, True), (33, False)])
def test_both_sides_of_the_row_word_threshold(threshold, flagged):
    """Case 8: a horizontal edge inside the first band (three bands; the third is covered whole, so the set has a cover either
    way).  Flagged, the rows above the edge are covered and the rows below empty, per row; not flagged (a threshold no rectangle
    reaches), the band's words stand and the rectangles under the edge are leafy on every row of the band."""
    h = 96
    tape, want, _ = lowered(PP.edge_in_band(), h=h)
    m = RW.row_words(tape, W, 0, h, threshold=threshold)
    assert bool(m['flagged'].any()) == flagged
    c = renders(tape, want, h=h, y1=h, threshold=threshold)
    other = PP.model(tape, W, 0, h, threshold=34 - threshold)[0]
    assert (c['tile_rows']['leafless_only'] > other['tile_rows']['leafless_only']) == flagged and c != other


def test_deferring_sin_in_the_background():
    """Case 9b: the tiles from x = 106 on are deferred by the background's Sin with or without the pre-pass: the same count."""
    tape, want, _ = lowered(PP.sin_in_background())
    on, off = context(tape), context(tape, prepass=False)
    try:
        counts = []
        for ctx in (on, off):
            for i in range(4):
                assert np.array_equal(rows(ctx, W, H, 0, H)[0], want), (ctx is on, i)
                ctx.debug_row_words()
            counts.append(ctx.deferred_count)
        assert on.prepass_count >= 1 and off.prepass_count == 0
        assert counts[0] == counts[1] and counts[0] >= H, counts
    finally:
        on.close()
        off.close()


def test_deferring_sin_in_a_leafy_rectangle_defers_no_more():
    """Case 9a's count: the Sin sits in a leaf the pre-pass does not evaluate, and its lanes are quiet in the pre-pass."""
    tape, want, _ = lowered(PP.sin_in_leaf())
    on, off = context(tape), context(tape, prepass=False)
    try:
        counts = []
        for ctx in (on, off):
            for i in range(4):
                assert np.array_equal(rows(ctx, W, H, 0, H)[0], want), (ctx is on, i)
                ctx.debug_row_words()
            counts.append(ctx.deferred_count)
        assert on.prepass_count >= 1 and counts[0] == counts[1], counts
    finally:
        on.close()
        off.close()


def test_parameters():
    """Case 10: c, read by PIXEL ops alone, changes between launches of a kept set; t, read by the ROW section, is another key."""
    color, decl = PP.pixel_param()
    spec = dict(color=color, params=decl)
    scene, _ = PR.declared(spec, (W, H))
    tape = scene.lower()
    assert tape.info['row_params'] == 1 and tape.jit_source_prepass
    on, off = context(tape), context(tape, prepass=False)
    try:
        seen = 0
        for t, c in ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0), (0.0, 0.25), (0.0, 2.0), (5.0, 2.0), (5.0, 2.0), (5.0, 2.0), (5.0, 0.5), (0.0, 0.5)):
            want = PR.oracle_frame(spec, (W, H), (t, c), want_f64=False)[0]
            assert np.array_equal(rows(on, W, H, 0, H, (t, c))[0], want), (t, c)
            assert np.array_equal(rows(off, W, H, 0, H, (t, c))[0], want), (t, c)
            on.debug_row_words()
            off.debug_row_words()
            if on.prepass_count > seen:
                seen = on.prepass_count
                assert device_classes(on, tape, H) == PP.model(tape, W, 0, H, params=(t, c))[0], (t, c)
        assert seen >= 4 and off.prepass_count == 0 and on.rowscan_count == 2
    finally:
        on.close()
        off.close()


def test_f64_planes_take_the_existing_path():
    """Case 11: with f64 planes requested the tile is not wide: no pre-pass, the same kernel, identical planes."""
    tape, want, want64 = lowered(PP.covered_leafy_empty(), want_f64=True)
    on, off = context(tape), context(tape, prepass=False)
    try:
        for ctx in (on, off):
            for i in range(4):
                got8, got64 = rows(ctx, W, H, 0, H, want_f64=True)
                assert np.array_equal(got8, want) and PR.same_f64(got64, want64), (ctx is on, i)
                ctx.debug_row_words()
        assert on.prepass_count >= 1 and off.prepass_count == 0
    finally:
        on.close()
        off.close()


_DEVICE = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
import prepass_scenes as PP
from test_gpu_prepass import context, lowered
# an unaligned d_rgb8 (every tile off the fast path), a width that is no multiple of 4 (rows alternate), and the aligned case
for w, shift in ((512, 1), (510, 0), (512, 0)):
    tape, want, _ = lowered(PP.covered_leafy_empty(), w=w)
    got = {}
    for on in (True, False):
        ctx = context(tape, prepass=on)
        buf = torch.zeros(PP.H * w * 3 + 16, dtype=torch.uint8, device='cuda')
        assert buf.data_ptr() %% 16 == 0
        for i in range(4):
            buf.zero_()
            torch.cuda.synchronize()
            ctx.render_rows_device(w, PP.H, 0, PP.H, d_rgb8=buf.data_ptr() + shift)
            torch.cuda.synchronize()
            out = buf.cpu().numpy()
            assert np.array_equal(out[shift:shift + PP.H * w * 3].reshape(want.shape), want), (w, shift, on, i)
            assert not out[:shift].any() and not out[shift + PP.H * w * 3:].any(), (w, shift, on, i)
            ctx.debug_row_words()
        assert (ctx.prepass_count >= 1) == on
        ctx.close()
# interleaved row blocks: three blocks of 32 rows 64 apart in one launch, over a picture of 200 rows
w, h, y0, blk, stride, n = 512, 200, 0, 32, 64, 3
data = M.Scene  # (keep the name in scope)
from marayb import encode
from oracle_ffi import Scene as OScene
color = PP.two_ors()
blob = encode((w, h), color)
tape = M.Scene(blob).lower()
want = np.concatenate([OScene(blob).render_rows(w, h, y0 + i * stride, y0 + i * stride + blk, want_f64=False)[0] for i in range(n)])
for on in (True, False):
    ctx = context(tape, prepass=on)
    d = torch.zeros((n * blk, w, 3), dtype=torch.uint8, device='cuda')
    for i in range(4):
        d.zero_()
        torch.cuda.synchronize()
        ctx.render_blocks_device(w, h, y0, blk, stride, n, d_rgb8=d.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), want), (on, i)
        ctx.debug_row_words()
    assert (ctx.prepass_count >= 1) == on
    ctx.close()
print('device ok')
"""


def test_slow_paths_and_interleaved_blocks():
    """Cases 11 and 12: an unaligned d_rgb8 pointer, a width that is not a multiple of 4, and render_blocks_device.  A process of
    its own: the device buffers come from PyTorch."""
    code = _DEVICE % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('device ok'), r.stdout[-2000:] + r.stderr[-4000:]


_chess = {}


def chess(scale=1):
    if scale not in _chess:
        s = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read())
        if scale > 1:
            s.rescale(scale, scale)
        _chess[scale] = (s.lower(), OScene(s.encode()))
    return _chess[scale]


@pytest.mark.parametrize('scale,w,y0,y1', [(1, 1024, 512, 576), (4, 4096, 2176, 2240)])
def test_chess_windows(scale, w, y0, y1):
    """Case 13: a window over a horizontal cell boundary at 1024^2, and band 68 (64 rows) of the scene rescaled to 4096^2, as
    tests/test_gpu_rowwords.py cuts them."""
    tape, oracle = chess(scale)
    c = renders(tape, oracle.render_rows(w, 1024 * scale, y0, y1, want_f64=False)[0], w=w, h=1024 * scale, y0=y0, y1=y1, classes=('mixed',))
    assert c['narrow_passes_after'] < c['narrow_passes_before']


import cover_fuzz_scenes as F  # noqa: E402

SOUPS = [(c, None) for c in F.PLAIN] + [(c, 1) for c in F.PLANTED]


@pytest.mark.parametrize('case,n_vectors', SOUPS, ids=['%s-%d-%s%s' % (c[0], c[1], 'A' if c[2] == F.A else 'B', '-planted' if n else '') for c, n in SOUPS])
def test_the_twenty_soups(case, n_vectors):
    """tests/cover_fuzz_scenes.py's soups at their own geometries: four launches knob on, three knob off, RGB8 against the oracle."""
    from test_gpu_cover_fuzz import oracle
    tape, color, decl, vectors, _ = F.lowered(case, n_vectors)
    geo, values = case[2], vectors[0]
    want = oracle(color, decl, values, geo, want_f64=False)[0]
    on, off = context(tape), context(tape, prepass=False)
    try:
        for ctx, n in ((on, 4), (off, 3)):
            for i in range(n):
                got = rows(ctx, geo[0], geo[1], geo[2], geo[3], values)[0]
                assert np.array_equal(got, want), (case, ctx is on, i)
                ctx.debug_row_words()
        assert off.prepass_count == 0
        if tape.jit_source_prepass:
            assert on.prepass_count >= 1 and device_classes(on, tape, geo[3] - geo[2]) == PP.model(tape, geo[0], geo[2], geo[3] - geo[2], params=values)[0]
    finally:
        on.close()
        off.close()
