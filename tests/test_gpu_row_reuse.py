"""A specialised context keeps a geometry's ROW outputs while the parameters its ROW section reads are unchanged
(maray_amd/csrc/row_reuse.hpp).  Every raster here is compared byte for byte with a context that has never reused
anything -- a fresh one, or one created with MARAY_JIT_ROW_REUSE=0 -- and the ROW passes and launch-order kernels a context
has enqueued are read from its counters (Context.launch_counts)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import maray_amd as M
import row_reuse_scenes as RS
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
W, H = RS.W, RS.H


def context(tape, reuse=True, **kw):
    """A MARAY_BACKEND_JIT context; reuse=False: created with the knob at 0 (read when the context is created)."""
    old = os.environ.get('MARAY_JIT_ROW_REUSE')
    os.environ['MARAY_JIT_ROW_REUSE'] = '1' if reuse else '0'
    try:
        return M.Context(tape, backend=M.BACKEND_JIT, **kw)
    finally:
        if old is None:
            del os.environ['MARAY_JIT_ROW_REUSE']
        else:
            os.environ['MARAY_JIT_ROW_REUSE'] = old


def rows(ctx, w, h, y0, y1, values=None):
    if values is not None:
        ctx.set_params(list(values))
    return ctx.render_rows(w, h, y0, y1, want_f64=False)[0]


def fresh(tape, w, h, y0, y1, values=None, **kw):
    ctx = context(tape, **kw)
    out = rows(ctx, w, h, y0, y1, values)
    ctx.close()
    return out


_chess = {}


def chess():
    """(tape, {(y0, y1): raster of a knob-off context}) of the committed chess at 1024^2, rendered by rows."""
    if not _chess:
        _chess['tape'] = M.Scene(open(os.path.join(GOLDEN, 'chess.maray'), 'rb').read()).lower()
        _chess['want'] = {}
        _chess['off'] = context(_chess['tape'], reuse=False)
    tape, want, off = _chess['tape'], _chess['want'], _chess['off']

    def get(y0, y1):
        if (y0, y1) not in want:
            want[(y0, y1)] = rows(off, 1024, 1024, y0, y1)
        return want[(y0, y1)]
    return tape, get


@pytest.fixture(scope='module', autouse=True)
def _close_the_reference_context():
    yield
    if _chess:
        _chess.pop('off').close()
        _chess.clear()


A, B = (0, 64), (512, 640)


def test_the_same_geometry_five_times():
    tape, want = chess()
    for g in (A, B):
        ctx = context(tape)
        for i in range(5):
            assert np.array_equal(rows(ctx, 1024, 1024, *g), want(*g)), (g, i)
        assert ctx.launch_counts == (1, 1), g
        ctx.close()
    assert np.array_equal(fresh(tape, 1024, 1024, *B), want(*B))         # the knob-off reference against a fresh context
    _, t = RS.lowered(RS.plain())
    ctx = context(t)
    first = rows(ctx, W, H, 0, H)
    for i in range(4):
        assert np.array_equal(rows(ctx, W, H, 0, H), first)
    assert ctx.launch_counts == (1, 1)              # three guard groups, the last one ragged: an order all the same
    assert np.array_equal(first, fresh(t, W, H, 0, H, reuse=False))
    ctx.close()


def test_the_knob_restores_a_row_pass_per_launch():
    tape, want = chess()
    ctx = context(tape, reuse=False)
    for i in range(4):
        assert np.array_equal(rows(ctx, 1024, 1024, *B), want(*B))
    assert ctx.launch_counts == (4, 1)
    ctx.close()


def test_two_geometries_in_turn_then_more_than_the_kept_sets_hold():
    tape, want = chess()
    ctx = context(tape)
    for rnd in range(3):
        for g in (A, B):
            assert np.array_equal(rows(ctx, 1024, 1024, *g), want(*g)), (rnd, g)
        if rnd == 1:
            after_second = ctx.launch_counts
    # no ROW pass after the second round (an order kernel, yes: the first launch that finds a kept set filled computes its order)
    assert ctx.launch_counts[0] == after_second[0] <= 4
    # nine geometries in rotation: past the count limit of the kept sets (the ninth lives in the scratch); ten: past that too
    for n in (9, 10):
        geoms = [(64 * i + 8, 64 * i + 72) for i in range(n)]
        before = ctx.launch_counts[0]
        per_round = []
        for rnd in range(4):
            for g in geoms:
                assert np.array_equal(rows(ctx, 1024, 1024, *g), want(*g)), (n, rnd, g)
            per_round.append(ctx.launch_counts[0])
        if n == 9:
            assert per_round[0] - before >= n - 1       # the counter grows: every new geometry runs its pass
        else:
            assert per_round[3] > per_round[2] > per_round[1]       # ... and goes on growing when the sets cannot hold the rotation
    ctx.close()


def test_a_tiled_render_three_times():
    """What a context shows of itself is two counters, so "the first call allocates no kept set" is asserted where the sets
    can be seen: tests/native/row_reuse_check.cpp (run by tests/test_row_reuse.py), whose model keeps the three tables'
    capacities per set as the backend does -- its second block is this render (kept_sets == 0 and no kept capacity after the
    first frame, no release and no growth in the third)."""
    _, tape = RS.lowered(RS.plain())
    tiles = [(0, 32), (32, 64), (64, H)]
    want = fresh(tape, W, H, 0, H, reuse=False)
    ctx = context(tape)
    counts = [ctx.launch_counts[0]]
    for call in range(3):
        img = np.zeros((H, W, 3), np.uint8)
        ctx.render_tiles(W, H, tiles, img)
        assert np.array_equal(img, want), call
        counts.append(ctx.launch_counts[0])
    assert counts[1] - counts[0] == len(tiles)      # a one-shot render: one ROW pass per tile (and the scratch set only: the policy's CPU test)
    assert counts[3] == counts[2]                   # the third frame runs none
    ctx.close()


def test_row_read_and_pixel_only_parameters():
    """Parameter 0 moves the shapes in x (ROW-read), parameter 1 scales a colour (PIXEL only)."""
    _, tape = RS.lowered(RS.move_and_colour())
    assert tape.info['row_params'] == 1
    want = {}

    def check(ctx, values, what):
        if values not in want:
            want[values] = fresh(tape, W, H, 0, H, values)
        assert np.array_equal(rows(ctx, W, H, 0, H, values), want[values]), (what, values)

    ctx = context(tape)                             # a ROW-read parameter: a, b, a -- one pass per change
    for k, t in enumerate((3.0, -40.5, 3.0)):
        check(ctx, (t, 0.5), 'row-read')
        assert ctx.launch_counts[0] == k + 1
    ctx.close()
    ctx = context(tape)                             # a PIXEL-only parameter: a, b, a -- one pass, and one order kernel
    for u in (0.25, 1.0, 0.25):
        check(ctx, (3.0, u), 'pixel-only')
        assert ctx.launch_counts[0] == 1
    assert ctx.launch_counts == (1, 1)
    check(ctx, (-40.5, 0.75), 'both at once')
    assert ctx.launch_counts[0] == 2
    ctx.set_params([-40.5, 0.75])                   # identical bits
    check(ctx, (-40.5, 0.75), 'identical bits')
    assert ctx.launch_counts[0] == 2
    check(ctx, (0.0, 0.75), '+0.0')
    check(ctx, (-0.0, 0.75), '-0.0 is another key')
    assert ctx.launch_counts[0] == 4
    ctx.close()
    assert len({w.tobytes() for w in want.values()}) >= 5


def test_colour_animation_pays_one_row_pass():
    """max_i(shape_i . c_i) with both colours moving: no parameter is ROW-read."""
    _, tape = RS.lowered(RS.colour())
    assert tape.info['row_params'] == 0 and tape.param_count == 2
    ctx = context(tape)
    off = context(tape, reuse=False)
    seen = set()
    for k in range(6):
        v = (k / 8.0, 1.0 - k / 5.0)
        got = rows(ctx, W, H, 0, H, v)
        assert np.array_equal(got, rows(off, W, H, 0, H, v)), v
        seen.add(got.tobytes())
    assert len(seen) == 6 and ctx.launch_counts == (1, 1) and off.launch_counts[0] == 6
    ctx.close()
    off.close()


@pytest.mark.parametrize('name', ['colour', 'move_x'])
def test_shutter_of_four_frames(name):
    spec = getattr(RS, name)()
    _, tape = RS.lowered(spec)
    n_par = len(spec[1])
    lo, hi = (0.0, 1.0) if name == 'colour' else (-30.0, 30.0)
    frames = np.array([[lo + (hi - lo) * (k + 0.5) / 4] * n_par for k in range(4)])
    ctx, off = context(tape), context(tape, reuse=False)
    for c in (ctx, off):
        c.set_params([frames[0][0]] * n_par)
    want = off.render_rows_shutter(W, H, 0, H, frames)
    counts = []
    for call in range(3):
        assert np.array_equal(ctx.render_rows_shutter(W, H, 0, H, frames), want), call
        counts.append(ctx.launch_counts[0])
    assert np.array_equal(rows(ctx, W, H, 0, H), rows(off, W, H, 0, H))          # the values from before the call are back
    if name == 'colour':
        assert counts == [1, 1, 1]
    else:
        assert counts[0] == 4 and counts[2] == counts[1] <= 8      # the frames' keys come back: kept from the second call on
    assert off.launch_counts[0] == 4 + 1
    ctx.close()
    off.close()


def test_supersampled_context():
    """k = 2: keyed on the sample grid.  The same geometry twice, then another, then back."""
    _, tape = RS.lowered(RS.plain(), samples=2)
    w, h = W, H                                     # output geometry; the ROW stage covers 512 x 192 samples
    ctx = context(tape, samples=2)
    assert ctx.kernel_name == 'maray_jit_pixels_ss'
    g1, g2 = (0, h), (8, 72)
    want = {g: fresh(tape, w, h, *g, samples=2, reuse=False) for g in (g1, g2)}
    passes = []
    for g in (g1, g1, g2, g1, g2, g1):
        assert np.array_equal(rows(ctx, w, h, *g), want[g]), g
        passes.append(ctx.launch_counts[0])
    assert passes[:3] == [1, 1, 2] and passes[5] == passes[4] and ctx.launch_counts[1] == 0
    ctx.close()


def test_time_rows_then_a_render():
    tape, want = chess()
    ctx = context(tape)
    assert np.array_equal(rows(ctx, 1024, 1024, *B), want(*B))
    ms = ctx.time_rows(1024, 1024, *B, reps=3)
    assert ms > 0.0
    assert ctx.launch_counts == (1, 1)              # its launches found the tables there
    assert np.array_equal(rows(ctx, 1024, 1024, *B), want(*B))
    ctx.time_rows(1024, 1024, *A, reps=3)
    assert np.array_equal(rows(ctx, 1024, 1024, *A), want(*A))
    assert np.array_equal(rows(ctx, 1024, 1024, *B), want(*B))
    ctx.close()


def test_deferred_tiles_read_the_set_in_use():
    """Sines beyond the reduction range: tiles go to the interpreter behind the context, which reads the y values of the set
    the launch used."""
    _, tape = RS.lowered(RS.sines())
    assert tape.info['sin_bounded'] < tape.info['sin_ops']
    want = {v: fresh(tape, W, H, 0, H, v) for v in ((2.0 ** 40,), (1.5,))}
    assert not np.array_equal(*want.values())
    ctx = context(tape)
    for values in ((2.0 ** 40,), (1.5,), (2.0 ** 40,), (2.0 ** 40,), (1.5,)):
        for again in range(2):
            assert np.array_equal(rows(ctx, W, H, 0, H, values), want[values]), (values, again)
    assert ctx.launch_counts[0] == 3                # the phase is ROW-read: a pass per key that no set holds (2^40, 1.5, 2^40 into a kept set)
    ctx.close()


_STREAMS = r"""
import os, sys
import numpy as np, torch
sys.path[:0] = [%(root)r, %(tests)r]
import maray_amd as M
import row_reuse_scenes as RS
from test_gpu_row_reuse import context, chess, _chess, B
tape, want = chess()
ctx = context(tape)
s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
n = B[1] - B[0]
bufs = [torch.zeros((n, 1024, 3), dtype=torch.uint8, device='cuda') for _ in range(6)]
torch.cuda.synchronize()
for k, buf in enumerate(bufs):                      # filled on one stream, reused on the other, and back
    ctx.render_rows_device(1024, 1024, B[0], B[1], d_rgb8=buf.data_ptr(), stream=(s1, s2)[k %% 2].cuda_stream)
torch.cuda.synchronize()
for k, buf in enumerate(bufs):
    assert np.array_equal(buf.cpu().numpy(), want(*B)), k
assert ctx.launch_counts == (1, 1), ctx.launch_counts
ctx.close()
_chess.pop('off').close()
# the shutter's device entry point, a PIXEL-only parameter, on a stream of the caller's
_, t = RS.lowered(RS.colour())
frames = np.array([[0.125, 0.5], [0.375, 0.25], [0.625, 1.0], [0.875, 0.0]])
outs = []
for reuse in (True, False):
    c = context(t, reuse=reuse)
    c.set_params([0.5, 0.5])
    d = torch.zeros((RS.H, RS.W, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    for call in range(2):
        c.render_rows_shutter_device(RS.W, RS.H, 0, RS.H, frames, d.data_ptr(), stream=s1.cuda_stream)
    s1.synchronize()
    outs.append(d.cpu().numpy())
    assert c.launch_counts[0] == (1 if reuse else 8), (reuse, c.launch_counts)
    c.close()
assert np.array_equal(outs[0], outs[1]) and outs[0].std() > 0
print('streams ok')
"""


def test_two_streams_in_turn_and_the_shutter_on_a_stream():
    """Launches alternating between two streams on one geometry: equal rasters, one ROW pass (a process of its own: the
    streams and device buffers come from PyTorch, imported before the library)."""
    code = _STREAMS % {'root': ROOT, 'tests': HERE}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('streams ok'), r.stdout[-2000:] + r.stderr[-4000:]
